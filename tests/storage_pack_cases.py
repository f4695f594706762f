"""Inputs of bmqcrc_storage_event_pack that both the model test and the GPU
test run: a small partition as the primary wrote it, and one mutation of it per
refusal condition of include/bmqcrc_protocol.h, each with the refusal it must
produce -- worked out here from the layout of the partition (which record is of
which type, where every DATA record lies and how long it is), not by the model.

TOO_MANY_PIECES has no case: it takes more than 64 GiB of application data.

The partition is storage_apply_cases.partition(): 17 records,
    0 QUEUE_OP CREATION, 16 JOURNAL_OP (a sync point),
    MESSAGE records 1, 4, 5, 8, 9, 12, 13 with 0, 1, 7, 8, 33, 200, 5 bytes of
    application data, a CONFIRM and a DELETION behind records 1, 5, 9 and 13;
DATA records of 12 + length bytes padded to the next multiple of 8 (8 more when
it is one already), back to back from byte 40 of the DATA file.
"""
import collections

import numpy as np

import storage_apply_cases as A
import storage_pack_model as M

PARTITION = A.PARTITION
JOURNAL_POS = A.JOURNAL_POS
N = 17
MESSAGES = (1, 4, 5, 8, 9, 12, 13)
REC = dict(zip(MESSAGES, (16, 16, 24, 24, 48, 216, 24)))     # bytes of the DATA records
AT = dict(zip(MESSAGES, (40, 56, 72, 96, 120, 168, 384)))    # where they lie in the DATA file
DATA_BYTES = 408
EVENT_FIRST = (0, 5, 10, 15, 17)
# 8 + 72 per record + the DATA records of the event's MESSAGE records
EVENT_BYTES = (8 + 5 * 72 + 16 + 16, 8 + 5 * 72 + 24 + 24 + 48, 8 + 5 * 72 + 216 + 24, 8 + 2 * 72)
TOTAL = sum(EVENT_BYTES)

Case = collections.namedtuple("Case", "run data kw want")
put32 = A.put32


def base():
    """(record run, DATA file, keywords): 17 records in 4 events of 5, 5, 5 and 2."""
    run, d = A.partition()
    assert run.size == 60 * N and d.size == DATA_BYTES and TOTAL == 1624
    for i in range(N):
        assert (int(run[60 * i]) >> 4 == 1) == (i in MESSAGES)
    for i in MESSAGES:
        assert 8 * int.from_bytes(run[60 * i + 32:60 * i + 36].tobytes(), "big") == AT[i]
        assert 4 * (int.from_bytes(d[AT[i]:AT[i] + 4].tobytes(), "big") & 0x1FFFFFFF) == REC[i]
    kw = dict(journal_pos=JOURNAL_POS, data_file_pos=0, partition_id=PARTITION,
              event_first=np.array(EVENT_FIRST, np.uint64), flags=None, max_event_bytes=0,
              max_payload_bytes=0, dst_bytes=TOTAL)
    return run, d, kw


def refusal_cases():
    """name -> Case.  `want` is the Refusal the call must report."""
    run, d, kw = base()
    cases = {}

    def add(name, want, j=None, data=None, **changes):
        cases[name] = Case(run if j is None else j, d if data is None else data,
                           dict(kw, **changes), M.Refusal(*want))

    def edited(buf, edit):
        out = buf.copy()
        edit(out)
        return out

    def first(*entries):
        return np.array(entries, np.uint64)

    # RECORD_HEADER
    add("record_type_0", (1, 6), j=edited(run, lambda j: j.__setitem__(60 * 6, 0x0F)))
    add("record_type_6_in_the_last_record", (1, 16),
        j=edited(run, lambda j: j.__setitem__(60 * 16, 0x60)))
    add("record_type_15", (1, 2), j=edited(run, lambda j: j.__setitem__(60 * 2, 0xF0)))
    add("lease_id_0", (1, 2), j=edited(run, lambda j: put32(j, 60 * 2 + 8, 0)))
    add("sequence_number_0", (1, 3),
        j=edited(run, lambda j: j.__setitem__(slice(60 * 3 + 2, 60 * 3 + 8), 0)))
    add("wrong_magic", (1, 10), j=edited(run, lambda j: j.__setitem__(60 * 10 + 59, 0x64)))
    add("queue_op_0", (1, 0), j=edited(run, lambda j: put32(j, 32, 0)))
    add("queue_op_5", (1, 0), j=edited(run, lambda j: put32(j, 32, 5)))
    # DATA_OFFSET
    add("data_offset_0", (2, 4), j=edited(run, lambda j: put32(j, 60 * 4 + 32, 0)))
    add("data_offset_below_the_window", (2, 1), data=d[56:], data_file_pos=56)
    add("data_offset_past_the_window", (2, 13), data=d[:AT[13] - 1])
    # DATA_RECORD
    add("fewer_than_8_bytes_of_window", (3, 13), data=d[:AT[13]])
    r8 = AT[8]
    for name, edit in (
            ("data_header_words_0", lambda b: put32(b, r8, REC[8] // 4)),
            ("data_message_words_0", lambda b: put32(b, r8, 3 << 29)),
            ("options_fill_the_record", lambda b: put32(b, r8 + 4, (REC[8] // 4 - 3) << 8)),
            ("padding_byte_0", lambda b: b.__setitem__(r8 + REC[8] - 1, 0)),
            ("padding_byte_9", lambda b: b.__setitem__(r8 + REC[8] - 1, 9))):
        add(name, (3, 8), data=edited(d, edit))
    add("record_past_the_window", (3, 13),
        data=edited(d, lambda b: put32(b, AT[13], (3 << 29) | (REC[13] // 4 + 2))))
    # record 1: 12 bytes of header, no application data, 4 of padding
    add("padding_larger_than_the_data", (3, 1),
        data=edited(d, lambda b: b.__setitem__(AT[1] + REC[1] - 1, 8)))
    # EVENT_FIRST
    add("event_first_begins_at_1", (4, 0), event_first=first(1, 5, 10, 15, 17))
    add("event_first_repeats", (4, 1), event_first=first(0, 5, 5, 15, 17))
    add("event_first_decreases", (4, 2), event_first=first(0, 5, 10, 9, 17))
    add("event_first_ends_below_n", (4, 4), event_first=first(0, 5, 10, 15, 16))
    add("event_first_ends_above_n", (4, 4), event_first=first(0, 5, 10, 15, 18))
    add("event_first_entry_far_above_n", (4, 3), event_first=first(0, 5, 10, 1 << 40, 17))
    # PAYLOAD_TOO_BIG
    add("payload_cap_below_the_longest", (5, 12), max_payload_bytes=60 + REC[12] - 1)
    add("payload_cap_below_two", (5, 9), max_payload_bytes=60 + REC[9] - 1)
    add("payload_cap_below_a_journal_record", (5, 0), max_payload_bytes=59)
    # EVENT_TOO_BIG
    add("event_cap_below_the_longest", (6, 2), max_event_bytes=EVENT_BYTES[2] - 1)
    add("event_cap_below_two", (6, 1), max_event_bytes=EVENT_BYTES[1] - 1)
    add("event_cap_below_all", (6, 0), max_event_bytes=EVENT_BYTES[3] - 1)
    add("one_event_above_the_cap", (6, 0), event_first=None, max_event_bytes=TOTAL - 24 - 1,
        dst_bytes=TOTAL - 24)
    # DST_TOO_SMALL
    add("dst_one_byte_short", (7, 3), dst_bytes=TOTAL - 1)
    add("dst_ends_inside_event_1", (7, 1), dst_bytes=EVENT_BYTES[0] + EVENT_BYTES[1] - 1)
    add("dst_holds_event_0_exactly", (7, 1), dst_bytes=EVENT_BYTES[0])
    add("dst_empty", (7, 0), dst_bytes=0)
    return cases


def precedence_cases():
    """Two violations at once: the lowest kind wins, within a kind the lowest
    index; a refusal of kinds 1..5 hides the kinds behind them."""
    run, d, kw = base()
    cases = {}
    j = run.copy()
    j[60 * 16] = 0x60           # RECORD_HEADER in the last record
    b = d.copy()
    b[AT[1] + REC[1] - 1] = 9   # DATA_RECORD in record 1
    cases["lower_kind_in_a_later_record"] = Case(j, b, kw, M.Refusal(1, 16))
    j = run.copy()
    j[60 * 6] = 0x0F
    put32(j, 60 * 3 + 8, 0)
    cases["same_kind_in_two_records"] = Case(j, d, kw, M.Refusal(1, 3))
    j = run.copy()
    put32(j, 60 * 12 + 32, 0)   # DATA_OFFSET in record 12
    cases["data_offset_before_data_record"] = Case(j, b, kw, M.Refusal(2, 12))
    cases["event_first_before_the_payload_cap"] = Case(
        run, d, dict(kw, event_first=np.array((0, 5, 10, 15, 16), np.uint64), max_payload_bytes=59),
        M.Refusal(4, 4))
    cases["data_record_before_event_first"] = Case(
        run, b, dict(kw, event_first=np.array((0, 5, 5, 15, 17), np.uint64)), M.Refusal(3, 1))
    cases["payload_cap_hides_the_later_kinds"] = Case(
        run, d, dict(kw, max_payload_bytes=60 + REC[12] - 1, max_event_bytes=100, dst_bytes=0),
        M.Refusal(5, 12))
    cases["event_cap_before_dst"] = Case(
        run, d, dict(kw, max_event_bytes=EVENT_BYTES[2] - 1, dst_bytes=0), M.Refusal(6, 2))
    return cases
