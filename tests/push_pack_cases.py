"""Inputs of bmqcrc_push_event_pack that both the model test and the GPU test
run: a small partition, a delivery of eight messages from it, and one mutation
per refusal condition of include/bmqcrc_protocol.h, each with the refusal it
must produce -- worked out here from the layout of the partition (which record
is of which type, where every DATA record lies and how long its application
data is), not by the model.

TOO_MANY_PIECES has no case: it takes more than 64 GiB of application data.

The partition is storage_apply_cases.partition(): 17 records,
    0 QUEUE_OP CREATION, 16 JOURNAL_OP (a sync point),
    MESSAGE records 1, 4, 5, 8, 9, 12, 13 with 0, 1, 7, 8, 33, 200, 5 bytes of
    application data, a CONFIRM and a DELETION behind records 1, 5, 9 and 13;
DATA records of 12 + length bytes padded to the next multiple of 8 (8 more when
it is one already), back to back from byte 40 of the DATA file.

The delivery: messages 0..7 are records 1, 4, 5, 8, 9, 12, 13 and 9 again, in
option mode 1 (4 bytes), so a message takes 36 + length + padding bytes:
    40, 40, 44, 48, 72, 240, 44, 72
in three events of 3, 3 and 2 messages.
"""
import collections

import numpy as np

import push_pack_model as M
import storage_apply_cases as A

N_RECORDS = 17
MESSAGES = (1, 4, 5, 8, 9, 12, 13)
LENGTH = dict(zip(MESSAGES, (0, 1, 7, 8, 33, 200, 5)))       # bytes of application data
REC = dict(zip(MESSAGES, (16, 16, 24, 24, 48, 216, 24)))     # bytes of the DATA records
AT = dict(zip(MESSAGES, (40, 56, 72, 96, 120, 168, 384)))    # where they lie in the DATA file
DATA_BYTES = 408
RECORDS = (1, 4, 5, 8, 9, 12, 13, 9)
N = 8
MESSAGE_BYTES = (40, 40, 44, 48, 72, 240, 44, 72)
EVENT_FIRST = (0, 3, 6, 8)
EVENT_BYTES = (8 + 40 + 40 + 44, 8 + 48 + 72 + 240, 8 + 44 + 72)
TOTAL = sum(EVENT_BYTES)
QUEUE_IDS = (7, -1, (1 << 31) - 1, 0, 12, 12, 3, 13)
RDA = (5, 0, 255, 1, 2, 3, 0x85, 4)

Case = collections.namedtuple("Case", "run data kw want")
put32 = A.put32


def base():
    """(record run, DATA file, keywords)."""
    run, d = A.partition()
    assert run.size == 60 * N_RECORDS and d.size == DATA_BYTES and TOTAL == 624
    for i in range(N_RECORDS):
        assert (int(run[60 * i]) >> 4 == 1) == (i in MESSAGES)
    for i in MESSAGES:
        assert 8 * int.from_bytes(run[60 * i + 32:60 * i + 36].tobytes(), "big") == AT[i]
        assert 4 * (int.from_bytes(d[AT[i]:AT[i] + 4].tobytes(), "big") & 0x1FFFFFFF) == REC[i]
        assert REC[i] - 12 - int(d[AT[i] + REC[i] - 1]) == LENGTH[i]
    for m, i in enumerate(RECORDS):
        assert MESSAGE_BYTES[m] == 36 + LENGTH[i] + 4 - LENGTH[i] % 4
    kw = dict(data_file_pos=0, queue_ids=np.array(QUEUE_IDS, np.int32),
              records=np.array(RECORDS, np.uint32), flags=None, option_mode=1,
              rda=np.array(RDA, np.uint8), sub_ids=None,
              event_first=np.array(EVENT_FIRST, np.uint64), max_event_bytes=0,
              max_payload_bytes=0, dst_bytes=TOTAL)
    return run, d, kw


def _records(**changes):
    r = np.array(RECORDS, np.uint32)
    for m, i in changes.items():
        r[int(m[1:])] = i
    return r


def _flags(**changes):
    f = np.zeros(N, np.uint8)
    for m, v in changes.items():
        f[int(m[1:])] = v
    return f


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

    # RECORD_INDEX
    add("record_index_n_records", (1, 5), records=_records(m5=N_RECORDS))
    add("record_index_all_ones_in_the_last_message", (1, 7), records=_records(m7=0xFFFFFFFF))
    add("record_index_in_two_messages", (1, 2), records=_records(m6=99, m2=17))
    # RECORD
    add("queue_op_record", (2, 2), records=_records(m2=0))
    add("confirm_record", (2, 3), records=_records(m3=2))
    add("deletion_record", (2, 0), records=_records(m0=3))
    add("journal_op_record_in_the_last_message", (2, 7), records=_records(m7=16))
    add("record_type_0", (2, 1), j=edited(run, lambda j: j.__setitem__(60 * 4, 0x0F)))
    add("record_type_15", (2, 5), j=edited(run, lambda j: j.__setitem__(60 * 12, 0xF0)))
    add("lease_id_0", (2, 3), j=edited(run, lambda j: put32(j, 60 * 8 + 8, 0)))
    # record 9 is messages 4 and 7
    add("sequence_number_0", (2, 4),
        j=edited(run, lambda j: j.__setitem__(slice(60 * 9 + 2, 60 * 9 + 8), 0)))
    add("wrong_magic", (2, 6), j=edited(run, lambda j: j.__setitem__(60 * 13 + 59, 0x64)))
    # (a malformed record nobody names is never read)
    # DATA_OFFSET
    add("data_offset_0", (3, 1), j=edited(run, lambda j: put32(j, 60 * 4 + 32, 0)))
    add("data_offset_below_the_window", (3, 0), data=d[56:], data_file_pos=56)
    add("data_offset_past_the_window", (3, 6), data=d[:AT[13] - 1])
    # DATA_RECORD
    add("fewer_than_8_bytes_of_window", (4, 6), data=d[:AT[13]])
    r8 = AT[8]
    for name, edit in (
            ("data_header_words_0", lambda b: put32(b, r8, REC[8] // 4)),
            ("data_message_words_0", lambda b: put32(b, r8, 3 << 29)),
            ("options_fill_the_record", lambda b: put32(b, r8 + 4, (REC[8] // 4 - 3) << 8)),
            ("padding_byte_0", lambda b: b.__setitem__(r8 + REC[8] - 1, 0)),
            ("padding_byte_9", lambda b: b.__setitem__(r8 + REC[8] - 1, 9))):
        add(name, (4, 3), data=edited(d, edit))
    add("record_past_the_window", (4, 6),
        data=edited(d, lambda b: put32(b, AT[13], (3 << 29) | (REC[13] // 4 + 2))))
    # record 1: 12 bytes of header, no application data, 4 of padding
    add("padding_larger_than_the_data", (4, 0),
        data=edited(d, lambda b: b.__setitem__(AT[1] + REC[1] - 1, 8)))
    add("data_record_named_twice", (4, 4),
        data=edited(d, lambda b: b.__setitem__(AT[9] + REC[9] - 1, 0)))
    # FLAGS
    add("flag_message_properties", (5, 5), flags=_flags(m5=2))
    add("flag_implicit_payload", (5, 2), flags=_flags(m2=8, m6=1))
    add("flag_beside_out_of_order", (5, 0), flags=_flags(m0=6, m1=4))
    add("flag_high_bit_in_the_last_message", (5, 7), flags=_flags(m7=0x80))
    # EVENT_FIRST
    add("event_first_begins_at_1", (6, 0), event_first=first(1, 3, 6, 8))
    add("event_first_repeats", (6, 1), event_first=first(0, 3, 3, 8))
    add("event_first_decreases", (6, 1), event_first=first(0, 6, 3, 8))
    add("event_first_ends_below_n", (6, 3), event_first=first(0, 3, 6, 7))
    add("event_first_ends_above_n", (6, 3), event_first=first(0, 3, 6, 9))
    add("event_first_entry_far_above_n", (6, 1), event_first=first(0, 1 << 40, 6, 8))
    # PAYLOAD_TOO_BIG
    add("payload_cap_below_the_longest", (7, 5), max_payload_bytes=199)
    add("payload_cap_below_three", (7, 4), max_payload_bytes=32)
    # EVENT_TOO_BIG
    add("event_cap_below_the_longest", (8, 1), max_event_bytes=EVENT_BYTES[1] - 1)
    add("event_cap_below_two", (8, 0), max_event_bytes=EVENT_BYTES[0] - 1)
    add("event_cap_below_all", (8, 0), max_event_bytes=EVENT_BYTES[2] - 1)
    add("one_event_above_the_cap", (8, 0), event_first=None, max_event_bytes=TOTAL - 16 - 1,
        dst_bytes=TOTAL - 16)
    add("size_only_event_above_the_cap", (8, 1), max_event_bytes=EVENT_BYTES[1] - 1,
        dst_bytes=None)
    # DST_TOO_SMALL
    add("dst_one_byte_short", (9, 2), dst_bytes=TOTAL - 1)
    add("dst_ends_inside_event_1", (9, 1), dst_bytes=EVENT_BYTES[0] + EVENT_BYTES[1] - 1)
    add("dst_holds_event_0_exactly", (9, 1), dst_bytes=EVENT_BYTES[0])
    add("dst_empty", (9, 0), dst_bytes=0)
    return cases


def precedence_cases():
    """Two violations at once: the lowest kind wins, within a kind the lowest
    index; a refusal of kinds 1..7 hides the kinds behind them."""
    run, d, kw = base()
    cases = {}
    b = d.copy()
    b[AT[1] + REC[1] - 1] = 9   # DATA_RECORD in record 1, message 0
    cases["lower_kind_in_a_later_message"] = Case(
        run, b, dict(kw, records=_records(m7=17)), M.Refusal(1, 7))
    cases["same_kind_in_two_messages"] = Case(
        run, d, dict(kw, records=_records(m5=16, m2=0)), M.Refusal(2, 2))
    j = run.copy()
    put32(j, 60 * 12 + 32, 0)   # DATA_OFFSET in record 12, message 5
    cases["data_offset_before_data_record"] = Case(j, b, kw, M.Refusal(3, 5))
    cases["data_record_before_flags"] = Case(run, b, dict(kw, flags=_flags(m3=1)),
                                             M.Refusal(4, 0))
    cases["two_kinds_in_one_message"] = Case(run, b, dict(kw, flags=_flags(m0=1)),
                                             M.Refusal(4, 0))
    cases["flags_before_event_first"] = Case(
        run, d, dict(kw, flags=_flags(m7=1), event_first=np.array((1, 3, 6, 8), np.uint64)),
        M.Refusal(5, 7))
    cases["event_first_before_the_payload_cap"] = Case(
        run, d, dict(kw, event_first=np.array((0, 3, 6, 7), np.uint64), max_payload_bytes=32),
        M.Refusal(6, 3))
    cases["payload_cap_hides_the_later_kinds"] = Case(
        run, d, dict(kw, max_payload_bytes=199, max_event_bytes=100, dst_bytes=0),
        M.Refusal(7, 5))
    cases["event_cap_before_dst"] = Case(
        run, d, dict(kw, max_event_bytes=EVENT_BYTES[1] - 1, dst_bytes=0), M.Refusal(8, 1))
    return cases
