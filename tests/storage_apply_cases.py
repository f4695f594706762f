"""Inputs of bmqcrc_storage_event_apply that both the model test and the GPU
test run: a small replicated partition as STORAGE events, and one mutation of
it per refusal condition of include/bmqcrc_protocol.h, each with the refusal
it must produce -- worked out here from the layout of the events (where every
StorageHeader lies), not by the model.

TOO_MANY_PIECES has no case: it takes more than 64 GiB of application data.
"""
import collections

import numpy as np

from blazingmq_amd import storage as S
from blazingmq_amd import storage_event as E
from blazingmq_amd import synth
import storage_apply_model as M

PARTITION = 3
JOURNAL_POS = S.PartitionWriter.JOURNAL_HEADER
DATA_POS = 40
PER_EVENT = 5

Case = collections.namedtuple("Case", "events offsets kw want")
Layout = collections.namedtuple("Layout", "event index header record type")


def put32(buf, where, v):
    buf[where:where + 4] = np.frombuffer(int(v).to_bytes(4, "big"), np.uint8)


def partition(lengths=(0, 1, 7, 8, 33, 200, 5), seed=3):
    """(record run, DATA file): a queue's CREATION, then per length a MESSAGE
    with that much application data, every other one followed by its CONFIRM
    and DELETION, a SYNCPOINT at the end -- 2 + len + 2 ceil(len / 2) records."""
    rng = np.random.default_rng(seed)
    w = S.PartitionWriter(lease_id=2, partition_id=PARTITION)
    w.queue_op(S.OP_CREATION, S.DEFAULT_QUEUE_KEY)
    for i, n in enumerate(lengths):
        _, guid = w.message(rng.integers(0, 256, size=int(n), dtype=np.uint8).tobytes(),
                            S.DEFAULT_QUEUE_KEY, data_flags=i)
        if i % 2 == 0:
            w.confirm(guid, S.DEFAULT_QUEUE_KEY)
            w.deletion(guid, S.DEFAULT_QUEUE_KEY)
    w.sync_point()
    j, d = w.files()
    return j[JOURNAL_POS:], d


def layout(events, offsets):
    """Every message of well-formed events, by the host iterator."""
    out = []
    for e in range(len(offsets) - 1):
        beg = int(offsets[e])
        for m in E.StorageMessageIterator(events[beg:int(offsets[e + 1])]):
            out.append(Layout(e, len(out), beg + m["header_offset"], beg + m["record_offset"],
                              m["message_type"]))
    return out


def base():
    """(events, offsets, keywords, layout): 17 messages in 4 events of 5, 5, 5
    and 2, applied to an empty partition by a replica that knows no write head."""
    run, d = partition()
    events, offsets = synth.storage_events(run, d, 0, JOURNAL_POS, PARTITION, PER_EVENT)
    n = run.size // 60
    kw = dict(partition_id=PARTITION, journal_pos=JOURNAL_POS, data_file_pos=DATA_POS, lease_id=0,
              seq=0, msg_cap=n, journal_dst_bytes=60 * n, data_dst_bytes=d.size - DATA_POS)
    return events, offsets, kw, layout(events, offsets)


def _grow(events, offsets, e, extra):
    """`extra` bytes appended to event e, its length field following."""
    end = int(offsets[e + 1])
    ev = np.concatenate([events[:end], np.asarray(extra, np.uint8), events[end:]])
    offs = offsets.copy()
    offs[e + 1:] += len(extra)
    put32(ev, int(offs[e]), int(offs[e + 1] - offs[e]))
    return ev, offs


def _message(mtype, record_type, payload, jow=0):
    """A storage message by hand: header, a journal record of `record_type`, payload."""
    record = np.zeros(60, np.uint8)
    record[0] = record_type << 4
    h = np.zeros(12, np.uint8)
    put32(h, 0, 3 + 15 + len(payload) // 4)
    h[4], h[5], h[7] = (1 << 4) | 3, mtype, PARTITION
    put32(h, 8, jow)
    return np.concatenate([h, record, np.asarray(payload, np.uint8)])


def refusal_cases():
    """name -> Case.  `want` is the Refusal the call must report."""
    events, offsets, kw, lay = base()
    size, n = events.size, len(lay)
    first = [sum(1 for m in lay if m.event < e) for e in range(len(offsets))]
    head1, last0 = lay[first[1]], lay[first[1] - 1]   # first message of event 1, last of event 0
    data = [m for m in lay if m.type == 1]
    cases = {}

    def add(name, want, ev=None, offs=None, **changes):
        cases[name] = Case(events if ev is None else ev, offsets if offs is None else offs,
                           dict(kw, **changes), M.Refusal(*want))

    def edited(edit):
        ev = events.copy()
        edit(ev)
        return ev

    # EVENT_OFFSETS
    o = offsets.copy()
    o[-1] = size + 4
    add("offsets_past_the_buffer", (1, 3, first[3], int(o[3])), offs=o)
    o = offsets.copy()
    o[1] += 2   # event 0 is two bytes longer than its length field says: kind 2, which loses
    add("offset_not_a_multiple_of_4", (1, 1, 0, int(o[1])), offs=o)
    o = offsets.copy()
    o[2] = o[1] - 4
    add("offset_above_its_successor", (1, 1, first[1], int(o[1])), offs=o)
    # EVENT_HEADER
    add("event_shorter_than_8", (2, 4, n, size),
        ev=np.concatenate([events, np.zeros(4, np.uint8)]),
        offs=np.concatenate([offsets, [size + 4]]).astype(np.uint64))
    at = int(offsets[1])
    add("event_length_field", (2, 1, first[1], at),
        ev=edited(lambda ev: put32(ev, at, offsets[2] - offsets[1] + 4)))
    add("event_type_put", (2, 1, first[1], at + 4),
        ev=edited(lambda ev: ev.__setitem__(at + 4, (1 << 6) | 2)))
    add("event_header_words_1", (2, 1, first[1], at + 5),
        ev=edited(lambda ev: ev.__setitem__(at + 5, 1)))
    empty = np.array([0, 0, 0, 8, (1 << 6) | 8, 3, 0, 0], np.uint8)
    add("event_header_words_past_the_event", (2, 4, n, size + 5),
        ev=np.concatenate([events, empty]),
        offs=np.concatenate([offsets, [size + 8]]).astype(np.uint64))
    # STORAGE_HEADER, on the first message of event 1 and the last of event 0
    ev, o = _grow(events, offsets, 0, np.zeros(8, np.uint8))
    add("truncated_storage_header", (3, 0, first[1], int(offsets[1])), ev=ev, offs=o)
    for who, m in (("first", head1), ("last", last0)):
        h = m.header
        words = int.from_bytes(events[h:h + 4].tobytes(), "big") & 0x07FFFFFF
        add("storage_header_words_2_" + who, (3, m.event, m.index, h),
            ev=edited(lambda ev: ev.__setitem__(h + 4, (1 << 4) | 2)))
        add("message_words_below_the_header_" + who, (3, m.event, m.index, h),
            ev=edited(lambda ev: put32(ev, h, 2)))
        add("message_past_the_event_" + who, (3, m.event, m.index, h),
            ev=edited(lambda ev: put32(ev, h, words + (1 if who == "last" else 10000))))
        add("message_type_0_" + who, (3, m.event, m.index, h),
            ev=edited(lambda ev: ev.__setitem__(h + 5, 0)))
        add("message_type_7_" + who, (3, m.event, m.index, h),
            ev=edited(lambda ev: ev.__setitem__(h + 5, 7)))
        add("another_partition_" + who, (3, m.event, m.index, h),
            ev=edited(lambda ev: ev.__setitem__(h + 7, PARTITION + 1)))
    short = _message(E.MSG_DELETION, S.REC_DELETION, [])[:-4]
    put32(short, 0, 3 + 14)
    ev, o = _grow(events, offsets, 3, short)
    add("fewer_than_60_payload_bytes", (3, 3, n, size), ev=ev, offs=o)
    d0 = data[1]
    add("data_message_with_a_deletion_record", (3, d0.event, d0.index, d0.header),
        ev=edited(lambda ev: ev.__setitem__(d0.record, S.REC_DELETION << 4)))
    # DATA_RECORD: a DATA message appended to the last event, and the second DATA message
    ev, o = _grow(events, offsets, 3, _message(E.MSG_DATA, S.REC_MESSAGE, [0, 0, 0, 0]))
    add("fewer_than_8_bytes_of_data_record", (4, 3, n, size + 72), ev=ev, offs=o)
    dr = d0.record + 60
    rec_words = int.from_bytes(events[dr:dr + 4].tobytes(), "big") & 0x1FFFFFFF
    for name, edit in (
            ("data_header_words_0", lambda ev: put32(ev, dr, rec_words)),
            ("data_message_words_0", lambda ev: put32(ev, dr, 3 << 29)),
            ("options_fill_the_record", lambda ev: put32(ev, dr + 4, (rec_words - 3) << 8)),
            ("record_past_the_message", lambda ev: put32(ev, dr, (3 << 29) | (rec_words + 2))),
            ("padding_byte_0", lambda ev: ev.__setitem__(dr + 4 * rec_words - 1, 0)),
            ("padding_byte_9", lambda ev: ev.__setitem__(dr + 4 * rec_words - 1, 9))):
        add(name, (4, d0.event, d0.index, dr), ev=edited(edit))
    tiny = np.zeros(16, np.uint8)   # header 12, 4 bytes left, padding byte 8
    put32(tiny, 0, (3 << 29) | 4)
    tiny[15] = 8
    ev, o = _grow(events, offsets, 3, _message(E.MSG_DATA, S.REC_MESSAGE, tiny))
    add("padding_larger_than_the_data", (4, 3, n, size + 72), ev=ev, offs=o)
    # TOO_MANY_MESSAGES
    add("msg_cap_one_short", (5, 3, first[3], int(offsets[3])), msg_cap=n - 1)
    add("msg_cap_inside_event_1", (5, 1, first[1], int(offsets[1])), msg_cap=first[1] + 2)
    add("msg_cap_0", (5, 0, 0, 0), msg_cap=0)
    # OUT_OF_SYNC
    add("journal_pos_ahead", (6, 0, 0, lay[0].header), journal_pos=JOURNAL_POS + 60)
    add("journal_offset_of_one_message", (6, 1, head1.index, head1.header),
        ev=edited(lambda ev: put32(ev, head1.header + 8, 1)))
    add("lease_below_the_predecessor", (6, last0.event, last0.index, last0.header),
        ev=edited(lambda ev: put32(ev, last0.record + 8, 1)))
    # (the predecessor of event 1's first message is in event 0)
    add("sequence_gap_across_events", (6, 1, head1.index, head1.header),
        ev=edited(lambda ev: put32(ev, head1.record + 4, head1.index + 3)))
    add("sequence_repeated", (6, 0, 1, lay[1].header),
        ev=edited(lambda ev: put32(ev, lay[1].record + 4, 1)))
    add("write_head_of_the_same_lease", (6, 0, 0, lay[0].header), lease_id=2, seq=5)
    add("write_head_of_a_later_lease", (6, 0, 0, lay[0].header), lease_id=3, seq=0)
    add("data_file_pos_ahead", (6, data[0].event, data[0].index, data[0].header),
        data_file_pos=DATA_POS + 8)
    add("data_offset_of_one_message", (6, d0.event, d0.index, d0.header),
        ev=edited(lambda ev: put32(ev, d0.record + 32, 4)))
    # DST_TOO_SMALL
    add("journal_dst_one_byte_short", (7, 3, n - 1, lay[-1].header), journal_dst_bytes=60 * n - 1)
    add("journal_dst_holds_two", (7, 0, 2, lay[2].header), journal_dst_bytes=179)
    add("data_dst_one_byte_short", (7, data[-1].event, data[-1].index, data[-1].header),
        data_dst_bytes=kw["data_dst_bytes"] - 1)
    add("data_dst_empty", (7, data[0].event, data[0].index, data[0].header), data_dst_bytes=0)
    add("both_destinations_short", (7, 0, 1, lay[1].header), journal_dst_bytes=60,
        data_dst_bytes=0)
    return cases


def precedence_cases():
    """Two violations in different events: the lowest kind wins, within a kind
    the lowest event; a walk refusal hides OUT_OF_SYNC and DST_TOO_SMALL."""
    events, offsets, kw, lay = base()
    first = [sum(1 for m in lay if m.event < e) for e in range(len(offsets))]
    d_in_0 = next(m for m in lay if m.type == 1 and m.event == 0)
    cases = {}
    # DATA_RECORD in event 0, STORAGE_HEADER in event 2: kind 3 wins.  Event 0
    # then counts the messages in front of its violation only.
    ev = events.copy()
    dr = d_in_0.record + 60
    put32(ev, dr, 3 << 29)
    m2 = lay[first[2] + 1]
    ev[m2.header + 5] = 9
    index = d_in_0.index + (first[2] - first[1]) + 1
    cases["lower_kind_in_a_later_event"] = Case(ev, offsets, kw, M.Refusal(3, 2, index, m2.header))
    # STORAGE_HEADER in events 1 and 2: event 1 wins
    ev = events.copy()
    m1 = lay[first[1] + 2]
    ev[m1.header + 5] = 0
    ev[m2.header + 5] = 9
    cases["same_kind_in_two_events"] = Case(ev, offsets, kw, M.Refusal(3, 1, m1.index, m1.header))
    # a malformed last event with everything else out of sync and too small
    ev = events.copy()
    ev[int(offsets[3]) + 4] = (1 << 6) | 2
    cases["walk_refusal_hides_the_later_kinds"] = Case(
        ev, offsets, dict(kw, journal_pos=JOURNAL_POS + 60, journal_dst_bytes=0),
        M.Refusal(2, 3, first[3], int(offsets[3]) + 4))
    # out of sync and too small: OUT_OF_SYNC is the lower kind
    cases["out_of_sync_before_too_small"] = Case(
        events, offsets, dict(kw, data_file_pos=DATA_POS + 8, journal_dst_bytes=0),
        M.Refusal(6, d_in_0.event, d_in_0.index, d_in_0.header))
    return cases


# ---- large inputs: record_pool.py's run through storage_apply_model.apply_fast -----
#
# What the cases past one walk grid plant, as (what, where) pairs: a violation
# of the walk in an event or at a message, or a value the checks behind the
# walk compare.  `lay` is storage_apply_model.layout_fast's.

WALK_PLANTS = ("offsets", "event_length", "partition", "padding")


def spoil(events, offsets, lay, what, at):
    """One plant, in place.  Of the walk's: "offsets" (event `at` starts 2
    bytes late), "event_length" (its EventHeader 4 bytes long), "partition"
    (message `at` names another partition), "padding" (DATA message `at` ends
    with a padding byte of 9).  Of the checks': "data_offset" (MESSAGE record
    `at` 8 bytes further in the DATA file), "journal_offset" (message `at` one
    word further in the journal)."""
    p = int(lay.pos[at]) if what not in ("offsets", "event_length") else 0
    if what == "offsets":
        offsets[at] += 2
    elif what == "event_length":
        beg = int(offsets[at])
        put32(events, beg, int(offsets[at + 1]) - beg + 4)
    elif what == "partition":
        events[p + 7] ^= 1
    elif what == "padding":
        assert lay.size[at] > 0
        events[p + 72 + int(lay.size[at]) - 1] = 9
    elif what == "data_offset":
        assert lay.size[at] > 0
        put32(events, p + 12 + 32, M._be32(events, p + 12 + 32) + 1)
    elif what == "journal_offset":
        put32(events, p + 8, M._be32(events, p + 8) + 1)
    else:
        raise KeyError(what)


def planted(lay, plants):
    """(corrupt, suspects) for apply_fast of the (what, where) pairs `plants`."""
    def corrupt(events, offsets):
        for what, at in plants:
            spoil(events, offsets, lay, what, at)
    suspects = set()
    for what, at in plants:
        if what == "offsets":           # (event at - 1 ends 2 bytes late too)
            suspects.update({at - 1, at})
        elif what == "event_length":
            suspects.add(at)
        elif what in ("partition", "padding"):
            suspects.add(int(lay.event[at]))
    return corrupt, sorted(suspects)


def sequence_gap(run, at):
    """`run` with 1 added to the sequence number of every record from `at` on:
    record `at` alone no longer follows its predecessor."""
    recs = np.array(run, np.uint8).reshape(-1, 60)
    seq = (recs[at:, 2:8].astype(np.int64) << (8 * np.arange(5, -1, -1))).sum(axis=1) + 1
    recs[at:, 2:8] = (seq[:, None] >> (8 * np.arange(5, -1, -1))) & 0xFF
    return recs.reshape(-1)


def new_lease(run, at):
    """`run` with the lease id raised by one from record `at` on and the
    sequence numbers restarting at 1 there."""
    recs = np.array(run, np.uint8).reshape(-1, 60)
    lease = M._be32(recs[at], 8) + 1
    seq = 1 + np.arange(recs.shape[0] - at, dtype=np.int64)
    recs[at:, 2:8] = (seq[:, None] >> (8 * np.arange(5, -1, -1))) & 0xFF
    recs[at:, 8:12] = np.frombuffer(int(lease).to_bytes(4, "big"), np.uint8)
    return recs.reshape(-1)
