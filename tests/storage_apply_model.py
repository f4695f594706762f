"""A numpy model of bmqcrc_storage_event_apply (ABI 2.15): what the call
writes, what it reports and what it refuses, with the precedence of refusals,
from the comment block in include/bmqcrc_protocol.h alone.  The GPU tests
compare the device against it; tests/test_storage_apply_model.py checks it
against the reference's fixture partition and the host iterator.

The checksum to compare with is the caller's (``crc32c``).
"""
import collections

import numpy as np

(OK, EVENT_OFFSETS, EVENT_HEADER, STORAGE_HEADER, DATA_RECORD, TOO_MANY_MESSAGES, OUT_OF_SYNC,
 DST_TOO_SMALL, TOO_MANY_PIECES) = range(9)

Refusal = collections.namedtuple("Refusal", "kind event index offset")
Applied = collections.namedtuple(
    "Applied", "journal data types flags payload_offsets payload_lengths record_offsets lengths "
               "expected crcs event_first result")
_Msg = collections.namedtuple("_Msg", "event header record type flags payload_length rec hdr "
                                      "app length")


def _be32(ev, at):
    return int.from_bytes(ev[at:at + 4].tobytes(), "big")


def _walk_event(ev, beg, end, partition_id):
    """([messages in front of the first violation], None or (kind, offset))."""
    if beg > end or end > ev.size or beg % 4:
        return [], (EVENT_OFFSETS, beg)
    size = end - beg
    if size < 8:
        return [], (EVENT_HEADER, beg)
    hw = int(ev[beg + 5]) * 4
    if (_be32(ev, beg) & 0x7FFFFFFF) != size:
        return [], (EVENT_HEADER, beg)
    if (int(ev[beg + 4]) & 0x3F) not in (8, 10):
        return [], (EVENT_HEADER, beg + 4)
    if hw < 8 or hw > size:
        return [], (EVENT_HEADER, beg + 5)
    msgs, pos = [], beg + hw
    while pos < end:
        if pos + 12 > end:
            return msgs, (STORAGE_HEADER, pos)
        w0 = _be32(ev, pos)
        msg, shw, mtype = (w0 & 0x07FFFFFF) * 4, (int(ev[pos + 4]) & 0xF) * 4, int(ev[pos + 5])
        pid = int.from_bytes(ev[pos + 6:pos + 8].tobytes(), "big")
        if (shw < 12 or msg < shw or pos + msg > end or not 1 <= mtype <= 6 or msg - shw < 60
                or pid != partition_id):
            return msgs, (STORAGE_HEADER, pos)
        jr, stop = pos + shw, pos + msg
        rec = hdr = app = length = 0
        if mtype == 1:
            if int(ev[jr]) >> 4 != 1:
                return msgs, (STORAGE_HEADER, pos)
            dr = jr + 60
            if dr + 8 > stop:
                return msgs, (DATA_RECORD, dr)
            h0, h1 = _be32(ev, dr), _be32(ev, dr + 4)
            hs, rec, opt = (h0 >> 29) * 4, (h0 & 0x1FFFFFFF) * 4, (h1 >> 8) * 4
            if hs == 0 or rec == 0 or hs + opt >= rec or dr + rec > stop:
                return msgs, (DATA_RECORD, dr)
            pad = int(ev[dr + rec - 1])
            if not 1 <= pad <= 8 or rec < hs + opt + pad:
                return msgs, (DATA_RECORD, dr)
            hdr, app, length = hs + opt, dr + hs + opt, rec - hs - opt - pad
        msgs.append(_Msg(0, pos, jr, mtype, w0 >> 27, msg - shw - 60, rec, hdr, app, length))
        pos = stop
    return msgs, None


def _psn(ev, jr):
    return (_be32(ev, jr + 8),
            (int.from_bytes(ev[jr + 2:jr + 4].tobytes(), "big") << 32) | _be32(ev, jr + 4))


def apply(events, event_offsets, *, partition_id, journal_pos, data_file_pos, lease_id=0, seq=0,
          msg_cap, journal_dst_bytes, data_dst_bytes, crc32c):
    """The call on host arrays.  ``event_offsets`` None: one event, the whole
    buffer.  ``crc32c(bytes) -> int`` is the checksum to compare with.
    Returns a ``Refusal`` (nothing is written then) or an ``Applied`` whose
    ``journal`` / ``data`` are the bytes written and ``result`` the result
    struct's fields."""
    ev = np.asarray(events, np.uint8)
    offs = [0, ev.size] if event_offsets is None else [int(x) for x in event_offsets]
    n_events = len(offs) - 1
    walked = [_walk_event(ev, offs[e], offs[e + 1], partition_id) for e in range(n_events)]
    first = [0]
    for msgs, _ in walked:
        first.append(first[-1] + len(msgs))
    # across events the lowest kind wins, within it the lowest event
    bad = [(v[0], e, v[1]) for e, (_, v) in enumerate(walked) if v]
    if bad:
        kind, e, offset = min(bad)
        stopped = kind in (STORAGE_HEADER, DATA_RECORD)
        return Refusal(kind, e, first[e + 1] if stopped else first[e], offset)
    for e in range(n_events):
        if first[e] <= msg_cap < first[e + 1]:
            return Refusal(TOO_MANY_MESSAGES, e, first[e], offs[e] if event_offsets is not None
                           else 0)
    msgs = [m._replace(event=e) for e, (ms, _) in enumerate(walked) for m in ms]
    n = len(msgs)
    q = [0]
    for m in msgs:
        q.append(q[-1] + m.rec)
    head = (lease_id, seq)
    for i, m in enumerate(msgs):
        lease, s = _psn(ev, m.record)
        sync = 4 * _be32(ev, m.header + 8) == journal_pos + 60 * i and lease >= head[0] and (
            lease > head[0] or s == head[1] + 1)
        if m.type == 1:
            sync = sync and 8 * _be32(ev, m.record + 32) == data_file_pos + q[i]
        if not sync:
            return Refusal(OUT_OF_SYNC, m.event, i, m.header)
        head = (lease, s)
    if 60 * n > journal_dst_bytes:
        i = journal_dst_bytes // 60
        return Refusal(DST_TOO_SMALL, msgs[i].event, i, msgs[i].header)
    for i, m in enumerate(msgs):
        if m.rec and q[i + 1] > data_dst_bytes:
            return Refusal(DST_TOO_SMALL, m.event, i, m.header)
    if sum(((m.length + 15) >> 4) + 1 for m in msgs if m.length) > 0xFFFFFFFF:
        return Refusal(TOO_MANY_PIECES, msgs[0].event, 0, msgs[0].header)
    journal = np.concatenate([ev[m.record:m.record + 60] for m in msgs] + [np.zeros(0, np.uint8)])
    data = np.concatenate([ev[m.record + 60:m.record + 60 + m.rec] for m in msgs] +
                          [np.zeros(0, np.uint8)])
    expected = np.array([_be32(ev, m.record + 52) if m.type == 1 else 0 for m in msgs], np.uint32)
    crcs = np.array([crc32c(ev[m.app:m.app + m.length].tobytes()) if m.type == 1 else 0
                     for m in msgs], np.uint32)
    is_data = np.array([m.type == 1 for m in msgs], bool)
    wrong = np.flatnonzero(is_data & (expected != crcs))
    result = dict(n_events=n_events, n_msgs=n, n_data=int(is_data.sum()), journal_bytes=60 * n,
                  data_bytes=q[n], head_seq=head[1], head_lease_id=head[0], refused_kind=0,
                  n_bad=wrong.size, first_bad=int(wrong[0]) if wrong.size else n,
                  refused_event=0, refused_index=0, refused_offset=0)
    if n_events == 0:   # nothing is launched: not even the two leading zeros are written
        q, first = [], []
    return Applied(journal, data, np.array([m.type for m in msgs], np.uint8),
                   np.array([m.flags for m in msgs], np.uint8),
                   np.array([m.record + 60 for m in msgs], np.uint64),
                   np.array([m.payload_length for m in msgs], np.uint32),
                   np.array(q, np.uint64), np.array([m.length for m in msgs], np.uint32),
                   expected, crcs, np.array(first, np.uint64), result)


# ---- the same without a Python loop per message ---------------------------------

def _be32_at(buf, at):
    """The big-endian 32-bit values at the byte positions `at` of buf, as int64."""
    rows = buf[np.asarray(at, np.int64)[:, None] + np.arange(4)]
    return np.ascontiguousarray(rows).view(">u4")[:, 0].astype(np.int64)


Layout = collections.namedtuple("Layout", "pos offsets size length event data_at")


def layout_fast(run, data, event_first):
    """Where ``storage_events_fast`` puts the records of `run`: Layout(every
    message's StorageHeader, the event offsets, the DATA record's bytes and the
    application data's by record (0: not a MESSAGE record), the event of every
    record, where the first DATA record lies in `data`).  The DATA records lie
    back to back (asserted)."""
    import record_pool
    recs = np.asarray(run, np.uint8).reshape(-1, 60)
    n = recs.shape[0]
    first = np.asarray(event_first).astype(np.int64)
    where = np.flatnonzero(recs[:, 0] >> 4 == 1)
    at, _, rec, app, _ = record_pool.data_fields(run, data, where)
    assert where.size == 0 or np.array_equal(at[1:], (at + rec)[:-1])
    size, length = np.zeros(n, np.int64), np.zeros(n, np.int64)
    size[where], length[where] = rec, app
    before = np.concatenate([[0], np.cumsum(72 + size)])
    event = np.searchsorted(first, np.arange(n), side="right") - 1
    return Layout(before[:-1] + 8 * (event + 1), 8 * np.arange(first.size) + before[first], size,
                  length, event, int(at[0]) if where.size else 0)


Built = collections.namedtuple("Built", "events run lay types first flags journal_pos partition_id")


def build_fast(run, data, event_first, *, journal_pos, partition_id, flags=None):
    """The events of ``apply_fast`` and where everything lies in them, for
    ``answer_fast``: built once for the cases that share an input."""
    import storage_pack_model
    first = np.asarray(event_first).astype(np.int64)
    n = np.asarray(run).size // 60
    packed = storage_pack_model.storage_events_fast(
        run, data, journal_pos=journal_pos, data_file_pos=0, partition_id=partition_id,
        event_first=first, flags=flags, record_crcs=np.zeros(n, np.uint32), empty_events=True)
    lay = layout_fast(run, data, first)
    assert np.array_equal(lay.offsets, packed.event_offsets.astype(np.int64))
    assert np.array_equal(np.flatnonzero(packed.types == 1), np.flatnonzero(lay.size))
    f = np.asarray(flags).astype(np.uint8) & 0x1F if flags is not None else np.zeros(n, np.uint8)
    return Built(packed.events, np.asarray(run, np.uint8).reshape(-1), lay, packed.types, first, f,
                 journal_pos, partition_id)


def events_with(built, run):
    """A copy of the built events with the records of `run` that differ from
    the run they were built of written over theirs (the records' types and
    DATA offsets stay what they were)."""
    events = built.events.copy()
    recs = np.asarray(run, np.uint8).reshape(-1, 60)
    changed = np.flatnonzero((recs != built.run.reshape(-1, 60)).any(axis=1))
    events[(built.lay.pos[changed] + 12)[:, None] + np.arange(60)] = recs[changed]
    return events


def answer_fast(built, events, offsets, run, data, *, data_file_pos, lease_id=0, seq=0, msg_cap,
                journal_dst_bytes, data_dst_bytes, record_crcs, suspects=()):
    """What ``apply`` answers to `events` / `offsets`: the built ones or a
    changed copy of them, `run` and `data` being the records and the DATA file
    they now carry.  Only the events in ``suspects`` are walked."""
    lay, first = built.lay, built.first
    pos, size, event = lay.pos, lay.size, lay.event
    recs = np.asarray(run, np.uint8).reshape(-1, 60)
    n, n_events = recs.shape[0], first.size - 1
    where = np.flatnonzero(size)
    q = np.concatenate([[0], np.cumsum(size)])
    # the walk: across events the lowest kind wins, within it the lowest event
    counts = np.diff(first)
    bad = []
    for e in suspects:
        msgs, v = _walk_event(events, int(offsets[e]), int(offsets[e + 1]), built.partition_id)
        if v:
            counts[e] = len(msgs)
            bad.append((v[0], e, v[1]))
        else:
            assert len(msgs) == counts[e]
    if bad:
        found = np.concatenate([[0], np.cumsum(counts)])
        kind, e, offset = min(bad)
        stopped = kind in (STORAGE_HEADER, DATA_RECORD)
        return Refusal(kind, e, int(found[e + 1] if stopped else found[e]), offset)
    if n > msg_cap:     # the lowest event whose last message lies past msg_cap
        e = int(np.searchsorted(first, msg_cap, side="right")) - 1
        return Refusal(TOO_MANY_MESSAGES, e, int(first[e]), int(offsets[e]))
    # the checks that need a message's predecessor or the prefix q
    i = np.arange(n, dtype=np.int64)
    lease = _be32_at(events, pos + 12 + 8)
    s = (_be32_at(events, pos + 12) & 0xFFFF) << 32 | _be32_at(events, pos + 12 + 4)
    before_lease = np.concatenate([[lease_id], lease[:-1]])
    before_s = np.concatenate([[seq], s[:-1]])
    sync = (4 * _be32_at(events, pos + 8) == built.journal_pos + 60 * i) & (
        lease >= before_lease) & ((lease > before_lease) | (s == before_s + 1))
    sync[where] &= 8 * _be32_at(events, pos[where] + 12 + 32) == data_file_pos + q[where]
    if not sync.all():
        i = int(np.flatnonzero(~sync)[0])
        return Refusal(OUT_OF_SYNC, int(event[i]), i, int(pos[i]))
    if 60 * n > journal_dst_bytes:
        i = journal_dst_bytes // 60
        return Refusal(DST_TOO_SMALL, int(event[i]), i, int(pos[i]))
    over = where[q[where + 1] > data_dst_bytes]
    if over.size:
        i = int(over[0])
        return Refusal(DST_TOO_SMALL, int(event[i]), i, int(pos[i]))
    lengths = lay.length
    assert int((((lengths[where] + 15) >> 4) + 1)[lengths[where] > 0].sum()) <= 0xFFFFFFFF
    crcs = np.asarray(record_crcs, np.uint32)
    expected = np.zeros(n, np.uint32)
    expected[where] = np.ascontiguousarray(recs[where, 52:56]).view(">u4")[:, 0]
    wrong = where[expected[where] != crcs[where]]
    assert not crcs[size == 0].any()
    result = dict(n_events=n_events, n_msgs=n, n_data=int(where.size), journal_bytes=60 * n,
                  data_bytes=int(q[n]), head_seq=int(s[-1]), head_lease_id=int(lease[-1]),
                  refused_kind=0, n_bad=int(wrong.size),
                  first_bad=int(wrong[0]) if wrong.size else n, refused_event=0, refused_index=0,
                  refused_offset=0)
    return Applied(
        recs.reshape(-1), data[lay.data_at:lay.data_at + int(q[n])], built.types, built.flags,
        (pos + 72).astype(np.uint64), size.astype(np.uint32), q.astype(np.uint64),
        lengths.astype(np.uint32), expected, crcs, first.astype(np.uint64), result)


def apply_fast(run, data, event_first, *, partition_id, journal_pos, data_file_pos, lease_id=0,
               seq=0, msg_cap, journal_dst_bytes, data_dst_bytes, record_crcs, flags=None,
               corrupt=None, suspects=()):
    """(events, event offsets, what ``apply`` answers) for the record run `run`
    with its DATA file `data` (whole, from byte 0), sent in the events
    ``event_first`` (entries may repeat: an empty event) from ``journal_pos``,
    in numpy alone.  The bytes are ``storage_events_fast``'s.  ``corrupt(events,
    offsets)`` may then change them in place (or return new offsets); the events
    it touched in a way the walk refuses are to be named in ``suspects``: only
    those are walked, with ``_walk_event``, every other event's message count is
    the split's.  Changes the walk accepts -- a sequence number, a journal or
    DATA offset -- need no suspect: the checks behind the walk read the events'
    own bytes.  ``record_crcs``: the CRC32C of every MESSAGE record's
    application data (0 elsewhere).  The records' DATA records lie back to back
    in `data` (asserted).  ``build_fast`` and ``answer_fast`` are its two
    halves, for callers that share one input among many answers."""
    built = build_fast(run, data, event_first, journal_pos=journal_pos,
                       partition_id=partition_id, flags=flags)
    events, offsets = built.events, built.lay.offsets.copy()
    if corrupt is not None:
        changed = corrupt(events, offsets)
        offsets = offsets if changed is None else np.asarray(changed).astype(np.int64)
    return events, offsets, answer_fast(
        built, events, offsets, run, data, data_file_pos=data_file_pos, lease_id=lease_id, seq=seq,
        msg_cap=msg_cap, journal_dst_bytes=journal_dst_bytes, data_dst_bytes=data_dst_bytes,
        record_crcs=record_crcs, suspects=suspects)


def refused_result(r, n_events):
    """The result struct's fields after the refusal `r`."""
    return dict(n_events=n_events, n_msgs=0, n_data=0, journal_bytes=0, data_bytes=0, head_seq=0,
                head_lease_id=0, refused_kind=r.kind, n_bad=0, first_bad=0,
                refused_event=r.event, refused_index=r.index, refused_offset=r.offset)
