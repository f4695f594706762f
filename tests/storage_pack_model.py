"""A numpy model of bmqcrc_storage_event_pack (ABI 2.16): what the call
writes, what it reports and what it refuses, with the precedence of refusals,
from the comment block in include/bmqcrc_protocol.h alone.  The bytes come from
the host ``StorageEventBuilder`` with a ``flush()`` at every ``event_first``
boundary.  The GPU tests compare the device against it;
tests/test_storage_pack_model.py checks it against the reference's fixture
partition, ``synth.storage_events`` and the host iterator.

The checksum to compare with is the caller's (``crc32c``).
"""
import collections

import numpy as np

from blazingmq_amd import storage_event as E

(OK, RECORD_HEADER, DATA_OFFSET, DATA_RECORD, EVENT_FIRST, PAYLOAD_TOO_BIG, EVENT_TOO_BIG,
 DST_TOO_SMALL, TOO_MANY_PIECES) = range(9)

MAX_EVENT_BYTES = (1 << 31) - 1
MAGIC = bytes([0x2A, 0x72, 0x45, 0x63])

Refusal = collections.namedtuple("Refusal", "kind index")
Packed = collections.namedtuple("Packed", "events event_offsets types crcs expected result")
_Rec = collections.namedtuple("_Rec", "type at rec hdr length")   # `at`: the DATA record in the window


def _be32(a, at):
    return int.from_bytes(a[at:at + 4].tobytes(), "big")


def _classify(r, data, data_file_pos):
    """(_Rec, None) or (None, kind) for the 60-byte record r."""
    rtype = int(r[0]) >> 4
    seq = int.from_bytes(r[2:8].tobytes(), "big")
    if rtype == 0 or rtype > 5 or _be32(r, 8) == 0 or seq == 0 or r[56:60].tobytes() != MAGIC:
        return None, RECORD_HEADER
    if rtype == 4:
        op = _be32(r, 32)
        if not 1 <= op <= 4:
            return None, RECORD_HEADER
        return _Rec(E.MSG_QUEUE_OP if op in (1, 3) else E.MSG_QLIST, 0, 0, 0, 0), None
    if rtype != 1:
        return _Rec({2: E.MSG_CONFIRM, 3: E.MSG_DELETION, 5: E.MSG_JOURNAL_OP}[rtype],
                    0, 0, 0, 0), None
    o, end = 8 * _be32(r, 32), data.size
    if o == 0 or o < data_file_pos or o - data_file_pos > end:
        return None, DATA_OFFSET
    ow = o - data_file_pos
    if ow + 8 > end:
        return None, DATA_RECORD
    h0, h1 = _be32(data, ow), _be32(data, ow + 4)
    hs, rec, opt = (h0 >> 29) * 4, (h0 & 0x1FFFFFFF) * 4, (h1 >> 8) * 4
    if hs == 0 or rec == 0 or hs + opt >= rec or ow + rec > end:
        return None, DATA_RECORD
    pad = int(data[ow + rec - 1])
    if not 1 <= pad <= 8 or rec < hs + opt + pad:
        return None, DATA_RECORD
    return _Rec(E.MSG_DATA, ow, rec, hs + opt, rec - hs - opt - pad), None


def pack(journal, data, *, journal_pos, data_file_pos, partition_id, event_first=None, flags=None,
         event_type=0, storage_protocol_version=E.STORAGE_PROTOCOL_VERSION, max_event_bytes=0,
         max_payload_bytes=0, dst_bytes, crc32c):
    """The call on host arrays.  ``event_first`` None: one event.
    ``crc32c(bytes) -> int`` is the checksum to compare with.  Returns a
    ``Refusal`` (nothing is written then) or a ``Packed`` whose ``events`` are
    the bytes written and ``result`` the result struct's fields."""
    recs = np.asarray(journal, np.uint8).reshape(-1, 60)
    data = np.asarray(data, np.uint8)
    n = recs.shape[0]
    max_event_bytes = max_event_bytes or E.MAX_EVENT_SIZE_SOFT
    max_payload_bytes = max_payload_bytes or E.MAX_PAYLOAD_SIZE_SOFT
    if n == 0:   # nothing is launched: not even event_offsets is written
        return Packed(np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint8),
                      np.zeros(0, np.uint32), np.zeros(0, np.uint32),
                      dict(n_events=0, n_msgs=0, n_data=0, total_bytes=0, n_bad=0, first_bad=0,
                           refused_kind=0, refused_index=0))
    first = [0, n] if event_first is None else [int(x) for x in event_first]
    n_events = len(first) - 1
    found, bad = [], []
    for i, r in enumerate(recs):
        rec, kind = _classify(r, data, data_file_pos)
        found.append(rec)
        if kind:
            bad.append((kind, i))
        elif 60 + rec.rec > max_payload_bytes:
            bad.append((PAYLOAD_TOO_BIG, i))
    for e in range(n_events + 1):
        if first[e] != n if e == n_events else (e == 0 and first[e] != 0) or first[e] >= first[e + 1]:
            bad.append((EVENT_FIRST, e))
    if bad:   # the lowest kind wins, within it the lowest index
        return Refusal(*min(bad))
    before = [0]
    for rec in found:
        before.append(before[-1] + 72 + rec.rec)
    ends = [8 * (e + 1) + before[first[e + 1]] for e in range(n_events)]
    for e in range(n_events):
        if 8 + before[first[e + 1]] - before[first[e]] > max_event_bytes:
            return Refusal(EVENT_TOO_BIG, e)
    for e in range(n_events):
        if ends[e] > dst_bytes:
            return Refusal(DST_TOO_SMALL, e)
    if sum(((rec.length + 15) >> 4) + 1 for rec in found if rec.length) > 0xFFFFFFFF:
        return Refusal(TOO_MANY_PIECES, 0)
    b = E.StorageEventBuilder(event_type or E.EVENT_TYPE_STORAGE, storage_protocol_version,
                              max_event_bytes=1 << 62)
    for e in range(n_events):
        for i in range(first[e], first[e + 1]):
            rec = found[i]
            b.pack_message(rec.type, partition_id, (journal_pos + 60 * i) // 4, recs[i],
                           data[rec.at:rec.at + rec.rec] if rec.type == E.MSG_DATA else b"",
                           flags=int(flags[i]) if flags is not None else 0)
        b.flush()
    events, offsets = b.finalize()
    assert offsets.tolist() == [0] + ends
    is_data = np.array([rec.type == E.MSG_DATA for rec in found], bool)
    expected = np.array([_be32(r, 52) if d else 0 for r, d in zip(recs, is_data)], np.uint32)
    crcs = np.array([crc32c(data[rec.at + rec.hdr:rec.at + rec.hdr + rec.length].tobytes())
                     if rec.type == E.MSG_DATA else 0 for rec in found], np.uint32)
    wrong = np.flatnonzero(is_data & (expected != crcs))
    result = dict(n_events=n_events, n_msgs=n, n_data=int(is_data.sum()), total_bytes=events.size,
                  n_bad=wrong.size, first_bad=int(wrong[0]) if wrong.size else n, refused_kind=0,
                  refused_index=0)
    return Packed(events, offsets, np.array([rec.type for rec in found], np.uint8), crcs, expected,
                  result)


def refused_result(r, n_events):
    """The result struct's fields after the refusal `r`."""
    return dict(n_events=n_events, n_msgs=0, n_data=0, total_bytes=0, n_bad=0, first_bad=0,
                refused_kind=r.kind, refused_index=r.index)


# ---- the same without a Python loop per record ---------------------------------

def _be32s(rows):
    """The big-endian 32-bit values of (k, 4) uint8 rows, as int64."""
    return np.ascontiguousarray(rows, np.uint8).view(">u4")[:, 0].astype(np.int64)


def storage_events_fast(journal, data, *, journal_pos, data_file_pos, partition_id,
                        event_first=None, flags=None, event_type=0,
                        storage_protocol_version=E.STORAGE_PROTOCOL_VERSION, max_event_bytes=0,
                        max_payload_bytes=0, dst_bytes=None, crc32c=None, record_crcs=None,
                        empty_events=False):
    """``pack`` in numpy alone, for records that are well formed (asserted):
    the StorageHeaders and journal records as an (n, 72) array scattered to
    their offsets, the DATA records by one gather of dwords.  Of the refusals
    it knows PAYLOAD_TOO_BIG, EVENT_TOO_BIG and DST_TOO_SMALL (``dst_bytes``
    None: room for everything).  The CRCs are ``record_crcs`` (one per record,
    computed once by the caller) or ``crc32c`` of every MESSAGE record's
    application data.  ``empty_events``: ``event_first`` may repeat an entry --
    an event of its EventHeader alone, which the packer refuses (EVENT_FIRST)
    and the apply's tests feed to the apply."""
    from put_pack_model import be_bytes, byte_runs, scatter_frames
    recs = np.asarray(journal, np.uint8).reshape(-1, 60)
    data = np.asarray(data, np.uint8)
    n = recs.shape[0]
    assert n > 0
    rtype = (recs[:, 0] >> 4).astype(np.int64)
    seq = recs[:, 2:8].astype(np.int64)
    op = _be32s(recs[:, 32:36])
    assert rtype.min() >= 1 and rtype.max() <= 5 and _be32s(recs[:, 8:12]).min() > 0
    assert seq.any(axis=1).all() and bool((recs[:, 56:60] == np.frombuffer(MAGIC, np.uint8)).all())
    types = np.array([0, E.MSG_DATA, E.MSG_CONFIRM, E.MSG_DELETION, 0, E.MSG_JOURNAL_OP],
                     np.uint8)[rtype]
    queue_op = rtype == 4
    assert bool(((op[queue_op] >= 1) & (op[queue_op] <= 4)).all())
    types[queue_op] = np.where(op[queue_op] & 1, E.MSG_QUEUE_OP, E.MSG_QLIST)
    is_data = rtype == 1
    where = np.flatnonzero(is_data)
    at = 8 * op[where] - data_file_pos
    assert at.size == 0 or (at.min() >= 0 and 8 * op[where].min() > 0 and
                            at.max() + 8 <= data.size)
    h0 = _be32s(data[at[:, None] + np.arange(4)])
    h1 = _be32s(data[at[:, None] + 4 + np.arange(4)])
    hs, rec, opt = (h0 >> 29) * 4, (h0 & 0x1FFFFFFF) * 4, (h1 >> 8) * 4
    assert bool(((hs > 0) & (hs + opt < rec) & (at + rec <= data.size)).all())
    pad = data[at + rec - 1].astype(np.int64)
    assert bool(((pad >= 1) & (pad <= 8) & (rec >= hs + opt + pad)).all())
    length = rec - hs - opt - pad
    size = np.zeros(n, np.int64)
    size[where] = rec
    first = np.array([0, n], np.int64) if event_first is None else np.asarray(
        event_first).astype(np.int64)
    n_events = first.size - 1
    assert first[0] == 0 and first[-1] == n
    assert bool((np.diff(first) >= 0).all() if empty_events else (np.diff(first) > 0).all())
    before = np.concatenate([[0], np.cumsum(72 + size)])
    offsets = 8 * np.arange(n_events + 1) + before[first]
    big = np.flatnonzero(60 + size > (max_payload_bytes or E.MAX_PAYLOAD_SIZE_SOFT))
    if big.size:
        return Refusal(PAYLOAD_TOO_BIG, int(big[0]))
    big = np.flatnonzero(np.diff(offsets) > (max_event_bytes or E.MAX_EVENT_SIZE_SOFT))
    if big.size:
        return Refusal(EVENT_TOO_BIG, int(big[0]))
    if dst_bytes is not None and offsets[-1] > dst_bytes:
        return Refusal(DST_TOO_SMALL, int(np.flatnonzero(offsets[1:] > dst_bytes)[0]))
    event = np.searchsorted(first, np.arange(n), side="right") - 1
    pos = before[:-1] + 8 * (event + 1)
    events = np.zeros(int(offsets[-1]), np.uint8)
    heads = np.zeros((n_events, 8), np.uint8)
    heads[:, 0:4] = be_bytes(np.diff(offsets), 4)
    heads[:, 4] = (E.PROTOCOL_VERSION << 6) | (event_type or E.EVENT_TYPE_STORAGE)
    heads[:, 5] = 2
    scatter_frames(events, offsets[:-1], heads)
    f = np.asarray(flags).astype(np.int64) & 0x1F if flags is not None else np.zeros(n, np.int64)
    frames = np.zeros((n, 72), np.uint8)
    frames[:, 0:4] = be_bytes((f << 27) | ((72 + size) // 4), 4)
    frames[:, 4] = ((storage_protocol_version & 3) << 4) | 3
    frames[:, 5] = types
    frames[:, 6:8] = be_bytes(np.full(n, int(partition_id)), 2)
    frames[:, 8:12] = be_bytes((int(journal_pos) + 60 * np.arange(n, dtype=np.int64)) // 4, 4)
    frames[:, 12:] = recs
    scatter_frames(events, pos, frames)
    # the DATA records, whole, as dwords: they start on multiples of 8 of the
    # file and their sizes are word counts (the window may start anywhere)
    owner, to = byte_runs((pos[where] + 72) // 4, rec // 4)
    within = to - ((pos[where] + 72) // 4)[owner]
    source = at[owner] + 4 * within
    dwords = np.stack([data[source + k] for k in range(4)], axis=1)
    events.view(np.uint32)[to] = np.ascontiguousarray(dwords).view(np.uint32)[:, 0]
    expected = np.zeros(n, np.uint32)
    expected[where] = _be32s(recs[where, 52:56])
    if record_crcs is not None:
        crcs = np.array(record_crcs, np.uint32)
        assert crcs.size == n and not crcs[~is_data].any()
    else:
        crcs = np.zeros(n, np.uint32)
        crcs[where] = [crc32c(data[a:a + ln].tobytes())
                       for a, ln in zip((at + hs + opt).tolist(), length.tolist())]
    wrong = np.flatnonzero(is_data & (expected != crcs))
    result = dict(n_events=n_events, n_msgs=n, n_data=int(where.size),
                  total_bytes=int(offsets[-1]), n_bad=int(wrong.size),
                  first_bad=int(wrong[0]) if wrong.size else n, refused_kind=0, refused_index=0)
    return Packed(events, offsets.astype(np.uint64), types, crcs, expected, result)
