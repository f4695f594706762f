"""A numpy model of bmqcrc_push_event_pack (ABI 2.17): what the call writes,
what it reports and what it refuses, with the precedence of refusals, from the
comment block in include/bmqcrc_protocol.h alone.  The bytes come from the host
``PushEventBuilder``, one builder per event: a flush at every ``event_first``
boundary.  The GPU tests compare the device against it;
tests/test_push_pack_model.py checks it against spelled-out events, the
reference's fixture partition and the host iterator.

The checksum to compare with is the caller's (``crc32c``).
"""
import collections

import numpy as np

from blazingmq_amd import push_event as E

(OK, RECORD_INDEX, RECORD, DATA_OFFSET, DATA_RECORD, FLAGS, EVENT_FIRST, PAYLOAD_TOO_BIG,
 EVENT_TOO_BIG, DST_TOO_SMALL, TOO_MANY_PIECES) = range(11)

MAGIC = bytes([0x2A, 0x72, 0x45, 0x63])
OPTION_BYTES = (0, 4, 8, 12)

Refusal = collections.namedtuple("Refusal", "kind index")
Packed = collections.namedtuple("Packed", "events event_offsets crcs lengths expected result")
# `at`: the application data in the window
_Msg = collections.namedtuple("_Msg", "record at length cat props schema guid")


def _be32(a, at):
    return int.from_bytes(a[at:at + 4].tobytes(), "big")


def _classify(recs, data, data_file_pos, index):
    """(_Msg, None) or (None, kind) for the message that names record `index`."""
    if index >= recs.shape[0]:
        return None, RECORD_INDEX
    r = recs[index]
    rtype = int(r[0]) >> 4
    seq = int.from_bytes(r[2:8].tobytes(), "big")
    if rtype != 1 or _be32(r, 8) == 0 or seq == 0 or r[56:60].tobytes() != MAGIC:
        return None, RECORD
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
    schema = int.from_bytes(data[ow + 8:ow + 10].tobytes(), "big") if hs >= 12 else 0
    return _Msg(index, ow + hs + opt, rec - hs - opt - pad, int(r[21]) & 7, bool(h1 & 1), schema,
                r[36:52].tobytes()), None


def _empty(n_events=0):
    return dict(n_events=n_events, n_msgs=0, total_bytes=0, n_bad=0, first_bad=0, refused_kind=0,
                refused_index=0)


def pack(journal, data, *, data_file_pos, queue_ids, records=None, flags=None, option_mode=0,
         rda=None, sub_ids=None, event_first=None, max_event_bytes=0, max_payload_bytes=0,
         dst_bytes, crc32c):
    """The call on host arrays.  ``event_first`` None: one event; ``dst_bytes``
    None: the size-only call.  ``crc32c(bytes) -> int`` is the checksum to
    compare with.  Returns a ``Refusal`` (nothing is written then) or a
    ``Packed`` whose ``events`` are the bytes written (none when size only) and
    ``result`` the result struct's fields."""
    recs = np.asarray(journal, np.uint8).reshape(-1, 60)
    data = np.asarray(data, np.uint8)
    index = list(range(recs.shape[0])) if records is None else [int(x) for x in records]
    n = len(index)
    assert len(queue_ids) == n
    max_event_bytes = max_event_bytes or E.MAX_EVENT_SIZE_SOFT
    max_payload_bytes = max_payload_bytes or E.MAX_PAYLOAD_SIZE_SOFT
    if n == 0:   # nothing is launched: not even event_offsets is written
        return Packed(np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32),
                      np.zeros(0, np.uint32), np.zeros(0, np.uint32), _empty())
    first = [0, n] if event_first is None else [int(x) for x in event_first]
    n_events = len(first) - 1
    found, bad = [], []
    for m, i in enumerate(index):
        msg, kind = _classify(recs, data, data_file_pos, i)
        found.append(msg)
        if kind:
            bad.append((kind, m))
        elif msg.length > max_payload_bytes:
            bad.append((PAYLOAD_TOO_BIG, m))
        if flags is not None and int(flags[m]) & ~4:
            bad.append((FLAGS, m))
    for e in range(n_events + 1):
        if first[e] != n if e == n_events else (e == 0 and first[e] != 0) or first[e] >= first[e + 1]:
            bad.append((EVENT_FIRST, e))
    if bad:   # the lowest kind wins, within it the lowest index
        return Refusal(*min(bad))
    lead = 32 + OPTION_BYTES[option_mode]
    before = [0]
    for msg in found:
        before.append(before[-1] + lead + msg.length + 4 - msg.length % 4)
    ends = [8 * (e + 1) + before[first[e + 1]] for e in range(n_events)]
    for e in range(n_events):
        if 8 + before[first[e + 1]] - before[first[e]] > max_event_bytes:
            return Refusal(EVENT_TOO_BIG, e)
    if dst_bytes is not None:
        for e in range(n_events):
            if ends[e] > dst_bytes:
                return Refusal(DST_TOO_SMALL, e)
    if sum(((msg.length + 15) >> 4) + 1 for msg in found if msg.length) > 0xFFFFFFFF:
        return Refusal(TOO_MANY_PIECES, 0)
    offsets = np.array([0] + ends, np.uint64)
    result = dict(n_events=n_events, n_msgs=n, total_bytes=ends[-1], n_bad=0, first_bad=n,
                  refused_kind=0, refused_index=0)
    none = np.zeros(0, np.uint32)
    if dst_bytes is None:
        return Packed(np.zeros(0, np.uint8), offsets, none, none, none, result)
    out = []
    for e in range(n_events):
        b = E.PushEventBuilder(max_event_bytes=1 << 62)
        for m in range(first[e], first[e + 1]):
            msg = found[m]
            if option_mode == E.OPTION_PACKED_RDA:
                b.add_sub_queue_infos_option([(E.DEFAULT_SUB_QUEUE_ID, int(rda[m]))], True)
            elif option_mode == E.OPTION_SUB_QUEUE_ID:
                b.add_sub_queue_infos_option([(int(sub_ids[m]), 0)], False)
            elif option_mode == E.OPTION_SUB_QUEUE_INFO:
                b.add_sub_queue_infos_option([(int(sub_ids[m]), int(rda[m]))], True,
                                             allow_packed=False)
            b.pack_message(data[msg.at:msg.at + msg.length], int(queue_ids[m]), msg.guid,
                           flags=int(flags[m]) if flags is not None else 0,
                           compression=msg.cat, properties=msg.props, schema_id=msg.schema)
        out.append(b.blob())
    events = np.concatenate(out)
    assert [0] + list(np.cumsum([len(x) for x in out])) == [0] + ends
    expected = np.array([_be32(recs[msg.record], 52) for msg in found], np.uint32)
    crcs = np.array([crc32c(data[msg.at:msg.at + msg.length].tobytes()) for msg in found],
                    np.uint32)
    wrong = np.flatnonzero(expected != crcs)
    result.update(n_bad=wrong.size, first_bad=int(wrong[0]) if wrong.size else n)
    return Packed(events, offsets, crcs, np.array([msg.length for msg in found], np.uint32),
                  expected, result)


def refused_result(r, n_events):
    """The result struct's fields after the refusal `r`."""
    return dict(_empty(n_events), refused_kind=r.kind, refused_index=r.index)


# ---- the same without a Python loop per message --------------------------------

def _be32s(rows):
    """The big-endian 32-bit values of (k, 4) uint8 rows, as int64."""
    return np.ascontiguousarray(rows, np.uint8).view(">u4")[:, 0].astype(np.int64)


def push_events_fast(journal, data, *, data_file_pos, queue_ids, records=None, flags=None,
                     option_mode=0, rda=None, sub_ids=None, event_first=None, max_event_bytes=0,
                     max_payload_bytes=0, dst_bytes="room", crc32c=None, record_crcs=None):
    """``pack`` in numpy alone, for messages that name well-formed MESSAGE
    records (asserted): every distinct record is read once and gathered, the
    PushHeaders and options are an (n, 32..44) array scattered to their
    offsets, the application data one gather, the padding one scatter.  Of the
    refusals it knows FLAGS, PAYLOAD_TOO_BIG, EVENT_TOO_BIG and DST_TOO_SMALL
    (``dst_bytes`` "room": room for everything; None: the size-only call).  The
    CRCs are ``record_crcs`` (one per record of the journal, computed once by
    the caller) or ``crc32c`` of every distinct record's application data."""
    from put_pack_model import be_bytes, place_payload, scatter_frames
    recs = np.asarray(journal, np.uint8).reshape(-1, 60)
    data = np.asarray(data, np.uint8)
    index = np.arange(recs.shape[0]) if records is None else np.asarray(records).astype(np.int64)
    n = index.size
    assert n > 0 and len(queue_ids) == n and index.min() >= 0 and index.max() < recs.shape[0]
    uniq, inverse = np.unique(index, return_inverse=True)
    r = recs[uniq]
    assert bool((r[:, 0] >> 4 == 1).all()) and _be32s(r[:, 8:12]).min() > 0
    assert r[:, 2:8].any(axis=1).all() and bool((r[:, 56:60] == np.frombuffer(MAGIC, np.uint8)).all())
    at = 8 * _be32s(r[:, 32:36]) - data_file_pos
    assert at.min() >= 0 and 8 * _be32s(r[:, 32:36]).min() > 0 and at.max() + 8 <= data.size
    h0 = _be32s(data[at[:, None] + np.arange(4)])
    h1 = _be32s(data[at[:, None] + 4 + np.arange(4)])
    hs, rec, opt = (h0 >> 29) * 4, (h0 & 0x1FFFFFFF) * 4, (h1 >> 8) * 4
    assert bool(((hs > 0) & (hs + opt < rec) & (at + rec <= data.size)).all())
    pad8 = data[at + rec - 1].astype(np.int64)
    assert bool(((pad8 >= 1) & (pad8 <= 8) & (rec >= hs + opt + pad8)).all())
    schema = np.where(hs >= 12, (data[at + 8].astype(np.int64) << 8) | data[at + 9], 0)
    app = (at + hs + opt)[inverse]
    length = (rec - hs - opt - pad8)[inverse]
    first = np.array([0, n], np.int64) if event_first is None else np.asarray(
        event_first).astype(np.int64)
    n_events = first.size - 1
    assert first[0] == 0 and first[-1] == n and bool((np.diff(first) > 0).all())
    bad = []
    if flags is not None:
        wrong = np.flatnonzero(np.asarray(flags).astype(np.int64) & ~4)
        bad += [(FLAGS, int(wrong[0]))] if wrong.size else []
    big = np.flatnonzero(length > (max_payload_bytes or E.MAX_PAYLOAD_SIZE_SOFT))
    bad += [(PAYLOAD_TOO_BIG, int(big[0]))] if big.size else []
    if bad:
        return Refusal(*min(bad))
    lead = 32 + OPTION_BYTES[option_mode]
    pad = 4 - length % 4
    before = np.concatenate([[0], np.cumsum(lead + length + pad)])
    offsets = 8 * np.arange(n_events + 1) + before[first]
    big = np.flatnonzero(np.diff(offsets) > (max_event_bytes or E.MAX_EVENT_SIZE_SOFT))
    if big.size:
        return Refusal(EVENT_TOO_BIG, int(big[0]))
    if dst_bytes is not None and not isinstance(dst_bytes, str) and offsets[-1] > dst_bytes:
        return Refusal(DST_TOO_SMALL, int(np.flatnonzero(offsets[1:] > dst_bytes)[0]))
    result = dict(n_events=n_events, n_msgs=n, total_bytes=int(offsets[-1]), n_bad=0, first_bad=n,
                  refused_kind=0, refused_index=0)
    none = np.zeros(0, np.uint32)
    if dst_bytes is None:
        return Packed(np.zeros(0, np.uint8), offsets.astype(np.uint64), none, none, none, result)
    event = np.searchsorted(first, np.arange(n), side="right") - 1
    pos = before[:-1] + 8 * (event + 1)
    events = np.zeros(int(offsets[-1]), np.uint8)
    heads = np.zeros((n_events, 8), np.uint8)
    heads[:, 0:4] = be_bytes(np.diff(offsets), 4)
    heads[:, 4:6] = ((E.PROTOCOL_VERSION << 6) | E.EVENT_TYPE_PUSH, 2)
    scatter_frames(events, offsets[:-1], heads)
    f = np.asarray(flags).astype(np.int64) & 0xF if flags is not None else np.zeros(n, np.int64)
    f = f | np.where((h1 & 1)[inverse] != 0, 2, 0)             # MESSAGE_PROPERTIES
    cat = (r[:, 21].astype(np.int64) & 7)[inverse]
    frames = np.zeros((n, lead), np.uint8)
    frames[:, 0:4] = be_bytes((f << 28) | ((lead + length + pad) // 4), 4)
    frames[:, 4:8] = be_bytes((((lead - 32) // 4) << 8) | (cat << 5) | 8, 4)
    frames[:, 8:12] = be_bytes(np.asarray(queue_ids).astype(np.int64) & 0xFFFFFFFF, 4)
    frames[:, 12:28] = r[:, 36:52][inverse]
    frames[:, 28:30] = be_bytes(schema[inverse], 2)
    if option_mode == E.OPTION_PACKED_RDA:
        frames[:, 32:36] = be_bytes((3 << 26) | (1 << 25) | (np.asarray(rda).astype(np.int64) & 0xFF), 4)
    elif option_mode == E.OPTION_SUB_QUEUE_ID:
        frames[:, 32:36] = be_bytes(np.full(n, (1 << 26) | 2), 4)
        frames[:, 36:40] = be_bytes(np.asarray(sub_ids).astype(np.int64) & 0xFFFFFFFF, 4)
    elif option_mode == E.OPTION_SUB_QUEUE_INFO:
        frames[:, 32:36] = be_bytes(np.full(n, (3 << 26) | (2 << 21) | 3), 4)
        frames[:, 36:40] = be_bytes(np.asarray(sub_ids).astype(np.int64) & 0xFFFFFFFF, 4)
        frames[:, 40] = np.asarray(rda).astype(np.int64) & 0xFF
    scatter_frames(events, pos, frames)
    place_payload(events, data, app, length, pos + lead, pad)
    expected = _be32s(r[:, 52:56]).astype(np.uint32)[inverse]
    if record_crcs is not None:
        crcs = np.asarray(record_crcs, np.uint32)[index]
    else:
        crcs = np.array([crc32c(data[a:a + ln].tobytes()) for a, ln in zip(
            (at + hs + opt).tolist(), (rec - hs - opt - pad8).tolist())], np.uint32)[inverse]
    wrong = np.flatnonzero(expected != crcs)
    result.update(n_bad=int(wrong.size), first_bad=int(wrong[0]) if wrong.size else n)
    return Packed(events, offsets.astype(np.uint64), crcs, length.astype(np.uint32), expected,
                  result)
