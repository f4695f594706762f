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
