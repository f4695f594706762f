"""A numpy model of bmqcrc_partition_rollover (ABI 2.18): what the call writes,
what it reports and what it refuses, with the precedence of refusals.  It
restates the reference's loop -- FileStore::rolloverImpl walking d_records and
handing each record to FileStore::writeRolledOverRecord, then writing one sync
point behind them -- for a d_records that holds exactly the kept records in run
order, in a cluster that is not QLIST aware:

  * a MESSAGE record's whole DATA record (4 x DataHeader.messageWords bytes) is
    copied to the new DATA file's position, which advances by that much, and
    its journal record is copied with MessageOffsetDwords set to the position
    the DATA record went to, in dwords;
  * a QUEUE_OP CREATION / ADDITION record is copied with
    queueUriRecordOffsetWords set to 0 (newQlistOffset stays 0);
  * every other kept record is copied as it is;
  * the sync point takes the PSN of the run's sync point in header and body, the
    new timestamp, sync point type REGULAR and the new DATA file's position.

The GPU tests compare the device against it; tests/test_rollover_model.py holds
it to hand-written journals, the reference's fixture partition, the recovery
walk and a dictionary restatement of the CONFIRM join.

The checksum to compare with is the caller's (``crc32c``).
"""
import collections

import numpy as np

(OK, RECORD_HEADER, KEEP_JOURNAL_OP, SYNC_POINT, DATA_OFFSET, DATA_RECORD, DST_TOO_SMALL,
 DATA_FILE_FULL, TOO_MANY_PIECES) = range(9)
CONFIRMS_AS_KEPT, CONFIRMS_FOLLOW_MESSAGES = 0, 1
MAX_FILE_BYTES = 8 * 0xFFFFFFFF   # where MessageOffsetDwords stops
MAGIC = bytes([0x2A, 0x72, 0x45, 0x63])
NOT_KEPT = 0xFFFFFFFF

Refusal = collections.namedtuple("Refusal", "kind index")
Rolled = collections.namedtuple("Rolled", "data journal new_index crcs result")
_Data = collections.namedtuple("_Data", "at rec hdr length")   # `at`: the DATA record in the window


def _be32(a, at):
    return int.from_bytes(a[at:at + 4].tobytes(), "big")


def _header_ok(r):
    rtype = int(r[0]) >> 4
    seq = int.from_bytes(r[2:8].tobytes(), "big")
    if rtype == 0 or rtype > 5 or _be32(r, 8) == 0 or seq == 0 or r[56:60].tobytes() != MAGIC:
        return False
    return rtype != 4 or 1 <= _be32(r, 32) <= 4


def _data_record(r, data, data_file_pos):
    """(_Data, None) or (None, kind) for the MESSAGE record r."""
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
    return _Data(ow, rec, hs + opt, rec - hs - opt - pad), None


def _keys(recs, guid_at):
    """One row of 21 bytes per record: the GUID and the queue key."""
    return np.ascontiguousarray(np.concatenate([recs[:, guid_at:guid_at + 16], recs[:, 22:27]], 1))


def kept_records(recs, keep, confirm_mode):
    """Which records are rolled, as a bool array; JOURNAL_OP records never are.
    (The refusal for a non-zero keep on one is rollover()'s.)"""
    n = recs.shape[0]
    types = recs[:, 0] >> 4
    want = np.ones(n, bool) if keep is None else np.asarray(keep, np.uint8) != 0
    kept = want & (types != 5)
    if confirm_mode == CONFIRMS_FOLLOW_MESSAGES:
        confirms = types == 2
        rows = np.dtype((np.void, 21))
        have = _keys(recs[kept & (types == 1)], 36).view(rows).reshape(-1)
        asked = _keys(recs[confirms], 32).view(rows).reshape(-1)
        kept[confirms] = np.isin(asked, have)
    return kept


def sync_point_record(s, timestamp, data_file_end):
    """The first sync point of the new journal, from the run's sync point `s`."""
    o = np.zeros(60, np.uint8)
    o[0] = 0x50
    o[2:12] = s[2:12]
    o[12:20] = np.frombuffer(int(timestamp).to_bytes(8, "big"), np.uint8)
    o[23] = 1
    o[24:28] = np.frombuffer((2).to_bytes(4, "big"), np.uint8)
    o[28:44] = s[28:44]
    o[44:48] = np.frombuffer((data_file_end // 8).to_bytes(4, "big"), np.uint8)
    o[56:60] = np.frombuffer(MAGIC, np.uint8)
    return o


def rollover(journal, data, *, data_file_pos, new_data_file_pos, keep=None,
             confirm_mode=CONFIRMS_AS_KEPT, sync_point=None, timestamp=0, dst_bytes,
             journal_dst_bytes, crc32c):
    """The call on host arrays.  ``sync_point`` None: none is restated.
    ``crc32c(bytes) -> int`` is the checksum to compare with.  Returns a
    ``Refusal`` (nothing is written then) or a ``Rolled`` whose ``data`` and
    ``journal`` are the bytes written and ``result`` the result struct's
    fields."""
    recs = np.asarray(journal, np.uint8).reshape(-1, 60)
    data = np.asarray(data, np.uint8)
    n = recs.shape[0]
    if n == 0:
        return Rolled(np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(0, np.uint32),
                      np.zeros(0, np.uint32),
                      dict(n_records=0, n_kept=0, n_messages=0, journal_bytes=0, data_bytes=0,
                           n_bad=0, first_bad=0, refused_kind=0, refused_index=0))
    types = recs[:, 0] >> 4
    bad = [(RECORD_HEADER, i) for i in range(n) if not _header_ok(recs[i])]
    if keep is not None:
        bad += [(KEEP_JOURNAL_OP, int(i))
                for i in np.flatnonzero((types == 5) & (np.asarray(keep, np.uint8) != 0))]
    if sync_point is not None and not (types[sync_point] == 5 and
                                       _be32(recs[sync_point], 24) == 2):
        bad.append((SYNC_POINT, sync_point))
    kept = kept_records(recs, keep, confirm_mode)
    found = {}
    for i in np.flatnonzero(kept & (types == 1)):
        found[int(i)], kind = _data_record(recs[i], data, data_file_pos)
        if kind:
            bad.append((kind, int(i)))
    if bad:   # the lowest kind wins, within it the lowest index
        return Refusal(*min(bad))
    # the loop: positions first, so that nothing is written when a bound is passed
    order = [int(i) for i in np.flatnonzero(kept)]
    q, where = 0, {}
    for i in order:
        if i in found:
            where[i] = q
            q += found[i].rec
    full = [i for i in order if i in found and new_data_file_pos + where[i] + found[i].rec >
            MAX_FILE_BYTES]
    small = [i for j, i in enumerate(order)
             if 60 * (j + 1) > journal_dst_bytes or
             (i in found and where[i] + found[i].rec > dst_bytes)]
    if sync_point is not None and 60 * (len(order) + 1) > journal_dst_bytes:
        small.append(n)
    if new_data_file_pos > MAX_FILE_BYTES:
        full.append(n)
    if small:
        return Refusal(DST_TOO_SMALL, small[0])
    if full:
        return Refusal(DATA_FILE_FULL, full[0])
    if sum(((d.length + 15) >> 4) + 1 for d in found.values() if d.length) > 0xFFFFFFFF:
        return Refusal(TOO_MANY_PIECES, 0)
    new_data, new_journal = [], []
    new_index = np.full(n, NOT_KEPT, np.uint32)
    crcs, wrong = np.zeros(n, np.uint32), []
    for j, i in enumerate(order):
        r = recs[i].copy()
        if i in found:
            d = found[i]
            new_data.append(data[d.at:d.at + d.rec])
            r[32:36] = np.frombuffer(((new_data_file_pos + where[i]) // 8).to_bytes(4, "big"),
                                     np.uint8)
            crcs[i] = crc32c(data[d.at + d.hdr:d.at + d.hdr + d.length].tobytes())
            if int(crcs[i]) != _be32(r, 52):
                wrong.append(i)
        elif types[i] == 4 and _be32(r, 32) in (2, 4):
            r[36:40] = 0
        new_journal.append(r)
        new_index[i] = j
    if sync_point is not None:
        new_journal.append(sync_point_record(recs[sync_point], timestamp, new_data_file_pos + q))
    out_data = np.concatenate(new_data + [np.zeros(0, np.uint8)])
    out_journal = np.concatenate(new_journal + [np.zeros(0, np.uint8)])
    result = dict(n_records=n, n_kept=len(order), n_messages=len(found),
                  journal_bytes=out_journal.size, data_bytes=out_data.size, n_bad=len(wrong),
                  first_bad=wrong[0] if wrong else n, refused_kind=0, refused_index=0)
    return Rolled(out_data, out_journal, new_index, crcs, result)


def refused_result(r, n_records):
    """The result struct's fields after the refusal `r`."""
    return dict(n_records=n_records, n_kept=0, n_messages=0, journal_bytes=0, data_bytes=0,
                n_bad=0, first_bad=0, refused_kind=r.kind, refused_index=r.index)
