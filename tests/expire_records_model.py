"""A numpy model of bmqcrc_expire_records_pack (ABI 2.20): what the call
writes, what it reports and what it refuses, with the precedence of refusals.
It restates the reference's sequential path, not the device's reductions:

  * recovery (FileBackedStorage::processMessageRecord / processDeletionRecord):
    per queue key a dictionary ``d_handles`` from GUID to the MESSAGE record,
    in journal order (an ordered map, as the reference's), filled from the
    selected MESSAGE records of the run and emptied of every key a DELETION
    record names;
  * the garbage collection (FileStore::gcExpiredMessages over every storage,
    FileBackedStorage::gcExpiredMessages with no limit): per queue that has an
    entry in the table, walk ``d_handles`` from its head; a message for which
    ``secondsFromEpoch - timestamp <= d_ttlSeconds`` in unsigned 64-bit
    arithmetic has not expired and ends the walk; every message before it gets
    a DELETION record flagged e_TTL_EXPIRATION with ``secondsFromEpoch`` as its
    timestamp and leaves the dictionary.

Where the call differs from the reference the model follows the call: the
records come out in journal order (the reference visits storages in its map's
order), so the deleted messages are sorted by record before they are written.

The GPU tests compare the device against it; tests/test_expire_records_model.py
holds it to hand-written journals and the reference's fixture partition.
"""
import collections

import numpy as np

OK, RECORD_HEADER, DUPLICATE_MESSAGE, QUEUE_KEY, DST_TOO_SMALL = range(5)
TTL_EXPIRATION = 2
MAGIC = bytes([0x2A, 0x72, 0x45, 0x63])
NONE = 0xFFFFFFFF
M64 = (1 << 64) - 1

Refusal = collections.namedtuple("Refusal", "kind index")
Expired = collections.namedtuple(
    "Expired", "journal expired new_index select_out queue_expired queue_front result")


def _be(recs, at, n):
    """Bytes at..at+n of every record as one big-endian integer."""
    v = np.zeros(recs.shape[0], np.uint64)
    for k in range(n):
        v = (v << np.uint64(8)) | recs[:, at + k].astype(np.uint64)
    return v


def _headers_ok(recs):
    rtype = recs[:, 0] >> 4
    ok = (rtype >= 1) & (rtype <= 5) & (_be(recs, 8, 4) != 0) & (_be(recs, 2, 6) != 0)
    ok &= (recs[:, 56:60] == np.frombuffer(MAGIC, np.uint8)).all(axis=1)
    op = _be(recs, 32, 4)
    return ok & ((rtype != 4) | ((op >= 1) & (op <= 4)))


def _deletion(seq, lease_id, now, queue_key, guid):
    r = bytearray(60)
    r[0:2] = ((3 << 12) | TTL_EXPIRATION).to_bytes(2, "big")
    r[2:8] = int(seq).to_bytes(6, "big")
    r[8:12] = int(lease_id).to_bytes(4, "big")
    r[12:20] = (int(now) & M64).to_bytes(8, "big")
    r[23:28] = queue_key
    r[28:44] = guid
    r[56:60] = MAGIC
    return bytes(r)


def _rows(recs, lo, hi, which=None):
    """Bytes lo..hi of every record (or of the records `which`), as a
    dictionary from the record to its bytes."""
    which = np.arange(recs.shape[0]) if which is None else which
    width = hi - lo
    blob = np.ascontiguousarray(recs[which, lo:hi]).tobytes()
    return {r: blob[width * i:width * (i + 1)] for i, r in enumerate(which.tolist())}


def expire_records(journal, queue_keys, ttl_seconds, *, now, lease_id, first_seq, select=None,
                   journal_dst_bytes=None):
    """The call on host arrays.  ``journal_dst_bytes`` None: size only (no
    DST_TOO_SMALL).  Returns a ``Refusal`` (nothing is written then) or an
    ``Expired`` whose ``journal`` is the bytes written and ``result`` the
    result struct's fields."""
    recs = np.asarray(journal, np.uint8).reshape(-1, 60)
    table = np.asarray(queue_keys, np.uint8).reshape(-1, 5)
    ttls = [int(t) & M64 for t in np.asarray(ttl_seconds).reshape(-1).tolist()]
    n_records, n_queues = recs.shape[0], table.shape[0]
    assert len(ttls) == n_queues
    now = int(now) & M64
    if n_records == 0:      # nothing is launched: the table is not looked at
        return Expired(np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(0, np.uint32),
                       np.zeros(0, np.uint8), None, None,
                       dict(n_records=0, n_live=0, n_expired=0, n_no_queue=0, journal_bytes=0,
                            next_seq=first_seq, refused_kind=0, refused_index=0))
    bad = [(RECORD_HEADER, int(i)) for i in np.flatnonzero(~_headers_ok(recs))]
    types = recs[:, 0] >> 4
    stamps = _be(recs, 12, 8).tolist()
    # the table: d_ttlSeconds of every storage
    entry_of = {}
    for q, key in _rows(table, 0, 5).items():
        if not any(key):
            bad.append((QUEUE_KEY, q))
        elif key in entry_of:
            bad.append((QUEUE_KEY, entry_of[key]))      # the first is the lowest
        else:
            entry_of[key] = q
    # recovery: the messages every storage holds, then what the run deletes
    selected = types == 1 if select is None else (types == 1) & (np.asarray(select) != 0)
    selected = np.flatnonzero(selected)
    guid_m, key_m = _rows(recs, 36, 52, selected), _rows(recs, 22, 27, selected)
    d_handles, record_of = {}, {}
    for r in selected.tolist():
        key = (key_m[r], guid_m[r])
        if key in record_of:
            bad.append((DUPLICATE_MESSAGE, record_of[key]))   # the first is the lowest
            continue
        record_of[key] = r
        d_handles.setdefault(key_m[r], {})[guid_m[r]] = r
    deletions = np.flatnonzero(types == 3)
    guid_d, key_d = _rows(recs, 28, 44, deletions), _rows(recs, 23, 28, deletions)
    for r in deletions.tolist():
        d_handles.get(key_d[r], {}).pop(guid_d[r], None)
    # the garbage collection, storage by storage
    n_live = n_no_queue = 0
    deleted = []
    queue_expired = np.zeros(n_queues, np.uint32)
    queue_front = np.full(n_queues, NONE, np.uint32)
    for queue_key, handles in d_handles.items():
        n_live += len(handles)
        if queue_key not in entry_of:
            n_no_queue += len(handles)
            continue
        q = entry_of[queue_key]
        for guid, r in list(handles.items()):       # from the head, in arrival order
            if (now - stamps[r]) & M64 <= ttls[q]:
                queue_front[q] = r                  # has not expired: the walk ends here
                break
            deleted.append(r)
            del handles[guid]
            queue_expired[q] += 1
    deleted.sort()                                  # the call writes in journal order
    expired = np.zeros(n_records, np.uint8)
    new_index = np.full(n_records, NONE, np.uint32)
    out = []
    for j, r in enumerate(deleted):
        expired[r], new_index[r] = 1, j
        out.append(_deletion(first_seq + j, lease_id, now, key_m[r], guid_m[r]))
        if journal_dst_bytes is not None and 60 * (j + 1) > journal_dst_bytes:
            bad.append((DST_TOO_SMALL, r))
    if bad:   # the lowest kind wins, within it the lowest index
        return Refusal(*min(bad))
    select_out = np.zeros(n_records, np.uint8)
    for handles in d_handles.values():
        select_out[list(handles.values())] = 1
    result = dict(n_records=n_records, n_live=n_live, n_expired=len(out), n_no_queue=n_no_queue,
                  journal_bytes=60 * len(out), next_seq=first_seq + len(out), refused_kind=0,
                  refused_index=0)
    return Expired(np.frombuffer(b"".join(out), np.uint8).copy(), expired, new_index, select_out,
                   queue_expired, queue_front, result)


def refused_result(r, n_records):
    """The result struct's fields after the refusal `r`."""
    return dict(n_records=n_records, n_live=0, n_expired=0, n_no_queue=0, journal_bytes=0,
                next_seq=0, refused_kind=r.kind, refused_index=r.index)
