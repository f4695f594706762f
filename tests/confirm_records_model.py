"""A numpy model of bmqcrc_confirm_records_pack (ABI 2.19): what the call
writes, what it reports and what it refuses, with the precedence of refusals.
It restates the reference's sequential path, not the device's reductions:

  * recovery (FileBackedStorage::processMessageRecord / processConfirmRecord /
    processDeletionRecord): a dictionary ``d_refCount`` from (GUID, queue key)
    to the outstanding count, filled from the selected MESSAGE records of the
    run, decremented (never below zero) by every CONFIRM record of the run
    that is not AUTO_CONFIRMED, and emptied of every key a DELETION record
    names;
  * the confirms (FileBackedStorage::confirm), one after the other: a key that
    is not in the dictionary is e_GUID_NOT_FOUND; otherwise the count is
    decremented, and when it reaches zero FileBackedStorage::remove writes the
    DELETION record in the CONFIRM record's place and drops the key, else
    FileStore::writeConfirmRecord appends the CONFIRM record.

Where the call differs from the reference the model follows the call: a key
that this very batch has brought to zero (or that was at zero already) and
that is confirmed again is OVER_CONFIRMED, not e_GUID_NOT_FOUND.

The GPU tests compare the device against it; tests/test_confirm_records_model.py
holds it to hand-written journals, the reference's fixture partition and the
recovery walk.
"""
import collections

import numpy as np

(OK, RECORD_HEADER, DUPLICATE_MESSAGE, NULL_KEY, REASON, OVER_CONFIRMED,
 DST_TOO_SMALL) = range(7)
STATUS_CONFIRM, STATUS_DELETION, STATUS_NOT_FOUND = 0, 1, 2
AUTO_CONFIRMED = 2
MAGIC = bytes([0x2A, 0x72, 0x45, 0x63])
NONE = 0xFFFFFFFF

Refusal = collections.namedtuple("Refusal", "kind index")
Confirmed = collections.namedtuple("Confirmed",
                                   "journal status target new_index left_out result")


def _be32(a, at):
    return int.from_bytes(a[at:at + 4].tobytes(), "big")


def _header_ok(r):
    rtype = int(r[0]) >> 4
    seq = int.from_bytes(r[2:8].tobytes(), "big")
    if rtype == 0 or rtype > 5 or _be32(r, 8) == 0 or seq == 0 or r[56:60].tobytes() != MAGIC:
        return False
    return rtype != 4 or 1 <= _be32(r, 32) <= 4


def _flags(r):
    return ((int(r[0]) & 0x0F) << 8) | int(r[1])


def _record(rtype, flags, seq, lease_id, timestamp, body):
    r = bytearray(60)
    r[0:2] = ((rtype << 12) | flags).to_bytes(2, "big")
    r[2:8] = int(seq).to_bytes(6, "big")
    r[8:12] = int(lease_id).to_bytes(4, "big")
    r[12:20] = (int(timestamp) & 0xFFFFFFFFFFFFFFFF).to_bytes(8, "big")
    for at, b in body:
        r[at:at + len(b)] = b
    r[56:60] = MAGIC
    return bytes(r)


def confirm_records(journal, guids, queue_keys, *, lease_id, first_seq, select=None,
                    app_keys=None, reasons=None, timestamp=0, timestamps=None,
                    journal_dst_bytes=None):
    """The call on host arrays.  ``journal_dst_bytes`` None: size only (no
    DST_TOO_SMALL).  Returns a ``Refusal`` (nothing is written then) or a
    ``Confirmed`` whose ``journal`` is the bytes written and ``result`` the
    result struct's fields."""
    recs = np.asarray(journal, np.uint8).reshape(-1, 60)
    guids = np.asarray(guids, np.uint8).reshape(-1, 16)
    queue_keys = np.asarray(queue_keys, np.uint8).reshape(-1, 5)
    n, n_records = guids.shape[0], recs.shape[0]
    if app_keys is not None:
        app_keys = np.asarray(app_keys, np.uint8).reshape(-1, 5)
    if n == 0:
        return Confirmed(np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(0, np.uint32),
                         np.zeros(0, np.uint32), np.zeros(n_records, np.uint32),
                         dict(n_confirms=0, n_written=0, n_confirm_records=0, n_deletions=0,
                              n_not_found=0, journal_bytes=0, next_seq=first_seq, refused_kind=0,
                              refused_index=0))
    bad = [(RECORD_HEADER, i) for i in range(n_records) if not _header_ok(recs[i])]
    types = recs[:, 0] >> 4
    # recovery: the messages, then what the run says about them
    d_ref_count, record_of = {}, {}
    for r in range(n_records):
        if types[r] == 1 and (select is None or select[r]):
            key = recs[r, 36:52].tobytes() + recs[r, 22:27].tobytes()
            if key in record_of:
                bad.append((DUPLICATE_MESSAGE, record_of[key]))   # the first is the lowest
                continue
            record_of[key] = r
            d_ref_count[key] = (int(recs[r, 20]) << 12) | _flags(recs[r])
    for r in range(n_records):
        if types[r] == 2 and _flags(recs[r]) != AUTO_CONFIRMED:
            key = recs[r, 32:48].tobytes() + recs[r, 22:27].tobytes()
            if d_ref_count.get(key, 0) > 0:
                d_ref_count[key] -= 1
    for r in range(n_records):
        if types[r] == 3:
            d_ref_count.pop(recs[r, 28:44].tobytes() + recs[r, 23:28].tobytes(), None)
    for i in range(n):
        if not guids[i].any() or not queue_keys[i].any():
            bad.append((NULL_KEY, i))
        if reasons is not None and reasons[i] > 1:
            bad.append((REASON, i))
    # the confirms, one after the other
    out, status = [], np.zeros(n, np.uint8)
    target, new_index = np.full(n, NONE, np.uint32), np.full(n, NONE, np.uint32)
    first_confirm, spent = {}, set()
    for i in range(n):
        key = guids[i].tobytes() + queue_keys[i].tobytes()
        if key in spent or d_ref_count.get(key, 1) == 0:
            bad.append((OVER_CONFIRMED, first_confirm.get(key, i)))
            target[i] = record_of[key]
            continue
        if key not in d_ref_count:
            status[i] = STATUS_NOT_FOUND
            continue
        first_confirm.setdefault(key, i)
        target[i], new_index[i] = record_of[key], len(out)
        ts = timestamp if timestamps is None else int(timestamps[i])
        d_ref_count[key] -= 1
        if d_ref_count[key] == 0:
            del d_ref_count[key]
            spent.add(key)
            status[i] = STATUS_DELETION
            out.append(_record(3, 0, first_seq + len(out), lease_id, ts,
                               [(23, queue_keys[i].tobytes()), (28, guids[i].tobytes())]))
        else:
            body = [(22, queue_keys[i].tobytes()), (32, guids[i].tobytes())]
            if app_keys is not None:
                body.append((27, app_keys[i].tobytes()))
            out.append(_record(2, 0 if reasons is None else int(reasons[i]),
                               first_seq + len(out), lease_id, ts, body))
        if journal_dst_bytes is not None and 60 * len(out) > journal_dst_bytes:
            bad.append((DST_TOO_SMALL, i))
    if bad:   # the lowest kind wins, within it the lowest index
        return Refusal(*min(bad))
    left_out = np.zeros(n_records, np.uint32)
    for key, left in d_ref_count.items():
        left_out[record_of[key]] = left
    n_del = int((status == STATUS_DELETION).sum())
    result = dict(n_confirms=n, n_written=len(out), n_confirm_records=len(out) - n_del,
                  n_deletions=n_del, n_not_found=int((status == STATUS_NOT_FOUND).sum()),
                  journal_bytes=60 * len(out), next_seq=first_seq + len(out), refused_kind=0,
                  refused_index=0)
    return Confirmed(np.frombuffer(b"".join(out), np.uint8).copy(), status, target, new_index,
                     left_out, result)


def refused_result(r, n):
    """The result struct's fields after the refusal `r`."""
    return dict(n_confirms=n, n_written=0, n_confirm_records=0, n_deletions=0, n_not_found=0,
                journal_bytes=0, next_seq=0, refused_kind=r.kind, refused_index=r.index)
