"""A sequential model of bmqcrc_pending_records_list (ABI 2.21): what the call
lists, what it reports and what it refuses, with the precedence of refusals.
It restates the reference's path, not the device's reductions and sort:

  * recovery: one storage per queue key (FileBackedStorage) with ``d_handles``,
    an ordered dictionary from GUID to the message's handle, and in every
    handle the set of app ordinals that have confirmed it (the virtual
    storages' state).  ``processMessageRecord`` fills it from the selected
    MESSAGE records in journal order; ``processConfirmRecord`` looks the
    handle up, counts a missing one, ignores the null app key, looks the app
    key up among the queue's apps (an unknown one is counted and ignored, as
    under #STORAGE_INVALID_CONFIRM) and marks the ordinal;
    ``processDeletionRecord`` removes the handle.
  * delivery: per queue of the table and per app of it,
    ``getIterator(appKey)``: walk ``d_handles`` from its head and skip what the
    app has confirmed (``VirtualStorageIterator::advance``) and what lies below
    the caller's cursor; stop listing at the caller's limit and remember the
    next one.

Where the call differs from the reference the model follows the call: a
CONFIRM record counts wherever it stands in the run (an auto-confirm may stand
before its message, and a late one behind the DELETION), so the three record
types are replayed in three walks -- messages, then confirms, then deletions --
each in journal order.

The GPU tests compare the device against it; tests/test_pending_list_model.py
holds it to the reference's own two iterator cases and hand-made journals.
"""
import collections

import numpy as np

from expire_records_model import _headers_ok, _rows

(OK, RECORD_HEADER, DUPLICATE_MESSAGE, QUEUE_KEY, APP_FIRST, APP_KEY, FROM_RECORD,
 LIST_TOO_SMALL) = range(8)
MAX_APPS = 32
NULL_KEY = bytes(5)
NO_LIMIT = 0xFFFFFFFF

Refusal = collections.namedtuple("Refusal", "kind index")
Pending = collections.namedtuple(
    "Pending", "records queue_ids sub_ids list_first app_pending app_next pending_mask result")


def _u32(values, n):
    return None if values is None else \
        (np.asarray(values).reshape(-1).astype(np.int64) & 0xFFFFFFFF).tolist()[:n]


def pending_records(journal, queue_keys, app_first, app_keys, queue_ids, *, sub_ids=None,
                    from_record=None, limit=None, select=None, list_cap=None):
    """The call on host arrays.  ``list_cap`` None: size only (no
    LIST_TOO_SMALL).  Returns a ``Refusal`` (nothing is written then) or a
    ``Pending`` whose lists hold the entries written and ``result`` the result
    struct's fields."""
    recs = np.asarray(journal, np.uint8).reshape(-1, 60)
    table = np.asarray(queue_keys, np.uint8).reshape(-1, 5)
    apps = np.asarray(app_keys, np.uint8).reshape(-1, 5)
    first = [int(f) & ((1 << 64) - 1) for f in np.asarray(app_first).reshape(-1).tolist()]
    n_records, n_queues, n_apps = recs.shape[0], table.shape[0], apps.shape[0]
    assert len(first) == n_queues + 1 and np.asarray(queue_ids).size == n_apps
    queue_ids = np.asarray(queue_ids).reshape(-1).astype(np.int32)
    sub_ids = None if sub_ids is None else \
        (np.asarray(sub_ids).reshape(-1).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)
    cursor, limits = _u32(from_record, n_apps), _u32(limit, n_apps)
    if n_records == 0:      # nothing is launched: the table is not looked at
        return Pending(np.zeros(0, np.uint32), np.zeros(0, np.int32),
                       None if sub_ids is None else np.zeros(0, np.uint32), None, None, None,
                       np.zeros(0, np.uint32),
                       dict(n_records=0, n_live=0, n_no_queue=0, n_pending=0, n_listed=0,
                            n_unknown_confirms=0, n_not_found=0, refused_kind=0, refused_index=0))
    bad = [(RECORD_HEADER, int(i)) for i in np.flatnonzero(~_headers_ok(recs))]
    types = recs[:, 0] >> 4
    # the table: one storage per queue, its virtual storages by ordinal
    entry_of = {}
    for q, key in _rows(table, 0, 5).items():
        if not any(key):
            bad.append((QUEUE_KEY, q))
        elif key in entry_of:
            bad.append((QUEUE_KEY, entry_of[key]))      # the first is the lowest
        else:
            entry_of[key] = q
    if first[0] != 0:
        bad.append((APP_FIRST, 0))
    if first[n_queues] != n_apps:
        bad.append((APP_FIRST, n_queues))
    app_key = _rows(apps, 0, 5)
    for q in range(n_queues):
        lo, hi = first[q], first[q + 1]
        if lo > hi or hi - lo > MAX_APPS:
            bad.append((APP_FIRST, q))
        elif hi <= n_apps:
            seen = {}
            for a in range(lo, hi):
                if app_key[a] in seen:
                    bad.append((APP_KEY, seen[app_key[a]]))     # the first is the lowest
                else:
                    seen[app_key[a]] = a
    if cursor is not None:
        bad += [(FROM_RECORD, a) for a in range(n_apps) if cursor[a] > n_records]
    # recovery, walk 1: processMessageRecord
    selected = types == 1 if select is None else (types == 1) & (np.asarray(select) != 0)
    selected = np.flatnonzero(selected)
    guid_m, key_m = _rows(recs, 36, 52, selected), _rows(recs, 22, 27, selected)
    storages = {}                                       # queue key -> d_handles
    for r in selected.tolist():
        handles = storages.setdefault(key_m[r], {})
        if guid_m[r] in handles:
            bad.append((DUPLICATE_MESSAGE, handles[guid_m[r]][0]))   # the first is the lowest
            continue
        handles[guid_m[r]] = (r, set())
    if bad:   # the lowest kind wins, within it the lowest index; such a table is never walked
        return Refusal(*min(bad))
    # walk 2: processConfirmRecord
    confirms = np.flatnonzero(types == 2)
    guid_c, key_c, app_c = (_rows(recs, 32, 48, confirms), _rows(recs, 22, 27, confirms),
                            _rows(recs, 27, 32, confirms))
    n_not_found = n_unknown = 0
    for r in confirms.tolist():
        handle = storages.get(key_c[r], {}).get(guid_c[r])
        if handle is None:
            n_not_found += 1
            continue
        if app_c[r] == NULL_KEY:
            continue
        q = entry_of.get(key_c[r])
        ordinal = None
        if q is not None:
            for o, a in enumerate(range(first[q], first[q + 1])):
                if app_key[a] == app_c[r]:
                    ordinal = o
                    break
        if ordinal is None:
            n_unknown += 1
        else:
            handle[1].add(ordinal)
    # walk 3: processDeletionRecord
    deletions = np.flatnonzero(types == 3)
    guid_d, key_d = _rows(recs, 28, 44, deletions), _rows(recs, 23, 28, deletions)
    for r in deletions.tolist():
        storages.get(key_d[r], {}).pop(guid_d[r], None)
    n_live = sum(len(h) for h in storages.values())
    n_no_queue = sum(len(h) for k, h in storages.items() if k not in entry_of)
    # delivery: getIterator(appKey) per queue and app, in table order
    pending_mask = np.zeros(n_records, np.uint32)
    out_records, out_queue_ids, out_sub_ids = [], [], []
    list_first = np.zeros(n_apps + 1, np.uint64)
    app_pending = np.zeros(n_apps, np.uint32)
    app_next = np.full(n_apps, n_records, np.uint32)
    by_app = {}
    for key, q in entry_of.items():
        handles = storages.get(key, {})
        for o, a in enumerate(range(first[q], first[q + 1])):
            start = cursor[a] if cursor is not None else 0
            mine = []
            for r, confirmed in handles.values():           # from the head, in arrival order
                if o in confirmed or r < start:             # advance() skips it
                    continue
                mine.append(r)
                pending_mask[r] |= np.uint32(1 << o)
            by_app[a] = mine
    n_pending = 0
    for a in range(n_apps):
        mine = by_app.get(a, [])
        cap = limits[a] if limits is not None else NO_LIMIT
        app_pending[a] = len(mine)
        n_pending += len(mine)
        if len(mine) > cap:
            app_next[a] = mine[cap]
        listed = mine[:cap]
        out_records += listed
        out_queue_ids += [int(queue_ids[a])] * len(listed)
        if sub_ids is not None:
            out_sub_ids += [int(sub_ids[a])] * len(listed)
        list_first[a + 1] = len(out_records)
        if list_cap is not None and len(out_records) > list_cap:
            return Refusal(LIST_TOO_SMALL, a)               # the first is the lowest
    assert n_pending < 1 << 32
    result = dict(n_records=n_records, n_live=n_live, n_no_queue=n_no_queue, n_pending=n_pending,
                  n_listed=len(out_records), n_unknown_confirms=n_unknown,
                  n_not_found=n_not_found, refused_kind=0, refused_index=0)
    return Pending(np.array(out_records, np.uint32), np.array(out_queue_ids, np.int32),
                   None if sub_ids is None else np.array(out_sub_ids, np.uint32), list_first,
                   app_pending, app_next, pending_mask, result)


def refused_result(r, n_records):
    """The result struct's fields after the refusal `r`."""
    return dict(n_records=n_records, n_live=0, n_no_queue=0, n_pending=0, n_listed=0,
                n_unknown_confirms=0, n_not_found=0, refused_kind=r.kind, refused_index=r.index)
