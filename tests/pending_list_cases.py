"""Journals and consumer tables for the tests of bmqcrc_pending_records_list
(no test in here).  Runs are written with numpy, a row per record, in the
layout PartitionWriter writes (test_pending_list_model.py holds the two to one
another), so that the large cases cost no Python per record."""
import collections

import numpy as np

MAGIC = (0x2A, 0x72, 0x45, 0x63)
MESSAGE, CONFIRM, DELETION, QUEUE_OP, JOURNAL_OP = 1, 2, 3, 4, 5
NULL_KEY = bytes(5)

Case = collections.namedtuple(
    "Case", "run queue_keys app_first app_keys queue_ids sub_ids from_record limit select")


def guids(ids):
    """The 16-byte GUIDs PartitionWriter gives messages 1, 2, ...: (n, 16)."""
    ids = np.asarray(ids, np.uint64)
    out = np.zeros((ids.size, 16), np.uint8)
    out[:, 0] = 0x40
    out[:, 8:] = ids.astype(">u8").view(np.uint8).reshape(-1, 8)
    return out


def records(types, queue_keys, guid_rows, app_keys=None, flags=None, lease_id=7,
            timestamp=0x6720EAB4):
    """A run of len(types) records: row i has type types[i], the queue key
    queue_keys[i] (n, 5), the GUID guid_rows[i] (n, 16) and, a CONFIRM record,
    the app key app_keys[i] (n, 5), each where its type keeps it; sequence
    numbers from 1 on.  QUEUE_OP records are ADDITIONs, JOURNAL_OP records sync
    points of no further content."""
    types = np.asarray(types, np.uint8)
    n = types.size
    r = np.zeros((n, 60), np.uint8)
    flags = np.zeros(n, np.uint16) if flags is None else np.asarray(flags, np.uint16)
    r[:, 0] = (types << 4) | (flags >> 8).astype(np.uint8)
    r[:, 1] = flags & 0xFF
    r[:, 2:8] = (np.arange(1, n + 1, dtype=np.uint64)).astype(">u8").view(np.uint8).reshape(
        -1, 8)[:, 2:]
    r[:, 8:12] = np.frombuffer(int(lease_id).to_bytes(4, "big"), np.uint8)
    r[:, 12:20] = np.frombuffer(int(timestamp).to_bytes(8, "big"), np.uint8)
    r[:, 56:60] = MAGIC
    queue_keys = np.asarray(queue_keys, np.uint8).reshape(n, 5)
    guid_rows = np.asarray(guid_rows, np.uint8).reshape(n, 16)
    m, c, d, o = (types == t for t in (MESSAGE, CONFIRM, DELETION, QUEUE_OP))
    r[m, 22:27], r[m, 36:52] = queue_keys[m], guid_rows[m]
    r[m, 1] |= 1                                    # refCount 1
    r[c, 22:27], r[c, 32:48] = queue_keys[c], guid_rows[c]
    if app_keys is not None:
        r[c, 27:32] = np.asarray(app_keys, np.uint8).reshape(n, 5)[c]
    r[d, 23:28], r[d, 28:44] = queue_keys[d], guid_rows[d]
    r[o, 22:27] = queue_keys[o]
    r[o, 35] = 4
    return r.reshape(-1)


def distinct_keys(rng, n):
    """n distinct 5-byte keys without a zero byte: (n, 5)."""
    keys = {}
    while len(keys) < n:
        for row in rng.integers(1, 256, size=(n, 5), dtype=np.uint8):
            keys.setdefault(row.tobytes(), None)
    return np.frombuffer(b"".join(list(keys)[:n]), np.uint8).reshape(n, 5).copy()


def table(rng, apps_per_queue, null_every=3):
    """(queue_keys, app_first, app_keys, queue_ids, sub_ids) of queues with the
    given numbers of apps: distinct queue keys, app keys distinct inside a queue
    (every `null_every`-th queue's first app has the null key), queue ids and
    sub ids that tell every app from every other."""
    counts = np.asarray(apps_per_queue, np.int64)
    n_queues, n_apps = counts.size, int(counts.sum())
    app_first = np.zeros(n_queues + 1, np.uint64)
    app_first[1:] = np.cumsum(counts)
    app_keys = np.zeros((n_apps, 5), np.uint8)
    if n_apps:
        # the ordinal in the first byte: distinct inside a queue whatever the rest
        ordinal = np.arange(n_apps) - np.repeat(app_first[:-1].astype(np.int64), counts)
        app_keys[:, 0] = ordinal + 1
        app_keys[:, 1:] = rng.integers(0, 256, size=(n_apps, 4), dtype=np.uint8)
        nulls = app_first[:-1][(np.arange(n_queues) % null_every == 0) & (counts > 0)]
        app_keys[nulls.astype(np.int64)] = 0
    queue_ids = (1000 + np.arange(n_apps)).astype(np.int32)
    sub_ids = (0xF0000000 + 7 * np.arange(n_apps)).astype(np.uint32)
    return distinct_keys(rng, n_queues), app_first, app_keys, queue_ids, sub_ids


def scenario(seed, n_records, apps_per_queue, *, p_message=0.6, p_confirm=0.25, p_deletion=0.08,
             cursors=True, limits=True, absent_queue=True, select_some=True):
    """A random run over a table of queues with the given app counts: MESSAGE
    records of every queue (and, `absent_queue`, of one that is not in the
    table), CONFIRM records that name a message anywhere in the run -- before
    or behind it -- with an app key of its queue, the null key, a key no app has
    or a GUID no message has, DELETION records likewise, and QUEUE_OP and
    JOURNAL_OP records between them; cursors and limits per app; a selection
    that leaves some MESSAGE records out."""
    rng = np.random.default_rng(seed)
    queue_keys, app_first, app_keys, queue_ids, sub_ids = table(rng, apps_per_queue)
    n_queues, n_apps = queue_keys.shape[0], app_keys.shape[0]
    all_keys = np.concatenate([queue_keys, distinct_keys(rng, 1)]) if absent_queue or not n_queues \
        else queue_keys
    if n_records == 0:
        return Case(np.zeros(0, np.uint8), queue_keys.reshape(-1), app_first, app_keys.reshape(-1),
                    queue_ids, sub_ids, None, None, None)
    u = rng.random(n_records)
    types = np.full(n_records, JOURNAL_OP, np.uint8)
    types[u < p_message + p_confirm + p_deletion + 0.03] = QUEUE_OP
    types[u < p_message + p_confirm + p_deletion] = DELETION
    types[u < p_message + p_confirm] = CONFIRM
    types[u < p_message] = MESSAGE
    msgs = np.flatnonzero(types == MESSAGE)
    if msgs.size == 0:
        types[0] = MESSAGE
        msgs = np.array([0])
    queue_of = np.zeros(n_records, np.int64)
    queue_of[msgs] = rng.integers(0, all_keys.shape[0], size=msgs.size)
    ids = np.arange(1, n_records + 1, dtype=np.uint64)
    # a CONFIRM or DELETION record names a message somewhere in the run
    others = np.flatnonzero((types == CONFIRM) | (types == DELETION))
    named = msgs[rng.integers(0, msgs.size, size=others.size)]
    queue_of[others] = queue_of[named]
    ids[others] = ids[named]
    stray = others[rng.random(others.size) < 0.05]
    ids[stray] += 1 << 40                           # a GUID no message has
    keys_of = np.zeros((n_records, 5), np.uint8)
    confirms = np.flatnonzero(types == CONFIRM)
    if n_apps:
        q = np.minimum(queue_of[confirms], n_queues - 1)
        lo = app_first[q].astype(np.int64)
        cnt = app_first[q + 1].astype(np.int64) - lo
        pick = lo + (rng.integers(0, 1 << 30, size=confirms.size) % np.maximum(cnt, 1))
        keys_of[confirms] = app_keys[np.minimum(pick, n_apps - 1)]
        how = rng.random(confirms.size)
        keys_of[confirms[how < 0.05]] = 0                       # the null key
        keys_of[confirms[(how >= 0.05) & (how < 0.1)], 0] = 0xEE   # a key no app has
    run = records(types, all_keys[queue_of], guids(ids), keys_of,
                  flags=np.where(types == CONFIRM, rng.integers(0, 3, size=n_records), 0))
    from_record = rng.integers(0, max(n_records // 3, 1), size=n_apps).astype(np.uint32) \
        if cursors else None
    if cursors and n_apps:
        from_record[rng.random(n_apps) < 0.5] = 0
        from_record[-1] = n_records
    limit = None
    if limits:
        limit = rng.integers(0, 6, size=n_apps).astype(np.uint32)
        limit[rng.random(n_apps) < 0.6] = 0xFFFFFFFF
    select = None
    if select_some:
        select = (rng.random(n_records) < 0.95).astype(np.uint8)
    return Case(run, queue_keys.reshape(-1), app_first, app_keys.reshape(-1), queue_ids, sub_ids,
                from_record, limit, select)


def messages_only(n, apps_per_queue, seed=5, which=None):
    """n MESSAGE records and nothing else over a table with the given app
    counts, message i in queue i % n_queues (or in queue which[i]);
    no cursor, no limit, no selection: every message is pending for every app of
    its queue."""
    rng = np.random.default_rng(seed)
    queue_keys, app_first, app_keys, queue_ids, sub_ids = table(rng, apps_per_queue, null_every=2)
    n_queues = queue_keys.shape[0]
    which = np.arange(n) % n_queues if which is None else np.asarray(which, np.int64)
    run = records(np.full(n, MESSAGE, np.uint8), queue_keys[which], guids(np.arange(1, n + 1)))
    return Case(run, queue_keys.reshape(-1), app_first, app_keys.reshape(-1), queue_ids, sub_ids,
                None, None, None)


def model_args(c):
    """(args, kwargs) of pending_list_model.pending_records for the case."""
    return (c.run, c.queue_keys, c.app_first, c.app_keys, c.queue_ids), dict(
        sub_ids=c.sub_ids, from_record=c.from_record, limit=c.limit, select=c.select)
