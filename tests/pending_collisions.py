"""Messages, confirms, deletions and queue keys chosen to collide in the two
open-addressing tables of bmqcrc_pending_records_list (no test in here:
test_pending_collisions.py checks what this module claims on the CPU and holds
the device to the model on it).

The call's JoinTable is the one join_collisions.py restates (key_hash of the
GUID and the queue key).  Its queue table is crc32c_join_key.h's QueueTable: a
power of two of slots, at least twice the queues, probed with (s + 1) & mask
from key_hash of the queue key under the null GUID -- the walk
expire_collisions.py restates for the expire call's own copy, so its
`queue_home`, `queue_slots` and `queue_colliders` serve here as they are, and
test_pending_collisions.py compares the header's text with MIRRORED below.
The model knows nothing of any hash."""
import functools

import numpy as np

import expire_collisions as X
import join_collisions as J
import pending_list_cases as C

# The bodies the restatement was written from, whitespace-normalised: (the text
# the body follows, the body), all of crc32c_join_key.h.
MIRRORED = {
    "table_key": (
        "JoinKey table_key(uint32_t q0, uint32_t q1)",
        "{ return {{0u, 0u, 0u, 0u}, q0, q1}; }"),
    "table_key_of": (
        "JoinKey table_key_of(const QueueTable& t, uint64_t e)",
        "{ const uint8_t null_guid[16] = {0}; return join_key_bytes(null_guid, t.keys + 5 * e); }"),
}
# ... and how both walks start and step
WALK = ("const uint64_t mask = t.slots - 1; uint64_t s = key_hash(k) & mask; for (uint64_t "
        "step = 0; step < t.slots; ++step, s = (s + 1) & mask) {")

QUEUES, ABSENT_QUEUES = 24, 4       # colliding queue keys in the table, and not in it
MESSAGES, ABSENT = 150, 30          # colliding message keys in the run, and named by no MESSAGE
APPS = 3


def guids_colliding(queue_keys, slots, home, count, seed):
    """`count` (GUID, queue key) pairs, the queue keys taken in turn from
    `queue_keys`, whose home in a JoinTable of `slots` is `home`.  A seeded
    search."""
    rng = np.random.default_rng([seed, slots, home])
    found = []
    keys = np.frombuffer(b"".join(queue_keys), np.uint8).reshape(-1, 5)
    for _ in range(64):
        rows = np.zeros((1 << 18, 21), np.uint8)
        rows[:, :16] = rng.integers(0, 256, size=(rows.shape[0], 16), dtype=np.uint8)
        rows[:, 16:] = keys[np.arange(rows.shape[0]) % keys.shape[0]]
        for r in rows[np.flatnonzero(J.key_hash(rows, slots) == home)]:
            found.append((r[:16].tobytes(), r[16:].tobytes()))
            if len(found) == count:
                return found
    raise AssertionError("no %d keys with home %d of %d" % (count, home, slots))


def _case(types, pairs, app_keys_of, table_keys, n_apps_each=APPS, seed=7):
    rng = np.random.default_rng(seed)
    n = len(types)
    queue_keys = np.frombuffer(b"".join(p[1] for p in pairs), np.uint8).reshape(n, 5)
    guid_rows = np.frombuffer(b"".join(p[0] for p in pairs), np.uint8).reshape(n, 16)
    run = C.records(types, queue_keys, guid_rows, app_keys_of)
    n_queues = len(table_keys)
    app_first = (n_apps_each * np.arange(n_queues + 1)).astype(np.uint64)
    n_apps = n_apps_each * n_queues
    app_keys = np.zeros((n_apps, 5), np.uint8)
    app_keys[:, 0] = np.arange(n_apps) % n_apps_each + 1
    app_keys[:, 1:] = rng.integers(0, 256, size=(n_apps, 4), dtype=np.uint8)
    run.setflags(write=False)
    return C.Case(run, np.frombuffer(b"".join(table_keys), np.uint8), app_first,
                  app_keys.reshape(-1), (100 + np.arange(n_apps)).astype(np.int32),
                  (7 * np.arange(n_apps)).astype(np.uint32), None, None, None), app_keys


@functools.lru_cache(maxsize=None)
def both_chains():
    """QUEUES queue keys with one home three slots before the queue table's end
    (and ABSENT_QUEUES more with that home that are not in the table), and
    MESSAGES MESSAGE records of them whose (GUID, queue key) all have one home
    eight slots before the JoinTable's end.  Behind them, shuffled: a CONFIRM
    record for the second app of every third message, a DELETION record for
    every tenth, and CONFIRM and DELETION records of ABSENT more keys with the
    same home that no MESSAGE record has.  Returns (case, info)."""
    confirmed = [i for i in range(MESSAGES) if i % 3 == 0]
    deleted = [i for i in range(MESSAGES) if i % 10 == 5]
    n = MESSAGES + len(confirmed) + len(deleted) + ABSENT
    slots, qslots = J.join_slots(n), X.queue_slots(QUEUES)
    home, qhome = slots - 8, qslots - 3
    qkeys = X.queue_colliders(qslots, qhome, QUEUES + ABSENT_QUEUES, 71)
    pairs = guids_colliding(qkeys, slots, home, MESSAGES + ABSENT, 72)
    rng = np.random.default_rng(73)
    table_order = rng.permutation(QUEUES).tolist()
    table_keys = [qkeys[k] for k in table_order]
    entry = {key: q for q, key in enumerate(table_keys)}
    _, app_keys = _case([C.MESSAGE], pairs[:1], None, table_keys)
    rest = [(C.CONFIRM, i) for i in confirmed] + [(C.DELETION, i) for i in deleted] + \
        [(C.CONFIRM if k % 2 else C.DELETION, MESSAGES + k) for k in range(ABSENT)]
    rest = [rest[i] for i in rng.permutation(len(rest))]
    order = [(C.MESSAGE, i) for i in rng.permutation(MESSAGES).tolist()] + rest
    types = [t for t, _ in order]
    keys_of = np.zeros((n, 5), np.uint8)
    for r, (t, i) in enumerate(order):
        if t == C.CONFIRM:
            q = entry.get(pairs[i][1], 0)
            keys_of[r] = app_keys[APPS * q + 1]
    case, _ = _case(types, [pairs[i] for _, i in order], keys_of, table_keys)
    in_table = [pairs[i][1] in entry for i in range(MESSAGES)]
    info = dict(slots=slots, home=home, qslots=qslots, qhome=qhome, pairs=pairs, qkeys=qkeys,
                n_no_queue=sum(1 for i in range(MESSAGES) if not in_table[i] and i not in deleted),
                n_unknown=sum(1 for i in confirmed if not in_table[i]),
                n_not_found=sum(1 for k in range(ABSENT) if k % 2),
                n_live=MESSAGES - len(deleted),
                n_pending=sum(APPS - (1 if i in confirmed else 0) for i in range(MESSAGES)
                              if in_table[i] and i not in deleted))
    return case, info


@functools.lru_cache(maxsize=None)
def duplicate_message_behind_the_chain():
    """both_chains' run with its last MESSAGE record's key once more at the
    end: the duplicate is met at the chain's end, across the table's end."""
    case, info = both_chains()
    rows = case.run.reshape(-1, 60)
    last = int(np.flatnonzero(rows[:, 0] >> 4 == C.MESSAGE)[-1])
    run = np.concatenate([case.run, rows[last]])
    return case._replace(run=run), last


@functools.lru_cache(maxsize=None)
def duplicate_queue_behind_the_chain():
    """both_chains' table with its last queue key once more in a further
    entry of no apps."""
    case, info = both_chains()
    keys = case.queue_keys.reshape(-1, 5)
    first = np.concatenate([case.app_first, case.app_first[-1:]])
    return case._replace(queue_keys=np.concatenate([keys, keys[-1:]]).reshape(-1),
                         app_first=first), QUEUES - 1
