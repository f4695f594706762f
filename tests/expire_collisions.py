"""Queue keys and messages chosen to collide in the two open-addressing tables
of bmqcrc_expire_records_pack (no test in here: test_expire_collisions.py checks
what this module claims on the CPU, test_gpu_expire_records.py holds the device
to the model on it).

The call's JoinTable is the one join_collisions.py crafts runs for; those runs
serve here as they are.  Its second table holds the queue table's entries: a
power of two of slots, at least twice the entries, probed with (s + 1) & mask
from key_hash of the queue key under the null GUID -- so `queue_home` is
join_collisions.key_hash of 16 zero bytes and the key, and
test_expire_collisions.py compares the kernel's own text with MIRRORED below.
The model knows nothing of any hash and stays the reference for whatever keys
are picked."""
import collections
import functools

import numpy as np

from blazingmq_amd import storage as S
import expire_records_cases as C
import join_collisions as J

JH = S.PartitionWriter.JOURNAL_HEADER
NULL_GUID = bytes(16)

# The bodies the restatement was written from, whitespace-normalised: (the text
# the body follows, the body), all of crc32c_expire_records.hip.
MIRRORED = {
    "queue_key": (
        "JoinKey queue_key(uint32_t q0, uint32_t q1)",
        "{ return {{0u, 0u, 0u, 0u}, q0, q1}; }"),
    "queue_key_of": (
        "JoinKey queue_key_of(const ExpArgs& a, uint64_t e)",
        "{ const uint8_t null_guid[16] = {0}; return join_key_bytes(null_guid, a.queue_keys + "
        "5 * e); }"),
}
# ... and how both walks start and step
WALK = ("const uint64_t mask = a.qslots - 1; uint64_t s = key_hash(k) & mask; for (uint64_t "
        "step = 0; step < a.qslots; ++step, s = (s + 1) & mask) {")


def queue_home(keys, slots):
    """Home slots of 5-byte queue keys in the queue table's hash of `slots`."""
    return J.key_hash([NULL_GUID + bytes(k) for k in keys], slots)


def queue_slots(n_queues):
    """Slots of the queue table's hash as the host sizes it, n_queues > 0."""
    return J.join_slots(n_queues)


@functools.lru_cache(maxsize=None)
def queue_colliders(slots, home, count, seed):
    """`count` distinct queue keys without a zero byte whose home slot in a
    table of `slots` is `home`, as a tuple of bytes.  A seeded search."""
    rng = np.random.default_rng([seed, slots, home])
    found = {}
    for _ in range(64 + 8 * count * slots // (1 << 20)):
        raw = rng.integers(1, 256, size=(1 << 20, 5), dtype=np.uint8)
        rows = np.zeros((raw.shape[0], 21), np.uint8)
        rows[:, 16:] = raw
        for r in raw[np.flatnonzero(J.key_hash(rows, slots) == home)]:
            found.setdefault(r.tobytes(), None)
            if len(found) == count:
                return tuple(found)
    raise AssertionError("no %d queue keys with home %d of %d" % (count, home, slots))


Crafted = collections.namedtuple("Crafted", "run table kw slots home keys info")
NOW, TS = 5000, 4000          # every crafted message is 1,000 seconds old
CHAIN, ABSENT = 200, 40
LONG = 1100
BEHIND = 100


def _finish(w, entries, n_table):
    run = w.files()[0][JH:].copy()
    run.setflags(write=False)
    assert len(entries) == n_table
    return run, C.table(entries), dict(now=NOW, lease_id=7, first_seq=w.seq + 1)


@functools.lru_cache(maxsize=None)
def queue_chain():
    """CHAIN queue keys whose home is eight slots before the table's end, in a
    table of CHAIN entries (TTL 500 and 2,000 in turn), and ABSENT keys with the
    same home that are not in it.  Two messages of every queue, shuffled; of
    every tenth queue the first message is deleted by a DELETION record."""
    slots = queue_slots(CHAIN)
    home = slots - 8
    keys = queue_colliders(slots, home, CHAIN + ABSENT, 61)
    rng = np.random.default_rng(62)
    w = S.PartitionWriter(lease_id=7)
    w.queue_op(S.OP_CREATION, keys[0])
    order = rng.permutation(np.repeat(np.arange(CHAIN + ABSENT), 2))
    seen, gone = set(), []
    for k in order.tolist():
        guid = w.message(b"", keys[k], timestamp=TS)[1]
        if k % 10 == 0 and k not in seen:
            gone.append((guid, keys[k]))
        seen.add(k)
    for guid, key in gone:
        w.deletion(guid, key)
    table_order = rng.permutation(CHAIN).tolist()
    entries = [(keys[k], 500 if k % 2 == 0 else 2000) for k in table_order]
    run, table, kw = _finish(w, entries, CHAIN)
    info = dict(n_expired=2 * (CHAIN // 2) - sum(1 for _, key in gone
                                                 if keys.index(key) < CHAIN),
                n_no_queue=2 * ABSENT - sum(1 for _, key in gone if keys.index(key) >= CHAIN),
                table_order=table_order)
    return Crafted(run, table, kw, slots, home, keys, info)


@functools.lru_cache(maxsize=None)
def queue_long():
    """LONG queue keys with one home, a chain longer than a block of threads,
    across the table's end; one message each, all expired."""
    slots = queue_slots(LONG)
    home = slots - 300
    keys = queue_colliders(slots, home, LONG, 63)
    w = S.PartitionWriter(lease_id=7)
    for k in np.random.default_rng(64).permutation(LONG).tolist():
        w.message(b"", keys[k], timestamp=TS)
    run, table, kw = _finish(w, [(k, 10) for k in keys], LONG)
    return Crafted(run, table, kw, slots, home, keys, {})


@functools.lru_cache(maxsize=None)
def queue_duplicate():
    """BEHIND queue keys in one chain, the last key in a second entry at the
    table's end."""
    slots = queue_slots(BEHIND + 1)
    home = slots - 8
    keys = queue_colliders(slots, home, BEHIND, 65)
    w = S.PartitionWriter(lease_id=7)
    for key in keys[:5]:
        w.message(b"", key, timestamp=TS)
    run, table, kw = _finish(w, [(k, 10) for k in keys + keys[-1:]], BEHIND + 1)
    return Crafted(run, table, kw, slots, home, keys, {})
