"""Keys chosen to collide in the device calls' open-addressing tables, and the
journals built from them (no test in here: test_join_collisions.py checks what
this module claims on the CPU, the three GPU files hold the device to the
models on it).

Three tables decide results on the device: the JoinTable of
crc32c_join_key.h (bmqcrc_partition_rollover in FOLLOW mode,
bmqcrc_confirm_records_pack) and the queue-key and GUID tables of
crc32c_journal_select.hip.  All are a power of two of slots probed with
(s + 1) & mask from a multiply-shift hash, so a key with a prescribed home slot
is found by hashing random keys: `colliders`.  The hashes are restated here in
numpy (`key_hash`, `guid_home`, `key_home`); test_join_collisions.py compares
the kernels' own text with MIRRORED below and fails when a hash changes under
its mirror.  The models know nothing of any hash and stay the reference for
whatever keys are picked.

A key is bytes: 21 for kind "join" (the GUID's 16, the queue key's 5), 16 for
"guid", 5 for "queue"."""
import collections
import functools

import numpy as np

from blazingmq_amd import storage as S

WIDTH = {"join": 21, "guid": 16, "queue": 5}

# The bodies the mirrors were written from, whitespace-normalised: (file under
# blazingmq_amd/csrc, the text the body follows, the body).
MIRRORED = {
    "key_hash": (
        "crc32c_join_key.h", "uint32_t key_hash(const JoinKey& k)",
        "{ uint32_t h = 0x9E3779B9u; const uint32_t w[6] = {k.g[0], k.g[1], k.g[2], k.g[3], "
        "k.q0, k.q1}; #pragma unroll for (uint32_t j = 0; j < 6; ++j) { h = (h ^ w[j]) * "
        "0x85EBCA6Bu; h ^= h >> 15; } h *= 0xC2B2AE35u; return h ^ (h >> 16); }"),
    "guid_home": (
        "crc32c_journal_select.hip",
        "uint64_t guid_home(const JselArgs& a, uint32_t g0, uint32_t g1, uint32_t g2, uint32_t g3)",
        "{ u64 h = ((u64)g1 << 32 | g0) * 0x9E3779B97F4A7C15ull; h ^= h >> 32; h += ((u64)g3 << 32 "
        "| g2) * 0xD6E8FEB86659FD93ull; h ^= h >> 32; h *= 0xFF51AFD7ED558CCDull; h ^= h >> 29; "
        "return h & (a.gslots - 1); }"),
    "key_home": (
        "crc32c_journal_select.hip", "uint64_t key_home(const JselArgs& a, u64 key)",
        "{ u64 h = key * 0x9E3779B97F4A7C15ull; h ^= h >> 29; return h & (a.qslots - 1); }"),
}


# ---- the hashes ----------------------------------------------------------------

def _rows(keys, width):
    """`keys` (a sequence of bytes or an array) as an (n, width) uint8 array."""
    if isinstance(keys, np.ndarray):
        a = keys.astype(np.uint8, copy=False)
    else:
        a = np.frombuffer(b"".join(bytes(k) for k in keys), np.uint8)
    return np.ascontiguousarray(a.reshape(-1, width))


def _le(rows, at, n, dtype):
    """Bytes at..at+n of every row as one little-endian integer."""
    v = np.zeros(rows.shape[0], dtype)
    for k in range(n):
        v |= rows[:, at + k].astype(dtype) << dtype(8 * k)
    return v


def join_words(keys):
    """The six words join_key forms from a record that holds these GUIDs and
    queue keys: g[0..3] as the GUID's dwords lie in memory, the queue key's
    first two bytes in q0 and the other three in q1."""
    rows = _rows(keys, 21)
    return np.stack([_le(rows, 4 * j, 4, np.uint32) for j in range(4)] +
                    [_le(rows, 16, 2, np.uint32), _le(rows, 18, 3, np.uint32)], axis=1)


def _key_hash_words(w, slots):
    h = np.full(w.shape[0], 0x9E3779B9, np.uint32)
    for j in range(6):
        h = (h ^ w[:, j]) * np.uint32(0x85EBCA6B)
        h ^= h >> np.uint32(15)
    h = h * np.uint32(0xC2B2AE35)
    return (h ^ (h >> np.uint32(16))) & np.uint32(slots - 1)


def key_hash(keys, slots):
    """Home slots of 21-byte join keys in a JoinTable of `slots`."""
    return _key_hash_words(join_words(keys), slots).astype(np.int64)


def _guid_home_words(lo, hi, slots):
    h = lo * np.uint64(0x9E3779B97F4A7C15)
    h ^= h >> np.uint64(32)
    h = h + hi * np.uint64(0xD6E8FEB86659FD93)
    h ^= h >> np.uint64(32)
    h = h * np.uint64(0xFF51AFD7ED558CCD)
    h ^= h >> np.uint64(29)
    return h & np.uint64(slots - 1)


def guid_home(keys, slots):
    """Home slots of 16-byte GUIDs in journal_select's table of DELETIONs."""
    rows = _rows(keys, 16)
    return _guid_home_words(_le(rows, 0, 8, np.uint64), _le(rows, 8, 8, np.uint64),
                            slots).astype(np.int64)


def _key_home_words(key, slots):
    h = key * np.uint64(0x9E3779B97F4A7C15)
    h ^= h >> np.uint64(29)
    return h & np.uint64(slots - 1)


def key_home(keys, slots):
    """Home slots of 5-byte queue keys in journal_select's queue table."""
    return _key_home_words(_le(_rows(keys, 5), 0, 5, np.uint64), slots).astype(np.int64)


HOME = {"join": key_hash, "guid": guid_home, "queue": key_home}


# ---- the tables as the host sizes them -------------------------------------------

def _pow2_at_least(v):
    p = 64
    while p < v:
        p <<= 1
    return p


def join_slots(n_records):
    """Slots of the JoinTable and of the GUID table for a run of `n_records`
    records of every type."""
    return _pow2_at_least(2 * n_records)


def queue_slots(queue_cap, n_records, n_queue_keys=0):
    """Slots of the queue table; `n_queue_keys` counts with CSL only."""
    return _pow2_at_least(2 * min(queue_cap, n_records + n_queue_keys))


# ---- keys with a prescribed home ----------------------------------------------

_KIND_SEED = {"join": 1, "guid": 2, "queue": 3}
_BATCH = 1 << 20


def _draw(kind, rng, high, batch=_BATCH):
    """(`batch` candidate keys as rows of bytes, their hashes' input).  Bytes come
    from 0..255; with `high` every queue-key byte is 0x80 or more."""
    if kind == "join":
        raw = rng.integers(0, 256, size=(batch, 24), dtype=np.uint8)
        if high:
            raw[:, 16:] |= 0x80
        w = raw.view(np.uint32) & np.array([0xFFFFFFFF] * 4 + [0xFFFF, 0xFFFFFF], np.uint32)
        return raw[:, [*range(16), 16, 17, 20, 21, 22]], w
    if kind == "guid":
        raw = rng.integers(0, 256, size=(batch, 16), dtype=np.uint8)
        return raw, raw.view(np.uint64)
    raw = rng.integers(0, 256, size=(batch, 8), dtype=np.uint8)
    if high:
        raw |= 0x80
    return raw[:, :5], raw.view(np.uint64)[:, 0] & np.uint64(0xFFFFFFFFFF)


def _homes_of(kind, w, slots):
    if kind == "join":
        return _key_hash_words(w, slots)
    if kind == "guid":
        return _guid_home_words(w[:, 0], w[:, 1], slots)
    return _key_home_words(w, slots)


def _non_null(kind, rows):
    ok = rows[:, :16].any(axis=1) if kind != "queue" else rows.any(axis=1)
    return ok & rows[:, 16:].any(axis=1) if kind == "join" else ok


@functools.lru_cache(maxsize=None)
def colliders(kind, slots, home, count, seed, high=False):
    """`count` distinct non-null keys whose home slot in a table of `slots` is
    `home`, as a tuple of bytes.  A seeded search: the same arguments give the
    same keys."""
    assert slots & (slots - 1) == 0 and 0 <= home < slots
    rng = np.random.default_rng([seed, _KIND_SEED[kind], slots, home])
    found = {}
    for _ in range(64 + 4 * count * slots // _BATCH):
        rows, w = _draw(kind, rng, high)
        hit = np.flatnonzero((_homes_of(kind, w, slots) == home) & _non_null(kind, rows))
        for r in rows[hit]:
            found.setdefault(r.tobytes(), None)
            if len(found) == count:
                return tuple(found)
    raise AssertionError("no %d %s keys with home %d of %d" % (count, kind, home, slots))


@functools.lru_cache(maxsize=None)
def near_pair(kind, slots, differ_at, seed, home=None):
    """Two non-null keys that differ in bit 0x80 of exactly one byte and share a
    home slot (`home`, when given).  `differ_at` counts over GUID bytes 0..15
    and queue-key bytes 16..20, whatever the kind holds of them.  key_hash has
    such pairs at every byte; the two hashes of journal_select move the home
    with some bits whatever the rest of the key (byte 15 of a GUID, bytes 0..3
    of a queue key in tables this small): the search fails there."""
    at = differ_at - 16 if kind == "queue" else differ_at
    assert 0 <= at < WIDTH[kind]
    # (guid_home adds that bit as 2^63, folds it to bit 31 and multiplies by an
    # odd number: bit 31 of the product always differs, and with it the home)
    assert (kind, at) != ("guid", 15), "bit 63 of guid_home's second word always moves the home"
    rng = np.random.default_rng([seed, _KIND_SEED[kind], slots, differ_at, 77])
    # the word of the hash's input that holds the byte, and the bit in it
    word, bit = {"join": (at // 4, 8 * (at % 4)) if at < 16 else
                         ((4, 8 * (at - 16)) if at < 18 else (5, 8 * (at - 18))),
                 "guid": (at // 8, 8 * (at % 8)), "queue": (0, 8 * at)}[kind]
    batch = min(_BATCH, 4 * slots * (slots if home is not None else 16))
    for _ in range(16):
        rows, w = _draw(kind, rng, False, batch)
        rows = rows.copy()
        rows[:, at] &= 0x7F
        w = w.copy()
        flip = w.dtype.type(0x80 << bit)
        if w.ndim == 1:
            w &= ~flip
            twin = w | flip
        else:
            w[:, word] &= ~flip
            twin = w.copy()
            twin[:, word] |= flip
        ha = _homes_of(kind, w, slots)
        same = (ha == _homes_of(kind, twin, slots)) & _non_null(kind, rows)
        if home is not None:
            same &= ha == home
        hit = np.flatnonzero(same)
        if hit.size:
            a = rows[hit[0]].tobytes()
            b = bytearray(a)
            b[at] |= 0x80
            return a, bytes(b)
    raise AssertionError("no near pair at byte %d of %d slots" % (differ_at, slots))


# ---- linear probing on the CPU -----------------------------------------------------

class Layout(collections.namedtuple("Layout", "slots slot steps clusters")):
    """What `probe_lengths` returns: `slot[i]` where key i went, `steps[i]` the
    slots its insert visited, `clusters` the maximal runs of taken slots as
    (first slot, length), a run that passes the last slot counted once."""

    def wraps(self):
        """Does a run of taken slots cross from the last slot to slot 0?"""
        return any(first + length > self.slots for first, length in self.clusters)

    def longest(self):
        return max(length for _, length in self.clusters)

    def walk(self, home):
        """Slots a probe from `home` visits up to and with the empty one."""
        for first, length in self.clusters:
            at = (home - first) % self.slots
            if at < length:
                return length - at + 1
        return 1


def probe_lengths(homes, slots):
    """Linear probing with (s + 1) & mask of keys with these home slots, one
    slot each, inserted in the given order."""
    taken = np.zeros(slots, bool)
    slot, steps = [], []
    for h in homes:
        s, k = int(h), 1
        while taken[s]:
            s, k = (s + 1) & (slots - 1), k + 1
            assert k <= slots
        taken[s] = True
        slot.append(s)
        steps.append(k)
    clusters = []
    free = np.flatnonzero(~taken)
    if free.size == 0:
        clusters.append((0, slots))
    elif taken.any():
        # walk once round the table from a free slot
        start = int(free[0])
        run = 0
        for k in range(1, slots + 1):
            s = (start + k) & (slots - 1)
            if taken[s]:
                run += 1
            elif run:
                clusters.append(((s - run) % slots, run))
                run = 0
    return Layout(slots, slot, steps, clusters)


# ---- the crafted runs --------------------------------------------------------------

JH = S.PartitionWriter.JOURNAL_HEADER
QUEUE = b"\x9C\xE1\x80\xFF\xB7"        # the CREATION record of the JoinTable runs
CHAIN, ABSENT_SAME, ABSENT_MID = 200, 40, 10
LONG, BEHIND, PAIRS = 1100, 100, 21

Crafted = collections.namedtuple("Crafted", "run data slots home keys info")


def split(key):
    return key[:16], key[16:]


def _finish(w, planned, slots):
    j, d = w.files()
    run = j[JH:].copy()
    assert run.size == 60 * planned and join_slots(planned) == slots
    run.setflags(write=False)
    d.setflags(write=False)
    return run, d


def _messages_then(w, keys, ref_count, rest, rng):
    """MESSAGE records of `keys` in run order, then `rest` (callables on the
    writer) shuffled.  Returns the record of each key."""
    record = {}
    for k, key in enumerate(keys):
        record.setdefault(key, len(w.recs))      # of a repeated key: the lowest
        w.message(bytes([k & 0xFF]) * (k % 5), split(key)[1], guid=split(key)[0],
                  ref_count=ref_count)
    for i in rng.permutation(len(rest)):
        rest[i](w)
    return record


@functools.lru_cache(maxsize=None)
def confirm_chain():
    """confirm_records: a CREATION and CHAIN MESSAGE records of refCount 3 whose
    keys all have home slots - 8 (every queue-key byte 0x80 or more), a third of
    them with one CONFIRM record, a tenth with a DELETION record.  info: the
    pairs of the live messages, the absent keys with the same home and the
    absent keys whose home lies mid-chain, the live messages' records."""
    confirmed = [i for i in range(CHAIN) if i % 3 == 0]
    deleted = [i for i in range(CHAIN) if i % 10 == 5]
    planned = 1 + CHAIN + len(confirmed) + len(deleted)
    slots = join_slots(planned)
    home = slots - 8
    keys = colliders("join", slots, home, CHAIN + ABSENT_SAME, 31, True)
    mid = colliders("join", slots, CHAIN // 2, ABSENT_MID, 32, True)
    w = S.PartitionWriter(lease_id=6)
    w.queue_op(S.OP_CREATION, QUEUE)
    rest = [lambda w, k=keys[i]: w.confirm(*split(k)) for i in confirmed] + \
           [lambda w, k=keys[i]: w.deletion(*split(k)) for i in deleted]
    record = _messages_then(w, keys[:CHAIN], 3, rest, np.random.default_rng(33))
    run, d = _finish(w, planned, slots)
    live = [keys[i] for i in range(CHAIN) if i not in deleted]
    info = dict(live=live, same=keys[CHAIN:], mid=mid, record=record, next_seq=w.seq + 1,
                lease_id=6)
    return Crafted(run, d, slots, home, keys[:CHAIN], info)


def confirm_chain_batch():
    """(pairs of the shuffled batch over confirm_chain: every live message
    once, the absent keys among them; per confirm the record it names or None)."""
    c = confirm_chain()
    pairs = list(c.info["live"]) + list(c.info["same"]) + list(c.info["mid"])
    order = np.random.default_rng(34).permutation(len(pairs))
    pairs = [pairs[i] for i in order]
    return [split(k) for k in pairs], [c.info["record"].get(k) for k in pairs]


def confirm_chain_select():
    """(select over confirm_chain's run with every collider but one live
    message unselected, that message's record)."""
    c = confirm_chain()
    only = c.info["record"][c.info["live"][77]]
    select = np.zeros(c.run.size // 60, np.uint8)
    select[[0, only]] = 1
    return select, only


def long_order():
    """The shuffled order confirm_long's messages are confirmed in."""
    return np.random.default_rng(38).permutation(LONG)


@functools.lru_cache(maxsize=None)
def confirm_long():
    """confirm_records: LONG MESSAGE records of refCount 1 with one home, a
    chain longer than a block of threads, across the table's end."""
    planned = 1 + LONG
    slots = join_slots(planned)
    home = slots - 300
    keys = colliders("join", slots, home, LONG, 35)
    w = S.PartitionWriter(lease_id=6)
    w.queue_op(S.OP_CREATION, QUEUE)
    record = _messages_then(w, keys, 1, [], np.random.default_rng(0))
    run, d = _finish(w, planned, slots)
    return Crafted(run, d, slots, home, keys, dict(record=record, next_seq=w.seq + 1, lease_id=6))


def _pairs(slots, swapped, seed):
    """The near pairs of all 21 key bytes in one chain from slots - 4, as
    (first in the run, its twin)."""
    home = slots - 4
    pairs = [near_pair("join", slots, b, seed, home) for b in range(PAIRS)]
    return home, [(b, a) if swapped else (a, b) for a, b in pairs]


@functools.lru_cache(maxsize=None)
def confirm_pairs(swapped):
    """confirm_records: for each of the 21 key bytes two MESSAGE records of
    refCount 1 that differ in that byte only, all 42 in one chain."""
    planned = 1 + 2 * PAIRS
    slots = join_slots(planned)
    home, pairs = _pairs(slots, swapped, 36)
    keys = [k for p in pairs for k in p]
    w = S.PartitionWriter(lease_id=6)
    w.queue_op(S.OP_CREATION, QUEUE)
    record = _messages_then(w, keys, 1, [], np.random.default_rng(0))
    run, d = _finish(w, planned, slots)
    return Crafted(run, d, slots, home, tuple(keys),
                   dict(pairs=pairs, record=record, next_seq=w.seq + 1, lease_id=6))


@functools.lru_cache(maxsize=None)
def confirm_duplicate():
    """confirm_records: BEHIND MESSAGE records in one chain, the last key under
    a second MESSAGE record at the run's end."""
    planned = 2 + BEHIND
    slots = join_slots(planned)
    home = slots - 8
    keys = colliders("join", slots, home, BEHIND, 37)
    w = S.PartitionWriter(lease_id=6)
    w.queue_op(S.OP_CREATION, QUEUE)
    record = _messages_then(w, keys + keys[-1:], 1, [], np.random.default_rng(0))
    run, d = _finish(w, planned, slots)
    return Crafted(run, d, slots, home, keys, dict(record=record, next_seq=w.seq + 1, lease_id=6))


def _rollover(keys, kept, confirms, seed):
    """rollover_records: a CREATION (kept), the MESSAGE records of `keys` kept
    where `kept` says, then CONFIRM records of `confirms`, shuffled.  The table
    holds the kept MESSAGE records of a run of every record."""
    planned = 1 + len(keys) + len(confirms)
    w = S.PartitionWriter(lease_id=9)
    w.queue_op(S.OP_CREATION, QUEUE)
    rest = [lambda w, k=k: w.confirm(*split(k)) for k in confirms]
    _messages_then(w, keys, 1, rest, np.random.default_rng(seed))
    run, d = _finish(w, planned, join_slots(planned))
    keep = np.zeros(planned, np.uint8)
    keep[0] = 1
    keep[1:1 + len(keys)] = kept
    keep[1 + len(keys):] = np.arange(len(confirms)) & 1      # ignored in FOLLOW mode
    return run, d, keep


def survivors(run, keep):
    """Per CONFIRM record of the run: does a kept MESSAGE record have its key?
    From the bytes alone, with a set."""
    recs = np.asarray(run).reshape(-1, 60)
    types = recs[:, 0] >> 4
    have = {recs[r, 36:52].tobytes() + recs[r, 22:27].tobytes()
            for r in np.flatnonzero((types == 1) & (keep != 0))}
    return [recs[r, 32:48].tobytes() + recs[r, 22:27].tobytes() in have
            for r in np.flatnonzero(types == 2)]


@functools.lru_cache(maxsize=None)
def rollover_chain(only=None):
    """CHAIN MESSAGE records with home slots - 8, every second one kept (or
    with `only` that message alone), and a CONFIRM record for each."""
    planned = 1 + 2 * CHAIN
    slots = join_slots(planned)
    home = slots - 8
    keys = colliders("join", slots, home, CHAIN, 41, True)
    kept = np.arange(CHAIN) % 2 == 0 if only is None else np.arange(CHAIN) == only
    run, d, keep = _rollover(keys, kept, keys, 42)
    in_table = tuple(k for k, yes in zip(keys, kept) if yes)
    return Crafted(run, d, slots, home, in_table, dict(keep=keep, n_kept_messages=int(kept.sum())))


@functools.lru_cache(maxsize=None)
def rollover_long():
    planned = 1 + 2 * LONG
    slots = join_slots(planned)
    home = slots - 300
    keys = colliders("join", slots, home, LONG, 43)
    run, d, keep = _rollover(keys, np.ones(LONG, bool), keys, 44)
    return Crafted(run, d, slots, home, keys, dict(keep=keep, n_kept_messages=LONG))


@functools.lru_cache(maxsize=None)
def rollover_pairs(swapped):
    """Of each near pair the first in the run is kept; a CONFIRM for both."""
    planned = 1 + 4 * PAIRS
    slots = join_slots(planned)
    home, pairs = _pairs(slots, swapped, 45)
    keys = [k for p in pairs for k in p]
    run, d, keep = _rollover(keys, np.arange(2 * PAIRS) % 2 == 0, keys, 46)
    return Crafted(run, d, slots, home, tuple(a for a, _ in pairs),
                   dict(keep=keep, pairs=pairs, n_kept_messages=PAIRS))


@functools.lru_cache(maxsize=None)
def rollover_duplicate():
    """BEHIND MESSAGE records in one chain and a second MESSAGE record of the
    last key, all kept, with a CONFIRM record of that key."""
    planned = 3 + BEHIND
    slots = join_slots(planned)
    home = slots - 8
    keys = colliders("join", slots, home, BEHIND, 47)
    run, d, keep = _rollover(keys + keys[-1:], np.ones(BEHIND + 1, bool), keys[-1:], 48)
    return Crafted(run, d, slots, home, keys, dict(keep=keep, n_kept_messages=BEHIND + 1))


# ---- journal_select ----------------------------------------------------------------

QUEUES = 300
WITHHELD = 151
APP = b"\x77\x66\x55\x44\x33"


@functools.lru_cache(maxsize=None)
def select_queues(queue_deletions):
    """journal_select: QUEUES distinct queue keys (every byte 0x80 or more)
    with home slots - 4 of the queue table a queue_cap of QUEUES gives.  Per
    queue a CREATION and messages; whole-queue and per-app PURGEs, an ADDITION,
    messages deleted by DELETION records and, with `queue_deletions`, queue
    DELETIONs followed by a re-CREATION (with CSL the reference fails a journal
    that has them: a known queue's DELETION, an unknown queue's CREATION).
    Returns (journal file, DATA file, keys, slots, home)."""
    slots = queue_slots(QUEUES, 3 * QUEUES)
    home = slots - 4
    keys = colliders("queue", slots, home, QUEUES, 51, True)
    w = S.PartitionWriter(lease_id=2)
    ops = []
    for i, q in enumerate(keys):
        ops.append([lambda w, q=q: w.queue_op(S.OP_CREATION, q)])
        mine = ops[-1]
        mine.append(lambda w, q=q, i=i: w.message(b"first of %d" % i, q))
        if i == 1:
            mine.append(lambda w, q=q: w.queue_op(S.OP_ADDITION, q, APP))
        if i % 7 == 3:
            mine.append(lambda w, q=q: w.queue_op(S.OP_PURGE, q))
        if i % 7 == 5:
            mine.append(lambda w, q=q: w.queue_op(S.OP_PURGE, q, APP))
        if i % 10 == 0 and queue_deletions:
            mine.append(lambda w, q=q: w.queue_op(S.OP_DELETION, q))
            mine.append(lambda w, q=q: w.queue_op(S.OP_CREATION, q))
        if i % 4 == 1:
            def gone(w, q=q):
                w.deletion(w.message(b"consumed", q)[1], q)
            mine.append(gone)
        if i % 3 == 0:
            mine.append(lambda w, q=q, i=i: w.message(b"last of %d" % i, q))
    # the queues' records interleaved: each queue's own stay in their order
    rng = np.random.default_rng(52)
    turn = np.repeat(np.arange(QUEUES), [len(o) for o in ops])
    rng.shuffle(turn)
    for i in turn:
        ops[i].pop(0)(w)
    j, d = w.files()
    assert queue_slots(QUEUES, len(w.recs)) == slots
    return j, d, keys, slots, home


GUID_CHAIN = 300
GUID_ABSENT = 30
Q1 = b"\x01\x02\x03\x04\x05"


@functools.lru_cache(maxsize=None)
def select_guid_chain():
    """journal_select: GUID_CHAIN MESSAGE records and GUID_CHAIN DELETION
    records whose GUIDs all have home slots - 4 of the GUID table, which then
    holds one chain of GUID_CHAIN DELETIONs across its end.  Inside: two
    DELETIONs of one GUID above two MESSAGEs of it (the higher message is
    skipped, the lower stays), a DELETION below its MESSAGE, a DELETION of a
    GUID no message has, one GUID under two MESSAGE records and one DELETION,
    and GUID_ABSENT undeleted messages whose GUIDs home at the chain's start and
    mid-chain.  Returns (journal file, DATA file, slots, home, the GUIDs of the
    DELETION records, the absent GUIDs, expected counts)."""
    planned = 1 + 2 * GUID_CHAIN + GUID_ABSENT
    slots = join_slots(planned)
    home = slots - 4
    plain = GUID_CHAIN - 5
    g = colliders("guid", slots, home, plain + 4 + GUID_ABSENT // 2, 53)
    twice, twins, below, orphan = g[plain:plain + 4]
    absent = g[plain + 4:] + colliders("guid", slots, GUID_CHAIN // 2,
                                       GUID_ABSENT - GUID_ABSENT // 2, 54)
    rng = np.random.default_rng(55)
    w = S.PartitionWriter(lease_id=2)
    w.queue_op(S.OP_CREATION, Q1)
    w.deletion(below, Q1)
    msgs = list(g[:plain]) + [twice, twice, twins, twins, below] + list(absent)
    for i in rng.permutation(len(msgs)):
        w.message(b"m%d" % i, Q1, guid=msgs[i])
    dels = list(g[:plain]) + [twice, twice, twins, orphan]
    for i in rng.permutation(len(dels)):
        w.deletion(dels[i], Q1)
    j, d = w.files()
    assert len(w.recs) == planned
    in_table = tuple(g[:plain]) + (twice, twice, twins, below, orphan)
    want = dict(n_deleted=plain + 2, n_selected=GUID_ABSENT + 3, n_purged=0)
    return j, d, slots, home, in_table, tuple(absent), want
