"""The journal and DATA file the large cases of test_gpu_storage_pack.py and
test_gpu_push_pack.py pack (shared with the CPU tests of both models, which
assert what the cases rely on; not a test module).

One run of N_FRAME records, written once per process with PartitionWriter, and
its whole DATA file; a smaller size is a prefix of the run (with the whole DATA
file: a shorter run leaves its end unread).  A queue's CREATION, then messages
of 0..40 bytes behind DataHeaders of 3 and 5 words with 0..2 option words --
so the bytes between a DATA record's start and its application data take all
of 12, 16, 20, 24 and 28 -- with random DataHeader flags (MESSAGE_PROPERTIES),
schema ids and CAT bytes; a CONFIRM behind every seventh message, a DELETION
behind every 21st, and in front of every 16th a queue ADDITION, PURGE, DELETION
or CREATION or a sync point, in turn.  Two messages are longer than a 64 KiB
chunk of the copy pass: LONG[0] bytes in the second tile of block 0 at N_TILES,
the longest of all, and LONG[1] bytes in the second tile of a block behind the
64th.  The last record of the run is a MESSAGE record.

`msgs` are the MESSAGE records' indices.  PUSH message m names record
msgs[(m * STEP + 5) % len(msgs)]: neighbours in a wave name records far apart,
and past len(msgs) messages the records repeat."""
import collections
import functools

import numpy as np

from blazingmq_amd import storage as S
import test_grid_regimes as G

JH = S.PartitionWriter.JOURNAL_HEADER
QK = S.DEFAULT_QUEUE_KEY
STEP = 7919
LONG = (90000, 70000)
# (the first MESSAGE record at or behind each gets the long message)
LONG_AT = (1024 + 500, 70 * 2048 + 1024 + 300)
SPECIALS = (S.OP_ADDITION, S.OP_PURGE, S.OP_DELETION, None, S.OP_CREATION)   # None: a sync point

Pool = collections.namedtuple("Pool", "run data msgs crcs long")


def be32(rows):
    """The big-endian 32-bit values of (k, 4) uint8 rows, as int64."""
    return np.ascontiguousarray(rows, np.uint8).view(">u4")[:, 0].astype(np.int64)


@functools.lru_cache(maxsize=None)
def pool():
    """Pool(record run, DATA file, indices of the MESSAGE records, the CRC32C of
    every MESSAGE record's application data by record (0 elsewhere), the long
    messages' records).  Shared and read-only."""
    n = G.N_FRAME
    rng = np.random.default_rng(1816)
    blob = rng.integers(0, 256, size=1 << 20, dtype=np.uint8).tobytes()
    sizes = rng.integers(0, 41, size=n)
    words = rng.integers(0, 6, size=n)         # DataHeader words 3 or 5, 0..2 option words
    at = rng.integers(0, len(blob) - max(LONG), size=n)
    w = S.PartitionWriter(lease_id=4, partition_id=1)
    w.queue_op(S.OP_CREATION, QK)
    k = specials = 0
    long_at, long_recs = list(LONG_AT), []
    while len(w.recs) < n:
        if k % 16 == 15 and specials == k // 16 and len(w.recs) < n - 1:
            op = SPECIALS[specials % len(SPECIALS)]
            if op is None:
                w.sync_point()
            else:
                w.queue_op(op, QK, b"\1\2\3\4\5")
            specials += 1
            continue
        size = int(sizes[k])
        if long_at and len(w.recs) >= long_at[0]:
            size = LONG[len(long_recs)]
            long_recs.append(len(w.recs))
            del long_at[0]
        o = int(at[k])
        app = blob[o:o + size]
        before = w.dpos
        _, guid = w.message(app, QK)
        hw, opt = (3, 5)[int(words[k]) & 1], int(words[k]) >> 1
        lead = 4 * (hw + opt)
        total = (lead + size) // 8 * 8 + 8
        pad = total - lead - size
        o = (o * 31 + 7) % (len(blob) - 64)
        w.data[-1] = (((hw << 29) | (total // 4)).to_bytes(4, "big") +
                      ((opt << 8) | blob[o]).to_bytes(4, "big") + blob[o + 1:o + 1 + lead - 8] +
                      app + bytes([pad]) * pad)
        w.dpos = before + total
        if k % 7 == 0 and len(w.recs) < n - 1:
            w.confirm(guid, QK)
        if k % 21 == 0 and len(w.recs) < n - 1:
            w.deletion(guid, QK)
        k += 1
    j, d = w.files()
    run = j[JH:]
    recs = run.reshape(n, 60)
    msgs = np.flatnonzero(recs[:, 0] >> 4 == S.REC_MESSAGE)
    recs[msgs, 21] = rng.integers(0, 256, size=msgs.size)      # CAT in the low 3 bits
    crcs = np.zeros(n, np.uint32)
    crcs[msgs] = be32(recs[msgs, 52:56])     # PartitionWriter's: Crc32c.calculate of the data
    for a in (run, d, msgs, crcs):
        a.setflags(write=False)
    return Pool(run, d, msgs, crcs, tuple(long_recs))


def records(n):
    """(the first n records of the run, the whole DATA file)."""
    p = pool()
    return p.run[:60 * n], p.data


def push_records(n):
    """The record of each of n PUSH messages."""
    msgs = pool().msgs
    return msgs[(np.arange(n, dtype=np.int64) * STEP + 5) % msgs.size]


@functools.lru_cache(maxsize=None)
def message_journal():
    """The first N_TILES MESSAGE records as a journal of their own, for the
    identity path (records == NULL)."""
    p = pool()
    run = p.run.reshape(-1, 60)[p.msgs[:G.N_TILES]].reshape(-1)
    run.setflags(write=False)
    return run


def data_fields(run, data, index):
    """(window offset, header + option bytes, record bytes, application bytes,
    DataHeader flags byte) of the DATA records of the MESSAGE records `index`."""
    recs = np.asarray(run).reshape(-1, 60)
    at = 8 * be32(recs[index, 32:36])
    h0 = be32(data[at[:, None] + np.arange(4)])
    h1 = be32(data[at[:, None] + 4 + np.arange(4)])
    rec = (h0 & 0x1FFFFFFF) * 4
    lead = (h0 >> 29) * 4 + (h1 >> 8) * 4
    return at, lead, rec, rec - lead - data[at + rec - 1], h1 & 0xFF


def check_properties():
    """What the large cases rely on."""
    p = pool()
    recs = p.run.reshape(-1, 60)
    types = recs[:, 0] >> 4
    ops = be32(recs[:, 32:36])
    assert recs.shape[0] == G.N_FRAME and types[-1] == S.REC_MESSAGE
    assert np.array_equal(p.msgs, np.flatnonzero(types == 1))
    at, lead, rec, length, flags = data_fields(p.run, p.data, p.msgs)
    by_record = {name: np.zeros(G.N_FRAME, np.int64) for name in ("lead", "pad", "length")}
    by_record["lead"][p.msgs] = lead
    by_record["pad"][p.msgs] = rec - lead - length
    by_record["length"][p.msgs] = length + 1        # (0: no MESSAGE record)
    assert int(at[0]) == 40 and np.array_equal(at[1:], (at + rec)[:-1])
    assert int(at[-1] + rec[-1]) == p.data.size
    for n in (G.N_WAVES, G.N_FULL, G.N_TILES, G.N_FRAME):
        per_block = G.regime(n).per_block
        for lo in range(0, n, per_block):
            mine = slice(lo, min(lo + per_block, n))
            if mine.stop - lo < 1024:
                continue
            # every record type, and of the QUEUE_OP records all four ops
            assert set(types[mine].tolist()) == {1, 2, 3, 4, 5}, (n, lo)
            assert set(ops[mine][types[mine] == 4].tolist()) == {1, 2, 3, 4}, (n, lo)
            for t in range(lo, mine.stop - 1023, 1024):       # its whole tiles
                tile = slice(t, t + 1024)
                assert set(by_record["lead"][tile].tolist()) == {0, 12, 16, 20, 24, 28}, (n, t)
                assert set(by_record["pad"][tile].tolist()) == set(range(9)), (n, t)
                assert (by_record["length"][tile] == 1).any(), (n, t)
    assert int((p.msgs < G.N_TILES).sum()) >= 100000
    # the long messages
    per_block = G.regime(G.N_TILES).per_block
    assert per_block == 2048 and len(p.long) == 2
    a, b = p.long
    assert a // per_block == 0 and a % per_block >= 1024
    assert b // per_block > 64 and b % per_block >= 1024 and b < G.N_TILES
    longest = np.sort(length)[-3:]
    assert [int(by_record["length"][i]) - 1 for i in p.long] == list(LONG)
    assert longest.tolist() == [40, LONG[1], LONG[0]] and LONG[1] > 65536
    # CAT bits and the MESSAGE_PROPERTIES flag vary from message to message
    cat = recs[p.msgs, 21] & 7
    assert set(cat[:1024].tolist()) == set(range(8)) and 100 < int((flags[:1024] & 1).sum()) < 900
    assert len(set(zip(cat[:256].tolist(), (flags[:256] & 1).tolist()))) == 16
    assert int((cat[1:64] != cat[:63]).sum()) > 32
    # the PUSH message list: every MESSAGE record once in any len(msgs) messages
    assert np.gcd(STEP, p.msgs.size) == 1 and p.msgs.size < G.N_FRAME
    named = push_records(G.N_FRAME)
    assert np.array_equal(np.sort(named[:p.msgs.size]), p.msgs)
    assert np.array_equal(named[p.msgs.size:], named[:G.N_FRAME - p.msgs.size])
    assert int(np.abs(np.diff(named[:64])).min()) > 4096
    # the all-MESSAGE journal
    assert p.msgs.size >= G.N_TILES and message_journal().size == 60 * G.N_TILES
    assert bool((message_journal().reshape(-1, 60)[:, 0] >> 4 == 1).all())
