"""The source ranges the large cases of test_gpu_put_pack.py and
test_gpu_records_pack.py pack (shared with the CPU tests of both models, which
assert what the cases rely on; not a test module).

A pool of POOL distinct (offset, length) pairs inside the first SRC_BYTES of a
source; message i takes pair (i * STEP + 5) % POOL, so any POOL messages in a
row take every pair once and a CRC is computed once per pair.  POOL is prime
(no multiple of the 1,024-message tile: no two tiles see the same lengths in
the same lanes).  Seen in the order the messages visit them the lengths are
0..40 over and over -- every padding count of both framings, 4 - len % 4 and
8 - (12 + len) % 8, and the empty message -- but for a handful between 200 and
700 and one of LONG bytes, longer than a 64 KiB chunk of the copy pass.  The
offsets take all 16 misalignments.  The source is MARGIN bytes longer than the
SRC_BYTES a refusal case declares, so that a broken range check still reads
inside the allocation."""
import functools

import numpy as np

import test_grid_regimes as G

POOL, STEP = 3001, 7919
SRC_BYTES, MARGIN = 1 << 20, 1 << 17
LONG, LONG_VISIT = 70000, 1500          # message 1,500 is the first of LONG bytes
MIDDLE = {97: 200, 611: 333, 1203: 512, 1777: 641, 2410: 700, 2903: 257}  # visit -> length


def index(n):
    """The pool pair of each of n messages."""
    return (np.arange(n, dtype=np.int64) * STEP + 5) % POOL


@functools.lru_cache(maxsize=None)
def pool():
    """(src, pool offsets, pool lengths), read-only."""
    assert all(POOL % p for p in range(2, int(POOL ** 0.5) + 1)) and POOL % 1024 and STEP % POOL
    rng = np.random.default_rng(20)
    src = rng.integers(0, 256, size=SRC_BYTES + MARGIN, dtype=np.uint8)
    visit = np.arange(POOL) % 41
    for k, ln in MIDDLE.items():
        visit[k] = ln
    visit[LONG_VISIT] = LONG
    plen = np.zeros(POOL, np.int64)
    plen[index(POOL)] = visit
    poff = rng.integers(0, (SRC_BYTES - plen) // 16, size=POOL) * 16 + np.arange(POOL) % 16
    assert np.all(poff + plen <= SRC_BYTES) and len(set(zip(poff.tolist(), plen.tolist()))) == POOL
    for a in (src, poff, plen):
        a.setflags(write=False)
    return src, poff, plen


def messages(n):
    """(src, src offsets, lengths, pool index) of the first n messages."""
    src, poff, plen = pool()
    ix = index(n)
    return src, poff[ix], plen[ix], ix


def check_properties(pad_of):
    """What the large cases rely on, for the framing whose padding pad_of gives."""
    src, soff, lens, ix = messages(G.N_FRAME)
    _, poff, plen = pool()
    assert set(poff % 16) == set(range(16)) and set(soff[:1024] % 16) == set(range(16))
    assert set(range(41)) <= set(plen) and sum(200 <= x <= 700 for x in plen) == len(MIDDLE)
    assert int(plen.max()) == LONG > 65536 and int((plen == LONG).sum()) == 1
    # every block that owns a whole tile: every pad count and an empty message
    pads = set(pad_of(np.arange(41)).tolist())
    for n in (G.N_WAVES, G.N_FULL, G.N_TILES, G.N_FRAME):
        per_block = G.regime(n).per_block
        for lo in range(0, n, per_block):
            for t in range(lo, min(lo + per_block, n) - 1023, 1024):  # its whole tiles
                tile = lens[t:t + 1024]
                assert set(pad_of(tile).tolist()) == pads and (tile == 0).any(), (n, t)
    # the long message: in the second tile of block 0 at N_TILES, and again in
    # the second tile of a block behind the 64th
    at = np.flatnonzero(lens[:G.N_TILES] == LONG)
    per_block = G.regime(G.N_TILES).per_block
    assert per_block == 2048 and int(at[0]) == LONG_VISIT and LONG_VISIT % per_block >= 1024
    assert np.array_equal(at, LONG_VISIT + POOL * np.arange(at.size))
    assert any(i // per_block > 64 and i % per_block >= 1024 for i in at.tolist())
