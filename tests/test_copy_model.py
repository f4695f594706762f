"""CPU model of the fused copy + CRC kernels (crc32c_copy.hip, DESIGN.md
section 11), checked against the oracle: pieces cut on the destination's
16-byte boundaries, the piece space and its 4,096-piece chunks, lanes dealt to
messages by the prefix of piece counts, per-lane Horner over 1 KiB rows through
the generated XROW tables, the move by x^(8 * bytes after) (XBYTES, XNEG8 for a
last piece cut by the message end), the XOR combine over lanes and chunks, the
seed's share, and the bounds refusals.  The model walks rows and lanes the way
the kernel does and writes the destination image too, so it pins the
arithmetic, the new table and the byte-exact copy without a GPU."""
import os
import re

import numpy as np
import pytest

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK_PIECES = 4096   # kCopyChunkPieces
CHUNK_BYTES = 16 * CHUNK_PIECES
NONE = 0xFFFFFFFF
POLY_R = 0x82F63B78


def _header_table(name):
    """A brace-initialised table from the generated crc32c_consts.h."""
    text = open(os.path.join(ROOT, "blazingmq_amd", "csrc", "crc32c_consts.h")).read()
    body = text[text.index("#define %s " % name):]
    body = body[:body.index("}\n") + 1]
    return [int(v, 16) for v in re.findall(r"0x([0-9a-f]{8})u", body)]


def _rows(flat, n):
    assert len(flat) >= 256 * n
    return [flat[256 * k:256 * (k + 1)] for k in range(n)]


XROW = _rows(_header_table("BMQCRC_XROW"), 4)
TY = _rows(_header_table("BMQCRC_TY"), 4)
XB = _rows(_header_table("BMQCRC_XBYTES"), 4)
XNEG = _header_table("BMQCRC_XNEG8")


def gmul(a, b):
    """a * b mod P, reflected (the kernel's gmul)."""
    p, m = 0, 1 << 31
    while m:
        if a & m:
            p ^= b
        b = (b >> 1) ^ (POLY_R if b & 1 else 0)
        m >>= 1
    return p


def mul_tab(tab, v):
    return (tab[0][v & 0xff] ^ tab[1][(v >> 8) & 0xff] ^ tab[2][(v >> 16) & 0xff] ^
            tab[3][v >> 24])


def xbytes_factor(f, dist):
    for i in range(1, 4):
        b = (dist >> (8 * i)) & 0xff
        if b:
            f = gmul(f, XB[i][b])
    return f


class Model:
    """k_copy_count + k_copy_scan + k_copy_fold over numpy buffers.
    `dst_base` is the destination allocation's address modulo 16."""

    def __init__(self, src, src_bytes, soff, lens, dst, dst_bytes, doff, seeds, dst_base=0,
                 nwaves=7):
        self.src, self.dst = src, dst
        self.soff, self.doff, self.lens = soff, doff, lens
        self.dst_base = dst_base
        n = len(lens)
        self.n = n
        self.out = [None] * n
        self.refused = []
        self.atomics = [0] * n
        self.windows_skipped = 0
        pieces = []
        for i in range(n):
            ok = (soff[i] <= src_bytes and lens[i] <= src_bytes - soff[i] and
                  doff[i] <= dst_bytes and lens[i] <= dst_bytes - doff[i])
            if not ok:
                self.refused.append(i)
            al = (dst_base + doff[i]) & 15
            pieces.append((al + lens[i] + 15) >> 4 if ok and lens[i] else 0)
            if ok:
                seed = seeds[i] if seeds is not None else 0
                f = xbytes_factor(XB[0][lens[i] & 0xff], lens[i])
                self.out[i] = gmul(~seed & 0xFFFFFFFF, f) ^ 0xFFFFFFFF
        self.first = [0]
        for p in pieces:
            self.first.append(self.first[-1] + p)
        assert self.first[-1] < 1 << 32
        total = self.first[-1]
        ntiles = (total + CHUNK_PIECES - 1) // CHUNK_PIECES
        # chunks in the order a grid of `nwaves` waves takes them (any order
        # gives the same result: the combine is an XOR)
        for w in range(nwaves):
            for t in range(w, ntiles, nwaves):
                self.chunk(t * CHUNK_PIECES, min(total, (t + 1) * CHUNK_PIECES))

    def find(self, g):
        """copy_find: last i with first[i] <= g, 64 probes per step."""
        lo, hi = 0, self.n
        while hi - lo > 1:
            step = (hi - lo + 63) >> 6
            cnt = 0
            for lane in range(64):
                idx = lo + (lane + 1) * step
                if idx < hi and self.first[idx] <= g:
                    cnt += 1
            nlo = lo + cnt * step
            hi, lo = min(hi, nlo + step), nlo
        return lo

    def deal(self, cur_m, gr):
        """The marks of a row that holds more than one message, then the
        inclusive max-scan: message of each lane."""
        mark = [0] * 64
        wb = cur_m + 1
        while True:
            last_in_row = False
            for lane in range(64):
                idx = wb + lane
                if idx < self.n:
                    st, en = self.first[idx], self.first[idx + 1]
                    in_row = 0 <= st - gr < 64
                    if in_row and en > st:
                        mark[st - gr] = idx - cur_m
                    if lane == 63:
                        last_in_row = in_row
            if not last_in_row:
                break
            # a window of empty messages only: one search skips the whole run
            if all(wb + l < self.n and self.first[wb + l + 1] == self.first[wb + l]
                   for l in range(64)):
                j = self.find(self.first[wb + 63])
                assert j > wb + 63 or j == self.n - 1
                self.windows_skipped += j - (wb + 64)
                wb = j - 64
            wb += 64
        return [cur_m + int(v) for v in np.maximum.accumulate(mark)]

    # True: the doubling steps compare message keys instead of run heads --
    # the rule that loses lanes when one message is held by two separate runs
    # (test_two_runs_of_one_message shows the cases here tell the two apart)
    segment_by_key = False

    def flush(self, lanes, pred):
        """The kernel's flush, lane for lane: every lane's value moved to its
        message end, the head lane of each run of adjacent equal keys found,
        six doubling steps that XOR in the lane d above when it belongs to
        the same run, one atomic XOR per head."""
        key, val = [NONE] * 64, [0] * 64
        for l in pred:
            s = lanes[l]
            v = s["a"][0]
            for k in (1, 2, 3):
                v = mul_tab(TY, v) ^ s["a"][k]
            v = mul_tab(TY, v)
            after = s["after"]
            assert -15 <= after < 1 << 32
            if after < 0:
                f = XNEG[-after]
            else:
                f = xbytes_factor(XB[0][after & 0xff], after)
            key[l], val[l] = s["held"], gmul(v, f)
        head = [l == 0 or key[l - 1] != key[l] for l in range(64)]
        run = [int(v) for v in np.maximum.accumulate([l if head[l] else 0 for l in range(64)])]
        seg = key if self.segment_by_key else run
        d = 1
        while d < 64:
            val = [val[l] ^ (val[l + d] if l + d < 64 and seg[l + d] == seg[l] else 0)
                   for l in range(64)]
            d <<= 1
        for l in range(64):
            if key[l] != NONE and head[l]:
                self.out[key[l]] ^= val[l]
                self.atomics[key[l]] += 1
        for l in pred:
            lanes[l].update(held=NONE, a=[0, 0, 0, 0])

    def chunk(self, g0, g1):
        lanes = [dict(held=NONE, a=[0, 0, 0, 0], after=0) for _ in range(64)]
        cur_m = self.find(g0)
        gr = g0
        while gr < g1:
            cur_first, cur_end = self.first[cur_m], self.first[cur_m + 1]
            row_end = min(gr + 64, g1)
            msgs = [cur_m] * 64
            next_m = cur_m
            if row_end > cur_end:
                msgs = self.deal(cur_m, gr)
                next_m = msgs[row_end - gr - 1]
            valid = [gr + l < g1 for l in range(64)]
            change = [l for l in range(64)
                      if valid[l] and lanes[l]["held"] not in (NONE, msgs[l])]
            if change:
                self.flush(lanes, change)
            rows = 1
            if row_end <= cur_end:
                al = (self.dst_base + self.doff[cur_m]) & 15
                full_lo = cur_first + (1 if al else 0)
                full_hi = min(cur_first + ((al + self.lens[cur_m]) >> 4), g1)
                if gr >= full_lo and gr + 256 <= full_hi:
                    rows = 4 * ((full_hi - gr) // 256)  # the four-row loop, all whole pieces
            for r in range(rows):
                for l in range(64):
                    g = gr + 64 * r + l
                    if g >= g1:
                        continue
                    m = msgs[l]
                    ln, so, do = self.lens[m], self.soff[m], self.doff[m]
                    al = (self.dst_base + do) & 15
                    rel0 = 16 * (g - self.first[m]) - al
                    lo, hi = max(rel0, 0), min(rel0 + 16, ln)
                    assert lo < hi
                    if rows > 1:
                        assert (lo, hi) == (rel0, rel0 + 16)
                    piece = bytearray(16)
                    piece[lo - rel0:hi - rel0] = self.src[so + lo:so + hi].tobytes()
                    self.dst[do + lo:do + hi] = self.src[so + lo:so + hi]
                    w = np.frombuffer(bytes(piece), dtype="<u4")
                    s = lanes[l]
                    s["a"] = [mul_tab(XROW, s["a"][k]) ^ int(w[k]) for k in range(4)]
                    s["held"] = m
                    s["after"] = ln - (rel0 + 16)
            gr = gr + 64 * rows if rows > 1 else row_end
            cur_m = next_m
        self.flush(lanes, [l for l in range(64) if lanes[l]["held"] != NONE])


def run(src, soff, lens, doff, seeds, dst_size, dst_base=0, src_bytes=None, dst_bytes=None):
    dst = np.full(dst_size, 0xA5, np.uint8)
    m = Model(src, src.size if src_bytes is None else src_bytes, soff, lens, dst,
              dst_size if dst_bytes is None else dst_bytes, doff, seeds, dst_base)
    image = np.full(dst_size, 0xA5, np.uint8)
    want = []
    for i, (so, ln, do) in enumerate(zip(soff, lens, doff)):
        if i in m.refused:
            want.append(None)
            continue
        image[do:do + ln] = src[so:so + ln]
        want.append(oracle.crc32c(src[so:so + ln].tobytes(), seeds[i] if seeds is not None else 0))
    return m, dst, image, want


def test_new_table_is_the_row_step():
    # XROW[k][b] = (b << 8k) * x^(8 * 1024): a CRC carried past 1,024 zero bytes
    assert len(_header_table("BMQCRC_XROW")) == 1024
    rng = np.random.default_rng(1)
    for _ in range(20):
        a = rng.integers(0, 256, size=int(rng.integers(1, 40)), dtype=np.uint8).tobytes()
        raw = oracle.crc32c(a, 0xFFFFFFFF) ^ 0xFFFFFFFF  # zero initial value, no final xor
        assert mul_tab(XROW, raw) == oracle.crc32c(a + bytes(1024), 0xFFFFFFFF) ^ 0xFFFFFFFF


def test_every_length_at_every_misalignment():
    """Lengths 0..2,200 with random seeds; source and destination misalignment
    as random pairs that cover each value of both."""
    rng = np.random.default_rng(2)
    lens = list(range(2201))
    rng.shuffle(lens)
    smis = [i % 16 for i in range(len(lens))]
    dmis = [int(v) for v in rng.permutation(len(lens)) % 16]
    assert set(smis) == set(dmis) == set(range(16))
    soff, doff, s, d = [], [], 0, 0
    for ln, sm, dm in zip(lens, smis, dmis):
        s = (s + 15) // 16 * 16 + sm
        d = (d + 15) // 16 * 16 + dm
        soff.append(s)
        doff.append(d)
        s += ln
        d += ln + int(rng.integers(0, 3))
    src = rng.integers(0, 256, size=s + 16, dtype=np.uint8)
    seeds = [int(v) for v in rng.integers(0, 1 << 32, size=len(lens), dtype=np.uint64)]
    m, dst, image, want = run(src, soff, lens, doff, seeds, d + 16)
    assert m.out == want
    assert np.array_equal(dst, image)


@pytest.mark.parametrize("ln", [1, 15, 16, 17, 33, 1024, 1039])
def test_all_256_misalignment_pairs(ln):
    rng = np.random.default_rng(ln)
    pitch = 16 * (ln // 16 + 3)
    src = rng.integers(0, 256, size=256 * pitch, dtype=np.uint8)
    soff = [pitch * k + k % 16 for k in range(256)]
    doff = [pitch * k + k // 16 for k in range(256)]
    m, dst, image, want = run(src, soff, [ln] * 256, doff, None, 256 * pitch)
    assert m.out == want and np.array_equal(dst, image)


@pytest.mark.parametrize("base", [0, 5])
def test_one_message_over_three_chunks(base):
    """2 C + 17 bytes span three chunks: the four-row loop, rows cut by the
    chunk ends, and three partial results XORed into out[i]; neighbours at
    both ends share its first and last 16-byte piece."""
    rng = np.random.default_rng(3)
    lens = [40, 2 * CHUNK_BYTES + 17, 40, 0, 9]
    src = rng.integers(0, 256, size=sum(lens) + 64, dtype=np.uint8)
    soff = [7, 60, 11, 0, 3]
    doff, d = [], 3
    for ln in lens:  # packed end to end
        doff.append(d)
        d += ln
    seeds = [1, 0xDEADBEEF, 0, 77, 0xFFFFFFFF]
    m, dst, image, want = run(src, soff, lens, doff, seeds, d + 32, dst_base=base)
    assert m.out == want and np.array_equal(dst, image)
    assert m.atomics[1] >= 3


@pytest.mark.parametrize("ln", [CHUNK_BYTES - 1, CHUNK_BYTES, CHUNK_BYTES + 1])
def test_lengths_around_the_chunk(ln):
    rng = np.random.default_rng(ln)
    src = rng.integers(0, 256, size=ln + 32, dtype=np.uint8)
    for so, do in ((0, 0), (5, 0), (0, 9), (13, 2)):
        m, dst, image, want = run(src, [so], [ln], [do], [12345], ln + 32)
        assert m.out == want and np.array_equal(dst, image)


def test_packed_small_messages_and_empties():
    """Rows shared by many messages, runs of empty messages longer than the
    64-entry window, a message per piece."""
    rng = np.random.default_rng(4)
    lens = [int(v) for v in rng.integers(1, 300, size=400)]
    lens[50:200:3] = [0] * len(lens[50:200:3])
    lens[210:300] = [0] * 90
    lens[300:380] = [int(v) for v in rng.integers(1, 17, size=80)]
    n = len(lens)
    src = rng.integers(0, 256, size=8192, dtype=np.uint8)
    soff = [int(rng.integers(0, src.size - ln)) for ln in lens]
    doff = [0] * n
    d = 5
    for i in range(n):
        doff[i] = d
        d += lens[i]
    seeds = [int(v) for v in rng.integers(0, 1 << 32, size=n, dtype=np.uint64)]
    m, dst, image, want = run(src, soff, lens, doff, seeds, d + 16)
    assert m.out == want and np.array_equal(dst, image)
    assert [m.out[i] for i in range(210, 300)] == seeds[210:300]  # empty: out = seed


def test_refused_messages_own_no_piece():
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, size=4096, dtype=np.uint8)
    lens = [100, 200, 300, 64, 50, 0]
    soff = [0, 3900, 100, 3937, 500, 4001]   # 1: src end 4100 > 4000; 3: 4001 > 4000; 5: offset > size
    doff = [0, 200, 1800, 500, 1990, 0]      # 2: dst end 2100 > 2000; 4: 2040 > 2000
    m, dst, image, want = run(src, soff, lens, doff, None, 4096, src_bytes=4000, dst_bytes=2000)
    assert m.refused == [1, 2, 3, 4, 5]
    assert m.out == want and m.out[1] is None
    assert np.array_equal(dst, image)


def _packed(lens, seed, dmis=0):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, size=sum(lens) + 64, dtype=np.uint8)
    soff, doff, so, do = [], [], 5, dmis
    for ln in lens:
        soff.append(so)
        doff.append(do)
        so += ln
        do += ln
    seeds = [int(v) for v in rng.integers(0, 1 << 32, size=len(lens), dtype=np.uint64)]
    return src, soff, doff, seeds, do + 32


# a long message followed by a few short ones at the very end of the batch: the
# last row is partial, the lanes past it still hold the row before, and the
# long message is held by two separate runs of lanes at the final flush
TWO_RUN_CASES = [([5000, 20], 0), ([CHUNK_BYTES + 700, 40, 9], 0), ([3000, 1, 1], 3),
                 ([40, 2100, 500, 30], 7), ([5000], 0), ([CHUNK_BYTES + 1200, 0, 17], 11)]


@pytest.mark.parametrize("lens,dmis", TWO_RUN_CASES)
def test_two_runs_of_one_message(lens, dmis):
    src, soff, doff, seeds, size = _packed(lens, 21, dmis)
    m, dst, image, want = run(src, soff, lens, doff, seeds, size)
    assert m.out == want and np.array_equal(dst, image)


def test_two_run_cases_tell_the_segment_rules_apart(monkeypatch):
    # reducing over "lanes with the same message" instead of "adjacent lanes
    # with the same message" gets [5000, 20] wrong: the case discriminates
    monkeypatch.setattr(Model, "segment_by_key", True)
    src, soff, doff, seeds, size = _packed([5000, 20], 21)
    m, _, _, want = run(src, soff, [5000, 20], doff, seeds, size)
    assert m.out[0] != want[0] and m.out[1] == want[1]


def test_random_short_batches_ending_anywhere():
    # 1-5 packed messages below 3,000 bytes: every way a batch can end in a
    # partial row after a message of several rows
    rng = np.random.default_rng(22)
    for trial in range(120):
        lens = [int(v) for v in rng.integers(0, 3000, size=int(rng.integers(1, 6)))]
        src, soff, doff, seeds, size = _packed(lens, 100 + trial, int(rng.integers(0, 16)))
        m, dst, image, want = run(src, soff, lens, doff, seeds, size)
        assert m.out == want and np.array_equal(dst, image), lens


def test_long_runs_of_empty_messages_are_searched_not_walked():
    rng = np.random.default_rng(23)
    lens = [100] + [0] * 5000 + [33, 700] + [0] * 777 + [5] + [0] * 300
    src = rng.integers(0, 256, size=4096, dtype=np.uint8)
    soff = [int(rng.integers(0, 3000)) for _ in lens]
    doff, d = [], 9
    for ln in lens:
        doff.append(d)
        d += ln
    seeds = [int(v) for v in rng.integers(0, 1 << 32, size=len(lens), dtype=np.uint64)]
    m, dst, image, want = run(src, soff, lens, doff, seeds, d + 16)
    assert m.out == want and np.array_equal(dst, image)
    assert m.windows_skipped > 5000
