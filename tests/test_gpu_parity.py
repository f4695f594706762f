"""GPU parity: the HIP batch path (through the C ABI) vs the CPU oracle.

Bit-exact comparisons.  Small cases compare every message against the oracle
and the reference's golden vectors; BASELINE-size cases compare sampled
messages plus size-independent properties.  Mirrors the reference's own test
plan (bmqp_crc32c.t.cpp test1-test8, fuzz s_bmqfuzz_bmqp_crc32c.fuzz.cpp).
"""
import os

import numpy as np
import pytest

import oracle
from blazingmq_amd import Crc32c

pytestmark = pytest.mark.gpu


def _dev_batch(cuda, arena_np, offs, lens, seeds=None, seg_bytes=0):
    import torch
    arena = torch.from_numpy(np.array(arena_np, dtype=np.uint8, copy=True)).to(cuda)
    o = torch.tensor(np.asarray(offs, dtype=np.int64), device=cuda)
    ln = torch.tensor(np.asarray(lens, dtype=np.uint32).view(np.int32), device=cuda)
    sd = None
    if seeds is not None:
        sd = torch.tensor(np.asarray(seeds, dtype=np.uint32).view(np.int32), device=cuda)
    out = Crc32c.calculate_batch(arena, o, ln, sd, seg_bytes=seg_bytes)
    return out.cpu().numpy().view(np.uint32)


def _pack(bufs, align=1, lead=0):
    offs, chunks, pos = [], [], lead
    chunks.append(b"\xAA" * lead)
    for b in bufs:
        pad = (-pos) % align
        chunks.append(b"\x55" * pad)
        pos += pad
        offs.append(pos)
        chunks.append(b)
        pos += len(b)
    chunks.append(b"\x33" * 256)
    return np.frombuffer(b"".join(chunks), dtype=np.uint8), offs, [len(b) for b in bufs]


def test_golden_calculate(cuda, golden):
    vecs = golden["calculate"] + golden["rfc3720"]
    bufs = [bytes.fromhex(v["hex"]) for v in vecs]
    arena, offs, lens = _pack(bufs)
    got = _dev_batch(cuda, arena, offs, lens)
    assert [int(x) for x in got] == [v["crc"] for v in vecs]


def test_golden_chained(cuda, golden):
    # test4: crc(suffix, seed=crc(prefix)); plus (buf,0,prev) and (0,0,prev) -> prev
    vecs = golden["chained"]
    bufs, seeds, expect = [], [], []
    for v in vecs:
        b = bytes.fromhex(v["hex"])
        p = v["prefix_len"]
        prefix_crc = oracle.crc32c(b[:p])
        bufs += [b[p:], b""]
        seeds += [prefix_crc, v["crc"]]
        expect += [v["crc"], v["crc"]]
    arena, offs, lens = _pack(bufs)
    got = _dev_batch(cuda, arena, offs, lens, seeds)
    assert [int(x) for x in got] == expect


def test_golden_misaligned(cuda, golden):
    # test3: every vector at 1..7 bytes past an alignment boundary
    vecs = golden["calculate"]
    for mis in range(1, 8):
        bufs = [bytes.fromhex(v["hex"]) for v in vecs]
        arena, offs, lens = _pack(bufs, align=8, lead=0)
        offs = [o + mis for o in offs]
        arena2 = np.zeros(arena.size + 8, np.uint8)
        for o, b in zip(offs, bufs):
            arena2[o:o + len(b)] = np.frombuffer(b, np.uint8) if b else arena2[o:o]
        got = _dev_batch(cuda, arena2, offs, lens)
        assert [int(x) for x in got] == [v["crc"] for v in vecs], mis


def test_golden_blob_as_segments(cuda, golden):
    # test7/8: blob CRC == CRC of the concatenation (one message per blob)
    bufs = [b"".join(bytes.fromhex(h) for h in v["buffers_hex"]) for v in golden["blob"]]
    arena, offs, lens = _pack(bufs)
    got = _dev_batch(cuda, arena, offs, lens)
    assert [int(x) for x in got] == [v["crc"] for v in golden["blob"]]


def test_data_file_fixture(cuda, golden):
    # journal recovery: CRC of the app data of each MESSAGE record in the DATA file
    import os
    df = golden["data_file"]
    data = np.fromfile(os.path.join(os.path.dirname(__file__), "golden", df["file"]), np.uint8)
    offs = [r["record_offset"] + r["header_bytes"] for r in df["records"]]
    lens = [r["app_data_len"] for r in df["records"]]
    got = _dev_batch(cuda, data, offs, lens)
    assert [int(x) for x in got] == [r["crc"] for r in df["records"]]


@pytest.mark.parametrize("seg_bytes", [256, 384, 1024, 16384, 65536])
def test_random_vs_oracle(cuda, seg_bytes):
    rng = np.random.default_rng(1234 + seg_bytes)
    arena = rng.integers(0, 256, size=3 << 20, dtype=np.uint8)
    n = 3000
    lens = rng.choice([0, 1, 2, 3, 4, 5, 7, 31, 32, 33, 127, 128, 129, 255, 256, 257, 1000,
                       4096, 5000, 65536, 100000], size=n)
    offs = np.array([rng.integers(0, arena.size - l + 1) for l in lens], dtype=np.int64)
    seeds = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    seeds[rng.random(n) < 0.3] = 0
    got = _dev_batch(cuda, arena, offs, lens, seeds, seg_bytes=seg_bytes)
    exp = oracle.batch(arena, offs, lens, seeds, nthreads=8)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, [(int(i), int(offs[i]), int(lens[i])) for i in bad[:10]]


def test_small_ragged_batches(cuda):
    # Small mixed batches (a PUT event's worth of messages): the planner's
    # size-class sort puts a message's segments into different buckets, so a
    # wave can hold one message in two separate lane runs.
    import torch
    rng = np.random.default_rng(4321)
    arena_np = rng.integers(0, 256, size=4 << 20, dtype=np.uint8)
    arena = torch.from_numpy(arena_np).to(cuda)
    for t in range(240):
        n = int(rng.integers(2, 70))
        seg = int(rng.choice([0, 0, 256, 384, 512, 1024]))
        hi = 100000 if seg == 0 else 3000
        lens = rng.integers(0, hi, size=n).astype(np.uint32)
        offs = np.array([rng.integers(0, arena_np.size - l + 1) for l in lens], np.int64)
        seeds = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
        got = Crc32c.calculate_batch(arena, torch.from_numpy(offs).to(cuda),
                                     torch.from_numpy(lens.astype(np.int32)).to(cuda),
                                     torch.from_numpy(seeds.view(np.int32)).to(cuda),
                                     seg_bytes=seg).cpu().numpy().view(np.uint32)
        exp = oracle.batch(arena_np, offs, lens, seeds)
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, (t, seg, [(int(i), int(offs[i]), int(lens[i])) for i in bad[:5]])


@pytest.mark.parametrize("host", [False, True])
def test_whole_messages_flag(cuda, golden, host):
    # BMQCRC_F_WHOLE_MESSAGES: one lane per message, no planner -- any lengths
    # (empty, tiny, line-crossing, and long ones that keep a wave busy)
    import torch
    rng = np.random.default_rng(99 + host)
    arena_np = rng.integers(0, 256, size=3 << 20, dtype=np.uint8)
    lens = rng.choice([0, 0, 1, 2, 3, 4, 5, 31, 127, 128, 129, 255, 256, 1000, 4096, 16385,
                       70000, 300000], size=5000).astype(np.uint32)
    offs = np.array([rng.integers(0, arena_np.size - l + 1) for l in lens], np.int64)
    seeds = rng.integers(0, 2**32, size=lens.size, dtype=np.uint64).astype(np.uint32)
    seeds[rng.random(lens.size) < 0.3] = 0
    exp = oracle.batch(arena_np, offs, lens, seeds, nthreads=8)
    if host:
        got = Crc32c.calculate_batch(arena_np, offs, lens, seeds, whole_messages=True)
    else:
        got = Crc32c.calculate_batch(
            torch.from_numpy(arena_np).to(cuda), torch.from_numpy(offs).to(cuda),
            torch.from_numpy(lens.view(np.int32)).to(cuda),
            torch.from_numpy(seeds.view(np.int32)).to(cuda),
            whole_messages=True).cpu().numpy().view(np.uint32)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, [(int(i), int(offs[i]), int(lens[i])) for i in bad[:8]]
    # golden vectors, one batch
    vec = golden["calculate"]
    blob = b"".join(bytes.fromhex(v["hex"]) for v in vec)
    o = np.cumsum([0] + [len(bytes.fromhex(v["hex"])) for v in vec])[:-1]
    ln = np.array([len(bytes.fromhex(v["hex"])) for v in vec], np.uint32)
    got = Crc32c.calculate_batch(np.frombuffer(blob, np.uint8), o, ln, whole_messages=True)
    assert got.tolist() == [v["crc"] for v in vec]


def test_line_boundary_edges(cuda):
    # starts near the end of a 128-byte line (seed word crossing lines), tiny lengths
    rng = np.random.default_rng(7)
    arena = rng.integers(0, 256, size=1 << 16, dtype=np.uint8)
    offs, lens = [], []
    for base in (0, 1024, 4096):
        for s in range(116, 140):
            for ln in (1, 2, 3, 4, 5, 6, 9, 125, 126, 127, 128, 129, 130, 300):
                offs.append(base + s)
                lens.append(ln)
    seeds = rng.integers(0, 2**32, size=len(offs), dtype=np.uint64).astype(np.uint32)
    for seg in (256, 16384):
        got = _dev_batch(cuda, arena, offs, lens, seeds, seg_bytes=seg)
        exp = oracle.batch(arena, offs, lens, seeds)
        assert np.array_equal(got, exp), seg


def test_threaded_equivalent(cuda):
    # test5: 10000 payloads of lengths 1..10000 (here one batch; serial oracle)
    rng = np.random.default_rng(5)
    lens = np.arange(1, 10001, dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    arena = rng.integers(0, 256, size=int(lens.sum()) + 64, dtype=np.uint8)
    got = _dev_batch(cuda, arena, offs, lens)
    exp = oracle.batch(arena, offs, lens, nthreads=8)
    assert np.array_equal(got, exp)


def test_host_pointer_path(cuda):
    rng = np.random.default_rng(11)
    arena = rng.integers(0, 256, size=1 << 20, dtype=np.uint8)
    lens = rng.integers(0, 20000, size=200)
    offs = np.array([rng.integers(0, arena.size - l + 1) for l in lens], dtype=np.uint64)
    got = Crc32c.calculate_batch(arena, offs, lens)
    exp = oracle.batch(arena, offs, lens)
    assert np.array_equal(got, exp)


def test_overlapping_messages(cuda):
    rng = np.random.default_rng(13)
    arena = rng.integers(0, 256, size=1 << 16, dtype=np.uint8)
    offs = np.arange(0, 4000, 3)
    lens = np.full(offs.size, 60000 - 4000)
    got = _dev_batch(cuda, arena, offs, lens, seg_bytes=512)
    exp = oracle.batch(arena, offs, lens, nthreads=8)
    assert np.array_equal(got, exp)


def test_overlapping_ragged_overflow(cuda):
    # Ragged messages that overlap so much that the segment count exceeds the
    # planner's map (n + arena/seg): segments past it are resolved by binary
    # search over the prefix in the fold (the overflow path).
    rng = np.random.default_rng(14)
    arena = rng.integers(0, 256, size=1 << 16, dtype=np.uint8)
    n = 3000
    lens = rng.integers(0, 60000, size=n)
    offs = np.array([rng.integers(0, arena.size - l + 1) for l in lens], np.int64)
    segs = int(((lens + 511) // 512).sum())
    assert segs > n + arena.size // 512 + 64  # really past the map
    got = _dev_batch(cuda, arena, offs, lens, seg_bytes=512)
    exp = oracle.batch(arena, offs, lens, nthreads=8)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, [(int(i), int(offs[i]), int(lens[i])) for i in bad[:8]]


def test_fill_matches_oracle_stream(cuda):
    import torch
    from blazingmq_amd import fill_synthetic
    t = torch.empty(100003, dtype=torch.uint8, device=cuda)
    fill_synthetic(t, 42)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), oracle.fill_payload(0, t.numel(), 42))


# ----------------------------------------------------------------------------
# BASELINE.json configurations at full size
# ----------------------------------------------------------------------------
def _device_batch_from_stream(cuda, lens, seed, seg_bytes=0):
    import torch
    from blazingmq_amd import fill_synthetic
    lens = np.asarray(lens, dtype=np.uint32)
    offs = np.zeros(lens.size, dtype=np.int64)
    np.cumsum(lens[:-1], dtype=np.int64, out=offs[1:])
    total = int(lens.sum(dtype=np.uint64))
    arena = torch.empty(total + 8, dtype=torch.uint8, device=cuda)
    fill_synthetic(arena, seed)
    o = torch.from_numpy(offs).to(cuda)
    ln = torch.from_numpy(lens.view(np.int32)).to(cuda)
    out = Crc32c.calculate_batch(arena, o, ln, seg_bytes=seg_bytes)
    return arena, offs, lens, out.cpu().numpy().view(np.uint32)


def _oracle_all(arena_t, offs, lens):
    host = arena_t.cpu().numpy()
    return oracle.batch(host, offs.astype(np.uint64), lens, nthreads=16)


def test_config_1k_x_4KiB_planned_then_speculative(cuda):
    """configs[0] exactly as bench.py runs it (1,000 x 4,096 B of synthetic
    stream 0xB1A2E5, contiguous, automatic segments): the first batch on a
    fresh stream is planned; the next ones are ONE k_fold launch that assumes
    u = 16 segments of 256 B per message (BatchArgs::spec).  Every CRC of
    every batch equals the oracle's (the reference's CPU case for this size
    is bmqp_crc32c.h:122)."""
    import torch
    from blazingmq_amd import fill_synthetic, forget_shape, last_launch
    n, size, seed = 1000, 4096, 0xB1A2E5
    arena = torch.empty(n * size, dtype=torch.uint8, device=cuda)
    s = torch.cuda.Stream(cuda)
    with torch.cuda.stream(s):
        fill_synthetic(arena, seed, stream=s)
    s.synchronize()
    host = oracle.fill_payload(0, n * size, seed)
    assert np.array_equal(arena.cpu().numpy(), host)
    offs = np.arange(n, dtype=np.int64) * size
    lens = np.full(n, size, dtype=np.uint32)
    exp = oracle.batch(host, offs.astype(np.uint64), lens)
    o = torch.from_numpy(offs).to(cuda)
    ln = torch.from_numpy(lens.view(np.int32)).to(cuda)

    def run():
        got = Crc32c.calculate_batch(arena, o, ln, stream=s)
        s.synchronize()
        bad = np.nonzero(got.cpu().numpy().view(np.uint32) != exp)[0]
        assert bad.size == 0, bad[:8]
        return last_launch(cuda.index, s)

    forget_shape(cuda.index, s)
    planned = run()
    assert planned["spec"] == 0 and planned["kernels"] >= 2 and planned["seg_bytes"] == 256
    for _ in range(3):
        assert run() == {"kernels": 1, "spec": 16, "seg_bytes": 256, "map": 0}
    forget_shape(cuda.index, s)
    assert run()["spec"] == 0                   # planned again, then speculative again
    assert run()["spec"] == 16
    # with the prediction dropped, a declared length range that has one
    # uniform segment count (bmqcrc_opts.min_len / max_len, ABI 2.5) is the
    # same single launch, no planner and no history needed

    def declared():
        got = Crc32c.calculate_batch(arena, o, ln, stream=s, max_len=size, min_len=size)
        s.synchronize()
        assert np.array_equal(got.cpu().numpy().view(np.uint32), exp)
        return last_launch(cuda.index, s)

    for _ in range(3):
        forget_shape(cuda.index, s)
        assert declared() == {"kernels": 1, "spec": 16, "seg_bytes": 256, "map": 0}


def test_config_1M_x_256B_full(cuda):
    arena, offs, lens, got = _device_batch_from_stream(cuda, np.full(1 << 20, 256), 1)
    assert np.array_equal(got, _oracle_all(arena, offs, lens))


def test_config_64k_x_64KiB_full_and_seg_invariant(cuda):
    # the headline batch, every one of its 65,536 messages against the oracle
    arena, offs, lens, got = _device_batch_from_stream(cuda, np.full(65536, 65536), 2)
    exp = _oracle_all(arena, offs, lens)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, bad[:8]
    # size-independent property: the segment size must not change any result
    import torch
    o = torch.from_numpy(offs).to(cuda)
    ln = torch.from_numpy(lens.view(np.int32)).to(cuda)
    for seg in (1024, 4096, 65536):
        alt = Crc32c.calculate_batch(arena, o, ln, seg_bytes=seg).cpu().numpy().view(np.uint32)
        assert np.array_equal(alt, got), seg


def test_config_16_x_256MiB_full(cuda):
    arena, offs, lens, got = _device_batch_from_stream(cuda, np.full(16, 256 << 20), 5)
    assert np.array_equal(got, _oracle_all(arena, offs, lens))
    # chaining property: CRC of the 4 GiB concatenation equals combining the
    # 16 message CRCs (here: one 2^32-1-byte-capped message cannot hold it,
    # so check pairs: crc(m0||m1) == combine(crc m0, crc m1, len m1))
    import torch
    o = torch.tensor([0], dtype=torch.int64, device=cuda)
    ln = torch.tensor([np.uint32(512 << 20).view(np.int32)], dtype=torch.int32, device=cuda)
    pair = int(Crc32c.calculate_batch(arena, o, ln).cpu().numpy().view(np.uint32)[0])
    assert pair == Crc32c.combine(int(got[0]), int(got[1]), 256 << 20)


def test_config_zipf_full(cuda):
    rng = np.random.default_rng(3)
    r = np.arange(1, 16385, dtype=np.float64)
    p = r ** -1.5
    p /= p.sum()
    lens = (64 * rng.choice(16384, size=4 << 20, p=p) + 64).astype(np.uint32)
    arena, offs, lens, got = _device_batch_from_stream(cuda, lens, 4)
    assert np.array_equal(got, _oracle_all(arena, offs, lens))


def test_multi_device_host_api(cuda):
    from blazingmq_amd import calculate_batch_multi, device_count
    rng = np.random.default_rng(17)
    arena = rng.integers(0, 256, size=8 << 20, dtype=np.uint8)
    lens = rng.integers(0, 70000, size=400)
    offs = np.array([rng.integers(0, arena.size - l + 1) for l in lens], dtype=np.uint64)
    devs = list(range(device_count())) * 2  # same device twice = two shards/streams
    got = calculate_batch_multi(arena, offs, lens, devices=devs)
    assert np.array_equal(got, oracle.batch(arena, offs, lens, nthreads=8))


def test_cpp_dropin_gpu_batch(cuda):
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(__file__), "cpp", "bin", "bmqp_selftest")
    env = dict(os.environ, BMQCRC_GOLDEN_DIR=os.path.join(os.path.dirname(__file__), "golden"))
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr


def test_shape_hint_misprediction(cuda):
    # After a closed-form batch (every message one segment) the next batch on
    # the same stream skips the segment-map launches; a ragged batch then maps
    # its segments by binary search in k_fold.  Both must be bit-exact, and so
    # must the ragged batch after it (planned again) and a closed-form one after
    # that (mispredicted the other way: map launches that exit early).
    import torch
    rng = np.random.default_rng(77)
    arena_np = rng.integers(0, 256, size=6 << 20, dtype=np.uint8)
    arena = torch.from_numpy(arena_np).to(cuda)
    s = torch.cuda.Stream(cuda)

    def run(lens):
        lens = np.asarray(lens, np.uint32)
        offs = np.array([rng.integers(0, arena_np.size - l + 1) for l in lens], np.int64)
        seeds = rng.integers(0, 2**32, size=lens.size, dtype=np.uint64).astype(np.uint32)
        got = Crc32c.calculate_batch(arena, torch.from_numpy(offs).to(cuda),
                                     torch.from_numpy(lens.view(np.int32)).to(cuda),
                                     torch.from_numpy(seeds.view(np.int32)).to(cuda),
                                     stream=s, seg_bytes=1024)
        s.synchronize()
        exp = oracle.batch(arena_np, offs, lens, seeds, nthreads=8)
        bad = np.nonzero(got.cpu().numpy().view(np.uint32) != exp)[0]
        assert bad.size == 0, [(int(i), int(lens[i])) for i in bad[:8]]

    closed = rng.integers(1, 1025, size=5000)          # one segment each
    uniform = np.full(3000, 3000)                       # three segments each
    ragged = rng.integers(0, 20000, size=4000)
    # planner blocks of 1024 messages: the first five uniform (k_plan skips
    # their seg_first, the binary search recomputes it), the rest ragged
    mixed = np.concatenate([rng.integers(1, 1025, size=5120), rng.integers(0, 9000, size=3000)])
    for lens in (closed, mixed, closed, ragged, ragged, uniform, ragged, closed, mixed, closed):
        run(lens)


def test_auto_2k_batch_every_planner_path(cuda):
    """An automatically sized 2 KiB batch (>= 512 MiB of arena) of 1.5M short
    messages with long ones mixed in -- lengths on either side of 64 KiB and
    of 4 KiB multiples up to 1 MiB, seeds -- bit-exact through every planner
    path: the light planner's search, the size-class map (past four tiles
    per block: register and reloaded tiles), a given-up map, and the
    host-buffer call that sees the lengths.  (Round 6 ran a two-tier
    segmentation experiment against it, Appendix A.)"""
    import torch
    from blazingmq_amd import last_launch, plan_wait
    rng = np.random.default_rng(2024)
    arena_np = rng.integers(0, 256, size=640 << 20, dtype=np.uint8)
    arena = torch.from_numpy(arena_np).to(cuda)
    edges = np.array([65535, 65536, 65537, 65536 + 4095, 65536 + 4096, 65536 + 4097,
                      2 * 65536 - 1, 4096 * 63, 4096 * 64 + 1, 1 << 20], np.uint32)
    lens = np.concatenate([rng.integers(1, 2048, size=1_500_000),
                           rng.integers(4096, 65536, size=3000),
                           rng.integers(65536, 600_000, size=1500),
                           np.repeat(edges, 20)]).astype(np.uint32)
    rng.shuffle(lens)
    offs = (rng.random(lens.size) * (arena_np.size - lens + 1)).astype(np.int64)
    seeds = rng.integers(0, 2**32, size=lens.size, dtype=np.uint64).astype(np.uint32)
    exp = oracle.batch(arena_np, offs, lens, seeds, nthreads=8)
    d_offs = torch.from_numpy(offs).to(cuda)
    d_lens = torch.from_numpy(lens.view(np.int32)).to(cuda)
    d_seeds = torch.from_numpy(seeds.view(np.int32)).to(cuda)
    s = torch.cuda.Stream(cuda)

    def check(tag):
        got = Crc32c.calculate_batch(arena, d_offs, d_lens, d_seeds, stream=s)
        s.synchronize()
        bad = np.nonzero(got.cpu().numpy().view(np.uint32) != exp)[0]
        assert bad.size == 0, (tag, bad.size, [(int(i), int(lens[i])) for i in bad[:6]])
        return last_launch(cuda.index, s)

    ll = check("first batch (light planner, search)")
    assert ll["seg_bytes"] == 2048, ll
    ll = check("size-class map")
    assert ll["map"] == 1, ll
    check("map again")
    plan_wait(cuda.index, s, 0)
    check("map given up")
    plan_wait(cuda.index, s, 100)
    check("mapped after")
    got = Crc32c.calculate_batch(arena_np, offs, lens, seeds)
    assert np.array_equal(np.asarray(got).view(np.uint32), exp)


def test_planner_map_given_up(cuda, record_property, perf_bound):
    # Ragged batches are planned by one kernel whose blocks meet once,
    # grid-wide.  When they cannot all run at once a block stops waiting after
    # bmqcrc_plan_wait's limit and the map is given up; every block still
    # writes seg_first and the out[] initialisation, and the fold then maps
    # segments by searching seg_first (round 4; round 3 folded every message
    # whole in one lane, so a multi-MiB message held its wave for its whole
    # length).  A zero limit gives every map up before the first poll: the
    # CRCs must not change, the counter must count every such batch, and a
    # given-up batch holding 32 MiB messages must stay within a small factor
    # of the mapped step.  The default limit maps normally.
    import time

    import torch
    from blazingmq_amd import last_launch, plan_wait
    rng = np.random.default_rng(91)
    arena_np = rng.integers(0, 256, size=96 << 20, dtype=np.uint8)
    arena = torch.from_numpy(arena_np).to(cuda)
    s = torch.cuda.Stream(cuda)
    # more than four planner tiles per block (> 1.3M messages): the
    # single-pass planner, not the round-2 pair
    lens = np.concatenate([rng.integers(0, 200, size=1_400_000),
                           rng.integers(0, 300000, size=300),
                           rng.integers(1000, 9000, size=5000),
                           np.full(3, 32 << 20)]).astype(np.uint32)
    rng.shuffle(lens)
    offs = (rng.random(lens.size) * (arena_np.size - lens + 1)).astype(np.int64)
    seeds = rng.integers(0, 2**32, size=lens.size, dtype=np.uint64).astype(np.uint32)
    exp = oracle.batch(arena_np, offs, lens, seeds, nthreads=8)
    d_offs = torch.from_numpy(offs).to(cuda)
    d_lens = torch.from_numpy(lens.view(np.int32)).to(cuda)
    d_seeds = torch.from_numpy(seeds.view(np.int32)).to(cuda)

    def run(reps=1):
        # the fastest of `reps` synchronised batches: a noisy neighbour on the
        # GPU or host can only lengthen a sample, so the minimum is the stable
        # statistic for the ratio asserted below
        best = float("inf")
        for _ in range(reps):
            torch.cuda.synchronize(cuda)
            t0 = time.perf_counter()
            got = Crc32c.calculate_batch(arena, d_offs, d_lens, d_seeds, stream=s,
                                         seg_bytes=2048, sync=False)
            s.synchronize()
            best = min(best, time.perf_counter() - t0)
            bad = np.nonzero(got.cpu().numpy().view(np.uint32) != exp)[0]
            assert bad.size == 0, [(int(i), int(lens[i])) for i in bad[:8]]
        return best

    v0 = plan_wait(cuda.index, s)
    run()
    t_map = run(5)
    assert last_launch(cuda.index, s)["kernels"] == 2  # k_plan_map + k_fold
    assert plan_wait(cuda.index, s, 0) == v0  # a lone stream: every map was kept
    run()
    t_void = run(5)
    v1 = plan_wait(cuda.index, s, 1000)
    assert v1 == v0 + 6  # the zero limit gives up every launch's map
    print("mapped %.3f ms, given up %.3f ms per batch" % (1e3 * t_map, 1e3 * t_void))
    record_property("given_up_over_mapped", round(t_void / t_map, 3))
    # DESIGN.md 4 claims 1.14x on Zipf; the wall clock here includes the
    # launch and synchronisation overhead common to both, so the bound is
    # 1.3x plus 0.2 ms (asserted under -m perf only, recorded always)
    perf_bound("given_up_within_1.3x", t_void < 1.3 * t_map + 2e-4,
               {"t_map_ms": round(1e3 * t_map, 3), "t_void_ms": round(1e3 * t_void, 3)})
    run()  # back to mapping
    assert plan_wait(cuda.index, s) == v1


def test_given_up_map_switches_the_workspace_to_the_pair(cuda):
    # After k_fold reports a given-up map on a workspace, the host plans that
    # workspace's next kPairAfterVoid (16) ragged batches with the meeting-free
    # pair k_plan + k_plan_sort (3 kernels), then tries the single-pass
    # planner again (2 kernels).  A zero limit (the test hook) never switches.
    import torch
    from blazingmq_amd import last_launch, plan_wait
    rng = np.random.default_rng(93)
    arena_np = rng.integers(0, 256, size=16 << 20, dtype=np.uint8)
    arena = torch.from_numpy(arena_np).to(cuda)
    s = torch.cuda.Stream(cuda)
    lens = np.concatenate([rng.integers(0, 300, size=1_400_000),
                           rng.integers(0, 100000, size=100)]).astype(np.uint32)
    rng.shuffle(lens)
    offs = (rng.random(lens.size) * (arena_np.size - lens + 1)).astype(np.int64)
    exp = oracle.batch(arena_np, offs, lens, None, nthreads=8)
    d_offs = torch.from_numpy(offs).to(cuda)
    d_lens = torch.from_numpy(lens.view(np.int32)).to(cuda)

    def run():
        got = Crc32c.calculate_batch(arena, d_offs, d_lens, stream=s, seg_bytes=2048)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), exp)
        return last_launch(cuda.index, s)["kernels"]

    plan_wait(cuda.index, s, 0)
    assert [run() for _ in range(3)] == [2, 2, 2]  # the hook: every map given up, no switch
    v = plan_wait(cuda.index, s, 1000)
    kernels = [run() for _ in range(18)]
    assert kernels == [3] * 16 + [2, 2], kernels
    assert plan_wait(cuda.index, s) == v  # the pair and the retried single pass kept their maps


def test_planners_on_two_streams_at_once(cuda, record_property):
    # Two large ragged batches enqueued on two streams without waiting: their
    # single-pass planners may share the GPU, so a planner's blocks may not
    # all be resident together and a block may give its map up (exact either
    # way).  Every CRC of both batches must match, with the default wait
    # limit and with a zero limit that gives every map up; the number of
    # given-up maps is recorded (test property plan_voided).
    import torch
    from blazingmq_amd import plan_wait
    rng = np.random.default_rng(92)
    arena_np = rng.integers(0, 256, size=64 << 20, dtype=np.uint8)
    arena = torch.from_numpy(arena_np).to(cuda)
    streams = [torch.cuda.Stream(cuda), torch.cuda.Stream(cuda)]
    batches = []
    for j in range(2):
        lens = np.concatenate([rng.integers(0, 300, size=1_400_000),
                               rng.integers(0, 200000, size=200 + 100 * j)]).astype(np.uint32)
        rng.shuffle(lens)
        offs = (rng.random(lens.size) * (arena_np.size - lens + 1)).astype(np.int64)
        batches.append((torch.from_numpy(offs).to(cuda), torch.from_numpy(lens.view(np.int32)).to(cuda),
                        oracle.batch(arena_np, offs, lens, None, nthreads=8)))
    torch.cuda.synchronize(cuda)
    voided = {}
    for wait_us in (1000, 0, 1000):
        before = [plan_wait(cuda.index, s, wait_us) for s in streams]
        for _ in range(3):
            outs = [Crc32c.calculate_batch(arena, o, ln, None, stream=s, sync=False)
                    for (o, ln, _), s in zip(batches, streams)]
        torch.cuda.synchronize(cuda)
        for (_, _, exp), got in zip(batches, outs):
            assert np.array_equal(got.cpu().numpy().view(np.uint32), exp)
        after = [plan_wait(cuda.index, s, wait_us) for s in streams]
        n = sum(b - a for a, b in zip(before, after))
        voided["wait_%dus" % wait_us] = voided.get("wait_%dus" % wait_us, 0) + n
        if wait_us == 0:
            assert n == 6  # 3 batches x 2 streams, every map given up
    record_property("plan_voided", voided)
    print("plan_voided", voided)


def test_max_length_messages(cuda):
    # The reference's length is an unsigned int (bmqp_crc32c.h:244-246), so the
    # longest message is 2^32 - 1 bytes.  Two such messages (odd offsets,
    # seeds, one overlapping the other) beside a short one, under the
    # automatic shape and the smallest and largest segment sizes.
    import torch
    from blazingmq_amd import fill_synthetic
    nbytes = (1 << 32) + 64
    arena = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
    fill_synthetic(arena, 9)
    offs = np.array([3, 0, 17], dtype=np.int64)
    lens = np.array([0xFFFFFFFF, 1000, 0xFFFFFFFF - 16], dtype=np.uint32)
    seeds = np.array([0x12345678, 0, 0xFFFFFFFF], dtype=np.uint32)
    host = arena.cpu().numpy()
    exp = oracle.batch(host, offs.astype(np.uint64), lens, seeds, nthreads=3)
    del host
    o = torch.from_numpy(offs).to(cuda)
    ln = torch.from_numpy(lens.view(np.int32)).to(cuda)
    sd = torch.from_numpy(seeds.view(np.int32)).to(cuda)
    for seg in (0, 256, 1 << 30):
        got = Crc32c.calculate_batch(arena, o, ln, sd, seg_bytes=seg).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, exp), (seg, got, exp)


@pytest.mark.parametrize("shape", ["uniform", "ragged"])
def test_segment_count_past_32_bits(cuda, shape):
    """Overlapping messages can hold more segments than 32-bit indices count:
    2,200 messages of ~512 MiB at 256-byte segments is ~4.6e9.  The planner
    flags it and the fold takes every message in one lane -- the CRCs stay
    exact (never a wrapped count).  Checked against the planned path at 64 KiB
    segments (19.6M segments, no overflow) and, for three messages, the oracle."""
    import torch
    from blazingmq_amd import fill_synthetic
    L = 1 << 29
    n = 2200
    arena = torch.empty(L + 4096, dtype=torch.uint8, device=cuda)
    fill_synthetic(arena, 21)
    offs = np.arange(n, dtype=np.int64) * 3
    if shape == "uniform":
        lens = np.full(n, L - 4096, dtype=np.uint32)
    else:
        lens = (L - 4096 - np.arange(n) * 7).astype(np.uint32)
    assert int(((lens.astype(np.uint64) + 255) // 256).sum()) > 2**32
    o = torch.from_numpy(offs).to(cuda)
    ln = torch.from_numpy(lens.view(np.int32)).to(cuda)
    got = Crc32c.calculate_batch(arena, o, ln, seg_bytes=256).cpu().numpy().view(np.uint32)
    ref = Crc32c.calculate_batch(arena, o, ln, seg_bytes=65536).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, ref)
    host = arena[:L + 4096].cpu().numpy()
    for i in (0, n // 2, n - 1):
        assert int(got[i]) == oracle.crc32c(host[offs[i]:offs[i] + int(lens[i])].tobytes()), i


def test_batch_leaves_current_device_unchanged(cuda):
    """A drop-in must not retarget the caller's thread: after a batch on an
    explicit device the HIP current device is what it was before."""
    import torch
    from blazingmq_amd import _native as N
    dev_before = torch.cuda.current_device()
    a = np.arange(4096, dtype=np.uint8)
    offs, lens = np.array([0, 100], np.uint64), np.array([4000, 3], np.uint32)
    out = np.zeros(2, np.uint32)
    import ctypes
    for d in range(torch.cuda.device_count()):
        o = N.make_opts(device=d)
        N.check(N.lib.bmqcrc_crc32c_batch(a.ctypes.data, a.size, offs.ctypes.data,
                                          lens.ctypes.data, None, out.ctypes.data, 2,
                                          ctypes.byref(o)))
        assert torch.cuda.current_device() == dev_before
    assert out.tolist() == [oracle.crc32c(a[:4000].tobytes()), oracle.crc32c(a[100:103].tobytes())]


def test_speculative_single_launch(cuda):
    """After a batch of one segment per message, the next batch on the same
    stream runs as ONE k_fold launch with no planner (BatchArgs::spec): lane
    g folds message g, and a message longer than one segment is queued and
    folded in chunks of 64 segments by the waves still running.  Every batch
    of a sequence that mispredicts in every way -- long messages scattered
    among short ones (including the last group), all messages long (one
    chunk each), messages of thousands of segments (many chunks XOR into one
    out word), empty messages, seeds -- is bit-exact against the oracle."""
    import torch
    rng = np.random.default_rng(78)
    arena_np = rng.integers(0, 256, size=48 << 20, dtype=np.uint8)
    arena = torch.from_numpy(arena_np).to(cuda)
    s = torch.cuda.Stream(cuda)
    n = 300_000  # >= 64 messages for every k_fold wave: eligible

    def run(lens, tag):
        lens = np.asarray(lens, np.uint32)
        offs = np.array(rng.integers(0, arena_np.size - lens.astype(np.int64) + 1), np.int64)
        seeds = rng.integers(0, 2**32, size=lens.size, dtype=np.uint64).astype(np.uint32)
        seeds[::3] = 0
        got = Crc32c.calculate_batch(arena, torch.from_numpy(offs).to(cuda),
                                     torch.from_numpy(lens.view(np.int32)).to(cuda),
                                     torch.from_numpy(seeds.view(np.int32)).to(cuda),
                                     stream=s)
        s.synchronize()
        exp = oracle.batch(arena_np, offs, lens, seeds, nthreads=8)
        bad = np.nonzero(got.cpu().numpy().view(np.uint32) != exp)[0]
        assert bad.size == 0, (tag, [(int(i), int(lens[i])) for i in bad[:8]])

    short = lambda: rng.integers(0, 257, size=n)  # noqa: E731  one segment at every auto shape
    scattered = short()
    where = np.concatenate([rng.integers(0, n, size=60), np.arange(n - 40, n)])
    scattered[where] = rng.integers(300, 300_000, size=where.size)
    scattered[-1] = 5 << 20  # thousands of segments, in the very last group
    all_long = np.full(n, 2000)
    for tag, lens in (("identity", short()), ("spec identity", short()),
                      ("spec scattered", scattered), ("planned after", short()),
                      ("spec again", short()), ("spec all long", all_long),
                      ("planned", short()), ("spec empties", np.where(
                          rng.integers(0, 4, size=n) == 0, 0, short())),
                      ("spec", short())):
        run(lens, tag)


def test_one_segment_many_rows(cuda):
    """The 8-wave one-segment kernel over many rows of groups: 1.5M messages
    are 12 groups per wave on 256 CUs.  Repeated launches on one stream, a
    second stream's workspace in between, and mispredicted long messages in
    the first rows and (3,000 of them) in the last third, folded by the
    waves' second pass, are all bit-exact; every speculative batch is one
    launch.  (Round 6 A/B'd a dynamic tail for this kernel against it.)"""
    import torch
    from blazingmq_amd.crc32c import last_launch
    rng = np.random.default_rng(1515)
    arena_np = rng.integers(0, 256, size=64 << 20, dtype=np.uint8)
    arena = torch.from_numpy(arena_np).to(cuda)
    s1, s2 = torch.cuda.Stream(cuda), torch.cuda.Stream(cuda)
    n = 1_500_000

    def run(lens, tag, s):
        lens = np.asarray(lens, np.uint32)
        offs = np.array(rng.integers(0, arena_np.size - lens.astype(np.int64) + 1), np.int64)
        seeds = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
        got = Crc32c.calculate_batch(arena, torch.from_numpy(offs).to(cuda),
                                     torch.from_numpy(lens.view(np.int32)).to(cuda),
                                     torch.from_numpy(seeds.view(np.int32)).to(cuda), stream=s)
        s.synchronize()
        exp = oracle.batch(arena_np, offs, lens, seeds, nthreads=8)
        bad = np.nonzero(got.cpu().numpy().view(np.uint32) != exp)[0]
        assert bad.size == 0, (tag, bad.size, [(int(i), int(lens[i])) for i in bad[:8]])
        return last_launch(cuda.index, s)

    short = lambda: rng.integers(1, 257, size=n)  # noqa: E731  (one segment each: identity)
    run(short(), "planned", s1)
    for k in range(3):
        ll = run(short(), "spec %d" % k, s1)
        assert ll["spec"] == 1 and ll["kernels"] == 1, ll
        if k == 1:
            run(short(), "other stream", s2)
    mixed = short()
    tail = np.arange(n - n // 3, n)
    where = np.concatenate([rng.choice(tail, size=3000, replace=False),
                            rng.integers(0, n - n // 3, size=200)])
    mixed[where] = rng.integers(300, 20_000, size=where.size)
    run(mixed, "spec mispredicted in the tail", s1)
    run(short(), "planned again", s1)
    ll = run(short(), "spec after", s1)
    assert ll["spec"] == 1, ll


@pytest.mark.parametrize("n", [1_000, 100_003, 600_000])
def test_one_segment_pipeline_shapes(cuda, n):
    """The one-segment kernel (every message declared to fit one segment):
    consecutive groups of different line counts (1 to 17 lines at 2 KiB
    segments) in a wave's sequence, the batch's partial last group, 4-wave
    blocks (n = 1,000 and 100,003) and 8-wave blocks (600,000), with and
    without seeds, contiguous 64/256-byte messages like the bench's, and a
    few messages past the declared bound, folded by the second pass.  (Round
    5 A/B'd a rolling two-slot pipeline for this kernel against these
    shapes: correct, but not faster; DESIGN.md Appendix A.)"""
    import torch
    from blazingmq_amd.crc32c import last_launch
    rng = np.random.default_rng(94 + n)
    arena_np = rng.integers(0, 256, size=160 << 20, dtype=np.uint8)  # > 600,000 x 256 B
    arena = torch.from_numpy(arena_np).to(cuda)
    s = torch.cuda.Stream(cuda)

    def run(lens, tag, seeds=True, aligned=False):
        lens = np.asarray(lens, np.uint32)
        if aligned:  # contiguous, like the bench (every stream starts on a line)
            offs = np.zeros(lens.size, np.int64)
            np.cumsum(lens[:-1], out=offs[1:])
        else:
            offs = np.array(rng.integers(0, arena_np.size - lens.astype(np.int64) + 1), np.int64)
        # device-pointer batches are not range-checked by the library: check here
        assert int((offs + lens).max()) <= arena_np.size, tag
        sd = rng.integers(0, 2**32, size=lens.size, dtype=np.uint64).astype(np.uint32)
        got = Crc32c.calculate_batch(arena, torch.from_numpy(offs).to(cuda),
                                     torch.from_numpy(lens.view(np.int32)).to(cuda),
                                     torch.from_numpy(sd.view(np.int32)).to(cuda) if seeds else None,
                                     stream=s, seg_bytes=2048, max_len=2048)
        s.synchronize()
        exp = oracle.batch(arena_np, offs, lens, sd if seeds else None, nthreads=8)
        bad = np.nonzero(got.cpu().numpy().view(np.uint32) != exp)[0]
        assert bad.size == 0, (tag, [(int(i), int(lens[i])) for i in bad[:8]])
        ll = last_launch(cuda.index, s)
        assert ll["kernels"] == 1 and ll["spec"] == 1, (tag, ll)

    per_group = rng.choice([1, 60, 128, 256, 500, 2048], size=(n + 63) // 64)
    blocky = np.repeat(per_group, 64)[:n]       # one line count per group, varying
    mixed = rng.integers(0, 2049, size=n)
    run(mixed, "mixed")
    run(mixed, "mixed, no seeds", seeds=False)
    run(blocky, "one length per group")
    run(np.where(rng.integers(0, 2, size=n) == 0, blocky, mixed), "half and half", seeds=False)
    run(np.full(n, 256), "256 B contiguous", aligned=True, seeds=False)
    run(np.full(n, 64), "64 B contiguous", aligned=True)
    run(rng.integers(0, 129, size=n), "one line or two")
    # streams of at most 64 bytes at any alignment: every group in its lines'
    # second halves (half-line rounds, round 5), with byte cuts at both ends
    # and seed words anywhere in the half
    run(rng.integers(0, 50, size=n), "at most 49 B (half lines)")
    run(rng.integers(0, 50, size=n), "at most 49 B, no seeds", seeds=False)
    run(np.where(rng.integers(0, 8, size=n) == 0, 64, rng.integers(0, 50, size=n)),
        "half lines with full-line groups between")
    past = rng.integers(0, 2049, size=n)
    past[rng.integers(0, n, size=max(1, n // 20000))] = rng.integers(2049, 100_000)
    run(past, "a few past the bound")


def test_declared_max_len_single_launch(cuda):
    """bmqcrc_opts.max_len (ABI 2.4): a device-resident batch whose declared
    bound fits one segment is ONE k_fold launch even right after a ragged
    batch on the same stream (no shape history needed); a bound that some
    messages break, or no bound, stays bit-exact against the oracle."""
    import torch
    from blazingmq_amd.crc32c import last_launch
    rng = np.random.default_rng(91)
    arena_np = rng.integers(0, 256, size=64 << 20, dtype=np.uint8)
    arena = torch.from_numpy(arena_np).to(cuda)
    s = torch.cuda.Stream(cuda)
    n = 300_000

    def run(lens, tag, **kw):
        lens = np.asarray(lens, np.uint32)
        offs = np.array(rng.integers(0, arena_np.size - lens.astype(np.int64) + 1), np.int64)
        seeds = rng.integers(0, 2**32, size=lens.size, dtype=np.uint64).astype(np.uint32)
        got = Crc32c.calculate_batch(arena, torch.from_numpy(offs).to(cuda),
                                     torch.from_numpy(lens.view(np.int32)).to(cuda),
                                     torch.from_numpy(seeds.view(np.int32)).to(cuda),
                                     stream=s, **kw)
        s.synchronize()
        exp = oracle.batch(arena_np, offs, lens, seeds, nthreads=8)
        bad = np.nonzero(got.cpu().numpy().view(np.uint32) != exp)[0]
        assert bad.size == 0, (tag, [(int(i), int(lens[i])) for i in bad[:8]])
        return last_launch(cuda.index, s)

    ragged = lambda: np.minimum(rng.zipf(1.5, size=n) * 64, 1 << 20)  # noqa: E731
    short = lambda: rng.integers(0, 257, size=n)  # noqa: E731
    assert run(ragged(), "ragged")["kernels"] >= 2
    ll = run(short(), "declared after ragged", max_len=256)
    assert ll["kernels"] == 1 and ll["spec"] == 1, ll
    assert run(ragged(), "ragged again")["kernels"] >= 2
    broken = short()
    broken[rng.integers(0, n, size=50)] = rng.integers(300, 200_000, size=50)
    ll = run(broken, "declared bound broken", max_len=256)
    assert ll["kernels"] == 1, ll
    assert run(short(), "after a broken bound, planned")["kernels"] >= 2
    # a bound beyond one segment is only a bound: the launch is planned
    assert run(ragged(), "bound over a segment", max_len=1 << 20)["kernels"] >= 2
    # BMQCRC_F_PLAN takes precedence
    assert run(short(), "plan wins", max_len=256, plan=True)["kernels"] >= 2
    # a declared range of one segment count u (u | 64): the uniform single
    # launch (configs[0]'s shape, 1,000 x 4 KiB), then the range broken
    assert run(ragged()[:1000], "small ragged")["kernels"] >= 2
    ll = run(np.full(1000, 4096), "declared uniform range", max_len=4096, min_len=4096)
    u = (4096 - 1) // ll["seg_bytes"] + 1
    if 2 <= u <= 64 and 64 % u == 0:
        assert ll["kernels"] == 1 and ll["spec"] == u, ll
    broken = np.full(1000, 4096)
    broken[[0, 77, 999]] = [5000, 0, 100]
    run(broken, "declared uniform range broken", max_len=4096, min_len=4096)
    run(rng.integers(3900, 4097, size=1000), "range inside one u", max_len=4096, min_len=3900)


def test_ranks_shard_a_batch_on_the_gpu(cuda):
    """N ranks, one process each (torch.distributed.run, gloo for the result
    hand-off only), each CRCs its byte-balanced slice of one Zipf batch
    through the HIP path on device rank % device_count, every CRC checked
    against the oracle; rank 0 checks the stitched batch.  On a one-GPU box
    both ranks share the GPU; on a node they run on distinct devices."""
    import socket
    import subprocess
    import sys
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    worker = os.path.join(os.path.dirname(__file__), "mp_shard_worker.py")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes", "1",
                        "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), worker],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "bit_exact=True" in r.stdout


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0, 0, 0]])
def test_host_batch_and_verify_over_device_listings(cuda, devices):
    """bmqcrc_opts.ndevices on the plain host-buffer calls: the batch splits
    its messages byte-balanced over the listings, verify cuts the arena into
    ranges (straddling messages on the first listing); both equal the
    one-device call and the oracle, bounded reports included."""
    rng = np.random.default_rng(23)
    arena = rng.integers(0, 256, size=6 << 20, dtype=np.uint8)
    lens = rng.integers(0, 90000, size=700).astype(np.uint32)
    offs = np.array([rng.integers(0, arena.size - l + 1) for l in lens], dtype=np.uint64)
    seeds = rng.integers(0, 2**32, size=lens.size, dtype=np.uint64).astype(np.uint32)
    exp = oracle.batch(arena, offs, lens, seeds, nthreads=8)
    got = Crc32c.calculate_batch(arena, offs, lens, seeds, devices=devices)
    assert np.array_equal(got, exp)
    plain = oracle.batch(arena, offs, lens, nthreads=8)
    wrong = plain.copy()
    victims = sorted(set(int(i) for i in rng.integers(0, lens.size, size=23)))
    wrong[victims] ^= 1
    n_bad, bad = Crc32c.verify_batch(arena, offs, lens, wrong, devices=devices)
    assert n_bad == len(victims) and bad.tolist() == victims
    n_bad, bad = Crc32c.verify_batch(arena, offs, lens, wrong, bad_cap=5, devices=devices)
    assert n_bad == len(victims) and bad.tolist() == victims[:5]


def test_verify_list_longer_than_device_buffer(cuda):
    """The device keeps at most 4 Mi mismatch indices whatever bad_cap is; a
    longer answer comes back in windows: every index, ascending, exactly
    min(n_bad, bad_cap) of them."""
    n = (1 << 22) + 300_001
    arena = np.arange(256, dtype=np.uint8)
    offs = (np.arange(n, dtype=np.uint64) * 7) % 200
    lens = (np.arange(n, dtype=np.uint32) % 50)
    exp = oracle.batch(arena, offs, lens, nthreads=8)
    wrong = exp ^ 1
    wrong[::3] = exp[::3]                        # a third of them intact
    bad_all = np.nonzero(wrong != exp)[0]
    n_bad, bad = Crc32c.verify_batch(arena, offs, lens, wrong, bad_cap=n)
    assert n_bad == bad_all.size and np.array_equal(bad, bad_all)
    cap = (1 << 22) + 17
    n_bad, bad = Crc32c.verify_batch(arena, offs, lens, wrong, bad_cap=cap)
    assert n_bad == bad_all.size and np.array_equal(bad, bad_all[:cap])


def test_speculative_uniform_launch(cuda):
    """After a batch of u segments per message with u dividing 64, the next
    batch on the stream is ONE k_fold launch (BatchArgs::spec = u): a group
    holds 64/u whole messages.  Messages of another segment count (shorter,
    longer, empty, thousands of segments) are folded by their wave's second
    pass; every batch of the sequence is bit-exact, including u = 3 (not a
    divisor of 64: planned as before) and batches smaller than the grid."""
    import torch
    rng = np.random.default_rng(79)
    arena_np = rng.integers(0, 256, size=64 << 20, dtype=np.uint8)
    arena = torch.from_numpy(arena_np).to(cuda)
    s = torch.cuda.Stream(cuda)
    seg = 1024

    def run(lens, tag):
        lens = np.asarray(lens, np.uint32)
        offs = np.array(rng.integers(0, arena_np.size - lens.astype(np.int64) + 1), np.int64)
        seeds = rng.integers(0, 2**32, size=lens.size, dtype=np.uint64).astype(np.uint32)
        seeds[::4] = 0
        got = Crc32c.calculate_batch(arena, torch.from_numpy(offs).to(cuda),
                                     torch.from_numpy(lens.view(np.int32)).to(cuda),
                                     torch.from_numpy(seeds.view(np.int32)).to(cuda),
                                     stream=s, seg_bytes=seg)
        s.synchronize()
        exp = oracle.batch(arena_np, offs, lens, seeds, nthreads=8)
        bad = np.nonzero(got.cpu().numpy().view(np.uint32) != exp)[0]
        assert bad.size == 0, (tag, [(int(i), int(lens[i])) for i in bad[:8]])

    def uniform(u, n):  # lengths of exactly u segments of seg bytes
        return rng.integers((u - 1) * seg + 1, u * seg + 1, size=n)

    for u, n in ((4, 50_000), (16, 1_000), (64, 3_000), (2, 200_000)):
        run(uniform(u, n), "planned u=%d" % u)
        run(uniform(u, n), "spec u=%d" % u)
        odd = uniform(u, n)
        where = rng.integers(0, n, size=max(8, n // 500))
        odd[where] = rng.choice([0, 1, seg, (u + 1) * seg, 100 * seg], size=where.size)
        odd[-1] = 3 << 20  # thousands of segments, in the last group
        run(odd, "spec mispredicted u=%d" % u)
        run(uniform(u, n), "planned again u=%d" % u)
    run(uniform(3, 30_000), "u=3")
    run(uniform(3, 30_000), "u=3 again (not speculative)")
