"""32-bit offset descriptors (BMQCRC_F_OFFSETS32, ABI 2.8) on the GPU: every
kernel the launcher can select, reading uint32 offsets widened by
bmqcrc_opts.offset_shift, against the CPU oracle and against the 64-bit form
of the same call."""
import os

import numpy as np
import pytest

import oracle
from blazingmq_amd import (BmqCrcError, Crc32c, _native as N, last_launch, last_offsets,
                           plan_wait)
from blazingmq_amd.crc32c import verify_batch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _i32(a):
    """A numpy integer array as the int32 tensor the torch form reads as u32."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32))


def _last_offsets():
    """bmqcrc_last_offsets of device 0's default stream, where host-buffer calls run."""
    return last_offsets(0)


class _Arena:
    """One device arena and two streams: the 32-bit calls run on `s`, the
    64-bit form of each call on `s64`, so both streams see the same sequence
    of batch shapes (the shape prediction is per stream)."""

    def __init__(self, cuda, size, seed):
        import torch
        self.cuda, self.rng = cuda, np.random.default_rng(seed)
        self.host = self.rng.integers(0, 256, size=size, dtype=np.uint8)
        self.dev = torch.from_numpy(self.host).to(cuda)
        self.s, self.s64 = torch.cuda.Stream(cuda), torch.cuda.Stream(cuda)

    def run(self, lens, seeds=True, **kw):
        """One batch of random byte-granular offsets in both forms; returns
        last_launch() of the 32-bit call."""
        import torch
        rng, cuda = self.rng, self.cuda
        lens = np.asarray(lens, np.uint32)
        offs = (rng.random(lens.size) * (self.host.size - lens.astype(np.int64) + 1)).astype(
            np.int64)
        sd = rng.integers(0, 2**32, size=lens.size, dtype=np.uint64).astype(np.uint32) \
            if seeds else None
        d_len = _i32(lens).to(cuda)
        d_sd = _i32(sd).to(cuda) if seeds else None
        got = Crc32c.calculate_batch(self.dev, _i32(offs).to(cuda), d_len, d_sd, stream=self.s,
                                     offset_shift=0, **kw)
        launch = last_launch(cuda.index, self.s, offsets=True)
        wide = Crc32c.calculate_batch(self.dev, torch.from_numpy(offs).to(cuda), d_len, d_sd,
                                      stream=self.s64, **kw)
        got = got.cpu().numpy().view(np.uint32)
        exp = oracle.batch(self.host, offs, lens, sd, nthreads=8)
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, [(int(i), int(offs[i]), int(lens[i])) for i in bad[:8]]
        assert np.array_equal(wide.cpu().numpy().view(np.uint32), exp)
        assert launch["offset_bits"] == 32 and launch["offset_shift"] == 0, launch
        assert last_offsets(cuda.index, self.s64) == (64, 0)
        return launch


def test_every_fold_and_planner_path(cuda):
    a = _Arena(cuda, 6 << 20, 77)
    rng = a.rng
    kw = dict(seg_bytes=1024)
    # test_shape_hint_misprediction's sequence; n % 4 takes 1, 2 and 3 (the
    # planner's partial quad)
    closed = rng.integers(1, 1025, size=5001)           # one segment each
    uniform = np.full(3001, 3000)                        # three segments each
    ragged = rng.integers(0, 20000, size=4003)
    ragged[0] = 0                                        # an empty message keeps its seed
    mixed = np.concatenate([rng.integers(1, 1025, size=5120), rng.integers(0, 9000, size=3002)])
    assert sorted({closed.size % 4, mixed.size % 4, ragged.size % 4}) == [1, 2, 3]
    for lens in (closed, mixed, closed, ragged, ragged, uniform, ragged, closed, mixed, closed):
        a.run(lens, **kw)
    for lens in ([9000], [0, 5000], [3, 1025, 2000]):    # the tail alone: no whole quad
        a.run(lens, plan=True, **kw)
        a.run(lens, **kw)
    assert a.run(rng.integers(0, 3001, size=2003), whole_messages=True, **kw)["kernels"] == 1
    assert a.run(ragged, plan=True, **kw)["kernels"] >= 2
    # declared bounds: one launch; the few longer messages take the second pass
    small = rng.integers(1, 1025, size=3001)
    small[rng.integers(0, small.size, size=5)] = rng.integers(1025, 9001, size=5)
    launch = a.run(small, max_len=1024, **kw)
    assert launch["kernels"] == 1 and launch["spec"] == 1, launch
    launch = a.run(rng.integers(1025, 2049, size=3002), min_len=1025, max_len=2048, **kw)
    assert launch["kernels"] == 1 and launch["spec"] == 2, launch   # the uniform single launch
    a.run([0], **kw)
    a.run(ragged, seeds=False, **kw)


def test_pair_planner_and_given_up_map(cuda):
    # test_given_up_map_switches_the_workspace_to_the_pair, in 32 bits: a map
    # given up (zero wait limit), then the pair k_plan + k_plan_sort
    a = _Arena(cuda, 6 << 20, 93)
    lens = a.rng.integers(0, 20001, size=4001)
    plan_wait(cuda.index, a.s64, 0)
    voided = plan_wait(cuda.index, a.s, 0)   # (the call sets the limit and returns the count)
    for _ in range(3):   # light planner, then the single-pass one, its map given up
        assert a.run(lens, seg_bytes=1024)["kernels"] == 2
    assert plan_wait(cuda.index, a.s, 0) > voided
    for s in (a.s, a.s64):
        plan_wait(cuda.index, s)             # the default limit: the workspace takes the pair
    kernels = [a.run(lens, seg_bytes=1024)["kernels"] for _ in range(2)]
    assert kernels == [3, 3], kernels


def test_eight_wave_blocks(cuda):
    import torch
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    wide_segs = 16 * cus * 64      # the launcher's bound on segments for 8-wave blocks
    a = _Arena(cuda, 48 << 20, 5)
    n1 = max(300_001, wide_segs + wide_segs // 8 + 1)
    one = a.rng.integers(1, 257, size=n1)
    assert a.run(one, seg_bytes=256)["kernels"] == 2      # planned
    launch = a.run(one, seg_bytes=256)                    # predicted: the one-segment kernel
    assert launch["kernels"] == 1 and launch["spec"] == 1, launch
    # the launcher goes by its bound on the segments, messages + arena / segment size
    n2 = max(100_003, (wide_segs - a.host.size // 256) // 4 * 4 + 7)
    assert n2 + a.host.size // 256 + 64 >= wide_segs and n2 % 4 == 3
    ragged = a.rng.integers(0, 2049, size=n2)
    assert a.run(ragged, seg_bytes=256)["spec"] == 0
    launch = a.run(ragged, seg_bytes=256)
    assert launch["spec"] == 0 and launch["map"] == 1, launch


def test_offsets_past_2g_and_4g(cuda):
    import torch
    rng = np.random.default_rng(4)
    mib, four_g = 1 << 20, 1 << 32
    arena = torch.empty(four_g + 2 * mib, dtype=torch.uint8, device=cuda)  # allocated, not filled
    windows = {}
    for base in (0, four_g - mib, four_g + mib):
        windows[base] = rng.integers(0, 256, size=mib, dtype=np.uint8)
        arena[base:base + mib].copy_(torch.from_numpy(windows[base]).to(cuda))
    s = torch.cuda.Stream(cuda)
    n = 2000

    def run(base, shift):
        unit = 1 << shift
        lens = rng.integers(1, 3001, size=n).astype(np.uint32)
        rel = (rng.random(n) * (mib - lens.astype(np.int64) + 1)).astype(np.int64) // unit * unit
        offs = rel + base                       # multiples of the unit: base is one of 2^20
        seeds = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
        exp = oracle.batch(windows[base], rel, lens, seeds, nthreads=8)
        d_len, d_sd = _i32(lens).to(cuda), _i32(seeds).to(cuda)
        o32 = offs >> shift
        assert o32.max() < four_g
        got = Crc32c.calculate_batch(arena, _i32(o32).to(cuda), d_len, d_sd, stream=s,
                                     seg_bytes=1024, offset_shift=shift)
        launch = last_launch(cuda.index, s, offsets=True)
        assert launch["offset_bits"] == 32 and launch["offset_shift"] == shift, launch
        bad = np.nonzero(got.cpu().numpy().view(np.uint32) != exp)[0]
        assert bad.size == 0, (base, shift, [(int(i), int(offs[i])) for i in bad[:8]])
        wide = Crc32c.calculate_batch(arena, torch.from_numpy(offs).to(cuda), d_len, d_sd,
                                      stream=s, seg_bytes=1024)
        assert np.array_equal(wide.cpu().numpy().view(np.uint32), exp)
        return o32

    o32 = run(four_g - mib, 0)
    assert (o32.astype(np.uint32).view(np.int32) < 0).all()   # a sign extension shows here
    for shift in (2, 7):                                     # a 32-bit shift shows here
        o32 = run(four_g + mib, shift)
        assert (o32 << shift).min() >= four_g
    run(0, 2)
    run(four_g - mib, 0)    # planned above, predicted here


def test_host_pointers(cuda):
    rng = np.random.default_rng(6)
    arena = rng.integers(0, 256, size=1 << 20, dtype=np.uint8)
    n = 5001
    lens = rng.integers(0, 3000, size=n).astype(np.uint32)
    offs = (rng.random(n) * (arena.size - lens.astype(np.int64) + 1)).astype(np.uint64)
    seeds = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    exp = oracle.batch(arena, offs.astype(np.int64), lens, seeds, nthreads=8)
    wide = Crc32c.calculate_batch(arena, offs, lens, seeds)
    assert _last_offsets() == (64, 0)
    got = Crc32c.calculate_batch(arena, offs.astype(np.uint32), lens, seeds, offset_shift=0)
    assert _last_offsets() == (32, 0)
    assert np.array_equal(got, exp) and np.array_equal(wide, exp)
    got = Crc32c.calculate_batch(arena, offs.astype(np.uint32), lens, seeds, offset_shift=0,
                                 devices=[0, 0])
    assert np.array_equal(got, exp)
    # units of 8 bytes, whole and over two listings of the device
    o8 = (offs >> 3).astype(np.uint32)
    exp8 = oracle.batch(arena, (o8.astype(np.int64) << 3), lens, seeds, nthreads=8)
    for devices in (None, [0, 0]):
        got = Crc32c.calculate_batch(arena, o8, lens, seeds, offset_shift=3, devices=devices)
        assert np.array_equal(got, exp8), devices
    # 0x40000000 << 2 wraps to 0 in 32-bit arithmetic: refused, by index
    o = np.zeros(8, np.uint32)
    o[3] = 0x40000000
    with pytest.raises(BmqCrcError) as e:
        Crc32c.calculate_batch(arena, o, np.full(8, 16, np.uint32), offset_shift=2)
    assert e.value.rc == N.BMQCRC_EINVAL and "message 3 " in str(e.value)
    # (off << shift) + len == arena_bytes is the last message that fits
    edge_off = np.array([(arena.size - 64) >> 2], np.uint32)
    edge_len = np.array([64], np.uint32)
    got = Crc32c.calculate_batch(arena, edge_off, edge_len, offset_shift=2)
    assert got[0] == Crc32c.calculate(arena[-64:])
    with pytest.raises(BmqCrcError):
        Crc32c.calculate_batch(arena, edge_off, edge_len + 1, offset_shift=2)


def test_verify(cuda):
    rng = np.random.default_rng(8)
    arena = rng.integers(0, 256, size=4 << 20, dtype=np.uint8)
    n = 10_000
    lens = rng.integers(0, 2000, size=n).astype(np.uint32)
    offs = (rng.random(n) * (arena.size - lens.astype(np.int64) + 1)).astype(np.uint64)
    expected = oracle.batch(arena, offs.astype(np.int64), lens, None, nthreads=8)
    bad = np.sort(rng.choice(n, size=7, replace=False))
    expected[bad] ^= 0x00010000
    ref = verify_batch(arena, offs, lens, expected)
    assert ref[0] == 7 and ref[1].tolist() == bad.tolist()
    for devices in (None, [0, 0, 0]):
        got = verify_batch(arena, offs.astype(np.uint32), lens, expected, offset_shift=0,
                           devices=devices)
        assert got[0] == ref[0] and got[1].tolist() == ref[1].tolist(), devices
    assert _last_offsets() == (32, 0)


def _after_a_64_bit_batch():
    """Leave the default stream's workspace saying 64, so that a walk's 32 is its own."""
    arena = np.arange(64, dtype=np.uint8)
    Crc32c.calculate_batch(arena, np.array([0], np.uint64), np.array([8], np.uint32))
    assert _last_offsets() == (64, 0)


def test_put_event_walks_choose_the_narrow_form(cuda):
    from blazingmq_amd.put_event import PutEventBuilder, PutMessageIterator
    rng = np.random.default_rng(9)
    apps = [rng.integers(0, 256, size=int(k), dtype=np.uint8).tobytes()
            for k in rng.integers(0, 400, size=257)]
    now, later = PutEventBuilder(defer_crc=False), PutEventBuilder(defer_crc=True)
    for i, app in enumerate(apps):
        now.pack_message(app, queue_id=i)
        later.pack_message(app, queue_id=i)
    want = now.finalize()
    _after_a_64_bit_batch()
    ev = later.finalize()                      # bmqcrc_put_event_fill_crcs
    assert _last_offsets() == (32, 0)
    assert np.array_equal(ev, want)
    _after_a_64_bit_batch()
    assert PutMessageIterator(ev).verify_crcs()[:2] == (257, 0)
    assert _last_offsets() == (32, 0)
    # over two listings of the device each slice keeps the form
    assert PutMessageIterator(ev).verify_crcs(devices=[0, 0])[:2] == (257, 0)
    spread = PutEventBuilder(defer_crc=True, devices=[0, 0])
    for i, app in enumerate(apps):
        spread.pack_message(app, queue_id=i)
    assert np.array_equal(spread.finalize(), want)


def test_storage_walks_choose_the_narrow_form(cuda):
    from blazingmq_amd import csl, storage
    j = np.fromfile(os.path.join(GOLD, "test.bmq_journal"), np.uint8)
    d = np.fromfile(os.path.join(GOLD, "test.bmq_data"), np.uint8)
    _after_a_64_bit_batch()
    r = storage.verify_partition(j, d)
    assert r["n_messages"] > 0 and r["n_bad"] == 0, r
    assert _last_offsets() == (32, 0)
    log = np.fromfile(os.path.join(GOLD, "test.bmq_csl"), np.uint8)
    _after_a_64_bit_batch()
    rc, end, _ = csl.validate_log(log)
    assert rc == 0 and end > 0
    assert _last_offsets() == (32, 0)
