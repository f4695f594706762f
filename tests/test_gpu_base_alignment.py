"""The batch CRC and the fused copy at the base-pointer alignments the ABI
permits.  Everywhere else in the suite a buffer starts where a torch
allocation starts, a multiple of 256 bytes: misalignment comes from offsets
only, and every term of the kernels that reads the low bits of a base pointer
(k_fold's lines and pieces from `arena + off`, the planners' last-segment
class, the copy's pieces from `dst + dof`) is evaluated with those bits zero.
Here the arena, `src`, `dst` and the descriptor and output arrays are views
inside longer allocations (tests/device_views.py): every test asserts the
phase of each pointer it shifts, and checks the sentinel margins around what
the library may write."""
import ctypes

import numpy as np
import pytest

import device_views as V
import oracle
import test_gpu_copy as TC
from blazingmq_amd import (BmqCrcError, Crc32c, HostRegistration, _native as N,
                           calculate_batch_ptr, forget_shape, last_copy, last_launch, plan_wait)

pytestmark = pytest.mark.gpu

SEG = 1024
ARENA = (1 << 20) + 77
PHASES = (1, 3, 4, 8, 12, 15, 16, 17, 63, 64, 65, 100, 127)
# lengths at the edges of a dword, a 16-byte piece, a 128-byte line and of one
# and two segments
EDGES = (0, 1, 2, 3, 4, 5, 15, 16, 17, 127, 128, 129, SEG - 1, SEG, SEG + 1, 2 * SEG - 1, 2 * SEG,
         2 * SEG + 1)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)


def _settle(cuda, stream, dev, size):
    """A pool stream may carry another test's planner history: the default
    wait limit, no batches left for the pair planner (it takes the 16 ragged
    batches after a map given up), no shape prediction."""
    import torch
    plan_wait(cuda.index, stream)
    lens = np.arange(1500, dtype=np.uint32) * 7 % 5000
    offs = torch.from_numpy(np.arange(1500, dtype=np.int64) * 600 % (size - 5000)).to(cuda)
    lens = torch.from_numpy(lens.view(np.int32)).to(cuda)
    for _ in range(20):
        Crc32c.calculate_batch(dev, offs, lens, stream=stream, seg_bytes=SEG)
        launch = last_launch(cuda.index, stream)
        if launch["kernels"] == 2 and launch["map"] == 1:
            break
    else:
        raise AssertionError("the stream's planner did not settle: %r" % (launch,))
    forget_shape(cuda.index, stream)


class _Arena:
    """One host arena as a device view at `phase`, and two fresh streams: the
    32-bit form of every batch runs on `s`, the 64-bit form on `s64` (the
    shape prediction is per stream).  `launches` collects last_launch of both.
    Runs with the same seed make the same batches, whatever the phase: `ref`
    (shared between them) keeps each batch's oracle CRCs, computed once."""

    def __init__(self, cuda, host, phase, seed, ref, shift=0):
        import torch
        self.cuda, self.host, self.ref, self.shift = cuda, host, ref, shift
        self.rng = np.random.default_rng(seed)
        self.dev = V.place(host, phase, cuda)
        assert V.phase_of(self.dev) == phase and self.dev.data_ptr() % 128 == phase % 128
        self.s, self.s64 = torch.cuda.Stream(cuda), torch.cuda.Stream(cuda)
        for s in (self.s, self.s64):
            _settle(cuda, s, self.dev, host.size)
        self.launches = []

    def run(self, lens, seeds=True, pinned=0, **kw):
        """One batch of random byte-granular offsets (multiples of the unit of
        `shift`) in both forms.  Of the first 2 * `pinned` messages the first
        half begin at offset 0 of the view and the second half end on its last
        byte (with a shift, in its last unit)."""
        import torch
        rng, cuda, size, unit = self.rng, self.cuda, self.host.size, 1 << self.shift
        lens = np.asarray(lens, np.uint32)
        room = size - lens.astype(np.int64)
        offs = (rng.random(lens.size) * (room + 1)).astype(np.int64)
        offs[:pinned] = 0
        offs[pinned:2 * pinned] = room[pinned:2 * pinned]
        offs = offs // unit * unit
        sd = rng.integers(0, 2**32, size=lens.size, dtype=np.uint64).astype(np.uint32) \
            if seeds else None
        d_len = torch.from_numpy(_i32(lens)).to(cuda)
        d_sd = torch.from_numpy(_i32(sd)).to(cuda) if seeds else None
        got = Crc32c.calculate_batch(self.dev, torch.from_numpy(_i32(offs >> self.shift)).to(cuda),
                                     d_len, d_sd, stream=self.s, offset_shift=self.shift, **kw)
        launch = last_launch(cuda.index, self.s, offsets=True)
        wide = Crc32c.calculate_batch(self.dev, torch.from_numpy(offs).to(cuda), d_len, d_sd,
                                      stream=self.s64, **kw)
        self.launches.append((launch, last_launch(cuda.index, self.s64, offsets=True)))
        key = len(self.launches)
        if key not in self.ref:
            self.ref[key] = (offs, lens, oracle.batch(self.host, offs, lens, sd, nthreads=8))
        o, l, exp = self.ref[key]
        assert np.array_equal(o, offs) and np.array_equal(l, lens)   # the same batch at every phase
        got = got.cpu().numpy().view(np.uint32)
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, [(int(i), int(offs[i]), int(lens[i])) for i in bad[:8]]
        assert np.array_equal(wide.cpu().numpy().view(np.uint32), exp)
        assert launch["offset_bits"] == 32 and launch["offset_shift"] == self.shift, launch
        V.check_margins(self.dev)
        return launch


def _edged(lens, lo, hi):
    """`lens` with the edge lengths inside [lo, hi] put three times at its
    head: _Arena.run pins the first set to offset 0 and the second to the
    view's end, the third lies anywhere.  Returns (lens, pinned)."""
    e = [x for x in EDGES if lo <= x <= hi]
    lens = np.array(lens)
    lens[:3 * len(e)] = e * 3
    return lens, len(e)


def _every_path(a):
    """test_gpu_offsets32.py::test_every_fold_and_planner_path's sequence with
    smaller batches, every batch with the edge lengths its shape allows."""
    rng = a.rng
    kw = dict(seg_bytes=SEG)
    closed = _edged(rng.integers(1, SEG + 1, size=3001), 1, SEG)     # one segment each
    uniform = (np.full(2001, 3000), 0)                               # three segments each
    ragged = _edged(rng.integers(0, 20000, size=2503), 0, 20000)     # (with an empty message)
    mixed = _edged(np.concatenate([rng.integers(1, SEG + 1, size=2560),
                                   rng.integers(0, 9000, size=1502)]), 0, 9000)
    assert sorted({closed[0].size % 4, mixed[0].size % 4, ragged[0].size % 4}) == [1, 2, 3]
    for lens, pinned in (closed, mixed, closed, ragged, ragged, uniform, ragged, closed, mixed,
                         closed):
        a.run(lens, pinned=pinned, **kw)
    for lens in ([9000], [0, 5000], [3, 1025, 2000]):    # the tail alone: no whole quad
        a.run(lens, plan=True, pinned=1, **kw)
        a.run(lens, pinned=1, **kw)
    lens, pinned = _edged(rng.integers(0, 3001, size=2003), 0, 3001)
    assert a.run(lens, whole_messages=True, pinned=pinned, **kw)["kernels"] == 1
    assert a.run(ragged[0], plan=True, pinned=ragged[1], **kw)["kernels"] >= 2
    # declared bounds: one launch; the few longer messages take the second pass
    small, pinned = _edged(rng.integers(1, SEG + 1, size=3001), 1, SEG)
    small[rng.integers(100, small.size, size=5)] = rng.integers(SEG + 1, 9001, size=5)
    launch = a.run(small, max_len=SEG, pinned=pinned, **kw)
    assert launch["kernels"] == 1 and launch["spec"] == 1, launch
    two, pinned = _edged(rng.integers(SEG + 1, 2 * SEG + 1, size=2002), SEG + 1, 2 * SEG)
    launch = a.run(two, min_len=SEG + 1, max_len=2 * SEG, pinned=pinned, **kw)
    assert launch["kernels"] == 1 and launch["spec"] == 2, launch   # the uniform single launch
    a.run([0], **kw)
    a.run(ragged[0], seeds=False, pinned=ragged[1], **kw)
    return [[{k: l[k] for k in ("kernels", "spec", "map")} for l in pair] for pair in a.launches]


def _arena_bytes(seed):
    return np.random.default_rng(seed).integers(0, 256, size=ARENA, dtype=np.uint8)


def test_every_fold_and_planner_path_at_every_arena_phase(cuda):
    host, ref = _arena_bytes(70), {}
    want = _every_path(_Arena(cuda, host, 0, 77, ref))
    assert {(l["kernels"], l["spec"], l["map"]) for pair in want for l in pair} >= {
        (1, 1, 0), (1, 2, 0), (2, 0, 0), (2, 0, 1)}, want
    for phase in PHASES:
        got = _every_path(_Arena(cuda, host, phase, 77, ref))
        assert got == want, (phase, [(i, g, w) for i, (g, w) in enumerate(zip(got, want))
                                     if g != w])


@pytest.mark.parametrize("phase", [0, 5, 120])
def test_pair_planner_and_given_up_map(cuda, phase):
    # test_gpu_offsets32.py::test_pair_planner_and_given_up_map with the arena
    # at an odd phase and at one that is 8 mod 16 (0: the sequence itself)
    assert phase in (0, 5) or phase % 16 == 8
    a = _Arena(cuda, _arena_bytes(71), phase, 93, {})
    lens, pinned = _edged(a.rng.integers(0, 20001, size=4001), 0, 20001)
    plan_wait(cuda.index, a.s64, 0)
    voided = plan_wait(cuda.index, a.s, 0)   # (the call sets the limit and returns the count)
    for _ in range(3):   # light planner, then the single-pass one, its map given up
        assert a.run(lens, pinned=pinned, seg_bytes=SEG)["kernels"] == 2
    assert plan_wait(cuda.index, a.s, 0) > voided
    for s in (a.s, a.s64):
        plan_wait(cuda.index, s)             # the default limit: the workspace takes the pair
    kernels = [a.run(lens, pinned=pinned, seg_bytes=SEG)["kernels"] for _ in range(2)]
    assert kernels == [3, 3], kernels


@pytest.mark.parametrize("phase", [33, 72])
def test_eight_wave_blocks(cuda, phase):
    # test_gpu_offsets32.py::test_eight_wave_blocks, its shapes, at an odd
    # phase and at 72
    import torch
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    wide_segs = 16 * cus * 64      # the launcher's bound on segments for 8-wave blocks
    host = np.random.default_rng(72).integers(0, 256, size=48 << 20, dtype=np.uint8)
    a = _Arena(cuda, host, phase, 5, {})
    n1 = max(300_001, wide_segs + wide_segs // 8 + 1)
    one = a.rng.integers(1, 257, size=n1)
    assert a.run(one, pinned=4, seg_bytes=256)["kernels"] == 2      # planned
    launch = a.run(one, pinned=4, seg_bytes=256)        # predicted: the one-segment kernel
    assert launch["kernels"] == 1 and launch["spec"] == 1, launch
    # the launcher goes by its bound on the segments, messages + arena / segment size
    n2 = max(100_003, (wide_segs - host.size // 256) // 4 * 4 + 7)
    assert n2 + host.size // 256 + 64 >= wide_segs and n2 % 4 == 3
    ragged = a.rng.integers(0, 2049, size=n2)
    assert a.run(ragged, pinned=4, seg_bytes=256)["spec"] == 0
    launch = a.run(ragged, pinned=4, seg_bytes=256)
    assert launch["spec"] == 0 and launch["map"] == 1, launch


@pytest.mark.parametrize("shift,phase", [(0, 67), (2, 1), (7, 100)])
def test_32_bit_offsets_in_units(cuda, shift, phase):
    # with shift 2 at phase 1 every offset is a multiple of 4 and no address is
    a = _Arena(cuda, _arena_bytes(73), phase, 11, {}, shift=shift)
    rng = a.rng
    for lens, lo, hi in ((rng.integers(1, SEG + 1, size=3001), 1, SEG),
                         (rng.integers(0, 9000, size=2502), 0, 9000),
                         (rng.integers(0, 9000, size=2503), 0, 9000)):
        lens, pinned = _edged(lens, lo, hi)
        a.run(lens, pinned=pinned, seg_bytes=SEG)
        a.run(lens, pinned=pinned, seg_bytes=SEG, plan=True)
    lens, pinned = _edged(rng.integers(0, 3001, size=2001), 0, 3001)
    a.run(lens, pinned=pinned, seg_bytes=SEG, whole_messages=True)


# ---- descriptor and output arrays at element alignment ------------------------

def _batch(rng, n, size, hi):
    lens = rng.integers(0, hi, size=n).astype(np.uint32)
    lens[:len(EDGES)] = [e for e in EDGES if e < hi] + [1] * sum(e >= hi for e in EDGES)
    offs = (rng.random(n) * (size - lens.astype(np.int64) + 1)).astype(np.int64)
    seeds = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    return offs, lens, seeds


# (offsets, lengths, seeds, out) phases: int64 offsets at 8 mod 16; the 32-bit
# arrays at 4, 8 and 12 mod 16, each array's phase different from the others'
ARRAY_PHASES = [((8, 24), 4, 8, 12), ((72, 8), 12, 4, 8), ((120, 12), 8, 12, 4),
                ((8, 4), 140, 72, 60)]


@pytest.mark.parametrize("n", [2001, 2002, 2003, 4000])
@pytest.mark.parametrize("phases", ARRAY_PHASES)
def test_descriptor_and_output_arrays_at_element_alignment(cuda, n, phases):
    import torch
    rng = np.random.default_rng(n)
    host = _arena_bytes(74)
    arena = V.place(host, 0, cuda)
    (p64, p32), p_len, p_sd, p_out = phases
    assert p64 % 16 == 8 and len({p32 % 16, p_len % 16, p_sd % 16, p_out % 16} - {0}) >= 3
    offs, lens, seeds = _batch(rng, n, host.size, 6000)
    exp = oracle.batch(host, offs, lens, seeds, nthreads=8)
    exp0 = oracle.batch(host, offs, lens, None, nthreads=8)
    one = np.minimum(lens, SEG)                     # a batch of one-segment messages
    exp1 = oracle.batch(host, offs, one, seeds, nthreads=8)
    s = torch.cuda.Stream(cuda)
    _settle(cuda, s, arena, host.size)

    def run(form, lens, want, seeds=seeds, **kw):
        d_off = V.place(offs, p64, cuda) if form == 64 else V.place(_i32(offs), p32, cuda)
        d_len, d_sd = V.place(_i32(lens), p_len, cuda), None
        out = V.filled(n, np.uint32, 0x5A5A5A5A, p_out, cuda)
        views = [d_off, d_len, out]
        if seeds is not None:
            d_sd = V.place(_i32(seeds), p_sd, cuda)
            views.append(d_sd)
        assert [V.phase_of(v) for v in views] == [p64 if form == 64 else p32, p_len, p_out] + \
            [p_sd] * (seeds is not None)
        res = Crc32c.calculate_batch(arena, d_off, d_len, d_sd, out, stream=s, seg_bytes=SEG,
                                     offset_shift=None if form == 64 else 0, **kw)
        assert res is out
        got = out.cpu().numpy().view(np.uint32)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (form, kw, [(int(i), int(lens[i])) for i in bad[:8]])
        V.check_margins(*views)     # (out's margins: the elements around it)
        return last_launch(cuda.index, s)

    for form in (64, 32):
        forget_shape(cuda.index, s)
        assert run(form, lens, exp)["kernels"] == 2                    # planned, light
        launch = run(form, lens, exp)                                  # planned, with the map
        assert launch["kernels"] >= 2 and launch["map"] == 1, launch
        run(form, lens, exp0, seeds=None)
        assert run(form, lens, exp, plan=True)["kernels"] >= 2
        assert run(form, lens, exp, whole_messages=True)["kernels"] == 1
        assert run(form, one, exp1, plan=True)["kernels"] >= 2
        run(form, one, exp1)                             # by the stream's history
        launch = run(form, one, exp1, max_len=SEG)       # declared: the one-segment launch
        assert launch["kernels"] == 1 and launch["spec"] == 1, launch


@pytest.mark.parametrize("phases", ARRAY_PHASES[:2])
def test_predicted_single_launch_with_arrays_at_element_alignment(cuda, phases):
    # enough one-segment messages for the launcher to predict the one-segment
    # kernel from the batch before (test_eight_wave_blocks' first shape)
    import torch
    rng = np.random.default_rng(15)
    host = _arena_bytes(76)
    arena = V.place(host, 0, cuda)
    (p64, p32), p_len, p_sd, p_out = phases
    n = 300_001
    lens = rng.integers(1, 257, size=n).astype(np.uint32)
    offs = (rng.random(n) * (host.size - 256)).astype(np.int64)
    seeds = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    exp = oracle.batch(host, offs, lens, seeds, nthreads=8)
    s = torch.cuda.Stream(cuda)
    _settle(cuda, s, arena, host.size)
    for form in (64, 32):
        forget_shape(cuda.index, s)
        for kernels in (2, 1):      # planned, then predicted
            d_off = V.place(offs, p64, cuda) if form == 64 else V.place(_i32(offs), p32, cuda)
            d_len, d_sd = V.place(_i32(lens), p_len, cuda), V.place(_i32(seeds), p_sd, cuda)
            out = V.filled(n, np.uint32, 0x5A5A5A5A, p_out, cuda)
            assert [V.phase_of(v) for v in (d_off, d_len, d_sd, out)] == \
                [p64 if form == 64 else p32, p_len, p_sd, p_out]
            Crc32c.calculate_batch(arena, d_off, d_len, d_sd, out, stream=s, seg_bytes=256,
                                   offset_shift=None if form == 64 else 0)
            launch = last_launch(cuda.index, s)
            assert launch["kernels"] == kernels and launch["spec"] == 2 - kernels, launch
            assert np.array_equal(out.cpu().numpy().view(np.uint32), exp)
            V.check_margins(d_off, d_len, d_sd, out)


@pytest.mark.parametrize("n,phases", [(1001, ARRAY_PHASES[0]), (1002, ARRAY_PHASES[1]),
                                      (1003, ARRAY_PHASES[2])])
def test_verify_on_device_arrays_at_element_alignment(cuda, n, phases):
    # bmqcrc_crc32c_verify over device arrays, `expected` shifted like the
    # others; the report (host memory) at 8 mod 16
    import torch
    rng = np.random.default_rng(n)
    host = _arena_bytes(75)
    arena = V.place(host, 9, cuda)
    (p64, p32), p_len, p_exp, _ = phases
    offs, lens, _ = _batch(rng, n, host.size, 6000)
    expected = oracle.batch(host, offs, lens, None, nthreads=8)
    bad = np.sort(rng.choice(n, size=7, replace=False))
    expected[bad] ^= 0x00010000
    stream = torch.cuda.Stream(cuda)
    for form in (64, 32):
        d_off = V.place(offs, p64, cuda) if form == 64 else V.place(_i32(offs), p32, cuda)
        d_len, d_exp = V.place(_i32(lens), p_len, cuda), V.place(_i32(expected), p_exp, cuda)
        assert [V.phase_of(v) for v in (arena, d_off, d_len, d_exp)] == \
            [9, p64 if form == 64 else p32, p_len, p_exp]
        report = V.filled(16, np.uint64, 0x5A5A5A5A5A5A5A5A, 8, "cpu")
        nbad = ctypes.c_uint64()
        o = N.make_opts(device=cuda.index, stream=stream.cuda_stream, seg_bytes=SEG,
                        flags=N.BMQCRC_F_DEVICE_PTRS, offset_shift=None if form == 64 else 0)
        rc = N.lib.bmqcrc_crc32c_verify(arena.data_ptr(), arena.numel(), d_off.data_ptr(),
                                        d_len.data_ptr(), d_exp.data_ptr(), n, ctypes.byref(nbad),
                                        report.data_ptr(), 16, ctypes.byref(o))
        assert rc == 0, N.lib.bmqcrc_last_error()
        assert nbad.value == 7
        got = report.numpy().view(np.uint64)
        assert got[:7].tolist() == bad.tolist() and (got[7:] == 0x5A5A5A5A5A5A5A5A).all()
        V.check_margins(arena, d_off, d_len, d_exp, report)


@pytest.mark.parametrize("lead", [1, 72])
def test_zero_copy_host_arena_inside_the_registration(cuda, lead):
    import torch
    rng = np.random.default_rng(51)
    arena_np = rng.integers(0, 256, size=(2 << 20) + 77, dtype=np.uint8)
    with HostRegistration(arena_np, device=cuda.index or 0) as reg:
        assert reg.dev_ptr % 16 == 0       # (page-locked memory: the phase is `lead` itself)
        size = reg.nbytes - 129
        assert lead + size < reg.nbytes and (reg.dev_ptr + lead) % 16 == lead % 16 != 0
        window = arena_np[lead:lead + size]
        offs, lens, seeds = _batch(rng, 3003, size, 5000)
        offs[:4], offs[4:8] = 0, size - lens[4:8].astype(np.int64)
        exp = oracle.batch(window, offs, lens, seeds, nthreads=8)
        for kw in (dict(), dict(seg_bytes=SEG), dict(seg_bytes=SEG)):
            got = calculate_batch_ptr(reg.dev_ptr + lead, size, torch.from_numpy(offs).to(cuda),
                                      torch.from_numpy(_i32(lens)).to(cuda),
                                      torch.from_numpy(_i32(seeds)).to(cuda), **kw)
            assert np.array_equal(got.cpu().numpy().view(np.uint32), exp), kw


# ---- the fused copy ------------------------------------------------------------

COPY_PHASES = [(1, 0), (0, 1), (5, 11), (8, 4), (15, 15), (64, 3), (127, 120)]
COPY_LAYOUTS = {"every_length": TC._every_length_at_every_misalignment,
                "all_pairs": TC._all_misalignment_pairs,
                "around_the_chunk": TC._lengths_around_the_chunk,
                "packed": TC._packed_layout}
_copy_cases = {}


@pytest.mark.parametrize("phases", COPY_PHASES)
@pytest.mark.parametrize("layout", sorted(COPY_LAYOUTS))
def test_copy_layouts_at_base_phases(cuda, layout, phases):
    # test_gpu_copy.py's layouts and checks (out against the oracle, the whole
    # destination against the image, the source unchanged), and the margins of
    # both views
    if layout not in _copy_cases:
        _copy_cases[layout] = COPY_LAYOUTS[layout]()
    TC._check(cuda, *_copy_cases[layout], phases=phases)


@pytest.mark.parametrize("phases", [(5, 11), (127, 120)])
def test_copy_fan_out_and_in_place(cuda, phases):
    rng = np.random.default_rng(7)
    src = rng.integers(0, 256, size=8192, dtype=np.uint8)
    # one source range to two destinations, overlapping source ranges
    soff = np.array([100, 100, 150, 100], np.int64)
    lens = np.array([1000, 1000, 700, 33], np.uint32)
    doff = np.array([5, 1005, 2100, 2900], np.int64)
    TC._check(cuda, src, soff, lens, doff, 4096, TC._seeds(rng, 4), phases=phases)
    # dst is src: compaction in place
    buf = rng.integers(0, 256, size=16384, dtype=np.uint8)
    soff = np.array([8192 + 3, 9000, 12000 + 7, 16000], np.int64)
    lens = np.array([500, 2000, 3000, 384], np.uint32)     # (the last ends on the last byte)
    doff = np.array([0, 501, 2501, 5501], np.int64)        # (the first begins on the first)
    d_buf = V.place(buf, phases[0], cuda)
    assert V.phase_of(d_buf) == phases[0]
    seeds = TC._seeds(rng, 4)
    out = Crc32c.copy_batch(d_buf, TC._i64(soff).to(cuda), TC._i32(lens).to(cuda), d_buf,
                            TC._i64(doff).to(cuda), TC._i32(seeds).to(cuda))
    assert np.array_equal(out.cpu().numpy().view(np.uint32), oracle.batch(buf, soff, lens, seeds))
    img = buf.copy()
    for so, ln, do in zip(soff, lens, doff):
        img[do:do + ln] = buf[so:so + ln]
    assert np.array_equal(d_buf.cpu().numpy(), img)
    V.check_margins(d_buf)


def test_copy_bounds_are_enforced_from_the_shifted_bases(cuda):
    # test_gpu_copy.py::test_bounds_are_enforced_on_the_device with src at
    # phase 5 and dst at 11, the descriptor arrays and out at element alignment
    import torch
    rng = np.random.default_rng(8)
    n = 300
    src = rng.integers(0, 256, size=1 << 16, dtype=np.uint8)
    lens = rng.integers(1, 200, size=n).astype(np.uint32)
    soff = (rng.random(n) * 30000).astype(np.int64)
    doff = 2 + np.concatenate([[0], np.cumsum(lens + 2)[:-1]]).astype(np.int64)
    # the declared sizes are smaller than the views: a broken check stays inside them
    src_bytes, dst_bytes = 32768, 40000
    assert doff[-1] + lens[-1] < dst_bytes
    soff[41], lens[41] = src_bytes - 10, 11          # one byte past the declared source
    doff[97] = dst_bytes - int(lens[97]) + 1          # one byte past the declared destination
    soff[250] = (1 << 63) - 8                         # far outside; the sum needs 64 bits
    soff[7], lens[7] = src_bytes - 40, 40             # ends on the declared source's last byte
    doff[298] = dst_bytes - int(lens[298])            # ends on the declared destination's last
    refused = (41, 97, 250)
    d_src = V.place(src, 5, cuda)
    d_dst = V.place(np.full(1 << 16, TC.FILL, np.uint8), 11, cuda)
    out = V.filled(n, np.uint32, 0x5A5A5A5A, 12, cuda)
    d_soff, d_doff, d_len = V.place(soff, 8, cuda), V.place(doff, 24, cuda), \
        V.place(_i32(lens), 4, cuda)
    assert [V.phase_of(v) for v in (d_src, d_dst, out, d_soff, d_doff, d_len)] == \
        [5, 11, 12, 8, 24, 4]
    stream = torch.cuda.current_stream(cuda)

    def call(flags):
        o = N.make_opts(device=cuda.index, stream=stream.cuda_stream, flags=flags)
        return N.lib.bmqcrc_crc32c_copy(d_src.data_ptr(), src_bytes, d_soff.data_ptr(),
                                        d_len.data_ptr(), d_dst.data_ptr(), dst_bytes,
                                        d_doff.data_ptr(), None, out.data_ptr(), n,
                                        ctypes.byref(o))

    rc = call(N.BMQCRC_F_DEVICE_PTRS)
    err = N.lib.bmqcrc_last_error()
    assert rc == N.BMQCRC_EINVAL and b"message 41 " in err, (rc, err)
    assert last_copy(cuda.index, stream) == (n, 3, 41)
    got = out.cpu().numpy().view(np.uint32)
    ok = np.array([i not in refused for i in range(n)])
    exp = oracle.batch(src, np.where(ok, soff, 0), np.where(ok, lens, 0))
    assert np.array_equal(got[ok], exp[ok])
    assert all(got[i] == 0x5A5A5A5A for i in refused)  # left unwritten
    img = TC._image(src, soff, lens, doff, 1 << 16, skip=refused)
    assert np.array_equal(d_dst.cpu().numpy(), img)    # refused destinations still 0xA5
    assert call(N.BMQCRC_F_DEVICE_PTRS | N.BMQCRC_F_ASYNC) == 0
    assert last_copy(cuda.index, stream) == (n, 3, 41)
    V.check_margins(d_src, d_dst, out, d_soff, d_doff, d_len)


@pytest.mark.parametrize("phases", [(1, 0), (8, 4), (127, 120)])
def test_copy_ends_on_the_views_last_byte(cuda, phases):
    # the views are the declared sizes: a message that ends on the last byte
    # of both passes, the same message one byte longer is refused and nothing
    # of it is written (the sentinel behind dst is the byte it would reach)
    rng = np.random.default_rng(9)
    src = rng.integers(0, 256, size=5000, dtype=np.uint8)
    lens = np.array([333, 1000, 77], np.uint32)
    soff = np.array([5000 - 333, 17, 0], np.int64)
    doff = np.array([3000 - 333, 1001, 0], np.int64)
    TC._check(cuda, src, soff, lens, doff, 3000, TC._seeds(rng, 3), phases=phases)
    for k, (s_at, d_at) in enumerate(((5000 - 333, 3000 - 334), (5000 - 334, 3000 - 333))):
        d_src = V.place(src, phases[0], cuda)
        d_dst = V.place(np.full(3000, TC.FILL, np.uint8), phases[1], cuda)
        assert (V.phase_of(d_src), V.phase_of(d_dst)) == phases
        with pytest.raises(BmqCrcError) as e:
            Crc32c.copy_batch(d_src, TC._i64([17, s_at]).to(cuda), TC._i32([100, 334]).to(cuda),
                              d_dst, TC._i64([1001, d_at]).to(cuda))
        assert e.value.rc == N.BMQCRC_EINVAL and "message 1 " in str(e.value), k
        img = TC._image(src, [17], [100], [1001], 3000)
        assert np.array_equal(d_dst.cpu().numpy(), img)
        V.check_margins(d_src, d_dst)
