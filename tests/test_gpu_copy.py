"""Fused copy + CRC (bmqcrc_crc32c_copy, ABI 2.9) on the GPU.  Every check
compares `out` with the CPU oracle and the WHOLE destination tensor with an
image built in numpy (0xA5 everywhere, the messages copied in): a stray or a
missing byte anywhere fails."""
import ctypes

import numpy as np
import pytest

import device_views as V
import oracle
import test_grid_regimes as G
from blazingmq_amd import BmqCrcError, Crc32c, _native as N, last_copy, last_launch

pytestmark = pytest.mark.gpu

C = 65536  # kCopyChunkBytes: a wave's unit of work
FILL = 0xA5


def _i32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32))


def _i64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64))


def _image(src, soff, lens, doff, size, skip=()):
    img = np.full(size, FILL, np.uint8)
    for i, (so, ln, do) in enumerate(zip(soff, lens, doff)):
        if i not in skip:
            img[int(do):int(do) + int(ln)] = src[int(so):int(so) + int(ln)]
    return img


def _check(cuda, src, soff, lens, doff, dst_size, seeds=None, phases=None, **kw):
    """One copy_batch into a fresh 0xA5 destination: out against the oracle,
    the whole destination against the image.  Returns (out, dst tensor).
    `phases` = (src, dst) base-pointer phases: both buffers are then views
    inside longer allocations (tests/device_views.py) whose margins are checked
    too; None is the start of a fresh allocation each."""
    import torch
    lens = np.asarray(lens, np.uint32)
    if phases is None:
        d_src = torch.from_numpy(src).to(cuda)
        d_dst = torch.full((dst_size,), FILL, dtype=torch.uint8, device=cuda)
    else:
        d_src = V.place(src, phases[0], cuda)
        d_dst = V.place(np.full(dst_size, FILL, np.uint8), phases[1], cuda)
        assert (V.phase_of(d_src), V.phase_of(d_dst)) == tuple(phases)
    if phases is None:
        d_sd = _i32(seeds).to(cuda) if seeds is not None else None
        out = Crc32c.copy_batch(d_src, _i64(soff).to(cuda), _i32(lens).to(cuda), d_dst,
                                _i64(doff).to(cuda), d_sd, **kw)
    else:
        # the descriptor and output arrays at their elements' alignment, no more
        arrays = [V.place(np.asarray(soff, np.int64), 8, cuda), V.place(lens, 12, cuda),
                  V.place(np.asarray(doff, np.int64), 72, cuda),
                  V.filled(lens.size, np.uint32, 0x5A5A5A5A, 20, cuda)]
        d_sd = V.place(np.asarray(seeds, np.uint32), 4, cuda) if seeds is not None else None
        assert [V.phase_of(a) for a in arrays] == [8, 12, 72, 20]
        out = Crc32c.copy_batch(d_src, arrays[0], arrays[1], d_dst, arrays[2], d_sd,
                                out=arrays[3], **kw)
        V.check_margins(*arrays)
    torch.cuda.synchronize(cuda)
    got = out.cpu().numpy().view(np.uint32)
    exp = oracle.batch(src, soff, lens, seeds, nthreads=8)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, [(int(i), int(soff[i]), int(doff[i]), int(lens[i])) for i in bad[:8]]
    img = _image(src, soff, lens, doff, dst_size)
    host = d_dst.cpu().numpy()
    diff = np.nonzero(host != img)[0]
    assert diff.size == 0, (diff.size, [int(i) for i in diff[:8]])
    assert torch.equal(d_src.cpu(), torch.from_numpy(src))  # the source is only read
    if phases is not None:
        V.check_margins(d_src, d_dst)
    return got, d_dst


def _layout(rng, lens, smis, dmis, gap=3):
    """Offsets with the given misalignments (mod 16), ranges disjoint."""
    soff, doff, s, d = [], [], 0, 0
    for ln, sm, dm in zip(lens, smis, dmis):
        s = (s + 15) // 16 * 16 + int(sm)
        d = (d + 15) // 16 * 16 + int(dm)
        soff.append(s)
        doff.append(d)
        s += int(ln)
        d += int(ln) + int(rng.integers(0, gap))
    return np.array(soff, np.int64), np.array(doff, np.int64), s + 16, d + 16


def _seeds(rng, n):
    return rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)


def _every_length_at_every_misalignment():
    rng = np.random.default_rng(1)
    lens = rng.permutation(2201)
    smis = np.arange(lens.size) % 16
    dmis = rng.permutation(lens.size) % 16
    assert set(smis) == set(dmis) == set(range(16))
    soff, doff, ssize, dsize = _layout(rng, lens, smis, dmis)
    src = rng.integers(0, 256, size=ssize, dtype=np.uint8)
    return src, soff, lens, doff, dsize, _seeds(rng, lens.size)


def test_every_length_at_every_misalignment(cuda):
    _check(cuda, *_every_length_at_every_misalignment())


def _all_misalignment_pairs():
    # every (source, destination) misalignment pair at lengths around one and
    # two pieces and around a row
    rng = np.random.default_rng(2)
    lens, smis, dmis = [], [], []
    for ln in (1, 15, 16, 17, 31, 33, 1023, 1024, 1041):
        for k in range(256):
            lens.append(ln)
            smis.append(k % 16)
            dmis.append(k // 16)
    soff, doff, ssize, dsize = _layout(rng, lens, smis, dmis)
    src = rng.integers(0, 256, size=ssize, dtype=np.uint8)
    return src, soff, lens, doff, dsize, _seeds(rng, len(lens))


def test_all_misalignment_pairs(cuda):
    _check(cuda, *_all_misalignment_pairs())


def _lengths_around_the_chunk():
    rng = np.random.default_rng(3)
    lens = [C - 1, C, C + 1, 2 * C + 17] * 3
    smis = [0] * 4 + [5] * 4 + [11] * 4
    dmis = [0] * 4 + [0] * 4 + [3] * 4
    soff, doff, ssize, dsize = _layout(rng, lens, smis, dmis)
    src = rng.integers(0, 256, size=ssize, dtype=np.uint8)
    return src, soff, lens, doff, dsize, _seeds(rng, len(lens))


def test_lengths_around_the_chunk(cuda):
    _check(cuda, *_lengths_around_the_chunk())


def _packed_layout():
    # destination ranges end to end with no gap: neighbours share 16-byte
    # pieces, which a read-modify-write of a shared piece would corrupt
    rng = np.random.default_rng(4)
    n = 5003
    lens = rng.integers(1, 301, size=n)
    doff = 7 + np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    src = rng.integers(0, 256, size=1 << 20, dtype=np.uint8)
    soff = (rng.random(n) * (src.size - lens)).astype(np.int64)
    return src, soff, lens, doff, int(doff[-1] + lens[-1]) + 9, _seeds(rng, n)


def test_packed_layout_shares_pieces_between_waves(cuda):
    _check(cuda, *_packed_layout())


def test_long_message_alone_and_among_short_ones(cuda):
    import torch
    rng = np.random.default_rng(5)
    big = 3 * (1 << 20) + 5
    src = rng.integers(0, 256, size=big + (1 << 20), dtype=np.uint8)
    _check(cuda, src, [13], [big], [6], big + 64, np.array([0xCAFEF00D], np.uint32))
    lens = rng.integers(0, 300, size=2001)
    lens[1000] = big
    soff = (rng.random(lens.size) * (1 << 19)).astype(np.int64)
    doff = 3 + np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    seeds = _seeds(rng, lens.size)
    size = int(doff[-1] + lens[-1]) + 32
    first, _ = _check(cuda, src, soff, lens, doff, size, seeds)
    again, _ = _check(cuda, src, soff, lens, doff, size, seeds)
    assert np.array_equal(first, again)
    torch.cuda.synchronize(cuda)


def test_edge_cases(cuda):
    import torch
    rng = np.random.default_rng(6)
    src = rng.integers(0, 256, size=4096, dtype=np.uint8)
    # n = 0
    got, _ = _check(cuda, src, np.zeros(0, np.int64), np.zeros(0, np.uint32),
                    np.zeros(0, np.int64), 256)
    assert got.size == 0
    # n not a multiple of 64, seeds=None
    lens = rng.integers(0, 40, size=131)
    soff = (rng.random(131) * 4000).astype(np.int64)
    doff = 1 + np.concatenate([[0], np.cumsum(lens + 1)[:-1]]).astype(np.int64)
    _check(cuda, src, soff, lens, doff, int(doff[-1]) + 64)
    # all-zero lengths: out = seeds, dst untouched (offsets at the very ends are in range)
    seeds = _seeds(rng, 70)
    soff = np.full(70, 4096, np.int64)
    got, _ = _check(cuda, src, soff, np.zeros(70, np.uint32), np.full(70, 256, np.int64), 256,
                    seeds)
    assert np.array_equal(got, seeds)
    # out given by the caller is the tensor returned
    out = torch.zeros(1, dtype=torch.int32, device=cuda)
    d_src = torch.from_numpy(src).to(cuda)
    d_dst = torch.zeros(64, dtype=torch.uint8, device=cuda)
    res = Crc32c.copy_batch(d_src, _i64([5]).to(cuda), _i32([40]).to(cuda), d_dst,
                            _i64([3]).to(cuda), out=out)
    assert res is out
    assert int(out.cpu().numpy().view(np.uint32)[0]) == oracle.crc32c(src[5:45].tobytes())


def test_fan_out_and_in_place(cuda):
    import torch
    rng = np.random.default_rng(7)
    src = rng.integers(0, 256, size=8192, dtype=np.uint8)
    # one source range to two destinations, overlapping source ranges
    soff = np.array([100, 100, 150, 100], np.int64)
    lens = np.array([1000, 1000, 700, 33], np.uint32)
    doff = np.array([5, 1005, 2100, 2900], np.int64)
    _check(cuda, src, soff, lens, doff, 4096, _seeds(rng, 4))
    # dst is src: compaction in place, destination ranges disjoint from every source range
    buf = rng.integers(0, 256, size=16384, dtype=np.uint8)
    soff = np.array([8192 + 3, 9000, 12000 + 7, 16000], np.int64)
    lens = np.array([500, 2000, 3000, 384], np.uint32)
    doff = np.array([1, 501, 2501, 5501], np.int64)
    d_buf = torch.from_numpy(buf).to(cuda)
    seeds = _seeds(rng, 4)
    out = Crc32c.copy_batch(d_buf, _i64(soff).to(cuda), _i32(lens).to(cuda), d_buf,
                            _i64(doff).to(cuda), _i32(seeds).to(cuda))
    assert np.array_equal(out.cpu().numpy().view(np.uint32), oracle.batch(buf, soff, lens, seeds))
    img = buf.copy()
    for so, ln, do in zip(soff, lens, doff):
        img[do:do + ln] = buf[so:so + ln]
    assert np.array_equal(d_buf.cpu().numpy(), img)


def test_bounds_are_enforced_on_the_device(cuda):
    import torch
    rng = np.random.default_rng(8)
    n = 300
    src = rng.integers(0, 256, size=1 << 16, dtype=np.uint8)
    lens = rng.integers(1, 200, size=n).astype(np.uint32)
    soff = (rng.random(n) * 30000).astype(np.int64)
    doff = 2 + np.concatenate([[0], np.cumsum(lens + 2)[:-1]]).astype(np.int64)
    # the declared sizes are smaller than the tensors: a broken check stays inside them
    src_bytes, dst_bytes = 32768, 40000
    assert doff[-1] + lens[-1] < dst_bytes
    soff[41], lens[41] = src_bytes - 10, 11          # one byte past the declared source
    doff[97] = dst_bytes - int(lens[97]) + 1          # one byte past the declared destination
    soff[250] = (1 << 63) - 8                         # far outside; the sum needs 64 bits
    refused = (41, 97, 250)
    d_src = torch.from_numpy(src).to(cuda)
    d_dst = torch.full((1 << 16,), FILL, dtype=torch.uint8, device=cuda)
    out = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=cuda)
    stream = torch.cuda.current_stream(cuda)
    args = (d_src.data_ptr(), src_bytes, _i64(soff).to(cuda), _i32(lens).to(cuda),
            d_dst.data_ptr(), dst_bytes, _i64(doff).to(cuda))

    def call(flags):
        o = N.make_opts(device=cuda.index, stream=stream.cuda_stream, flags=flags)
        return N.lib.bmqcrc_crc32c_copy(args[0], args[1], args[2].data_ptr(), args[3].data_ptr(),
                                        args[4], args[5], args[6].data_ptr(), None,
                                        out.data_ptr(), n, ctypes.byref(o))

    rc = call(N.BMQCRC_F_DEVICE_PTRS)
    err = N.lib.bmqcrc_last_error()
    assert rc == N.BMQCRC_EINVAL and b"message 41 " in err, (rc, err)
    assert last_copy(cuda.index, stream) == (n, 3, 41)
    got = out.cpu().numpy().view(np.uint32)
    ok = np.array([i not in refused for i in range(n)])
    exp = oracle.batch(src, np.where(ok, soff, 0), np.where(ok, lens, 0))
    assert np.array_equal(got[ok], exp[ok])
    assert all(got[i] == 0x5A5A5A5A for i in refused)  # left unwritten
    img = _image(src, soff, lens, doff, 1 << 16, skip=refused)
    assert np.array_equal(d_dst.cpu().numpy(), img)    # refused destinations still 0xA5
    # asynchronous: the call returns 0 and last_copy reports
    assert call(N.BMQCRC_F_DEVICE_PTRS | N.BMQCRC_F_ASYNC) == 0
    assert last_copy(cuda.index, stream) == (n, 3, 41)
    # the Python wrapper raises for the synchronous form
    with pytest.raises(BmqCrcError) as e:
        Crc32c.copy_batch(d_src[:src_bytes], args[2], args[3], d_dst[:dst_bytes], args[6])
    assert e.value.rc == N.BMQCRC_EINVAL and "message 41 " in str(e.value)
    # a clean call clears the report
    Crc32c.copy_batch(d_src, args[2][:40], args[3][:40], d_dst, args[6][:40])
    assert last_copy(cuda.index, stream) == (40, 0, 40)


def test_prediction_untouched(cuda):
    import torch
    rng = np.random.default_rng(9)
    host = rng.integers(0, 256, size=1 << 20, dtype=np.uint8)
    arena = torch.from_numpy(host).to(cuda)
    lens = rng.integers(1, 1025, size=5001).astype(np.uint32)
    dst = torch.zeros(int(lens.sum()) + 16, dtype=torch.uint8, device=cuda)
    offs = (rng.random(lens.size) * (host.size - 1100)).astype(np.int64)
    d_off, d_len = _i64(offs).to(cuda), _i32(lens).to(cuda)
    doff = _i64(np.concatenate([[0], np.cumsum(lens)[:-1]])).to(cuda)
    plans = []
    for with_copy in (False, True):
        s = torch.cuda.Stream(cuda)
        with torch.cuda.stream(s):
            Crc32c.calculate_batch(arena, d_off, d_len, stream=s, seg_bytes=1024)
            before = last_launch(cuda.index, s, offsets=True)
            if with_copy:
                Crc32c.copy_batch(arena, d_off, d_len, dst, doff, stream=s)
                assert last_launch(cuda.index, s, offsets=True) == before
            out = Crc32c.calculate_batch(arena, d_off, d_len, stream=s, seg_bytes=1024)
            plans.append(last_launch(cuda.index, s, offsets=True))
        s.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), oracle.batch(host, offs, lens))
    assert plans[0] == plans[1], plans


def test_golden_vectors(cuda, golden):
    # the reference's vectors: plain ones with seed 0, chained ones as
    # crc(suffix, seed = crc(prefix))
    datas, seeds, crcs = [], [], []
    for v in golden["calculate"] + golden["rfc3720"]:
        datas.append(bytes.fromhex(v["hex"]))
        seeds.append(0)
        crcs.append(v["crc"])
    for v in golden["chained"]:
        b, p = bytes.fromhex(v["hex"]), v["prefix_len"]
        datas.append(b[p:])
        seeds.append(oracle.crc32c(b[:p]))
        crcs.append(v["crc"])
    lens = np.array([len(d) for d in datas], np.uint32)
    soff = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    src = np.frombuffer(b"".join(datas) + bytes(16), dtype=np.uint8).copy()
    doff = 9 + np.concatenate([[0], np.cumsum(lens + 5)[:-1]]).astype(np.int64)
    got, _ = _check(cuda, src, soff, lens, doff, int(doff[-1] + lens[-1]) + 16,
                    np.array(seeds, np.uint32))
    assert [int(g) for g in got] == crcs


def _packed(rng, lens, dmis):
    lens = np.asarray(lens, np.int64)
    src = rng.integers(0, 256, size=int(lens.sum()) + 64, dtype=np.uint8)
    soff = 5 + np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    doff = dmis + np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    return src, soff, doff, int(doff[-1] + lens[-1]) + 32


@pytest.mark.parametrize("lens,dmis", [
    ([5000, 20], 0), ([C + 700, 40, 9], 0), ([3000, 1, 1], 3), ([40, 2100, 500, 30], 7),
    ([5000], 0), ([C + 1200, 0, 17], 11), ([2 * C + 17, 300, 2], 5)])
def test_batch_ends_in_a_partial_row_after_a_long_message(cuda, lens, dmis):
    # the last row is partial and the lanes past it still hold the row before:
    # the long message is held by two separate runs of lanes at the last flush
    rng = np.random.default_rng(31)
    src, soff, doff, size = _packed(rng, lens, dmis)
    _check(cuda, src, soff, lens, doff, size, _seeds(rng, len(lens)))


def test_random_short_batches_ending_anywhere(cuda):
    # 1-5 packed messages below 3,000 bytes, every way a batch can end
    rng = np.random.default_rng(32)
    for _ in range(60):
        lens = rng.integers(0, 3000, size=int(rng.integers(1, 6)))
        src, soff, doff, size = _packed(rng, lens, int(rng.integers(0, 16)))
        _check(cuda, src, soff, lens, doff, size, _seeds(rng, lens.size))


def test_long_runs_of_empty_messages(cuda):
    rng = np.random.default_rng(33)
    lens = np.array([100] + [0] * 5000 + [33, 700] + [0] * 777 + [5] + [0] * 300, np.int64)
    src = rng.integers(0, 256, size=4096, dtype=np.uint8)
    soff = (rng.random(lens.size) * 3000).astype(np.int64)
    doff = 9 + np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    seeds = _seeds(rng, lens.size)
    got, _ = _check(cuda, src, soff, lens, doff, int(doff[-1] + lens[-1]) + 16, seeds)
    assert np.array_equal(got[lens == 0], seeds[lens == 0])


def _two_tiles_per_block():
    # N_TILES messages of 0..300 bytes with runs of 600 empties (one across a
    # tile's end, one across a block's, one at the batch's end); sources at
    # index mod 16; a third of the destinations end to end with their
    # predecessor (neighbours share 16-byte pieces), the others at the next
    # offset with the misalignment a permutation gives them
    rng = np.random.default_rng(34)
    n = G.N_TILES
    lens = rng.integers(0, 301, size=n)
    for at in (700, 2048 - 300, 100 * 2048 + 1024 - 300, n - 600):
        lens[at:at + 600] = 0
    smis = np.arange(n) % 16
    dmis = rng.permutation(n) % 16
    packed = rng.random(n) < 1 / 3
    soff, doff, s, d = np.zeros(n, np.int64), np.zeros(n, np.int64), 0, 7
    for i, ln in enumerate(lens.tolist()):
        s = (s + 15) // 16 * 16 + int(smis[i])
        if not packed[i]:
            d += (int(dmis[i]) - d) % 16
        soff[i], doff[i] = s, d
        s += ln
        d += ln
    src = rng.integers(0, 256, size=s + 16, dtype=np.uint8)
    return src, soff, lens, doff, d + 16, _seeds(rng, n)


def test_two_tiles_per_block_called_directly(cuda):
    """256 * 1,024 + 1,025 messages: the copy's own count and scan kernels run
    two tiles per block (layout_split gives 129 blocks of 2,048), which the
    suite reached through the packers only."""
    import torch
    assert G.regime(G.N_TILES)[:2] == (129, 2048)
    src, soff, lens, doff, size, seeds = _two_tiles_per_block()
    assert set((doff % 16).tolist()) == set(range(16)) and int((lens == 0).sum()) > 2400
    _check(cuda, src, soff, lens, doff, size, seeds)
    assert last_copy(cuda.index, torch.cuda.current_stream(cuda)) == (G.N_TILES, 0, G.N_TILES)
