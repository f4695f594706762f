"""Device-side PUT-event packer (bmqcrc_put_event_pack, ABI 2.10) on the GPU.
The oracle throughout is the concatenated PutEventBuilder(defer_crc=False)
bytes plus host CRCs: every check compares the packed bytes byte for byte,
`out`, `event_offsets`, and the canary behind the total."""
import ctypes
import functools

import numpy as np
import pytest

from blazingmq_amd import (BmqCrcError, Crc32c, _native as N, last_copy, last_launch,
                           last_put_pack, pack_events)
import device_views as V
import pack_pool
import test_grid_regimes as G
from put_pack_model import (EVT, HDR, host_crcs, layout, model_bytes, model_bytes_fast,
                            oracle_events, pad_of, pool_crcs, pooled_crcs, random_meta)

pytestmark = pytest.mark.gpu

FILL = 0xA5
FILL32 = 0x5A5A5A5A
FILL64 = 0x5A5A5A5A5A5A5A5A
CAP = 66 << 20


def _t(cuda, a, dtype, place=None, name=None):
    """`a` on the device at the start of an allocation, or with `place` (a
    device_views.Placer) inside one, at the phase the placer has for `name`."""
    import torch
    a = np.ascontiguousarray(a, dtype=dtype)
    if place is not None:
        return place.put(name, a)
    if dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(cuda)


def _inputs(cuda, src, soff, lens, qids, guids, flags, ef, place=None):
    t = lambda name, a, dtype: _t(cuda, a, dtype, place, name)
    return dict(src=t("src", src, np.uint8), src_offsets=t("src_offsets", soff, np.int64),
                lengths=t("lengths", lens, np.uint32), queue_ids=t("queue_ids", qids, np.int32),
                guids=t("guids", guids, np.uint8),
                flags=t("flags", flags, np.uint8) if flags is not None else None,
                event_first=t("event_first", ef, np.int64) if ef is not None else None)


def _check_placed(cuda, place, src, soff, lens, qids, guids, flags, ef, slack, max_event_bytes=0):
    """_check's call and checks through the raw call, every buffer placed."""
    exp = np.concatenate(oracle_events(src, soff, lens, qids, guids, flags, ef))
    total, n, n_events = exp.size, len(lens), 1 if ef is None else len(ef) - 1
    d = _inputs(cuda, src, soff, lens, qids, guids, flags, ef, place)
    dst = place.fill("dst", total + slack, np.uint8, FILL)
    out = place.fill("out", n, np.uint32, FILL32)
    evoff = place.fill("event_offsets", n_events + 1, np.uint64, FILL64)
    rc, err, got_total = _raw(cuda, d, n, n_events, dst, total + slack, out, evoff,
                              max_event_bytes=max_event_bytes)
    assert rc == 0 and got_total == total, (rc, err, got_total)
    import torch
    assert last_put_pack(cuda.index, torch.cuda.current_stream(cuda)) == (
        n, n_events, total, N.BMQCRC_PUT_PACK_OK, 0)
    host = dst.cpu().numpy()
    diff = np.nonzero(host[:total] != exp)[0]
    assert diff.size == 0, (diff.size, [int(i) for i in diff[:8]])
    assert np.all(host[total:] == FILL)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), host_crcs(src, soff, lens))
    assert np.array_equal(evoff.cpu().numpy(), layout(lens, ef)[1])
    assert np.array_equal(d["src"].cpu().numpy(), src)  # the source is only read
    place.check()
    return host[:total]


def _check(cuda, src, soff, lens, qids, guids, flags=None, ef=None, slack=64, phases=None,
           model=None, inputs=None, **kw):
    """One pack into a canary destination against the oracle.  Returns the
    packed bytes (host).  `phases` maps every pointer of the call (src,
    src_offsets, lengths, queue_ids, guids, flags, event_first, dst,
    event_offsets, out) to the phase of its base: the call then goes through
    the raw entry point and the sentinel margins around every buffer are
    checked; None: the wrapper, every buffer at the start of an allocation.
    `model` is (expected bytes, event offsets, CRCs) of this very call when the
    caller has them already: the oracle and the host CRCs are not run then.
    `inputs` is _inputs' answer for these arguments, already on the device."""
    import torch
    if phases is not None:
        return _check_placed(cuda, V.Placer(cuda, phases), src, soff, lens, qids, guids, flags, ef,
                             slack, **kw)
    # (n = 0 writes nothing, not even an empty event)
    if model is not None:
        exp, want_ev, want_crcs = model
    else:
        exp = np.concatenate(oracle_events(src, soff, lens, qids, guids, flags, ef)) \
            if len(lens) else np.zeros(0, np.uint8)
        want_ev, want_crcs = layout(lens, ef)[1], host_crcs(src, soff, lens)
    total = exp.size
    d = inputs if inputs is not None else _inputs(cuda, src, soff, lens, qids, guids, flags, ef)
    dst = torch.full((total + slack,), FILL, dtype=torch.uint8, device=cuda)
    out = torch.full((len(lens),), FILL32, dtype=torch.int32, device=cuda)
    rdst, evoff, rout = pack_events(dst=dst, out=out, **d, **kw)
    assert rdst is dst and rout is out
    stream = torch.cuda.current_stream(cuda)
    n_events = 1 if ef is None else len(ef) - 1
    assert last_put_pack(cuda.index, stream) == (len(lens), n_events if len(lens) else 0, total,
                                                 N.BMQCRC_PUT_PACK_OK, 0)
    host = dst.cpu().numpy()
    diff = np.nonzero(host[:total] != exp)[0]
    assert diff.size == 0, (diff.size, [int(i) for i in diff[:8]])
    assert np.all(host[total:] == FILL)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want_crcs)
    if len(lens):
        assert np.array_equal(evoff.cpu().numpy(), want_ev)
    assert np.array_equal(d["src"].cpu().numpy(), src)  # the source is only read
    return host[:total]


def _raw(cuda, d, n, n_events, dst, dst_bytes, out, evoff, flags=N.BMQCRC_F_DEVICE_PTRS,
         max_event_bytes=0, src_bytes=None):
    import torch
    p = N.PutPack()
    p.struct_size = ctypes.sizeof(N.PutPack)
    p.src = d["src"].data_ptr()
    p.src_bytes = d["src"].numel() if src_bytes is None else src_bytes
    p.src_offsets, p.lengths = d["src_offsets"].data_ptr(), d["lengths"].data_ptr()
    p.queue_ids, p.guids = d["queue_ids"].data_ptr(), d["guids"].data_ptr()
    p.flags = d["flags"].data_ptr() if d["flags"] is not None else None
    p.event_first = d["event_first"].data_ptr() if d["event_first"] is not None else None
    p.n, p.n_events, p.max_event_bytes = n, n_events, max_event_bytes
    p.dst, p.dst_bytes = dst.data_ptr(), dst_bytes
    p.event_offsets, p.out = evoff.data_ptr(), out.data_ptr()
    stream = torch.cuda.current_stream(cuda)
    o = N.make_opts(device=cuda.index, stream=stream.cuda_stream, flags=flags)
    total = ctypes.c_uint64(FILL64)
    rc = N.lib.bmqcrc_put_event_pack(ctypes.byref(p), ctypes.byref(total), ctypes.byref(o))
    return rc, N.lib.bmqcrc_last_error(), total.value


def _refused(cuda, kind, index, src, soff, lens, qids, guids, flags=None, ef=None,
             dst_bytes=None, phases=None, size=None, inputs=None, **kw):
    """The call is refused with (kind, index), synchronously and asynchronously,
    and the whole dst, out and event_offsets keep their canaries.  `phases`:
    as in _check.  `size` is the destination's, when the caller has the layout
    already (no less than every event of these lengths takes); `inputs` is
    _inputs' answer for these arguments, already on the device."""
    import torch
    n, n_events = len(lens), 1 if ef is None else len(ef) - 1
    place = V.Placer(cuda, phases) if phases is not None else None
    d = inputs if inputs is not None else \
        _inputs(cuda, src, soff, lens, qids, guids, flags, ef, place)
    if size is None:
        size = int(layout(lens, None)[1][-1]) + 8 * n_events + 64
    stream = torch.cuda.current_stream(cuda)
    name = {1: b"SRC_RANGE", 2: b"EVENT_FIRST", 3: b"EVENT_TOO_BIG", 4: b"DST_TOO_SMALL"}[kind]
    for flags_ in (N.BMQCRC_F_DEVICE_PTRS, N.BMQCRC_F_DEVICE_PTRS | N.BMQCRC_F_ASYNC):
        if place is not None:
            dst = place.fill("dst", size, np.uint8, FILL)
            out = place.fill("out", n, np.uint32, FILL32)
            evoff = place.fill("event_offsets", n_events + 1, np.uint64, FILL64)
        else:
            dst = torch.full((size,), FILL, dtype=torch.uint8, device=cuda)
            out = torch.full((n,), FILL32, dtype=torch.int32, device=cuda)
            evoff = torch.full((n_events + 1,), FILL64, dtype=torch.int64, device=cuda)
        rc, err, total = _raw(cuda, d, n, n_events, dst, size if dst_bytes is None else dst_bytes,
                              out, evoff, flags_, **kw)
        if flags_ & N.BMQCRC_F_ASYNC:
            assert rc == 0 and total == FILL64, (rc, err)
        else:
            assert rc == N.BMQCRC_EINVAL and name in err and total == 0, (rc, err)
            assert (" %d " % index).encode() in err or ("[%d]" % index).encode() in err, err
        assert last_put_pack(cuda.index, stream) == (n, n_events, 0, kind, index)
        assert bool((dst == FILL).all()) and bool((out == FILL32).all())
        assert bool((evoff == FILL64).all())
        if place is not None:
            place.check()


def _short(rng, n, lo=1, hi=41, src_size=1 << 16):
    src = rng.integers(0, 256, size=src_size, dtype=np.uint8)
    lens = rng.integers(lo, hi, size=n)
    soff = rng.integers(0, src_size - hi, size=n)
    return (src, soff, lens) + random_meta(rng, n)


def test_every_length_at_every_source_misalignment(cuda):
    # lengths 0..67 in one event: every padding count, and (the 36-byte header
    # shifts a payload by 4 mod 16 per message) every destination alignment
    rng = np.random.default_rng(1)
    lens = np.arange(68)
    src = rng.integers(0, 256, size=68 * 96 + 64, dtype=np.uint8)
    for mis in range(16):
        soff = 96 * np.arange(68) + mis + 16 * rng.integers(0, 2, size=68)
        assert np.all(soff % 16 == mis)
        qids, guids, flags = random_meta(rng, 68)
        _check(cuda, src, soff, rng.permutation(lens), qids, guids, flags)
    assert set((36 + layout(lens)[0]) % 16) == {0, 4, 8, 12}


def test_smallest_cases(cuda):
    rng = np.random.default_rng(2)
    src = rng.integers(0, 256, size=256, dtype=np.uint8)
    for ln in (0, 1):
        qids, guids, flags = random_meta(rng, 1)
        got = _check(cuda, src, [7], [ln], qids, guids, flags)
        assert got.size == 8 + 36 + 4 and list(got[44 + ln:]) == [4 - ln] * (4 - ln)
    # flags=None is zero flags; event_first given for one event
    qids, guids, _ = random_meta(rng, 1)
    _check(cuda, src, [3], [5], qids, guids, None, [0, 1])
    # n = 0: nothing is written
    got = _check(cuda, src, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int32),
                 np.zeros((0, 16), np.uint8))
    assert got.size == 0


def test_wrapper_allocates_the_exact_destination(cuda):
    rng = np.random.default_rng(3)
    src, soff, lens, qids, guids, flags = _short(rng, 77, 0, 30)
    ef = [0, 10, 77]
    d = _inputs(cuda, src, soff, lens, qids, guids, flags, ef)
    dst, evoff, out = pack_events(**d)
    exp = np.concatenate(oracle_events(src, soff, lens, qids, guids, flags, ef))
    assert dst.numel() == exp.size and np.array_equal(dst.cpu().numpy(), exp)
    assert int(evoff[-1]) == exp.size
    with pytest.raises(ValueError, match="dst is required"):
        pack_events(sync=False, **d)


@pytest.mark.parametrize("n", [1025, 3 * 1024 + 1])
def test_more_than_one_layout_block(cuda, n):
    rng = np.random.default_rng(4)
    case = _short(rng, n)
    ef = sorted(set([0, 1, 1024, 1025, n]))
    assert [b - a for a, b in zip(ef, ef[1:])].count(1) >= 2  # single-message events
    _check(cuda, *case, ef=ef)
    _check(cuda, *case)  # and as one event


@pytest.mark.parametrize("own_event", [False, True])
def test_a_long_message_among_short_ones(cuda, own_event):
    rng = np.random.default_rng(5)
    src, soff, lens, qids, guids, flags = _short(rng, 41, 0, 200, src_size=1 << 19)
    lens[20], soff[20] = 300000, 13  # longer than a 64 KiB chunk of the copy pass
    ef = [0, 20, 21, 41] if own_event else None
    first = _check(cuda, src, soff, lens, qids, guids, flags, ef)
    again = _check(cuda, src, soff, lens, qids, guids, flags, ef)
    assert np.array_equal(first, again)


def _cap_case(rng, last_len):
    # event 1 = 40 messages of 100 framed bytes and one of 36 + last_len + pad
    lens = np.array([5, 6] + [60] * 40 + [last_len])
    src = rng.integers(0, 256, size=4096, dtype=np.uint8)
    soff = rng.integers(0, 4000, size=lens.size)
    return (src, soff, lens) + random_meta(rng, lens.size), [0, 2, lens.size]


def test_event_size_cap(cuda):
    rng = np.random.default_rng(6)
    case, ef = _cap_case(rng, 48)
    assert np.diff(layout(case[2], ef)[1])[1] == 4096
    _check(cuda, *case, ef=ef, max_event_bytes=4096)          # exactly at the cap
    case, ef = _cap_case(rng, 52)
    assert np.diff(layout(case[2], ef)[1])[1] == 4100          # one word over
    _refused(cuda, N.BMQCRC_PUT_PACK_EVENT_TOO_BIG, 1, *case, ef=ef, max_event_bytes=4096)
    _check(cuda, *case, ef=ef, max_event_bytes=4100)
    with pytest.raises(BmqCrcError, match="EVENT_TOO_BIG: event 1 "):
        pack_events(**_inputs(cuda, *case, ef), max_event_bytes=4096)


def test_destination_size(cuda):
    rng = np.random.default_rng(7)
    case = _short(rng, 300)
    ef = [0, 100, 299, 300]
    total = int(layout(case[2], ef)[1][-1])
    _check(cuda, *case, ef=ef, slack=0)                        # dst_bytes == total
    _refused(cuda, N.BMQCRC_PUT_PACK_DST_TOO_SMALL, 2, *case, ef=ef, dst_bytes=total - 4)
    _refused(cuda, N.BMQCRC_PUT_PACK_DST_TOO_SMALL, 0, *case, ef=ef, dst_bytes=64)


def test_source_range(cuda):
    rng = np.random.default_rng(8)
    src, soff, lens, qids, guids, flags = _short(rng, 1500, src_size=1 << 15)
    src_bytes = 20000  # declared smaller than the tensor: a broken check stays inside it
    soff = soff % (src_bytes - 64)
    soff[1200], lens[1200] = src_bytes - 10, 11               # one byte past
    soff[1300] = (1 << 63) - 8                                 # the sum needs 64 bits
    soff[77], lens[77] = src_bytes, 0                          # empty at the very end: legal
    _refused(cuda, N.BMQCRC_PUT_PACK_SRC_RANGE, 1200, src, soff, lens, qids, guids, flags,
             src_bytes=src_bytes)


@pytest.mark.parametrize("ef,index", [
    ([1, 5, 20], 0),        # not starting at 0
    ([0, 5, 5, 20], 1),     # not increasing
    ([0, 9, 5, 20], 1),     # decreasing
    ([0, 5, 19], 2),        # not ending at n
    ([0, 5, 21], 2)])       # ending past n
def test_bad_event_first(cuda, ef, index):
    rng = np.random.default_rng(9)
    _refused(cuda, N.BMQCRC_PUT_PACK_EVENT_FIRST, index, *_short(rng, 20), ef=ef)


def test_asynchronous_call(cuda):
    import torch
    rng = np.random.default_rng(10)
    src, soff, lens, qids, guids, flags = _short(rng, 2000, 0, 300)
    ef = [0, 500, 2000]
    got = _check(cuda, src, soff, lens, qids, guids, flags, ef, sync=False)
    s = torch.cuda.Stream(cuda)
    with torch.cuda.stream(s):
        again = _check(cuda, src, soff, lens, qids, guids, flags, ef, sync=False, stream=s)
    assert np.array_equal(got, again)


def test_state_untouched(cuda):
    import torch
    rng = np.random.default_rng(11)
    host = rng.integers(0, 256, size=1 << 20, dtype=np.uint8)
    arena = torch.from_numpy(host).to(cuda)
    lens = rng.integers(1, 1025, size=5001).astype(np.uint32)
    offs = (rng.random(lens.size) * (host.size - 1100)).astype(np.int64)
    d_off, d_len = _t(cuda, offs, np.int64), _t(cuda, lens, np.uint32)
    copy_dst = torch.zeros(int(lens.sum()) + 16, dtype=torch.uint8, device=cuda)
    doff = _t(cuda, np.concatenate([[0], np.cumsum(lens)[:-1]]), np.int64)
    qids, guids, flags = random_meta(rng, lens.size)
    pack = _inputs(cuda, host, offs, lens, qids, guids, flags, None)
    pack["src"] = arena
    plans = []
    for with_pack in (False, True):
        s = torch.cuda.Stream(cuda)
        with torch.cuda.stream(s):
            Crc32c.copy_batch(arena, d_off[:40], d_len[:40], copy_dst, doff[:40], stream=s)
            Crc32c.calculate_batch(arena, d_off, d_len, stream=s, seg_bytes=1024)
            before = last_launch(cuda.index, s, offsets=True)
            assert last_copy(cuda.index, s) == (40, 0, 40)
            if with_pack:
                pack_events(stream=s, **pack)
                pack_events(stream=s, sync=False, dst=torch.zeros(64, dtype=torch.uint8,
                                                                  device=cuda), **pack)
                assert last_put_pack(cuda.index, s)[3] == N.BMQCRC_PUT_PACK_DST_TOO_SMALL
                assert last_launch(cuda.index, s, offsets=True) == before
                assert last_copy(cuda.index, s) == (40, 0, 40)
            out = Crc32c.calculate_batch(arena, d_off, d_len, stream=s, seg_bytes=1024)
            plans.append(last_launch(cuda.index, s, offsets=True))
        s.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32),
                              host_crcs(host, offs, lens))
    assert plans[0] == plans[1], plans


def test_a_layout_block_of_two_tiles(cuda):
    # 258 tiles of 1,024 messages for at most 256 blocks: per_block is 2,048
    # and each of the 129 blocks scans two tiles, the second on top of the
    # first's carry -- the smallest n at which a block loops.  Events meet the
    # first block seam from both sides; lengths 0..7 keep it at some 11 MB.
    import torch
    rng = np.random.default_rng(13)
    n = 256 * 1024 + 1025
    src, soff, lens, qids, guids, flags = _short(rng, n, 0, 8)
    ef = [0, 2047, 2048, 2049, n - 1, n]
    ev = layout(lens, ef)[1]
    total = int(ev[-1])
    assert int(np.diff(ev).max()) <= CAP  # the long event fits the cap given below
    d = _inputs(cuda, src, soff, lens, qids, guids, flags, ef)
    dst = torch.full((total + 64,), FILL, dtype=torch.uint8, device=cuda)
    out = torch.full((n,), FILL32, dtype=torch.int32, device=cuda)
    _, evoff, _ = pack_events(dst=dst, out=out, max_event_bytes=CAP, **d)
    assert last_put_pack(cuda.index, torch.cuda.current_stream(cuda)) == (n, 5, total, 0, 0)
    assert np.array_equal(evoff.cpu().numpy(), ev)
    crcs = host_crcs(src, soff, lens)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), crcs)
    host = dst.cpu().numpy()
    assert np.all(host[total:] == FILL)
    # every byte against the numpy model, which test_put_pack_model.py holds to
    # PutEventBuilder; the four short events against PutEventBuilder itself
    diff = np.nonzero(host[:total] != model_bytes(src, soff, lens, qids, guids, flags, ef, crcs))[0]
    assert diff.size == 0, (diff.size, [int(i) for i in diff[:8]])
    short = [0, 1, 2, 4]
    for e, exp in zip(short, oracle_events(src, soff, lens, qids, guids, flags, ef, events=short)):
        assert np.array_equal(host[int(ev[e]):int(ev[e + 1])], exp), e
    # the same inputs with message 2048, the first of the second block, out of range
    soff[2048] = src.size - int(lens[2048]) + 1
    _refused(cuda, N.BMQCRC_PUT_PACK_SRC_RANGE, 2048, src, soff, lens, qids, guids, flags, ef)


def test_crossing_4_gib(cuda):
    # 70 events of 66 messages of 2^20 - 4 framed bytes: 8 bytes under the
    # 66 MiB cap each, 4.5 GiB in all -- what a 32-bit prefix gets wrong.
    # Every payload lies in one 1 MiB source region (source ranges overlap).
    import torch
    rng = np.random.default_rng(12)
    per, n_events, ln = 66, 70, (1 << 20) - 44
    n = per * n_events
    src = rng.integers(0, 256, size=1 << 20, dtype=np.uint8)
    soff = 4 * (np.arange(n) % 11)
    lens = np.full(n, ln)
    qids, guids, flags = random_meta(rng, n)
    ef = per * np.arange(n_events + 1)
    hdr, ev = layout(lens, ef)
    total = int(ev[-1])
    assert total > (1 << 32) + (1 << 28) and int(np.diff(ev).max()) == CAP - 256 <= CAP
    dst = torch.empty(total + 64, dtype=torch.uint8, device=cuda)
    dst[total:] = FILL
    d = _inputs(cuda, src, soff, lens, qids, guids, flags, ef)
    _, evoff, out = pack_events(dst=dst, **d)
    assert np.array_equal(evoff.cpu().numpy(), ev)
    assert last_put_pack(cuda.index, torch.cuda.current_stream(cuda)) == (n, n_events, total, 0, 0)
    first, last = oracle_events(src, soff, lens, qids, guids, flags, ef, events=[0, n_events - 1])
    assert torch.equal(dst[:first.size].cpu(), torch.from_numpy(first))
    assert torch.equal(dst[int(ev[-2]):total].cpu(), torch.from_numpy(last))
    assert bool((dst[total:] == FILL).all())
    crc11 = host_crcs(src, soff[:11], lens[:11])
    assert np.array_equal(out.cpu().numpy().view(np.uint32), crc11[np.arange(n) % 11])


# ---- past one tile per block (DESIGN.md sections 12 and 20) -------------------
#
# One set of N_FRAME messages (pack_pool.py: variable lengths, every padding
# count and an empty message in every tile, one message of 70,000 bytes every
# 3,001), built once; the smaller sizes are its prefixes.  The expected bytes
# come from model_bytes_fast, which test_put_pack_model.py holds to the loop
# model and to PutEventBuilder, once per (size, events).  The caches below live
# as long as the session, as test_gpu_rollover.py's do: some 150 MB on the host
# (the inputs and five images of 6 to 48 MB) and 25 MB on the device.

@functools.lru_cache(maxsize=None)
def _large():
    """((src, soff, lens, qids, guids, flags) of N_FRAME messages, their CRCs
    from one CRC per pool pair).  Shared, never modified."""
    src, soff, lens, ix = pack_pool.messages(G.N_FRAME)
    case = (src, soff, lens) + random_meta(np.random.default_rng(21), G.N_FRAME)
    crcs = pooled_crcs(pool_crcs(*pack_pool.pool()), ix)
    for a in case + (crcs,):
        a.setflags(write=False)
    return case, crcs


@functools.lru_cache(maxsize=None)
def _large_dev(cuda):
    return _inputs(cuda, *(np.array(a) for a in _large()[0]), None)


def _events_of(n, per):
    return None if per is None else np.append(np.arange(0, n, per), n)


def _first(cuda, n, ef=None):
    """(the first n messages on the host, the same on the device with `ef`)."""
    case = _large()[0]
    dev = {k: v if k == "src" else v[:n] for k, v in _large_dev(cuda).items()
           if k != "event_first"}
    dev["event_first"] = _t(cuda, ef, np.int64) if ef is not None else None
    return (case[0],) + tuple(a[:n] for a in case[1:]), dev


def _patched(dev, **changes):
    """`dev` with clones of the named tensors, entry i set to v for every
    (i, v) of the name's dict."""
    out = dict(dev)
    for name, entries in changes.items():
        out[name] = dev[name].clone()
        for i, v in entries.items():
            out[name][i] = v
    return out


@functools.lru_cache(maxsize=None)
def _expected(n, per):
    """(expected bytes, event offsets, CRCs) of the first n messages in events
    of `per` messages (None: one event)."""
    case, crcs = _large()
    host = (case[0],) + tuple(a[:n] for a in case[1:])
    ef = _events_of(n, per)
    img = model_bytes_fast(*host, ef, crcs[:n])
    ev = layout(host[2], ef)[1]
    # the framed totals are the model's
    assert img.size == int(ev[-1]) == EVT * (ev.size - 1) + int(
        (HDR + host[2] + pad_of(host[2])).sum())
    return img, ev, crcs[:n]


@functools.lru_cache(maxsize=None)
def _event_offsets(n, per):
    return layout(_large()[0][2][:n], _events_of(n, per))[1]


LARGE = [(G.N_WAVES, 3), (G.N_FULL, None), (G.N_TILES, 3), (G.N_TILES, 1), (G.N_FRAME, 1)]
LARGE_IDS = ["N_WAVES-events_of_3", "N_FULL-one_event", "N_TILES-events_of_3",
             "N_TILES-own_events", "N_FRAME-own_events"]


@pytest.mark.parametrize("n,per", LARGE, ids=LARGE_IDS)
def test_past_one_tile_per_block(cuda, n, per):
    # N_WAVES: 66 blocks, some 342 events a block, two of three block seams
    # inside an event.  N_FULL: all 256 blocks under one event.  N_TILES: two
    # tiles a block; with an event per message a block spans 2,048 events and
    # seal_offsets searches event_first in global memory, not in LDS.  N_FRAME:
    # three steps of the shape check and of events_check, two of
    # event_headers, and k_pack_frame's per-message regime.
    model = _expected(n, per)
    assert int(np.diff(model[1]).max()) <= CAP
    ef = _events_of(n, per)
    host, dev = _first(cuda, n, ef)
    _check(cuda, *host, ef=ef, model=model, inputs=dev)


def test_past_one_tile_per_block_on_a_side_stream(cuda):
    import torch
    n = G.N_TILES
    ef = _events_of(n, 3)
    host, dev = _first(cuda, n, ef)
    torch.cuda.synchronize(cuda)
    s = torch.cuda.Stream(cuda, priority=-1)
    with torch.cuda.stream(s):
        _check(cuda, *host, ef=ef, model=_expected(n, 3), inputs=dev, sync=False, stream=s)


def test_event_first_refused_in_a_late_step_of_the_shape_loop(cuda):
    # one event per message at N_FRAME: 175,104 threads over 524,290 entries
    n = G.N_FRAME
    threads = G.regime(n).nblocks * 1024
    assert 2 * threads < n < 3 * threads
    good = _events_of(n, 1)
    size = int(_event_offsets(n, 1)[-1]) + 64
    host, dev = _first(cuda, n)

    def refused(index, entries):
        ef = good.copy()
        for e, v in entries.items():
            ef[e] = v
        _refused(cuda, N.BMQCRC_PUT_PACK_EVENT_FIRST, index, *host, ef=ef, size=size,
                 inputs=dict(dev, event_first=_t(cuda, ef, np.int64)))

    late = 2 * threads + 50000          # read in the third step alone
    refused(late, {late: late + 1})     # equal to the next entry
    refused(n, {n: n + 1})              # the last entry is not n
    # a high entry of an early thread's third step, a lower one of a later
    # thread's second step: the lower index
    high, low = 2 * threads + 10, threads + 170000
    refused(low, {high: high + 1, low: low + 1})
    assert np.array_equal(dev["src"].cpu().numpy(), host[0])


def test_source_range_refused_past_one_tile_per_block(cuda):
    n = G.N_TILES
    per_block = G.regime(n).per_block
    ef = _events_of(n, 3)
    size = int(_event_offsets(n, 3)[-1]) + 64
    host, dev = _first(cuda, n, ef)
    declared = pack_pool.SRC_BYTES  # smaller than the tensor: a broken check stays inside it
    assert host[0].size >= declared + 64

    def refused(kind, index, at, inputs=dev):
        bad = _patched(inputs, src_offsets={i: declared - 10 for i in at},
                       lengths={i: 11 for i in at})   # one byte past
        _refused(cuda, kind, index, *host, ef=ef, size=size, inputs=bad, src_bytes=declared)

    # in the second tile of block 0, below one in block 1
    assert 1024 <= 1030 < per_block <= 2100
    refused(N.BMQCRC_PUT_PACK_SRC_RANGE, 1030, (1030, 2100))
    # the last message of the last block
    refused(N.BMQCRC_PUT_PACK_SRC_RANGE, n - 1, (n - 1,))
    # with a bad event_first entry at a lower index: kind 1 wins over kind 2
    bad_ef = ef.copy()
    bad_ef[7] = bad_ef[8]
    refused(N.BMQCRC_PUT_PACK_SRC_RANGE, 150000, (150000,),
            dict(dev, event_first=_t(cuda, bad_ef, np.int64)))
    _refused(cuda, N.BMQCRC_PUT_PACK_EVENT_FIRST, 7, *host, ef=bad_ef, size=size,
             inputs=dict(dev, event_first=_t(cuda, bad_ef, np.int64)))
    assert np.array_equal(dev["src"].cpu().numpy(), host[0])


def test_event_size_cap_past_one_tile_per_block(cuda):
    # events of 3 at N_TILES with two messages made the longest of all: each is
    # the first of its event and lies in the second tile of a block behind the
    # 64th, where p0 is off[f0], with the tile carry in it, plus bpre[f0 / 2048]
    n = G.N_TILES
    per_block = G.regime(n).per_block
    ef = _events_of(n, 3)
    ia, ib = 70 * per_block + 1525, 100 * per_block + 1024
    for i in (ia, ib):
        assert i % 3 == 0 and i % per_block >= 1024 and i // per_block > 64
    host, dev = _first(cuda, n, ef)
    src, soff, lens = host[0], host[1].copy(), host[2].copy()
    soff[[ia, ib]], lens[[ia, ib]] = (5, 9), (80000, 90000)
    dev = _patched(dev, src_offsets={ia: 5, ib: 9}, lengths={ia: 80000, ib: 90000})
    ev = layout(lens, ef)[1]
    sizes = np.diff(ev)
    order = np.argsort(sizes)
    assert [int(e) for e in order[-2:]] == [ia // 3, ib // 3] and \
        sizes[order[-3]] < sizes[ia // 3] - 4 and sizes[ia // 3] < sizes[ib // 3] - 4
    case = (src, soff, lens) + host[3:]
    size = int(ev[-1]) + 64
    # one event over the cap, then two: the lower index
    _refused(cuda, N.BMQCRC_PUT_PACK_EVENT_TOO_BIG, ib // 3, *case, ef=ef, size=size, inputs=dev,
             max_event_bytes=int(sizes[ib // 3]) - 4)
    _refused(cuda, N.BMQCRC_PUT_PACK_EVENT_TOO_BIG, ia // 3, *case, ef=ef, size=size, inputs=dev,
             max_event_bytes=int(sizes[ia // 3]) - 4)
    # the cap exactly the largest event
    crcs = _large()[1][:n].copy()
    crcs[[ia, ib]] = host_crcs(src, soff[[ia, ib]], lens[[ia, ib]])
    img = model_bytes_fast(*case, ef, crcs)
    _check(cuda, *case, ef=ef, model=(img, ev, crcs), inputs=dev,
           max_event_bytes=int(sizes[ib // 3]))


def test_destination_size_past_one_tile_per_block(cuda):
    n = G.N_TILES
    ef = _events_of(n, 3)
    ev = _event_offsets(n, 3)
    total, n_events = int(ev[-1]), ev.size - 1
    host, dev = _first(cuda, n, ef)
    kind = N.BMQCRC_PUT_PACK_DST_TOO_SMALL
    _refused(cuda, kind, n_events - 1, *host, ef=ef, size=total + 64, inputs=dev,
             dst_bytes=total - 4)
    # halfway through the image: the first event that ends past it, while
    # every later one, in every block of the check grid, refuses as well
    half = total // 2
    first = int(np.searchsorted(ev[1:], half, side="right"))
    assert ev[first] <= half < ev[first + 1] and n_events // 3 < first < 2 * n_events // 3
    _refused(cuda, kind, first, *host, ef=ef, size=total + 64, inputs=dev, dst_bytes=half)
    _check(cuda, *host, ef=ef, model=_expected(n, 3), inputs=dev, slack=0)  # dst_bytes == total
    # one event per message at N_FRAME: some 260,000 events refuse, over three
    # steps of every block of the check grid
    n = G.N_FRAME
    ef = _events_of(n, 1)
    ev = _event_offsets(n, 1)
    total = int(ev[-1])
    half = total // 2
    first = int(np.searchsorted(ev[1:], half, side="right"))
    assert ev[first] <= half < ev[first + 1] and n - first > 200000
    host, dev = _first(cuda, n, ef)
    _refused(cuda, kind, first, *host, ef=ef, size=total + 64, inputs=dev, dst_bytes=half)
    assert np.array_equal(dev["src"].cpu().numpy(), host[0])
