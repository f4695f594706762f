"""Device-side DATA/journal record packer (bmqcrc_message_records_pack, ABI
2.11) on the GPU.  The oracle throughout is tests/records_pack_model.py, which
the CPU tests hold to PartitionWriter and to the reference's fixture: every
check compares both destinations byte for byte, `out`, `record_offsets`, and
the canaries behind both totals."""
import ctypes
import functools

import numpy as np
import pytest

from blazingmq_amd import (BmqCrcError, Crc32c, _native as N, last_copy, last_launch,
                           last_put_pack, last_records_pack, pack_events, pack_records)
from blazingmq_amd import storage as S
import device_views as V
import pack_pool
import put_pack_model as P
import test_grid_regimes as G
from records_pack_model import (DH, REC, data_bytes_fast, golden_case, host_crcs,
                                journal_bytes_fast, layout, model_bytes, pad_of, pool_crcs,
                                pooled_crcs, random_meta, wrap_partition)

pytestmark = pytest.mark.gpu

FILL = 0xA5
FILL32 = 0x5A5A5A5A
FILL64 = 0x5A5A5A5A5A5A5A5A
KW = dict(file_key=b"\x11\x22\x33\x44\x55", lease_id=3, first_seq=2, data_file_pos=40,
          timestamp=0x6720EAB4)
OPTIONAL = {"data_flags": np.uint8, "ref_counts": np.uint32, "timestamps": np.int64,
            "expected": np.uint32}
KIND_NAME = {1: b"RECORD_TOO_BIG", 2: b"SRC_RANGE", 3: b"DST_TOO_SMALL", 4: b"DATA_FILE_FULL"}


def _side_stream(cuda):
    """A stream of its own from the high-priority pool.  The pool of default
    priority hands its 32 streams out in turn and a workspace, with its
    planner history, belongs to (device, stream): tests elsewhere that assert
    a launch plan rely on which of them they are given, so none is taken here."""
    import torch
    return torch.cuda.Stream(cuda, priority=-1)


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


def _inputs(cuda, src, soff, lens, qkeys, guids, kw, place=None):
    t = lambda name, a, dtype: _t(cuda, a, dtype, place, name)
    d = dict(src=t("src", src, np.uint8), src_offsets=t("src_offsets", soff, np.int64),
             lengths=t("lengths", lens, np.uint32), queue_keys=t("queue_keys", qkeys, np.uint8),
             guids=t("guids", guids, np.uint8))
    for name, dt in OPTIONAL.items():
        d[name] = t(name, kw[name], dt) if kw.get(name) is not None else None
    return d


def _scalars(kw):
    return {k: v for k, v in kw.items() if k not in OPTIONAL}


def _result(n, total, n_bad=0, first_bad=None, kind=0, index=0):
    return dict(n_msgs=n, data_bytes=total, journal_bytes=0 if kind else REC * n, n_bad=n_bad,
                first_bad=n if first_bad is None else first_bad, refused_kind=kind,
                refused_index=index)


def _check(cuda, src, soff, lens, qkeys, guids, kw=KW, slack=64, sync=True, stream=None,
           n_bad=0, first_bad=None, phases=None, model=None, inputs=None):
    """One pack into canary destinations against the model.  Returns the
    packed (DATA, journal) bytes (host).  `phases` maps every pointer of the
    call (src, src_offsets, lengths, queue_keys, guids, the optional arrays,
    dst, journal_dst, record_offsets, out) to the phase of its base: the call
    then goes through the raw entry point (synchronous, on the current stream)
    and the sentinel margins around every buffer are checked; None: the
    wrapper, every buffer at the start of an allocation.  `model` is (DATA
    bytes, journal bytes, CRCs) of this very call when the caller has them
    already: the model and the host CRCs are not run then.  `inputs` is
    _inputs' answer for these arguments, already on the device."""
    import torch
    place = V.Placer(cuda, phases) if phases is not None else None
    n = len(lens)
    if model is not None:
        exp_d, exp_j, crcs = model
    else:
        crcs = host_crcs(src, soff, lens)
        stored = crcs if kw.get("expected") is None else np.asarray(kw["expected"], np.uint32)
        model_kw = {k: v for k, v in kw.items() if k != "expected"}
        exp_d, exp_j = model_bytes(src, soff, lens, qkeys, guids, stored, **model_kw)
    total = exp_d.size
    d = inputs if inputs is not None else _inputs(cuda, src, soff, lens, qkeys, guids, kw, place)
    if place is not None:
        assert sync and stream is None
        dst = place.fill("dst", total + slack, np.uint8, FILL)
        jour = place.fill("journal_dst", REC * n + slack, np.uint8, FILL)
        out = place.fill("out", n, np.uint32, FILL32)
        roff = place.fill("record_offsets", n + 1, np.uint64, FILL64)
        rc, err, r = _raw(cuda, d, dict(dict(timestamp=0), **kw), n, dst, total + slack, jour, roff, out,
                          N.BMQCRC_F_DEVICE_PTRS)
        assert rc == 0, err
        res = r.as_dict()
        place.check()
    else:
        dst = torch.full((total + slack,), FILL, dtype=torch.uint8, device=cuda)
        jour = torch.full((REC * n + slack,), FILL, dtype=torch.uint8, device=cuda)
        out = torch.full((n,), FILL32, dtype=torch.int32, device=cuda)
        rdst, rjour, roff, rout, res = pack_records(dst=dst, journal_dst=jour, out=out, sync=sync,
                                                    stream=stream, **d, **_scalars(kw))
        assert rdst is dst and rjour is jour and rout is out
    s = stream if stream is not None else torch.cuda.current_stream(cuda)
    want = _result(n, total, n_bad, first_bad)
    assert res == (want if sync else None)
    assert last_records_pack(cuda.index, s) == want
    host_d, host_j = dst.cpu().numpy(), jour.cpu().numpy()
    for got, exp in ((host_d, exp_d), (host_j, exp_j)):
        diff = np.nonzero(got[:exp.size] != exp)[0]
        assert diff.size == 0, (diff.size, [int(i) for i in diff[:8]])
        assert np.all(got[exp.size:] == FILL)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), crcs)
    assert np.array_equal(roff.cpu().numpy(), layout(lens)[1])
    assert np.array_equal(d["src"].cpu().numpy(), np.asarray(src))  # only read
    return host_d[:total], host_j[:REC * n]


def _raw(cuda, d, kw, n, dst, dst_bytes, jour, roff, out, flags, src_bytes=None):
    import torch
    p = N.RecordsPack()
    p.struct_size = ctypes.sizeof(N.RecordsPack)
    p.src = d["src"].data_ptr()
    p.src_bytes = d["src"].numel() if src_bytes is None else src_bytes
    p.src_offsets, p.lengths = d["src_offsets"].data_ptr(), d["lengths"].data_ptr()
    p.queue_keys, p.guids = d["queue_keys"].data_ptr(), d["guids"].data_ptr()
    for name in OPTIONAL:
        setattr(p, name, d[name].data_ptr() if d[name] is not None else None)
    p.file_key = (ctypes.c_uint8 * 5)(*kw["file_key"])
    p.lease_id, p.first_seq, p.timestamp = kw["lease_id"], kw["first_seq"], kw["timestamp"]
    p.data_file_pos, p.n = kw["data_file_pos"], n
    p.dst, p.dst_bytes = dst.data_ptr(), dst_bytes
    p.journal_dst, p.journal_bytes = jour.data_ptr(), jour.numel()
    p.record_offsets, p.out = roff.data_ptr(), out.data_ptr()
    stream = torch.cuda.current_stream(cuda)
    o = N.make_opts(device=cuda.index, stream=stream.cuda_stream, flags=flags)
    res = N.RecordsResult()
    res.n_msgs = FILL64
    rc = N.lib.bmqcrc_message_records_pack(ctypes.byref(p), ctypes.byref(res), ctypes.byref(o))
    return rc, N.lib.bmqcrc_last_error(), res


def _refused(cuda, kind, index, src, soff, lens, qkeys, guids, kw=KW, dst_bytes=None,
             src_bytes=None, size=None, phases=None, inputs=None):
    """The call is refused with (kind, index), synchronously and asynchronously,
    and dst, journal_dst, out and record_offsets keep their canaries whole.
    `phases`: as in _check.  `inputs` is _inputs' answer for these arguments,
    already on the device."""
    import torch
    n = len(lens)
    place = V.Placer(cuda, phases) if phases is not None else None
    d = inputs if inputs is not None else \
        _inputs(cuda, src, soff, lens, qkeys, guids, kw, place)
    if size is None:
        size = int(layout(lens)[1][-1]) + 64
    stream = torch.cuda.current_stream(cuda)
    for flags in (N.BMQCRC_F_DEVICE_PTRS, N.BMQCRC_F_DEVICE_PTRS | N.BMQCRC_F_ASYNC):
        if place is not None:
            dst = place.fill("dst", size, np.uint8, FILL)
            jour = place.fill("journal_dst", REC * n + 64, np.uint8, FILL)
            out = place.fill("out", n, np.uint32, FILL32)
            roff = place.fill("record_offsets", n + 1, np.uint64, FILL64)
        else:
            dst = torch.full((size,), FILL, dtype=torch.uint8, device=cuda)
            jour = torch.full((REC * n + 64,), FILL, dtype=torch.uint8, device=cuda)
            out = torch.full((n,), FILL32, dtype=torch.int32, device=cuda)
            roff = torch.full((n + 1,), FILL64, dtype=torch.int64, device=cuda)
        rc, err, res = _raw(cuda, d, kw, n, dst, size if dst_bytes is None else dst_bytes, jour,
                            roff, out, flags, src_bytes)
        want = _result(n, 0, kind=kind, index=index)
        if flags & N.BMQCRC_F_ASYNC:
            assert rc == 0 and res.n_msgs == FILL64, (rc, err)
        else:
            assert rc == N.BMQCRC_EINVAL and b"BMQCRC_REC_PACK_" + KIND_NAME[kind] in err, err
            assert (" %d " % index).encode() in err, err
            assert res.as_dict() == want
        assert last_records_pack(cuda.index, stream) == want
        assert bool((dst == FILL).all()) and bool((jour == FILL).all())
        assert bool((out == FILL32).all()) and bool((roff == FILL64).all())
        if place is not None:
            place.check()


def _short(rng, n, lo=1, hi=41, src_size=1 << 16):
    src = rng.integers(0, 256, size=src_size, dtype=np.uint8)
    lens = rng.integers(lo, hi, size=n)
    soff = rng.integers(0, src_size - hi, size=n)
    return (src, soff, lens) + random_meta(rng, n)


def _all_options(rng, n, kw=KW):
    return dict(kw, data_flags=rng.integers(0, 256, size=n, dtype=np.uint8),
                ref_counts=rng.choice(np.array([1, 2, 4095, 4096, (1 << 20) - 1], np.uint32), n),
                timestamps=rng.integers(1, 1 << 62, size=n, dtype=np.int64))


def test_every_length_at_every_source_misalignment(cuda):
    # lengths 0..39: every padding count 1..8; records are 8-byte aligned, so
    # a payload lands at 4 or 12 mod 16
    rng = np.random.default_rng(1)
    lens = np.arange(40)
    src = rng.integers(0, 256, size=40 * 96 + 64, dtype=np.uint8)
    seen = set()
    for mis in range(16):
        soff = 96 * np.arange(40) + mis + 16 * rng.integers(0, 2, size=40)
        assert np.all(soff % 16 == mis)
        perm = rng.permutation(lens)
        qkeys, guids = random_meta(rng, 40)
        _check(cuda, src, soff, perm, qkeys, guids, _all_options(rng, 40))
        seen |= set((layout(perm)[1][:-1] + DH) % 16)
    assert seen == {4, 12}
    assert set(layout(lens)[0] - DH - lens) == set(range(1, 9))


def test_smallest_cases(cuda):
    rng = np.random.default_rng(2)
    src = rng.integers(0, 256, size=256, dtype=np.uint8)
    for ln in (0, 1):
        qkeys, guids = random_meta(rng, 1)
        data, jour = _check(cuda, src, [7], [ln], qkeys, guids)
        assert data.size == 16 and list(data[DH + ln:]) == [4 - ln] * (4 - ln) and jour.size == 60
    # n = 0: nothing is written, zeros are reported
    data, jour = _check(cuda, src, np.zeros(0, np.int64), np.zeros(0, np.int64),
                        np.zeros((0, 5), np.uint8), np.zeros((0, 16), np.uint8))
    assert data.size == 0 and jour.size == 0
    # every optional array absent (above), then all present
    case = _short(rng, 9, 0, 30, src_size=256)
    crcs = host_crcs(*case[:3])
    _check(cuda, *case, dict(_all_options(rng, 9), expected=crcs))


def test_wrapper_allocates_the_exact_destinations(cuda):
    rng = np.random.default_rng(3)
    case = _short(rng, 77, 0, 30)
    d = _inputs(cuda, *case, KW)
    dst, jour, roff, out, res = pack_records(**d, **_scalars(KW))
    exp_d, exp_j = model_bytes(*case, host_crcs(*case[:3]), **KW)
    assert dst.numel() == exp_d.size and np.array_equal(dst.cpu().numpy(), exp_d)
    assert jour.numel() == exp_j.size and np.array_equal(jour.cpu().numpy(), exp_j)
    assert int(roff[-1]) == exp_d.size and res == _result(77, exp_d.size)
    with pytest.raises(ValueError, match="dst is required"):
        pack_records(sync=False, **d, **_scalars(KW))


@pytest.mark.parametrize("n", [1025, 3 * 1024 + 1])
def test_more_than_one_layout_block(cuda, n):
    rng = np.random.default_rng(4)
    case = _short(rng, n)
    _check(cuda, *case, _all_options(rng, n))
    _check(cuda, *case)


def test_a_layout_block_of_two_tiles(cuda):
    # 258 tiles of 1,024 messages for at most 256 blocks: per_block is 2,048
    # and each of the 129 blocks scans two tiles, the second on top of the
    # first's carry -- the smallest n at which a block loops.  Lengths 0..7
    # keep both destinations below 20 MB; every byte is checked.
    rng = np.random.default_rng(16)
    n = 256 * 1024 + 1025
    src, soff, lens, qkeys, guids = _short(rng, n, 0, 8)
    _check(cuda, src, soff, lens, qkeys, guids)
    # the same inputs with message 2048, the first of the second block, out of range
    soff[2048] = src.size - int(lens[2048]) + 1
    _refused(cuda, N.BMQCRC_REC_PACK_SRC_RANGE, 2048, src, soff, lens, qkeys, guids)


def test_a_long_message_among_short_ones(cuda):
    rng = np.random.default_rng(5)
    src, soff, lens, qkeys, guids = _short(rng, 41, 1, 41, src_size=1 << 19)
    lens[20], soff[20] = 300 << 10, 13  # longer than a 64 KiB chunk of the copy pass
    first = _check(cuda, src, soff, lens, qkeys, guids)
    again = _check(cuda, src, soff, lens, qkeys, guids)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])


def test_record_too_big(cuda):
    # a length the DataHeader's 29 bits of words cannot hold, far outside the
    # small src as well: RECORD_TOO_BIG depends on lengths alone and outranks
    # SRC_RANGE, so sizing dst never needs an out-of-range length
    rng = np.random.default_rng(6)
    src, soff, lens, qkeys, guids = _short(rng, 1300, src_size=1 << 12)
    lens[1234] = 0x80000000
    lens[1290] = 0xFFFFFFFF
    size = int(layout(np.where(lens > 40, 0, lens))[1][-1]) + 64
    _refused(cuda, N.BMQCRC_REC_PACK_RECORD_TOO_BIG, 1234, src, soff, lens, qkeys, guids,
             size=size)


def test_source_range(cuda):
    rng = np.random.default_rng(7)
    src, soff, lens, qkeys, guids = _short(rng, 1500, src_size=1 << 15)
    src_bytes = 20000  # declared smaller than the tensor: a broken check stays inside it
    soff = soff % (src_bytes - 64)
    soff[1200], lens[1200] = src_bytes - 10, 11               # one byte past
    soff[1300] = (1 << 63) - 8                                 # the sum needs 64 bits
    soff[77], lens[77] = src_bytes, 0                          # empty at the very end: legal
    _refused(cuda, N.BMQCRC_REC_PACK_SRC_RANGE, 1200, src, soff, lens, qkeys, guids,
             src_bytes=src_bytes)


def test_destination_size(cuda):
    rng = np.random.default_rng(8)
    case = _short(rng, 2300)
    Q = layout(case[2])[1]
    total = int(Q[-1])
    _check(cuda, *case, slack=0)                               # dst_bytes == total
    _refused(cuda, N.BMQCRC_REC_PACK_DST_TOO_SMALL, 2299, *case, dst_bytes=total - 1)
    _refused(cuda, N.BMQCRC_REC_PACK_DST_TOO_SMALL, 1024, *case, dst_bytes=int(Q[1025]) - 8)
    _refused(cuda, N.BMQCRC_REC_PACK_DST_TOO_SMALL, 1023, *case, dst_bytes=int(Q[1024]) - 1)
    _refused(cuda, N.BMQCRC_REC_PACK_DST_TOO_SMALL, 0, *case, dst_bytes=8)
    with pytest.raises(BmqCrcError, match="DST_TOO_SMALL: the record of message 2299 "):
        import torch
        pack_records(**_inputs(cuda, *case, KW), **_scalars(KW),
                     dst=torch.zeros(total - 8, dtype=torch.uint8, device=cuda))


def test_data_file_full(cuda):
    rng = np.random.default_rng(9)
    src = rng.integers(0, 256, size=256, dtype=np.uint8)
    qkeys, guids = random_meta(rng, 5)
    kw = dict(KW, data_file_pos=8 * ((1 << 32) - 1) - 64)      # 64 bytes of file are left
    lens, soff = np.array([0, 1, 2, 3, 4]), np.arange(5) * 9
    assert list(layout(lens)[1]) == [0, 16, 32, 48, 64, 88]
    _refused(cuda, N.BMQCRC_REC_PACK_DATA_FILE_FULL, 4, src, soff, lens, qkeys, guids, kw)
    # four records fill the file to its last addressable byte
    data, jour = _check(cuda, src, soff[:4], lens[:4], qkeys[:4], guids[:4], kw)
    assert int.from_bytes(jour[180 + 32:180 + 36].tobytes(), "big") == (1 << 32) - 1 - 2


def test_two_kinds_at_once_report_the_lowest(cuda):
    rng = np.random.default_rng(10)
    src, soff, lens, qkeys, guids = _short(rng, 1100, src_size=1 << 12)
    soff[1050] = 1 << 40
    # SRC_RANGE at 1050 and a dst that message 3 already overruns
    _refused(cuda, N.BMQCRC_REC_PACK_SRC_RANGE, 1050, src, soff, lens, qkeys, guids,
             dst_bytes=int(layout(lens)[1][3]) + 8)
    # DST_TOO_SMALL at 3 and DATA_FILE_FULL at 0
    soff[1050] = 0
    _refused(cuda, N.BMQCRC_REC_PACK_DST_TOO_SMALL, 3, src, soff, lens, qkeys, guids,
             dict(KW, data_file_pos=8 * ((1 << 32) - 1) - 8),
             dst_bytes=int(layout(lens)[1][3]) + 8)
    # RECORD_TOO_BIG at 1099 and SRC_RANGE at 2
    soff[2], lens[1099] = 1 << 40, 0x80000000
    _refused(cuda, N.BMQCRC_REC_PACK_RECORD_TOO_BIG, 1099, src, soff, lens, qkeys, guids,
             size=1 << 16)


def test_message_offset_dwords_across_4_gib_of_file(cuda):
    rng = np.random.default_rng(11)
    case = _short(rng, 200)
    kw = dict(KW, data_file_pos=(1 << 32) - 64)
    data, jour = _check(cuda, *case, kw)
    offs = [int.from_bytes(jour[REC * i + 32:REC * i + 36].tobytes(), "big") for i in range(200)]
    Q = layout(case[2])[1]
    assert offs == [(kw["data_file_pos"] + int(q)) // 8 for q in Q[:-1]]
    assert offs[0] < (1 << 29) <= offs[-1]  # 8 * 2^29 = 4 GiB


def test_expected_crcs_go_to_the_journal_and_are_checked(cuda):
    rng = np.random.default_rng(12)
    case = _short(rng, 1500, 0, 41)
    crcs = host_crcs(*case[:3])
    right = _check(cuda, *case, dict(KW, expected=crcs))
    plain = _check(cuda, *case)
    assert np.array_equal(right[0], plain[0]) and np.array_equal(right[1], plain[1])
    wrong = crcs.copy()
    for i in (1301, 64, 700):
        wrong[i] ^= 1 << (i % 32)
    got = _check(cuda, *case, dict(KW, expected=wrong), n_bad=3, first_bad=64)
    assert np.array_equal(got[0], plain[0])  # dst is the same either way
    stored = [int.from_bytes(got[1][REC * i + 52:REC * i + 56].tobytes(), "big")
              for i in range(1500)]
    assert stored == [int(x) for x in wrong]


def test_asynchronous_call(cuda):
    import torch
    rng = np.random.default_rng(13)
    case = _short(rng, 2000, 0, 300)
    kw = _all_options(rng, 2000)
    got = _check(cuda, *case, kw, sync=False)
    s = _side_stream(cuda)
    with torch.cuda.stream(s):
        again = _check(cuda, *case, kw, sync=False, stream=s)
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1])


def test_state_untouched(cuda):
    import torch
    rng = np.random.default_rng(14)
    host = rng.integers(0, 256, size=1 << 20, dtype=np.uint8)
    arena = torch.from_numpy(host).to(cuda)
    lens = rng.integers(1, 1025, size=5001).astype(np.uint32)
    offs = (rng.random(lens.size) * (host.size - 1100)).astype(np.int64)
    d_off, d_len = _t(cuda, offs, np.int64), _t(cuda, lens, np.uint32)
    copy_dst = torch.zeros(int(lens.sum()) + 16, dtype=torch.uint8, device=cuda)
    doff = _t(cuda, np.concatenate([[0], np.cumsum(lens)[:-1]]), np.int64)
    qkeys, guids = random_meta(rng, lens.size)
    qids, _, flags = P.random_meta(rng, 30)
    rec = _inputs(cuda, host, offs, lens, qkeys, guids, KW)
    rec["src"] = arena
    plans = []
    for with_pack in (False, True):
        s = _side_stream(cuda)
        with torch.cuda.stream(s):
            Crc32c.copy_batch(arena, d_off[:40], d_len[:40], copy_dst, doff[:40], stream=s)
            pack_events(arena, d_off[:30], d_len[:30], _t(cuda, qids, np.int32),
                        _t(cuda, guids[:30], np.uint8), _t(cuda, flags, np.uint8), stream=s)
            put = last_put_pack(cuda.index, s)
            assert put[:2] == (30, 1) and put[3:] == (0, 0)
            Crc32c.calculate_batch(arena, d_off, d_len, stream=s, seg_bytes=1024)
            before = last_launch(cuda.index, s, offsets=True)
            assert last_copy(cuda.index, s) == (40, 0, 40)
            if with_pack:
                assert last_records_pack(cuda.index, s) == _result(0, 0)  # none yet on s
                pack_records(stream=s, **rec, **_scalars(KW))
                pack_records(stream=s, sync=False, **rec, **_scalars(KW),
                             dst=torch.zeros(64, dtype=torch.uint8, device=cuda),
                             journal_dst=torch.zeros(REC * lens.size, dtype=torch.uint8,
                                                     device=cuda))
                assert last_records_pack(cuda.index, s)["refused_kind"] == \
                    N.BMQCRC_REC_PACK_DST_TOO_SMALL
                assert last_launch(cuda.index, s, offsets=True) == before
                assert last_copy(cuda.index, s) == (40, 0, 40)
                assert last_put_pack(cuda.index, s) == put
            out = Crc32c.calculate_batch(arena, d_off, d_len, stream=s, seg_bytes=1024)
            plans.append(last_launch(cuda.index, s, offsets=True))
        s.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), host_crcs(host, offs, lens))
    assert plans[0] == plans[1], plans


@pytest.mark.parametrize("k", [0, 1])
def test_the_reference_fixture_on_the_device(cuda, k):
    src, soff, lens, qkeys, guids, crc, kw, want_data, want_rec = golden_case(k)
    data, jour = _check(cuda, src, soff, lens, qkeys, guids, kw)
    assert np.array_equal(data, want_data) and np.array_equal(jour, want_rec)


def test_put_events_to_verified_partition(cuda):
    # producer to store to recovery, on the device: payloads are packed into a
    # PUT event, the event's payloads into records with the event's CRCs as
    # `expected`, and the partition they make passes the recovery check
    rng = np.random.default_rng(15)
    n = 300
    src, soff, lens, qkeys, guids = _short(rng, n, 0, 120)
    qkeys[:] = qkeys[0]
    qids, _, flags = P.random_meta(rng, n)
    ev, _, ev_crcs = pack_events(_t(cuda, src, np.uint8), _t(cuda, soff, np.int64),
                                 _t(cuda, lens, np.uint32), _t(cuda, qids, np.int32),
                                 _t(cuda, guids, np.uint8), _t(cuda, flags, np.uint8))
    app = _t(cuda, P.layout(lens)[0] + P.HDR, np.int64)
    kw = dict(KW, lease_id=1)
    dst, jour, roff, crcs, res = pack_records(
        ev, app, _t(cuda, lens, np.uint32), _t(cuda, qkeys, np.uint8),
        _t(cuda, guids, np.uint8), expected=ev_crcs, **kw)
    assert res == _result(n, int(layout(lens)[1][-1]))
    assert np.array_equal(crcs.cpu().numpy(), ev_crcs.cpu().numpy())
    jf, df = wrap_partition(dst.cpu().numpy(), jour.cpu().numpy(), qkeys[0])
    got = S.verify_partition(jf, df)
    assert (got["recovery_rc"], got["n_messages"], got["n_bad"]) == (0, n, 0)
    victim = next(i for i in range(100, n) if lens[i] > 0)
    df[40 + int(roff[victim]) + DH] ^= 0x40
    got = S.verify_partition(jf, df)
    assert (got["recovery_rc"], got["n_messages"], got["n_bad"]) == (0, n, 1)
    assert list(got["bad_record_offsets"]) == [44 + 60 + REC * victim]


# ---- past one tile per block (DESIGN.md sections 13 and 20) -------------------
#
# One set of N_FRAME messages (pack_pool.py: variable lengths, every padding
# count and an empty message in every tile, one message of 70,000 bytes every
# 3,001), built once; the smaller sizes are its prefixes.  The expected bytes
# come from data_bytes_fast and journal_bytes_fast, which
# test_records_pack_model.py holds to the loop model and to PartitionWriter.
# The caches below live as long as the session, as test_gpu_rollover.py's do:
# some 80 MB on the host (the inputs, two DATA images of 32 MB) and 30 MB on
# the device.

MAX_FILE = 8 * 0xFFFFFFFF  # kRecMaxFileBytes: where MessageOffsetDwords stops


@functools.lru_cache(maxsize=None)
def _large():
    """((src, soff, lens, qkeys, guids) of N_FRAME messages, KW with every
    optional array but `expected`, their CRCs from one CRC per pool pair).
    Shared, never modified."""
    src, soff, lens, ix = pack_pool.messages(G.N_FRAME)
    rng = np.random.default_rng(22)
    case = (src, soff, lens) + random_meta(rng, G.N_FRAME)
    kw = _all_options(rng, G.N_FRAME)
    crcs = pooled_crcs(pool_crcs(*pack_pool.pool()), ix)
    for a in case + (crcs,) + tuple(kw[k] for k in OPTIONAL if k in kw):
        a.setflags(write=False)
    return case, kw, crcs


@functools.lru_cache(maxsize=None)
def _large_dev(cuda):
    case, kw, _ = _large()
    return _inputs(cuda, *(np.array(a) for a in case),
                   {k: np.array(kw[k]) for k in OPTIONAL if k in kw})


@functools.lru_cache(maxsize=None)
def _large_data(with_flags):
    """(the DATA bytes of all N_FRAME records, Q).  The first n records' bytes
    are the first Q[n] of them."""
    case, kw, _ = _large()
    data = data_bytes_fast(*case[:3], kw["data_flags"] if with_flags else None)
    Q = layout(case[2])[1]
    assert data.size == int(Q[-1]) == int((DH + case[2] + pad_of(case[2])).sum())  # the model's total
    return data, Q


def _first(cuda, n, options=True, expected=None, **scalars):
    """The first n messages: (host case, keywords with `scalars` changed, the
    device inputs, (DATA bytes, journal bytes, CRCs) expected)."""
    case, kw, crcs = _large()
    host = (case[0],) + tuple(a[:n] for a in case[1:])
    kw = {k: (v[:n] if k in OPTIONAL else v) for k, v in kw.items() if options or k not in OPTIONAL}
    kw.update(scalars)
    dev = {}
    for k, v in _large_dev(cuda).items():
        if k in OPTIONAL:
            dev[k] = v[:n] if options and v is not None else None
        else:
            dev[k] = v if k == "src" else v[:n]
    stored = crcs[:n]
    if expected is not None:
        kw["expected"] = stored = expected
        dev["expected"] = _t(cuda, expected, np.uint32)
    data, Q = _large_data(options)
    jour = journal_bytes_fast(host[2], host[3], host[4], stored,
                              **{k: v for k, v in kw.items() if k not in ("data_flags", "expected")})
    return host, kw, dev, (data[:int(Q[n])], jour, crcs[:n])


def _patched(dev, **changes):
    """`dev` with clones of the named tensors, entry i set to v for every
    (i, v) of the name's dict."""
    out = dict(dev)
    for name, entries in changes.items():
        out[name] = dev[name].clone()
        for i, v in entries.items():
            out[name][i] = v
    return out


@pytest.mark.parametrize("n", [G.N_WAVES, G.N_FULL, G.N_TILES, G.N_FRAME],
                         ids=["N_WAVES", "N_FULL", "N_TILES", "N_FRAME"])
def test_past_one_tile_per_block(cuda, n):
    # N_WAVES: block_prefix's cross-wave leg and the journal loop's later steps.
    # N_FULL: all 256 blocks; the DataHeader loop's second step; the sequence
    # number's high half changes inside the call.  N_TILES: two tiles a block.
    # N_FRAME: three, and both per-message regimes of k_rec_frame.
    first_seq = (1 << 32) - 1000 if n == G.N_FULL else 2
    host, kw, dev, model = _first(cuda, n, first_seq=first_seq)
    _check(cuda, *host, kw, model=model, inputs=dev)


def test_a_file_filled_to_its_last_addressable_byte(cuda):
    n = G.N_TILES
    total = int(_large_data(True)[1][n])
    host, kw, dev, model = _first(cuda, n, data_file_pos=MAX_FILE - total)
    data, jour = _check(cuda, *host, kw, model=model, inputs=dev)  # record_offsets[n] included
    last = jour[REC * (n - 1):]
    assert int.from_bytes(last[32:36].tobytes(), "big") + \
        int(layout(host[2])[0][-1]) // 8 == 0xFFFFFFFF
    # one byte of file less
    _refused(cuda, N.BMQCRC_REC_PACK_DATA_FILE_FULL, n - 1, *host,
             dict(_scalars(kw), data_file_pos=MAX_FILE - total + 8), size=total + 64, inputs=dev)


def test_past_one_tile_per_block_without_the_optional_arrays(cuda):
    host, kw, dev, model = _first(cuda, G.N_TILES, options=False)
    assert not any(k in kw for k in OPTIONAL) and all(dev[k] is None for k in OPTIONAL)
    _check(cuda, *host, kw, model=model, inputs=dev)


def test_past_one_tile_per_block_on_a_side_stream(cuda):
    import torch
    host, kw, dev, model = _first(cuda, G.N_TILES)
    torch.cuda.synchronize(cuda)
    s = _side_stream(cuda)
    with torch.cuda.stream(s):
        _check(cuda, *host, kw, model=model, inputs=dev, sync=False, stream=s)


CRC_DWORD = 13  # of a journal record's 15: the stored CRC, bytes 52..55


def _crc_dword(m):
    """The index of record m's CRC dword among the journal's: the thread of
    k_rec_frame's journal loop that compares it, modulo the grid."""
    return G.RECORD_DWORDS * m + CRC_DWORD


def _crc_wave(m):
    """The wave and step of k_rec_frame's journal loop that holds record m's
    CRC dword: 64 consecutive dwords, and the grid is a multiple of 64."""
    return _crc_dword(m) // 64


def test_expected_mismatches_in_every_step_of_the_journal_loop(cuda):
    n = G.N_FRAME
    grid = G.constants()["kPackFrameThreads"] * G.constants()["kPackFrameBlocks"]
    crcs = _large()[2]
    # every 1,000th record (999, 1,999, ...), the record after one of them,
    # whose CRC dword lies in the same wave, and the last record, the only one
    # past the frame grid's first step of records
    pair = 200999
    assert _crc_wave(pair) == _crc_wave(pair + 1) and pair % 1000 == 999
    bad = np.concatenate([np.arange(999, n, 1000), [pair + 1, n - 1]])
    assert np.unique(bad).size == bad.size == n // 1000 + 2 and n - 1 == grid
    steps = {_crc_dword(int(m)) // grid for m in bad}
    assert steps == set(range(G.RECORD_DWORDS + 1))  # a mismatch in every step, the 16th too
    wrong = crcs.copy()
    wrong[bad] ^= (1 << (bad % 32)).astype(np.uint32)
    host, kw, dev, model = _first(cuda, n, expected=wrong)
    data, jour = _check(cuda, *host, kw, model=model, inputs=dev, n_bad=bad.size, first_bad=999)
    stored = jour.reshape(n, REC)[:, 52:56]
    assert np.array_equal(stored, wrong.astype(">u4").view(np.uint8).reshape(n, 4))
    # the only mismatch at record 524,288
    wrong = crcs.copy()
    wrong[grid] ^= 0x80000000
    host, kw, dev, model = _first(cuda, n, expected=wrong)
    _check(cuda, *host, kw, model=model, inputs=dev, n_bad=1, first_bad=grid)


def test_bounds_found_by_bisection_in_a_late_block_of_two_tiles(cuda):
    # k_rec_place searches off[] as pass 1 left it, block-local with the tile
    # carry in it, in the one block with before <= bound < after
    n = G.N_TILES
    per_block = G.regime(n).per_block
    host, kw, dev, _ = _first(cuda, n)
    kw = _scalars(kw)
    Q = _large_data(True)[1][:n + 1]
    total = int(Q[-1])
    lo = 100 * per_block
    assert per_block == 2048 and lo // per_block > 64 and lo + per_block < n
    ks = (lo, lo + 1023, lo + 1024, lo + 2047)

    def refused(kind, index, dst_bytes=total + 64, room=None):
        _refused(cuda, kind, index, *host,
                 kw if room is None else dict(kw, data_file_pos=MAX_FILE - room),
                 dst_bytes=dst_bytes, size=total + 64, inputs=dev)

    small, full = N.BMQCRC_REC_PACK_DST_TOO_SMALL, N.BMQCRC_REC_PACK_DATA_FILE_FULL
    for k in ks:
        refused(small, k, int(Q[k + 1]) - 8)
    refused(small, lo, int(Q[lo]))            # the bound is the block's `before`
    refused(small, lo - 1, int(Q[lo]) - 8)    # the previous block's last record
    refused(small, n - 1, total - 8)
    for k in ks:
        refused(full, k, room=int(Q[k + 1]) - 8)
    # both bounds, in different blocks, the file's in the earlier one: kind 3
    k_dst, k_file = 120 * per_block + 1030, 50 * per_block + 7
    refused(small, k_dst, int(Q[k_dst + 1]) - 8, room=int(Q[k_file + 1]) - 8)
    assert np.array_equal(dev["src"].cpu().numpy(), host[0])


def test_message_refusals_past_one_tile_per_block(cuda):
    n = G.N_TILES
    per_block = G.regime(n).per_block
    host, kw, dev, _ = _first(cuda, n)
    kw = _scalars(kw)
    size = int(_large_data(True)[1][n]) + 64
    declared = pack_pool.SRC_BYTES  # smaller than the tensor: a broken check stays inside it
    assert host[0].size >= declared + 64

    def out_of_range(index, at):
        bad = _patched(dev, src_offsets={i: declared - 10 for i in at},
                       lengths={i: 11 for i in at})   # one byte past
        _refused(cuda, N.BMQCRC_REC_PACK_SRC_RANGE, index, *host, kw, size=size, inputs=bad,
                 src_bytes=declared)

    # in the second tile of block 0, below one in block 1
    assert 1024 <= 1030 < per_block <= 2100
    out_of_range(1030, (1030, 2100))
    out_of_range(n - 1, (n - 1,))             # the last record of the last block
    # a length the DataHeader cannot hold, out of the source's range as well:
    # kind 1.  The call is refused before anything is read.
    bad = _patched(dev, lengths={200001: -(1 << 31)})   # 2^31 as the tensor's int32
    _refused(cuda, N.BMQCRC_REC_PACK_RECORD_TOO_BIG, 200001, *host, kw, size=size, inputs=bad,
             src_bytes=declared)
    assert np.array_equal(dev["src"].cpu().numpy(), host[0])
