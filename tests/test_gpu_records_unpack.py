"""Device-side walk of journal and DATA records (bmqcrc_message_records_unpack,
ABI 2.13) on the GPU.  The oracle throughout is tests/records_unpack_model.py.
Every raw call hands the library canary-filled output arrays with guard
elements behind msg_cap: the guards are checked after every call, the slots
the call leaves untouched after a successful one, and every element after a
refused one."""
import ctypes
import functools

import numpy as np
import pytest

from blazingmq_amd import (BmqCrcError, Crc32c, _native as N, last_copy, last_launch,
                           last_put_pack, last_put_unpack, last_records_pack,
                           last_records_unpack, pack_events, pack_records, unpack_events,
                           unpack_records)
from blazingmq_amd import storage as S
import device_views as V
import put_pack_model as P
import put_unpack_model as PU
import records_unpack_model as M
from records_pack_model import host_crcs, random_meta, wrap_partition

pytestmark = pytest.mark.gpu

GUARD = 8
SLACK = 64   # bytes kept behind every input buffer
CANARY = {"record_index": 0x5A5A5A5A, "app_offsets": 0x5A5A5A5A5A5A5A5A, "lengths": 0x5A5A5A5A,
          "queue_keys": 0xA5, "guids": 0xA5, "data_flags": 0xA5, "ref_counts": 0x5A5A5A5A,
          "timestamps": 0x5A5A5A5A5A5A5A5A, "expected": 0x5A5A5A5A, "out": 0x5A5A5A5A}
PER = {"record_index": 1, "app_offsets": 1, "lengths": 1, "queue_keys": 5, "guids": 16,
       "data_flags": 1, "ref_counts": 1, "timestamps": 1, "expected": 1, "out": 1}
PLACED = ("record_index", "queue_keys", "guids", "data_flags", "ref_counts", "timestamps")
KIND_NAME = {1: b"RECORD_HEADER", 2: b"MESSAGE_RECORD", 3: b"DATA_OFFSET", 4: b"DATA_RECORD",
             5: b"TOO_MANY_MESSAGES"}
KEY = b"\x11\x22\x33\x44\x55"


def _side_stream(cuda):
    """A stream of its own from the high-priority pool (the default pool's
    streams carry planner history that tests elsewhere rely on)."""
    import torch
    return torch.cuda.Stream(cuda, priority=-1)


def _t(cuda, a, dtype):
    import torch
    a = np.ascontiguousarray(a, dtype=dtype)
    if dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(cuda)


def _dev(cuda, buf, place=None, name=None):
    """`buf` on the device as a view of a longer allocation: one that starts
    with it, or with `place` (a device_views.Placer) one that holds it at the
    phase the placer has for `name`."""
    import torch
    buf = np.array(buf, dtype=np.uint8)  # (a copy: shared inputs are read-only)
    if place is not None:
        return place.put(name, buf)
    back = torch.full((buf.size + SLACK,), 0xEE, dtype=torch.uint8, device=cuda)
    back[:buf.size] = torch.from_numpy(buf).to(cuda)
    return back[:buf.size]


def _raw(cuda, run, data, pos, cap, select=None, verify=True, sync=True, stream=None, skip=(),
         place=None):
    """One bmqcrc_message_records_unpack over device tensors into canary-filled
    arrays.  Returns (rc, error text, result of the call or of
    bmqcrc_last_records_unpack, the arrays on the host with their guards).
    With `place` (a device_views.Placer that placed `run` and `data`) `select`
    and every array lie at the placer's phase for their names, and the sentinel
    margins around all of them are checked after the call."""
    import torch
    stream = stream or torch.cuda.current_stream(cuda)
    dt = {"record_index": torch.int32, "app_offsets": torch.int64, "lengths": torch.int32,
          "queue_keys": torch.uint8, "guids": torch.uint8, "data_flags": torch.uint8,
          "ref_counts": torch.int32, "timestamps": torch.int64, "expected": torch.int32,
          "out": torch.int32}
    with torch.cuda.stream(stream):
        if select is None:
            d_sel = None
        elif place is not None:
            d_sel = place.put("select", np.ascontiguousarray(select, dtype=np.uint8))
        else:
            d_sel = _t(cuda, select, np.uint8)
        arr = {}
        for name, t in dt.items():
            if name in skip or (name == "out" and not verify):
                continue
            if place is not None:
                arr[name] = place.fill(name, (cap + GUARD) * PER[name],
                                       {torch.int64: np.uint64, torch.int32: np.uint32,
                                        torch.uint8: np.uint8}[t], CANARY[name])
                continue
            fill = CANARY[name] - (1 << 64 if t == torch.int64 and CANARY[name] >> 63 else 0)
            arr[name] = torch.full(((cap + GUARD) * PER[name],), fill, dtype=t, device=cuda)
        p = N.RecordsUnpack()
        p.struct_size = ctypes.sizeof(N.RecordsUnpack)
        p.journal, p.journal_bytes = run.data_ptr(), run.numel()
        p.n_records = run.numel() // M.REC
        p.data, p.data_bytes, p.data_file_pos = data.data_ptr(), data.numel(), pos
        p.select = d_sel.data_ptr() if d_sel is not None else None
        p.msg_cap = cap
        for name, t in arr.items():
            setattr(p, name, t.data_ptr())
        o = N.make_opts(device=cuda.index, stream=stream.cuda_stream,
                        flags=N.BMQCRC_F_DEVICE_PTRS | (0 if sync else N.BMQCRC_F_ASYNC))
        r = N.RecordsUnpackResult()
        rc = N.lib.bmqcrc_message_records_unpack(ctypes.byref(p), ctypes.byref(r), ctypes.byref(o))
        err = N.lib.bmqcrc_last_error()
        res = r.as_dict() if sync else None
        if not sync:
            assert rc == 0, (rc, err)
            # written by a synchronous call only
            assert r.as_dict() == N.RecordsUnpackResult().as_dict()
            res = last_records_unpack(cuda.index, stream)
        host = {}
        for name, t in arr.items():
            a = t.cpu().numpy()
            host[name] = a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.itemsize])
        if place is not None:
            place.check()
    return rc, err, res, host


def _canary(name, a):
    return bool(np.all(a == CANARY[name]))


def _guards_intact(host, cap):
    for name, a in host.items():
        at = cap * PER[name]
        assert a.size == at + GUARD * PER[name] and _canary(name, a[at:]), name


def _ok(cuda, run, data, pos=0, select=None, cap=None, verify=True, sync=True, stream=None,
        model=None, n_bad=0, first_bad=None, skip=(), phases=None):
    """A call over host bytes that must succeed, against the model.  `phases`
    maps every pointer of the call (journal, data, select and the arrays by
    name) to the phase of its base; None: every buffer starts its allocation.
    Returns (model, arrays)."""
    place = V.Placer(cuda, phases) if phases is not None else None
    m = model or M.model(run, data, pos, select)
    assert m["refused"] is None
    n = m["n"]
    cap = n + 5 if cap is None else cap
    rc, err, res, host = _raw(cuda, _dev(cuda, run, place, "journal"),
                              _dev(cuda, data, place, "data"), pos, cap, select, verify, sync,
                              stream, skip, place)
    assert rc == 0, (rc, err)
    assert res == dict(n_records=m["n_records"], n_msgs=n, n_skipped=m["n_skipped"], n_bad=n_bad,
                       first_bad=n if first_bad is None else first_bad, refused_kind=0,
                       refused_index=0), res
    _guards_intact(host, cap)
    for name in M.FIELDS:
        if name in host:
            k = n * PER[name]
            assert np.array_equal(host[name][:k].astype(np.uint64),
                                  m[name].reshape(-1).astype(np.uint64)), name
    for name in PLACED:  # untouched where no message is
        if name in host:
            assert _canary(name, host[name][n * PER[name]:]), name
    if "out" in host and n_bad == 0:
        assert np.array_equal(host["out"][:n], m["crcs"])
    return m, host


def _refused(cuda, run, data, pos=0, cap=None, select=None, want=None, verify=True,
             phases=None):
    """A call that must be refused, synchronously and asynchronously: the
    model's (kind, record), and not one element written.  `phases`: as in _ok."""
    place = V.Placer(cuda, phases) if phases is not None else None
    kind, index = want or M.model(run, data, pos, select, cap, crcs=False)["refused"]
    cap = run.size // M.REC if cap is None else cap
    d_run, d_data = _dev(cuda, run, place, "journal"), _dev(cuda, data, place, "data")
    for sync in (True, False):
        rc, err, res, host = _raw(cuda, d_run, d_data, pos, cap, select, verify, sync,
                                  place=place)
        if sync:
            assert rc == N.BMQCRC_EINVAL and KIND_NAME[kind] in err and \
                b"nothing was written" in err, (rc, err)
            assert (b"record %d " % index) in err, err
        assert res == dict(n_records=run.size // M.REC, n_msgs=0, n_skipped=0, n_bad=0,
                           first_bad=0, refused_kind=kind, refused_index=index), (sync, res)
        for name, a in host.items():
            assert _canary(name, a), (sync, name)
    return kind, index


@functools.lru_cache(maxsize=None)
def _base():
    """(record run without the CREATION record, DATA file): 2,200 messages of
    0..120 bytes with CONFIRM and SYNCPOINT records among them, more than
    2,049 records in all.  Shared, never modified: callers copy."""
    rng = np.random.default_rng(2049)
    j, d = M.build_partition(rng, rng.integers(0, 121, size=2200), others=0.3)
    run = j[M.JH + M.REC:]
    assert run.size // M.REC > 2049
    run.setflags(write=False)
    d.setflags(write=False)
    return run, d


def _put32(buf, where, v):
    buf[where:where + 4] = np.frombuffer(int(v).to_bytes(4, "big"), np.uint8)


# ---- round trip --------------------------------------------------------------

def test_round_trip_with_the_packer(cuda):
    import torch
    rng = np.random.default_rng(41)
    lens = np.concatenate([np.arange(64), rng.integers(0, 5001, size=30)]).astype(np.uint32)
    assert set((12 + lens.astype(np.int64)) % 8) == set(range(8))  # all 8 padding residues
    rng.shuffle(lens)
    n = lens.size
    soff = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    src = rng.integers(0, 256, size=int(lens.sum()), dtype=np.uint8)
    qkeys, guids = random_meta(rng, n)
    refs = rng.integers(0, 1 << 20, size=n).astype(np.uint32)
    stamps = rng.integers(0, 1 << 63, size=n).astype(np.int64)
    dflags = rng.integers(0, 256, size=n).astype(np.uint8)
    kw = dict(file_key=KEY, lease_id=7, first_seq=(1 << 32) + 5, data_file_pos=40)
    dst, jour, roff, crcs, _ = pack_records(
        _t(cuda, src, np.uint8), _t(cuda, soff, np.int64), _t(cuda, lens, np.uint32),
        _t(cuda, qkeys, np.uint8), _t(cuda, guids, np.uint8), ref_counts=_t(cuda, refs, np.uint32),
        timestamps=_t(cuda, stamps, np.int64), data_flags=_t(cuda, dflags, np.uint8), **kw)
    want = host_crcs(src, soff, lens)
    u = unpack_records(jour, dst, data_file_pos=40)
    res = last_records_unpack(cuda.index, torch.cuda.current_stream(cuda))
    assert res == dict(n_records=n, n_msgs=n, n_skipped=0, n_bad=0, first_bad=n, refused_kind=0,
                       refused_index=0)
    assert np.array_equal(u.record_index.cpu().numpy(), np.arange(n))
    assert np.array_equal(u.app_offsets.cpu().numpy(), roff.cpu().numpy()[:-1] + 12)
    assert np.array_equal(u.lengths.cpu().numpy().view(np.uint32), lens)
    assert np.array_equal(u.queue_keys.cpu().numpy(), qkeys) and u.queue_keys.shape == (n, 5)
    assert np.array_equal(u.guids.cpu().numpy(), guids) and u.guids.shape == (n, 16)
    assert np.array_equal(u.data_flags.cpu().numpy(), dflags)
    assert np.array_equal(u.ref_counts.cpu().numpy().view(np.uint32), refs)
    assert np.array_equal(u.timestamps.cpu().numpy(), stamps)
    assert np.array_equal(u.expected.cpu().numpy().view(np.uint32), want)
    assert np.array_equal(u.crcs.cpu().numpy().view(np.uint32), want)
    assert np.array_equal(crcs.cpu().numpy().view(np.uint32), want)
    dst2, jour2, roff2, _, res2 = pack_records(
        dst, u.app_offsets, u.lengths, u.queue_keys, u.guids, ref_counts=u.ref_counts,
        timestamps=u.timestamps, data_flags=u.data_flags, expected=u.expected, **kw)
    assert torch.equal(dst2, dst) and torch.equal(jour2, jour) and torch.equal(roff2, roff)
    assert res2["n_bad"] == 0
    # and the canary form of the same call, against the model
    _ok(cuda, jour.cpu().numpy(), dst.cpu().numpy(), pos=40)


# ---- wave, block and grid edges ----------------------------------------------

@pytest.mark.parametrize("count", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_record_counts(cuda, count):
    run, d = _base()
    m, _ = _ok(cuda, run[:M.REC * count], d, cap=None)
    assert 0 < m["n"] <= count and (count < 64 or m["n"] < count)  # other types among them


def test_more_records_than_one_step_of_the_layout_grid(cuda):
    # above 256 x 1,024 records a block owns more than one tile of 1,024: the
    # first 2,049 records 129 times over (the call checks no sequence numbers)
    run, d = _base()
    k, reps = 2049, 129
    assert k * reps > 256 * 1024
    small = M.model(run[:M.REC * k], d)
    n = small["n"] * reps
    model = dict(refused=None, n_records=k * reps, n=n, n_skipped=0)
    for name in M.FIELDS + ("crcs",):
        a = small[name]
        model[name] = np.concatenate([a] * reps)
    model["record_index"] = (np.tile(small["record_index"], reps).astype(np.uint64) +
                             np.repeat(np.arange(reps, dtype=np.uint64) * k,
                                       small["n"])).astype(np.uint32)
    _ok(cuda, np.tile(run[:M.REC * k], reps), d, model=model, cap=n)


def test_more_messages_than_one_step_of_the_publish_grid(cuda):
    # above 2,048 x 256 messages a publish thread copies a second slot, and with
    # msg_cap 300,000 above the count a placing thread empties a second one: a
    # message-only run of 2,049 records 257 times over, all over one DATA window
    rng = np.random.default_rng(48)
    k, reps = 2049, 257
    assert k * reps > 2048 * 256
    j, d = M.build_partition(rng, rng.integers(0, 24, size=k), others=0.0)
    run = j[M.JH + M.REC:]
    small = M.model(run, d)
    assert small["n"] == small["n_records"] == k
    n = k * reps
    model = dict(refused=None, n_records=n, n=n, n_skipped=0)
    for name in M.FIELDS + ("crcs",):
        model[name] = np.concatenate([small[name]] * reps)
    model["record_index"] = np.arange(n, dtype=np.uint32)
    tiled = np.tile(run, reps)
    _, exact = _ok(cuda, tiled, d, model=model, cap=n)
    # more than one step of the placing grid of empty slots behind the messages
    _, wide = _ok(cuda, tiled, d, model=model, cap=n + 300000)
    for name, a in exact.items():
        assert np.array_equal(wide[name][:n * PER[name]], a[:n * PER[name]]), name
    # one wrong stored CRC in the second step
    victim = 2048 * 256 + 1000
    tiled[M.REC * victim + 55] ^= 0x01
    wrong = dict(model, expected=model["expected"].copy())
    wrong["expected"][victim] ^= 1
    _, host = _ok(cuda, tiled, d, model=wrong, cap=n, n_bad=1, first_bad=victim)
    assert np.array_equal(host["out"][:n], model["crcs"])


def test_no_message_record_and_msg_cap_0(cuda):
    w = S.PartitionWriter(lease_id=2)
    w.queue_op(S.OP_CREATION, S.DEFAULT_QUEUE_KEY)
    for i in range(70):
        if i % 3:
            w.confirm(bytes([i + 1] * 16), S.DEFAULT_QUEUE_KEY)
        else:
            w.sync_point()
    j, d = w.files()
    for verify in (True, False):
        m, _ = _ok(cuda, j[M.JH:], d, cap=0, verify=verify)
        assert m["n"] == 0 and m["n_records"] == 71


def test_message_only_run(cuda):
    rng = np.random.default_rng(42)
    j, d = M.build_partition(rng, rng.integers(0, 700, size=130), others=0.0)
    m, _ = _ok(cuda, j[M.JH + M.REC:], d, cap=130)
    assert m["n"] == m["n_records"] == 130


def test_one_long_message_among_short_ones(cuda):
    rng = np.random.default_rng(43)
    j, d = M.build_partition(rng, [3, 100, 2 << 20, 0, 17], others=0.5)
    m, _ = _ok(cuda, j[M.JH:], d)
    assert list(m["lengths"]) == [3, 100, 2 << 20, 0, 17]


def test_data_headers_with_options_and_other_header_sizes(cuda):
    rng = np.random.default_rng(44)
    j, d = M.build_partition(rng, rng.integers(0, 200, size=150), variants=True)
    m, _ = _ok(cuda, j[M.JH:], d)
    gap = m["app_offsets"].astype(np.int64)[1:] - m["app_offsets"].astype(np.int64)[:-1]
    assert m["n"] == 150 and len(set(int(g) % 8 for g in gap)) > 1  # not all 12-byte headers


def test_window_at_the_top_of_the_data_file(cuda):
    # MessageOffsetDwords close to 2^32: o = 8 x dwords needs 35 bits, and the
    # window coordinates are differences of such numbers
    rng = np.random.default_rng(45)
    pos = 8 * (2 ** 32 - 1) - 4096
    lens = np.array([0, 1, 4, 11, 12, 13, 100, 333, 1000], np.uint32)
    R = ((lens.astype(np.int64) + 12) // 8 + 1) * 8
    lens = np.append(lens, 4096 - int(R.sum()) - 12 - 4).astype(np.uint32)  # the last ends at 4,096
    n = lens.size
    soff = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    src = rng.integers(0, 256, size=int(lens.sum()), dtype=np.uint8)
    qkeys, guids = random_meta(rng, n)
    dst, jour, roff, _, res = pack_records(
        _t(cuda, src, np.uint8), _t(cuda, soff, np.int64), _t(cuda, lens, np.uint32),
        _t(cuda, qkeys, np.uint8), _t(cuda, guids, np.uint8), file_key=KEY, lease_id=1,
        first_seq=1, data_file_pos=pos)
    assert res["data_bytes"] == dst.numel() == 4096
    run, data = jour.cpu().numpy(), dst.cpu().numpy()
    assert int.from_bytes(run[32:36].tobytes(), "big") * 8 == pos
    m, _ = _ok(cuda, run, data, pos=pos, cap=n)
    assert np.array_equal(m["lengths"], lens)
    assert np.array_equal(m["app_offsets"], roff.cpu().numpy()[:-1].astype(np.uint64) + 12)
    # one dword lower and the first record lies below the window; a window
    # shorter by 8 bytes ends before the last record does
    assert _refused(cuda, run, data, pos=pos + 8) == (M.K_OFFSET, 0)
    assert _refused(cuda, run, data[:-8], pos=pos) == (M.K_DATA, n - 1)


# ---- select ------------------------------------------------------------------

def test_select(cuda):
    run, d = _base()
    run, d = run[:M.REC * 300].copy(), d.copy()
    msgs = M.message_records(run)
    out = msgs[[0, 5, 64, len(msgs) - 1]]
    sel = np.ones(300, np.uint8)
    sel[out] = 0
    sel[np.setdiff1d(np.arange(300), msgs)[:7]] = 0   # other record types: select is ignored
    for r in out:  # their DATA records become garbage
        o = 8 * int.from_bytes(run[M.REC * r + 32:M.REC * r + 36].tobytes(), "big")
        d[o:o + 8] = 0xFF
    assert M.model(run, d, crcs=False)["refused"] == (M.K_DATA, int(out[0]))
    m, host = _ok(cuda, run, d, select=sel)
    assert m["n"] == len(msgs) - 4 and m["n_skipped"] == 4
    assert not set(out) & set(host["record_index"][:m["n"]])
    _refused(cuda, run, d, want=(M.K_DATA, int(out[0])))
    # an unselected record is still checked up to its data offset
    bad = run.copy()
    _put32(bad, M.REC * int(out[2]) + 32, 0)
    assert _refused(cuda, bad, d, select=sel) == (M.K_OFFSET, int(out[2]))
    bad = run.copy()
    bad[M.REC * int(out[1]) + 36:M.REC * int(out[1]) + 52] = 0
    assert _refused(cuda, bad, d, select=sel) == (M.K_MESSAGE, int(out[1]))


# ---- refusals ----------------------------------------------------------------

@pytest.mark.parametrize("name", M.VARIANTS)
def test_malformed_input_is_refused_like_the_model(cuda, name):
    j, d, last = M.malformed(name)
    kind, index = _refused(cuda, j[M.JH:], d)
    assert index == last and kind == M.VARIANT_KIND.get(name, M.K_DATA)


@pytest.mark.parametrize("what", ["type", "lease", "seq", "magic"])
def test_record_header_is_checked_on_every_record_type(cuda, what):
    run, d = _base()
    run = run[:M.REC * 200].copy()
    r = int(np.setdiff1d(np.arange(200), M.message_records(run))[3])  # a CONFIRM or SYNCPOINT
    at = M.REC * r
    if what == "type":
        run[at] &= 0x0F
    elif what == "lease":
        run[at + 8:at + 12] = 0
    elif what == "seq":
        run[at + 2:at + 8] = 0
    else:
        run[at + 57] ^= 0x20
    assert _refused(cuda, run, d) == (M.K_HEADER, r)


def test_refusal_precedence(cuda):
    run, d = _base()
    run, d = run[:M.REC * 2100].copy(), d.copy()
    msgs = M.message_records(run)
    lo, mid, hi = int(msgs[3]), int(msgs[msgs >= 1100][0]), int(msgs[msgs >= 2050][0])
    assert lo < 1024 <= mid < 2048 <= hi  # three blocks of the layout grid
    o = 8 * int.from_bytes(run[M.REC * lo + 32:M.REC * lo + 36].tobytes(), "big")
    d[o] &= 0x1F                                        # kind 4, the lowest record
    run[M.REC * hi + 22:M.REC * hi + 27] = 0            # kind 2, the highest
    _put32(run, M.REC * mid + 32, 0)                    # kind 3 between them
    assert _refused(cuda, run, d) == (M.K_MESSAGE, hi)  # the lower kind at the higher index
    run[M.REC * mid + 36:M.REC * mid + 52] = 0          # kind 2 at a lower index
    assert _refused(cuda, run, d) == (M.K_MESSAGE, mid)
    assert _refused(cuda, run, d, cap=1) == (M.K_MESSAGE, mid)  # before TOO_MANY_MESSAGES
    run[M.REC * 2000 + 59] ^= 1                         # kind 1 beats them all
    assert _refused(cuda, run, d) == (M.K_HEADER, 2000)


def test_msg_cap_edge(cuda):
    run, d = _base()
    run = run[:M.REC * 1500]
    msgs = M.message_records(run)
    n = len(msgs)
    _ok(cuda, run, d, cap=n)
    _ok(cuda, run, d, cap=n + 5)
    assert _refused(cuda, run, d, cap=n - 1) == (M.K_MANY, int(msgs[-1]))
    assert _refused(cuda, run, d, cap=700) == (M.K_MANY, int(msgs[700]))
    assert _refused(cuda, run, d, cap=0, verify=False) == (M.K_MANY, int(msgs[0]))


def test_python_wrapper_raises_and_reports(cuda):
    import torch
    j, d, last = M.malformed("padding_9")
    run, data = _dev(cuda, j[M.JH:]), _dev(cuda, d)
    with pytest.raises(BmqCrcError, match="BMQCRC_REC_UNPACK_DATA_RECORD") as e:
        unpack_records(run, data, data_file_pos=0)
    assert e.value.rc == N.BMQCRC_EINVAL
    s = _side_stream(cuda)
    with torch.cuda.stream(s):
        u = unpack_records(run, data, data_file_pos=0, msg_cap=32, stream=s, sync=False)
        assert u.lengths.numel() == 32 and u.guids.shape == (32, 16) and \
            u.queue_keys.shape == (32, 5)
        res = last_records_unpack(cuda.index, s)
    assert (res["refused_kind"], res["refused_index"]) == (M.K_DATA, last)
    good = M.malformed("padding_9")[1].copy()
    good[-1] = 4
    u = unpack_records(run, _dev(cuda, good), data_file_pos=0, verify=False)
    assert u.crcs is None and u.lengths.numel() == 5  # msg_cap None: the record count, sliced


# ---- verify ------------------------------------------------------------------

def test_verify_counts_a_corrupt_payload_and_a_corrupt_stored_crc(cuda):
    run, d = _base()
    run, d = run[:M.REC * 400].copy(), d.copy()
    good = M.model(run, d)
    n = good["n"]
    a = next(i for i in range(70, n) if good["lengths"][i] > 0)
    b = n - 1
    d[int(good["app_offsets"][a])] ^= 0x10
    run[M.REC * int(good["record_index"][b]) + 55] ^= 0x01
    m, host = _ok(cuda, run, d, n_bad=2, first_bad=a)
    assert list(np.nonzero(host["out"][:n] != host["expected"][:n])[0]) == [a, b]
    assert np.array_equal(host["out"][:n], m["crcs"])
    assert host["out"][b] == good["crcs"][b] and host["expected"][b] == good["crcs"][b] ^ 1


def test_walk_only_leaves_the_launch_record(cuda):
    import torch
    run, d = _base()
    run, d = run[:M.REC * 200], d.copy()
    d[int(M.model(run, d, crcs=False)["app_offsets"][5])] ^= 1
    s = _side_stream(cuda)
    with torch.cuda.stream(s):
        arena = _t(cuda, d, np.uint8)
        Crc32c.calculate_batch(arena, _t(cuda, [0, 64], np.int64), _t(cuda, [64, 100], np.uint32),
                               stream=s, seg_bytes=1024)
        before = last_launch(cuda.index, s, offsets=True)
        _ok(cuda, run, d, verify=False, stream=s)  # n_bad == 0: nothing was compared
        assert last_launch(cuda.index, s, offsets=True) == before


# ---- state -------------------------------------------------------------------

def test_state(cuda):
    import torch
    rng = np.random.default_rng(46)
    host = rng.integers(0, 256, size=1 << 18, dtype=np.uint8)
    arena = torch.from_numpy(host).to(cuda)
    lens = rng.integers(1, 1025, size=3001).astype(np.uint32)
    offs = (rng.random(lens.size) * (host.size - 1100)).astype(np.int64)
    d_off, d_len = _t(cuda, offs, np.int64), _t(cuda, lens, np.uint32)
    doff = _t(cuda, np.concatenate([[0], np.cumsum(lens[:40])[:-1]]), np.int64)
    copy_dst = torch.zeros(int(lens[:40].sum()) + 16, dtype=torch.uint8, device=cuda)
    qids, guids, flags = P.random_meta(rng, 30)
    buf, evoffs = PU.concat([PU.build_event(rng, rng.integers(0, 300, size=50))
                             for _ in range(2)])
    run, d = _base()
    run = run[:M.REC * 500]
    s = _side_stream(cuda)
    with torch.cuda.stream(s):
        Crc32c.copy_batch(arena, d_off[:40], d_len[:40], copy_dst, doff, stream=s)
        pack_events(arena, d_off[:30], d_len[:30], _t(cuda, qids, np.int32),
                    _t(cuda, guids, np.uint8), _t(cuda, flags, np.uint8), stream=s)
        pack_records(arena, d_off[:30], d_len[:30],
                     _t(cuda, np.full((30, 5), 7), np.uint8), _t(cuda, guids, np.uint8),
                     file_key=KEY, lease_id=3, first_seq=2, data_file_pos=40, stream=s)
        unpack_events(_dev(cuda, buf), _t(cuda, evoffs, np.int64), stream=s)
        put, rec = last_put_pack(cuda.index, s), last_records_pack(cuda.index, s)
        unp = last_put_unpack(cuda.index, s)
        assert unp["n_msgs"] == 100
        # none yet on s
        assert last_records_unpack(cuda.index, s) == N.RecordsUnpackResult().as_dict()
        _ok(cuda, run, d, stream=s)
        _ok(cuda, run, d, stream=s, sync=False)
        assert last_copy(cuda.index, s) == (40, 0, 40)
        assert last_put_pack(cuda.index, s) == put
        assert last_records_pack(cuda.index, s) == rec
        assert last_put_unpack(cuda.index, s) == unp
        plan = last_launch(cuda.index, s, offsets=True)
        # a planned batch: planner and fold, nothing speculated, 64-bit offsets
        assert plan["kernels"] >= 2 and plan["spec"] == 0 and plan["offset_bits"] == 64, plan
        out = Crc32c.calculate_batch(arena, d_off, d_len, stream=s)
    s.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), P.host_crcs(host, offs, lens))


# ---- the loop closed on the device -------------------------------------------

def test_put_events_to_a_partition_verified_on_the_device(cuda):
    import torch
    rng = np.random.default_rng(47)
    n = 300
    key = bytes([9, 8, 7, 6, 5])
    buf, evoffs = PU.concat([PU.build_event(rng, rng.integers(0, 120, size=100))
                             for _ in range(3)])
    pm = PU.model(buf, evoffs)
    victim = next(i for i in range(100, n) if pm["lengths"][i] > 0)
    kw = dict(file_key=KEY, lease_id=1, first_seq=2, data_file_pos=40, timestamp=0x6720EAB4)
    cur = torch.cuda.current_stream(cuda)
    for corrupt in (False, True):
        ev = buf.copy()
        if corrupt:
            ev[int(pm["app_offsets"][victim])] ^= 0x40
        events = _dev(cuda, ev)
        u = unpack_events(events, _t(cuda, evoffs, np.int64), msg_cap=n)
        qkeys = torch.from_numpy(np.frombuffer(key, np.uint8).copy()).to(cuda).repeat(n, 1)
        dst, jour, _, _, _ = pack_records(events, u.app_offsets, u.lengths, qkeys, u.guids,
                                          expected=u.expected, **kw)
        r = unpack_records(jour, dst, data_file_pos=40, msg_cap=n)
        res = last_records_unpack(cuda.index, cur)
        assert (res["n_msgs"], res["n_bad"], res["refused_kind"]) == (n, int(corrupt), 0)
        jf, df = wrap_partition(dst.cpu().numpy(), jour.cpu().numpy(),
                                np.frombuffer(key, np.uint8))
        got = S.verify_partition(jf, df)
        assert (got["recovery_rc"], got["n_messages"], got["n_bad"]) == (0, n, res["n_bad"])
        if corrupt:
            assert res["first_bad"] == victim
            index = int(r.record_index[res["first_bad"]].item())
            assert list(got["bad_record_offsets"]) == [44 + 60 * (1 + index)]
        else:
            assert res["first_bad"] == n
