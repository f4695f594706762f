"""A device-resident partition rolled over on the GPU
(bmqcrc_partition_rollover, ABI 2.18).  The oracle throughout is
tests/rollover_model.py.  Every raw call hands the library sentinel-filled
destinations and output arrays with guard bytes and elements behind them: the
guards are checked after every call, and every byte and element after a refused
one."""
import ctypes
import functools

import numpy as np
import pytest

from blazingmq_amd import (BmqCrcError, Crc32c, _native as N, apply_events, last_copy,
                           last_journal_select, last_launch, last_push_pack, last_put_pack,
                           last_put_unpack, last_records_pack, last_records_unpack,
                           last_rollover, last_storage_apply, last_storage_pack, pack_events,
                           pack_push_events, pack_records, pack_storage_events,
                           rollover_records, select_records, unpack_events, unpack_records)
from blazingmq_amd import storage as S
from blazingmq_amd import synth
import device_views as V
import join_collisions as J
import put_pack_model as P
import put_unpack_model as PU
import rollover_cases as C
import rollover_model as M
import test_grid_regimes as G
from records_pack_model import random_meta

pytestmark = pytest.mark.gpu

GUARD = 8      # elements behind every output array
SLACK = 64     # bytes behind every input buffer and both destinations
SENTINEL = 0xC3
JH = S.PartitionWriter.JOURNAL_HEADER
CANARY = {"new_index": 0x5A5A5A5A, "out": 0xA5A5A5A5}
KINDS = ("OK", "RECORD_HEADER", "KEEP_JOURNAL_OP", "SYNC_POINT", "DATA_OFFSET", "DATA_RECORD",
         "DST_TOO_SMALL", "DATA_FILE_FULL", "TOO_MANY_PIECES")
KIND_NAME = {k: ("BMQCRC_ROLLOVER_" + n).encode() for k, n in enumerate(KINDS) if k}
CRC = Crc32c.calculate
QK, QK2 = S.DEFAULT_QUEUE_KEY, b"\x26\xda\xcd\xc9\x75"
# the base pointers the ABI permits: 4-byte ones at +4, 8-byte ones at +8, bytes at +1
PHASES = {"journal": 4, "journal_dst": 4, "data": 8, "dst": 8, "keep": 1, "new_index": 4,
          "out": 4}


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


def _kw(**changes):
    """Keywords of a call over the whole DATA file into destinations of the
    exact size (the model refuses smaller ones)."""
    kw = dict(data_file_pos=0, new_data_file_pos=40, keep=None, confirm_mode=0, sync_point=None,
              timestamp=C.TIMESTAMP, dst_bytes=None, journal_dst_bytes=None)
    kw.update(changes)
    return kw


def _filled(cuda, place, name, count, dt, value):
    import torch
    if place is not None:
        return place.fill(name, count, dt, value)
    fill = np.array([value], np.uint64).astype(dt)
    return torch.from_numpy(np.repeat(fill, count).view(
        {np.uint32: np.int32}.get(dt, dt))).to(cuda)


def _raw(cuda, run, data, kw, sync=True, stream=None, skip=(), phases=None):
    """One bmqcrc_partition_rollover over device tensors into sentinel-filled
    destinations and arrays.  Returns (rc, error text, result of the call or of
    bmqcrc_last_rollover, everything written on the host with its guards).
    `phases` maps every pointer of the call to the phase of its base; the
    sentinel margins around each are checked after the call.  None: every
    buffer starts its allocation."""
    import torch
    place = V.Placer(cuda, phases) if phases is not None else None
    stream = stream or torch.cuda.current_stream(cuda)
    n = len(run) // 60
    with torch.cuda.stream(stream):
        d_run, d_data = _dev(cuda, run, place, "journal"), _dev(cuda, data, place, "data")
        d_keep = _dev(cuda, kw["keep"], place, "keep") if kw["keep"] is not None else None
        arr = {"dst": _filled(cuda, place, "dst", kw["dst_bytes"] + SLACK, np.uint8, SENTINEL),
               "journal_dst": _filled(cuda, place, "journal_dst", kw["journal_dst_bytes"] + SLACK,
                                      np.uint8, SENTINEL)}
        for name in CANARY:
            if name not in skip:
                arr[name] = _filled(cuda, place, name, n + GUARD, np.uint32, CANARY[name])
        # (an empty tensor has no address: the call wants one)
        spare = torch.zeros(8, dtype=torch.uint8, device=cuda)
        p = N.Rollover()
        p.struct_size = ctypes.sizeof(N.Rollover)
        p.journal, p.journal_bytes = d_run.data_ptr() or spare.data_ptr(), d_run.numel()
        p.n_records = n
        p.data, p.data_bytes = d_data.data_ptr() or spare.data_ptr(), d_data.numel()
        p.data_file_pos, p.new_data_file_pos = kw["data_file_pos"], kw["new_data_file_pos"]
        p.keep = d_keep.data_ptr() if d_keep is not None and n else None
        p.confirm_mode, p.timestamp = kw["confirm_mode"], kw["timestamp"]
        p.sync_point = N.BMQCRC_ROLLOVER_NO_SYNC_POINT if kw["sync_point"] is None \
            else kw["sync_point"]
        p.dst, p.dst_bytes = arr["dst"].data_ptr(), kw["dst_bytes"]
        p.journal_dst, p.journal_dst_bytes = arr["journal_dst"].data_ptr(), kw["journal_dst_bytes"]
        for name in CANARY:
            setattr(p, name, arr[name].data_ptr() if name in arr else None)
        o = N.make_opts(device=cuda.index, stream=stream.cuda_stream,
                        flags=N.BMQCRC_F_DEVICE_PTRS | (0 if sync else N.BMQCRC_F_ASYNC))
        r = N.RolloverResult()
        rc = N.lib.bmqcrc_partition_rollover(ctypes.byref(p), ctypes.byref(r), ctypes.byref(o))
        err = N.lib.bmqcrc_last_error()
        res = r.as_dict() if sync else last_rollover(cuda.index, stream)
        host = {name: t.cpu().numpy() for name, t in arr.items()}
        if place is not None:
            place.check()
    for name in CANARY:
        if name in host:
            host[name] = host[name].view(np.uint32)
    return rc, err, res, host


def _untouched(name, a):
    return bool((a == (CANARY[name] if name in CANARY else SENTINEL)).all())


def _check(cuda, run, data, kw, sync=True, stream=None, skip=(), phases=None, model=None):
    """The call against the model: a refusal identical and nothing written, or
    every destination byte, array entry and result field.  `dst_bytes` /
    `journal_dst_bytes` None is the exact size.  `model` is M.rollover's answer
    to this very call when the caller has it already (a size left None: its
    answer with room to spare); the model is not run then.  Returns (model,
    host)."""
    kw = dict(kw)
    exact = [k for k in ("dst_bytes", "journal_dst_bytes") if kw[k] is None]
    if model is not None:
        for k in exact:
            kw[k] = model.result[{"dst_bytes": "data_bytes",
                                  "journal_dst_bytes": "journal_bytes"}[k]] \
                if isinstance(model, M.Rolled) else 4096
    elif exact:
        big = dict(kw)
        big.update({k: 1 << 40 for k in exact})
        m = M.rollover(run, data, crc32c=CRC, **big)
        for k in exact:
            kw[k] = m.result[{"dst_bytes": "data_bytes", "journal_dst_bytes": "journal_bytes"}[k]] \
                if isinstance(m, M.Rolled) else 4096
    m = model if model is not None else M.rollover(run, data, crc32c=CRC, **kw)
    rc, err, res, host = _raw(cuda, run, data, kw, sync=sync, stream=stream, skip=skip,
                              phases=phases)
    n = len(run) // 60
    if isinstance(m, M.Refusal):
        if sync:
            assert rc == N.BMQCRC_EINVAL and KIND_NAME[m.kind] in err, (rc, err, m)
            assert b"nothing was written" in err and (b"%d" % m.index) in err, (err, m)
        else:
            assert rc == 0, err
        assert res == M.refused_result(m, n), (res, m)
        for name, a in host.items():
            assert _untouched(name, a), name
        return m, host
    assert rc == 0, err
    assert res == m.result, (res, m.result)
    for name, want in (("dst", m.data), ("journal_dst", m.journal), ("new_index", m.new_index),
                       ("out", m.crcs)):
        if name in skip:
            continue
        assert np.array_equal(host[name][:len(want)], want), name
        assert _untouched(name, host[name][len(want):]), name
    return m, host


@functools.lru_cache(maxsize=None)
def _records(n, seed=7, options=False, lengths=None, confirm_every=3):
    """(record run of n records, DATA file): two queues' CREATIONs, then
    messages of 0..40 bytes (or of `lengths`, in turn) alternating between the
    queues, every third (every `confirm_every`-th) followed by its CONFIRM,
    every third of those by its DELETION too, in front of every 16th a queue
    ADDITION, PURGE or DELETION or a sync point; with `options` DATA headers of
    3 and 5 words with 0..2 option words.  Shared, never modified."""
    rng = np.random.default_rng(seed)
    w = S.PartitionWriter(lease_id=4, partition_id=1)
    w.queue_op(S.OP_CREATION, QK)
    if n > 1:
        w.queue_op(S.OP_CREATION, QK2)
    k = specials = 0
    while len(w.recs) < n:
        if k % 16 == 15 and specials == k // 16:
            if specials % 4 == 3:
                w.sync_point()
            else:
                w.queue_op((S.OP_ADDITION, S.OP_PURGE, S.OP_DELETION)[specials % 4], QK,
                           b"\1\2\3\4\5")
            specials += 1
            continue
        size = int(rng.integers(0, 41)) if lengths is None else lengths[k % len(lengths)]
        app = rng.integers(0, 256, size=size, dtype=np.uint8).tobytes()
        before = w.dpos
        key = (QK, QK2)[k & 1]
        _, guid = w.message(app, key, data_flags=k & 0xFF)
        if options:
            hw, opt = (3, 5)[int(rng.integers(0, 2))], int(rng.integers(0, 3))
            lead = 4 * (hw + opt)
            total = (lead + len(app)) // 8 * 8 + 8
            pad = total - lead - len(app)
            w.data[-1] = (((hw << 29) | (total // 4)).to_bytes(4, "big") +
                          ((opt << 8) | (k & 0xFF)).to_bytes(4, "big") +
                          bytes(rng.integers(0, 256, size=lead - 8, dtype=np.uint8)) + app +
                          bytes([pad]) * pad)
            w.dpos = before + total
        if k % confirm_every == 0 and len(w.recs) < n:
            w.confirm(guid, key)
        if k % (3 * confirm_every) == 0 and len(w.recs) < n:
            w.deletion(guid, key)
        k += 1
    j, d = w.files()
    run = j[JH:]
    run.setflags(write=False)
    d.setflags(write=False)
    return run, d


def _types(run):
    return np.asarray(run).reshape(-1, 60)[:, 0] >> 4


def _keep(run, how):
    """keep[] over a run: JOURNAL_OP records are never asked for."""
    t = _types(run)
    n = t.size
    keep = {"all": np.ones(n, np.uint8), "none": np.zeros(n, np.uint8),
            "second": (np.arange(n) % 2).astype(np.uint8)}[how]
    keep[t == 5] = 0
    return keep


def _last_sync(run):
    s = np.flatnonzero(_types(run) == 5)
    return int(s[-1]) if s.size else None


# ---- wave, tile and grid edges -----------------------------------------------

@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 1023, 1025])
def test_record_counts(cuda, count, mode):
    run, d = _records(1025)
    run = run[:60 * count]
    m, _ = _check(cuda, run, d, _kw(confirm_mode=mode, sync_point=_last_sync(run)))
    assert m.result["n_records"] == count


@pytest.mark.parametrize("how", ["all", "none", "second", None])
@pytest.mark.parametrize("mode", [0, 1])
def test_three_thousand_mixed_records(cuda, how, mode):
    # three layout blocks: both block prefixes cross blocks
    run, d = _records(3000, seed=11)
    assert set(_types(run).tolist()) == {1, 2, 3, 4, 5}
    keep = _keep(run, how) if how else None
    m, _ = _check(cuda, run, d, _kw(keep=keep, confirm_mode=mode, sync_point=_last_sync(run),
                                    new_data_file_pos=4096))
    if how == "none":
        assert m.result["n_kept"] == 0 and m.result["journal_bytes"] == 60
    elif how != "second":
        assert m.result["n_messages"] == int((_types(run) == 1).sum())


def test_application_data_lengths_and_padding(cuda):
    # 0 and 1..17 (every padding value 1..8 and the copy's tails), 255..257,
    # 64 KiB, and 300 KiB + 3: the copy's long path
    lengths = tuple(range(18)) + (255, 256, 257, 64 * 1024, 300 * 1024 + 3)
    run, d = _records(46, seed=9, lengths=lengths)
    m, _ = _check(cuda, run, d, _kw(new_data_file_pos=48))
    assert m.result["n_messages"] >= len(lengths) and m.result["n_bad"] == 0
    pads = set()
    for i in np.flatnonzero(_types(run) == 1):
        o = 8 * int.from_bytes(run[60 * i + 32:60 * i + 36].tobytes(), "big")
        pads.add(int(d[o + 4 * (int.from_bytes(d[o:o + 4].tobytes(), "big") & 0x1FFFFFFF) - 1]))
    assert pads == set(range(1, 9))


def test_option_words_and_header_sizes(cuda):
    run, d = _records(700, seed=8, options=True)
    m, _ = _check(cuda, run, d, _kw(keep=_keep(run, "second"), confirm_mode=1))
    leads = set()
    for i in np.flatnonzero(m.crcs != 0):
        o = 8 * int.from_bytes(run[60 * i + 32:60 * i + 36].tobytes(), "big")
        leads.add(4 * ((int(d[o]) >> 5) + int.from_bytes(d[o + 4:o + 7].tobytes(), "big")))
    assert leads == {12, 16, 20, 24, 28}


def test_two_kept_records_sharing_a_data_record_each_get_a_copy(cuda):
    run, d = _records(130)
    msgs = np.flatnonzero(_types(run) == 1)
    twin = run.copy()
    twin[60 * msgs[7] + 32:60 * msgs[7] + 36] = run[60 * msgs[3] + 32:60 * msgs[3] + 36]
    twin[60 * msgs[7] + 52:60 * msgs[7] + 56] = run[60 * msgs[3] + 52:60 * msgs[3] + 56]
    m, host = _check(cuda, twin, d, _kw())
    assert m.result["n_bad"] == 0 and m.crcs[msgs[7]] == m.crcs[msgs[3]]
    at = [8 * int.from_bytes(host["journal_dst"][60 * int(m.new_index[i]) + 32:][:4].tobytes(),
                             "big") - 40 for i in (msgs[3], msgs[7])]
    assert at[0] != at[1]


def test_a_window_inside_the_file(cuda):
    run, d = _records(300)
    msgs = [i for i in range(300) if int(run[60 * i]) >> 4 == 1]
    lo, hi = msgs[10], msgs[-5]
    at = [8 * int.from_bytes(run[60 * i + 32:60 * i + 36].tobytes(), "big") for i in (lo, hi)]
    part = run[60 * lo:60 * hi]          # its last MESSAGE record's DATA record ends at at[1]
    window = d[at[0]:at[1]]
    kw = _kw(data_file_pos=at[0], sync_point=_last_sync(part), confirm_mode=1)
    m, _ = _check(cuda, part, window, kw)
    assert m.result["n_messages"] > 50
    # one byte less, and the last record is refused
    short, _ = _check(cuda, part, window[:-1], kw)
    assert short == M.Refusal(M.DATA_RECORD, max(i for i in msgs if i < hi) - lo)


@pytest.mark.parametrize("skip", ["new_index", "out"])
def test_null_outputs(cuda, skip):
    run, d = _records(140)
    _check(cuda, run, d, _kw(sync_point=_last_sync(run)), skip=(skip,))
    refused, _ = _check(cuda, run, d, _kw(dst_bytes=8), skip=(skip,))
    assert refused.kind == M.DST_TOO_SMALL


# ---- the hand-worked cases ---------------------------------------------------

@pytest.mark.parametrize("w", C.written(), ids=lambda w: w.case.name)
def test_small_journals_byte_by_byte(cuda, w):
    data, journal = C.expected_bytes(w)
    kw = dict(w.case.kw, dst_bytes=data.size, journal_dst_bytes=journal.size)
    m, host = _check(cuda, w.case.run, w.case.data, kw)
    assert host["dst"][:data.size].tobytes() == data.tobytes()
    assert host["journal_dst"][:journal.size].tobytes() == journal.tobytes()


@pytest.mark.parametrize("r", C.refused()[0], ids=lambda r: r.case.name)
def test_every_refusal_kind_and_their_precedence(cuda, r):
    for sync in (True, False):
        m, _ = _check(cuda, r.case.run, r.case.data, r.case.kw, sync=sync)
        assert m == M.Refusal(r.kind, r.index)


@pytest.mark.parametrize("case", C.refused()[1], ids=lambda c: c.name)
def test_what_is_no_refusal(cuda, case):
    m, _ = _check(cuda, case.run, case.data, case.kw)
    assert isinstance(m, M.Rolled)


def test_a_violation_in_the_last_record_of_the_last_block(cuda):
    run, d = _records(1025)
    bad = run.copy()
    bad[60 * 1024 + 59] ^= 0xFF           # the magic of record 1,024, the second block's only one
    refused, _ = _check(cuda, bad, d, _kw())
    assert refused == M.Refusal(M.RECORD_HEADER, 1024)
    # and with an earlier violation of a higher kind in the first block
    last = max(i for i in range(1024) if int(run[60 * i]) >> 4 == 1)
    bad[60 * last + 32:60 * last + 36] = 0
    refused, _ = _check(cuda, bad, d, _kw())
    assert refused == M.Refusal(M.RECORD_HEADER, 1024)
    bad[60 * 1024 + 59] ^= 0xFF
    refused, _ = _check(cuda, bad, d, _kw())
    assert refused == M.Refusal(M.DATA_OFFSET, last)
    # dropped, the record's offset is never looked at
    keep = _keep(run, "all")
    keep[last] = 0
    m, _ = _check(cuda, bad, d, _kw(keep=keep))
    assert isinstance(m, M.Rolled)


# ---- past one tile per block, past one wave of block sums, past the frame grid
# (test_grid_regimes.py names the regimes and pins the sizes) ---------------------

@functools.lru_cache(maxsize=None)
def _large(n):
    """The run of n records the tests below share, and its DATA file: the
    first n records of one run of N_FRAME, written once (seconds of host time,
    more than every device call here together), with the whole DATA file (a
    shorter run leaves its end unread).  Varied DATA
    record sizes (`options`), so that a shifted position shows; a CONFIRM behind
    every seventh message only, so that with every second record kept more than
    100,000 of N_TILES records are kept MESSAGE records."""
    run, d = _records(G.N_FRAME, seed=289, options=True, confirm_every=7)
    return run[:60 * n], d


def _large_kw(n, how, mode, sync=True, window=False):
    run, _ = _large(n)
    return _kw(keep=_keep(run, how) if how else None, confirm_mode=mode,
               sync_point=_last_sync(run) if sync else None,
               data_file_pos=40 if window else 0, new_data_file_pos=4096)


@functools.lru_cache(maxsize=None)
def _large_model(n, how, mode, sync=True, window=False):
    """The model's answer to _large_kw's call with room to spare, run once."""
    run, d = _large(n)
    kw = dict(_large_kw(n, how, mode, sync, window), dst_bytes=1 << 40, journal_dst_bytes=1 << 40)
    return M.rollover(run, d[40:] if window else d, crc32c=CRC, **kw)


def _every_whole_tile_block_holds_every_type(run):
    """Every layout block that owns a whole tile or more (N_WAVES leaves its
    last block one record) holds records of all five types."""
    t = _types(run)
    r = G.regime(t.size)
    for b in range(r.nblocks):
        mine = t[b * r.per_block:(b + 1) * r.per_block]
        assert mine.size < 1024 or set(mine.tolist()) == {1, 2, 3, 4, 5}, b


def _confirms_kept_and_dropped(run, m):
    confirms = _types(run) == 2
    kept = m.new_index[confirms] != M.NOT_KEPT
    return int(kept.sum()), int((~kept).sum())


@pytest.mark.parametrize("n,mode", [(G.N_WAVES, 1), (G.N_TILES, 0), (G.N_TILES, 1),
                                    (G.N_FRAME, 1)],
                         ids=["waves-follow", "tiles-as_kept", "tiles-follow", "frame-follow"])
def test_every_second_record_kept_past_one_tile_per_block(cuda, n, mode):
    """N_WAVES: the frame's dword loop steps twice and the block sums of both
    prefixes cross waves.  N_TILES: two tiles per block -- stage()'s second
    tile, both layout_count carries, the join over two tiles.  N_FRAME: three
    tiles, and the frame's per-record loop steps twice (record 524,288)."""
    run, d = _large(n)
    r = G.regime(n)
    assert r.dwords_past_grid and r.cross_wave
    assert (r.per_block > 1024) == (n >= G.N_TILES) and r.units_past_grid == (n == G.N_FRAME)
    _every_whole_tile_block_holds_every_type(run)
    want = _large_model(n, "second", mode)
    assert isinstance(want, M.Rolled) and want.result["n_bad"] == 0
    if mode:
        kept, dropped = _confirms_kept_and_dropped(run, want)
        assert 10 * kept >= kept + dropped and 10 * dropped >= kept + dropped
    if n == G.N_TILES:
        assert want.result["n_messages"] > 100000
    # (N_FRAME: record 524,288 is the only one of the frame's second step; a
    # step not taken leaves the canaries in its new_index and out entries)
    m, _ = _check(cuda, run, d, _large_kw(n, "second", mode), model=want)
    assert m is want


def test_all_256_blocks_of_one_tile_with_everything_kept(cuda):
    run, d = _large(G.N_FULL)
    assert G.regime(G.N_FULL)[:2] == (256, 1024)
    _every_whole_tile_block_holds_every_type(run)
    want = _large_model(G.N_FULL, "all", 0, sync=False)
    assert want.result["n_messages"] == int((_types(run) == 1).sum()) > 100000
    assert want.result["n_kept"] == int((_types(run) != 5).sum())
    _check(cuda, run, d, _large_kw(G.N_FULL, "all", 0, sync=False), model=want)


def test_a_window_over_two_tiles_per_block_with_no_keep_array(cuda):
    run, d = _large(G.N_TILES)
    want = _large_model(G.N_TILES, None, 0, window=True)
    assert isinstance(want, M.Rolled) and want.result["n_messages"] > 100000
    assert want.result["n_messages"] == int((_types(run) == 1).sum())
    _check(cuda, run, d[40:], _large_kw(G.N_TILES, None, 0, window=True), model=want)


def _refusal_in_the_second_tile():
    """(a) the magic of record 1,024 + 5, in the second tile of block 0, and of
    record 2,048 + 3, in the first tile of block 1: the lower one is named."""
    run, d = _large(G.N_TILES)
    bad = run.copy()
    for i in (1024 + 5, 2048 + 3):
        bad[60 * i + 59] ^= 0xFF
    return bad, d, {}, M.Refusal(M.RECORD_HEADER, 1029)


def _refusal_kinds_across_blocks():
    """(b) a kept MESSAGE record's DATA record below record 100 (its last
    padding byte 9: DATA_RECORD) and the header of record 200,001: the lower
    kind wins over the lower index."""
    run, d = _large(G.N_TILES)
    victim = [i for i in range(1, 100, 2) if int(run[60 * i]) >> 4 == 1][3]
    o = 8 * int.from_bytes(run[60 * victim + 32:60 * victim + 36].tobytes(), "big")
    data = d.copy()
    data[o + 4 * (int.from_bytes(d[o:o + 4].tobytes(), "big") & 0x1FFFFFFF) - 1] = 9
    alone = M.rollover(run[:60 * 100], data, crc32c=CRC,
                       **_kw(keep=_keep(run[:60 * 100], "second"), dst_bytes=1 << 40,
                             journal_dst_bytes=1 << 40))
    assert alone == M.Refusal(M.DATA_RECORD, victim)
    bad = run.copy()
    bad[60 * 200001 + 8:60 * 200001 + 12] = 0        # primaryLeaseId 0
    return bad, data, {}, M.Refusal(M.RECORD_HEADER, 200001)


def _refusal_in_the_last_record_of_the_last_block():
    """(c) the magic of record n - 1, the 1,025th record of block 128."""
    run, d = _large(G.N_TILES)
    r = G.regime(G.N_TILES)
    assert G.N_TILES - 1 - (r.nblocks - 1) * r.per_block == 1024
    bad = run.copy()
    bad[60 * (G.N_TILES - 1) + 59] ^= 0xFF
    return bad, d, {}, M.Refusal(M.RECORD_HEADER, G.N_TILES - 1)


def _journal_destination_one_record_short():
    """(d) journal_dst one record short: the sync point behind the kept
    records of all 129 blocks is what no longer fits, named as record n."""
    run, d = _large(G.N_TILES)
    want = _large_model(G.N_TILES, "second", 1)
    short = dict(journal_dst_bytes=want.result["journal_bytes"] - 60,
                 dst_bytes=want.result["data_bytes"])
    return run, d, short, M.Refusal(M.DST_TOO_SMALL, G.N_TILES)


def _data_destination_one_byte_short():
    """(d) dst one byte short: the last kept MESSAGE record's DATA record ends
    one byte past it."""
    run, d = _large(G.N_TILES)
    want = _large_model(G.N_TILES, "second", 1)
    short = dict(journal_dst_bytes=want.result["journal_bytes"],
                 dst_bytes=want.result["data_bytes"] - 1)
    last = np.flatnonzero((_types(run) == 1) & (want.new_index != M.NOT_KEPT))[-1]
    return run, d, short, M.Refusal(M.DST_TOO_SMALL, int(last))


@pytest.mark.parametrize("case", [
    _refusal_in_the_second_tile, _refusal_kinds_across_blocks,
    _refusal_in_the_last_record_of_the_last_block, _journal_destination_one_record_short,
    _data_destination_one_byte_short], ids=lambda f: f.__name__.strip("_"))
def test_refusals_across_tiles_and_blocks(cuda, case):
    """Over N_TILES records, every second kept, FOLLOW: what the model refuses,
    synchronous and asynchronous, with nothing written."""
    run, data, sizes, expected = case()
    kw = dict(_large_kw(G.N_TILES, "second", 1), **sizes)
    room = {k: kw[k] if kw[k] is not None else 1 << 40 for k in ("dst_bytes", "journal_dst_bytes")}
    want = M.rollover(run, data, crc32c=CRC, **dict(kw, **room))
    assert want == expected
    for sync in (True, False):
        m, _ = _check(cuda, run, data, kw, sync=sync, model=want)
        assert m == expected


# ---- the join ----------------------------------------------------------------

def _join_run(guids_keys_keep, confirms):
    """MESSAGE records (guid, key, kept) then CONFIRM records (guid, key)."""
    w = S.PartitionWriter(lease_id=9)
    keep = []
    for k, (guid, key, kept) in enumerate(guids_keys_keep):
        w.message(bytes([k & 0xFF]) * (k % 7), key, guid=guid)
        keep.append(kept)
    for guid, key in confirms:
        w.confirm(guid, key)
        keep.append(len(keep) & 1)       # ignored in FOLLOW mode
    j, d = w.files()
    return j[JH:].copy(), d, np.array(keep, np.uint8)


def _follow(cuda, run, d, keep):
    m, _ = _check(cuda, run, d, _kw(keep=keep, confirm_mode=1))
    assert isinstance(m, M.Rolled)
    return m.new_index != M.NOT_KEPT


def test_two_thousand_confirms_of_one_guid(cuda):
    g = [bytes([0x40 + i]) + bytes(15) for i in range(3)]
    run, d, keep = _join_run([(g[0], QK, 1), (g[1], QK, 0), (g[2], QK, 1)],
                             [(g[0], QK)] * 2000 + [(g[1], QK)] * 30)
    kept = _follow(cuda, run, d, keep)
    assert kept.tolist() == [True, False, True] + [True] * 2000 + [False] * 30


@pytest.mark.parametrize("at", [0, 15])
def test_guids_that_differ_in_one_byte_only(cuda, at):
    guids = [bytes(at) + bytes([i]) + bytes(15 - at) for i in range(256)]
    run, d, keep = _join_run([(g, QK, i % 3 == 0) for i, g in enumerate(guids)],
                             [(g, QK) for g in reversed(guids)] + [(guids[0], QK2)])
    kept = _follow(cuda, run, d, keep)
    assert kept[256:512].tolist() == [i % 3 == 0 for i in reversed(range(256))]
    assert not kept[512]                 # the GUID of a kept message under another queue key


def test_the_join_cases_of_the_model_test(cuda):
    # a CONFIRM below its MESSAGE, of a dropped message, under another key,
    # several of one GUID, a kept and a dropped MESSAGE with the same GUID
    run, d, keep, want = C.join_partition()
    kept = _follow(cuda, run, d, keep)
    assert np.flatnonzero(kept).tolist() == want


# ---- keys chosen to collide in the JoinTable (join_collisions.py) -------------

def _confirms_kept(cuda, c):
    """Which CONFIRM records of the crafted run `c` are rolled, in run order;
    the set restatement of the join (J.survivors) agrees."""
    kept = _follow(cuda, c.run, c.data, c.info["keep"])[_types(c.run) == 2].tolist()
    assert kept == J.survivors(c.run, c.info["keep"])
    return kept


def test_one_chain_across_the_tables_end(cuda):
    """200 messages with one home eight slots before the table's end (every
    queue-key byte 0x80 or more), every second one kept: the table holds a
    chain of 100 that the dropped messages' CONFIRM records walk to its end.
    Twice: the outputs are equal."""
    c = J.rollover_chain()
    kept = _confirms_kept(cuda, c)
    assert len(kept) == J.CHAIN and sum(kept) == J.CHAIN // 2
    kw = _kw(keep=c.info["keep"], confirm_mode=1)
    (_, host), (_, again) = _check(cuda, c.run, c.data, kw), _check(cuda, c.run, c.data, kw)
    assert sorted(again) == sorted(host)
    assert all(np.array_equal(host[name], again[name]) for name in host)


def test_a_chain_longer_than_a_block(cuda):
    assert sum(_confirms_kept(cuda, J.rollover_long())) == J.LONG == 1100


@pytest.mark.parametrize("swapped", [False, True], ids=["low_first", "high_first"])
def test_near_pairs_in_one_chain(cuda, swapped):
    """Per key byte two messages that differ in bit 0x80 of it only, the first
    of each kept, all 21 kept ones in one chain: the twin's CONFIRM record
    meets its twin in the table and is dropped."""
    c = J.rollover_pairs(swapped)
    kept = _confirms_kept(cuda, c)
    assert len(kept) == 2 * J.PAIRS and sum(kept) == J.PAIRS == 21
    confirms = np.asarray(c.run).reshape(-1, 60)[_types(c.run) == 2]
    assert {r[32:48].tobytes() + r[22:27].tobytes() for r in confirms[kept]} == \
        {first for first, _ in c.info["pairs"]}


def test_a_duplicate_behind_a_chain(cuda):
    c = J.rollover_duplicate()
    m, _ = _check(cuda, c.run, c.data, _kw(keep=c.info["keep"], confirm_mode=1))
    assert m.result["n_messages"] == J.BEHIND + 1 and m.result["n_kept"] == J.BEHIND + 3


def test_keep_leaves_one_collider_in_the_table(cuda):
    c = J.rollover_chain(137)
    kept = _confirms_kept(cuda, c)
    assert sum(kept) == 1 and c.info["n_kept_messages"] == 1


# ---- verify on rollover ------------------------------------------------------

def test_a_flipped_payload_byte_is_counted_and_rolled(cuda):
    run, d = _records(400)
    good = M.rollover(run, d, crc32c=CRC, **dict(_kw(), dst_bytes=1 << 30,
                                                 journal_dst_bytes=1 << 30))
    victim = int(np.flatnonzero(good.crcs != 0)[40])
    o = 8 * int.from_bytes(run[60 * victim + 32:60 * victim + 36].tobytes(), "big")
    bad = d.copy()
    bad[o + 12] ^= 0x10
    m, host = _check(cuda, run, bad, _kw())
    assert (m.result["n_bad"], m.result["first_bad"]) == (1, victim)
    diff = np.flatnonzero(host["dst"][:good.data.size] != good.data)
    assert diff.size == 1 and host["dst"][diff[0]] == bad[o + 12]


# ---- pointers that do not start an allocation --------------------------------

@pytest.mark.parametrize("mode", [0, 1])
def test_the_base_alignments_the_abi_permits(cuda, mode):
    run, d = _records(700, seed=8, options=True)
    for name, phase in PHASES.items():
        assert phase % {"data": 8, "dst": 8, "keep": 1}.get(name, 4) == 0
    _check(cuda, run, d[40:], _kw(data_file_pos=40, keep=_keep(run, "second"), confirm_mode=mode,
                                  sync_point=_last_sync(run)), phases=PHASES)
    refused, _ = _check(cuda, run, d[40:], _kw(data_file_pos=40, keep=_keep(run, "all"),
                                               dst_bytes=1000), phases=PHASES)
    assert refused.kind == M.DST_TOO_SMALL


# ---- the wrapper, asynchronous calls and state --------------------------------

def test_python_wrapper_raises_and_reports(cuda):
    import torch
    bad = [r for r in C.refused()[0] if r.case.name == "padding_9"][0]
    run, data = _dev(cuda, bad.case.run), _dev(cuda, bad.case.data)
    with pytest.raises(BmqCrcError, match="BMQCRC_ROLLOVER_DATA_RECORD: kept MESSAGE record 2 ") as e:
        rollover_records(run, data, data_file_pos=0, new_data_file_pos=40)
    assert e.value.rc == N.BMQCRC_EINVAL
    w = C.written()[0]
    want = M.rollover(w.case.run, w.case.data, crc32c=CRC, **w.case.kw)
    s = _side_stream(cuda)
    with torch.cuda.stream(s):
        dst = torch.zeros(256, dtype=torch.uint8, device=cuda)
        u = rollover_records(run, data, data_file_pos=0, new_data_file_pos=40, dst=dst, stream=s,
                             sync=False)
        assert u.result is None
        assert last_rollover(cuda.index, s) == M.refused_result(M.Refusal(bad.kind, bad.index),
                                                                C.N)
        assert not dst.any()
        u = rollover_records(_dev(cuda, w.case.run), _dev(cuda, w.case.data), data_file_pos=0,
                             new_data_file_pos=40, sync_point=11, timestamp=C.TIMESTAMP, dst=dst,
                             stream=s, sync=False)
        res = last_rollover(cuda.index, s)
    assert res == want.result
    assert np.array_equal(dst.cpu().numpy()[:want.data.size], want.data)
    assert np.array_equal(u.journal_dst.cpu().numpy()[:want.journal.size], want.journal)
    r = rollover_records(_dev(cuda, w.case.run), _dev(cuda, w.case.data), data_file_pos=0,
                         new_data_file_pos=40, sync_point=11, timestamp=C.TIMESTAMP)
    assert r.result == want.result
    assert np.array_equal(r.dst.cpu().numpy(), want.data)
    assert np.array_equal(r.journal_dst.cpu().numpy(), want.journal)
    assert np.array_equal(r.new_index.cpu().numpy().view(np.uint32), want.new_index)
    assert np.array_equal(r.crcs.cpu().numpy().view(np.uint32), want.crcs)


def test_state(cuda):
    import torch
    rng = np.random.default_rng(56)
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
    run, d = _records(400)
    msgs = np.flatnonzero(_types(run) == 1)
    events, offsets = synth.storage_events(run[60:], d, 0, JH + 60, 1, 33)
    kw = _kw(keep=_keep(run, "second"), confirm_mode=1, sync_point=_last_sync(run))
    s = _side_stream(cuda)

    def records():
        return (last_launch(cuda.index, s, offsets=True), last_copy(cuda.index, s),
                last_put_pack(cuda.index, s), last_records_pack(cuda.index, s),
                last_put_unpack(cuda.index, s), last_records_unpack(cuda.index, s),
                last_journal_select(cuda.index, s), last_storage_apply(cuda.index, s),
                last_storage_pack(cuda.index, s), last_push_pack(cuda.index, s))
    with torch.cuda.stream(s):
        # none yet on s
        assert last_rollover(cuda.index, s) == M.refused_result(M.Refusal(0, 0), 0)
        Crc32c.calculate_batch(arena, d_off, d_len, stream=s)
        Crc32c.copy_batch(arena, d_off[:40], d_len[:40], copy_dst, doff, stream=s)
        pack_events(arena, d_off[:30], d_len[:30], _t(cuda, qids, np.int32),
                    _t(cuda, guids, np.uint8), _t(cuda, flags, np.uint8), stream=s)
        pack_records(arena, d_off[:30], d_len[:30], _t(cuda, np.full((30, 5), 7), np.uint8),
                     _t(cuda, guids, np.uint8), file_key=b"\x11\x22\x33\x44\x55", lease_id=3,
                     first_seq=2, data_file_pos=40, stream=s)
        unpack_events(_dev(cuda, buf), _t(cuda, evoffs, np.int64), stream=s)
        unpack_records(_dev(cuda, run), _dev(cuda, d), data_file_pos=0, stream=s)
        select_records(_dev(cuda, run), data_file_bytes=d.size, stream=s)
        apply_events(_dev(cuda, events), _t(cuda, offsets.view(np.int64), np.int64),
                     partition_id=1, journal_pos=JH + 60, data_file_pos=40, stream=s)
        pack_storage_events(_dev(cuda, run), _dev(cuda, d), journal_pos=JH, data_file_pos=0,
                            partition_id=1, stream=s)
        pack_push_events(_dev(cuda, run), _dev(cuda, d), data_file_pos=0,
                         records=_t(cuda, msgs.astype(np.uint32), np.uint32),
                         queue_ids=_t(cuda, np.arange(msgs.size), np.int32), stream=s)
        before = records()
        _check(cuda, run, d, kw, stream=s)
        _check(cuda, run, d, kw, stream=s, sync=False)
        _check(cuda, run, d, dict(kw, dst_bytes=100), stream=s)   # a refused one
        assert records() == before
        assert before[1] == (40, 0, 40)
        out = Crc32c.calculate_batch(arena, d_off, d_len, stream=s)
    s.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), P.host_crcs(host, offs, lens))


# ---- the pipeline ------------------------------------------------------------

def test_a_partition_compacted_on_one_device(cuda):
    # pack_records -> (CONFIRM and DELETION records appended) -> select_records
    # -> rollover_records(keep=select, FOLLOW) -> select_records,
    # unpack_records(verify=True) and pack_push_events over the new partition
    import torch
    rng = np.random.default_rng(63)
    lens = rng.integers(0, 701, size=300).astype(np.uint32)
    n = lens.size
    soff = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    src = rng.integers(0, 256, size=int(lens.sum()), dtype=np.uint8)
    qkeys, guids = random_meta(rng, n)
    qkeys[:] = np.frombuffer(QK, np.uint8)
    dst, jour, _, _, _ = pack_records(
        _t(cuda, src, np.uint8), _t(cuda, soff, np.int64), _t(cuda, lens, np.uint32),
        _t(cuda, qkeys, np.uint8), _t(cuda, guids, np.uint8), file_key=b"\x11\x22\x33\x44\x55",
        lease_id=7, first_seq=2, data_file_pos=40)
    w = S.PartitionWriter(lease_id=7, partition_id=2)
    w.queue_op(S.OP_CREATION, QK)
    w.seq = n + 1
    deleted = set(range(5, n, 4))
    for i in range(0, n, 3):             # confirmed: some of them deleted later
        w.confirm(guids[i].tobytes(), QK)
    for i in sorted(deleted):
        w.deletion(guids[i].tobytes(), QK)
    w.sync_point()
    tail = np.frombuffer(b"".join(w.recs[1:]), np.uint8).copy()
    journal = torch.cat([_t(cuda, np.frombuffer(w.recs[0], np.uint8).copy(), np.uint8), jour,
                         _t(cuda, tail, np.uint8)])
    n_records = journal.numel() // 60
    select, sel = select_records(journal, data_file_bytes=40 + dst.numel())
    assert sel["recovery_rc"] == 0 and sel["n_selected"] == n - len(deleted)
    old = unpack_records(journal, dst, data_file_pos=40, select=select, verify=True)
    keep = select.clone()
    keep[0] = 1                          # the queue's CREATION: the caller's decision
    r = rollover_records(journal, dst, data_file_pos=40, new_data_file_pos=40, keep=keep,
                         confirm_mode=S.CONFIRMS_FOLLOW_MESSAGES, sync_point=n_records - 1,
                         timestamp=99)
    confirmed = len([i for i in range(0, n, 3) if i not in deleted])
    assert r.result == dict(
        n_records=n_records, n_kept=1 + n - len(deleted) + confirmed, n_messages=n - len(deleted),
        journal_bytes=60 * (2 + n - len(deleted) + confirmed), data_bytes=r.dst.numel(), n_bad=0,
        first_bad=n_records, refused_kind=0, refused_index=0)
    model = M.rollover(journal.cpu().numpy(), dst.cpu().numpy(), data_file_pos=40,
                       new_data_file_pos=40, keep=keep.cpu().numpy(), confirm_mode=1,
                       sync_point=n_records - 1, timestamp=99, dst_bytes=dst.numel(),
                       journal_dst_bytes=journal.numel(), crc32c=CRC)
    assert np.array_equal(r.journal_dst.cpu().numpy(), model.journal)
    assert np.array_equal(r.dst.cpu().numpy(), model.data)
    # the new run: every MESSAGE record is selected, and verifies
    select2, sel2 = select_records(r.journal_dst, data_file_bytes=40 + r.dst.numel())
    assert sel2["recovery_rc"] == 0 and sel2["n_selected"] == n - len(deleted)
    types2 = _types(r.journal_dst.cpu().numpy())
    assert np.array_equal(select2.cpu().numpy() != 0, types2 == 1)
    new = unpack_records(r.journal_dst, r.dst, data_file_pos=40, select=select2, verify=True)
    res = last_records_unpack(cuda.index, torch.cuda.current_stream(cuda))
    assert (res["n_msgs"], res["n_bad"], res["refused_kind"]) == (n - len(deleted), 0, 0)
    assert torch.equal(new.guids, old.guids) and torch.equal(new.crcs, old.crcs)
    assert torch.equal(new.lengths, old.lengths) and torch.equal(new.expected, old.expected)
    # the host's recovery over the new files agrees
    jfile = np.concatenate([w.files()[0][:JH], r.journal_dst.cpu().numpy()])
    dfile = np.concatenate([w.files()[1][:40], r.dst.cpu().numpy()])
    v = S.verify_partition(jfile, dfile)
    assert (v["n_messages"], v["n_bad"], v["recovery_rc"]) == (n - len(deleted), 0, 0)
    # delivery: the same PUSH events from the old partition and the new one
    qids = _t(cuda, np.arange(n - len(deleted)) % 5, np.int32)
    a = pack_push_events(journal, dst, data_file_pos=40, queue_ids=qids,
                         records=old.record_index)
    b = pack_push_events(r.journal_dst, r.dst, data_file_pos=40, queue_ids=qids,
                         records=new.record_index)
    assert a.result["n_bad"] == b.result["n_bad"] == 0
    assert torch.equal(a.events, b.events) and torch.equal(a.event_offsets, b.event_offsets)
