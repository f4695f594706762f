"""Journal and DATA records packed into STORAGE events on the GPU
(bmqcrc_storage_event_pack, ABI 2.16).  The oracle throughout is
tests/storage_pack_model.py.  Every raw call hands the library a
sentinel-filled destination and output arrays with guard bytes and elements
behind them: the guards are checked after every call, and every byte and
element after a refused one."""
import ctypes
import functools

import numpy as np
import pytest

from blazingmq_amd import (BmqCrcError, Crc32c, _native as N, apply_events, last_copy,
                           last_journal_select, last_launch, last_put_pack, last_put_unpack,
                           last_records_pack, last_records_unpack, last_storage_apply,
                           last_storage_pack, pack_events, pack_records, pack_storage_events,
                           select_records, unpack_events, unpack_records)
from blazingmq_amd import storage as S
from blazingmq_amd import storage_event as E
from blazingmq_amd import synth
import device_views as V
import put_pack_model as P
import put_unpack_model as PU
import record_pool as R
import storage_pack_cases as C
import storage_pack_model as M
import test_grid_regimes as G
from records_pack_model import random_meta

pytestmark = pytest.mark.gpu

GUARD = 8      # elements behind every output array
SLACK = 64     # bytes behind every input buffer and the destination
SENTINEL = 0xC3
JH = S.PartitionWriter.JOURNAL_HEADER
CANARY = {"event_offsets": 0x5A5A5A5A5A5A5A5A, "types": 0xA5, "out": 0x5A5A5A5A}
NP = {"event_offsets": np.uint64, "types": np.uint8, "out": np.uint32}
MODEL = {"event_offsets": "event_offsets", "types": "types", "out": "crcs"}
KIND_NAME = {k: ("BMQCRC_STORAGE_PACK_" + n).encode() for k, n in enumerate(E.PACK_REFUSALS) if k}
CRC = Crc32c.calculate
QK = S.DEFAULT_QUEUE_KEY


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


def _kw(run, d, **changes):
    """Keywords of a call over the whole DATA file into a destination of the
    exact size (the model refuses a smaller one)."""
    kw = dict(journal_pos=JH, data_file_pos=0, partition_id=1, event_first=None, flags=None,
              event_type=0, storage_protocol_version=E.STORAGE_PROTOCOL_VERSION,
              max_event_bytes=0, max_payload_bytes=0, dst_bytes=None)
    kw.update(changes)
    return kw


def _raw(cuda, run, data, kw, sync=True, stream=None, skip=(), phases=None):
    """One bmqcrc_storage_event_pack over device tensors into a sentinel-filled
    destination and arrays.  Returns (rc, error text, result of the call or of
    bmqcrc_last_storage_pack, everything written on the host with its guards).
    `phases` maps every pointer of the call (journal, data, flags, event_first,
    dst, event_offsets, types, out) to the phase of its base; the sentinel
    margins around each are checked after the call.  None: every buffer starts
    its allocation."""
    import torch
    place = V.Placer(cuda, phases) if phases is not None else None
    stream = stream or torch.cuda.current_stream(cuda)
    n = len(run) // 60
    first = kw["event_first"]
    n_events = 1 if first is None else len(first) - 1
    count = {"event_offsets": n_events + 1, "types": n, "out": n}
    with torch.cuda.stream(stream):
        d_run, d_data = _dev(cuda, run, place, "journal"), _dev(cuda, data, place, "data")
        d_flags = _dev(cuda, kw["flags"], place, "flags") if kw["flags"] is not None else None
        if first is None:
            d_first = None
        elif place is not None:
            d_first = place.put("event_first", np.asarray(first, np.uint64))
        else:
            d_first = _t(cuda, np.asarray(first, np.uint64).view(np.int64), np.int64)
        if place is not None:
            arr = {"dst": place.fill("dst", kw["dst_bytes"] + SLACK, np.uint8, SENTINEL)}
        else:
            # (`dst_alloc`: a destination declared shorter than its allocation)
            size = max(kw["dst_bytes"], kw.get("dst_alloc", 0))
            arr = {"dst": torch.full((size + SLACK,), SENTINEL, dtype=torch.uint8, device=cuda)}
        for name, dt in NP.items():
            if name in skip:
                continue
            if place is not None:
                arr[name] = place.fill(name, count[name] + GUARD, dt, CANARY[name])
                continue
            fill = np.array([CANARY[name]], np.uint64).astype(dt)
            arr[name] = torch.from_numpy(np.repeat(fill, count[name] + GUARD).view(
                {np.uint32: np.int32, np.uint64: np.int64}.get(dt, dt))).to(cuda)
        # (an empty tensor has no address: the call wants one)
        spare = torch.zeros(8, dtype=torch.uint8, device=cuda)
        p = N.StoragePack()
        p.struct_size = ctypes.sizeof(N.StoragePack)
        p.journal, p.journal_bytes = d_run.data_ptr() or spare.data_ptr(), d_run.numel()
        p.n_records, p.journal_pos = n, kw["journal_pos"]
        p.data, p.data_bytes = d_data.data_ptr() or spare.data_ptr(), d_data.numel()
        p.data_file_pos, p.partition_id = kw["data_file_pos"], kw["partition_id"]
        p.event_type, p.storage_protocol_version = kw["event_type"], kw["storage_protocol_version"]
        p.flags = d_flags.data_ptr() if d_flags is not None else None
        p.event_first = d_first.data_ptr() if d_first is not None else None
        p.n_events = n_events
        p.max_event_bytes, p.max_payload_bytes = kw["max_event_bytes"], kw["max_payload_bytes"]
        p.dst, p.dst_bytes = arr["dst"].data_ptr(), kw["dst_bytes"]
        for name in NP:
            setattr(p, name, arr[name].data_ptr() if name in arr else None)
        o = N.make_opts(device=cuda.index, stream=stream.cuda_stream,
                        flags=N.BMQCRC_F_DEVICE_PTRS | (0 if sync else N.BMQCRC_F_ASYNC))
        r = N.StoragePackResult()
        rc = N.lib.bmqcrc_storage_event_pack(ctypes.byref(p), ctypes.byref(r), ctypes.byref(o))
        err = N.lib.bmqcrc_last_error()
        res = r.as_dict() if sync else last_storage_pack(cuda.index, stream)
        host = {name: t.cpu().numpy() for name, t in arr.items()}
        if place is not None:
            place.check()
    for name, dt in NP.items():
        if name in host:
            host[name] = host[name].view(dt)
    return rc, err, res, host


def _untouched(name, a):
    want = SENTINEL if name == "dst" else np.array([CANARY[name]], np.uint64).astype(NP[name])[0]
    return bool((a == want).all())


def _check(cuda, run, data, kw, sync=True, stream=None, skip=(), model=None, phases=None):
    """The call against the model: a refusal identical and nothing written, or
    every destination byte, array entry and result field.  `dst_bytes` None is
    the exact size.  `phases`: as in _raw.  Returns (model, host)."""
    kw = dict(kw)
    if kw["dst_bytes"] is None:
        kw["dst_bytes"] = 1 << 40
        m = M.pack(run, data, crc32c=CRC, **kw) if model is None else model
        kw["dst_bytes"] = m.result["total_bytes"] if isinstance(m, M.Packed) else 4096
    m = model if model is not None else M.pack(run, data, crc32c=CRC, **kw)
    rc, err, res, host = _raw(cuda, run, data, kw, sync=sync, stream=stream, skip=skip,
                              phases=phases)
    n = len(run) // 60
    n_events = (1 if kw["event_first"] is None else len(kw["event_first"]) - 1) if n else 0
    if isinstance(m, M.Refusal):
        if sync:
            assert rc == N.BMQCRC_EINVAL and KIND_NAME[m.kind] in err, (rc, err, m)
            assert b"nothing was written" in err and (b"%d" % m.index) in err, (err, m)
        else:
            assert rc == 0, err
        assert res == M.refused_result(m, n_events), (res, m)
        for name, a in host.items():
            assert _untouched(name, a), name
        return m, host
    assert rc == 0, err
    assert res == m.result, (res, m.result)
    used = m.result["total_bytes"]
    assert np.array_equal(host["dst"][:used], m.events)
    assert _untouched("dst", host["dst"][used:])
    for name in NP:
        if name in skip:
            continue
        want = getattr(m, MODEL[name])
        assert np.array_equal(host[name][:len(want)], want), name
        assert _untouched(name, host[name][len(want):]), name
    return m, host


def _cuts(n, per_event):
    return np.array(list(range(0, n, per_event)) + [n], np.uint64)


@functools.lru_cache(maxsize=None)
def _records(n, seed=7, options=False, lengths=None):
    """(record run of n records, DATA file): a queue's CREATION, then messages
    of 0..40 bytes (or of `lengths`, in turn), every third followed by its
    CONFIRM, every ninth by its DELETION too, in front of every 16th a queue
    ADDITION, PURGE or DELETION or a sync point; with `options` DATA headers of
    3 and 5 words with 0..2 option words.  Shared, never modified."""
    rng = np.random.default_rng(seed)
    w = S.PartitionWriter(lease_id=4, partition_id=1)
    w.queue_op(S.OP_CREATION, QK)
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
        _, guid = w.message(app, QK, data_flags=k & 0xFF)
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
        if k % 3 == 0 and len(w.recs) < n:
            w.confirm(guid, QK)
        if k % 9 == 0 and len(w.recs) < n:
            w.deletion(guid, QK)
        k += 1
    j, d = w.files()
    run = j[JH:]
    run.setflags(write=False)
    d.setflags(write=False)
    return run, d


# ---- wave, tile and grid edges -----------------------------------------------

@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 1023, 1024, 1025])
def test_record_counts(cuda, count):
    run, d = _records(1025)
    run = run[:60 * count]
    m, _ = _check(cuda, run, d, _kw(run, d))
    assert m.result["n_msgs"] == count


@pytest.mark.parametrize("per_event", [1, 3, 17, 40, 1024])
def test_event_cuts(cuda, per_event):
    # every message its own event; cuts inside a wave's 64 records; a cut at a
    # block's boundary, record 1,024
    n = 1025 if per_event == 1024 else 140
    run, d = _records(1025)
    run = run[:60 * n]
    m, _ = _check(cuda, run, d, _kw(run, d, event_first=_cuts(n, per_event)))
    assert m.result["n_events"] == -(-n // per_event)


@pytest.mark.parametrize("per_event", [4099, 1])
def test_a_quarter_million_records_against_synth(cuda, per_event):
    # 262,145 records: the first size at which a layout block takes a second
    # tile and the carry matters.  Every 8th record a MESSAGE of 8 bytes, the
    # others CONFIRM and DELETION records; the expected bytes are
    # synth.storage_events', which tests/test_storage_pack_model.py holds equal
    # to the model on such runs.  With every record its own event a block's
    # 2,048 records lie in more events than the seal searches in LDS
    import torch
    n = 256 * 1024 + 1
    k = -(-n // 8)
    journal, data, app_off, app_len = synth.partition(k, 8, seed=61)
    msgs = journal[JH + 60:].reshape(k, 60)
    recs = np.zeros((n, 60), np.uint8)
    recs[:, 0] = np.where(np.arange(n) % 2, S.REC_CONFIRM, S.REC_DELETION) << 4
    recs[::8] = msgs
    seq = 1 + np.arange(n, dtype=np.uint64)
    recs[:, 4:8] = synth._be(seq, ">u4")
    recs[:, 8:12] = msgs[0, 8:12]
    recs[:, 56:60] = msgs[0, 56:60]
    run = recs.reshape(-1)
    want, want_offsets = synth.storage_events(run, data, 0, JH + 60, 7, per_event)
    first = _cuts(n, per_event)
    dst = torch.full((want.size + SLACK,), SENTINEL, dtype=torch.uint8, device=cuda)
    p = pack_storage_events(torch.from_numpy(run).to(cuda), _dev(cuda, data),
                            journal_pos=JH + 60, data_file_pos=0, partition_id=7,
                            event_first=_t(cuda, first.view(np.int64), np.int64),
                            dst=dst[:want.size])
    assert p.result == dict(n_events=first.size - 1, n_msgs=n, n_data=k, total_bytes=want.size,
                            n_bad=0, first_bad=n, refused_kind=0, refused_index=0)
    assert torch.equal(p.events.cpu(), torch.from_numpy(want))
    assert bool((dst[want.size:] == SENTINEL).all())
    assert np.array_equal(p.event_offsets.cpu().numpy().view(np.uint64), want_offsets)
    types = p.types.cpu().numpy()
    assert np.array_equal(types, np.where(np.arange(n) % 8 == 0, 1,
                                          np.where(np.arange(n) % 2, 3, 4)))
    crcs = p.crcs.cpu().numpy().view(np.uint32)
    assert np.array_equal(crcs[::8], synth.host_crcs(data, app_off, app_len))
    assert not crcs.reshape(-1)[np.arange(n) % 8 != 0].any()


# ---- what the records carry --------------------------------------------------

def test_every_record_type_and_queue_op_flags_and_the_header_fields(cuda):
    run, d = _records(260)
    n = 260
    flags = (np.arange(n) * 37 % 256).astype(np.uint8)
    kw = _kw(run, d, flags=flags, event_type=E.EVENT_TYPE_PARTITION_SYNC, partition_id=65535,
             storage_protocol_version=2, event_first=_cuts(n, 33))
    m, host = _check(cuda, run, d, kw)
    assert sorted(set(m.types.tolist())) == [1, 2, 3, 4, 5, 6]
    ops = {int.from_bytes(run[60 * i + 32:60 * i + 36].tobytes(), "big")
           for i in range(n) if int(run[60 * i]) >> 4 == S.REC_QUEUE_OP}
    assert ops == {1, 2, 3, 4}
    got = [(ms["flags"], ms["partition_id"], ms["storage_protocol_version"])
           for e in range(len(m.event_offsets) - 1) for ms in E.StorageMessageIterator(
               host["dst"][int(m.event_offsets[e]):int(m.event_offsets[e + 1])])]
    assert got == [(int(f) & 31, 65535, 2) for f in flags]
    assert host["dst"][4] == (1 << 6) | 10
    _check(cuda, run, d, _kw(run, d, partition_id=0, event_type=E.EVENT_TYPE_STORAGE))


def test_option_words_header_sizes_and_every_alignment(cuda):
    run, d = _records(700, seed=8, options=True)
    m, host = _check(cuda, run, d, _kw(run, d, event_first=_cuts(700, 50)))
    # The copy cuts a message on the 16-byte pieces of its destination and reads
    # its source with unaligned 16-byte loads.  Records and messages are
    # multiples of 8 long, so source and destination start 0 or 8 bytes apart
    # mod 16: every 4-byte phase of either inside a piece occurs, in all 8
    # pairs there are, with headers of 12 to 28 bytes
    leads, pairs, pos = set(), set(), {}
    for e in range(len(m.event_offsets) - 1):
        beg = int(m.event_offsets[e])
        for ms in E.StorageMessageIterator(m.events[beg:int(m.event_offsets[e + 1])]):
            pos[len(pos)] = beg + ms["payload_offset"]
    for i in np.flatnonzero(m.types == 1):
        o = 8 * int.from_bytes(run[60 * i + 32:60 * i + 36].tobytes(), "big")
        lead = 4 * ((int(d[o]) >> 5) + (int.from_bytes(d[o + 4:o + 7].tobytes(), "big")))
        leads.add(lead)
        pairs.add(((o + lead) % 16 // 4, (pos[int(i)] + lead) % 16 // 4))
    assert leads == {12, 16, 20, 24, 28} and len(pairs) == 8
    assert {a for a, _ in pairs} == {b for _, b in pairs} == {0, 1, 2, 3}


def test_application_data_lengths(cuda):
    # 0 and 1..24 (every padding value 1..8), 255..257, 64 KiB, and 300 KiB + 3:
    # the copy's long path
    lengths = tuple(range(25)) + (255, 256, 257, 64 * 1024, 300 * 1024 + 3)
    run, d = _records(46, seed=9, lengths=lengths)
    m, _ = _check(cuda, run, d, _kw(run, d, event_first=_cuts(46, 17)))
    assert m.result["n_data"] == len(lengths) and m.result["n_bad"] == 0
    pads = set()
    for i in np.flatnonzero(m.types == 1):
        o = 8 * int.from_bytes(run[60 * i + 32:60 * i + 36].tobytes(), "big")
        pads.add(int(d[o + 4 * (int.from_bytes(d[o:o + 4].tobytes(), "big") & 0x1FFFFFFF) - 1]))
    assert pads == set(range(1, 9))


def test_a_window_inside_the_file_that_ends_with_its_last_record(cuda):
    run, d = _records(300)
    msgs = [i for i in range(300) if int(run[60 * i]) >> 4 == 1]
    lo, hi = msgs[10], msgs[-5]
    at = [8 * int.from_bytes(run[60 * i + 32:60 * i + 36].tobytes(), "big") for i in (lo, hi)]
    part = run[60 * lo:60 * hi]          # its last MESSAGE record's DATA record ends at at[1]
    window = d[at[0]:at[1]]
    kw = _kw(part, window, journal_pos=JH + 60 * lo, data_file_pos=at[0],
             event_first=_cuts(hi - lo, 40))
    m, _ = _check(cuda, part, window, kw)
    whole = M.pack(run, d, crc32c=CRC, **dict(_kw(run, d), dst_bytes=1 << 30))
    assert np.array_equal(m.crcs, whole.crcs[lo:hi]) and m.result["n_data"] > 50
    # one byte less, and the last record is refused
    short, _ = _check(cuda, part, window[:-1], kw)
    assert short == M.Refusal(M.DATA_RECORD, max(i for i in msgs if i < hi) - lo)


@pytest.mark.parametrize("skip", ["event_offsets", "types", "out"])
def test_null_outputs(cuda, skip):
    run, d = _records(140)
    _check(cuda, run, d, _kw(run, d, event_first=_cuts(140, 17)), skip=(skip,))
    refused, _ = _check(cuda, run, d, _kw(run, d, dst_bytes=64), skip=(skip,))
    assert refused == M.Refusal(M.DST_TOO_SMALL, 0)


# ---- verify on send ----------------------------------------------------------

def test_a_flipped_payload_byte_is_counted_and_sent(cuda):
    run, d = _records(400)
    good = M.pack(run, d, crc32c=CRC, **dict(_kw(run, d), dst_bytes=1 << 30))
    victim = int(np.flatnonzero((good.types == 1) & (good.crcs != 0))[40])
    o = 8 * int.from_bytes(run[60 * victim + 32:60 * victim + 36].tobytes(), "big")
    bad = d.copy()
    bad[o + 12] ^= 0x10
    m, host = _check(cuda, run, bad, _kw(run, d, event_first=_cuts(400, 33)))
    assert (m.result["n_bad"], m.result["first_bad"]) == (1, victim)
    assert np.flatnonzero(host["out"][:400] != m.expected).tolist() == [victim]
    one = M.pack(run, d, crc32c=CRC, **dict(_kw(run, d, event_first=_cuts(400, 33)),
                                            dst_bytes=1 << 30))
    diff = np.flatnonzero(host["dst"][:one.events.size] != one.events)
    assert diff.size == 1 and host["dst"][diff[0]] == bad[o + 12]


# ---- refusals ----------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(C.refusal_cases()))
def test_refusal_like_the_model(cuda, name):
    case = C.refusal_cases()[name]
    m, _ = _check(cuda, case.run, case.data, _kw(None, None, **case.kw))
    assert m == case.want


@pytest.mark.parametrize("name", sorted(C.precedence_cases()))
def test_refusal_precedence(cuda, name):
    case = C.precedence_cases()[name]
    for sync in (True, False):
        m, _ = _check(cuda, case.run, case.data, _kw(None, None, **case.kw), sync=sync)
        assert m == case.want


def test_a_violation_in_the_last_record_of_the_last_block(cuda):
    run, d = _records(1025)
    bad = run.copy()
    bad[60 * 1024 + 59] ^= 0xFF           # the magic of record 1,024, the second block's only one
    refused, _ = _check(cuda, bad, d, _kw(run, d, event_first=_cuts(1025, 1024)))
    assert refused == M.Refusal(M.RECORD_HEADER, 1024)
    # and with an earlier violation of a higher kind in the first block
    last = max(i for i in range(1024) if int(run[60 * i]) >> 4 == 1)
    C.put32(bad, 60 * last + 32, 0)
    refused, _ = _check(cuda, bad, d, _kw(run, d))
    assert refused == M.Refusal(M.RECORD_HEADER, 1024)
    bad[60 * 1024 + 59] ^= 0xFF
    refused, _ = _check(cuda, bad, d, _kw(run, d))
    assert refused == M.Refusal(M.DATA_OFFSET, last)


def test_python_wrapper_raises_reports_and_sizes_the_destination(cuda):
    import torch
    case = C.refusal_cases()["padding_byte_9"]
    run, data = _dev(cuda, case.run), _dev(cuda, case.data)
    first = _t(cuda, np.asarray(C.EVENT_FIRST, np.int64), np.int64)
    state = dict(journal_pos=C.JOURNAL_POS, data_file_pos=0, partition_id=C.PARTITION)
    with pytest.raises(BmqCrcError, match="BMQCRC_STORAGE_PACK_DATA_RECORD: MESSAGE record 8 ") as e:
        pack_storage_events(run, data, event_first=first, **state)
    assert e.value.rc == N.BMQCRC_EINVAL
    with pytest.raises(ValueError, match="sync=False"):
        pack_storage_events(run, data, sync=False, **state)
    base_run, base_data, kw = C.base()
    want = M.pack(base_run, base_data, crc32c=CRC, **kw)
    s = _side_stream(cuda)
    with torch.cuda.stream(s):
        dst = torch.zeros(4096, dtype=torch.uint8, device=cuda)
        u = pack_storage_events(run, data, event_first=first, dst=dst, stream=s, sync=False,
                                **state)
        assert u.result is None and u.types.numel() == 17 and u.event_offsets.numel() == 5
        assert last_storage_pack(cuda.index, s) == M.refused_result(case.want, 4)
        assert not dst.any()
        u = pack_storage_events(_dev(cuda, base_run), _dev(cuda, base_data), event_first=first,
                                dst=dst, stream=s, sync=False, **state)
        res = last_storage_pack(cuda.index, s)
    assert res == want.result
    assert np.array_equal(dst.cpu().numpy()[:C.TOTAL], want.events)
    assert np.array_equal(u.crcs.cpu().numpy().view(np.uint32), want.crcs)
    # dst=None: the bound 8 n_events + 72 n + data.numel() holds every event
    p = pack_storage_events(_dev(cuda, base_run), _dev(cuda, base_data), event_first=first,
                            **state)
    assert p.result == want.result and p.events.numel() == C.TOTAL
    assert np.array_equal(p.events.cpu().numpy(), want.events)
    assert np.array_equal(p.event_offsets.cpu().numpy().view(np.uint64), want.event_offsets)
    assert np.array_equal(p.types.cpu().numpy(), want.types)


# ---- state -------------------------------------------------------------------

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
    events, offsets = synth.storage_events(run[60:], d, 0, JH + 60, 1, 33)
    kw = _kw(run, d, event_first=_cuts(400, 33))
    s = _side_stream(cuda)

    def records():
        return (last_launch(cuda.index, s, offsets=True), last_copy(cuda.index, s),
                last_put_pack(cuda.index, s), last_records_pack(cuda.index, s),
                last_put_unpack(cuda.index, s), last_records_unpack(cuda.index, s),
                last_journal_select(cuda.index, s), last_storage_apply(cuda.index, s))
    with torch.cuda.stream(s):
        # none yet on s
        assert last_storage_pack(cuda.index, s) == M.refused_result(M.Refusal(0, 0), 0)
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
        before = records()
        _check(cuda, run, d, kw, stream=s)
        _check(cuda, run, d, kw, stream=s, sync=False)
        _check(cuda, run, d, dict(kw, max_event_bytes=100), stream=s)   # a refused one
        assert records() == before
        assert before[1] == (40, 0, 40)
        out = Crc32c.calculate_batch(arena, d_off, d_len, stream=s)
    s.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), P.host_crcs(host, offs, lens))


# ---- the pipeline ------------------------------------------------------------

def test_round_trip_through_the_replica(cuda):
    import torch
    run, d = _records(700, seed=8, options=True)
    n = 700
    first = _t(cuda, _cuts(n, 50).view(np.int64), np.int64)
    p = pack_storage_events(_dev(cuda, run), _dev(cuda, d[40:]), journal_pos=JH,
                            data_file_pos=40, partition_id=1, event_first=first)
    assert p.result["n_bad"] == 0 and p.result["n_msgs"] == n
    a = apply_events(p.events, p.event_offsets, partition_id=1, journal_pos=JH, data_file_pos=40)
    assert np.array_equal(a.journal.cpu().numpy(), run)
    assert np.array_equal(a.data.cpu().numpy(), d[40:])
    last = run[60 * (n - 1):]
    assert a.result["head_lease_id"] == int.from_bytes(last[8:12].tobytes(), "big")
    assert a.result["head_seq"] == int.from_bytes(last[2:8].tobytes(), "big")
    assert (a.result["n_msgs"], a.result["n_data"]) == (n, p.result["n_data"])
    assert torch.equal(a.types, p.types) and torch.equal(a.crcs, p.crcs)


def test_a_partitions_whole_life_on_one_device(cuda):
    # pack_records -> pack_storage_events -> apply_events -> select_records ->
    # unpack_records(verify=True) reports what verify_partition reports on the
    # primary's files
    import torch
    rng = np.random.default_rng(62)
    lens = rng.integers(0, 701, size=300).astype(np.uint32)
    n = lens.size
    soff = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    src = rng.integers(0, 256, size=int(lens.sum()), dtype=np.uint8)
    qkeys, guids = random_meta(rng, n)
    qkeys[:] = np.frombuffer(QK, np.uint8)
    w = S.PartitionWriter(lease_id=7, partition_id=2)
    w.queue_op(S.OP_CREATION, QK)
    jfile, dfile = w.files()
    for corrupt in (False, True):
        dst, jour, roff, _, _ = pack_records(
            _t(cuda, src, np.uint8), _t(cuda, soff, np.int64), _t(cuda, lens, np.uint32),
            _t(cuda, qkeys, np.uint8), _t(cuda, guids, np.uint8), file_key=b"\x11\x22\x33\x44\x55",
            lease_id=7, first_seq=2, data_file_pos=40)
        victim = 123
        if corrupt:   # a bit rots in the primary's HBM after the record was written
            assert lens[victim] > 5
            dst[int(roff[victim].item()) + 12 + 5] ^= 0x04
        journal = torch.cat([_t(cuda, jfile[JH:], np.uint8), jour])
        want = S.verify_partition(np.concatenate([jfile[:JH], journal.cpu().numpy()]),
                                  np.concatenate([dfile, dst.cpu().numpy()]))
        p = pack_storage_events(journal, dst, journal_pos=JH, data_file_pos=40, partition_id=2,
                                event_first=_t(cuda, _cuts(n + 1, 25).view(np.int64), np.int64))
        assert p.result["n_bad"] == int(corrupt)
        assert p.result["first_bad"] == (victim + 1 if corrupt else n + 1)
        a = apply_events(p.events, p.event_offsets, partition_id=2, journal_pos=JH,
                         data_file_pos=40)
        assert a.result["n_bad"] == int(corrupt) and a.result["n_msgs"] == n + 1
        assert torch.equal(a.journal, journal) and torch.equal(a.data, dst)
        select, sel = select_records(a.journal, data_file_bytes=40 + a.data.numel())
        u = unpack_records(a.journal, a.data, data_file_pos=40, select=select, verify=True)
        res = last_records_unpack(cuda.index, torch.cuda.current_stream(cuda))
        assert (sel["recovery_rc"], res["refused_kind"]) == (want["recovery_rc"], 0) == (0, 0)
        assert (res["n_msgs"], res["n_bad"]) == (want["n_messages"], want["n_bad"])
        assert want["n_messages"] == n and want["n_bad"] == int(corrupt)
        if corrupt:
            index = int(u.record_index[res["first_bad"]].item())
            assert list(want["bad_record_offsets"]) == [JH + 60 * index] and index == victim + 1


# ---- past one tile per block ----------------------------
#
# One run of N_FRAME records (record_pool.py: all five record types and four
# queue ops in every block, DATA records of varied sizes behind headers of 12
# to 28 bytes, two messages longer than a chunk of the copy), written once; the
# smaller sizes are its prefixes.  The expected bytes are storage_events_fast's,
# which test_storage_pack_model.py holds to the loop model and to
# StorageEventBuilder.  A model is built for the case that needs it and dropped
# with it: an image is up to 61 MB.

def _split(n, how):
    """event_first of n records: events of 3, every record its own event, one
    event (None), or test_grid_regimes.py's split at the seal's boundary."""
    if how == "of_3":
        return np.array(G.events_of_3(n), np.uint64)
    if how == "own":
        return np.arange(n + 1, dtype=np.uint64)
    if how == "boundary":
        return np.array(G.boundary_split(n, G.regime(n).per_block), np.uint64)
    assert how is None
    return None


def _fast(run, d, kw, **changes):
    """storage_events_fast's answer to the call `kw` with room to spare, the
    CRCs taken from the pool's."""
    kw = dict(kw, **changes)
    kw.pop("dst_alloc", None)
    if kw["dst_bytes"] is None:
        del kw["dst_bytes"]
    return M.storage_events_fast(run, d, record_crcs=R.pool().crcs[:len(run) // 60], **kw)


@functools.lru_cache(maxsize=None)
def _message_bytes():
    """72 + the DATA record's bytes of every record of the pool."""
    p = R.pool()
    size = np.full(G.N_FRAME, 72, np.int64)
    size[p.msgs] += R.data_fields(p.run, p.data, p.msgs)[2]
    size.setflags(write=False)
    return size


def _event_offsets(n, first):
    before = np.concatenate([[0], np.cumsum(_message_bytes()[:n])])
    first = np.asarray(first).astype(np.int64)
    return 8 * np.arange(first.size) + before[first]


def _large_case(name):
    """(records, DATA file as passed, keywords) of a large success case."""
    n, how, changes = {
        "waves-events_of_3-flags": (G.N_WAVES, "of_3", {}),
        "full-one_event-header_fields": (G.N_FULL, None, dict(
            event_type=E.EVENT_TYPE_PARTITION_SYNC, storage_protocol_version=2,
            partition_id=65535)),
        "tiles-own_events": (G.N_TILES, "own", {}),
        "tiles-window": (G.N_TILES, "of_3", dict(data_file_pos=40)),
        "tiles-largest_journal_pos": (G.N_TILES, "of_3", dict(
            journal_pos=4 * ((1 << 32) - 1) - 60 * G.N_TILES)),
        "frame-own_events": (G.N_FRAME, "own", {}),
        "frame-events_of_3": (G.N_FRAME, "of_3", {}),
        "frame-seal_boundary": (G.N_FRAME, "boundary", {}),
    }[name]
    run, d = R.records(n)
    if name.startswith("waves"):
        # eight random bits a record: the low five are sent
        changes["flags"] = np.random.default_rng(30).integers(0, 256, size=n, dtype=np.uint8)
    kw = _kw(run, d, event_first=_split(n, how), **changes)
    return run, d[kw["data_file_pos"]:], kw


LARGE = ["waves-events_of_3-flags", "full-one_event-header_fields", "tiles-own_events",
         "tiles-window", "tiles-largest_journal_pos", "frame-own_events", "frame-events_of_3",
         "frame-seal_boundary"]


@pytest.mark.parametrize("name", LARGE)
def test_past_one_tile_per_block(cuda, name):
    # N_WAVES: 66 blocks, the 18-dword frame loop in its third step.  N_FULL:
    # all 256 blocks under one event.  N_TILES: two tiles a block; with an
    # event per record a block spans 2,048 events and seal_offsets searches
    # event_first in global memory.  N_FRAME: three tiles a block, the
    # per-record loop of k_spk_frame in its second step (record 524,288), three
    # steps of the shape check and of events_check and two of event_headers;
    # events of 3 fill the seal's LDS array exactly, the boundary split is one
    # event past it from block SEAL_BLOCK on.
    run, d, kw = _large_case(name)
    n = len(run) // 60
    r = G.regime(n)
    assert r.dwords_past_grid and r.cross_wave and r.units_past_grid == (n == G.N_FRAME)
    want = _fast(run, d, kw)
    assert want.result["n_bad"] == 0 and want.result["n_data"] == int((R.pool().msgs < n).sum())
    assert sorted(set(want.types.tolist())) == [1, 2, 3, 4, 5, 6]
    if name == "tiles-largest_journal_pos":
        at = int(want.event_offsets[-2]) + 8 + int(_message_bytes()[n - 3:n - 1].sum())
        assert want.events[at + 8:at + 12].tolist() == [0xFF, 0xFF, 0xFF, 0xF0]
    if name.startswith("waves"):
        assert int((kw["flags"] > 31).sum()) > n // 2
    m, _ = _check(cuda, run, d, kw, model=want)
    assert m is want


def test_past_one_tile_per_block_on_a_side_stream(cuda):
    import torch
    run, d = R.records(G.N_TILES)
    kw = _kw(run, d, event_first=_split(G.N_TILES, "of_3"))
    want = _fast(run, d, kw)
    torch.cuda.synchronize(cuda)
    s = _side_stream(cuda)
    with torch.cuda.stream(s):
        _check(cuda, run, d, kw, sync=False, stream=s, model=want)


def test_stored_crc_mismatches_in_every_step_of_the_frame_loop(cuda):
    # the stored CRC (journal bytes 52..55) of the MESSAGE record nearest to
    # records 999, 1,999, ... flipped, of its next MESSAGE record in the same
    # wave for the first, and of record 524,288, which a frame thread reaches
    # in its second step alone
    n = G.N_FRAME
    run, d = R.records(n)
    msgs = R.pool().msgs
    at = np.searchsorted(msgs, np.arange(999, n, 1000))
    at = np.unique(np.concatenate([at[at < msgs.size], [at[0] + 1, msgs.size - 1]]))
    victims = msgs[at]
    assert victims[0] // 64 == victims[1] // 64 == 999 // 64 and victims[-1] == n - 1 == 524288
    assert victims.size == 526 and int(np.abs(victims[2:-1] - np.arange(1999, n, 1000)).max()) < 8
    bad = run.copy()
    bad[60 * victims[:, None] + 52 + np.arange(4)] ^= np.array([0x80, 1, 0, 0x10], np.uint8)
    kw = _kw(run, d, event_first=_split(n, "own"))
    want = _fast(bad, d, kw)
    assert (want.result["n_bad"], want.result["first_bad"]) == (526, int(victims[0]))
    m, host = _check(cuda, bad, d, kw, model=want)
    assert np.array_equal(np.flatnonzero(host["out"][:n] != want.expected), victims)
    # sent as stored: record i's bytes 52..55 behind event i's EventHeader and
    # the StorageHeader
    sent = host["dst"][want.event_offsets[victims].astype(np.int64)[:, None] + 8 + 12 + 52 +
                       np.arange(4)]
    assert np.array_equal(sent, bad.reshape(-1, 60)[victims, 52:56])
    assert not np.array_equal(sent, run.reshape(-1, 60)[victims, 52:56])


def _refused_both_ways(cuda, run, d, kw, want):
    """The call refused as `want`, synchronous and asynchronous, into a
    destination that would hold every event, with nothing written."""
    n = len(run) // 60
    first = kw["event_first"]
    room = int(_event_offsets(n, first if first is not None else [0, n])[-1])
    kw = dict(kw, dst_alloc=room)
    if kw["dst_bytes"] is None:
        kw["dst_bytes"] = room
    for sync in (True, False):
        m, _ = _check(cuda, run, d, kw, sync=sync, model=want)
        assert m == want


def test_record_refusals_across_tiles_and_blocks(cuda):
    n = G.N_TILES
    run, d = R.records(n)
    types = run.reshape(-1, 60)[:, 0] >> 4
    r = G.regime(n)
    assert (r.nblocks, r.per_block) == (129, 2048)
    kw = _kw(run, d, event_first=_split(n, "of_3"))
    room = dict(dst_bytes=1 << 40, crc32c=CRC)
    # (a) the magic of record 1,024 + 5, in the second tile of block 0, and of
    # record 2,048 + 3, in the first tile of block 1: the lower one
    bad = run.copy()
    for i in (1029, 2051):
        bad[60 * i + 59] ^= 0xFF
    want = M.Refusal(M.RECORD_HEADER, 1029)
    assert M.pack(bad[:60 * 2100], d, **dict(_kw(run, d), **room)) == want
    _refused_both_ways(cuda, bad, d, kw, want)
    # (b) the last padding byte of a DATA record below record 100 made 9 and
    # primaryLeaseId 0 in record 200,001: the lower kind wins over the lower index
    # (of 9 bytes or more with its padding: a check that lets it pass still
    # finds a length inside the record)
    early = R.pool().msgs[:60]
    at, lead, rec, length, _ = R.data_fields(run, d, early)
    pick = int(np.flatnonzero(rec - lead >= 16)[3])
    victim, at, rec = int(early[pick]), at[pick:], rec[pick:]
    assert 3 < victim < 100
    data = d.copy()
    data[int(at[0] + rec[0]) - 1] = 9
    assert M.pack(run[:60 * 100], data, **dict(_kw(run, d), **room)) == M.Refusal(
        M.DATA_RECORD, victim)
    _refused_both_ways(cuda, run, data, kw, M.Refusal(M.DATA_RECORD, victim))
    bad = run.copy()
    bad[60 * 200001 + 8:60 * 200001 + 12] = 0
    _refused_both_ways(cuda, bad, data, kw, M.Refusal(M.RECORD_HEADER, 200001))
    # (c) the last record of the last block, the 1,025th record of block 128,
    # and the last MESSAGE record: a data offset of 0
    last = n - 1
    assert last - (r.nblocks - 1) * r.per_block == 1024
    last_msg = int(R.pool().msgs[R.pool().msgs < n][-1])
    bad = run.copy()
    C.put32(bad, 60 * last_msg + 32, 0)
    tail = 60 * (n - 50)
    assert last_msg >= n - 50
    assert M.pack(bad[tail:], d, **dict(_kw(run, d), **room)) == M.Refusal(
        M.DATA_OFFSET, last_msg - (n - 50))
    _refused_both_ways(cuda, bad, d, kw, M.Refusal(M.DATA_OFFSET, last_msg))
    if types[last] != S.REC_MESSAGE:
        bad[60 * last + 59] ^= 0xFF
        assert M.pack(bad[tail:], d, **dict(_kw(run, d), **room)) == M.Refusal(
            M.RECORD_HEADER, 49)
        _refused_both_ways(cuda, bad, d, kw, M.Refusal(M.RECORD_HEADER, last))
    assert last_msg // r.per_block == r.nblocks - 1


def test_payload_cap_at_the_long_message_of_a_second_tile(cuda):
    n = G.N_TILES
    run, d = R.records(n)
    long = R.pool().long[0]
    size = 60 + int(R.data_fields(run, d, np.array([long]))[2][0])
    assert size == int(_message_bytes().max()) - 12 and 1024 <= long < 2048
    kw = _kw(run, d, event_first=_split(n, "of_3"))
    want = M.Refusal(M.PAYLOAD_TOO_BIG, long)
    assert M.pack(run[:60 * 1600], d, crc32c=CRC,
                  **dict(_kw(run, d), dst_bytes=1 << 40, max_payload_bytes=size - 4)) == want
    assert _fast(run, d, kw, max_payload_bytes=size - 4) == want
    _refused_both_ways(cuda, run, d, dict(kw, max_payload_bytes=size - 4), want)
    # the cap exactly the longest message
    kw["max_payload_bytes"] = size
    _check(cuda, run, d, kw, model=_fast(run, d, kw))


def _shape_refusal(first, n):
    """The lowest entry of event_first that breaks its shape."""
    first = np.asarray(first).astype(np.int64)
    bad = np.concatenate([first[:-1] >= first[1:], [first[-1] != n]])
    bad[0] |= first[0] != 0
    return M.Refusal(M.EVENT_FIRST, int(np.flatnonzero(bad)[0]))


def test_event_first_refused_in_a_late_step_of_the_shape_loop(cuda):
    # one event per record at N_FRAME: 175,104 threads over 524,290 entries.
    # Every bad entry is itself an index below n
    n = G.N_FRAME
    run, d = R.records(n)
    threads = G.regime(n).nblocks * 1024
    assert 2 * threads < n < 3 * threads
    good = _split(n, "own")

    def refused(index, entries):
        first = good.copy()
        for e, v in entries.items():
            first[e] = v
        assert int(first.max()) <= n and all(v < n for v in entries.values())
        want = M.Refusal(M.EVENT_FIRST, index)
        assert _shape_refusal(first, n) == want
        kw = _kw(run, d, event_first=first)
        room = int(_event_offsets(n, good)[-1])
        for sync in (True, False):
            m, _ = _check(cuda, run, d, dict(kw, dst_bytes=room), sync=sync, model=want)
            assert m == want

    late = 2 * threads + 50000            # read in the third step alone
    refused(late, {late: late + 1})       # equal to the next entry
    # the last entry is n - 1, not n: the entry before it is then not below
    # it either, and is the one named
    refused(n - 1, {n: n - 1})
    # a high entry of an early thread's third step, a lower one of a later
    # thread's second step: the lower index
    high, low = 2 * threads + 10, threads + 170000
    refused(low, {high: high + 1, low: low + 1})


def test_event_size_cap_past_one_tile_per_block(cuda):
    # events of 3 at N_TILES but for two of 3,000 and 4,500 records, whose first
    # records lie in the second tiles of blocks 70 and 100: p0 there is off[f0],
    # with the tile carry in it, plus bpre[f0 / 2048]
    n = G.N_TILES
    per_block = G.regime(n).per_block
    run, d = R.records(n)
    ia, ib = 70 * per_block + 1102, 100 * per_block + 1024
    cuts = [c for c in G.events_of_3(n) if not ia < c < ia + 3000 and not ib < c < ib + 4500]
    first = np.array(cuts, np.uint64)
    ea, eb = cuts.index(ia), cuts.index(ib)
    for i in (ia, ib):
        assert i % 3 == 0 and i % per_block >= 1024 and i // per_block in (70, 100)
    sizes = np.diff(_event_offsets(n, first))
    order = np.argsort(sizes)
    assert [int(e) for e in order[-2:]] == [ea, eb] and sizes[order[-3]] < sizes[ea] - 4 and \
        sizes[ea] < sizes[eb] - 4
    kw = _kw(run, d, event_first=first)
    # one event over the cap, then two: the lower index
    for cap, event in ((int(sizes[eb]) - 4, eb), (int(sizes[ea]) - 4, ea)):
        want = M.Refusal(M.EVENT_TOO_BIG, event)
        assert _fast(run, d, kw, max_event_bytes=cap) == want
        _refused_both_ways(cuda, run, d, dict(kw, max_event_bytes=cap), want)
    # the cap exactly the largest event
    kw["max_event_bytes"] = int(sizes[eb])
    _check(cuda, run, d, kw, model=_fast(run, d, kw))


def test_destination_size_past_one_tile_per_block(cuda):
    n = G.N_TILES
    run, d = R.records(n)
    first = _split(n, "of_3")
    ev = _event_offsets(n, first)
    total, n_events = int(ev[-1]), ev.size - 1
    kw = _kw(run, d, event_first=first)
    want = M.Refusal(M.DST_TOO_SMALL, n_events - 1)
    assert _fast(run, d, kw, dst_bytes=total - 4) == want
    _refused_both_ways(cuda, run, d, dict(kw, dst_bytes=total - 4), want)
    # half the image: the first event that ends past it, while every later one
    # refuses as well
    want = _fast(run, d, kw, dst_bytes=total // 2)
    assert want.kind == M.DST_TOO_SMALL and n_events // 3 < want.index < 2 * n_events // 3
    assert ev[want.index] <= total // 2 < ev[want.index + 1]
    _refused_both_ways(cuda, run, d, dict(kw, dst_bytes=total // 2), want)
    # one event per record at N_FRAME: some 260,000 events refuse, over three
    # steps of every block of the check grid
    n = G.N_FRAME
    run, d = R.records(n)
    first = _split(n, "own")
    ev = _event_offsets(n, first)
    half = int(ev[-1]) // 2
    index = int(np.searchsorted(ev[1:], half, side="right"))
    assert ev[index] <= half < ev[index + 1] and n - index > 200000
    kw = _kw(run, d, event_first=first)
    _refused_both_ways(cuda, run, d, dict(kw, dst_bytes=half), M.Refusal(M.DST_TOO_SMALL, index))
