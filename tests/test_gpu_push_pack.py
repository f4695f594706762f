"""Stored messages packed into PUSH events on the GPU (bmqcrc_push_event_pack,
ABI 2.17).  The oracle throughout is tests/push_pack_model.py.  Every raw call
hands the library a sentinel-filled destination and output arrays with guard
bytes and elements behind them: the guards are checked after every call, and
every byte and element after a refused one."""
import ctypes
import functools

import numpy as np
import pytest

from blazingmq_amd import (BmqCrcError, Crc32c, PushMessageIterator, _native as N, apply_events,
                           last_copy, last_journal_select, last_launch, last_push_pack,
                           last_put_pack, last_put_unpack, last_records_pack,
                           last_records_unpack, last_storage_apply, last_storage_pack,
                           pack_events, pack_push_events, pack_records, pack_storage_events,
                           select_records, unpack_events, unpack_records)
from blazingmq_amd import push_event as E
from blazingmq_amd import storage as S
from blazingmq_amd import synth
import push_pack_cases as C
import push_pack_model as M
import put_pack_model as P
import put_unpack_model as PU
import device_views as V
import record_pool as R
import test_grid_regimes as G

pytestmark = pytest.mark.gpu

GUARD = 8      # elements behind every output array
SLACK = 64     # bytes behind every input buffer and the destination
SENTINEL = 0xC3
JH = S.PartitionWriter.JOURNAL_HEADER
CANARY = {"event_offsets": 0x5A5A5A5A5A5A5A5A, "out": 0x5A5A5A5A, "lengths": 0xA5A5A5A5}
NP = {"event_offsets": np.uint64, "out": np.uint32, "lengths": np.uint32}
MODEL = {"event_offsets": "event_offsets", "out": "crcs", "lengths": "lengths"}
KIND_NAME = {k: ("BMQCRC_PUSH_PACK_" + n).encode() for k, n in enumerate(E.PACK_REFUSALS) if k}
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


def _kw(n, **changes):
    """Keywords of a call of n messages into a destination of the exact size
    (the model refuses a smaller one)."""
    kw = dict(data_file_pos=0, queue_ids=(np.arange(n) * 7 - 3).astype(np.int32), records=None,
              flags=None, option_mode=0, rda=None, sub_ids=None, event_first=None,
              max_event_bytes=0, max_payload_bytes=0, dst_bytes="exact")
    kw.update(changes)
    return kw


def _raw(cuda, run, data, kw, sync=True, stream=None, skip=(), phases=None):
    """One bmqcrc_push_event_pack over device tensors into a sentinel-filled
    destination and arrays; dst_bytes None is the size-only call.  Returns (rc,
    error text, result of the call or of bmqcrc_last_push_pack, everything
    written on the host with its guards).  `phases` maps every pointer of the
    call (journal, data, records, queue_ids, flags, rda, sub_ids, event_first,
    dst, event_offsets, out, lengths) to the phase of its base; the sentinel
    margins around each are checked after the call.  None: every buffer starts
    its allocation."""
    import torch
    place = V.Placer(cuda, phases) if phases is not None else None
    stream = stream or torch.cuda.current_stream(cuda)
    n = len(kw["queue_ids"])
    first = kw["event_first"]
    n_events = 1 if first is None else len(first) - 1
    count = {"event_offsets": n_events + 1, "out": n, "lengths": n}
    with torch.cuda.stream(stream):
        d_run, d_data = _dev(cuda, run, place, "journal"), _dev(cuda, data, place, "data")
        spare = torch.zeros(8, dtype=torch.uint8, device=cuda)
        ins = {}
        for name, dt in (("records", np.uint32), ("queue_ids", np.int32), ("flags", np.uint8),
                         ("rda", np.uint8), ("sub_ids", np.uint32)):
            if kw[name] is not None and place is not None:
                ins[name] = place.put(name, np.asarray(kw[name]).astype(dt))
            elif kw[name] is not None:
                ins[name] = _t(cuda, np.asarray(kw[name]).astype(dt), dt)
        if first is None:
            d_first = None
        elif place is not None:
            d_first = place.put("event_first", np.asarray(first, np.uint64))
        else:
            d_first = _t(cuda, np.asarray(first, np.uint64).view(np.int64), np.int64)
        arr = {}
        if kw["dst_bytes"] is not None and place is not None:
            arr["dst"] = place.fill("dst", kw["dst_bytes"] + SLACK, np.uint8, SENTINEL)
        elif kw["dst_bytes"] is not None:
            # (`dst_alloc`: a destination declared shorter than its allocation)
            size = max(kw["dst_bytes"], kw.get("dst_alloc", 0))
            arr["dst"] = torch.full((size + SLACK,), SENTINEL, dtype=torch.uint8, device=cuda)
        for name, dt in NP.items():
            if name in skip:
                continue
            if place is not None:
                arr[name] = place.fill(name, count[name] + GUARD, dt, CANARY[name])
                continue
            fill = np.array([CANARY[name]], np.uint64).astype(dt)
            arr[name] = torch.from_numpy(np.repeat(fill, count[name] + GUARD).view(
                {np.uint32: np.int32, np.uint64: np.int64}.get(dt, dt))).to(cuda)
        p = N.PushPack()
        p.struct_size = ctypes.sizeof(N.PushPack)
        p.journal, p.journal_bytes = d_run.data_ptr() or spare.data_ptr(), d_run.numel()
        p.n_records, p.n = len(run) // 60, n
        p.data, p.data_bytes = d_data.data_ptr() or spare.data_ptr(), d_data.numel()
        p.data_file_pos, p.option_mode = kw["data_file_pos"], kw["option_mode"]
        for name in ("records", "queue_ids", "flags", "rda", "sub_ids"):
            # (an empty tensor has no address: the call wants one)
            setattr(p, name, (ins[name].data_ptr() or spare.data_ptr()) if name in ins else None)
        p.queue_ids = p.queue_ids or spare.data_ptr()
        p.event_first = d_first.data_ptr() if d_first is not None else None
        p.n_events = n_events
        p.max_event_bytes, p.max_payload_bytes = kw["max_event_bytes"], kw["max_payload_bytes"]
        if "dst" in arr:
            p.dst, p.dst_bytes = arr["dst"].data_ptr(), kw["dst_bytes"]
        for name in NP:
            setattr(p, name, arr[name].data_ptr() if name in arr else None)
        o = N.make_opts(device=cuda.index, stream=stream.cuda_stream,
                        flags=N.BMQCRC_F_DEVICE_PTRS | (0 if sync else N.BMQCRC_F_ASYNC))
        r = N.PushPackResult()
        rc = N.lib.bmqcrc_push_event_pack(ctypes.byref(p), ctypes.byref(r), ctypes.byref(o))
        err = N.lib.bmqcrc_last_error()
        res = r.as_dict() if sync else last_push_pack(cuda.index, stream)
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
    every destination byte, array entry and result field.  `dst_bytes` "exact"
    is the exact size, None the size-only call.  `phases`: as in _raw.  Returns
    (model, host)."""
    kw = dict(kw)
    if kw["dst_bytes"] == "exact":
        kw["dst_bytes"] = 1 << 40
        m = M.pack(run, data, crc32c=CRC, **kw) if model is None else model
        kw["dst_bytes"] = m.result["total_bytes"] if isinstance(m, M.Packed) else 4096
    m = model if model is not None else M.pack(run, data, crc32c=CRC, **kw)
    rc, err, res, host = _raw(cuda, run, data, kw, sync=sync, stream=stream, skip=skip,
                              phases=phases)
    n = len(kw["queue_ids"])
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
    if "dst" in host:
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
def _messages(n, seed=7, options=False, lengths=None, mixed=False):
    """(record run, DATA file, the MESSAGE records' indices): n messages of
    0..40 bytes (or of `lengths`, in turn).  With `options` DATA headers of 3
    and 5 words with 0..2 option words, random DataHeader flags, schema ids
    and CAT bytes; with `mixed` a queue's CREATION in front, CONFIRM and
    DELETION records between the messages and a queue PURGE or a sync point in
    front of every 16th.  Shared, never modified."""
    rng = np.random.default_rng(seed)
    w = S.PartitionWriter(lease_id=4, partition_id=1)
    msgs = []
    if mixed:
        w.queue_op(S.OP_CREATION, QK)
    for k in range(n):
        if mixed and k % 16 == 15:
            if k % 32 == 15:
                w.sync_point()
            else:
                w.queue_op(S.OP_PURGE, QK, b"\1\2\3\4\5")
        size = int(rng.integers(0, 41)) if lengths is None else lengths[k % len(lengths)]
        app = rng.integers(0, 256, size=size, dtype=np.uint8).tobytes()
        before = w.dpos
        msgs.append(len(w.recs))
        _, guid = w.message(app, QK, data_flags=k & 0xFF)
        if options:
            hw, opt = (3, 5)[int(rng.integers(0, 2))], int(rng.integers(0, 3))
            lead = 4 * (hw + opt)
            total = (lead + len(app)) // 8 * 8 + 8
            pad = total - lead - len(app)
            w.data[-1] = (((hw << 29) | (total // 4)).to_bytes(4, "big") +
                          ((opt << 8) | int(rng.integers(0, 256))).to_bytes(4, "big") +
                          bytes(rng.integers(0, 256, size=lead - 8, dtype=np.uint8)) + app +
                          bytes([pad]) * pad)
            w.dpos = before + total
            r = bytearray(w.recs[-1])
            r[21] = int(rng.integers(0, 256))      # CAT in the low 3 bits
            w.recs[-1] = bytes(r)
        if mixed and k % 3 == 0:
            w.confirm(guid, QK)
        if mixed and k % 9 == 0:
            w.deletion(guid, QK)
    j, d = w.files()
    run = j[JH:]
    run.setflags(write=False)
    d.setflags(write=False)
    return run, d, tuple(msgs)


# ---- wave, tile and grid edges -----------------------------------------------

@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 1023, 1024, 1025])
def test_message_counts(cuda, count):
    run, d, _ = _messages(1025)
    run = run[:60 * count]
    m, _ = _check(cuda, run, d, _kw(count, option_mode=1, rda=np.arange(count) % 256))
    assert m.result["n_msgs"] == count


@pytest.mark.parametrize("per_event", [1, 3, 17, 40, 1024])
def test_event_cuts(cuda, per_event):
    # every message its own event; cuts inside a wave's 64 messages; a cut at a
    # block's boundary, message 1,024
    n = 1025 if per_event == 1024 else 140
    run, d, _ = _messages(1025)
    run = run[:60 * n]
    m, _ = _check(cuda, run, d, _kw(n, event_first=_cuts(n, per_event)))
    assert m.result["n_events"] == -(-n // per_event)


def _uniform(run, d, records, qids, rda, first):
    """The events of messages that all carry 16 bytes, in option mode 1, from
    the formulas alone: 56 bytes a message."""
    records = np.asarray(records, np.int64)
    n = records.size
    recs = run.reshape(-1, 60)[records]
    at = 8 * recs[:, 32:36].astype(np.int64).dot([1 << 24, 1 << 16, 1 << 8, 1]) + 12
    msg = np.zeros((n, 56), np.uint8)
    msg[:, 0] = (d[at - 5] & 1) << 5           # MESSAGE_PROPERTIES from DataHeader.flags
    msg[:, 3] = 8 + 1 + 5                      # MessageWords
    msg[:, 6:8] = (1, 8)                       # OptionsWords 1 | CAT 0 | HeaderWords 8
    msg[:, 8:12] = np.asarray(qids, ">i4").view(np.uint8).reshape(n, 4)
    msg[:, 12:28] = recs[:, 36:52]
    msg[:, 32] = (3 << 2) | 2                  # SUB_QUEUE_INFOS, packed
    msg[:, 35] = rda
    msg[:, 36:52] = d[at[:, None] + np.arange(16)]
    msg[:, 52:] = 4
    first = np.asarray(first, np.int64)
    sizes = 8 + 56 * np.diff(first)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    out = np.zeros(int(starts[-1]), np.uint8)
    where = np.repeat(8 * (np.arange(first.size - 1) + 1), np.diff(first)) + 56 * np.arange(n)
    out[where[:, None] + np.arange(56)] = msg
    head = np.zeros((first.size - 1, 8), np.uint8)
    head[:, 0:4] = sizes.astype(">u4").view(np.uint8).reshape(-1, 4)
    head[:, 4:6] = ((1 << 6) | 4, 2)
    out[starts[:-1, None] + np.arange(8)] = head
    return out, starts.astype(np.uint64)


@pytest.mark.parametrize("n_events", [5, 0])
def test_a_quarter_million_messages(cuda, n_events):
    # 262,145 messages: the first size at which a layout block takes a second
    # tile and the carry matters -- a gather with repeats over 1,024 records of
    # 16 bytes.  The expected bytes are _uniform's, held equal to the model on
    # the first 100 messages here.  With every message its own event
    # (n_events 0) a block's 2,048 messages lie in more events than the seal
    # searches in LDS
    import torch
    n = 256 * 1024 + 1
    run, d, _ = _messages(1024, seed=12, lengths=(16,))
    records = (np.arange(n, dtype=np.int64) * 7919 + 5) % 1024
    qids = (np.arange(n) - 70000).astype(np.int32)
    rda = (np.arange(n) % 251).astype(np.uint8)
    first = _cuts(n, -(-n // n_events)) if n_events else np.arange(n + 1, dtype=np.uint64)
    small = M.pack(run, d, crc32c=CRC, **_kw(100, queue_ids=qids[:100], records=records[:100],
                                             option_mode=1, rda=rda[:100],
                                             event_first=[0, 33, 100], dst_bytes=1 << 20))
    got, offs = _uniform(run, d, records[:100], qids[:100], rda[:100], [0, 33, 100])
    assert np.array_equal(got, small.events) and np.array_equal(offs, small.event_offsets)
    want, want_offsets = _uniform(run, d, records, qids, rda, first)
    dst = torch.full((want.size + SLACK,), SENTINEL, dtype=torch.uint8, device=cuda)
    p = pack_push_events(torch.from_numpy(run.copy()).to(cuda), _dev(cuda, d), data_file_pos=0,
                         queue_ids=_t(cuda, qids, np.int32),
                         records=_t(cuda, records.astype(np.uint32), np.uint32), option_mode=1,
                         rda=_t(cuda, rda, np.uint8),
                         event_first=_t(cuda, first.view(np.int64), np.int64),
                         dst=dst[:want.size])
    assert p.result == dict(n_events=first.size - 1, n_msgs=n, total_bytes=want.size, n_bad=0,
                            first_bad=n, refused_kind=0, refused_index=0)
    assert torch.equal(p.events.cpu(), torch.from_numpy(want))
    assert bool((dst[want.size:] == SENTINEL).all())
    assert np.array_equal(p.event_offsets.cpu().numpy().view(np.uint64), want_offsets)
    assert bool((p.lengths == 16).all())
    crcs = small.crcs[np.argsort(records[:100])]
    order = np.sort(records[:100])
    by_record = dict(zip(order.tolist(), crcs.tolist()))
    got_crcs = p.crcs.cpu().numpy().view(np.uint32)
    assert all(got_crcs[m] == by_record[int(records[m])] for m in range(0, n, 4099)
               if int(records[m]) in by_record)
    assert np.array_equal(got_crcs[:100], small.crcs)


# ---- what the messages carry -------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_option_modes_and_the_header_fields(cuda, mode):
    # queue ids -1 and 2^31 - 1, RDA 0 and 255, sub-queue id 2^32 - 1, both
    # values of the flag; CAT, SchemaId and MESSAGE_PROPERTIES from the records
    n = 260
    run, d, _ = _messages(n, seed=8, options=True)
    qids = (np.arange(n) * 16777259 % (1 << 32)).astype(np.uint32).view(np.int32)
    qids[:4] = (-1, (1 << 31) - 1, -(1 << 31), 0)
    rda = (np.arange(n) * 37 % 256).astype(np.uint8)
    rda[:2] = (0, 255)
    sub = (np.arange(n) * 2654435761 % (1 << 32)).astype(np.uint32)
    sub[:2] = ((1 << 32) - 1, 0)
    flags = (np.arange(n) % 3 == 0).astype(np.uint8) * 4
    kw = _kw(n, queue_ids=qids, flags=flags, option_mode=mode,
             rda=rda if mode in (1, 3) else None, sub_ids=sub if mode in (2, 3) else None,
             event_first=_cuts(n, 33))
    m, host = _check(cuda, run, d, kw)
    got = [ms for e in range(len(m.event_offsets) - 1) for ms in PushMessageIterator(
        host["dst"][int(m.event_offsets[e]):int(m.event_offsets[e + 1])], allow_empty=True)]
    assert [ms["queue_id"] for ms in got] == qids.tolist()
    assert [ms["flags"] & 4 for ms in got] == flags.tolist()
    want = {0: [[]] * n, 1: [[(0, int(r))] for r in rda], 2: [[(int(s), None)] for s in sub],
            3: [[(int(s), int(r))] for s, r in zip(sub, rda)]}[mode]
    assert [ms["sub_queue_infos"] for ms in got] == want
    # from the records, read here by hand
    at = [8 * int.from_bytes(run[60 * i + 32:60 * i + 36].tobytes(), "big") for i in range(n)]
    assert [ms["compression"] for ms in got] == [int(run[60 * i + 21]) & 7 for i in range(n)]
    assert [ms["schema_id"] for ms in got] == [
        int.from_bytes(d[o + 8:o + 10].tobytes(), "big") for o in at]
    assert [ms["flags"] >> 1 & 1 for ms in got] == [int(d[o + 7]) & 1 for o in at]
    assert [ms["guid"] for ms in got] == [run[60 * i + 36:60 * i + 52].tobytes()
                                          for i in range(n)]
    assert len({ms["compression"] for ms in got}) == 8 and {ms["flags"] for ms in got} == {
        0, 2, 4, 6}


def test_header_sizes_option_words_and_every_alignment(cuda):
    run, d, _ = _messages(700, seed=8, options=True)
    m, _ = _check(cuda, run, d, _kw(700, option_mode=1, rda=np.arange(700) % 256,
                                    event_first=_cuts(700, 50)))
    # The copy cuts a message on the 16-byte pieces of its destination and reads
    # its source with unaligned 16-byte loads.  DATA records start on multiples
    # of 8 behind headers and options of 12 to 28 bytes, PUSH messages on any
    # multiple of 4: every 4-byte phase of source and destination inside a
    # piece occurs, in all 16 pairs
    leads, pairs, pos = set(), set(), []
    for e in range(len(m.event_offsets) - 1):
        beg = int(m.event_offsets[e])
        pos += [beg + ms["app_offset"] for ms in PushMessageIterator(
            m.events[beg:int(m.event_offsets[e + 1])], allow_empty=True)]
    for i in range(700):
        o = 8 * int.from_bytes(run[60 * i + 32:60 * i + 36].tobytes(), "big")
        lead = 4 * ((int(d[o]) >> 5) + (int.from_bytes(d[o + 4:o + 7].tobytes(), "big")))
        leads.add(lead)
        pairs.add(((o + lead) % 16 // 4, pos[i] % 16 // 4))
    assert leads == {12, 16, 20, 24, 28} and len(pairs) == 16


def test_application_data_lengths(cuda):
    # 0 and 1..24 (every padding value), 255..257, 64 KiB, and 300 KiB + 3: the
    # copy's long path
    lengths = tuple(range(25)) + (255, 256, 257, 64 * 1024, 300 * 1024 + 3)
    n = len(lengths)
    run, d, _ = _messages(n, seed=9, lengths=lengths)
    for mode in (0, 3):
        kw = _kw(n, option_mode=mode, event_first=_cuts(n, 17))
        if mode:
            kw.update(rda=np.arange(n), sub_ids=np.arange(n) + 5)
        m, _ = _check(cuda, run, d, kw)
        assert m.lengths.tolist() == list(lengths) and m.result["n_bad"] == 0


# ---- gathers -----------------------------------------------------------------

@pytest.mark.parametrize("gather", ["identity", "reversed", "three_times", "skipping"])
def test_gathers(cuda, gather):
    n = 200
    if gather == "skipping":
        run, d, msgs = _messages(n, seed=10, mixed=True)
        types = {int(run[60 * i]) >> 4 for i in range(run.size // 60)}
        assert types == {S.REC_MESSAGE, S.REC_CONFIRM, S.REC_DELETION, S.REC_QUEUE_OP,
                         S.REC_JOURNAL_OP}
        records = np.array(msgs)
    else:
        run, d, msgs = _messages(n, seed=10)
        records = {"identity": None, "reversed": np.arange(n)[::-1],
                   "three_times": np.repeat(np.arange(n), 3)}[gather]
    count = n if records is None else len(records)
    kw = _kw(count, records=records, option_mode=2, sub_ids=np.arange(count),
             event_first=_cuts(count, 41))
    m, _ = _check(cuda, run, d, kw)
    assert m.result["n_msgs"] == count and m.result["n_bad"] == 0
    if gather == "identity":
        same, _ = _check(cuda, run, d, dict(kw, records=np.arange(n)))
        assert np.array_equal(same.events, m.events)
    if gather == "skipping":
        # one record off and the call is refused, naming the message
        off = records.copy()
        off[78] += 1                   # its CONFIRM
        assert int(run[60 * int(off[78])]) >> 4 == S.REC_CONFIRM
        refused, _ = _check(cuda, run, d, dict(kw, records=off))
        assert refused == M.Refusal(M.RECORD, 78)


def test_a_window_inside_the_file_that_ends_with_its_last_record(cuda):
    run, d, msgs = _messages(300)
    lo, hi = 10, 295
    at = [8 * int.from_bytes(run[60 * i + 32:60 * i + 36].tobytes(), "big") for i in (lo, hi)]
    window = d[at[0]:at[1]]          # record hi - 1's DATA record ends at at[1]
    records = np.arange(lo, hi)
    kw = _kw(hi - lo, records=records, data_file_pos=at[0], event_first=_cuts(hi - lo, 40))
    m, _ = _check(cuda, run, window, kw)
    whole = M.pack(run, d, crc32c=CRC, **dict(_kw(300), dst_bytes=1 << 30))
    assert np.array_equal(m.crcs, whole.crcs[lo:hi])
    # one byte less, and the last message is refused; a record in front of the
    # window likewise
    short, _ = _check(cuda, run, window[:-1], kw)
    assert short == M.Refusal(M.DATA_RECORD, hi - lo - 1)
    records[3] = lo - 1
    below, _ = _check(cuda, run, window, dict(kw, records=records))
    assert below == M.Refusal(M.DATA_OFFSET, 3)


@pytest.mark.parametrize("skip", ["event_offsets", "out", "lengths"])
def test_null_outputs(cuda, skip):
    run, d, _ = _messages(140)
    _check(cuda, run, d, _kw(140, event_first=_cuts(140, 17)), skip=(skip,))
    refused, _ = _check(cuda, run, d, _kw(140, dst_bytes=64), skip=(skip,))
    assert refused == M.Refusal(M.DST_TOO_SMALL, 0)


# ---- verify on delivery --------------------------------------------------------

def test_a_corrupt_payload_and_a_corrupt_stored_crc_are_counted_and_delivered(cuda):
    n = 400
    run, d, _ = _messages(n)
    good = M.pack(run, d, crc32c=CRC, **dict(_kw(n), dst_bytes=1 << 30))
    victim = int(np.flatnonzero(good.lengths > 4)[40])
    other = victim + 123
    o = 8 * int.from_bytes(run[60 * victim + 32:60 * victim + 36].tobytes(), "big")
    bad, j = d.copy(), run.copy()
    bad[o + 12 + 3] ^= 0x10            # a bit rots in the payload
    j[60 * other + 52] ^= 0x80         # and one in a stored CRC
    kw = _kw(n, event_first=_cuts(n, 33))
    m, host = _check(cuda, j, bad, kw)
    assert (m.result["n_bad"], m.result["first_bad"]) == (2, victim)
    assert np.flatnonzero(host["out"][:n] != m.expected).tolist() == [victim, other]
    one = M.pack(run, d, crc32c=CRC, **dict(kw, dst_bytes=1 << 30))
    diff = np.flatnonzero(host["dst"][:one.events.size] != one.events)
    assert diff.size == 1 and host["dst"][diff[0]] == bad[o + 12 + 3]
    # the gather names the rotten record twice: both messages are counted
    m, _ = _check(cuda, j, bad, _kw(3, records=[victim, 0, victim]))
    assert (m.result["n_bad"], m.result["first_bad"]) == (2, 0)


# ---- sizing ------------------------------------------------------------------

def test_size_only_agrees_with_the_full_call_and_writes_nothing_else(cuda):
    n = 1500
    run, d, _ = _messages(300, seed=8, options=True)
    records = np.arange(n) * 31 % 300
    kw = _kw(n, records=records, option_mode=3, rda=np.arange(n) % 256, sub_ids=np.arange(n),
             event_first=_cuts(n, 107))
    full, _ = _check(cuda, run, d, kw)
    sized, host = _check(cuda, run, d, dict(kw, dst_bytes=None))
    assert "dst" not in host and sized.result == dict(full.result, n_bad=0, first_bad=n)
    assert np.array_equal(host["event_offsets"][:len(full.event_offsets)], full.event_offsets)
    # with repeats the DATA file bounds nothing: the events are longer than it
    assert full.result["total_bytes"] > 2 * d.size
    # asynchronously too, and a refusal is a refusal
    _check(cuda, run, d, dict(kw, dst_bytes=None), sync=False, skip=("out", "lengths"))
    refused, _ = _check(cuda, run, d, dict(kw, dst_bytes=None, max_event_bytes=500))
    assert refused.kind == M.EVENT_TOO_BIG
    refused, _ = _check(cuda, run, d, dict(kw, dst_bytes=None, records=records + 1))
    assert refused == M.Refusal(M.RECORD_INDEX, int(np.flatnonzero(records == 299)[0]))


def test_dst_of_exactly_total_bytes_and_one_byte_less(cuda):
    n = 140
    run, d, _ = _messages(n)
    kw = _kw(n, event_first=_cuts(n, 17))
    m, _ = _check(cuda, run, d, kw)
    refused, _ = _check(cuda, run, d, dict(kw, dst_bytes=m.result["total_bytes"] - 1))
    assert refused == M.Refusal(M.DST_TOO_SMALL, m.result["n_events"] - 1)


# ---- refusals ----------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(C.refusal_cases()))
def test_refusal_like_the_model(cuda, name):
    case = C.refusal_cases()[name]
    m, _ = _check(cuda, case.run, case.data, case.kw)
    assert m == case.want


@pytest.mark.parametrize("name", sorted(C.precedence_cases()))
def test_refusal_precedence(cuda, name):
    case = C.precedence_cases()[name]
    for sync in (True, False):
        m, _ = _check(cuda, case.run, case.data, case.kw, sync=sync)
        assert m == case.want


def test_a_violation_in_the_last_message_of_the_last_block(cuda):
    run, d, _ = _messages(1025)
    bad = run.copy()
    bad[60 * 1024 + 59] ^= 0xFF           # the magic of record 1,024, the second block's only one
    refused, _ = _check(cuda, bad, d, _kw(1025, event_first=_cuts(1025, 1024)))
    assert refused == M.Refusal(M.RECORD, 1024)
    # and with an earlier violation of a higher kind in the first block
    C.put32(bad, 60 * 1023 + 32, 0)
    refused, _ = _check(cuda, bad, d, _kw(1025))
    assert refused == M.Refusal(M.RECORD, 1024)
    bad[60 * 1024 + 59] ^= 0xFF
    refused, _ = _check(cuda, bad, d, _kw(1025))
    assert refused == M.Refusal(M.DATA_OFFSET, 1023)
    # the flags of the last message alone
    flags = np.zeros(1025, np.uint8)
    flags[1024] = 1
    refused, _ = _check(cuda, run, d, _kw(1025, flags=flags))
    assert refused == M.Refusal(M.FLAGS, 1024)


def test_python_wrapper_raises_reports_and_sizes_the_destination(cuda):
    import torch
    case = C.refusal_cases()["padding_byte_9"]
    run, data = _dev(cuda, case.run), _dev(cuda, case.data)
    first = _t(cuda, np.asarray(C.EVENT_FIRST, np.int64), np.int64)
    args = dict(data_file_pos=0, queue_ids=_t(cuda, C.QUEUE_IDS, np.int32),
                records=_t(cuda, C.RECORDS, np.uint32), option_mode=E.OPTION_PACKED_RDA,
                rda=_t(cuda, C.RDA, np.uint8), event_first=first)
    with pytest.raises(BmqCrcError, match="BMQCRC_PUSH_PACK_DATA_RECORD: the record of message 3 ") \
            as e:
        pack_push_events(run, data, **args)
    assert e.value.rc == N.BMQCRC_EINVAL
    with pytest.raises(ValueError, match="sync=False"):
        pack_push_events(run, data, sync=False, **args)
    with pytest.raises(ValueError, match="one entry per message"):
        pack_push_events(run, data, **dict(args, rda=args["rda"][:5]))
    with pytest.raises(BmqCrcError, match="rda is required"):
        pack_push_events(run, data, **dict(args, rda=None))
    base_run, base_data, kw = C.base()
    want = M.pack(base_run, base_data, crc32c=CRC, **kw)
    s = _side_stream(cuda)
    with torch.cuda.stream(s):
        dst = torch.zeros(4096, dtype=torch.uint8, device=cuda)
        u = pack_push_events(run, data, dst=dst, stream=s, sync=False, **args)
        assert u.result is None and u.crcs.numel() == 8 and u.event_offsets.numel() == 4
        assert last_push_pack(cuda.index, s) == M.refused_result(case.want, 3)
        assert not dst.any()
        u = pack_push_events(_dev(cuda, base_run), _dev(cuda, base_data), dst=dst, stream=s,
                             sync=False, **args)
        res = last_push_pack(cuda.index, s)
    assert res == want.result
    assert np.array_equal(dst.cpu().numpy()[:C.TOTAL], want.events)
    assert np.array_equal(u.crcs.cpu().numpy().view(np.uint32), want.crcs)
    assert np.array_equal(u.lengths.cpu().numpy().view(np.uint32), want.lengths)
    # dst=None: the size-only call first, then exactly that many bytes
    p = pack_push_events(_dev(cuda, base_run), _dev(cuda, base_data), **args)
    assert p.result == want.result and p.events.numel() == C.TOTAL
    assert p.events.untyped_storage().nbytes() == C.TOTAL
    assert np.array_equal(p.events.cpu().numpy(), want.events)
    assert np.array_equal(p.event_offsets.cpu().numpy().view(np.uint64), want.event_offsets)
    # no message
    none = torch.zeros(0, dtype=torch.int32, device=cuda)
    p = pack_push_events(_dev(cuda, base_run), _dev(cuda, base_data), data_file_pos=0,
                         queue_ids=none, records=none)
    assert p.events.numel() == 0 and p.result == M.refused_result(M.Refusal(0, 0), 0)


# ---- state -------------------------------------------------------------------

def test_state(cuda):
    import torch
    rng = np.random.default_rng(57)
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
    run, d, msgs = _messages(200, seed=10, mixed=True)
    events, offsets = synth.storage_events(run[60:], d, 0, JH + 60, 1, 33)
    n = len(msgs)
    kw = _kw(n, records=np.array(msgs), option_mode=1, rda=np.arange(n) % 256,
             event_first=_cuts(n, 33))
    s = _side_stream(cuda)

    def records():
        return (last_launch(cuda.index, s, offsets=True), last_copy(cuda.index, s),
                last_put_pack(cuda.index, s), last_records_pack(cuda.index, s),
                last_put_unpack(cuda.index, s), last_records_unpack(cuda.index, s),
                last_journal_select(cuda.index, s), last_storage_apply(cuda.index, s),
                last_storage_pack(cuda.index, s))
    with torch.cuda.stream(s):
        # none yet on s
        assert last_push_pack(cuda.index, s) == M.refused_result(M.Refusal(0, 0), 0)
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
        before = records()
        _check(cuda, run, d, kw, stream=s)
        _check(cuda, run, d, kw, stream=s, sync=False)
        _check(cuda, run, d, dict(kw, dst_bytes=None), stream=s)        # a size-only one
        _check(cuda, run, d, dict(kw, max_event_bytes=100), stream=s)   # a refused one
        assert records() == before
        assert before[1] == (40, 0, 40)
        out = Crc32c.calculate_batch(arena, d_off, d_len, stream=s)
    s.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), P.host_crcs(host, offs, lens))


# ---- the pipeline ------------------------------------------------------------

def test_put_in_to_push_out_on_one_device(cuda):
    # unpack_events -> pack_records -> select_records -> unpack_records(verify)
    # -> pack_push_events(records=record_index): no payload byte on the host
    # until the comparison
    import torch
    rng = np.random.default_rng(63)
    n = 300
    buf, evoffs = PU.concat([PU.build_event(rng, rng.integers(1, 400, size=100))
                             for _ in range(3)])
    pm = PU.model(buf, evoffs)
    events = _dev(cuda, buf)
    u = unpack_events(events, _t(cuda, evoffs, np.int64), msg_cap=n)
    qkeys = torch.from_numpy(np.frombuffer(QK, np.uint8).copy()).to(cuda).repeat(n, 1)
    dst, jour, _, _, _ = pack_records(events, u.app_offsets, u.lengths, qkeys, u.guids,
                                      expected=u.expected, file_key=b"\x11\x22\x33\x44\x55",
                                      lease_id=7, first_seq=2, data_file_pos=40)
    w = S.PartitionWriter(lease_id=7)
    w.queue_op(S.OP_CREATION, QK)
    jfile, _ = w.files()
    journal = torch.cat([_t(cuda, jfile[JH:], np.uint8), jour])
    select, sel = select_records(journal, data_file_bytes=40 + dst.numel())
    r = unpack_records(journal, dst, data_file_pos=40, select=select, verify=True)
    assert sel["recovery_rc"] == 0 and r.record_index.numel() == n
    p = pack_push_events(journal, dst, data_file_pos=40, records=r.record_index,
                         queue_ids=u.queue_ids, option_mode=E.OPTION_SUB_QUEUE_ID,
                         sub_ids=u.queue_ids,
                         event_first=_t(cuda, _cuts(n, 64).view(np.int64), np.int64))
    assert p.result["n_bad"] == 0 and p.result["n_msgs"] == n and p.result["n_events"] == 5
    out, offs = p.events.cpu().numpy(), p.event_offsets.cpu().numpy()
    got = [m for e in range(5) for m in PushMessageIterator(out[int(offs[e]):int(offs[e + 1])])]
    assert len(got) == n
    for i, m in enumerate(got):
        at, ln = int(pm["app_offsets"][i]), int(pm["lengths"][i])
        assert m["payload"] == buf[at:at + ln].tobytes()
        assert m["guid"] == pm["guids"][i].tobytes() and m["queue_id"] == int(pm["queue_ids"][i])
    assert np.array_equal(p.crcs.cpu().numpy().view(np.uint32), pm["crcs"])


# ---- past one tile per block ----------------------------
#
# N_FRAME messages over record_pool.py's journal of N_FRAME records: message m
# names MESSAGE record msgs[(m * STEP + 5) % len(msgs)], so neighbours name
# records far apart and past len(msgs) messages the records repeat; the smaller
# sizes are prefixes.  Messages LONG_MESSAGES name the two records longer than a
# chunk of the copy instead.  Queue ids, RDA counters and sub-queue ids are
# random, the flags 0 or 4.  The expected bytes are push_events_fast's, which
# test_push_pack_model.py holds to the loop model and to PushEventBuilder.  A
# model is built for the case that needs it and dropped with it.

LONG_MESSAGES = (1024 + 476, 70 * 2048 + 1024 + 300)    # second tiles of blocks 0 and 70 at N_TILES


@functools.lru_cache(maxsize=None)
def _large_inputs():
    """(records, queue_ids, flags, rda, sub_ids, application bytes) of N_FRAME
    messages.  Shared, never modified."""
    n = G.N_FRAME
    rng = np.random.default_rng(31)
    p = R.pool()
    records = R.push_records(n).astype(np.uint32)
    records[list(LONG_MESSAGES)] = p.long
    qids = rng.integers(-2**31, 2**31, size=n, dtype=np.int64).astype(np.int32)
    qids[rng.integers(0, n, size=3000)] = np.tile(np.array([-1, -2**31, 2**31 - 1], np.int32), 1000)
    flags = (4 * rng.integers(0, 2, size=n)).astype(np.uint8)
    rda = rng.integers(0, 256, size=n, dtype=np.uint8)
    sub = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    by_record = np.zeros(n, np.int64)
    by_record[p.msgs] = R.data_fields(p.run, p.data, p.msgs)[3]
    out = (records, qids, flags, rda, sub, by_record[records])
    for a in out:
        a.setflags(write=False)
    return out


def _split(n, how):
    """event_first of n messages: events of 3, every message its own event, one
    event (None), or test_grid_regimes.py's split at the seal's boundary."""
    if how == "of_3":
        return np.array(G.events_of_3(n), np.uint64)
    if how == "own":
        return np.arange(n + 1, dtype=np.uint64)
    if how == "boundary":
        return np.array(G.boundary_split(n, G.regime(n).per_block), np.uint64)
    assert how is None
    return None


def _large_kw(n, mode, how, **changes):
    records, qids, flags, rda, sub, _ = _large_inputs()
    kw = _kw(n, queue_ids=qids[:n], records=records[:n], flags=flags[:n], option_mode=mode,
             rda=rda[:n] if mode in (1, 3) else None, sub_ids=sub[:n] if mode in (2, 3) else None,
             event_first=_split(n, how), dst_bytes="room")
    kw.update(changes)
    return kw


def _fast(run, d, kw, **changes):
    """push_events_fast's answer to the call `kw`, the CRCs taken from the
    pool's (`run` is the pool's journal)."""
    kw = dict(kw, **changes)
    kw.pop("dst_alloc", None)
    return M.push_events_fast(run, d, record_crcs=R.pool().crcs, **kw)


def _event_offsets(n, mode, first):
    length = _large_inputs()[5][:n]
    before = np.concatenate([[0], np.cumsum(32 + M.OPTION_BYTES[mode] + length + 4 - length % 4)])
    first = np.asarray(first if first is not None else [0, n]).astype(np.int64)
    return 8 * np.arange(first.size) + before[first]


def _exact(cuda, run, d, kw, want, **how):
    """The call into a destination of exactly the model's size."""
    return _check(cuda, run, d, dict(kw, dst_bytes=want.result["total_bytes"]), model=want, **how)


LARGE = {"waves-no_option-events_of_3": (G.N_WAVES, 0, "of_3"),
         "full-packed_rda-one_event": (G.N_FULL, 1, None),
         "tiles-sub_queue_info-own_events": (G.N_TILES, 3, "own"),
         "frame-sub_queue_info-own_events": (G.N_FRAME, 3, "own"),
         "frame-packed_rda-seal_boundary": (G.N_FRAME, 1, "boundary")}


@pytest.mark.parametrize("name", sorted(LARGE))
def test_past_one_tile_per_block(cuda, name):
    # N_WAVES: 66 blocks, the 8-dword header loop in its second step.  N_FULL:
    # all 256 blocks under one event.  N_TILES: two tiles a block; with an
    # event per message seal_offsets searches event_first in global memory.
    # N_FRAME: three tiles a block, the 11-dword header loop in its twelfth
    # step, the per-message loop of k_ppk_frame in its second (message
    # 524,288), records named a second time; the boundary split is one event
    # past the seal's LDS array from block SEAL_BLOCK on.
    n, mode, how = LARGE[name]
    p = R.pool()
    r = G.regime(n)
    assert r.dwords_past_grid and r.cross_wave and r.units_past_grid == (n == G.N_FRAME)
    kw = _large_kw(n, mode, how)
    want = _fast(p.run, p.data, kw)
    assert want.result["n_bad"] == 0 and sorted(set(kw["flags"].tolist())) == [0, 4]
    assert {-1, -2**31, 2**31 - 1} <= set(kw["queue_ids"].tolist())
    if n >= G.N_TILES:
        assert want.lengths[list(LONG_MESSAGES)].tolist() == list(R.LONG)
    if n == G.N_FRAME:
        assert np.array_equal(kw["records"][p.msgs.size + 5000:], kw["records"][5000:n - p.msgs.size])
    m, _ = _exact(cuda, p.run, p.data, kw, want)
    assert m is want


def test_past_one_tile_per_block_on_a_side_stream(cuda):
    import torch
    p = R.pool()
    kw = _large_kw(G.N_TILES, 2, "of_3")
    want = _fast(p.run, p.data, kw)
    torch.cuda.synchronize(cuda)
    s = _side_stream(cuda)
    with torch.cuda.stream(s):
        _exact(cuda, p.run, p.data, kw, want, sync=False, stream=s)


def test_past_one_tile_per_block_without_a_gather(cuda):
    # records == NULL over a journal of MESSAGE records alone, n_records == n
    n = G.N_TILES
    p = R.pool()
    run = R.message_journal()
    assert run.size == 60 * n
    kw = _large_kw(n, 1, "of_3", records=None)
    want = M.push_events_fast(run, p.data, record_crcs=p.crcs[p.msgs[:n]], **kw)
    named = M.push_events_fast(p.run, p.data, record_crcs=p.crcs, **dict(kw, records=p.msgs[:n]))
    assert np.array_equal(want.events, named.events) and want.result == named.result
    assert int(want.lengths.max()) == R.LONG[0] and want.result["n_bad"] == 0
    _exact(cuda, run, p.data, kw, want)


def test_past_one_tile_per_block_in_a_window(cuda):
    p = R.pool()
    kw = _large_kw(G.N_TILES, 2, "of_3", data_file_pos=40)
    want = _fast(p.run, p.data[40:], kw)
    whole = _fast(p.run, p.data, dict(kw, data_file_pos=0))
    assert np.array_equal(want.events, whole.events) and want.result == whole.result
    _exact(cuda, p.run, p.data[40:], kw, want)


@pytest.mark.parametrize("n,mode,how", [(G.N_TILES, 2, "of_3"), (G.N_FRAME, 3, "own")],
                         ids=["tiles-events_of_3", "frame-own_events"])
def test_size_only_past_one_tile_per_block(cuda, n, mode, how):
    # k_ppk_seal's own block_prefix and its own loop over n_events + 1 entries:
    # three steps at N_FRAME, with bpre[f / per_block] for blocks past the 64th.
    # DST_TOO_SMALL does not apply: the call declares no destination at all
    p = R.pool()
    kw = _large_kw(n, mode, how)
    full = _fast(p.run, p.data, kw)
    sized = _fast(p.run, p.data, kw, dst_bytes=None)
    assert isinstance(sized, M.Packed) and sized.result == dict(full.result, n_bad=0, first_bad=n)
    assert np.array_equal(sized.event_offsets, full.event_offsets)
    assert np.array_equal(full.event_offsets, _event_offsets(n, mode, kw["event_first"]))
    for sync in (True, False):
        m, host = _check(cuda, p.run, p.data, dict(kw, dst_bytes=None), sync=sync, model=sized)
        assert "dst" not in host and _untouched("out", host["out"]) and \
            _untouched("lengths", host["lengths"])
        assert np.array_equal(host["event_offsets"][:len(full.event_offsets)], full.event_offsets)
    # then the full call into exactly that many bytes
    _exact(cuda, p.run, p.data, kw, full)


def test_stored_crc_mismatches_in_every_step_of_the_frame_loop(cuda):
    # the stored CRCs (journal bytes 52..55) flipped of the records that
    # messages 999, 1,999, ..., message 1,003 of the same wave and message
    # 524,288 name, which a frame thread reaches in its second step alone; a
    # record named twice mismatches twice
    n = G.N_FRAME
    p = R.pool()
    kw = _large_kw(n, 3, "own")
    records = kw["records"].astype(np.int64)
    chosen = np.concatenate([np.arange(999, n, 1000), [1003, n - 1]])
    assert 999 // 64 == 1003 // 64 and n - 1 == 524288
    victims = np.unique(records[chosen])
    bad = p.run.copy()
    bad[60 * victims[:, None] + 52 + np.arange(4)] ^= np.array([0x80, 1, 0, 0x10], np.uint8)
    wrong = np.flatnonzero(np.isin(records, victims))
    assert wrong.size > chosen.size and wrong[0] <= 999 and wrong[-1] == n - 1
    want = _fast(bad, p.data, kw)
    assert (want.result["n_bad"], want.result["first_bad"]) == (wrong.size, int(wrong[0]))
    m, host = _exact(cuda, bad, p.data, kw, want)
    assert np.array_equal(np.flatnonzero(host["out"][:n] != want.expected), wrong)
    # delivered all the same: the bytes are those of the clean journal's call
    clean = _fast(p.run, p.data, kw)
    assert np.array_equal(host["dst"][:clean.events.size], clean.events)


def _refused_both_ways(cuda, run, d, kw, want):
    """The call refused as `want`, synchronous and asynchronous, into a
    destination that would hold every event, with nothing written."""
    n = len(kw["queue_ids"])
    room = int(_event_offsets(n, kw["option_mode"], kw["event_first"])[-1])
    kw = dict(kw, dst_alloc=room)
    if kw["dst_bytes"] == "room":
        kw["dst_bytes"] = room
    for sync in (True, False):
        m, _ = _check(cuda, run, d, kw, sync=sync, model=want)
        assert m == want


def _loop_model(run, d, kw, lo, hi):
    """M.pack over messages [lo, hi) alone, as one event."""
    part = {k: (v[lo:hi] if k in ("queue_ids", "records", "flags", "rda", "sub_ids")
                and v is not None else v) for k, v in kw.items()}
    part.pop("dst_alloc", None)
    return M.pack(run, d, crc32c=CRC, **dict(part, event_first=None, dst_bytes=1 << 40))


def test_message_refusals_across_tiles_and_blocks(cuda):
    n = G.N_TILES
    p = R.pool()
    r = G.regime(n)
    assert (r.nblocks, r.per_block) == (129, 2048) and p.run.size == 60 * G.N_FRAME
    kw = _large_kw(n, 3, "of_3")
    # (a) records[m] = n_records at message 1,024 + 5, in the second tile of
    # block 0, and at message 2,048 + 3, in the first tile of block 1: the lower
    records = kw["records"].copy()
    records[[1029, 2051]] = G.N_FRAME
    bad = dict(kw, records=records)
    want = M.Refusal(M.RECORD_INDEX, 1029)
    assert _loop_model(p.run, p.data, bad, 0, 2100) == want
    _refused_both_ways(cuda, p.run, p.data, bad, want)
    # (b) the last padding byte of the DATA record of a message below 100 made
    # 9, and message 200,001 naming a CONFIRM record: the lower kind wins over
    # the lower index.  (A message of 9 bytes or more with its padding: a check
    # that lets it pass still finds a length inside the record)
    early = kw["records"][:100].astype(np.int64)
    at, lead, rec, length, _ = R.data_fields(p.run, p.data, early)
    victim = int(np.flatnonzero(rec - lead >= 16)[3])
    assert int((kw["records"][:n] == early[victim]).sum()) == 1
    data = p.data.copy()
    data[int(at[victim] + rec[victim]) - 1] = 9
    want = M.Refusal(M.DATA_RECORD, victim)
    assert _loop_model(p.run, data, kw, 0, 100) == want
    _refused_both_ways(cuda, p.run, data, kw, want)
    confirm = int(np.flatnonzero(p.run.reshape(-1, 60)[:, 0] >> 4 == S.REC_CONFIRM)[1000])
    records = kw["records"].copy()
    records[200001] = confirm
    bad = dict(kw, records=records)
    assert _loop_model(p.run, data, bad, 200001, 200002) == M.Refusal(M.RECORD, 0)
    _refused_both_ways(cuda, p.run, data, bad, M.Refusal(M.RECORD, 200001))
    # (c) the flags of the last message of the last block, the 1,025th of block 128
    assert n - 1 - (r.nblocks - 1) * r.per_block == 1024
    flags = kw["flags"].copy()
    flags[n - 1] = 1
    bad = dict(kw, flags=flags)
    assert _loop_model(p.run, p.data, bad, n - 50, n) == M.Refusal(M.FLAGS, 49)
    _refused_both_ways(cuda, p.run, p.data, bad, M.Refusal(M.FLAGS, n - 1))


def test_payload_cap_at_the_long_message_of_a_second_tile(cuda):
    n = G.N_TILES
    p = R.pool()
    kw = _large_kw(n, 1, "of_3")
    visit = int(np.flatnonzero(kw["records"] == p.long[0])[0])
    assert visit == LONG_MESSAGES[0] and 1024 <= visit < 2048
    want = M.Refusal(M.PAYLOAD_TOO_BIG, visit)
    cap = R.LONG[0]
    assert _loop_model(p.run, p.data, dict(kw, max_payload_bytes=cap - 1), 0, 1600) == want
    assert _fast(p.run, p.data, kw, max_payload_bytes=cap - 1) == want
    _refused_both_ways(cuda, p.run, p.data, dict(kw, max_payload_bytes=cap - 1), want)
    # the cap exactly the longest message
    kw["max_payload_bytes"] = cap
    _exact(cuda, p.run, p.data, kw, _fast(p.run, p.data, kw))


def _shape_refusal(first, n):
    """The lowest entry of event_first that breaks its shape."""
    first = np.asarray(first).astype(np.int64)
    bad = np.concatenate([first[:-1] >= first[1:], [first[-1] != n]])
    bad[0] |= first[0] != 0
    return M.Refusal(M.EVENT_FIRST, int(np.flatnonzero(bad)[0]))


def test_event_first_refused_in_a_late_step_of_the_shape_loop(cuda):
    # one event per message at N_FRAME: 175,104 threads over 524,290 entries.
    # Every bad entry is itself an index below n
    n = G.N_FRAME
    p = R.pool()
    threads = G.regime(n).nblocks * 1024
    assert 2 * threads < n < 3 * threads
    kw = _large_kw(n, 0, "own")
    good = kw["event_first"]
    room = int(_event_offsets(n, 0, good)[-1])

    def refused(index, entries):
        first = good.copy()
        for e, v in entries.items():
            first[e] = v
        assert int(first.max()) <= n and all(v < n for v in entries.values())
        want = M.Refusal(M.EVENT_FIRST, index)
        assert _shape_refusal(first, n) == want
        for sync in (True, False):
            m, _ = _check(cuda, p.run, p.data, dict(kw, event_first=first, dst_bytes=room),
                          sync=sync, model=want)
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
    # events of 3 at N_TILES but for two of 3,000 and 6,000 messages, whose
    # first messages lie in the second tiles of blocks 70 and 100
    n = G.N_TILES
    p = R.pool()
    per_block = G.regime(n).per_block
    ia, ib = 70 * per_block + 1102, 100 * per_block + 1024
    cuts = [c for c in G.events_of_3(n) if not ia < c < ia + 3000 and not ib < c < ib + 6000]
    ea, eb = cuts.index(ia), cuts.index(ib)
    for i in (ia, ib):
        assert i % 3 == 0 and i % per_block >= 1024 and i // per_block in (70, 100)
    kw = _large_kw(n, 2, None, event_first=np.array(cuts, np.uint64))
    sizes = np.diff(_event_offsets(n, 2, cuts))
    order = np.argsort(sizes)
    assert [int(e) for e in order[-2:]] == [ea, eb] and sizes[order[-3]] < sizes[ea] - 4 and \
        sizes[ea] < sizes[eb] - 4
    # one event over the cap, then two: the lower index
    for cap, event in ((int(sizes[eb]) - 4, eb), (int(sizes[ea]) - 4, ea)):
        want = M.Refusal(M.EVENT_TOO_BIG, event)
        assert _fast(p.run, p.data, kw, max_event_bytes=cap) == want
        _refused_both_ways(cuda, p.run, p.data, dict(kw, max_event_bytes=cap), want)
        # the size-only call refuses alike
        for sync in (True, False):
            _check(cuda, p.run, p.data, dict(kw, max_event_bytes=cap, dst_bytes=None), sync=sync,
                   model=want)
    # the cap exactly the largest event
    kw["max_event_bytes"] = int(sizes[eb])
    _exact(cuda, p.run, p.data, kw, _fast(p.run, p.data, kw))


def test_destination_size_past_one_tile_per_block(cuda):
    n = G.N_TILES
    p = R.pool()
    kw = _large_kw(n, 3, "of_3")
    ev = _event_offsets(n, 3, kw["event_first"])
    total, n_events = int(ev[-1]), ev.size - 1
    want = M.Refusal(M.DST_TOO_SMALL, n_events - 1)
    assert _fast(p.run, p.data, kw, dst_bytes=total - 4) == want
    _refused_both_ways(cuda, p.run, p.data, dict(kw, dst_bytes=total - 4), want)
    # half the image: the first event that ends past it, while every later one
    # refuses as well
    want = _fast(p.run, p.data, kw, dst_bytes=total // 2)
    assert want.kind == M.DST_TOO_SMALL and n_events // 3 < want.index < 2 * n_events // 3
    assert ev[want.index] <= total // 2 < ev[want.index + 1]
    _refused_both_ways(cuda, p.run, p.data, dict(kw, dst_bytes=total // 2), want)
    # one event per message at N_FRAME: some 260,000 events refuse, over three
    # steps of every block of the check grid
    n = G.N_FRAME
    kw = _large_kw(n, 0, "own")
    ev = _event_offsets(n, 0, kw["event_first"])
    half = int(ev[-1]) // 2
    index = int(np.searchsorted(ev[1:], half, side="right"))
    assert ev[index] <= half < ev[index + 1] and n - index > 200000
    _refused_both_ways(cuda, p.run, p.data, dict(kw, dst_bytes=half),
                       M.Refusal(M.DST_TOO_SMALL, index))
