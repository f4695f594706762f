"""Messages past their TTL expired on the GPU (bmqcrc_expire_records_pack, ABI
2.20).  The oracle throughout is tests/expire_records_model.py.  Every raw call
hands the library a sentinel-filled destination and output arrays with guard
bytes and elements behind them: the guards are checked after every call, and
every byte and element after a refused or size-only one."""
import ctypes
import functools

import numpy as np
import pytest

from blazingmq_amd import (PushMessageIterator, _native as N, apply_events, expire_records,
                           last_confirm_records, last_copy, last_expire_records,
                           last_journal_select, last_launch, last_push_pack, last_put_pack,
                           last_put_unpack, last_records_pack, last_records_unpack,
                           last_rollover, last_storage_apply, last_storage_pack,
                           pack_push_events, pack_records, pack_storage_events, rollover_records,
                           select_records)
from blazingmq_amd import Crc32c
from blazingmq_amd import storage as S
import device_views as V
import expire_collisions as X
import expire_records_cases as C
import expire_records_model as M
import join_collisions as J
import put_pack_model as P
import test_grid_regimes as G
from records_pack_model import random_meta

pytestmark = pytest.mark.gpu

GUARD = 8      # elements behind every output array
SLACK = 64     # bytes behind every input buffer and the destination
SENTINEL = 0xC3
JH = S.PartitionWriter.JOURNAL_HEADER
# name -> (element type, canary, "r": one per record, "q": one per queue)
CANARY = {"expired": (np.uint8, 0x5A, "r"), "new_index": (np.uint32, 0xA5A5A5A5, "r"),
          "select_out": (np.uint8, 0x3C, "r"), "queue_expired": (np.uint32, 0x5A5A5A5A, "q"),
          "queue_front": (np.uint32, 0x3C3C3C3C, "q")}
KINDS = ("OK", "RECORD_HEADER", "DUPLICATE_MESSAGE", "QUEUE_KEY", "DST_TOO_SMALL")
KIND_NAME = {k: ("BMQCRC_EXPIRE_PACK_" + n).encode() for k, n in enumerate(KINDS) if k}
KEYS = [bytes([0x26, 0xda, 0xcd, 0xc9, 0x74 + k]) for k in range(4)]
# the base pointers the ABI permits: 4-byte ones at +4, the 8-byte one at +8, bytes at +1
PHASES = {"journal": 4, "journal_dst": 4, "select": 1, "queue_keys": 1, "ttl_seconds": 8,
          "expired": 1, "new_index": 4, "select_out": 1, "queue_expired": 4, "queue_front": 4}


def _side_stream(cuda):
    """A stream of its own from the high-priority pool (the default pool's
    streams carry planner history that tests elsewhere rely on)."""
    import torch
    return torch.cuda.Stream(cuda, priority=-1)


def _t(cuda, a, dtype):
    import torch
    a = np.array(a, dtype=dtype)     # (a copy: shared inputs are read-only)
    if dtype == np.uint32:
        a = a.view(np.int32)
    if dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to(cuda)


def _dev(cuda, buf, place, name):
    """`buf` on the device as a view of a longer allocation: one that starts
    with it, or with `place` (a device_views.Placer) one that holds it at the
    phase the placer has for `name`."""
    import torch
    buf = np.array(buf)  # (a copy: shared inputs are read-only)
    if place is not None:
        return place.put(name, buf)
    raw = buf.reshape(-1).view(np.uint8)
    back = torch.full((raw.size + SLACK,), 0xEE, dtype=torch.uint8, device=cuda)
    back[:raw.size] = torch.from_numpy(raw).to(cuda)
    return back[:raw.size].view({np.dtype(np.uint64): torch.int64}.get(buf.dtype, torch.uint8))


def _filled(cuda, place, name, count, dt, value):
    import torch
    if place is not None:
        return place.fill(name, count, dt, value)
    fill = np.array([value], np.uint64).astype(dt)
    return torch.from_numpy(np.repeat(fill, count).view(
        {np.uint32: np.int32}.get(dt, dt))).to(cuda)


def _raw(cuda, run, table, kw, sync=True, stream=None, skip=(), phases=None):
    """One bmqcrc_expire_records_pack over device tensors into a
    sentinel-filled destination and arrays.  `table`: (queue_keys,
    ttl_seconds).  `kw`: now, lease_id, first_seq, select, journal_dst_bytes
    (None: a size-only call, journal_dst NULL).  Returns (rc, error text, result
    of the call or of bmqcrc_last_expire_records, everything written on the
    host with its guards).  `phases` maps every pointer of the call to the
    phase of its base; the sentinel margins around each are checked after the
    call."""
    import torch
    place = V.Placer(cuda, phases) if phases is not None else None
    stream = stream or torch.cuda.current_stream(cuda)
    n_records, n_queues = len(run) // 60, len(table[1])
    room = kw.get("journal_dst_bytes")
    with torch.cuda.stream(stream):
        d_in = {"journal": _dev(cuda, np.asarray(run, np.uint8), place, "journal"),
                "queue_keys": _dev(cuda, np.asarray(table[0], np.uint8), place, "queue_keys"),
                "ttl_seconds": _dev(cuda, np.asarray(table[1], np.uint64), place, "ttl_seconds")}
        if kw.get("select") is not None:
            d_in["select"] = _dev(cuda, np.asarray(kw["select"], np.uint8), place, "select")
        arr = {"journal_dst": _filled(cuda, place, "journal_dst", (room or 0) + SLACK, np.uint8,
                                      SENTINEL)}
        for name, (dt, value, per) in CANARY.items():
            if name not in skip:
                count = n_records if per == "r" else n_queues
                arr[name] = _filled(cuda, place, name, count + GUARD, dt, value)
        # (an empty tensor has no address: the call wants one)
        spare = torch.zeros(8, dtype=torch.uint8, device=cuda)
        p = N.ExpirePack()
        p.struct_size = ctypes.sizeof(N.ExpirePack)
        p.journal, p.journal_bytes = d_in["journal"].data_ptr() or spare.data_ptr(), len(run)
        p.n_records, p.n_queues = n_records, n_queues
        p.select = d_in["select"].data_ptr() if "select" in d_in and n_records else None
        p.queue_keys = d_in["queue_keys"].data_ptr() if n_queues else None
        p.ttl_seconds = d_in["ttl_seconds"].data_ptr() if n_queues else None
        p.now, p.first_seq, p.lease_id = kw["now"], kw["first_seq"], kw["lease_id"]
        p.journal_dst = arr["journal_dst"].data_ptr() if room is not None else None
        p.journal_dst_bytes = room or 0
        for name in CANARY:
            setattr(p, name, arr[name].data_ptr() if name in arr else None)
        o = N.make_opts(device=cuda.index, stream=stream.cuda_stream,
                        flags=N.BMQCRC_F_DEVICE_PTRS | (0 if sync else N.BMQCRC_F_ASYNC))
        r = N.ExpirePackResult()
        rc = N.lib.bmqcrc_expire_records_pack(ctypes.byref(p), ctypes.byref(r), ctypes.byref(o))
        err = N.lib.bmqcrc_last_error()
        res = r.as_dict() if sync else last_expire_records(cuda.index, stream)
        host = {name: t.cpu().numpy() for name, t in arr.items()}
        if place is not None:
            place.check()
    for name, (dt, _, _) in CANARY.items():
        if name in host:
            host[name] = host[name].view(dt)
    return rc, err, res, host


def _untouched(name, a):
    return bool((a == (CANARY[name][1] if name in CANARY else SENTINEL)).all())


def _model(run, table, kw):
    """M.expire_records' answer to the call `kw` describes ("exact": size only)."""
    mkw = {k: kw.get(k) for k in ("now", "lease_id", "first_seq", "select", "journal_dst_bytes")}
    if mkw["journal_dst_bytes"] == "exact":
        mkw["journal_dst_bytes"] = None
    return M.expire_records(run, *table, **mkw)


def _check(cuda, run, table, kw, sync=True, stream=None, skip=(), phases=None, model=None):
    """The call against the model: a refusal identical and nothing written, or
    every destination byte, array entry and result field.  `journal_dst_bytes`
    "exact" is what the model says the call writes, None a size-only call.
    `model` is _model's answer to this very call when the caller has it already
    (a size-only call's answer serves for "exact" and the other way round: only
    DST_TOO_SMALL looks at the size); the model is not run then.  Returns
    (model, host)."""
    kw = dict(kw)
    sized = model if model is not None else \
        _model(run, table, kw) if kw.get("journal_dst_bytes") == "exact" else None
    if kw.get("journal_dst_bytes") == "exact":
        kw["journal_dst_bytes"] = \
            sized.result["journal_bytes"] if isinstance(sized, M.Expired) else 600
    m = model if model is not None else _model(run, table, kw)
    rc, err, res, host = _raw(cuda, run, table, kw, sync=sync, stream=stream, skip=skip,
                              phases=phases)
    n_records = len(run) // 60
    if isinstance(m, M.Refusal):
        if sync:
            assert rc == N.BMQCRC_EINVAL and KIND_NAME[m.kind] in err, (rc, err, m)
            assert b"nothing was written" in err and (b"%d" % m.index) in err, (err, m)
        else:
            assert rc == 0, err
        assert res == M.refused_result(m, n_records), (res, m)
        for name, a in host.items():
            assert _untouched(name, a), name
        return m, host
    assert rc == 0, err
    assert res == m.result, (res, m.result)
    if kw.get("journal_dst_bytes") is None or n_records == 0:   # size only, or nothing launched
        for name, a in host.items():
            assert _untouched(name, a), name
        return m, host
    for name, want in (("journal_dst", m.journal), ("expired", m.expired),
                       ("new_index", m.new_index), ("select_out", m.select_out),
                       ("queue_expired", m.queue_expired), ("queue_front", m.queue_front)):
        if name in skip:
            continue
        assert np.array_equal(host[name][:len(want)], want), name
        assert _untouched(name, host[name][len(want):]), name
    return m, host


# ---- runs ------------------------------------------------------------------------

NOW = 100000


def _queue_key(i):
    """Queue key number i (below 2^23): five bytes, none of them zero for the
    first, and different for different i."""
    return bytes([1 + (i & 0x7F), (i >> 7) & 0xFF, (i >> 15) & 0xFF, 0xA5, 0x5A])


def _table(n_queues, n_keys, seed, ttl_top=200):
    """A table of `n_queues` entries: the keys _queue_key(i) of a random choice
    of i below max(n_keys, n_queues) in a random order (with n_keys above
    n_queues some keys of a run over n_keys have no entry), TTLs below ttl_top
    and, here and there, the longest."""
    rng = np.random.default_rng([seed, n_queues])
    which = rng.permutation(max(n_keys, n_queues))[:n_queues]
    ttl = rng.integers(0, ttl_top, n_queues).astype(np.uint64)
    ttl[rng.random(n_queues) < 0.02] = np.uint64(M.M64)
    return C.table([(_queue_key(int(i)), 0) for i in which])[0], ttl


@functools.lru_cache(maxsize=None)
def _mixed(n=3000, seed=21, n_keys=4):
    """(run of n records of every type, the next sequence number): messages in
    n_keys queues with timestamps from 250 seconds before NOW to 50 after it,
    CONFIRM records, DELETION records of earlier and of LATER messages,
    QUEUE_OP and JOURNAL_OP records.  Written by PartitionWriter.  Shared,
    never modified."""
    rng = np.random.default_rng(seed)
    w = S.PartitionWriter(lease_id=9)
    msgs = []
    while len(w.recs) < n:
        roll = int(rng.integers(0, 10))
        if roll < 5 or not msgs:
            key = _queue_key(int(rng.integers(0, n_keys)))
            guid = (0x77000000 + len(msgs)).to_bytes(16, "big")
            w.message(b"", key, guid=guid, timestamp=NOW - 250 + int(rng.integers(0, 300)))
            msgs.append((guid, key))
        elif roll < 7:
            w.confirm(*msgs[int(rng.integers(0, len(msgs)))])
        elif roll == 7:
            if rng.random() < 0.5:
                w.deletion(*msgs[int(rng.integers(0, len(msgs)))])
            else:   # of the message that comes five messages on, should its key be the first
                w.deletion((0x77000000 + len(msgs) + 5).to_bytes(16, "big"), _queue_key(0))
        elif roll == 8:
            w.queue_op(int(rng.integers(1, 5)), _queue_key(int(rng.integers(0, n_keys))))
        else:
            w.sync_point()
    run = w.files()[0][JH:]
    assert run.size == 60 * n
    run.setflags(write=False)
    return run, w.seq + 1


def _be(values, width):
    """Integers as rows of `width` big-endian bytes."""
    v = np.asarray(values, np.uint64)
    return np.stack([(v >> np.uint64(8 * (width - 1 - k))).astype(np.uint8)
                     for k in range(width)], axis=1)


@functools.lru_cache(maxsize=None)
def _bulk(n, n_keys, seed, only_messages=False, age=None):
    """(run of n records laid out in numpy, the next sequence number, per
    record the queue number and the timestamp): the large runs, which
    PartitionWriter would take too long to write record by record.  Record r
    has sequence number r + 1; a MESSAGE record's GUID is r + 1; six records in
    ten are MESSAGE records, the rest the other four types in equal parts.
    Half of the CONFIRM and DELETION records name a MESSAGE record anywhere in
    the run, the others nobody.  Timestamps run from 250 seconds before NOW to
    50 after it, or are all NOW - age.  Shared, never modified."""
    rng = np.random.default_rng([seed, n])
    types = np.ones(n, np.uint8) if only_messages else \
        rng.choice(np.array([1, 2, 3, 4, 5], np.uint8), n, p=[0.6, 0.1, 0.1, 0.1, 0.1])
    queue = rng.integers(0, n_keys, n)
    ts = (NOW - 250 + rng.integers(0, 300, n)).astype(np.uint64) if age is None else \
        np.full(n, NOW - age, np.uint64)
    msgs = np.flatnonzero(types == 1)
    named = np.arange(n)
    if msgs.size:   # whom a CONFIRM or DELETION record names: a message, or itself (nobody)
        pick = msgs[rng.integers(0, msgs.size, n)]
        named = np.where(rng.random(n) < 0.5, pick, named)
    keys = np.stack([1 + (queue & 0x7F), (queue >> 7) & 0xFF, (queue >> 15) & 0xFF,
                     np.full(n, 0xA5), np.full(n, 0x5A)], axis=1).astype(np.uint8)
    guids = np.zeros((n, 16), np.uint8)
    guids[:, 8:] = _be(np.arange(1, n + 1), 8)
    recs = np.zeros((n, 60), np.uint8)
    recs[:, 0] = types << 4
    recs[:, 2:8] = _be(np.arange(1, n + 1), 6)
    recs[:, 11] = 9
    recs[:, 12:20] = _be(ts, 8)
    recs[:, 56:60] = np.frombuffer(M.MAGIC, np.uint8)
    m, c, d, q = (types == t for t in (1, 2, 3, 4))
    recs[m, 1] = 1                                   # refCount 1
    recs[m, 22:27], recs[m, 36:52] = keys[m], guids[m]
    recs[m, 32:36] = _be(np.full(int(m.sum()), 5), 4)
    recs[c, 22:27], recs[c, 32:48] = keys[named[c]], guids[named[c]]
    recs[d, 23:28], recs[d, 28:44] = keys[named[d]], guids[named[d]]
    recs[q, 22:27] = keys[q]
    recs[q, 32:36] = _be(rng.integers(1, 5, int(q.sum())), 4)
    run = recs.reshape(-1)
    run.setflags(write=False)
    return run, n + 1, queue, ts


def test_the_bulk_layout_is_the_writers():
    """_bulk's records parse as PartitionWriter's do: the same positions."""
    run, _, queue, ts = _bulk(200, 3, 1)
    recs = run.reshape(-1, 60)
    w = S.PartitionWriter(lease_id=9)
    for r in range(200):
        t = recs[r, 0] >> 4
        w.seq, w.ts = r, int(ts[r])
        if t == 1:
            w.message(b"", _queue_key(int(queue[r])), guid=recs[r, 36:52].tobytes())
            w.recs[-1] = w.recs[-1][:32] + recs[r, 32:36].tobytes() + w.recs[-1][36:52] + bytes(4) + \
                w.recs[-1][56:]      # (the writer's DATA offset and CRC)
        elif t == 2:
            w.confirm(recs[r, 32:48].tobytes(), recs[r, 22:27].tobytes())
        elif t == 3:
            w.deletion(recs[r, 28:44].tobytes(), recs[r, 23:28].tobytes())
        elif t == 4:
            w.queue_op(int(recs[r, 35]), _queue_key(int(queue[r])))
            w.recs[-1] = w.recs[-1][:36] + bytes(4) + w.recs[-1][40:]   # (its QLIST offset)
        else:
            w.recs.append(recs[r].tobytes())        # (a JOURNAL_OP record's body is not read)
    assert b"".join(w.recs) == run.tobytes()


# ---- sizes, selects, tables ---------------------------------------------------------

@pytest.mark.parametrize("n_queues", [0, 1, 3, 1025])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1025])
def test_run_sizes_and_table_sizes(cuda, n, n_queues):
    run, seq = _mixed()
    kw = dict(now=NOW, lease_id=9, first_seq=seq, journal_dst_bytes="exact")
    m, _ = _check(cuda, run[:60 * n], _table(n_queues, 4, n), kw)
    assert isinstance(m, M.Expired)


@pytest.mark.parametrize("n_queues", [0, 1, 3, 1025])
@pytest.mark.parametrize("select", ["all", "none", "second", None])
def test_mixed_records_over_three_blocks(cuda, select, n_queues):
    run, seq = _mixed()
    n_records = run.size // 60
    assert n_records == 3000 and set((run.reshape(-1, 60)[:, 0] >> 4).tolist()) == {1, 2, 3, 4, 5}
    sel = {"all": np.ones(n_records, np.uint8), "none": np.zeros(n_records, np.uint8),
           "second": (np.arange(n_records) % 2).astype(np.uint8), None: None}[select]
    # (three entries out of six keys and 1,025 out of 1,025: the run's four keys
    # are in the table or not, by the seed)
    table = _table(n_queues, 6 if n_queues == 3 else 4, 5, ttl_top=150)
    kw = dict(now=NOW, lease_id=9, first_seq=seq, select=sel, journal_dst_bytes="exact")
    m, _ = _check(cuda, run, table, kw)
    assert isinstance(m, M.Expired)
    if select == "none":
        assert m.result["n_live"] == 0 and not m.select_out.any()
    elif n_queues == 0:
        assert m.result["n_expired"] == 0 and m.result["n_no_queue"] == m.result["n_live"] > 500
    elif n_queues == 1025:
        assert m.result["n_no_queue"] == 0 and m.result["n_expired"] > 0


def test_all_five_types_four_queues_and_every_outcome(cuda):
    """The mixed run against a table that holds three of its four queues, with
    TTLs that let some messages of each expire: expired, shielded, young, dead
    and queue-less messages in one call."""
    run, seq = _mixed()
    table = C.table([(_queue_key(2), 60), (_queue_key(0), 150), (b"\x01\x02\x03\x04\x05", 9),
                     (_queue_key(1), 249)])
    kw = dict(now=NOW, lease_id=9, first_seq=seq, journal_dst_bytes="exact")
    m, _ = _check(cuda, run, table, kw)
    assert m.result["n_no_queue"] > 100 and m.result["n_expired"] >= 3
    assert all(f != M.NONE for f in m.queue_front[[0, 1, 3]]) and m.queue_front[2] == M.NONE
    assert m.queue_expired[2] == 0 and int(m.select_out.sum()) > 500


@pytest.mark.parametrize("case", C.HAND_WORKED, ids=lambda c: c.__name__)
def test_hand_worked(cuda, case):
    c = case()
    m, host = _check(cuda, c.run, c.table, dict(c.kw, journal_dst_bytes="exact"))
    n = c.run.size // 60
    assert np.flatnonzero(host["expired"][:n]).tolist() == c.expired
    assert np.flatnonzero(host["select_out"][:n]).tolist() == c.select_out
    assert host["queue_front"][:len(c.queue_front)].tolist() == c.queue_front
    assert host["queue_expired"][:len(c.queue_front)].tolist() == c.queue_expired


def test_the_references_garbage_collect_test(cuda):
    run, seq = C.ten_messages()
    table = C.table([(C.KEY_A, 20)])
    kw = dict(lease_id=C.LEASE, first_seq=seq, journal_dst_bytes="exact")
    m, _ = _check(cuda, run, table, dict(kw, now=5))
    assert m.result["n_expired"] == 0
    m, host = _check(cuda, run, table, dict(kw, now=26))
    assert m.result["n_expired"] == 5 and host["expired"][:10].tolist() == [1] * 5 + [0] * 5
    grown = np.concatenate([run, host["journal_dst"][:300]])
    m, host = _check(cuda, grown, table, dict(kw, now=100, first_seq=seq + 5))
    assert m.result["n_expired"] == 5 and not host["select_out"][:15].any()


@pytest.mark.parametrize("skip", list(CANARY) + ["all"])
def test_each_output_null(cuda, skip):
    run, seq = _mixed()
    kw = dict(now=NOW, lease_id=9, first_seq=seq, journal_dst_bytes="exact",
              select=np.ones(3000, np.uint8) if skip == "all" else None)
    _check(cuda, run, _table(3, 4, 2), kw, skip=tuple(CANARY) if skip == "all" else (skip,))


def test_size_only_then_the_real_call(cuda):
    run, seq = _mixed()
    table = _table(4, 4, 3)
    kw = dict(now=NOW, lease_id=9, first_seq=seq)
    sized, _ = _check(cuda, run, table, dict(kw, journal_dst_bytes=None))
    _check(cuda, run, table, dict(kw, journal_dst_bytes=None), sync=False)
    need = sized.result["journal_bytes"]
    assert need >= 120
    full, _ = _check(cuda, run, table, dict(kw, journal_dst_bytes=need))
    assert full.result == sized.result
    m, _ = _check(cuda, run, table, dict(kw, journal_dst_bytes=need - 1))
    assert m == M.Refusal(M.DST_TOO_SMALL, int(np.flatnonzero(sized.expired)[-1]))


def test_the_destination_is_the_tail_of_the_runs_own_allocation(cuda):
    import torch
    run, seq = _mixed()
    keys, ttl = _table(4, 4, 3)
    want = M.expire_records(run, keys, ttl, now=NOW, lease_id=9, first_seq=seq)
    room = want.result["journal_bytes"]
    assert room >= 120
    whole = torch.full((run.size + room + SLACK,), SENTINEL, dtype=torch.uint8, device=cuda)
    whole[:run.size] = torch.from_numpy(np.array(run)).to(cuda)
    d_keys, d_ttl = _t(cuda, keys, np.uint8), _t(cuda, ttl, np.uint64)
    r = expire_records(whole[:run.size], d_keys, d_ttl, now=NOW, lease_id=9, first_seq=seq,
                       journal_dst=whole[run.size:run.size + room])
    assert r.result == want.result
    got = whole.cpu().numpy()
    assert np.array_equal(got[:run.size], run)
    assert np.array_equal(got[run.size:run.size + room], want.journal)
    assert (got[run.size + room:] == SENTINEL).all()
    assert np.array_equal(r.select_out.cpu().numpy(), want.select_out)
    assert np.array_equal(r.queue_front.cpu().numpy().view(np.uint32), want.queue_front)
    # ... and the grown run is the next call's: nothing new expires, what did is gone
    again = expire_records(whole[:run.size + room], d_keys, d_ttl, now=NOW, lease_id=9,
                           first_seq=r.result["next_seq"])
    assert again.result["n_expired"] == 0 and again.journal_dst.numel() == 0
    assert again.result["n_live"] == want.result["n_live"] - want.result["n_expired"]
    assert np.array_equal(again.select_out.cpu().numpy()[:3000], want.select_out)
    assert np.array_equal(again.queue_front.cpu().numpy().view(np.uint32), want.queue_front)


def test_the_wrapper_sizes_the_destination_and_takes_an_empty_run_and_table(cuda):
    import torch
    run, seq = _mixed()
    keys, ttl = _table(4, 4, 3)
    want = M.expire_records(run, keys, ttl, now=NOW, lease_id=9, first_seq=seq)
    r = expire_records(_t(cuda, run, np.uint8), _t(cuda, keys, np.uint8), _t(cuda, ttl, np.uint64),
                       now=NOW, lease_id=9, first_seq=seq)
    assert r.result == want.result and last_expire_records(cuda.index) == want.result
    assert np.array_equal(r.journal_dst.cpu().numpy(), want.journal)
    assert np.array_equal(r.expired.cpu().numpy(), want.expired)
    assert np.array_equal(r.new_index.cpu().numpy().view(np.uint32), want.new_index)
    assert np.array_equal(r.queue_expired.cpu().numpy().view(np.uint32), want.queue_expired)
    none = expire_records(_t(cuda, run, np.uint8), torch.zeros(0, dtype=torch.uint8, device=cuda),
                          torch.zeros(0, dtype=torch.int64, device=cuda), now=NOW, lease_id=9,
                          first_seq=seq)
    assert none.result["n_expired"] == 0 and none.queue_front.numel() == 0
    assert none.result["n_no_queue"] == none.result["n_live"] == want.result["n_live"]
    empty = expire_records(torch.zeros(0, dtype=torch.uint8, device=cuda), _t(cuda, keys, np.uint8),
                           _t(cuda, ttl, np.uint64), now=NOW, lease_id=9, first_seq=seq)
    assert empty.result == M.expire_records(np.zeros(0, np.uint8), keys, ttl, now=NOW, lease_id=9,
                                            first_seq=seq).result
    assert empty.queue_front is None and empty.journal_dst.numel() == 0


# ---- refusals ------------------------------------------------------------------------

@pytest.mark.parametrize("sync", [True, False], ids=["sync", "async"])
@pytest.mark.parametrize("r", C.refused(), ids=lambda r: r.name)
def test_every_refusal(cuda, r, sync):
    m, _ = _check(cuda, r.run, r.table, r.kw, sync=sync)
    assert m == M.Refusal(r.kind, r.index)


@pytest.mark.parametrize("sync", [True, False], ids=["sync", "async"])
def test_a_violation_in_the_last_record_of_the_last_block_and_in_the_last_entry(cuda, sync):
    run, seq = _mixed()
    keys, ttl = _table(1025, 4, 5)
    kw = dict(now=NOW, lease_id=9, first_seq=seq, journal_dst_bytes=60)
    bad = np.array(run)
    bad[60 * 2999 + 59] ^= 1                 # the magic of record 2,999
    m, _ = _check(cuda, bad, (keys, ttl), kw, sync=sync)
    assert m == M.Refusal(M.RECORD_HEADER, 2999)
    # the last record a second MESSAGE record of the first one's key
    recs = np.array(run).reshape(-1, 60)
    first = int(np.flatnonzero(recs[:, 0] >> 4 == 1)[0])
    recs[2999, :2], recs[2999, 20:56] = recs[first, :2], recs[first, 20:56]
    m, _ = _check(cuda, recs.reshape(-1), (keys, ttl), kw, sync=sync)
    assert m == M.Refusal(M.DUPLICATE_MESSAGE, first)
    # the last entry: null, and entry 7's key again
    null = keys.copy()
    null[-5:] = 0
    m, _ = _check(cuda, run, (null, ttl), kw, sync=sync)
    assert m == M.Refusal(M.QUEUE_KEY, 1024)
    twice = keys.copy()
    twice[-5:] = twice[35:40]
    m, _ = _check(cuda, run, (twice, ttl), kw, sync=sync)
    assert m == M.Refusal(M.QUEUE_KEY, 7)
    # two kinds at once: the lower kind, though its index is the higher
    m, _ = _check(cuda, bad, (null, ttl), kw, sync=sync)
    assert m == M.Refusal(M.RECORD_HEADER, 2999)
    m, _ = _check(cuda, recs.reshape(-1), (twice, ttl), kw, sync=sync)
    assert m == M.Refusal(M.DUPLICATE_MESSAGE, first)
    # the last expired message's record is the one that does not fit
    want = M.expire_records(run, keys, ttl, now=NOW, lease_id=9, first_seq=seq)
    last = int(np.flatnonzero(want.expired)[-1])
    short = dict(kw, journal_dst_bytes=want.result["journal_bytes"] - 1)
    m, _ = _check(cuda, run, (keys, ttl), short, sync=sync)
    assert m == M.Refusal(M.DST_TOO_SMALL, last)
    m, _ = _check(cuda, run, (twice, ttl), short, sync=sync)
    assert m == M.Refusal(M.QUEUE_KEY, 7)


# ---- keys chosen to collide in each table (join_collisions.py, expire_collisions.py) ----

def _join_case(c, ttl_of):
    """A join_collisions run (every message of the writer's one timestamp) with
    a table of its messages' queue keys: TTL ttl_of(k) for the k-th distinct one."""
    recs = np.asarray(c.run).reshape(-1, 60)
    ts = int.from_bytes(recs[1, 12:20].tobytes(), "big")
    keys = list(dict.fromkeys(recs[r, 22:27].tobytes() for r in np.flatnonzero(recs[:, 0] >> 4 == 1)))
    table = C.table([(k, ttl_of(i)) for i, k in enumerate(keys)])
    kw = dict(now=ts + 100, lease_id=c.info["lease_id"], first_seq=c.info["next_seq"],
              journal_dst_bytes="exact")
    return table, kw


def test_one_join_chain_across_the_tables_end(cuda):
    """200 messages with one home eight slots before the JoinTable's end,
    DELETION records of the run among them, every queue-key byte 0x80 or more;
    every second queue's TTL has run out.  Twice: the outputs are equal."""
    c = J.confirm_chain()
    table, kw = _join_case(c, lambda i: 50 if i % 2 else 200)
    m, host = _check(cuda, c.run, table, kw)
    assert isinstance(m, M.Expired)
    assert m.result["n_live"] == J.CHAIN - J.CHAIN // 10 and 80 <= m.result["n_expired"] <= 100
    _, again = _check(cuda, c.run, table, kw, model=m)
    assert sorted(again) == sorted(host)
    assert all(np.array_equal(host[name], again[name]) for name in host)


def test_a_join_chain_longer_than_a_block(cuda):
    c = J.confirm_long()
    table, kw = _join_case(c, lambda i: 99)
    m, _ = _check(cuda, c.run, table, kw)
    assert m.result["n_expired"] == J.LONG


@pytest.mark.parametrize("swapped", [False, True], ids=["low_first", "high_first"])
def test_near_pairs_in_one_join_chain(cuda, swapped):
    """Per key byte two messages that differ in bit 0x80 of it only, all 42 in
    one chain; a DELETION record appended for the first of each pair: its twin
    stays live and expires."""
    c = J.confirm_pairs(swapped)
    w = S.PartitionWriter(lease_id=c.info["lease_id"])
    w.seq = c.info["next_seq"] - 1
    for a, _ in c.info["pairs"]:
        w.deletion(*J.split(a))
    run = np.concatenate([c.run, np.frombuffer(b"".join(w.recs), np.uint8)])
    table, kw = _join_case(c, lambda i: 99)
    m, host = _check(cuda, run, table, dict(kw, first_seq=w.seq + 1))
    assert m.result["n_live"] == m.result["n_expired"] == J.PAIRS
    assert np.flatnonzero(host["expired"][:64]).tolist() == list(range(2, 43, 2))


def test_a_duplicate_behind_a_join_chain(cuda):
    c = J.confirm_duplicate()
    table, kw = _join_case(c, lambda i: 99)
    m, _ = _check(cuda, c.run, table, kw)
    assert m == M.Refusal(M.DUPLICATE_MESSAGE, J.BEHIND)


def test_one_queue_chain_across_the_tables_end(cuda):
    """200 table entries with one home eight slots before the queue hash's end
    and 40 absent keys that walk the whole chain.  Twice: the outputs are equal."""
    c = X.queue_chain()
    kw = dict(c.kw, journal_dst_bytes="exact")
    m, host = _check(cuda, c.run, c.table, kw)
    assert (m.result["n_expired"], m.result["n_no_queue"]) == (180, 76)
    _, again = _check(cuda, c.run, c.table, kw, model=m)
    assert all(np.array_equal(host[name], again[name]) for name in host)


def test_a_queue_chain_longer_than_a_block(cuda):
    c = X.queue_long()
    m, host = _check(cuda, c.run, c.table, dict(c.kw, journal_dst_bytes="exact"))
    assert m.result["n_expired"] == X.LONG
    assert host["queue_expired"][:X.LONG].tolist() == [1] * X.LONG


def test_a_duplicate_behind_a_queue_chain(cuda):
    c = X.queue_duplicate()
    m, _ = _check(cuda, c.run, c.table, dict(c.kw, journal_dst_bytes="exact"))
    assert m == M.Refusal(M.QUEUE_KEY, X.BEHIND - 1)


# ---- past one tile per block, past one wave of block sums, past the frame grid
# (test_grid_regimes.py names the regimes and pins the sizes) ---------------------

def _outcomes(run, queue, ts, table, m):
    """(expired, shielded, queue-less) messages of the model's answer `m`:
    shielded is live, in the table, not young by its own timestamp and yet not
    expired."""
    keys, ttl = table
    entry = {bytes(k): q for q, k in enumerate(np.asarray(keys).reshape(-1, 5))}
    of_record = np.array([entry.get(_queue_key(int(i)), -1) for i in range(int(queue.max()) + 1)])
    q = of_record[queue]
    has = q >= 0
    young = np.zeros(run.size // 60, bool)
    young[has] = (np.uint64(NOW) - ts[has]) <= ttl[q[has]]       # uint64: it wraps
    kept = m.select_out != 0
    return m.result["n_expired"], int((kept & has & ~young).sum()), m.result["n_no_queue"]


@functools.lru_cache(maxsize=None)
def _two_tiles_case():
    run, seq, queue, ts = _bulk(G.N_TILES, 44000, 31)
    table = _table(40000, 44000, 32)
    kw = dict(now=NOW, lease_id=9, first_seq=seq, journal_dst_bytes="exact")
    return run, table, kw, queue, ts


@pytest.mark.parametrize("select", [None, "second"])
def test_two_tiles_of_records_per_block_and_40000_queues(cuda, select):
    """Records in regime D (stage()'s second tile, layout_count's carry, the
    record loops of every kernel a second time), the table in 40 blocks beside
    them in k_exp_classify."""
    run, table, kw, queue, ts = _two_tiles_case()
    assert G.regime(G.N_TILES)[:2] == (129, 2048) and G.regime(40000).nblocks == 40
    sel = (np.arange(G.N_TILES) % 2).astype(np.uint8) if select else None
    want = _model(run, table, dict(kw, select=sel))
    assert isinstance(want, M.Expired)
    assert min(_outcomes(run, queue, ts, table, want)) > 1000, \
        _outcomes(run, queue, ts, table, want)
    _check(cuda, run, table, dict(kw, select=sel), model=want)


def test_records_past_the_frame_grid_all_expiring(cuda):
    """Regime E: both record loops of k_exp_frame take a second step (record
    524,288 is thread 0's).  Every record is a message, and every one expires.
    The size-only call reports what the full call reports."""
    run, seq, queue, ts = _bulk(G.N_FRAME, 3, 33, only_messages=True, age=500)
    assert G.regime(G.N_FRAME).units_past_grid
    table = C.table([(_queue_key(1), 100), (_queue_key(0), 499), (_queue_key(2), 0)])
    kw = dict(now=NOW, lease_id=9, first_seq=seq, journal_dst_bytes="exact")
    want = _model(run, table, kw)
    assert want.result["n_expired"] == G.N_FRAME and not want.select_out.any()
    assert int(want.queue_expired.sum()) == G.N_FRAME
    full, host = _check(cuda, run, table, kw, model=want)
    assert host["new_index"].size == G.N_FRAME + GUARD
    sized, _ = _check(cuda, run, table, dict(kw, journal_dst_bytes=None), model=want)
    assert sized.result == full.result


def _lds_queues():
    """kExpLdsQueues: the longest table k_exp_front and k_exp_seal reduce in LDS."""
    return G.constants(("kExpLdsQueues",))["kExpLdsQueues"]


@pytest.mark.parametrize("past", [0, 1], ids=["at", "past"])
def test_the_table_at_and_past_the_length_that_is_reduced_in_lds(cuda, past):
    """kExpLdsQueues entries: each block lowers fronts and counts in LDS and
    hands them on once; one more: every thread goes to memory."""
    run, seq = _mixed()
    n_queues = _lds_queues() + past
    assert n_queues == 2048 + past
    kw = dict(now=NOW, lease_id=9, first_seq=seq, journal_dst_bytes="exact")
    m, _ = _check(cuda, run, _table(n_queues, 4, 6, ttl_top=150), kw)
    assert m.result["n_no_queue"] == 0 and m.result["n_expired"] > 0
    assert int((m.queue_front != M.NONE).sum()) >= 2


@pytest.mark.parametrize("n_queues", [1, 2049], ids=["in_lds", "in_memory"])
@pytest.mark.parametrize("young", ["one", "all_but_five"])
def test_one_queue_of_n_few_messages(cuda, young, n_queues):
    """One queue: its single young message at index N_FEW - 2 (every message
    before it expires, the old one behind it is shielded), or every message
    young but the first five (N_FEW - 5 threads lower one front).  The queue is
    the table's last entry; behind 2,048 others the threads meet at one word of
    memory, and N_FEW - 2 of them at the queue's count."""
    run, seq, _, _ = _bulk(G.N_FEW, 1, 34, only_messages=True, age=500)
    recs = np.array(run).reshape(-1, 60)
    fresh = [G.N_FEW - 2] if young == "one" else list(range(5, G.N_FEW))
    recs[fresh, 12:20] = _be(np.full(len(fresh), NOW - 1), 8)
    assert n_queues == 1 or n_queues > _lds_queues()
    table = C.table([(_queue_key(1 + i), 7) for i in range(n_queues - 1)] + [(_queue_key(0), 100)])
    kw = dict(now=NOW, lease_id=9, first_seq=seq, journal_dst_bytes="exact")
    m, host = _check(cuda, recs.reshape(-1), table, kw)
    assert m.result["n_expired"] == fresh[0] and host["queue_front"][n_queues - 1] == fresh[0]
    assert np.flatnonzero(host["select_out"][:G.N_FEW]).tolist() == \
        list(range(fresh[0], G.N_FEW))


def _duplicate_message_in_two_tiles_of_one_block():
    """The first MESSAGE record of block 3 of N_TILES records again in the
    block's second tile."""
    run, table, kw, _, _ = _two_tiles_case()
    recs = np.array(run).reshape(-1, 60)
    lo = 3 * G.regime(G.N_TILES).per_block
    first = lo + int(np.flatnonzero(recs[lo:lo + 1024, 0] >> 4 == 1)[0])
    twin = lo + 1024 + 11
    recs[twin, :2], recs[twin, 20:56] = recs[first, :2], recs[first, 20:56]
    return recs.reshape(-1), table, kw, M.Refusal(M.DUPLICATE_MESSAGE, first)


def _queue_key_twice_in_the_tables_last_block():
    """Entry 39,999 of 40,000 (block 39 of the table's 40) holds entry 1,030's
    key (block 1), and the run's last record has a wrong magic: RECORD_HEADER is
    the lower kind."""
    run, (keys, ttl), kw, _, _ = _two_tiles_case()
    keys = keys.copy()
    keys[-5:] = keys[5 * 1030:5 * 1031]
    bad = np.array(run)
    bad[-1] ^= 1
    return bad, (keys, ttl), kw, M.Refusal(M.RECORD_HEADER, G.N_TILES - 1)


def _queue_key_twice_across_blocks():
    run, (keys, ttl), kw, _, _ = _two_tiles_case()
    keys = keys.copy()
    keys[-5:] = keys[5 * 1030:5 * 1031]
    return run, (keys, ttl), kw, M.Refusal(M.QUEUE_KEY, 1030)


def _destination_one_record_short():
    """The last expired message of N_TILES records, behind the sums of 129
    blocks of two tiles, is the one that does not fit."""
    run, table, kw, _, _ = _two_tiles_case()
    want = _model(run, table, kw)
    last = int(np.flatnonzero(want.expired)[-1])
    assert last > G.N_TILES - 2048          # in the last block
    short = dict(kw, journal_dst_bytes=want.result["journal_bytes"] - 60)
    return run, table, short, M.Refusal(M.DST_TOO_SMALL, last)


@pytest.mark.parametrize("case", [
    _duplicate_message_in_two_tiles_of_one_block, _queue_key_twice_in_the_tables_last_block,
    _queue_key_twice_across_blocks, _destination_one_record_short],
    ids=lambda f: f.__name__.strip("_"))
def test_refusals_across_tiles_and_blocks(cuda, case):
    """What the model refuses past one tile per block, synchronous and
    asynchronous, with nothing written."""
    run, table, kw, expected = case()
    want = _model(run, table, kw)
    assert want == expected
    for sync in (True, False):
        m, _ = _check(cuda, run, table, kw, sync=sync, model=want)
        assert m == expected


def test_every_base_pointer_at_the_smallest_alignment_the_abi_permits(cuda):
    run, seq = _mixed()
    kw = dict(now=NOW, lease_id=9, first_seq=seq, select=np.ones(3000, np.uint8),
              journal_dst_bytes="exact")
    m, _ = _check(cuda, run[:60 * 1025], _table(1025, 4, 5), dict(kw, select=np.ones(1025, np.uint8)),
                  phases=PHASES)
    assert m.result["n_expired"] > 0
    r = C.refused()[-1]
    _check(cuda, r.run, r.table, r.kw, phases=PHASES)     # refused


def test_state(cuda):
    import torch
    rng = np.random.default_rng(56)
    host = rng.integers(0, 256, size=1 << 18, dtype=np.uint8)
    arena = torch.from_numpy(host).to(cuda)
    lens = rng.integers(1, 1025, size=3001).astype(np.uint32)
    offs = (rng.random(lens.size) * (host.size - 1100)).astype(np.int64)
    d_off, d_len = _t(cuda, offs, np.int64), _t(cuda, lens, np.uint32)
    qkeys, guids = random_meta(rng, 30)
    run, seq = _mixed()
    table = _table(3, 4, 2)
    kw = dict(now=NOW, lease_id=9, first_seq=seq, journal_dst_bytes="exact")
    s = _side_stream(cuda)

    def records():
        return (last_launch(cuda.index, s, offsets=True), last_copy(cuda.index, s),
                last_put_pack(cuda.index, s), last_records_pack(cuda.index, s),
                last_put_unpack(cuda.index, s), last_records_unpack(cuda.index, s),
                last_journal_select(cuda.index, s), last_storage_apply(cuda.index, s),
                last_storage_pack(cuda.index, s), last_push_pack(cuda.index, s),
                last_rollover(cuda.index, s), last_confirm_records(cuda.index, s))
    with torch.cuda.stream(s):
        # none yet on s
        assert last_expire_records(cuda.index, s) == M.refused_result(M.Refusal(0, 0), 0)
        Crc32c.calculate_batch(arena, d_off, d_len, stream=s)
        dst, jour, _, _, _ = pack_records(
            arena, d_off[:30], d_len[:30], _t(cuda, qkeys, np.uint8), _t(cuda, guids, np.uint8),
            file_key=b"\x11\x22\x33\x44\x55", lease_id=3, first_seq=2, data_file_pos=40, stream=s)
        select_records(jour, data_file_bytes=40 + dst.numel(), stream=s)
        rollover_records(jour, dst, data_file_pos=40, new_data_file_pos=40, stream=s)
        pack_storage_events(jour, dst, journal_pos=JH, data_file_pos=40, partition_id=1, stream=s)
        pack_push_events(jour, dst, data_file_pos=40,
                         queue_ids=_t(cuda, np.arange(30), np.int32), stream=s)
        S.confirm_records(jour, _t(cuda, guids[:3], np.uint8), _t(cuda, qkeys[:3], np.uint8),
                          lease_id=3, first_seq=40, stream=s)
        before = records()
        _check(cuda, run, table, kw, stream=s)
        _check(cuda, run, table, kw, stream=s, sync=False)
        _check(cuda, run, table, dict(kw, journal_dst_bytes=59), stream=s)    # a refused one
        _check(cuda, run, table, dict(kw, journal_dst_bytes=None), stream=s)  # a size-only one
        assert records() == before
        out = Crc32c.calculate_batch(arena, d_off, d_len, stream=s)
    s.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), P.host_crcs(host, offs, lens))


# ---- the pipeline ------------------------------------------------------------

def test_a_partition_that_expires_on_one_device(cuda):
    # pack_records (two queues, TTL 10 and 1,000) -> expire_records ->
    # pack_storage_events over the new records -> apply_events on a second
    # partition -> select_records -> rollover_records(keep=select) ->
    # pack_push_events delivers only the unexpired messages.  No payload byte
    # comes to the host before the delivery is read back.
    import torch
    rng = np.random.default_rng(20)
    n = 200
    lens = rng.integers(1, 301, size=n).astype(np.uint32)
    soff = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    src = rng.integers(0, 256, size=int(lens.sum()), dtype=np.uint8)
    qkeys, guids = random_meta(rng, n)
    short = np.arange(n) % 2 == 0
    qkeys[:] = np.frombuffer(KEYS[1], np.uint8)
    qkeys[short] = np.frombuffer(KEYS[0], np.uint8)
    w = S.PartitionWriter(lease_id=7, partition_id=2)
    w.queue_op(S.OP_CREATION, KEYS[0])
    w.queue_op(S.OP_CREATION, KEYS[1])
    head = _t(cuda, np.frombuffer(b"".join(w.recs), np.uint8).copy(), np.uint8)
    data, jour, _, _, _ = pack_records(
        _t(cuda, src, np.uint8), _t(cuda, soff, np.int64), _t(cuda, lens, np.uint32),
        _t(cuda, qkeys, np.uint8), _t(cuda, guids, np.uint8), file_key=b"\x11\x22\x33\x44\x55",
        lease_id=7, first_seq=3, data_file_pos=40, timestamp=5000)
    journal = torch.cat([head, jour])
    keys, ttl = C.table([(KEYS[1], 1000), (KEYS[0], 10)])
    e = expire_records(journal, _t(cuda, keys, np.uint8), _t(cuda, ttl, np.uint64), now=5100,
                       lease_id=7, first_seq=n + 3)
    assert e.result == dict(n_records=n + 2, n_live=n, n_expired=n // 2, n_no_queue=0,
                            journal_bytes=60 * (n // 2), next_seq=n + 3 + n // 2, refused_kind=0,
                            refused_index=0)
    assert e.queue_expired.tolist() == [0, n // 2] and e.queue_front.tolist() == [3, -1]
    model = M.expire_records(journal.cpu().numpy(), keys, ttl, now=5100, lease_id=7,
                             first_seq=n + 3)
    assert np.array_equal(e.journal_dst.cpu().numpy(), model.journal)
    # replication of what was appended, and a replica that applies it
    p = pack_storage_events(e.journal_dst, data, journal_pos=JH + 60 * (n + 2), data_file_pos=40,
                            partition_id=2)
    assert p.result["n_msgs"] == n // 2 and p.result["n_data"] == 0
    replica = apply_events(p.events, p.event_offsets, partition_id=2,
                           journal_pos=JH + 60 * (n + 2), data_file_pos=40 + data.numel(),
                           lease_id=7, seq=n + 2)
    assert torch.equal(replica.journal, e.journal_dst)
    # recovery over the grown run selects what expire_records says is left
    w.seq = e.result["next_seq"] - 1
    w.sync_point()
    sync = _t(cuda, np.frombuffer(w.recs[-1], np.uint8).copy(), np.uint8)
    journal = torch.cat([journal, replica.journal, sync])
    n_records = journal.numel() // 60
    select, sel = select_records(journal, data_file_bytes=40 + data.numel())
    assert sel["recovery_rc"] == 0 and sel["n_selected"] == n // 2 and sel["n_deleted"] == n // 2
    assert torch.equal(select[:n + 2], e.select_out) and not select[n + 2:].any()
    r = rollover_records(journal, data, data_file_pos=40, new_data_file_pos=40, keep=select,
                         sync_point=n_records - 1, timestamp=99)
    assert r.result["n_messages"] == n // 2
    push = pack_push_events(r.journal_dst, r.dst, data_file_pos=40,
                            records=_t(cuda, np.arange(n // 2, dtype=np.uint32), np.uint32),
                            queue_ids=_t(cuda, np.full(n // 2, 3), np.int32))
    assert push.result["n_bad"] == 0
    delivered = [m["guid"] for m in PushMessageIterator(push.events.cpu().numpy())]
    assert delivered == [guids[i].tobytes() for i in range(n) if not short[i]]
