"""bmqcrc_pending_records_list (ABI 2.21) on the device against the sequential
model of tests/pending_list_model.py: every output byte, every result field,
every refusal with its precedence, and that a refused or size-only call writes
nothing.  Every buffer of every call lies between sentinel margins
(device_views.py), which are checked after it."""
import ctypes
import functools

import numpy as np
import pytest

from blazingmq_amd import (PushMessageIterator, _native as N, confirm_records, expire_records,
                           last_confirm_records, last_copy, last_expire_records,
                           last_journal_select, last_launch, last_pending_records,
                           last_push_pack, last_put_pack, last_put_unpack, last_records_pack,
                           last_records_unpack, last_rollover, last_storage_apply,
                           last_storage_pack, pack_push_events, pack_records, pending_records)
from blazingmq_amd import Crc32c
from blazingmq_amd.push_event import OPTION_SUB_QUEUE_ID
import device_views as V
import pending_list_cases as C
import pending_list_model as M
import put_pack_model as P
import test_grid_regimes as G
from records_pack_model import random_meta

pytestmark = pytest.mark.gpu

GUARD = 8      # elements behind every output array
KINDS = ("OK", "RECORD_HEADER", "DUPLICATE_MESSAGE", "QUEUE_KEY", "APP_FIRST", "APP_KEY",
         "FROM_RECORD", "LIST_TOO_SMALL")
KIND_NAME = {k: ("BMQCRC_PENDING_LIST_" + n).encode() for k, n in enumerate(KINDS) if k}
# name -> (dtype, canary, counted in: c list_cap, a apps, a1 apps + 1, r records)
OUTPUTS = {"records": (np.uint32, 0xA5A5A5A5, "c"), "out_queue_ids": (np.uint32, 0xB6B6B6B6, "c"),
           "out_sub_ids": (np.uint32, 0xC7C7C7C7, "c"),
           "list_first": (np.uint64, 0xD8D8D8D8D8D8D8D8, "a1"),
           "app_pending": (np.uint32, 0xE9E9E9E9, "a"), "app_next": (np.uint32, 0xFAFAFAFA, "a"),
           "pending_mask": (np.uint32, 0x9C9C9C9C, "r")}
INPUTS = {"journal": np.uint8, "select": np.uint8, "queue_keys": np.uint8, "app_first": np.uint64,
          "app_keys": np.uint8, "queue_ids": np.int32, "sub_ids": np.uint32,
          "from_record": np.uint32, "limit": np.uint32}
ALIGNED = {name: 0 for name in list(INPUTS) + list(OUTPUTS)}
# the smallest alignment the ABI permits: the key tables and select at odd
# addresses, the 32-bit arrays at +4, the 64-bit ones at +8
SMALLEST = dict({name: 4 for name in ALIGNED}, select=1, queue_keys=3, app_keys=1, app_first=8,
                list_first=8)
APPS = [3, 0, 32, 1, 2, 5]      # a queue without an app, one with every bit of the mask


def _side_stream(cuda):
    """A stream of its own from the high-priority pool (the default pool's
    streams carry planner history that tests elsewhere rely on)."""
    import torch
    return torch.cuda.Stream(cuda, priority=-1)


def _t(cuda, a, dtype):
    import torch
    a = np.array(a, dtype=dtype)     # (a copy: shared inputs are read-only)
    a = a.view({np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype, a.dtype))
    return torch.from_numpy(a).to(cuda)


def _raw(cuda, c, list_cap, sync=True, stream=None, skip=(), phases=ALIGNED):
    """One bmqcrc_pending_records_list over the case `c` into canary-filled
    lists of `list_cap` entries (None: a size-only call, records NULL) and
    arrays.  Returns (rc, error text, result of the call or of
    bmqcrc_last_pending_records, everything written on the host with its
    guards)."""
    import torch
    place = V.Placer(cuda, phases)
    stream = stream or torch.cuda.current_stream(cuda)
    n_records, n_queues, n_apps = len(c.run) // 60, len(c.app_first) - 1, len(c.queue_ids)
    count = {"c": list_cap or 0, "a": n_apps, "a1": n_apps + 1, "r": n_records}
    with torch.cuda.stream(stream):
        spare = torch.zeros(8, dtype=torch.int64, device=cuda)
        p = N.PendingList()
        p.struct_size = ctypes.sizeof(N.PendingList)
        given = dict(journal=c.run, select=c.select, queue_keys=c.queue_keys,
                     app_first=c.app_first, app_keys=c.app_keys, queue_ids=c.queue_ids,
                     sub_ids=c.sub_ids, from_record=c.from_record, limit=c.limit)
        for name, value in given.items():
            if value is not None:
                t = place.put(name, np.asarray(value, INPUTS[name]))
                setattr(p, name, t.data_ptr() or spare.data_ptr())
        p.journal_bytes, p.n_records, p.n_queues, p.n_apps = len(c.run), n_records, n_queues, n_apps
        arr = {}
        for name, (dt, value, per) in OUTPUTS.items():
            if name in skip or (name == "out_sub_ids" and c.sub_ids is None):
                continue
            arr[name] = place.fill(name, count[per] + GUARD, dt, value)
            if list_cap is not None or per != "c":
                setattr(p, name, arr[name].data_ptr())
        p.list_cap = list_cap or 0
        o = N.make_opts(device=cuda.index, stream=stream.cuda_stream,
                        flags=N.BMQCRC_F_DEVICE_PTRS | (0 if sync else N.BMQCRC_F_ASYNC))
        r = N.PendingListResult()
        rc = N.lib.bmqcrc_pending_records_list(ctypes.byref(p), ctypes.byref(r), ctypes.byref(o))
        err = N.lib.bmqcrc_last_error()
        res = r.as_dict() if sync else last_pending_records(cuda.index, stream)
        host = {name: t.cpu().numpy().view(OUTPUTS[name][0]) for name, t in arr.items()}
        place.check()
    return rc, err, res, host


def _untouched(name, a):
    return bool((a == OUTPUTS[name][1]).all())


def _model(c, list_cap):
    args, kw = C.model_args(c)
    return M.pending_records(*args, list_cap=list_cap, **kw)


def _check(cuda, c, list_cap="exact", sync=True, stream=None, skip=(), phases=ALIGNED, model=None):
    """The call against the model: a refusal identical and nothing written, or
    every list entry, array entry and result field.  `list_cap` "exact" is what
    the model says the call writes, None a size-only call.  `model` is the
    model's size-only answer when the caller has it already.  Returns (model,
    host)."""
    sized = model if model is not None else _model(c, None)
    if list_cap == "exact":
        list_cap = sized.result["n_listed"] if isinstance(sized, M.Pending) else 10
    m = sized
    if isinstance(sized, M.Pending) and list_cap is not None and \
            list_cap < sized.result["n_listed"]:
        m = _model(c, list_cap)
    rc, err, res, host = _raw(cuda, c, list_cap, sync=sync, stream=stream, skip=skip,
                              phases=phases)
    n_records = len(c.run) // 60
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
    if list_cap is None or n_records == 0:      # size only, or nothing launched
        for name, a in host.items():
            assert _untouched(name, a), name
        return m, host
    for name, want in (("records", m.records), ("out_queue_ids", m.queue_ids.view(np.uint32)),
                       ("out_sub_ids", m.sub_ids), ("list_first", m.list_first),
                       ("app_pending", m.app_pending), ("app_next", m.app_next),
                       ("pending_mask", m.pending_mask)):
        if name not in host:
            continue
        assert np.array_equal(host[name][:len(want)], want), name
        assert _untouched(name, host[name][len(want):]), name
    return m, host


# ---- sizes -------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1025])
def test_run_sizes(cuda, n):
    m, _ = _check(cuda, C.scenario(n, n, APPS))
    if n == 1025:
        assert m.result["n_pending"] > 1024 and int(m.pending_mask.max()) >> 31 == 1
        assert m.result["n_unknown_confirms"] and m.result["n_not_found"]
        assert m.result["n_no_queue"] and 0 < m.result["n_listed"] < m.result["n_pending"]


@functools.lru_cache(maxsize=None)
def _large(n):
    c = C.scenario(77, n, [6, 4, 6])
    return c, _model(c, None)


@pytest.mark.parametrize("n", [G.N_WAVES, G.N_TILES], ids=["N_WAVES", "N_TILES"])
def test_the_cross_wave_block_prefix_and_a_blocks_second_tile(cuda, n):
    # N_WAVES: 66 blocks of records; N_TILES: 129 blocks of two tiles, and more
    # than 262,144 pairs: the sort's blocks hold two tiles too, past 64 of them
    c, m = _large(n)
    assert G.regime(n).cross_wave and (n != G.N_TILES or G.regime(n).per_block == 2048)
    assert m.result["n_pending"] > (262144 if n == G.N_TILES else 65536)
    _check(cuda, c, model=m)


@pytest.mark.parametrize("pairs", [64, 65])
@pytest.mark.parametrize("apps", ["one", "all_different"])
def test_a_wave_of_pairs_with_one_digit_and_with_64(cuda, pairs, apps):
    if apps == "one":
        # every message in the second queue: all lanes of the wave hold app 1
        c = C.messages_only(pairs, [1, 1], which=np.ones(pairs, np.int64))
    else:
        # one message a queue: 32 + 32 (+ 1) apps, every lane another
        c = C.messages_only(2 if pairs == 64 else 3, [32, 32, 1])
    m, _ = _check(cuda, c)
    assert m.result["n_pending"] == pairs
    assert int((m.app_pending > 0).sum()) == (1 if apps == "one" else pairs)


@pytest.mark.parametrize("n_apps", [1, 2, 256, 257])
def test_the_number_of_apps_decides_the_passes(cuda, n_apps):
    counts = {1: [1], 2: [2], 256: [32] * 8, 257: [32] * 8 + [1]}[n_apps]
    c = C.scenario(n_apps, 3000, counts, absent_queue=False, cursors=False)
    assert len(c.queue_ids) == n_apps
    m, _ = _check(cuda, c)
    assert m.result["n_pending"] > 1024
    c = C.messages_only(5 * len(counts), counts)
    m, _ = _check(cuda, c)
    assert (m.app_pending == 5).all()       # the last app too: the digit's first use


@functools.lru_cache(maxsize=None)
def _third_digit():
    # 2,048 queues of 32 apps and one of one: 65,537 apps, three messages a queue
    counts = [32] * 2048 + [1]
    c = C.messages_only(3 * 2049, counts)
    rng = np.random.default_rng(3)
    c = c._replace(limit=rng.integers(0, 5, size=65537).astype(np.uint32),
                   from_record=(rng.integers(0, 2, size=65537) * 2049).astype(np.uint32))
    return c, _model(c, None)


def test_65537_apps_take_a_third_digit(cuda):
    c, m = _third_digit()
    assert len(c.queue_ids) == 65537 and m.app_pending[65536] > 0
    assert m.result["n_pending"] > 65536 + 1024
    _check(cuda, c, model=m)


def test_apps_with_empty_lists_at_the_start_middle_and_end(cuda):
    rng = np.random.default_rng(8)
    queue_keys, app_first, app_keys, queue_ids, sub_ids = C.table(rng, [2, 1, 0, 3, 2, 1])
    which = np.array([1, 4] * 40)                   # messages of the second and fifth queue only
    run = C.records(np.full(80, C.MESSAGE, np.uint8), queue_keys[which],
                    C.guids(np.arange(1, 81)))
    c = C.Case(run, queue_keys.reshape(-1), app_first, app_keys.reshape(-1), queue_ids, sub_ids,
               None, None, None)
    m, _ = _check(cuda, c)
    assert m.app_pending.tolist() == [0, 0, 40, 0, 0, 0, 40, 40, 0]
    assert m.list_first.tolist() == [0, 0, 0, 40, 40, 40, 40, 80, 120, 120]


# ---- refusals ----------------------------------------------------------------

def _base():
    return C.scenario(41, 1500, APPS)


def _planted(kinds):
    """The base case with a violation of every kind in `kinds` planted, two of
    each where an index decides."""
    c = _base()
    run = c.run.copy().reshape(-1, 60)
    qk = c.queue_keys.copy().reshape(-1, 5)
    ak = c.app_keys.copy().reshape(-1, 5)
    first, cursor = c.app_first.copy(), c.from_record.copy()
    msgs = np.flatnonzero((run[:, 0] >> 4 == 1) & (c.select != 0))
    if M.RECORD_HEADER in kinds:
        run[1400, 56] ^= 1
        run[900, 8:12] = 0
    if M.DUPLICATE_MESSAGE in kinds:
        run[msgs[-1]] = run[msgs[5]]
        run[msgs[-2]] = run[msgs[9]]
    if M.QUEUE_KEY in kinds:
        qk[5] = qk[2]
        qk[4] = 0
    if M.APP_FIRST in kinds:
        first[4], first[5] = first[5], first[4]     # queue 3 falls behind queue 4
    if M.APP_KEY in kinds:
        ak[20], ak[30] = ak[10], ak[12]             # apps of the 32-app queue (3 .. 34)
    if M.FROM_RECORD in kinds:
        cursor[40], cursor[17] = 1501, 0xFFFFFFFF
    return c._replace(run=run.reshape(-1), queue_keys=qk.reshape(-1), app_keys=ak.reshape(-1),
                      app_first=first, from_record=cursor)


WANT = {M.RECORD_HEADER: 900, M.QUEUE_KEY: 2, M.APP_KEY: 10, M.FROM_RECORD: 17}


@pytest.mark.parametrize("sync", [True, False], ids=["sync", "async"])
@pytest.mark.parametrize("kind", range(1, 7), ids=KINDS[1:7])
def test_every_refusal_alone_and_under_all_the_higher_kinds(cuda, kind, sync):
    for kinds in ({kind}, set(range(kind, 7))):
        m, _ = _check(cuda, _planted(kinds), sync=sync)
        assert isinstance(m, M.Refusal) and m.kind == kind, (m, kinds)
        assert m.index == WANT.get(kind, m.index)


@pytest.mark.parametrize("sync", [True, False], ids=["sync", "async"])
def test_lists_too_small(cuda, sync):
    c = _base()
    sized = _model(c, None)
    n, first = sized.result["n_listed"], sized.list_first.astype(np.int64)
    m, _ = _check(cuda, c, list_cap=n - 1, sync=sync, model=sized)
    assert m == M.Refusal(M.LIST_TOO_SMALL, int(np.flatnonzero(first[1:] == n)[0]))
    m, _ = _check(cuda, c, list_cap=0, sync=sync, model=sized)
    assert m == M.Refusal(M.LIST_TOO_SMALL, int(np.flatnonzero(first[1:] > 0)[0]))
    _check(cuda, _planted({M.FROM_RECORD}), list_cap=0, sync=sync)      # the lower kind wins


def test_a_queue_with_33_apps_and_the_other_app_first_violations(cuda):
    for counts, broken, index in (([2, 33, 1], None, 1), ([2, 3], [1, 2, 5], 0),
                                  ([2, 3], [0, 2, 4], 2), ([2, 3], [0, 2, 6], 2),
                                  ([2, 3], [0, 6, 5], 1), ([], [1], 0)):
        c = C.messages_only(50, counts or [1])
        if not counts:
            c = c._replace(queue_keys=c.queue_keys[:0], app_keys=c.app_keys[:0],
                           queue_ids=c.queue_ids[:0], sub_ids=c.sub_ids[:0])
        if broken is not None:
            c = c._replace(app_first=np.array(broken, np.uint64))
        m, _ = _check(cuda, c)
        assert m == M.Refusal(M.APP_FIRST, index), (counts, broken, m)


def test_an_empty_table_and_a_table_without_apps(cuda):
    c = C.messages_only(70, [1])
    none = c._replace(queue_keys=c.queue_keys[:0], app_keys=c.app_keys[:0],
                      queue_ids=c.queue_ids[:0], sub_ids=None, app_first=np.zeros(1, np.uint64))
    m, host = _check(cuda, none)
    assert m.result["n_no_queue"] == 70 and host["list_first"][0] == 0
    bare = c._replace(app_keys=c.app_keys[:0], queue_ids=c.queue_ids[:0], sub_ids=None,
                      app_first=np.zeros(2, np.uint64))
    m, _ = _check(cuda, bare)
    assert m.result == dict(n_records=70, n_live=70, n_no_queue=0, n_pending=0, n_listed=0,
                            n_unknown_confirms=0, n_not_found=0, refused_kind=0, refused_index=0)


# ---- the call's modes ----------------------------------------------------------

def test_size_only_then_the_real_call_and_two_calls_give_the_same_bytes(cuda):
    c = C.scenario(9, 5000, APPS)
    sized = _model(c, None)
    _check(cuda, c, list_cap=None, model=sized)
    _check(cuda, c, list_cap=None, sync=False, model=sized)
    _, one = _check(cuda, c, model=sized)
    _, two = _check(cuda, c, model=sized, sync=False)
    assert all(one[name].tobytes() == two[name].tobytes() for name in OUTPUTS)
    _check(cuda, c, list_cap=sized.result["n_listed"] + 100, model=sized)


@pytest.mark.parametrize("skip", ["out_sub_ids", "app_pending", "app_next", "pending_mask", "all"])
def test_each_optional_output_null(cuda, skip):
    c = C.scenario(10, 2000, APPS)
    _check(cuda, c, skip=("out_sub_ids", "app_pending", "app_next", "pending_mask")
           if skip == "all" else (skip,))
    if skip == "all":
        _check(cuda, c._replace(sub_ids=None, from_record=None, limit=None, select=None))


def test_every_base_pointer_at_the_smallest_alignment_the_abi_permits(cuda):
    m, _ = _check(cuda, C.scenario(11, 1025, APPS), phases=SMALLEST)
    assert m.result["n_listed"] > 0
    _check(cuda, _planted({M.APP_KEY}), phases=SMALLEST)    # refused


def test_the_wrapper_sizes_the_lists_and_takes_an_empty_run(cuda):
    import torch
    c = C.scenario(12, 2000, APPS)
    m = _model(c, None)
    dev = dict(sub_ids=_t(cuda, c.sub_ids, np.uint32), from_record=_t(cuda, c.from_record, np.uint32),
               limit=_t(cuda, c.limit, np.uint32), select=_t(cuda, c.select, np.uint8))
    args = (_t(cuda, c.queue_keys, np.uint8), _t(cuda, c.app_first, np.uint64),
            _t(cuda, c.app_keys, np.uint8), _t(cuda, c.queue_ids, np.int32))
    got = pending_records(_t(cuda, c.run, np.uint8), *args, **dev)
    assert got.result == m.result == last_pending_records(cuda.index)
    for name, want in zip(got._fields[:7], m[:7]):
        assert np.array_equal(getattr(got, name).cpu().numpy().view(want.dtype), want), name
    got = pending_records(_t(cuda, c.run, np.uint8), *args, list_cap=m.result["n_listed"] + 5,
                          sync=False, **dev)
    assert got.result is None and got.records.numel() == m.result["n_listed"] + 5
    assert last_pending_records(cuda.index) == m.result
    assert np.array_equal(got.records.cpu().numpy().view(np.uint32)[:-5], m.records)
    with pytest.raises(ValueError, match="list_cap is required"):
        pending_records(_t(cuda, c.run, np.uint8), *args, sync=False)
    with pytest.raises(N.BmqCrcError, match="LIST_TOO_SMALL"):
        pending_records(_t(cuda, c.run, np.uint8), *args, list_cap=3, **dev)
    empty = pending_records(torch.zeros(0, dtype=torch.uint8, device=cuda), *args,
                            **dict(dev, select=None))
    assert empty.records.numel() == 0 and empty.result["n_records"] == 0


def test_state(cuda):
    import torch
    rng = np.random.default_rng(56)
    host = rng.integers(0, 256, size=1 << 18, dtype=np.uint8)
    arena = torch.from_numpy(host).to(cuda)
    lens = rng.integers(1, 1025, size=3001).astype(np.uint32)
    offs = (rng.random(lens.size) * (host.size - 1100)).astype(np.int64)
    d_off, d_len = _t(cuda, offs, np.int64), _t(cuda, lens, np.uint32)
    qkeys, guids = random_meta(rng, 30)
    c = C.scenario(13, 3000, APPS)
    sized = _model(c, None)
    s = _side_stream(cuda)
    from blazingmq_amd import (pack_storage_events, rollover_records, select_records)

    def records():
        return (last_launch(cuda.index, s, offsets=True), last_copy(cuda.index, s),
                last_put_pack(cuda.index, s), last_records_pack(cuda.index, s),
                last_put_unpack(cuda.index, s), last_records_unpack(cuda.index, s),
                last_journal_select(cuda.index, s), last_storage_apply(cuda.index, s),
                last_storage_pack(cuda.index, s), last_push_pack(cuda.index, s),
                last_rollover(cuda.index, s), last_confirm_records(cuda.index, s),
                last_expire_records(cuda.index, s))
    with torch.cuda.stream(s):
        # none yet on s
        assert last_pending_records(cuda.index, s) == M.refused_result(M.Refusal(0, 0), 0)
        Crc32c.calculate_batch(arena, d_off, d_len, stream=s)
        dst, jour, _, _, _ = pack_records(
            arena, d_off[:30], d_len[:30], _t(cuda, qkeys, np.uint8), _t(cuda, guids, np.uint8),
            file_key=b"\x11\x22\x33\x44\x55", lease_id=3, first_seq=2, data_file_pos=40, stream=s)
        select_records(jour, data_file_bytes=40 + dst.numel(), stream=s)
        rollover_records(jour, dst, data_file_pos=40, new_data_file_pos=40, stream=s)
        pack_storage_events(jour, dst, journal_pos=44, data_file_pos=40, partition_id=1, stream=s)
        pack_push_events(jour, dst, data_file_pos=40,
                         queue_ids=_t(cuda, np.arange(30), np.int32), stream=s)
        confirm_records(jour, _t(cuda, guids[:3], np.uint8), _t(cuda, qkeys[:3], np.uint8),
                        lease_id=3, first_seq=40, stream=s)
        expire_records(jour, _t(cuda, qkeys[:1].reshape(-1), np.uint8),
                       _t(cuda, [5], np.uint64), now=1 << 40, lease_id=3, first_seq=50, stream=s)
        before = records()
        _check(cuda, c, stream=s, model=sized)
        _check(cuda, c, stream=s, sync=False, model=sized)
        _check(cuda, c, list_cap=1, stream=s, model=sized)          # a refused one
        _check(cuda, c, list_cap=None, stream=s, model=sized)       # a size-only one
        assert records() == before
        out = Crc32c.calculate_batch(arena, d_off, d_len, stream=s)
    s.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), P.host_crcs(host, offs, lens))


# ---- the pipeline ------------------------------------------------------------

def test_a_fanout_queue_delivered_on_one_device(cuda):
    # pack_records(ref_counts=2) -> pending_records (two apps, a limit) ->
    # pack_push_events fed from its outputs -> confirm_records for app 1 on half
    # of what it got -> pending_records from app_next on -> expire_records ->
    # pending_records with select=select_out.  No index list is built on the
    # host: what the host decides is the consumers' confirms.
    import torch
    rng = np.random.default_rng(21)
    n, lim = 120, 50
    lens = rng.integers(1, 301, size=n).astype(np.uint32)
    soff = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    src = rng.integers(0, 256, size=int(lens.sum()), dtype=np.uint8)
    qkeys, guids = random_meta(rng, n)
    key = b"\x26\xda\xcd\xc9\x74"
    qkeys[:] = np.frombuffer(key, np.uint8)
    app1, app2 = b"\xA1" * 5, b"\xA2" * 5
    data, journal, _, _, _ = pack_records(
        _t(cuda, src, np.uint8), _t(cuda, soff, np.int64), _t(cuda, lens, np.uint32),
        _t(cuda, qkeys, np.uint8), _t(cuda, guids, np.uint8), file_key=b"\x11\x22\x33\x44\x55",
        lease_id=7, first_seq=1, data_file_pos=40, timestamp=5000,
        ref_counts=_t(cuda, np.full(n, 2), np.uint32))
    table = (_t(cuda, np.frombuffer(key, np.uint8), np.uint8), _t(cuda, [0, 2], np.uint64),
             _t(cuda, np.frombuffer(app1 + app2, np.uint8), np.uint8), _t(cuda, [31, 32], np.int32))
    subs = _t(cuda, [501, 502], np.uint32)
    first = pending_records(journal, *table, sub_ids=subs, limit=_t(cuda, [lim, lim], np.uint32))
    assert first.result["n_pending"] == 2 * n and first.result["n_listed"] == 2 * lim
    assert first.app_next.tolist() == [lim, lim] and first.list_first.tolist() == [0, lim, 2 * lim]
    push = pack_push_events(journal, data, data_file_pos=40, records=first.records,
                            queue_ids=first.queue_ids, sub_ids=first.sub_ids,
                            option_mode=OPTION_SUB_QUEUE_ID)
    assert push.result["n_bad"] == 0
    delivered = [m["guid"] for m in PushMessageIterator(push.events.cpu().numpy())]
    assert delivered == [guids[i].tobytes() for i in range(lim)] * 2
    # app 1 confirms every second message it got
    done = np.arange(0, lim, 2)
    cf = confirm_records(journal, _t(cuda, guids[done], np.uint8), _t(cuda, qkeys[done], np.uint8),
                         app_keys=_t(cuda, np.tile(np.frombuffer(app1, np.uint8), done.size),
                                     np.uint8), lease_id=7, first_seq=n + 1)
    assert cf.result["n_written"] == done.size
    journal = torch.cat([journal, cf.journal_dst])
    # ... and both ask again from their cursors on: app 1 gets the rest, app 2 everything
    again = pending_records(journal, *table, sub_ids=subs, from_record=first.app_next)
    assert again.app_pending.tolist() == [n - lim, n - lim]
    assert again.records.tolist() == list(range(lim, n)) * 2
    # without the cursor app 1 still has the unconfirmed half of its first delivery
    whole = pending_records(journal, *table, sub_ids=subs)
    assert whole.records.tolist()[:n - done.size] == \
        [r for r in range(n) if r >= lim or r % 2 == 1]
    assert whole.app_pending.tolist() == [n - done.size, n]
    # the TTL runs out for all of them
    e = expire_records(journal, table[0], _t(cuda, [10], np.uint64), now=6000, lease_id=7,
                       first_seq=n + 1 + done.size)
    assert e.result["n_expired"] == n
    last = pending_records(journal, *table, sub_ids=subs, select=e.select_out)
    assert last.records.numel() == 0 and last.result["n_live"] == 0
    assert last.app_pending.tolist() == [0, 0] and last.list_first.tolist() == [0, 0, 0]
