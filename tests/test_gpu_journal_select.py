"""Recovery's selection on the GPU (bmqcrc_journal_select, ABI 2.14): the record
run of every partition of journal_select_cases goes to the device, and what
comes back is held to the native host walk (selected records, recovery_rc,
offending record) and to the order-free model (first_record and the three
counts).  Then the shapes the kernels care about, the refusal, the composition
with unpack_records, and the call's state."""
import functools

import numpy as np
import pytest

from blazingmq_amd import (BmqCrcError, Crc32c, _native as N, last_copy, last_journal_select,
                           last_launch, last_put_pack, last_put_unpack, last_records_pack,
                           last_records_unpack, pack_events, pack_records, select_records, synth,
                           unpack_events, unpack_records)
from blazingmq_amd import storage as S
import join_collisions as J
import journal_select_cases as C
import journal_select_model as M
import put_pack_model as P
import put_unpack_model as PU
from records_pack_model import wrap_partition
from test_recovery_selection import Q1, Q2, Q3, rich_partition

pytestmark = pytest.mark.gpu

SLACK = 64   # bytes kept behind every input buffer
KEY = b"\x11\x22\x33\x44\x55"


def _dev(cuda, buf):
    """`buf` on the device as a view of a longer allocation."""
    import torch
    buf = np.array(buf, dtype=np.uint8)
    back = torch.full((buf.size + SLACK,), 0xEE, dtype=torch.uint8, device=cuda)
    back[:buf.size] = torch.from_numpy(buf).to(cuda)
    return back[:buf.size]


def _t(cuda, a, dtype):
    import torch
    a = np.ascontiguousarray(a, dtype=dtype)
    return torch.from_numpy(a.view(np.int32) if dtype == np.uint32 else a).to(cuda)


def _hold(cuda, j, d, csl=False, keys=(), model=True, **kw):
    """select_records over the files' record run == the native walk (and the
    model); returns (select on the host, result)."""
    run, _ = M.record_run(j)
    n = len(run) // 60
    sel, rc, err = M.host_view(j, d, with_csl=csl, queue_keys=keys)
    select, res = select_records(_dev(cuda, run), data_file_bytes=d.size, with_csl=csl,
                                 queue_keys=keys, **kw)
    select = select.cpu().numpy()
    assert select.dtype == np.uint8 and select.size == n and set(np.unique(select)) <= {0, 1}
    assert np.flatnonzero(select).tolist() == sel
    assert (res["recovery_rc"], res["error_record"]) == (rc, err)
    assert (res["n_records"], res["n_selected"], res["refused_kind"]) == (n, len(sel), 0)
    assert not select[:res["first_record"]].any()
    if model:
        m = M.select_model(run, d.size, with_csl=csl, queue_keys=keys)
        assert np.array_equal(select, m["select"])
        assert {k: res[k] for k in ("first_record", "n_selected", "n_deleted", "n_purged")} == \
            {k: m[k] for k in ("first_record", "n_selected", "n_deleted", "n_purged")}
    return select, res


@pytest.mark.parametrize("name", C.ALL)
def test_device_equals_the_host_walk(cuda, name):
    j, d, csl, keys = C.case(name)
    _hold(cuda, j, d, csl, keys)


@functools.lru_cache(maxsize=None)
def _long_run():
    return C.random_files(3, steps=3400, safe=True)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, None])
def test_wave_and_block_edges(cuda, n):
    """Prefixes of one long run (about 3,000 records: three blocks, the last
    partial, DELETIONs whose MESSAGEs lie in other blocks)."""
    j, d, keep = _long_run()
    if n is not None:
        j = j[:44 + 60 * n]
    _, res = _hold(cuda, j, d)
    if n is None:
        assert res["n_records"] > 3000 and res["recovery_rc"] == 0
        assert res["n_selected"] > 1000 and res["n_deleted"] > 200 and res["n_purged"] > 100
        _hold(cuda, j, d, True, tuple(keep))


def test_the_unsafe_long_run_fails_where_the_host_walk_fails(cuda):
    j, d, _ = C.random_files(5, steps=3400)
    _hold(cuda, j, d)


@functools.lru_cache(maxsize=None)
def _big():
    """More records than one tile per block of the 256-block grid (262,144 +
    1,024): every second message deleted, all DELETIONs behind the messages."""
    j, d, _, _ = synth.partition(270000, 0)
    return synth.append_deletions(j), d


def test_more_than_one_tile_per_block(cuda):
    j, d = _big()
    run, _ = M.record_run(j)
    assert len(run) // 60 == 1 + 270000 + 135000 > 262144 + 1024
    select, res = _hold(cuda, j, d, model=False)
    assert (res["n_selected"], res["n_deleted"], res["n_purged"]) == (135000, 135000, 0)
    assert res["first_record"] == 0 and res["recovery_rc"] == 0
    # every second message, from the second on
    assert np.array_equal(np.flatnonzero(select), np.arange(2, 270001, 2))
    # a failure in the lowest block reaches a result that 255 blocks above built
    j = j.copy()
    j[44 + 60 * 700 + 36:44 + 60 * 700 + 52] = 0     # an unset GUID
    select, res = _hold(cuda, j, d, model=False)
    assert (res["recovery_rc"], res["error_record"], res["first_record"]) == \
        (S.RC_INVALID_MESSAGE_RECORD, 700, 701)


def test_queue_cap_counts_distinct_keys(cuda):
    import torch
    j, d = rich_partition()[:2]          # QueueOp records of Q1, Q2 and Q3
    run = _dev(cuda, M.record_run(j)[0])
    other = b"\x61\x62\x63\x64\x65"
    for csl, keys, distinct in ((False, (), 3), (True, (Q1, Q2, Q3), 3), (True, (Q1, other), 4)):
        kw = dict(data_file_bytes=d.size, with_csl=csl, queue_keys=keys)
        with pytest.raises(BmqCrcError) as e:
            select_records(run, queue_cap=distinct - 1, **kw)
        assert e.value.rc == N.BMQCRC_EINVAL and "queue_cap" in str(e.value)
        assert "BMQCRC_JSEL_TOO_MANY_QUEUES" in str(e.value)
        res = last_journal_select(cuda.index, torch.cuda.current_stream(cuda))
        n = run.numel() // 60
        assert res == dict(n_records=n, first_record=n, n_selected=0, n_deleted=0, n_purged=0,
                           error_record=n, recovery_rc=0, refused_kind=1)
        # asynchronously: no error, select all zero, the refusal in the result
        select = select_records(run, queue_cap=distinct - 1, sync=False, **kw)
        assert last_journal_select(cuda.index, torch.cuda.current_stream(cuda)) == res
        assert not select.any().item()
        select, res = select_records(run, queue_cap=distinct, **kw)
        assert res["refused_kind"] == 0
    _hold(cuda, j, d, queue_cap=3)
    _hold(cuda, j, d, queue_cap=1 << 40)


# ---- keys chosen to collide in the two tables (join_collisions.py) ------------

def _same(a, b):
    return a[1] == b[1] and np.array_equal(a[0], b[0])


def _all_three(res):
    return res["recovery_rc"] == 0 and min(res["n_selected"], res["n_deleted"],
                                            res["n_purged"]) > 0


def test_many_queues_with_one_home(cuda):
    """300 queue keys (every byte 0x80 or more) whose home is four slots before
    the end of the 1,024 slots a queue_cap of 300 gives: one block's threads
    publish one chain of 300 at once.  Queue DELETIONs with a re-CREATION,
    PURGEs, an ADDITION and deleted messages among them.  Twice: equal."""
    j, d, keys, _, _ = J.select_queues(True)
    first = _hold(cuda, j, d, queue_cap=J.QUEUES)
    assert _all_three(first[1])
    assert _same(first, _hold(cuda, j, d, queue_cap=J.QUEUES))


def test_many_queues_with_one_home_under_csl(cuda):
    """The same keys without the queue DELETIONs, which the reference fails
    under CSL: without CSL, with all 300 keys as queue_keys, with one of them
    withheld (its CREATION is the host walk's failing record)."""
    j, d, keys, _, _ = J.select_queues(False)
    assert _all_three(_hold(cuda, j, d, queue_cap=J.QUEUES)[1])
    assert _all_three(_hold(cuda, j, d, True, keys, queue_cap=J.QUEUES)[1])
    short = keys[:J.WITHHELD] + keys[J.WITHHELD + 1:]
    _, res = _hold(cuda, j, d, True, short, queue_cap=J.QUEUES)
    assert res["recovery_rc"] == S.RC_INVALID_QUEUE_KEY and res["n_selected"] == 0


@pytest.mark.parametrize("deletions", [True, False], ids=["queue_deletions", "csl"])
def test_queue_cap_one_below_the_colliding_keys(cuda, deletions):
    import torch
    j, d, keys, _, _ = J.select_queues(deletions)
    run = _dev(cuda, M.record_run(j)[0])
    n = run.numel() // 60
    kw = dict(data_file_bytes=d.size, with_csl=not deletions, queue_keys=() if deletions else keys)
    with pytest.raises(BmqCrcError) as e:
        select_records(run, queue_cap=J.QUEUES - 1, **kw)
    assert e.value.rc == N.BMQCRC_EINVAL and "queue_cap" in str(e.value)
    assert "BMQCRC_JSEL_TOO_MANY_QUEUES" in str(e.value)
    res = last_journal_select(cuda.index, torch.cuda.current_stream(cuda))
    assert res == dict(n_records=n, first_record=n, n_selected=0, n_deleted=0, n_purged=0,
                       error_record=n, recovery_rc=0, refused_kind=1)


def test_deletions_in_one_guid_chain(cuda):
    """300 DELETION records in one chain across the end of the GUID table's
    2,048 slots, the MESSAGE records they name walking it: two DELETIONs of one
    GUID, a DELETION below its MESSAGE, one of no message, one GUID under two
    MESSAGE records, and 30 undeleted messages that walk to the empty slot from
    the chain's start and from mid-chain.  Twice: equal."""
    j, d, _, _, _, _, want = J.select_guid_chain()
    first = _hold(cuda, j, d)
    assert first[1]["recovery_rc"] == 0 and {k: first[1][k] for k in want} == want
    assert _same(first, _hold(cuda, j, d))


def test_empty_run(cuda):
    import torch
    run = torch.empty(0, dtype=torch.uint8, device=cuda)
    select, res = select_records(run, data_file_bytes=40)
    assert select.numel() == 0
    assert res == dict(n_records=0, first_record=0, n_selected=0, n_deleted=0, n_purged=0,
                       error_record=0, recovery_rc=0, refused_kind=0)


def test_queue_keys_as_a_device_tensor(cuda):
    j, d, csl, keys = C.case("random:2:csl")
    run = _dev(cuda, M.record_run(j)[0])
    a, ra = select_records(run, data_file_bytes=d.size, with_csl=True, queue_keys=keys)
    flat = _t(cuda, np.frombuffer(b"".join(keys), np.uint8).copy(), np.uint8)
    b, rb = select_records(run, data_file_bytes=d.size, with_csl=True, queue_keys=flat)
    assert ra == rb and (a == b).all().item()
    # without CSL the keys are not looked at
    c, rc = select_records(run, data_file_bytes=d.size, queue_keys=flat)
    assert rc == select_records(run, data_file_bytes=d.size)[1]


def test_deterministic(cuda):
    j, d, _ = _long_run()
    run = _dev(cuda, M.record_run(j)[0])
    first = select_records(run, data_file_bytes=d.size)
    for _ in range(3):
        again = select_records(run, data_file_bytes=d.size)
        assert again[1] == first[1] and (again[0] == first[0]).all().item()


# ---- composition --------------------------------------------------------------

def test_select_then_unpack_recovers_the_rich_partition(cuda):
    """Every skipped payload of rich_partition is corrupted and one skipped
    DataHeader malformed: the unpack over the selection sees none of them."""
    j, d = rich_partition()[:2]
    run, start = M.record_run(j)
    nat = S.scan_partition(j, d)
    d_run, d_data = _dev(cuda, run), _dev(cuda, d)
    select, res = select_records(d_run, data_file_bytes=d.size)
    first = res["first_record"]
    u = unpack_records(d_run[60 * first:], d_data, data_file_pos=0, select=select[first:],
                       msg_cap=res["n_selected"], verify=True)
    import torch
    out = last_records_unpack(cuda.index, torch.cuda.current_stream(cuda))
    assert (out["n_msgs"], out["n_bad"], out["refused_kind"]) == (nat["record_offset"].size, 0, 0)
    assert out["n_skipped"] == res["n_deleted"] + res["n_purged"]
    order = np.argsort(-(u.record_index.cpu().numpy() + first))      # the walk's backward order
    assert ((u.record_index.cpu().numpy() + first)[order] * 60 + start).tolist() == \
        nat["record_offset"].tolist()
    assert u.app_offsets.cpu().numpy()[order].tolist() == nat["app_offset"].tolist()
    assert u.lengths.cpu().numpy()[order].tolist() == nat["app_length"].tolist()
    assert u.crcs.cpu().numpy().view(np.uint32)[order].tolist() == nat["crc32c"].tolist()
    # without the selection the same unpack meets what was skipped
    try:
        unpack_records(d_run[60 * first:], d_data, data_file_pos=0, verify=True)
        bad = last_records_unpack(cuda.index, torch.cuda.current_stream(cuda))["n_bad"]
    except BmqCrcError as e:
        assert "BMQCRC_REC_UNPACK_DATA_RECORD" in str(e)
        bad = -1
    assert bad != 0


def test_put_events_to_a_partition_selected_and_verified_on_the_device(cuda):
    """unpack_events -> pack_records -> DELETION records appended on the device
    -> select_records -> unpack_records == verify_partition on the downloaded
    files."""
    import torch
    rng = np.random.default_rng(48)
    n = 300
    buf, evoffs = PU.concat([PU.build_event(rng, rng.integers(1, 120, size=100))
                             for _ in range(3)])
    pm = PU.model(buf, evoffs)
    gone = np.arange(0, n, 3)                       # consumed: every third message
    kept_victim, gone_victim = 100, 99
    ev = buf.copy()
    ev[int(pm["app_offsets"][kept_victim])] ^= 0x40   # an outstanding payload: an alarm
    ev[int(pm["app_offsets"][gone_victim])] ^= 0x40   # a consumed one: never read
    events = _dev(cuda, ev)
    u = unpack_events(events, _t(cuda, evoffs, np.int64), msg_cap=n)
    qkeys = torch.from_numpy(np.frombuffer(KEY, np.uint8).copy()).to(cuda).repeat(n, 1)
    jour = torch.zeros(60 * (n + gone.size), dtype=torch.uint8, device=cuda)
    dst, _, _, _, _ = pack_records(events, u.app_offsets, u.lengths, qkeys, u.guids,
                                   expected=u.expected, journal_dst=jour, file_key=KEY,
                                   lease_id=1, first_seq=2, data_file_pos=40,
                                   timestamp=0x6720EAB4)
    # the DELETION records: headers from the host, GUIDs from the device
    w = S.PartitionWriter(lease_id=1)
    w.seq = 1 + n
    for _ in gone:
        w.deletion(bytes(16), KEY)
    dels = torch.from_numpy(np.frombuffer(b"".join(w.recs), np.uint8).copy()).to(cuda)
    dels = dels.reshape(gone.size, 60)
    dels[:, 28:44] = u.guids.reshape(-1, 16)[torch.from_numpy(gone).to(cuda)]
    jour[60 * n:] = dels.reshape(-1)
    size = 40 + dst.numel()
    select, res = select_records(jour, data_file_bytes=size, with_csl=True, queue_keys=[KEY])
    assert (res["recovery_rc"], res["first_record"], res["n_selected"], res["n_deleted"]) == \
        (0, 0, n - gone.size, gone.size)
    r = unpack_records(jour, dst, data_file_pos=40, select=select, msg_cap=res["n_selected"])
    out = last_records_unpack(cuda.index, torch.cuda.current_stream(cuda))
    jf, df = wrap_partition(dst.cpu().numpy(), jour.cpu().numpy(), np.frombuffer(KEY, np.uint8))
    got = S.verify_partition(jf, df)
    assert (got["recovery_rc"], got["n_messages"], got["n_bad"]) == (0, out["n_msgs"], 1)
    assert out["n_bad"] == 1
    index = int(r.record_index[out["first_bad"]].item())
    assert index == kept_victim and list(got["bad_record_offsets"]) == [44 + 60 * (1 + index)]


# ---- the call's state ---------------------------------------------------------

def _side_stream(cuda):
    import torch
    return torch.cuda.Stream(cuda, priority=-1)


def test_async_and_last_journal_select(cuda):
    import torch
    j, d, csl, keys = C.case("rich")
    run = _dev(cuda, M.record_run(j)[0])
    s = _side_stream(cuda)
    with torch.cuda.stream(s):
        assert last_journal_select(cuda.index, s) == N.JournalSelectResult().as_dict()
        want_sel, want = select_records(run, data_file_bytes=d.size, stream=s)
        got_sel = select_records(run, data_file_bytes=d.size, stream=s, sync=False)
        assert isinstance(got_sel, torch.Tensor)
        assert last_journal_select(cuda.index, s) == want
        assert (got_sel == want_sel).all().item()
    # a failing journal is a result, not an error, in both forms
    j, d, csl, keys = C.case("fail:unset_guid_confirm")
    run = _dev(cuda, M.record_run(j)[0])
    with torch.cuda.stream(s):
        select_records(run, data_file_bytes=d.size, stream=s, sync=False)
        res = last_journal_select(cuda.index, s)
    assert (res["recovery_rc"], res["error_record"], res["first_record"]) == \
        (S.RC_INVALID_CONFIRM_RECORD, 2, 3)


def test_two_streams_give_independent_results(cuda):
    import torch
    ja, da, _, _ = C.case("rich")
    jb, db, _, _ = C.case("fail:seq_gap")
    ra, rb = _dev(cuda, M.record_run(ja)[0]), _dev(cuda, M.record_run(jb)[0])
    sa, sb = _side_stream(cuda), _side_stream(cuda)
    a = select_records(ra, data_file_bytes=da.size, stream=sa, sync=False)
    b = select_records(rb, data_file_bytes=db.size, stream=sb, sync=False)
    res_b, res_a = last_journal_select(cuda.index, sb), last_journal_select(cuda.index, sa)
    assert res_a["n_records"] == ra.numel() // 60 and res_a["recovery_rc"] == 0
    assert res_b["n_records"] == rb.numel() // 60
    assert res_b["recovery_rc"] == S.RC_INVALID_SEQ_NUMBER
    assert np.flatnonzero(a.cpu().numpy()).tolist() == M.host_view(ja, da)[0]
    assert np.flatnonzero(b.cpu().numpy()).tolist() == M.host_view(jb, db)[0]
    cur = torch.cuda.current_stream(cuda)
    assert cur not in (sa, sb)


def test_state(cuda):
    """Every other bmqcrc_last_* and the shape prediction are as they were."""
    import torch
    rng = np.random.default_rng(49)
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
    j, d = rich_partition()[:2]
    run, data = _dev(cuda, M.record_run(j)[0]), _dev(cuda, d)
    s = _side_stream(cuda)
    with torch.cuda.stream(s):
        Crc32c.copy_batch(arena, d_off[:40], d_len[:40], copy_dst, doff, stream=s)
        pack_events(arena, d_off[:30], d_len[:30], _t(cuda, qids, np.int32),
                    _t(cuda, guids, np.uint8), _t(cuda, flags, np.uint8), stream=s)
        pack_records(arena, d_off[:30], d_len[:30],
                     _t(cuda, np.full((30, 5), 7), np.uint8), _t(cuda, guids, np.uint8),
                     file_key=KEY, lease_id=3, first_seq=2, data_file_pos=40, stream=s)
        unpack_events(_dev(cuda, buf), _t(cuda, evoffs, np.int64), stream=s)
        Crc32c.calculate_batch(arena, d_off, d_len, stream=s)
        before = (last_copy(cuda.index, s), last_put_pack(cuda.index, s),
                  last_records_pack(cuda.index, s), last_put_unpack(cuda.index, s),
                  last_records_unpack(cuda.index, s), last_launch(cuda.index, s, offsets=True))
        select, res = select_records(run, data_file_bytes=d.size, stream=s)
        select_records(run, data_file_bytes=d.size, stream=s, sync=False)
        assert last_journal_select(cuda.index, s) == res
        after = (last_copy(cuda.index, s), last_put_pack(cuda.index, s),
                 last_records_pack(cuda.index, s), last_put_unpack(cuda.index, s),
                 last_records_unpack(cuda.index, s), last_launch(cuda.index, s, offsets=True))
        assert after == before
        out = Crc32c.calculate_batch(arena, d_off, d_len, stream=s)
        # and a records unpack after it leaves the select's record alone
        unpack_records(run, data, data_file_pos=0, select=select, stream=s)
        assert last_journal_select(cuda.index, s) == res
    s.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), P.host_crcs(host, offs, lens))
    assert torch.cuda.current_device() == cuda.index
