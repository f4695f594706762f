"""tests/pending_list_model.py held to the reference's own two iterator cases
(mqbs_filebackedstorage.t.cpp, "Iterator- No virtual storages Test" and
"Iterator Test- In presence of Virtual") and to hand-made journals, and
tests/pending_list_cases.py held to PartitionWriter (no GPU needed)."""
import numpy as np
import pytest

from blazingmq_amd import storage as S
import pending_list_cases as C
import pending_list_model as M

JH = S.PartitionWriter.JOURNAL_HEADER
QK, QK2, QK3 = b"\x26\xda\xcd\xc9\x74", b"\x01\x02\x03\x04\x05", b"\x09\x09\x09\x09\x09"
APP1, APP2, APP3 = b"\xA1" * 5, b"\xA2" * 5, b"\xA3" * 5
NULL = bytes(5)


def _run(w):
    return w.files()[0][JH:]


def _table(queues):
    """[(queue key, [(app key, queue id, sub id), ...]), ...] as the call's arrays."""
    first, apps = [0], []
    for _, mine in queues:
        apps += mine
        first.append(len(apps))
    return (np.frombuffer(b"".join(k for k, _ in queues), np.uint8),
            np.array(first, np.uint64), np.frombuffer(b"".join(a[0] for a in apps), np.uint8),
            np.array([a[1] for a in apps], np.int32)), np.array([a[2] for a in apps], np.uint32)


def _lists(got):
    first = got.list_first.astype(np.int64).tolist()
    return [got.records[first[a]:first[a + 1]].tolist() for a in range(len(first) - 1)]


def test_reference_case_1_no_virtual_storages():
    w = S.PartitionWriter(lease_id=3)
    w.queue_op(S.OP_CREATION, QK)
    recs = [(w.message(bytes([i]), QK)[0] - JH) // 60 for i in range(10)]
    table, subs = _table([(QK, [(NULL, 11, 0)])])
    got = M.pending_records(_run(w), *table, sub_ids=subs)
    assert _lists(got) == [recs] and got.queue_ids.tolist() == [11] * 10
    assert got.app_next.tolist() == [11] and got.app_pending.tolist() == [10]
    # "Check Iterator from specific point": from guids[5] on
    got = M.pending_records(_run(w), *table, from_record=[recs[5]])
    assert _lists(got) == [recs[5:]] and got.result["n_pending"] == 5
    assert got.pending_mask.tolist() == [0] * 6 + [1] * 5


def test_reference_case_2_with_virtual_storages():
    w = S.PartitionWriter(lease_id=3)
    w.queue_op(S.OP_CREATION, QK)
    msgs = [w.message(bytes([i]), QK, ref_count=2) for i in range(60)]
    recs = [(off - JH) // 60 for off, _ in msgs]
    for _, guid in msgs[20:40]:
        w.confirm(guid, QK, APP1)
    table, subs = _table([(QK, [(NULL, 5, 0), (APP1, 5, 1), (APP2, 5, 2)])])
    got = M.pending_records(_run(w), *table, sub_ids=subs)
    assert _lists(got) == [recs, recs[:20] + recs[40:], recs]
    assert got.sub_ids.tolist() == [0] * 60 + [1] * 40 + [2] * 60
    assert got.result == dict(n_records=81, n_live=60, n_no_queue=0, n_pending=160, n_listed=160,
                              n_unknown_confirms=0, n_not_found=0, refused_kind=0,
                              refused_index=0)
    assert [int(got.pending_mask[r]) for r in (recs[0], recs[20], recs[59])] == [7, 5, 7]


def _hand_made():
    """Three queues (the second without an app) and a message of a fourth."""
    w = S.PartitionWriter(lease_id=3)
    g = {}
    w.confirm((0x40 << 120 | 1).to_bytes(16, "big"), QK, APP1, reason=2)   # 0: before its message
    g["a"] = w.message(b"a", QK, ref_count=2)[1]                           # 1: auto-confirmed
    g["b"] = w.message(b"b", QK, ref_count=2)[1]                           # 2
    g["c"] = w.message(b"c", QK, ref_count=2)[1]                           # 3
    w.message(b"x", QK2)                                                   # 4: a queue with no app
    w.message(b"y", QK3)                                                   # 5: a message with no queue
    w.confirm(g["b"], QK, NULL)                                            # 6: marks nothing
    w.confirm(g["b"], QK, APP3)                                            # 7: unknown app key
    w.confirm(b"\x77" * 16, QK, APP1)                                      # 8: no such message
    g["d"] = w.message(b"d", QK, ref_count=2)[1]                           # 9
    w.deletion(g["c"], QK)                                                 # 10
    w.confirm(g["c"], QK, APP2)                                            # 11: behind the DELETION
    g["e"] = w.message(b"e", QK, ref_count=2)[1]                           # 12
    table, subs = _table([(QK, [(APP1, 1, 10), (APP2, 2, 20)]), (QK2, [])])
    return _run(w), table, subs


def test_hand_made_confirms_deletion_and_counts():
    run, table, subs = _hand_made()
    got = M.pending_records(run, *table, sub_ids=subs)
    assert _lists(got) == [[2, 9, 12], [1, 2, 9, 12]]
    assert got.result == dict(n_records=13, n_live=6, n_no_queue=1, n_pending=7, n_listed=7,
                              n_unknown_confirms=1, n_not_found=1, refused_kind=0,
                              refused_index=0)
    assert got.pending_mask.tolist() == [0, 2, 3, 0, 0, 0, 0, 0, 0, 3, 0, 0, 3]
    assert got.app_next.tolist() == [13, 13] and got.list_first.tolist() == [0, 3, 7]


@pytest.mark.parametrize("limit,lists,nexts", [
    ([0, 0], [[], []], [2, 1]),
    ([3, 4], [[2, 9, 12], [1, 2, 9, 12]], [13, 13]),          # equal to |list|
    ([2, 3], [[2, 9], [1, 2, 9]], [12, 12]),                  # one less
])
def test_hand_made_limits(limit, lists, nexts):
    run, table, subs = _hand_made()
    got = M.pending_records(run, *table, limit=limit)
    assert _lists(got) == lists and got.app_next.tolist() == nexts
    assert got.app_pending.tolist() == [3, 4] and got.result["n_pending"] == 7
    assert got.result["n_listed"] == sum(map(len, lists)) and got.sub_ids is None


def test_hand_made_cursors_and_the_size_check():
    run, table, subs = _hand_made()
    got = M.pending_records(run, *table, from_record=[13, 3])     # from_record == n_records
    assert _lists(got) == [[], [9, 12]] and got.pending_mask.tolist()[9] == 2
    assert M.pending_records(run, *table, from_record=[14, 0]) == M.Refusal(M.FROM_RECORD, 0)
    assert M.pending_records(run, *table, list_cap=6) == M.Refusal(M.LIST_TOO_SMALL, 1)
    assert M.pending_records(run, *table, list_cap=2) == M.Refusal(M.LIST_TOO_SMALL, 0)
    assert isinstance(M.pending_records(run, *table, list_cap=7), M.Pending)
    assert isinstance(M.pending_records(run, *table, list_cap=0, limit=[0, 0]), M.Pending)


def test_table_refusals_and_their_order():
    run, (qk, first, ak, ids), _ = _hand_made()
    two = np.frombuffer(QK + QK, np.uint8)
    assert M.pending_records(run, two, first, ak, ids) == M.Refusal(M.QUEUE_KEY, 0)
    assert M.pending_records(run, np.frombuffer(QK + NULL, np.uint8), first, ak, ids) == \
        M.Refusal(M.QUEUE_KEY, 1)
    for bad, index in (([1, 2, 2], 0), ([0, 3, 2], 1), ([0, 2, 3], 2), ([0, 0, 1], 2)):
        assert M.pending_records(run, qk, np.array(bad, np.uint64), ak, ids) == \
            M.Refusal(M.APP_FIRST, index), bad
    same = np.frombuffer(APP1 + APP1, np.uint8)
    assert M.pending_records(run, qk, first, same, ids) == M.Refusal(M.APP_KEY, 0)
    nulls = np.frombuffer(NULL + NULL, np.uint8)
    assert M.pending_records(run, qk, first, nulls, ids) == M.Refusal(M.APP_KEY, 0)
    # the lowest kind wins: a repeated queue key before a repeated app key
    assert M.pending_records(run, two, first, same, ids) == M.Refusal(M.QUEUE_KEY, 0)
    # 33 apps in one queue
    keys = np.zeros((33, 5), np.uint8)
    keys[:, 0] = np.arange(1, 34)
    big = M.pending_records(run, qk, np.array([0, 33, 33], np.uint64), keys.reshape(-1),
                            np.zeros(33, np.int32))
    assert big == M.Refusal(M.APP_FIRST, 0)
    broken = run.copy()
    broken[60 * 4 + 56] ^= 1
    assert M.pending_records(broken, two, first, same, ids) == M.Refusal(M.RECORD_HEADER, 4)
    twice = np.concatenate([run, run[60:120]])
    assert M.pending_records(twice, qk, first, ak, ids) == M.Refusal(M.DUPLICATE_MESSAGE, 1)


def test_an_empty_run_and_an_empty_table():
    got = M.pending_records(np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(1, np.uint64),
                            np.zeros(0, np.uint8), np.zeros(0, np.int32))
    assert got.records.size == 0 and got.list_first is None and got.result["n_records"] == 0
    run, _, _ = _hand_made()
    got = M.pending_records(run, np.zeros(0, np.uint8), np.zeros(1, np.uint64),
                            np.zeros(0, np.uint8), np.zeros(0, np.int32))
    assert got.result["n_live"] == got.result["n_no_queue"] == 6
    assert got.list_first.tolist() == [0] and got.result["n_unknown_confirms"] == 3


def test_the_numpy_runs_are_partition_writers_bytes():
    w = S.PartitionWriter(lease_id=7)
    _, g1 = w.message(b"", QK)
    w.confirm(g1, QK, APP1, reason=2)
    w.deletion(g1, QK)
    w.queue_op(S.OP_ADDITION, QK2)
    run = C.records([C.MESSAGE, C.CONFIRM, C.DELETION, C.QUEUE_OP],
                    np.frombuffer(QK + QK + QK + QK2, np.uint8),
                    C.guids([1, 1, 1, 0]), np.frombuffer(NULL + APP1 + NULL + NULL, np.uint8),
                    flags=[0, 2, 0, 0]).reshape(4, 60)
    want = _run(w).reshape(4, 60).copy()
    # what the numpy rows leave out: the DATA offset and CRC of a MESSAGE record,
    # the QLIST offset of a QUEUE_OP record
    want[0, 32:36], want[0, 52:56], want[3, 36:40] = 0, 0, 0
    assert run.tobytes() == want.tobytes()


@pytest.mark.parametrize("seed", range(4))
def test_random_scenarios_are_valid_and_exercise_every_count(seed):
    c = C.scenario(seed, 3000, [3, 0, 32, 1, 2, 5])
    args, kw = C.model_args(c)
    got = M.pending_records(*args, **kw)
    assert isinstance(got, M.Pending)
    r = got.result
    assert r["n_no_queue"] and r["n_unknown_confirms"] and r["n_not_found"]
    assert 0 < r["n_listed"] < r["n_pending"] and r["n_live"] < int(c.select.sum())
    assert int(got.pending_mask.max()) >> 31 == 1           # the 32nd app of the third queue
    assert (got.app_pending == 0).any() and (got.app_next < 3000).any()
    # every list is in journal order and names live messages of its queue only
    first = got.list_first.astype(np.int64)
    for a in range(first.size - 1):
        mine = got.records[first[a]:first[a + 1]].astype(np.int64)
        assert (np.diff(mine) > 0).all()
        assert (mine >= int(c.from_record[a])).all() and mine.size <= int(c.limit[a])
