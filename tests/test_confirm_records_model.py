"""tests/confirm_records_model.py -- the numpy model the GPU tests of
bmqcrc_confirm_records_pack compare with -- against a journal and a batch
spelled out byte by byte, the reference's fixture partition, the native
recovery walk over the extended journal, chained calls and one case per refusal
condition.  No GPU."""
import os

import numpy as np
import pytest

from blazingmq_amd import confirm_records, last_confirm_records  # noqa: F401  (the feature under test)
from blazingmq_amd import storage as S

import confirm_records_cases as C
import confirm_records_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
JH = S.PartitionWriter.JOURNAL_HEADER


def test_every_record_form_byte_by_byte():
    got = M.confirm_records(C.run(), **C.batch(), **C.KW, journal_dst_bytes=240)
    assert isinstance(got, M.Confirmed), got
    assert got.journal.tobytes() == C.expected_bytes().tobytes()
    assert got.status.tolist() == C.EXPECTED_STATUS
    assert got.target.tolist() == C.EXPECTED_TARGET
    assert got.new_index.tolist() == C.EXPECTED_INDEX
    assert got.left_out.tolist() == C.EXPECTED_LEFT
    assert got.result == C.EXPECTED_RESULT
    # size only: the same answer
    sized = M.confirm_records(C.run(), **C.batch(), **C.KW)
    assert sized.result == C.EXPECTED_RESULT


def test_the_records_are_the_writers():
    """PartitionWriter.confirm / .deletion give the same 60 bytes."""
    w = S.PartitionWriter(lease_id=C.LEASE, timestamp=C.TS0)
    w.seq = C.FIRST_SEQ - 1
    w.confirm(C.G1, C.KEY_A, app_key=C.APP, reason=1)
    w.ts = C.TS0 + 2
    w.deletion(C.G0, C.KEY_A)
    assert b"".join(w.recs) == C.expected_bytes()[:120].tobytes()


def test_an_empty_batch():
    got = M.confirm_records(C.run(), np.zeros(0, np.uint8), np.zeros(0, np.uint8), **C.KW)
    assert got.journal.size == 0 and got.result["n_written"] == 0
    assert got.result["next_seq"] == C.FIRST_SEQ


def _pair(guid, key):
    return dict(guids=np.frombuffer(guid, np.uint8), queue_keys=np.frombuffer(key, np.uint8))


def test_auto_confirmed_records_do_not_count():
    """Record 2 has refCount 3, one CONFIRM and one AUTO_CONFIRMED record: two
    confirms are left, not one."""
    both = dict(guids=np.frombuffer(C.G1 * 2, np.uint8), queue_keys=np.frombuffer(C.KEY_A * 2, np.uint8))
    got = M.confirm_records(C.run(), **both, **C.KW)
    assert got.status.tolist() == [0, 1]
    # ... and were the auto-confirm an ordinary one, the second would be one too many
    run = C.run()
    assert run[60 * 4 + 1] == 2
    run[60 * 4 + 1] = 0
    assert M.confirm_records(run, **both, **C.KW) == M.Refusal(M.OVER_CONFIRMED, 0)


def test_a_deletion_below_its_message_counts():
    got = M.confirm_records(C.run(), **_pair(C.G3, C.KEY_B), **C.KW)
    assert got.status.tolist() == [2] and got.result["n_not_found"] == 1
    run = C.run()
    run[60 * 5 + 43] ^= 1   # the DELETION record's GUID: it names nothing now
    got = M.confirm_records(run, **_pair(C.G3, C.KEY_B), **C.KW)
    assert got.status.tolist() == [1] and got.target.tolist() == [7]


def _extended(journal, out):
    return np.concatenate([journal, out])


def test_fixture_partition_both_messages_confirmed_leave_nothing():
    """The reference's partition (bmqstoragetool's two "hello world" messages,
    records 3 and 10, refCount 1 each).  The broker that wrote it had the first
    one confirmed already: records 5 and 6 are its CONFIRM and DELETION.  With
    those two records taken out both messages are live and confirming both
    writes two DELETION records, the first of them the reference's own record 6
    but for sequence number and timestamp (the walk is not asked: the cut
    leaves a gap in the sequence numbers).  On the files as they are the first
    confirm finds nothing, the second writes the one DELETION record, and the
    host walk over the extended journal selects nothing."""
    j = np.fromfile(os.path.join(GOLDEN, "test.bmq_journal"), np.uint8)
    d = np.fromfile(os.path.join(GOLDEN, "test.bmq_data"), np.uint8)
    recs = j[JH:].reshape(-1, 60)
    assert (recs[:, 0] >> 4).tolist() == [5, 4, 5, 1, 5, 2, 3, 5, 5, 5, 1, 5, 5]
    guids = np.concatenate([recs[3, 36:52], recs[10, 36:52]])
    keys = np.concatenate([recs[3, 22:27], recs[10, 22:27]])
    last = recs[-1]
    kw = dict(lease_id=int.from_bytes(last[8:12].tobytes(), "big"),
              first_seq=int.from_bytes(last[2:8].tobytes(), "big") + 1,
              timestamp=int.from_bytes(last[12:20].tobytes(), "big"))
    # both live
    fresh = np.concatenate([j[:JH], np.delete(recs, [5, 6], 0).reshape(-1)])
    got = M.confirm_records(fresh[JH:], guids, keys, **kw)
    assert isinstance(got, M.Confirmed), got
    assert got.status.tolist() == [1, 1] and got.result["n_deletions"] == 2
    assert got.target.tolist() == [3, 8] and not got.left_out.any()
    out = got.journal.reshape(2, 60)
    assert (out[:, 0] >> 4).tolist() == [3, 3]
    assert out[0].tobytes() == recs[6, :2].tobytes() + out[0, 2:20].tobytes() + recs[6, 20:].tobytes()
    # as they are
    assert len(S.scan_partition(j, d)["record_offset"]) == 1
    got = M.confirm_records(j[JH:], guids, keys, **kw)
    assert got.status.tolist() == [2, 1] and got.target.tolist() == [M.NONE, 10]
    after = S.scan_partition(_extended(j, got.journal), d)
    assert after["recovery_rc"] == 0 and len(after["record_offset"]) == 0


def _random_partition(rng, n_msgs):
    keys = [bytes([k] * 5) for k in (1, 2, 3, 4)]
    w = S.PartitionWriter(lease_id=5)
    for k in keys:
        w.queue_op(S.OP_CREATION, k)
    msgs = []
    for i in range(n_msgs):
        k = keys[int(rng.integers(0, 4))]
        ref = int(rng.integers(1, 5))
        _, guid = w.message(bytes([i & 0xFF]) * int(rng.integers(0, 20)), k, ref_count=ref)
        msgs.append((guid, k, ref))
    w.sync_point()
    return w, msgs


def _random_batch(rng, msgs, left, size, gone=True):
    """Confirms of random messages, never more of one than it has left, stale
    GUIDs among them and, with `gone`, messages that had none left when the
    batch began.  `left` is updated."""
    guids, keys, began = [], [], list(left)
    for _ in range(size):
        m = int(rng.integers(0, len(msgs)))
        if rng.random() < 0.15:
            guids.append(bytes(rng.integers(1, 256, 16, dtype=np.uint8)))
            keys.append(msgs[m][1])
        elif left[m] > 0 or (gone and began[m] == 0 and rng.random() < 0.3):
            left[m] -= 1 if left[m] > 0 else 0
            guids.append(msgs[m][0])
            keys.append(msgs[m][1])
    return (np.frombuffer(b"".join(guids), np.uint8).copy(),
            np.frombuffer(b"".join(keys), np.uint8).copy())


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_recovery_selects_exactly_the_messages_with_references_left(seed):
    rng = np.random.default_rng(seed)
    w, msgs = _random_partition(rng, 60)
    j, d = w.files()
    left = [m[2] for m in msgs]
    seq = w.seq + 1
    for _ in range(4):
        guids, keys = _random_batch(rng, msgs, left, 50)
        got = M.confirm_records(j[JH:], guids, keys, lease_id=5, first_seq=seq, timestamp=9)
        assert isinstance(got, M.Confirmed), got
        seq = got.result["next_seq"]
        j = _extended(j, got.journal)
        scan = S.scan_partition(j, d)
        assert scan["recovery_rc"] == 0
        selected = sorted(((scan["record_offset"].astype(np.int64) - JH) // 60).tolist())
        assert selected == np.flatnonzero(got.left_out > 0).tolist()
        by_record = {4 + i: n for i, n in enumerate(left)}
        assert {r: int(got.left_out[r]) for r in by_record} == by_record
    assert 0 < len(selected) < 60


def test_two_calls_on_the_growing_run_equal_one_call():
    rng = np.random.default_rng(7)
    w, msgs = _random_partition(rng, 40)
    j, _ = w.files()
    run = j[JH:]
    left = [m[2] for m in msgs]
    g1, k1 = _random_batch(rng, msgs, left, 40, gone=False)
    g2, k2 = _random_batch(rng, msgs, left, 40, gone=False)
    kw = dict(lease_id=5, timestamp=3)
    one = M.confirm_records(run, np.concatenate([g1, g2]), np.concatenate([k1, k2]),
                            first_seq=w.seq + 1, **kw)
    a = M.confirm_records(run, g1, k1, first_seq=w.seq + 1, **kw)
    b = M.confirm_records(_extended(run, a.journal), g2, k2, first_seq=a.result["next_seq"], **kw)
    # a message's DELETION record is the last record that names it, in one call or two
    assert np.concatenate([a.journal, b.journal]).tobytes() == one.journal.tobytes()
    assert b.left_out[:run.size // 60].tolist() == one.left_out.tolist()
    assert b.result["next_seq"] == one.result["next_seq"]
    assert np.concatenate([a.status, b.status]).tolist() == one.status.tolist()


@pytest.mark.parametrize("r", C.refused(), ids=lambda r: r.name)
def test_every_refusal_kind_and_their_precedence(r):
    kw = dict(C.KW, journal_dst_bytes=240)
    kw.update(r.kw)
    got = M.confirm_records(r.run, **r.batch, **kw)
    assert got == M.Refusal(r.kind, r.index)
