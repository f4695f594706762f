"""tests/rollover_model.py -- the numpy model the GPU tests of
bmqcrc_partition_rollover compare with -- against journals spelled out byte by
byte, the reference's fixture partition, the native recovery walk over the
rolled partition, a second roll, a dictionary restatement of the CONFIRM join
and one case per refusal condition.  No GPU."""
import os

import numpy as np
import pytest

from blazingmq_amd import Crc32c, rollover_records  # noqa: F401  (the feature under test)
from blazingmq_amd import storage as S

import rollover_cases as C
import rollover_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CRC = Crc32c.calculate
JH = S.PartitionWriter.JOURNAL_HEADER


def _roll(case):
    return M.rollover(case.run, case.data, crc32c=CRC, **case.kw)


@pytest.mark.parametrize("w", C.written(), ids=lambda w: w.case.name)
def test_small_journals_byte_by_byte(w):
    data, journal = C.expected_bytes(w)
    got = _roll(w.case)
    assert isinstance(got, M.Rolled), got
    assert got.data.tobytes() == data.tobytes()
    assert got.journal.tobytes() == journal.tobytes()
    index = np.full(C.N, M.NOT_KEPT, np.uint32)
    index[list(w.kept)] = np.arange(len(w.kept))
    assert got.new_index.tolist() == index.tolist()
    crcs = np.zeros(C.N, np.uint32)
    for r, app in zip(C.MESSAGES, C.APPS):
        if r in w.kept:
            crcs[r] = CRC(app)
    assert got.crcs.tolist() == crcs.tolist()
    assert got.result == dict(
        n_records=C.N, n_kept=len(w.kept), n_messages=len(w.offsets), journal_bytes=journal.size,
        data_bytes=data.size, n_bad=0, first_bad=C.N, refused_kind=0, refused_index=0)


def test_empty_run():
    got = M.rollover(np.zeros(0, np.uint8), np.zeros(64, np.uint8), data_file_pos=0,
                     new_data_file_pos=40, dst_bytes=0, journal_dst_bytes=0, crc32c=CRC)
    assert got.data.size == got.journal.size == 0 and not any(got.result.values())


def _fixture():
    j = np.fromfile(os.path.join(GOLDEN, "test.bmq_journal"), np.uint8)
    d = np.fromfile(os.path.join(GOLDEN, "test.bmq_data"), np.uint8)
    run = j[JH:]
    assert run.size == 13 * 60 and d.size == 88
    return j, d, run


def test_fixture_partition_to_its_own_position_and_to_another():
    """The reference's partition (two "hello world" MESSAGE records at 40 and
    64): rolled to position 40 with everything kept, the DATA records and the
    MESSAGE records come out exactly; to another position only the four
    MessageOffsetDwords bytes of each record differ."""
    _, d, run = _fixture()
    recs = run.reshape(13, 60)
    msgs = np.flatnonzero(recs[:, 0] >> 4 == 1)
    assert msgs.size == 2
    kw = dict(data_file_pos=0, dst_bytes=48, journal_dst_bytes=60 * 13, crc32c=CRC)
    same = M.rollover(run, d, new_data_file_pos=40, **kw)
    assert same.data.tobytes() == d[40:].tobytes()
    new = same.journal.reshape(-1, 60)
    assert same.result["n_messages"] == 2 and same.result["n_bad"] == 0
    for m in msgs:
        assert new[same.new_index[m]].tobytes() == recs[m].tobytes()
    # JOURNAL_OP records are the only ones dropped
    assert same.result["n_kept"] == int((recs[:, 0] >> 4 != 5).sum())
    moved = M.rollover(run, d, new_data_file_pos=4096, **kw)
    assert moved.data.tobytes() == same.data.tobytes()
    differ = np.flatnonzero(moved.journal != same.journal)
    rows = sorted(int(same.new_index[m]) for m in msgs)
    assert set(differ.tolist()) <= {60 * r + b for r in rows for b in range(32, 36)}
    got = [int.from_bytes(moved.journal[60 * r + 32:60 * r + 36].tobytes(), "big") for r in rows]
    assert got == [4096 // 8, (4096 + 24) // 8]


def _files(rolled, new_data_file_pos, partition_id=0):
    """The rolled run and window wrapped in file headers (new_data_file_pos 40:
    the DATA file's FileHeader and DataFileHeader)."""
    assert new_data_file_pos == 40
    journal = S.file_header(S.FILE_TYPE_JOURNAL, partition_id).tobytes() + bytes([3, 15]) + \
        bytes(10) + rolled.journal.tobytes()
    data = S.file_header(S.FILE_TYPE_DATA, partition_id).tobytes() + bytes([2, 0, 0, 0, 0, 0, 0, 0]) + \
        rolled.data.tobytes()
    return np.frombuffer(journal, np.uint8).copy(), np.frombuffer(data, np.uint8).copy()


def _outstanding(journal, data):
    """(GUID, queue key, length, CRC) of what the native recovery walk selects, in its order."""
    scan = S.scan_partition(journal, data)
    assert scan["recovery_rc"] == 0
    out = []
    for off, length, crc in zip(scan["record_offset"], scan["app_length"], scan["crc32c"]):
        r = journal[int(off):int(off) + 60]
        out.append((r[36:52].tobytes(), r[22:27].tobytes(), int(length), int(crc)))
    return out


def _busy_partition():
    """Three queues, deletions, a purge and sync points: what recovery has to decide."""
    rng = np.random.default_rng(18)
    w = S.PartitionWriter(lease_id=3)
    keys = [bytes([k] * 5) for k in (1, 2, 3)]
    for k in keys:
        w.queue_op(S.OP_CREATION, k)
    guids = []
    for i in range(40):
        k = keys[i % 3]
        app = rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8).tobytes()
        guids.append((w.message(app, k)[1], k))
        if i % 4 == 1:
            w.confirm(guids[-1][0], k)
        if i % 7 == 3:
            w.deletion(*guids[i - 2])
        if i == 20:
            w.queue_op(S.OP_PURGE, keys[2])
        if i % 10 == 9:
            w.sync_point()
    w.sync_point()
    return w.files()


def test_recovery_selects_the_same_messages_after_the_roll_and_a_second_roll_changes_nothing():
    j, d = _busy_partition()
    run = j[JH:]
    n = run.size // 60
    before = _outstanding(j, d)
    assert 10 < len(before) < 40
    # keep what recovery selects (the scan's records), every record that is not
    # a MESSAGE or JOURNAL_OP record, and restate the last sync point
    scan = S.scan_partition(j, d)
    types = run.reshape(n, 60)[:, 0] >> 4
    keep = ((types != 1) & (types != 5)).astype(np.uint8)
    keep[(scan["record_offset"].astype(np.int64) - JH) // 60] = 1
    kw = dict(data_file_pos=0, new_data_file_pos=40, keep=keep, sync_point=n - 1, timestamp=77,
              dst_bytes=d.size, journal_dst_bytes=run.size, crc32c=CRC)
    rolled = M.rollover(run, d, **kw)
    assert rolled.result["n_messages"] == len(before) and rolled.result["n_bad"] == 0
    j2, d2 = _files(rolled, 40)
    assert _outstanding(j2, d2) == before
    # what verify_partition checks, on the host (the batched verify needs a
    # GPU: tests/test_gpu_rollover.py runs it over the same files)
    scan2 = S.scan_partition(j2, d2)
    for off, length, crc in zip(scan2["app_offset"], scan2["app_length"], scan2["crc32c"]):
        assert CRC(d2[int(off):int(off) + int(length)].tobytes()) == int(crc)
    # idempotence: everything kept, same position and timestamp
    run2 = j2[JH:]
    again = M.rollover(run2, d2, **dict(kw, keep=None, sync_point=run2.size // 60 - 1,
                                        dst_bytes=d2.size, journal_dst_bytes=run2.size))
    assert again.journal.tobytes() == rolled.journal.tobytes()
    assert again.data.tobytes() == rolled.data.tobytes()


def _follow_by_dictionary(recs, keep):
    """CONFIRMS_FOLLOW_MESSAGES restated with a dictionary, record by record."""
    have = {}
    for i, r in enumerate(recs):
        if r[0] >> 4 == 1 and (keep is None or keep[i]):
            have[(r[36:52].tobytes(), r[22:27].tobytes())] = i
    kept = []
    for i, r in enumerate(recs):
        t = r[0] >> 4
        if t == 5:
            kept.append(False)
        elif t == 2:
            kept.append((r[32:48].tobytes(), r[22:27].tobytes()) in have)
        else:
            kept.append(keep is None or bool(keep[i]))
    return kept


def test_confirms_follow_messages_against_a_dictionary():
    run, d, keep, kept = C.join_partition()
    recs = run.reshape(-1, 60)
    want = _follow_by_dictionary(recs, keep)
    assert np.flatnonzero(want).tolist() == kept
    assert M.kept_records(recs, keep, M.CONFIRMS_FOLLOW_MESSAGES).tolist() == want
    got = M.rollover(run, d, data_file_pos=0, new_data_file_pos=40, keep=keep, confirm_mode=1,
                     dst_bytes=d.size, journal_dst_bytes=run.size, crc32c=CRC)
    assert np.flatnonzero(got.new_index != M.NOT_KEPT).tolist() == [0, 2, 5, 6, 7, 8, 9, 11, 14]
    # keep == NULL: every MESSAGE is kept, so every CONFIRM with a MESSAGE is
    want = _follow_by_dictionary(recs, None)
    assert M.kept_records(recs, None, M.CONFIRMS_FOLLOW_MESSAGES).tolist() == want
    assert [i for i in (0, 1, 4, 12) if want[i]] == [0, 1]
    # random keeps over the busy partition
    j, _ = _busy_partition()
    recs = j[JH:].reshape(-1, 60)
    rng = np.random.default_rng(5)
    for _ in range(20):
        keep = (rng.random(recs.shape[0]) < 0.5).astype(np.uint8)
        assert M.kept_records(recs, keep, 1).tolist() == _follow_by_dictionary(recs, keep)


@pytest.mark.parametrize("r", C.refused()[0], ids=lambda r: r.case.name)
def test_every_refusal_kind_and_their_precedence(r):
    got = _roll(r.case)
    assert got == M.Refusal(r.kind, r.index), got
    assert M.refused_result(got, C.N)["refused_kind"] == r.kind


@pytest.mark.parametrize("case", C.refused()[1], ids=lambda c: c.name)
def test_what_is_no_refusal(case):
    assert isinstance(_roll(case), M.Rolled)


def test_a_wrong_stored_crc_is_counted_and_rolled():
    run, data, _ = C.partition()
    data = data.copy()
    data[80 + 12 + 3] ^= 0x40           # m2's application data
    got = M.rollover(run, data, crc32c=CRC, **C.written()[0].case.kw)
    assert got.result["n_bad"] == 1 and got.result["first_bad"] == 5
    assert got.data.tobytes() == data[40:].tobytes()
