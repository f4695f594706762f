"""tests/storage_pack_model.py -- the numpy model the GPU tests of
bmqcrc_storage_event_pack compare with -- against the reference's fixture
partition, synth.storage_events, the host iterator, a hand-assembled QLIST
event and one case per refusal condition.  No GPU."""
import os

import numpy as np
import pytest

from blazingmq_amd import Crc32c, StorageMessageIterator
from blazingmq_amd import storage as S
from blazingmq_amd import storage_event as E
from blazingmq_amd import synth
import record_pool
import storage_apply_cases as A
import storage_apply_model as AM
import storage_pack_cases as C
import storage_pack_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CRC = Crc32c.calculate
JH = S.PartitionWriter.JOURNAL_HEADER


def _pack(case):
    return M.pack(case.run, case.data, crc32c=CRC, **case.kw)


def test_fixture_partition_round_trip():
    """The reference's own partition, replicated: its records packed by the
    model and applied by the replica's model to the same positions give the
    fixture's bytes back in both files, and the host iterator walks every event."""
    j = np.fromfile(os.path.join(GOLDEN, "test.bmq_journal"), np.uint8)
    d = np.fromfile(os.path.join(GOLDEN, "test.bmq_data"), np.uint8)
    run = j[JH:]
    assert run.size == 13 * 60 and d.size == 88
    for cuts in (None, [0, 4, 8, 12, 13], list(range(14))):
        p = M.pack(run, d, journal_pos=JH, data_file_pos=0, partition_id=0,
                   event_first=cuts, dst_bytes=1 << 20, crc32c=CRC)
        assert isinstance(p, M.Packed), p
        n_events = len(cuts) - 1 if cuts else 1
        assert p.result == dict(n_events=n_events, n_msgs=13, n_data=2, n_bad=0, first_bad=13,
                                total_bytes=8 * n_events + 13 * 72 + 48, refused_kind=0,
                                refused_index=0)
        # (the fixture's QUEUE_OP record is a CREATION: a QLIST message)
        assert p.types.tolist() == [5, 2, 5, 1, 5, 3, 4, 5, 5, 5, 1, 5, 5]
        walked = 0
        for e in range(n_events):
            ev = p.events[int(p.event_offsets[e]):int(p.event_offsets[e + 1])]
            for m in StorageMessageIterator(ev):
                assert m["message_type"] == p.types[walked] and m["partition_id"] == 0
                assert m["journal_offset_words"] * 4 == JH + 60 * walked
                walked += 1
        assert walked == 13
        a = AM.apply(p.events, p.event_offsets, partition_id=0, journal_pos=JH, data_file_pos=40,
                     msg_cap=13, journal_dst_bytes=run.size, data_dst_bytes=48, crc32c=CRC)
        assert isinstance(a, AM.Applied), a
        assert np.array_equal(a.journal, run) and np.array_equal(a.data, d[40:])
        assert np.array_equal(a.crcs, p.crcs) and np.array_equal(a.expected, p.expected)
    # the DATA window may begin anywhere: only the records' own bytes are taken
    q = M.pack(run, d[40:], journal_pos=JH, data_file_pos=40, partition_id=0, event_first=cuts,
               dst_bytes=1 << 20, crc32c=CRC)
    assert np.array_equal(q.events, p.events)


@pytest.mark.parametrize("per_event", [1, 3, 17, 40])
def test_model_emits_what_synth_emits(per_event):
    # without its first record, the queue's CREATION, which synth makes a QUEUE_OP message
    run, d = A.partition()
    run = run[60:]
    n = run.size // 60
    want, want_offsets = synth.storage_events(run, d, 0, A.JOURNAL_POS + 60, A.PARTITION,
                                              per_event)
    cuts = list(range(0, n, per_event)) + [n]
    p = M.pack(run, d, journal_pos=A.JOURNAL_POS + 60, data_file_pos=0, partition_id=A.PARTITION,
               event_first=cuts, dst_bytes=want.size, crc32c=CRC)
    assert isinstance(p, M.Packed), p
    assert np.array_equal(p.events, want) and np.array_equal(p.event_offsets, want_offsets)
    assert p.result["n_bad"] == 0 and p.result["n_data"] == 7
    assert p.result["total_bytes"] == want.size


def test_a_creation_record_becomes_a_qlist_message_of_72_bytes():
    """One PARTITION_SYNC event of a queue's CREATION record alone, spelled byte
    by byte from the header diagrams of bmqp_protocol.h (EventHeader :746,
    StorageHeader :2807): a QLIST message that carries the journal record only,
    which is what FileStore::writeQueueCreationRecord hands replicateRecord
    when the cluster is not QLIST aware (mqbs_filestore.cpp:5095-5102, 6030)."""
    run, d = A.partition()
    record = run[:60]
    assert int(record[0]) >> 4 == S.REC_QUEUE_OP
    assert int.from_bytes(record[32:36].tobytes(), "big") == S.OP_CREATION
    event = bytes([
        0x00, 0x00, 0x00, 0x50,     # EventHeader: fragment 0 | length 80 = 8 + 72
        0x4A, 0x02, 0x00, 0x00,     # PV 1 | type PARTITION_SYNC (10); HeaderWords 2; 0; 0
        0xB8, 0x00, 0x00, 0x12,     # StorageHeader: flags 23 | MessageWords 18
        0x23, 0x02, 0xFF, 0xFE,     # reserved | SPV 2 | HeaderWords 3; QLIST; partition 65534
        0x00, 0x00, 0x00, 0x0B,     # journal offset 11 words = byte 44
    ]) + record.tobytes()
    p = M.pack(record, d, journal_pos=44, data_file_pos=0, partition_id=65534,
               flags=np.array([0xF7], np.uint8), event_type=E.EVENT_TYPE_PARTITION_SYNC,
               storage_protocol_version=2, dst_bytes=80, crc32c=CRC)
    assert p.events.tobytes() == event and p.event_offsets.tolist() == [0, 80]
    assert p.types.tolist() == [E.MSG_QLIST] and p.crcs.tolist() == [0]
    # ADDITION likewise; PURGE and DELETION stay QUEUE_OP messages
    for op, want in ((S.OP_ADDITION, E.MSG_QLIST), (S.OP_PURGE, E.MSG_QUEUE_OP),
                     (S.OP_DELETION, E.MSG_QUEUE_OP)):
        r = record.copy()
        A.put32(r, 32, op)
        q = M.pack(r, d, journal_pos=44, data_file_pos=0, partition_id=0, dst_bytes=80, crc32c=CRC)
        assert q.types.tolist() == [want] and q.events.size == 80 and q.events[13] == want


@pytest.mark.parametrize("name", sorted(C.refusal_cases()))
def test_refusal(name):
    case = C.refusal_cases()[name]
    assert _pack(case) == case.want


@pytest.mark.parametrize("name", sorted(C.precedence_cases()))
def test_precedence(name):
    case = C.precedence_cases()[name]
    assert _pack(case) == case.want


def test_the_unmodified_base_packs_and_a_flipped_byte_is_counted():
    run, d, kw = C.base()
    p = M.pack(run, d, crc32c=CRC, **kw)
    assert isinstance(p, M.Packed)
    assert p.event_offsets.tolist() == [0] + list(np.cumsum(C.EVENT_BYTES))
    assert p.result == dict(n_events=4, n_msgs=17, n_data=7, total_bytes=C.TOTAL, n_bad=0,
                            first_bad=17, refused_kind=0, refused_index=0)
    assert [i for i, t in enumerate(p.types) if t == 1] == list(C.MESSAGES)
    # exact capacities are enough, and a flipped payload byte is counted, not refused
    b = d.copy()
    b[C.AT[12] + 12 + 100] ^= 0x40
    q = M.pack(run, b, crc32c=CRC, **kw)
    assert (q.result["n_bad"], q.result["first_bad"]) == (1, 12)
    assert np.flatnonzero(q.events != p.events).size == 1
    assert np.flatnonzero(q.crcs != q.expected).tolist() == [12]
    # flags: the low five bits, for any type
    f = (np.arange(17) * 37 % 256).astype(np.uint8)
    q = M.pack(run, d, crc32c=CRC, **dict(kw, flags=f))
    got = [m["flags"] for e in range(4) for m in StorageMessageIterator(
        q.events[int(q.event_offsets[e]):int(q.event_offsets[e + 1])])]
    assert got == (f & 31).tolist()


def test_no_record():
    p = M.pack(np.zeros(0, np.uint8), np.zeros(8, np.uint8), journal_pos=44, data_file_pos=0,
               partition_id=0, dst_bytes=0, crc32c=CRC)
    assert p.result == M.refused_result(M.Refusal(0, 0), 0) and p.events.size == 0


# ---- the numpy-only model of the large GPU cases --------------------------------

N_POOL = 4101        # records of the pool: four tiles and five records, the long message among them
SPLITS = {"own_events": np.arange(N_POOL + 1), "one_event": None,
          "events_of_3": np.append(np.arange(0, N_POOL, 3), N_POOL),
          "events_of_1024": np.append(np.arange(0, N_POOL, 1024), N_POOL),
          "uneven": np.array([0, 1, 2, 1500, 1524, 1525, 3000, 4100, N_POOL])}


def test_the_pool_holds_what_the_large_cases_rely_on():
    record_pool.check_properties()


@pytest.mark.parametrize("split", sorted(SPLITS))
@pytest.mark.parametrize("call", ["plain", "flags_and_fields", "window", "journal_pos_past_2_31"])
def test_fast_model_is_the_loop_model_and_the_builder(split, call):
    run, d = record_pool.records(N_POOL)
    assert record_pool.pool().long[0] < N_POOL
    kw = dict(journal_pos=JH, data_file_pos=0, partition_id=1, event_first=SPLITS[split])
    if call == "flags_and_fields":
        kw.update(flags=(np.arange(N_POOL) * 37 % 256).astype(np.uint8), partition_id=65535,
                  event_type=E.EVENT_TYPE_PARTITION_SYNC, storage_protocol_version=2)
    elif call == "window":
        kw.update(data_file_pos=40)
        d = d[40:]
    elif call == "journal_pos_past_2_31":
        kw.update(journal_pos=4 * (1 << 31) - 60 * 2000)
        words = (kw["journal_pos"] + 60 * np.arange(N_POOL)) // 4
        assert words[0] < 1 << 31 < words[-1] < 1 << 32
    want = M.pack(run, d, crc32c=CRC, dst_bytes=1 << 40, **kw)
    for crcs in (None, record_pool.pool().crcs[:N_POOL]):
        got = M.storage_events_fast(run, d, crc32c=CRC, record_crcs=crcs, **kw)
        assert got.result == want.result and got.result["n_bad"] == 0
        for name in ("events", "event_offsets", "types", "crcs", "expected"):
            a, b = getattr(got, name), getattr(want, name)
            assert a.dtype == b.dtype and np.array_equal(a, b), name


def test_fast_model_counts_mismatches_and_refuses_like_the_loop_model():
    run, d = record_pool.records(N_POOL)
    long = record_pool.pool().long[0]
    kw = dict(journal_pos=JH, data_file_pos=0, partition_id=1, event_first=SPLITS["events_of_3"])
    bad = run.copy()
    victims = record_pool.pool().msgs[[5, 700]]
    bad[60 * victims[:, None] + 52 + np.arange(4)] ^= 0x5A
    want = M.pack(bad, d, crc32c=CRC, dst_bytes=1 << 40, **kw)
    got = M.storage_events_fast(bad, d, crc32c=CRC, **kw)
    assert got.result == want.result and want.result["n_bad"] == 2
    assert np.array_equal(got.events, want.events) and np.array_equal(got.expected, want.expected)
    total, size = want.result["total_bytes"], 60 + record_pool.LONG[0] + 28
    for change in (dict(max_payload_bytes=size), dict(max_payload_bytes=size - 28),
                   dict(max_event_bytes=1000), dict(dst_bytes=total - 4),
                   dict(dst_bytes=total // 2), dict(dst_bytes=total)):
        want = M.pack(run, d, crc32c=CRC, **dict(dict(kw, dst_bytes=1 << 40), **change))
        got = M.storage_events_fast(run, d, crc32c=CRC, **dict(kw, **change))
        if isinstance(want, M.Refusal):
            assert got == want, change
        else:
            assert got.result == want.result, change
    refused = M.storage_events_fast(run, d, crc32c=CRC, **dict(kw, max_payload_bytes=size - 28))
    assert refused == M.Refusal(M.PAYLOAD_TOO_BIG, long)
