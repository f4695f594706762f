"""The host PushEventBuilder and PushMessageIterator, and
tests/push_pack_model.py -- the numpy model the GPU tests of
bmqcrc_push_event_pack compare with -- against events spelled out byte by byte,
the reference's fixture partition and one case per refusal condition.  No GPU."""
import os

import numpy as np
import pytest

from blazingmq_amd import Crc32c, PushEventBuilder, PushMessageIterator
from blazingmq_amd import push_event as E
from blazingmq_amd import storage as S
import push_pack_cases as C
import push_pack_model as M
import record_pool

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CRC = Crc32c.calculate
JH = S.PartitionWriter.JOURNAL_HEADER
GUID = bytes([0x40] + [0] * 14 + [0x01])


def _pack(case):
    return M.pack(case.run, case.data, crc32c=CRC, **case.kw)


def _events(p):
    return [p.events[int(p.event_offsets[e]):int(p.event_offsets[e + 1])]
            for e in range(len(p.event_offsets) - 1)]


def test_one_message_with_a_packed_rda_counter_spelled_out():
    """From the header diagrams of bmqp_protocol.h (EventHeader :746, PushHeader
    :2008, OptionHeader :948)."""
    event = bytes([
        0x00, 0x00, 0x00, 0x34,     # EventHeader: fragment 0 | length 52 = 8 + 32 + 4 + 8
        0x44, 0x02, 0x00, 0x00,     # PV 1 | type PUSH (4); HeaderWords 2; 0; 0
        0x00, 0x00, 0x00, 0x0B,     # PushHeader: flags 0 | MessageWords 11 = 8 + 1 + 2
        0x00, 0x00, 0x01, 0x08,     # OptionsWords 1 | CAT 0 | HeaderWords 8
        0x00, 0x00, 0x00, 0x07,     # queue id 7
    ]) + GUID + bytes([
        0x00, 0x00, 0x00, 0x00,     # SchemaId 0; reserved
        0x0E, 0x00, 0x00, 0x05,     # OptionHeader: SUB_QUEUE_INFOS (3) | packed | RDA 5
    ]) + b"hello" + bytes([3, 3, 3])
    assert len(event) == 52
    b = PushEventBuilder()
    b.add_sub_queue_infos_option([(E.DEFAULT_SUB_QUEUE_ID, 5)], pack_rda_counter=True)
    assert b.event_size() == 8 + 32 + 4
    b.pack_message(b"hello", 7, GUID)
    assert b.blob().tobytes() == event
    assert b.message_count() == 1 and b.event_size() == 52


@pytest.mark.parametrize("mode,option", [
    (0, b""),
    # SUB_QUEUE_IDS_OLD (1), 2 words; the id
    (2, bytes([0x04, 0x00, 0x00, 0x02, 0xFF, 0xFF, 0xFF, 0xFE])),
    # SUB_QUEUE_INFOS (3), TypeSpecific 2 (a SubQueueInfo's words), 3 words; the id; RDA | reserved
    (3, bytes([0x0C, 0x40, 0x00, 0x03, 0xFF, 0xFF, 0xFF, 0xFE, 0x85, 0x00, 0x00, 0x00]))])
def test_the_other_option_forms_spelled_out(mode, option):
    words = len(option) // 4
    event = (bytes([0, 0, 0, 8 + 32 + len(option) + 4, 0x44, 0x02, 0, 0]) +
             bytes([0, 0, 0, 8 + words + 1, 0, 0, words, 0x08, 0xFF, 0xFF, 0xFF, 0xFF]) + GUID +
             bytes(4) + option + b"abc\x01")
    b = PushEventBuilder()
    if mode == 2:
        b.add_sub_queue_infos_option([(0xFFFFFFFE, 0x85)], pack_rda_counter=False)
    elif mode == 3:
        b.add_sub_queue_infos_option([(0xFFFFFFFE, 0x85)], pack_rda_counter=True)
    b.pack_message(b"abc", -1, GUID)
    assert b.blob().tobytes() == event
    # and through the model: one MESSAGE record whose application data is "abc"
    w = S.PartitionWriter()
    w.message(b"abc", S.DEFAULT_QUEUE_KEY, guid=GUID)
    j, d = w.files()
    p = M.pack(j[JH:], d, data_file_pos=0, queue_ids=[-1], option_mode=mode,
               rda=[0x85] if mode == 3 else None, sub_ids=[0xFFFFFFFE] if mode else None,
               dst_bytes=len(event), crc32c=CRC)
    assert p.events.tobytes() == event and p.crcs.tolist() == [CRC(b"abc")]


def test_properties_schema_compression_and_out_of_order_spelled_out():
    """DataHeader.flags = 1 (MESSAGE_PROPERTIES), schema id 5, CAT 1 (ZLIB) in
    the MessageRecord, OUT_OF_ORDER from the caller: the first word's top
    nibble is 2 | 4."""
    app = b"12345678"
    event = bytes([
        0x00, 0x00, 0x00, 0x34,     # 52 = 8 + 32 + 8 + 4
        0x44, 0x02, 0x00, 0x00,
        0x60, 0x00, 0x00, 0x0B,     # flags 6 | MessageWords 11 = 8 + 3
        0x00, 0x00, 0x00, 0x28,     # OptionsWords 0 | CAT 1 | HeaderWords 8
        0x7F, 0xFF, 0xFF, 0xFF,     # queue id 2^31 - 1
    ]) + GUID + bytes([0x00, 0x05, 0x00, 0x00]) + app + bytes([4, 4, 4, 4])
    b = PushEventBuilder()
    b.pack_message(app, (1 << 31) - 1, GUID, flags=E.FLAG_OUT_OF_ORDER, compression=1,
                   properties=True, schema_id=5)
    assert b.blob().tobytes() == event
    w = S.PartitionWriter()
    total = 12 + 8 + 4
    w.message(app, S.DEFAULT_QUEUE_KEY, guid=GUID,
              data_header=((3 << 29) | (total // 4)).to_bytes(4, "big") + bytes([0, 0, 0, 1]) +
              bytes([0x00, 0x05, 0, 0]))
    j, d = w.files()
    run = j[JH:].copy()
    run[21] = 0x01              # MessageRecord @21: CAT
    p = M.pack(run, d, data_file_pos=0, queue_ids=[(1 << 31) - 1], flags=[4], dst_bytes=52,
               crc32c=CRC)
    assert p.events.tobytes() == event
    # a DataHeader of two words has no SchemaId: the bytes there are options or data
    short = d.copy()
    short[40:44] = np.frombuffer(((2 << 29) | (total // 4)).to_bytes(4, "big"), np.uint8)
    q = M.pack(run, short, data_file_pos=0, queue_ids=[0], dst_bytes=64, crc32c=CRC)
    (m,) = PushMessageIterator(q.events)
    assert m["schema_id"] == 0 and m["payload"] == bytes([0x00, 0x05, 0, 0]) + app


def test_the_iterator_gives_back_what_the_builder_took():
    rng = np.random.default_rng(5)
    b = PushEventBuilder()
    want = []
    for k in range(40):
        app = rng.integers(0, 256, size=1 + k % 23, dtype=np.uint8).tobytes()
        guid = rng.integers(0, 256, size=16, dtype=np.uint8).tobytes()
        infos = [[], [(0, k)], [(k + 1, 3)], [(7, 1), (9, 2)]][k % 4]
        pack_rda = k % 8 < 4
        b.add_sub_queue_infos_option(infos, pack_rda)
        b.pack_message(app, k - 20, guid, flags=(k % 2) * 4, compression=k % 3,
                       properties=k % 5 == 0, schema_id=k * 1000)
        want.append((k - 20, guid, (k % 2) * 4 | (2 if k % 5 == 0 else 0), k % 3, k * 1000,
                     [(i, r if pack_rda else None) for i, r in infos], app))
    got = [(m["queue_id"], m["guid"], m["flags"], m["compression"], m["schema_id"],
            m["sub_queue_infos"], m["payload"]) for m in PushMessageIterator(b.blob())]
    assert got == want and b.message_count() == 40


def test_the_iterators_checks():
    b = PushEventBuilder()
    b.pack_message(b"hello", 1, GUID)
    b.pack_message(b"", 2, GUID)
    ev = b.blob()
    assert [m["app_length"] for m in PushMessageIterator(ev, allow_empty=True)] == [5, 0]
    # the reference refuses application data of length 0, which its builder packs
    with pytest.raises(ValueError, match="INVALID_APPLICATION_DATA_SIZE at 48"):
        list(PushMessageIterator(ev))
    one = ev[:48].copy()
    one[3] = 48
    assert len(list(PushMessageIterator(one))) == 1

    def broken(edit, size=48):
        bad = one[:size].copy()
        bad[0:4] = np.frombuffer(size.to_bytes(4, "big"), np.uint8)
        edit(bad)
        return bad
    for what, bad in (
            ("NO_PUSH_HEADER at 8", broken(lambda e: None, size=12)),
            ("NO_PUSH_HEADER at 8", broken(lambda e: e.__setitem__(15, 1))),        # 4 bytes
            ("NO_PUSH_HEADER at 8", broken(lambda e: e.__setitem__(15, 11))),       # 44 bytes
            ("INVALID_MESSAGE_SIZE at 8", broken(lambda e: e.__setitem__(11, 0))),
            ("NOT_ENOUGH_BYTES at 8", broken(lambda e: e.__setitem__(11, 11))),
            ("INVALID_OPTIONS_OFFSET at 8", broken(lambda e: e.__setitem__(14, 3))),
            ("INVALID_APPLICATION_DATA_SIZE at 8", broken(lambda e: e.__setitem__(47, 5))),
            ("INVALID_APPLICATION_DATA_SIZE at 8", broken(lambda e: e.__setitem__(47, 0)))):
        with pytest.raises(ValueError, match=what):
            list(PushMessageIterator(bad))
    with pytest.raises(ValueError, match="not a PUSH event"):
        PushMessageIterator(broken(lambda e: e.__setitem__(4, 0x42)))
    # an implicit payload is not measured
    (m,) = PushMessageIterator(broken(lambda e: e.__setitem__(slice(8, 12), [0x10, 0, 0, 8]),
                                      size=40))
    assert m["flags"] == E.FLAG_IMPLICIT_PAYLOAD and m["payload"] == b""


def test_fixture_partition_with_a_repeat():
    """The reference's own partition: its two MESSAGE records (DATA offsets 40
    and 64, both with the CRC bmqstoragetool prints, 3381945770) delivered as
    first, second, first."""
    j = np.fromfile(os.path.join(GOLDEN, "test.bmq_journal"), np.uint8)
    d = np.fromfile(os.path.join(GOLDEN, "test.bmq_data"), np.uint8)
    run = j[JH:]
    assert run.size == 13 * 60 and d.size == 88
    msgs = [i for i in range(13) if int(run[60 * i]) >> 4 == 1]
    assert msgs == [3, 10]
    payloads = []
    for i in msgs:
        o = 8 * int.from_bytes(run[60 * i + 32:60 * i + 36].tobytes(), "big")
        size = 4 * (int.from_bytes(d[o:o + 4].tobytes(), "big") & 0x1FFFFFFF)
        head = 4 * (int(d[o]) >> 5)
        payloads.append(d[o + head:o + size - int(d[o + size - 1])].tobytes())
        assert CRC(payloads[-1]) == 3381945770
    assert [8 * int.from_bytes(run[60 * i + 32:60 * i + 36].tobytes(), "big")
            for i in msgs] == [40, 64]
    for cuts in (None, [0, 1, 3], [0, 1, 2, 3]):
        p = M.pack(run, d, data_file_pos=0, records=[3, 10, 3], queue_ids=[5, 6, 7],
                   option_mode=2, sub_ids=[1, 2, 3], event_first=cuts, dst_bytes=1 << 20,
                   crc32c=CRC)
        assert isinstance(p, M.Packed), p
        n_events = len(cuts) - 1 if cuts else 1
        assert p.result == dict(n_events=n_events, n_msgs=3, n_bad=0, first_bad=3,
                                total_bytes=p.events.size, refused_kind=0, refused_index=0)
        got = [m for ev in _events(p) for m in PushMessageIterator(ev)]
        assert [m["payload"] for m in got] == [payloads[0], payloads[1], payloads[0]]
        assert [m["queue_id"] for m in got] == [5, 6, 7]
        assert [m["guid"] for m in got] == [run[60 * i + 36:60 * i + 52].tobytes()
                                            for i in (3, 10, 3)]
        assert [m["sub_queue_infos"] for m in got] == [[(1, None)], [(2, None)], [(3, None)]]
        assert p.crcs.tolist() == [3381945770] * 3 and p.lengths.tolist() == [
            len(payloads[0]), len(payloads[1]), len(payloads[0])]
    # the identity needs every record to be a MESSAGE record
    q = M.pack(run, d, data_file_pos=0, queue_ids=[0] * 13, dst_bytes=1 << 20, crc32c=CRC)
    assert q == M.Refusal(M.RECORD, 0)
    # the DATA window may begin anywhere: only the records' own bytes are taken
    q = M.pack(run, d[40:], data_file_pos=40, records=[3, 10, 3], queue_ids=[5, 6, 7],
               option_mode=2, sub_ids=[1, 2, 3], event_first=cuts, dst_bytes=1 << 20, crc32c=CRC)
    assert np.array_equal(q.events, p.events)


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
    assert p.result == dict(n_events=3, n_msgs=8, total_bytes=C.TOTAL, n_bad=0, first_bad=8,
                            refused_kind=0, refused_index=0)
    assert p.lengths.tolist() == [C.LENGTH[i] for i in C.RECORDS]
    got = [m for ev in _events(p) for m in PushMessageIterator(ev, allow_empty=True)]
    assert [m["queue_id"] for m in got] == list(C.QUEUE_IDS)
    assert [m["sub_queue_infos"] for m in got] == [[(0, r)] for r in C.RDA]
    assert [len(ev) for ev in _events(p)] == list(C.EVENT_BYTES)
    # the size-only call: the offsets and the total, nothing else
    s = M.pack(run, d, crc32c=CRC, **dict(kw, dst_bytes=None))
    assert s.events.size == 0 and np.array_equal(s.event_offsets, p.event_offsets)
    assert s.result == p.result
    # a flipped payload byte is counted, not refused: record 9 is messages 4 and 7
    b = d.copy()
    b[C.AT[9] + 12 + 20] ^= 0x40
    q = M.pack(run, b, crc32c=CRC, **kw)
    assert (q.result["n_bad"], q.result["first_bad"]) == (2, 4)
    assert np.flatnonzero(q.events != p.events).size == 2
    assert np.flatnonzero(q.crcs != q.expected).tolist() == [4, 7]
    # a stored CRC that is wrong
    j = run.copy()
    j[60 * 5 + 55] ^= 1
    q = M.pack(j, d, crc32c=CRC, **kw)
    assert (q.result["n_bad"], q.result["first_bad"]) == (1, 2)
    assert np.array_equal(q.events, p.events)


def test_no_message():
    run, d, _ = C.base()
    p = M.pack(run, d, data_file_pos=0, records=[], queue_ids=[], dst_bytes=0, crc32c=CRC)
    assert p.result == M.refused_result(M.Refusal(0, 0), 0) and p.events.size == 0


# ---- the numpy-only model of the large GPU cases --------------------------------

N_POOL = 4101        # messages of the pool: four tiles and five messages
SPLITS = {"own_events": np.arange(N_POOL + 1), "one_event": None,
          "events_of_3": np.append(np.arange(0, N_POOL, 3), N_POOL),
          "events_of_1024": np.append(np.arange(0, N_POOL, 1024), N_POOL),
          "uneven": np.array([0, 1, 2, 1500, 1501, 1502, 3000, 4100, N_POOL])}


def _pool_call(mode, with_flags, gather=True):
    """(journal, DATA file, keywords) of N_POOL messages of the pool; message
    1,500 and a repeat name the longest record."""
    rng = np.random.default_rng(77)
    p = record_pool.pool()
    records = record_pool.push_records(N_POOL).copy()
    records[[1500, 2900]] = p.long[0]
    qids = rng.integers(-2**31, 2**31, size=N_POOL, dtype=np.int64).astype(np.int32)
    qids[:3] = (-1, -2**31, 2**31 - 1)
    kw = dict(data_file_pos=0, queue_ids=qids, records=records if gather else None,
              option_mode=mode, flags=4 * rng.integers(0, 2, size=N_POOL) if with_flags else None,
              rda=rng.integers(0, 256, size=N_POOL) if mode in (1, 3) else None,
              sub_ids=rng.integers(0, 1 << 32, size=N_POOL, dtype=np.uint64) if mode in (2, 3)
              else None)
    run = p.run if gather else record_pool.message_journal()[:60 * N_POOL]
    return run, p.data, kw


def _same(got, want):
    assert got.result == want.result
    for name in ("events", "event_offsets", "crcs", "lengths", "expected"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and np.array_equal(a, b), name


@pytest.mark.parametrize("split", sorted(SPLITS))
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("with_flags", [False, True])
def test_fast_model_is_the_loop_model_and_the_builder(split, mode, with_flags):
    run, d, kw = _pool_call(mode, with_flags)
    kw["event_first"] = SPLITS[split]
    want = M.pack(run, d, crc32c=CRC, dst_bytes=1 << 40, **kw)
    assert want.result["n_bad"] == 0 and int(want.lengths.max()) == record_pool.LONG[0]
    _same(M.push_events_fast(run, d, crc32c=CRC, **kw), want)
    _same(M.push_events_fast(run, d, record_crcs=record_pool.pool().crcs, **kw), want)
    sized = M.pack(run, d, crc32c=CRC, **dict(kw, dst_bytes=None))
    _same(M.push_events_fast(run, d, crc32c=CRC, **dict(kw, dst_bytes=None)), sized)


@pytest.mark.parametrize("call", ["window", "identity"])
def test_fast_model_in_a_window_and_without_a_gather(call):
    run, d, kw = _pool_call(3, True, gather=call != "identity")
    kw["event_first"] = SPLITS["events_of_3"]
    if call == "window":
        kw["data_file_pos"], d = 40, d[40:]
    want = M.pack(run, d, crc32c=CRC, dst_bytes=1 << 40, **kw)
    _same(M.push_events_fast(run, d, crc32c=CRC, **kw), want)


def test_fast_model_counts_mismatches_and_refuses_like_the_loop_model():
    run, d, kw = _pool_call(1, True)
    kw["event_first"] = SPLITS["events_of_3"]
    bad = run.copy()
    victims = kw["records"][[5, 700]]
    kw["records"][3000] = victims[1]               # named twice: counted twice
    bad[60 * victims[:, None] + 52 + np.arange(4)] ^= 0x5A
    want = M.pack(bad, d, crc32c=CRC, dst_bytes=1 << 40, **kw)
    assert (want.result["n_bad"], want.result["first_bad"]) == (3, 5)
    _same(M.push_events_fast(bad, d, crc32c=CRC, **kw), want)
    total = want.result["total_bytes"]
    flags = kw["flags"].copy()
    flags[[4000, 4100]] = (1, 6)
    for change in (dict(max_payload_bytes=record_pool.LONG[0]),
                   dict(max_payload_bytes=record_pool.LONG[0] - 1), dict(max_event_bytes=1000),
                   dict(dst_bytes=total - 1), dict(dst_bytes=total // 2), dict(dst_bytes=total),
                   dict(flags=flags), dict(flags=flags, max_payload_bytes=10)):
        want = M.pack(run, d, crc32c=CRC, **dict(dict(kw, dst_bytes=1 << 40), **change))
        got = M.push_events_fast(run, d, crc32c=CRC, **dict(kw, **change))
        if isinstance(want, M.Refusal):
            assert got == want, change
        else:
            assert got.result == want.result, change
    refused = M.push_events_fast(run, d, crc32c=CRC,
                                 **dict(kw, max_payload_bytes=record_pool.LONG[0] - 1))
    assert refused == M.Refusal(M.PAYLOAD_TOO_BIG, 1500)
