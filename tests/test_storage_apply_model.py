"""STORAGE events on the host: StorageEventBuilder and StorageMessageIterator
against the wire format, synth.storage_events, and tests/storage_apply_model.py
-- the numpy model the GPU tests of bmqcrc_storage_event_apply compare with --
against the reference's fixture partition, the host iterator and one case per
refusal condition.  No GPU."""
import os

import numpy as np
import pytest

from blazingmq_amd import Crc32c, StorageEventBuilder, StorageMessageIterator
from blazingmq_amd import storage as S
from blazingmq_amd import storage_event as E
from blazingmq_amd import synth
import storage_apply_cases as C
import storage_apply_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CRC = Crc32c.calculate


def _apply(case):
    return M.apply(case.events, case.offsets, crc32c=CRC, **case.kw)


def test_builder_reproduces_a_hand_assembled_event():
    """One STORAGE event of a DATA and a DELETION message, spelled byte by byte
    from the header diagrams of bmqp_protocol.h (EventHeader :746, StorageHeader
    :2807) and mqbs_filestoreprotocol.h (DataHeader :703).  The reference has
    no tool that prints a storage event, so the layout rests on those
    headers' documentation, not on a recorded reference output."""
    message = bytes([0x10, 0x01, 0, 0, 0, 0, 0, 7, 0, 0, 0, 2]) + bytes(range(48))
    deletion = bytes([0x30, 0x00, 0, 0, 0, 0, 0, 8, 0, 0, 0, 2]) + bytes(range(100, 148))
    record = bytes([
        0x60, 0x00, 0x00, 0x04,     # DataHeader: HeaderWords 3 | MessageWords 4
        0x00, 0x00, 0x00, 0x05,     # OptionsWords 0 | Flags 5
        0x00, 0x00, 0x00, 0x00,     # SchemaId, Reserved
        0xAA, 0xBB, 0x02, 0x02])    # two bytes of application data, padding 2 2
    event = bytes([
        0x00, 0x00, 0x00, 0xA8,     # EventHeader: fragment 0 | length 168 = 8 + 88 + 72
        0x48, 0x02, 0x00, 0x00,     # PV 1 | type STORAGE (8); HeaderWords 2; type specific; 0
        0x08, 0x00, 0x00, 0x16,     # StorageHeader: flags RECEIPT_REQUESTED | MessageWords 22
        0x13, 0x01, 0x00, 0x09,     # reserved | SPV 1 | HeaderWords 3; DATA; partition 9
        0x00, 0x00, 0x00, 0x0B,     # journal offset 11 words = byte 44
    ]) + message + record + bytes([
        0x00, 0x00, 0x00, 0x12,     # StorageHeader: no flags | MessageWords 18
        0x13, 0x04, 0x00, 0x09,     # DELETION; partition 9
        0x00, 0x00, 0x00, 0x1A,     # journal offset 26 words = byte 104
    ]) + deletion
    assert len(event) == 168
    b = StorageEventBuilder()
    b.pack_message(E.MSG_DATA, 9, 11, message, record, flags=E.FLAG_RECEIPT_REQUESTED)
    # (a payload is appended for DATA and QLIST messages only)
    b.pack_message(E.MSG_DELETION, 9, 26, deletion, b"ignored!")
    assert (b.message_count(), b.event_size()) == (2, 168)
    events, offsets = b.finalize()
    assert events.tobytes() == event and offsets.tolist() == [0, 168]
    got = list(StorageMessageIterator(events))
    assert [(m["message_type"], m["flags"], m["partition_id"], m["journal_offset_words"],
             m["header_offset"], m["record_offset"], m["payload_offset"], m["payload_length"],
             m["storage_protocol_version"]) for m in got] == [
        (1, 1, 9, 11, 8, 20, 80, 16, 1), (4, 0, 9, 26, 96, 108, 168, 0, 1)]


def test_builder_flushes_at_the_event_size_limit():
    b = StorageEventBuilder(max_event_bytes=8 + 2 * 72)
    for i in range(5):
        b.pack_message(E.MSG_CONFIRM, 0, 11 + 15 * i, bytes(60))
    events, offsets = b.finalize()
    assert offsets.tolist() == [0, 152, 304, 384]
    assert [len(list(StorageMessageIterator(events[int(a):int(z)])))
            for a, z in zip(offsets, offsets[1:])] == [2, 2, 1]
    with pytest.raises(ValueError, match="EVENT_TOO_BIG"):
        StorageEventBuilder(max_event_bytes=64).pack_message(E.MSG_CONFIRM, 0, 11, bytes(60))
    with pytest.raises(ValueError, match="60 bytes"):
        StorageEventBuilder().pack_message(E.MSG_CONFIRM, 0, 11, bytes(59))
    with pytest.raises(ValueError, match="STORAGE or PARTITION_SYNC"):
        StorageEventBuilder(event_type=2)
    b = StorageEventBuilder(event_type=E.EVENT_TYPE_PARTITION_SYNC)
    b.flush()   # an event with no message is legal
    events, offsets = b.finalize()
    assert events.tolist() == [0, 0, 0, 8, (1 << 6) | 10, 2, 0, 0] and offsets.tolist() == [0, 8]
    assert list(StorageMessageIterator(events)) == []


@pytest.mark.parametrize("per_event", [1, 3, 17, 40])
def test_synth_emits_what_the_builder_emits(per_event):
    run, d = C.partition()
    b = StorageEventBuilder()
    for i, r in enumerate(run.reshape(-1, 60)):
        if i and i % per_event == 0:
            b.flush()
        kind = {S.REC_MESSAGE: E.MSG_DATA, S.REC_CONFIRM: E.MSG_CONFIRM,
                S.REC_DELETION: E.MSG_DELETION, S.REC_QUEUE_OP: E.MSG_QUEUE_OP,
                S.REC_JOURNAL_OP: E.MSG_JOURNAL_OP}[int(r[0]) >> 4]
        payload = b""
        if kind == E.MSG_DATA:
            at = int.from_bytes(r[32:36].tobytes(), "big") * 8
            payload = d[at:at + 4 * (int.from_bytes(d[at:at + 4].tobytes(), "big") & 0x1FFFFFFF)]
        b.pack_message(kind, C.PARTITION, (C.JOURNAL_POS + 60 * i) // 4, r, payload)
    events, offsets = b.finalize()
    got, got_offsets = synth.storage_events(run, d, 0, C.JOURNAL_POS, C.PARTITION, per_event)
    assert np.array_equal(got, events) and np.array_equal(got_offsets, offsets)
    assert got_offsets.dtype == np.uint64 and got.dtype == np.uint8
    none, one = synth.storage_events(run[:0], d, 0, C.JOURNAL_POS, C.PARTITION, per_event)
    assert none.tolist() == [0, 0, 0, 8, (1 << 6) | 8, 2, 0, 0] and one.tolist() == [0, 8]


def test_iterator_refuses_what_the_reference_refuses():
    events, offsets, _, lay = C.base()
    ev = events[:int(offsets[1])].copy()
    h = lay[1].header
    for edit, text in ((lambda e: e.__setitem__(h + 4, 0x11), "NO_STORAGEHEADER"),
                       (lambda e: C.put32(e, h, 2), "INVALID_MESSAGE_SIZE"),
                       (lambda e: C.put32(e, h, 10000), "NOT_ENOUGH_BYTES")):
        bad = ev.copy()
        edit(bad)
        with pytest.raises(ValueError, match=text):
            list(StorageMessageIterator(bad))
    with pytest.raises(ValueError, match="matching length"):
        StorageMessageIterator(ev[:-4])


def test_fixture_partition_round_trip():
    """The reference's own partition, replicated: its records built into
    events and applied by the model to the same positions give the fixture's
    bytes back in both files."""
    j = np.fromfile(os.path.join(GOLDEN, "test.bmq_journal"), np.uint8)
    d = np.fromfile(os.path.join(GOLDEN, "test.bmq_data"), np.uint8)
    jh = S.PartitionWriter.JOURNAL_HEADER
    run = j[jh:]
    assert run.size == 13 * 60 and d.size == 88
    for per_event in (1, 4, 13):
        events, offsets = synth.storage_events(run, d, 0, jh, 0, per_event)
        assert offsets.size - 1 == -(-13 // per_event)
        a = M.apply(events, offsets, partition_id=0, journal_pos=jh, data_file_pos=40, msg_cap=13,
                    journal_dst_bytes=run.size, data_dst_bytes=48, crc32c=CRC)
        assert isinstance(a, M.Applied), a
        assert np.array_equal(a.journal, run) and np.array_equal(a.data, d[40:])
        assert a.result == dict(
            n_events=offsets.size - 1, n_msgs=13, n_data=2, journal_bytes=780, data_bytes=48,
            head_seq=4, head_lease_id=2, refused_kind=0, n_bad=0, first_bad=13, refused_event=0,
            refused_index=0, refused_offset=0)
        assert a.record_offsets.tolist() == [0] * 4 + [24] * 7 + [48] * 3
        assert a.types.tolist() == [5, 6, 5, 1, 5, 3, 4, 5, 5, 5, 1, 5, 5]
    # the DATA window may begin anywhere: only the records' own bytes are taken
    events2, _ = synth.storage_events(run, d[40:], 40, jh, 0, 13)
    assert np.array_equal(events2, events)


def _mixed_partition(n, seed):
    """A record run of n records and its DATA file: MESSAGE records whose DATA
    headers are 12 or 20 bytes long and carry 0..2 option words, CONFIRM and
    DELETION records among them."""
    rng = np.random.default_rng(seed)
    w = S.PartitionWriter(lease_id=4, partition_id=1)
    w.queue_op(S.OP_CREATION, S.DEFAULT_QUEUE_KEY)
    while len(w.recs) < n:
        k = len(w.recs)
        app = rng.integers(0, 256, size=int(rng.integers(0, 90)), dtype=np.uint8).tobytes()
        hw, opt = (3, 5)[k % 2], k % 3
        lead = hw * 4 + opt * 4
        total = (lead + len(app)) // 8 * 8 + 8
        header = (((hw << 29) | (total // 4)).to_bytes(4, "big") +
                  ((opt << 8) | (k & 0xFF)).to_bytes(4, "big") + bytes(lead - 8))
        # (the writer frames for a 12-byte header: put the record and the file position right)
        before = w.dpos
        _, guid = w.message(app, S.DEFAULT_QUEUE_KEY, data_header=header[:12])
        pad = total - lead - len(app)
        w.data[-1] = header + app + bytes([pad]) * pad
        w.dpos = before + total
        if k % 4 == 1 and len(w.recs) < n:
            w.deletion(guid, S.DEFAULT_QUEUE_KEY)
    j, d = w.files()
    return j[S.PartitionWriter.JOURNAL_HEADER:], d


@pytest.mark.parametrize("per_event", [1, 2, 63, 64, 65])
def test_model_against_the_iterator(per_event):
    run, d = _mixed_partition(140, per_event)
    n = run.size // 60
    jh = S.PartitionWriter.JOURNAL_HEADER
    events, offsets = synth.storage_events(run, d, 0, jh, 1, per_event)
    a = M.apply(events, offsets, partition_id=1, journal_pos=jh, data_file_pos=40, msg_cap=n,
                journal_dst_bytes=run.size, data_dst_bytes=d.size - 40, crc32c=CRC)
    assert isinstance(a, M.Applied), a
    assert np.array_equal(a.journal, run) and np.array_equal(a.data, d[40:])
    i, leads = 0, set()
    for e in range(offsets.size - 1):
        assert a.event_first[e] == i
        beg = int(offsets[e])
        for m in StorageMessageIterator(events[beg:int(offsets[e + 1])]):
            assert (a.types[i], a.flags[i]) == (m["message_type"], m["flags"])
            assert a.payload_offsets[i] == beg + m["payload_offset"]
            assert a.payload_lengths[i] == m["payload_length"]
            assert m["journal_offset_words"] * 4 == jh + 60 * i
            if m["message_type"] == E.MSG_DATA:
                assert a.payload_lengths[i] == a.record_offsets[i + 1] - a.record_offsets[i]
                pad = int(events[beg + m["payload_offset"] + m["payload_length"] - 1])
                lead = a.payload_lengths[i] - pad - a.lengths[i]
                leads.add(int(lead))
                assert a.crcs[i] == a.expected[i]
            else:
                assert (a.lengths[i], a.expected[i], a.crcs[i]) == (0, 0, 0)
                assert a.record_offsets[i + 1] == a.record_offsets[i]
            i += 1
    assert i == n == a.event_first[-1] and a.result["n_bad"] == 0
    assert a.result["n_data"] == int((a.types == 1).sum()) > 0
    assert leads == {12, 16, 20, 24, 28}   # headers of 3 and 5 words, 0..2 option words


@pytest.mark.parametrize("name", sorted(C.refusal_cases()))
def test_refusal(name):
    case = C.refusal_cases()[name]
    assert _apply(case) == case.want


@pytest.mark.parametrize("name", sorted(C.precedence_cases()))
def test_precedence(name):
    case = C.precedence_cases()[name]
    assert _apply(case) == case.want


def test_the_unmodified_base_applies_and_a_higher_lease_is_accepted():
    events, offsets, kw, lay = C.base()
    a = M.apply(events, offsets, crc32c=CRC, **kw)
    run, d = C.partition()
    assert isinstance(a, M.Applied) and np.array_equal(a.journal, run)
    assert np.array_equal(a.data, d[40:])
    assert (a.result["head_lease_id"], a.result["head_seq"]) == (2, len(lay))
    # a new primary: from some message on a higher lease id, sequence numbers from anywhere
    ev = events.copy()
    for m in lay[7:]:
        C.put32(ev, m.record + 8, 9)
        C.put32(ev, m.record + 4, 1000 + m.index)
    b = M.apply(ev, offsets, crc32c=CRC, **kw)
    assert isinstance(b, M.Applied)
    assert (b.result["head_lease_id"], b.result["head_seq"]) == (9, 1000 + len(lay) - 1)
    # exact capacities are enough, and a flipped payload byte is counted, not refused
    victim = next(m for m in lay if m.type == 1 and m.index > 3)
    ev = events.copy()
    ev[victim.record + 60 + 12] ^= 0x40
    c = M.apply(ev, offsets, crc32c=CRC, **kw)
    assert (c.result["n_bad"], c.result["first_bad"]) == (1, victim.index)
    assert np.flatnonzero(c.data != d[40:]).size == 1 and np.array_equal(c.journal, run)


def test_no_event_and_an_empty_event():
    kw = dict(partition_id=0, journal_pos=44, data_file_pos=40, lease_id=6, seq=77, msg_cap=0,
              journal_dst_bytes=0, data_dst_bytes=0, crc32c=CRC)
    a = M.apply(np.zeros(0, np.uint8), np.zeros(1, np.uint64), **kw)
    assert a.result == dict(n_events=0, n_msgs=0, n_data=0, journal_bytes=0, data_bytes=0,
                            head_seq=77, head_lease_id=6, refused_kind=0, n_bad=0, first_bad=0,
                            refused_event=0, refused_index=0, refused_offset=0)
    b = StorageEventBuilder()
    b.flush()
    events, offsets = b.finalize()
    a = M.apply(events, None, **kw)
    assert a.result["n_events"] == 1 and a.result["n_msgs"] == 0 and a.journal.size == 0
    assert (a.result["head_lease_id"], a.result["head_seq"]) == (6, 77)
    assert a.event_first.tolist() == [0, 0] and a.record_offsets.tolist() == [0]


# ---- apply_fast, the model of the large GPU cases, against apply ------------------

N_SMALL = 4101      # the long message of record_pool.py (record 1,524) among them


def _pool_kw(n, **changes):
    import record_pool as R
    p = R.pool()
    total = int(R.data_fields(p.run, p.data, p.msgs[p.msgs < n])[2].sum())
    return dict(dict(partition_id=1, journal_pos=S.PartitionWriter.JOURNAL_HEADER,
                     data_file_pos=40, lease_id=4, seq=0, msg_cap=n, journal_dst_bytes=60 * n,
                     data_dst_bytes=total), **changes)


def _same(fast, slow):
    assert type(fast) is type(slow), (fast, slow)
    if isinstance(slow, M.Refusal):
        assert fast == slow
        return
    assert fast.result == slow.result
    for name in M.Applied._fields[:-1]:
        a, b = getattr(fast, name), getattr(slow, name)
        assert a.dtype == b.dtype and np.array_equal(a, b), name


def _both(run, data, first, kw, plants=(), crcs=None, flags=None):
    """apply_fast's answer, held to apply's over the same bytes."""
    import record_pool as R
    n = len(run) // 60
    lay = M.layout_fast(run, data, first)
    corrupt, suspects = C.planted(lay, plants)
    events, offsets, fast = M.apply_fast(
        run, data, first, record_crcs=R.pool().crcs[:n] if crcs is None else crcs, flags=flags,
        corrupt=corrupt, suspects=suspects, **kw)
    _same(fast, M.apply(events, offsets, crc32c=CRC, **kw))
    return fast


def _splits(n):
    import test_grid_regimes as G
    return {"ones": G.ones(n), "ragged": G.ragged(n, empties=False), "empties": G.ragged(n)}


@pytest.mark.parametrize("split", ["ones", "ragged", "empties"])
def test_apply_fast_applies_what_apply_applies(split):
    import record_pool as R
    run, data = R.records(N_SMALL)
    first = _splits(N_SMALL)[split]
    flags = np.random.default_rng(5).integers(0, 256, size=N_SMALL, dtype=np.uint8)
    a = _both(run, data, first, _pool_kw(N_SMALL), flags=flags)
    assert np.array_equal(a.journal, run) and np.array_equal(a.data, data[40:40 + a.data.size])
    assert sorted(set(a.types.tolist())) == [1, 2, 3, 4, 5, 6] and a.result["n_bad"] == 0
    assert a.result["head_lease_id"] == 4 and len(set(a.flags.tolist())) == 32
    assert int(a.lengths.max()) == R.LONG[0]
    # from a head of (0, 0) too, and not from the last record's own
    _both(run, data, first, _pool_kw(N_SMALL, lease_id=0, seq=0))
    r = _both(run, data, first, _pool_kw(N_SMALL, seq=1))
    assert r[:1] + r[2:3] == (M.OUT_OF_SYNC, 0)


def test_apply_fast_counts_mismatches_like_apply():
    import record_pool as R
    run, data = R.records(N_SMALL)
    first = _splits(N_SMALL)["empties"]
    msgs = R.pool().msgs
    bad = run.copy()
    victims = msgs[[3, 700, 2000]]
    bad[60 * victims[:, None] + 52 + np.arange(4)] ^= np.array([0x80, 1, 0, 0x10], np.uint8)
    a = _both(bad, data, first, _pool_kw(N_SMALL))
    assert (a.result["n_bad"], a.result["first_bad"]) == (3, int(victims[0]))
    assert np.array_equal(a.journal, bad)
    # one payload byte of the long message: its true CRC is another
    long_rec = R.pool().long[0]
    at, lead, _, length, _ = R.data_fields(run, data, np.array([long_rec]))
    flipped = data.copy()
    flipped[int(at[0] + lead[0]) + 77777] ^= 0x20
    crcs = R.pool().crcs[:N_SMALL].copy()
    crcs[long_rec] = CRC(flipped[int(at[0] + lead[0]):int(at[0] + lead[0] + length[0])].tobytes())
    a = _both(run, flipped, first, _pool_kw(N_SMALL), crcs=crcs)
    assert (a.result["n_bad"], a.result["first_bad"]) == (1, long_rec)
    assert np.flatnonzero(a.data != data[40:40 + a.data.size]).size == 1


@pytest.mark.parametrize("what", C.WALK_PLANTS)
def test_apply_fast_refuses_the_walks_violations_like_apply(what):
    import record_pool as R
    run, data = R.records(N_SMALL)
    first = _splits(N_SMALL)["empties"]
    lay = M.layout_fast(run, data, first)
    msgs = R.pool().msgs
    lo, hi = int(msgs[600]), int(msgs[3000])            # two MESSAGE records, events apart
    assert lay.event[lo] + 2 < lay.event[hi] and first[lay.event[lo]] < lo
    at = (lambda i: int(lay.event[i])) if what in ("offsets", "event_length") else (lambda i: i)
    both = _both(run, data, first, _pool_kw(N_SMALL), [(what, at(hi)), (what, at(lo))])
    one = _both(run, data, first, _pool_kw(N_SMALL), [(what, at(hi))])
    kind = {"offsets": M.EVENT_OFFSETS, "event_length": M.EVENT_HEADER,
            "partition": M.STORAGE_HEADER, "padding": M.DATA_RECORD}[what]
    assert (both.kind, both.event) == (kind, lay.event[lo])
    assert (one.kind, one.event) == (kind, lay.event[hi])
    # a stopped walk reports the messages in front of the violation
    stopped = what in ("partition", "padding")
    # (the event in front of a late start ends late: refused too, it counts nothing)
    assert both.index == (lo if stopped else first[lay.event[lo] - (what == "offsets")])
    # a lower kind in a higher event beats a higher kind in a lower event
    if what != "offsets":
        lower = C.WALK_PLANTS[C.WALK_PLANTS.index(what) - 1]
        at_hi = int(lay.event[hi]) if lower in ("offsets", "event_length") else hi
        r = _both(run, data, first, _pool_kw(N_SMALL), [(what, at(lo)), (lower, at_hi)])
        assert (r.kind, r.event) == (kind - 1, lay.event[hi])


def test_apply_fast_refuses_what_the_checks_refuse_like_apply():
    import record_pool as R
    run, data = R.records(N_SMALL)
    splits = _splits(N_SMALL)
    first = splits["empties"]
    lay = M.layout_fast(run, data, first)
    msgs = R.pool().msgs
    kw = _pool_kw(N_SMALL)
    total = kw["data_dst_bytes"]
    # TOO_MANY_MESSAGES: inside an event, at an event's first message, one short
    for cap in (2000, int(first[40]), int(first[40]) - 1, N_SMALL - 1, 0):
        r = _both(run, data, first, dict(kw, msg_cap=cap))
        assert r.kind == M.TOO_MANY_MESSAGES and first[r.event] <= cap < first[r.event + 1]
    # OUT_OF_SYNC: a sequence gap, a DATA offset, a journal offset, two at once
    for at in (1, 2048, N_SMALL - 1):
        r = _both(C.sequence_gap(run, at), data, first, kw)
        assert (r.kind, r.index, r.event) == (M.OUT_OF_SYNC, at, lay.event[at])
    a, b = int(msgs[900]), int(msgs[2500])
    assert _both(run, data, first, kw, [("data_offset", b)])[:3] == (6, lay.event[b], b)
    assert _both(run, data, first, kw, [("journal_offset", 3999)])[:3] == (6, lay.event[3999],
                                                                           3999)
    r = _both(C.sequence_gap(run, 3000), data, first, kw, [("data_offset", a)])
    assert (r.kind, r.index) == (M.OUT_OF_SYNC, a)
    # DST_TOO_SMALL: the journal one byte short, the data one byte short, the
    # data ending inside the run; OUT_OF_SYNC first when both hold
    r = _both(run, data, first, dict(kw, journal_dst_bytes=60 * N_SMALL - 1))
    assert (r.kind, r.index) == (M.DST_TOO_SMALL, N_SMALL - 1)
    r = _both(run, data, first, dict(kw, data_dst_bytes=total - 1))
    assert (r.kind, r.index) == (M.DST_TOO_SMALL, int(msgs[msgs < N_SMALL][-1]))
    r = _both(run, data, first, dict(kw, data_dst_bytes=total // 2))
    assert r.kind == M.DST_TOO_SMALL and r.index in msgs and 0 < r.index < N_SMALL - 1
    r = _both(C.sequence_gap(run, 4000), data, first, dict(kw, data_dst_bytes=total // 2))
    assert (r.kind, r.index) == (M.OUT_OF_SYNC, 4000)
    # a refused message between two empty events: its event and StorageHeader
    at = int(first[20])
    assert first[21] > at + 1
    between = np.concatenate([first[:21], [at, at + 1, at + 1], first[21:]])
    r = _both(C.sequence_gap(run, at), data, between, kw)
    assert (r.kind, r.event, r.index) == (M.OUT_OF_SYNC, 21, at)
    assert r.offset == int(M.layout_fast(run, data, between).pos[at])
    # a new primary's lease from some record on is applied
    ok = _both(C.new_lease(run, 2048), data, first, kw)
    assert (ok.result["head_lease_id"], ok.result["head_seq"]) == (5, N_SMALL - 2048)
