"""The device calls of bmqcrc_protocol.h with every pointer at the finest
alignment its header line allows.  Their own test files hand them buffers
that start an allocation (a multiple of 256 bytes); here every input,
destination and output array is a view inside a longer allocation
(tests/device_views.py) at a phase of its own, and each call goes through its
file's raw `_check` against its Python model: every output and destination
exactly, the guard elements behind every array, after a refusal every byte
unchanged -- and the sentinel margins in front of and behind every buffer.

Phases.  `events`, `journal`, `dst`, `journal_dst` (4-byte pointers) take 4,
8, 12, 60 and 124; `data` and `data_dst` (8-byte pointers) 8, 24, 72 and 120;
32-bit arrays lie at 4 or 12 mod 16, 64-bit arrays at 8 mod 16, byte arrays
at odd addresses.  Within a call no two pointers share a phase, and over the
five phase sets K every 4-byte pointer takes 4, 8 and 12 mod 16."""
import numpy as np
import pytest

import device_views as V
import journal_select_cases as JC
import journal_select_model as JM
import push_pack_cases as PPC
import push_pack_model as PPM
import storage_apply_cases as SAC
import storage_apply_model as SAM
import storage_pack_cases as SPC
import storage_pack_model as SPM
import put_unpack_model as PUM
import records_unpack_model as RUM
import test_gpu_journal_select as JS
import test_gpu_push_pack as PP
import test_gpu_put_pack as PK
import test_gpu_put_unpack as PU
import test_gpu_records_pack as RP
import test_gpu_records_unpack as RU
import test_gpu_storage_apply as SA
import test_gpu_storage_pack as SP
from blazingmq_amd import _native as N, last_journal_select, synth
from put_pack_model import layout as put_layout, random_meta as random_put_meta
from records_pack_model import (host_crcs as rp_crcs, layout as rp_layout,
                                random_meta as random_rec_meta)

pytestmark = pytest.mark.gpu

P4 = (4, 8, 12, 60, 124)                      # 4-byte pointers
P8 = (8, 24, 72, 120)                         # 8-byte pointers
A32 = (20, 28, 36, 44, 52, 76, 84, 92)        # 32-bit arrays: 4 or 12 mod 16
A64 = (40, 56, 88, 104, 136, 152)             # 64-bit arrays: 8 mod 16
ODD = (5, 7, 9, 11, 13, 15, 17, 19)           # byte arrays
K = range(5)
COUNTS = (1, 63, 64, 65, 1025)


def _phases(k, p4=(), p8=(), a32=(), a64=(), odd=()):
    """A phase for every named pointer, all different; set k of five."""
    out = {}
    for names, pool in ((p4, P4), (p8, P8), (a32, A32), (a64, A64), (odd, ODD)):
        assert len(names) <= len(pool)
        for i, name in enumerate(names):
            out[name] = pool[(i + k + (pool is P8)) % len(pool)]
    assert len(set(out.values())) == len(out)
    assert all(out[n] % 4 == 0 and out[n] % 16 for n in p4 + a32)
    assert all(out[n] % 16 == 8 for n in p8 + a64) and all(out[n] % 2 for n in odd)
    return out


def test_the_phase_sets_reach_every_residue():
    for names, pool, want in ((("a", "b", "c"), P4, {4, 8, 12}), (("a", "b"), P8, {8})):
        for i, name in enumerate(names):
            assert {pool[(i + k) % len(pool)] % 16 for k in K} == want
    assert {p % 16 for p in A32} == {4, 12} and {p % 16 for p in A64} == {8}


# ---- bmqcrc_storage_event_pack ------------------------------------------------------

def _sp(k):
    return _phases(k, p4=("journal", "dst"), p8=("data",), a32=("out",),
                   a64=("event_first", "event_offsets"), odd=("flags", "types"))


@pytest.mark.parametrize("k,count", list(enumerate(COUNTS)))
def test_storage_pack_record_counts(cuda, k, count):
    run, d = SP._records(1025)
    run = run[:60 * count]
    flags = (np.arange(count) * 37 % 256).astype(np.uint8)
    m, _ = SP._check(cuda, run, d, SP._kw(run, d, flags=flags, event_first=SP._cuts(count, 64)),
                     phases=_sp(k))
    assert m.result["n_msgs"] == count


@pytest.mark.parametrize("k", K)
def test_storage_pack_every_alignment(cuda, k):
    run, d = SP._records(700, seed=8, options=True)
    m, _ = SP._check(cuda, run, d, SP._kw(run, d, event_first=SP._cuts(700, 50)), phases=_sp(k))
    assert isinstance(m, SPM.Packed)


@pytest.mark.parametrize("k", [1, 2, 4])
def test_storage_pack_application_data_lengths(cuda, k):
    lengths = tuple(range(25)) + (255, 256, 257, 64 * 1024, 300 * 1024 + 3)
    run, d = SP._records(46, seed=9, lengths=lengths)
    m, _ = SP._check(cuda, run, d, SP._kw(run, d, event_first=SP._cuts(46, 17)), phases=_sp(k))
    assert m.result["n_data"] == len(lengths) and m.result["n_bad"] == 0


def test_storage_pack_a_flipped_payload_byte(cuda):
    run, d = SP._records(400)
    good = SPM.pack(run, d, crc32c=SP.CRC, **dict(SP._kw(run, d), dst_bytes=1 << 30))
    victim = int(np.flatnonzero((good.types == 1) & (good.crcs != 0))[40])
    o = 8 * int.from_bytes(run[60 * victim + 32:60 * victim + 36].tobytes(), "big")
    bad = d.copy()
    bad[o + 12] ^= 0x10
    m, host = SP._check(cuda, run, bad, SP._kw(run, d, event_first=SP._cuts(400, 33)),
                        phases=_sp(3))
    assert (m.result["n_bad"], m.result["first_bad"]) == (1, victim)
    assert np.flatnonzero(host["out"][:400] != m.expected).tolist() == [victim]


_SP_TABLE = [(t, name) for t, cases in (("refusal", SPC.refusal_cases()),
                                        ("precedence", SPC.precedence_cases()))
             for name in sorted(cases)]


@pytest.mark.parametrize("k,table,name", [(i % 5,) + c for i, c in enumerate(_SP_TABLE)])
def test_storage_pack_refusals(cuda, k, table, name):
    case = (SPC.refusal_cases() if table == "refusal" else SPC.precedence_cases())[name]
    for sync in (True, False):
        m, _ = SP._check(cuda, case.run, case.data, SP._kw(None, None, **case.kw), sync=sync,
                         phases=_sp(k))
        assert m == case.want


# ---- bmqcrc_storage_event_apply -----------------------------------------------------

def _sa(k):
    return _phases(k, p4=("events", "journal"), p8=("data",),
                   a32=("payload_lengths", "lengths", "expected", "out"),
                   a64=("event_offsets", "payload_offsets", "record_offsets", "event_first"),
                   odd=("types", "flags"))


@pytest.mark.parametrize("k,count", list(enumerate(COUNTS)))
def test_storage_apply_event_counts(cuda, k, count):
    # one message to an event (the scan's tile of 1,024 events) ...
    run, d = SA._records(1025)
    run = run[:60 * count]
    events, offsets = synth.storage_events(run, d, 0, SA.JH, 1, 1)
    assert offsets.size - 1 == count
    SA._check(cuda, events, offsets, dict(SA._exact(run, d), data_dst_bytes=d.size),
              phases=_sa(k))


@pytest.mark.parametrize("k,per_event", list(enumerate((1, 63, 64, 65, 130))))
def test_storage_apply_messages_per_event(cuda, k, per_event):
    # ... and the wave's 64 lanes, which place 64 messages of an event at a time
    run, d = SA._records(140)
    events, offsets = synth.storage_events(run, d, 0, SA.JH, 1, per_event)
    m, _ = SA._check(cuda, events, offsets, SA._exact(run, d), phases=_sa(k))
    assert m.event_first[1] == min(per_event, 140)


@pytest.mark.parametrize("k", K)
def test_storage_apply_every_alignment(cuda, k):
    run, d = SA._records(700, seed=8, options=True)
    events, offsets = SA._widen_event_headers(*synth.storage_events(run, d, 0, SA.JH, 1, 50))
    m, _ = SA._check(cuda, events, offsets, SA._exact(run, d), phases=_sa(k))
    assert isinstance(m, SAM.Applied)


@pytest.mark.parametrize("k", [0, 3])
def test_storage_apply_long_messages(cuda, k):
    # messages of 64 KiB and of 300 KiB + 3 among short ones: the copy's long path
    from blazingmq_amd import storage as S
    rng = np.random.default_rng(9)
    w = S.PartitionWriter(lease_id=4, partition_id=1)
    for size in tuple(range(25)) + (255, 256, 257, 64 * 1024, 300 * 1024 + 3):
        w.message(rng.integers(0, 256, size=size, dtype=np.uint8).tobytes(), S.DEFAULT_QUEUE_KEY)
    j, d = w.files()
    run = j[SA.JH:]
    events, offsets = synth.storage_events(run, d, 0, SA.JH, 1, 7)
    m, _ = SA._check(cuda, events, offsets, SA._exact(run, d), phases=_sa(k))
    assert m.result["n_bad"] == 0 and int(m.lengths.max()) == 300 * 1024 + 3


def test_storage_apply_a_flipped_payload_byte_and_a_flipped_stored_crc(cuda):
    run, d = SA._records(400)
    events, offsets = synth.storage_events(run, d, 0, SA.JH, 1, 33)
    good = SAM.apply(events, offsets, crc32c=SA.CRC, **SA._exact(run, d))
    data = np.flatnonzero((good.types == 1) & (good.lengths > 0))
    a, b = int(data[40]), int(data[-1])
    events[int(good.payload_offsets[a]) + 12] ^= 0x10          # application data
    events[int(good.payload_offsets[b]) - 60 + 55] ^= 0x01     # the MessageRecord's CRC
    m, host = SA._check(cuda, events, offsets, SA._exact(run, d), phases=_sa(2))
    assert (m.result["n_bad"], m.result["first_bad"]) == (2, a)
    assert list(np.flatnonzero(host["out"][:400] != host["expected"][:400])) == [a, b]


_SA_TABLE = [(t, name) for t, cases in (("refusal", SAC.refusal_cases()),
                                        ("precedence", SAC.precedence_cases()))
             for name in sorted(cases)]


@pytest.mark.parametrize("k,table,name", [(i % 5,) + c for i, c in enumerate(_SA_TABLE)])
def test_storage_apply_refusals(cuda, k, table, name):
    case = (SAC.refusal_cases() if table == "refusal" else SAC.precedence_cases())[name]
    for sync in (True, False):
        m, _ = SA._check(cuda, case.events, case.offsets, case.kw, sync=sync, phases=_sa(k))
        assert m == case.want


# ---- bmqcrc_push_event_pack ---------------------------------------------------------

def _pp(k):
    return _phases(k, p4=("journal", "dst"), p8=("data",),
                   a32=("records", "queue_ids", "sub_ids", "out", "lengths"),
                   a64=("event_first", "event_offsets"), odd=("flags", "rda"))


@pytest.mark.parametrize("k,count", list(enumerate(COUNTS)))
def test_push_pack_message_counts(cuda, k, count):
    run, d, _ = PP._messages(1025)
    run = run[:60 * count]
    kw = PP._kw(count, option_mode=3, rda=np.arange(count) % 256, sub_ids=np.arange(count) + 5,
                records=np.arange(count)[::-1], flags=np.arange(count) % 2 * 4,
                event_first=PP._cuts(count, 64))
    m, _ = PP._check(cuda, run, d, kw, phases=_pp(k))
    assert m.result["n_msgs"] == count


@pytest.mark.parametrize("k", K)
def test_push_pack_every_alignment(cuda, k):
    run, d, _ = PP._messages(700, seed=8, options=True)
    m, _ = PP._check(cuda, run, d, PP._kw(700, option_mode=1, rda=np.arange(700) % 256,
                                          event_first=PP._cuts(700, 50)), phases=_pp(k))
    assert isinstance(m, PPM.Packed)


@pytest.mark.parametrize("k,mode", [(1, 0), (2, 3), (4, 3)])
def test_push_pack_application_data_lengths(cuda, k, mode):
    lengths = tuple(range(25)) + (255, 256, 257, 64 * 1024, 300 * 1024 + 3)
    n = len(lengths)
    run, d, _ = PP._messages(n, seed=9, lengths=lengths)
    kw = PP._kw(n, option_mode=mode, event_first=PP._cuts(n, 17))
    if mode:
        kw.update(rda=np.arange(n), sub_ids=np.arange(n) + 5)
    m, _ = PP._check(cuda, run, d, kw, phases=_pp(k))
    assert m.lengths.tolist() == list(lengths) and m.result["n_bad"] == 0


def test_push_pack_a_corrupt_payload_and_a_corrupt_stored_crc(cuda):
    n = 400
    run, d, _ = PP._messages(n)
    good = PPM.pack(run, d, crc32c=PP.CRC, **dict(PP._kw(n), dst_bytes=1 << 30))
    victim = int(np.flatnonzero(good.lengths > 4)[40])
    other = victim + 123
    o = 8 * int.from_bytes(run[60 * victim + 32:60 * victim + 36].tobytes(), "big")
    bad, j = d.copy(), run.copy()
    bad[o + 12 + 3] ^= 0x10            # a bit rots in the payload
    j[60 * other + 52] ^= 0x80         # and one in a stored CRC
    m, host = PP._check(cuda, j, bad, PP._kw(n, event_first=PP._cuts(n, 33)), phases=_pp(3))
    assert (m.result["n_bad"], m.result["first_bad"]) == (2, victim)
    assert np.flatnonzero(host["out"][:n] != m.expected).tolist() == [victim, other]


_PP_TABLE = [(t, name) for t, cases in (("refusal", PPC.refusal_cases()),
                                        ("precedence", PPC.precedence_cases()))
             for name in sorted(cases)]


@pytest.mark.parametrize("k,table,name", [(i % 5,) + c for i, c in enumerate(_PP_TABLE)])
def test_push_pack_refusals(cuda, k, table, name):
    case = (PPC.refusal_cases() if table == "refusal" else PPC.precedence_cases())[name]
    for sync in (True, False):
        m, _ = PP._check(cuda, case.run, case.data, case.kw, sync=sync, phases=_pp(k))
        assert m == case.want


# ---- bmqcrc_put_event_pack ----------------------------------------------------------

def _pk(k):
    # (src and guids may sit at any byte)
    p = _phases(k, p4=("dst",), a32=("lengths", "queue_ids", "out"),
                a64=("src_offsets", "event_first", "event_offsets"), odd=("src", "flags"))
    p["guids"] = (1, 2, 3)[k % 3]
    return p


@pytest.mark.parametrize("k,count", list(enumerate(COUNTS)))
def test_put_pack_message_counts(cuda, k, count):
    rng = np.random.default_rng(count)
    ef = sorted({0, 1, count // 2, count - 1, count} - {-1}) if count > 1 else [0, 1]
    PK._check(cuda, *PK._short(rng, count, 0, 41), ef=ef, phases=_pk(k))


@pytest.mark.parametrize("k", K)
def test_put_pack_every_length_at_every_source_misalignment(cuda, k):
    # lengths 0..67 in one event: every padding count and every destination
    # alignment, at every source misalignment (on top of src's odd phase)
    rng = np.random.default_rng(1)
    lens = np.arange(68)
    src = rng.integers(0, 256, size=68 * 96 + 64, dtype=np.uint8)
    for mis in range(16):
        soff = 96 * np.arange(68) + mis + 16 * rng.integers(0, 2, size=68)
        qids, guids, flags = random_put_meta(rng, 68)
        PK._check(cuda, src, soff, rng.permutation(lens), qids, guids, flags, phases=_pk(k))


@pytest.mark.parametrize("k,own_event", [(0, False), (2, True), (4, True)])
def test_put_pack_a_long_message_among_short_ones(cuda, k, own_event):
    rng = np.random.default_rng(5)
    src, soff, lens, qids, guids, flags = PK._short(rng, 41, 0, 200, src_size=1 << 19)
    lens[20], soff[20] = 300 * 1024 + 3, 13  # longer than a 64 KiB chunk of the copy pass
    lens[7], soff[7] = 64 * 1024, 4099
    ef = [0, 20, 21, 41] if own_event else None
    PK._check(cuda, src, soff, lens, qids, guids, flags, ef, phases=_pk(k))


def test_put_pack_refusals(cuda):
    # test_gpu_put_pack.py's refusals, each sync and async, every buffer placed
    rng = np.random.default_rng(6)
    case, ef = PK._cap_case(rng, 52)
    PK._refused(cuda, N.BMQCRC_PUT_PACK_EVENT_TOO_BIG, 1, *case, ef=ef, max_event_bytes=4096,
                phases=_pk(0))
    PK._check(cuda, *case, ef=ef, max_event_bytes=4100, phases=_pk(0))
    case = PK._short(np.random.default_rng(7), 300)
    ef = [0, 100, 299, 300]
    total = int(put_layout(case[2], ef)[1][-1])
    PK._check(cuda, *case, ef=ef, slack=0, phases=_pk(1))                 # dst_bytes == total
    PK._refused(cuda, N.BMQCRC_PUT_PACK_DST_TOO_SMALL, 2, *case, ef=ef, dst_bytes=total - 4,
                phases=_pk(1))
    PK._refused(cuda, N.BMQCRC_PUT_PACK_DST_TOO_SMALL, 0, *case, ef=ef, dst_bytes=64,
                phases=_pk(2))
    src, soff, lens, qids, guids, flags = PK._short(np.random.default_rng(8), 1500,
                                                    src_size=1 << 15)
    src_bytes = 20000  # declared smaller than the view: a broken check stays inside it
    soff = soff % (src_bytes - 64)
    soff[1200], lens[1200] = src_bytes - 10, 11               # one byte past
    soff[1300] = (1 << 63) - 8                                 # the sum needs 64 bits
    soff[77], lens[77] = src_bytes, 0                          # empty at the very end: legal
    PK._refused(cuda, N.BMQCRC_PUT_PACK_SRC_RANGE, 1200, src, soff, lens, qids, guids, flags,
                src_bytes=src_bytes, phases=_pk(3))
    for k, (ef, index) in enumerate([([1, 5, 20], 0), ([0, 5, 5, 20], 1), ([0, 9, 5, 20], 1),
                                     ([0, 5, 19], 2), ([0, 5, 21], 2)]):
        PK._refused(cuda, N.BMQCRC_PUT_PACK_EVENT_FIRST, index,
                    *PK._short(np.random.default_rng(9), 20), ef=ef, phases=_pk(k))


# ---- bmqcrc_put_event_unpack --------------------------------------------------------

def _pu(k):
    p = _phases(k, p4=("events",), a32=("lengths", "queue_ids", "expected", "out"),
                a64=("event_offsets", "app_offsets", "event_first"), odd=("flags",))
    p["guids"] = (1, 2, 3)[k % 3]
    return p


@pytest.mark.parametrize("k,count", list(enumerate(COUNTS)))
def test_put_unpack_message_counts(cuda, k, count):
    rng = np.random.default_rng(count)
    ev = PUM.build_event(rng, rng.integers(0, 40, size=count))
    m, host = PU._ok(cuda, ev, np.array([0, ev.size]), cap=count, phases=_pu(k))
    assert np.array_equal(host["out"][:count], m["crcs"])


@pytest.mark.parametrize("k", K)
def test_put_unpack_every_window_position_and_header_variant(cuda, k):
    ev = PUM.ramp_event(np.random.default_rng(1))
    m, host = PU._ok(cuda, ev, None, phases=_pu(k))
    assert m["n"] == 1024 and np.array_equal(host["out"][:1024], m["crcs"])
    rng = np.random.default_rng(26)
    n = 70
    lens = rng.integers(0, 90, size=n)
    options = [PUM.payload(rng, 4 * int(x)) for x in rng.integers(0, 6, size=n)]
    plain = PUM.build_event(rng, lens)
    buf, offs = PUM.concat([PUM.long_event_header(plain), PUM.long_put_headers(plain),
                            PUM.build_event(rng, lens, options), PUM.with_cat_bits(plain)])
    m, host = PU._ok(cuda, buf, offs, phases=_pu(k))
    assert m["n"] == 4 * n and np.array_equal(host["out"][:4 * n], m["crcs"])


@pytest.mark.parametrize("k", [1, 3])
def test_put_unpack_long_messages_among_short_ones(cuda, k):
    rng = np.random.default_rng(22)
    ev = PUM.build_event(rng, [3, 5000, 0, 64 * 1024, 17, 5000, 300 * 1024 + 3, 1, 2])
    m, host = PU._ok(cuda, ev, None, phases=_pu(k))
    assert np.array_equal(host["out"][:9], m["crcs"])


def test_put_unpack_a_corrupt_payload(cuda):
    rng = np.random.default_rng(27)
    n = 200
    buf, offs = PUM.concat([PUM.build_event(rng, rng.integers(1, 120, size=100))
                            for _ in range(2)])
    good = PUM.model(buf, offs)
    victims = [0, 64, n - 1]
    bad = buf.copy()
    for v in victims:
        bad[int(good["app_offsets"][v])] ^= 0x10
    m, host = PU._ok(cuda, bad, offs, n_bad=3, first_bad=0, phases=_pu(2))
    assert list(np.nonzero(host["out"][:n] != host["expected"][:n])[0]) == victims
    assert np.array_equal(host["out"][:n], m["crcs"])


@pytest.mark.parametrize("k,name", [(i % 5, name) for i, name in enumerate(PUM.VARIANTS)])
def test_put_unpack_malformed_input(cuda, k, name):
    buf, offs = PUM.malformed(name)
    kind, event, _ = PU._refused(cuda, buf, offs, 64, phases=_pu(k))
    assert event == (2 if name == "offsets_past_end" else 1)
    assert kind == PUM.model(buf, offs)["refused"][0]


def test_put_unpack_refusal_precedence(cuda):
    rng = np.random.default_rng(30)
    good = PUM.build_event(rng, [4, 5, 6])
    pad, typ = PUM._mutate("padding_0", good), PUM._mutate("type_3", good)
    buf, offs = PUM.concat([good, pad, typ, typ])
    assert PU._refused(cuda, buf, offs, 64, phases=_pu(0))[:2] == (PUM.K_EVENT, 2)
    buf, offs = PUM.concat([pad, good, pad] + [good] * 40 + [pad])
    assert PU._refused(cuda, buf, offs, 256, phases=_pu(1))[:2] == (PUM.K_PAD, 0)
    buf, offs = PUM.concat([good, pad, good])
    assert PU._refused(cuda, buf, offs, 2, phases=_pu(2))[:2] == (PUM.K_PAD, 1)


# ---- bmqcrc_message_records_pack ----------------------------------------------------

def _rp(k):
    p = _phases(k, p4=("journal_dst",), p8=("dst",),
                a32=("lengths", "ref_counts", "expected", "out"),
                a64=("src_offsets", "timestamps", "record_offsets"),
                odd=("src", "queue_keys", "data_flags"))
    p["guids"] = (1, 2, 3)[k % 3]
    return p


@pytest.mark.parametrize("k,count", list(enumerate(COUNTS)))
def test_records_pack_message_counts(cuda, k, count):
    rng = np.random.default_rng(count)
    case = RP._short(rng, count, 0, 41)
    RP._check(cuda, *case, dict(RP._all_options(rng, count), expected=rp_crcs(*case[:3])),
              phases=_rp(k))


@pytest.mark.parametrize("k", K)
def test_records_pack_every_length_at_every_source_misalignment(cuda, k):
    rng = np.random.default_rng(1)
    lens = np.arange(40)
    src = rng.integers(0, 256, size=40 * 96 + 64, dtype=np.uint8)
    for mis in range(16):
        soff = 96 * np.arange(40) + mis + 16 * rng.integers(0, 2, size=40)
        qkeys, guids = random_rec_meta(rng, 40)
        RP._check(cuda, src, soff, rng.permutation(lens), qkeys, guids, RP._all_options(rng, 40),
                  phases=_rp(k))


@pytest.mark.parametrize("k", [0, 3])
def test_records_pack_long_messages_among_short_ones(cuda, k):
    rng = np.random.default_rng(5)
    src, soff, lens, qkeys, guids = RP._short(rng, 41, 0, 200, src_size=1 << 19)
    lens[20], soff[20] = 300 * 1024 + 3, 13
    lens[7], soff[7] = 64 * 1024, 4099
    RP._check(cuda, src, soff, lens, qkeys, guids, phases=_rp(k))


def test_records_pack_wrong_expected_crcs_are_counted(cuda):
    rng = np.random.default_rng(12)
    case = RP._short(rng, 1500, 0, 41)
    wrong = rp_crcs(*case[:3]).copy()
    for i in (1301, 64, 700):
        wrong[i] ^= 1 << (i % 32)
    RP._check(cuda, *case, dict(RP.KW, expected=wrong), n_bad=3, first_bad=64, phases=_rp(2))


def test_records_pack_refusals(cuda):
    # test_gpu_records_pack.py's refusals, each sync and async, every buffer placed
    rng = np.random.default_rng(6)
    src, soff, lens, qkeys, guids = RP._short(rng, 1300, src_size=1 << 12)
    lens[1234] = 0x80000000
    lens[1290] = 0xFFFFFFFF
    size = int(rp_layout(np.where(lens > 40, 0, lens))[1][-1]) + 64
    RP._refused(cuda, N.BMQCRC_REC_PACK_RECORD_TOO_BIG, 1234, src, soff, lens, qkeys, guids,
                size=size, phases=_rp(0))
    src, soff, lens, qkeys, guids = RP._short(np.random.default_rng(7), 1500, src_size=1 << 15)
    src_bytes = 20000
    soff = soff % (src_bytes - 64)
    soff[1200], lens[1200] = src_bytes - 10, 11               # one byte past
    soff[1300] = (1 << 63) - 8                                 # the sum needs 64 bits
    soff[77], lens[77] = src_bytes, 0                          # empty at the very end: legal
    RP._refused(cuda, N.BMQCRC_REC_PACK_SRC_RANGE, 1200, src, soff, lens, qkeys, guids,
                src_bytes=src_bytes, phases=_rp(1))
    case = RP._short(np.random.default_rng(8), 2300)
    Q = rp_layout(case[2])[1]
    total = int(Q[-1])
    RP._check(cuda, *case, slack=0, phases=_rp(2))             # dst_bytes == total
    RP._refused(cuda, N.BMQCRC_REC_PACK_DST_TOO_SMALL, 2299, *case, dst_bytes=total - 1,
                phases=_rp(2))
    RP._refused(cuda, N.BMQCRC_REC_PACK_DST_TOO_SMALL, 1024, *case, dst_bytes=int(Q[1025]) - 8,
                phases=_rp(3))
    RP._refused(cuda, N.BMQCRC_REC_PACK_DST_TOO_SMALL, 0, *case, dst_bytes=8, phases=_rp(4))
    rng = np.random.default_rng(9)
    src = rng.integers(0, 256, size=256, dtype=np.uint8)
    qkeys, guids = random_rec_meta(rng, 5)
    kw = dict(RP.KW, data_file_pos=8 * ((1 << 32) - 1) - 64)   # 64 bytes of file are left
    RP._refused(cuda, N.BMQCRC_REC_PACK_DATA_FILE_FULL, 4, src, np.arange(5) * 9,
                np.array([0, 1, 2, 3, 4]), qkeys, guids, kw, phases=_rp(0))
    # two kinds at once report the lowest
    src, soff, lens, qkeys, guids = RP._short(np.random.default_rng(10), 1100, src_size=1 << 12)
    soff[1050] = 1 << 40
    RP._refused(cuda, N.BMQCRC_REC_PACK_SRC_RANGE, 1050, src, soff, lens, qkeys, guids,
                dst_bytes=int(rp_layout(lens)[1][3]) + 8, phases=_rp(1))
    soff[1050] = 0
    RP._refused(cuda, N.BMQCRC_REC_PACK_DST_TOO_SMALL, 3, src, soff, lens, qkeys, guids,
                dict(RP.KW, data_file_pos=8 * ((1 << 32) - 1) - 8),
                dst_bytes=int(rp_layout(lens)[1][3]) + 8, phases=_rp(3))


# ---- bmqcrc_message_records_unpack --------------------------------------------------

def _ru(k):
    p = _phases(k, p4=("journal",), p8=("data",),
                a32=("record_index", "lengths", "ref_counts", "expected", "out"),
                a64=("app_offsets", "timestamps"), odd=("select", "queue_keys", "data_flags"))
    p["guids"] = (1, 2, 3)[k % 3]
    return p


@pytest.mark.parametrize("k,count", list(enumerate(COUNTS)))
def test_records_unpack_record_counts(cuda, k, count):
    run, d = RU._base()
    m, _ = RU._ok(cuda, run[:RUM.REC * count], d, cap=None, select=np.ones(count, np.uint8),
                  phases=_ru(k))
    assert 0 < m["n"] <= count


@pytest.mark.parametrize("k", K)
def test_records_unpack_header_sizes_and_every_alignment(cuda, k):
    rng = np.random.default_rng(44)
    j, d = RUM.build_partition(rng, rng.integers(0, 200, size=150), variants=True)
    m, _ = RU._ok(cuda, j[RUM.JH:], d, phases=_ru(k))
    gap = m["app_offsets"].astype(np.int64)[1:] - m["app_offsets"].astype(np.int64)[:-1]
    assert m["n"] == 150 and len(set(int(g) % 8 for g in gap)) > 1


@pytest.mark.parametrize("k", [1, 4])
def test_records_unpack_long_messages_among_short_ones(cuda, k):
    rng = np.random.default_rng(43)
    j, d = RUM.build_partition(rng, [3, 100, 64 * 1024, 0, 300 * 1024 + 3, 17], others=0.5)
    m, _ = RU._ok(cuda, j[RUM.JH:], d, phases=_ru(k))
    assert list(m["lengths"]) == [3, 100, 64 * 1024, 0, 300 * 1024 + 3, 17]


def test_records_unpack_a_corrupt_payload_and_a_corrupt_stored_crc(cuda):
    run, d = RU._base()
    run, d = run[:RUM.REC * 400].copy(), d.copy()
    good = RUM.model(run, d)
    n = good["n"]
    a = next(i for i in range(70, n) if good["lengths"][i] > 0)
    b = n - 1
    d[int(good["app_offsets"][a])] ^= 0x10
    run[RUM.REC * int(good["record_index"][b]) + 55] ^= 0x01
    m, host = RU._ok(cuda, run, d, n_bad=2, first_bad=a, phases=_ru(3))
    assert list(np.nonzero(host["out"][:n] != host["expected"][:n])[0]) == [a, b]
    assert np.array_equal(host["out"][:n], m["crcs"])


@pytest.mark.parametrize("k,name", [(i % 5, name) for i, name in enumerate(RUM.VARIANTS)])
def test_records_unpack_malformed_input(cuda, k, name):
    j, d, last = RUM.malformed(name)
    kind, index = RU._refused(cuda, j[RUM.JH:], d, phases=_ru(k))
    assert index == last and kind == RUM.VARIANT_KIND.get(name, RUM.K_DATA)


def test_records_unpack_refusal_precedence(cuda):
    run, d = RU._base()
    run, d = run[:RUM.REC * 2100].copy(), d.copy()
    msgs = RUM.message_records(run)
    lo, mid, hi = int(msgs[3]), int(msgs[msgs >= 1100][0]), int(msgs[msgs >= 2050][0])
    o = 8 * int.from_bytes(run[RUM.REC * lo + 32:RUM.REC * lo + 36].tobytes(), "big")
    d[o] &= 0x1F                                            # kind 4, the lowest record
    run[RUM.REC * hi + 22:RUM.REC * hi + 27] = 0            # kind 2, the highest
    RU._put32(run, RUM.REC * mid + 32, 0)                   # kind 3 between them
    assert RU._refused(cuda, run, d, phases=_ru(0)) == (RUM.K_MESSAGE, hi)
    run[RUM.REC * mid + 36:RUM.REC * mid + 52] = 0          # kind 2 at a lower index
    assert RU._refused(cuda, run, d, phases=_ru(1)) == (RUM.K_MESSAGE, mid)
    assert RU._refused(cuda, run, d, cap=1, phases=_ru(2)) == (RUM.K_MESSAGE, mid)
    run[RUM.REC * 2000 + 59] ^= 1                           # kind 1 beats them all
    assert RU._refused(cuda, run, d, phases=_ru(4)) == (RUM.K_HEADER, 2000)


# ---- bmqcrc_journal_select ----------------------------------------------------------

def _select(cuda, j, d, csl, keys, k, queue_cap=1 << 16):
    """The raw call with `journal` at a 4-byte phase, `queue_keys` and `select`
    at odd ones (select with guard bytes behind it), sync and async, held to
    the native host walk and the model like test_gpu_journal_select.py's
    _hold.  Returns the synchronous result."""
    import ctypes
    import torch
    run, _ = JM.record_run(j)
    n = len(run) // 60
    sel, want_rc, want_err = JM.host_view(j, d, with_csl=csl, queue_keys=keys)
    m = JM.select_model(run, d.size, with_csl=csl, queue_keys=keys)
    stream = torch.cuda.current_stream(cuda)
    for sync in (True, False):
        place = V.Placer(cuda, _phases(k, p4=("journal",), odd=("queue_keys", "select")))
        d_run = place.put("journal", np.array(run, dtype=np.uint8))
        select = place.fill("select", n + 8, np.uint8, 0xA5)
        p = N.JournalSelect()
        p.struct_size = ctypes.sizeof(N.JournalSelect)
        p.journal, p.journal_bytes = d_run.data_ptr(), d_run.numel()
        p.n_records, p.data_file_bytes, p.with_csl = n, d.size, 1 if csl else 0
        if keys:
            d_keys = place.put("queue_keys", np.frombuffer(b"".join(bytes(x) for x in keys), np.uint8).copy())
            p.queue_keys, p.n_queue_keys = d_keys.data_ptr(), len(keys)
        p.queue_cap, p.select = queue_cap, select.data_ptr()
        o = N.make_opts(device=cuda.index, stream=stream.cuda_stream,
                        flags=N.BMQCRC_F_DEVICE_PTRS | (0 if sync else N.BMQCRC_F_ASYNC))
        r = N.JournalSelectResult()
        rc = N.lib.bmqcrc_journal_select(ctypes.byref(p), ctypes.byref(r), ctypes.byref(o))
        assert rc == 0, N.lib.bmqcrc_last_error()
        res = r.as_dict() if sync else last_journal_select(cuda.index, stream)
        got = select.cpu().numpy()
        place.check()
        assert (got[n:] == 0xA5).all()                       # the guard bytes
        assert np.flatnonzero(got[:n]).tolist() == sel and set(np.unique(got[:n])) <= {0, 1}
        assert (res["recovery_rc"], res["error_record"]) == (want_rc, want_err)
        assert (res["n_records"], res["n_selected"], res["refused_kind"]) == (n, len(sel), 0)
        assert np.array_equal(got[:n], m["select"])
        assert {f: res[f] for f in ("first_record", "n_selected", "n_deleted", "n_purged")} == \
            {f: m[f] for f in ("first_record", "n_selected", "n_deleted", "n_purged")}
        if sync:
            first = res
    return first


@pytest.mark.parametrize("k,name", [(i % 5, name) for i, name in enumerate(JC.ALL)])
def test_journal_select_equals_the_host_walk(cuda, k, name):
    j, d, csl, keys = JC.case(name)
    _select(cuda, j, d, csl, tuple(keys), k)


@pytest.mark.parametrize("k,n", list(enumerate(COUNTS)))
def test_journal_select_wave_and_block_edges(cuda, k, n):
    j, d, _ = JS._long_run()
    _select(cuda, j[:44 + 60 * n], d, False, (), k)


def test_journal_select_too_many_queues(cuda):
    # the call's one refusal, sync and async: select all zero behind and in
    # front of intact margins
    import ctypes
    import torch
    j, d = JS.rich_partition()[:2]          # QueueOp records of Q1, Q2 and Q3
    run = np.array(JM.record_run(j)[0], dtype=np.uint8)
    n = run.size // 60
    stream = torch.cuda.current_stream(cuda)
    for k, sync in ((1, True), (2, False)):
        place = V.Placer(cuda, _phases(k, p4=("journal",), odd=("select",)))
        d_run = place.put("journal", run)
        select = place.fill("select", n + 8, np.uint8, 0xA5)
        p = N.JournalSelect()
        p.struct_size = ctypes.sizeof(N.JournalSelect)
        p.journal, p.journal_bytes, p.n_records = d_run.data_ptr(), d_run.numel(), n
        p.data_file_bytes, p.queue_cap, p.select = d.size, 2, select.data_ptr()
        o = N.make_opts(device=cuda.index, stream=stream.cuda_stream,
                        flags=N.BMQCRC_F_DEVICE_PTRS | (0 if sync else N.BMQCRC_F_ASYNC))
        r = N.JournalSelectResult()
        rc = N.lib.bmqcrc_journal_select(ctypes.byref(p), ctypes.byref(r), ctypes.byref(o))
        assert rc == (N.BMQCRC_EINVAL if sync else 0)
        assert last_journal_select(cuda.index, stream) == dict(
            n_records=n, first_record=n, n_selected=0, n_deleted=0, n_purged=0, error_record=n,
            recovery_rc=0, refused_kind=1)
        got = select.cpu().numpy()
        assert not got[:n].any() and (got[n:] == 0xA5).all()
        place.check()


# ---- the chains, through the Python wrappers ----------------------------------------

def _blank(cuda, size, phase):
    return V.place(np.full(size, 0xA5, np.uint8), phase, cuda)


def test_put_in_to_push_out_with_every_supplied_buffer_shifted(cuda):
    # test_gpu_push_pack.py::test_put_in_to_push_out_on_one_device; every
    # buffer the test supplies, the destinations included, is a shifted view
    import torch
    from blazingmq_amd import (pack_push_events, pack_records, select_records, unpack_events,
                               unpack_records)
    from blazingmq_amd import push_event as E, storage as S
    rng = np.random.default_rng(63)
    n = 300
    buf, evoffs = PUM.concat([PUM.build_event(rng, rng.integers(1, 400, size=100))
                              for _ in range(3)])
    pm = PUM.model(buf, evoffs)
    events = V.place(buf, 12, cuda)
    d_evoffs = V.place(np.asarray(evoffs, np.int64), 40, cuda)
    u = unpack_events(events, d_evoffs, msg_cap=n)
    qkeys = V.place(np.tile(np.frombuffer(PP.QK, np.uint8), (n, 1)), 5, cuda)
    w = S.PartitionWriter(lease_id=7)
    w.queue_op(S.OP_CREATION, PP.QK)
    jfile, _ = w.files()
    # the journal's record run: the CREATION record, then what pack_records writes
    journal = _blank(cuda, 60 * (n + 1), 60)
    journal[:60] = torch.from_numpy(jfile[PP.JH:].copy()).to(cuda)
    data = _blank(cuda, int(rp_layout(pm["lengths"])[1][-1]), 72)
    placed = [events, d_evoffs, qkeys, journal, data]
    assert [V.phase_of(v) for v in placed] == [12, 40, 5, 60, 72]
    assert journal[60:].data_ptr() % 16 == 8
    dst, jour, _, _, res = pack_records(events, u.app_offsets, u.lengths, qkeys, u.guids,
                                        expected=u.expected, file_key=b"\x11\x22\x33\x44\x55",
                                        lease_id=7, first_seq=2, data_file_pos=40, dst=data,
                                        journal_dst=journal[60:])
    assert res["data_bytes"] == data.numel() and res["n_bad"] == 0
    select, sel = select_records(journal, data_file_bytes=40 + data.numel())
    r = unpack_records(journal, data, data_file_pos=40, select=select, verify=True)
    assert sel["recovery_rc"] == 0 and r.record_index.numel() == n
    first = V.place(PP._cuts(n, 64), 56, cuda)
    kw = dict(data_file_pos=40, records=r.record_index, queue_ids=u.queue_ids,
              option_mode=E.OPTION_SUB_QUEUE_ID, sub_ids=u.queue_ids, event_first=first)
    sized = pack_push_events(journal, data, **kw)
    push = _blank(cuda, sized.events.numel(), 124)
    assert (V.phase_of(first), V.phase_of(push)) == (56, 124)
    p = pack_push_events(journal, data, dst=push, **kw)
    assert p.result == sized.result and torch.equal(push, sized.events)
    assert p.result["n_bad"] == 0 and p.result["n_msgs"] == n and p.result["n_events"] == 5
    out, offs = push.cpu().numpy(), p.event_offsets.cpu().numpy()
    got = [m for e in range(5)
           for m in E.PushMessageIterator(out[int(offs[e]):int(offs[e + 1])])]
    assert len(got) == n
    for i, m in enumerate(got):
        at, ln = int(pm["app_offsets"][i]), int(pm["lengths"][i])
        assert m["payload"] == buf[at:at + ln].tobytes()
        assert m["guid"] == pm["guids"][i].tobytes() and m["queue_id"] == int(pm["queue_ids"][i])
    assert np.array_equal(p.crcs.cpu().numpy().view(np.uint32), pm["crcs"])
    V.check_margins(*placed, first, push)


def test_a_partitions_whole_life_with_every_supplied_buffer_shifted(cuda):
    # test_gpu_storage_pack.py::test_a_partitions_whole_life_on_one_device;
    # every buffer the test supplies, the destinations included, is a shifted view
    import torch
    from blazingmq_amd import (apply_events, last_records_unpack, pack_records,
                               pack_storage_events, select_records, unpack_records)
    from blazingmq_amd import storage as S
    rng = np.random.default_rng(62)
    lens = rng.integers(0, 701, size=300).astype(np.uint32)
    n = lens.size
    soff = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    src = rng.integers(0, 256, size=int(lens.sum()), dtype=np.uint8)
    qkeys, guids = random_rec_meta(rng, n)
    qkeys[:] = np.frombuffer(SP.QK, np.uint8)
    w = S.PartitionWriter(lease_id=7, partition_id=2)
    w.queue_op(S.OP_CREATION, SP.QK)
    jfile, dfile = w.files()
    total = int(rp_layout(lens)[1][-1])
    for corrupt in (False, True):
        ins = [V.place(src, 7, cuda), V.place(soff, 88, cuda), V.place(lens, 20, cuda),
               V.place(qkeys, 9, cuda), V.place(guids, 3, cuda)]
        journal, data = _blank(cuda, 60 * (n + 1), 4), _blank(cuda, total, 120)
        journal[:60] = torch.from_numpy(jfile[SP.JH:].copy()).to(cuda)
        assert [V.phase_of(v) for v in ins + [journal, data]] == [7, 88, 20, 9, 3, 4, 120]
        dst, jour, roff, _, _ = pack_records(*ins, file_key=b"\x11\x22\x33\x44\x55", lease_id=7,
                                             first_seq=2, data_file_pos=40, dst=data,
                                             journal_dst=journal[60:])
        victim = 123
        if corrupt:   # a bit rots in the primary's HBM after the record was written
            assert lens[victim] > 5
            data[int(roff[victim].item()) + 12 + 5] ^= 0x04
        want = S.verify_partition(np.concatenate([jfile[:SP.JH], journal.cpu().numpy()]),
                                  np.concatenate([dfile, data.cpu().numpy()]))
        first = V.place(SP._cuts(n + 1, 25), 104, cuda)
        kw = dict(journal_pos=SP.JH, data_file_pos=40, partition_id=2, event_first=first)
        sized = pack_storage_events(journal, data, **kw)
        events = _blank(cuda, sized.events.numel(), 8)
        p = pack_storage_events(journal, data, dst=events, **kw)
        assert p.result == sized.result and torch.equal(events, sized.events)
        assert p.result["n_bad"] == int(corrupt)
        assert p.result["first_bad"] == (victim + 1 if corrupt else n + 1)
        replica_j, replica_d = _blank(cuda, 60 * (n + 1), 12), _blank(cuda, total, 24)
        assert [V.phase_of(v) for v in (first, events, replica_j, replica_d)] == [104, 8, 12, 24]
        a = apply_events(events, p.event_offsets, partition_id=2, journal_pos=SP.JH,
                         data_file_pos=40, journal_dst=replica_j, data_dst=replica_d)
        assert a.result["n_bad"] == int(corrupt) and a.result["n_msgs"] == n + 1
        assert torch.equal(replica_j, journal) and torch.equal(replica_d, data)
        select, sel = select_records(replica_j, data_file_bytes=40 + replica_d.numel())
        u = unpack_records(replica_j, replica_d, data_file_pos=40, select=select, verify=True)
        res = last_records_unpack(cuda.index, torch.cuda.current_stream(cuda))
        assert (sel["recovery_rc"], res["refused_kind"]) == (want["recovery_rc"], 0) == (0, 0)
        assert (res["n_msgs"], res["n_bad"]) == (want["n_messages"], want["n_bad"])
        assert want["n_messages"] == n and want["n_bad"] == int(corrupt)
        if corrupt:
            index = int(u.record_index[res["first_bad"]].item())
            assert list(want["bad_record_offsets"]) == [SP.JH + 60 * index] and index == victim + 1
        V.check_margins(*ins, journal, data, first, events, replica_j, replica_d)
