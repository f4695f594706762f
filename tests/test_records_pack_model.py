"""The layout bmqcrc_message_records_pack (ABI 2.11) promises, restated in
numpy (tests/records_pack_model.py), against PartitionWriter, the native
journal walk and the two MESSAGE records of the reference's own fixture
partition.  CPU only."""
import numpy as np
import pytest

from blazingmq_amd import pack_records  # noqa: F401  (ABI 2.11: absent before it)
from blazingmq_amd import storage as S
import pack_pool
from records_pack_model import (DH, REC, golden_case, host_crcs, layout, model_bytes,
                                model_bytes_fast, oracle_bytes, pad_of, pool_crcs, pooled_crcs,
                                random_meta, wrap_partition)

LENS = np.arange(40)  # 0..39: every padding count five times
KW = dict(file_key=bytes(5), lease_id=7, first_seq=2, data_file_pos=40, timestamp=0x6720EAB4)


def _case(seed=0):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, size=4096, dtype=np.uint8)
    lens = rng.permutation(LENS)
    soff = rng.integers(0, 4096 - 40, size=lens.size)
    return (src, soff, lens) + random_meta(rng, lens.size)


def test_padding_is_one_to_eight_and_equals_its_count():
    assert set(pad_of(LENS)) == set(range(1, 9))
    R, Q = layout(LENS)
    assert np.all(R % 8 == 0) and np.all(Q % 8 == 0) and np.all(pad_of(LENS[LENS % 8 == 4]) == 8)
    assert list(R[:5]) == [16, 16, 16, 16, 24] and int(Q[-1]) == int(R.sum())


@pytest.mark.parametrize("variant", ["plain", "ref_counts", "file_key", "data_flags",
                                     "timestamps", "all"])
def test_model_is_byte_for_byte_the_partition_writer(variant):
    src, soff, lens, qkeys, guids = _case()
    n = lens.size
    kw = dict(KW)
    if variant in ("ref_counts", "all"):
        kw["ref_counts"] = np.resize(np.array([1, 4095, 4096, (1 << 20) - 1], np.uint32), n)
    if variant in ("file_key", "all"):
        kw["file_key"] = b"\x9a\x00\xff\x01\x7e"
    if variant in ("data_flags", "all"):
        kw["data_flags"] = (np.arange(n) % 2).astype(np.uint8)
    if variant in ("timestamps", "all"):
        kw["timestamps"] = (1 << 40) + 3 * np.arange(n)
    if variant == "all":
        kw.update(first_seq=(1 << 48) - n, data_file_pos=(1 << 32) - 64, lease_id=0xFEDCBA98)
    crcs = host_crcs(src, soff, lens)
    data, jour = model_bytes(src, soff, lens, qkeys, guids, crcs, **kw)
    odata, ojour = oracle_bytes(src, soff, lens, qkeys, guids, crcs, **kw)
    assert np.array_equal(data, odata) and np.array_equal(jour, ojour)
    assert data.size == int(layout(lens)[1][-1]) and jour.size == REC * n


N_POOLED = pack_pool.POOL + 1100  # every pool pair, the long one included, and a second lap


@pytest.mark.parametrize("variant", ["plain", "ref_counts", "data_flags", "timestamps", "all",
                                     "expected", "seq_past_32_bits", "offset_across_2_31"])
def test_fast_model_is_the_loop_model_and_the_partition_writer(variant):
    src, soff, lens, ix = pack_pool.messages(N_POOLED)
    n = N_POOLED
    rng = np.random.default_rng(4)
    qkeys, guids = random_meta(rng, n)
    assert set(pad_of(lens)) == set(range(1, 9)) and (lens == 0).any()
    assert int(lens[pack_pool.LONG_VISIT]) == pack_pool.LONG
    kw = dict(KW)
    if variant in ("ref_counts", "all"):
        kw["ref_counts"] = rng.choice(np.array([1, 2, 4095, 4096, (1 << 20) - 1], np.uint32), n)
    if variant in ("data_flags", "all"):
        kw["data_flags"] = rng.integers(0, 256, size=n, dtype=np.uint8)
    if variant in ("timestamps", "all"):
        kw["timestamps"] = rng.integers(1, 1 << 62, size=n, dtype=np.int64)
    if variant == "all":
        kw.update(file_key=b"\x9a\x00\xff\x01\x7e", lease_id=0xFEDCBA98)
    if variant in ("seq_past_32_bits", "all"):
        kw["first_seq"] = (1 << 32) - 1000       # the high half changes inside the run
    Q = layout(lens)[1]
    if variant == "offset_across_2_31":
        kw["data_file_pos"] = (1 << 34) - int(Q[n // 2])
    crcs = pooled_crcs(pool_crcs(*pack_pool.pool()), ix)
    assert np.array_equal(crcs, host_crcs(src, soff, lens))
    stored = crcs
    if variant == "expected":
        stored = crcs ^ (np.arange(n) % 7 == 3).astype(np.uint32)  # not the computed CRC
        assert int((stored != crcs).sum()) > 500
    data, jour = model_bytes_fast(src, soff, lens, qkeys, guids, stored, **kw)
    if variant == "offset_across_2_31":
        dw = jour.reshape(n, REC)[:, 32:36]
        assert dw[0, 0] == 0x7F and dw[n // 2 - 1, 0] == 0x7F and dw[n // 2, 0] == 0x80
    for other in (model_bytes, oracle_bytes):
        d, j = other(src, soff, lens, qkeys, guids, stored, **kw)
        assert np.array_equal(data, d) and np.array_equal(jour, j), other.__name__
    assert data.size == int(Q[-1]) and jour.size == REC * n


def test_fast_model_of_nothing():
    src, soff, lens, ix = pack_pool.messages(0)
    data, jour = model_bytes_fast(src, soff, lens, np.zeros((0, 5), np.uint8),
                                  np.zeros((0, 16), np.uint8), np.zeros(0, np.uint32), **KW)
    assert data.size == 0 and jour.size == 0


def test_the_pool_holds_what_the_large_cases_rely_on():
    pack_pool.check_properties(pad_of)


def test_defaults_of_the_writer_are_todays_bytes():
    # the keywords added to PartitionWriter.message change nothing when left out
    w = S.PartitionWriter()
    w.message(b"abcde", b"\x01\x02\x03\x04\x05")
    j, d = w.files()
    r = j[44:104]
    assert r[0] == 0x10 and r[1] == 0x01 and r[20] == 0 and r[21] == 0
    assert r[27:32].tobytes() == bytes(5) and r[12:20].tobytes() == (0x6720EAB4).to_bytes(8, "big")
    assert d[40:52].tobytes() == ((3 << 29) | 6).to_bytes(4, "big") + bytes(8)


def test_model_through_the_native_walk():
    src, soff, lens, qkeys, guids = _case(1)
    qkeys[:] = qkeys[0]  # one queue: the CREATION record in front names it
    crcs = host_crcs(src, soff, lens)
    data, jour = model_bytes(src, soff, lens, qkeys, guids, crcs, **dict(KW, lease_id=1))
    jf, df = wrap_partition(data, jour, qkeys[0])
    got = S.scan_partition(jf, df)
    assert got["recovery_rc"] == 0 and got["record_offset"].size == lens.size
    Q = layout(lens)[1]
    order = slice(None, None, -1)  # the walk runs backward
    assert np.array_equal(got["record_offset"].astype(np.int64),
                          (44 + 60 + REC * np.arange(lens.size))[order])
    assert np.array_equal(got["app_offset"].astype(np.int64), (40 + Q[:-1] + DH)[order])
    assert np.array_equal(got["app_length"].astype(np.int64), lens[order])
    assert np.array_equal(got["crc32c"], crcs[order])


@pytest.mark.parametrize("k", [0, 1])
def test_model_reproduces_the_reference_fixture(k):
    src, soff, lens, qkeys, guids, crc, kw, want_data, want_rec = golden_case(k)
    assert (kw["lease_id"], kw["first_seq"]) == ((1, 4), (2, 2))[k]
    data, jour = model_bytes(src, soff, lens, qkeys, guids, crc, **kw)
    assert np.array_equal(data, want_data) and np.array_equal(jour, want_rec)
    # the CRC the broker stored is the payload's own
    assert int(host_crcs(src, soff, lens)[0]) == int(crc[0])
