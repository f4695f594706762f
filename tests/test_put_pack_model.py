"""The layout bmqcrc_put_event_pack (ABI 2.10) promises, restated in numpy
(tests/put_pack_model.py), against the byte-exact Python mirror of
PutEventBuilder and the native event walk.  CPU only."""
import numpy as np
import pytest

from blazingmq_amd.put_event import PutMessageIterator
import pack_pool
from put_pack_model import (EVT, HDR, host_crcs, layout, model_bytes, model_bytes_fast,
                            oracle_events, pad_of, pool_crcs, pooled_crcs, random_meta)

LENS = np.arange(68)  # 0..67: every padding count, many times over
CUTS = [None, [0, 68], [0, 1, 68], [0, 1, 2, 67, 68], [0, 17, 18, 40, 68], list(range(69))]


def _case(seed=0):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, size=4096, dtype=np.uint8)
    soff = rng.integers(0, 4096 - 67, size=LENS.size)
    return (src, soff, LENS) + random_meta(rng, LENS.size)


def test_padding_is_one_to_four_and_equals_its_count():
    assert set(pad_of(LENS)) == {1, 2, 3, 4}
    assert np.all((LENS + pad_of(LENS)) % 4 == 0) and np.all(pad_of(LENS[LENS % 4 == 0]) == 4)


@pytest.mark.parametrize("cuts", CUTS)
def test_model_is_byte_for_byte_the_builder(cuts):
    src, soff, lens, qids, guids, flags = _case()
    crcs = host_crcs(src, soff, lens)
    img = model_bytes(src, soff, lens, qids, guids, flags, cuts, crcs)
    events = oracle_events(src, soff, lens, qids, guids, flags, cuts)
    assert np.array_equal(img, np.concatenate(events))
    hdr, ev = layout(lens, cuts)
    assert [int(x) for x in np.diff(ev)] == [e.size for e in events]
    assert int(ev[-1]) == img.size and np.all(hdr % 4 == 0) and np.all(ev % 4 == 0)


@pytest.mark.parametrize("cuts", CUTS)
def test_model_through_the_native_walk(cuts):
    src, soff, lens, qids, guids, flags = _case(1)
    crcs = host_crcs(src, soff, lens)
    img = model_bytes(src, soff, lens, qids, guids, flags, cuts, crcs)
    hdr, ev = layout(lens, cuts)
    ef = [0, lens.size] if cuts is None else cuts
    for e in range(len(ef) - 1):
        at = int(ev[e])
        event = img[at:int(ev[e + 1])]
        off, ln, pos = PutMessageIterator(event).scan()
        sl = slice(ef[e], ef[e + 1])
        assert np.array_equal(off.astype(np.int64), hdr[sl] - at + HDR)
        assert np.array_equal(ln.astype(np.int64), lens[sl])
        assert np.array_equal(pos.astype(np.int64), hdr[sl] - at + 28)
        n_msgs = 0
        for i, m in zip(range(ef[e], ef[e + 1]), PutMessageIterator(event)):
            assert m["flags"] == int(flags[i]) and m["queue_id"] == int(qids[i])
            assert m["guid"] == bytes(guids[i]) and m["crc32c"] == int(crcs[i])
            assert m["app_data"] == src[int(soff[i]):int(soff[i]) + int(lens[i])].tobytes()
            n_msgs += 1
        assert n_msgs == ef[e + 1] - ef[e]


N_POOLED = pack_pool.POOL + 1100  # every pool pair, the long one included, and a second lap


def _pooled_case():
    src, soff, lens, ix = pack_pool.messages(N_POOLED)
    rng = np.random.default_rng(2)
    return (src, soff, lens) + random_meta(rng, N_POOLED), ix


@pytest.mark.parametrize("cuts,with_flags", [
    (None, True),
    ([0, N_POOLED], False),
    (list(range(0, N_POOLED, 3)) + [N_POOLED], True),        # events of 3, the last shorter
    (list(range(N_POOLED + 1)), False),                       # every message its own event
    ([0, 1, 2, 1024, 1025, 1500, 1501, 2048, N_POOLED - 1, N_POOLED], True)])
def test_fast_model_is_the_loop_model_and_the_builder(cuts, with_flags):
    (src, soff, lens, qids, guids, flags), ix = _pooled_case()
    assert set(pad_of(lens)) == {1, 2, 3, 4} and (lens == 0).any()
    assert int(lens[pack_pool.LONG_VISIT]) == pack_pool.LONG
    if not with_flags:
        flags = None
    crcs = pooled_crcs(pool_crcs(*pack_pool.pool()), ix)
    assert np.array_equal(crcs, host_crcs(src, soff, lens))
    fast = model_bytes_fast(src, soff, lens, qids, guids, flags, cuts, crcs)
    assert np.array_equal(fast, model_bytes(src, soff, lens, qids, guids, flags, cuts, crcs))
    assert np.array_equal(fast, np.concatenate(
        oracle_events(src, soff, lens, qids, guids, flags, cuts)))


def test_fast_model_of_nothing_and_of_one():
    src, soff, lens, ix = pack_pool.messages(1)
    qids, guids, flags = random_meta(np.random.default_rng(3), 1)
    crcs = host_crcs(src, soff, lens)
    assert np.array_equal(model_bytes_fast(src, soff, lens, qids, guids, flags, None, crcs),
                          model_bytes(src, soff, lens, qids, guids, flags, None, crcs))
    none = (src, soff[:0], lens[:0], qids[:0], guids[:0], None, None, crcs[:0])
    assert np.array_equal(model_bytes_fast(*none), model_bytes(*none))  # an empty event


def test_the_pool_holds_what_the_large_cases_rely_on():
    pack_pool.check_properties(pad_of)


def test_event_formulas():
    lens = np.array([0, 1, 2, 3, 4, 5], np.int64)
    hdr, ev = layout(lens, [0, 2, 3, 6])
    B = [40, 40, 40, 40, 44, 44]
    assert list(hdr) == [8, 48, 8 + 80 + 8, 8 + 120 + 16, 8 + 160 + 16, 8 + 204 + 16]
    assert list(ev) == [0, 8 + 80, 16 + 120, 24 + sum(B)]
    assert EVT == 8 and HDR == 36
