"""The layout bmqcrc_put_event_pack (ABI 2.10) promises, restated in numpy
(tests/put_pack_model.py), against the byte-exact Python mirror of
PutEventBuilder and the native event walk.  CPU only."""
import numpy as np
import pytest

from blazingmq_amd.put_event import PutMessageIterator
from put_pack_model import (EVT, HDR, host_crcs, layout, model_bytes, oracle_events, pad_of,
                            random_meta)

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


def test_event_formulas():
    lens = np.array([0, 1, 2, 3, 4, 5], np.int64)
    hdr, ev = layout(lens, [0, 2, 3, 6])
    B = [40, 40, 40, 40, 44, 44]
    assert list(hdr) == [8, 48, 8 + 80 + 8, 8 + 120 + 16, 8 + 160 + 16, 8 + 204 + 16]
    assert list(ev) == [0, 8 + 80, 16 + 120, 24 + sum(B)]
    assert EVT == 8 and HDR == 36
