"""tests/records_unpack_model.py pinned to things other than the code under
test (CPU only): the host recovery walk (storage.scan_partition, reversed:
it walks backward), the reference's fixture partition, and for every refusal
the host walk's recovery_rc and error_record_offset."""
import os

import numpy as np
import pytest

from blazingmq_amd import storage as S
import records_unpack_model as M
from records_pack_model import GOLDEN, GOLDEN_RECORDS, golden_case

# what the device call must offer for the model to be its oracle
from blazingmq_amd import last_records_unpack, unpack_records  # noqa: F401


@pytest.mark.parametrize("seed,count,variants", [(1, 1, False), (2, 70, False), (3, 300, True),
                                                 (4, 40, True)])
def test_model_equals_the_host_walk_reversed(seed, count, variants):
    rng = np.random.default_rng(seed)
    j, d = M.build_partition(rng, rng.integers(0, 300, size=count), variants=variants)
    run = j[M.JH:]
    types = set(int(t) for t in run.reshape(-1, M.REC)[:, 0] >> 4)
    assert types <= {S.REC_MESSAGE, S.REC_CONFIRM, S.REC_QUEUE_OP, S.REC_JOURNAL_OP}
    if count >= 40:
        assert types == {S.REC_MESSAGE, S.REC_CONFIRM, S.REC_QUEUE_OP, S.REC_JOURNAL_OP}
    host = S.scan_partition(j, d)
    assert host["recovery_rc"] == 0
    # the host walk returns every MESSAGE record: the selection is all of them
    assert host["record_offset"].size == M.message_records(run).size == count
    m = M.model(run, d)
    assert m["refused"] is None and m["n"] == count and m["n_skipped"] == 0
    assert np.array_equal(M.JH + M.REC * m["record_index"].astype(np.uint64),
                          host["record_offset"][::-1])
    assert np.array_equal(m["app_offsets"], host["app_offset"][::-1])
    assert np.array_equal(m["lengths"], host["app_length"][::-1])
    assert np.array_equal(m["expected"], host["crc32c"][::-1])
    assert np.array_equal(m["crcs"], m["expected"])  # the writer stores true CRCs


def test_model_on_the_reference_fixture():
    j = np.fromfile(os.path.join(GOLDEN, "test.bmq_journal"), np.uint8)
    d = np.fromfile(os.path.join(GOLDEN, "test.bmq_data"), np.uint8)
    _, last = S.journal_bounds(j)
    run = j[M.JH:last + M.REC]
    m = M.model(run, d)
    assert m["refused"] is None
    assert list(M.JH + M.REC * m["record_index"]) == [at for at, _, _ in GOLDEN_RECORDS]
    assert list(m["app_offsets"]) == [a + 12 for _, a, _ in GOLDEN_RECORDS]
    apps = [d[int(a):int(a) + int(l)].tobytes() for a, l in zip(m["app_offsets"], m["lengths"])]
    assert b"hello world" in apps
    assert int(m["crcs"][apps.index(b"hello world")]) == 3381945770
    assert np.array_equal(m["crcs"], m["expected"])
    for k in range(len(GOLDEN_RECORDS)):
        app, _, lens, qkeys, guids, crc, kw, _, _ = golden_case(k)
        assert apps[k] == app.tobytes() and int(m["lengths"][k]) == int(lens[0])
        assert np.array_equal(m["queue_keys"][k], qkeys[0])
        assert np.array_equal(m["guids"][k], guids[0])
        assert int(m["expected"][k]) == int(crc[0])
        assert int(m["ref_counts"][k]) == int(kw["ref_counts"][0])
        assert int(m["timestamps"][k]) == kw["timestamp"]
    # the window form: the same records seen through a window that starts at byte 40
    w = M.model(run, d[40:], pos=40)
    assert np.array_equal(w["app_offsets"] + 40, m["app_offsets"])
    assert np.array_equal(w["crcs"], m["crcs"])


@pytest.mark.parametrize("name", M.VARIANTS)
def test_refusals_against_the_host_walk(name):
    j, d, last = M.malformed(name)
    m = M.model(j[M.JH:], d)
    kind, index = m["refused"]
    assert index == last and kind == M.VARIANT_KIND.get(name, M.K_DATA)
    host = S.scan_partition(j, d)
    assert host["recovery_rc"] == M.KIND_RC[kind]
    assert host["error_record_offset"] == M.JH + M.REC * index


def test_record_header_refusal_and_precedence():
    rng = np.random.default_rng(9)
    j, d = M.build_partition(rng, [10] * 12, others=0.0)
    run = j[M.JH:].copy()
    assert M.model(run, d)["refused"] is None
    for what, at in (("type", 0), ("lease", 8), ("seq", 2), ("magic", 56)):
        bad = run.copy()
        r = 5
        if what == "type":
            bad[M.REC * r] &= 0x0F
        elif what == "magic":
            bad[M.REC * r + 59] ^= 1
        else:
            bad[M.REC * r + at:M.REC * r + (12 if what == "lease" else 8)] = 0
        assert M.model(bad, d)["refused"] == (M.K_HEADER, r), what
    bad = run.copy()
    bad[M.REC * 9 + 59] ^= 1                    # kind 1 at record 9
    bad[M.REC * 2 + 36:M.REC * 2 + 52] = 0      # kind 2 at record 2
    bad[M.REC * 4 + 36:M.REC * 4 + 52] = 0      # kind 2 at record 4
    assert M.model(bad, d)["refused"] == (M.K_HEADER, 9)
    bad[M.REC * 9 + 59] ^= 1
    assert M.model(bad, d)["refused"] == (M.K_MESSAGE, 2)
    # unselected records: checked up to the data offset, no slot, counted
    sel = np.ones(13, np.uint8)
    sel[[2, 4]] = 0
    assert M.model(bad, d, select=sel)["refused"] == (M.K_MESSAGE, 2)
    m = M.model(run, d, select=sel)
    assert m["n"] == 10 and m["n_skipped"] == 2 and 2 not in m["record_index"]
    assert M.model(run, d, cap=11)["refused"] == (M.K_MANY, 12)
    assert M.model(run, d, cap=12)["refused"] is None
