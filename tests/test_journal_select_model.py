"""The order-free restatement of the recovery selection (journal_select_model,
DESIGN.md section 16) is the reference: held to the native walk
(``scan_partition``) and its Python restatement (``recovery_selection_py``) on
every partition of journal_select_cases -- selected records, recovery_rc and
offending record, with and without CSL -- with the reductions visited in a
shuffled order.  CPU only."""
import numpy as np
import pytest

from blazingmq_amd import storage as S
import journal_select_cases as C
import journal_select_model as M
from test_recovery_selection import Q1, _random_partition


def _hold(name, shuffle_seed=1):
    j, d, csl, keys = C.case(name)
    kw = dict(with_csl=csl, queue_keys=keys)
    run, start = M.record_run(j)
    n = len(run) // 60
    sel, rc, err = M.host_view(j, d, **kw)
    py = S.recovery_selection_py(j, d, **kw)
    assert sorted((o - start) // 60 for o in py["record_offset"]) == sel
    assert py["recovery_rc"] == rc
    order = np.random.default_rng(shuffle_seed).permutation(n)
    m = M.select_model(run, d.size, order=order, **kw)
    assert np.flatnonzero(m["select"]).tolist() == sel, name
    assert (m["recovery_rc"], m["error_record"]) == (rc, err), name
    assert m["n_selected"] == len(sel)
    assert not m["select"][:m["first_record"]].any()
    if rc == 0:
        assert m["first_record"] == m["stop"] + 1
    else:
        assert m["first_record"] == (n if m["first_pass"] else err + 1)
    # the visiting order changes nothing
    again = M.select_model(run, d.size, **kw)
    assert all(np.array_equal(again[k], m[k]) for k in m)
    return m, sel, rc, err


@pytest.mark.parametrize("name", C.ALL)
def test_model_equals_the_reference(name):
    _hold(name)


def test_the_restated_generator_is_the_original():
    for seed in range(25):
        j, d, _ = C.random_files(seed)
        assert S.scan_partition(j, d)["record_offset"].tolist() == \
            _random_partition(seed)["record_offset"].tolist()


def test_the_cases_are_not_vacuous():
    """Judged on the REFERENCE walk alone (and the model only where the walk
    does not say: which rule skipped a message)."""
    ok = msgs = 0
    codes = set()
    guid_skip = queue_skip = False
    for name in C.ALL:
        j, d, csl, keys = C.case(name)
        nat = S.scan_partition(j, d, with_csl=csl, queue_keys=keys)
        codes.add(nat["recovery_rc"])
        if name.startswith("random:") and not csl:
            if nat["recovery_rc"] == 0:
                ok += 1
                msgs += nat["record_offset"].size
            m = M.select_model(M.record_run(j)[0], d.size)
            guid_skip |= m["n_deleted"] > 0
            queue_skip |= m["n_purged"] > 0
    assert ok >= 15 and msgs >= 200
    want = {getattr(S, n) for n in dir(S) if n.startswith("RC_")} - {S.RC_INVALID_DATA_RECORD}
    assert codes == want
    assert guid_skip and queue_skip


@pytest.mark.parametrize("name,selected,rc", [
    ("d_m1_m2", 1, 0), ("d_d_m", 1, 0), ("d_m1_d_m2", 1, 0), ("deletion_purged", 1, 0),
    ("purged_between", 1, 0), ("stop_in_the_middle", 1, S.RC_INVALID_QUEUE_KEY),
    ("addition_below_creation", 0, S.RC_DUPLICATE_QUEUE_KEY), ("addition_above_creation", 1, 0),
    ("recreated_key", 2, 0), ("two_failures", 1, S.RC_INVALID_DELETION_RECORD),
    ("first_pass_below_second", 0, S.RC_DUPLICATE_QUEUE_KEY),
    ("unknown_queue_deleted_message", 1, 0)])
def test_directed_cases_say_what_they_are_for(name, selected, rc):
    m, sel, got, _ = _hold(name, shuffle_seed=7)
    assert (len(sel), got) == (selected, rc)


def test_guid_and_queue_skips_are_counted():
    assert _hold("d_m1_m2")[0]["n_deleted"] == 1
    assert _hold("d_m1_d_m2")[0]["n_deleted"] == 2
    m = _hold("purged_between")[0]
    assert (m["n_deleted"], m["n_purged"], m["n_selected"]) == (1, 1, 1)
    m = _hold("rich")[0]
    assert m["n_deleted"] == 3 and m["n_purged"] == 7


def test_data_record_checks_are_the_stated_difference():
    """No DATA byte is read: where the host walk fails a selected message with
    INVALID_DATA_RECORD (-17), the model keeps it selected (unpack_records then
    refuses it), and goes on to what lies below."""
    w = S.PartitionWriter()
    w.queue_op(S.OP_CREATION, Q1)
    below, _ = w.message(b"below", Q1)
    bad, _ = w.message(b"its DataHeader is malformed", Q1)
    above, _ = w.message(b"above", Q1)
    j, d = w.files()
    j, d = j.copy(), d.copy()
    doff = int.from_bytes(j[bad + 32:bad + 36].tobytes(), "big") * 8
    d[doff] &= 0x1F  # headerWords = 0
    nat = S.scan_partition(j, d)
    assert (nat["recovery_rc"], nat["error_record_offset"]) == (S.RC_INVALID_DATA_RECORD, bad)
    assert nat["record_offset"].tolist() == [above]
    run, start = M.record_run(j)
    m = M.select_model(run, d.size)
    assert m["recovery_rc"] == 0 and m["error_record"] == len(run) // 60
    assert np.flatnonzero(m["select"]).tolist() == [(o - start) // 60 for o in (below, bad, above)]
