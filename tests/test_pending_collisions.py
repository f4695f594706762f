"""What tests/pending_collisions.py claims, checked on the CPU before the GPU
tests below rely on it: that the queue table's hash in crc32c_join_key.h is the
text its restatement was written from, that the crafted run and table are as
adversarial as they say (one chain of the stated length across each table's
last slot), and that every crafted case is a valid input with the stated
outcome by the model alone.  Then the device against the model on them."""
import os

import numpy as np
import pytest

from blazingmq_amd import _native as N  # noqa: F401
import expire_collisions as X
import join_collisions as J
import pending_collisions as PC
import pending_list_cases as C
import pending_list_model as M
import test_join_collisions as TJ

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "blazingmq_amd", "csrc")


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return " ".join(f.read().split())


def _body(text, signature):
    at = text.index(signature) + len(signature)
    assert text[at:at + 2] == " {", text[at:at + 20]
    depth, end = 0, at + 1
    while True:
        depth += {"{": 1, "}": -1}.get(text[end], 0)
        end += 1
        if depth == 0:
            return text[at + 1:end]


@pytest.mark.parametrize("name", sorted(PC.MIRRORED))
def test_the_headers_queue_key_is_the_text_its_restatement_was_written_from(name):
    signature, body = PC.MIRRORED[name]
    assert _body(_text("crc32c_join_key.h"), signature) == body, \
        "%s changed: update expire_collisions.queue_home and pending_collisions.MIRRORED" % name


def test_both_walks_start_at_key_hash_and_step_by_one_and_the_unit_has_no_hash_of_its_own():
    text = _text("crc32c_join_key.h")
    for signature in ("uint32_t table_insert(const QueueTable& t, const JoinKey& k, uint64_t e)",
                      "uint32_t table_find(const QueueTable& t, const JoinKey& k)"):
        assert _body(text, signature).startswith("{ " + PC.WALK), signature
    unit = _text("crc32c_pending_list.hip")
    assert "key_hash(" not in unit and "0x9E3779B9" not in unit
    # ... and it is the walk the expire unit's copy takes, which expire_collisions.py restates
    assert PC.WALK.replace("t.slots", "a.qslots") == X.WALK
    assert PC.MIRRORED["table_key"][1] == X.MIRRORED["queue_key"][1]
    assert PC.MIRRORED["table_key_of"][1].replace("t.keys", "a.queue_keys") == \
        X.MIRRORED["queue_key_of"][1]


def test_the_crafted_keys_are_one_chain_across_each_tables_end():
    case, info = PC.both_chains()
    n = len(case.run) // 60
    assert J.join_slots(n) == J.join_slots(n + 1) == info["slots"]
    assert X.queue_slots(PC.QUEUES) == X.queue_slots(PC.QUEUES + 1) == info["qslots"]
    keys = [g + q for g, q in info["pairs"]]
    assert len(set(keys)) == PC.MESSAGES + PC.ABSENT
    assert set(J.key_hash(keys, info["slots"]).tolist()) == {info["home"]}
    assert [TJ.scalar_home("join", k, info["slots"]) for k in keys[:20]] == [info["home"]] * 20
    lay = J.probe_lengths(J.key_hash(keys[:PC.MESSAGES], info["slots"]), info["slots"])
    assert lay.clusters == [(info["home"], PC.MESSAGES)] and lay.wraps()
    qkeys = list(info["qkeys"])
    assert len(set(qkeys)) == PC.QUEUES + PC.ABSENT_QUEUES and all(0 not in k for k in qkeys)
    assert set(X.queue_home(qkeys, info["qslots"]).tolist()) == {info["qhome"]}
    table = [bytes(k) for k in case.queue_keys.reshape(-1, 5)]
    assert sorted(table) == sorted(qkeys[:PC.QUEUES]) and table != qkeys[:PC.QUEUES]
    lay = J.probe_lengths(X.queue_home(table, info["qslots"]), info["qslots"])
    assert lay.clusters == [(info["qhome"], PC.QUEUES)] and lay.wraps()
    # the records' keys are those keys: MESSAGE, CONFIRM and DELETION alike
    rows = case.run.reshape(-1, 60)
    types = rows[:, 0] >> 4
    for t, g, q in ((C.MESSAGE, 36, 22), (C.CONFIRM, 32, 22), (C.DELETION, 28, 23)):
        mine = rows[types == t]
        assert mine.shape[0] >= 15
        assert {bytes(r[g:g + 16]) + bytes(r[q:q + 5]) for r in mine} <= set(keys)


def test_the_crafted_cases_by_the_model_alone():
    case, info = PC.both_chains()
    args, kw = C.model_args(case)
    got = M.pending_records(*args, **kw)
    assert isinstance(got, M.Pending)
    for name in ("n_live", "n_no_queue", "n_pending", "n_not_found"):
        assert got.result[name] == info[name] > 0, name
    assert got.result["n_unknown_confirms"] == info["n_unknown"] > 0
    assert got.result["n_listed"] == info["n_pending"]
    dup, index = PC.duplicate_message_behind_the_chain()
    args, kw = C.model_args(dup)
    assert M.pending_records(*args, **kw) == M.Refusal(M.DUPLICATE_MESSAGE, index)
    dup, index = PC.duplicate_queue_behind_the_chain()
    args, kw = C.model_args(dup)
    assert M.pending_records(*args, **kw) == M.Refusal(M.QUEUE_KEY, index)


# ---- the device --------------------------------------------------------------

@pytest.mark.gpu
def test_both_chains_across_the_tables_ends(cuda):
    from test_gpu_pending_list import _check
    case, info = PC.both_chains()
    m, _ = _check(cuda, case)
    assert m.result["n_pending"] == info["n_pending"]


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["message", "queue"])
def test_a_duplicate_behind_a_chain(cuda, which):
    from test_gpu_pending_list import _check
    case, index = (PC.duplicate_message_behind_the_chain if which == "message"
                   else PC.duplicate_queue_behind_the_chain)()
    m, _ = _check(cuda, case)
    assert isinstance(m, M.Refusal) and m.index == index
