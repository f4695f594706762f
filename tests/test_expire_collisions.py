"""What tests/expire_collisions.py claims, checked on the CPU before any GPU
test relies on it: that the queue table's hash in crc32c_expire_records.hip is
the text its restatement was written from, that the crafted tables are as
adversarial as they say (one chain of the stated length across the table's last
slot), and that every crafted case is a valid input with the stated outcome by
the model alone."""
import os

import numpy as np
import pytest

import expire_collisions as X
import expire_records_model as M
import join_collisions as J
import test_join_collisions as TJ

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                      "blazingmq_amd", "csrc", "crc32c_expire_records.hip")


def _text():
    with open(SOURCE) as f:
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


@pytest.mark.parametrize("name", sorted(X.MIRRORED))
def test_the_kernels_queue_key_is_the_text_its_restatement_was_written_from(name):
    signature, body = X.MIRRORED[name]
    assert _body(_text(), signature) == body, \
        "%s changed: update expire_collisions.queue_home and MIRRORED" % name


def test_both_walks_start_at_key_hash_and_step_by_one():
    text = _text()
    for signature in ("uint32_t queue_insert(const ExpArgs& a, const JoinKey& k, uint64_t e)",
                      "uint32_t queue_find(const ExpArgs& a, const JoinKey& k)"):
        assert _body(text, signature).startswith("{ " + X.WALK), signature
    # the only hash in the unit is crc32c_join_key.h's, which test_join_collisions.py mirrors
    assert text.count("key_hash(") == 2 and "0x9E3779B9" not in text


def test_queue_home_equals_the_scalar_restatement_under_the_null_guid():
    rng = np.random.default_rng(4)
    keys = [rng.integers(0, 256, 5, dtype=np.uint8).tobytes() for _ in range(400)]
    keys += [b"\xFF" * 5, b"\x80" * 5, bytes(4) + b"\x01"]
    for slots in (64, 1024, 4096):
        assert X.queue_home(keys, slots).tolist() == \
            [TJ.scalar_home("join", X.NULL_GUID + k, slots) for k in keys]


def test_the_table_as_the_host_sizes_it():
    assert [X.queue_slots(n) for n in (1, 3, 32, 33, 1025, 40000)] == \
        [64, 64, 64, 128, 4096, 131072]


@pytest.mark.parametrize("case,count", [(X.queue_chain, X.CHAIN), (X.queue_long, X.LONG),
                                        (X.queue_duplicate, X.BEHIND)])
def test_the_crafted_tables_are_one_chain_across_the_tables_end(case, count):
    c = case()
    table_keys = [bytes(k) for k in np.asarray(c.table[0]).reshape(-1, 5)]
    distinct = list(dict.fromkeys(table_keys))
    assert len(distinct) == count and X.queue_slots(len(table_keys)) == c.slots
    assert set(X.queue_home(distinct, c.slots).tolist()) == {c.home}
    lay = J.probe_lengths(X.queue_home(distinct, c.slots), c.slots)
    assert lay.clusters == [(c.home, count)] and lay.wraps()
    assert all(0 not in k for k in c.keys)
    if case is X.queue_long:
        assert lay.longest() > 1024


def test_the_crafted_cases_by_the_model_alone():
    c = X.queue_chain()
    got = M.expire_records(c.run, *c.table, **c.kw)
    assert isinstance(got, M.Expired)
    assert got.result["n_expired"] == c.info["n_expired"] == 180
    assert got.result["n_no_queue"] == c.info["n_no_queue"] == 76
    assert got.result["n_live"] == 2 * (X.CHAIN + X.ABSENT) - 24
    # a queue of TTL 2,000 keeps both messages and its front is the first of them
    fronts = got.queue_front.tolist()
    assert sum(f != M.NONE for f in fronts) == X.CHAIN // 2
    assert [f != M.NONE for f in fronts] == [k % 2 == 1 for k in c.info["table_order"]]
    c = X.queue_long()
    got = M.expire_records(c.run, *c.table, **c.kw)
    assert got.result["n_expired"] == X.LONG and got.queue_expired.tolist() == [1] * X.LONG
    c = X.queue_duplicate()
    assert M.expire_records(c.run, *c.table, **c.kw) == M.Refusal(M.QUEUE_KEY, X.BEHIND - 1)
