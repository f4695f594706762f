"""What tests/join_collisions.py claims, checked on the CPU before any GPU test
relies on it: that its hash mirrors are the kernels' hashes, that the crafted
runs are as adversarial as they say (one chain of the stated length across the
table's last slot, near pairs that share a home), and that every crafted run is
a valid input with the stated outcome by the reference alone -- the models, and
for select_records the native host walk."""
import os
import re

import numpy as np
import pytest

from blazingmq_amd import Crc32c
from blazingmq_amd import storage as S
import confirm_records_model as CM
import join_collisions as J
import journal_select_model as SM
import rollover_model as RM

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "blazingmq_amd", "csrc")


# ---- the mirrors ---------------------------------------------------------------

def _body(name):
    """The body of the mirrored function `name` in the kernels' source,
    whitespace-normalised."""
    path, signature, _ = J.MIRRORED[name]
    with open(os.path.join(CSRC, path)) as f:
        text = " ".join(f.read().split())
    at = text.index(signature) + len(signature)
    assert text[at:at + 2] == " {", (name, text[at:at + 20])
    depth, end = 0, at + 1
    while True:
        depth += {"{": 1, "}": -1}.get(text[end], 0)
        end += 1
        if depth == 0:
            return text[at + 1:end]


@pytest.mark.parametrize("name", sorted(J.MIRRORED))
def test_the_kernels_hash_is_the_text_its_mirror_was_written_from(name):
    assert _body(name) == J.MIRRORED[name][2], \
        "%s of %s changed: update join_collisions.%s and MIRRORED" % (name, J.MIRRORED[name][0],
                                                                      name)


def _literals(name):
    """(the multipliers and seeds, the right shifts) in the source's order."""
    body = _body(name)
    return ([int(x, 16) for x in re.findall(r"0x([0-9A-Fa-f]+)u", body)],
            [int(x) for x in re.findall(r">> (\d+)", body)])


def scalar_home(kind, key, slots):
    """The home slot in Python integers, with the constants read from the
    kernels' source: what the numpy mirrors are held to."""
    le = lambda b: int.from_bytes(b, "little")
    if kind == "join":
        (seed, mul, last), (fold, final) = _literals("key_hash")
        h = seed
        for w in [le(key[4 * j:4 * j + 4]) for j in range(4)] + [le(key[16:18]), le(key[18:21])]:
            h = ((h ^ w) * mul) & 0xFFFFFFFF
            h ^= h >> fold
        h = (h * last) & 0xFFFFFFFF
        return (h ^ (h >> final)) & (slots - 1)
    m64 = (1 << 64) - 1
    if kind == "guid":
        (a, b, c), (s0, s1, s2) = _literals("guid_home")
        h = (le(key[:8]) * a) & m64
        h ^= h >> s0
        h = (h + le(key[8:]) * b) & m64
        h ^= h >> s1
        h = (h * c) & m64
        h ^= h >> s2
        return h & (slots - 1)
    (a,), (s0,) = _literals("key_home")
    h = (le(key) * a) & m64
    return (h ^ (h >> s0)) & (slots - 1)


def _homes(kind, keys, slots):
    return [scalar_home(kind, k, slots) for k in keys]


@pytest.mark.parametrize("kind", sorted(J.WIDTH))
def test_the_mirrors_equal_the_scalar_restatement(kind):
    rng = np.random.default_rng(3)
    keys = [rng.integers(0, 256, J.WIDTH[kind], dtype=np.uint8).tobytes() for _ in range(600)]
    keys += [b"\xFF" * J.WIDTH[kind], b"\x80" * J.WIDTH[kind], bytes(J.WIDTH[kind] - 1) + b"\x01"]
    for slots in (64, 1024, 1 << 13, 1 << 20):
        assert J.HOME[kind](keys, slots).tolist() == _homes(kind, keys, slots)


def test_the_tables_as_the_host_sizes_them():
    assert [J.join_slots(n) for n in (0, 1, 32, 33, 256, 257, 1101)] == \
        [64, 64, 64, 128, 512, 1024, 4096]
    assert J.queue_slots(1 << 16, 10, 3) == 64 and J.queue_slots(300, 5000) == 1024
    assert J.queue_slots(299, 5000, 300) == 1024 and J.queue_slots(1 << 40, 700, 300) == 2048


def test_probe_lengths_on_a_hand_worked_table():
    lay = J.probe_lengths([6, 6, 6, 2, 7, 3], 8)
    assert lay.slot == [6, 7, 0, 2, 1, 3] and lay.steps == [1, 2, 3, 1, 3, 1]
    assert lay.clusters == [(6, 6)] and lay.wraps() and lay.longest() == 6
    assert lay.walk(6) == 7 and lay.walk(1) == 4 and lay.walk(4) == 1
    lay = J.probe_lengths([1, 1, 5], 8)
    assert lay.clusters == [(1, 2), (5, 1)] and not lay.wraps()


def test_colliders_and_near_pairs_are_what_they_say():
    for kind, slots, home in (("join", 512, 504), ("guid", 2048, 2044), ("queue", 1024, 1020)):
        keys = J.colliders(kind, slots, home, 50, 9)
        assert len(set(keys)) == 50 and all(len(k) == J.WIDTH[kind] for k in keys)
        assert set(_homes(kind, keys, slots)) == {home}
        assert keys == J.colliders.__wrapped__(kind, slots, home, 50, 9)      # seeded
        seen = np.frombuffer(b"".join(keys), np.uint8)
        assert seen.min() < 0x20 and seen.max() >= 0xE0                       # the full range
    for kind in ("join", "queue"):
        keys = J.colliders(kind, 256, 3, 20, 9, True)
        assert all(b >= 0x80 for k in keys for b in k[-5:])
    for kind, where in (("join", range(21)), ("guid", range(15)), ("queue", [20])):
        for at in where:
            a, b = J.near_pair(kind, 128, at, 5)
            i = at - 16 if kind == "queue" else at
            assert [x ^ y for x, y in zip(a, b)] == [0x80 if k == i else 0 for k in range(len(a))]
            assert scalar_home(kind, a, 128) == scalar_home(kind, b, 128)


# ---- the inputs are adversarial ------------------------------------------------------

def _one_chain(kind, keys, slots, home, length):
    """The keys (one slot each) make one run of `length` taken slots that
    starts at `home` and passes the table's last slot."""
    homes = _homes(kind, keys, slots)
    assert set(homes) == {home}
    lay = J.probe_lengths(homes, slots)
    assert lay.clusters == [(home, length)] and lay.wraps() and lay.longest() == length
    assert max(lay.steps) == length and home + length > slots
    return lay


@pytest.mark.parametrize("case,slots,length", [
    (J.confirm_chain, 1024, J.CHAIN), (J.confirm_long, 4096, J.LONG),
    (J.confirm_duplicate, 256, J.BEHIND), (J.rollover_chain, 1024, J.CHAIN // 2),
    (J.rollover_long, 8192, J.LONG), (J.rollover_duplicate, 256, J.BEHIND)],
    ids=lambda c: getattr(c, "__name__", None))
def test_the_join_table_runs_hold_one_chain_across_the_tables_end(case, slots, length):
    c = case()
    assert c.slots == slots == J.join_slots(c.run.size // 60)
    assert len(set(c.keys)) == length
    _one_chain("join", c.keys, slots, c.home, length)


def test_the_chain_runs_probes_and_bytes():
    c = J.confirm_chain()
    lay = _one_chain("join", c.keys, c.slots, c.home, J.CHAIN)
    assert c.home == c.slots - 8
    # absent keys: the whole chain to the empty slot, and from mid-chain
    assert len(c.info["same"]) == 40 and len(c.info["mid"]) == 10
    assert {lay.walk(h) for h in _homes("join", c.info["same"], c.slots)} == {J.CHAIN + 1}
    assert {lay.walk(h) for h in _homes("join", c.info["mid"], c.slots)} == {J.CHAIN - 108 + 1}
    assert not set(c.info["same"]) & set(c.keys) and not set(c.info["mid"]) & set(c.keys)
    # every queue-key byte would show a wrong shift or a sign extension
    for keys in (c.keys, c.info["same"], c.info["mid"], J.rollover_chain().keys):
        assert all(b >= 0x80 for k in keys for b in k[16:])
    types = c.run.reshape(-1, 60)[:, 0] >> 4
    assert [int((types == t).sum()) for t in (1, 2, 3, 4)] == [200, 67, 20, 1]
    # with all colliders but one unselected (or dropped) the table holds one key
    one = J.rollover_chain(137)
    assert len(one.keys) == 1 and one.info["n_kept_messages"] == 1


@pytest.mark.parametrize("case", [J.confirm_pairs, J.rollover_pairs],
                         ids=lambda c: c.__name__)
@pytest.mark.parametrize("swapped", [False, True])
def test_the_near_pairs_share_a_home_and_a_chain(case, swapped):
    c = case(swapped)
    pairs = c.info["pairs"]
    assert len(pairs) == 21 and c.slots == J.join_slots(c.run.size // 60)
    for at, (a, b) in enumerate(pairs):
        assert [x ^ y for x, y in zip(a, b)] == [0x80 if k == at else 0 for k in range(21)]
        assert (a[at] & 0x80 != 0) == swapped
        assert scalar_home("join", a, c.slots) == scalar_home("join", b, c.slots) == c.home
    every = [k for p in pairs for k in p]
    assert len(set(every)) == 42
    # all 42 in the confirms' table; of each pair the first in the rollover's
    _one_chain("join", every if case is J.confirm_pairs else c.keys, c.slots, c.home,
               42 if case is J.confirm_pairs else 21)
    assert set(J.confirm_pairs(False).info["pairs"]) == \
        {(b, a) for a, b in J.confirm_pairs(True).info["pairs"]}


def test_the_select_runs_hold_one_chain_across_the_tables_end():
    for deletions in (True, False):
        j, d, keys, slots, home = J.select_queues(deletions)
        assert slots == 1024 == J.queue_slots(J.QUEUES, len(SM.record_run(j)[0]) // 60, J.QUEUES)
        assert J.queue_slots(J.QUEUES - 1, 5000) == slots and home == slots - 4
        assert len(set(keys)) == J.QUEUES and all(b >= 0x80 for k in keys for b in k)
        _one_chain("queue", keys, slots, home, J.QUEUES)
        recs = SM.record_run(j)[0].reshape(-1, 60)
        ops = recs[recs[:, 0] >> 4 == 4]
        assert {r[22:27].tobytes() for r in ops} == set(keys)     # the table's keys, all of them
        kinds = {int.from_bytes(r[32:36].tobytes(), "big") for r in ops}
        assert kinds == ({1, 2, 3, 4} if deletions else {1, 2, 4})
        assert len(ops) < 1024                                    # one phase of one block
    j, d, slots, home, in_table, absent, _ = J.select_guid_chain()
    n = len(SM.record_run(j)[0]) // 60
    assert slots == 2048 == J.join_slots(n) and home == slots - 4
    assert len(in_table) == J.GUID_CHAIN and len(set(in_table)) == J.GUID_CHAIN - 1
    lay = _one_chain("guid", in_table, slots, home, J.GUID_CHAIN)
    recs = SM.record_run(j)[0].reshape(-1, 60)
    assert sorted(r[28:44].tobytes() for r in recs[recs[:, 0] >> 4 == 3]) == sorted(in_table)
    # the undeleted messages walk to the empty slot from the start and from mid-chain
    walks = [lay.walk(h) for h in _homes("guid", absent, slots)]
    assert sorted(set(walks)) == [J.GUID_CHAIN - 154 + 1, J.GUID_CHAIN + 1]
    assert len(absent) == 30 and not set(absent) & set(in_table)


# ---- the inputs are valid, by the reference alone ---------------------------------------

def _plain(pairs):
    return dict(guids=np.frombuffer(b"".join(g for g, _ in pairs), np.uint8),
                queue_keys=np.frombuffer(b"".join(k for _, k in pairs), np.uint8))


def _confirm(c, pairs, select=None):
    return CM.confirm_records(c.run, **_plain(pairs), lease_id=c.info["lease_id"],
                              first_seq=c.info["next_seq"], select=select)


def test_confirm_chain_by_the_model():
    c = J.confirm_chain()
    pairs, names = J.confirm_chain_batch()
    m = _confirm(c, pairs)
    assert isinstance(m, CM.Confirmed)
    assert (m.result["n_not_found"], m.result["n_written"], m.result["n_deletions"]) == (50, 180, 0)
    assert m.target.tolist() == [CM.NONE if r is None else r for r in names]
    assert sorted(set(m.left_out.tolist())) == [0, 1, 2]      # dead and not a message; 3 - 1 - 1; 3 - 1
    # all colliders but one unselected: one confirm finds its message
    select, only = J.confirm_chain_select()
    m = _confirm(c, pairs, select)
    assert (m.result["n_not_found"], m.result["n_written"]) == (len(pairs) - 1, 1)
    assert m.target[m.target != CM.NONE].tolist() == [only] and select.sum() == 2


def test_confirm_long_pairs_and_duplicate_by_the_model():
    c = J.confirm_long()
    order = J.long_order()
    m = _confirm(c, [J.split(c.keys[i]) for i in order])
    assert m.result["n_deletions"] == J.LONG and m.target.tolist() == (order + 1).tolist()
    for swapped in (False, True):
        c = J.confirm_pairs(swapped)
        firsts = [a for a, _ in c.info["pairs"]]
        m = _confirm(c, [J.split(a) for a in firsts])
        assert m.result["n_deletions"] == 21 and m.result["n_not_found"] == 0
        assert m.target.tolist() == [c.info["record"][a] for a in firsts] == list(range(1, 43, 2))
        assert m.left_out.tolist() == [0] + [0, 1] * 21            # the twins untouched
    c = J.confirm_duplicate()
    m = _confirm(c, [J.split(c.keys[0])])
    assert m == CM.Refusal(CM.DUPLICATE_MESSAGE, J.BEHIND)


def _rolled(c):
    m = RM.rollover(c.run, c.data, data_file_pos=0, new_data_file_pos=40, keep=c.info["keep"],
                    confirm_mode=1, dst_bytes=1 << 40, journal_dst_bytes=1 << 40,
                    crc32c=Crc32c.calculate)
    assert isinstance(m, RM.Rolled) and m.result["n_bad"] == 0
    assert m.result["n_messages"] == c.info["n_kept_messages"]
    types = c.run.reshape(-1, 60)[:, 0] >> 4
    kept = (m.new_index != RM.NOT_KEPT)[types == 2].tolist()
    assert kept == J.survivors(c.run, c.info["keep"])
    return kept


def test_the_rollover_runs_by_the_model():
    kept = _rolled(J.rollover_chain())
    assert len(kept) == J.CHAIN and sum(kept) == J.CHAIN // 2
    kept = _rolled(J.rollover_chain(137))
    assert sum(kept) == 1
    assert sum(_rolled(J.rollover_long())) == J.LONG
    for swapped in (False, True):
        kept = _rolled(J.rollover_pairs(swapped))
        assert len(kept) == 42 and sum(kept) == 21
    assert _rolled(J.rollover_duplicate()) == [True]


def _selected(j, d, **kw):
    """Host walk and model agree; returns the model's answer."""
    run = SM.record_run(j)[0]
    sel, rc, err = SM.host_view(j, d, **kw)
    m = SM.select_model(run, d.size, **kw)
    assert np.flatnonzero(m["select"]).tolist() == sel
    assert (m["recovery_rc"], m["error_record"]) == (rc, err)
    return m


def test_the_select_runs_by_the_host_walk_and_the_model():
    j, d, keys, _, _ = J.select_queues(True)
    m = _selected(j, d)
    assert m["recovery_rc"] == 0 and min(m["n_selected"], m["n_deleted"], m["n_purged"]) > 0
    j, d, keys, _, _ = J.select_queues(False)
    for kw in (dict(), dict(with_csl=True, queue_keys=keys)):
        m = _selected(j, d, **kw)
        assert m["recovery_rc"] == 0 and min(m["n_selected"], m["n_deleted"], m["n_purged"]) > 0
    short = keys[:J.WITHHELD] + keys[J.WITHHELD + 1:]
    m = _selected(j, d, with_csl=True, queue_keys=short)
    recs = SM.record_run(j)[0].reshape(-1, 60)
    creation = [r for r in range(len(recs)) if recs[r, 0] >> 4 == 4 and
                recs[r, 22:27].tobytes() == keys[J.WITHHELD]]
    assert (m["recovery_rc"], [m["error_record"]]) == (S.RC_INVALID_QUEUE_KEY, creation)
    j, d, _, _, _, _, want = J.select_guid_chain()
    m = _selected(j, d)
    assert m["recovery_rc"] == 0 and {k: m[k] for k in want} == want
