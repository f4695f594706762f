"""Device-side PUT-event walk (bmqcrc_put_event_unpack, ABI 2.12) on the GPU.
The oracle throughout is tests/put_unpack_model.py (the host's own walks plus
host CRCs).  Every raw call hands the library canary-filled output arrays with
guard elements behind msg_cap: the guards are checked after every call, the
slots the call leaves untouched after a successful one, and every element
after a refused one."""
import ctypes
import functools

import numpy as np
import pytest

from blazingmq_amd import (BmqCrcError, Crc32c, _native as N, last_copy, last_launch,
                           last_put_pack, last_put_unpack, last_records_pack, pack_events,
                           pack_records, unpack_events)
from blazingmq_amd import storage as S
import device_views as V
import pack_pool
import put_pack_model as P
import put_unpack_model as M
import test_grid_regimes as G
from records_pack_model import REC, wrap_partition

pytestmark = pytest.mark.gpu

GUARD = 8
SLACK = 64   # bytes kept behind every events buffer (offsets_past_end points into them)
CANARY = {"app_offsets": 0x5A5A5A5A5A5A5A5A, "lengths": 0x5A5A5A5A, "queue_ids": 0x5A5A5A5A,
          "guids": 0xA5, "flags": 0xA5, "expected": 0x5A5A5A5A, "out": 0x5A5A5A5A,
          "event_first": 0x5A5A5A5A5A5A5A5A}
PER = {"app_offsets": 1, "lengths": 1, "queue_ids": 1, "guids": 16, "flags": 1, "expected": 1,
       "out": 1}
KIND_NAME = {1: b"EVENT_OFFSETS", 2: b"EVENT_HEADER", 3: b"PUT_HEADER", 4: b"PADDING",
             5: b"TOO_MANY_MESSAGES"}


def _side_stream(cuda):
    """A stream of its own from the high-priority pool (the default pool's
    streams carry planner history that tests elsewhere rely on)."""
    import torch
    return torch.cuda.Stream(cuda, priority=-1)


def _t(cuda, a, dtype):
    import torch
    a = np.ascontiguousarray(a, dtype=dtype)
    if dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(cuda)


def _device_events(cuda, buf, place=None):
    """`buf` on the device as a view of a longer allocation: one that starts
    with it, or with `place` (a device_views.Placer) one that holds it, and
    the SLACK bytes behind it, at the placer's phase for `events`."""
    import torch
    if place is not None:
        whole = np.concatenate([np.asarray(buf, np.uint8), np.full(SLACK, 0xEE, np.uint8)])
        return place.put("events", whole)[:buf.size]
    back = torch.full((buf.size + SLACK,), 0xEE, dtype=torch.uint8, device=cuda)
    back[:buf.size] = torch.from_numpy(np.ascontiguousarray(buf)).to(cuda)
    return back[:buf.size]


def _raw(cuda, events, offs, cap, verify=True, sync=True, stream=None, skip=(), place=None):
    """One bmqcrc_put_event_unpack into canary-filled arrays.  Returns (rc,
    error text, result of the call or of bmqcrc_last_put_unpack, the arrays
    on the host with their guards).  With `place` (a device_views.Placer that
    placed `events`) every array lies at the placer's phase for its name, and
    the sentinel margins around all of them are checked after the call."""
    import torch
    stream = stream or torch.cuda.current_stream(cuda)
    n_events = 1 if offs is None else len(offs) - 1
    dt = {"app_offsets": torch.int64, "lengths": torch.int32, "queue_ids": torch.int32,
          "guids": torch.uint8, "flags": torch.uint8, "expected": torch.int32,
          "out": torch.int32, "event_first": torch.int64}
    with torch.cuda.stream(stream):
        if offs is None:
            d_offs = None
        elif place is not None:
            d_offs = place.put("event_offsets", np.ascontiguousarray(offs, dtype=np.int64))
        else:
            d_offs = _t(cuda, offs, np.int64)
        arr = {}
        for name, t in dt.items():
            if name in skip or (name == "out" and not verify):
                continue
            size = n_events + 1 + GUARD if name == "event_first" else (cap + GUARD) * PER[name]
            if place is not None:
                arr[name] = place.fill(name, size, {torch.int64: np.uint64, torch.int32: np.uint32,
                                                    torch.uint8: np.uint8}[t], CANARY[name])
                continue
            fill = CANARY[name] - (1 << 64 if t == torch.int64 and CANARY[name] >> 63 else 0)
            arr[name] = torch.full((size,), fill, dtype=t, device=cuda)
        p = N.PutUnpack()
        p.struct_size = ctypes.sizeof(N.PutUnpack)
        p.events, p.events_bytes = events.data_ptr(), events.numel()
        p.event_offsets = d_offs.data_ptr() if d_offs is not None else None
        p.n_events, p.msg_cap = n_events, cap
        for name, t in arr.items():
            setattr(p, name, t.data_ptr())
        o = N.make_opts(device=cuda.index, stream=stream.cuda_stream,
                        flags=N.BMQCRC_F_DEVICE_PTRS | (0 if sync else N.BMQCRC_F_ASYNC))
        r = N.PutUnpackResult()
        rc = N.lib.bmqcrc_put_event_unpack(ctypes.byref(p), ctypes.byref(r), ctypes.byref(o))
        err = N.lib.bmqcrc_last_error()
        res = r.as_dict() if sync else None
        if not sync:
            assert rc == 0, (rc, err)
            assert r.as_dict() == N.PutUnpackResult().as_dict()  # written by a synchronous call only
            res = last_put_unpack(cuda.index, stream)
        host = {}
        for name, t in arr.items():
            a = t.cpu().numpy()
            host[name] = a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.itemsize]) \
                if name != "queue_ids" else a
        if place is not None:
            place.check()
    return rc, err, res, host


def _canary(name, a):
    want = CANARY[name] if name != "queue_ids" else np.int32(CANARY[name])
    return bool(np.all(a == want))


def _guards_intact(host, cap, n_events):
    for name, a in host.items():
        at = n_events + 1 if name == "event_first" else cap * PER[name]
        assert a.size == at + GUARD * PER.get(name, 1) and _canary(name, a[at:]), name


def _ok(cuda, buf, offs, cap=None, verify=True, sync=True, stream=None, model=None, n_bad=0,
        first_bad=None, skip=(), phases=None):
    """A call that must succeed, against the model.  `phases` maps every
    pointer of the call (events, event_offsets and the arrays by name) to the
    phase of its base; None: every buffer starts its allocation.  Returns
    (model, arrays)."""
    place = V.Placer(cuda, phases) if phases is not None else None
    m = model or M.model(buf, offs)
    assert m["refused"] is None
    n = m["n"]
    cap = n + 5 if cap is None else cap
    n_events = 1 if offs is None else len(offs) - 1
    rc, err, res, host = _raw(cuda, _device_events(cuda, buf, place), offs, cap, verify, sync,
                              stream, skip, place)
    assert rc == 0, (rc, err)
    assert res == dict(n_events=n_events, n_msgs=n, n_bad=n_bad,
                       first_bad=n if first_bad is None else first_bad, refused_kind=0,
                       refused_event=0, refused_offset=0), res
    _guards_intact(host, cap, n_events)
    for name in ("app_offsets", "lengths", "queue_ids", "flags", "expected", "event_first"):
        if name in host:
            k = len(m[name])
            assert np.array_equal(host[name][:k].astype(np.int64), m[name].astype(np.int64)), name
    if "guids" in host:
        assert np.array_equal(host["guids"][:16 * n].reshape(n, 16), m["guids"])
    for name in ("queue_ids", "guids", "flags"):  # untouched where no message is
        if name in host:
            assert _canary(name, host[name][n * PER[name]:]), name
    return m, host


def _refused(cuda, buf, offs, cap, want=None, verify=True, phases=None):
    """A call that must be refused, synchronously and asynchronously: the
    model's (kind, event, offset), and not one element written.  `phases`: as
    in _ok."""
    kind, event, offset = want or M.model(buf, offs, cap)["refused"]
    place = V.Placer(cuda, phases) if phases is not None else None
    events = _device_events(cuda, buf, place)
    n_events = 1 if offs is None else len(offs) - 1
    for sync in (True, False):
        rc, err, res, host = _raw(cuda, events, offs, cap, verify, sync, place=place)
        if sync:
            assert rc == N.BMQCRC_EINVAL and KIND_NAME[kind] in err and \
                b"nothing was written" in err, (rc, err)
            assert (b"%d" % event) in err and (b"offset %d" % offset) in err, err
        assert res == dict(n_events=n_events, n_msgs=0, n_bad=0, first_bad=0, refused_kind=kind,
                           refused_event=event, refused_offset=offset), (sync, res)
        for name, a in host.items():
            assert _canary(name, a), (sync, name)
    return kind, event, offset


# ---- round trip --------------------------------------------------------------

def test_round_trip_with_the_packer(cuda):
    import torch
    rng = np.random.default_rng(21)
    lens = np.arange(71, dtype=np.uint32)
    rng.shuffle(lens)
    soff = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    src = rng.integers(0, 256, size=int(lens.sum()), dtype=np.uint8)
    qids, guids, flags = P.random_meta(rng, 71)
    qids[:3] = [-1, -2**31, 2**31 - 1]
    ef = np.array([0, 1, 12, 13, 30, 45, 64, 71], np.int64)
    events, evoff, crcs = pack_events(
        _t(cuda, src, np.uint8), _t(cuda, soff, np.int64), _t(cuda, lens, np.uint32),
        _t(cuda, qids, np.int32), _t(cuda, guids, np.uint8), _t(cuda, flags, np.uint8),
        _t(cuda, ef, np.int64))
    want = P.host_crcs(src, soff, lens)
    u = unpack_events(events, evoff)
    res = last_put_unpack(cuda.index, torch.cuda.current_stream(cuda))
    assert (res["n_events"], res["n_msgs"], res["n_bad"], res["first_bad"],
            res["refused_kind"]) == (7, 71, 0, 71, 0)
    assert np.array_equal(u.lengths.cpu().numpy().view(np.uint32), lens)
    assert np.array_equal(u.queue_ids.cpu().numpy(), qids)
    assert np.array_equal(u.guids.cpu().numpy(), guids) and u.guids.shape == (71, 16)
    assert np.array_equal(u.flags.cpu().numpy(), flags)
    assert np.array_equal(u.event_first.cpu().numpy(), ef)
    assert np.array_equal(u.expected.cpu().numpy().view(np.uint32), want)
    assert np.array_equal(u.crcs.cpu().numpy().view(np.uint32), want)
    assert np.array_equal(crcs.cpu().numpy().view(np.uint32), want)
    again, evoff2, _ = pack_events(events, u.app_offsets, u.lengths, u.queue_ids, u.guids, u.flags,
                                   u.event_first)
    assert torch.equal(again, events) and torch.equal(evoff2, evoff)
    # and the canary form of the same call, against the model
    _ok(cuda, events.cpu().numpy(), evoff.cpu().numpy())


# ---- window and lane edges ---------------------------------------------------

def test_every_window_position(cuda):
    ev = M.ramp_event(np.random.default_rng(1))
    m, host = _ok(cuda, ev, None)
    assert m["n"] == 1024
    assert np.array_equal(host["out"][:1024], m["crcs"])


@pytest.mark.parametrize("count", [1, 63, 64, 65, 128, 129])
def test_lane_edges(cuda, count):
    rng = np.random.default_rng(count)
    ev = M.build_event(rng, rng.integers(0, 40, size=count))
    m, host = _ok(cuda, ev, np.array([0, ev.size]), cap=count)
    assert np.array_equal(host["out"][:count], m["crcs"])


def test_long_messages_among_short_ones(cuda):
    rng = np.random.default_rng(22)
    ev = M.build_event(rng, [3, 5000, 0, 70000, 17, 5000, 70001, 1, 2])
    m, host = _ok(cuda, ev, None)
    assert np.array_equal(host["out"][:9], m["crcs"])


def test_an_event_with_no_message_between_two_others(cuda):
    rng = np.random.default_rng(23)
    buf, offs = M.concat([M.build_event(rng, [4, 9]), M.build_event(rng, []),
                          M.build_event(rng, [0, 1, 2])])
    assert offs[2] - offs[1] == 8
    m, host = _ok(cuda, buf, offs)
    assert list(m["event_first"]) == [0, 2, 2, 5]
    assert np.array_equal(host["out"][:5], m["crcs"])
    # nothing but empty events: no message, and msg_cap 0 is legal
    buf, offs = M.concat([M.build_event(rng, [])] * 3)
    _ok(cuda, buf, offs, cap=0)


def test_more_events_than_the_walk_grid(cuda):
    rng = np.random.default_rng(24)
    buf, offs = M.concat([M.build_event(rng, [int(k)]) for k in rng.integers(0, 24, size=5000)])
    m, host = _ok(cuda, buf, offs)
    assert m["n"] == 5000 and np.array_equal(host["out"][:5000], m["crcs"])


def test_more_messages_than_one_step_of_the_publish_grid(cuda):
    # above 2,048 x 256 messages a publish thread copies a second slot, and with
    # msg_cap 300,000 above the count a placing thread empties a second one: one
    # event of 2,049 short messages 257 times over, the model tiled with it
    rng = np.random.default_rng(34)
    k, reps = 2049, 257
    assert k * reps > 2048 * 256
    ev = M.build_event(rng, rng.integers(0, 24, size=k))
    small = M.model(ev)
    n = k * reps
    model = dict(refused=None, n=n)
    for name in ("lengths", "queue_ids", "guids", "flags", "expected", "crcs"):
        model[name] = np.concatenate([small[name]] * reps)
    model["app_offsets"] = np.tile(small["app_offsets"], reps) + \
        np.repeat(np.arange(reps, dtype=np.int64) * ev.size, k)
    model["event_first"] = np.arange(reps + 1, dtype=np.int64) * k
    buf, offs = np.tile(ev, reps), np.arange(reps + 1, dtype=np.int64) * ev.size
    _, exact = _ok(cuda, buf, offs, cap=n, model=model)
    assert np.array_equal(exact["out"][:n], model["crcs"])
    # more than one step of the placing grid of empty slots behind the messages
    _, wide = _ok(cuda, buf, offs, cap=n + 300000, model=model)
    for name, a in exact.items():
        used = a.size - GUARD * PER.get(name, 1)
        assert np.array_equal(wide[name][:used], a[:used]), name
    # one wrong header CRC in the second step
    victim = 2048 * 256 + 1000
    bad = buf.copy()
    bad[(victim // k) * ev.size + M.walk(ev)[0][victim % k] + 28] ^= 0x01
    wrong = dict(model, expected=model["expected"].copy())
    wrong["expected"][victim] ^= 0x01000000
    _, host = _ok(cuda, bad, offs, cap=n, model=wrong, n_bad=1, first_bad=victim)
    assert np.array_equal(host["out"][:n], model["crcs"])


def test_one_event_without_offsets_and_optional_arrays_left_out(cuda):
    rng = np.random.default_rng(25)
    ev = M.build_event(rng, rng.integers(0, 200, size=150))
    m = M.model(ev)
    _ok(cuda, ev, None, model=m)
    _ok(cuda, ev, None, model=m, skip=("queue_ids", "guids", "flags", "expected", "event_first"))
    _ok(cuda, ev, None, model=m, verify=False, skip=("guids",))
    u = unpack_events(_device_events(cuda, ev))  # msg_cap None: the most the buffer can hold
    assert u.lengths.numel() == 150 and u.event_first.tolist() == [0, 150]
    assert np.array_equal(u.crcs.cpu().numpy().view(np.uint32), m["crcs"])


def test_events_beyond_4_gib_of_buffer(cuda):
    # positions with bits 31 and 32 set: nothing in the walk, the placing or
    # the refusal may hold a byte position in 32 bits or sign-extend one
    import torch
    base = (1 << 32) + (1 << 31) + 64
    rng = np.random.default_rng(33)
    buf, offs = M.concat([M.build_event(rng, rng.integers(0, 3000, size=k)) for k in (70, 3, 0)])
    m = M.model(buf, offs)
    back = torch.empty(base + buf.size + SLACK, dtype=torch.uint8, device=cuda)
    back[base:base + buf.size] = torch.from_numpy(buf).to(cuda)
    events, cap = back[:base + buf.size], m["n"] + 3
    rc, err, res, host = _raw(cuda, events, offs + base, cap)
    assert rc == 0, (rc, err)
    assert res == dict(n_events=3, n_msgs=73, n_bad=0, first_bad=73, refused_kind=0,
                       refused_event=0, refused_offset=0), res
    _guards_intact(host, cap, 3)
    assert np.array_equal(host["app_offsets"][:73].astype(np.int64), m["app_offsets"] + base)
    for name in ("lengths", "queue_ids", "flags", "expected"):
        assert np.array_equal(host[name][:73].astype(np.int64), m[name].astype(np.int64)), name
    assert np.array_equal(host["out"][:73], m["crcs"])
    assert np.array_equal(host["guids"][:16 * 73].reshape(73, 16), m["guids"])
    assert list(host["event_first"][:4]) == [0, 70, 73, 73]
    # and a refusal there names a byte beyond 4 GiB
    bad, offs = M.malformed("padding_5")
    kind, event, offset = M.model(bad, offs)["refused"]
    back[base:base + bad.size] = torch.from_numpy(bad).to(cuda)
    for sync in (True, False):
        rc, err, res, host = _raw(cuda, back[:base + bad.size], offs + base, 64, sync=sync)
        assert (res["refused_kind"], res["refused_event"], res["refused_offset"]) == \
            (kind, event, offset + base), res
        assert all(_canary(name, a) for name, a in host.items())
    del back, events
    torch.cuda.empty_cache()


# ---- header variants ---------------------------------------------------------

def test_header_variants(cuda):
    rng = np.random.default_rng(26)
    n = 70
    lens = rng.integers(0, 90, size=n)
    options = [M.payload(rng, 4 * int(k)) for k in rng.integers(0, 6, size=n)]
    plain = M.build_event(rng, lens)
    buf, offs = M.concat([M.long_event_header(plain), M.long_put_headers(plain),
                          M.build_event(rng, lens, options), M.with_cat_bits(plain)])
    m, host = _ok(cuda, buf, offs)
    assert m["n"] == 4 * n and np.array_equal(host["out"][:4 * n], m["crcs"])
    assert np.array_equal(m["expected"], m["crcs"])


# ---- verify ------------------------------------------------------------------

def test_verify_counts_corrupt_payloads_and_corrupt_header_crcs(cuda):
    rng = np.random.default_rng(27)
    n = 200
    buf, offs = M.concat([M.build_event(rng, rng.integers(1, 120, size=100)) for _ in range(2)])
    good = M.model(buf, offs)
    victims = [0, 64, n - 1]
    for what in ("payload", "header"):
        bad = buf.copy()
        for v in victims:
            at = int(good["app_offsets"][v])
            if what == "payload":
                bad[at] ^= 0x10
            else:
                hdr = [o + h for o, ev in ((offs[0], buf[:offs[1]]), (offs[1], buf[offs[1]:]))
                       for h in M.walk(ev)[0]][v]
                bad[hdr + 28] ^= 0x01
        m, host = _ok(cuda, bad, offs, n_bad=3, first_bad=0)
        differ = np.nonzero(host["out"][:n] != host["expected"][:n])[0]
        assert list(differ) == victims
        assert np.array_equal(host["out"][:n], m["crcs"])
        assert np.array_equal(host["expected"][:n], m["expected"])


def test_walk_only_leaves_the_launch_record(cuda):
    import torch
    rng = np.random.default_rng(28)
    buf, offs = M.concat([M.build_event(rng, rng.integers(1, 120, size=60)) for _ in range(3)])
    bad = buf.copy()
    bad[int(M.model(buf, offs)["app_offsets"][5])] ^= 1
    s = _side_stream(cuda)
    with torch.cuda.stream(s):
        arena = _t(cuda, buf, np.uint8)
        Crc32c.calculate_batch(arena, _t(cuda, [0, 64], np.int64), _t(cuda, [64, 100], np.uint32),
                               stream=s, seg_bytes=1024)
        before = last_launch(cuda.index, s, offsets=True)
        _ok(cuda, bad, offs, verify=False, stream=s)  # n_bad == 0: nothing was compared
        assert last_launch(cuda.index, s, offsets=True) == before


# ---- refusals ----------------------------------------------------------------

@pytest.mark.parametrize("name", M.VARIANTS)
def test_malformed_input_is_refused_like_the_host_walk(cuda, name):
    buf, offs = M.malformed(name)
    kind, event, _ = _refused(cuda, buf, offs, 64)
    assert event == (2 if name == "offsets_past_end" else 1)
    assert kind == M.model(buf, offs)["refused"][0]


def test_msg_cap_edge(cuda):
    rng = np.random.default_rng(29)
    buf, offs = M.concat([M.build_event(rng, ln) for ln in ([1, 2], [], [3, 4, 5], [])])
    _ok(cuda, buf, offs, cap=5)
    assert _refused(cuda, buf, offs, 4) == (M.K_MANY, 2, int(offs[2]))
    assert _refused(cuda, buf, offs, 0, verify=False) == (M.K_MANY, 0, 0)
    ev = M.build_event(rng, range(130))
    assert _refused(cuda, ev, None, 129) == (M.K_MANY, 0, 0)


def test_refusal_precedence(cuda):
    rng = np.random.default_rng(30)
    good = M.build_event(rng, [4, 5, 6])
    pad, typ = M._mutate("padding_0", good), M._mutate("type_3", good)
    buf, offs = M.concat([good, pad, typ, typ])
    assert _refused(cuda, buf, offs, 64)[:2] == (M.K_EVENT, 2)    # the lower kind
    buf, offs = M.concat([pad, good, pad] + [good] * 40 + [pad])
    assert _refused(cuda, buf, offs, 256)[:2] == (M.K_PAD, 0)     # the lower event
    buf, offs = M.concat([good, pad, good])
    assert _refused(cuda, buf, offs, 2)[:2] == (M.K_PAD, 1)       # before TOO_MANY_MESSAGES


def test_python_wrapper_raises_and_reports(cuda):
    import torch
    buf, offs = M.malformed("padding_5")
    kind, event, offset = M.model(buf, offs)["refused"]
    events, d_offs = _device_events(cuda, buf), _t(cuda, offs, np.int64)
    with pytest.raises(BmqCrcError, match="BMQCRC_PUT_UNPACK_PADDING") as e:
        unpack_events(events, d_offs)
    assert e.value.rc == N.BMQCRC_EINVAL
    s = _side_stream(cuda)
    with torch.cuda.stream(s):
        u = unpack_events(events, d_offs, msg_cap=32, stream=s, sync=False)
        assert u.lengths.numel() == 32 and u.guids.shape == (32, 16)
        res = last_put_unpack(cuda.index, s)
    assert (res["refused_kind"], res["refused_event"], res["refused_offset"]) == \
        (kind, event, offset)


# ---- state -------------------------------------------------------------------

def test_state(cuda):
    import torch
    rng = np.random.default_rng(31)
    host = rng.integers(0, 256, size=1 << 18, dtype=np.uint8)
    arena = torch.from_numpy(host).to(cuda)
    lens = rng.integers(1, 1025, size=3001).astype(np.uint32)
    offs = (rng.random(lens.size) * (host.size - 1100)).astype(np.int64)
    d_off, d_len = _t(cuda, offs, np.int64), _t(cuda, lens, np.uint32)
    doff = _t(cuda, np.concatenate([[0], np.cumsum(lens[:40])[:-1]]), np.int64)
    copy_dst = torch.zeros(int(lens[:40].sum()) + 16, dtype=torch.uint8, device=cuda)
    qids, guids, flags = P.random_meta(rng, 30)
    buf, evoffs = M.concat([M.build_event(rng, rng.integers(0, 300, size=50)) for _ in range(4)])
    s = _side_stream(cuda)
    with torch.cuda.stream(s):
        Crc32c.copy_batch(arena, d_off[:40], d_len[:40], copy_dst, doff, stream=s)
        pack_events(arena, d_off[:30], d_len[:30], _t(cuda, qids, np.int32),
                    _t(cuda, guids, np.uint8), _t(cuda, flags, np.uint8), stream=s)
        pack_records(arena, d_off[:30], d_len[:30],
                     _t(cuda, np.full((30, 5), 7), np.uint8), _t(cuda, guids, np.uint8),
                     file_key=b"\x11\x22\x33\x44\x55", lease_id=3, first_seq=2,
                     data_file_pos=40, stream=s)
        put, rec = last_put_pack(cuda.index, s), last_records_pack(cuda.index, s)
        assert last_put_unpack(cuda.index, s) == N.PutUnpackResult().as_dict()  # none yet on s
        _ok(cuda, buf, evoffs, stream=s)
        _ok(cuda, buf, evoffs, stream=s, sync=False)
        assert last_copy(cuda.index, s) == (40, 0, 40)
        assert last_put_pack(cuda.index, s) == put
        assert last_records_pack(cuda.index, s) == rec
        plan = last_launch(cuda.index, s, offsets=True)
        # a planned batch: planner and fold, nothing speculated, 64-bit offsets
        assert plan["kernels"] >= 2 and plan["spec"] == 0 and plan["offset_bits"] == 64, plan
        out = Crc32c.calculate_batch(arena, d_off, d_len, stream=s)
    s.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), P.host_crcs(host, offs, lens))


# ---- the loop closed ---------------------------------------------------------

def test_put_events_to_verified_partition_without_host_descriptors(cuda):
    rng = np.random.default_rng(32)
    n = 300
    key = bytes([9, 8, 7, 6, 5])
    buf, evoffs = M.concat([M.build_event(rng, rng.integers(0, 120, size=100)) for _ in range(3)])
    m = M.model(buf, evoffs)
    victim = next(i for i in range(100, n) if m["lengths"][i] > 0)
    kw = dict(file_key=b"\x11\x22\x33\x44\x55", lease_id=1, first_seq=2, data_file_pos=40,
              timestamp=0x6720EAB4)
    import torch
    for corrupt in (False, True):
        ev = buf.copy()
        if corrupt:
            ev[int(m["app_offsets"][victim])] ^= 0x40
        events = _device_events(cuda, ev)
        u = unpack_events(events, _t(cuda, evoffs, np.int64), msg_cap=n)
        res = last_put_unpack(cuda.index, torch.cuda.current_stream(cuda))
        assert (res["n_msgs"], res["n_bad"]) == (n, int(corrupt))
        qkeys = torch.from_numpy(np.frombuffer(key, np.uint8).copy()).to(cuda).repeat(n, 1)
        dst, jour, roff, crcs, rres = pack_records(events, u.app_offsets, u.lengths, qkeys,
                                                   u.guids, expected=u.expected, **kw)
        assert (rres["n_msgs"], rres["n_bad"], rres["refused_kind"]) == (n, int(corrupt), 0)
        if corrupt:
            assert res["first_bad"] == rres["first_bad"] == victim
        jf, df = wrap_partition(dst.cpu().numpy(), jour.cpu().numpy(),
                                np.frombuffer(key, np.uint8))
        got = S.verify_partition(jf, df)
        assert (got["recovery_rc"], got["n_messages"], got["n_bad"]) == (0, n, int(corrupt))
        if corrupt:
            assert list(got["bad_record_offsets"]) == [44 + 60 + REC * victim]


# ---- past one walk grid ---------------------------------
#
# pack_pool.py's messages (lengths 0..40 with every padding count, a handful of
# 200 to 700 bytes, one of 70,000 every 3,001) with random queue ids, GUIDs and
# flags, sent in test_grid_regimes.py's event splits.  The events and what
# walking them gives are put_unpack_model.unpack_fast's, which
# test_put_unpack_model.py holds to the loop model field for field.

@functools.lru_cache(maxsize=None)
def _pool_messages(n):
    src, soff, lens, ix = pack_pool.messages(n)
    _, poff, plen = pack_pool.pool()
    crcs = P.pooled_crcs(_pool_crcs(), ix)
    qids, guids, flags = P.random_meta(np.random.default_rng(9), n)
    for a in (crcs, qids, guids, flags):
        a.setflags(write=False)
    return (src, soff, lens, qids, guids, flags), crcs


@functools.lru_cache(maxsize=None)
def _pool_crcs():
    src, poff, plen = pack_pool.pool()
    return P.pool_crcs(src, poff, plen)


@functools.lru_cache(maxsize=None)
def _built(n, split):
    """unpack_fast's (events, event offsets, model) of the first n messages of
    the pool in the events G.ones or G.ragged: built once, shared, read-only."""
    msgs, crcs = _pool_messages(n)
    buf, offs, want = M.unpack_fast(*msgs, getattr(G, split)(n), crcs)
    for a in (buf, offs) + tuple(v for v in want.values() if isinstance(v, np.ndarray)):
        a.setflags(write=False)
    return buf, offs, want


BUILDS = [(G.N_WAVES, "ragged"), (G.N_FULL, "ragged"), (G.N_TILES, "ragged"),
          (G.N_FRAME, "ragged"), (G.N_FRAME, "ones"), (G.N_TILES, "ones")]


@pytest.fixture(scope="module")
def large():
    """The pool and every shared build, made before the first case that asks."""
    for key in BUILDS:
        _built(*key)


def _refusal(n, split, plants=(), msg_cap=None):
    """(events, event offsets, the refusal) of _built's events with `plants`."""
    buf, offs, _ = _built(n, split)
    buf, offs = buf.copy(), offs.copy()
    corrupt, suspects, _ = _planted(n, getattr(G, split)(n), plants)
    corrupt(buf, offs)
    return buf, offs, M.refused_fast(buf, offs, getattr(G, split)(n), suspects, msg_cap)


def _planted(n, first, plants):
    """(corrupt, suspects, header offsets) for unpack_fast of the (what, where)
    pairs `plants` (put_unpack_model.spoil)."""
    lens = _pool_messages(n)[0][2]
    hdr, _ = P.layout(lens, first)
    event = np.searchsorted(first, np.arange(n), side="right") - 1

    def corrupt(buf, offs):
        for what, at in plants:
            M.spoil(buf, offs, hdr, lens, what, at)
    suspects = set()
    for what, at in plants:
        e = at if what in ("offsets", "event_length") else int(event[at])
        suspects.update({e - 1, e} if what == "offsets" else {e})
    return corrupt, sorted(suspects), hdr


LARGE = {"waves-ragged": (G.N_WAVES, "ragged", 0),
         "full-ragged": (G.N_FULL, "ragged", 0),
         "tiles-ragged": (G.N_TILES, "ragged", 0),
         "frame-ragged": (G.N_FRAME, "ragged", 0),
         "frame-ones": (G.N_FRAME, "ones", 0),
         "tiles-null_outputs": (G.N_TILES, "ragged", 0),
         "frame-msg_cap_300000_above": (G.N_FRAME, "ragged", 300000)}


@pytest.mark.parametrize("name", sorted(LARGE))
def test_past_one_walk_grid(cuda, large, name):
    # RAGGED: events of 1, 63, 64, 65, 130 and 7 messages with empty events
    # first, last, 65 in a row and at event 4,096.  From N_FULL on a walk block
    # walks a second event and the scan a fifth tile; at N_FRAME a publish
    # thread copies a second message, and with an event per message a second
    # event_first entry, and the scan runs 513 tiles.
    n, split, above = LARGE[name]
    crcs = _pool_messages(n)[1]
    buf, offs, want = _built(n, split)
    assert buf.size <= 61 << 20 and want["n"] == n
    skip = ("queue_ids", "guids", "flags", "expected", "event_first") \
        if name == "tiles-null_outputs" else ()
    _, host = _ok(cuda, buf, offs, cap=n + above, model=want, skip=skip)
    assert np.array_equal(host["out"][:n], crcs)


def test_past_one_walk_grid_on_a_side_stream(cuda, large):
    import torch
    n = G.N_FULL
    crcs = _pool_messages(n)[1]
    buf, offs, want = _built(n, "ragged")
    torch.cuda.synchronize(cuda)
    s = _side_stream(cuda)
    with torch.cuda.stream(s):
        _, host = _ok(cuda, buf, offs, cap=n, model=want, sync=False, stream=s)
    assert np.array_equal(host["out"][:n], crcs)


def test_stored_crc_mismatches_in_both_steps_of_the_publish_loop(cuda, large):
    n = G.N_FRAME
    msgs, crcs = _pool_messages(n)
    victims = [10, n // 2, 2048 * 256]
    stored = crcs.copy()
    stored[victims] ^= 0x01000080
    buf, offs, want = _built(n, "ragged")
    buf = buf.copy()    # the shared events with other CRCs in three PutHeaders
    for v in victims:
        M.put32(buf, int(want["app_offsets"][v]) - 36 + 28, int(stored[v]))
    want = dict(want, expected=stored)
    _, host = _ok(cuda, buf, offs, cap=n, model=want, n_bad=3, first_bad=10)
    assert np.array_equal(host["out"][:n], crcs)
    assert np.flatnonzero(host["out"][:n] != host["expected"][:n]).tolist() == victims


def test_a_flipped_byte_of_the_long_message_is_counted(cuda, large):
    n, victim = G.N_WAVES, pack_pool.LONG_VISIT
    msgs, crcs = _pool_messages(n)
    src, soff, lens = msgs[:3]
    assert lens[victim] == pack_pool.LONG == 70000
    app = src[soff[victim]:soff[victim] + 70000].copy()
    app[60000] ^= 0x40
    true = crcs.copy()
    true[victim] = Crc32c.calculate(app.tobytes())
    hdr, _ = P.layout(lens, G.ragged(n))

    def flip(buf, offs):
        buf[int(hdr[victim]) + 36 + 60000] ^= 0x40

    buf, offs, want = M.unpack_fast(*msgs, G.ragged(n), true, stored=crcs, corrupt=flip)
    _, host = _ok(cuda, buf, offs, cap=n, model=want, n_bad=1, first_bad=victim)
    assert np.array_equal(host["out"][:n], true) and true[victim] != crcs[victim]


@pytest.mark.parametrize("which", ["both", "higher_alone"])
@pytest.mark.parametrize("what", M.PLANTS)
def test_the_walk_refuses_in_a_blocks_second_and_third_event(cuda, large, what, which):
    # one event per message: events 4,096.. are the walk blocks' second step,
    # 8,192.. their third; two refused events of different steps, or the
    # higher alone
    n, lo, hi = G.N_TILES, 4099, 9000
    lens = _pool_messages(n)[0][2]
    kind = 1 + M.PLANTS.index(what)
    plants, e = {"both": ([(what, hi), (what, lo)], lo), "higher_alone": ([(what, hi)], hi)}[which]
    buf, offs, refused = _refusal(n, "ones", plants)
    offset = int(offs[e]) + {"offsets": 0, "event_length": 0, "header_words": 8,
                             "padding": 8 + 36 + int(lens[e]) + 3 - int(lens[e]) % 4}[what]
    assert refused == (kind, e, offset)
    _refused(cuda, buf, offs, n, want=refused)


@pytest.mark.parametrize("which", ["alone", "next_to_the_lower_kind"])
@pytest.mark.parametrize("what", ["event_length", "header_words", "padding"])
def test_the_lower_kind_of_a_later_step_wins(cuda, large, what, which):
    # RAGGED: message 99 of event 4,097, a block's second event of 130
    # messages, refused alone, or next to a lower kind in a higher event of
    # the first step of another block
    n = G.N_TILES
    first = G.ragged(n)
    assert first[4098] - first[4097] == 130
    lo, hi = int(first[4097]) + 99, int(first[4500]) + 3
    hdr, _ = P.layout(_pool_messages(n)[0][2], first)
    per_event = what == "event_length"
    kind = 1 + M.PLANTS.index(what)
    plants, want = [(what, 4097 if per_event else lo)], (kind, 4097)
    if which != "alone":
        lower = M.PLANTS[kind - 2]
        plants.append((lower, 4500 if lower in ("offsets", "event_length") else hi))
        want = (kind - 1, 4500)
    buf, offs, refused = _refusal(n, "ragged", plants)
    assert refused[:2] == want
    if which == "alone" and not per_event:
        assert int(hdr[lo]) <= refused[2] < int(hdr[lo + 1])
    _refused(cuda, buf, offs, n, want=refused)


@pytest.mark.parametrize("name", ["frame-ones-last_event", "tiles-ragged-third_tile"])
def test_too_many_messages_from_late_tiles_of_the_scan(cuda, large, name):
    if name == "frame-ones-last_event":
        # one event per message at N_FRAME: the last event, in the scan's 513th tile
        n, split, e = G.N_FRAME, "ones", G.N_FRAME - 1
        cap = n - 1
    else:
        # RAGGED at N_TILES: msg_cap inside a 130-message event of the third tile
        n, split = G.N_TILES, "ragged"
        first = G.ragged(n)
        e, cap = G.cap_inside_the_third_tile(first)
        assert 2048 < e < 3072 and first[e] < cap < first[e + 1] - 1
    buf, offs, refused = _refusal(n, split, msg_cap=cap)
    assert refused == (M.K_MANY, e, int(offs[e]))
    _refused(cuda, buf, offs, cap, want=refused)
