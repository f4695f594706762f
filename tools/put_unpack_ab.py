#!/usr/bin/env python3
"""PUT events walked and verified on the device (unpack_events, ABI 2.12)
against its CRC pass alone, same process, alternated step by step (GPU box).

  tools/put_unpack_ab.py [--shapes 64kx64K/63,64kx64K/4096,1Mx256/5,1Mx256/4096,4Mx64/4096]
                         [--warmup 5] [--steps 20] [--copies N]

A shape is `messages x size / events`: uniform messages, spread evenly over
the events, packed into PUT events on the device by pack_events.  `copies`
rotating sets of event buffers (default: 4 for the small-message shapes, 1 for
64k x 64 KiB), so the small shapes read from HBM and not from the 256 MiB
cache.  Two legs alternate:

  crc_only  Crc32c.calculate_batch(plan=True) over the application-data
            offsets and lengths computed on the host beforehand: the CRC pass
            alone, a BMQCRC_F_DEVICE_PTRS | BMQCRC_F_PLAN batch
  unpack    unpack_events(verify=True, msg_cap=n): both walks, the scan, the
            same CRC pass over the workspace's descriptors, the publish (and
            the wrapper's eight output tensors from torch's caching allocator)

each timed with device events around the whole leg, `steps` timed steps after
`warmup`.  After the last step the unpack's result (n messages, none bad,
nothing refused), its app_offsets, lengths, queue ids, GUIDs, flags and
event_first are compared with what was packed, and its CRCs with the crc_only
leg's.  One JSON line per leg: median, min and max (us), payload GiB/s at the
median.  A last line per shape gives unpack - crc_only and unpack / crc_only.
Nothing is barred: the few-event shapes walk a serial chain per event and are
expected to lose."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = {"64kx64K": (64 << 10, 64 << 10), "1Mx256": (1 << 20, 256), "4Mx64": (4 << 20, 64)}
DEFAULT = "64kx64K/63,64kx64K/4096,1Mx256/5,1Mx256/4096,4Mx64/4096"


def main():
    p = argparse.ArgumentParser(description=__doc__,
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--shapes", default=DEFAULT)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--copies", type=int, default=0)
    a = p.parse_args()
    import numpy as np
    import torch
    import blazingmq_amd as bmq
    from blazingmq_amd import Crc32c, pack_events, unpack_events
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev)
    rng = np.random.default_rng(6)
    ok = True
    for shape in a.shapes.split(","):
        name, n_events = shape.split("/")
        n_events = int(n_events)
        n, size = SIZES[name]
        total = n * size
        framed = 36 + (size // 4 + 1) * 4
        per_event = -(-n // n_events)
        ef = np.append(np.arange(0, n, per_event), n).astype(np.int64)
        assert ef.size - 1 == n_events, (shape, ef.size - 1)
        hdr = 8 * (np.searchsorted(ef, np.arange(n), side="right")) + framed * np.arange(n)
        packed = 8 * n_events + framed * n
        copies = a.copies or (1 if total >= 1 << 30 else 4)
        soff = torch.arange(n, dtype=torch.int64, device=dev) * size
        lens = torch.full((n,), size, dtype=torch.int32, device=dev)
        app = torch.from_numpy(hdr + 36).to(dev)
        d_ef = torch.from_numpy(ef).to(dev)
        qids_h = rng.integers(-2**31, 2**31, size=n, dtype=np.int64).astype(np.int32)
        guids_h = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
        flags_h = rng.integers(0, 16, size=n, dtype=np.uint8)
        qids, guids, flags = (torch.from_numpy(x).to(dev) for x in (qids_h, guids_h, flags_h))
        src = torch.empty(total, dtype=torch.uint8, device=dev)
        sets = []
        for c in range(copies):
            bmq.fill_synthetic(src, 43 + c)
            events, evoff, _ = pack_events(src, soff, lens, qids, guids, flags, d_ef,
                                           dst=torch.zeros(packed, dtype=torch.uint8, device=dev))
            sets.append((events, torch.empty(n, dtype=torch.int32, device=dev)))
        del src
        torch.cuda.synchronize(dev)
        turn = {"crc_only": 0, "unpack": 0}

        def step(leg):
            events, out = sets[turn[leg] % copies]
            turn[leg] += 1
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            res = None
            e0.record(s)
            if leg == "unpack":
                res = unpack_events(events, evoff, msg_cap=n, verify=True, stream=s, sync=False)
            else:
                Crc32c.calculate_batch(events, app, lens, None, out, stream=s, sync=False,
                                       plan=True)
            e1.record(s)
            return e0, e1, (out, res)

        times = {"crc_only": [], "unpack": []}
        last = {}
        for i in range(a.warmup + a.steps):
            for leg in ("crc_only", "unpack"):
                e0, e1, last[leg] = step(leg)
                torch.cuda.synchronize(dev)
                if i >= a.warmup:
                    times[leg].append(e0.elapsed_time(e1) * 1e3)
        # the last unpack against what was packed, and against the crc_only leg
        # (both legs' last steps read the same set: they alternate)
        u = last["unpack"][1]
        state = bmq.last_put_unpack(0, s)
        good = state == dict(n_events=n_events, n_msgs=n, n_bad=0, first_bad=n, refused_kind=0,
                             refused_event=0, refused_offset=0)
        good = good and torch.equal(u.app_offsets, app) and torch.equal(u.lengths, lens)
        good = good and torch.equal(u.queue_ids, qids) and torch.equal(u.guids, guids)
        good = good and torch.equal(u.flags, flags) and torch.equal(u.event_first, d_ef)
        good = good and torch.equal(u.crcs, last["crc_only"][0]) and torch.equal(u.crcs, u.expected)
        res = {}
        for leg in ("crc_only", "unpack"):
            us = times[leg]
            med = statistics.median(us)
            res[leg] = (med, min(us), max(us))
            print(json.dumps({
                "shape": shape, "n": n, "size": size, "events": n_events, "leg": leg,
                "copies": copies, "warmup": a.warmup, "steps": a.steps,
                "us_median": round(med, 1), "us_min": round(min(us), 1),
                "us_max": round(max(us), 1),
                "payload_GiBps": round(total / 2**30 / (med * 1e-6), 1),
                "event_bytes": packed}), flush=True)
        a_med = res["crc_only"][0]
        print(json.dumps({"shape": shape,
                          "unpack_over_crc_only": round(res["unpack"][0] / a_med, 3),
                          "unpack_minus_crc_only_us": round(res["unpack"][0] - a_med, 1),
                          "crc_only_range_us": round(res["crc_only"][2] - res["crc_only"][1], 1),
                          "unpack_matches_packed": bool(good)}), flush=True)
        ok = ok and good
        del sets, u, last
        torch.cuda.empty_cache()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
