#!/usr/bin/env python3
"""PUT-event packing on the device (pack_events, ABI 2.10) against its
payload-only lower bound, same process, alternated step by step (GPU box).

  tools/put_pack_ab.py [--shapes 64kx64K,1Mx256,4Mx64] [--warmup 5] [--steps 20]
                       [--copies N]

Per shape: messages contiguous in the source, destination events of the
default cap (66 MiB), as many messages in each as fit.  `copies` rotating sets
of buffers (default: enough for 1 GiB of source), so the small shapes read
from HBM and not from the 256 MiB cache.  Two legs alternate:

  copy_only  Crc32c.copy_batch with dst_offsets of the same layout computed on
             the host beforehand: the payload pass alone, no framing written
  pack       pack_events: layout on the device, the same payload pass, frame

each timed with device events around the whole leg, `steps` timed steps after
`warmup`.  After the last step the pack's event_offsets are compared with the
host layout and 64 sampled messages (header, data, padding) with
PutEventBuilder's bytes.  One JSON line per leg: median, min and max (us),
payload GiB/s at the median, framing bytes as a share of the bytes written.
A last line per shape gives the bar (asserted for 64k x 64 KiB only, reported
for the rest): pack median <= copy_only median + (copy_only max - min) + 20 us,
the 20 us standing for the four added launches."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"64kx64K": (64 << 10, 64 << 10), "1Mx256": (1 << 20, 256), "4Mx64": (4 << 20, 64)}
CAP = 66 << 20
LAUNCH_ALLOWANCE_US = 20.0


def main():
    p = argparse.ArgumentParser(description=__doc__,
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--shapes", default=",".join(SHAPES))
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--copies", type=int, default=0)
    a = p.parse_args()
    import numpy as np
    import torch
    import blazingmq_amd as bmq
    from blazingmq_amd import Crc32c, pack_events
    from blazingmq_amd.put_event import PutEventBuilder
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev)
    rng = np.random.default_rng(5)
    ok = True
    for name in a.shapes.split(","):
        n, size = SHAPES[name]
        total = n * size
        framed = 36 + (size // 4 + 1) * 4
        per_event = (CAP - 8) // framed
        ef = np.append(np.arange(0, n, per_event), n).astype(np.int64)
        n_events = ef.size - 1
        hdr = 8 * (np.searchsorted(ef, np.arange(n), side="right")) + framed * np.arange(n)
        packed = 8 * n_events + framed * n
        copies = a.copies or max(1, (1 << 30) // total)
        soff = torch.arange(n, dtype=torch.int64, device=dev) * size
        lens = torch.full((n,), size, dtype=torch.int32, device=dev)
        doff = torch.from_numpy(hdr + 36).to(dev)
        d_ef = torch.from_numpy(ef).to(dev)
        qids_h = rng.integers(-2**31, 2**31, size=n, dtype=np.int64).astype(np.int32)
        guids_h = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
        flags_h = rng.integers(0, 16, size=n, dtype=np.uint8)
        qids, guids, flags = (torch.from_numpy(x).to(dev) for x in (qids_h, guids_h, flags_h))
        sets = []
        for c in range(copies):
            src = torch.empty(total, dtype=torch.uint8, device=dev)
            bmq.fill_synthetic(src, 41 + c)
            sets.append((src, torch.zeros(packed, dtype=torch.uint8, device=dev),
                         torch.empty(n, dtype=torch.int32, device=dev)))
        torch.cuda.synchronize(dev)
        turn = {"copy_only": 0, "pack": 0}
        last_pack = None

        def step(leg):
            src, dst, out = sets[turn[leg] % copies]
            turn[leg] += 1
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            res = None
            e0.record(s)
            if leg == "pack":
                res = pack_events(src, soff, lens, qids, guids, flags, d_ef, None, dst, out,
                                  stream=s, sync=False)
            else:
                Crc32c.copy_batch(src, soff, lens, dst, doff, None, out, stream=s, sync=False)
            e1.record(s)
            return e0, e1, (src, res)

        times = {"copy_only": [], "pack": []}
        for i in range(a.warmup + a.steps):
            for leg in ("copy_only", "pack"):
                e0, e1, last = step(leg)
                torch.cuda.synchronize(dev)
                if i >= a.warmup:
                    times[leg].append(e0.elapsed_time(e1) * 1e3)
                if leg == "pack":
                    last_pack = last
        # the last pack against the host: event offsets, then sampled messages
        src, (dst, evoff, out) = last_pack
        state = bmq.last_put_pack(0, s)
        good = state == (n, n_events, packed, 0, 0)
        good = good and np.array_equal(evoff.cpu().numpy(), 8 * np.arange(ef.size) + framed * ef)
        for j in np.linspace(0, n - 1, 64).astype(np.int64):
            b = PutEventBuilder(defer_crc=False)
            b.pack_message(src[int(j) * size:(int(j) + 1) * size].cpu().numpy().tobytes(),
                           queue_id=int(qids_h[j]), guid=bytes(guids_h[j]), flags=int(flags_h[j]))
            exp = b.finalize()[8:]
            got = dst[int(hdr[j]):int(hdr[j]) + framed].cpu().numpy()
            good = good and np.array_equal(got, exp)
        res = {}
        for leg in ("copy_only", "pack"):
            us = times[leg]
            med = statistics.median(us)
            res[leg] = (med, min(us), max(us))
            print(json.dumps({
                "shape": name, "n": n, "size": size, "events": int(n_events), "leg": leg,
                "copies": copies, "warmup": a.warmup, "steps": a.steps,
                "us_median": round(med, 1), "us_min": round(min(us), 1),
                "us_max": round(max(us), 1),
                "payload_GiBps": round(total / 2**30 / (med * 1e-6), 1),
                "bytes_written": packed if leg == "pack" else total,
                "framing_share": round((packed - total) / packed, 4) if leg == "pack" else 0.0}),
                flush=True)
        a_med, a_min, a_max = res["copy_only"]
        within = res["pack"][0] <= a_med + (a_max - a_min) + LAUNCH_ALLOWANCE_US
        barred = name == "64kx64K"
        print(json.dumps({"shape": name, "pack_over_copy_only": round(res["pack"][0] / a_med, 3),
                          "pack_minus_copy_only_us": round(res["pack"][0] - a_med, 1),
                          "copy_only_range_us": round(a_max - a_min, 1),
                          "pack_within_bar": within, "bar_applies": barred,
                          "pack_matches_builder": bool(good)}), flush=True)
        ok = ok and good and (within or not barred)
        del sets
        torch.cuda.empty_cache()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
