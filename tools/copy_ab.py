#!/usr/bin/env python3
"""Fused copy + CRC (Crc32c.copy_batch) against the two passes it replaces,
same process, alternated step by step (GPU box).

  tools/copy_ab.py [--shapes 64kx64K,64kx64K+0,1Mx256,4Mx64] [--warmup 5]
                   [--steps 20] [--copies N]

Per shape: messages contiguous in the source; the destination contiguous at
+3 bytes (the misaligned case: every load is misaligned against its store),
or at +0 for the shapes named `+0`.  `copies` rotating sets of buffers
(default: enough for 1 GiB of source, as bench.py --rotate does), so the small
shapes read from HBM and not from the 256 MiB cache.  Two legs alternate:

  two_pass  Crc32c.calculate_batch, then dst.copy_(src) of the same bytes
  fused     Crc32c.copy_batch

each timed with device events around the whole leg, `steps` timed steps after
`warmup`.  The last fused step's destination is compared with the source and
a 256-message sample of both legs' CRCs with the CPU oracle.  One JSON line
per leg: median, min and max (us), payload GiB/s at the median, and the bytes
the leg has to move (two_pass 3 x payload + 4 n, fused 2 x payload + 4 n) over
the median as a share of 8 TB/s.  A last line per shape gives the verdict of
the bar: fused median <= two_pass median + (two_pass max - two_pass min)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"64kx64K": (64 << 10, 64 << 10, 3), "64kx64K+0": (64 << 10, 64 << 10, 0),
          "1Mx256": (1 << 20, 256, 3), "4Mx64": (4 << 20, 64, 3)}
PEAK = 8e12


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
    import oracle
    from blazingmq_amd import Crc32c
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev)
    for name in a.shapes.split(","):
        n, size, shift = SHAPES[name]
        total = n * size
        copies = a.copies or max(1, (1 << 30) // total)
        soff = torch.arange(n, dtype=torch.int64, device=dev) * size
        doff = soff + shift
        lens = torch.full((n,), size, dtype=torch.int32, device=dev)
        sets = []
        for c in range(copies):
            src = torch.empty(total, dtype=torch.uint8, device=dev)
            bmq.fill_synthetic(src, 41 + c)
            sets.append((src, torch.zeros(total + 16, dtype=torch.uint8, device=dev),
                         torch.empty(n, dtype=torch.int32, device=dev)))
        torch.cuda.synchronize(dev)
        turn = {"two_pass": 0, "fused": 0}

        def step(leg):
            src, dst, out = sets[turn[leg] % copies]
            turn[leg] += 1
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            if leg == "fused":
                Crc32c.copy_batch(src, soff, lens, dst, doff, None, out, stream=s, sync=False)
            else:
                Crc32c.calculate_batch(src, soff, lens, None, out, stream=s, sync=False)
                dst[shift:shift + total].copy_(src)
            e1.record(s)
            return e0, e1, (src, dst, out)

        times = {"two_pass": [], "fused": []}
        bad = {}
        for i in range(a.warmup + a.steps):
            for leg in ("two_pass", "fused"):
                e0, e1, last = step(leg)
                torch.cuda.synchronize(dev)
                if i >= a.warmup:
                    times[leg].append(e0.elapsed_time(e1) * 1e3)
                if i == a.warmup + a.steps - 1:
                    src, dst, out = last
                    idx = np.linspace(0, n - 1, 256).astype(np.int64)
                    host = np.concatenate([src[int(j) * size:(int(j) + 1) * size].cpu().numpy()
                                           for j in idx])
                    exp = oracle.batch(host, np.arange(256) * size,
                                       np.full(256, size, np.uint32), None, nthreads=8)
                    bad[leg] = int((out.cpu().numpy().view(np.uint32)[idx] != exp).sum())
                    if leg == "fused":
                        dst.zero_()
                        Crc32c.copy_batch(src, soff, lens, dst, doff, None, out, stream=s)
                        bad["dst_equal"] = bool(torch.equal(dst[shift:shift + total], src)) and \
                            int(dst[:shift].sum()) == 0 and int(dst[shift + total:].sum()) == 0
        res = {}
        for leg in ("two_pass", "fused"):
            us = times[leg]
            med = statistics.median(us)
            moved = (3 if leg == "two_pass" else 2) * total + 4 * n
            res[leg] = (med, min(us), max(us))
            print(json.dumps({
                "shape": name, "n": n, "size": size, "dst_shift": shift, "leg": leg,
                "copies": copies, "warmup": a.warmup, "steps": a.steps,
                "us_median": round(med, 1), "us_min": round(min(us), 1),
                "us_max": round(max(us), 1),
                "payload_GiBps": round(total / 2**30 / (med * 1e-6), 1),
                "bytes_moved": moved,
                "share_of_8TBps": round(moved / (med * 1e-6) / PEAK, 3),
                "sample_mismatches": bad[leg]}), flush=True)
        a_med, a_min, a_max = res["two_pass"]
        print(json.dumps({"shape": name, "fused_over_two_pass": round(res["fused"][0] / a_med, 3),
                          "two_pass_range_us": round(a_max - a_min, 1),
                          "fused_within_bar": res["fused"][0] <= a_med + (a_max - a_min),
                          "dst_equals_src": bad["dst_equal"]}), flush=True)
        del sets
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
