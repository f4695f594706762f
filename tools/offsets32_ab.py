#!/usr/bin/env python3
"""64-bit against 32-bit offset descriptors (BMQCRC_F_OFFSETS32) on small
uniform messages, same process, alternated (GPU box).

  tools/offsets32_ab.py [--shapes 4Mx64,2Mx128,1Mx256] [--turns 4]
                        [--warmup 5] [--steps 20] [--copies 4]

Per shape: `copies` rotating copies of the batch (arena, both offset arrays,
lengths, out), so that every step reads its data and descriptors from HBM
(bench.py's method for 1M_x_256B), then `turns` turns of A B: `warmup`
untimed and `steps` timed steps of the 64-bit leg, then of the 32-bit leg,
fold-kernel time from BMQCRC_F_TIME_KERNEL.  A 256-message sample of each
leg's CRCs is checked against the CPU oracle.  One JSON line per leg: the
k_fold average of each turn (us), their range, and the derived ratio of bytes
moved to algorithmic bytes, (size + descriptors + 4) / (size + 4).

Run under `rocprofv3 --pmc FETCH_SIZE --kernel-trace` (and WRITE_SIZE, one
counter per run, one shape per run: --shapes) the two legs are told apart by
their kernels: the last template argument of k_fold is the offset form.

  tools/offsets32_ab.py --traffic <dir>

summarises such runs: <dir>/<shape>_<COUNTER>/run_counter_collection.csv ->
one JSON line per shape and leg with the measured bytes per launch (read =
2 x FETCH_SIZE KB x 1024 on gfx950, write = WRITE_SIZE KB x 1024), measured
and derived ratios to algorithmic bytes, and per shape the difference between
the legs in bytes per message."""
import argparse
import csv
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"4Mx64": (4 << 20, 64), "2Mx128": (2 << 20, 128), "1Mx256": (1 << 20, 256)}


def derived(size, desc):
    """Bytes moved over algorithmic bytes: a message's data, its descriptors
    (offset + length: 12 bytes, 8 with 32-bit offsets) and its CRC written,
    over data + CRC."""
    return (size + desc + 4) / (size + 4)


def measure(a):
    import numpy as np
    import torch
    import blazingmq_amd as bmq
    import oracle
    from blazingmq_amd import Crc32c
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev)
    for name in a.shapes.split(","):
        n, size = SHAPES[name]
        o64 = torch.arange(n, dtype=torch.int64, device=dev) * size
        copies = []
        for c in range(a.copies):
            arena = torch.empty(n * size, dtype=torch.uint8, device=dev)
            bmq.fill_synthetic(arena, 31 + c)
            copies.append((arena, o64.clone(), o64.to(torch.int32),
                           torch.full((n,), size, dtype=torch.int32, device=dev),
                           torch.empty(n, dtype=torch.int32, device=dev)))
        torch.cuda.synchronize(dev)
        turn = [0]

        def step(narrow, timed):
            arena, w, w32, lens, out = copies[turn[0] % a.copies]
            turn[0] += 1
            Crc32c.calculate_batch(arena, w32 if narrow else w, lens, None, out, stream=s,
                                   sync=False, time_kernel=timed,
                                   offset_shift=0 if narrow else None)
            return arena, out

        legs = {False: [], True: []}
        bad = {False: 0, True: 0}
        launch = {}
        for _ in range(a.turns):
            for narrow in (False, True):
                for _ in range(a.warmup):
                    step(narrow, False)
                torch.cuda.synchronize(dev)
                bmq.kernel_timing(0, s)  # reset
                for _ in range(a.steps):
                    arena, out = step(narrow, True)
                torch.cuda.synchronize(dev)
                ms, cnt = bmq.kernel_timing(0, s)
                legs[narrow].append(ms / max(cnt, 1) * 1e3)
                launch[narrow] = bmq.last_launch(0, s, offsets=True)
                # the last step's copy: a sample of its CRCs against the oracle
                idx = np.linspace(0, n - 1, 256).astype(np.int64)
                host = arena.cpu().numpy()
                exp = oracle.batch(host, idx * size, np.full(256, size, np.uint32), None, nthreads=4)
                bad[narrow] += int((out.cpu().numpy().view(np.uint32)[idx] != exp).sum())
        for narrow in (False, True):
            us = legs[narrow]
            print(json.dumps({
                "shape": name, "n": n, "size": size, "offset_bits": 32 if narrow else 64,
                "copies": a.copies, "warmup": a.warmup, "steps": a.steps,
                "k_fold_us_per_turn": [round(x, 2) for x in us],
                "k_fold_us_min": round(min(us), 2), "k_fold_us_max": round(max(us), 2),
                "alg_bytes": n * (size + 4),
                "derived_over_alg": round(derived(size, 8 if narrow else 12), 4),
                "last_launch": launch[narrow], "sample_mismatches": bad[narrow]}), flush=True)
        del copies
        torch.cuda.empty_cache()
    return 0


def leg_of(kernel_name):
    """32 or 64 from a k_fold kernel name (demangled or mangled), else None."""
    if "k_fold" not in kernel_name:
        return None
    m = re.search(r"k_fold<([^>]*)>", kernel_name)
    if m:
        return 32 if m.group(1).split(",")[-1].strip() == "true" else 64
    m = re.search(r"k_foldI.*Lb([01])EEv", kernel_name)
    return None if not m else (32 if m.group(1) == "1" else 64)


def traffic(root):
    for name, (n, size) in SHAPES.items():
        kb = {}
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            path = os.path.join(root, "%s_%s" % (name, counter), "run_counter_collection.csv")
            if not os.path.exists(path):
                continue
            for r in csv.DictReader(open(path)):
                leg = leg_of(r["Kernel_Name"])
                if leg is not None and r["Counter_Name"] == counter:
                    kb.setdefault((leg, counter), []).append(float(r["Counter_Value"]))
        alg = n * (size + 4)
        per_msg = {}
        for leg in (64, 32):
            if (leg, "FETCH_SIZE") not in kb or (leg, "WRITE_SIZE") not in kb:
                continue
            f, w = kb[(leg, "FETCH_SIZE")], kb[(leg, "WRITE_SIZE")]
            rd, wr = 2 * 1024 * sum(f) / len(f), 1024 * sum(w) / len(w)
            per_msg[leg] = (rd + wr) / n
            print(json.dumps({
                "shape": name, "offset_bits": leg, "launches": [len(f), len(w)],
                "hbm_read_bytes": rd, "hbm_write_bytes": wr, "alg_bytes": alg,
                "measured_over_alg": round((rd + wr) / alg, 4),
                "derived_over_alg": round(derived(size, 8 if leg == 32 else 12), 4),
                "read_spread_bytes_per_msg": round(2 * 1024 * (max(f) - min(f)) / n, 3),
                "bytes_per_msg": round((rd + wr) / n, 3)}))
        if len(per_msg) == 2:
            print(json.dumps({"shape": name, "saved_bytes_per_msg":
                              round(per_msg[64] - per_msg[32], 3), "derived": 4}))
    return 0


def main():
    p = argparse.ArgumentParser(description=__doc__,
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--shapes", default=",".join(SHAPES))
    p.add_argument("--turns", type=int, default=4)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--copies", type=int, default=4)
    p.add_argument("--traffic", metavar="DIR")
    a = p.parse_args()
    return traffic(a.traffic) if a.traffic else measure(a)


if __name__ == "__main__":
    sys.exit(main())
