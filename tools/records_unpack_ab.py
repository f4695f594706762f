#!/usr/bin/env python3
"""Journal and DATA records walked and verified on the device (unpack_records,
ABI 2.13) against its CRC pass alone, same process, alternated step by step
(GPU box).

  tools/records_unpack_ab.py [--shapes 64kx64K,1Mx256,4Mx64] [--warmup 5] [--steps 20]
                             [--copies N]

A shape is `messages x size`: uniform messages packed into DATA records and
journal MessageRecords on the device by pack_records (data_file_pos 40).
`copies` rotating sets of partitions (default: 4 for the small-message shapes,
1 for 64k x 64 KiB), so the small shapes read from HBM and not from the 256 MiB
cache.  Two legs alternate:

  crc_only  Crc32c.calculate_batch(plan=True) over the application-data
            offsets and lengths computed on the host beforehand: the CRC pass
            alone, a BMQCRC_F_DEVICE_PTRS | BMQCRC_F_PLAN batch
  unpack    unpack_records(verify=True, msg_cap=n): classify, place, the same
            CRC pass over the workspace's descriptors, the publish (and the
            wrapper's ten output tensors from torch's caching allocator)

each timed with device events around the whole leg, `steps` timed steps after
`warmup`.  After the last step the unpack's result (n messages, none bad,
nothing refused) and every array are compared with what was packed, and its
CRCs with the crc_only leg's.  One JSON line per leg: median, min and max
(us), payload GiB/s at the median.  A last line per shape gives unpack -
crc_only, unpack / crc_only and the crc_only leg's own min-max range."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = {"64kx64K": (64 << 10, 64 << 10), "1Mx256": (1 << 20, 256), "4Mx64": (4 << 20, 64)}
DEFAULT = "64kx64K,1Mx256,4Mx64"


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
    from blazingmq_amd import Crc32c, pack_records, unpack_records
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev)
    rng = np.random.default_rng(7)
    pos = 40
    ok = True
    for shape in a.shapes.split(","):
        n, size = SIZES[shape]
        total = n * size
        record = ((size + 12) // 8 + 1) * 8
        packed = record * n
        copies = a.copies or (1 if total >= 1 << 30 else 4)
        soff = torch.arange(n, dtype=torch.int64, device=dev) * size
        lens = torch.full((n,), size, dtype=torch.int32, device=dev)
        app = torch.arange(n, dtype=torch.int64, device=dev) * record + 12
        qkeys_h = rng.integers(1, 256, size=(n, 5), dtype=np.uint8)
        guids_h = rng.integers(1, 256, size=(n, 16), dtype=np.uint8)
        refs_h = rng.integers(0, 1 << 20, size=n, dtype=np.int64).astype(np.int32)
        stamps_h = rng.integers(0, 1 << 62, size=n, dtype=np.int64)
        dflags_h = rng.integers(0, 256, size=n, dtype=np.uint8)
        qkeys, guids, refs, stamps, dflags = (
            torch.from_numpy(x).to(dev) for x in (qkeys_h, guids_h, refs_h, stamps_h, dflags_h))
        src = torch.empty(total, dtype=torch.uint8, device=dev)
        sets = []
        for c in range(copies):
            bmq.fill_synthetic(src, 47 + c)
            dst, jour, _, _, _ = pack_records(
                src, soff, lens, qkeys, guids, file_key=b"\x11\x22\x33\x44\x55", lease_id=1,
                first_seq=2, data_file_pos=pos, ref_counts=refs, timestamps=stamps,
                data_flags=dflags, dst=torch.zeros(packed, dtype=torch.uint8, device=dev))
            sets.append((jour, dst, torch.empty(n, dtype=torch.int32, device=dev)))
        del src
        torch.cuda.synchronize(dev)
        turn = {"crc_only": 0, "unpack": 0}

        def step(leg):
            jour, dst, out = sets[turn[leg] % copies]
            turn[leg] += 1
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            res = None
            e0.record(s)
            if leg == "unpack":
                res = unpack_records(jour, dst, data_file_pos=pos, msg_cap=n, verify=True,
                                     stream=s, sync=False)
            else:
                Crc32c.calculate_batch(dst, app, lens, None, out, stream=s, sync=False, plan=True)
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
        state = bmq.last_records_unpack(0, s)
        good = state == dict(n_records=n, n_msgs=n, n_skipped=0, n_bad=0, first_bad=n,
                             refused_kind=0, refused_index=0)
        good = good and torch.equal(u.app_offsets, app) and torch.equal(u.lengths, lens)
        good = good and torch.equal(u.record_index,
                                    torch.arange(n, dtype=torch.int32, device=dev))
        good = good and torch.equal(u.queue_keys, qkeys) and torch.equal(u.guids, guids)
        good = good and torch.equal(u.data_flags, dflags) and torch.equal(u.ref_counts, refs)
        good = good and torch.equal(u.timestamps, stamps)
        good = good and torch.equal(u.crcs, last["crc_only"][0]) and torch.equal(u.crcs, u.expected)
        res = {}
        for leg in ("crc_only", "unpack"):
            us = times[leg]
            med = statistics.median(us)
            res[leg] = (med, min(us), max(us))
            print(json.dumps({
                "shape": shape, "n": n, "size": size, "leg": leg, "copies": copies,
                "warmup": a.warmup, "steps": a.steps, "us_median": round(med, 1),
                "us_min": round(min(us), 1), "us_max": round(max(us), 1),
                "payload_GiBps": round(total / 2**30 / (med * 1e-6), 1),
                "data_bytes": packed, "journal_bytes": 60 * n}), flush=True)
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
