#!/usr/bin/env python3
"""DATA and journal records packed on the device (pack_records, ABI 2.11)
against the payload-only lower bound, same process, alternated step by step
(GPU box).

  tools/records_pack_ab.py [--shapes 64kx64K,1Mx256,4Mx64] [--warmup 5] [--steps 20]
                           [--copies N] [--out FILE]

Per shape: messages contiguous in the source, DATA records back to back.
`copies` rotating sets of buffers (default: enough for 1 GiB of source), so the
small shapes read from HBM and not from the 256 MiB cache.  Two legs alternate:

  copy_only  Crc32c.copy_batch with dst_offsets of the same layout computed on
             the host beforehand: the payload pass alone, no record written
  pack       pack_records: layout on the device, the same payload pass, frame
             (DataHeaders, padding, journal records)

each timed with device events around the whole leg, `steps` timed steps after
`warmup`.  After the last step the pack's record_offsets are compared with the
host layout and 64 sampled messages (DATA record and journal record) with
PartitionWriter's bytes.  One JSON line per leg: median, min and max (us),
payload GiB/s at the median, framing bytes as a share of the bytes written.
A last line per shape gives the bar (asserted for 64k x 64 KiB only, reported
for the rest): pack median <= copy_only median + (copy_only max - min) + 15 us,
the 15 us standing for the three added launches at 5 us each.  --out appends
the lines to a file as well."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"64kx64K": (64 << 10, 64 << 10), "1Mx256": (1 << 20, 256), "4Mx64": (4 << 20, 64)}
ADDED_LAUNCHES = 3
LAUNCH_ALLOWANCE_US = 5.0 * ADDED_LAUNCHES
KW = dict(file_key=b"\x0a\x0b\x0c\x0d\x0e", lease_id=7, first_seq=1000, data_file_pos=40,
          timestamp=0x6720EAB4)


def main():
    p = argparse.ArgumentParser(description=__doc__,
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--shapes", default=",".join(SHAPES))
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--copies", type=int, default=0)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import numpy as np
    import torch
    import blazingmq_amd as bmq
    from blazingmq_amd import Crc32c, pack_records
    from blazingmq_amd.storage import PartitionWriter
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev)
    rng = np.random.default_rng(5)
    sink = open(a.out, "a") if a.out else None

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    ok = True
    for name in a.shapes.split(","):
        n, size = SHAPES[name]
        total = n * size
        rec = ((size + 12) // 8 + 1) * 8
        packed = rec * n
        copies = a.copies or max(1, (1 << 30) // total)
        soff = torch.arange(n, dtype=torch.int64, device=dev) * size
        lens = torch.full((n,), size, dtype=torch.int32, device=dev)
        doff = torch.arange(n, dtype=torch.int64, device=dev) * rec + 12
        qkeys_h = rng.integers(1, 256, size=(n, 5), dtype=np.uint8)
        guids_h = rng.integers(1, 256, size=(n, 16), dtype=np.uint8)
        qkeys, guids = torch.from_numpy(qkeys_h).to(dev), torch.from_numpy(guids_h).to(dev)
        sets = []
        for c in range(copies):
            src = torch.empty(total, dtype=torch.uint8, device=dev)
            bmq.fill_synthetic(src, 41 + c)
            sets.append((src, torch.zeros(packed, dtype=torch.uint8, device=dev),
                         torch.zeros(60 * n, dtype=torch.uint8, device=dev),
                         torch.empty(n, dtype=torch.int32, device=dev)))
        torch.cuda.synchronize(dev)
        turn = {"copy_only": 0, "pack": 0}
        last_pack = None

        def step(leg):
            src, dst, jour, out = sets[turn[leg] % copies]
            turn[leg] += 1
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            res = None
            e0.record(s)
            if leg == "pack":
                res = pack_records(src, soff, lens, qkeys, guids, dst=dst, journal_dst=jour,
                                   out=out, stream=s, sync=False, **KW)
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
        # the last pack against the host: record offsets, then sampled messages
        src, (dst, jour, roff, out, _) = last_pack
        state = bmq.last_records_pack(0, s)
        good = state == dict(n_msgs=n, data_bytes=packed, journal_bytes=60 * n, n_bad=0,
                             first_bad=n, refused_kind=0, refused_index=0)
        good = good and np.array_equal(roff.cpu().numpy(), rec * np.arange(n + 1))
        for j in np.linspace(0, n - 1, 64).astype(np.int64):
            j = int(j)
            w = PartitionWriter(lease_id=KW["lease_id"], timestamp=KW["timestamp"])
            w.seq, w.dpos = KW["first_seq"] + j - 1, KW["data_file_pos"] + rec * j
            w.message(src[j * size:(j + 1) * size].cpu().numpy().tobytes(), bytes(qkeys_h[j]),
                      guid=bytes(guids_h[j]), file_key=KW["file_key"])
            good = good and dst[rec * j:rec * (j + 1)].cpu().numpy().tobytes() == w.data[-1]
            good = good and jour[60 * j:60 * (j + 1)].cpu().numpy().tobytes() == w.recs[-1]
        res = {}
        for leg in ("copy_only", "pack"):
            us = times[leg]
            med = statistics.median(us)
            res[leg] = (med, min(us), max(us))
            written = packed + 60 * n if leg == "pack" else total
            emit({"shape": name, "n": n, "size": size, "leg": leg, "copies": copies,
                  "warmup": a.warmup, "steps": a.steps, "us_median": round(med, 1),
                  "us_min": round(min(us), 1), "us_max": round(max(us), 1),
                  "payload_GiBps": round(total / 2**30 / (med * 1e-6), 1),
                  "bytes_written": written,
                  "framing_share": round((written - total) / written, 4)})
        a_med, a_min, a_max = res["copy_only"]
        within = res["pack"][0] <= a_med + (a_max - a_min) + LAUNCH_ALLOWANCE_US
        barred = name == "64kx64K"
        emit({"shape": name, "pack_over_copy_only": round(res["pack"][0] / a_med, 3),
              "pack_minus_copy_only_us": round(res["pack"][0] - a_med, 1),
              "copy_only_range_us": round(a_max - a_min, 1),
              "launch_allowance_us": LAUNCH_ALLOWANCE_US,
              "pack_within_bar": within, "bar_applies": barred,
              "pack_matches_writer": bool(good)})
        ok = ok and good and (within or not barred)
        del sets
        torch.cuda.empty_cache()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
