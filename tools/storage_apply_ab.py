#!/usr/bin/env python3
"""STORAGE events applied on the device (apply_events, ABI 2.15) against the
payload-only lower bound, same process, alternated step by step (GPU box).

  tools/storage_apply_ab.py [--shapes 64kx64K_4096,1Mx256_4096,1Mx256_5] [--warmup 5]
                            [--steps 20] [--copies N] [--out FILE]

Per shape n x size_events: n DATA messages of `size` application bytes, packed
into DATA and journal records by pack_records and from there into STORAGE
events on the device, the messages spread evenly over the events.  `copies`
rotating sets of buffers (default: as many as 4 GiB of events hold, 4 at the
most), so the small shapes read from HBM and not from the 256 MiB cache.  Two legs alternate:

  copy_only  Crc32c.copy_batch over the same application data with source and
             destination offsets computed on the host beforehand: the payload
             pass alone, no walk, no record written
  apply      apply_events: two walks and the scan, the layout and its checks,
             the same payload pass, the frame (journal records, DataHeaders,
             padding, the per-message arrays); the wrapper's output tensors
             included

each timed with device events around the whole leg, `steps` timed steps after
`warmup`.  After the last step the applied journal run and DATA window are
compared with what pack_records wrote.  One JSON line per leg: median, min and
max (us), payload GiB/s at the median.  A last line per shape gives the bar
(asserted for 64kx64K_4096 only, reported for the rest): apply median <=
copy_only median + (copy_only max - min) + 35 us + 28.8 us -- 5 us for each of
the 7 launches the call adds to the copy, and for the two chain walks 2 x 16
steps (the messages of an event of that shape) at 0.9 us, the upper per-step
time DESIGN.md section 14 measured.  --out appends the lines to a file as
well."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"64kx64K_4096": (64 << 10, 64 << 10, 4096), "1Mx256_4096": (1 << 20, 256, 4096),
          "1Mx256_5": (1 << 20, 256, 5)}
ADDED_LAUNCHES = 7
LAUNCH_ALLOWANCE_US = 5.0 * ADDED_LAUNCHES
CHAIN_ALLOWANCE_US = 2 * 16 * 0.9
JPOS, DPOS, PARTITION = 44 + 60, 40, 1
KW = dict(file_key=b"\x0a\x0b\x0c\x0d\x0e", lease_id=7, first_seq=1000, data_file_pos=DPOS,
          timestamp=0x6720EAB4)


def build_events(torch, jour, dst, n, rec, n_events):
    """Events on the device from a record run and its DATA records of `rec`
    bytes each: event e holds messages [first[e], first[e + 1]).  Returns
    (events, event_offsets, first)."""
    dev = jour.device
    msg = 72 + rec
    first = [(n * e) // n_events for e in range(n_events + 1)]
    index = torch.arange(n, dtype=torch.int64, device=dev)
    sh = torch.zeros((n, 12), dtype=torch.uint8, device=dev)
    for k, word in ((0, msg // 4), (8, None)):
        w = index * 15 + JPOS // 4 if word is None else torch.full_like(index, word)
        for b in range(4):
            sh[:, k + b] = ((w >> (8 * (3 - b))) & 0xFF).to(torch.uint8)
    sh[:, 4], sh[:, 5], sh[:, 7] = (1 << 4) | 3, 1, PARTITION
    msgs = torch.cat([sh, jour.view(n, 60), dst.view(n, rec)], dim=1)
    del sh
    parts, offsets = [], [0]
    for e in range(n_events):
        k = first[e + 1] - first[e]
        size = 8 + k * msg
        head = torch.tensor(list(size.to_bytes(4, "big")) + [(1 << 6) | 8, 2, 0, 0],
                            dtype=torch.uint8, device=dev)
        parts += [head, msgs[first[e]:first[e + 1]].reshape(-1)]
        offsets.append(offsets[-1] + size)
    events = torch.cat(parts)
    return events, torch.tensor(offsets, dtype=torch.int64, device=dev), first


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
    from blazingmq_amd import Crc32c, apply_events, pack_records
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
        n, size, n_events = SHAPES[name]
        total = n * size
        rec = ((size + 12) // 8 + 1) * 8
        msg = 72 + rec
        copies = a.copies or max(1, min(4, (4 << 30) // (n * msg)))
        soff = torch.arange(n, dtype=torch.int64, device=dev) * size
        lens = torch.full((n,), size, dtype=torch.int32, device=dev)
        doff = torch.arange(n, dtype=torch.int64, device=dev) * rec + 12
        qkeys = torch.from_numpy(rng.integers(1, 256, size=(n, 5), dtype=np.uint8)).to(dev)
        guids = torch.from_numpy(rng.integers(1, 256, size=(n, 16), dtype=np.uint8)).to(dev)
        sets = []
        for c in range(copies):
            src = torch.empty(total, dtype=torch.uint8, device=dev)
            bmq.fill_synthetic(src, 41 + c)
            dst, jour, _, _, _ = pack_records(src, soff, lens, qkeys, guids, stream=s, **KW)
            del src
            events, offsets, first = build_events(torch, jour, dst, n, rec, n_events)
            event_of = torch.repeat_interleave(
                torch.arange(n_events, dtype=torch.int64, device=dev),
                torch.tensor(np.diff(first), dtype=torch.int64, device=dev))
            # application data of message i in the events: behind the event headers up to
            # its own, the messages before it, its StorageHeader, record and DataHeader
            app = 8 * (event_of + 1) + torch.arange(n, dtype=torch.int64, device=dev) * msg + 84
            sets.append((events, offsets, app, dst, jour,
                         torch.zeros(rec * n, dtype=torch.uint8, device=dev),
                         torch.zeros(60 * n, dtype=torch.uint8, device=dev),
                         torch.empty(n, dtype=torch.int32, device=dev)))
        torch.cuda.synchronize(dev)
        turn = {"copy_only": 0, "apply": 0}
        last_apply = None

        def step(leg):
            events, offsets, app, _, _, ddst, jdst, out = sets[turn[leg] % copies]
            which = turn[leg] % copies
            turn[leg] += 1
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            if leg == "apply":
                apply_events(events, offsets, partition_id=PARTITION, journal_pos=JPOS,
                             data_file_pos=DPOS, lease_id=KW["lease_id"],
                             seq=KW["first_seq"] - 1, msg_cap=n, journal_dst=jdst, data_dst=ddst,
                             stream=s, sync=False)
            else:
                Crc32c.copy_batch(events, app, lens, ddst, doff, None, out, stream=s, sync=False)
            e1.record(s)
            return e0, e1, which

        times = {"copy_only": [], "apply": []}
        for i in range(a.warmup + a.steps):
            for leg in ("copy_only", "apply"):
                e0, e1, which = step(leg)
                torch.cuda.synchronize(dev)
                if i >= a.warmup:
                    times[leg].append(e0.elapsed_time(e1) * 1e3)
                if leg == "apply":
                    last_apply = which
        # the last apply against what the packer wrote
        _, _, _, dst, jour, ddst, jdst, _ = sets[last_apply]
        state = bmq.last_storage_apply(0, s)
        good = state == dict(n_events=n_events, n_msgs=n, n_data=n, journal_bytes=60 * n,
                             data_bytes=rec * n, head_seq=KW["first_seq"] + n - 1,
                             head_lease_id=KW["lease_id"], refused_kind=0, n_bad=0, first_bad=n,
                             refused_event=0, refused_index=0, refused_offset=0)
        good = good and torch.equal(ddst, dst) and torch.equal(jdst, jour)
        res = {}
        for leg in ("copy_only", "apply"):
            us = times[leg]
            med = statistics.median(us)
            res[leg] = (med, min(us), max(us))
            emit({"shape": name, "n": n, "size": size, "events": n_events, "leg": leg,
                  "copies": copies, "warmup": a.warmup, "steps": a.steps,
                  "us_median": round(med, 1), "us_min": round(min(us), 1),
                  "us_max": round(max(us), 1),
                  "payload_GiBps": round(total / 2**30 / (med * 1e-6), 1)})
        a_med, a_min, a_max = res["copy_only"]
        allowed = a_med + (a_max - a_min) + LAUNCH_ALLOWANCE_US + CHAIN_ALLOWANCE_US
        within = res["apply"][0] <= allowed
        barred = name == "64kx64K_4096"
        emit({"shape": name, "apply_over_copy_only": round(res["apply"][0] / a_med, 3),
              "apply_minus_copy_only_us": round(res["apply"][0] - a_med, 1),
              "copy_only_range_us": round(a_max - a_min, 1),
              "launch_allowance_us": LAUNCH_ALLOWANCE_US,
              "chain_allowance_us": CHAIN_ALLOWANCE_US, "allowed_us": round(allowed, 1),
              "apply_within_bar": within, "bar_applies": barred,
              "apply_matches_packer": bool(good)})
        ok = ok and good and (within or not barred)
        del sets
        torch.cuda.empty_cache()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
