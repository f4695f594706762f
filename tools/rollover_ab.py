#!/usr/bin/env python3
"""A device-resident partition rolled over on the device (rollover_records, ABI
2.18) against the payload-only lower bound, same process, alternated step by
step (GPU box).

  tools/rollover_ab.py [--shapes 64kx64K_half,1Mx256_confirms_half] [--warmup 5]
                       [--steps 20] [--copies N] [--out FILE]

Shapes:
  64kx64K_half           65,536 MESSAGE records of 64 KiB written by
                         pack_records, no other record; every second one kept
                         (keep[], CONFIRMS_AS_KEPT)
  1Mx256_confirms_half   1,048,576 MESSAGE records of 256 bytes, each followed by
                         its CONFIRM record (2,097,152 records); every second
                         message kept and CONFIRMS_FOLLOW_MESSAGES: the join
                         decides the CONFIRM records
  1Mx256_confirms_half_as_kept   (not in the default list) the same records and
                         the same outcome with CONFIRMS_AS_KEPT and keep[] set on
                         the kept messages' CONFIRM records: what the join costs
                         is the difference
`copies` rotating sets of buffers (default: as many as 4 GiB of new DATA window
hold, 4 at the most), so the small shape reads from HBM and not from the
256 MiB cache.  Two legs alternate:

  copy_only  Crc32c.copy_batch over the kept messages' application data with
             source and destination offsets computed on the host beforehand:
             the payload pass alone, no record classified, no header written
  rollover   rollover_records with `dst` and `journal_dst` given: the
             classification, the join, the layout and its checks, the same
             payload pass over the record slots, the frame (journal records,
             DataHeaders, padding, the arrays); the wrapper's output tensors
             included

each timed with device events around the whole leg, `steps` timed steps after
`warmup`.  After the last step both destinations are compared with what torch
builds from the same records.  One JSON line per leg: median, min and max (us),
payload GiB/s at the median.  A last line per shape gives the bar (asserted for
64kx64K_half only, reported for the other): rollover median <= copy_only median
+ (copy_only max - min) + 5 us for each launch the call adds around the copy --
the 5 kernels (classify, count, check, seal, frame) and the memset of its
counters, 30 us; in FOLLOW mode the memset of the hash too, 35 us.  --out
appends the lines to a file as well."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"64kx64K_half": (64 << 10, 64 << 10, False, False),
          "1Mx256_confirms_half": (1 << 20, 256, True, True),
          "1Mx256_confirms_half_as_kept": (1 << 20, 256, True, False)}
DEFAULT_SHAPES = "64kx64K_half,1Mx256_confirms_half"
DPOS = 40
KW = dict(file_key=b"\x0a\x0b\x0c\x0d\x0e", lease_id=7, first_seq=1000, data_file_pos=DPOS,
          timestamp=0x6720EAB4)
BARRED = "64kx64K_half"


def confirms_of(torch, jour, n):
    """One CONFIRM record per MESSAGE record of `jour`, with its GUID and queue
    key and the sequence numbers behind the messages'."""
    m = jour.view(n, 60)
    c = torch.zeros_like(m)
    c[:, 0] = 2 << 4
    seq = torch.arange(n, dtype=torch.int64, device=jour.device) + (1 << 24)
    for b in range(4):
        c[:, 4 + b] = ((seq >> (8 * (3 - b))) & 0xFF).to(torch.uint8)
    c[:, 8:20] = m[:, 8:20]            # lease id, timestamp
    c[:, 22:27] = m[:, 22:27]          # queue key
    c[:, 32:48] = m[:, 36:52]          # GUID
    c[:, 56:60] = m[:, 56:60]          # magic
    return torch.stack([m, c], 1).reshape(-1)


def main():
    p = argparse.ArgumentParser(description=__doc__,
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--shapes", default=DEFAULT_SHAPES)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--copies", type=int, default=0)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import numpy as np
    import torch
    import blazingmq_amd as bmq
    from blazingmq_amd import Crc32c, pack_records, rollover_records
    from blazingmq_amd import storage as S
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
        n, size, with_confirms, follow = SHAPES[name]
        rec = ((size + 12) // 8 + 1) * 8
        kept = torch.arange(1, n, 2, dtype=torch.int64, device=dev)     # every second message
        k = kept.numel()
        total = k * size
        new_bytes = k * rec
        copies = a.copies or max(1, min(4, (4 << 30) // new_bytes))
        soff = torch.arange(n, dtype=torch.int64, device=dev) * size
        lens = torch.full((n,), size, dtype=torch.int32, device=dev)
        qkeys = torch.from_numpy(rng.integers(1, 256, size=(n, 5), dtype=np.uint8)).to(dev)
        guids = torch.from_numpy(rng.integers(1, 256, size=(n, 16), dtype=np.uint8)).to(dev)
        # copy_only: the kept messages' application data, old place and new
        a_src = kept * rec + 12
        a_dst = torch.arange(k, dtype=torch.int64, device=dev) * rec + 12
        a_len = lens[:k].contiguous()
        per = 2 if with_confirms else 1
        keep = torch.zeros(n * per, dtype=torch.uint8, device=dev)
        keep[kept * per] = 1
        if with_confirms and not follow:
            keep[kept * per + 1] = 1
        mode = S.CONFIRMS_FOLLOW_MESSAGES if follow else S.CONFIRMS_AS_KEPT
        launches = 7 if follow else 6
        sets = []
        for c in range(copies):
            src = torch.empty(n * size, dtype=torch.uint8, device=dev)
            bmq.fill_synthetic(src, 41 + c)
            data, jour, _, _, _ = pack_records(src, soff, lens, qkeys, guids, stream=s, **KW)
            del src
            if with_confirms:
                jour = confirms_of(torch, jour, n)
            sets.append((jour, data, torch.zeros(new_bytes, dtype=torch.uint8, device=dev),
                         torch.zeros(60 * k * per, dtype=torch.uint8, device=dev),
                         torch.empty(k, dtype=torch.int32, device=dev)))
        torch.cuda.synchronize(dev)
        turn = {"copy_only": 0, "rollover": 0}
        last = None

        def step(leg):
            which = turn[leg] % copies
            jour, data, new, newj, out = sets[which]
            turn[leg] += 1
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            if leg == "rollover":
                rollover_records(jour, data, data_file_pos=DPOS, new_data_file_pos=DPOS, keep=keep,
                                 confirm_mode=mode, dst=new, journal_dst=newj, stream=s,
                                 sync=False)
            else:
                Crc32c.copy_batch(data, a_src, a_len, new, a_dst, None, out, stream=s, sync=False)
            e1.record(s)
            return e0, e1, which

        times = {"copy_only": [], "rollover": []}
        for i in range(a.warmup + a.steps):
            for leg in ("copy_only", "rollover"):
                e0, e1, which = step(leg)
                torch.cuda.synchronize(dev)
                if i >= a.warmup:
                    times[leg].append(e0.elapsed_time(e1) * 1e3)
                if leg == "rollover":
                    last = which
        # the last rollover against what torch builds from the same records
        jour, data, new, newj, _ = sets[last]
        state = bmq.last_rollover(0, s)
        good = state == dict(n_records=n * per, n_kept=k * per, n_messages=k,
                             journal_bytes=60 * k * per, data_bytes=new_bytes, n_bad=0,
                             first_bad=n * per, refused_kind=0, refused_index=0)
        good = good and torch.equal(new.view(k, rec), data.view(n, rec)[kept])
        want = jour.view(n, per * 60)[kept].clone()
        at = (DPOS + torch.arange(k, dtype=torch.int64, device=dev) * rec) >> 3
        for b in range(4):
            want[:, 32 + b] = ((at >> (8 * (3 - b))) & 0xFF).to(torch.uint8)
        good = good and torch.equal(newj, want.reshape(-1))
        del want
        res = {}
        for leg in ("copy_only", "rollover"):
            us = times[leg]
            med = statistics.median(us)
            res[leg] = (med, min(us), max(us))
            emit({"shape": name, "n_records": n * per, "size": size, "kept_messages": k,
                  "leg": leg, "copies": copies, "warmup": a.warmup, "steps": a.steps,
                  "us_median": round(med, 1), "us_min": round(min(us), 1),
                  "us_max": round(max(us), 1),
                  "payload_GiBps": round(total / 2**30 / (med * 1e-6), 1)})
        a_med, a_min, a_max = res["copy_only"]
        allowance = 5.0 * launches
        allowed = a_med + (a_max - a_min) + allowance
        within = res["rollover"][0] <= allowed
        barred = name == BARRED
        emit({"shape": name, "rollover_over_copy_only": round(res["rollover"][0] / a_med, 3),
              "rollover_minus_copy_only_us": round(res["rollover"][0] - a_med, 1),
              "copy_only_range_us": round(a_max - a_min, 1), "added_launches": launches,
              "launch_allowance_us": allowance, "allowed_us": round(allowed, 1),
              "rollover_within_bar": within, "bar_applies": barred,
              "rollover_matches_torch": bool(good)})
        ok = ok and good and (within or not barred)
        del sets
        torch.cuda.empty_cache()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
