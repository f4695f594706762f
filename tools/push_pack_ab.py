#!/usr/bin/env python3
"""Stored messages packed into PUSH events on the device (pack_push_events,
ABI 2.17) against the payload-only lower bound, same process, alternated step
by step (GPU box).

  tools/push_pack_ab.py [--shapes 64kx64K_4096,1Mx256_4096,1Mx256_5] [--warmup 5]
                        [--steps 20] [--copies N] [--out FILE]

Per shape n x size_events: n MESSAGE records of `size` application bytes,
written by pack_records, delivered once each in record order (records=None),
spread evenly over the events.  `copies` rotating sets of buffers (default: as
many as 4 GiB of events hold, 4 at the most), so the small shapes read from HBM
and not from the 256 MiB cache.  Two legs alternate:

  copy_only  Crc32c.copy_batch over the same application data with source and
             destination offsets computed on the host beforehand: the payload
             pass alone, no record classified, no header written
  pack       pack_push_events with `dst` given, in option mode 1 (a packed RDA
             counter): the classification, the layout and its checks, the same
             payload pass, the frame (PushHeaders, options, padding,
             EventHeaders, the arrays); the wrapper's output tensors included

each timed with device events around the whole leg, `steps` timed steps after
`warmup`.  After the last step the events are compared with the ones the host
PushEventBuilder makes from the same records, event by event.  One JSON line
per leg: median, min and max (us), payload GiB/s at the median.  A last line
per shape gives the bar (asserted for 64kx64K_4096 only, reported for the
rest): pack median <= copy_only median + (copy_only max - min) + 25 us -- 5 us
for each of the 5 kernels the call launches around the copy (classify, count,
check, seal, frame; the memset of its counters is not counted).  --out appends
the lines to a file as well."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"64kx64K_4096": (64 << 10, 64 << 10, 4096), "1Mx256_4096": (1 << 20, 256, 4096),
          "1Mx256_5": (1 << 20, 256, 5)}
ADDED_LAUNCHES = 5
LAUNCH_ALLOWANCE_US = 5.0 * ADDED_LAUNCHES
DPOS = 40
KW = dict(file_key=b"\x0a\x0b\x0c\x0d\x0e", lease_id=7, first_seq=1000, data_file_pos=DPOS,
          timestamp=0x6720EAB4)
CHECK_BYTES = 256 << 20   # of events brought to the host at a time for the comparison


def matches_builder(torch, E, events, jour, data, rec, size, qids, rda, first):
    """The device's events against the host builder's, a run of events at a time."""
    n_events = len(first) - 1
    msg = 36 + size + 4 - size % 4
    e = 0
    while e < n_events:
        stop = e + 1
        while stop < n_events and 8 * (stop + 1 - e) + msg * (first[stop + 1] - first[e]) \
                <= CHECK_BYTES:
            stop += 1
        lo, hi = first[e], first[stop]
        at = 8 * e + msg * lo
        got = events[at:at + 8 * (stop - e) + msg * (hi - lo)].cpu().numpy()
        guids = jour[60 * lo:60 * hi].view(-1, 60)[:, 36:52].cpu().numpy()
        apps = data[rec * lo:rec * hi].view(-1, rec)[:, 12:12 + size].cpu().numpy()
        want = []
        for k in range(e, stop):
            b = E.PushEventBuilder(max_event_bytes=1 << 62)
            for m in range(first[k], first[k + 1]):
                b.add_sub_queue_infos_option([(E.DEFAULT_SUB_QUEUE_ID, int(rda[m]))], True)
                b.pack_message(apps[m - lo].tobytes(), int(qids[m]), guids[m - lo].tobytes())
            want.append(b.blob().tobytes())
        if got.tobytes() != b"".join(want):
            return False
        e = stop
    return True


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
    from blazingmq_amd import Crc32c, pack_push_events, pack_records
    from blazingmq_amd import push_event as E
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
        msg = 36 + size + 4 - size % 4
        nbytes = 8 * n_events + n * msg
        copies = a.copies or max(1, min(4, (4 << 30) // nbytes))
        soff = torch.arange(n, dtype=torch.int64, device=dev) * size
        lens = torch.full((n,), size, dtype=torch.int32, device=dev)
        roff = torch.arange(n, dtype=torch.int64, device=dev) * rec + 12
        qkeys = torch.from_numpy(rng.integers(1, 256, size=(n, 5), dtype=np.uint8)).to(dev)
        guids = torch.from_numpy(rng.integers(1, 256, size=(n, 16), dtype=np.uint8)).to(dev)
        qids = rng.integers(-2**31, 2**31, size=n).astype(np.int32)
        rda = rng.integers(0, 256, size=n).astype(np.uint8)
        d_qids, d_rda = torch.from_numpy(qids).to(dev), torch.from_numpy(rda).to(dev)
        first = [(n * e) // n_events for e in range(n_events + 1)]
        d_first = torch.tensor(first, dtype=torch.int64, device=dev)
        event_of = torch.repeat_interleave(
            torch.arange(n_events, dtype=torch.int64, device=dev),
            torch.tensor(np.diff(first), dtype=torch.int64, device=dev))
        # application data of message i in the events: behind the event headers up to its
        # own, the messages before it, its PushHeader and option
        app = 8 * (event_of + 1) + torch.arange(n, dtype=torch.int64, device=dev) * msg + 36
        del event_of
        sets = []
        for c in range(copies):
            src = torch.empty(total, dtype=torch.uint8, device=dev)
            bmq.fill_synthetic(src, 41 + c)
            dst, jour, _, _, _ = pack_records(src, soff, lens, qkeys, guids, stream=s, **KW)
            del src
            sets.append((jour, dst, torch.zeros(nbytes, dtype=torch.uint8, device=dev),
                         torch.empty(n, dtype=torch.int32, device=dev)))
        torch.cuda.synchronize(dev)
        turn = {"copy_only": 0, "pack": 0}
        last_pack = None

        def step(leg):
            which = turn[leg] % copies
            jour, dst, events, out = sets[which]
            turn[leg] += 1
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            if leg == "pack":
                pack_push_events(jour, dst, data_file_pos=DPOS, queue_ids=d_qids,
                                 option_mode=E.OPTION_PACKED_RDA, rda=d_rda, event_first=d_first,
                                 dst=events, stream=s, sync=False)
            else:
                Crc32c.copy_batch(dst, roff, lens, events, app, None, out, stream=s, sync=False)
            e1.record(s)
            return e0, e1, which

        times = {"copy_only": [], "pack": []}
        for i in range(a.warmup + a.steps):
            for leg in ("copy_only", "pack"):
                e0, e1, which = step(leg)
                torch.cuda.synchronize(dev)
                if i >= a.warmup:
                    times[leg].append(e0.elapsed_time(e1) * 1e3)
                if leg == "pack":
                    last_pack = which
        # the last pack against the events the host builder makes from the same records
        jour, dst, events, _ = sets[last_pack]
        state = bmq.last_push_pack(0, s)
        good = state == dict(n_events=n_events, n_msgs=n, total_bytes=nbytes, n_bad=0,
                             first_bad=n, refused_kind=0, refused_index=0)
        good = good and matches_builder(torch, E, events, jour, dst, rec, size, qids, rda, first)
        res = {}
        for leg in ("copy_only", "pack"):
            us = times[leg]
            med = statistics.median(us)
            res[leg] = (med, min(us), max(us))
            emit({"shape": name, "n": n, "size": size, "events": n_events, "leg": leg,
                  "copies": copies, "warmup": a.warmup, "steps": a.steps,
                  "us_median": round(med, 1), "us_min": round(min(us), 1),
                  "us_max": round(max(us), 1),
                  "payload_GiBps": round(total / 2**30 / (med * 1e-6), 1)})
        a_med, a_min, a_max = res["copy_only"]
        allowed = a_med + (a_max - a_min) + LAUNCH_ALLOWANCE_US
        within = res["pack"][0] <= allowed
        barred = name == "64kx64K_4096"
        emit({"shape": name, "pack_over_copy_only": round(res["pack"][0] / a_med, 3),
              "pack_minus_copy_only_us": round(res["pack"][0] - a_med, 1),
              "copy_only_range_us": round(a_max - a_min, 1),
              "launch_allowance_us": LAUNCH_ALLOWANCE_US, "allowed_us": round(allowed, 1),
              "pack_within_bar": within, "bar_applies": barred,
              "pack_matches_builder": bool(good)})
        ok = ok and good and (within or not barred)
        del sets
        torch.cuda.empty_cache()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
