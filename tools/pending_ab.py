#!/usr/bin/env python3
"""Each app's pending messages listed on the device (pending_records, ABI 2.21):
the call's time for two shapes, same process (GPU box).

  tools/pending_ab.py [--shapes 64k_64q_1app,1M+1M_4096q_2apps] [--warmup 5] [--steps 20]
                      [--copies N] [--legs pending,expire] [--out FILE]

Shapes:
  64k_64q_1app        65,536 MESSAGE records in 64 queues of one app with the
                      null key: 64 apps, one digit pass, 65,536 pairs
  1M+1M_4096q_2apps   1,048,576 MESSAGE records in 4,096 queues of two apps, each
                      followed by one CONFIRM record (2,097,152 records) that
                      carries the first app's key behind every second message
                      and the null key behind the others: 8,192 apps, two digit
                      passes, 1,572,864 pairs
`copies` rotating sets of buffers (default 4), so that a step does not find the
run of the step before in the 256 MiB cache.  No other call does this work, and
it moves no payload, so there is no leg to hold a bar against:

  pending  pending_records with `list_cap` given and sync=False: the memset of
           the workspace, the four mask kernels, the host's read of the pair
           count, the emit, the sort's passes, the bounds, check and frame
           kernels, the wrapper's output tensors
  expire   for context, expire_records over the same runs in the same session
           with the older half of every queue expired (tools/expire_ab.py's leg)

timed with device events around the whole call, `steps` timed steps after
`warmup`.  After the last step of the pending leg the lists, the arrays and the
result are compared with the model under tests/.  One JSON line per shape and
leg: median, min and max (us) and records of the run per microsecond at the
median.  --out appends the lines to a file as well."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# messages, queues, apps a queue, a CONFIRM record behind every MESSAGE record
SHAPES = {"64k_64q_1app": (64 << 10, 64, 1, False), "1M+1M_4096q_2apps": (1 << 20, 4096, 2, True)}
DEFAULT_SHAPES = "64k_64q_1app,1M+1M_4096q_2apps"
LEASE, T0 = 7, 0x6720EAB4


def be(torch, values, nbytes):
    """int64 `values` as `nbytes` big-endian bytes each, (n, nbytes) uint8."""
    return torch.stack([((values >> (8 * (nbytes - 1 - b))) & 0xFF).to(torch.uint8)
                        for b in range(nbytes)], 1)


def build_run(torch, n, with_confirms, qkeys, guids, confirm_keys):
    """n MESSAGE records, message i with timestamp T0 + i, each followed by one
    CONFIRM record with the app key confirm_keys[i] with `with_confirms`,
    sequence numbers from 1 on."""
    dev = guids.device
    per = 2 if with_confirms else 1
    r = torch.zeros((n, per, 60), dtype=torch.uint8, device=dev)
    seq = torch.arange(n * per, dtype=torch.int64, device=dev).view(n, per) + 1
    for k in range(per):
        r[:, k, 2:8] = be(torch, seq[:, k], 6)
    r[:, :, 8:12] = torch.tensor(list(LEASE.to_bytes(4, "big")), dtype=torch.uint8, device=dev)
    r[:, :, 12:20] = be(torch, torch.arange(n, dtype=torch.int64, device=dev) + T0, 8)[:, None, :]
    r[:, :, 56:60] = torch.tensor([0x2A, 0x72, 0x45, 0x63], dtype=torch.uint8, device=dev)
    r[:, :, 22:27] = qkeys[:, None, :]
    r[:, 0, 0], r[:, 0, 1] = 1 << 4, per             # MESSAGE, refCount in the flags
    r[:, 0, 32:36] = be(torch, torch.arange(n, dtype=torch.int64, device=dev) * 2 + 5, 4)
    r[:, 0, 36:52] = guids
    if with_confirms:
        r[:, 1, 0] = 2 << 4                          # CONFIRM, reason CONFIRMED
        r[:, 1, 27:32] = confirm_keys
        r[:, 1, 32:48] = guids
    return r.reshape(-1)


def main():
    p = argparse.ArgumentParser(description=__doc__,
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--shapes", default=DEFAULT_SHAPES)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--copies", type=int, default=4)
    p.add_argument("--legs", default="pending,expire")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import numpy as np
    import torch
    import blazingmq_amd as bmq
    from blazingmq_amd import expire_records, pending_records
    import pending_list_model as PM
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

    def timed(call):
        """`call(i)` for warmup + steps steps: (the timed steps' us, the last answer)."""
        times, got = [], None
        for i in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            got = call(i)
            e1.record(s)
            torch.cuda.synchronize(dev)
            if i >= a.warmup:
                times.append(e0.elapsed_time(e1) * 1e3)
        return times, got

    ok = True
    for name in a.shapes.split(","):
        n, n_queues, per_queue, with_confirms = SHAPES[name]
        per = 2 if with_confirms else 1
        n_apps = n_queues * per_queue
        n_pairs = n * per_queue - (n // 2 if with_confirms else 0)
        now, ttl = T0 + n, n // 2
        sets = []
        for c in range(a.copies):
            table = rng.integers(1, 256, size=(n_queues, 5), dtype=np.uint8)
            table[:, 0] = np.arange(n_queues) & 0xFF        # (distinct keys)
            table[:, 1] = 1 + (np.arange(n_queues) >> 8)
            app_keys = rng.integers(1, 256, size=(n_apps, 5), dtype=np.uint8)
            app_keys[:, 0] = 1 + np.arange(n_apps) % per_queue     # (distinct inside a queue)
            if per_queue == 1:
                app_keys[:] = 0                                    # the null key
            which = rng.integers(0, n_queues, n)
            confirm_keys = app_keys[which * per_queue].copy()
            confirm_keys[1::2] = 0
            qkeys = torch.from_numpy(table[which]).to(dev)
            guids = torch.from_numpy(rng.integers(1, 256, size=(n, 16), dtype=np.uint8)).to(dev)
            run = build_run(torch, n, with_confirms, qkeys, guids,
                            torch.from_numpy(confirm_keys).to(dev))
            sets.append(dict(
                run=run, table=torch.from_numpy(table.reshape(-1)).to(dev),
                app_first=torch.arange(0, n_apps + 1, per_queue, dtype=torch.int64, device=dev),
                app_keys=torch.from_numpy(app_keys.reshape(-1)).to(dev),
                queue_ids=torch.arange(n_apps, dtype=torch.int32, device=dev),
                sub_ids=torch.arange(n_apps, dtype=torch.int32, device=dev) + 500,
                ttl=torch.full((n_queues,), ttl, dtype=torch.int64, device=dev),
                out=torch.zeros(60 * n, dtype=torch.uint8, device=dev)))
        torch.cuda.synchronize(dev)
        last = sets[(a.warmup + a.steps - 1) % a.copies]
        for leg in a.legs.split(","):
            if leg == "pending":
                def call(i):
                    t = sets[i % a.copies]
                    return pending_records(t["run"], t["table"], t["app_first"], t["app_keys"],
                                           t["queue_ids"], sub_ids=t["sub_ids"], list_cap=n_pairs,
                                           stream=s, sync=False)
                times, got = timed(call)
                state = bmq.last_pending_records(0, s)
                want = PM.pending_records(*(last[k].cpu().numpy() for k in (
                    "run", "table", "app_first", "app_keys", "queue_ids")),
                    sub_ids=last["sub_ids"].cpu().numpy(), list_cap=n_pairs)
                good = isinstance(want, PM.Pending) and state == want.result and \
                    state["n_pending"] == state["n_listed"] == n_pairs and all(
                        np.array_equal(getattr(got, f).cpu().numpy().view(getattr(want, f).dtype),
                                       getattr(want, f)) for f in got._fields[:7])
                extra = {"n_queues": n_queues, "n_apps": n_apps, "n_pairs": state["n_pending"],
                         "matches_model": bool(good)}
                ok = ok and good
            else:
                def call(i):
                    t = sets[i % a.copies]
                    return expire_records(t["run"], t["table"], t["ttl"], now=now, lease_id=LEASE,
                                          first_seq=n * per + 1, journal_dst=t["out"], stream=s,
                                          sync=False)
                times, got = timed(call)
                extra = {"n_queues": n_queues,
                         "n_expired": bmq.last_expire_records(0, s)["n_expired"]}
            med = statistics.median(times)
            emit(dict({"shape": name, "n_records": n * per, "leg": leg, "copies": a.copies,
                       "warmup": a.warmup, "steps": a.steps, "us_median": round(med, 1),
                       "us_min": round(min(times), 1), "us_max": round(max(times), 1),
                       "records_per_us": round(n * per / med, 1)}, **extra))
        sets = last = None
        torch.cuda.empty_cache()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
