#!/usr/bin/env python3
"""Messages past their TTL expired on the device (expire_records, ABI 2.20): the
call's time for two shapes, same process (GPU box).

  tools/expire_ab.py [--shapes 64k_half,1M+1M_4096q_half] [--warmup 5] [--steps 20]
                     [--copies N] [--legs expire,confirm] [--out FILE]

Shapes:
  64k_half           65,536 MESSAGE records of refCount 1 in 64 queues whose
                     timestamps rise with the record: the older half of every
                     queue has expired
  1M+1M_4096q_half   1,048,576 MESSAGE records of refCount 2 in 4,096 queues,
                     each followed by one CONFIRM record (2,097,152 records):
                     again the older half of every queue has expired
`copies` rotating sets of buffers (default 4), so that a step does not find the
run of the step before in the 256 MiB cache.  No other call does this work, and
it moves no payload, so there is no leg to hold a bar against:

  expire   expire_records with `journal_dst` given and sync=False: the two
           memsets of the workspace, the six kernels, the wrapper's output
           tensors
  confirm  for context, confirm_records over the same runs in the same session:
           one confirm for every message in a random order, each of which
           writes a DELETION record (tools/confirm_ab.py's shapes)

timed with device events around the whole call, `steps` timed steps after
`warmup`.  After the last step of each leg the destination, the arrays and the
result are compared with the leg's model under tests/.  One JSON line per shape
and leg: median, min and max (us) and records of the run per microsecond at the
median.  --out appends the lines to a file as well."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# messages, queues, refCount, a CONFIRM record behind every MESSAGE record
SHAPES = {"64k_half": (64 << 10, 64, 1, False), "1M+1M_4096q_half": (1 << 20, 4096, 2, True)}
DEFAULT_SHAPES = "64k_half,1M+1M_4096q_half"
LEASE, T0 = 7, 0x6720EAB4


def be(torch, values, nbytes):
    """int64 `values` as `nbytes` big-endian bytes each, (n, nbytes) uint8."""
    return torch.stack([((values >> (8 * (nbytes - 1 - b))) & 0xFF).to(torch.uint8)
                        for b in range(nbytes)], 1)


def build_run(torch, n, ref_count, with_confirms, qkeys, guids):
    """n MESSAGE records of `ref_count`, message i with timestamp T0 + i, each
    followed by one CONFIRM record with `with_confirms`, sequence numbers from
    1 on."""
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
    r[:, 0, 0], r[:, 0, 1] = 1 << 4, ref_count       # MESSAGE, refCount in the flags
    r[:, 0, 32:36] = be(torch, torch.arange(n, dtype=torch.int64, device=dev) * 2 + 5, 4)
    r[:, 0, 36:52] = guids
    if with_confirms:
        r[:, 1, 0] = 2 << 4                          # CONFIRM, reason CONFIRMED
        r[:, 1, 32:48] = guids
    return r.reshape(-1)


def main():
    p = argparse.ArgumentParser(description=__doc__,
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--shapes", default=DEFAULT_SHAPES)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--copies", type=int, default=4)
    p.add_argument("--legs", default="expire,confirm")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import numpy as np
    import torch
    import blazingmq_amd as bmq
    from blazingmq_amd import confirm_records, expire_records
    import confirm_records_model as CM
    import expire_records_model as EM
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

    def same(got, want, fields):
        return all(np.array_equal(getattr(got, f).cpu().numpy().view(getattr(want, f).dtype),
                                  getattr(want, f)) for f in fields)

    ok = True
    for name in a.shapes.split(","):
        n, n_queues, ref_count, with_confirms = SHAPES[name]
        per = 2 if with_confirms else 1
        # the older half of every queue: message i is n - i seconds old
        now, ttl = T0 + n, n // 2
        sets = []
        for c in range(a.copies):
            table = rng.integers(1, 256, size=(n_queues, 5), dtype=np.uint8)
            table[:, 0] = np.arange(n_queues) & 0xFF        # (distinct keys)
            table[:, 1] = 1 + (np.arange(n_queues) >> 8)
            which = rng.integers(0, n_queues, n)
            qkeys = torch.from_numpy(table[which]).to(dev)
            guids = torch.from_numpy(rng.integers(1, 256, size=(n, 16), dtype=np.uint8)).to(dev)
            run = build_run(torch, n, ref_count, with_confirms, qkeys, guids)
            order = torch.from_numpy(rng.permutation(n)).to(dev)
            sets.append(dict(
                run=run, table=torch.from_numpy(table.reshape(-1)).to(dev),
                ttl=torch.full((n_queues,), ttl, dtype=torch.int64, device=dev),
                guids=guids[order].contiguous().view(-1), qkeys=qkeys[order].contiguous().view(-1),
                out=torch.zeros(60 * n, dtype=torch.uint8, device=dev)))
        first_seq = n * per + 1
        torch.cuda.synchronize(dev)
        last = sets[(a.warmup + a.steps - 1) % a.copies]
        for leg in a.legs.split(","):
            if leg == "expire":
                def call(i):
                    t = sets[i % a.copies]
                    return expire_records(t["run"], t["table"], t["ttl"], now=now, lease_id=LEASE,
                                          first_seq=first_seq, journal_dst=t["out"], stream=s,
                                          sync=False)
                times, got = timed(call)
                state = bmq.last_expire_records(0, s)
                want = EM.expire_records(last["run"].cpu().numpy(), last["table"].cpu().numpy(),
                                         last["ttl"].cpu().numpy(), now=now, lease_id=LEASE,
                                         first_seq=first_seq, journal_dst_bytes=60 * n)
                good = isinstance(want, EM.Expired) and state == want.result and \
                    state["n_expired"] == n // 2 and \
                    np.array_equal(last["out"].cpu().numpy()[:want.journal.size], want.journal) and \
                    same(got, want, ("expired", "new_index", "select_out", "queue_expired",
                                     "queue_front"))
                extra = {"n_queues": n_queues, "n_expired": state["n_expired"]}
            else:
                def call(i):
                    t = sets[i % a.copies]
                    return confirm_records(t["run"], t["guids"], t["qkeys"], lease_id=LEASE,
                                           first_seq=first_seq, timestamp=now, journal_dst=t["out"],
                                           stream=s, sync=False)
                times, got = timed(call)
                state = bmq.last_confirm_records(0, s)
                want = CM.confirm_records(last["run"].cpu().numpy(), last["guids"].cpu().numpy(),
                                          last["qkeys"].cpu().numpy(), lease_id=LEASE,
                                          first_seq=first_seq, timestamp=now,
                                          journal_dst_bytes=60 * n)
                good = isinstance(want, CM.Confirmed) and state == want.result and \
                    state["n_deletions"] == n and \
                    np.array_equal(last["out"].cpu().numpy(), want.journal) and \
                    same(got, want, ("status", "target", "new_index", "left_out"))
                extra = {"n_confirms": n}
            med = statistics.median(times)
            emit(dict({"shape": name, "n_records": n * per, "leg": leg, "copies": a.copies,
                       "warmup": a.warmup, "steps": a.steps, "us_median": round(med, 1),
                       "us_min": round(min(times), 1), "us_max": round(max(times), 1),
                       "records_per_us": round(n * per / med, 1),
                       "matches_model": bool(good)}, **extra))
            ok = ok and good
        sets = last = None
        torch.cuda.empty_cache()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
