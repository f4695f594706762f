#!/usr/bin/env python3
"""Consumer confirms recorded on the device (confirm_records, ABI 2.19): the
call's time for two shapes, same process (GPU box).

  tools/confirm_ab.py [--shapes 64kx64k,1Mx2M_deleting] [--warmup 5] [--steps 20]
                      [--copies N] [--out FILE]

Shapes:
  64kx64k          65,536 confirms, one for each of 65,536 MESSAGE records of
                   refCount 1, in a random order: every confirm writes a
                   DELETION record
  1Mx2M_deleting   1,048,576 confirms against a run of 1,048,576 MESSAGE records
                   of refCount 2, each followed by one CONFIRM record (2,097,152
                   records): every confirm is the last one and writes a DELETION
                   record
`copies` rotating sets of buffers (default 4), so that a step does not find the
run of the step before in the 256 MiB cache.  There is one leg: no other call
does this work, and it moves no payload, so the fused copy is no yardstick.

  confirm  confirm_records with `journal_dst` given and sync=False: the memset
           of the workspace, the five kernels, the wrapper's output tensors

timed with device events around the whole call, `steps` timed steps after
`warmup`.  After the last step the destination, the four arrays and the result
are compared with tests/confirm_records_model.py.  One JSON line per shape:
median, min and max (us) and records of the run per microsecond at the median.
--out appends the lines to a file as well."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {"64kx64k": (64 << 10, 1, False), "1Mx2M_deleting": (1 << 20, 2, True)}
DEFAULT_SHAPES = "64kx64k,1Mx2M_deleting"
LEASE, TIMESTAMP = 7, 0x6720EAB4


def be(torch, values, nbytes):
    """int64 `values` as `nbytes` big-endian bytes each, (n, nbytes) uint8."""
    return torch.stack([((values >> (8 * (nbytes - 1 - b))) & 0xFF).to(torch.uint8)
                        for b in range(nbytes)], 1)


def build_run(torch, n, ref_count, with_confirms, qkeys, guids):
    """n MESSAGE records of `ref_count`, each followed by one CONFIRM record
    with `with_confirms`, sequence numbers from 1 on."""
    dev = guids.device
    per = 2 if with_confirms else 1
    r = torch.zeros((n, per, 60), dtype=torch.uint8, device=dev)
    seq = torch.arange(n * per, dtype=torch.int64, device=dev).view(n, per) + 1
    for k in range(per):
        r[:, k, 2:8] = be(torch, seq[:, k], 6)
    r[:, :, 8:12] = torch.tensor(list(LEASE.to_bytes(4, "big")), dtype=torch.uint8, device=dev)
    r[:, :, 12:20] = torch.tensor(list(TIMESTAMP.to_bytes(8, "big")), dtype=torch.uint8, device=dev)
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
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import numpy as np
    import torch
    import blazingmq_amd as bmq
    from blazingmq_amd import confirm_records
    import confirm_records_model as M
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
        n, ref_count, with_confirms = SHAPES[name]
        per = 2 if with_confirms else 1
        sets = []
        for c in range(a.copies):
            qkeys = torch.from_numpy(rng.integers(1, 256, size=(n, 5), dtype=np.uint8)).to(dev)
            guids = torch.from_numpy(rng.integers(1, 256, size=(n, 16), dtype=np.uint8)).to(dev)
            run = build_run(torch, n, ref_count, with_confirms, qkeys, guids)
            order = torch.from_numpy(rng.permutation(n)).to(dev)
            sets.append((run, guids[order].contiguous().view(-1), qkeys[order].contiguous().view(-1),
                         torch.zeros(60 * n, dtype=torch.uint8, device=dev)))
        first_seq = n * per + 1
        torch.cuda.synchronize(dev)
        times, got = [], None
        for i in range(a.warmup + a.steps):
            run, g, q, out = sets[i % a.copies]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            got = confirm_records(run, g, q, lease_id=LEASE, first_seq=first_seq,
                                  timestamp=TIMESTAMP + 1, journal_dst=out, stream=s, sync=False)
            e1.record(s)
            torch.cuda.synchronize(dev)
            if i >= a.warmup:
                times.append(e0.elapsed_time(e1) * 1e3)
        # the last call against the model
        run, g, q, out = sets[(a.warmup + a.steps - 1) % a.copies]
        state = bmq.last_confirm_records(0, s)
        want = M.confirm_records(run.cpu().numpy(), g.cpu().numpy(), q.cpu().numpy(),
                                 lease_id=LEASE, first_seq=first_seq, timestamp=TIMESTAMP + 1,
                                 journal_dst_bytes=60 * n)
        good = isinstance(want, M.Confirmed) and state == want.result and \
            state["n_deletions"] == n
        good = good and np.array_equal(out.cpu().numpy(), want.journal)
        for field in ("status", "target", "new_index", "left_out"):
            have = getattr(got, field).cpu().numpy()
            good = good and np.array_equal(have.view(getattr(want, field).dtype),
                                           getattr(want, field))
        med = statistics.median(times)
        emit({"shape": name, "n_records": n * per, "n_confirms": n, "leg": "confirm",
              "copies": a.copies, "warmup": a.warmup, "steps": a.steps,
              "us_median": round(med, 1), "us_min": round(min(times), 1),
              "us_max": round(max(times), 1), "records_per_us": round(n * per / med, 1),
              "confirm_matches_model": bool(good)})
        ok = ok and good
        del sets
        torch.cuda.empty_cache()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
