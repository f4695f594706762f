#!/usr/bin/env python3
"""Recovery's selection made on the device (select_records, ABI 2.14) in front
of unpack_records, against the same unpack with the selection computed
beforehand, same process, alternated step by step (GPU box).

  tools/journal_select_ab.py [--shapes 64kx64K,1Mx256d,4Mx64d] [--warmup 5] [--steps 20]
                             [--copies N] [--no-host-scan]

A shape is `messages x size`: uniform messages of one queue packed into DATA
records and journal MessageRecords on the device by pack_records
(data_file_pos 40); a trailing `d` appends a DELETION record for every second
message, so half of them are consumed.  The queue is live by the cluster state
(with_csl, one key, on the device).  `copies` rotating sets of partitions
(default: 4 for the small-message shapes, 1 for 64k x 64 KiB), so the small
shapes read from HBM and not from the 256 MiB cache.  Three legs alternate:

  unpack         (a) unpack_records(select=<computed beforehand>, msg_cap=
                 n_selected, verify=True)
  select_unpack  (b) select_records, then the same unpack over its select
  select         select_records alone: one memset and six kernels

each timed with device events around the whole leg, `steps` timed steps after
`warmup`.  After the last step the select of leg (b) is compared with the one
computed beforehand, both with what was built (every second message), and the
unpack's result with n_selected messages, none bad.  One JSON line per leg:
median, min and max (us).  A last line per shape gives b - a, leg (a)'s own
min-max range, the launches the call adds, the bar (range + 5 us per launch)
and, as context, the wall time of ONE native host walk (bmqcrc_journal_scan)
over the same journal on this box: what the call replaces, no download
counted.  The host walk is handed a DATA file image that holds the DataHeaders
and padding bytes it reads and zeros for the payloads it never reads."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = {"64kx64K": (64 << 10, 64 << 10, False), "1Mx256d": (1 << 20, 256, True),
         "4Mx64d": (4 << 20, 64, True), "4kx256d": (4 << 10, 256, True)}
DEFAULT = "64kx64K,1Mx256d,4Mx64d"
KEY = b"\x11\x22\x33\x44\x55"
LAUNCHES = 7   # one memset of the workspace and six kernels
LEGS = ("unpack", "select_unpack", "select")


def deletions(np, S, n, guids, every=2):
    """DELETION records of messages 0, every, ... of a pack with first_seq 2."""
    idx = np.arange(0, n, every)
    seq = (2 + n + np.arange(idx.size)).astype(">u8")
    d = np.zeros((idx.size, 60), np.uint8)
    d[:, 0] = S.REC_DELETION << 4
    d[:, 2:8] = seq.view(np.uint8).reshape(-1, 8)[:, 2:]
    d[:, 8:12] = (0, 0, 0, 1)                      # lease id 1
    d[:, 23:28] = np.frombuffer(KEY, np.uint8)
    d[:, 28:44] = guids[idx]
    d[:, 56:60] = np.frombuffer(S.RECORD_MAGIC.to_bytes(4, "big"), np.uint8)
    return d.reshape(-1)


def host_scan_ms(np, S, N, run, n, size, record, packed):
    """Wall time of one native host walk over the journal file of `run`."""
    head = np.concatenate([S.file_header(S.FILE_TYPE_JOURNAL),
                           np.array([3, 15] + [0] * 10, np.uint8)])
    jf = np.concatenate([head, run])
    df = np.zeros(40 + packed, np.uint8)           # untouched pages stay unmapped
    df[:32] = S.file_header(S.FILE_TYPE_DATA)
    df[32] = 2
    at = 40 + np.arange(n, dtype=np.int64) * record
    word = np.frombuffer(((3 << 29) | (record // 4)).to_bytes(4, "big"), np.uint8)
    for k in range(4):
        df[at + k] = word[k]
    df[at + record - 1] = record - 12 - size       # the padding count, 1..8
    cfg, keys = S._cfg(True, [KEY])
    rrc, err = ctypes.c_int(0), ctypes.c_uint64(0)
    t0 = time.perf_counter()
    got = N.lib.bmqcrc_journal_scan(jf.ctypes.data, jf.size, df.ctypes.data, df.size,
                                    ctypes.byref(cfg), ctypes.byref(rrc), ctypes.byref(err),
                                    None, None, None, None, 0)
    ms = (time.perf_counter() - t0) * 1e3
    return ms, int(got), int(rrc.value)


def main():
    p = argparse.ArgumentParser(description=__doc__,
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--shapes", default=DEFAULT)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--copies", type=int, default=0)
    p.add_argument("--no-host-scan", action="store_true")
    a = p.parse_args()
    import numpy as np
    import torch
    import blazingmq_amd as bmq
    from blazingmq_amd import _native as N, pack_records, select_records, unpack_records
    from blazingmq_amd import storage as S
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev)
    rng = np.random.default_rng(7)
    pos = 40
    ok = True
    keys = torch.from_numpy(np.frombuffer(KEY, np.uint8).copy()).to(dev)
    for shape in a.shapes.split(","):
        n, size, deleted = SIZES[shape]
        total = n * size
        record = ((size + 12) // 8 + 1) * 8
        packed = record * n
        copies = a.copies or (1 if total >= 1 << 30 else 4)
        soff = torch.arange(n, dtype=torch.int64, device=dev) * size
        lens = torch.full((n,), size, dtype=torch.int32, device=dev)
        guids_h = rng.integers(1, 256, size=(n, 16), dtype=np.uint8)
        guids = torch.from_numpy(guids_h).to(dev)
        qkeys = keys.repeat(n, 1)
        tail_h = deletions(np, S, n, guids_h) if deleted else np.zeros(0, np.uint8)
        tail = torch.from_numpy(tail_h).to(dev)
        n_records = n + tail_h.size // 60
        want = torch.ones(n_records, dtype=torch.uint8, device=dev)
        want[n:] = 0
        if deleted:
            want[0:n:2] = 0
        n_sel = int(want.sum().item())
        src = torch.empty(total, dtype=torch.uint8, device=dev)
        sets = []
        for c in range(copies):
            bmq.fill_synthetic(src, 47 + c)
            jour = torch.empty(60 * n_records, dtype=torch.uint8, device=dev)
            jour[60 * n:] = tail
            dst, _, _, _, _ = pack_records(
                src, soff, lens, qkeys, guids, file_key=KEY, lease_id=1, first_seq=2,
                data_file_pos=pos, dst=torch.zeros(packed, dtype=torch.uint8, device=dev),
                journal_dst=jour)
            before, res = select_records(jour, data_file_bytes=pos + packed, with_csl=True,
                                         queue_keys=keys)
            ok = ok and torch.equal(before, want) and res["recovery_rc"] == 0
            sets.append((jour, dst, before))
        del src
        torch.cuda.synchronize(dev)
        turn = dict.fromkeys(LEGS, 0)

        def step(leg):
            jour, dst, before = sets[turn[leg] % copies]
            turn[leg] += 1
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            select = before
            e0.record(s)
            if leg != "unpack":
                select = select_records(jour, data_file_bytes=pos + packed, with_csl=True,
                                        queue_keys=keys, stream=s, sync=False)
            if leg != "select":
                unpack_records(jour, dst, data_file_pos=pos, select=select, msg_cap=n_sel,
                               verify=True, stream=s, sync=False)
            e1.record(s)
            return e0, e1, select

        times = {leg: [] for leg in LEGS}
        last = {}
        for i in range(a.warmup + a.steps):
            for leg in LEGS:
                e0, e1, last[leg] = step(leg)
                torch.cuda.synchronize(dev)
                if i >= a.warmup:
                    times[leg].append(e0.elapsed_time(e1) * 1e3)
        sel = bmq.last_journal_select(0, s)
        unp = bmq.last_records_unpack(0, s)
        good = torch.equal(last["select_unpack"], want) and torch.equal(last["select"], want)
        good = good and sel == dict(n_records=n_records, first_record=0, n_selected=n_sel,
                                    n_deleted=n - n_sel, n_purged=0, error_record=n_records,
                                    recovery_rc=0, refused_kind=0)
        good = good and (unp["n_msgs"], unp["n_bad"], unp["refused_kind"]) == (n_sel, 0, 0)
        res = {}
        for leg in LEGS:
            us = times[leg]
            med = statistics.median(us)
            res[leg] = (med, min(us), max(us))
            print(json.dumps({
                "shape": shape, "n": n, "size": size, "records": n_records, "selected": n_sel,
                "leg": leg, "copies": copies, "warmup": a.warmup, "steps": a.steps,
                "us_median": round(med, 1), "us_min": round(min(us), 1),
                "us_max": round(max(us), 1)}), flush=True)
        a_med, a_range = res["unpack"][0], res["unpack"][2] - res["unpack"][1]
        line = {"shape": shape, "b_minus_a_us": round(res["select_unpack"][0] - a_med, 1),
                "a_range_us": round(a_range, 1), "launches_added": LAUNCHES,
                "bar_us": round(a_range + 5 * LAUNCHES, 1),
                "bar_applies": shape == "64kx64K",
                "within_bar": bool(res["select_unpack"][0] - a_med <= a_range + 5 * LAUNCHES),
                "select_matches": bool(good)}
        if not a.no_host_scan:
            run = sets[0][0].cpu().numpy()
            ms, got, rrc = host_scan_ms(np, S, N, run, n, size, record, packed)
            good = good and (got, rrc) == (n_sel, 0)
            line.update(host_scan_ms=round(ms, 2), host_scan_selected=got)
        print(json.dumps(line), flush=True)
        ok = ok and good
        del sets, last
        torch.cuda.empty_cache()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
