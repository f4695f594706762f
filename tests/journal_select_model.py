"""Order-free model of the recovery selection: which
MESSAGE records FileStore::recoverMessages CRCs, the result code and the
offending record, computed from a run of journal records with reductions only.

The reference (``walk_recovery``, restated by ``storage.recovery_selection_py``)
walks the journal backwards twice with hash sets that grow and shrink and
returns at the first failure.  Here nothing is carried from record to record:
every table is a maximum or a minimum over records visited in ANY order
(``order`` is the permutation used; the tests pass shuffled ones), a DELETION's
claim is the maximum over the messages that name it, and the failure is the
failing record with the highest index.  This is what the kernels of
crc32c_journal_select.hip compute; test_journal_select_model.py holds it to
the reference, test_gpu_journal_select.py holds the kernels to both.

One stated difference: no DATA byte is read, so INVALID_DATA_RECORD (-17) is
never raised and the INVALID_QUEUE_KEY check of a MESSAGE record is made as if
the DATA checks had passed."""
import numpy as np

from blazingmq_amd import storage as S

REC = S.JOURNAL_RECORD_SIZE
NONE = -1  # "no such record": below every index


def record_run(journal):
    """(the journal file's record run up to its last valid record, the file
    offset of record 0): what the caller of the device call uploads."""
    j = S._as_u8(journal)
    fh = S.parse_file_header(j, S.FILE_TYPE_JOURNAL)
    start = fh + int(j[fh]) * S.WORD
    _, last = S.journal_bounds(j)
    if last == 0:
        return j[:0].copy(), start
    return j[start:last + REC].copy(), start


def host_view(journal, data, **kw):
    """The native walk's answer in record indices: (sorted selected indices,
    recovery_rc, offending index or the record count)."""
    run, start = record_run(journal)
    nat = S.scan_partition(journal, data, **kw)
    sel = sorted((int(o) - start) // REC for o in nat["record_offset"])
    err = (nat["error_record_offset"] - start) // REC if nat["recovery_rc"] else len(run) // REC
    return sel, nat["recovery_rc"], err


def _int(b, off, n):
    return int.from_bytes(b[off:off + n], "big")


def select_model(run, data_file_bytes, with_csl=False, queue_keys=(), order=None):
    run = bytes(S._as_u8(run))
    n = len(run) // REC
    rec = [run[REC * r:REC * (r + 1)] for r in range(n)]
    order = list(range(n)) if order is None else [int(r) for r in order]
    assert sorted(order) == list(range(n))
    typ = [b[0] >> 4 for b in rec]
    seq = [(_int(b, 2, 2) << 32) | _int(b, 4, 4) for b in rec]
    lease = [_int(b, 8, 4) for b in rec]
    out = {"select": np.zeros(n, np.uint8), "recovery_rc": 0, "error_record": n,
           "first_record": n, "n_selected": 0, "n_deleted": 0, "n_purged": 0,
           "first_pass": False, "stop": NONE}
    if n == 0:
        return out
    T = n - 1

    # 1. the walked run
    stop = max((r for r in order if typ[r] == 0 or lease[r] == 0 or seq[r] == 0 or
                _int(rec[r], 56, 4) != S.RECORD_MAGIC), default=NONE)
    out["stop"] = stop
    W = [r for r in order if r > stop]
    first_sync = min((r for r in W if typ[r] == S.REC_JOURNAL_OP), default=0)

    # 2. first pass: reductions over the QueueOp records
    known = set(bytes(k) for k in queue_keys) if with_csl else set()
    qops = [(r, bytes(rec[r][22:27]), bytes(rec[r][27:32]), _int(rec[r], 32, 4))
            for r in W if typ[r] == S.REC_QUEUE_OP]
    qdel, topcreate, purge = {}, {}, {}
    for r, k, a, op in qops:
        if op == S.OP_DELETION and a == S.NULL_KEY and k != S.NULL_KEY:
            qdel[k] = max(qdel.get(k, NONE), r)
    for r, k, a, op in qops:
        if op == S.OP_CREATION and k != S.NULL_KEY and r > qdel.get(k, NONE):
            topcreate[k] = max(topcreate.get(k, NONE), r)
    live = known if with_csl else set(topcreate)
    fail1 = []
    for r, k, a, op in qops:
        code = 0
        if op == 0:
            code = S.RC_INVALID_QUEUE_OP_RECORD
        elif k == S.NULL_KEY:
            code = S.RC_NULL_QUEUE_KEY
        elif op == S.OP_DELETION:
            if with_csl and a == S.NULL_KEY and k in known:
                code = S.RC_INVALID_DELETION_RECORD
        elif op in (S.OP_CREATION, S.OP_ADDITION) and r > qdel.get(k, NONE):
            if with_csl:
                if k not in known:
                    code = S.RC_INVALID_QUEUE_KEY
            elif r < topcreate.get(k, NONE):
                code = S.RC_DUPLICATE_QUEUE_KEY
        if code:
            fail1.append((r, code))
    if fail1:
        out["error_record"], out["recovery_rc"] = max(fail1)
        out["first_pass"] = True
        return out
    for r, k, a, op in qops:
        if op == S.OP_PURGE and a == S.NULL_KEY and k in live and r > qdel.get(k, NONE):
            purge[k] = max(purge.get(k, NONE), r)

    def eligible(k, r):
        return r >= qdel.get(k, NONE) and r >= purge.get(k, NONE)

    # 3. second pass: every record on its own
    fail2, deletions, messages, n_purged = [], {}, [], []
    for r in W:
        b, L, s = rec[r], lease[r], seq[r]
        L2, s2 = (lease[r + 1], seq[r + 1]) if r < T else (L, s + 1)
        code = 0
        if L > L2:
            code = S.RC_INVALID_PRIMARY_LEASE_ID
        elif L == L2 and (s != s2 - 1 if r >= first_sync else s > s2 - 1):
            code = S.RC_INVALID_SEQ_NUMBER
        elif typ[r] == S.REC_JOURNAL_OP:
            sp_seq, sp_lease = (_int(b, 28, 4) << 32) | _int(b, 32, 4), _int(b, 40, 4)
            doff = _int(b, 44, 4) * S.DWORD
            if b[23] == 0:
                code = S.RC_INVALID_SYNC_PT_SUB_TYPE
            elif doff == 0 or doff > data_file_bytes:
                code = S.RC_INVALID_DATA_OFFSET
            elif sp_lease == 0:
                code = S.RC_INVALID_PRIMARY_LEASE_ID
            elif sp_seq == 0:
                code = S.RC_INVALID_SEQ_NUMBER
            elif sp_lease > L:
                code = S.RC_INVALID_PRIMARY_LEASE_ID
            elif sp_lease == L and sp_seq != s:
                code = S.RC_INVALID_SEQ_NUMBER
        elif typ[r] == S.REC_QUEUE_OP:
            k, op = bytes(b[22:27]), _int(b, 32, 4)
            if r >= qdel.get(k, NONE) and op == S.OP_ADDITION and not with_csl and k not in live:
                code = S.RC_INVALID_QUEUE_KEY
        elif typ[r] == S.REC_DELETION:
            k, g = bytes(b[23:28]), bytes(b[28:44])
            if g == bytes(16) or k == S.NULL_KEY:
                code = S.RC_INVALID_DELETION_RECORD
            elif eligible(k, r):
                deletions.setdefault(g, set()).add(r)
        elif typ[r] == S.REC_CONFIRM:
            if bytes(b[32:48]) == bytes(16) or bytes(b[22:27]) == S.NULL_KEY:
                code = S.RC_INVALID_CONFIRM_RECORD
        elif typ[r] == S.REC_MESSAGE:
            k, g = bytes(b[22:27]), bytes(b[36:52])
            o = _int(b, 32, 4) * S.DWORD
            if g == bytes(16) or k == S.NULL_KEY:
                code = S.RC_INVALID_MESSAGE_RECORD
            elif o == 0 or o > data_file_bytes:
                code = S.RC_INVALID_DATA_OFFSET
            elif eligible(k, r):
                messages.append((r, k, g))
            else:
                n_purged.append(r)
        if code:
            fail2.append((r, code))

    # GUID matching: every message names the lowest DELETION of its GUID above
    # it; a DELETION's claim is the highest message that names it
    names, claim = {}, {}
    for m, k, g in messages:
        above = [d for d in deletions.get(g, ()) if d > m]
        if above:
            names[m] = min(above)
            claim[names[m]] = max(claim.get(names[m], NONE), m)
    skipped, chosen = [], []
    for m, k, g in messages:
        if m in names and claim[names[m]] == m:
            skipped.append(m)
        elif k not in live:
            fail2.append((m, S.RC_INVALID_QUEUE_KEY))
        else:
            chosen.append(m)

    # 4. the result
    E = NONE
    if fail2:
        E, out["recovery_rc"] = max(fail2)
        out["error_record"] = E
    first = max(stop, E) + 1
    out["first_record"] = first
    for m in chosen:
        if m >= first:
            out["select"][m] = 1
    out["n_selected"] = int(out["select"].sum())
    out["n_deleted"] = sum(1 for m in skipped if m >= first)
    out["n_purged"] = sum(1 for m in n_purged if m >= first)
    return out
