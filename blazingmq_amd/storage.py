"""Batched recovery-time CRC32C verification over BlazingMQ partition files.

Host-side mirror of the CRC part of ``mqbs::FileStore::recoverMessages``
(/root/reference/src/groups/mqb/mqbs/mqbs_filestore.cpp:1045, two backward
passes :1120-1453 and :1490-2646, DATA checks :2494-2575, CRC check
:2603-2624).  The reference CRCs the outstanding messages one at a time as it
walks; here the same records are selected first (deleted GUIDs, purged
queues and records before their queue's DELETION are skipped, their DATA
never read), then all payloads are verified with ONE batched GPU call.

The product path is native: ``scan_partition`` / ``verify_partition`` call
``bmqcrc_journal_scan`` / ``bmqcrc_recover_verify`` (include/bmqcrc_protocol.h,
csrc/bmqcrc_protocol.cpp).  ``recovery_selection_py`` restates the selection
in Python; the CPU tests hold the two against each other, against
bmqstoragetool's fixture and its outstanding-message outputs, and against
partitions built by ``PartitionWriter`` with every record type.

On-disk layouts (mqbs_filestoreprotocol.h):
  FileHeader (:306)        magic1 "!bmq", magic2 "BMQ!", PV(2b)|HW(6b), B(1b)|FileType(7b),
                           ..., partitionId (BE, byte 20)
  JournalFileHeader (:483) headerWords, recordWords (15 = 60-byte records), ...
  DataFileHeader (:426)    headerWords, reserved, fileKey[5], reserved
  RecordHeader (:1014)     BE u16 type(4b)|flags(12b), seqNum hi/lo, leaseId, timestamp
  MessageRecord (:1125)    header(20) refCountHi(1) CAT(1) queueKey(5) fileKey(5)
                           messageOffsetDwords(BE u32 @32) GUID(16 @36) CRC32C(BE @52)
                           magic 0x2A724563 "*rEc" (@56)
  ConfirmRecord (:1339)    queueKey @22, appKey @27, GUID @32
  DeletionRecord (:1518)   queueKey @23, GUID @28
  QueueOpRecord (:1694)    queueKey @22, appKey @27, BE i32 QueueOpType @32, uri offset @36
  JournalOpRecord (:1953)  syncPointType @23, BE i32 JournalOpType @24, seq @28/@32,
                           leaseId @40, dataFileOffsetDwords @44, qlistFileOffsetWords @48
  DataHeader (:703)        BE u32 HW(3b)|messageWords(29b), BE u32 optionsWords(24b)|flags(8b)
  A DATA record is DataHeader + options + application data + 1..8 padding
  bytes, each equal to the padding count (bmqp_protocolutil.cpp:44, dword
  padding); MessageOffsetDwords counts 8-byte units.
"""
import collections
import ctypes

import numpy as np

from . import _native as N
from .crc32c import Crc32c

MAGIC1 = 0x21626D71  # !bmq
MAGIC2 = 0x424D5121  # BMQ!
RECORD_MAGIC = 0x2A724563  # *rEc
JOURNAL_RECORD_SIZE = 60
FILE_TYPE_DATA, FILE_TYPE_JOURNAL, FILE_TYPE_QLIST = 1, 2, 3
REC_MESSAGE, REC_CONFIRM, REC_DELETION, REC_QUEUE_OP, REC_JOURNAL_OP = 1, 2, 3, 4, 5
WORD, DWORD = 4, 8


class StorageFormatError(ValueError):
    """Invalid journal/DATA content (the reference returns rc_INVALID_* codes)."""


def _be32(a, off):
    return (a[off].astype(np.uint32) << 24) | (a[off + 1].astype(np.uint32) << 16) | \
           (a[off + 2].astype(np.uint32) << 8) | a[off + 3].astype(np.uint32)


def _as_u8(buf):
    if isinstance(buf, np.ndarray):
        return buf.view(np.uint8).reshape(-1)
    return np.frombuffer(bytes(buf), dtype=np.uint8)


def parse_file_header(buf, expect_type):
    """Return the byte size of the BlazingMQ FileHeader (FileHeader::headerWords)."""
    a = _as_u8(buf)
    if a.size < 32 or int(_be32(a, 0)) != MAGIC1 or int(_be32(a, 4)) != MAGIC2:
        raise StorageFormatError("bad BlazingMQ file magic")
    hw = int(a[8]) & 0x3F
    ftype = int(a[9]) & 0x7F
    if ftype != expect_type:
        raise StorageFormatError("file type %d, expected %d" % (ftype, expect_type))
    return hw * WORD


# FileStore::recoverMessages result codes (mqbs_filestore.cpp:1073-1091)
RC_SUCCESS = 0
RC_INVALID_PRIMARY_LEASE_ID = -2
RC_INVALID_SEQ_NUMBER = -3
RC_INVALID_QUEUE_OP_RECORD = -4
RC_NULL_QUEUE_KEY = -5
RC_DUPLICATE_QUEUE_KEY = -7
RC_INVALID_QUEUE_KEY = -8
RC_INVALID_DATA_OFFSET = -11
RC_INVALID_SYNC_PT_SUB_TYPE = -12
RC_INVALID_DELETION_RECORD = -14
RC_INVALID_CONFIRM_RECORD = -15
RC_INVALID_MESSAGE_RECORD = -16
RC_INVALID_DATA_RECORD = -17

# QueueOpType (mqbs_filestoreprotocol.h:1630), JournalOpType (:1841)
OP_PURGE, OP_CREATION, OP_DELETION, OP_ADDITION = 1, 2, 3, 4
JOURNAL_OP_SYNCPOINT = 2
NULL_KEY = bytes(5)


class RecoveryConfig(ctypes.Structure):
    """include/bmqcrc_protocol.h bmqcrc_recovery_cfg: the queues recovery
    knows.  with_csl=False: the journal's own QueueOp CREATION records;
    with_csl=True: the cluster state's queue keys (5 bytes each)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("with_csl", ctypes.c_int32),
                ("queue_keys", ctypes.c_void_p), ("n_queue_keys", ctypes.c_uint64)]


def _cfg(with_csl, queue_keys):
    if not with_csl:
        return None, None
    keys = np.frombuffer(b"".join(bytes(k) for k in queue_keys), np.uint8).copy()
    if keys.size != 5 * len(queue_keys):
        raise ValueError("queue keys are 5 bytes each")
    c = RecoveryConfig(ctypes.sizeof(RecoveryConfig), 1,
                       keys.ctypes.data if keys.size else None, len(queue_keys))
    return c, keys  # keep the key buffer alive with the struct


def _int(b, off, n):
    return int.from_bytes(bytes(b[off:off + n]), "big")


def journal_bounds_py(journal):
    """FileStoreProtocolUtil::lastJournalSyncPoint / lastJournalRecord
    (mqbs_filestoreprotocolutil.cpp:165-289), restated: (last sync point
    offset, last record offset), 0 meaning none."""
    a = _as_u8(journal)
    fh = parse_file_header(a, FILE_TYPE_JOURNAL)
    start = fh + int(a[fh]) * WORD
    n = (a.size - start) // JOURNAL_RECORD_SIZE if a.size > start else 0
    lsp = 0
    for i in range(n - 1, -1, -1):
        r = a[start + i * JOURNAL_RECORD_SIZE:start + (i + 1) * JOURNAL_RECORD_SIZE]
        seq = (_int(r, 2, 2) << 32) | _int(r, 4, 4)
        if (r[0] >> 4) == REC_JOURNAL_OP and _int(r, 24, 4) == JOURNAL_OP_SYNCPOINT and \
                _int(r, 8, 4) and seq and _int(r, 56, 4) == RECORD_MAGIC:
            lsp = start + i * JOURNAL_RECORD_SIZE
            break
    if a.size <= start:
        return 0, 0
    cur, prev = (lsp + JOURNAL_RECORD_SIZE, lsp) if lsp else (start, 0)
    while cur + JOURNAL_RECORD_SIZE <= a.size:
        if (a[cur] >> 4) == 0 or _int(a, cur + 56, 4) != RECORD_MAGIC:
            break
        prev, cur = cur, cur + JOURNAL_RECORD_SIZE
    return lsp, prev


def recovery_selection_py(journal, data, with_csl=False, queue_keys=()):
    """Pure-Python restatement of the MESSAGE records mqbs::FileStore::
    recoverMessages CRCs (mqbs_filestore.cpp:1045-2646), used by the tests to
    hold the native walk (``scan_partition``) to the reference's decisions.

    Two backward passes from the journal's last record, each stopping at the
    first record with an undefined type, a zero lease id / sequence number or
    a bad magic.  First pass (:1120-1453): queue DELETION offsets, queues
    alive (CREATION records, or the cluster state with CSL), the first sync
    point.  Second pass (:1490-2646): PSN checks against the write head (the
    last record), sync point checks, whole-queue PURGEs, DELETION GUIDs, and
    every MESSAGE that survives them -- DATA record checks, then its CRC.
    Returns dict(recovery_rc, error_record_offset, record_offset, app_offset,
    app_length, crc32c) in the backward order."""
    j, d = _as_u8(journal), _as_u8(data)
    fh = parse_file_header(j, FILE_TYPE_JOURNAL)
    parse_file_header(d, FILE_TYPE_DATA)
    start = fh + int(j[fh]) * WORD
    out = {"recovery_rc": 0, "error_record_offset": 0, "record_offset": [], "app_offset": [],
           "app_length": [], "crc32c": []}
    _, last = journal_bounds_py(j)
    if last == 0:
        return out

    def hdr(pos):
        r = j[pos:pos + JOURNAL_RECORD_SIZE]
        return int(r[0]) >> 4, (_int(r, 2, 2) << 32) | _int(r, 4, 4), _int(r, 8, 4), r

    positions = []
    for pos in range(last, start - 1, -JOURNAL_RECORD_SIZE):
        t, seq, lease, r = hdr(pos)
        if t == 0 or seq == 0 or lease == 0 or _int(r, 56, 4) != RECORD_MAGIC:
            break
        positions.append(pos)

    def fail(rc, pos):
        out["recovery_rc"], out["error_record_offset"] = rc, pos
        return out

    live = set(bytes(k) for k in queue_keys) if with_csl else set()
    deleted_queue, deleted_app, first_sync = {}, {}, 0
    for pos in positions:
        t, _, _, r = hdr(pos)
        if t == REC_JOURNAL_OP:
            first_sync = pos
            continue
        if t != REC_QUEUE_OP:
            continue
        op, qkey, akey = _int(r, 32, 4), bytes(r[22:27]), bytes(r[27:32])
        if op == 0:
            return fail(RC_INVALID_QUEUE_OP_RECORD, pos)
        if qkey == NULL_KEY:
            return fail(RC_NULL_QUEUE_KEY, pos)
        if op == OP_DELETION:
            if with_csl and akey == NULL_KEY and qkey in live:
                return fail(RC_INVALID_DELETION_RECORD, pos)
            if akey == NULL_KEY:
                deleted_queue.setdefault(qkey, pos)
            else:
                deleted_app.setdefault(akey, pos)
        elif op in (OP_CREATION, OP_ADDITION):
            if qkey in deleted_queue:
                continue
            if with_csl:
                if qkey not in live:
                    return fail(RC_INVALID_QUEUE_KEY, pos)
            elif qkey in live:
                return fail(RC_DUPLICATE_QUEUE_KEY, pos)
            elif op == OP_CREATION:
                live.add(qkey)

    deleted_guids, purged = set(), set()
    lease, seq = hdr(last)[2], hdr(last)[1] + 1

    def before_deletion(qkey, pos):
        return qkey in deleted_queue and pos < deleted_queue[qkey]

    for pos in positions:
        t, s, ls, r = hdr(pos)
        if ls > lease:
            return fail(RC_INVALID_PRIMARY_LEASE_ID, pos)
        if ls == lease and (s != seq - 1 if pos >= first_sync else s > seq - 1):
            return fail(RC_INVALID_SEQ_NUMBER, pos)
        lease, seq = ls, s
        if t == REC_JOURNAL_OP:
            sp_seq, sp_lease, doff = (_int(r, 28, 4) << 32) | _int(r, 32, 4), _int(r, 40, 4), \
                _int(r, 44, 4) * DWORD
            if r[23] == 0:
                return fail(RC_INVALID_SYNC_PT_SUB_TYPE, pos)
            if doff == 0 or d.size < doff:
                return fail(RC_INVALID_DATA_OFFSET, pos)
            # the reference's order (:1647-1713): lease 0, seq 0, lease ahead, seq mismatch
            if sp_lease == 0:
                return fail(RC_INVALID_PRIMARY_LEASE_ID, pos)
            if sp_seq == 0:
                return fail(RC_INVALID_SEQ_NUMBER, pos)
            if sp_lease > lease:
                return fail(RC_INVALID_PRIMARY_LEASE_ID, pos)
            if sp_lease == lease and sp_seq != seq:
                return fail(RC_INVALID_SEQ_NUMBER, pos)
        elif t == REC_QUEUE_OP:
            qkey, akey, op = bytes(r[22:27]), bytes(r[27:32]), _int(r, 32, 4)
            if before_deletion(qkey, pos):
                continue
            if op == OP_ADDITION and not with_csl and qkey not in live:
                # an ADDITION whose CREATION the first pass did not see (:2018-2030)
                return fail(RC_INVALID_QUEUE_KEY, pos)
            if op == OP_PURGE and qkey in live and akey == NULL_KEY:
                purged.add(qkey)
        elif t == REC_DELETION:
            qkey, guid = bytes(r[23:28]), bytes(r[28:44])
            if guid == bytes(16) or qkey == NULL_KEY:
                return fail(RC_INVALID_DELETION_RECORD, pos)
            if not before_deletion(qkey, pos) and qkey not in purged:
                deleted_guids.add(guid)
        elif t == REC_CONFIRM:
            if bytes(r[32:48]) == bytes(16) or bytes(r[22:27]) == NULL_KEY:
                return fail(RC_INVALID_CONFIRM_RECORD, pos)
        elif t == REC_MESSAGE:
            qkey, guid = bytes(r[22:27]), bytes(r[36:52])
            if guid == bytes(16) or qkey == NULL_KEY:
                return fail(RC_INVALID_MESSAGE_RECORD, pos)
            o = _int(r, 32, 4) * DWORD
            if o == 0 or o > d.size:
                return fail(RC_INVALID_DATA_OFFSET, pos)
            if before_deletion(qkey, pos) or qkey in purged:
                continue
            if guid in deleted_guids:
                deleted_guids.discard(guid)
                continue
            if o + 8 > d.size:
                return fail(RC_INVALID_DATA_RECORD, pos)
            w0, w1 = _int(d, o, 4), _int(d, o + 4, 4)
            hs, total, opt = (w0 >> 29) * WORD, (w0 & 0x1FFFFFFF) * WORD, (w1 >> 8) * WORD
            if hs == 0 or total == 0 or hs + opt >= total or o + total > d.size:
                return fail(RC_INVALID_DATA_RECORD, pos)
            pad = int(d[o + total - 1])
            if pad < 1 or pad > DWORD or total < hs + opt + pad:
                return fail(RC_INVALID_DATA_RECORD, pos)
            if qkey not in live:
                return fail(RC_INVALID_QUEUE_KEY, pos)
            out["record_offset"].append(pos)
            out["app_offset"].append(o + hs + opt)
            out["app_length"].append(total - hs - opt - pad)
            out["crc32c"].append(_int(r, 52, 4))
    return out


def _native_call(fn, *args):
    try:
        return fn(*args)
    except N.BmqCrcError as e:
        if e.rc == N.BMQCRC_EINVAL:
            raise StorageFormatError(str(e)) from e
        raise


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a.size else None


def journal_bounds(journal):
    """Native ``bmqcrc_journal_bounds``: (last sync point offset, last record
    offset) as JournalFileIterator bounds the journal (0 = none)."""
    j = np.ascontiguousarray(_as_u8(journal))
    lsp, last = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _native_call(lambda: N.check(N.lib.bmqcrc_journal_bounds(
        _ptr(j), j.size, ctypes.byref(lsp), ctypes.byref(last))))
    return int(lsp.value), int(last.value)


def scan_partition(journal, data, with_csl=False, queue_keys=()):
    """Native walk (``bmqcrc_journal_scan``, CPU only): the MESSAGE records
    FileStore::recoverMessages would CRC, in its (backward) order, as numpy
    arrays (record_offset, app_offset, app_length, crc32c), plus the
    reference's recovery_rc and the offending record's error_record_offset."""
    j, d = np.ascontiguousarray(_as_u8(journal)), np.ascontiguousarray(_as_u8(data))
    cfg, _keys = _cfg(with_csl, queue_keys)
    rrc, err = ctypes.c_int(0), ctypes.c_uint64(0)

    def scan(cap, *arrs):
        n = N.lib.bmqcrc_journal_scan(_ptr(j), j.size, _ptr(d), d.size,
                                      ctypes.byref(cfg) if cfg is not None else None,
                                      ctypes.byref(rrc), ctypes.byref(err),
                                      *[_ptr(a) if a is not None else None for a in arrs], cap)
        return N.check_count(n)

    n = _native_call(scan, 0, None, None, None, None)
    out = {"record_offset": np.zeros(n, np.uint64), "app_offset": np.zeros(n, np.uint64),
           "app_length": np.zeros(n, np.uint32), "crc32c": np.zeros(n, np.uint32)}
    _native_call(scan, n, out["record_offset"], out["app_offset"], out["app_length"],
                 out["crc32c"])
    out["recovery_rc"] = int(rrc.value)
    out["error_record_offset"] = int(err.value)
    return out


def verify_partition(journal, data, bad_cap=1 << 20, device=-1, with_csl=False, queue_keys=(),
                     devices=None):
    """Recovery CRC check of a whole partition: one native walk selecting the
    records FileStore::recoverMessages CRCs, one batched GPU verify
    (``bmqcrc_recover_verify``).

    Returns dict(n_messages, n_bad, bad_record_offsets, recovery_rc,
    error_record_offset).  A mismatch is what the reference reports with
    BMQTSK_ALARMLOG_ALARM("RECOVERY") (mqbs_filestore.cpp:2613-2624) and
    keeps going; offsets come in the order it raises them (backward).
    ``devices`` (several ordinals, repeats allowed) spreads the DATA file's
    staging and verify over those devices (bmqcrc_opts.ndevices).
    """
    j, d = np.ascontiguousarray(_as_u8(journal)), np.ascontiguousarray(_as_u8(data))
    cfg, _keys = _cfg(with_csl, queue_keys)
    n_msgs, n_bad = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rrc, err = ctypes.c_int(0), ctypes.c_uint64(0)
    bad = np.zeros(max(int(bad_cap), 1), np.uint64)
    opts = N.make_opts(device=device, devices=devices)

    def run():
        return N.check(N.lib.bmqcrc_recover_verify(
            _ptr(j), j.size, _ptr(d), d.size, ctypes.byref(cfg) if cfg is not None else None,
            ctypes.byref(rrc), ctypes.byref(err), ctypes.byref(n_msgs), ctypes.byref(n_bad),
            _ptr(bad), int(bad_cap), ctypes.byref(opts)))

    _native_call(run)
    k = min(int(n_bad.value), int(bad_cap))
    return {"n_messages": int(n_msgs.value), "n_bad": int(n_bad.value),
            "bad_record_offsets": bad[:k].copy(), "recovery_rc": int(rrc.value),
            "error_record_offset": int(err.value)}


# ----------------------------------------------------------------------------
# Writer (tests and synthetic partitions): the layout FileStore produces.
# ----------------------------------------------------------------------------
def file_header(file_type, partition_id=0):
    h = np.zeros(32, np.uint8)
    h[0:4] = np.frombuffer(MAGIC1.to_bytes(4, "big"), np.uint8)
    h[4:8] = np.frombuffer(MAGIC2.to_bytes(4, "big"), np.uint8)
    h[8] = (1 << 6) | 8          # protocol version 1, 8 header words
    h[9] = 0x80 | file_type      # bitness 64, file type
    h[20:24] = np.frombuffer(int(partition_id).to_bytes(4, "big"), np.uint8)
    return h


class PartitionWriter:
    """Builds a (journal, DATA) file pair record by record, in the layout
    FileStore writes (mqbs_filestoreprotocol.h: RecordHeader :1014,
    MessageRecord :1125, ConfirmRecord :1339, DeletionRecord :1518,
    QueueOpRecord :1694, JournalOpRecord :1953, DataHeader :703).  Every
    record takes the next sequence number of the current primary lease;
    ``new_lease`` starts a new primary (sequence numbers restart at 1).  Each
    method returns the record's journal offset (``message`` also its GUID)."""

    JOURNAL_HEADER = 32 + 12  # FileHeader + JournalFileHeader (3 words)

    def __init__(self, lease_id=1, timestamp=0x6720EAB4, partition_id=0):
        self.lease, self.seq, self.ts = lease_id, 0, timestamp
        self.recs = []
        self.data = [file_header(FILE_TYPE_DATA, partition_id).tobytes(),
                     bytes([2, 0, 0, 0, 0, 0, 0, 0])]
        self.dpos = 40
        self.partition_id = partition_id
        self._guid = 0

    def _record(self, rtype, body, flags=0):
        self.seq += 1
        r = bytearray(JOURNAL_RECORD_SIZE)
        r[0:2] = ((rtype << 12) | (flags & 0xFFF)).to_bytes(2, "big")
        r[2:4] = (self.seq >> 32).to_bytes(2, "big")
        r[4:8] = (self.seq & 0xFFFFFFFF).to_bytes(4, "big")
        r[8:12] = self.lease.to_bytes(4, "big")
        r[12:20] = self.ts.to_bytes(8, "big")
        for off, b in body:
            r[off:off + len(b)] = b
        r[56:60] = RECORD_MAGIC.to_bytes(4, "big")
        self.recs.append(bytes(r))
        return self.JOURNAL_HEADER + (len(self.recs) - 1) * JOURNAL_RECORD_SIZE

    def new_lease(self, lease_id):
        self.lease, self.seq = lease_id, 0

    def sync_point(self, sync_type=1):
        """JournalOpRecord SYNCPOINT for the current PSN (its own sequence
        number, :1953), pointing at the current end of the DATA file."""
        seq = self.seq + 1
        return self._record(REC_JOURNAL_OP, [
            (23, bytes([sync_type])), (24, JOURNAL_OP_SYNCPOINT.to_bytes(4, "big")),
            (28, (seq >> 32).to_bytes(4, "big")), (32, (seq & 0xFFFFFFFF).to_bytes(4, "big")),
            (40, self.lease.to_bytes(4, "big")), (44, (self.dpos // DWORD).to_bytes(4, "big")),
            (48, (9).to_bytes(4, "big"))])

    def queue_op(self, op, queue_key, app_key=NULL_KEY):
        return self._record(REC_QUEUE_OP, [
            (22, bytes(queue_key)), (27, bytes(app_key)), (32, int(op).to_bytes(4, "big")),
            (36, (9 if op in (OP_CREATION, OP_ADDITION) else 0).to_bytes(4, "big"))])

    def message(self, app, queue_key, crc=None, guid=None, data_header=None, file_key=NULL_KEY,
                ref_count=1, data_flags=0, timestamp=None):
        """MESSAGE record + its DATA record (12-byte DataHeader, no options,
        1..8 padding bytes).  `crc` overrides the stored CRC (default: the
        CRC32C of `app`); `data_header` overrides the DataHeader bytes.
        `file_key` is the DATA file's key, `ref_count` the 20-bit reference
        count (low 12 bits in the RecordHeader's flags, the rest at @20),
        `data_flags` the DataHeader's flags byte and `timestamp` this
        record's own (default: the writer's)."""
        app = bytes(app)
        rem = (12 + len(app)) % DWORD
        pad = DWORD - rem if rem else DWORD
        total = 12 + len(app) + pad
        hdr = data_header if data_header is not None else \
            ((3 << 29) | (total // WORD)).to_bytes(4, "big") + \
            (int(data_flags) & 0xFF).to_bytes(4, "big") + bytes(4)
        self.data.append(bytes(hdr) + app + bytes([pad]) * pad)
        if guid is None:
            self._guid += 1
            guid = (0x40000000000000000000000000000000 | self._guid).to_bytes(16, "big")
        crc = Crc32c.calculate(app) if crc is None else int(crc)
        ref_count = int(ref_count) & 0xFFFFF
        body = [(20, bytes([ref_count >> 12])), (22, bytes(queue_key)), (27, bytes(file_key)),
                (32, (self.dpos // DWORD).to_bytes(4, "big")), (36, bytes(guid)),
                (52, crc.to_bytes(4, "big"))]
        if timestamp is not None:
            body.append((12, int(timestamp).to_bytes(8, "big")))
        off = self._record(REC_MESSAGE, body, flags=ref_count & 0xFFF)
        self.dpos += total
        return off, bytes(guid)

    def confirm(self, guid, queue_key, app_key=NULL_KEY, reason=0):
        """`reason` is the ConfirmReason in the RecordHeader's flags: 0
        CONFIRMED, 1 REJECTED, 2 AUTO_CONFIRMED."""
        return self._record(REC_CONFIRM, [(22, bytes(queue_key)), (27, bytes(app_key)),
                                          (32, bytes(guid))], flags=int(reason))

    def deletion(self, guid, queue_key, flags=0):
        """`flags` is the DeletionRecordFlag in the RecordHeader's flags: 0
        none, 1 IMPLICIT_CONFIRM, 2 TTL_EXPIRATION, 3 NO_SC_QUORUM."""
        return self._record(REC_DELETION, [(23, bytes(queue_key)), (28, bytes(guid))],
                            flags=int(flags))

    def files(self):
        journal = file_header(FILE_TYPE_JOURNAL, self.partition_id).tobytes() + \
            bytes([3, 15]) + bytes(10) + b"".join(self.recs)
        return (np.frombuffer(journal, np.uint8).copy(),
                np.frombuffer(b"".join(self.data), np.uint8).copy())


DEFAULT_QUEUE_KEY = b"\x26\xda\xcd\xc9\x74"


def write_partition(app_datas, crcs=None, lease_id=1, timestamp=0x6720EAB4,
                    queue_key=DEFAULT_QUEUE_KEY):
    """(journal, data) byte arrays of one queue: a QueueOp CREATION record,
    then one MESSAGE record per entry of `app_datas` (bytes), all of them
    outstanding.  `crcs` (optional) overrides the CRC stored in the journal
    (default: the true CRC32C of the app data)."""
    w = PartitionWriter(lease_id=lease_id, timestamp=timestamp)
    w.queue_op(OP_CREATION, queue_key)
    for i, app in enumerate(app_datas):
        w.message(app, queue_key, crc=None if crcs is None else crcs[i])
    return w.files()


# ----------------------------------------------------------------------------
# Device-side writer: DATA records and journal MessageRecords in one call.
# ----------------------------------------------------------------------------
def pack_records(src, src_offsets, lengths, queue_keys, guids, *, file_key, lease_id, first_seq,
                 data_file_pos, timestamp=0, timestamps=None, ref_counts=None, data_flags=None,
                 expected=None, dst=None, journal_dst=None, out=None, stream=None, sync=True):
    """Pack device-resident payloads into DATA-file records and their journal
    MessageRecords on the GPU (``bmqcrc_message_records_pack``): the bytes
    ``PartitionWriter.message`` appends to both files for n messages, what
    ``FileStore::writeMessageRecord`` writes with no options.  Message i's
    application data is ``src[src_offsets[i]:][:lengths[i]]``; its DATA record
    stands for byte ``data_file_pos + record_offsets[i]`` of the DATA file and
    its sequence number is ``first_seq + i``.

    Device tensors only, all on one MI355X, contiguous: ``src`` / ``dst`` /
    ``journal_dst`` uint8, ``src_offsets`` / ``timestamps`` int64, ``lengths``
    / ``ref_counts`` / ``expected`` / ``out`` int32 (read as u32),
    ``queue_keys`` uint8 with 5 and ``guids`` uint8 with 16 bytes per message,
    ``data_flags`` uint8.  ``file_key`` is 5 bytes.  With ``expected`` the
    journal stores those CRCs, as the broker stores the one that arrived with
    the message, and the result counts the messages whose computed CRC
    differs.  ``dst=None`` allocates exactly the bytes needed, which takes a
    sum of the lengths on the host and so ``sync=True``; ``journal_dst=None``
    allocates 60 n bytes.

    Returns ``(dst, journal_dst, record_offsets, crcs, result)``:
    ``record_offsets`` (int64, one per record and the total last), ``crcs``
    the computed CRCs (``out``, or a new int32 tensor) and ``result`` the
    dict of ``last_records_pack`` (None with ``sync=False``).  All or nothing:
    a record above the DataHeader's size field, a source range outside
    ``src``, a ``dst`` too small or a DATA file position past what
    MessageOffsetDwords addresses writes nothing and, with ``sync=True``,
    raises ``BmqCrcError`` (BMQCRC_EINVAL) naming the kind and the lowest
    message; with ``sync=False`` ask ``last_records_pack``.  Not meant to be
    captured into a graph."""
    import torch
    n = src_offsets.numel() if isinstance(src_offsets, torch.Tensor) else -1
    for name, t, dt in (("src", src, torch.uint8), ("src_offsets", src_offsets, torch.int64),
                        ("lengths", lengths, torch.int32), ("queue_keys", queue_keys, torch.uint8),
                        ("guids", guids, torch.uint8)):
        if not (isinstance(t, torch.Tensor) and t.dtype == dt and t.is_contiguous()):
            raise TypeError("%s must be a contiguous %s tensor" % (name, dt))
    if lengths.numel() != n or queue_keys.numel() != 5 * n or guids.numel() != 16 * n:
        raise ValueError("src_offsets/lengths/queue_keys/guids size mismatch")
    dev = src.device
    for name, t, dt in (("data_flags", data_flags, torch.uint8),
                        ("ref_counts", ref_counts, torch.int32),
                        ("timestamps", timestamps, torch.int64),
                        ("expected", expected, torch.int32), ("out", out, torch.int32)):
        if t is not None and not (isinstance(t, torch.Tensor) and t.device == dev and
                                  t.dtype == dt and t.is_contiguous() and t.numel() == n):
            raise TypeError("%s must be a contiguous %s tensor of %d elements on %s"
                            % (name, dt, n, dev))
    for name, t in (("dst", dst), ("journal_dst", journal_dst)):
        if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and
                                  t.is_contiguous()):
            raise TypeError("%s must be a contiguous %s tensor" % (name, torch.uint8))
    file_key = bytes(file_key)
    if len(file_key) != 5:
        raise ValueError("file_key is 5 bytes")
    if not src.is_cuda:
        raise TypeError("pack_records takes device tensors only (src is on %s)" % dev)
    for name, t in (("src_offsets", src_offsets), ("lengths", lengths),
                    ("queue_keys", queue_keys), ("guids", guids), ("dst", dst),
                    ("journal_dst", journal_dst)):
        if t is not None and t.device != dev:
            raise TypeError("%s must be on %s like src" % (name, dev))
    if dst is None:
        if not sync:
            raise ValueError("dst is required when sync=False: sizing it reads the lengths back")
        dwords = (((lengths.to(torch.int64) & 0xFFFFFFFF) + 12) >> 3) + 1
        dst = torch.empty(int((8 * dwords).sum().item()) if n else 0, dtype=torch.uint8,
                          device=dev)
    if journal_dst is None:
        journal_dst = torch.empty(JOURNAL_RECORD_SIZE * n, dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=dev)
    record_offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    p = N.RecordsPack()
    p.struct_size = ctypes.sizeof(N.RecordsPack)
    p.src, p.src_bytes = src.data_ptr(), src.numel()
    p.src_offsets, p.lengths = src_offsets.data_ptr(), lengths.data_ptr()
    p.queue_keys, p.guids = queue_keys.data_ptr(), guids.data_ptr()
    for name, t in (("data_flags", data_flags), ("ref_counts", ref_counts),
                    ("timestamps", timestamps), ("expected", expected)):
        setattr(p, name, t.data_ptr() if t is not None else None)
    p.file_key = (ctypes.c_uint8 * 5)(*file_key)
    p.lease_id, p.first_seq, p.timestamp = int(lease_id), int(first_seq), int(timestamp)
    p.data_file_pos, p.n = int(data_file_pos), n
    p.dst, p.dst_bytes = dst.data_ptr(), dst.numel()
    p.journal_dst, p.journal_bytes = journal_dst.data_ptr(), journal_dst.numel()
    p.record_offsets, p.out = record_offsets.data_ptr(), out.data_ptr()
    o = N.make_opts(device=dev.index if dev.index is not None else -1, stream=stream.cuda_stream,
                    flags=N.BMQCRC_F_DEVICE_PTRS | (0 if sync else N.BMQCRC_F_ASYNC))
    res = N.RecordsResult()
    N.check(N.lib.bmqcrc_message_records_pack(ctypes.byref(p), ctypes.byref(res), ctypes.byref(o)))
    return dst, journal_dst, record_offsets, out, res.as_dict() if sync else None


def last_records_pack(device, stream=None):
    """Result of the previous ``pack_records`` on (device, stream)
    (bmqcrc_last_records_pack); waits for it.  A dict: ``n_msgs``,
    ``data_bytes`` and ``journal_bytes`` (both 0 when refused), ``n_bad`` and
    ``first_bad`` (the messages whose computed CRC differs from ``expected``
    and the lowest of them, ``n_msgs`` when none), ``refused_kind`` (0,
    ``BMQCRC_REC_PACK_OK``, or the kind refused) and ``refused_index`` (the
    lowest offending message).  ``stream=None`` is the device's default
    stream."""
    res = N.RecordsResult()
    N.check(N.lib.bmqcrc_last_records_pack(
        device, stream.cuda_stream if stream is not None else None, ctypes.byref(res)))
    return res.as_dict()


# ----------------------------------------------------------------------------
# Device-side reader: the inverse of pack_records.
# ----------------------------------------------------------------------------
UnpackedRecords = collections.namedtuple(
    "UnpackedRecords", "record_index app_offsets lengths queue_keys guids data_flags ref_counts "
                       "timestamps expected crcs")


def unpack_records(journal, data, *, data_file_pos, msg_cap=None, select=None, verify=True,
                   stream=None, sync=True):
    """Walk device-resident journal records and their DATA records on the GPU
    (``bmqcrc_message_records_unpack``), the inverse of ``pack_records``: every
    MESSAGE record and its DataHeader checked as ``FileStore::recoverMessages``
    checks them, and what the packers take for every message, as device
    tensors, with no payload byte and no descriptor crossing PCIe.

    ``journal`` is a contiguous uint8 device tensor (4-byte aligned) of whole
    60-byte records -- the record run, not the journal file with its headers;
    ``journal_dst`` of ``pack_records`` is one.  ``data`` (uint8, 8-byte
    aligned) stands for bytes ``[data_file_pos, data_file_pos + data.numel())``
    of the DATA file; 0 means the whole file.  ``select`` (uint8, one byte per
    record, or None) leaves the MESSAGE records whose byte is 0 out: they are
    checked up to their data offset, take no slot, and their DATA record is
    never read.  ``msg_cap`` is the capacity of the per-message arrays; None
    is the record count.  With ``verify`` every message's application data is
    CRC'd and compared with the stored CRC (ask ``last_records_unpack`` for
    n_bad / first_bad); the CRC pass runs over all ``msg_cap`` slots, so a
    tight ``msg_cap`` is cheaper.

    Returns the named tuple ``(record_index, app_offsets, lengths, queue_keys,
    guids, data_flags, ref_counts, timestamps, expected, crcs)``: int32 record
    indices, int64 offsets in ``data`` of the application data, int32 lengths,
    uint8 queue keys (5 per message), GUIDs (16) and DataHeader flags, int32
    reference counts, int64 timestamps, the stored CRCs and the computed ones
    (int32; ``crcs`` is None when ``verify=False``).  With ``sync=True`` the
    tensors are sliced to the messages found, and a malformed record or more
    than ``msg_cap`` messages raises ``BmqCrcError`` (BMQCRC_EINVAL) naming
    kind and record: nothing is written then.  With ``sync=False`` the tensors
    keep their full capacity and ``last_records_unpack`` reports the outcome.
    Not meant to be captured into a graph."""
    import torch
    for name, t in (("journal", journal), ("data", data), ("select", select)):
        if name == "select" and t is None:
            continue
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.is_contiguous()):
            raise TypeError("%s must be a contiguous %s tensor" % (name, torch.uint8))
    dev = journal.device
    if not journal.is_cuda:
        raise TypeError("unpack_records takes device tensors only (journal is on %s)" % dev)
    for name, t in (("data", data), ("select", select)):
        if t is not None and t.device != dev:
            raise TypeError("%s must be on %s like journal" % (name, dev))
    if journal.numel() % JOURNAL_RECORD_SIZE:
        raise ValueError("journal must hold whole 60-byte records")
    n_records = journal.numel() // JOURNAL_RECORD_SIZE
    if select is not None and select.numel() != n_records:
        raise ValueError("select needs one byte per record")
    cap = n_records if msg_cap is None else int(msg_cap)
    if cap < 0:
        raise ValueError("msg_cap must not be negative")

    def new(shape, dt):
        return torch.empty(shape, dtype=dt, device=dev)
    u = UnpackedRecords(new(cap, torch.int32), new(cap, torch.int64), new(cap, torch.int32),
                        new((cap, 5), torch.uint8), new((cap, 16), torch.uint8),
                        new(cap, torch.uint8), new(cap, torch.int32), new(cap, torch.int64),
                        new(cap, torch.int32), new(cap, torch.int32) if verify else None)
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    # (an empty tensor has no address: the call wants one for the required arrays)
    spare = new(1, torch.int64)
    p = N.RecordsUnpack()
    p.struct_size = ctypes.sizeof(N.RecordsUnpack)
    p.journal, p.journal_bytes = journal.data_ptr() or spare.data_ptr(), journal.numel()
    p.n_records = n_records
    p.data, p.data_bytes = data.data_ptr() or spare.data_ptr(), data.numel()
    p.data_file_pos = int(data_file_pos)
    p.select = select.data_ptr() if select is not None else None
    p.msg_cap = cap
    for name in u._fields[:9]:
        setattr(p, name, getattr(u, name).data_ptr())
    p.app_offsets = p.app_offsets or spare.data_ptr()
    p.lengths = p.lengths or spare.data_ptr()
    p.out = u.crcs.data_ptr() if verify else None
    o = N.make_opts(device=dev.index if dev.index is not None else -1, stream=stream.cuda_stream,
                    flags=N.BMQCRC_F_DEVICE_PTRS | (0 if sync else N.BMQCRC_F_ASYNC))
    r = N.RecordsUnpackResult()
    N.check(N.lib.bmqcrc_message_records_unpack(ctypes.byref(p), ctypes.byref(r), ctypes.byref(o)))
    if not sync:
        return u
    n = int(r.n_msgs)
    return UnpackedRecords(*[t[:n] if t is not None else None for t in u])


def last_records_unpack(device, stream=None):
    """The result of the previous ``unpack_records`` on (device, stream)
    (bmqcrc_last_records_unpack), as a dict; waits for it.  ``n_records``,
    ``n_msgs`` and ``n_skipped`` (the slots taken and the unselected MESSAGE
    records; both 0 when refused), ``n_bad`` and ``first_bad`` (slots whose
    computed CRC differs from the stored one, and the lowest; ``n_msgs`` when
    none), ``refused_kind`` (0, ``BMQCRC_REC_UNPACK_OK``, or the kind) and
    ``refused_index`` (a record index).  ``stream=None`` is the device's
    default stream."""
    r = N.RecordsUnpackResult()
    N.check(N.lib.bmqcrc_last_records_unpack(
        device, stream.cuda_stream if stream is not None else None, ctypes.byref(r)))
    return r.as_dict()


# ----------------------------------------------------------------------------
# Device-side selection: which MESSAGE records recovery CRCs.
# ----------------------------------------------------------------------------
def select_records(journal, *, data_file_bytes, with_csl=False, queue_keys=(), queue_cap=1 << 16,
                   stream=None, sync=True):
    """The MESSAGE records ``FileStore::recoverMessages`` CRCs, decided on the
    GPU from a device-resident run of journal records
    (``bmqcrc_journal_select``): what ``scan_partition`` decides on the host,
    as the ``select`` bytes ``unpack_records`` takes, so that ``unpack_events
    -> pack_records -> select_records -> unpack_records(verify=True)`` recovers
    a partition that lies in HBM with no per-record work on the host.

    ``journal`` is a contiguous uint8 device tensor (4-byte aligned) of whole
    60-byte records: the record run up to the journal's last valid record
    (``journal_bounds`` gives it for a file), not the file with its headers.
    ``data_file_bytes`` is the size of the DATA file; no DATA byte is read, so
    a selected message with a malformed DATA record stays selected and
    ``unpack_records`` refuses it (where the host walk says
    RC_INVALID_DATA_RECORD).  With ``with_csl`` the live queues are
    ``queue_keys``: a sequence of 5-byte keys, which is uploaded, or a uint8
    device tensor of 5 bytes per key.  ``queue_cap`` bounds the distinct queue
    keys (QueueOp records' and ``queue_keys``') the call holds.

    Returns ``select``, a uint8 tensor on the journal's device with one byte
    per record; with ``sync=True`` ``(select, result)``, ``result`` being the
    dict of ``last_journal_select``.  A non-zero
    ``recovery_rc`` is a result: the records above ``error_record`` are still
    selected, as the reference had CRC'd them.  More distinct keys than
    ``queue_cap`` raises ``BmqCrcError`` (BMQCRC_EINVAL) with ``sync=True``.
    Not meant to be captured into a graph."""
    import torch
    if not (isinstance(journal, torch.Tensor) and journal.dtype == torch.uint8 and
            journal.is_contiguous()):
        raise TypeError("journal must be a contiguous %s tensor" % torch.uint8)
    dev = journal.device
    if not journal.is_cuda:
        raise TypeError("select_records takes device tensors only (journal is on %s)" % dev)
    if journal.numel() % JOURNAL_RECORD_SIZE:
        raise ValueError("journal must hold whole 60-byte records")
    if isinstance(queue_keys, torch.Tensor):
        if not (queue_keys.dtype == torch.uint8 and queue_keys.is_contiguous() and
                queue_keys.device == dev and queue_keys.numel() % 5 == 0):
            raise TypeError("queue_keys must be a contiguous %s tensor of 5 bytes per key on %s"
                            % (torch.uint8, dev))
        keys = queue_keys
    else:
        raw = b"".join(bytes(k) for k in queue_keys)
        if len(raw) != 5 * len(queue_keys):
            raise ValueError("queue keys are 5 bytes each")
        keys = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev) if raw else None
    n_records = journal.numel() // JOURNAL_RECORD_SIZE
    select = torch.empty(n_records, dtype=torch.uint8, device=dev)
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    # (an empty tensor has no address: the call wants one for the required arrays)
    spare = torch.empty(8, dtype=torch.uint8, device=dev)
    p = N.JournalSelect()
    p.struct_size = ctypes.sizeof(N.JournalSelect)
    p.journal, p.journal_bytes = journal.data_ptr() or spare.data_ptr(), journal.numel()
    p.n_records, p.data_file_bytes = n_records, int(data_file_bytes)
    p.with_csl = 1 if with_csl else 0
    if keys is not None and keys.numel():
        p.queue_keys, p.n_queue_keys = keys.data_ptr(), keys.numel() // 5
    p.queue_cap = int(queue_cap)
    p.select = select.data_ptr() or spare.data_ptr()
    o = N.make_opts(device=dev.index if dev.index is not None else -1, stream=stream.cuda_stream,
                    flags=N.BMQCRC_F_DEVICE_PTRS | (0 if sync else N.BMQCRC_F_ASYNC))
    r = N.JournalSelectResult()
    N.check(N.lib.bmqcrc_journal_select(ctypes.byref(p), ctypes.byref(r), ctypes.byref(o)))
    return (select, r.as_dict()) if sync else select


def last_journal_select(device, stream=None):
    """The result of the previous ``select_records`` on (device, stream)
    (bmqcrc_last_journal_select), as a dict; waits for it.  ``n_records``;
    ``first_record`` (``select`` is meaningful from there on and 0 below: the
    record above the walk's lower end or above the failing record;
    ``n_records`` when nothing is selected); ``n_selected``, ``n_deleted`` and
    ``n_purged`` (MESSAGE records of that run kept, skipped by a DELETION of
    their GUID, skipped by their queue's PURGE or DELETION); ``recovery_rc``
    (0 or a ``RC_*`` code) and ``error_record`` (the offending record's index,
    ``n_records`` when none); ``refused_kind`` (0 or
    ``BMQCRC_JSEL_TOO_MANY_QUEUES``).  ``stream=None`` is the device's default
    stream."""
    r = N.JournalSelectResult()
    N.check(N.lib.bmqcrc_last_journal_select(
        device, stream.cuda_stream if stream is not None else None, ctypes.byref(r)))
    return r.as_dict()


# ----------------------------------------------------------------------------
# Device-side compaction: the outstanding records into a new run and window.
# ----------------------------------------------------------------------------
CONFIRMS_AS_KEPT = N.BMQCRC_ROLLOVER_CONFIRMS_AS_KEPT
CONFIRMS_FOLLOW_MESSAGES = N.BMQCRC_ROLLOVER_CONFIRMS_FOLLOW_MESSAGES

RolledRecords = collections.namedtuple("RolledRecords", "dst journal_dst new_index crcs result")


def rollover_records(journal, data, *, data_file_pos, new_data_file_pos, keep=None,
                     confirm_mode=CONFIRMS_AS_KEPT, sync_point=None, timestamp=0, dst=None,
                     journal_dst=None, stream=None, sync=True):
    """Roll the outstanding records of a device-resident partition over into a
    new journal run and a new DATA window on the GPU
    (``bmqcrc_partition_rollover``): the loop of ``FileStore::rolloverImpl``
    over ``writeRolledOverRecord`` and the sync point behind it, with every
    kept message's stored CRC checked against the bytes carried over.

    ``journal`` (uint8, 4-byte aligned, whole 60-byte records) and ``data``
    (uint8, 8-byte aligned, standing for bytes ``[data_file_pos, data_file_pos
    + data.numel())`` of the DATA file) are what ``unpack_records`` takes.
    ``keep`` (uint8, one byte per record, or None for every record that may be
    kept) says which records are rolled; for MESSAGE records it is the
    ``select`` of ``select_records``.  A JOURNAL_OP record is never rolled and
    a non-zero ``keep`` on one refuses the call.  With ``confirm_mode =
    CONFIRMS_FOLLOW_MESSAGES`` a CONFIRM record is kept exactly when a kept
    MESSAGE record of the run has its GUID and queue key, whatever ``keep``
    says.  ``sync_point`` (a record index, or None) names the run's SYNCPOINT
    record restated behind the kept records with ``timestamp`` and the new DATA
    file's end.  ``new_data_file_pos`` is the byte of the new DATA file that
    ``dst[0]`` stands for (a non-zero multiple of 8: the new file's headers).

    ``dst=None`` allocates ``data.numel()`` bytes and ``journal_dst=None`` 60
    bytes per record and sync point: both bounds hold unless two kept MESSAGE
    records share a DATA record.

    Returns the named tuple ``(dst, journal_dst, new_index, crcs, result)``:
    ``new_index`` (int32, the record's position in the new run, -1 when not
    kept), ``crcs`` (int32, the computed CRC of a kept MESSAGE record's
    application data, 0 elsewhere) and ``result`` the dict of
    ``last_rollover`` (None with ``sync=False``); with ``sync=True`` ``dst``
    and ``journal_dst`` are sliced to the bytes written.  All or nothing: a
    malformed record, a destination too small or a DATA file position past
    what MessageOffsetDwords addresses writes nothing and, with ``sync=True``,
    raises ``BmqCrcError`` (BMQCRC_EINVAL) naming kind and record.  A CRC
    mismatch does not fail the call: ``result["n_bad"]`` counts them.  Not
    meant to be captured into a graph."""
    import torch
    for name, t in (("journal", journal), ("data", data), ("keep", keep), ("dst", dst),
                    ("journal_dst", journal_dst)):
        if t is None and name not in ("journal", "data"):
            continue
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.is_contiguous()):
            raise TypeError("%s must be a contiguous %s tensor" % (name, torch.uint8))
    dev = journal.device
    if not journal.is_cuda:
        raise TypeError("rollover_records takes device tensors only (journal is on %s)" % dev)
    for name, t in (("data", data), ("keep", keep), ("dst", dst), ("journal_dst", journal_dst)):
        if t is not None and t.device != dev:
            raise TypeError("%s must be on %s like journal" % (name, dev))
    if journal.numel() % JOURNAL_RECORD_SIZE:
        raise ValueError("journal must hold whole 60-byte records")
    n_records = journal.numel() // JOURNAL_RECORD_SIZE
    if keep is not None and keep.numel() != n_records:
        raise ValueError("keep needs one byte per record")
    if dst is None:
        dst = torch.empty(data.numel(), dtype=torch.uint8, device=dev)
    if journal_dst is None:
        journal_dst = torch.empty(JOURNAL_RECORD_SIZE * (n_records + (sync_point is not None)),
                                  dtype=torch.uint8, device=dev)
    new_index = torch.empty(n_records, dtype=torch.int32, device=dev)
    crcs = torch.empty(n_records, dtype=torch.int32, device=dev)
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    # (an empty tensor has no address: the call wants one for the required arrays)
    spare = torch.empty(8, dtype=torch.uint8, device=dev)
    p = N.Rollover()
    p.struct_size = ctypes.sizeof(N.Rollover)
    p.journal, p.journal_bytes = journal.data_ptr() or spare.data_ptr(), journal.numel()
    p.n_records = n_records
    p.data, p.data_bytes = data.data_ptr() or spare.data_ptr(), data.numel()
    p.data_file_pos = int(data_file_pos)
    p.keep = keep.data_ptr() if keep is not None and n_records else None
    p.confirm_mode = int(confirm_mode)
    p.sync_point = N.BMQCRC_ROLLOVER_NO_SYNC_POINT if sync_point is None else int(sync_point)
    p.timestamp = int(timestamp)
    p.new_data_file_pos = int(new_data_file_pos)
    p.dst, p.dst_bytes = dst.data_ptr() or spare.data_ptr(), dst.numel()
    p.journal_dst = journal_dst.data_ptr() or spare.data_ptr()
    p.journal_dst_bytes = journal_dst.numel()
    p.new_index = new_index.data_ptr() if n_records else None
    p.out = crcs.data_ptr() if n_records else None
    o = N.make_opts(device=dev.index if dev.index is not None else -1, stream=stream.cuda_stream,
                    flags=N.BMQCRC_F_DEVICE_PTRS | (0 if sync else N.BMQCRC_F_ASYNC))
    r = N.RolloverResult()
    N.check(N.lib.bmqcrc_partition_rollover(ctypes.byref(p), ctypes.byref(r), ctypes.byref(o)))
    if not sync:
        return RolledRecords(dst, journal_dst, new_index, crcs, None)
    return RolledRecords(dst[:int(r.data_bytes)], journal_dst[:int(r.journal_bytes)], new_index,
                         crcs, r.as_dict())


def last_rollover(device, stream=None):
    """The result of the previous ``rollover_records`` on (device, stream)
    (bmqcrc_last_rollover), as a dict; waits for it.  ``n_records``;
    ``n_kept`` (records rolled, the sync point not counted) and ``n_messages``
    (the MESSAGE records among them); ``journal_bytes`` (the sync point
    included) and ``data_bytes`` written; ``n_bad`` and ``first_bad`` (kept
    MESSAGE records whose computed CRC differs from the stored one, and the
    lowest; ``n_records`` when none); ``refused_kind`` (0,
    ``BMQCRC_ROLLOVER_OK``, or the kind) and ``refused_index`` (a record, or
    ``n_records`` for the sync point).  After a refused call only
    ``n_records`` and the two ``refused_*`` are set.  ``stream=None`` is the
    device's default stream."""
    r = N.RolloverResult()
    N.check(N.lib.bmqcrc_last_rollover(
        device, stream.cuda_stream if stream is not None else None, ctypes.byref(r)))
    return r.as_dict()


# ----------------------------------------------------------------------------
# Device-side confirms: the CONFIRM and DELETION records of a batch.
# ----------------------------------------------------------------------------
CONFIRM_STATUS_CONFIRM, CONFIRM_STATUS_DELETION, CONFIRM_STATUS_NOT_FOUND = 0, 1, 2

ConfirmedRecords = collections.namedtuple(
    "ConfirmedRecords", "journal_dst status target new_index left_out result")


def confirm_records(journal, guids, queue_keys, *, lease_id, first_seq, select=None, app_keys=None,
                    reasons=None, timestamp=0, timestamps=None, journal_dst=None, stream=None,
                    sync=True):
    """Turn a batch of consumer confirms into the CONFIRM and DELETION records
    of a device-resident partition on the GPU (``bmqcrc_confirm_records_pack``):
    what ``FileBackedStorage::confirm`` appends through
    ``FileStore::writeConfirmRecord`` and, when a message's count reaches
    zero, ``writeDeletionRecord``.  There is no CRC in this call: a confirm
    carries no payload.

    The journal is the state: ``journal`` (uint8, 4-byte aligned, whole 60-byte
    records) is the partition's run, and the outstanding count of every message
    is derived from it on every call -- the MESSAGE record's refCount less its
    CONFIRM records (AUTO_CONFIRMED ones excepted), nothing once a DELETION
    record names it.  ``select`` (uint8, one byte per record, the output of
    ``select_records``, or None for every MESSAGE record) says which MESSAGE
    records count.  Appending ``journal_dst`` to the run and calling again
    needs no other bookkeeping; ``journal_dst`` may be the tail of the tensor
    ``journal`` is a slice of.

    The batch is ``guids`` (uint8, 16 bytes per confirm), ``queue_keys``
    (uint8, 5 per confirm), ``app_keys`` (uint8, 5 per confirm, or None for
    the null key), ``reasons`` (uint8, 0 CONFIRMED or 1 REJECTED, or None) and
    ``timestamps`` (int64 per confirm, or None for ``timestamp``).  A confirm
    whose message is not live writes nothing (status 2); every other one writes
    one record, sequence numbers from ``first_seq`` on under ``lease_id``: the
    DELETION record in place of the confirm that brings the count to zero
    (status 1), a CONFIRM record otherwise (status 0).

    ``journal_dst=None`` sizes the destination exactly with a size-only call
    first, which takes ``sync=True``.

    Returns the named tuple ``(journal_dst, status, target, new_index,
    left_out, result)``: ``status`` (uint8 per confirm), ``target`` (int32,
    the MESSAGE record, -1 for none), ``new_index`` (int32, the record's place
    in ``journal_dst``, -1 for none), ``left_out`` (int32 per record of the
    run: the references a MESSAGE record has left after this call, so
    ``left_out > 0`` is the next ``select``; None for an empty batch, which
    launches nothing) and ``result`` the dict of
    ``last_confirm_records`` (None with ``sync=False``); with ``sync=True``
    ``journal_dst`` is sliced to the bytes written.  All or nothing: a
    malformed record, two selected MESSAGE records with one key, a null GUID
    or queue key, a message confirmed more often in one call than it has
    references left, or a destination too small writes nothing and, with
    ``sync=True``, raises ``BmqCrcError`` (BMQCRC_EINVAL) naming kind and
    index.  Not meant to be captured into a graph."""
    import torch
    for name, t in (("journal", journal), ("guids", guids), ("queue_keys", queue_keys),
                    ("select", select), ("app_keys", app_keys), ("reasons", reasons),
                    ("journal_dst", journal_dst)):
        if t is None and name not in ("journal", "guids", "queue_keys"):
            continue
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.is_contiguous()):
            raise TypeError("%s must be a contiguous %s tensor" % (name, torch.uint8))
    dev = journal.device
    if not journal.is_cuda:
        raise TypeError("confirm_records takes device tensors only (journal is on %s)" % dev)
    if timestamps is not None and not (isinstance(timestamps, torch.Tensor) and
                                       timestamps.dtype == torch.int64 and
                                       timestamps.is_contiguous()):
        raise TypeError("timestamps must be a contiguous %s tensor" % torch.int64)
    for name, t in (("guids", guids), ("queue_keys", queue_keys), ("select", select),
                    ("app_keys", app_keys), ("reasons", reasons), ("timestamps", timestamps),
                    ("journal_dst", journal_dst)):
        if t is not None and t.device != dev:
            raise TypeError("%s must be on %s like journal" % (name, dev))
    if journal.numel() % JOURNAL_RECORD_SIZE:
        raise ValueError("journal must hold whole 60-byte records")
    n_records = journal.numel() // JOURNAL_RECORD_SIZE
    if guids.numel() % 16:
        raise ValueError("guids must hold 16 bytes per confirm")
    n = guids.numel() // 16
    if queue_keys.numel() != 5 * n:
        raise ValueError("queue_keys needs 5 bytes per confirm")
    for name, t, per in (("select", select, None), ("app_keys", app_keys, 5),
                         ("reasons", reasons, 1), ("timestamps", timestamps, 1)):
        if t is not None and t.numel() != (n_records if per is None else per * n):
            raise ValueError("%s has the wrong size" % name)
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    # (an empty tensor has no address: the call wants one for the required arrays)
    spare = torch.empty(8, dtype=torch.uint8, device=dev)
    p = N.ConfirmPack()
    p.struct_size = ctypes.sizeof(N.ConfirmPack)
    p.journal, p.journal_bytes = journal.data_ptr() or spare.data_ptr(), journal.numel()
    p.n_records = n_records
    p.select = select.data_ptr() if select is not None and n_records else None
    p.guids = guids.data_ptr() or spare.data_ptr()
    p.queue_keys = queue_keys.data_ptr() or spare.data_ptr()
    for name, t in (("app_keys", app_keys), ("reasons", reasons), ("timestamps", timestamps)):
        setattr(p, name, t.data_ptr() if t is not None and n else None)
    p.n, p.timestamp = n, int(timestamp)
    p.first_seq, p.lease_id = int(first_seq), int(lease_id)
    dev_index = dev.index if dev.index is not None else -1
    if journal_dst is None:
        if not sync:
            raise ValueError("journal_dst is required when sync=False: sizing it waits for a "
                             "size-only call")
        o = N.make_opts(device=dev_index, stream=stream.cuda_stream, flags=N.BMQCRC_F_DEVICE_PTRS)
        r = N.ConfirmPackResult()
        N.check(N.lib.bmqcrc_confirm_records_pack(ctypes.byref(p), ctypes.byref(r),
                                                  ctypes.byref(o)))
        journal_dst = torch.empty(int(r.journal_bytes), dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.uint8, device=dev)
    target = torch.empty(n, dtype=torch.int32, device=dev)
    new_index = torch.empty(n, dtype=torch.int32, device=dev)
    left_out = torch.empty(n_records, dtype=torch.int32, device=dev) if n else None
    p.journal_dst = journal_dst.data_ptr() or spare.data_ptr()
    p.journal_dst_bytes = journal_dst.numel()
    p.status = status.data_ptr() if n else None
    p.target = target.data_ptr() if n else None
    p.new_index = new_index.data_ptr() if n else None
    p.left_out = left_out.data_ptr() if n and n_records else None
    o = N.make_opts(device=dev_index, stream=stream.cuda_stream,
                    flags=N.BMQCRC_F_DEVICE_PTRS | (0 if sync else N.BMQCRC_F_ASYNC))
    r = N.ConfirmPackResult()
    N.check(N.lib.bmqcrc_confirm_records_pack(ctypes.byref(p), ctypes.byref(r), ctypes.byref(o)))
    if not sync:
        return ConfirmedRecords(journal_dst, status, target, new_index, left_out, None)
    return ConfirmedRecords(journal_dst[:int(r.journal_bytes)], status, target, new_index,
                            left_out, r.as_dict())


def last_confirm_records(device, stream=None):
    """The result of the previous ``confirm_records`` on (device, stream)
    (bmqcrc_last_confirm_records), as a dict; waits for it.  ``n_confirms``;
    ``n_written`` records, of which ``n_confirm_records`` CONFIRM and
    ``n_deletions`` DELETION records; ``n_not_found`` confirms without a live
    message; ``journal_bytes`` written (or, after a size-only call, needed);
    ``next_seq``, the sequence number behind the last record; ``refused_kind``
    (0, ``BMQCRC_CONFIRM_PACK_OK``, or the kind) and ``refused_index`` (a
    record or a confirm, by kind).  After a refused call only ``n_confirms``
    and the two ``refused_*`` are set.  ``stream=None`` is the device's default
    stream."""
    r = N.ConfirmPackResult()
    N.check(N.lib.bmqcrc_last_confirm_records(
        device, stream.cuda_stream if stream is not None else None, ctypes.byref(r)))
    return r.as_dict()


# ----------------------------------------------------------------------------
# Device-side TTL: the DELETION records of the messages that have expired.
# ----------------------------------------------------------------------------
ExpiredRecords = collections.namedtuple(
    "ExpiredRecords",
    "journal_dst expired new_index select_out queue_expired queue_front result")


def expire_records(journal, queue_keys, ttl_seconds, *, now, lease_id, first_seq, select=None,
                   journal_dst=None, stream=None, sync=True):
    """Expire the messages of a device-resident partition whose TTL has run out
    on the GPU (``bmqcrc_expire_records_pack``): the DELETION records, flagged
    ``e_TTL_EXPIRATION``, that ``FileBackedStorage::gcExpiredMessages`` appends
    through ``FileStore::writeDeletionRecord``.  There is no CRC in this call:
    no payload byte is read.

    The journal is the state, as for ``confirm_records``: ``journal`` (uint8,
    4-byte aligned, whole 60-byte records) is the partition's run and ``select``
    (uint8, one byte per record, or None for every MESSAGE record) says which
    MESSAGE records count.  A message is live when it is selected and no
    DELETION record of the run names it; reference counts play no part.

    The queue table is ``queue_keys`` (uint8, 5 bytes per queue) and
    ``ttl_seconds`` (int64 per queue, read as unsigned); it may be empty.  With
    ``now`` the seconds from the epoch, a live message of queue q is young when
    ``(now - timestamp) mod 2**64 <= ttl_seconds[q]`` -- unsigned, as the
    reference computes it, so a timestamp in the future reads as expired -- and
    a live message expires when no young message of its queue stands before it
    in the run: the reference walks a queue from its head and stops at the
    first message that has not expired.  A live message whose queue is not in
    the table never expires.  Every expired message writes one DELETION record,
    in journal order, sequence numbers from ``first_seq`` on under ``lease_id``
    and with ``now`` as its timestamp.

    ``journal_dst=None`` sizes the destination exactly with a size-only call
    first, which takes ``sync=True``; ``journal_dst`` may be the tail of the
    tensor ``journal`` is a slice of.

    Returns the named tuple ``(journal_dst, expired, new_index, select_out,
    queue_expired, queue_front, result)``: ``expired`` (uint8 per record),
    ``new_index`` (int32, the DELETION record's place in ``journal_dst``, -1 for
    none), ``select_out`` (uint8, 1 for the MESSAGE records that are live and
    not expired: the next ``select``), ``queue_expired`` (int32 per queue) and
    ``queue_front`` (int32 per queue: the record of the queue's first young
    message, -1 for none), the last two None for an empty run, which launches
    nothing; ``result`` the dict of ``last_expire_records`` (None with
    ``sync=False``).  With ``sync=True`` ``journal_dst`` is sliced to the bytes
    written.  All or nothing: a malformed record, two selected MESSAGE records
    with one key, a null or repeated queue key in the table, or a destination
    too small writes nothing and, with ``sync=True``, raises ``BmqCrcError``
    (BMQCRC_EINVAL) naming kind and index.  Not meant to be captured into a
    graph."""
    import torch
    for name, t in (("journal", journal), ("queue_keys", queue_keys), ("select", select),
                    ("journal_dst", journal_dst)):
        if t is None and name not in ("journal", "queue_keys"):
            continue
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.is_contiguous()):
            raise TypeError("%s must be a contiguous %s tensor" % (name, torch.uint8))
    dev = journal.device
    if not journal.is_cuda:
        raise TypeError("expire_records takes device tensors only (journal is on %s)" % dev)
    if not (isinstance(ttl_seconds, torch.Tensor) and ttl_seconds.dtype == torch.int64 and
            ttl_seconds.is_contiguous()):
        raise TypeError("ttl_seconds must be a contiguous %s tensor" % torch.int64)
    for name, t in (("queue_keys", queue_keys), ("ttl_seconds", ttl_seconds), ("select", select),
                    ("journal_dst", journal_dst)):
        if t is not None and t.device != dev:
            raise TypeError("%s must be on %s like journal" % (name, dev))
    if journal.numel() % JOURNAL_RECORD_SIZE:
        raise ValueError("journal must hold whole 60-byte records")
    n_records = journal.numel() // JOURNAL_RECORD_SIZE
    n_queues = ttl_seconds.numel()
    if queue_keys.numel() != 5 * n_queues:
        raise ValueError("queue_keys needs 5 bytes per entry of ttl_seconds")
    if select is not None and select.numel() != n_records:
        raise ValueError("select has the wrong size")
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    # (an empty tensor has no address: the call wants one for the required arrays)
    spare = torch.empty(8, dtype=torch.uint8, device=dev)
    p = N.ExpirePack()
    p.struct_size = ctypes.sizeof(N.ExpirePack)
    p.journal, p.journal_bytes = journal.data_ptr() or spare.data_ptr(), journal.numel()
    p.n_records, p.n_queues = n_records, n_queues
    p.select = select.data_ptr() if select is not None and n_records else None
    p.queue_keys = queue_keys.data_ptr() if n_queues else None
    p.ttl_seconds = ttl_seconds.data_ptr() if n_queues else None
    p.now = int(now) & 0xFFFFFFFFFFFFFFFF
    p.first_seq, p.lease_id = int(first_seq), int(lease_id)
    dev_index = dev.index if dev.index is not None else -1
    if journal_dst is None:
        if not sync:
            raise ValueError("journal_dst is required when sync=False: sizing it waits for a "
                             "size-only call")
        o = N.make_opts(device=dev_index, stream=stream.cuda_stream, flags=N.BMQCRC_F_DEVICE_PTRS)
        r = N.ExpirePackResult()
        N.check(N.lib.bmqcrc_expire_records_pack(ctypes.byref(p), ctypes.byref(r),
                                                 ctypes.byref(o)))
        journal_dst = torch.empty(int(r.journal_bytes), dtype=torch.uint8, device=dev)
    expired = torch.empty(n_records, dtype=torch.uint8, device=dev)
    new_index = torch.empty(n_records, dtype=torch.int32, device=dev)
    select_out = torch.empty(n_records, dtype=torch.uint8, device=dev)
    per_queue = n_records != 0
    queue_expired = torch.empty(n_queues, dtype=torch.int32, device=dev) if per_queue else None
    queue_front = torch.empty(n_queues, dtype=torch.int32, device=dev) if per_queue else None
    p.journal_dst = journal_dst.data_ptr() or spare.data_ptr()
    p.journal_dst_bytes = journal_dst.numel()
    p.expired = expired.data_ptr() if n_records else None
    p.new_index = new_index.data_ptr() if n_records else None
    p.select_out = select_out.data_ptr() if n_records else None
    p.queue_expired = queue_expired.data_ptr() if per_queue and n_queues else None
    p.queue_front = queue_front.data_ptr() if per_queue and n_queues else None
    o = N.make_opts(device=dev_index, stream=stream.cuda_stream,
                    flags=N.BMQCRC_F_DEVICE_PTRS | (0 if sync else N.BMQCRC_F_ASYNC))
    r = N.ExpirePackResult()
    N.check(N.lib.bmqcrc_expire_records_pack(ctypes.byref(p), ctypes.byref(r), ctypes.byref(o)))
    if not sync:
        return ExpiredRecords(journal_dst, expired, new_index, select_out, queue_expired,
                              queue_front, None)
    return ExpiredRecords(journal_dst[:int(r.journal_bytes)], expired, new_index, select_out,
                          queue_expired, queue_front, r.as_dict())


def last_expire_records(device, stream=None):
    """The result of the previous ``expire_records`` on (device, stream)
    (bmqcrc_last_expire_records), as a dict; waits for it.  ``n_records``;
    ``n_live`` live MESSAGE records, of which ``n_expired`` wrote a DELETION
    record and ``n_no_queue`` have no entry in the queue table;
    ``journal_bytes`` written (or, after a size-only call, needed);
    ``next_seq``, the sequence number behind the last record; ``refused_kind``
    (0, ``BMQCRC_EXPIRE_PACK_OK``, or the kind) and ``refused_index`` (a record
    or a table entry, by kind).  After a refused call only ``n_records`` and the
    two ``refused_*`` are set.  ``stream=None`` is the device's default
    stream."""
    r = N.ExpirePackResult()
    N.check(N.lib.bmqcrc_last_expire_records(
        device, stream.cuda_stream if stream is not None else None, ctypes.byref(r)))
    return r.as_dict()


# ----------------------------------------------------------------------------
# Device-side delivery lists: each app's pending messages.
# ----------------------------------------------------------------------------
PendingRecords = collections.namedtuple(
    "PendingRecords",
    "records queue_ids sub_ids list_first app_pending app_next pending_mask result")


def pending_records(journal, queue_keys, app_first, app_keys, queue_ids, *, sub_ids=None,
                    from_record=None, limit=None, select=None, list_cap=None, stream=None,
                    sync=True):
    """List the messages of a device-resident partition that each consumer
    still has to see, on the GPU (``bmqcrc_pending_records_list``): what
    ``mqbi::Storage::getIterator(appKey)`` walks, as the ``records``,
    ``queue_ids`` and ``sub_ids`` that ``pack_push_events`` takes.  There is no
    CRC in this call: no payload byte is read.

    The journal is the state, as for ``confirm_records`` and ``expire_records``:
    ``journal`` (uint8, 4-byte aligned, whole 60-byte records) is the
    partition's run and ``select`` (uint8, one byte per record, or None for
    every MESSAGE record) says which MESSAGE records count.  A message is live
    when it is selected and no DELETION record of the run names it.

    The consumer table is in CSR form: queue q is ``queue_keys`` (uint8, 5 bytes
    per queue) and owns the apps ``app_first[q] .. app_first[q + 1] - 1``
    (int64, one entry more than there are queues; at most 32 apps a queue); an
    app's ordinal is its position in that range.  App a is ``app_keys`` (uint8,
    5 bytes per app, all zero for the null key), ``queue_ids[a]`` and
    ``sub_ids[a]`` (int32, what the PUSH packer wants for this consumer; the
    latter optional), ``from_record[a]`` (int32 read as unsigned, or None for
    all 0: the delivery cursor, messages below it are not listed) and
    ``limit[a]`` (int32 read as unsigned, or None for no limit).

    A live message of a queue in the table is pending for an app of that queue
    unless a CONFIRM record of the run (any reason, anywhere in the run) names
    the message and the app's non-null key; an app with the null key sees every
    live message of its queue.  Per-app PURGE records are not honoured.

    ``list_cap=None`` sizes the lists exactly with a size-only call first,
    which takes ``sync=True``.

    Returns the named tuple ``(records, queue_ids, sub_ids, list_first,
    app_pending, app_next, pending_mask, result)``: the three lists (int32;
    ``sub_ids`` None without ``sub_ids``), grouped by app in table order and in
    journal order inside an app, app a's entries at ``[list_first[a],
    list_first[a + 1])`` (int64); ``app_pending`` (int32 per app: its pending
    messages, listed or not), ``app_next`` (int32 per app: the first pending
    record beyond its limit, the next call's ``from_record``; the number of
    records when there is none), ``pending_mask`` (int32 per record: bit
    ``ordinal`` for every app the message is pending for); ``result`` the dict
    of ``last_pending_records`` (None with ``sync=False``).  With ``sync=True``
    the lists are sliced to the entries written.  An empty run launches nothing
    and leaves every array unwritten.  All or nothing: a malformed record or
    table, or lists too small, writes nothing and, with ``sync=True``, raises
    ``BmqCrcError`` (BMQCRC_EINVAL) naming kind and index.  The call waits for
    its pair count on the host in either mode; ``sync=False`` leaves the sort
    and the stores in flight.  Not meant to be captured into a graph."""
    import torch
    typed = (("journal", journal, torch.uint8, True), ("queue_keys", queue_keys, torch.uint8, True),
             ("app_first", app_first, torch.int64, True), ("app_keys", app_keys, torch.uint8, True),
             ("queue_ids", queue_ids, torch.int32, True), ("sub_ids", sub_ids, torch.int32, False),
             ("from_record", from_record, torch.int32, False), ("limit", limit, torch.int32, False),
             ("select", select, torch.uint8, False))
    for name, t, dtype, required in typed:
        if t is None and not required:
            continue
        if not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.is_contiguous()):
            raise TypeError("%s must be a contiguous %s tensor" % (name, dtype))
    dev = journal.device
    if not journal.is_cuda:
        raise TypeError("pending_records takes device tensors only (journal is on %s)" % dev)
    for name, t, _, _ in typed[1:]:
        if t is not None and t.device != dev:
            raise TypeError("%s must be on %s like journal" % (name, dev))
    if journal.numel() % JOURNAL_RECORD_SIZE:
        raise ValueError("journal must hold whole 60-byte records")
    n_records = journal.numel() // JOURNAL_RECORD_SIZE
    n_queues, n_apps = app_first.numel() - 1, queue_ids.numel()
    if n_queues < 0 or queue_keys.numel() != 5 * n_queues:
        raise ValueError("queue_keys needs 5 bytes per queue and app_first one entry more than "
                         "there are queues")
    if app_keys.numel() != 5 * n_apps:
        raise ValueError("app_keys needs 5 bytes per entry of queue_ids")
    for name, t in (("sub_ids", sub_ids), ("from_record", from_record), ("limit", limit)):
        if t is not None and t.numel() != n_apps:
            raise ValueError("%s needs one entry per app, like queue_ids" % name)
    if select is not None and select.numel() != n_records:
        raise ValueError("select has the wrong size")
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    # (an empty tensor has no address: the call wants one for the required arrays)
    spare = torch.empty(8, dtype=torch.int64, device=dev)

    def at(t, needed=True):
        return (t.data_ptr() or spare.data_ptr()) if t is not None and needed else None

    p = N.PendingList()
    p.struct_size = ctypes.sizeof(N.PendingList)
    p.journal, p.journal_bytes = at(journal), journal.numel()
    p.n_records, p.n_queues, p.n_apps = n_records, n_queues, n_apps
    p.select = at(select, n_records)
    p.queue_keys, p.app_first = at(queue_keys, n_queues), at(app_first)
    p.app_keys, p.queue_ids = at(app_keys, n_apps), at(queue_ids, n_apps)
    p.sub_ids, p.from_record, p.limit = at(sub_ids, n_apps), at(from_record, n_apps), \
        at(limit, n_apps)
    dev_index = dev.index if dev.index is not None else -1
    if list_cap is None:
        if not sync:
            raise ValueError("list_cap is required when sync=False: sizing the lists waits for a "
                             "size-only call")
        o = N.make_opts(device=dev_index, stream=stream.cuda_stream, flags=N.BMQCRC_F_DEVICE_PTRS)
        r = N.PendingListResult()
        N.check(N.lib.bmqcrc_pending_records_list(ctypes.byref(p), ctypes.byref(r),
                                                  ctypes.byref(o)))
        list_cap = int(r.n_listed)
    list_cap = int(list_cap)
    records = torch.empty(list_cap, dtype=torch.int32, device=dev)
    out_queue_ids = torch.empty(list_cap, dtype=torch.int32, device=dev)
    with_subs = sub_ids is not None and n_apps != 0
    out_sub_ids = torch.empty(list_cap, dtype=torch.int32, device=dev) if with_subs else None
    list_first = torch.empty(n_apps + 1, dtype=torch.int64, device=dev)
    app_pending = torch.empty(n_apps, dtype=torch.int32, device=dev)
    app_next = torch.empty(n_apps, dtype=torch.int32, device=dev)
    pending_mask = torch.empty(n_records, dtype=torch.int32, device=dev)
    p.records, p.out_queue_ids, p.out_sub_ids = at(records), at(out_queue_ids), at(out_sub_ids)
    p.list_cap, p.list_first = list_cap, at(list_first)
    p.app_pending, p.app_next = at(app_pending, n_apps), at(app_next, n_apps)
    p.pending_mask = at(pending_mask, n_records)
    o = N.make_opts(device=dev_index, stream=stream.cuda_stream,
                    flags=N.BMQCRC_F_DEVICE_PTRS | (0 if sync else N.BMQCRC_F_ASYNC))
    r = N.PendingListResult()
    N.check(N.lib.bmqcrc_pending_records_list(ctypes.byref(p), ctypes.byref(r), ctypes.byref(o)))
    if not sync:
        return PendingRecords(records, out_queue_ids, out_sub_ids, list_first, app_pending,
                              app_next, pending_mask, None)
    n = int(r.n_listed)
    return PendingRecords(records[:n], out_queue_ids[:n],
                          out_sub_ids[:n] if out_sub_ids is not None else None, list_first,
                          app_pending, app_next, pending_mask, r.as_dict())


def last_pending_records(device, stream=None):
    """The result of the previous ``pending_records`` on (device, stream)
    (bmqcrc_last_pending_records), as a dict; waits for it.  ``n_records``;
    ``n_live`` live MESSAGE records, of which ``n_no_queue`` have no queue in the
    table; ``n_pending``, the pending (app, message) pairs; ``n_listed``, the
    entries written (or, after a size-only call, needed); ``n_unknown_confirms``
    and ``n_not_found``, the CONFIRM records whose app key no app of the queue
    has and those without a message; ``refused_kind`` (0,
    ``BMQCRC_PENDING_LIST_OK``, or the kind) and ``refused_index`` (a record, a
    queue or an app, by kind).  After a refused call only ``n_records`` and the
    two ``refused_*`` are set.  ``stream=None`` is the device's default
    stream."""
    r = N.PendingListResult()
    N.check(N.lib.bmqcrc_last_pending_records(
        device, stream.cuda_stream if stream is not None else None, ctypes.byref(r)))
    return r.as_dict()
