"""What bmqcrc_message_records_unpack (ABI 2.13) yields and refuses, restated in
numpy (shared by test_records_unpack_model.py and test_gpu_records_unpack.py;
not a test module).  It holds no product code: the only things it takes from
the package are the host CRC and the PartitionWriter that builds its inputs.

Record r is bytes [60 r, 60 r + 60) of the record run.  A MESSAGE record
(type 1) whose select byte is not 0 is a message; with o = 8 x the BE u32 @32
its DATA record lies at o - data_file_pos of the window.
"""
import numpy as np

from blazingmq_amd import Crc32c
from blazingmq_amd import storage as S

REC = 60
JH = 44          # FileHeader + JournalFileHeader in front of a journal file's records
MAGIC = 0x2A724563
K_HEADER, K_MESSAGE, K_OFFSET, K_DATA, K_MANY = 1, 2, 3, 4, 5
# FileStore::recoverMessages' result for the kinds that have one
KIND_RC = {K_MESSAGE: -16, K_OFFSET: -11, K_DATA: -17}
FIELDS = ("record_index", "app_offsets", "lengths", "queue_keys", "guids", "data_flags",
          "ref_counts", "timestamps", "expected")


def _be(b, lo, hi):
    return int.from_bytes(bytes(b[lo:hi]), "big")


def classify(rec, data, pos, selected):
    """One record: (kind refused or 0, None | "skipped" | dict of the message)."""
    rec = bytes(rec)
    rtype = rec[0] >> 4
    if rtype == 0 or _be(rec, 8, 12) == 0 or _be(rec, 2, 8) == 0 or _be(rec, 56, 60) != MAGIC:
        return K_HEADER, None
    if rtype != 1:
        return 0, None
    if rec[36:52] == bytes(16) or rec[22:27] == bytes(5):
        return K_MESSAGE, None
    o = 8 * _be(rec, 32, 36)
    end = len(data)
    if o == 0 or o < pos or o > pos + end:
        return K_OFFSET, None
    if not selected:
        return 0, "skipped"
    o -= pos
    if o + 8 > end:
        return K_DATA, None
    w0, w1 = _be(data, o, o + 4), _be(data, o + 4, o + 8)
    hs, total, opt = 4 * (w0 >> 29), 4 * (w0 & 0x1FFFFFFF), 4 * (w1 >> 8)
    if hs == 0 or total == 0 or hs + opt >= total or o + total > end:
        return K_DATA, None
    pad = int(data[o + total - 1])
    if pad < 1 or pad > 8 or total < hs + opt + pad:
        return K_DATA, None
    return 0, dict(app_offsets=o + hs + opt, lengths=total - hs - opt - pad,
                   queue_keys=np.frombuffer(rec[22:27], np.uint8),
                   guids=np.frombuffer(rec[36:52], np.uint8), data_flags=w1 & 0xFF,
                   ref_counts=(rec[20] << 12) | (_be(rec, 0, 2) & 0xFFF),
                   timestamps=_be(rec, 12, 20), expected=_be(rec, 52, 56))


def model(run, data, pos=0, select=None, cap=None, crcs=True):
    """The call's outcome for the record run `run` and the DATA window `data`
    standing for byte `pos` of the file.  `refused` is None or (kind, record);
    otherwise `n`, `n_skipped`, the arrays of FIELDS and `crcs` (host CRCs of
    the application data)."""
    run, data = np.asarray(run, np.uint8), np.asarray(data, np.uint8)
    assert run.size % REC == 0
    n_records = run.size // REC
    found, worst, skipped = [], None, 0
    for r in range(n_records):
        kind, what = classify(run[REC * r:REC * (r + 1)], data, pos,
                              select is None or select[r] != 0)
        if kind:
            worst = min(worst or (kind, r), (kind, r))
        elif what == "skipped":
            skipped += 1
        elif what is not None:
            what["record_index"] = r
            found.append(what)
    if worst is None and cap is not None and len(found) > cap:
        worst = (K_MANY, found[cap]["record_index"])
    m = dict(refused=worst, n_records=n_records)
    if worst is not None:
        return m
    n = len(found)
    m.update(n=n, n_skipped=skipped)
    dts = dict(record_index=np.uint32, app_offsets=np.uint64, lengths=np.uint32,
               data_flags=np.uint8, ref_counts=np.uint32, timestamps=np.uint64,
               expected=np.uint32)
    for name, dt in dts.items():
        m[name] = np.array([f[name] for f in found], dt)
    m["queue_keys"] = np.array([f["queue_keys"] for f in found], np.uint8).reshape(n, 5)
    m["guids"] = np.array([f["guids"] for f in found], np.uint8).reshape(n, 16)
    if crcs:
        m["crcs"] = np.array([Crc32c.calculate(data[int(a):int(a) + int(l)].tobytes())
                              for a, l in zip(m["app_offsets"], m["lengths"])], np.uint32)
    return m


# ---- inputs ------------------------------------------------------------------

def payload(rng, n):
    return rng.integers(0, 256, size=int(n), dtype=np.uint8).tobytes()


def data_header(app_len, options=b"", hs_words=3, flags=0):
    """(DataHeader bytes of hs_words words + options, total record bytes)."""
    assert len(options) % 4 == 0 and hs_words >= 2
    body = 4 * hs_words + len(options) + app_len
    total = (body // 8 + 1) * 8
    head = ((hs_words << 29) | (total // 4)).to_bytes(4, "big") + \
        (((len(options) // 4) << 8) | (flags & 0xFF)).to_bytes(4, "big") + \
        bytes(4 * (hs_words - 2))
    return head + bytes(options), total


def append_message(w, app, queue_key, options=b"", hs_words=3, **kw):
    """PartitionWriter.message with a DataHeader of `hs_words` words followed by
    `options`: the writer appends the journal record, pointing at the DATA
    file's end, and the DATA record it laid out is replaced by this one."""
    app = bytes(app)
    head, total = data_header(len(app), options, hs_words, kw.pop("data_flags", 0))
    pad = total - len(head) - len(app)
    at = w.dpos
    crc = kw.pop("crc", Crc32c.calculate(app))
    off, guid = w.message(b"", queue_key, crc=crc, **kw)
    w.data[-1] = head + app + bytes([pad]) * pad
    w.dpos = at + total
    return off, guid


def build_partition(rng, lens, others=0.5, queue_key=S.DEFAULT_QUEUE_KEY, variants=False):
    """(journal file, DATA file) of one queue: a CREATION record, then one
    MESSAGE record per entry of `lens` with random reference counts,
    timestamps and DataHeader flags, and after each, with probability
    `others`, a CONFIRM or a SYNCPOINT record.  No DELETION, PURGE or
    queue-DELETION record: recovery selects every MESSAGE record.  `variants`
    gives some messages options and a DataHeader of 2 or 4..7 words."""
    w = S.PartitionWriter(lease_id=3, timestamp=0x6720EAB4)
    w.queue_op(S.OP_CREATION, queue_key)
    for ln in lens:
        kw = dict(ref_count=int(rng.integers(0, 1 << 20)), data_flags=int(rng.integers(0, 256)),
                  timestamp=int(rng.integers(0, 1 << 63)))
        opts, hs = b"", 3
        if variants and rng.random() < 0.6:
            opts = payload(rng, 4 * int(rng.integers(0, 5)))
            hs = int(rng.choice([2, 3, 4, 5, 7]))
        _, guid = append_message(w, payload(rng, ln), queue_key, opts, hs, **kw)
        if rng.random() < others:
            if rng.random() < 0.5:
                w.confirm(guid, queue_key)
            else:
                w.sync_point()
    return w.files()


def message_records(run):
    run = np.asarray(run, np.uint8).reshape(-1, REC)
    return np.nonzero(run[:, 0] >> 4 == 1)[0]


VARIANTS = ("zero_guid", "zero_queue_key", "offset_0", "offset_past_end", "header_truncated",
            "header_words_0", "message_words_0", "header_and_options_fill_record",
            "record_past_end", "padding_0", "padding_9", "padding_exceeds_data")
VARIANT_KIND = dict(zero_guid=K_MESSAGE, zero_queue_key=K_MESSAGE, offset_0=K_OFFSET,
                    offset_past_end=K_OFFSET)


def malformed(name, seed=5):
    """(journal file, DATA file, index of the corrupted record): a good
    partition whose LAST record, an empty MESSAGE (total 16, padding 4), is
    corrupted -- the record the backward host walk visits first."""
    rng = np.random.default_rng(seed)
    w = S.PartitionWriter(lease_id=2)
    w.queue_op(S.OP_CREATION, S.DEFAULT_QUEUE_KEY)
    for ln in (5, 0, 130, 64):
        _, guid = w.message(payload(rng, ln), S.DEFAULT_QUEUE_KEY)
    w.confirm(guid, S.DEFAULT_QUEUE_KEY)
    w.sync_point()
    w.message(b"", S.DEFAULT_QUEUE_KEY)
    j, d = w.files()
    last = (j.size - JH) // REC - 1
    at = JH + REC * last
    o = 8 * _be(j, at + 32, at + 36)
    assert o == d.size - 16 and d[-1] == 4

    def put32(buf, where, v):
        buf[where:where + 4] = np.frombuffer(int(v).to_bytes(4, "big"), np.uint8)
    if name == "zero_guid":
        j[at + 36:at + 52] = 0
    elif name == "zero_queue_key":
        j[at + 22:at + 27] = 0
    elif name == "offset_0":
        put32(j, at + 32, 0)
    elif name == "offset_past_end":
        put32(j, at + 32, d.size // 8 + 1)
    elif name == "header_truncated":
        put32(j, at + 32, d.size // 8)        # o == end: a legal offset, no room for a header
    elif name == "header_words_0":
        d[o] &= 0x1F
    elif name == "message_words_0":
        put32(d, o, 3 << 29)
    elif name == "header_and_options_fill_record":
        put32(d, o + 4, 1 << 8)               # 12 + 4 >= 16
    elif name == "record_past_end":
        put32(d, o, (3 << 29) | 6)            # 24 bytes where 16 are left
    elif name == "padding_0":
        d[-1] = 0
    elif name == "padding_9":
        d[-1] = 9
    elif name == "padding_exceeds_data":
        d[-1] = 8                             # 12 + 8 > 16
    else:
        raise KeyError(name)
    return j, d, last
