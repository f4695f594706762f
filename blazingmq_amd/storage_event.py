"""STORAGE events: what a replica receives, and their application to a
device-resident partition (the replica side of the storage path).

Host-side mirror of ``bmqp::StorageEventBuilder`` / ``bmqp::StorageMessageIterator``
wire format (bmqp_storageeventbuilder.cpp, bmqp_storagemessageiterator.cpp,
bmqp_protocol.h):

  EventHeader (bmqp_protocol.h:746, 8 bytes)
      BE u32  F(1b)|Length(31b); u8 PV(2b)|Type(6b); u8 HeaderWords=2; u8 typeSpecific; u8 0
      Type is STORAGE (8) or PARTITION_SYNC (10)
  per message: StorageHeader (bmqp_protocol.h:2807, 12 bytes)
      BE u32  Flags(5b)|MessageWords(27b)
      u8      Reserved(2b)|StorageProtocolVersion(2b)|HeaderWords(4b)=3
      u8      MessageType (StorageMessageType, :2735: DATA 1, QLIST 2, CONFIRM 3,
              DELETION 4, JOURNAL_OP 5, QUEUE_OP 6)
      BE u16  PartitionId;  BE u32 JournalOffsetWords
  then the 60-byte journal record and, for DATA and QLIST, the payload: the
  whole DATA record (DataHeader, options, application data, 1..8 padding
  bytes) or the QLIST record.  No padding of the message: every part is a
  whole number of words.

``apply_events`` is the device-side form of ``FileStore::processStorageEvent``
(mqbs_filestore.cpp:6339) with ``FileStoreUtil::writeMessageRecordImpl``
(mqbs_filestoreutil.cpp:1408): ``bmqcrc_storage_event_apply``, which also
checks the CRC the producer stored at the cost of the copy the replica has to
make anyway.  ``pack_storage_events`` is the primary's side,
``FileStore::replicateRecord`` (mqbs_filestore.cpp:5763) with the builder above:
``bmqcrc_storage_event_pack``, which checks the same CRC on the way out.
"""
import collections
import ctypes

import numpy as np

from . import _native as N
from .storage import JOURNAL_RECORD_SIZE

EVENT_HEADER_SIZE = 8
STORAGE_HEADER_SIZE = 12
EVENT_TYPE_STORAGE = 8
EVENT_TYPE_PARTITION_SYNC = 10
PROTOCOL_VERSION = 1
STORAGE_PROTOCOL_VERSION = 1
WORD = 4
MAX_EVENT_SIZE_SOFT = 512 * 1024 * 1024           # EventHeader::k_MAX_SIZE_SOFT
MAX_PAYLOAD_SIZE_SOFT = (64 + 1) * 1024 * 1024    # StorageHeader::k_MAX_PAYLOAD_SIZE_SOFT
MSG_DATA, MSG_QLIST, MSG_CONFIRM, MSG_DELETION, MSG_JOURNAL_OP, MSG_QUEUE_OP = 1, 2, 3, 4, 5, 6
FLAG_RECEIPT_REQUESTED = 1                        # StorageHeaderFlags::e_RECEIPT_REQUESTED


class StorageEventBuilder:
    """Build STORAGE events.  ``pack_message`` is
    ``bmqp::StorageEventBuilder::packMessage``: a StorageHeader with
    ``headerWords = 3`` and ``messageWords = 3 + (60 + payload) / 4``, the
    journal record and, for DATA and QLIST messages, the payload.  A message
    that would take the event past ``max_event_bytes``
    (``EventHeader::k_MAX_SIZE_SOFT``) closes the event and starts the next,
    which is ``FileStore::replicateRecord``'s flush and retry; ``flush`` closes
    the event by hand.  ``finalize`` returns every event back to back with
    their offsets."""

    def __init__(self, event_type=EVENT_TYPE_STORAGE,
                 storage_protocol_version=STORAGE_PROTOCOL_VERSION,
                 max_event_bytes=MAX_EVENT_SIZE_SOFT):
        if event_type not in (EVENT_TYPE_STORAGE, EVENT_TYPE_PARTITION_SYNC):
            raise ValueError("a storage event is of type STORAGE or PARTITION_SYNC")
        self.event_type = event_type
        self.spv = storage_protocol_version
        self.max_event_bytes = max_event_bytes
        self._done = []      # closed events, as bytes
        self._chunks = []    # the open event behind its header
        self._size = EVENT_HEADER_SIZE
        self._count = 0

    def event_size(self):
        return self._size

    def message_count(self):
        """Messages of the open event."""
        return self._count

    def pack_message(self, message_type, partition_id, journal_offset_words, journal_record,
                     payload=b"", flags=0):
        record, payload = bytes(journal_record), bytes(payload)
        if len(record) != JOURNAL_RECORD_SIZE:
            raise ValueError("a journal record is 60 bytes")
        if len(payload) % WORD:
            raise ValueError("the payload must be word aligned")
        if message_type not in (MSG_DATA, MSG_QLIST):
            payload = b""    # packMessageImp appends the payload buffer for DATA and QLIST only
        total = len(record) + len(payload)
        if total > MAX_PAYLOAD_SIZE_SOFT:
            raise ValueError("PAYLOAD_TOO_BIG")
        if self._size + STORAGE_HEADER_SIZE + total > self.max_event_bytes:
            if not self._count:
                raise ValueError("EVENT_TOO_BIG")
            self.flush()
        words = STORAGE_HEADER_SIZE // WORD
        h = bytearray(STORAGE_HEADER_SIZE)
        h[0:4] = (((flags & 0x1F) << 27) | (words + total // WORD)).to_bytes(4, "big")
        h[4] = ((self.spv & 3) << 4) | words
        h[5] = message_type
        h[6:8] = int(partition_id).to_bytes(2, "big")
        h[8:12] = int(journal_offset_words).to_bytes(4, "big")
        self._chunks += [bytes(h), record, payload]
        self._size += STORAGE_HEADER_SIZE + total
        self._count += 1

    def flush(self):
        """Close the open event, empty or not."""
        h = bytearray(EVENT_HEADER_SIZE)
        h[0:4] = (self._size & 0x7FFFFFFF).to_bytes(4, "big")
        h[4] = (PROTOCOL_VERSION << 6) | self.event_type
        h[5] = EVENT_HEADER_SIZE // WORD
        self._done.append(bytes(h) + b"".join(self._chunks))
        self._chunks, self._size, self._count = [], EVENT_HEADER_SIZE, 0

    def finalize(self):
        """``(events, event_offsets)``: uint8 bytes of all events back to back
        and uint64 offsets, one per event and the total last.  An open event
        with messages is closed first."""
        if self._count:
            self.flush()
        sizes = np.array([len(e) for e in self._done], np.uint64)
        offsets = np.concatenate([np.zeros(1, np.uint64), np.cumsum(sizes, dtype=np.uint64)])
        return np.frombuffer(b"".join(self._done), np.uint8).copy(), offsets


class StorageMessageIterator:
    """Iterate the messages of one STORAGE event with
    ``bmqp::StorageMessageIterator::next``'s checks in its order; a violation
    raises ``ValueError``.  Yields dicts: the StorageHeader's fields, the
    offsets in the event of the header, the journal record and the payload,
    and the payload's length."""

    def __init__(self, event):
        self.ev = np.frombuffer(bytes(event), dtype=np.uint8) if not isinstance(
            event, np.ndarray) else event.view(np.uint8)
        if self.ev.size < EVENT_HEADER_SIZE:
            raise ValueError("shorter than an EventHeader")
        length = int.from_bytes(self.ev[0:4].tobytes(), "big") & 0x7FFFFFFF
        if length != self.ev.size or (int(self.ev[4]) & 0x3F) not in (
                EVENT_TYPE_STORAGE, EVENT_TYPE_PARTITION_SYNC):
            raise ValueError("not a STORAGE event of matching length")
        self.header_size = int(self.ev[5]) * WORD

    def __iter__(self):
        pos, ev = self.header_size, self.ev
        while pos < ev.size:
            if pos + 5 > ev.size:
                raise ValueError("NO_STORAGEHEADER at %d" % pos)
            hw = (int(ev[pos + 4]) & 0xF) * WORD
            if hw < 5 or pos + hw > ev.size:
                raise ValueError("NO_STORAGEHEADER at %d" % pos)
            w0 = int.from_bytes(ev[pos:pos + 4].tobytes(), "big")
            size = (w0 & 0x07FFFFFF) * WORD
            if size < hw:
                raise ValueError("INVALID_MESSAGE_SIZE at %d" % pos)
            if pos + size > ev.size:
                raise ValueError("NOT_ENOUGH_BYTES at %d" % pos)
            yield {
                "flags": w0 >> 27,
                "storage_protocol_version": (int(ev[pos + 4]) >> 4) & 3,
                "message_type": int(ev[pos + 5]),
                "partition_id": int.from_bytes(ev[pos + 6:pos + 8].tobytes(), "big"),
                "journal_offset_words": int.from_bytes(ev[pos + 8:pos + 12].tobytes(), "big")
                if hw >= 12 else 0,
                "header_offset": pos,
                "record_offset": pos + hw,
                "payload_offset": pos + hw + JOURNAL_RECORD_SIZE,
                "payload_length": size - hw - JOURNAL_RECORD_SIZE,
            }
            pos += size


Applied = collections.namedtuple(
    "Applied", "journal data types flags payload_offsets payload_lengths record_offsets lengths "
               "expected crcs event_first result")

REFUSALS = ("OK", "EVENT_OFFSETS", "EVENT_HEADER", "STORAGE_HEADER", "DATA_RECORD",
            "TOO_MANY_MESSAGES", "OUT_OF_SYNC", "DST_TOO_SMALL", "TOO_MANY_PIECES")


def apply_events(events, event_offsets=None, *, partition_id, journal_pos, data_file_pos,
                 lease_id=0, seq=0, msg_cap=None, journal_dst=None, data_dst=None, stream=None,
                 sync=True):
    """Apply device-resident STORAGE events to a device-resident partition on
    the GPU (``bmqcrc_storage_event_apply``): every message's journal record
    to ``journal_dst + 60 i``, every DATA message's DATA record to ``data_dst``
    behind its predecessor's, byte for byte what the reference's replica
    appends to its two files -- and the application data's CRC32-C compared
    with the one the producer stored, which the reference leaves to recovery.

    ``events`` is a contiguous uint8 device tensor (4-byte aligned),
    ``event_offsets`` int64 with one entry more than there are events or None
    for one event, the whole buffer.  The replica's state: ``partition_id``;
    ``journal_pos`` and ``data_file_pos``, the file positions that
    ``journal_dst[0]`` and ``data_dst[0]`` stand for; ``(lease_id, seq)``, the
    primary sequence number of the last record applied (``lease_id=0``: none
    known yet).  ``msg_cap`` is the capacity of the per-message arrays; None
    is ``events.numel() // 72``, the most a buffer can hold.  ``journal_dst``
    / ``data_dst`` (uint8; ``data_dst`` 8-byte aligned) None allocates
    ``60 msg_cap`` bytes and as many as ``events`` has: no event holds more.
    With ``sync=True`` they are sliced to what was written.  ``sync=False``
    requires both.

    Returns the named tuple ``(journal, data, types, flags, payload_offsets,
    payload_lengths, record_offsets, lengths, expected, crcs, event_first,
    result)``: uint8 message types and StorageHeader flags, what follows the
    journal record (int64 offset in ``events``, int32 length: a QLIST
    message's record, which the caller writes), int64 offsets in ``data`` of
    the DATA records with the total last, int32 application-data lengths,
    stored and computed CRCs (all 0 for a message that is not DATA), the first
    message of each event with the count last, and the dict of
    ``last_storage_apply`` (None with ``sync=False``).  CRC mismatches do not
    fail the call: ``result["n_bad"]`` / ``["first_bad"]`` report them and the
    bytes are applied.  All or nothing: a malformed event, a message of
    another partition, one that does not continue the journal, the DATA file
    or the sequence numbers, more than ``msg_cap`` messages or a destination
    too small writes nothing and, with ``sync=True``, raises ``BmqCrcError``
    (BMQCRC_EINVAL) naming kind, event, message and offset; with
    ``sync=False`` ask ``last_storage_apply``.  Not meant to be captured into
    a graph."""
    import torch
    for name, t, dt in (("events", events, torch.uint8),
                        ("event_offsets", event_offsets, torch.int64),
                        ("journal_dst", journal_dst, torch.uint8),
                        ("data_dst", data_dst, torch.uint8)):
        if name != "events" and t is None:
            continue
        if not (isinstance(t, torch.Tensor) and t.dtype == dt and t.is_contiguous()):
            raise TypeError("%s must be a contiguous %s tensor" % (name, dt))
    dev = events.device
    if not events.is_cuda:
        raise TypeError("apply_events takes device tensors only (events is on %s)" % dev)
    for name, t in (("event_offsets", event_offsets), ("journal_dst", journal_dst),
                    ("data_dst", data_dst)):
        if t is not None and t.device != dev:
            raise TypeError("%s must be on %s like events" % (name, dev))
    if event_offsets is not None and event_offsets.numel() < 1:
        raise ValueError("event_offsets needs one entry more than there are events")
    if not sync and (journal_dst is None or data_dst is None):
        raise ValueError("journal_dst and data_dst are required when sync=False")
    n_events = event_offsets.numel() - 1 if event_offsets is not None else 1
    cap = events.numel() // (STORAGE_HEADER_SIZE + JOURNAL_RECORD_SIZE) if msg_cap is None \
        else int(msg_cap)
    if cap < 0:
        raise ValueError("msg_cap must not be negative")

    def new(shape, dt):
        return torch.empty(shape, dtype=dt, device=dev)
    spare = new(8, torch.uint8)  # (an empty tensor has no address: the call wants one)
    if journal_dst is None:
        journal_dst = new(JOURNAL_RECORD_SIZE * cap, torch.uint8)
    if data_dst is None:
        data_dst = new(events.numel(), torch.uint8)
    u = Applied(journal_dst, data_dst, new(cap, torch.uint8), new(cap, torch.uint8),
                new(cap, torch.int64), new(cap, torch.int32), new(cap + 1, torch.int64),
                new(cap, torch.int32), new(cap, torch.int32), new(cap, torch.int32),
                new(n_events + 1, torch.int64), None)
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    p = N.StorageApply()
    p.struct_size = ctypes.sizeof(N.StorageApply)
    p.events, p.events_bytes = events.data_ptr() or spare.data_ptr(), events.numel()
    p.event_offsets = event_offsets.data_ptr() if event_offsets is not None else None
    p.n_events, p.msg_cap = n_events, cap
    p.partition_id, p.lease_id, p.seq = int(partition_id), int(lease_id), int(seq)
    p.journal_pos, p.data_file_pos = int(journal_pos), int(data_file_pos)
    p.journal_dst = journal_dst.data_ptr() or spare.data_ptr()
    p.journal_dst_bytes = journal_dst.numel()
    p.data_dst, p.data_dst_bytes = data_dst.data_ptr() or spare.data_ptr(), data_dst.numel()
    for name, t in zip(("types", "flags", "payload_offsets", "payload_lengths", "record_offsets",
                        "lengths", "expected", "out", "event_first"), u[2:11]):
        setattr(p, name, t.data_ptr() or None)
    o = N.make_opts(device=dev.index if dev.index is not None else -1, stream=stream.cuda_stream,
                    flags=N.BMQCRC_F_DEVICE_PTRS | (0 if sync else N.BMQCRC_F_ASYNC))
    r = N.StorageApplyResult()
    N.check(N.lib.bmqcrc_storage_event_apply(ctypes.byref(p), ctypes.byref(r), ctypes.byref(o)))
    if not sync:
        return u
    n = int(r.n_msgs)
    return Applied(journal_dst[:int(r.journal_bytes)], data_dst[:int(r.data_bytes)],
                   *[t[:n] for t in u[2:6]], u.record_offsets[:n + 1],
                   *[t[:n] for t in u[7:10]], u.event_first, r.as_dict())


Packed = collections.namedtuple("Packed", "events event_offsets types crcs result")

PACK_REFUSALS = ("OK", "RECORD_HEADER", "DATA_OFFSET", "DATA_RECORD", "EVENT_FIRST",
                 "PAYLOAD_TOO_BIG", "EVENT_TOO_BIG", "DST_TOO_SMALL", "TOO_MANY_PIECES")


def pack_storage_events(journal_run, data, *, journal_pos, data_file_pos, partition_id,
                        event_first=None, flags=None, event_type=EVENT_TYPE_STORAGE,
                        storage_protocol_version=STORAGE_PROTOCOL_VERSION,
                        max_event_bytes=None, max_payload_bytes=None, dst=None, stream=None,
                        sync=True):
    """Pack device-resident journal records and the DATA records they name
    into STORAGE events on the GPU (``bmqcrc_storage_event_pack``): the
    device-side form of ``FileStore::replicateRecord`` with
    ``StorageEventBuilder.pack_message``, byte for byte what the builder emits
    -- and the application data's CRC32-C compared with the one the
    MessageRecord stores, at the cost of the copy the primary has to make
    anyway ("verify on send").

    ``journal_run`` is a contiguous uint8 device tensor of 60-byte records (the
    record run, not the journal file with its headers; 4-byte aligned) whose
    record 0 stands for byte ``journal_pos`` of the journal file; ``data`` a
    uint8 window of the DATA file (8-byte aligned) whose byte 0 stands for byte
    ``data_file_pos`` of that file.  A MESSAGE record becomes a DATA message
    with its whole DATA record as payload, CONFIRM, DELETION and JOURNAL_OP
    records messages of their own type, a QUEUE_OP record a QUEUE_OP message
    (PURGE, DELETION) or a QLIST message carrying the journal record only
    (CREATION, ADDITION).  ``event_first`` (int64, one entry more than there
    are events, 0 first and the record count last) cuts the events; None is one
    event.  ``flags`` (uint8 per record, low 5 bits) are the StorageHeader
    flags; None is 0.  ``max_event_bytes`` / ``max_payload_bytes`` None are the
    reference's soft limits.  ``dst=None`` allocates the bound
    ``8 n_events + 72 n + data.numel()``, which is enough when no two MESSAGE
    records share a DATA record; otherwise the call refuses with
    DST_TOO_SMALL and the caller passes a larger ``dst``.  With ``sync=True``
    the events are sliced to ``total_bytes``.  ``sync=False`` requires ``dst``.

    Returns the named tuple ``(events, event_offsets, types, crcs, result)``:
    the event bytes, int64 offsets of the events with the total last, uint8
    message types, int32 computed CRCs (0 for a record that is not a MESSAGE
    record) and the dict of ``last_storage_pack`` (None with ``sync=False``).
    CRC mismatches do not fail the call: ``result["n_bad"]`` /
    ``["first_bad"]`` report them and the bytes go out as they are.  All or
    nothing: a malformed record, a DATA record outside the window, a bad
    ``event_first``, a payload or event above its cap or a destination too
    small (``PACK_REFUSALS``) writes nothing and, with ``sync=True``, raises
    ``BmqCrcError`` (BMQCRC_EINVAL) naming kind and index; with ``sync=False``
    ask ``last_storage_pack``.  Not meant to be captured into a graph."""
    import torch
    for name, t, dt in (("journal_run", journal_run, torch.uint8), ("data", data, torch.uint8),
                        ("event_first", event_first, torch.int64), ("flags", flags, torch.uint8),
                        ("dst", dst, torch.uint8)):
        if name not in ("journal_run", "data") and t is None:
            continue
        if not (isinstance(t, torch.Tensor) and t.dtype == dt and t.is_contiguous()):
            raise TypeError("%s must be a contiguous %s tensor" % (name, dt))
    dev = journal_run.device
    if not journal_run.is_cuda:
        raise TypeError("pack_storage_events takes device tensors only (journal_run is on %s)"
                        % dev)
    for name, t in (("data", data), ("event_first", event_first), ("flags", flags), ("dst", dst)):
        if t is not None and t.device != dev:
            raise TypeError("%s must be on %s like journal_run" % (name, dev))
    if journal_run.numel() % JOURNAL_RECORD_SIZE:
        raise ValueError("journal_run must hold whole 60-byte records")
    n = journal_run.numel() // JOURNAL_RECORD_SIZE
    if event_first is not None and event_first.numel() < 1:
        raise ValueError("event_first needs one entry more than there are events")
    if flags is not None and flags.numel() != n:
        raise ValueError("flags needs one entry per record")
    if not sync and dst is None:
        raise ValueError("dst is required when sync=False")
    n_events = event_first.numel() - 1 if event_first is not None else 1

    def new(shape, dt):
        return torch.empty(shape, dtype=dt, device=dev)
    spare = new(8, torch.uint8)  # (an empty tensor has no address: the call wants one)
    if dst is None:
        dst = new(EVENT_HEADER_SIZE * n_events +
                  (STORAGE_HEADER_SIZE + JOURNAL_RECORD_SIZE) * n + data.numel(), torch.uint8)
    u = Packed(dst, new(n_events + 1, torch.int64), new(n, torch.uint8), new(n, torch.int32), None)
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    p = N.StoragePack()
    p.struct_size = ctypes.sizeof(N.StoragePack)
    p.journal = journal_run.data_ptr() or spare.data_ptr()
    p.journal_bytes, p.n_records, p.journal_pos = journal_run.numel(), n, int(journal_pos)
    p.data, p.data_bytes = data.data_ptr() or spare.data_ptr(), data.numel()
    p.data_file_pos, p.partition_id = int(data_file_pos), int(partition_id)
    p.event_type, p.storage_protocol_version = int(event_type), int(storage_protocol_version)
    p.flags = flags.data_ptr() or None if flags is not None else None
    p.event_first = event_first.data_ptr() if event_first is not None else None
    p.n_events = n_events
    p.max_event_bytes = int(max_event_bytes or 0)
    p.max_payload_bytes = int(max_payload_bytes or 0)
    p.dst, p.dst_bytes = dst.data_ptr() or spare.data_ptr(), dst.numel()
    p.event_offsets = u.event_offsets.data_ptr()
    p.types, p.out = u.types.data_ptr() or None, u.crcs.data_ptr() or None
    o = N.make_opts(device=dev.index if dev.index is not None else -1, stream=stream.cuda_stream,
                    flags=N.BMQCRC_F_DEVICE_PTRS | (0 if sync else N.BMQCRC_F_ASYNC))
    r = N.StoragePackResult()
    N.check(N.lib.bmqcrc_storage_event_pack(ctypes.byref(p), ctypes.byref(r), ctypes.byref(o)))
    if not sync:
        return u
    return Packed(dst[:int(r.total_bytes)], u.event_offsets, u.types, u.crcs, r.as_dict())


def last_storage_pack(device, stream=None):
    """The result of the previous ``pack_storage_events`` on (device, stream)
    (bmqcrc_last_storage_pack), as a dict; waits for it.  ``n_events``,
    ``n_msgs`` (the records), ``n_data`` (DATA messages), ``total_bytes`` (of
    all events), ``n_bad`` and ``first_bad`` (MESSAGE records whose computed
    CRC differs from the stored one, and the lowest; ``n_msgs`` when none),
    ``refused_kind`` (0, ``BMQCRC_STORAGE_PACK_OK``, or the kind, see
    ``PACK_REFUSALS``: then all of the above but ``n_events`` are 0) and
    ``refused_index`` (a record, an ``event_first`` entry or an event, by
    kind).  ``stream=None`` is the device's default stream."""
    r = N.StoragePackResult()
    N.check(N.lib.bmqcrc_last_storage_pack(
        device, stream.cuda_stream if stream is not None else None, ctypes.byref(r)))
    return r.as_dict()


def last_storage_apply(device, stream=None):
    """The result of the previous ``apply_events`` on (device, stream)
    (bmqcrc_last_storage_apply), as a dict; waits for it.  ``n_events``,
    ``n_msgs``, ``n_data`` (DATA messages), ``journal_bytes`` and
    ``data_bytes`` (what was written: 60 n_msgs and the DATA records' bytes),
    ``head_lease_id`` and ``head_seq`` (the last message's primary sequence
    number, the replica's new write head; the one given when there was no
    message), ``n_bad`` and ``first_bad`` (DATA messages whose computed CRC
    differs from the stored one, and the lowest; ``n_msgs`` when none),
    ``refused_kind`` (0, ``BMQCRC_STORAGE_APPLY_OK``, or the kind: then all of
    the above but ``n_events`` are 0), ``refused_event``, ``refused_index``
    (the message) and ``refused_offset`` (a byte of ``events``).
    ``stream=None`` is the device's default stream."""
    r = N.StorageApplyResult()
    N.check(N.lib.bmqcrc_last_storage_apply(
        device, stream.cuda_stream if stream is not None else None, ctypes.byref(r)))
    return r.as_dict()
