"""PUSH events: what a consumer receives, and their packing from a
device-resident partition (the delivery side of the path).

Host-side mirror of ``bmqp::PushEventBuilder`` / ``bmqp::PushMessageIterator``
wire format (bmqp_pusheventbuilder.cpp, bmqp_pushmessageiterator.cpp,
bmqp_protocol.h):

  EventHeader (bmqp_protocol.h:746, 8 bytes)
      BE u32  F(1b)|Length(31b); u8 PV(2b)|Type(6b)=PUSH 4; u8 HeaderWords=2; u8 0; u8 0
  per message: PushHeader (bmqp_protocol.h:2008, 32 bytes)
      BE u32  Flags(4b)|MessageWords(28b)
      BE u32  OptionsWords(24b)|CAT(3b)|HeaderWords(5b)=8
      BE i32  QueueId;  GUID[16];  SchemaId(2) Reserved(2)
  then options, each behind an OptionHeader (bmqp_protocol.h:948)
      BE u32  Type(6b)|Packed(1b)|TypeSpecific(4b)|Words(21b)
  the application data (properties + payload, as stored) and 1..4 padding
  bytes each equal to the padding count.

``pack_push_events`` is the device-side form of ``mqba::ClientSession``'s
delivery loop with ``PushEventBuilder::packMessage``
(mqba_clientsession.cpp:1789, bmqp_pusheventbuilder.cpp:66):
``bmqcrc_push_event_pack``, which also checks the CRC the journal stores
against the bytes about to be delivered, a check the reference never makes, at
the cost of the copy the broker has to make anyway.
"""
import collections
import ctypes

import numpy as np

from . import _native as N
from .storage import JOURNAL_RECORD_SIZE

EVENT_HEADER_SIZE = 8
PUSH_HEADER_SIZE = 32
PUSH_MIN_HEADER_SIZE = 8                          # PushHeader::k_MIN_HEADER_SIZE
EVENT_TYPE_PUSH = 4
PROTOCOL_VERSION = 1
WORD = 4
MAX_EVENT_SIZE_SOFT = 512 * 1024 * 1024           # EventHeader::k_MAX_SIZE_SOFT
MAX_PAYLOAD_SIZE_SOFT = 64 * 1024 * 1024          # PushHeader::k_MAX_PAYLOAD_SIZE_SOFT
FLAG_IMPLICIT_PAYLOAD, FLAG_MESSAGE_PROPERTIES, FLAG_OUT_OF_ORDER = 1, 2, 4   # PushHeaderFlags
OPTION_SUB_QUEUE_IDS_OLD, OPTION_MSG_GROUP_ID, OPTION_SUB_QUEUE_INFOS = 1, 2, 3   # OptionType
SUB_QUEUE_INFO_SIZE = 8                           # sizeof(bmqp::SubQueueInfo)
DEFAULT_SUB_QUEUE_ID = 0                          # bmqp::Protocol::k_DEFAULT_SUBSCRIPTION_ID
# bmqcrc_push_pack.option_mode
OPTION_NONE, OPTION_PACKED_RDA, OPTION_SUB_QUEUE_ID, OPTION_SUB_QUEUE_INFO = 0, 1, 2, 3


def _pad_len(n):
    # calcNumWordsAndPadding: numWords = (len + 4) / 4, padding = 4 numWords - len (1..4)
    return ((n + WORD) // WORD) * WORD - n


def _option_header(option_type, words, packed=False, type_specific=0):
    return ((option_type << 26) | (int(packed) << 25) | (type_specific << 21) |
            words).to_bytes(4, "big")


class PushEventBuilder:
    """Build one PUSH event.  Options are added in front of the message they
    belong to, as in the reference: ``add_sub_queue_infos_option`` is
    ``PushEventBuilder::addSubQueueInfosOption`` and emits, by its arguments,
    nothing (no sub-queue), the packed SUB_QUEUE_INFOS header (the default
    sub-queue alone, with its RDA counter), SUB_QUEUE_IDS_OLD (no RDA counter)
    or the unpacked SUB_QUEUE_INFOS.  ``pack_message`` is ``packMessage``: a
    PushHeader with ``headerWords = 8``, the pending options, the application
    data and its padding.  ``blob()`` returns the event with its EventHeader
    filled, ``reset()`` starts the next one."""

    def __init__(self, max_event_bytes=MAX_EVENT_SIZE_SOFT):
        self.max_event_bytes = max_event_bytes
        self.reset()

    def reset(self):
        self._chunks = []     # the event behind its header
        self._size = EVENT_HEADER_SIZE
        self._count = 0
        self._options = b""   # of the message not yet packed

    def event_size(self):
        return self._size + (PUSH_HEADER_SIZE + len(self._options) if self._options else 0)

    def message_count(self):
        return self._count

    def add_sub_queue_infos_option(self, sub_queue_infos, pack_rda_counter=True,
                                   allow_packed=True):
        """``sub_queue_infos``: ``(sub_queue_id, rda)`` pairs, ``rda`` the
        RdaInfo's byte.  ``allow_packed=False`` writes the default sub-queue
        unpacked like any other, which the reference never does and
        ``bmqcrc_push_event_pack``'s mode 3 does for every sub-queue id."""
        infos = [(int(i), int(r)) for i, r in sub_queue_infos]
        if not infos:
            return    # no OptionHeader without option payload
        if not pack_rda_counter:
            option = _option_header(OPTION_SUB_QUEUE_IDS_OLD, 1 + len(infos)) + b"".join(
                i.to_bytes(4, "big") for i, _ in infos)
        elif allow_packed and len(infos) == 1 and infos[0][0] == DEFAULT_SUB_QUEUE_ID:
            option = _option_header(OPTION_SUB_QUEUE_INFOS, infos[0][1], packed=True)
        else:
            option = _option_header(
                OPTION_SUB_QUEUE_INFOS, 1 + len(infos) * SUB_QUEUE_INFO_SIZE // WORD,
                type_specific=SUB_QUEUE_INFO_SIZE // WORD) + b"".join(
                    i.to_bytes(4, "big") + bytes([r, 0, 0, 0]) for i, r in infos)
        self._options += option

    def pack_message(self, app_data, queue_id, guid, flags=0, compression=0,
                     properties=False, schema_id=0):
        """Append one message.  ``properties`` and ``schema_id`` are the
        ``MessagePropertiesInfo`` applied to the header: the
        e_MESSAGE_PROPERTIES flag and the SchemaId."""
        app, guid = bytes(app_data), bytes(guid)
        if len(guid) != 16:
            raise ValueError("a GUID is 16 bytes")
        if len(app) > MAX_PAYLOAD_SIZE_SOFT:
            self._options = b""
            raise ValueError("PAYLOAD_TOO_BIG")
        pad = _pad_len(len(app))
        total = PUSH_HEADER_SIZE + len(self._options) + len(app) + pad
        if self._size + total > self.max_event_bytes:
            self._options = b""
            raise ValueError("EVENT_TOO_BIG")
        header_words, options_words = PUSH_HEADER_SIZE // WORD, len(self._options) // WORD
        f = (flags & 0xF) | (FLAG_MESSAGE_PROPERTIES if properties else 0)
        h = bytearray(PUSH_HEADER_SIZE)
        h[0:4] = ((f << 28) | (total // WORD)).to_bytes(4, "big")
        h[4:8] = ((options_words << 8) | ((compression & 7) << 5) | header_words).to_bytes(4, "big")
        h[8:12] = int(queue_id).to_bytes(4, "big", signed=True)
        h[12:28] = guid
        h[28:30] = int(schema_id).to_bytes(2, "big")
        self._chunks += [bytes(h), self._options, app, bytes([pad]) * pad]
        self._size += total
        self._count += 1
        self._options = b""

    def blob(self):
        """The event's bytes (uint8), EventHeader filled."""
        h = bytearray(EVENT_HEADER_SIZE)
        h[0:4] = (self._size & 0x7FFFFFFF).to_bytes(4, "big")
        h[4] = (PROTOCOL_VERSION << 6) | EVENT_TYPE_PUSH
        h[5] = EVENT_HEADER_SIZE // WORD
        return np.frombuffer(bytes(h) + b"".join(self._chunks), np.uint8).copy()


class PushMessageIterator:
    """Iterate the messages of one PUSH event with
    ``bmqp::PushMessageIterator::next``'s checks in its order; a violation
    raises ``ValueError`` naming the reference's code.  Yields dicts: the
    PushHeader's fields, the option bytes and the sub-queue infos read from
    them as ``(sub_queue_id, rda)`` pairs (``rda`` None where the option
    carries none), the application data's offset in the event, its length and
    its bytes, as stored: properties are not split off and nothing is
    decompressed.

    The reference refuses application data of length 0
    (rc_INVALID_APPLICATION_DATA_SIZE) although its builder packs it;
    ``allow_empty=True`` lets such a message through."""

    def __init__(self, event, allow_empty=False):
        self.ev = np.frombuffer(bytes(event), dtype=np.uint8) if not isinstance(
            event, np.ndarray) else event.view(np.uint8)
        self.allow_empty = allow_empty
        if self.ev.size < EVENT_HEADER_SIZE:
            raise ValueError("shorter than an EventHeader")
        length = int.from_bytes(self.ev[0:4].tobytes(), "big") & 0x7FFFFFFF
        if length != self.ev.size or (int(self.ev[4]) & 0x3F) != EVENT_TYPE_PUSH:
            raise ValueError("not a PUSH event of matching length")
        self.header_size = int(self.ev[5]) * WORD

    @staticmethod
    def _sub_queue_infos(options):
        """OptionsView's reading of the sub-queue options."""
        infos, pos = [], 0
        while pos + WORD <= len(options):
            w = int.from_bytes(options[pos:pos + 4], "big")
            otype, packed, spec, words = w >> 26, (w >> 25) & 1, (w >> 21) & 0xF, w & 0x1FFFFF
            if packed:
                if otype == OPTION_SUB_QUEUE_INFOS:
                    infos.append((DEFAULT_SUB_QUEUE_ID, words))
                pos += WORD
                continue
            if words == 0 or pos + words * WORD > len(options):
                raise ValueError("INVALID_OPTIONS at %d" % pos)
            body = options[pos + WORD:pos + words * WORD]
            if otype == OPTION_SUB_QUEUE_IDS_OLD:
                infos += [(int.from_bytes(body[k:k + 4], "big"), None)
                          for k in range(0, len(body), 4)]
            elif otype == OPTION_SUB_QUEUE_INFOS:
                item = (spec or SUB_QUEUE_INFO_SIZE // WORD) * WORD
                infos += [(int.from_bytes(body[k:k + 4], "big"), body[k + 4])
                          for k in range(0, len(body), item)]
            pos += words * WORD
        return infos

    def __iter__(self):
        pos, ev = self.header_size, self.ev
        while pos < ev.size:
            if pos + PUSH_MIN_HEADER_SIZE > ev.size:
                raise ValueError("NO_PUSH_HEADER at %d" % pos)
            w0 = int.from_bytes(ev[pos:pos + 4].tobytes(), "big")
            w1 = int.from_bytes(ev[pos + 4:pos + 8].tobytes(), "big")
            hs = (w1 & 0x1F) * WORD
            if hs < PUSH_MIN_HEADER_SIZE or pos + hs > ev.size:
                raise ValueError("NO_PUSH_HEADER at %d" % pos)
            size = (w0 & 0x0FFFFFFF) * WORD
            if size == 0:
                raise ValueError("INVALID_MESSAGE_SIZE at %d" % pos)
            if pos + size > ev.size:
                raise ValueError("NOT_ENOUGH_BYTES at %d" % pos)
            opts = (w1 >> 8) * WORD
            if pos + hs + opts > ev.size:
                raise ValueError("INVALID_OPTIONS_OFFSET at %d" % pos)
            flags = w0 >> 28
            head = bytes(ev[pos:pos + hs]) + bytes(max(0, PUSH_HEADER_SIZE - hs))
            options = bytes(ev[pos + hs:pos + hs + opts])
            m = {
                "flags": flags,
                "compression": (w1 >> 5) & 7,
                "queue_id": int.from_bytes(head[8:12], "big", signed=True),
                "guid": head[12:28],
                "schema_id": int.from_bytes(head[28:30], "big"),
                "options": options,
                "sub_queue_infos": self._sub_queue_infos(options),
                "header_offset": pos,
                "app_offset": pos + hs + opts,
                "app_length": 0,
                "payload": b"",
            }
            if not flags & FLAG_IMPLICIT_PAYLOAD:
                last = int(ev[pos + size - 1])
                length = size - hs - opts - last if 1 <= last <= WORD else -1
                if length < 0 or (length == 0 and not self.allow_empty):
                    raise ValueError("INVALID_APPLICATION_DATA_SIZE at %d" % pos)
                m["app_length"] = length
                m["payload"] = bytes(ev[m["app_offset"]:m["app_offset"] + length])
            yield m
            pos += size


PushPacked = collections.namedtuple("PushPacked", "events event_offsets crcs lengths result")

PACK_REFUSALS = ("OK", "RECORD_INDEX", "RECORD", "DATA_OFFSET", "DATA_RECORD", "FLAGS",
                 "EVENT_FIRST", "PAYLOAD_TOO_BIG", "EVENT_TOO_BIG", "DST_TOO_SMALL",
                 "TOO_MANY_PIECES")


def pack_push_events(journal_run, data, *, data_file_pos, queue_ids, records=None, flags=None,
                     option_mode=OPTION_NONE, rda=None, sub_ids=None, event_first=None, dst=None,
                     max_event_bytes=None, max_payload_bytes=None, stream=None, sync=True):
    """Pack stored messages, journal and DATA records both in device memory,
    into PUSH events on the GPU (``bmqcrc_push_event_pack``): the device-side
    form of the delivery loop with ``PushEventBuilder.pack_message``, byte for
    byte what the builder emits -- and the application data's CRC32-C compared
    with the one the MessageRecord stores, at the cost of the copy the broker
    has to make anyway ("verify on delivery").

    ``journal_run`` is a contiguous uint8 device tensor of 60-byte records (the
    record run, 4-byte aligned), ``data`` a uint8 window of the DATA file
    (8-byte aligned) whose byte 0 stands for byte ``data_file_pos`` of that
    file.  Message m is record ``records[m]`` (int32 read as u32; any order,
    repeats allowed: a fan-out to several handles), which must be a MESSAGE
    record; None is every record in turn.  ``queue_ids`` (int32) has one entry
    per message.  ``flags`` (uint8) may carry e_OUT_OF_ORDER (4) only; None is
    0.  ``option_mode`` chooses the one sub-queue option every message gets:
    ``OPTION_NONE``, ``OPTION_PACKED_RDA`` (``rda``, uint8), ``OPTION_SUB_QUEUE_ID``
    (``sub_ids``, int32 read as u32) or ``OPTION_SUB_QUEUE_INFO`` (both); an
    array the mode does not use must be None.  ``event_first`` (int64, one entry
    more than there are events, 0 first and the message count last) cuts the
    events; None is one event.  ``max_event_bytes`` / ``max_payload_bytes`` None
    are the reference's soft limits.  ``dst=None`` makes the size-only call
    first and allocates exactly, which takes a synchronisation and so
    ``sync=True``; ``sync=False`` requires ``dst``.

    Returns the named tuple ``(events, event_offsets, crcs, lengths, result)``:
    the event bytes (sliced to ``total_bytes`` with ``sync=True``), int64
    offsets of the events with the total last, int32 computed CRCs and
    application-data lengths and the dict of ``last_push_pack`` (None with
    ``sync=False``).  CRC mismatches do not fail the call:
    ``result["n_bad"]`` / ``["first_bad"]`` report them and the bytes go out as
    they are.  All or nothing: a record index out of range, a record that is no
    well-formed MESSAGE record, a DATA record outside the window, a flag other
    than 4, a bad ``event_first``, a payload or event above its cap or a
    destination too small (``PACK_REFUSALS``) writes nothing and, with
    ``sync=True``, raises ``BmqCrcError`` (BMQCRC_EINVAL) naming kind and index;
    with ``sync=False`` ask ``last_push_pack``.  Not meant to be captured into
    a graph."""
    import torch
    required = ("journal_run", "data", "queue_ids")
    for name, t, dt in (("journal_run", journal_run, torch.uint8), ("data", data, torch.uint8),
                        ("queue_ids", queue_ids, torch.int32), ("records", records, torch.int32),
                        ("flags", flags, torch.uint8), ("rda", rda, torch.uint8),
                        ("sub_ids", sub_ids, torch.int32),
                        ("event_first", event_first, torch.int64), ("dst", dst, torch.uint8)):
        if name not in required and t is None:
            continue
        if not (isinstance(t, torch.Tensor) and t.dtype == dt and t.is_contiguous()):
            raise TypeError("%s must be a contiguous %s tensor" % (name, dt))
    dev = journal_run.device
    if not journal_run.is_cuda:
        raise TypeError("pack_push_events takes device tensors only (journal_run is on %s)" % dev)
    for name, t in (("data", data), ("queue_ids", queue_ids), ("records", records),
                    ("flags", flags), ("rda", rda), ("sub_ids", sub_ids),
                    ("event_first", event_first), ("dst", dst)):
        if t is not None and t.device != dev:
            raise TypeError("%s must be on %s like journal_run" % (name, dev))
    if journal_run.numel() % JOURNAL_RECORD_SIZE:
        raise ValueError("journal_run must hold whole 60-byte records")
    n_records = journal_run.numel() // JOURNAL_RECORD_SIZE
    n = queue_ids.numel()
    if records is not None and records.numel() != n:
        raise ValueError("records needs one entry per message, like queue_ids")
    if records is None and n != n_records:
        raise ValueError("records=None is every record in turn: queue_ids needs one entry per "
                         "record")
    for name, t in (("flags", flags), ("rda", rda), ("sub_ids", sub_ids)):
        if t is not None and t.numel() != n:
            raise ValueError("%s needs one entry per message" % name)
    if event_first is not None and event_first.numel() < 1:
        raise ValueError("event_first needs one entry more than there are events")
    if not sync and dst is None:
        raise ValueError("dst is required when sync=False")
    n_events = event_first.numel() - 1 if event_first is not None else 1

    def new(shape, dt):
        return torch.empty(shape, dtype=dt, device=dev)
    spare = new(8, torch.uint8)  # (an empty tensor has no address: the call wants one)
    u = PushPacked(dst, new(n_events + 1, torch.int64), new(n, torch.int32), new(n, torch.int32),
                   None)
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    p = N.PushPack()
    p.struct_size = ctypes.sizeof(N.PushPack)
    p.journal = journal_run.data_ptr() or spare.data_ptr()
    p.journal_bytes, p.n_records = journal_run.numel(), n_records
    p.data, p.data_bytes = data.data_ptr() or spare.data_ptr(), data.numel()
    p.data_file_pos, p.n = int(data_file_pos), n
    p.records = (records.data_ptr() or spare.data_ptr()) if records is not None else None
    p.queue_ids = queue_ids.data_ptr() or spare.data_ptr()
    p.flags = flags.data_ptr() or None if flags is not None else None
    p.option_mode = int(option_mode)
    p.rda = (rda.data_ptr() or spare.data_ptr()) if rda is not None else None
    p.sub_ids = (sub_ids.data_ptr() or spare.data_ptr()) if sub_ids is not None else None
    p.event_first = event_first.data_ptr() if event_first is not None else None
    p.n_events = n_events
    p.max_event_bytes = int(max_event_bytes or 0)
    p.max_payload_bytes = int(max_payload_bytes or 0)
    p.event_offsets = u.event_offsets.data_ptr()
    o = N.make_opts(device=dev.index if dev.index is not None else -1, stream=stream.cuda_stream,
                    flags=N.BMQCRC_F_DEVICE_PTRS | (0 if sync else N.BMQCRC_F_ASYNC))
    r = N.PushPackResult()
    if dst is None:
        # size only: the layout kernels are the walk that sizes the destination
        N.check(N.lib.bmqcrc_push_event_pack(ctypes.byref(p), ctypes.byref(r), ctypes.byref(o)))
        dst = new(int(r.total_bytes), torch.uint8)
        if not n:
            return PushPacked(dst, u.event_offsets, u.crcs, u.lengths, r.as_dict())
    p.dst, p.dst_bytes = dst.data_ptr() or spare.data_ptr(), dst.numel()
    p.out, p.lengths = u.crcs.data_ptr() or None, u.lengths.data_ptr() or None
    N.check(N.lib.bmqcrc_push_event_pack(ctypes.byref(p), ctypes.byref(r), ctypes.byref(o)))
    if not sync:
        return PushPacked(dst, *u[1:])
    return PushPacked(dst[:int(r.total_bytes)], u.event_offsets, u.crcs, u.lengths, r.as_dict())


def last_push_pack(device, stream=None):
    """The result of the previous ``pack_push_events`` on (device, stream)
    (bmqcrc_last_push_pack), as a dict; waits for it.  ``n_events``, ``n_msgs``,
    ``total_bytes`` (of all events), ``n_bad`` and ``first_bad`` (messages whose
    computed CRC differs from the stored one, and the lowest; ``n_msgs`` when
    none), ``refused_kind`` (0, ``BMQCRC_PUSH_PACK_OK``, or the kind, see
    ``PACK_REFUSALS``: then all of the above but ``n_events`` are 0) and
    ``refused_index`` (a message, an ``event_first`` entry or an event, by
    kind).  ``stream=None`` is the device's default stream."""
    r = N.PushPackResult()
    N.check(N.lib.bmqcrc_last_push_pack(
        device, stream.cuda_stream if stream is not None else None, ctypes.byref(r)))
    return r.as_dict()
