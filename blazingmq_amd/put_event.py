"""PUT events with a deferred, batched CRC32C (the producer side of the path).

Host-side mirror of ``bmqp::PutEventBuilder`` / ``bmqp::PutMessageIterator``
wire format (/root/reference/src/groups/bmq/bmqp/bmqp_puteventbuilder.cpp,
bmqp_protocol.h):

  EventHeader (bmqp_protocol.h:746, 8 bytes)
      BE u32  F(1b)|Length(31b); u8 PV(2b)|Type(6b); u8 HeaderWords=2; u8 typeSpecific; u8 0
  per message: PutHeader (bmqp_protocol.h:1374, 36 bytes)
      BE u32  Flags(4b)|MessageWords(28b)
      BE u32  OptionsWords(24b)|CAT(3b)|HeaderWords(5b)=9
      BE i32  QueueId;  GUID[16];  BE u32 CRC32-C (@28);  SchemaId(2) Reserved(2)
  then options, application data (properties + payload) and 1..4 padding
  bytes each equal to the padding count (ProtocolUtil::calcNumWordsAndPadding,
  bmqp_protocolutil.h:312; k_PADDING_DATA bmqp_protocolutil.cpp:44).

The reference computes ``Crc32c::calculate(appData)`` once per message inside
``packMessage`` (bmqp_puteventbuilder.cpp:302,320,400,413) and writes it into
``PutHeader::d_crc32c`` (:146-153).  ``PutEventBuilder(defer_crc=True)`` packs
every message with the CRC field pending and ``finalize()`` fills all of them
with one batched GPU call before the event is posted
(``bmqcrc_put_event_fill_crcs``: a native walk of the event, then one batch).
``PutMessageIterator.verify_crcs()`` is the batched form of the iterator's
recompute (bmqp_putmessageiterator.cpp:670-679): ``bmqcrc_put_event_verify``.
"""
import collections
import ctypes

import numpy as np

from . import _native as N
from .crc32c import Crc32c

EVENT_HEADER_SIZE = 8
PUT_HEADER_SIZE = 36
EVENT_TYPE_PUT = 2
PROTOCOL_VERSION = 1
WORD = 4


def _pad_len(n):
    # calcNumWordsAndPadding: numWords = (len + 4) / 4, padding = 4*numWords - len (1..4)
    return ((n + WORD) // WORD) * WORD - n


class PutEventBuilder:
    """Build one PUT event.  ``pack_message`` appends a message; with
    ``defer_crc=False`` the CRC is computed immediately on the CPU (like the
    reference), with ``defer_crc=True`` ``finalize()`` computes all CRCs in one
    batch on the GPU."""

    def __init__(self, defer_crc=True, devices=None):
        self.defer_crc = defer_crc
        self.devices = devices  # several ordinals: spread the deferred fill over them
        self._chunks = [bytes(EVENT_HEADER_SIZE)]
        self._size = EVENT_HEADER_SIZE
        self._app_off = []   # offset of app data inside the event
        self._app_len = []
        self._crc_pos = []   # offset of the PutHeader CRC field
        self._finalized = False

    def pack_message(self, app_data, queue_id=0, guid=None, flags=0, options=b""):
        """Append one message: ``app_data`` = properties + payload (bytes)."""
        if self._finalized:
            raise RuntimeError("event already finalized")
        app = bytes(app_data)
        if len(options) % WORD:
            raise ValueError("options must be word aligned")
        pad = _pad_len(len(app))
        header_words = PUT_HEADER_SIZE // WORD
        options_words = len(options) // WORD
        msg_words = header_words + options_words + (len(app) + pad) // WORD
        h = bytearray(PUT_HEADER_SIZE)
        h[0:4] = (((flags & 0xF) << 28) | msg_words).to_bytes(4, "big")
        h[4:8] = ((options_words << 8) | header_words).to_bytes(4, "big")
        h[8:12] = int(queue_id).to_bytes(4, "big", signed=True)
        h[12:28] = bytes(guid) if guid is not None else bytes(16)
        crc = 0 if self.defer_crc else Crc32c.calculate(app)
        h[28:32] = crc.to_bytes(4, "big")
        self._crc_pos.append(self._size + 28)
        self._app_off.append(self._size + PUT_HEADER_SIZE + len(options))
        self._app_len.append(len(app))
        self._chunks += [bytes(h), bytes(options), app, bytes([pad]) * pad]
        self._size += PUT_HEADER_SIZE + len(options) + len(app) + pad
        return len(self._app_off) - 1

    def message_count(self):
        return len(self._app_off)

    def finalize(self):
        """Return the event bytes (EventHeader filled; pending CRCs computed
        in one GPU batch when ``defer_crc``)."""
        ev = np.frombuffer(b"".join(self._chunks), dtype=np.uint8).copy()
        ev[0:4] = np.frombuffer((self._size & 0x7FFFFFFF).to_bytes(4, "big"), np.uint8)
        ev[4] = (PROTOCOL_VERSION << 6) | EVENT_TYPE_PUT
        ev[5] = EVENT_HEADER_SIZE // WORD
        if self.defer_crc and self._app_off:
            opts = N.make_opts(devices=self.devices)
            n = N.check_count(N.lib.bmqcrc_put_event_fill_crcs(
                ctypes.c_void_p(ev.ctypes.data), ev.size, ctypes.byref(opts)))
            if n != len(self._app_off):
                raise RuntimeError("PUT event walk found %d messages, packed %d"
                                   % (n, len(self._app_off)))
        self._finalized = True
        return ev


def pack_events(src, src_offsets, lengths, queue_ids, guids, flags=None, event_first=None,
                max_event_bytes=None, dst=None, out=None, *, stream=None, sync=True):
    """Pack device-resident payloads into PUT events on the GPU
    (``bmqcrc_put_event_pack``): what ``PutEventBuilder(defer_crc=False)``
    emits with no options, one builder per event, the events back to back in
    ``dst``.  Message i's application data is ``src[src_offsets[i]:][:lengths[i]]``.

    Device tensors only, all on one MI355X, contiguous: ``src`` / ``dst``
    uint8, ``src_offsets`` int64, ``lengths`` / ``queue_ids`` / ``out`` int32
    (lengths and out read as u32), ``guids`` uint8 with 16 bytes per message,
    ``flags`` uint8 (low 4 bits) or None, ``event_first`` int64 with one entry
    more than there are events (event e holds messages ``[event_first[e],
    event_first[e+1])``) or None for one event.  ``max_event_bytes=None`` is
    the reference's 66 MiB.  ``dst=None`` allocates exactly the bytes needed,
    which takes a sum of the lengths on the host and so ``sync=True``; with
    ``sync=False`` ``dst`` is required.

    Returns ``(dst, event_offsets, crcs)``: ``event_offsets`` (int64, one per
    event and the total last) and ``crcs`` (``out``, or a new int32 tensor).
    All or nothing: a source range outside ``src``, a malformed
    ``event_first``, an event above the cap or a ``dst`` too small writes
    nothing and, with ``sync=True``, raises ``BmqCrcError`` (BMQCRC_EINVAL)
    naming the kind and the lowest index; with ``sync=False`` ask
    ``last_put_pack``.  Not meant to be captured into a graph."""
    import torch
    n = src_offsets.numel() if isinstance(src_offsets, torch.Tensor) else -1
    for name, t, dt in (("src", src, torch.uint8), ("src_offsets", src_offsets, torch.int64),
                        ("lengths", lengths, torch.int32), ("queue_ids", queue_ids, torch.int32),
                        ("guids", guids, torch.uint8)):
        if not (isinstance(t, torch.Tensor) and t.dtype == dt and t.is_contiguous()):
            raise TypeError("%s must be a contiguous %s tensor" % (name, dt))
    if lengths.numel() != n or queue_ids.numel() != n or guids.numel() != 16 * n:
        raise ValueError("src_offsets/lengths/queue_ids/guids size mismatch")
    dev = src.device
    for name, t, dt, want in (("flags", flags, torch.uint8, n), ("out", out, torch.int32, n)):
        if t is not None and not (isinstance(t, torch.Tensor) and t.device == dev and
                                  t.dtype == dt and t.is_contiguous() and t.numel() == want):
            raise TypeError("%s must be a contiguous %s tensor of %d elements on %s"
                            % (name, dt, want, dev))
    for name, t, dt in (("event_first", event_first, torch.int64), ("dst", dst, torch.uint8)):
        if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == dt and
                                  t.is_contiguous()):
            raise TypeError("%s must be a contiguous %s tensor" % (name, dt))
    if event_first is not None and event_first.numel() < 1:
        raise ValueError("event_first needs one entry more than there are events")
    if not src.is_cuda:
        raise TypeError("pack_events takes device tensors only (src is on %s)" % dev)
    for name, t in (("src_offsets", src_offsets), ("lengths", lengths), ("queue_ids", queue_ids),
                    ("guids", guids), ("event_first", event_first), ("dst", dst)):
        if t is not None and t.device != dev:
            raise TypeError("%s must be on %s like src" % (name, dev))
    n_events = event_first.numel() - 1 if event_first is not None else 1
    if dst is None:
        if not sync:
            raise ValueError("dst is required when sync=False: sizing it reads the lengths back")
        words = ((lengths.to(torch.int64) & 0xFFFFFFFF) >> 2) + 1
        total = int((4 * words + PUT_HEADER_SIZE).sum().item()) if n else 0
        dst = torch.empty(total + (EVENT_HEADER_SIZE * n_events if n else 0), dtype=torch.uint8,
                          device=dev)
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=dev)
    event_offsets = torch.zeros(n_events + 1, dtype=torch.int64, device=dev)
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    p = N.PutPack()
    p.struct_size = ctypes.sizeof(N.PutPack)
    p.src, p.src_bytes = src.data_ptr(), src.numel()
    p.src_offsets, p.lengths = src_offsets.data_ptr(), lengths.data_ptr()
    p.queue_ids, p.guids = queue_ids.data_ptr(), guids.data_ptr()
    p.flags = flags.data_ptr() if flags is not None else None
    p.event_first = event_first.data_ptr() if event_first is not None else None
    p.n, p.n_events = n, n_events
    p.max_event_bytes = int(max_event_bytes) if max_event_bytes is not None else 0
    p.dst, p.dst_bytes = dst.data_ptr(), dst.numel()
    p.event_offsets, p.out = event_offsets.data_ptr(), out.data_ptr()
    o = N.make_opts(device=dev.index if dev.index is not None else -1, stream=stream.cuda_stream,
                    flags=N.BMQCRC_F_DEVICE_PTRS | (0 if sync else N.BMQCRC_F_ASYNC))
    N.check(N.lib.bmqcrc_put_event_pack(ctypes.byref(p), None, ctypes.byref(o)))
    return dst, event_offsets, out


def last_put_pack(device, stream=None):
    """(n_msgs, n_events, total_bytes, refused_kind, refused_index) of the
    previous ``pack_events`` on (device, stream) (bmqcrc_last_put_pack); waits
    for it.  ``refused_kind`` is 0 (``BMQCRC_PUT_PACK_OK``) or the kind
    refused, ``refused_index`` the lowest offending message or event, and
    ``total_bytes`` 0 when refused.  ``stream=None`` is the device's default
    stream."""
    n, ne, tot, idx = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    kind = ctypes.c_uint32()
    N.check(N.lib.bmqcrc_last_put_pack(
        device, stream.cuda_stream if stream is not None else None, ctypes.byref(n),
        ctypes.byref(ne), ctypes.byref(tot), ctypes.byref(kind), ctypes.byref(idx)))
    return n.value, ne.value, tot.value, kind.value, idx.value


Unpacked = collections.namedtuple(
    "Unpacked", "app_offsets lengths queue_ids guids flags expected crcs event_first")


def unpack_events(events, event_offsets=None, msg_cap=None, verify=True, *, stream=None,
                  sync=True):
    """Walk device-resident PUT events on the GPU (``bmqcrc_put_event_unpack``),
    the inverse of ``pack_events``: what ``PutMessageIterator`` reports for
    every message of every event, as device tensors, with no payload byte and
    no descriptor crossing PCIe.

    ``events`` is a contiguous uint8 device tensor (4-byte aligned),
    ``event_offsets`` int64 with one entry more than there are events (event e
    is ``events[event_offsets[e]:event_offsets[e+1]]``) or None for one event,
    the whole buffer.  ``msg_cap`` is the capacity of the per-message arrays;
    None is ``events.numel() // 40``, the most a buffer can hold.  With
    ``verify`` every message's application data is CRC'd and compared with its
    PutHeader CRC (ask ``last_put_unpack`` for n_bad / first_bad); the CRC
    pass runs over all ``msg_cap`` slots, so a tight ``msg_cap`` is cheaper.

    Returns the named tuple ``(app_offsets, lengths, queue_ids, guids, flags,
    expected, crcs, event_first)``: int64 offsets in ``events`` of the
    application data, int32 lengths and queue ids, uint8 GUIDs (16 per
    message) and PutHeader flags, the PutHeader CRCs and the computed ones
    (int32; ``crcs`` is None when ``verify=False``), and the first message of
    each event with the message count last (int64).  With ``sync=True`` the
    per-message tensors are sliced to the messages found, and a malformed
    event, bad ``event_offsets`` or more than ``msg_cap`` messages raises
    ``BmqCrcError`` (BMQCRC_EINVAL) naming kind, event and offset: nothing is
    written then.  With ``sync=False`` the tensors keep their full capacity
    and ``last_put_unpack`` reports the outcome.  Not meant to be captured
    into a graph."""
    import torch
    for name, t, dt in (("events", events, torch.uint8),
                        ("event_offsets", event_offsets, torch.int64)):
        if name == "event_offsets" and t is None:
            continue
        if not (isinstance(t, torch.Tensor) and t.dtype == dt and t.is_contiguous()):
            raise TypeError("%s must be a contiguous %s tensor" % (name, dt))
    dev = events.device
    if not events.is_cuda:
        raise TypeError("unpack_events takes device tensors only (events is on %s)" % dev)
    if event_offsets is not None and event_offsets.device != dev:
        raise TypeError("event_offsets must be on %s like events" % dev)
    if event_offsets is not None and event_offsets.numel() < 1:
        raise ValueError("event_offsets needs one entry more than there are events")
    n_events = event_offsets.numel() - 1 if event_offsets is not None else 1
    cap = events.numel() // (PUT_HEADER_SIZE + WORD) if msg_cap is None else int(msg_cap)
    if cap < 0:
        raise ValueError("msg_cap must not be negative")

    def new(shape, dt):
        return torch.empty(shape, dtype=dt, device=dev)
    u = Unpacked(new(cap, torch.int64), new(cap, torch.int32), new(cap, torch.int32),
                 new((cap, 16), torch.uint8), new(cap, torch.uint8), new(cap, torch.int32),
                 new(cap, torch.int32) if verify else None, new(n_events + 1, torch.int64))
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    p = N.PutUnpack()
    p.struct_size = ctypes.sizeof(N.PutUnpack)
    p.events, p.events_bytes = events.data_ptr(), events.numel()
    p.event_offsets = event_offsets.data_ptr() if event_offsets is not None else None
    p.n_events, p.msg_cap = n_events, cap
    # (an empty tensor has no address: the call wants one for the required arrays)
    p.app_offsets = u.app_offsets.data_ptr() or u.event_first.data_ptr()
    p.lengths = u.lengths.data_ptr() or u.event_first.data_ptr()
    p.queue_ids, p.guids, p.flags = u.queue_ids.data_ptr(), u.guids.data_ptr(), u.flags.data_ptr()
    p.expected = u.expected.data_ptr()
    p.out = u.crcs.data_ptr() if verify else None
    p.event_first = u.event_first.data_ptr()
    o = N.make_opts(device=dev.index if dev.index is not None else -1, stream=stream.cuda_stream,
                    flags=N.BMQCRC_F_DEVICE_PTRS | (0 if sync else N.BMQCRC_F_ASYNC))
    r = N.PutUnpackResult()
    N.check(N.lib.bmqcrc_put_event_unpack(ctypes.byref(p), ctypes.byref(r), ctypes.byref(o)))
    if not sync:
        return u
    n = int(r.n_msgs)
    return Unpacked(*[t[:n] if t is not None else None for t in u[:7]], u.event_first)


def last_put_unpack(device, stream=None):
    """The result of the previous ``unpack_events`` on (device, stream)
    (bmqcrc_last_put_unpack), as a dict; waits for it.  ``n_events``,
    ``n_msgs`` (0 when refused), ``n_bad`` and ``first_bad`` (messages whose
    computed CRC differs from the PutHeader's, and the lowest; ``n_msgs`` when
    none), ``refused_kind`` (0, ``BMQCRC_PUT_UNPACK_OK``, or the kind),
    ``refused_event`` and ``refused_offset`` (the byte in ``events`` the host
    walk would name).  ``stream=None`` is the device's default stream."""
    r = N.PutUnpackResult()
    N.check(N.lib.bmqcrc_last_put_unpack(
        device, stream.cuda_stream if stream is not None else None, ctypes.byref(r)))
    return r.as_dict()


class PutMessageIterator:
    """Iterate the messages of a PUT event: (put header fields, app data)."""

    def __init__(self, event):
        self.ev = np.frombuffer(bytes(event), dtype=np.uint8) if not isinstance(
            event, np.ndarray) else event.view(np.uint8)
        length = int.from_bytes(self.ev[0:4].tobytes(), "big") & 0x7FFFFFFF
        if length != self.ev.size or (int(self.ev[4]) & 0x3F) != EVENT_TYPE_PUT:
            raise ValueError("not a PUT event of matching length")
        self.header_size = int(self.ev[5]) * WORD

    def scan(self):
        """Native walk (``bmqcrc_put_event_scan``, CPU only): numpy arrays
        (app_offset, app_length, crc_pos) of every message."""
        ev = np.ascontiguousarray(self.ev)
        p = ctypes.c_void_p(ev.ctypes.data)
        n = N.check_count(N.lib.bmqcrc_put_event_scan(p, ev.size, None, None, None, 0))
        off, ln, pos = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint64)
        if n:
            N.check_count(N.lib.bmqcrc_put_event_scan(
                p, ev.size, ctypes.c_void_p(off.ctypes.data), ctypes.c_void_p(ln.ctypes.data),
                ctypes.c_void_p(pos.ctypes.data), n))
        return off, ln, pos

    def verify_crcs(self, bad_cap=1 << 16, device=-1, devices=None):
        """Check every PutHeader CRC against its application data in one GPU
        batch (``devices``: spread over several devices, bmqcrc_opts.ndevices).
        Returns (n_messages, n_bad, bad message indices)."""
        ev = np.ascontiguousarray(self.ev)
        n_msgs, n_bad = ctypes.c_uint64(0), ctypes.c_uint64(0)
        bad = np.zeros(max(int(bad_cap), 1), np.uint64)
        opts = N.make_opts(device=device, devices=devices)
        N.check(N.lib.bmqcrc_put_event_verify(
            ctypes.c_void_p(ev.ctypes.data), ev.size, ctypes.byref(n_msgs), ctypes.byref(n_bad),
            ctypes.c_void_p(bad.ctypes.data), int(bad_cap), ctypes.byref(opts)))
        k = min(int(n_bad.value), int(bad_cap))
        return int(n_msgs.value), int(n_bad.value), bad[:k].copy()

    def __iter__(self):
        pos = self.header_size
        ev = self.ev
        while pos < ev.size:
            w0 = int.from_bytes(ev[pos:pos + 4].tobytes(), "big")
            w1 = int.from_bytes(ev[pos + 4:pos + 8].tobytes(), "big")
            msg_bytes = (w0 & 0x0FFFFFFF) * WORD
            hw = (w1 & 0x1F) * WORD
            opt = (w1 >> 8) * WORD
            end = pos + msg_bytes
            pad = int(ev[end - 1])
            app = ev[pos + hw + opt:end - pad].tobytes()
            yield {
                "flags": w0 >> 28,
                "queue_id": int.from_bytes(ev[pos + 8:pos + 12].tobytes(), "big", signed=True),
                "guid": ev[pos + 12:pos + 28].tobytes(),
                "crc32c": int.from_bytes(ev[pos + 28:pos + 32].tobytes(), "big"),
                "app_data": app,
                "app_offset": pos + hw + opt,
            }
            pos = end
