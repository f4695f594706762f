"""CONFIRM events: what a consumer sends back, and their way into
``storage.confirm_records``.

Host-side mirror of ``bmqp::ConfirmEventBuilder`` / ``bmqp::ConfirmMessageIterator``
wire format (bmqp_confirmeventbuilder.cpp, bmqp_confirmmessageiterator.cpp,
bmqp_protocol.h):

  EventHeader (bmqp_protocol.h:746, 8 bytes)
      BE u32  F(1b)|Length(31b); u8 PV(2b)|Type(6b)=CONFIRM 3; u8 HeaderWords=2; u8 0; u8 0
  ConfirmHeader (bmqp_protocol.h:2345, 4 bytes)
      u8 HeaderWords(4b)=1|PerMessageWords(4b)=6; 3 reserved bytes
  per message: ConfirmMessage (bmqp_protocol.h:2439, 24 bytes)
      BE i32 QueueId;  GUID[16];  BE i32 SubQueueId

CONFIRM events arrive per client session, and which queue key and app key a
``(queueId, subQueueId)`` pair stands for is that session's state: the walk over
the wire stays on the host.  ``confirm_arrays`` turns events and the sessions'
handles into the arrays ``confirm_records`` takes.  A device walk of CONFIRM
events is not built.
"""
import numpy as np

EVENT_HEADER_SIZE = 8
CONFIRM_HEADER_SIZE = 4
CONFIRM_MESSAGE_SIZE = 24
EVENT_TYPE_CONFIRM = 3
PROTOCOL_VERSION = 1
WORD = 4
MAX_EVENT_SIZE_SOFT = 512 * 1024 * 1024           # EventHeader::k_MAX_SIZE_SOFT
NULL_KEY = bytes(5)


class ConfirmEventBuilder:
    """Build one CONFIRM event.  ``append_message`` is
    ``ConfirmEventBuilder::appendMessage``: it raises ``ValueError``
    ("EVENT_TOO_BIG") once the event holds ``max_message_count()`` messages,
    the most that fit below ``EventHeader::k_MAX_SIZE_SOFT``.  ``blob()``
    returns the event with its EventHeader filled, ``reset()`` starts the next
    one."""

    def __init__(self, max_event_bytes=MAX_EVENT_SIZE_SOFT):
        self.max_event_bytes = max_event_bytes
        self.reset()

    def reset(self):
        self._messages = []

    def max_message_count(self):
        return max(0, self.max_event_bytes - EVENT_HEADER_SIZE - CONFIRM_HEADER_SIZE) // \
            CONFIRM_MESSAGE_SIZE

    def message_count(self):
        return len(self._messages)

    def event_size(self):
        return EVENT_HEADER_SIZE + CONFIRM_HEADER_SIZE + CONFIRM_MESSAGE_SIZE * len(self._messages)

    def append_message(self, queue_id, sub_queue_id, guid):
        guid = bytes(guid)
        if len(guid) != 16:
            raise ValueError("a GUID is 16 bytes")
        if self.message_count() == self.max_message_count():
            raise ValueError("EVENT_TOO_BIG")
        self._messages.append(int(queue_id).to_bytes(4, "big", signed=True) + guid +
                              int(sub_queue_id).to_bytes(4, "big", signed=True))

    def blob(self):
        """The event's bytes (uint8), EventHeader filled."""
        h = bytearray(EVENT_HEADER_SIZE + CONFIRM_HEADER_SIZE)
        h[0:4] = (self.event_size() & 0x7FFFFFFF).to_bytes(4, "big")
        h[4] = (PROTOCOL_VERSION << 6) | EVENT_TYPE_CONFIRM
        h[5] = EVENT_HEADER_SIZE // WORD
        h[8] = ((CONFIRM_HEADER_SIZE // WORD) << 4) | (CONFIRM_MESSAGE_SIZE // WORD)
        return np.frombuffer(bytes(h) + b"".join(self._messages), np.uint8).copy()


class ConfirmMessageIterator:
    """Iterate the messages of one CONFIRM event as
    ``bmqp::ConfirmMessageIterator`` does: the ConfirmHeader's own word counts
    say where the messages start and how far apart they lie, so an event with a
    longer header or longer messages is read by their first 24 bytes.  A
    violation raises ``ValueError``.  Yields dicts ``queue_id``,
    ``sub_queue_id`` and ``guid``."""

    def __init__(self, event):
        self.ev = np.frombuffer(bytes(event), dtype=np.uint8) if not isinstance(
            event, np.ndarray) else event.view(np.uint8)
        if self.ev.size < EVENT_HEADER_SIZE:
            raise ValueError("shorter than an EventHeader")
        length = int.from_bytes(self.ev[0:4].tobytes(), "big") & 0x7FFFFFFF
        if length != self.ev.size or (int(self.ev[4]) & 0x3F) != EVENT_TYPE_CONFIRM:
            raise ValueError("not a CONFIRM event of matching length")
        self.header_size = int(self.ev[5]) * WORD
        if self.header_size < EVENT_HEADER_SIZE or \
                self.header_size + CONFIRM_HEADER_SIZE > self.ev.size:
            raise ValueError("NO_CONFIRM_HEADER")
        b = int(self.ev[self.header_size])
        self.confirm_header_size, self.per_message = (b >> 4) * WORD, (b & 0xF) * WORD
        if self.confirm_header_size < CONFIRM_HEADER_SIZE or \
                self.per_message < CONFIRM_MESSAGE_SIZE:
            raise ValueError("INVALID_CONFIRM_HEADER")
        body = self.ev.size - self.header_size - self.confirm_header_size
        if body < 0 or body % self.per_message:
            raise ValueError("NOT_ENOUGH_BYTES")
        self.count = body // self.per_message

    def __len__(self):
        return self.count

    def __iter__(self):
        pos = self.header_size + self.confirm_header_size
        for _ in range(self.count):
            m = self.ev[pos:pos + CONFIRM_MESSAGE_SIZE].tobytes()
            yield {"queue_id": int.from_bytes(m[0:4], "big", signed=True), "guid": m[4:20],
                   "sub_queue_id": int.from_bytes(m[20:24], "big", signed=True)}
            pos += self.per_message


def confirm_arrays(events, handles):
    """The confirms of ``events`` (CONFIRM events, in order) as the host arrays
    ``confirm_records`` takes on the device: ``(guids, queue_keys, app_keys)``,
    uint8 of 16, 5 and 5 bytes per confirm.  ``handles`` maps the session's
    ``(queue_id, sub_queue_id)`` to ``(queue_key, app_key)``, 5 bytes each
    (``app_key`` None: the null key); one mapping for all events, or one per
    event.  A pair the mapping does not hold raises ``KeyError``: the
    reference's session drops such a confirm with a warning, which is the
    caller's decision here."""
    events = list(events)
    per_event = handles if isinstance(handles, (list, tuple)) else [handles] * len(events)
    if len(per_event) != len(events):
        raise ValueError("one handles mapping per event")
    guids, queue_keys, app_keys = [], [], []
    for event, known in zip(events, per_event):
        for m in ConfirmMessageIterator(event):
            queue_key, app_key = known[(m["queue_id"], m["sub_queue_id"])]
            queue_key, app_key = bytes(queue_key), NULL_KEY if app_key is None else bytes(app_key)
            if len(queue_key) != 5 or len(app_key) != 5:
                raise ValueError("a queue key and an app key are 5 bytes")
            guids.append(m["guid"])
            queue_keys.append(queue_key)
            app_keys.append(app_key)
    return (np.frombuffer(b"".join(guids), np.uint8).copy(),
            np.frombuffer(b"".join(queue_keys), np.uint8).copy(),
            np.frombuffer(b"".join(app_keys), np.uint8).copy())
