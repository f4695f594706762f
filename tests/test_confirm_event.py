"""blazingmq_amd/confirm_event.py: the CONFIRM event's builder and iterator
against the wire layout spelled out byte by byte, the size cap and
``confirm_arrays``.  No GPU."""
import numpy as np
import pytest

from blazingmq_amd import ConfirmEventBuilder, ConfirmMessageIterator, confirm_arrays
from blazingmq_amd import confirm_event as E

G0, G1 = bytes(range(0xA0, 0xB0)), bytes(range(0xB0, 0xC0))
KEY_A, KEY_B, APP = b"\x11\x22\x33\x44\x55", b"\x11\x22\x33\x44\x56", b"\x01\x02\x03\x04\x05"


def test_header_bytes_and_round_trip():
    b = ConfirmEventBuilder()
    assert b.event_size() == 12 and b.message_count() == 0
    b.append_message(7, 0, G0)
    b.append_message(-2, 0x01020304, G1)
    ev = b.blob()
    assert ev.tobytes().hex() == (
        "0000003c" "43" "02" "0000"          # length 60, PV 1 | CONFIRM 3, 2 header words
        "16" "000000"                        # HeaderWords 1 | PerMessageWords 6
        "00000007" + G0.hex() + "00000000"
        "fffffffe" + G1.hex() + "01020304")
    it = ConfirmMessageIterator(ev)
    assert len(it) == 2
    assert list(it) == [{"queue_id": 7, "guid": G0, "sub_queue_id": 0},
                        {"queue_id": -2, "guid": G1, "sub_queue_id": 0x01020304}]
    b.reset()
    assert list(ConfirmMessageIterator(b.blob())) == []


def test_longer_headers_and_messages_are_read_by_their_word_counts():
    ev = bytearray(ConfirmEventBuilder().blob().tobytes())
    ev[8] = (2 << 4) | 7                                        # 8-byte header, 28-byte messages
    ev += bytes(4) + (5).to_bytes(4, "big") + G0 + (9).to_bytes(4, "big") + b"\xEE" * 4
    ev[0:4] = len(ev).to_bytes(4, "big")
    assert list(ConfirmMessageIterator(bytes(ev))) == [
        {"queue_id": 5, "guid": G0, "sub_queue_id": 9}]


@pytest.mark.parametrize("damage, text", [
    (lambda e: e[:6], "shorter"), (lambda e: e[:-1], "matching length"),
    (lambda e: e[:4] + b"\x44" + e[5:], "not a CONFIRM"),
    (lambda e: e[:8] + b"\x06" + e[9:], "INVALID_CONFIRM_HEADER"),
    (lambda e: e[:8] + b"\x15" + e[9:], "INVALID_CONFIRM_HEADER"),
    (lambda e: (len(e) + 4).to_bytes(4, "big") + e[4:] + bytes(4), "NOT_ENOUGH_BYTES")])
def test_the_iterator_refuses(damage, text):
    b = ConfirmEventBuilder()
    b.append_message(1, 0, G0)
    with pytest.raises(ValueError, match=text):
        ConfirmMessageIterator(damage(b.blob().tobytes()))


def test_the_size_cap():
    """ConfirmEventBuilder::maxMessageCount: what fits below the soft cap."""
    assert ConfirmEventBuilder().max_message_count() == (E.MAX_EVENT_SIZE_SOFT - 12) // 24
    b = ConfirmEventBuilder(max_event_bytes=12 + 24 * 3 + 23)
    for i in range(3):
        b.append_message(i, 0, G0)
    with pytest.raises(ValueError, match="EVENT_TOO_BIG"):
        b.append_message(3, 0, G0)
    assert b.message_count() == 3 and b.event_size() == 84 == b.blob().size
    with pytest.raises(ValueError, match="16 bytes"):
        b.append_message(0, 0, G0[:15])


def test_confirm_arrays():
    first, second = ConfirmEventBuilder(), ConfirmEventBuilder()
    first.append_message(1, 0, G0)
    first.append_message(2, 5, G1)
    second.append_message(1, 0, G1)
    handles = {(1, 0): (KEY_A, None), (2, 5): (KEY_B, APP)}
    guids, queue_keys, app_keys = confirm_arrays([first.blob(), second.blob()], handles)
    assert guids.dtype == queue_keys.dtype == app_keys.dtype == np.uint8
    assert guids.tobytes() == G0 + G1 + G1
    assert queue_keys.tobytes() == KEY_A + KEY_B + KEY_A
    assert app_keys.tobytes() == bytes(5) + APP + bytes(5)
    # one mapping per event: another session, another meaning of (1, 0)
    _, queue_keys, _ = confirm_arrays([first.blob(), second.blob()],
                                      [handles, {(1, 0): (KEY_B, None)}])
    assert queue_keys.tobytes() == KEY_A + KEY_B + KEY_B
    with pytest.raises(KeyError):
        confirm_arrays([first.blob()], {(1, 0): (KEY_A, None)})
    with pytest.raises(ValueError, match="5 bytes"):
        confirm_arrays([second.blob()], {(1, 0): (KEY_A[:4], None)})
    empty = confirm_arrays([], handles)
    assert [a.size for a in empty] == [0, 0, 0]
