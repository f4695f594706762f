"""The older entry points of the C ABI on a machine with a GPU: the refusals
that sit behind the device lookup, with their exact return code and full
bmqcrc_last_error() text (every one answers before a kernel is launched), and
one tiny batch through each host-pointer path against bmqcrc_crc32c."""
import ctypes

import pytest

from blazingmq_amd import _native as N
from blazingmq_amd.put_event import PUT_HEADER_SIZE, PutEventBuilder

pytestmark = pytest.mark.gpu

u8, u32, u64 = ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint64
FIRST_BUF = b"msg_first_buf must be non-decreasing and <= nbuf"
ORDINAL = b"device ordinal out of range"


def _outside(i):
    return b"message %d lies outside [arena, arena+arena_bytes)" % i


def _arena():
    return (u8 * 64)(*range(64))


def _answer(rc):
    return rc, N.lib.bmqcrc_last_error()


# message 1 ends 4 bytes past the 64-byte arena, in both offset forms
RANGES = [((u64 * 2)(0, 60), None), ((u32 * 2)(0, 15), 2)]


@pytest.mark.parametrize("offs,shift", RANGES, ids=["offsets64", "offsets32_shift2"])
def test_batch_message_outside_the_arena(cuda, offs, shift):
    lens, out = (u32 * 2)(8, 8), (u32 * 2)()
    o = N.make_opts(offset_shift=shift)
    assert _answer(N.lib.bmqcrc_crc32c_batch(_arena(), 64, offs, lens, None, out, 2,
                                             ctypes.byref(o))) == (N.BMQCRC_EINVAL, _outside(1))


@pytest.mark.parametrize("offs,shift", RANGES, ids=["offsets64", "offsets32_shift2"])
def test_verify_message_outside_the_arena(cuda, offs, shift):
    lens, exp, n_bad = (u32 * 2)(8, 8), (u32 * 2)(), u64(7)
    o = N.make_opts(offset_shift=shift)
    assert _answer(N.lib.bmqcrc_crc32c_verify(_arena(), 64, offs, lens, exp, 2,
                                              ctypes.byref(n_bad), None, 0, ctypes.byref(o))) == (
        N.BMQCRC_EINVAL, _outside(1))
    assert n_bad.value == 0


def test_blobs_buffer_outside_the_arena(cuda):
    offs, lens, first, out = (u64 * 2)(0, 60), (u32 * 2)(8, 8), (u64 * 2)(0, 2), (u32 * 1)()
    assert _answer(N.lib.bmqcrc_crc32c_blobs(_arena(), 64, offs, lens, 2, first, None, out, 1,
                                             None)) == (N.BMQCRC_EINVAL, _outside(1))


def test_blobs_first_buf_must_not_decrease(cuda):
    offs, lens, first, out = (u64 * 2)(0, 8), (u32 * 2)(8, 8), (u64 * 3)(0, 2, 1), (u32 * 2)()
    assert _answer(N.lib.bmqcrc_crc32c_blobs(_arena(), 64, offs, lens, 2, first, None, out, 2,
                                             None)) == (N.BMQCRC_EINVAL, FIRST_BUF)


def test_batch_device_ordinal_out_of_range(cuda):
    offs, lens, out = (u64 * 1)(0), (u32 * 1)(8), (u32 * 1)()
    o = N.make_opts(device=N.lib.bmqcrc_device_count())
    assert _answer(N.lib.bmqcrc_crc32c_batch(_arena(), 64, offs, lens, None, out, 1,
                                             ctypes.byref(o))) == (N.BMQCRC_EINVAL, ORDINAL)


def test_batch_multi_device_ordinal_out_of_range(cuda):
    offs, lens, out = (u64 * 1)(0), (u32 * 1)(8), (u32 * 1)()
    devs = (ctypes.c_int * 1)(N.lib.bmqcrc_device_count())
    assert _answer(N.lib.bmqcrc_crc32c_batch_multi(_arena(), 64, offs, lens, None, out, 1, devs,
                                                   1, 0)) == (N.BMQCRC_EINVAL, ORDINAL)


def test_verify_over_65_device_listings(cuda):
    offs, lens, exp, n_bad = (u64 * 1)(0), (u32 * 1)(8), (u32 * 1)(), u64(7)
    o = N.make_opts(devices=[0] * 65)
    assert _answer(N.lib.bmqcrc_crc32c_verify(_arena(), 64, offs, lens, exp, 1,
                                              ctypes.byref(n_bad), None, 0, ctypes.byref(o))) == (
        N.BMQCRC_EINVAL, b"at most 64 device listings")
    assert n_bad.value == 0


def test_batch_multi_message_outside_the_arena(cuda):
    offs, lens, out = (u64 * 2)(0, 60), (u32 * 2)(8, 8), (u32 * 2)()
    devs = (ctypes.c_int * 1)(0)
    assert _answer(N.lib.bmqcrc_crc32c_batch_multi(_arena(), 64, offs, lens, None, out, 2, devs,
                                                   1, 0)) == (
        N.BMQCRC_EINVAL, b"message outside arena")


def test_gather_refuses_async(cuda):
    a = _arena()
    bufs, lens, first, out = (ctypes.c_void_p * 1)(ctypes.addressof(a)), (u32 * 1)(8), \
        (u64 * 2)(0, 1), (u32 * 1)()
    o = N.make_opts(flags=N.BMQCRC_F_ASYNC)
    assert _answer(N.lib.bmqcrc_crc32c_gather(bufs, lens, 1, first, None, out, 1,
                                              ctypes.byref(o))) == (
        N.BMQCRC_EINVAL, b"gather takes host buffers, synchronously")


# Three messages of a 64-byte arena: empty, one byte, the whole arena (the
# edge shapes of the host-pointer paths' staging).
MSGS = [(0, 0), (5, 1), (0, 64)]


@pytest.fixture(scope="module")
def want():
    a = _arena()
    base = ctypes.addressof(a)
    return [N.lib.bmqcrc_crc32c(base + off, ln, 0) for off, ln in MSGS]


def test_host_batch_matches_the_cpu(cuda, want):
    offs, lens, out = (u64 * 3)(*[m[0] for m in MSGS]), (u32 * 3)(*[m[1] for m in MSGS]), (u32 * 3)()
    assert _answer(N.lib.bmqcrc_crc32c_batch(_arena(), 64, offs, lens, None, out, 3, None)) == (
        0, b"")
    assert list(out) == want


def test_gather_matches_the_cpu(cuda, want):
    a = _arena()
    base = ctypes.addressof(a)
    # message 0 has no buffer, messages 1 and 2 one each
    bufs = (ctypes.c_void_p * 2)(base + 5, base)
    lens, first, out = (u32 * 2)(1, 64), (u64 * 4)(0, 0, 1, 2), (u32 * 3)()
    assert _answer(N.lib.bmqcrc_crc32c_gather(bufs, lens, 2, first, None, out, 3, None)) == (
        0, b"")
    assert list(out) == want


def test_batch_multi_on_one_device_matches_the_cpu(cuda, want):
    offs, lens, out = (u64 * 3)(*[m[0] for m in MSGS]), (u32 * 3)(*[m[1] for m in MSGS]), (u32 * 3)()
    devs = (ctypes.c_int * 1)(0)
    assert _answer(N.lib.bmqcrc_crc32c_batch_multi(_arena(), 64, offs, lens, None, out, 3, devs,
                                                   1, 0)) == (0, b"")
    assert list(out) == want


def test_overlapped_compute_matches_the_cpu(cuda, want):
    # PutEventBuilder(defer_crc=True) fills the CRCs through the overlapped
    # compute path (bmqcrc_put_event_fill_crcs); defer_crc=False takes each
    # from bmqcrc_crc32c
    a = bytes(_arena())
    events = []
    for defer in (True, False):
        b = PutEventBuilder(defer_crc=defer)
        for i, (off, ln) in enumerate(MSGS):
            b.pack_message(a[off:off + ln], queue_id=i)
        events.append(b.finalize())
    assert bytes(events[0]) == bytes(events[1])
    # the last message: its PutHeader with the CRC in bytes 28..31, 64 bytes, 4 of padding
    crc_at = len(events[0]) - (64 + 4) - PUT_HEADER_SIZE + 28
    assert int.from_bytes(bytes(events[0][crc_at:crc_at + 4]), "big") == want[2]
