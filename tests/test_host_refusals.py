"""The older entry points of the C ABI (batch, verify, blobs, gather,
batch_multi, reserve, fill, host registration): the refusals that answer in
front of the device lookup, with their exact return code and full
bmqcrc_last_error() text.  They hold with or without a GPU."""
import ctypes

import pytest

from blazingmq_amd import _native as N

SEG = b"seg_bytes must be a multiple of 128 in [256, 2^30]"
NULLPTR = b"null pointer argument"
OFFSETS32_ONLY = (b"BMQCRC_F_OFFSETS32 applies to bmqcrc_crc32c_batch and "
                  b"bmqcrc_crc32c_verify only")
NODEV = b"no HIP device available (batch CRC32C runs only on the GPU)"

u8, u32, u64 = ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint64


def _arena():
    return (u8 * 64)(*range(64))


def _answer(rc):
    return rc, N.lib.bmqcrc_last_error()


def _batch(arena, offs, lens, out, n, opts=None):
    return _answer(N.lib.bmqcrc_crc32c_batch(arena, 64 if arena else 0, offs, lens, None, out, n,
                                             opts))


def _verify(offs, lens, exp, n, n_bad, bad_idx, bad_cap, opts=None):
    return _answer(N.lib.bmqcrc_crc32c_verify(_arena(), 64, offs, lens, exp, n, n_bad, bad_idx,
                                              bad_cap, opts))


def test_batch_of_nothing_is_ok():
    assert _batch(None, None, None, None, 0) == (0, b"")


def test_batch_null_offsets():
    lens, out = (u32 * 1)(8), (u32 * 1)()
    assert _batch(_arena(), None, lens, out, 1) == (N.BMQCRC_EINVAL, NULLPTR)


def test_batch_of_2_pow_32_messages_answers_before_reading():
    offs, lens, out = (u64 * 1)(0), (u32 * 1)(8), (u32 * 1)()
    assert _batch(_arena(), offs, lens, out, 1 << 32) == (
        N.BMQCRC_EINVAL, b"at most 2^32-1 messages per batch")


def test_batch_bad_seg_bytes():
    offs, lens, out = (u64 * 1)(0), (u32 * 1)(8), (u32 * 1)()
    o = N.make_opts(seg_bytes=100)
    assert _batch(_arena(), offs, lens, out, 1, ctypes.byref(o)) == (N.BMQCRC_EINVAL, SEG)


def test_verify_needs_n_bad():
    offs, lens, exp = (u64 * 1)(0), (u32 * 1)(8), (u32 * 1)(0)
    assert _verify(offs, lens, exp, 1, None, None, 0) == (N.BMQCRC_EINVAL, b"n_bad is required")


def test_verify_bad_cap_without_bad_idx():
    offs, lens, exp = (u64 * 1)(0), (u32 * 1)(8), (u32 * 1)(0)
    n_bad = u64(7)
    assert _verify(offs, lens, exp, 1, ctypes.byref(n_bad), None, 1) == (N.BMQCRC_EINVAL, NULLPTR)
    assert n_bad.value == 0


def test_verify_zeroes_n_bad_on_every_later_refusal():
    offs, lens, exp = (u64 * 1)(0), (u32 * 1)(8), (u32 * 1)(0)
    idx = (u64 * 1)()
    n_bad = u64(7)
    assert _verify(None, lens, exp, 1, ctypes.byref(n_bad), idx, 1) == (N.BMQCRC_EINVAL, NULLPTR)
    assert n_bad.value == 0
    n_bad.value = 7
    assert _verify(offs, lens, exp, 1 << 32, ctypes.byref(n_bad), idx, 1) == (
        N.BMQCRC_EINVAL, b"at most 2^32-1 messages per batch")
    assert n_bad.value == 0
    n_bad.value = 7
    o = N.make_opts(seg_bytes=100)
    assert _verify(offs, lens, exp, 1, ctypes.byref(n_bad), idx, 1, ctypes.byref(o)) == (
        N.BMQCRC_EINVAL, SEG)
    assert n_bad.value == 0
    n_bad.value = 7
    assert _verify(None, None, None, 0, ctypes.byref(n_bad), None, 0) == (0, b"")
    assert n_bad.value == 0


def _blobs(nbuf, opts=None):
    off, lens, first, out = (u64 * 1)(0), (u32 * 1)(8), (u64 * 2)(0, 1), (u32 * 1)()
    return _answer(N.lib.bmqcrc_crc32c_blobs(_arena(), 64, off, lens, nbuf, first, None, out, 1,
                                             opts))


def test_blobs_of_2_pow_32_buffers():
    assert _blobs(1 << 32) == (N.BMQCRC_EINVAL, b"at most 2^32-1 buffers and blobs per call")


def test_blobs_refuse_offsets32():
    o = N.make_opts(offset_shift=0)
    assert _blobs(1, ctypes.byref(o)) == (N.BMQCRC_EINVAL, OFFSETS32_ONLY)


def _gather(ptrs, lens, first, n):
    bufs = (ctypes.c_void_p * len(ptrs))(*ptrs)
    ln = (u32 * len(lens))(*lens)
    fb = (u64 * len(first))(*first)
    out = (u32 * n)()
    return _answer(N.lib.bmqcrc_crc32c_gather(bufs, ln, len(ptrs), fb, None, out, n, None))


def test_gather_first_buf_must_not_decrease():
    a = _arena()
    assert _gather([ctypes.addressof(a)], [8], [1, 0], 1) == (
        N.BMQCRC_EINVAL, b"msg_first_buf must be non-decreasing and <= nbuf")


def test_gather_null_buffer_with_a_length():
    a = _arena()
    assert _gather([ctypes.addressof(a), None], [4, 4], [0, 2], 1) == (
        N.BMQCRC_EINVAL, b"buffer 1 is NULL with a length")


def test_gather_message_above_2_pow_32_is_refused_before_any_byte_is_read():
    # 16 real bytes behind each pointer: reading 2 GiB from them would fault
    a = (u8 * 16)()
    p = ctypes.addressof(a)
    assert _gather([p, p], [0x80000000, 0x80000000], [0, 2], 1) == (
        N.BMQCRC_EINVAL, b"message 0 is longer than 2^32-1")


def _batch_multi(ndev, seg):
    offs, lens, out = (u64 * 1)(0), (u32 * 1)(8), (u32 * 1)()
    devs = (ctypes.c_int * 1)(0)
    return _answer(N.lib.bmqcrc_crc32c_batch_multi(_arena(), 64, offs, lens, None, out, 1, devs,
                                                   ndev, seg))


def test_batch_multi_without_devices():
    assert _batch_multi(0, 0) == (N.BMQCRC_EINVAL, b"bad arguments")


def test_batch_multi_bad_seg_bytes():
    assert _batch_multi(1, 100) == (N.BMQCRC_EINVAL, SEG)


def test_reserve_bad_seg_bytes():
    assert _answer(N.lib.bmqcrc_reserve(-1, None, 4, 64, 100)) == (N.BMQCRC_EINVAL, SEG)


def test_fill_synthetic_refuses_offsets32():
    o = N.make_opts(offset_shift=0)
    assert _answer(N.lib.bmqcrc_fill_synthetic(None, 0, 1, 0, ctypes.byref(o))) == (
        N.BMQCRC_EINVAL, OFFSETS32_ONLY)


def test_host_register_and_unregister_null_arguments():
    a = _arena()
    dptr = ctypes.c_void_p()
    want = (N.BMQCRC_EINVAL, b"host, bytes and dev_ptr are required")
    assert _answer(N.lib.bmqcrc_host_register(None, 64, -1, ctypes.byref(dptr))) == want
    assert _answer(N.lib.bmqcrc_host_register(a, 0, -1, ctypes.byref(dptr))) == want
    assert _answer(N.lib.bmqcrc_host_register(a, 64, -1, None)) == want
    assert _answer(N.lib.bmqcrc_host_unregister(None)) == (N.BMQCRC_EINVAL, b"null host pointer")


def test_no_device_is_enodev():
    if N.lib.bmqcrc_device_count() != 0:
        pytest.skip("a HIP device is present")
    a = _arena()
    offs, lens, exp, out = (u64 * 2)(0, 8), (u32 * 2)(8, 8), (u32 * 2)(), (u32 * 2)()
    first = (u64 * 2)(0, 2)
    assert _batch(a, offs, lens, out, 2) == (N.BMQCRC_ENODEV, NODEV)
    n_bad = u64(7)
    assert _verify(offs, lens, exp, 2, ctypes.byref(n_bad), None, 0) == (N.BMQCRC_ENODEV, NODEV)
    assert n_bad.value == 0
    assert _answer(N.lib.bmqcrc_crc32c_blobs(a, 64, offs, lens, 2, first, None, out, 1, None)) == (
        N.BMQCRC_ENODEV, NODEV)
    p = ctypes.addressof(a)
    assert _gather([p, p + 8], [8, 8], [0, 2], 1) == (N.BMQCRC_ENODEV, NODEV)
    assert _answer(N.lib.bmqcrc_reserve(-1, None, 4, 64, 0)) == (N.BMQCRC_ENODEV, NODEV)
    assert _batch_multi(1, 0) == (N.BMQCRC_ENODEV, b"no HIP device available")
