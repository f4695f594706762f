"""ABI 2.8: BMQCRC_F_OFFSETS32 and bmqcrc_opts.offset_shift, as far as they
answer without a GPU -- the struct's layout, the argument checks that sit in
front of the device lookup, and the Python wrappers' refusals."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from blazingmq_amd import Crc32c, _native as N, calculate_batch_ptr
from blazingmq_amd.crc32c import verify_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

UNKNOWN = b"unknown bmqcrc_opts.flags bits"


def _batch(opts, n=1):
    """bmqcrc_crc32c_batch over a 64-byte host arena with 32-bit offsets."""
    payload = (ctypes.c_uint8 * 64)(*range(64))
    offs = (ctypes.c_uint32 * n)(*([0] * n))
    lens = (ctypes.c_uint32 * n)(*([8] * n))
    out = (ctypes.c_uint32 * n)()
    rc = N.lib.bmqcrc_crc32c_batch(payload, 64, offs, lens, None, out, n, opts)
    return rc, N.lib.bmqcrc_last_error(), list(out), N.lib.bmqcrc_crc32c(payload, 8, 0)


def test_version_is_2_8():
    v = N.lib.bmqcrc_version()
    assert v >> 16 == 2 and v & 0xffff >= 8


def test_opts_layout_matches_the_header(tmp_path):
    src = tmp_path / "opts.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bmqcrc.h"\n'
                   'int main(void) { printf("%zu %zu %zu %u\\n", sizeof(bmqcrc_opts), '
                   'offsetof(bmqcrc_opts, min_len), offsetof(bmqcrc_opts, offset_shift), '
                   'BMQCRC_F_OFFSETS32); return 0; }\n')
    exe = tmp_path / "opts"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert got == [ctypes.sizeof(N.Opts), N.Opts.min_len.offset, N.Opts.offset_shift.offset,
                   N.BMQCRC_F_OFFSETS32]
    assert N.BMQCRC_F_OFFSETS32 == 0x20
    assert N.Opts.offset_shift.offset == N.Opts.min_len.offset + 4  # appended


def test_shift_above_7_is_einval():
    o = N.make_opts(offset_shift=0)
    o.offset_shift = 8
    rc, err, _, _ = _batch(ctypes.byref(o))
    assert rc == N.BMQCRC_EINVAL and b"offset_shift" in err, (rc, err)


def test_shift_without_the_flag_is_einval():
    o = N.make_opts()
    o.offset_shift = 1
    rc, err, _, _ = _batch(ctypes.byref(o))
    assert rc == N.BMQCRC_EINVAL and b"offset_shift" in err, (rc, err)


@pytest.mark.parametrize("shift", [0, 7])
def test_the_flag_is_known(shift):
    # ENODEV without a GPU, the CRC with one: never "unknown flags"
    rc, err, out, want = _batch(ctypes.byref(N.make_opts(offset_shift=shift)))
    assert rc in (0, N.BMQCRC_ENODEV), (rc, err)
    assert UNKNOWN not in err
    if rc == 0:
        assert out == [want]


def test_verify_takes_the_flag_and_checks_the_shift():
    payload = (ctypes.c_uint8 * 64)(*range(64))
    offs, lens, exp = (ctypes.c_uint32 * 1)(0), (ctypes.c_uint32 * 1)(8), (ctypes.c_uint32 * 1)(0)
    nbad = ctypes.c_uint64()
    o = N.make_opts(offset_shift=2)
    rc = N.lib.bmqcrc_crc32c_verify(payload, 64, offs, lens, exp, 1, ctypes.byref(nbad), None, 0,
                                    ctypes.byref(o))
    assert rc in (0, N.BMQCRC_ENODEV), (rc, N.lib.bmqcrc_last_error())
    o.offset_shift = 9
    rc = N.lib.bmqcrc_crc32c_verify(payload, 64, offs, lens, exp, 1, ctypes.byref(nbad), None, 0,
                                    ctypes.byref(o))
    assert rc == N.BMQCRC_EINVAL


def test_struct_that_ends_before_offset_shift_gets_shift_0():
    # a caller built against ABI 2.7 that sets the new flag: its struct ends at
    # offset_shift, and whatever follows it in memory is not read
    end = N.Opts.offset_shift.offset
    raw = (ctypes.c_uint8 * (end + 16))()
    ctypes.memset(raw, 0xA5, ctypes.sizeof(raw))  # an offset_shift of 0xA5A5A5A5 if read
    v27 = N.make_opts(offset_shift=0)
    v27.struct_size = end
    ctypes.memmove(raw, ctypes.byref(v27), end)
    rc, err, out, want = _batch(ctypes.cast(raw, ctypes.POINTER(N.Opts)))
    assert rc in (0, N.BMQCRC_ENODEV), (rc, err)
    if rc == 0:
        assert out == [want]


def test_zero_struct_size_cannot_carry_the_shift():
    # struct_size 0 is ABI 2.0: nothing past ndevices is read, so the flag (a
    # 2.0 field) arrives and the shift does not
    raw = (ctypes.c_uint8 * ctypes.sizeof(N.Opts))()
    ctypes.memset(raw, 0xA5, ctypes.sizeof(raw))
    v20 = N.make_opts(offset_shift=0)
    v20.struct_size = 0
    ctypes.memmove(raw, ctypes.byref(v20), N.Opts.ndevices.offset)
    rc, err, out, want = _batch(ctypes.cast(raw, ctypes.POINTER(N.Opts)))
    assert rc in (0, N.BMQCRC_ENODEV), (rc, err)
    if rc == 0:
        assert out == [want]


def test_blobs_gather_and_fill_refuse_the_flag():
    o = N.make_opts(offset_shift=0)
    payload = (ctypes.c_uint8 * 64)(*range(64))
    off64 = (ctypes.c_uint64 * 1)(0)
    lens = (ctypes.c_uint32 * 1)(8)
    first = (ctypes.c_uint64 * 2)(0, 1)
    out = (ctypes.c_uint32 * 1)()
    rc = N.lib.bmqcrc_crc32c_blobs(payload, 64, off64, lens, 1, first, None, out, 1,
                                   ctypes.byref(o))
    assert rc == N.BMQCRC_EINVAL and b"OFFSETS32" in N.lib.bmqcrc_last_error()
    bufs = (ctypes.c_void_p * 1)(ctypes.addressof(payload))
    rc = N.lib.bmqcrc_crc32c_gather(bufs, lens, 1, first, None, out, 1, ctypes.byref(o))
    assert rc == N.BMQCRC_EINVAL and b"OFFSETS32" in N.lib.bmqcrc_last_error()
    rc = N.lib.bmqcrc_fill_synthetic(None, 0, 1, 0, ctypes.byref(o))
    assert rc == N.BMQCRC_EINVAL and b"OFFSETS32" in N.lib.bmqcrc_last_error()


def test_format_walks_refuse_the_flag():
    # the walks choose the form themselves
    ev = (ctypes.c_uint8 * 8)()
    o = N.make_opts(offset_shift=0)
    n = N.lib.bmqcrc_put_event_fill_crcs(ev, 8, ctypes.byref(o))
    assert n == N.BMQCRC_EINVAL


@pytest.mark.parametrize("struct_size", [0, 24, N.Opts.max_len.offset,
                                         N.Opts.offset_shift.offset])
def test_format_walks_take_an_older_callers_struct(struct_size):
    # a caller built against an earlier, shorter bmqcrc_opts (struct_size 0:
    # ABI 2.0) passes it to a walk, e.g. to pick the device: read by its
    # struct_size like the batch calls do, the bytes after it never looked at
    from blazingmq_amd.put_event import PutEventBuilder
    b = PutEventBuilder(defer_crc=False)
    for i in range(5):
        b.pack_message(bytes(range(40 + i)), queue_id=i)
    ev = np.ascontiguousarray(b.finalize())
    raw = (ctypes.c_uint8 * (ctypes.sizeof(N.Opts) + 16))()
    ctypes.memset(raw, 0xA5, ctypes.sizeof(raw))
    old = N.make_opts(device=0)
    old.struct_size = struct_size
    ctypes.memmove(raw, ctypes.byref(old), struct_size or 24)
    n_msgs, n_bad = ctypes.c_uint64(), ctypes.c_uint64()
    rc = N.lib.bmqcrc_put_event_verify(ev.ctypes.data, ev.size, ctypes.byref(n_msgs),
                                       ctypes.byref(n_bad), None, 0,
                                       ctypes.cast(raw, ctypes.POINTER(N.Opts)))
    err = N.lib.bmqcrc_last_error()
    assert b"struct_size" not in err, err
    assert rc in (0, N.BMQCRC_ENODEV), (rc, err)
    assert n_msgs.value == 5
    if rc == 0:
        assert n_bad.value == 0


def test_python_takes_empty_offsets():
    from blazingmq_amd.crc32c import _host_offsets
    for empty in ([], np.zeros(0, np.uint64), np.zeros(0, np.float64)):
        off = _host_offsets(empty, 0)
        assert off.dtype == np.uint32 and off.size == 0


def test_python_refuses_what_does_not_fit():
    arena = np.zeros(64, np.uint8)
    lens = np.array([8], np.uint32)
    with pytest.raises(ValueError):
        Crc32c.calculate_batch(arena, np.array([1 << 32], np.uint64), lens, offset_shift=0)
    with pytest.raises(ValueError):
        Crc32c.calculate_batch(arena, np.array([-1], np.int64), lens, offset_shift=0)
    with pytest.raises(ValueError):
        verify_batch(arena, np.array([1 << 32], np.uint64), lens, lens, offset_shift=0)
    for bad in (8, -1, 1.0, True):
        with pytest.raises(ValueError):
            Crc32c.calculate_batch(arena, np.array([0], np.uint32), lens, offset_shift=bad)
        with pytest.raises(ValueError):
            verify_batch(arena, np.array([0], np.uint32), lens, lens, offset_shift=bad)


def test_python_refuses_int64_tensor_offsets():
    import torch
    arena = torch.zeros(64, dtype=torch.uint8)
    off64 = torch.zeros(1, dtype=torch.int64)
    lens = torch.full((1,), 8, dtype=torch.int32)
    with pytest.raises(TypeError):
        Crc32c.calculate_batch(arena, off64, lens, offset_shift=0)
    with pytest.raises(TypeError):
        calculate_batch_ptr(0, 64, off64, lens, offset_shift=0)
    with pytest.raises(ValueError):
        calculate_batch_ptr(0, 64, off64.to(torch.int32), lens, offset_shift=8)
