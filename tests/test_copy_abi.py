"""ABI 2.9: bmqcrc_crc32c_copy and bmqcrc_last_copy, as far as they answer
without a GPU -- the declarations, the exports, the argument checks that sit
in front of the device lookup, and the Python wrapper's refusals."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from blazingmq_amd import Crc32c, _native as N, last_copy  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "blazingmq_amd", "lib", "libbmqcrc.so")
NEW = {"bmqcrc_crc32c_copy", "bmqcrc_last_copy"}
HEADERS = ("bmqcrc.h", "bmqcrc_protocol.h")


def _declared():
    """Every bmqcrc_ function the public headers declare (as test_abi.py)."""
    src = ""
    for h in HEADERS:
        with open(os.path.join(ROOT, "include", h)) as f:
            src += f.read()
    return set(re.findall(r"^\w[\w\s\*]*?\b(bmqcrc_\w+)\s*\(", src, re.M))


def _copy(opts, n=1):
    """bmqcrc_crc32c_copy with host addresses: only ever reaches the argument
    checks (a machine with a GPU is handed n = 0 by the callers that pass them)."""
    src = (ctypes.c_uint8 * 64)(*range(64))
    dst = (ctypes.c_uint8 * 64)()
    so, do = (ctypes.c_uint64 * 1)(0), (ctypes.c_uint64 * 1)(0)
    lens, out = (ctypes.c_uint32 * 1)(8), (ctypes.c_uint32 * 1)()
    rc = N.lib.bmqcrc_crc32c_copy(src, 64, so, lens, dst, 64, do, None, out, n, opts)
    return rc, N.lib.bmqcrc_last_error()


def test_header_declares_both_names():
    text = open(os.path.join(ROOT, "include", "bmqcrc.h")).read()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, text, re.M), name
    assert "(2.9)" in text


def test_library_exports_both_names_and_nothing_else_new():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    assert NEW <= exported
    # nothing rides along undeclared (a launcher, a helper): exports = declarations
    assert set(n for n in exported if n.startswith("bmqcrc_")) == _declared()


def test_version_is_2_9():
    v = N.lib.bmqcrc_version()
    assert v >> 16 == 2 and v & 0xffff >= 9


@pytest.mark.parametrize("flag,name", [
    (N.BMQCRC_F_WHOLE_MESSAGES, b"WHOLE_MESSAGES"), (N.BMQCRC_F_PLAN, b"PLAN"),
    (N.BMQCRC_F_TIME_KERNEL, b"TIME_KERNEL"), (N.BMQCRC_F_OFFSETS32, b"OFFSETS32")])
def test_other_flags_are_einval_naming_the_flag(flag, name):
    o = N.make_opts(flags=N.BMQCRC_F_DEVICE_PTRS | flag)
    rc, err = _copy(ctypes.byref(o))
    assert rc == N.BMQCRC_EINVAL and name in err, (rc, err)
    o = N.make_opts(flags=N.BMQCRC_F_DEVICE_PTRS | N.BMQCRC_F_ASYNC | flag)
    rc, err = _copy(ctypes.byref(o))
    assert rc == N.BMQCRC_EINVAL and name in err, (rc, err)


def test_unknown_flag_bits_are_einval():
    o = N.make_opts(flags=N.BMQCRC_F_DEVICE_PTRS | 0x4000)
    rc, err = _copy(ctypes.byref(o))
    assert rc == N.BMQCRC_EINVAL and b"unknown" in err, (rc, err)


@pytest.mark.parametrize("opts", [None, "plain", "async"])
def test_missing_device_ptrs_is_einval(opts):
    o = None if opts is None else ctypes.byref(
        N.make_opts(flags=N.BMQCRC_F_ASYNC if opts == "async" else 0))
    rc, err = _copy(o)
    assert rc == N.BMQCRC_EINVAL and b"DEVICE_PTRS" in err, (rc, err)


def test_more_than_one_device_is_einval():
    o = N.make_opts(flags=N.BMQCRC_F_DEVICE_PTRS, devices=[0, 1])
    rc, err = _copy(ctypes.byref(o))
    assert rc == N.BMQCRC_EINVAL and b"ndevices" in err, (rc, err)


def test_null_arrays_are_einval():
    o = N.make_opts(flags=N.BMQCRC_F_DEVICE_PTRS)
    rc = N.lib.bmqcrc_crc32c_copy(None, 64, None, None, None, 64, None, None, None, 1,
                                  ctypes.byref(o))
    assert rc == N.BMQCRC_EINVAL and b"null" in N.lib.bmqcrc_last_error()


@pytest.mark.parametrize("flags", [N.BMQCRC_F_DEVICE_PTRS,
                                   N.BMQCRC_F_DEVICE_PTRS | N.BMQCRC_F_ASYNC])
def test_valid_flags_reach_the_device_lookup(flags):
    # seg_bytes, max_len and min_len are ignored, whatever they hold
    o = N.make_opts(flags=flags, seg_bytes=12345, max_len=7, min_len=9)
    rc, err = _copy(ctypes.byref(o), n=1 if N.lib.bmqcrc_device_count() == 0 else 0)
    assert rc == (N.BMQCRC_ENODEV if N.lib.bmqcrc_device_count() == 0 else 0), (rc, err)
    n, r, f = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    rc = N.lib.bmqcrc_last_copy(-1, None, ctypes.byref(n), ctypes.byref(r), ctypes.byref(f))
    assert rc == (N.BMQCRC_ENODEV if N.lib.bmqcrc_device_count() == 0 else 0)


def _tensors(n=3, size=64):
    return dict(src=torch.zeros(size, dtype=torch.uint8),
                src_offsets=torch.zeros(n, dtype=torch.int64),
                lengths=torch.full((n,), 8, dtype=torch.int32),
                dst=torch.zeros(size, dtype=torch.uint8),
                dst_offsets=torch.arange(n, dtype=torch.int64) * 8)


@pytest.mark.parametrize("name,dtype", [
    ("src", torch.int8), ("dst", torch.int32), ("src_offsets", torch.int32),
    ("dst_offsets", torch.int32), ("lengths", torch.int64)])
def test_python_refuses_wrong_dtypes(name, dtype):
    t = _tensors()
    t[name] = t[name].to(dtype)
    with pytest.raises(TypeError, match=name):
        Crc32c.copy_batch(**t)


def test_python_refuses_wrong_seeds_and_out():
    t = _tensors()
    with pytest.raises(TypeError, match="seeds"):
        Crc32c.copy_batch(seeds=torch.zeros(3, dtype=torch.int64), **t)
    with pytest.raises(TypeError, match="seeds"):
        Crc32c.copy_batch(seeds=torch.zeros(4, dtype=torch.int32), **t)
    with pytest.raises(TypeError, match="out"):
        Crc32c.copy_batch(out=torch.zeros(2, dtype=torch.int32), **t)
    with pytest.raises(TypeError, match="out"):
        Crc32c.copy_batch(out=torch.zeros(3, dtype=torch.uint8), **t)


@pytest.mark.parametrize("name", ["lengths", "dst_offsets"])
def test_python_refuses_wrong_sizes(name):
    t = _tensors()
    t[name] = t[name][:2].contiguous()
    with pytest.raises(ValueError, match="size mismatch"):
        Crc32c.copy_batch(**t)


@pytest.mark.parametrize("name", ["src", "dst", "src_offsets", "dst_offsets", "lengths"])
def test_python_refuses_non_contiguous(name):
    t = _tensors(n=3, size=64)
    wide = torch.zeros(2 * t[name].numel(), dtype=t[name].dtype)
    t[name] = wide[::2]
    assert not t[name].is_contiguous()
    with pytest.raises(TypeError, match=name):
        Crc32c.copy_batch(**t)


def test_python_refuses_host_tensors():
    # device pointers only: host-resident callers keep calculate_blobs (gather)
    with pytest.raises(TypeError, match="device tensors only"):
        Crc32c.copy_batch(**_tensors())
    with pytest.raises(TypeError):
        Crc32c.copy_batch(src_offsets=[0], lengths=[8], src=b"12345678", dst=bytearray(8),
                          dst_offsets=[0])
