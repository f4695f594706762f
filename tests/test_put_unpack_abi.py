"""ABI 2.12: bmqcrc_put_event_unpack and bmqcrc_last_put_unpack, as far as they
answer without a GPU -- the declarations, the exports, the struct layouts, the
argument checks that sit in front of the device lookup, and the Python
wrapper's refusals."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from blazingmq_amd import _native as N, last_put_unpack, unpack_events  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "blazingmq_amd", "lib", "libbmqcrc.so")
NEW = {"bmqcrc_put_event_unpack", "bmqcrc_last_put_unpack"}
HEADERS = ("bmqcrc.h", "bmqcrc_protocol.h")
NO_GPU = N.lib.bmqcrc_device_count() == 0
KINDS = ("OK", "EVENT_OFFSETS", "EVENT_HEADER", "PUT_HEADER", "PADDING", "TOO_MANY_MESSAGES")


def _declared():
    src = ""
    for h in HEADERS:
        with open(os.path.join(ROOT, "include", h)) as f:
            src += f.read()
    return set(re.findall(r"^\w[\w\s\*]*?\b(bmqcrc_\w+)\s*\(", src, re.M))


class _Call:
    """A valid two-event call on host addresses: it only ever reaches the
    argument checks (a machine with a GPU is handed n_events = 0 where it
    would pass)."""
    CAP = 4

    def __init__(self):
        self.buf = (ctypes.c_uint32 * 64)()
        self.offs = (ctypes.c_uint64 * 3)(0, 8, 16)
        self.app = (ctypes.c_uint64 * self.CAP)()
        self.lens = (ctypes.c_uint32 * self.CAP)()
        self.qid = (ctypes.c_int32 * self.CAP)()
        self.guid = (ctypes.c_uint8 * (16 * self.CAP))()
        self.flags = (ctypes.c_uint8 * self.CAP)()
        self.exp = (ctypes.c_uint32 * self.CAP)()
        self.out = (ctypes.c_uint32 * self.CAP)()
        self.first = (ctypes.c_uint64 * 3)()
        p = N.PutUnpack()
        p.struct_size = ctypes.sizeof(N.PutUnpack)
        p.events, p.events_bytes = ctypes.addressof(self.buf), 16
        p.event_offsets, p.n_events, p.msg_cap = ctypes.addressof(self.offs), 2, self.CAP
        p.app_offsets, p.lengths = ctypes.addressof(self.app), ctypes.addressof(self.lens)
        p.queue_ids, p.guids = ctypes.addressof(self.qid), ctypes.addressof(self.guid)
        p.flags, p.expected = ctypes.addressof(self.flags), ctypes.addressof(self.exp)
        p.out, p.event_first = ctypes.addressof(self.out), ctypes.addressof(self.first)
        self.p = p

    def run(self, flags=N.BMQCRC_F_DEVICE_PTRS, opts="make", **kw):
        o = N.make_opts(flags=flags, **kw) if opts == "make" else opts
        r = N.PutUnpackResult()
        rc = N.lib.bmqcrc_put_event_unpack(ctypes.byref(self.p), ctypes.byref(r),
                                           ctypes.byref(o) if o is not None else None)
        return rc, N.lib.bmqcrc_last_error()


def test_header_declares_both_names_and_the_kinds():
    text = open(os.path.join(ROOT, "include", "bmqcrc_protocol.h")).read()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, text, re.M), name
    for value, kind in enumerate(KINDS):
        assert re.search(r"#define BMQCRC_PUT_UNPACK_%s %d\b" % (kind, value), text), kind
    assert "a tight msg_cap" in text and "20 bytes per slot" in text
    main = open(os.path.join(ROOT, "include", "bmqcrc.h")).read()
    assert "(2.11)" in main and "(2.12)" in main


def test_library_exports_both_names_and_nothing_undeclared():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    assert NEW <= exported
    assert set(n for n in exported if n.startswith("bmqcrc_")) == _declared()


def test_version_is_2_12():
    v = N.lib.bmqcrc_version()
    assert v >> 16 == 2 and v & 0xffff >= 12


@pytest.mark.parametrize("struct,ctype,size", [("bmqcrc_put_unpack", N.PutUnpack, 112),
                                               ("bmqcrc_put_unpack_result", N.PutUnpackResult, 56)])
def test_struct_layouts_match_the_header(tmp_path, struct, ctype, size):
    fields = [f[0] for f in ctype._fields_]
    src = tmp_path / "unpack.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bmqcrc_protocol.h"\n'
                   'int main(void) { printf("%%zu", sizeof(%s));\n' % struct +
                   "".join('printf(" %%zu", offsetof(%s, %s));\n' % (struct, f) for f in fields) +
                   "".join('printf(" %%d", BMQCRC_PUT_UNPACK_%s);\n' % k for k in KINDS) +
                   'return 0; }\n')
    exe = tmp_path / "unpack"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert got == [ctypes.sizeof(ctype)] + [getattr(ctype, f).offset for f in fields] + [
        getattr(N, "BMQCRC_PUT_UNPACK_" + k) for k in KINDS]
    assert got[0] == size and got[-6:] == [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("flag,name", [
    (N.BMQCRC_F_WHOLE_MESSAGES, b"WHOLE_MESSAGES"), (N.BMQCRC_F_PLAN, b"PLAN"),
    (N.BMQCRC_F_TIME_KERNEL, b"TIME_KERNEL"), (N.BMQCRC_F_OFFSETS32, b"OFFSETS32")])
def test_other_flags_are_einval_naming_the_flag(flag, name):
    for extra in (0, N.BMQCRC_F_ASYNC):
        rc, err = _Call().run(N.BMQCRC_F_DEVICE_PTRS | extra | flag)
        assert rc == N.BMQCRC_EINVAL and name in err, (rc, err)


def test_unknown_flag_bits_are_einval():
    rc, err = _Call().run(N.BMQCRC_F_DEVICE_PTRS | 0x4000)
    assert rc == N.BMQCRC_EINVAL and b"unknown" in err, (rc, err)


@pytest.mark.parametrize("opts", [None, "plain", "async"])
def test_missing_device_ptrs_is_einval(opts):
    c = _Call()
    rc, err = c.run(opts=None) if opts is None else c.run(
        N.BMQCRC_F_ASYNC if opts == "async" else 0)
    assert rc == N.BMQCRC_EINVAL and b"DEVICE_PTRS" in err, (rc, err)


def test_more_than_one_device_is_einval():
    rc, err = _Call().run(devices=[0, 1])
    assert rc == N.BMQCRC_EINVAL and b"ndevices" in err, (rc, err)


def test_struct_size_and_reserved():
    c = _Call()
    c.p.struct_size -= 8
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"struct_size" in err, (rc, err)
    c = _Call()
    c.p.reserved = 1
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"reserved" in err, (rc, err)
    assert N.lib.bmqcrc_put_event_unpack(None, None, None) == N.BMQCRC_EINVAL


@pytest.mark.parametrize("name", ["events", "app_offsets", "lengths"])
def test_null_required_array_is_einval_naming_it(name):
    c = _Call()
    setattr(c.p, name, None)
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"null" in err and err.endswith(b": " + name.encode()), err


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_misaligned_events_is_einval(shift):
    c = _Call()
    c.p.events = ctypes.addressof(c.buf) + shift
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"4-byte aligned" in err, (rc, err)


@pytest.mark.parametrize("n_events", [0, 2])
def test_null_event_offsets_means_one_event(n_events):
    c = _Call()
    c.p.event_offsets, c.p.n_events = None, n_events
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"event_offsets == NULL" in err, (rc, err)


@pytest.mark.parametrize("name", ["n_events", "msg_cap"])
def test_counts_at_2_to_the_32_are_einval(name):
    c = _Call()
    setattr(c.p, name, 1 << 32)
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"2^32" in err, (rc, err)


@pytest.mark.parametrize("name,elem", [("app_offsets", 8), ("lengths", 4), ("queue_ids", 4),
                                       ("guids", 16), ("flags", 1), ("expected", 4),
                                       ("out", 4), ("event_first", None)])
@pytest.mark.parametrize("where", ["inside", "tail_in_events", "head_in_events"])
def test_output_array_meeting_the_events_is_einval(name, elem, where):
    c = _Call()
    buf = (ctypes.c_uint8 * 1024)()
    base = ctypes.addressof(buf)
    base += -base % 8
    size = elem * c.CAP if elem else 8 * 3
    # events = [base + 256, base + 512)
    c.p.events, c.p.events_bytes = base + 256, 256
    c.offs[2] = 256
    at = {"inside": base + 256 + 64, "tail_in_events": base + 256 - size + 1,
          "head_in_events": base + 511}[where]
    setattr(c.p, name, at)
    c.keep = buf
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"overlaps" in err and name.encode() in err, (rc, err)


def test_adjacent_output_arrays_reach_the_device_lookup():
    c = _Call()
    buf = (ctypes.c_uint8 * 1024)()
    base = ctypes.addressof(buf)
    base += -base % 8
    c.p.events, c.p.events_bytes = base + 256, 16
    c.p.app_offsets = base + 256 - 8 * c.CAP  # ends where the events begin
    c.p.lengths = base + 256 + 16             # begins where they end
    c.keep = buf
    if not NO_GPU:
        c.p.n_events = 0
    rc, err = c.run()
    assert rc == (N.BMQCRC_ENODEV if NO_GPU else 0), (rc, err)


@pytest.mark.parametrize("flags", [N.BMQCRC_F_DEVICE_PTRS,
                                   N.BMQCRC_F_DEVICE_PTRS | N.BMQCRC_F_ASYNC])
@pytest.mark.parametrize("optional", [True, False])
def test_valid_arguments_reach_the_device_lookup(flags, optional):
    c = _Call()
    if not optional:
        for name in ("queue_ids", "guids", "flags", "expected", "out", "event_first"):
            setattr(c.p, name, None)
    if not NO_GPU:
        c.p.n_events = 0
    rc, err = c.run(flags, seg_bytes=12345, max_len=7, min_len=9)
    assert rc == (N.BMQCRC_ENODEV if NO_GPU else 0), (rc, err)
    r = N.PutUnpackResult()
    rc = N.lib.bmqcrc_last_put_unpack(-1, None, ctypes.byref(r))
    assert rc == (N.BMQCRC_ENODEV if NO_GPU else 0)
    if not NO_GPU:
        assert r.as_dict() == dict(n_events=0, n_msgs=0, n_bad=0, first_bad=0, refused_kind=0,
                                   refused_event=0, refused_offset=0)


# ---- the Python wrapper ------------------------------------------------------

def test_python_refuses_wrong_types():
    ev = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(TypeError, match="events"):
        unpack_events(ev.to(torch.int8))
    with pytest.raises(TypeError, match="events"):
        unpack_events(torch.zeros(128, dtype=torch.uint8)[::2])
    with pytest.raises(TypeError, match="events"):
        unpack_events(b"12345678")
    with pytest.raises(TypeError, match="event_offsets"):
        unpack_events(ev, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(TypeError, match="event_offsets"):
        unpack_events(ev, [0, 64])


def test_python_refuses_host_tensors():
    with pytest.raises(TypeError, match="device tensors only"):
        unpack_events(torch.zeros(64, dtype=torch.uint8))
    with pytest.raises(TypeError, match="device tensors only"):
        unpack_events(torch.zeros(64, dtype=torch.uint8), torch.tensor([0, 64]))
