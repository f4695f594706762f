"""ABI 2.13: bmqcrc_message_records_unpack and bmqcrc_last_records_unpack, as
far as they answer without a GPU -- the declarations, the exports, the struct
layouts, the argument checks that sit in front of the device lookup, and the
Python wrapper's refusals."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from blazingmq_amd import _native as N, last_records_unpack, unpack_records  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "blazingmq_amd", "lib", "libbmqcrc.so")
NEW = {"bmqcrc_message_records_unpack", "bmqcrc_last_records_unpack"}
HEADERS = ("bmqcrc.h", "bmqcrc_protocol.h")
NO_GPU = N.lib.bmqcrc_device_count() == 0
KINDS = ("OK", "RECORD_HEADER", "MESSAGE_RECORD", "DATA_OFFSET", "DATA_RECORD",
         "TOO_MANY_MESSAGES")
OUTPUTS = (("record_index", 4), ("app_offsets", 8), ("lengths", 4), ("queue_keys", 5),
           ("guids", 16), ("data_flags", 1), ("ref_counts", 4), ("timestamps", 8),
           ("expected", 4), ("out", 4))
OPTIONAL = tuple(n for n, _ in OUTPUTS if n not in ("app_offsets", "lengths"))


def _declared():
    src = ""
    for h in HEADERS:
        with open(os.path.join(ROOT, "include", h)) as f:
            src += f.read()
    return set(re.findall(r"^\w[\w\s\*]*?\b(bmqcrc_\w+)\s*\(", src, re.M))


class _Call:
    """A valid call over two records on host addresses: it only ever reaches
    the argument checks (a machine with a GPU is handed n_records = 0 where it
    would pass)."""
    CAP = 4

    def __init__(self):
        self.jour = (ctypes.c_uint32 * 32)()    # 128 bytes: two records and a tail
        self.data = (ctypes.c_uint64 * 8)()
        self.sel = (ctypes.c_uint8 * 2)(1, 1)
        self.arr = {name: (ctypes.c_uint64 * (2 * self.CAP))() for name, _ in OUTPUTS}
        p = N.RecordsUnpack()
        p.struct_size = ctypes.sizeof(N.RecordsUnpack)
        p.journal, p.journal_bytes, p.n_records = ctypes.addressof(self.jour), 128, 2
        p.data, p.data_bytes, p.data_file_pos = ctypes.addressof(self.data), 64, 40
        p.select, p.msg_cap = ctypes.addressof(self.sel), self.CAP
        for name, a in self.arr.items():
            setattr(p, name, ctypes.addressof(a))
        self.p = p

    def run(self, flags=N.BMQCRC_F_DEVICE_PTRS, opts="make", **kw):
        o = N.make_opts(flags=flags, **kw) if opts == "make" else opts
        r = N.RecordsUnpackResult()
        rc = N.lib.bmqcrc_message_records_unpack(ctypes.byref(self.p), ctypes.byref(r),
                                                 ctypes.byref(o) if o is not None else None)
        return rc, N.lib.bmqcrc_last_error()


def test_header_declares_both_names_and_the_kinds():
    text = open(os.path.join(ROOT, "include", "bmqcrc_protocol.h")).read()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, text, re.M), name
    for value, kind in enumerate(KINDS):
        assert re.search(r"#define BMQCRC_REC_UNPACK_%s %d\b" % (kind, value), text), kind
    # what the call does not restate is said in the header
    for words in ("ordering checks", "queue liveness", "the selection itself",
                  "the journal bounds"):
        assert words in text, words
    assert text.index("ABI 2.12") < text.index("ABI 2.13")
    main = open(os.path.join(ROOT, "include", "bmqcrc.h")).read()
    assert "(2.11)" in main and "(2.12)" in main and "(2.13)" in main


def test_library_exports_both_names_and_nothing_undeclared():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    assert NEW <= exported
    assert set(n for n in exported if n.startswith("bmqcrc_")) == _declared()


def test_version_is_2_13():
    v = N.lib.bmqcrc_version()
    assert v >> 16 == 2 and v & 0xffff >= 13


def test_kind_constants():
    for value, kind in enumerate(KINDS):
        assert getattr(N, "BMQCRC_REC_UNPACK_" + kind) == value


@pytest.mark.parametrize("struct,ctype,size", [
    ("bmqcrc_records_unpack", N.RecordsUnpack, 152),
    ("bmqcrc_records_unpack_result", N.RecordsUnpackResult, 56)])
def test_struct_layouts_match_the_header(tmp_path, struct, ctype, size):
    fields = [f[0] for f in ctype._fields_]
    src = tmp_path / "unpack.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bmqcrc_protocol.h"\n'
                   'int main(void) { printf("%%zu", sizeof(%s));\n' % struct +
                   "".join('printf(" %%zu", offsetof(%s, %s));\n' % (struct, f) for f in fields) +
                   "".join('printf(" %%d", BMQCRC_REC_UNPACK_%s);\n' % k for k in KINDS) +
                   'return 0; }\n')
    exe = tmp_path / "unpack"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert got == [ctypes.sizeof(ctype)] + [getattr(ctype, f).offset for f in fields] + [
        getattr(N, "BMQCRC_REC_UNPACK_" + k) for k in KINDS]
    assert got[0] == size and got[-6:] == [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("flag,name", [
    (N.BMQCRC_F_WHOLE_MESSAGES, b"WHOLE_MESSAGES"), (N.BMQCRC_F_PLAN, b"PLAN"),
    (N.BMQCRC_F_TIME_KERNEL, b"TIME_KERNEL"), (N.BMQCRC_F_OFFSETS32, b"OFFSETS32")])
def test_other_flags_are_einval_naming_the_flag(flag, name):
    for extra in (0, N.BMQCRC_F_ASYNC):
        rc, err = _Call().run(N.BMQCRC_F_DEVICE_PTRS | extra | flag)
        assert rc == N.BMQCRC_EINVAL and name in err, (rc, err)
        assert b"bmqcrc_message_records_unpack" in err, err


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
    assert N.lib.bmqcrc_message_records_unpack(None, None, None) == N.BMQCRC_EINVAL


@pytest.mark.parametrize("name", ["journal", "data", "app_offsets", "lengths"])
def test_null_required_array_is_einval_naming_it(name):
    c = _Call()
    setattr(c.p, name, None)
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"null" in err and err.endswith(b": " + name.encode()), err


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_misaligned_journal_is_einval(shift):
    c = _Call()
    c.p.journal = ctypes.addressof(c.jour) + shift
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"journal must be 4-byte aligned" in err, (rc, err)


@pytest.mark.parametrize("shift", [1, 2, 4, 7])
def test_misaligned_data_is_einval(shift):
    c = _Call()
    c.p.data = ctypes.addressof(c.data) + shift
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"data must be 8-byte aligned" in err, (rc, err)


@pytest.mark.parametrize("pos", [1, 4, 44, (1 << 35) + 4])
def test_data_file_pos_must_be_a_multiple_of_8(pos):
    c = _Call()
    c.p.data_file_pos = pos
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"data_file_pos" in err and b"multiple of 8" in err, err


@pytest.mark.parametrize("name", ["n_records", "msg_cap"])
def test_counts_at_2_to_the_32_are_einval(name):
    c = _Call()
    setattr(c.p, name, 1 << 32)
    c.p.journal_bytes = 60 << 32
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"2^32" in err, (rc, err)


def test_journal_bytes_below_60_n_is_einval():
    c = _Call()
    c.p.journal_bytes = 119
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"journal_bytes is below 60 n_records" in err, (rc, err)
    c.p.journal_bytes = 120
    if not NO_GPU:
        c.p.n_records = 0
    rc, err = c.run()
    assert rc == (N.BMQCRC_ENODEV if NO_GPU else 0), (rc, err)


@pytest.mark.parametrize("name,elem", OUTPUTS)
@pytest.mark.parametrize("where", ["inside", "tail_in", "head_in"])
@pytest.mark.parametrize("region", ["journal", "data"])
def test_output_array_meeting_an_input_is_einval(name, elem, where, region):
    c = _Call()
    buf = (ctypes.c_uint8 * 2048)()
    base = ctypes.addressof(buf)
    base += -base % 8
    size = elem * c.CAP
    # journal = [base + 256, base + 512), data = [base + 1024, base + 1280)
    c.p.journal, c.p.journal_bytes = base + 256, 256
    c.p.data, c.p.data_bytes = base + 1024, 256
    lo = base + (256 if region == "journal" else 1024)
    at = {"inside": lo + 64, "tail_in": lo - size + 1, "head_in": lo + 255}[where]
    setattr(c.p, name, at)
    c.keep = buf
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"overlaps" in err and name.encode() in err, (rc, err)
    assert (b"[%s, " % region.encode()) in err, err


def test_adjacent_output_arrays_reach_the_device_lookup():
    c = _Call()
    buf = (ctypes.c_uint8 * 2048)()
    base = ctypes.addressof(buf)
    base += -base % 8
    c.p.journal, c.p.journal_bytes = base + 256, 120
    c.p.data, c.p.data_bytes = base + 1024, 64
    c.p.app_offsets = base + 256 - 8 * c.CAP   # ends where the journal begins
    c.p.lengths = base + 256 + 120             # begins where it ends
    c.p.guids = base + 1024 - 16 * c.CAP       # ends where the data begin
    c.p.expected = base + 1024 + 64            # begins where they end
    c.keep = buf
    if not NO_GPU:
        c.p.n_records = 0
    rc, err = c.run()
    assert rc == (N.BMQCRC_ENODEV if NO_GPU else 0), (rc, err)


@pytest.mark.parametrize("flags", [N.BMQCRC_F_DEVICE_PTRS,
                                   N.BMQCRC_F_DEVICE_PTRS | N.BMQCRC_F_ASYNC])
@pytest.mark.parametrize("optional", [True, False])
def test_valid_arguments_reach_the_device_lookup(flags, optional):
    c = _Call()
    if not optional:
        for name in OPTIONAL + ("select",):
            setattr(c.p, name, None)
        c.p.data_file_pos = 0
    if not NO_GPU:
        c.p.n_records = 0
    rc, err = c.run(flags, seg_bytes=12345, max_len=7, min_len=9)
    assert rc == (N.BMQCRC_ENODEV if NO_GPU else 0), (rc, err)
    r = N.RecordsUnpackResult()
    rc = N.lib.bmqcrc_last_records_unpack(-1, None, ctypes.byref(r))
    assert rc == (N.BMQCRC_ENODEV if NO_GPU else 0)
    if not NO_GPU:
        assert r.as_dict() == dict(n_records=0, n_msgs=0, n_skipped=0, n_bad=0, first_bad=0,
                                   refused_kind=0, refused_index=0)


# ---- the Python wrapper ------------------------------------------------------

def test_python_refuses_wrong_types():
    j, d = torch.zeros(120, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(TypeError, match="journal"):
        unpack_records(j.to(torch.int8), d, data_file_pos=0)
    with pytest.raises(TypeError, match="journal"):
        unpack_records(torch.zeros(240, dtype=torch.uint8)[::2], d, data_file_pos=0)
    with pytest.raises(TypeError, match="journal"):
        unpack_records(bytes(120), d, data_file_pos=0)
    with pytest.raises(TypeError, match="data"):
        unpack_records(j, d.to(torch.int32), data_file_pos=0)
    with pytest.raises(TypeError, match="data"):
        unpack_records(j, torch.zeros(128, dtype=torch.uint8)[::2], data_file_pos=0)
    with pytest.raises(TypeError, match="select"):
        unpack_records(j, d, data_file_pos=0, select=torch.ones(2, dtype=torch.bool))
    with pytest.raises(TypeError, match="select"):
        unpack_records(j, d, data_file_pos=0, select=[1, 1])


def test_python_refuses_host_tensors():
    j, d = torch.zeros(120, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(TypeError, match="device tensors only"):
        unpack_records(j, d, data_file_pos=0)
    with pytest.raises(TypeError, match="device tensors only"):
        unpack_records(j, d, data_file_pos=40, select=torch.ones(2, dtype=torch.uint8))
