"""ABI 2.18: bmqcrc_partition_rollover and bmqcrc_last_rollover, as far as they
answer without a GPU -- the declarations, the exports, the struct layouts, the
argument checks that sit in front of the device lookup, and the Python
wrapper's refusals."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import blazingmq_amd
from blazingmq_amd import _native as N, last_rollover, rollover_records  # noqa: F401
from blazingmq_amd import storage as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "blazingmq_amd", "lib", "libbmqcrc.so")
NEW = {"bmqcrc_partition_rollover", "bmqcrc_last_rollover"}
HEADERS = ("bmqcrc.h", "bmqcrc_protocol.h")
NO_GPU = N.lib.bmqcrc_device_count() == 0
KINDS = ("OK", "RECORD_HEADER", "KEEP_JOURNAL_OP", "SYNC_POINT", "DATA_OFFSET", "DATA_RECORD",
         "DST_TOO_SMALL", "DATA_FILE_FULL", "TOO_MANY_PIECES")
RECORDS = 4
# name -> bytes of a valid call's array
# (keep holds RECORDS bytes; the 8 keeps a neighbour placed against its end 8-byte aligned)
INPUTS = {"journal": 60 * RECORDS, "data": 256, "keep": 8}
OUTPUTS = {"dst": 512, "journal_dst": 60 * (RECORDS + 1), "new_index": 4 * RECORDS,
           "out": 4 * RECORDS}
SIZES = {"dst": "dst_bytes", "journal_dst": "journal_dst_bytes"}


def _declared():
    src = ""
    for h in HEADERS:
        with open(os.path.join(ROOT, "include", h)) as f:
            src += f.read()
    return set(re.findall(r"^\w[\w\s\*]*?\b(bmqcrc_\w+)\s*\(", src, re.M))


class _Call:
    """A valid call over four records on host addresses: it only ever reaches
    the argument checks (a machine with a GPU is handed n_records = 0 where it
    would pass)."""

    def __init__(self):
        self.buf = (ctypes.c_uint8 * 10240)()
        base = ctypes.addressof(self.buf)
        base += -base % 8
        self.base = base
        # 1 KiB apart, in this order
        self.at = {name: base + 1024 * (k + 1)
                   for k, name in enumerate(list(INPUTS) + list(OUTPUTS))}
        p = N.Rollover()
        p.struct_size = ctypes.sizeof(N.Rollover)
        for name, where in self.at.items():
            setattr(p, name, where)
        p.journal_bytes, p.n_records = 60 * RECORDS, RECORDS
        p.data_bytes, p.data_file_pos = 256, 40
        p.confirm_mode, p.sync_point, p.timestamp = 1, RECORDS - 1, 0x6720EAB4
        p.new_data_file_pos = 40
        p.dst_bytes, p.journal_dst_bytes = 512, 60 * (RECORDS + 1)
        self.p = p

    def run(self, flags=N.BMQCRC_F_DEVICE_PTRS, opts="make", **kw):
        o = N.make_opts(flags=flags, **kw) if opts == "make" else opts
        r = N.RolloverResult()
        rc = N.lib.bmqcrc_partition_rollover(ctypes.byref(self.p), ctypes.byref(r),
                                             ctypes.byref(o) if o is not None else None)
        return rc, N.lib.bmqcrc_last_error()

    def passes(self, flags=N.BMQCRC_F_DEVICE_PTRS, **kw):
        if not NO_GPU:
            self.p.n_records = self.p.journal_bytes = 0
            self.p.sync_point = N.BMQCRC_ROLLOVER_NO_SYNC_POINT
        rc, err = self.run(flags, **kw)
        assert rc == (N.BMQCRC_ENODEV if NO_GPU else 0), (rc, err)

    def einval(self, *words):
        rc, err = self.run()
        assert rc == N.BMQCRC_EINVAL, (rc, err)
        for w in words:
            assert w in err, (w, err)


def test_header_declares_both_names_and_the_kinds():
    text = open(os.path.join(ROOT, "include", "bmqcrc_protocol.h")).read()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, text, re.M), name
    for value, kind in enumerate(KINDS):
        assert re.search(r"#define BMQCRC_ROLLOVER_%s %d\b" % (kind, value), text), kind
    assert re.search(r"#define BMQCRC_ROLLOVER_CONFIRMS_AS_KEPT 0\b", text)
    assert re.search(r"#define BMQCRC_ROLLOVER_CONFIRMS_FOLLOW_MESSAGES 1\b", text)
    assert text.index("ABI 2.17") < text.index("ABI 2.18")
    main = open(os.path.join(ROOT, "include", "bmqcrc.h")).read()
    assert re.search(r"\(2\.18\) bmqcrc_partition_rollover, bmqcrc_last_rollover", main)


def test_library_exports_both_names_and_nothing_undeclared():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    assert NEW <= exported
    assert set(n for n in exported if n.startswith("bmqcrc_")) == _declared()


def test_version_is_2_18():
    v = N.lib.bmqcrc_version()
    assert v >> 16 == 2 and v & 0xffff >= 18


def test_kind_constants_and_package_exports():
    for value, kind in enumerate(KINDS):
        assert getattr(N, "BMQCRC_ROLLOVER_" + kind) == value
    assert N.BMQCRC_ROLLOVER_NO_SYNC_POINT == (1 << 64) - 1
    assert (S.CONFIRMS_AS_KEPT, S.CONFIRMS_FOLLOW_MESSAGES) == (0, 1)
    assert {"rollover_records", "last_rollover"} <= set(blazingmq_amd.__all__)
    assert blazingmq_amd.rollover_records is S.rollover_records
    assert blazingmq_amd.last_rollover is S.last_rollover


@pytest.mark.parametrize("struct,ctype,size", [
    ("bmqcrc_rollover", N.Rollover, 144),
    ("bmqcrc_rollover_result", N.RolloverResult, 72)])
def test_struct_layouts_match_the_header(tmp_path, struct, ctype, size):
    fields = [f[0] for f in ctype._fields_]
    src = tmp_path / "roll.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bmqcrc_protocol.h"\n'
                   'int main(void) { printf("%%zu", sizeof(%s));\n' % struct +
                   "".join('printf(" %%zu", offsetof(%s, %s));\n' % (struct, f) for f in fields) +
                   "".join('printf(" %%d", BMQCRC_ROLLOVER_%s);\n' % k for k in KINDS) +
                   'printf(" %d", BMQCRC_ROLLOVER_NO_SYNC_POINT == ~0ull);\n'
                   'return 0; }\n')
    exe = tmp_path / "roll"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert got == [ctypes.sizeof(ctype)] + [getattr(ctype, f).offset for f in fields] + [
        getattr(N, "BMQCRC_ROLLOVER_" + k) for k in KINDS] + [1]
    assert got[0] == size and got[-10:-1] == list(range(9))


@pytest.mark.parametrize("flag,name", [
    (N.BMQCRC_F_WHOLE_MESSAGES, b"WHOLE_MESSAGES"), (N.BMQCRC_F_PLAN, b"PLAN"),
    (N.BMQCRC_F_TIME_KERNEL, b"TIME_KERNEL"), (N.BMQCRC_F_OFFSETS32, b"OFFSETS32")])
def test_other_flags_are_einval_naming_the_flag(flag, name):
    for extra in (0, N.BMQCRC_F_ASYNC):
        rc, err = _Call().run(N.BMQCRC_F_DEVICE_PTRS | extra | flag)
        assert rc == N.BMQCRC_EINVAL and name in err, (rc, err)
        assert b"bmqcrc_partition_rollover" in err, err


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
    c.einval(b"struct_size")
    for name in ("reserved", "reserved2"):
        c = _Call()
        setattr(c.p, name, 1)
        c.einval(b"reserved")
    assert N.lib.bmqcrc_partition_rollover(None, None, None) == N.BMQCRC_EINVAL


@pytest.mark.parametrize("name", ["journal", "data", "dst", "journal_dst"])
def test_null_required_pointer_is_einval_naming_it(name):
    c = _Call()
    setattr(c.p, name, None)
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"null" in err and err.endswith(b": " + name.encode()), err


@pytest.mark.parametrize("name,shifts,words", [
    ("journal", (1, 2, 3), b"journal must be 4-byte aligned"),
    ("journal_dst", (1, 2, 3), b"journal_dst must be 4-byte aligned"),
    ("new_index", (1, 2, 3), b"new_index must be 4-byte aligned"),
    ("out", (1, 2, 3), b"out must be 4-byte aligned"),
    ("dst", (1, 2, 4, 7), b"dst must be 8-byte aligned"),
    ("data", (1, 2, 4, 7), b"data must be 8-byte aligned")])
def test_misaligned_pointer_is_einval(name, shifts, words):
    for shift in shifts:
        c = _Call()
        setattr(c.p, name, getattr(c.p, name) + shift)
        c.einval(words)


@pytest.mark.parametrize("nbytes", [0, 60 * RECORDS - 1, 60 * RECORDS + 60])
def test_journal_bytes_must_be_60_n_records(nbytes):
    c = _Call()
    c.p.journal_bytes = nbytes
    c.einval(b"journal_bytes must be 60 n_records")


@pytest.mark.parametrize("n", [1 << 32, (1 << 32) + 5, 1 << 40])
def test_n_records_must_be_below_2_32(n):
    c = _Call()
    c.p.n_records, c.p.journal_bytes = n, 60 * n
    c.p.sync_point = N.BMQCRC_ROLLOVER_NO_SYNC_POINT
    c.einval(b"n_records must be below 2^32")


@pytest.mark.parametrize("pos", [1, 4, 44, (1 << 35) + 4])
def test_data_file_pos_must_be_a_multiple_of_8(pos):
    c = _Call()
    c.p.data_file_pos = pos
    c.einval(b"data_file_pos", b"multiple of 8")


@pytest.mark.parametrize("pos", [0, 1, 4, 44, (1 << 35) + 4])
def test_new_data_file_pos_must_be_a_multiple_of_8_and_not_0(pos):
    c = _Call()
    c.p.new_data_file_pos = pos
    c.einval(b"new_data_file_pos", b"multiple of 8")


def test_confirm_mode_above_1():
    for mode in (2, 3, 1 << 31):
        c = _Call()
        c.p.confirm_mode = mode
        c.einval(b"confirm_mode")
    for mode in (0, 1):
        c = _Call()
        c.p.confirm_mode = mode
        c.passes()


def test_sync_point_must_be_a_record_or_the_no_value():
    for s in (RECORDS, RECORDS + 1, 1 << 40, (1 << 64) - 2):
        c = _Call()
        c.p.sync_point = s
        c.einval(b"sync_point")
    for s in (0, RECORDS - 1, N.BMQCRC_ROLLOVER_NO_SYNC_POINT):
        c = _Call()
        c.p.sync_point = s
        c.passes()


def test_an_empty_run_admits_no_sync_point():
    c = _Call()
    c.p.n_records = c.p.journal_bytes = 0
    c.p.sync_point = 0
    c.einval(b"sync_point")


# every destination and output array against every input and the outputs before it
MEETINGS = [(out, other) for k, out in enumerate(OUTPUTS)
            for other in list(INPUTS) + list(OUTPUTS)[:k]]


@pytest.mark.parametrize("where", ["inside", "tail_in", "head_in"])
@pytest.mark.parametrize("out,other", MEETINGS)
def test_output_meeting_an_input_or_another_output_is_einval(out, other, where):
    c = _Call()
    lo, size = c.at[other], dict(INPUTS, **OUTPUTS)[other]
    mine = OUTPUTS[out]
    # (8 keeps dst's alignment; the overlap is then 8 bytes)
    at = {"inside": lo, "tail_in": lo - mine + 8, "head_in": lo + size - 8}[where]
    setattr(c.p, out, at)
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"overlaps" in err, (rc, err)
    assert out.encode() in err and other.encode() in err, err


def test_adjacent_arrays_and_null_optionals_reach_the_device_lookup():
    c = _Call()
    c.p.dst = c.at["journal"] + 60 * RECORDS            # begins where the journal ends
    c.p.new_index = c.at["data"] - 4 * RECORDS          # ends where the DATA window begins
    c.p.out = c.p.dst + 512                             # begins where dst ends
    c.passes()
    c = _Call()
    c.p.keep = c.p.new_index = c.p.out = None
    c.passes()


@pytest.mark.parametrize("flags", [N.BMQCRC_F_DEVICE_PTRS,
                                   N.BMQCRC_F_DEVICE_PTRS | N.BMQCRC_F_ASYNC])
def test_valid_arguments_reach_the_device_lookup(flags):
    _Call().passes(flags, seg_bytes=12345, max_len=7, min_len=9)
    r = N.RolloverResult()
    rc = N.lib.bmqcrc_last_rollover(-1, None, ctypes.byref(r))
    assert rc == (N.BMQCRC_ENODEV if NO_GPU else 0)
    if not NO_GPU:
        assert r.as_dict() == dict.fromkeys((f[0] for f in N.RolloverResult._fields_
                                             if f[0] != "reserved"), 0)


# ---- the Python wrapper ------------------------------------------------------

def test_python_refuses_wrong_types():
    j, d = torch.zeros(120, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8)
    kw = dict(data_file_pos=0, new_data_file_pos=40)
    with pytest.raises(TypeError, match="journal"):
        rollover_records(j.to(torch.int8), d, **kw)
    with pytest.raises(TypeError, match="journal"):
        rollover_records(torch.zeros(240, dtype=torch.uint8)[::2], d, **kw)
    with pytest.raises(TypeError, match="data"):
        rollover_records(j, bytes(64), **kw)
    with pytest.raises(TypeError, match="keep"):
        rollover_records(j, d, keep=[1, 1], **kw)
    with pytest.raises(TypeError, match="dst"):
        rollover_records(j, d, dst=torch.zeros(512, dtype=torch.int8), **kw)
    with pytest.raises(TypeError, match="journal_dst"):
        rollover_records(j, d, journal_dst=torch.zeros(512, dtype=torch.int32), **kw)
    with pytest.raises(TypeError):
        rollover_records(j, d)    # the two positions are required


def test_python_refuses_host_tensors():
    j, d = torch.zeros(120, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8)
    kw = dict(data_file_pos=0, new_data_file_pos=40)
    with pytest.raises(TypeError, match="device tensors only"):
        rollover_records(j, d, **kw)
    with pytest.raises(TypeError, match="device tensors only"):
        rollover_records(j, d, sync=False, **kw)
