"""ABI 2.14: bmqcrc_journal_select and bmqcrc_last_journal_select, as far as
they answer without a GPU -- the declarations, the exports, the struct layouts,
the argument checks that sit in front of the device lookup, and the Python
wrapper's refusals."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from blazingmq_amd import _native as N, last_journal_select, select_records  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "blazingmq_amd", "lib", "libbmqcrc.so")
NEW = {"bmqcrc_journal_select", "bmqcrc_last_journal_select"}
HEADERS = ("bmqcrc.h", "bmqcrc_protocol.h")
NO_GPU = N.lib.bmqcrc_device_count() == 0
CALL = b"bmqcrc_journal_select"


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

    def __init__(self):
        self.jour = (ctypes.c_uint32 * 32)()    # 128 bytes: two records and a tail
        self.keys = (ctypes.c_uint8 * 10)()
        self.sel = (ctypes.c_uint8 * 8)()
        p = N.JournalSelect()
        p.struct_size = ctypes.sizeof(N.JournalSelect)
        p.journal, p.journal_bytes, p.n_records = ctypes.addressof(self.jour), 120, 2
        p.data_file_bytes, p.with_csl = 4096, 1
        p.queue_keys, p.n_queue_keys, p.queue_cap = ctypes.addressof(self.keys), 2, 16
        p.select = ctypes.addressof(self.sel)
        self.p = p

    def empty(self):
        self.p.n_records = self.p.journal_bytes = 0

    def run(self, flags=N.BMQCRC_F_DEVICE_PTRS, opts="make", **kw):
        o = N.make_opts(flags=flags, **kw) if opts == "make" else opts
        r = N.JournalSelectResult()
        rc = N.lib.bmqcrc_journal_select(ctypes.byref(self.p), ctypes.byref(r),
                                         ctypes.byref(o) if o is not None else None)
        return rc, N.lib.bmqcrc_last_error()


def test_header_declares_both_names_and_says_what_is_not_checked():
    text = open(os.path.join(ROOT, "include", "bmqcrc_protocol.h")).read()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, text, re.M), name
    assert re.search(r"#define BMQCRC_JSEL_OK 0\b", text)
    assert re.search(r"#define BMQCRC_JSEL_TOO_MANY_QUEUES 1\b", text)
    assert text.index("ABI 2.13") < text.index("ABI 2.14")
    section = text[text.index("ABI 2.14.  The selection"):]
    for words in ("no DATA byte is read", "BMQCRC_RECOVERY_INVALID_DATA_RECORD (-17) is never raised",
                  "BMQCRC_REC_UNPACK_DATA_RECORD", "made as if", "bmqcrc_journal_bounds"):
        assert words in re.sub(r"\s*\n \*\s*", " ", section), words
    # the records unpack's comment points at the call that now makes its "not restated" list
    unpack = text[text.index("ABI 2.13.  The inverse"):text.index("#define BMQCRC_REC_UNPACK_OK")]
    assert "bmqcrc_journal_select" in unpack
    main = open(os.path.join(ROOT, "include", "bmqcrc.h")).read()
    assert "(2.13)" in main and "(2.14)" in main
    assert re.search(r"\(2\.14\) bmqcrc_journal_select, bmqcrc_last_journal_select", main)


def test_library_exports_both_names_and_nothing_undeclared():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    assert NEW <= exported
    assert set(n for n in exported if n.startswith("bmqcrc_")) == _declared()


def test_version_is_2_14():
    v = N.lib.bmqcrc_version()
    assert v >> 16 == 2 and v & 0xffff >= 14


def test_constants_and_python_names():
    import blazingmq_amd
    assert (N.BMQCRC_JSEL_OK, N.BMQCRC_JSEL_TOO_MANY_QUEUES) == (0, 1)
    assert {"select_records", "last_journal_select"} <= set(blazingmq_amd.__all__)


@pytest.mark.parametrize("struct,ctype,size", [
    ("bmqcrc_journal_select_args", N.JournalSelect, 80),
    ("bmqcrc_journal_select_result", N.JournalSelectResult, 56)])
def test_struct_layouts_match_the_header(tmp_path, struct, ctype, size):
    fields = [f[0] for f in ctype._fields_]
    src = tmp_path / "jsel.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bmqcrc_protocol.h"\n'
                   'int main(void) { printf("%%zu", sizeof(%s));\n' % struct +
                   "".join('printf(" %%zu", offsetof(%s, %s));\n' % (struct, f) for f in fields) +
                   'printf(" %d %d", BMQCRC_JSEL_OK, BMQCRC_JSEL_TOO_MANY_QUEUES);\n'
                   'return 0; }\n')
    exe = tmp_path / "jsel"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert got == [ctypes.sizeof(ctype)] + [getattr(ctype, f).offset for f in fields] + [0, 1]
    assert got[0] == size


@pytest.mark.parametrize("flag,name", [
    (N.BMQCRC_F_WHOLE_MESSAGES, b"WHOLE_MESSAGES"), (N.BMQCRC_F_PLAN, b"PLAN"),
    (N.BMQCRC_F_TIME_KERNEL, b"TIME_KERNEL"), (N.BMQCRC_F_OFFSETS32, b"OFFSETS32")])
def test_other_flags_are_einval_naming_the_flag(flag, name):
    for extra in (0, N.BMQCRC_F_ASYNC):
        rc, err = _Call().run(N.BMQCRC_F_DEVICE_PTRS | extra | flag)
        assert rc == N.BMQCRC_EINVAL and name in err and CALL in err, (rc, err)


def test_unknown_flag_bits_are_einval():
    rc, err = _Call().run(N.BMQCRC_F_DEVICE_PTRS | 0x4000)
    assert rc == N.BMQCRC_EINVAL and b"unknown" in err, (rc, err)


@pytest.mark.parametrize("opts", [None, "plain", "async"])
def test_missing_device_ptrs_is_einval(opts):
    c = _Call()
    rc, err = c.run(opts=None) if opts is None else c.run(
        N.BMQCRC_F_ASYNC if opts == "async" else 0)
    assert rc == N.BMQCRC_EINVAL and b"DEVICE_PTRS" in err and CALL in err, (rc, err)


def test_more_than_one_device_is_einval():
    rc, err = _Call().run(devices=[0, 1])
    assert rc == N.BMQCRC_EINVAL and b"ndevices" in err and CALL in err, (rc, err)


def test_struct_size_and_reserved_fields():
    c = _Call()
    c.p.struct_size -= 8
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"struct_size" in err and CALL in err, (rc, err)
    for field in ("reserved", "reserved2"):
        c = _Call()
        setattr(c.p, field, 1)
        rc, err = c.run()
        assert rc == N.BMQCRC_EINVAL and field.encode() in err and CALL in err, (rc, err)
    assert N.lib.bmqcrc_journal_select(None, None, None) == N.BMQCRC_EINVAL


@pytest.mark.parametrize("name", ["journal", "select", "queue_keys"])
def test_null_required_array_is_einval_naming_it(name):
    c = _Call()
    setattr(c.p, name, None)
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"null" in err and CALL in err, err
    assert err.endswith(b": " + name.encode()), err


def test_null_queue_keys_with_no_keys_reaches_the_device_lookup():
    c = _Call()
    c.p.queue_keys, c.p.n_queue_keys = None, 0
    if not NO_GPU:
        c.empty()
    rc, err = c.run()
    assert rc == (N.BMQCRC_ENODEV if NO_GPU else 0), (rc, err)


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_misaligned_journal_is_einval(shift):
    c = _Call()
    c.p.journal = ctypes.addressof(c.jour) + shift
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"journal must be 4-byte aligned" in err and CALL in err, err


@pytest.mark.parametrize("nbytes", [0, 60, 119, 121, 128, 180])
def test_journal_bytes_must_be_60_n(nbytes):
    c = _Call()
    c.p.journal_bytes = nbytes
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"journal_bytes" in err and CALL in err, (rc, err)


def test_n_records_at_2_to_the_32_is_einval():
    c = _Call()
    c.p.n_records, c.p.journal_bytes = 1 << 32, 60 << 32
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"n_records" in err and b"2^32" in err and CALL in err, err


def test_queue_cap_zero_is_einval():
    c = _Call()
    c.p.queue_cap = 0
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"queue_cap" in err and CALL in err, (rc, err)


@pytest.mark.parametrize("flags", [N.BMQCRC_F_DEVICE_PTRS,
                                   N.BMQCRC_F_DEVICE_PTRS | N.BMQCRC_F_ASYNC])
def test_valid_arguments_reach_the_device_lookup(flags):
    c = _Call()
    if not NO_GPU:
        c.empty()
    rc, err = c.run(flags, seg_bytes=12345, max_len=7, min_len=9)
    assert rc == (N.BMQCRC_ENODEV if NO_GPU else 0), (rc, err)
    r = N.JournalSelectResult()
    rc = N.lib.bmqcrc_last_journal_select(-1, None, ctypes.byref(r))
    assert rc == (N.BMQCRC_ENODEV if NO_GPU else 0)
    if not NO_GPU:
        assert r.as_dict() == dict(n_records=0, first_record=0, n_selected=0, n_deleted=0,
                                   n_purged=0, error_record=0, recovery_rc=0, refused_kind=0)


# ---- the Python wrapper ------------------------------------------------------

def test_python_refuses_wrong_types():
    j = torch.zeros(120, dtype=torch.uint8)
    with pytest.raises(TypeError, match="journal"):
        select_records(j.to(torch.int8), data_file_bytes=64)
    with pytest.raises(TypeError, match="journal"):
        select_records(torch.zeros(240, dtype=torch.uint8)[::2], data_file_bytes=64)
    with pytest.raises(TypeError, match="journal"):
        select_records(bytes(120), data_file_bytes=64)


def test_python_refuses_host_tensors():
    with pytest.raises(TypeError, match="device tensors only"):
        select_records(torch.zeros(120, dtype=torch.uint8), data_file_bytes=64)
