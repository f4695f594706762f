"""ABI 2.16: bmqcrc_storage_event_pack and bmqcrc_last_storage_pack, as far as
they answer without a GPU -- the declarations, the exports, the struct
layouts, the argument checks that sit in front of the device lookup, and the
Python wrapper's refusals."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import blazingmq_amd
from blazingmq_amd import _native as N, last_storage_pack, pack_storage_events  # noqa: F401
from blazingmq_amd import storage_event as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "blazingmq_amd", "lib", "libbmqcrc.so")
NEW = {"bmqcrc_storage_event_pack", "bmqcrc_last_storage_pack"}
HEADERS = ("bmqcrc.h", "bmqcrc_protocol.h")
NO_GPU = N.lib.bmqcrc_device_count() == 0
KINDS = ("OK", "RECORD_HEADER", "DATA_OFFSET", "DATA_RECORD", "EVENT_FIRST", "PAYLOAD_TOO_BIG",
         "EVENT_TOO_BIG", "DST_TOO_SMALL", "TOO_MANY_PIECES")
RECORDS, EVENTS = 4, 2
# name -> bytes of a valid call's array
INPUTS = {"journal": 60 * RECORDS, "data": 256, "flags": RECORDS, "event_first": 8 * (EVENTS + 1)}
OUTPUTS = {"dst": 512, "event_offsets": 8 * (EVENTS + 1), "types": RECORDS, "out": 4 * RECORDS}


def _declared():
    src = ""
    for h in HEADERS:
        with open(os.path.join(ROOT, "include", h)) as f:
            src += f.read()
    return set(re.findall(r"^\w[\w\s\*]*?\b(bmqcrc_\w+)\s*\(", src, re.M))


class _Call:
    """A valid call over four records in two events on host addresses: it only
    ever reaches the argument checks (a machine with a GPU is handed
    n_records = 0 where it would pass)."""

    def __init__(self):
        self.buf = (ctypes.c_uint8 * 8192)()
        base = ctypes.addressof(self.buf)
        base += -base % 8
        self.base = base
        # 1 KiB apart, in this order
        self.at = {name: base + 1024 * (k + 1)
                   for k, name in enumerate(list(INPUTS) + list(OUTPUTS))}
        p = N.StoragePack()
        p.struct_size = ctypes.sizeof(N.StoragePack)
        for name, where in self.at.items():
            setattr(p, name, where)
        p.journal_bytes, p.n_records, p.journal_pos = 60 * RECORDS, RECORDS, 44
        p.data_bytes, p.data_file_pos = 256, 40
        p.partition_id, p.event_type, p.storage_protocol_version = 3, 8, 1
        p.n_events, p.dst_bytes = EVENTS, 512
        self.p = p

    def run(self, flags=N.BMQCRC_F_DEVICE_PTRS, opts="make", **kw):
        o = N.make_opts(flags=flags, **kw) if opts == "make" else opts
        r = N.StoragePackResult()
        rc = N.lib.bmqcrc_storage_event_pack(ctypes.byref(self.p), ctypes.byref(r),
                                             ctypes.byref(o) if o is not None else None)
        return rc, N.lib.bmqcrc_last_error()

    def passes(self, flags=N.BMQCRC_F_DEVICE_PTRS, **kw):
        if not NO_GPU:
            self.p.n_records = self.p.journal_bytes = 0
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
        assert re.search(r"#define BMQCRC_STORAGE_PACK_%s %d\b" % (kind, value), text), kind
    assert text.index("ABI 2.15") < text.index("ABI 2.16")
    main = open(os.path.join(ROOT, "include", "bmqcrc.h")).read()
    assert re.search(r"\(2\.16\) bmqcrc_storage_event_pack, bmqcrc_last_storage_pack", main)


def test_library_exports_both_names_and_nothing_undeclared():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    assert NEW <= exported
    assert set(n for n in exported if n.startswith("bmqcrc_")) == _declared()


def test_version_is_2_16():
    v = N.lib.bmqcrc_version()
    assert v >> 16 == 2 and v & 0xffff >= 16


def test_kind_constants_and_package_exports():
    for value, kind in enumerate(KINDS):
        assert getattr(N, "BMQCRC_STORAGE_PACK_" + kind) == value
    assert E.PACK_REFUSALS == KINDS
    assert {"pack_storage_events", "last_storage_pack"} <= set(blazingmq_amd.__all__)
    assert blazingmq_amd.pack_storage_events is E.pack_storage_events
    assert blazingmq_amd.last_storage_pack is E.last_storage_pack


@pytest.mark.parametrize("struct,ctype,size", [
    ("bmqcrc_storage_pack", N.StoragePack, 160),
    ("bmqcrc_storage_pack_result", N.StoragePackResult, 64)])
def test_struct_layouts_match_the_header(tmp_path, struct, ctype, size):
    fields = [f[0] for f in ctype._fields_]
    src = tmp_path / "pack.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bmqcrc_protocol.h"\n'
                   'int main(void) { printf("%%zu", sizeof(%s));\n' % struct +
                   "".join('printf(" %%zu", offsetof(%s, %s));\n' % (struct, f) for f in fields) +
                   "".join('printf(" %%d", BMQCRC_STORAGE_PACK_%s);\n' % k for k in KINDS) +
                   'return 0; }\n')
    exe = tmp_path / "pack"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert got == [ctypes.sizeof(ctype)] + [getattr(ctype, f).offset for f in fields] + [
        getattr(N, "BMQCRC_STORAGE_PACK_" + k) for k in KINDS]
    assert got[0] == size and got[-9:] == list(range(9))


@pytest.mark.parametrize("flag,name", [
    (N.BMQCRC_F_WHOLE_MESSAGES, b"WHOLE_MESSAGES"), (N.BMQCRC_F_PLAN, b"PLAN"),
    (N.BMQCRC_F_TIME_KERNEL, b"TIME_KERNEL"), (N.BMQCRC_F_OFFSETS32, b"OFFSETS32")])
def test_other_flags_are_einval_naming_the_flag(flag, name):
    for extra in (0, N.BMQCRC_F_ASYNC):
        rc, err = _Call().run(N.BMQCRC_F_DEVICE_PTRS | extra | flag)
        assert rc == N.BMQCRC_EINVAL and name in err, (rc, err)
        assert b"bmqcrc_storage_event_pack" in err, err


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
    assert N.lib.bmqcrc_storage_event_pack(None, None, None) == N.BMQCRC_EINVAL


@pytest.mark.parametrize("name", ["journal", "data", "dst"])
def test_null_required_pointer_is_einval_naming_it(name):
    c = _Call()
    setattr(c.p, name, None)
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"null" in err and err.endswith(b": " + name.encode()), err


@pytest.mark.parametrize("name,shifts,words", [
    ("journal", (1, 2, 3), b"journal must be 4-byte aligned"),
    ("dst", (1, 2, 3), b"dst must be 4-byte aligned"),
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


def test_event_counts():
    for n in (0, 2):
        c = _Call()
        c.p.event_first, c.p.n_events = None, n
        c.einval(b"n_events must be 1")
    for n in (0, RECORDS + 1, 1 << 40):
        c = _Call()
        c.p.n_events = n
        c.einval(b"n_events must lie in [1, n_records]")
    c = _Call()
    c.p.event_first, c.p.n_events = None, 1
    c.passes()


@pytest.mark.parametrize("pos", [0, 1, 2, 46, (1 << 33) + 2])
def test_journal_pos_must_be_a_multiple_of_4_and_not_0(pos):
    c = _Call()
    c.p.journal_pos = pos
    c.einval(b"journal_pos", b"multiple of 4")


def test_journal_offset_words_must_fit():
    top = 4 * ((1 << 32) - 1)
    for pos in (top - 60 * RECORDS + 4, top, top + 4, (1 << 64) - 4):
        c = _Call()
        c.p.journal_pos = pos
        c.einval(b"journal_pos + 60 n_records", b"JournalOffsetWords")
    c = _Call()
    c.p.journal_pos = top - 60 * RECORDS
    c.passes()


@pytest.mark.parametrize("pos", [1, 4, 44, (1 << 35) + 4])
def test_data_file_pos_must_be_a_multiple_of_8(pos):
    c = _Call()
    c.p.data_file_pos = pos
    c.einval(b"data_file_pos", b"multiple of 8")


def test_partition_id_event_type_and_protocol_version():
    c = _Call()
    c.p.partition_id = 65536
    c.einval(b"partition_id", b"65535")
    for t in (1, 2, 9, 11, 1 << 31):
        c = _Call()
        c.p.event_type = t
        c.einval(b"event_type")
    c = _Call()
    c.p.storage_protocol_version = 4
    c.einval(b"storage_protocol_version")
    for t in (0, 8, 10):
        c = _Call()
        c.p.partition_id, c.p.event_type, c.p.storage_protocol_version = 65535, t, 3
        c.p.data_file_pos = 0
        c.passes()


def test_caps_above_their_limits():
    c = _Call()
    c.p.max_event_bytes = 1 << 31
    c.einval(b"max_event_bytes", b"2^31-1")
    c = _Call()
    c.p.max_payload_bytes = 4 * ((1 << 27) - 1) - 12 + 1
    c.einval(b"max_payload_bytes", b"MessageWords")
    c = _Call()
    c.p.max_event_bytes, c.p.max_payload_bytes = (1 << 31) - 1, 4 * ((1 << 27) - 1) - 12
    c.passes()


# dst and every output array against every input, dst and the outputs before it
MEETINGS = [(out, other) for k, out in enumerate(OUTPUTS)
            for other in list(INPUTS) + list(OUTPUTS)[:k]]


@pytest.mark.parametrize("where", ["inside", "tail_in", "head_in"])
@pytest.mark.parametrize("out,other", MEETINGS)
def test_output_meeting_an_input_or_another_output_is_einval(out, other, where):
    c = _Call()
    lo, size = c.at[other], dict(INPUTS, **OUTPUTS)[other]
    mine = OUTPUTS[out]
    at = {"inside": lo, "tail_in": lo - mine + 4, "head_in": lo + size - 4}[where]
    setattr(c.p, out, at)
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"overlaps" in err, (rc, err)
    assert out.encode() in err and other.encode() in err, err


def test_adjacent_arrays_and_null_optionals_reach_the_device_lookup():
    c = _Call()
    c.p.dst = c.at["journal"] + 60 * RECORDS          # begins where the journal ends
    c.p.types = c.at["data"] - RECORDS                # ends where the DATA window begins
    c.p.out = c.p.dst + 512                           # begins where dst ends
    c.passes()
    c = _Call()
    c.p.flags = c.p.event_offsets = c.p.types = c.p.out = None
    c.passes()


@pytest.mark.parametrize("flags", [N.BMQCRC_F_DEVICE_PTRS,
                                   N.BMQCRC_F_DEVICE_PTRS | N.BMQCRC_F_ASYNC])
def test_valid_arguments_reach_the_device_lookup(flags):
    _Call().passes(flags, seg_bytes=12345, max_len=7, min_len=9)
    r = N.StoragePackResult()
    rc = N.lib.bmqcrc_last_storage_pack(-1, None, ctypes.byref(r))
    assert rc == (N.BMQCRC_ENODEV if NO_GPU else 0)
    if not NO_GPU:
        assert r.as_dict() == dict.fromkeys((f[0] for f in N.StoragePackResult._fields_
                                             if f[0] != "reserved"), 0)


# ---- the Python wrapper ------------------------------------------------------

def test_python_refuses_wrong_types():
    j, d = torch.zeros(120, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8)
    kw = dict(journal_pos=44, data_file_pos=0, partition_id=0)
    with pytest.raises(TypeError, match="journal_run"):
        pack_storage_events(j.to(torch.int8), d, **kw)
    with pytest.raises(TypeError, match="journal_run"):
        pack_storage_events(torch.zeros(240, dtype=torch.uint8)[::2], d, **kw)
    with pytest.raises(TypeError, match="data"):
        pack_storage_events(j, bytes(64), **kw)
    with pytest.raises(TypeError, match="event_first"):
        pack_storage_events(j, d, event_first=torch.zeros(2, dtype=torch.int32), **kw)
    with pytest.raises(TypeError, match="flags"):
        pack_storage_events(j, d, flags=[0, 0], **kw)
    with pytest.raises(TypeError, match="dst"):
        pack_storage_events(j, d, dst=torch.zeros(512, dtype=torch.int8), **kw)
    with pytest.raises(TypeError):
        pack_storage_events(j, d)    # the positions and the partition are required


def test_python_refuses_host_tensors():
    j, d = torch.zeros(120, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8)
    kw = dict(journal_pos=44, data_file_pos=0, partition_id=0)
    with pytest.raises(TypeError, match="device tensors only"):
        pack_storage_events(j, d, **kw)
    with pytest.raises(TypeError, match="device tensors only"):
        pack_storage_events(j, d, sync=False, **kw)
