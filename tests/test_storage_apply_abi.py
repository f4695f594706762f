"""ABI 2.15: bmqcrc_storage_event_apply and bmqcrc_last_storage_apply, as far as
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
from blazingmq_amd import _native as N, apply_events, last_storage_apply  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "blazingmq_amd", "lib", "libbmqcrc.so")
NEW = {"bmqcrc_storage_event_apply", "bmqcrc_last_storage_apply"}
HEADERS = ("bmqcrc.h", "bmqcrc_protocol.h")
NO_GPU = N.lib.bmqcrc_device_count() == 0
KINDS = ("OK", "EVENT_OFFSETS", "EVENT_HEADER", "STORAGE_HEADER", "DATA_RECORD",
         "TOO_MANY_MESSAGES", "OUT_OF_SYNC", "DST_TOO_SMALL", "TOO_MANY_PIECES")
OUTPUTS = (("types", 1), ("flags", 1), ("payload_offsets", 8), ("payload_lengths", 4),
           ("record_offsets", 8), ("lengths", 4), ("expected", 4), ("out", 4), ("event_first", 8))
REGIONS = ("events", "journal_dst", "data_dst")


def _declared():
    src = ""
    for h in HEADERS:
        with open(os.path.join(ROOT, "include", h)) as f:
            src += f.read()
    return set(re.findall(r"^\w[\w\s\*]*?\b(bmqcrc_\w+)\s*\(", src, re.M))


class _Call:
    """A valid call over two events on host addresses: it only ever reaches
    the argument checks (a machine with a GPU is handed n_events = 0 where it
    would pass)."""
    CAP = 4

    def __init__(self):
        self.buf = (ctypes.c_uint8 * 4096)()
        base = ctypes.addressof(self.buf)
        base += -base % 8
        self.base = base
        self.offs = (ctypes.c_uint64 * 3)(0, 8, 16)
        self.arr = {name: (ctypes.c_uint64 * (2 * self.CAP + 2))() for name, _ in OUTPUTS}
        p = N.StorageApply()
        p.struct_size = ctypes.sizeof(N.StorageApply)
        p.events, p.events_bytes = base + 256, 256
        p.event_offsets, p.n_events, p.msg_cap = ctypes.addressof(self.offs), 2, self.CAP
        p.partition_id, p.lease_id, p.seq = 3, 1, 9
        p.journal_pos, p.data_file_pos = 44, 40
        p.journal_dst, p.journal_dst_bytes = base + 1024, 256
        p.data_dst, p.data_dst_bytes = base + 2048, 256
        for name, a in self.arr.items():
            setattr(p, name, ctypes.addressof(a))
        self.p = p

    def run(self, flags=N.BMQCRC_F_DEVICE_PTRS, opts="make", **kw):
        o = N.make_opts(flags=flags, **kw) if opts == "make" else opts
        r = N.StorageApplyResult()
        rc = N.lib.bmqcrc_storage_event_apply(ctypes.byref(self.p), ctypes.byref(r),
                                              ctypes.byref(o) if o is not None else None)
        return rc, N.lib.bmqcrc_last_error()

    def passes(self, flags=N.BMQCRC_F_DEVICE_PTRS, **kw):
        if not NO_GPU:
            self.p.n_events = 0
        rc, err = self.run(flags, **kw)
        assert rc == (N.BMQCRC_ENODEV if NO_GPU else 0), (rc, err)


def test_header_declares_both_names_and_the_kinds():
    text = open(os.path.join(ROOT, "include", "bmqcrc_protocol.h")).read()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, text, re.M), name
    for value, kind in enumerate(KINDS):
        assert re.search(r"#define BMQCRC_STORAGE_APPLY_%s %d\b" % (kind, value), text), kind
    assert text.index("ABI 2.14") < text.index("ABI 2.15")
    main = open(os.path.join(ROOT, "include", "bmqcrc.h")).read()
    assert re.search(r"\(2\.15\) bmqcrc_storage_event_apply, bmqcrc_last_storage_apply", main)


def test_library_exports_both_names_and_nothing_undeclared():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    assert NEW <= exported
    assert set(n for n in exported if n.startswith("bmqcrc_")) == _declared()


def test_version_is_2_15():
    v = N.lib.bmqcrc_version()
    assert v >> 16 == 2 and v & 0xffff >= 15


def test_kind_constants_and_package_exports():
    for value, kind in enumerate(KINDS):
        assert getattr(N, "BMQCRC_STORAGE_APPLY_" + kind) == value
    assert {"StorageEventBuilder", "StorageMessageIterator", "apply_events",
            "last_storage_apply"} <= set(blazingmq_amd.__all__)


@pytest.mark.parametrize("struct,ctype,size", [
    ("bmqcrc_storage_apply", N.StorageApply, 184),
    ("bmqcrc_storage_apply_result", N.StorageApplyResult, 96)])
def test_struct_layouts_match_the_header(tmp_path, struct, ctype, size):
    fields = [f[0] for f in ctype._fields_]
    src = tmp_path / "apply.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bmqcrc_protocol.h"\n'
                   'int main(void) { printf("%%zu", sizeof(%s));\n' % struct +
                   "".join('printf(" %%zu", offsetof(%s, %s));\n' % (struct, f) for f in fields) +
                   "".join('printf(" %%d", BMQCRC_STORAGE_APPLY_%s);\n' % k for k in KINDS) +
                   'return 0; }\n')
    exe = tmp_path / "apply"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert got == [ctypes.sizeof(ctype)] + [getattr(ctype, f).offset for f in fields] + [
        getattr(N, "BMQCRC_STORAGE_APPLY_" + k) for k in KINDS]
    assert got[0] == size and got[-9:] == list(range(9))


@pytest.mark.parametrize("flag,name", [
    (N.BMQCRC_F_WHOLE_MESSAGES, b"WHOLE_MESSAGES"), (N.BMQCRC_F_PLAN, b"PLAN"),
    (N.BMQCRC_F_TIME_KERNEL, b"TIME_KERNEL"), (N.BMQCRC_F_OFFSETS32, b"OFFSETS32")])
def test_other_flags_are_einval_naming_the_flag(flag, name):
    for extra in (0, N.BMQCRC_F_ASYNC):
        rc, err = _Call().run(N.BMQCRC_F_DEVICE_PTRS | extra | flag)
        assert rc == N.BMQCRC_EINVAL and name in err, (rc, err)
        assert b"bmqcrc_storage_event_apply" in err, err


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
    assert N.lib.bmqcrc_storage_event_apply(None, None, None) == N.BMQCRC_EINVAL


@pytest.mark.parametrize("name", REGIONS)
def test_null_required_pointer_is_einval_naming_it(name):
    c = _Call()
    setattr(c.p, name, None)
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"null" in err and err.endswith(b": " + name.encode()), err


@pytest.mark.parametrize("name,shifts,words", [
    ("events", (1, 2, 3), b"events must be 4-byte aligned"),
    ("journal_dst", (1, 2, 3), b"journal_dst must be 4-byte aligned"),
    ("data_dst", (1, 2, 4, 7), b"data_dst must be 8-byte aligned")])
def test_misaligned_pointer_is_einval(name, shifts, words):
    for shift in shifts:
        c = _Call()
        setattr(c.p, name, getattr(c.p, name) + shift)
        rc, err = c.run()
        assert rc == N.BMQCRC_EINVAL and words in err, (rc, err)


def test_null_event_offsets_means_one_event():
    for n in (0, 2):
        c = _Call()
        c.p.event_offsets, c.p.n_events = None, n
        rc, err = c.run()
        assert rc == N.BMQCRC_EINVAL and b"n_events must be 1" in err, (rc, err)


@pytest.mark.parametrize("name", ["n_events", "msg_cap"])
def test_counts_at_2_to_the_32_are_einval(name):
    c = _Call()
    setattr(c.p, name, 1 << 32)
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"2^32" in err, (rc, err)


@pytest.mark.parametrize("pos", [0, 1, 2, 46, (1 << 35) + 2])
def test_journal_pos_must_be_a_multiple_of_4_and_not_0(pos):
    c = _Call()
    c.p.journal_pos = pos
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"journal_pos" in err and b"multiple of 4" in err, err


@pytest.mark.parametrize("pos", [0, 1, 4, 44, (1 << 35) + 4])
def test_data_file_pos_must_be_a_multiple_of_8_and_not_0(pos):
    c = _Call()
    c.p.data_file_pos = pos
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"data_file_pos" in err and b"multiple of 8" in err, err


def test_partition_id_and_write_head():
    c = _Call()
    c.p.partition_id = 65536
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"partition_id" in err and b"65535" in err, (rc, err)
    c = _Call()
    c.p.lease_id, c.p.seq = 0, 1
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"lease_id == 0" in err and b"seq" in err, (rc, err)
    c = _Call()
    c.p.partition_id, c.p.lease_id, c.p.seq = 65535, 0, 0
    c.passes()


# every output array against the three regions, and the two destinations against
# the events and each other (the pair is named data_dst first)
MEETINGS = [(name, elem, region) for name, elem in OUTPUTS for region in REGIONS] + [
    ("journal_dst", 0, "events"), ("data_dst", 0, "events"), ("data_dst", 0, "journal_dst")]


@pytest.mark.parametrize("where", ["inside", "tail_in", "head_in"])
@pytest.mark.parametrize("name,elem,region", MEETINGS)
def test_output_meeting_an_input_or_a_destination_is_einval(name, elem, region, where):
    c = _Call()
    lo = {"events": c.base + 256, "journal_dst": c.base + 1024, "data_dst": c.base + 2048}[region]
    # record_offsets has msg_cap + 1 entries, event_first n_events + 1, a destination 256 bytes
    size = {"record_offsets": 8 * (c.CAP + 1), "event_first": 8 * 3}.get(name, elem * c.CAP or 256)
    at = {"inside": lo + 64, "tail_in": lo - size + 8, "head_in": lo + 248}[where]
    setattr(c.p, name, at)
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"overlaps" in err and name.encode() in err, (rc, err)
    assert (b"[%s, " % region.encode()) in err, err


def test_adjacent_arrays_reach_the_device_lookup():
    c = _Call()
    c.p.journal_dst = c.base + 512                     # begins where the events end
    c.p.data_dst = c.base + 768                        # begins where the journal ends
    c.p.payload_offsets = c.base + 256 - 8 * c.CAP     # ends where the events begin
    c.p.record_offsets = c.base + 1024                 # begins where the DATA window ends
    c.p.types = c.base + 1024 + 8 * (c.CAP + 1)
    c.passes()


@pytest.mark.parametrize("flags", [N.BMQCRC_F_DEVICE_PTRS,
                                   N.BMQCRC_F_DEVICE_PTRS | N.BMQCRC_F_ASYNC])
@pytest.mark.parametrize("optional", [True, False])
def test_valid_arguments_reach_the_device_lookup(flags, optional):
    c = _Call()
    if not optional:
        for name, _ in OUTPUTS:
            setattr(c.p, name, None)
    c.passes(flags, seg_bytes=12345, max_len=7, min_len=9)
    r = N.StorageApplyResult()
    rc = N.lib.bmqcrc_last_storage_apply(-1, None, ctypes.byref(r))
    assert rc == (N.BMQCRC_ENODEV if NO_GPU else 0)
    if not NO_GPU:
        want = dict.fromkeys((f[0] for f in N.StorageApplyResult._fields_), 0)
        assert r.as_dict() == dict(want, head_lease_id=1, head_seq=9)


# ---- the Python wrapper ------------------------------------------------------

def test_python_refuses_wrong_types():
    ev = torch.zeros(160, dtype=torch.uint8)
    kw = dict(partition_id=0, journal_pos=44, data_file_pos=40)
    with pytest.raises(TypeError, match="events"):
        apply_events(ev.to(torch.int8), **kw)
    with pytest.raises(TypeError, match="events"):
        apply_events(torch.zeros(320, dtype=torch.uint8)[::2], **kw)
    with pytest.raises(TypeError, match="events"):
        apply_events(bytes(160), **kw)
    with pytest.raises(TypeError, match="event_offsets"):
        apply_events(ev, torch.zeros(2, dtype=torch.int32), **kw)
    with pytest.raises(TypeError, match="journal_dst"):
        apply_events(ev, journal_dst=torch.zeros(60, dtype=torch.int8), **kw)
    with pytest.raises(TypeError, match="data_dst"):
        apply_events(ev, data_dst=[0] * 64, **kw)
    with pytest.raises(TypeError):
        apply_events(ev)    # the replica's state is required


def test_python_refuses_host_tensors_and_a_missing_destination():
    ev = torch.zeros(160, dtype=torch.uint8)
    kw = dict(partition_id=0, journal_pos=44, data_file_pos=40)
    with pytest.raises(TypeError, match="device tensors only"):
        apply_events(ev, **kw)
    with pytest.raises(TypeError, match="device tensors only"):
        apply_events(ev, torch.zeros(2, dtype=torch.int64), sync=False, **kw)
