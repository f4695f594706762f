"""ABI 2.17: bmqcrc_push_event_pack and bmqcrc_last_push_pack, as far as they
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
from blazingmq_amd import _native as N, last_push_pack, pack_push_events  # noqa: F401
from blazingmq_amd import push_event as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "blazingmq_amd", "lib", "libbmqcrc.so")
NEW = {"bmqcrc_push_event_pack", "bmqcrc_last_push_pack"}
HEADERS = ("bmqcrc.h", "bmqcrc_protocol.h")
NO_GPU = N.lib.bmqcrc_device_count() == 0
KINDS = ("OK", "RECORD_INDEX", "RECORD", "DATA_OFFSET", "DATA_RECORD", "FLAGS", "EVENT_FIRST",
         "PAYLOAD_TOO_BIG", "EVENT_TOO_BIG", "DST_TOO_SMALL", "TOO_MANY_PIECES")
MODES = ("NONE", "PACKED_RDA", "SUB_QUEUE_ID", "SUB_QUEUE_INFO")
RECORDS, MSGS, EVENTS = 4, 8, 2
# name -> bytes of a valid call's array (option mode 3 uses every one)
INPUTS = {"journal": 60 * RECORDS, "data": 256, "records": 4 * MSGS, "queue_ids": 4 * MSGS,
          "flags": MSGS, "rda": MSGS, "sub_ids": 4 * MSGS, "event_first": 8 * (EVENTS + 1)}
OUTPUTS = {"dst": 512, "event_offsets": 8 * (EVENTS + 1), "out": 4 * MSGS, "lengths": 4 * MSGS}


def _declared():
    src = ""
    for h in HEADERS:
        with open(os.path.join(ROOT, "include", h)) as f:
            src += f.read()
    return set(re.findall(r"^\w[\w\s\*]*?\b(bmqcrc_\w+)\s*\(", src, re.M))


class _Call:
    """A valid call over eight messages from four records in two events on host
    addresses: it only ever reaches the argument checks (a machine with a GPU
    is handed n = 0 where it would pass)."""

    def __init__(self):
        self.buf = (ctypes.c_uint8 * 16384)()
        base = ctypes.addressof(self.buf)
        base += -base % 8
        self.base = base
        # 1 KiB apart, in this order
        self.at = {name: base + 1024 * (k + 1)
                   for k, name in enumerate(list(INPUTS) + list(OUTPUTS))}
        p = N.PushPack()
        p.struct_size = ctypes.sizeof(N.PushPack)
        for name, where in self.at.items():
            setattr(p, name, where)
        p.journal_bytes, p.n_records, p.n = 60 * RECORDS, RECORDS, MSGS
        p.data_bytes, p.data_file_pos = 256, 40
        p.option_mode = 3
        p.n_events, p.dst_bytes = EVENTS, 512
        self.p = p

    def run(self, flags=N.BMQCRC_F_DEVICE_PTRS, opts="make", **kw):
        o = N.make_opts(flags=flags, **kw) if opts == "make" else opts
        r = N.PushPackResult()
        rc = N.lib.bmqcrc_push_event_pack(ctypes.byref(self.p), ctypes.byref(r),
                                          ctypes.byref(o) if o is not None else None)
        return rc, N.lib.bmqcrc_last_error()

    def passes(self, flags=N.BMQCRC_F_DEVICE_PTRS, **kw):
        if not NO_GPU:
            self.p.n = 0
            if not self.p.records:
                self.p.n_records = self.p.journal_bytes = 0
        rc, err = self.run(flags, **kw)
        assert rc == (N.BMQCRC_ENODEV if NO_GPU else 0), (rc, err)

    def einval(self, *words):
        rc, err = self.run()
        assert rc == N.BMQCRC_EINVAL, (rc, err)
        for w in words:
            assert w in err, (w, err)


def test_header_declares_both_names_the_kinds_and_the_modes():
    text = open(os.path.join(ROOT, "include", "bmqcrc_protocol.h")).read()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, text, re.M), name
    for value, kind in enumerate(KINDS):
        assert re.search(r"#define BMQCRC_PUSH_PACK_%s %d\b" % (kind, value), text), kind
    for value, mode in enumerate(MODES):
        assert re.search(r"#define BMQCRC_PUSH_OPTION_%s %d\b" % (mode, value), text), mode
    assert text.index("ABI 2.16") < text.index("ABI 2.17")
    main = open(os.path.join(ROOT, "include", "bmqcrc.h")).read()
    assert re.search(r"\(2\.17\) bmqcrc_push_event_pack, bmqcrc_last_push_pack", main)


def test_library_exports_both_names_and_nothing_undeclared():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    assert NEW <= exported
    assert set(n for n in exported if n.startswith("bmqcrc_")) == _declared()


def test_version_is_2_17():
    v = N.lib.bmqcrc_version()
    assert v >> 16 == 2 and v & 0xffff >= 17


def test_kind_constants_and_package_exports():
    for value, kind in enumerate(KINDS):
        assert getattr(N, "BMQCRC_PUSH_PACK_" + kind) == value
    for value, mode in enumerate(MODES):
        assert getattr(N, "BMQCRC_PUSH_OPTION_" + mode) == value
    assert (E.OPTION_NONE, E.OPTION_PACKED_RDA, E.OPTION_SUB_QUEUE_ID,
            E.OPTION_SUB_QUEUE_INFO) == (0, 1, 2, 3)
    assert E.PACK_REFUSALS == KINDS
    names = {"pack_push_events", "last_push_pack", "PushEventBuilder", "PushMessageIterator"}
    assert names <= set(blazingmq_amd.__all__)
    for name in names:
        assert getattr(blazingmq_amd, name) is getattr(E, name)


@pytest.mark.parametrize("struct,ctype,size", [
    ("bmqcrc_push_pack", N.PushPack, 184),
    ("bmqcrc_push_pack_result", N.PushPackResult, 56)])
def test_struct_layouts_match_the_header(tmp_path, struct, ctype, size):
    fields = [f[0] for f in ctype._fields_]
    src = tmp_path / "pack.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bmqcrc_protocol.h"\n'
                   'int main(void) { printf("%%zu", sizeof(%s));\n' % struct +
                   "".join('printf(" %%zu", offsetof(%s, %s));\n' % (struct, f) for f in fields) +
                   "".join('printf(" %%d", BMQCRC_PUSH_PACK_%s);\n' % k for k in KINDS) +
                   'return 0; }\n')
    exe = tmp_path / "pack"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert got == [ctypes.sizeof(ctype)] + [getattr(ctype, f).offset for f in fields] + [
        getattr(N, "BMQCRC_PUSH_PACK_" + k) for k in KINDS]
    assert got[0] == size and got[-11:] == list(range(11))


@pytest.mark.parametrize("flag,name", [
    (N.BMQCRC_F_WHOLE_MESSAGES, b"WHOLE_MESSAGES"), (N.BMQCRC_F_PLAN, b"PLAN"),
    (N.BMQCRC_F_TIME_KERNEL, b"TIME_KERNEL"), (N.BMQCRC_F_OFFSETS32, b"OFFSETS32")])
def test_other_flags_are_einval_naming_the_flag(flag, name):
    for extra in (0, N.BMQCRC_F_ASYNC):
        rc, err = _Call().run(N.BMQCRC_F_DEVICE_PTRS | extra | flag)
        assert rc == N.BMQCRC_EINVAL and name in err, (rc, err)
        assert b"bmqcrc_push_event_pack" in err, err


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
    assert N.lib.bmqcrc_push_event_pack(None, None, None) == N.BMQCRC_EINVAL


@pytest.mark.parametrize("name", ["journal", "data", "queue_ids"])
def test_null_required_pointer_is_einval_naming_it(name):
    c = _Call()
    setattr(c.p, name, None)
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"null" in err and err.endswith(b": " + name.encode()), err


def test_null_dst_is_the_size_only_call_and_wants_dst_bytes_0():
    c = _Call()
    c.p.dst = None
    c.einval(b"dst == NULL", b"dst_bytes must be 0")
    c = _Call()
    c.p.dst, c.p.dst_bytes = None, 0
    c.passes()
    # and out and lengths may stay: a size-only call does not write them
    c = _Call()
    c.p.dst, c.p.dst_bytes, c.p.out, c.p.lengths = None, 0, None, None
    c.passes()


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


def test_message_counts():
    for n in (1 << 32, 1 << 40):
        c = _Call()
        c.p.n = n
        c.einval(b"n must be below 2^32")
    for n in (RECORDS - 1, RECORDS + 1, 0):
        c = _Call()
        c.p.records, c.p.n, c.p.n_events = None, n, 1
        c.einval(b"records == NULL", b"n must be n_records")
    c = _Call()
    c.p.records, c.p.n = None, RECORDS
    c.passes()


def test_event_counts():
    for n in (0, 2):
        c = _Call()
        c.p.event_first, c.p.n_events = None, n
        c.einval(b"n_events must be 1")
    for n in (0, MSGS + 1, 1 << 40):
        c = _Call()
        c.p.n_events = n
        c.einval(b"n_events must lie in [1, n]")
    c = _Call()
    c.p.event_first, c.p.n_events = None, 1
    c.passes()
    c = _Call()
    c.p.n_events = MSGS     # more events than records: the messages repeat them
    c.passes()


@pytest.mark.parametrize("pos", [1, 4, 44, (1 << 35) + 4])
def test_data_file_pos_must_be_a_multiple_of_8(pos):
    c = _Call()
    c.p.data_file_pos = pos
    c.einval(b"data_file_pos", b"multiple of 8")


def test_option_mode_and_its_arrays():
    for mode in (4, 5, 1 << 31):
        c = _Call()
        c.p.option_mode = mode
        c.einval(b"option_mode must be at most 3")
    for mode, rda, sub in ((0, 0, 0), (1, 1, 0), (2, 0, 1), (3, 1, 1)):
        for has_rda in (0, 1):
            for has_sub in (0, 1):
                c = _Call()
                c.p.option_mode = mode
                if not has_rda:
                    c.p.rda = None
                if not has_sub:
                    c.p.sub_ids = None
                if has_rda != rda:
                    c.einval(b"rda is required in option modes 1 and 3")
                elif has_sub != sub:
                    c.einval(b"sub_ids is required in option modes 2 and 3")
                else:
                    c.passes()


def test_caps_above_their_limits():
    c = _Call()
    c.p.max_event_bytes = 1 << 31
    c.einval(b"max_event_bytes", b"2^31-1")
    top = 4 * ((1 << 28) - 1) - 32 - 12 - 4
    c = _Call()
    c.p.max_payload_bytes = top + 1
    c.einval(b"max_payload_bytes", b"MessageWords")
    c = _Call()
    c.p.max_event_bytes, c.p.max_payload_bytes = (1 << 31) - 1, top
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
    c.p.lengths = c.at["data"] - 4 * MSGS             # ends where the DATA window begins
    c.p.out = c.p.dst + 512                           # begins where dst ends
    c.passes()
    c = _Call()
    c.p.flags = c.p.event_offsets = c.p.out = c.p.lengths = None
    c.passes()


@pytest.mark.parametrize("flags", [N.BMQCRC_F_DEVICE_PTRS,
                                   N.BMQCRC_F_DEVICE_PTRS | N.BMQCRC_F_ASYNC])
def test_valid_arguments_reach_the_device_lookup(flags):
    _Call().passes(flags, seg_bytes=12345, max_len=7, min_len=9)
    r = N.PushPackResult()
    rc = N.lib.bmqcrc_last_push_pack(-1, None, ctypes.byref(r))
    assert rc == (N.BMQCRC_ENODEV if NO_GPU else 0)
    if not NO_GPU:
        assert r.as_dict() == dict.fromkeys((f[0] for f in N.PushPackResult._fields_
                                             if f[0] != "reserved"), 0)


# ---- the Python wrapper ------------------------------------------------------

def test_python_refuses_wrong_types():
    j, d = torch.zeros(120, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8)
    q = torch.zeros(2, dtype=torch.int32)
    kw = dict(data_file_pos=0, queue_ids=q)
    with pytest.raises(TypeError, match="journal_run"):
        pack_push_events(j.to(torch.int8), d, **kw)
    with pytest.raises(TypeError, match="journal_run"):
        pack_push_events(torch.zeros(240, dtype=torch.uint8)[::2], d, **kw)
    with pytest.raises(TypeError, match="data"):
        pack_push_events(j, bytes(64), **kw)
    with pytest.raises(TypeError, match="queue_ids"):
        pack_push_events(j, d, data_file_pos=0, queue_ids=q.to(torch.int64))
    with pytest.raises(TypeError, match="records"):
        pack_push_events(j, d, records=torch.zeros(2, dtype=torch.int64), **kw)
    with pytest.raises(TypeError, match="event_first"):
        pack_push_events(j, d, event_first=torch.zeros(2, dtype=torch.int32), **kw)
    with pytest.raises(TypeError, match="flags"):
        pack_push_events(j, d, flags=[0, 0], **kw)
    with pytest.raises(TypeError, match="rda"):
        pack_push_events(j, d, option_mode=1, rda=q, **kw)
    with pytest.raises(TypeError, match="sub_ids"):
        pack_push_events(j, d, option_mode=2, sub_ids=torch.zeros(2, dtype=torch.uint8), **kw)
    with pytest.raises(TypeError, match="dst"):
        pack_push_events(j, d, dst=torch.zeros(512, dtype=torch.int8), **kw)
    with pytest.raises(TypeError):
        pack_push_events(j, d)    # the position and the queue ids are required


def test_python_refuses_host_tensors():
    j, d = torch.zeros(120, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8)
    kw = dict(data_file_pos=0, queue_ids=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(TypeError, match="device tensors only"):
        pack_push_events(j, d, **kw)
    with pytest.raises(TypeError, match="device tensors only"):
        pack_push_events(j, d, sync=False, **kw)
