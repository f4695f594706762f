"""ABI 2.20: bmqcrc_expire_records_pack and bmqcrc_last_expire_records, as far
as they answer without a GPU -- the declarations, the exports, the struct
layouts, the argument checks that sit in front of the device lookup, and the
Python wrapper's refusals."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import blazingmq_amd
from blazingmq_amd import _native as N, expire_records, last_expire_records  # noqa: F401
from blazingmq_amd import storage as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "blazingmq_amd", "lib", "libbmqcrc.so")
NEW = {"bmqcrc_expire_records_pack", "bmqcrc_last_expire_records"}
HEADERS = ("bmqcrc.h", "bmqcrc_protocol.h")
NO_GPU = N.lib.bmqcrc_device_count() == 0
KINDS = ("OK", "RECORD_HEADER", "DUPLICATE_MESSAGE", "QUEUE_KEY", "DST_TOO_SMALL")
RECORDS, QUEUES = 4, 8
# name -> bytes of a valid call's array (8 more than select holds, so that a
# neighbour placed against its end stays aligned)
INPUTS = {"journal": 60 * RECORDS, "select": 8, "queue_keys": 5 * QUEUES,
          "ttl_seconds": 8 * QUEUES}
OUTPUTS = {"journal_dst": 60 * RECORDS, "expired": RECORDS, "new_index": 4 * RECORDS,
           "select_out": RECORDS, "queue_expired": 4 * QUEUES, "queue_front": 4 * QUEUES}
# what the overlap check takes each array to hold
HELD = dict(INPUTS, select=RECORDS, **OUTPUTS)


def _declared():
    src = ""
    for h in HEADERS:
        with open(os.path.join(ROOT, "include", h)) as f:
            src += f.read()
    return set(re.findall(r"^\w[\w\s\*]*?\b(bmqcrc_\w+)\s*\(", src, re.M))


class _Call:
    """A valid call over four records and eight queues on host addresses: it
    only ever reaches the argument checks (a machine with a GPU is handed
    n_records = 0 where it would pass)."""

    def __init__(self):
        self.buf = (ctypes.c_uint8 * 16384)()
        base = ctypes.addressof(self.buf)
        base += -base % 8
        # 1 KiB apart, in this order
        self.at = {name: base + 1024 * (k + 1)
                   for k, name in enumerate(list(INPUTS) + list(OUTPUTS))}
        p = N.ExpirePack()
        p.struct_size = ctypes.sizeof(N.ExpirePack)
        for name, where in self.at.items():
            setattr(p, name, where)
        p.journal_bytes, p.n_records, p.n_queues = 60 * RECORDS, RECORDS, QUEUES
        p.now, p.first_seq, p.lease_id = 0x6720EAB4, 5, 3
        p.journal_dst_bytes = 60 * RECORDS
        self.p = p

    def run(self, flags=N.BMQCRC_F_DEVICE_PTRS, opts="make", **kw):
        o = N.make_opts(flags=flags, **kw) if opts == "make" else opts
        r = N.ExpirePackResult()
        rc = N.lib.bmqcrc_expire_records_pack(ctypes.byref(self.p), ctypes.byref(r),
                                              ctypes.byref(o) if o is not None else None)
        return rc, N.lib.bmqcrc_last_error(), r

    def passes(self, flags=N.BMQCRC_F_DEVICE_PTRS, **kw):
        if not NO_GPU:
            self.p.n_records, self.p.journal_bytes = 0, 0
        rc, err, r = self.run(flags, **kw)
        assert rc == (N.BMQCRC_ENODEV if NO_GPU else 0), (rc, err)
        return r

    def einval(self, *words):
        rc, err, _ = self.run()
        assert rc == N.BMQCRC_EINVAL, (rc, err)
        for w in words:
            assert w in err, (w, err)


def test_header_declares_both_names_and_the_kinds():
    text = open(os.path.join(ROOT, "include", "bmqcrc_protocol.h")).read()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, text, re.M), name
    for value, kind in enumerate(KINDS):
        assert re.search(r"#define BMQCRC_EXPIRE_PACK_%s %d\b" % (kind, value), text), kind
    assert text.index("ABI 2.19") < text.index("ABI 2.20")
    assert text.count("THIS CALL HAS NO CRC IN IT") == 2      # 2.19 and this one
    assert "e_NO_SC_QUORUM" in text[text.index("ABI 2.20"):]
    main = open(os.path.join(ROOT, "include", "bmqcrc.h")).read()
    assert re.search(r"\(2\.20\) bmqcrc_expire_records_pack, bmqcrc_last_expire_records", main)


def test_library_exports_both_names_and_nothing_undeclared():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    assert NEW <= exported
    assert set(n for n in exported if n.startswith("bmqcrc_")) == _declared()


def test_version_is_at_least_2_20():
    v = N.lib.bmqcrc_version()
    assert v >> 16 == 2 and v & 0xffff >= 20


def test_kind_constants_and_package_exports():
    for value, kind in enumerate(KINDS):
        assert getattr(N, "BMQCRC_EXPIRE_PACK_" + kind) == value
    assert {"expire_records", "last_expire_records"} <= set(blazingmq_amd.__all__)
    assert blazingmq_amd.expire_records is S.expire_records
    assert blazingmq_amd.last_expire_records is S.last_expire_records


@pytest.mark.parametrize("struct,ctype,size", [
    ("bmqcrc_expire_pack", N.ExpirePack, 144),
    ("bmqcrc_expire_pack_result", N.ExpirePackResult, 64)])
def test_struct_layouts_match_the_header(tmp_path, struct, ctype, size):
    fields = [f[0] for f in ctype._fields_]
    src = tmp_path / "exp.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bmqcrc_protocol.h"\n'
                   'int main(void) { printf("%%zu", sizeof(%s));\n' % struct +
                   "".join('printf(" %%zu", offsetof(%s, %s));\n' % (struct, f) for f in fields) +
                   "".join('printf(" %%d", BMQCRC_EXPIRE_PACK_%s);\n' % k for k in KINDS) +
                   'return 0; }\n')
    exe = tmp_path / "exp"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert got == [ctypes.sizeof(ctype)] + [getattr(ctype, f).offset for f in fields] + [
        getattr(N, "BMQCRC_EXPIRE_PACK_" + k) for k in KINDS]
    assert got[0] == size and got[-5:] == list(range(5))


@pytest.mark.parametrize("flag,name", [
    (N.BMQCRC_F_WHOLE_MESSAGES, b"WHOLE_MESSAGES"), (N.BMQCRC_F_PLAN, b"PLAN"),
    (N.BMQCRC_F_TIME_KERNEL, b"TIME_KERNEL"), (N.BMQCRC_F_OFFSETS32, b"OFFSETS32")])
def test_other_flags_are_einval_naming_the_flag(flag, name):
    for extra in (0, N.BMQCRC_F_ASYNC):
        rc, err, _ = _Call().run(N.BMQCRC_F_DEVICE_PTRS | extra | flag)
        assert rc == N.BMQCRC_EINVAL and name in err, (rc, err)
        assert b"bmqcrc_expire_records_pack" in err, err


def test_unknown_flag_bits_are_einval():
    rc, err, _ = _Call().run(N.BMQCRC_F_DEVICE_PTRS | 0x4000)
    assert rc == N.BMQCRC_EINVAL and b"unknown" in err, (rc, err)


@pytest.mark.parametrize("opts", [None, "plain", "async"])
def test_missing_device_ptrs_is_einval(opts):
    c = _Call()
    rc, err, _ = c.run(opts=None) if opts is None else c.run(
        N.BMQCRC_F_ASYNC if opts == "async" else 0)
    assert rc == N.BMQCRC_EINVAL and b"DEVICE_PTRS" in err, (rc, err)


def test_more_than_one_device_is_einval():
    rc, err, _ = _Call().run(devices=[0, 1])
    assert rc == N.BMQCRC_EINVAL and b"ndevices" in err, (rc, err)


def test_struct_size_and_reserved():
    c = _Call()
    c.p.struct_size -= 8
    c.einval(b"struct_size")
    for name in ("reserved", "reserved2"):
        c = _Call()
        setattr(c.p, name, 1)
        c.einval(b"reserved")
    assert N.lib.bmqcrc_expire_records_pack(None, None, None) == N.BMQCRC_EINVAL


def test_null_journal_is_einval_naming_it():
    c = _Call()
    c.p.journal = None
    rc, err, _ = c.run()
    assert rc == N.BMQCRC_EINVAL and b"null" in err and err.endswith(b": journal"), err


@pytest.mark.parametrize("name", ["queue_keys", "ttl_seconds"])
def test_a_null_table_is_einval_unless_it_is_empty(name):
    c = _Call()
    setattr(c.p, name, None)
    c.einval(b"null", name.encode(), b"n_queues")
    c = _Call()
    c.p.queue_keys, c.p.ttl_seconds, c.p.n_queues = None, None, 0
    c.passes()
    c = _Call()
    c.p.n_queues = 0        # ... and pointers that are not looked at
    c.passes()


def test_null_destination_with_bytes_is_einval_and_without_is_size_only():
    c = _Call()
    c.p.journal_dst = None
    c.einval(b"null", b"journal_dst")
    c = _Call()
    c.p.journal_dst, c.p.journal_dst_bytes = None, 0
    c.passes()


@pytest.mark.parametrize("name,shifts,words", [
    ("journal", (1, 2, 3), b"journal must be 4-byte aligned"),
    ("journal_dst", (1, 2, 3), b"journal_dst must be 4-byte aligned"),
    ("new_index", (1, 2, 3), b"new_index must be 4-byte aligned"),
    ("queue_expired", (1, 2, 3), b"queue_expired must be 4-byte aligned"),
    ("queue_front", (1, 2, 3), b"queue_front must be 4-byte aligned"),
    ("ttl_seconds", (1, 2, 4, 7), b"ttl_seconds must be 8-byte aligned")])
def test_misaligned_pointer_is_einval(name, shifts, words):
    for shift in shifts:
        c = _Call()
        setattr(c.p, name, getattr(c.p, name) + shift)
        c.einval(words)


@pytest.mark.parametrize("name", ["select", "queue_keys", "expired", "select_out"])
def test_byte_arrays_take_any_alignment(name):
    for shift in (1, 2, 3):
        c = _Call()
        setattr(c.p, name, getattr(c.p, name) + shift)
        c.passes()


@pytest.mark.parametrize("nbytes", [0, 60 * RECORDS - 1, 60 * RECORDS + 60])
def test_journal_bytes_must_be_60_n_records(nbytes):
    c = _Call()
    c.p.journal_bytes = nbytes
    c.einval(b"journal_bytes must be 60 n_records")


@pytest.mark.parametrize("n", [1 << 32, (1 << 32) + 5, 1 << 40])
def test_n_records_and_n_queues_must_be_below_2_32(n):
    c = _Call()
    c.p.n_records, c.p.journal_bytes = n, 60 * n
    c.einval(b"n_records must be below 2^32")
    c = _Call()
    c.p.n_queues = n
    c.einval(b"n_queues must be below 2^32")


def test_lease_id_and_first_seq():
    c = _Call()
    c.p.lease_id = 0
    c.einval(b"lease_id")
    for seq in (0, 1 << 48, (1 << 48) - RECORDS, (1 << 64) - 1):
        c = _Call()
        c.p.first_seq = seq
        c.einval(b"first_seq")
    for seq in (1, (1 << 48) - 1 - RECORDS):
        c = _Call()
        c.p.first_seq = seq
        if NO_GPU:      # (with a GPU `passes` sets n_records = 0, which the last value admits anyway)
            c.passes()


def test_every_now_is_taken():
    for now in (0, 1, (1 << 63), (1 << 64) - 1):
        c = _Call()
        c.p.now = now
        c.passes()


# the destination and every output array against every input and the outputs before it
MEETINGS = [(out, other) for k, out in enumerate(OUTPUTS)
            for other in list(INPUTS) + list(OUTPUTS)[:k]]


@pytest.mark.parametrize("where", ["inside", "tail_in", "head_in"])
@pytest.mark.parametrize("out,other", MEETINGS)
def test_output_meeting_an_input_or_another_output_is_einval(out, other, where):
    c = _Call()
    lo, size = c.at[other], HELD[other]
    mine = HELD[out]
    # (4 keeps the 32-bit arrays' alignment; the overlap is then 4 bytes)
    at = {"inside": lo, "tail_in": lo - mine + 4, "head_in": lo + size - 4}[where]
    setattr(c.p, out, at)
    rc, err, _ = c.run()
    assert rc == N.BMQCRC_EINVAL and b"overlaps" in err, (rc, err)
    assert out.encode() in err and other.encode() in err, err


def test_the_destination_may_follow_the_run_and_optionals_may_be_null():
    c = _Call()
    c.p.journal_dst = c.at["journal"] + 60 * RECORDS     # the tail of the run's allocation
    c.p.new_index = c.at["queue_keys"] - 4 * RECORDS     # ends where queue_keys begins
    c.passes()
    c = _Call()
    for name in ("select",) + tuple(OUTPUTS)[1:]:
        setattr(c.p, name, None)
    c.passes()


@pytest.mark.parametrize("flags", [N.BMQCRC_F_DEVICE_PTRS,
                                   N.BMQCRC_F_DEVICE_PTRS | N.BMQCRC_F_ASYNC])
def test_valid_arguments_reach_the_device_lookup(flags):
    _Call().passes(flags, seg_bytes=12345, max_len=7, min_len=9)
    r = N.ExpirePackResult()
    rc = N.lib.bmqcrc_last_expire_records(-1, None, ctypes.byref(r))
    assert rc == (N.BMQCRC_ENODEV if NO_GPU else 0)


def test_no_records_are_checked_like_any_and_launch_nothing():
    c = _Call()
    c.p.n_records, c.p.journal_bytes, c.p.journal_dst = 0, 0, c.p.journal_dst + 2
    c.einval(b"journal_dst must be 4-byte aligned")
    c = _Call()
    c.p.n_records, c.p.journal_bytes = 0, 0
    rc, err, r = c.run()
    assert rc == (N.BMQCRC_ENODEV if NO_GPU else 0), (rc, err)
    if not NO_GPU:
        assert r.as_dict() == dict(n_records=0, n_live=0, n_expired=0, n_no_queue=0,
                                   journal_bytes=0, next_seq=5, refused_kind=0, refused_index=0)
    assert bytes(c.buf) == bytes(len(c.buf))     # (host addresses: nothing was launched on them)


# ---- the Python wrapper ------------------------------------------------------

def test_python_refuses_wrong_types_and_sizes():
    j = torch.zeros(120, dtype=torch.uint8)
    q, t = torch.zeros(10, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64)
    kw = dict(now=5, lease_id=1, first_seq=1)
    with pytest.raises(TypeError, match="journal"):
        expire_records(j.to(torch.int8), q, t, **kw)
    with pytest.raises(TypeError, match="queue_keys"):
        expire_records(j, bytes(10), t, **kw)
    with pytest.raises(TypeError, match="select"):
        expire_records(j, q, t, select=[1, 1], **kw)
    with pytest.raises(TypeError, match="journal_dst"):
        expire_records(j, q, t, journal_dst=torch.zeros(120, dtype=torch.int32), **kw)
    with pytest.raises(TypeError):
        expire_records(j, q, t, lease_id=1, first_seq=1)    # now is required


def test_python_refuses_host_tensors():
    j = torch.zeros(120, dtype=torch.uint8)
    q, t = torch.zeros(10, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(TypeError, match="device tensors only"):
        expire_records(j, q, t, now=5, lease_id=1, first_seq=1)
    with pytest.raises(TypeError, match="device tensors only"):
        expire_records(j, q, t, now=5, lease_id=1, first_seq=1, sync=False,
                       journal_dst=torch.zeros(120, dtype=torch.uint8))


def test_the_writers_deletion_takes_flags_and_defaults_to_none():
    w = S.PartitionWriter(lease_id=2)
    w.deletion(b"\x11" * 16, b"\x01\x02\x03\x04\x05")
    w.deletion(b"\x11" * 16, b"\x01\x02\x03\x04\x05", flags=2)
    assert w.recs[0][:2] == b"\x30\x00" and w.recs[1][:2] == b"\x30\x02"
    assert w.recs[0][8:] == w.recs[1][8:]
