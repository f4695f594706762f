"""ABI 2.21: bmqcrc_pending_records_list and bmqcrc_last_pending_records, as far
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
from blazingmq_amd import _native as N, last_pending_records, pending_records  # noqa: F401
from blazingmq_amd import storage as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "blazingmq_amd", "lib", "libbmqcrc.so")
NEW = {"bmqcrc_pending_records_list", "bmqcrc_last_pending_records"}
HEADERS = ("bmqcrc.h", "bmqcrc_protocol.h")
NO_GPU = N.lib.bmqcrc_device_count() == 0
KINDS = ("OK", "RECORD_HEADER", "DUPLICATE_MESSAGE", "QUEUE_KEY", "APP_FIRST", "APP_KEY",
         "FROM_RECORD", "LIST_TOO_SMALL")
RECORDS, QUEUES, APPS, CAP = 4, 3, 8, 16
# name -> bytes of a valid call's array (8 more than select holds, so that a
# neighbour placed against its end stays aligned)
INPUTS = {"journal": 60 * RECORDS, "select": 8, "queue_keys": 5 * QUEUES,
          "app_first": 8 * (QUEUES + 1), "app_keys": 5 * APPS, "queue_ids": 4 * APPS,
          "sub_ids": 4 * APPS, "from_record": 4 * APPS, "limit": 4 * APPS}
OUTPUTS = {"records": 4 * CAP, "out_queue_ids": 4 * CAP, "out_sub_ids": 4 * CAP,
           "list_first": 8 * (APPS + 1), "app_pending": 4 * APPS, "app_next": 4 * APPS,
           "pending_mask": 4 * RECORDS}
# what the overlap check takes each array to hold
HELD = dict(INPUTS, select=RECORDS, **OUTPUTS)
WORDS32 = ("queue_ids", "sub_ids", "from_record", "limit", "records", "out_queue_ids",
           "out_sub_ids", "app_pending", "app_next", "pending_mask")


def _declared():
    src = ""
    for h in HEADERS:
        with open(os.path.join(ROOT, "include", h)) as f:
            src += f.read()
    return set(re.findall(r"^\w[\w\s\*]*?\b(bmqcrc_\w+)\s*\(", src, re.M))


class _Call:
    """A valid call over four records, three queues and eight apps on host
    addresses: it only ever reaches the argument checks (a machine with a GPU
    is handed n_records = 0 where it would pass)."""

    def __init__(self):
        self.buf = (ctypes.c_uint8 * 32768)()
        base = ctypes.addressof(self.buf)
        base += -base % 8
        # 1 KiB apart, in this order
        self.at = {name: base + 1024 * (k + 1)
                   for k, name in enumerate(list(INPUTS) + list(OUTPUTS))}
        p = N.PendingList()
        p.struct_size = ctypes.sizeof(N.PendingList)
        for name, where in self.at.items():
            setattr(p, name, where)
        p.journal_bytes, p.n_records = 60 * RECORDS, RECORDS
        p.n_queues, p.n_apps, p.list_cap = QUEUES, APPS, CAP
        self.p = p

    def run(self, flags=N.BMQCRC_F_DEVICE_PTRS, opts="make", **kw):
        o = N.make_opts(flags=flags, **kw) if opts == "make" else opts
        r = N.PendingListResult()
        rc = N.lib.bmqcrc_pending_records_list(ctypes.byref(self.p), ctypes.byref(r),
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
        assert re.search(r"#define BMQCRC_PENDING_LIST_%s %d\b" % (kind, value), text), kind
    assert text.index("ABI 2.20") < text.index("ABI 2.21")
    mine = text[text.index("ABI 2.21"):]
    assert "has no CRC in it" in mine and "Per-app PURGE" in mine and "getIterator" in mine
    main = open(os.path.join(ROOT, "include", "bmqcrc.h")).read()
    assert re.search(r"\(2\.21\) bmqcrc_pending_records_list, bmqcrc_last_pending_records", main)


def test_library_exports_both_names_and_nothing_undeclared():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    assert NEW <= exported
    assert set(n for n in exported if n.startswith("bmqcrc_")) == _declared()


def test_version_is_at_least_2_21():
    v = N.lib.bmqcrc_version()
    assert v >> 16 == 2 and v & 0xffff >= 21


def test_kind_constants_and_package_exports():
    for value, kind in enumerate(KINDS):
        assert getattr(N, "BMQCRC_PENDING_LIST_" + kind) == value
    assert {"pending_records", "last_pending_records"} <= set(blazingmq_amd.__all__)
    assert blazingmq_amd.pending_records is S.pending_records
    assert blazingmq_amd.last_pending_records is S.last_pending_records


@pytest.mark.parametrize("struct,ctype,size", [
    ("bmqcrc_pending_list", N.PendingList, 176),
    ("bmqcrc_pending_list_result", N.PendingListResult, 72)])
def test_struct_layouts_match_the_header(tmp_path, struct, ctype, size):
    fields = [f[0] for f in ctype._fields_]
    src = tmp_path / "pnd.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bmqcrc_protocol.h"\n'
                   'int main(void) { printf("%%zu", sizeof(%s));\n' % struct +
                   "".join('printf(" %%zu", offsetof(%s, %s));\n' % (struct, f) for f in fields) +
                   "".join('printf(" %%d", BMQCRC_PENDING_LIST_%s);\n' % k for k in KINDS) +
                   'return 0; }\n')
    exe = tmp_path / "pnd"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert got == [ctypes.sizeof(ctype)] + [getattr(ctype, f).offset for f in fields] + [
        getattr(N, "BMQCRC_PENDING_LIST_" + k) for k in KINDS]
    assert got[0] == size and got[-8:] == list(range(8))


@pytest.mark.parametrize("flag,name", [
    (N.BMQCRC_F_WHOLE_MESSAGES, b"WHOLE_MESSAGES"), (N.BMQCRC_F_PLAN, b"PLAN"),
    (N.BMQCRC_F_TIME_KERNEL, b"TIME_KERNEL"), (N.BMQCRC_F_OFFSETS32, b"OFFSETS32")])
def test_other_flags_are_einval_naming_the_flag(flag, name):
    for extra in (0, N.BMQCRC_F_ASYNC):
        rc, err, _ = _Call().run(N.BMQCRC_F_DEVICE_PTRS | extra | flag)
        assert rc == N.BMQCRC_EINVAL and name in err, (rc, err)
        assert b"bmqcrc_pending_records_list" in err, err


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
    c = _Call()
    c.p.reserved = 1
    c.einval(b"reserved")
    assert N.lib.bmqcrc_pending_records_list(None, None, None) == N.BMQCRC_EINVAL


@pytest.mark.parametrize("name", ["journal", "app_first", "out_queue_ids", "list_first"])
def test_a_required_pointer_null_is_einval_naming_it(name):
    c = _Call()
    setattr(c.p, name, None)
    c.einval(b"null pointer argument", name.encode())


@pytest.mark.parametrize("name,count", [("queue_keys", "n_queues"), ("app_keys", "n_apps"),
                                        ("queue_ids", "n_apps")])
def test_a_null_table_is_einval_unless_it_is_empty(name, count):
    c = _Call()
    setattr(c.p, name, None)
    c.einval(b"null", name.encode(), count.encode())
    c = _Call()
    c.p.queue_keys, c.p.n_queues = None, 0
    c.p.app_keys, c.p.queue_ids, c.p.n_apps = None, None, 0
    c.p.sub_ids = c.p.out_sub_ids = c.p.from_record = c.p.limit = None
    c.p.app_pending = c.p.app_next = None
    c.passes()


def test_null_records_with_a_capacity_is_einval_and_without_is_size_only():
    c = _Call()
    c.p.records = None
    c.einval(b"null", b"records", b"list_cap")
    c = _Call()
    c.p.records, c.p.list_cap = None, 0
    c.passes()
    c = _Call()         # ... and then no list and no list_first is asked for
    c.p.records, c.p.list_cap, c.p.out_queue_ids, c.p.out_sub_ids, c.p.list_first = \
        None, 0, None, None, None
    c.passes()


def test_out_sub_ids_without_sub_ids_is_einval_and_the_reverse_is_not():
    c = _Call()
    c.p.sub_ids = None
    c.einval(b"sub_ids", b"out_sub_ids")
    c = _Call()
    c.p.out_sub_ids = None
    c.passes()


@pytest.mark.parametrize("name", ("journal",) + WORDS32)
def test_a_misaligned_32_bit_pointer_is_einval(name):
    for shift in (1, 2, 3):
        c = _Call()
        setattr(c.p, name, getattr(c.p, name) + shift)
        c.einval(name.encode() + b" must be 4-byte aligned")


@pytest.mark.parametrize("name", ["app_first", "list_first"])
def test_a_misaligned_64_bit_pointer_is_einval(name):
    for shift in (1, 2, 4, 7):
        c = _Call()
        setattr(c.p, name, getattr(c.p, name) + shift)
        c.einval(name.encode() + b" must be 8-byte aligned")


@pytest.mark.parametrize("name", ["select", "queue_keys", "app_keys"])
def test_byte_arrays_take_any_alignment(name):
    for shift in (1, 2, 3):
        c = _Call()
        setattr(c.p, name, getattr(c.p, name) + shift)
        c.passes()


def test_the_permitted_alignments_pass():
    c = _Call()
    for name in WORDS32:
        setattr(c.p, name, getattr(c.p, name) + 4)
    c.p.app_first += 8
    c.p.list_first += 8
    c.passes()


@pytest.mark.parametrize("nbytes", [0, 60 * RECORDS - 1, 60 * RECORDS + 60])
def test_journal_bytes_must_be_60_n_records(nbytes):
    c = _Call()
    c.p.journal_bytes = nbytes
    c.einval(b"journal_bytes must be 60 n_records")


@pytest.mark.parametrize("n", [1 << 32, (1 << 32) + 5, 1 << 40])
def test_the_counts_must_be_below_2_32(n):
    c = _Call()
    c.p.n_records, c.p.journal_bytes = n, 60 * n
    c.einval(b"n_records must be below 2^32")
    c = _Call()
    c.p.n_queues = n
    c.einval(b"n_queues must be below 2^32")
    c = _Call()
    c.p.n_apps = n
    c.einval(b"n_apps must be below 2^32")


# every output array against every input and the outputs before it
MEETINGS = [(out, other) for k, out in enumerate(OUTPUTS)
            for other in list(INPUTS) + list(OUTPUTS)[:k]]


@pytest.mark.parametrize("where", ["inside", "tail_in", "head_in"])
@pytest.mark.parametrize("out,other", MEETINGS)
def test_output_meeting_an_input_or_another_output_is_einval(out, other, where):
    c = _Call()
    lo, size = c.at[other], HELD[other]
    mine = HELD[out]
    # (multiples of 8 keep every array's alignment; the overlap is then 4 or 8 bytes)
    step = 8 if "first" in out else 4
    at = {"inside": lo, "tail_in": lo - mine + step, "head_in": lo + size - step}[where]
    at -= at % step
    setattr(c.p, out, at)
    rc, err, _ = c.run()
    assert rc == N.BMQCRC_EINVAL and b"overlaps" in err, (rc, err)
    assert out.encode() in err and other.encode() in err, err


def test_neighbours_may_touch_and_optionals_may_be_null():
    c = _Call()
    c.p.records = c.at["journal"] + 60 * RECORDS        # the tail of the run's allocation
    c.p.app_next = c.at["queue_keys"] - 4 * APPS        # ends where queue_keys begins
    c.passes()
    c = _Call()
    for name in ("select", "sub_ids", "out_sub_ids", "from_record", "limit", "app_pending",
                 "app_next", "pending_mask"):
        setattr(c.p, name, None)
    c.passes()


@pytest.mark.parametrize("flags", [N.BMQCRC_F_DEVICE_PTRS,
                                   N.BMQCRC_F_DEVICE_PTRS | N.BMQCRC_F_ASYNC])
def test_valid_arguments_reach_the_device_lookup(flags):
    _Call().passes(flags, seg_bytes=12345, max_len=7, min_len=9)
    r = N.PendingListResult()
    rc = N.lib.bmqcrc_last_pending_records(-1, None, ctypes.byref(r))
    assert rc == (N.BMQCRC_ENODEV if NO_GPU else 0)


def test_no_records_are_checked_like_any_and_launch_nothing():
    c = _Call()
    c.p.n_records, c.p.journal_bytes, c.p.records = 0, 0, c.p.records + 2
    c.einval(b"records must be 4-byte aligned")
    c = _Call()
    c.p.n_records, c.p.journal_bytes = 0, 0
    rc, err, r = c.run()
    assert rc == (N.BMQCRC_ENODEV if NO_GPU else 0), (rc, err)
    if not NO_GPU:
        assert r.as_dict() == dict(n_records=0, n_live=0, n_no_queue=0, n_pending=0, n_listed=0,
                                   n_unknown_confirms=0, n_not_found=0, refused_kind=0,
                                   refused_index=0)
    assert bytes(c.buf) == bytes(len(c.buf))     # (host addresses: nothing was launched on them)


# ---- the Python wrapper ------------------------------------------------------

def _host_args():
    return (torch.zeros(120, dtype=torch.uint8), torch.zeros(5, dtype=torch.uint8),
            torch.zeros(2, dtype=torch.int64), torch.zeros(10, dtype=torch.uint8),
            torch.zeros(2, dtype=torch.int32))


def test_python_refuses_wrong_types_and_sizes():
    j, q, f, k, i = _host_args()
    with pytest.raises(TypeError, match="journal"):
        pending_records(j.to(torch.int8), q, f, k, i)
    with pytest.raises(TypeError, match="queue_keys"):
        pending_records(j, bytes(5), f, k, i)
    with pytest.raises(TypeError, match="app_first"):
        pending_records(j, q, f.to(torch.int32), k, i)
    with pytest.raises(TypeError, match="queue_ids"):
        pending_records(j, q, f, k, i.to(torch.int64))
    for name in ("sub_ids", "from_record", "limit", "select"):
        with pytest.raises(TypeError, match=name):
            pending_records(j, q, f, k, i, **{name: [1, 1]})


def test_python_refuses_host_tensors():
    with pytest.raises(TypeError, match="device tensors only"):
        pending_records(*_host_args())
    with pytest.raises(TypeError, match="device tensors only"):
        pending_records(*_host_args(), list_cap=4, sync=False)
