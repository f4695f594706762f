"""ABI 2.11: bmqcrc_message_records_pack and bmqcrc_last_records_pack, as far
as they answer without a GPU -- the declarations, the exports, the struct
layouts, the argument checks that sit in front of the device lookup, and the
Python wrapper's refusals."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from blazingmq_amd import _native as N, last_records_pack, pack_records  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "blazingmq_amd", "lib", "libbmqcrc.so")
NEW = {"bmqcrc_message_records_pack", "bmqcrc_last_records_pack"}
HEADERS = ("bmqcrc.h", "bmqcrc_protocol.h")
KINDS = ("OK", "RECORD_TOO_BIG", "SRC_RANGE", "DST_TOO_SMALL", "DATA_FILE_FULL", "TOO_MANY_PIECES")
NO_GPU = N.lib.bmqcrc_device_count() == 0


def _declared():
    src = ""
    for h in HEADERS:
        with open(os.path.join(ROOT, "include", h)) as f:
            src += f.read()
    return set(re.findall(r"^\w[\w\s\*]*?\b(bmqcrc_\w+)\s*\(", src, re.M))


class _Call:
    """A valid one-message call on host addresses: it only ever reaches the
    argument checks (a machine with a GPU is handed n = 0 where it would pass)."""

    def __init__(self):
        self.src = (ctypes.c_uint8 * 64)(*range(64))
        self.dst = (ctypes.c_uint64 * 16)()
        self.jour = (ctypes.c_uint32 * 16)()
        self.so = (ctypes.c_uint64 * 1)(0)
        self.lens = (ctypes.c_uint32 * 1)(8)
        self.qkey = (ctypes.c_uint8 * 5)(1, 2, 3, 4, 5)
        self.guid = (ctypes.c_uint8 * 16)(*range(1, 17))
        p = N.RecordsPack()
        p.struct_size = ctypes.sizeof(N.RecordsPack)
        p.src, p.src_bytes = ctypes.addressof(self.src), 64
        p.src_offsets, p.lengths = ctypes.addressof(self.so), ctypes.addressof(self.lens)
        p.queue_keys, p.guids = ctypes.addressof(self.qkey), ctypes.addressof(self.guid)
        p.lease_id, p.first_seq, p.data_file_pos, p.n = 1, 1, 40, 1
        p.dst, p.dst_bytes = ctypes.addressof(self.dst), 128
        p.journal_dst, p.journal_bytes = ctypes.addressof(self.jour), 64
        self.p = p

    def run(self, flags=N.BMQCRC_F_DEVICE_PTRS, opts="make", **kw):
        o = N.make_opts(flags=flags, **kw) if opts == "make" else opts
        rc = N.lib.bmqcrc_message_records_pack(ctypes.byref(self.p), None,
                                               ctypes.byref(o) if o is not None else None)
        return rc, N.lib.bmqcrc_last_error()


def test_header_declares_both_names_and_keeps_the_earlier_lines():
    text = open(os.path.join(ROOT, "include", "bmqcrc_protocol.h")).read()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, text, re.M), name
    for i, kind in enumerate(KINDS):
        assert re.search(r"^#define BMQCRC_REC_PACK_%s %d\b" % (kind, i), text, re.M), kind
    assert text.count("Options, compression (CAT)") == 2 and text.count("out of scope") >= 2
    main = open(os.path.join(ROOT, "include", "bmqcrc.h")).read()
    assert all("(2.%d)" % m in main for m in (8, 9, 10, 11))


def test_library_exports_both_names_and_nothing_undeclared():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    assert NEW <= exported
    assert set(n for n in exported if n.startswith("bmqcrc_")) == _declared()


def test_version_is_2_11():
    v = N.lib.bmqcrc_version()
    assert v >> 16 == 2 and v & 0xffff >= 11


def test_struct_layouts_match_the_header(tmp_path):
    pf = [f[0] for f in N.RecordsPack._fields_]
    rf = [f[0] for f in N.RecordsResult._fields_]
    src = tmp_path / "rec.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bmqcrc_protocol.h"\n'
                   'int main(void) { printf("%zu", sizeof(bmqcrc_records_pack));\n' +
                   "".join('printf(" %%zu", offsetof(bmqcrc_records_pack, %s));\n' % f
                           for f in pf) +
                   'printf(" %zu", sizeof(bmqcrc_records_result));\n' +
                   "".join('printf(" %%zu", offsetof(bmqcrc_records_result, %s));\n' % f
                           for f in rf) +
                   "".join('printf(" %%d", BMQCRC_REC_PACK_%s);\n' % k for k in KINDS) +
                   'return 0; }\n')
    exe = tmp_path / "rec"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    want = [ctypes.sizeof(N.RecordsPack)] + [getattr(N.RecordsPack, f).offset for f in pf] + \
        [ctypes.sizeof(N.RecordsResult)] + [getattr(N.RecordsResult, f).offset for f in rf] + \
        [getattr(N, "BMQCRC_REC_PACK_" + k) for k in KINDS]
    assert got == want
    assert got[0] == 184 and got[len(pf) + 1] == 56 and got[-6:] == [0, 1, 2, 3, 4, 5]


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
    assert N.lib.bmqcrc_message_records_pack(None, None, None) == N.BMQCRC_EINVAL


@pytest.mark.parametrize("name", ["src", "src_offsets", "lengths", "queue_keys", "guids", "dst",
                                  "journal_dst"])
def test_null_required_array_is_einval_naming_it(name):
    c = _Call()
    setattr(c.p, name, None)
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"null" in err and err.endswith(b": " + name.encode()), err


@pytest.mark.parametrize("shift", [1, 2, 4, 7])
def test_misaligned_dst_is_einval(shift):
    c = _Call()
    c.p.dst = ctypes.addressof(c.dst) + shift
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"dst must be 8-byte aligned" in err, (rc, err)


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_misaligned_journal_dst_is_einval(shift):
    c = _Call()
    c.p.journal_dst = ctypes.addressof(c.jour) + shift
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"journal_dst must be 4-byte aligned" in err, (rc, err)


@pytest.mark.parametrize("pos", [0, 4, 44, (1 << 32) + 1])
def test_data_file_pos_zero_or_off_a_dword_is_einval(pos):
    c = _Call()
    c.p.data_file_pos = pos
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"data_file_pos" in err, (rc, err)


def test_lease_id_zero_is_einval():
    c = _Call()
    c.p.lease_id = 0
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"lease_id" in err, (rc, err)


@pytest.mark.parametrize("first_seq,n", [(0, 1), (1 << 48, 1), ((1 << 48) - 1, 2),
                                         ((1 << 64) - 1, 1), ((1 << 48) - 3, 4)])
def test_sequence_numbers_outside_48_bits_are_einval(first_seq, n):
    c = _Call()
    c.p.first_seq, c.p.n = first_seq, n
    c.p.journal_bytes = 60 * n  # (never reached: nothing is read or written)
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"first_seq" in err, (rc, err)


def test_journal_too_small_is_einval():
    c = _Call()
    c.p.journal_bytes = 59
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"journal_bytes" in err, (rc, err)


@pytest.mark.parametrize("pair", ["src_dst", "src_journal", "dst_journal"])
@pytest.mark.parametrize("where", ["same", "inside", "tail"])
def test_ranges_meeting_are_einval(pair, where):
    c = _Call()
    buf = (ctypes.c_uint8 * 1024)()
    base = ctypes.addressof(buf)
    base += -base % 8
    # three ranges apart: src [0, 64), dst [256, 384), journal [512, 576)
    at = {"src": 0, "dst": 256, "journal": 512}
    size = {"src": 64, "dst": 128, "journal": 64}
    a, b = pair.split("_")
    # the second begins with the first, inside it, or in its last 8 bytes
    at[b] = at[a] + {"same": 0, "inside": 8, "tail": size[a] - 8}[where]
    c.p.src, c.p.dst, c.p.journal_dst = base + at["src"], base + at["dst"], base + at["journal"]
    c.keep = buf
    rc, err = c.run()
    assert rc == N.BMQCRC_EINVAL and b"overlaps" in err, (rc, err)


def test_adjacent_ranges_reach_the_device_lookup():
    c = _Call()
    buf = (ctypes.c_uint8 * 1024)()
    base = ctypes.addressof(buf)
    base += -base % 8
    c.p.src, c.p.dst, c.p.journal_dst = base, base + 64, base + 64 + 128  # each ends at the next
    c.keep = buf
    if not NO_GPU:
        c.p.n = 0
    rc, err = c.run()
    assert rc == (N.BMQCRC_ENODEV if NO_GPU else 0), (rc, err)


@pytest.mark.parametrize("flags", [N.BMQCRC_F_DEVICE_PTRS,
                                   N.BMQCRC_F_DEVICE_PTRS | N.BMQCRC_F_ASYNC])
def test_valid_arguments_reach_the_device_lookup(flags):
    c = _Call()
    c.p.first_seq = (1 << 48) - 1     # the last sequence number itself is legal
    c.p.data_file_pos = 8 * ((1 << 32) - 1)  # decided on the device, not here
    if not NO_GPU:
        c.p.n = 0
    res = N.RecordsResult()
    res.n_msgs = 77
    o = N.make_opts(flags=flags, seg_bytes=12345, max_len=7, min_len=9)
    rc = N.lib.bmqcrc_message_records_pack(ctypes.byref(c.p), ctypes.byref(res), ctypes.byref(o))
    assert rc == (N.BMQCRC_ENODEV if NO_GPU else 0), (rc, N.lib.bmqcrc_last_error())
    rc = N.lib.bmqcrc_last_records_pack(-1, None, ctypes.byref(res))
    assert rc == (N.BMQCRC_ENODEV if NO_GPU else 0)
    if not NO_GPU:
        assert set(res.as_dict().values()) == {0}  # n = 0 reports zeros
    assert N.lib.bmqcrc_last_records_pack(-1, None, None) == (N.BMQCRC_ENODEV if NO_GPU else 0)


# ---- the Python wrapper ------------------------------------------------------

KW = dict(file_key=bytes(5), lease_id=1, first_seq=1, data_file_pos=40)


def _tensors(n=3, size=64):
    return dict(src=torch.zeros(size, dtype=torch.uint8),
                src_offsets=torch.zeros(n, dtype=torch.int64),
                lengths=torch.full((n,), 8, dtype=torch.int32),
                queue_keys=torch.ones((n, 5), dtype=torch.uint8),
                guids=torch.ones((n, 16), dtype=torch.uint8))


@pytest.mark.parametrize("name,dtype", [
    ("src", torch.int8), ("src_offsets", torch.int32), ("lengths", torch.int64),
    ("queue_keys", torch.int32), ("guids", torch.int32)])
def test_python_refuses_wrong_dtypes(name, dtype):
    t = _tensors()
    t[name] = t[name].to(dtype)
    with pytest.raises(TypeError, match=name):
        pack_records(**t, **KW)


@pytest.mark.parametrize("name,good,bad", [
    ("data_flags", torch.uint8, torch.int32), ("ref_counts", torch.int32, torch.int64),
    ("timestamps", torch.int64, torch.int32), ("expected", torch.int32, torch.uint8),
    ("out", torch.int32, torch.uint8)])
def test_python_refuses_wrong_optional_tensors(name, good, bad):
    t = _tensors()
    with pytest.raises(TypeError, match=name):
        pack_records(**t, **KW, **{name: torch.zeros(3, dtype=bad)})
    with pytest.raises(TypeError, match=name):
        pack_records(**t, **KW, **{name: torch.zeros(4, dtype=good)})
    with pytest.raises(TypeError, match=name):
        pack_records(**t, **KW, **{name: torch.zeros(6, dtype=good)[::2]})


@pytest.mark.parametrize("name", ["dst", "journal_dst"])
def test_python_refuses_wrong_destinations(name):
    t = _tensors()
    with pytest.raises(TypeError, match=name):
        pack_records(**t, **KW, **{name: torch.zeros(256, dtype=torch.int32)})
    with pytest.raises(TypeError, match=name):
        pack_records(**t, **KW, **{name: torch.zeros(512, dtype=torch.uint8)[::2]})


@pytest.mark.parametrize("name", ["lengths", "queue_keys", "guids"])
def test_python_refuses_wrong_sizes(name):
    t = _tensors()
    t[name] = t[name][:2].contiguous()
    with pytest.raises(ValueError, match="size mismatch"):
        pack_records(**t, **KW)
    with pytest.raises(ValueError, match="file_key"):
        pack_records(**_tensors(), **dict(KW, file_key=bytes(4)))


@pytest.mark.parametrize("name", ["src", "src_offsets", "lengths", "queue_keys", "guids"])
def test_python_refuses_non_contiguous(name):
    t = _tensors()
    wide = torch.zeros(2 * t[name].numel(), dtype=t[name].dtype)
    t[name] = wide[::2]
    assert not t[name].is_contiguous()
    with pytest.raises(TypeError, match=name):
        pack_records(**t, **KW)


def test_python_refuses_host_tensors():
    with pytest.raises(TypeError, match="device tensors only"):
        pack_records(**_tensors(), **KW)
    with pytest.raises(TypeError):
        pack_records(b"12345678", [0], [8], bytes(5), bytes(16), **KW)
