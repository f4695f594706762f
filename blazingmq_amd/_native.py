"""ctypes binding to the in-tree C-ABI library ``lib/libbmqcrc.so``.

There is no pure-Python or CPU substitute for the batch path: if the library
is missing this module raises at import, and the batch entry point returns
BMQCRC_ENODEV (raised as ``BmqCrcError``) when no MI355X is usable.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libbmqcrc.so")

BMQCRC_OK = 0
BMQCRC_EIO = -5
BMQCRC_ENOMEM = -12
BMQCRC_ENODEV = -19
BMQCRC_EINVAL = -22
BMQCRC_F_DEVICE_PTRS = 0x1
BMQCRC_F_ASYNC = 0x2
BMQCRC_F_TIME_KERNEL = 0x4
BMQCRC_F_WHOLE_MESSAGES = 0x8
BMQCRC_F_PLAN = 0x10
BMQCRC_F_OFFSETS32 = 0x20


class BmqCrcError(RuntimeError):
    def __init__(self, rc, msg):
        super().__init__("bmqcrc error %d: %s" % (rc, msg))
        self.rc = rc


class Opts(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("device", ctypes.c_int32),
                ("stream", ctypes.c_void_p), ("flags", ctypes.c_uint32),
                ("seg_bytes", ctypes.c_uint32), ("ndevices", ctypes.c_uint32),
                ("devices", ctypes.c_void_p), ("max_len", ctypes.c_uint32),
                ("min_len", ctypes.c_uint32), ("offset_shift", ctypes.c_uint32)]


# One HIP runtime per process: when PyTorch-ROCm is present it ships its own
# libamdhip64.so (soname libamdhip64.so.7).  Loading torch first lets this
# library's DT_NEEDED libamdhip64.so.7 bind to that same runtime instead of
# pulling a second copy from /opt/rocm (two runtimes cannot share a device).
try:
    import torch  # noqa: F401
except ImportError:  # pragma: no cover - torch is optional for the C ABI itself
    torch = None

if not os.path.exists(LIB_PATH):
    raise ImportError("libbmqcrc.so not built (%s); run `python -c \"import __graft_entry__ as g; "
                      "g.build()\"` first" % LIB_PATH)

lib = ctypes.CDLL(LIB_PATH)
_u32, _u64, _vp, _int = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int

lib.bmqcrc_crc32c.restype = _u32
lib.bmqcrc_crc32c.argtypes = [_vp, _u32, _u32]
lib.bmqcrc_crc32c_blob.restype = _u32
lib.bmqcrc_crc32c_blob.argtypes = [ctypes.POINTER(_vp), ctypes.POINTER(_u32), _u32, _u32]
lib.bmqcrc_combine.restype = _u32
lib.bmqcrc_combine.argtypes = [_u32, _u32, _u64]
lib.bmqcrc_crc32c_batch.restype = _int
lib.bmqcrc_crc32c_batch.argtypes = [_vp, _u64, _vp, _vp, _vp, _vp, _u64, ctypes.POINTER(Opts)]
lib.bmqcrc_crc32c_verify.restype = _int
lib.bmqcrc_crc32c_verify.argtypes = [_vp, _u64, _vp, _vp, _vp, _u64, ctypes.POINTER(_u64), _vp,
                                     _u64, ctypes.POINTER(Opts)]
lib.bmqcrc_crc32c_blobs.restype = _int
lib.bmqcrc_crc32c_blobs.argtypes = [_vp, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _u64,
                                    ctypes.POINTER(Opts)]
lib.bmqcrc_crc32c_batch_multi.restype = _int
lib.bmqcrc_crc32c_gather.restype = _int
lib.bmqcrc_crc32c_gather.argtypes = [ctypes.POINTER(_vp), _vp, _u64, _vp, _vp, _vp, _u64,
                                     ctypes.POINTER(Opts)]
lib.bmqcrc_crc32c_batch_multi.argtypes = [_vp, _u64, _vp, _vp, _vp, _vp, _u64, _vp, _int, _u32]
lib.bmqcrc_reserve.restype = _int
lib.bmqcrc_reserve.argtypes = [_int, _vp, _u64, _u64, _u32]
lib.bmqcrc_fill_synthetic.restype = _int
lib.bmqcrc_fill_synthetic.argtypes = [_vp, _u64, _u64, _u64, ctypes.POINTER(Opts)]
lib.bmqcrc_kernel_timing.restype = _int
lib.bmqcrc_kernel_timing.argtypes = [_int, _vp, ctypes.POINTER(ctypes.c_double),
                                     ctypes.POINTER(_u32)]
lib.bmqcrc_last_plan.restype = _int
lib.bmqcrc_last_plan.argtypes = [_int, _vp, ctypes.POINTER(_u32)]
lib.bmqcrc_last_launch.restype = _int
lib.bmqcrc_last_launch.argtypes = [_int, _vp, ctypes.POINTER(_u32), ctypes.POINTER(_u32),
                                   ctypes.POINTER(_u32)]
if hasattr(lib, "bmqcrc_last_offsets"):  # ABI 2.8 (an older build loads for same-box A/B)
    lib.bmqcrc_last_offsets.restype = _int
    lib.bmqcrc_last_offsets.argtypes = [_int, _vp, ctypes.POINTER(_u32), ctypes.POINTER(_u32)]
if hasattr(lib, "bmqcrc_crc32c_copy"):  # ABI 2.9 (an older build loads for same-box A/B)
    lib.bmqcrc_crc32c_copy.restype = _int
    lib.bmqcrc_crc32c_copy.argtypes = [_vp, _u64, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _u64,
                                       ctypes.POINTER(Opts)]
    lib.bmqcrc_last_copy.restype = _int
    lib.bmqcrc_last_copy.argtypes = [_int, _vp, ctypes.POINTER(_u64), ctypes.POINTER(_u64),
                                     ctypes.POINTER(_u64)]
lib.bmqcrc_forget_shape.restype = _int
lib.bmqcrc_forget_shape.argtypes = [_int, _vp]
if hasattr(lib, "bmqcrc_plan_wait"):  # ABI 2.3 (an older build loads for same-box A/B)
    lib.bmqcrc_plan_wait.restype = _int
    lib.bmqcrc_plan_wait.argtypes = [_int, _vp, _u64, ctypes.POINTER(_u64)]
lib.bmqcrc_host_register.restype = _int
lib.bmqcrc_host_register.argtypes = [_vp, _u64, _int, ctypes.POINTER(_vp)]
lib.bmqcrc_host_unregister.restype = _int
lib.bmqcrc_host_unregister.argtypes = [_vp]
lib.bmqcrc_device_count.restype = _int
lib.bmqcrc_device_count.argtypes = []
lib.bmqcrc_last_error.restype = ctypes.c_char_p
lib.bmqcrc_last_error.argtypes = []
lib.bmqcrc_version.restype = _u32
lib.bmqcrc_version.argtypes = []

# include/bmqcrc_protocol.h
_i64, _pu64, _pint, _popts = ctypes.c_int64, ctypes.POINTER(_u64), ctypes.POINTER(_int), \
    ctypes.POINTER(Opts)
lib.bmqcrc_put_event_scan.restype = _i64
lib.bmqcrc_put_event_scan.argtypes = [_vp, _u64, _vp, _vp, _vp, _u64]
lib.bmqcrc_put_event_fill_crcs.restype = _i64
lib.bmqcrc_put_event_fill_crcs.argtypes = [_vp, _u64, _popts]
lib.bmqcrc_put_event_verify.restype = _int
lib.bmqcrc_put_event_verify.argtypes = [_vp, _u64, _pu64, _pu64, _vp, _u64, _popts]
BMQCRC_PUT_PACK_OK = 0
BMQCRC_PUT_PACK_SRC_RANGE = 1
BMQCRC_PUT_PACK_EVENT_FIRST = 2
BMQCRC_PUT_PACK_EVENT_TOO_BIG = 3
BMQCRC_PUT_PACK_DST_TOO_SMALL = 4
BMQCRC_PUT_PACK_TOO_MANY_PIECES = 5


class PutPack(ctypes.Structure):
    """bmqcrc_put_pack (include/bmqcrc_protocol.h, ABI 2.10)."""
    _fields_ = [("struct_size", _u32), ("reserved", _u32), ("src", _vp), ("src_bytes", _u64),
                ("src_offsets", _vp), ("lengths", _vp), ("queue_ids", _vp), ("guids", _vp),
                ("flags", _vp), ("event_first", _vp), ("n", _u64), ("n_events", _u64),
                ("max_event_bytes", _u64), ("dst", _vp), ("dst_bytes", _u64),
                ("event_offsets", _vp), ("out", _vp)]


if hasattr(lib, "bmqcrc_put_event_pack"):  # ABI 2.10 (an older build loads for same-box A/B)
    lib.bmqcrc_put_event_pack.restype = _int
    lib.bmqcrc_put_event_pack.argtypes = [ctypes.POINTER(PutPack), _pu64, _popts]
    lib.bmqcrc_last_put_pack.restype = _int
    lib.bmqcrc_last_put_pack.argtypes = [_int, _vp, _pu64, _pu64, _pu64, ctypes.POINTER(_u32),
                                         _pu64]
BMQCRC_REC_PACK_OK = 0
BMQCRC_REC_PACK_RECORD_TOO_BIG = 1
BMQCRC_REC_PACK_SRC_RANGE = 2
BMQCRC_REC_PACK_DST_TOO_SMALL = 3
BMQCRC_REC_PACK_DATA_FILE_FULL = 4
BMQCRC_REC_PACK_TOO_MANY_PIECES = 5


class RecordsPack(ctypes.Structure):
    """bmqcrc_records_pack (include/bmqcrc_protocol.h, ABI 2.11)."""
    _fields_ = [("struct_size", _u32), ("reserved", _u32), ("src", _vp), ("src_bytes", _u64),
                ("src_offsets", _vp), ("lengths", _vp), ("queue_keys", _vp), ("guids", _vp),
                ("data_flags", _vp), ("ref_counts", _vp), ("timestamps", _vp), ("expected", _vp),
                ("file_key", ctypes.c_uint8 * 5), ("reserved2", ctypes.c_uint8 * 3),
                ("lease_id", _u32), ("first_seq", _u64), ("timestamp", _u64),
                ("data_file_pos", _u64), ("n", _u64), ("dst", _vp), ("dst_bytes", _u64),
                ("journal_dst", _vp), ("journal_bytes", _u64), ("record_offsets", _vp),
                ("out", _vp)]


class RecordsResult(ctypes.Structure):
    """bmqcrc_records_result (include/bmqcrc_protocol.h, ABI 2.11)."""
    _fields_ = [("n_msgs", _u64), ("data_bytes", _u64), ("journal_bytes", _u64), ("n_bad", _u64),
                ("first_bad", _u64), ("refused_kind", _u32), ("reserved", _u32),
                ("refused_index", _u64)]

    def as_dict(self):
        return {f[0]: int(getattr(self, f[0])) for f in self._fields_ if f[0] != "reserved"}


if hasattr(lib, "bmqcrc_message_records_pack"):  # ABI 2.11 (an older build loads for same-box A/B)
    lib.bmqcrc_message_records_pack.restype = _int
    lib.bmqcrc_message_records_pack.argtypes = [ctypes.POINTER(RecordsPack),
                                                ctypes.POINTER(RecordsResult), _popts]
    lib.bmqcrc_last_records_pack.restype = _int
    lib.bmqcrc_last_records_pack.argtypes = [_int, _vp, ctypes.POINTER(RecordsResult)]
BMQCRC_PUT_UNPACK_OK = 0
BMQCRC_PUT_UNPACK_EVENT_OFFSETS = 1
BMQCRC_PUT_UNPACK_EVENT_HEADER = 2
BMQCRC_PUT_UNPACK_PUT_HEADER = 3
BMQCRC_PUT_UNPACK_PADDING = 4
BMQCRC_PUT_UNPACK_TOO_MANY_MESSAGES = 5


class PutUnpack(ctypes.Structure):
    """bmqcrc_put_unpack (include/bmqcrc_protocol.h, ABI 2.12)."""
    _fields_ = [("struct_size", _u32), ("reserved", _u32), ("events", _vp), ("events_bytes", _u64),
                ("event_offsets", _vp), ("n_events", _u64), ("msg_cap", _u64),
                ("app_offsets", _vp), ("lengths", _vp), ("queue_ids", _vp), ("guids", _vp),
                ("flags", _vp), ("expected", _vp), ("out", _vp), ("event_first", _vp)]


class PutUnpackResult(ctypes.Structure):
    """bmqcrc_put_unpack_result (include/bmqcrc_protocol.h, ABI 2.12)."""
    _fields_ = [("n_events", _u64), ("n_msgs", _u64), ("n_bad", _u64), ("first_bad", _u64),
                ("refused_kind", _u32), ("reserved", _u32), ("refused_event", _u64),
                ("refused_offset", _u64)]

    def as_dict(self):
        return {f[0]: int(getattr(self, f[0])) for f in self._fields_ if f[0] != "reserved"}


if hasattr(lib, "bmqcrc_put_event_unpack"):  # ABI 2.12 (an older build loads for same-box A/B)
    lib.bmqcrc_put_event_unpack.restype = _int
    lib.bmqcrc_put_event_unpack.argtypes = [ctypes.POINTER(PutUnpack),
                                            ctypes.POINTER(PutUnpackResult), _popts]
    lib.bmqcrc_last_put_unpack.restype = _int
    lib.bmqcrc_last_put_unpack.argtypes = [_int, _vp, ctypes.POINTER(PutUnpackResult)]
BMQCRC_REC_UNPACK_OK = 0
BMQCRC_REC_UNPACK_RECORD_HEADER = 1
BMQCRC_REC_UNPACK_MESSAGE_RECORD = 2
BMQCRC_REC_UNPACK_DATA_OFFSET = 3
BMQCRC_REC_UNPACK_DATA_RECORD = 4
BMQCRC_REC_UNPACK_TOO_MANY_MESSAGES = 5


class RecordsUnpack(ctypes.Structure):
    """bmqcrc_records_unpack (include/bmqcrc_protocol.h, ABI 2.13)."""
    _fields_ = [("struct_size", _u32), ("reserved", _u32), ("journal", _vp),
                ("journal_bytes", _u64), ("n_records", _u64), ("data", _vp), ("data_bytes", _u64),
                ("data_file_pos", _u64), ("select", _vp), ("msg_cap", _u64),
                ("record_index", _vp), ("app_offsets", _vp), ("lengths", _vp),
                ("queue_keys", _vp), ("guids", _vp), ("data_flags", _vp), ("ref_counts", _vp),
                ("timestamps", _vp), ("expected", _vp), ("out", _vp)]


class RecordsUnpackResult(ctypes.Structure):
    """bmqcrc_records_unpack_result (include/bmqcrc_protocol.h, ABI 2.13)."""
    _fields_ = [("n_records", _u64), ("n_msgs", _u64), ("n_skipped", _u64), ("n_bad", _u64),
                ("first_bad", _u64), ("refused_kind", _u32), ("reserved", _u32),
                ("refused_index", _u64)]

    def as_dict(self):
        return {f[0]: int(getattr(self, f[0])) for f in self._fields_ if f[0] != "reserved"}


if hasattr(lib, "bmqcrc_message_records_unpack"):  # ABI 2.13 (an older build loads for same-box A/B)
    lib.bmqcrc_message_records_unpack.restype = _int
    lib.bmqcrc_message_records_unpack.argtypes = [ctypes.POINTER(RecordsUnpack),
                                                  ctypes.POINTER(RecordsUnpackResult), _popts]
    lib.bmqcrc_last_records_unpack.restype = _int
    lib.bmqcrc_last_records_unpack.argtypes = [_int, _vp, ctypes.POINTER(RecordsUnpackResult)]
BMQCRC_JSEL_OK = 0
BMQCRC_JSEL_TOO_MANY_QUEUES = 1


class JournalSelect(ctypes.Structure):
    """bmqcrc_journal_select_args (include/bmqcrc_protocol.h, ABI 2.14)."""
    _fields_ = [("struct_size", _u32), ("reserved", _u32), ("journal", _vp),
                ("journal_bytes", _u64), ("n_records", _u64), ("data_file_bytes", _u64),
                ("with_csl", ctypes.c_int32), ("reserved2", ctypes.c_int32), ("queue_keys", _vp),
                ("n_queue_keys", _u64), ("queue_cap", _u64), ("select", _vp)]


class JournalSelectResult(ctypes.Structure):
    """bmqcrc_journal_select_result (include/bmqcrc_protocol.h, ABI 2.14)."""
    _fields_ = [("n_records", _u64), ("first_record", _u64), ("n_selected", _u64),
                ("n_deleted", _u64), ("n_purged", _u64), ("error_record", _u64),
                ("recovery_rc", ctypes.c_int32), ("refused_kind", _u32)]

    def as_dict(self):
        return {f[0]: int(getattr(self, f[0])) for f in self._fields_}


if hasattr(lib, "bmqcrc_journal_select"):  # ABI 2.14 (an older build loads for same-box A/B)
    lib.bmqcrc_journal_select.restype = _int
    lib.bmqcrc_journal_select.argtypes = [ctypes.POINTER(JournalSelect),
                                          ctypes.POINTER(JournalSelectResult), _popts]
    lib.bmqcrc_last_journal_select.restype = _int
    lib.bmqcrc_last_journal_select.argtypes = [_int, _vp, ctypes.POINTER(JournalSelectResult)]
BMQCRC_STORAGE_APPLY_OK = 0
BMQCRC_STORAGE_APPLY_EVENT_OFFSETS = 1
BMQCRC_STORAGE_APPLY_EVENT_HEADER = 2
BMQCRC_STORAGE_APPLY_STORAGE_HEADER = 3
BMQCRC_STORAGE_APPLY_DATA_RECORD = 4
BMQCRC_STORAGE_APPLY_TOO_MANY_MESSAGES = 5
BMQCRC_STORAGE_APPLY_OUT_OF_SYNC = 6
BMQCRC_STORAGE_APPLY_DST_TOO_SMALL = 7
BMQCRC_STORAGE_APPLY_TOO_MANY_PIECES = 8


class StorageApply(ctypes.Structure):
    """bmqcrc_storage_apply (include/bmqcrc_protocol.h, ABI 2.15)."""
    _fields_ = [("struct_size", _u32), ("reserved", _u32), ("events", _vp), ("events_bytes", _u64),
                ("event_offsets", _vp), ("n_events", _u64), ("msg_cap", _u64),
                ("partition_id", _u32), ("lease_id", _u32), ("seq", _u64), ("journal_pos", _u64),
                ("data_file_pos", _u64), ("journal_dst", _vp), ("journal_dst_bytes", _u64),
                ("data_dst", _vp), ("data_dst_bytes", _u64), ("types", _vp), ("flags", _vp),
                ("payload_offsets", _vp), ("payload_lengths", _vp), ("record_offsets", _vp),
                ("lengths", _vp), ("expected", _vp), ("out", _vp), ("event_first", _vp)]


class StorageApplyResult(ctypes.Structure):
    """bmqcrc_storage_apply_result (include/bmqcrc_protocol.h, ABI 2.15)."""
    _fields_ = [("n_events", _u64), ("n_msgs", _u64), ("n_data", _u64), ("journal_bytes", _u64),
                ("data_bytes", _u64), ("head_seq", _u64), ("head_lease_id", _u32),
                ("refused_kind", _u32), ("n_bad", _u64), ("first_bad", _u64),
                ("refused_event", _u64), ("refused_index", _u64), ("refused_offset", _u64)]

    def as_dict(self):
        return {f[0]: int(getattr(self, f[0])) for f in self._fields_}


if hasattr(lib, "bmqcrc_storage_event_apply"):  # ABI 2.15 (an older build loads for same-box A/B)
    lib.bmqcrc_storage_event_apply.restype = _int
    lib.bmqcrc_storage_event_apply.argtypes = [ctypes.POINTER(StorageApply),
                                               ctypes.POINTER(StorageApplyResult), _popts]
    lib.bmqcrc_last_storage_apply.restype = _int
    lib.bmqcrc_last_storage_apply.argtypes = [_int, _vp, ctypes.POINTER(StorageApplyResult)]
BMQCRC_STORAGE_PACK_OK = 0
BMQCRC_STORAGE_PACK_RECORD_HEADER = 1
BMQCRC_STORAGE_PACK_DATA_OFFSET = 2
BMQCRC_STORAGE_PACK_DATA_RECORD = 3
BMQCRC_STORAGE_PACK_EVENT_FIRST = 4
BMQCRC_STORAGE_PACK_PAYLOAD_TOO_BIG = 5
BMQCRC_STORAGE_PACK_EVENT_TOO_BIG = 6
BMQCRC_STORAGE_PACK_DST_TOO_SMALL = 7
BMQCRC_STORAGE_PACK_TOO_MANY_PIECES = 8


class StoragePack(ctypes.Structure):
    """bmqcrc_storage_pack (include/bmqcrc_protocol.h, ABI 2.16)."""
    _fields_ = [("struct_size", _u32), ("reserved", _u32), ("journal", _vp),
                ("journal_bytes", _u64), ("n_records", _u64), ("journal_pos", _u64),
                ("data", _vp), ("data_bytes", _u64), ("data_file_pos", _u64),
                ("partition_id", _u32), ("event_type", _u32),
                ("storage_protocol_version", _u32), ("reserved2", _u32), ("flags", _vp),
                ("event_first", _vp), ("n_events", _u64), ("max_event_bytes", _u64),
                ("max_payload_bytes", _u64), ("dst", _vp), ("dst_bytes", _u64),
                ("event_offsets", _vp), ("types", _vp), ("out", _vp)]


class StoragePackResult(ctypes.Structure):
    """bmqcrc_storage_pack_result (include/bmqcrc_protocol.h, ABI 2.16)."""
    _fields_ = [("n_events", _u64), ("n_msgs", _u64), ("n_data", _u64), ("total_bytes", _u64),
                ("n_bad", _u64), ("first_bad", _u64), ("refused_kind", _u32), ("reserved", _u32),
                ("refused_index", _u64)]

    def as_dict(self):
        return {f[0]: int(getattr(self, f[0])) for f in self._fields_ if f[0] != "reserved"}


if hasattr(lib, "bmqcrc_storage_event_pack"):  # ABI 2.16 (an older build loads for same-box A/B)
    lib.bmqcrc_storage_event_pack.restype = _int
    lib.bmqcrc_storage_event_pack.argtypes = [ctypes.POINTER(StoragePack),
                                              ctypes.POINTER(StoragePackResult), _popts]
    lib.bmqcrc_last_storage_pack.restype = _int
    lib.bmqcrc_last_storage_pack.argtypes = [_int, _vp, ctypes.POINTER(StoragePackResult)]
BMQCRC_PUSH_PACK_OK = 0
BMQCRC_PUSH_PACK_RECORD_INDEX = 1
BMQCRC_PUSH_PACK_RECORD = 2
BMQCRC_PUSH_PACK_DATA_OFFSET = 3
BMQCRC_PUSH_PACK_DATA_RECORD = 4
BMQCRC_PUSH_PACK_FLAGS = 5
BMQCRC_PUSH_PACK_EVENT_FIRST = 6
BMQCRC_PUSH_PACK_PAYLOAD_TOO_BIG = 7
BMQCRC_PUSH_PACK_EVENT_TOO_BIG = 8
BMQCRC_PUSH_PACK_DST_TOO_SMALL = 9
BMQCRC_PUSH_PACK_TOO_MANY_PIECES = 10
BMQCRC_PUSH_OPTION_NONE = 0
BMQCRC_PUSH_OPTION_PACKED_RDA = 1
BMQCRC_PUSH_OPTION_SUB_QUEUE_ID = 2
BMQCRC_PUSH_OPTION_SUB_QUEUE_INFO = 3


class PushPack(ctypes.Structure):
    """bmqcrc_push_pack (include/bmqcrc_protocol.h, ABI 2.17)."""
    _fields_ = [("struct_size", _u32), ("reserved", _u32), ("journal", _vp),
                ("journal_bytes", _u64), ("n_records", _u64), ("data", _vp), ("data_bytes", _u64),
                ("data_file_pos", _u64), ("records", _vp), ("n", _u64), ("queue_ids", _vp),
                ("flags", _vp), ("option_mode", _u32), ("reserved2", _u32), ("rda", _vp),
                ("sub_ids", _vp), ("event_first", _vp), ("n_events", _u64),
                ("max_event_bytes", _u64), ("max_payload_bytes", _u64), ("dst", _vp),
                ("dst_bytes", _u64), ("event_offsets", _vp), ("out", _vp), ("lengths", _vp)]


class PushPackResult(ctypes.Structure):
    """bmqcrc_push_pack_result (include/bmqcrc_protocol.h, ABI 2.17)."""
    _fields_ = [("n_events", _u64), ("n_msgs", _u64), ("total_bytes", _u64), ("n_bad", _u64),
                ("first_bad", _u64), ("refused_kind", _u32), ("reserved", _u32),
                ("refused_index", _u64)]

    def as_dict(self):
        return {f[0]: int(getattr(self, f[0])) for f in self._fields_ if f[0] != "reserved"}


if hasattr(lib, "bmqcrc_push_event_pack"):  # ABI 2.17 (an older build loads for same-box A/B)
    lib.bmqcrc_push_event_pack.restype = _int
    lib.bmqcrc_push_event_pack.argtypes = [ctypes.POINTER(PushPack),
                                           ctypes.POINTER(PushPackResult), _popts]
    lib.bmqcrc_last_push_pack.restype = _int
    lib.bmqcrc_last_push_pack.argtypes = [_int, _vp, ctypes.POINTER(PushPackResult)]
BMQCRC_ROLLOVER_OK = 0
BMQCRC_ROLLOVER_RECORD_HEADER = 1
BMQCRC_ROLLOVER_KEEP_JOURNAL_OP = 2
BMQCRC_ROLLOVER_SYNC_POINT = 3
BMQCRC_ROLLOVER_DATA_OFFSET = 4
BMQCRC_ROLLOVER_DATA_RECORD = 5
BMQCRC_ROLLOVER_DST_TOO_SMALL = 6
BMQCRC_ROLLOVER_DATA_FILE_FULL = 7
BMQCRC_ROLLOVER_TOO_MANY_PIECES = 8
BMQCRC_ROLLOVER_CONFIRMS_AS_KEPT = 0
BMQCRC_ROLLOVER_CONFIRMS_FOLLOW_MESSAGES = 1
BMQCRC_ROLLOVER_NO_SYNC_POINT = 0xFFFFFFFFFFFFFFFF


class Rollover(ctypes.Structure):
    """bmqcrc_rollover (include/bmqcrc_protocol.h, ABI 2.18)."""
    _fields_ = [("struct_size", _u32), ("reserved", _u32), ("journal", _vp),
                ("journal_bytes", _u64), ("n_records", _u64), ("data", _vp), ("data_bytes", _u64),
                ("data_file_pos", _u64), ("keep", _vp), ("confirm_mode", _u32),
                ("reserved2", _u32), ("sync_point", _u64), ("timestamp", _u64),
                ("new_data_file_pos", _u64), ("dst", _vp), ("dst_bytes", _u64),
                ("journal_dst", _vp), ("journal_dst_bytes", _u64), ("new_index", _vp),
                ("out", _vp)]


class RolloverResult(ctypes.Structure):
    """bmqcrc_rollover_result (include/bmqcrc_protocol.h, ABI 2.18)."""
    _fields_ = [("n_records", _u64), ("n_kept", _u64), ("n_messages", _u64),
                ("journal_bytes", _u64), ("data_bytes", _u64), ("n_bad", _u64),
                ("first_bad", _u64), ("refused_kind", _u32), ("reserved", _u32),
                ("refused_index", _u64)]

    def as_dict(self):
        return {f[0]: int(getattr(self, f[0])) for f in self._fields_ if f[0] != "reserved"}


if hasattr(lib, "bmqcrc_partition_rollover"):  # ABI 2.18 (an older build loads for same-box A/B)
    lib.bmqcrc_partition_rollover.restype = _int
    lib.bmqcrc_partition_rollover.argtypes = [ctypes.POINTER(Rollover),
                                              ctypes.POINTER(RolloverResult), _popts]
    lib.bmqcrc_last_rollover.restype = _int
    lib.bmqcrc_last_rollover.argtypes = [_int, _vp, ctypes.POINTER(RolloverResult)]
BMQCRC_CONFIRM_PACK_OK = 0
BMQCRC_CONFIRM_PACK_RECORD_HEADER = 1
BMQCRC_CONFIRM_PACK_DUPLICATE_MESSAGE = 2
BMQCRC_CONFIRM_PACK_NULL_KEY = 3
BMQCRC_CONFIRM_PACK_REASON = 4
BMQCRC_CONFIRM_PACK_OVER_CONFIRMED = 5
BMQCRC_CONFIRM_PACK_DST_TOO_SMALL = 6


class ConfirmPack(ctypes.Structure):
    """bmqcrc_confirm_pack (include/bmqcrc_protocol.h, ABI 2.19)."""
    _fields_ = [("struct_size", _u32), ("reserved", _u32), ("journal", _vp),
                ("journal_bytes", _u64), ("n_records", _u64), ("select", _vp), ("guids", _vp),
                ("queue_keys", _vp), ("app_keys", _vp), ("reasons", _vp), ("timestamps", _vp),
                ("n", _u64), ("timestamp", _u64), ("first_seq", _u64), ("lease_id", _u32),
                ("reserved2", _u32), ("journal_dst", _vp), ("journal_dst_bytes", _u64),
                ("status", _vp), ("target", _vp), ("new_index", _vp), ("left_out", _vp)]


class ConfirmPackResult(ctypes.Structure):
    """bmqcrc_confirm_pack_result (include/bmqcrc_protocol.h, ABI 2.19)."""
    _fields_ = [("n_confirms", _u64), ("n_written", _u64), ("n_confirm_records", _u64),
                ("n_deletions", _u64), ("n_not_found", _u64), ("journal_bytes", _u64),
                ("next_seq", _u64), ("refused_kind", _u32), ("reserved", _u32),
                ("refused_index", _u64)]

    def as_dict(self):
        return {f[0]: int(getattr(self, f[0])) for f in self._fields_ if f[0] != "reserved"}


if hasattr(lib, "bmqcrc_confirm_records_pack"):  # ABI 2.19 (an older build loads for same-box A/B)
    lib.bmqcrc_confirm_records_pack.restype = _int
    lib.bmqcrc_confirm_records_pack.argtypes = [ctypes.POINTER(ConfirmPack),
                                                ctypes.POINTER(ConfirmPackResult), _popts]
    lib.bmqcrc_last_confirm_records.restype = _int
    lib.bmqcrc_last_confirm_records.argtypes = [_int, _vp, ctypes.POINTER(ConfirmPackResult)]
BMQCRC_EXPIRE_PACK_OK = 0
BMQCRC_EXPIRE_PACK_RECORD_HEADER = 1
BMQCRC_EXPIRE_PACK_DUPLICATE_MESSAGE = 2
BMQCRC_EXPIRE_PACK_QUEUE_KEY = 3
BMQCRC_EXPIRE_PACK_DST_TOO_SMALL = 4


class ExpirePack(ctypes.Structure):
    """bmqcrc_expire_pack (include/bmqcrc_protocol.h, ABI 2.20)."""
    _fields_ = [("struct_size", _u32), ("reserved", _u32), ("journal", _vp),
                ("journal_bytes", _u64), ("n_records", _u64), ("select", _vp),
                ("queue_keys", _vp), ("ttl_seconds", _vp), ("n_queues", _u64), ("now", _u64),
                ("first_seq", _u64), ("lease_id", _u32), ("reserved2", _u32),
                ("journal_dst", _vp), ("journal_dst_bytes", _u64), ("expired", _vp),
                ("new_index", _vp), ("select_out", _vp), ("queue_expired", _vp),
                ("queue_front", _vp)]


class ExpirePackResult(ctypes.Structure):
    """bmqcrc_expire_pack_result (include/bmqcrc_protocol.h, ABI 2.20)."""
    _fields_ = [("n_records", _u64), ("n_live", _u64), ("n_expired", _u64),
                ("n_no_queue", _u64), ("journal_bytes", _u64), ("next_seq", _u64),
                ("refused_kind", _u32), ("reserved", _u32), ("refused_index", _u64)]

    def as_dict(self):
        return {f[0]: int(getattr(self, f[0])) for f in self._fields_ if f[0] != "reserved"}


if hasattr(lib, "bmqcrc_expire_records_pack"):  # ABI 2.20 (an older build loads for same-box A/B)
    lib.bmqcrc_expire_records_pack.restype = _int
    lib.bmqcrc_expire_records_pack.argtypes = [ctypes.POINTER(ExpirePack),
                                               ctypes.POINTER(ExpirePackResult), _popts]
    lib.bmqcrc_last_expire_records.restype = _int
    lib.bmqcrc_last_expire_records.argtypes = [_int, _vp, ctypes.POINTER(ExpirePackResult)]
BMQCRC_PENDING_LIST_OK = 0
BMQCRC_PENDING_LIST_RECORD_HEADER = 1
BMQCRC_PENDING_LIST_DUPLICATE_MESSAGE = 2
BMQCRC_PENDING_LIST_QUEUE_KEY = 3
BMQCRC_PENDING_LIST_APP_FIRST = 4
BMQCRC_PENDING_LIST_APP_KEY = 5
BMQCRC_PENDING_LIST_FROM_RECORD = 6
BMQCRC_PENDING_LIST_LIST_TOO_SMALL = 7


class PendingList(ctypes.Structure):
    """bmqcrc_pending_list (include/bmqcrc_protocol.h, ABI 2.21)."""
    _fields_ = [("struct_size", _u32), ("reserved", _u32), ("journal", _vp),
                ("journal_bytes", _u64), ("n_records", _u64), ("select", _vp),
                ("queue_keys", _vp), ("app_first", _vp), ("n_queues", _u64), ("app_keys", _vp),
                ("queue_ids", _vp), ("sub_ids", _vp), ("from_record", _vp), ("limit", _vp),
                ("n_apps", _u64), ("records", _vp), ("out_queue_ids", _vp),
                ("out_sub_ids", _vp), ("list_cap", _u64), ("list_first", _vp),
                ("app_pending", _vp), ("app_next", _vp), ("pending_mask", _vp)]


class PendingListResult(ctypes.Structure):
    """bmqcrc_pending_list_result (include/bmqcrc_protocol.h, ABI 2.21)."""
    _fields_ = [("n_records", _u64), ("n_live", _u64), ("n_no_queue", _u64),
                ("n_pending", _u64), ("n_listed", _u64), ("n_unknown_confirms", _u64),
                ("n_not_found", _u64), ("refused_kind", _u32), ("reserved", _u32),
                ("refused_index", _u64)]

    def as_dict(self):
        return {f[0]: int(getattr(self, f[0])) for f in self._fields_ if f[0] != "reserved"}


if hasattr(lib, "bmqcrc_pending_records_list"):  # ABI 2.21 (an older build loads for same-box A/B)
    lib.bmqcrc_pending_records_list.restype = _int
    lib.bmqcrc_pending_records_list.argtypes = [ctypes.POINTER(PendingList),
                                                ctypes.POINTER(PendingListResult), _popts]
    lib.bmqcrc_last_pending_records.restype = _int
    lib.bmqcrc_last_pending_records.argtypes = [_int, _vp, ctypes.POINTER(PendingListResult)]
lib.bmqcrc_journal_scan.restype = _i64
lib.bmqcrc_journal_scan.argtypes = [_vp, _u64, _vp, _u64, _vp, _pint, _pu64, _vp, _vp, _vp, _vp,
                                    _u64]
lib.bmqcrc_journal_bounds.restype = _int
lib.bmqcrc_journal_bounds.argtypes = [_vp, _u64, _pu64, _pu64]
lib.bmqcrc_recover_verify.restype = _int
lib.bmqcrc_recover_verify.argtypes = [_vp, _u64, _vp, _u64, _vp, _pint, _pu64, _pu64, _pu64, _vp,
                                      _u64, _popts]
lib.bmqcrc_csl_scan.restype = _i64
lib.bmqcrc_csl_scan.argtypes = [_vp, _u64, _vp, _vp, _vp, _vp, _u64, _pint, _pu64]
lib.bmqcrc_csl_validate.restype = _int
lib.bmqcrc_csl_validate.argtypes = [_vp, _u64, _vp, _pint, _pu64, _pu64, _popts]


def check(rc):
    if rc != BMQCRC_OK:
        raise BmqCrcError(rc, lib.bmqcrc_last_error().decode(errors="replace"))
    return rc


def check_count(n):
    """Scans return a count (>= 0) or a negative BMQCRC_E* code."""
    if n < 0:
        raise BmqCrcError(n, lib.bmqcrc_last_error().decode(errors="replace"))
    return n


def make_opts(device=-1, stream=None, flags=0, seg_bytes=0, devices=None, max_len=0,
              min_len=0, offset_shift=None):
    """bmqcrc_opts; `devices` (a sequence of ordinals, repeats allowed) spreads
    the format-walk entry points over several devices (ABI 2.1); `max_len`
    and `min_len` declare bounds on a device-resident batch's lengths (ABI 2.4);
    `offset_shift` (an int in 0..7, ABI 2.8) sets BMQCRC_F_OFFSETS32: the
    offsets are uint32 in units of 1 << offset_shift bytes."""
    o = Opts()
    o.struct_size = ctypes.sizeof(Opts)
    o.device = device
    o.stream = stream
    o.flags = flags
    o.seg_bytes = seg_bytes
    o.max_len = max_len
    o.min_len = min_len
    if offset_shift is not None:
        o.flags |= BMQCRC_F_OFFSETS32
        o.offset_shift = offset_shift
    if devices is not None and len(devices) > 1:
        arr = (ctypes.c_int32 * len(devices))(*devices)
        o._devices_keep = arr  # the array lives as long as the opts
        o.ndevices = len(devices)
        o.devices = ctypes.cast(arr, ctypes.c_void_p)
    return o
