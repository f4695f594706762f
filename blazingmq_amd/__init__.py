"""blazingmq_amd -- MI355X-native replacement for BlazingMQ's per-message
CRC32C integrity-checksum path (bmqp::Crc32c and its batch callers).

The product is the C-ABI library ``lib/libbmqcrc.so`` (HIP kernels for gfx950
+ host dispatcher); this package is its Python host-side mirror.
"""
from .crc32c import (Blob, BmqCrcError, Crc32c, HostRegistration,  # noqa: F401
                     calculate_batch_multi, calculate_batch_ptr, device_count, fill_synthetic,
                     forget_shape, kernel_timing, last_copy, last_launch, last_offsets, plan_wait,
                     reserve)
from .confirm_event import (ConfirmEventBuilder, ConfirmMessageIterator,  # noqa: F401
                            confirm_arrays)
from .put_event import (last_put_pack, last_put_unpack, pack_events,  # noqa: F401
                        unpack_events)
from .push_event import (PushEventBuilder, PushMessageIterator, last_push_pack,  # noqa: F401
                         pack_push_events)
from .storage import (confirm_records, expire_records, last_confirm_records,  # noqa: F401
                      last_expire_records, last_journal_select, last_pending_records,
                      last_records_pack, last_records_unpack, last_rollover, pack_records,
                      pending_records, rollover_records, select_records, unpack_records)
from .storage_event import (StorageEventBuilder, StorageMessageIterator,  # noqa: F401
                            apply_events, last_storage_apply, last_storage_pack,
                            pack_storage_events)

__all__ = ["Blob", "BmqCrcError", "Crc32c", "HostRegistration", "PushEventBuilder",
           "PushMessageIterator", "last_push_pack", "pack_push_events", "StorageEventBuilder",
           "StorageMessageIterator", "apply_events", "last_storage_apply", "calculate_batch_multi",
           "calculate_batch_ptr", "device_count", "fill_synthetic", "forget_shape", "plan_wait",
           "kernel_timing", "last_copy", "last_journal_select", "last_launch", "last_offsets",
           "last_put_pack", "last_put_unpack", "last_records_pack", "last_records_unpack",
           "last_rollover", "last_storage_pack", "pack_events", "pack_records", "pack_storage_events",
           "reserve", "rollover_records", "select_records", "unpack_events", "unpack_records",
           "confirm_records", "last_confirm_records", "expire_records", "last_expire_records",
           "pending_records", "last_pending_records", "ConfirmEventBuilder",
           "ConfirmMessageIterator", "confirm_arrays"]
