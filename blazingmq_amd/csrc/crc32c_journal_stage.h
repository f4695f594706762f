// crc32c_journal_stage.h -- how the kernels that read journal records bring
// them in, and the two checks every one of them makes before it trusts a
// record: the RecordHeader's and, for a MESSAGE record, its DATA record's.
// Device only, in the anonymous namespace like the units' own code.
//
//   stage               crc32c_records_unpack.hip, crc32c_journal_select.hip,
//                       crc32c_storage_pack.hip, crc32c_rollover.hip
//   record_header_ok,   crc32c_records_unpack.hip, crc32c_storage_pack.hip,
//   data_window_offset, crc32c_push_pack.hip, crc32c_rollover.hip
//   data_record         (DESIGN.md sections 15, 18, 19, 20)
//
// The grid is nblocks x kPackThreads over contiguous record ranges
// (layout_split), one record per thread and step.  A wave brings its 64
// records into LDS with 15 coalesced dword loads per lane and every lane reads
// its own record from there at a 15-dword stride (15 is odd: the lanes' dwords
// fall into different banks).
//
// data_record is the one piece of code that decides which bytes of the
// caller's DATA window [data, +data_bytes) a classify kernel loads: the two
// DataHeader words after ow + 8 <= end, the padding byte after
// ow + total <= end, nothing else.  The host walk makes the same decision
// (walk_recovery, bmqcrc_protocol.cpp); tests/test_data_record_cases.py holds
// the two and the units' models to one table.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmqcrc_internal.h"

namespace bmqcrc {
namespace {

constexpr uint32_t kWaves = kPackThreads / 64;
constexpr uint32_t kWaveDwords = 64 * kJournalRecordDwords;  // a wave's 64 records: 3,840 bytes
constexpr uint32_t kMagicLE = 0x6345722Au;                   // bytes 2A 72 45 63 loaded as a dword
// RecordType (mqbs_filestoreprotocol.h); the type field has four bits
constexpr uint32_t kRecMessage = 1, kRecConfirm = 2, kRecDeletion = 3, kRecQueueOp = 4,
                   kRecJournalOp = 5, kRecAnyType = 15;

// Records [r0, r0 + 64) below `hi` into the wave's kWaveDwords of LDS: lane l
// loads dwords l, l + 64, ... of the wave's run, all in flight together.
__device__ __forceinline__ void stage(const uint32_t* journal, uint64_t r0, uint64_t hi,
                                      uint32_t* mine, uint32_t lane)
{
    const uint32_t cnt = r0 < hi ? (uint32_t)min(hi - r0, (uint64_t)64) : 0u;
    const uint32_t ndw = cnt * kJournalRecordDwords;
    const uint32_t* g = journal + kJournalRecordDwords * r0;
    uint32_t v[kJournalRecordDwords];
#pragma unroll
    for (uint32_t j = 0; j < kJournalRecordDwords; ++j) {
        const uint32_t i = 64u * j + lane;
        v[j] = i < ndw ? g[i] : 0u;
    }
#pragma unroll
    for (uint32_t j = 0; j < kJournalRecordDwords; ++j) {
        mine[64u * j + lane] = v[j];
    }
}

// The RecordHeader of a record, from its dwords 0 (byte-swapped: type | flags |
// the sequence number's top), 1, 2 and 14: a type in [1, max_type], a lease id,
// a sequence number and the magic.
__device__ __forceinline__ bool record_header_ok(uint32_t w0, uint32_t d1, uint32_t d2,
                                                 uint32_t d14, uint32_t max_type)
{
    const uint32_t type = w0 >> 28;
    return !(type == 0 || type > max_type || d2 == 0 || ((w0 & 0xFFFFu) == 0 && d1 == 0) ||
             d14 != kMagicLE);
}

// Where a MESSAGE record's DATA record begins in the window that holds the
// DATA file from data_file_pos on, from its dword 8 (MessageOffsetDwords):
// *ow, a multiple of 8 and at most `end`, the window's bytes.  False: offset 0,
// or outside the window.
__device__ __forceinline__ bool data_window_offset(uint32_t d8, uint64_t data_file_pos,
                                                   uint64_t end, uint64_t* ow)
{
    const uint64_t o = (uint64_t)__builtin_bswap32(d8) * 8;
    if (o == 0 || o < data_file_pos || o - data_file_pos > end) {
        return false;
    }
    *ow = o - data_file_pos;
    return true;
}

// A well-formed DATA record: DataHeader, options, application data, 1..8
// padding bytes, each equal to their count.
struct DataRecord {
    uint64_t hdr;    // header + options bytes
    uint64_t total;  // the whole record's, at most 2^31 - 4
    uint64_t app;    // the application data's window offset
    uint32_t len;    // ... and its length
    uint32_t h1;     // the second DataHeader word: options words | flags
};

// The DATA record at window offset ow (from data_window_offset) of the window
// [data, +end).  Loads the header's 8 bytes after ow + 8 <= end and the last
// padding byte after ow + total <= end, and no other byte.  with_header(hs) is
// called with the header's bytes once the record is known to lie inside the
// window, after the padding byte's load and before its test: a caller's own
// load of a header field goes there, in flight with that byte.
template <class WithHeader>
__device__ __forceinline__ bool data_record(const uint8_t* data, uint64_t end, uint64_t ow,
                                            DataRecord* r, WithHeader with_header)
{
    bool bad = ow + 8 > end;
    if (!bad) {
        const uint64_t hw = *(const uint64_t*)(data + ow);
        const uint32_t h0 = __builtin_bswap32((uint32_t)hw);
        const uint32_t h1 = __builtin_bswap32((uint32_t)(hw >> 32));
        const uint64_t hs = (uint64_t)(h0 >> 29) * 4;
        const uint64_t total = (uint64_t)(h0 & 0x1FFFFFFFu) * 4;
        const uint64_t opt = (uint64_t)(h1 >> 8) * 4;
        bad = hs == 0 || total == 0 || hs + opt >= total || ow + total > end;
        if (!bad) {
            const uint32_t pad = data[ow + total - 1];
            with_header(hs);
            bad = pad < 1 || pad > 8 || total < hs + opt + pad;
            if (!bad) {
                r->hdr = hs + opt;
                r->total = total;
                r->app = ow + hs + opt;
                r->len = (uint32_t)(total - hs - opt - pad);
                r->h1 = h1;
            }
        }
    }
    return !bad;
}

__device__ __forceinline__ bool data_record(const uint8_t* data, uint64_t end, uint64_t ow,
                                            DataRecord* r)
{
    return data_record(data, end, ow, r, [](uint64_t) {});
}

}  // namespace
}  // namespace bmqcrc
