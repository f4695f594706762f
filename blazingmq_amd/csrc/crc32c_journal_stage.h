// crc32c_journal_stage.h -- how the kernels that read journal records bring
// them in (crc32c_records_unpack.hip, crc32c_journal_select.hip).  Device only,
// in the anonymous namespace like the units' own code.
//
// The grid is nblocks x kPackThreads over contiguous record ranges
// (layout_split), one record per thread and step.  A wave brings its 64
// records into LDS with 15 coalesced dword loads per lane and every lane reads
// its own record from there at a 15-dword stride (15 is odd: the lanes' dwords
// fall into different banks).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmqcrc_internal.h"

namespace bmqcrc {
namespace {

constexpr uint32_t kWaves = kPackThreads / 64;
constexpr uint32_t kWaveDwords = 64 * kJournalRecordDwords;  // a wave's 64 records: 3,840 bytes
constexpr uint32_t kMagicLE = 0x6345722Au;                   // bytes 2A 72 45 63 loaded as a dword

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

}  // namespace
}  // namespace bmqcrc
