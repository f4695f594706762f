// crc32c_unpack_slots.h -- the slot pass the device unpackers share
// (crc32c_put_unpack.hip, crc32c_records_unpack.hip, crc32c_storage_apply.hip;
// DESIGN.md sections 14, 15, 17).  Device only, in the anonymous namespace like
// the units' own code.  A template over the unit's args struct (UnpackArgs,
// RecUnpackArgs, SapArgs), of which it uses msg_cap, ws_off and ws_len.
//
// A slot is one message the call found: the placing kernel leaves its offset,
// length and stored CRC in the workspace, the fold reads the first two of all
// msg_cap slots and writes ws_out, and the publish kernel hands the four to
// the caller (the kSlotCtr* words of bmqcrc_internal.h count what it finds).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmqcrc_internal.h"

namespace bmqcrc {
namespace {

// The slots [used, msg_cap) no message took become empty messages (offset 0,
// length 0), so the fold never reads a descriptor the walk did not validate.
// Called by every thread of the placing grid, of block_threads a block.
template <class Args>
__device__ __forceinline__ void empty_slots(const Args& a, uint64_t used, uint32_t block_threads)
{
    const uint64_t stride = (uint64_t)gridDim.x * block_threads;
    for (uint64_t i = used + (uint64_t)blockIdx.x * block_threads + threadIdx.x; i < a.msg_cap;
         i += stride) {
        a.ws_off[i] = 0;
        a.ws_len[i] = 0;
    }
}

}  // namespace
}  // namespace bmqcrc
