// crc32c_put_pack.hip -- MI355X (gfx950) PUT-event framing around the fused
// copy + CRC (bmqcrc_put_event_pack, ABI 2.10).
//
// The device-side producer that PutEventBuilder::packMessage is on the host:
// per message a 36-byte PutHeader, the application data, 1..4 padding bytes
// each equal to their count; per event an 8-byte EventHeader.  No options, no
// compression, no schema id.
//
// With B[i] = 36 + lengths[i] + pad(lengths[i]) and P its 64-bit exclusive
// prefix, message i's header lies at 8 (e(i) + 1) + P[i] and event e starts at
// 8 e + P[event_first[e]].  Three steps on one stream:
//
//   1. Layout.  k_pack_count: pass 1 of crc32c_pack_layout.h over B, with
//      every source range checked; then event_first's shape.
//      k_pack_check (only when pass 1 refused nothing, so every event_first
//      entry is a valid index): P[j] = off[j] + the sum of the blocks before
//      j's; every event's length against the cap and its end against
//      dst_bytes.  k_pack_place: off[i] becomes the payload's destination
//      offset, 8 (e(i) + 1) + P[i] + 36 -- or, when anything was refused, an
//      offset past dst_bytes for EVERY message: the copy kernels then refuse
//      every message, own no piece and write neither dst nor out.
//   2. Payload.  bmqcrc_launch_copy (crc32c_copy.hip), as it is.
//   3. Frame.  k_pack_frame, after the fold, when out[i] is final: the 9
//      header dwords of every message, indexed across the grid so that
//      adjacent lanes store adjacent dwords; the padding bytes as byte stores;
//      the EventHeaders and event_offsets.  It leaves at once on a refusal.
//
// The refusal word, pass 1's scan, the prefix of the block sums and the event
// split (event_first's shape, the events' checks, the search of a message's
// event, the EventHeaders) are shared with the other packers and described in
// crc32c_pack_layout.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmqcrc_internal.h"
#include "crc32c_pack_layout.h"

namespace bmqcrc {
namespace {

// byte-aligned dword: a GUID array need not be 4-byte aligned
typedef uint32_t u32u __attribute__((aligned(1)));

constexpr uint32_t kPutHeaderBytes = 36;

// PutHeader + application data + padding (calcNumWordsAndPadding: 1..4 bytes)
__device__ __forceinline__ uint64_t framed_bytes(uint32_t len)
{
    return (uint64_t)kPutHeaderBytes + (((uint64_t)len >> 2) + 1) * 4;
}

// Pass 1: the shared scan, then event_first's shape.
__global__ __launch_bounds__(kPackThreads) void k_pack_count(PackArgs a)
{
    layout_count(a, [&a](uint64_t i, uint64_t so, uint32_t len) {
        if (!(so <= a.src_bytes && len <= a.src_bytes - so)) {
            refuse(a, BMQCRC_PACK_KIND_SRC_RANGE, i);
        }
        return framed_bytes(len);
    });
    event_first_shape(a, BMQCRC_PACK_KIND_EVENT_FIRST);
}

// Pass 2: the events, one per thread.  Runs only on a clean pass 1: every
// event_first entry is then at most n.
__global__ __launch_bounds__(kPackThreads) void k_pack_check(PackArgs a)
{
    if (a.ctr[kPackCtrRefusal] != 0) {
        return;
    }
    events_check(a, BMQCRC_PACK_KIND_EVENT_TOO_BIG, BMQCRC_PACK_KIND_DST_TOO_SMALL,
                 BMQCRC_PACK_KIND_TOO_MANY_PIECES, kPackCtrTotal);
}

// Pass 3: off[i] = where message i's application data goes.
__global__ __launch_bounds__(kPackThreads) void k_pack_place(PackArgs a)
{
    seal_offsets(a, [](uint64_t) { return kPutHeaderBytes; });
}

// Step 3.  Thread t of the grid owns header dword t % 9 of message t / 9.
__global__ __launch_bounds__(kPackFrameThreads) void k_pack_frame(PackArgs a)
{
    if (a.ctr[kPackCtrRefusal] != 0) {
        return;
    }
    const uint64_t stride = (uint64_t)gridDim.x * kPackFrameThreads;
    const uint64_t t0 = (uint64_t)blockIdx.x * kPackFrameThreads + threadIdx.x;
    const uint64_t ndw = 9 * a.n;
    // (n < 2^32: a dword's index needs 36 bits, its message's 32)
    const bool narrow = ndw <= 0xFFFFFFFFull;
    // (Four dwords per thread and step, their loads in flight together, was
    // measured and was no faster: 78.6 against 66.7 us on 1M x 256 B.)
    for (uint64_t t = t0; t < ndw; t += stride) {
        // the division in 32 bits whenever the call's indices fit
        const uint64_t m = narrow ? (uint32_t)t / 9u : t / 9;
        const uint32_t j = (uint32_t)(t - 9 * m);
        const uint64_t app = a.off[m];
        uint32_t v = 0;
        if (j == 0) {
            // Flags(4) | MessageWords(28): header, data and padding in words
            const uint32_t words = 9u + (a.lengths[m] >> 2) + 1u;
            v = __builtin_bswap32(((a.flags ? (uint32_t)a.flags[m] & 0xFu : 0u) << 28) | words);
        } else if (j == 1) {
            v = __builtin_bswap32(9u);  // OptionsWords 0 | CAT 0 | HeaderWords 9
        } else if (j == 2) {
            v = __builtin_bswap32((uint32_t)a.queue_ids[m]);
        } else if (j < 7) {
            v = ((const u32u*)a.guids)[4 * m + (j - 3)];
        } else if (j == 7) {
            v = __builtin_bswap32(a.out[m]);
        } else {
            // SchemaId 0, Reserved 0 -- and this lane writes the padding
            const uint32_t len = a.lengths[m];
            const uint32_t pad = 4u - (len & 3u);
            uint8_t* p = a.dst + app + len;
            for (uint32_t k = 0; k < pad; ++k) {
                p[k] = (uint8_t)pad;
            }
        }
        ((uint32_t*)(a.dst + (app - kPutHeaderBytes)))[j] = v;
    }
    // event e starts 8 + 36 bytes before its first message's data
    event_headers(a, [](uint64_t) { return kPutHeaderBytes; }, 0x42u /* PV 1 | PUT 2 */,
                  a.ctr[kPackCtrTotal]);
}

}  // namespace
}  // namespace bmqcrc

using namespace bmqcrc;

extern "C" int bmqcrc_launch_put_layout(const PackArgs* a, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    const uint64_t eblocks = (a->n_events + kPackThreads - 1) / kPackThreads;
    const uint32_t check = (uint32_t)(eblocks < 1 ? 1 : eblocks > kPackBlocks ? kPackBlocks : eblocks);
    hipLaunchKernelGGL(k_pack_count, dim3(a->nblocks), dim3(kPackThreads), 0, s, *a);
    hipLaunchKernelGGL(k_pack_check, dim3(check), dim3(kPackThreads), 0, s, *a);
    hipLaunchKernelGGL(k_pack_place, dim3(a->nblocks), dim3(kPackThreads), 0, s, *a);
    return hipGetLastError() != hipSuccess;
}

extern "C" int bmqcrc_launch_put_frame(const PackArgs* a, void* stream)
{
    const uint64_t work = 9 * a->n > a->n_events + 1 ? 9 * a->n : a->n_events + 1;
    const uint64_t want = (work + kPackFrameThreads - 1) / kPackFrameThreads;
    const uint32_t blocks = (uint32_t)(want > kPackFrameBlocks ? kPackFrameBlocks : want);
    hipLaunchKernelGGL(k_pack_frame, dim3(blocks), dim3(kPackFrameThreads), 0, (hipStream_t)stream,
                       *a);
    return hipGetLastError() != hipSuccess;
}
