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
// The refusal word, pass 1's scan and the prefix of the block sums are shared
// with crc32c_records_pack.hip and described in crc32c_pack_layout.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmqcrc_internal.h"
#include "crc32c_pack_layout.h"

namespace bmqcrc {
namespace {

// byte-aligned dword: a GUID array need not be 4-byte aligned
typedef uint32_t u32u __attribute__((aligned(1)));

constexpr uint32_t kPutHeaderBytes = 36, kEventHeaderBytes = 8;

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
    const uint32_t tid = threadIdx.x;
    // event_first: starts at 0, strictly increasing, ends at n
    if (a.event_first) {
        const uint64_t stride = (uint64_t)gridDim.x * kPackThreads;
        for (uint64_t e = (uint64_t)blockIdx.x * kPackThreads + tid; e <= a.n_events; e += stride) {
            const uint64_t f = a.event_first[e];
            const bool bad = e == a.n_events ? f != a.n
                                             : (e == 0 && f != 0) || f >= a.event_first[e + 1];
            if (bad) {
                refuse(a, BMQCRC_PACK_KIND_EVENT_FIRST, e);
            }
        }
    }
}

// Pass 2: the events, one per thread.  Runs only on a clean pass 1: every
// event_first entry is then at most n.
__global__ __launch_bounds__(kPackThreads) void k_pack_check(PackArgs a)
{
    __shared__ unsigned long long bpre[kPackBlocks + 1];
    if (a.ctr[kPackCtrRefusal] != 0) {
        return;
    }
    const unsigned long long pieces = block_prefix(a, bpre);
    const unsigned long long all = bpre[a.nblocks];
    const uint64_t stride = (uint64_t)gridDim.x * kPackThreads;
    for (uint64_t e = (uint64_t)blockIdx.x * kPackThreads + threadIdx.x; e < a.n_events;
         e += stride) {
        const uint64_t f0 = a.event_first ? a.event_first[e] : 0;
        const uint64_t f1 = a.event_first ? a.event_first[e + 1] : a.n;
        const unsigned long long p0 = a.off[f0] + bpre[f0 / a.per_block];  // f0 < f1 <= n
        const unsigned long long p1 = f1 == a.n ? all : a.off[f1] + bpre[f1 / a.per_block];
        if (kEventHeaderBytes + (p1 - p0) > a.max_event_bytes) {
            refuse(a, BMQCRC_PACK_KIND_EVENT_TOO_BIG, e);
        }
        if (kEventHeaderBytes * (e + 1) + p1 > a.dst_bytes) {
            refuse(a, BMQCRC_PACK_KIND_DST_TOO_SMALL, e);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (pieces > 0xFFFFFFFFull) {
            refuse(a, BMQCRC_PACK_KIND_TOO_MANY_PIECES, 0);
        }
        a.ctr[kPackCtrTotal] = kEventHeaderBytes * a.n_events + all;
    }
}

// Last e in [lo, hi] with first[e] <= i (first[lo] <= i is given).
__device__ __forceinline__ uint64_t event_of(const uint64_t* first, uint64_t lo, uint64_t hi,
                                             uint64_t i)
{
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (first[mid] <= i) {
            lo = mid;
        } else {
            hi = mid - 1;
        }
    }
    return lo;
}

// Pass 3: off[i] = where message i's application data goes.
__global__ __launch_bounds__(kPackThreads) void k_pack_place(PackArgs a)
{
    __shared__ unsigned long long bpre[kPackBlocks + 1];
    __shared__ uint64_t erange[2];
    const uint32_t tid = threadIdx.x;
    const uint64_t lo = (uint64_t)blockIdx.x * a.per_block;
    const uint64_t hi = min(lo + a.per_block, a.n);
    if (a.ctr[kPackCtrRefusal] != 0) {
        // past any dst_bytes: the copy kernels refuse the message
        for (uint64_t i = lo + tid; i < hi; i += kPackThreads) {
            a.off[i] = ~0ull;
        }
        return;
    }
    if (tid == 0) {
        // the events of this block's messages: the search of a message stays
        // inside them (one or two events, usually)
        uint64_t e0 = 0, e1 = 0;
        if (a.event_first && lo < hi) {
            e0 = event_of(a.event_first, 0, a.n_events - 1, lo);
            e1 = event_of(a.event_first, e0, a.n_events - 1, hi - 1);
        }
        erange[0] = e0;
        erange[1] = e1;
    }
    block_prefix(a, bpre);
    const unsigned long long before = bpre[blockIdx.x];
    const uint64_t e0 = erange[0], e1 = erange[1];
    for (uint64_t i = lo + tid; i < hi; i += kPackThreads) {
        const uint64_t e = e0 == e1 ? e0 : event_of(a.event_first, e0, e1, i);
        a.off[i] = a.off[i] + before + kEventHeaderBytes * (e + 1) + kPutHeaderBytes;
    }
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
    const uint64_t total = a.ctr[kPackCtrTotal];
    for (uint64_t e = t0; e <= a.n_events; e += stride) {
        // event e starts 8 + 36 bytes before its first message's data
        const uint64_t at = e == a.n_events
                                ? total
                                : a.off[a.event_first ? a.event_first[e] : 0] -
                                      (kEventHeaderBytes + kPutHeaderBytes);
        if (a.event_offsets) {
            a.event_offsets[e] = at;
        }
        if (e < a.n_events) {
            const uint64_t next = e + 1 == a.n_events
                                      ? total
                                      : a.off[a.event_first[e + 1]] -
                                            (kEventHeaderBytes + kPutHeaderBytes);
            uint32_t* h = (uint32_t*)(a.dst + at);
            h[0] = __builtin_bswap32((uint32_t)(next - at) & 0x7FFFFFFFu);
            h[1] = 0x00000242u;  // bytes: PV 1 | type PUT 2, HeaderWords 2, 0, 0
        }
    }
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
