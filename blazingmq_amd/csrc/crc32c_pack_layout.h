// crc32c_pack_layout.h -- the layout passes the device calls share (DESIGN.md
// sections 12, 13 and "Which header owns which shared pass").  Device only, in
// the anonymous namespace like the units' own code.  Templates over the unit's
// args struct, or over a LayoutView of it, of which they use src_offsets,
// lengths, n, off, bsum, ctr, per_block and nblocks.
//
//   refuse, wave_sum, tile_scan, block_prefix   every unit below
//   layout_count     crc32c_put_pack.hip, crc32c_records_pack.hip,
//                    crc32c_storage_apply.hip, crc32c_storage_pack.hip,
//                    crc32c_push_pack.hip, crc32c_rollover.hip
//   event_first_shape, events_check, event_of, seal_offsets, event_headers
//                    crc32c_put_pack.hip, crc32c_storage_pack.hip,
//                    crc32c_push_pack.hip (the event split, at the end)
//   (refuse, wave_sum, tile_scan, block_prefix alone: crc32c_put_unpack.hip,
//   crc32c_records_unpack.hip)
//
// Pass 1 (layout_count): the grid is nblocks x kPackThreads and block b owns
// the contiguous messages [b per_block, (b + 1) per_block).  With B[i] the
// framed bytes of message i, which the unit's `size` gives, off[i] becomes the
// BLOCK-LOCAL exclusive prefix of B, bsum[b] the block's sum of B and
// bsum[kPackBlocks + b] a bound on the block's 16-byte pieces of payload.  A
// later kernel turns the block sums into their own prefix (block_prefix), and
// off[i] + bpre[i / per_block] is the 64-bit exclusive prefix over the call.
//
// A refusal is one 64-bit word: ~((kind << 56) | index), raised with
// atomicMax, so the lowest kind and within it the lowest index wins whatever
// the order the blocks run in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmqcrc_internal.h"

namespace bmqcrc {
namespace {

template <class Args>
__device__ __forceinline__ void refuse(const Args& a, uint32_t kind, uint64_t index)
{
    atomicMax(&a.ctr[kLayoutCtrRefusal], ~(((unsigned long long)kind << 56) | index));
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        v += __shfl_down(v, d);
    }
    return v;  // lane 0
}

static_assert(kUnpackThreads == kPackThreads, "tile_scan: one tile is kPackThreads values");

// One tile of a 64-bit scan over the block's kPackThreads threads: returns the
// sum of the v of the threads before this one, *total = of all.  Called by the
// whole block; wtot is __shared__, kPackThreads / 64 words.  The first barrier
// follows the caller's loads of the tile, the second precedes its stores.
__device__ __forceinline__ unsigned long long tile_scan(unsigned long long v,
                                                        unsigned long long* wtot,
                                                        unsigned long long* total)
{
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    unsigned long long incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(incl, d);
        incl += lane >= (uint32_t)d ? o : 0ull;
    }
    if (lane == 63) {
        wtot[wv] = incl;
    }
    __syncthreads();
    unsigned long long woff = 0, tot = 0;
    for (uint32_t w = 0; w < kPackThreads / 64; ++w) {
        woff += w < wv ? wtot[w] : 0ull;
        tot += wtot[w];
    }
    __syncthreads();
    *total = tot;
    return woff + incl - v;
}

// What layout_count and block_prefix take of an args struct, for a unit whose
// messages are not its args' own src_offsets / lengths / n (the workspace's
// slots or records), or that scans a second prefix.
struct LayoutView {
    const unsigned long long* src_offsets;
    const uint32_t* lengths;
    uint64_t n;
    unsigned long long* off;
    unsigned long long* bsum;
    unsigned long long* ctr;
    uint64_t per_block;
    uint32_t nblocks;
};

// Pass 1, called by the whole block.  size(i, src_offset, len) returns B[i]
// and raises the unit's refusals of message i.
template <class Args, class Size>
__device__ __forceinline__ void layout_count(const Args& a, Size size)
{
    __shared__ unsigned long long wtot[kPackThreads / 64];
    __shared__ unsigned long long wpieces[kPackThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint64_t lo = (uint64_t)blockIdx.x * a.per_block;
    const uint64_t hi = min(lo + a.per_block, a.n);
    unsigned long long carry = 0, pieces = 0;
    for (uint64_t base = lo; base < hi; base += kPackThreads) {
        const uint64_t i = base + tid;
        const bool valid = i < hi;
        unsigned long long b = 0;
        if (valid) {
            const uint64_t so = a.src_offsets[i];
            const uint32_t len = a.lengths[i];
            b = size(i, so, len);
            // at most this many 16-byte pieces of destination, wherever it lies
            pieces += len ? (((uint64_t)len + 15u) >> 4) + 1u : 0u;
        }
        unsigned long long tot;
        const unsigned long long before = tile_scan(b, wtot, &tot);
        if (valid) {
            a.off[i] = carry + before;
        }
        carry += tot;
    }
    pieces = wave_sum(pieces);
    if (lane == 0) {
        wpieces[wv] = pieces;
    }
    __syncthreads();
    if (tid == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < kPackThreads / 64; ++w) {
            t += wpieces[w];
        }
        a.bsum[blockIdx.x] = carry;
        a.bsum[kPackBlocks + blockIdx.x] = t;
    }
}

static_assert(kPackBlocks == 256 && kPackThreads >= (int)kPackBlocks, "block_prefix: 4 waves");

// bpre[b] = framed bytes of the blocks before b, bpre[nblocks] = of all; the
// return value is the pieces of all blocks.  One load per thread (a serial
// walk of 256 dependent loads by one thread took 30 us), scanned by
// shuffles in the block's first four waves.  Called by the whole block.
template <class Args>
__device__ __forceinline__ unsigned long long block_prefix(const Args& a, unsigned long long* bpre)
{
    __shared__ unsigned long long wsum[2][kPackBlocks / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    unsigned long long incl = 0, v = 0, pieces = 0;
    if (tid < kPackBlocks) {
        v = tid < a.nblocks ? a.bsum[tid] : 0ull;
        pieces = tid < a.nblocks ? a.bsum[kPackBlocks + tid] : 0ull;
        incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long o = __shfl_up(incl, d);
            incl += lane >= (uint32_t)d ? o : 0ull;
        }
        pieces = wave_sum(pieces);
        if (lane == 63) {
            wsum[0][wv] = incl;
        }
        if (lane == 0) {
            wsum[1][wv] = pieces;
        }
    }
    __syncthreads();
    if (tid < kPackBlocks) {
        unsigned long long before = 0;
        for (uint32_t w = 0; w < wv; ++w) {
            before += wsum[0][w];
        }
        if (tid < a.nblocks) {
            bpre[tid] = before + incl - v;
        }
        if (tid + 1 == a.nblocks) {
            bpre[a.nblocks] = before + incl;
        }
    }
    __syncthreads();
    return wsum[1][0] + wsum[1][1] + wsum[1][2] + wsum[1][3];
}

// ---- the event split of the event packers (PUT, STORAGE, PUSH) --------------
//
// Event e holds the messages [event_first[e], event_first[e + 1]) -- one event
// of all n when event_first is null -- behind an 8-byte EventHeader.  With P
// the 64-bit exclusive prefix of B, message i's frame starts at
// 8 (e(i) + 1) + P[i].  Beyond layout_count's fields these use event_first,
// n_events, max_event_bytes, dst, dst_bytes and event_offsets.

constexpr uint32_t kEventHeaderBytes = 8;

// The block's LDS words for block_prefix's result: one array, whichever of the
// functions below and of the unit's own code asks for it.
__device__ __forceinline__ unsigned long long* shared_bpre()
{
    __shared__ unsigned long long bpre[kPackBlocks + 1];
    return bpre;
}

// event_first's shape: starts at 0, strictly increasing, ends at n.  Called by
// every thread of a kPackThreads grid.
template <class Args>
__device__ __forceinline__ void event_first_shape(const Args& a, uint32_t kind)
{
    if (a.event_first) {
        const uint64_t stride = (uint64_t)gridDim.x * kPackThreads;
        for (uint64_t e = (uint64_t)blockIdx.x * kPackThreads + threadIdx.x; e <= a.n_events;
             e += stride) {
            const uint64_t f = a.event_first[e];
            const bool bad = e == a.n_events ? f != a.n
                                             : (e == 0 && f != 0) || f >= a.event_first[e + 1];
            if (bad) {
                refuse(a, kind, e);
            }
        }
    }
}

// The events, one per thread: every event's size against the cap and (unless
// dst is null and null_dst_is_size_only) its end against dst_bytes; the pieces
// against the copy's limit; the bytes of all events to ctr[total_word].  Called
// by every thread of a kPackThreads grid, and only when every event_first
// entry is known to be a valid index (the shape and the messages were clean).
template <class Args>
__device__ __forceinline__ void events_check(const Args& a, uint32_t kind_event_too_big,
                                             uint32_t kind_dst_too_small,
                                             uint32_t kind_too_many_pieces, int total_word,
                                             bool null_dst_is_size_only = false)
{
    unsigned long long* bpre = shared_bpre();
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
            refuse(a, kind_event_too_big, e);
        }
        if (!(null_dst_is_size_only && !a.dst) &&
            kEventHeaderBytes * (e + 1) + p1 > a.dst_bytes) {
            refuse(a, kind_dst_too_small, e);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (pieces > 0xFFFFFFFFull) {
            refuse(a, kind_too_many_pieces, 0);
        }
        a.ctr[total_word] = kEventHeaderBytes * a.n_events + all;
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

constexpr uint32_t kSealEvents = 1024;  // seal_offsets: events of a block it searches in LDS

// off[i] becomes where message i's application data goes,
// 8 (e(i) + 1) + P[i] + lead(i), lead(i) the bytes between the message's frame
// start and its application data -- or, when anything was refused, an offset
// past any dst_bytes for EVERY message: the copy kernels then refuse every
// message, own no piece and write neither dst nor their CRCs.  Called by every
// thread of the nblocks x kPackThreads layout grid, when the refusal word is
// final.
template <class Args, class Lead>
__device__ __forceinline__ void seal_offsets(const Args& a, Lead lead)
{
    unsigned long long* bpre = shared_bpre();
    __shared__ uint64_t erange[2];
    __shared__ uint64_t efirst[kSealEvents];
    const uint32_t tid = threadIdx.x;
    const uint64_t lo = (uint64_t)blockIdx.x * a.per_block;
    const uint64_t hi = min(lo + a.per_block, a.n);
    if (a.ctr[kLayoutCtrRefusal] != 0) {
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
    // the block's events' first messages, when they fit: a message's search is
    // then a handful of LDS reads, not of dependent trips to L2
    const bool staged = e0 != e1 && e1 - e0 < kSealEvents;
    if (staged) {
        for (uint64_t k = tid; k <= e1 - e0; k += kPackThreads) {
            efirst[k] = a.event_first[e0 + k];
        }
    }
    __syncthreads();
    for (uint64_t i = lo + tid; i < hi; i += kPackThreads) {
        const uint64_t e = e0 == e1   ? e0
                           : staged ? e0 + event_of(efirst, 0, e1 - e0, i)
                                    : event_of(a.event_first, e0, e1, i);
        a.off[i] = a.off[i] + before + kEventHeaderBytes * (e + 1) + lead(i);
    }
}

// The EventHeaders and event_offsets, after the copy: event e starts
// 8 + lead(f) bytes before the application data of its first message f, and
// `total` bytes end the last one.  type_byte: PV 1 | the event's type.  Called
// by every thread of a kPackFrameThreads grid.
template <class Args, class Lead>
__device__ __forceinline__ void event_headers(const Args& a, Lead lead, uint32_t type_byte,
                                              uint64_t total)
{
    const uint64_t stride = (uint64_t)gridDim.x * kPackFrameThreads;
    for (uint64_t e = (uint64_t)blockIdx.x * kPackFrameThreads + threadIdx.x; e <= a.n_events;
         e += stride) {
        uint64_t at = total, next = total;
        if (e < a.n_events) {
            const uint64_t f = a.event_first ? a.event_first[e] : 0;
            at = a.off[f] - (kEventHeaderBytes + lead(f));
            if (e + 1 < a.n_events) {
                const uint64_t g = a.event_first[e + 1];
                next = a.off[g] - (kEventHeaderBytes + lead(g));
            }
            uint32_t* h = (uint32_t*)(a.dst + at);
            h[0] = __builtin_bswap32((uint32_t)(next - at) & 0x7FFFFFFFu);
            h[1] = 0x00000200u | type_byte;  // bytes: PV 1 | type, HeaderWords 2, 0, 0
        }
        if (a.event_offsets) {
            a.event_offsets[e] = at;
        }
    }
}

}  // namespace
}  // namespace bmqcrc
