// crc32c_pack_layout.h -- the layout passes the device packers share
// (crc32c_put_pack.hip, crc32c_records_pack.hip; DESIGN.md sections 12, 13).
// Device only, in the anonymous namespace like the units' own code.  Templates
// over the unit's args struct (PackArgs, RecArgs), of which they use src_bytes,
// src_offsets, lengths, n, off, bsum, ctr, per_block and nblocks.  The
// unpackers take refuse, wave_sum, block_prefix and tile_scan from here too.
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

}  // namespace
}  // namespace bmqcrc
