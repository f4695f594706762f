// crc32c_copy.hip -- MI355X (gfx950) fused copy + CRC32C (bmqcrc_crc32c_copy).
//
// For every message: copy lengths[i] bytes from src + src_offsets[i] to
// dst + dst_offsets[i] and CRC the same bytes, each payload byte read once
// and written once.
//
//   * A message is cut into 16-byte PIECES on the 16-byte boundaries of its
//     DESTINATION address.  Interior pieces are whole aligned dwordx4 stores
//     fed by one (generally unaligned) dwordx4 load; only a message's first
//     and last piece are narrower, and those are moved byte by byte -- no
//     byte of dst outside a message is read or written, so two messages that
//     share a 16-byte piece never race.
//   * The pieces of all messages, in message order, form one piece space.
//     k_copy_count / k_copy_scan check every message's bounds, build the
//     exclusive prefix of piece counts (first[]) and write each message's
//     seed contribution into out[i].  A refused message has no pieces.
//   * k_copy_fold is a persistent grid.  A wave takes CHUNKS of 4,096
//     consecutive pieces (64 KiB) of the piece space, grid-strided, and walks
//     a chunk in ROWS of 64 pieces: lane l of row r owns piece 64 r + l, so
//     one load or store instruction covers 1 KiB of consecutive payload of a
//     long message, and small messages share a row (lanes are dealt to
//     messages by the prefix of piece counts).
//   * Arithmetic: a lane keeps four accumulators, one per word of its piece,
//     and steps them from row to row with one multiply by x^(8 * 1024) per
//     word (Horner; four byte-sliced lookups in LDS) while its message stays
//     the same.  When the message changes, or the chunk ends, the lane's
//     value is moved to its message's end by x^(8 * bytes after) (byte-indexed
//     factors, as k_fold's mul_xbytes), XOR-reduced over the run of lanes
//     that hold the same message (segmented shuffle reduce) and XORed into
//     out[i] with one atomic per run.  XOR is order independent: results are
//     deterministic.
//
// The GF(2) helpers are copies of crc32c_kernels.hip's (the build has no
// relocatable device code, and that unit's kernels stay instruction for
// instruction what they were).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmqcrc_internal.h"
#include "crc32c_consts.h"

namespace bmqcrc {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// byte-aligned vector: one global_load_dwordx4 at any address (gfx950 runs
// global accesses in unaligned mode under HSA)
typedef uint32_t u32x4u __attribute__((ext_vector_type(4), aligned(1)));

static_assert(BMQCRC_COPY_ROW_BYTES == 16 * kWaveLanes, "XROW is the step of one 64-piece row");

__constant__ uint32_t cc_xrow[4][256] = BMQCRC_XROW;
__constant__ uint32_t cc_ty[8][256] = BMQCRC_TY;  // rows 0-3: times y = x^32
__constant__ uint32_t cc_xbytes[4][256] = BMQCRC_XBYTES;
__constant__ uint32_t cc_xneg8[136] = BMQCRC_XNEG8;

constexpr uint32_t kNone = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t xand(uint32_t acc, uint32_t mask, uint32_t col)
{
    return __builtin_amdgcn_bitop3_b32(acc, mask, col, 0x78);  // acc ^ (mask & col)
}

__device__ __forceinline__ uint32_t bitmask(uint32_t v, int t)
{
    return (uint32_t)__builtin_amdgcn_sbfe((int)v, t, 1);  // 0 or ~0
}

// v * w mod P (reflected), both variable: 32 shift-and-add steps, 160 VALU.
__device__ __forceinline__ uint32_t gmul(uint32_t v, uint32_t w)
{
    uint32_t acc = 0;
#pragma unroll
    for (int t = 31; t >= 0; --t) {  // bit t of v <-> x^(31-t); w tracks w * x^(31-t)
        acc = xand(acc, bitmask(v, t), w);
        w = xand(w >> 1, bitmask(w, 0), 0x82F63B78u);
    }
    return acc;
}

// Inclusive max-scan over the wave's 64 lanes by DPP (all lanes active).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_max(uint32_t v)
{
    return max(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROW_MASK, 0xf,
                                                        false));
}

__device__ __forceinline__ uint32_t wave_incl_max(uint32_t v)
{
    v = dpp_max<0x111, 0xf>(v);  // row_shr:1
    v = dpp_max<0x112, 0xf>(v);  // row_shr:2
    v = dpp_max<0x114, 0xf>(v);  // row_shr:4
    v = dpp_max<0x118, 0xf>(v);  // row_shr:8
    v = dpp_max<0x142, 0xa>(v);  // row_bcast:15 -> rows 1, 3
    v = dpp_max<0x143, 0xc>(v);  // row_bcast:31 -> rows 2, 3
    return v;
}

// LDS written by one lane of a wave and read by another, with no block barrier
// (the waves of a block walk different chunks).
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Byte-sliced multiply by a constant: tab[k][b] = (b << 8k) * c.
__device__ __forceinline__ uint32_t mul_tab(const uint32_t (*tab)[256], uint32_t v)
{
    return tab[0][v & 0xffu] ^ tab[1][(v >> 8) & 0xffu] ^ tab[2][(v >> 16) & 0xffu] ^ tab[3][v >> 24];
}

// x^(8 dist) as the product of the factors of dist's bytes (k_fold's
// mul_xbytes): a byte position no lane needs is skipped wave-uniformly.
__device__ __forceinline__ uint32_t xbytes_factor(const uint32_t (*xb)[256], uint32_t f,
                                                  uint32_t dist)
{
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        const uint32_t b = (dist >> (8 * i)) & 0xffu;
        if (__ballot(b != 0) != 0) {
            f = gmul(f, xb[i][b]);  // xb[i][0] = 1
        }
    }
    return f;
}

// Bounds check and piece count of message i: 0 pieces for an empty or a
// refused message.  The sums are taken in 64 bits without overflow.
__device__ __forceinline__ uint32_t msg_pieces(const CopyArgs& a, uint64_t i, bool* refused)
{
    const uint64_t so = a.src_offsets[i], dof = a.dst_offsets[i];
    const uint32_t len = a.lengths[i];
    const bool ok = so <= a.src_bytes && len <= a.src_bytes - so && dof <= a.dst_bytes &&
                    len <= a.dst_bytes - dof;
    *refused = !ok;
    if (!ok || len == 0) {
        return 0;
    }
    const uint32_t al = (uint32_t)((uintptr_t)a.dst + dof) & 15u;
    return (uint32_t)(((uint64_t)al + len + 15u) >> 4);
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        v += __shfl_down(v, d);
    }
    return v;  // lane 0
}

// Pass 1: per-block piece totals, and the refused messages.
__global__ __launch_bounds__(kCopyPlanThreads) void k_copy_count(CopyArgs a)
{
    __shared__ unsigned long long wsum[kCopyPlanThreads / 64];
    const uint64_t lo = (uint64_t)blockIdx.x * a.per_block;
    const uint64_t hi = min(lo + a.per_block, a.n);
    unsigned long long sum = 0;
    for (uint64_t i = lo + threadIdx.x; i < hi; i += kCopyPlanThreads) {
        bool refused;
        sum += msg_pieces(a, i, &refused);
        if (refused) {
            atomicAdd(&a.ctr[kCopyCtrRefused], 1ull);
            atomicMax(&a.ctr[kCopyCtrLowestInv], ~(unsigned long long)i);
        }
    }
    sum = wave_sum_u64(sum);
    if ((threadIdx.x & 63u) == 0) {
        wsum[threadIdx.x >> 6] = sum;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < kCopyPlanThreads / 64; ++w) {
            t += wsum[w];
        }
        a.bsum[blockIdx.x] = t;
    }
}

// Pass 2: first[i] = exclusive prefix of piece counts (first[n] = the total),
// out[i] = the seed's share of message i's CRC: ~(~seed * x^(8 len)); the
// fold XORs the payload's share in.  More than 2^32 - 1 pieces in one call:
// the flag is raised, the total is 0 and nothing is copied.
__global__ __launch_bounds__(kCopyPlanThreads) void k_copy_scan(CopyArgs a)
{
    __shared__ uint32_t xb[4][256];
    __shared__ unsigned long long red[2][kCopyPlanThreads / 64];
    __shared__ uint32_t wtot[kCopyPlanThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    unsigned long long before = 0, all = 0;
    for (uint32_t j = tid; j < a.nblocks; j += kCopyPlanThreads) {
        const unsigned long long v = a.bsum[j];
        all += v;
        before += j < blockIdx.x ? v : 0ull;
    }
    before = wave_sum_u64(before);
    all = wave_sum_u64(all);
    if (lane == 0) {
        red[0][wv] = before;
        red[1][wv] = all;
    }
    for (uint32_t i = tid; i < 1024; i += kCopyPlanThreads) {
        (&xb[0][0])[i] = (&cc_xbytes[0][0])[i];
    }
    __syncthreads();
    before = 0;
    all = 0;
    for (int w = 0; w < kCopyPlanThreads / 64; ++w) {
        before += red[0][w];
        all += red[1][w];
    }
    if (all > 0xFFFFFFFFull) {
        if (blockIdx.x == 0 && tid == 0) {
            a.ctr[kCopyCtrOverflow] = 1;
            a.first[a.n] = 0;
        }
        return;
    }
    if (blockIdx.x == 0 && tid == 0) {
        a.first[a.n] = (uint32_t)all;
    }
    const uint64_t lo = (uint64_t)blockIdx.x * a.per_block;
    const uint64_t hi = min(lo + a.per_block, a.n);
    uint32_t carry = (uint32_t)before;
    for (uint64_t base = lo; base < hi; base += kCopyPlanThreads) {
        const uint64_t i = base + tid;
        const bool valid = i < hi;
        bool refused = true;
        const uint32_t np = valid ? msg_pieces(a, i, &refused) : 0u;
        uint32_t incl = np;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d);
            incl += lane >= (uint32_t)d ? o : 0u;
        }
        if (lane == 63) {
            wtot[wv] = incl;
        }
        __syncthreads();
        uint32_t woff = 0, tot = 0;
        for (uint32_t w = 0; w < kCopyPlanThreads / 64; ++w) {
            woff += w < wv ? wtot[w] : 0u;
            tot += wtot[w];
        }
        __syncthreads();
        const uint32_t len = (valid && !refused) ? a.lengths[i] : 0u;
        const uint32_t seed = (valid && !refused && a.seeds) ? a.seeds[i] : 0u;
        const uint32_t f = xbytes_factor(xb, xb[0][len & 0xffu], len);
        const uint32_t share = ~gmul(~seed, f);
        if (valid) {
            a.first[i] = carry + woff + incl - np;
            if (!refused) {
                a.out[i] = share;
            }
        }
        carry += tot;
    }
}

struct CopyLds {
    uint32_t xrow[4][256];
    uint32_t ty[4][256];
    uint32_t xb[4][256];
    uint32_t xneg[16];
    uint32_t mark[kCopyWaves][64];
};

// Last i with first[i] <= g, for g below the total (first[n]): that message is
// not empty and owns piece g.  64 probes per step, one per lane.
__device__ __forceinline__ uint32_t copy_find(const uint32_t* first, uint64_t n, uint32_t g,
                                              uint32_t lane)
{
    uint64_t lo = 0, hi = n;  // first[lo] <= g < first[hi]
    while (hi - lo > 1) {
        const uint64_t step = (hi - lo + 63) >> 6;
        const uint64_t idx = lo + (uint64_t)(lane + 1) * step;
        const bool le = idx < hi && first[idx] <= g;
        const uint64_t nlo = lo + (uint64_t)__popcll(__ballot(le)) * step;
        hi = min(hi, nlo + step);
        lo = nlo;
    }
    return (uint32_t)lo;
}

// Per-lane Horner state: the message held (kNone: nothing), the four word
// accumulators of its pieces so far, and message end - end of the last piece.
struct Lane {
    uint32_t held, a0, a1, a2, a3;
    int64_t after;
};

// Lanes with `pred` give their value up: move it to the message end,
// XOR-reduce over each run of adjacent lanes holding the same message, one
// atomic per run.  Wave-uniform call (every lane takes part in the shuffles).
__device__ __forceinline__ void flush(const CopyArgs& a, const CopyLds& L, Lane& s, bool pred,
                                      uint32_t lane)
{
    uint32_t v = s.a0;
    v = mul_tab(L.ty, v) ^ s.a1;
    v = mul_tab(L.ty, v) ^ s.a2;
    v = mul_tab(L.ty, v) ^ s.a3;
    v = mul_tab(L.ty, v);  // the CRC's own x^32
    v = pred ? v : 0u;
    // after is in [-15, 2^32): a last piece cut by the message end carries
    // zero bytes after it, taken back by x^(-8 k)
    const bool neg = pred && s.after < 0;
    const uint32_t dist = (pred && !neg) ? (uint32_t)s.after : 0u;
    uint32_t f = neg ? L.xneg[(uint32_t)(-s.after) & 15u] : L.xb[0][dist & 0xffu];
    f = xbytes_factor(L.xb, f, dist);
    v = gmul(v, f);
    // Runs are segments of ADJACENT lanes with one key, not all lanes with
    // that key: at the end of a chunk whose last row is partial, the lanes
    // past it still hold the row before, so one message can be held by two
    // separate runs (the start of the last row and the top of the wave).
    // Every lane gets the lane index of its run's head (inclusive max-scan
    // of the head lanes' indices), and the doubling steps compare that.
    const uint32_t key = pred ? s.held : kNone;
    const uint32_t pk = __shfl_up(key, 1);
    const bool head = lane == 0 || pk != key;
    const uint32_t run = wave_incl_max(head ? lane : 0u);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t orun = __shfl_down(run, d);
        const uint32_t ov = __shfl_down(v, d);
        v ^= (lane + d < 64u && orun == run) ? ov : 0u;
    }
    if (pred && head) {
        atomicXor(&a.out[key], v);
    }
    if (pred) {
        s.held = kNone;
        s.a0 = s.a1 = s.a2 = s.a3 = 0;
    }
}

__device__ __forceinline__ void horner(const CopyLds& L, Lane& s, u32x4 w)
{
    s.a0 = mul_tab(L.xrow, s.a0) ^ w.x;
    s.a1 = mul_tab(L.xrow, s.a1) ^ w.y;
    s.a2 = mul_tab(L.xrow, s.a2) ^ w.z;
    s.a3 = mul_tab(L.xrow, s.a3) ^ w.w;
}

// A message's first or last piece: the bytes of the window that belong to
// the message, one at a time (rel0 = the window's offset from the message's
// first byte, negative in a first piece).  The other bytes of the word stay 0.
__device__ __forceinline__ u32x4 edge_piece(const uint8_t* S, uint8_t* D, int64_t rel0,
                                            uint32_t len, bool on)
{
    u32x4 w = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int64_t o = rel0 + j;
        if (on && o >= 0 && o < (int64_t)len) {
            const uint8_t b = S[o];
            D[o] = b;
            w[j >> 2] |= (uint32_t)b << (8 * (j & 3));
        }
    }
    return w;
}

__global__ __launch_bounds__(kCopyWaves * 64) void k_copy_fold(CopyArgs a)
{
    __shared__ CopyLds L;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    for (uint32_t i = tid; i < 1024; i += kCopyWaves * 64) {
        (&L.xrow[0][0])[i] = (&cc_xrow[0][0])[i];
        (&L.ty[0][0])[i] = (&cc_ty[0][0])[i];
        (&L.xb[0][0])[i] = (&cc_xbytes[0][0])[i];
    }
    if (tid < 16) {
        L.xneg[tid] = cc_xneg8[tid];
    }
    __syncthreads();
    uint32_t* mark = L.mark[wv];
    const uint32_t total = a.first[a.n];
    const uint64_t ntiles = ((uint64_t)total + kCopyChunkPieces - 1) / kCopyChunkPieces;
    const uint64_t nwaves = (uint64_t)gridDim.x * kCopyWaves;
    // neighbouring chunks go to different CUs (a batch of few chunks spreads out)
    for (uint64_t t = blockIdx.x + (uint64_t)gridDim.x * wv; t < ntiles; t += nwaves) {
        const uint32_t g0 = (uint32_t)(t * kCopyChunkPieces);
        const uint32_t g1 = (uint32_t)min((uint64_t)total, (uint64_t)g0 + kCopyChunkPieces);
        // the message of the row's first piece, wave-uniform
        uint32_t cur_m = kNone, cur_first = 0, cur_end = 0, cur_len = 0;
        const uint8_t* cur_s = nullptr;
        uint8_t* cur_d = nullptr;
        uint32_t next_m = copy_find(a.first, a.n, g0, lane);
        Lane s = {kNone, 0, 0, 0, 0, 0};
        uint32_t gr = g0;
        while (gr < g1) {
            if (next_m != cur_m) {
                cur_m = next_m;
                cur_first = a.first[cur_m];
                cur_end = a.first[cur_m + 1];
                cur_len = a.lengths[cur_m];
                cur_s = a.src + a.src_offsets[cur_m];
                cur_d = a.dst + a.dst_offsets[cur_m];
            }
            const uint32_t row_end = g1 - gr > 64u ? gr + 64u : g1;
            const uint32_t g = gr + lane;
            const bool valid = g < g1 && g >= gr;
            uint32_t my_m = cur_m, my_first = cur_first, my_len = cur_len;
            const uint8_t* S = cur_s;
            uint8_t* D = cur_d;
            if (row_end > cur_end) {
                // the row holds more than one message: the first piece of every
                // message that starts in it is marked with the message's index
                // (relative to cur_m), and an inclusive max-scan deals the lanes
                mark[lane] = 0;
                wave_lds_sync();
                for (uint64_t wb = (uint64_t)cur_m + 1;; wb += 64) {
                    const uint64_t idx = wb + lane;
                    uint32_t st = kNone, en = kNone;
                    if (idx < a.n) {
                        st = a.first[idx];
                        en = a.first[idx + 1];
                    }
                    const bool in_row = idx < a.n && (uint32_t)(st - gr) < 64u;
                    if (in_row && en > st) {  // (an empty message owns no piece)
                        mark[st - gr] = (uint32_t)(idx - cur_m);
                    }
                    // the window's last entry still lies in the row: look further
                    if (!(__ballot(in_row) >> 63)) {
                        break;
                    }
                    // a window of empty (or refused) messages only: they share
                    // one start, and the search finds the message that owns
                    // that piece -- a run of millions is one search, not a walk
                    if (__ballot(idx < a.n && en == st) == ~0ull) {
                        const uint32_t at = (uint32_t)__shfl((int)st, 63);
                        wb = (uint64_t)copy_find(a.first, a.n, at, lane) - 64;
                    }
                }
                wave_lds_sync();
                my_m = cur_m + wave_incl_max(mark[lane]);
                my_first = a.first[my_m];
                my_len = a.lengths[my_m];
                S = a.src + a.src_offsets[my_m];
                D = a.dst + a.dst_offsets[my_m];
                next_m = (uint32_t)__shfl((int)my_m, (int)(row_end - gr - 1u));
                next_m = (uint32_t)__builtin_amdgcn_readfirstlane((int)next_m);
            }
            // a lane whose message changes gives its value up first
            const bool change = valid && s.held != kNone && s.held != my_m;
            if (__ballot(change) != 0) {
                flush(a, L, s, change, lane);
            }
            const uint32_t al = (uint32_t)(uintptr_t)D & 15u;
            const int64_t rel0 = 16ll * (int64_t)(g - my_first) - (int64_t)al;
            if (row_end <= cur_end) {
                // rows of whole pieces of one message, four in flight
                const uint64_t full_lo = (uint64_t)cur_first + (al ? 1u : 0u);
                const uint64_t full_hi = min((uint64_t)cur_first + (((uint64_t)al + cur_len) >> 4),
                                             (uint64_t)g1);
                if (gr >= full_lo && (uint64_t)gr + 256u <= full_hi) {
                    int64_t rel = rel0;
                    do {
                        u32x4 w[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            w[r] = *(const u32x4u*)(S + rel + 1024 * r);
                        }
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            *(u32x4*)(D + rel + 1024 * r) = w[r];
                            horner(L, s, w[r]);
                        }
                        rel += 4096;
                        gr += 256u;
                    } while ((uint64_t)gr + 256u <= full_hi);
                    s.held = cur_m;
                    s.after = (int64_t)cur_len - (rel - 1024 + 16);  // the last row done
                    continue;
                }
            }
            const bool full = valid && rel0 >= 0 && rel0 + 16 <= (int64_t)my_len;
            u32x4 w = {0, 0, 0, 0};
            if (full) {
                w = *(const u32x4u*)(S + rel0);
                *(u32x4*)(D + rel0) = w;
            }
            const bool edge = valid && !full;
            if (__ballot(edge) != 0) {
                const u32x4 e = edge_piece(S, D, rel0, my_len, edge);
                w = edge ? e : w;
            }
            if (valid) {
                horner(L, s, w);
                s.held = my_m;
                s.after = (int64_t)my_len - (rel0 + 16);
            }
            gr = row_end;
        }
        flush(a, L, s, s.held != kNone, lane);
    }
}

}  // namespace
}  // namespace bmqcrc

using namespace bmqcrc;

extern "C" int bmqcrc_copy_occupancy(int* blocks_per_cu)
{
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, k_copy_fold,
                                                        kCopyWaves * 64, 0) != hipSuccess;
}

extern "C" int bmqcrc_launch_copy(const CopyArgs* a, void* stream, uint32_t fold_blocks)
{
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_copy_count, dim3(a->nblocks), dim3(kCopyPlanThreads), 0, s, *a);
    hipLaunchKernelGGL(k_copy_scan, dim3(a->nblocks), dim3(kCopyPlanThreads), 0, s, *a);
    hipLaunchKernelGGL(k_copy_fold, dim3(fold_blocks), dim3(kCopyWaves * 64), 0, s, *a);
    return hipGetLastError() != hipSuccess;
}
