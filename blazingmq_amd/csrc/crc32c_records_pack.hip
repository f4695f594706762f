// crc32c_records_pack.hip -- MI355X (gfx950) DATA-file and journal framing
// around the fused copy + CRC (bmqcrc_message_records_pack, ABI 2.11;
// DESIGN.md section 13).
//
// The device-side storage writer that FileStore::writeMessageRecord is on the
// host: per message a DATA record (12-byte DataHeader, the application data,
// 1..8 padding bytes each equal to their count) and a 60-byte journal
// MessageRecord pointing at it.  No options, no compression, no schema id.
//
// With R[i] = 12 + lengths[i] + pad and Q its 64-bit exclusive prefix, DATA
// record i lies at dst + Q[i] and journal record i at journal + 60 i.  Three
// steps on one stream:
//
//   1. Layout.  k_rec_count: pass 1 of crc32c_pack_layout.h over R, with every
//      record's size and source range checked.  k_rec_place: every
//      block scans the block sums; the block in whose range the records first
//      end past dst_bytes, or past the last byte MessageOffsetDwords can
//      address, finds that message by bisection and raises the refusal; off[i]
//      becomes the payload's destination offset Q[i] + 12 -- or, when anything
//      was refused, an offset past dst_bytes for EVERY message: the copy
//      kernels then refuse every message, own no piece and write neither dst
//      nor out.  (Whether the totals fit is the same answer in every block, so
//      the checks of section 12's k_pack_check need no launch of their own.)
//   2. Payload.  bmqcrc_launch_copy (crc32c_copy.hip), as it is.
//   3. Frame.  k_rec_frame, after the fold, when out[i] is final: the 15
//      dwords of every journal record, indexed across the grid so that
//      adjacent lanes store adjacent dwords; then the 3 DataHeader dwords of
//      every DATA record and its padding, as stores that cover padding bytes
//      only (no read-modify-write of a word that holds payload).  It leaves at
//      once on a refusal.
//
// The refusal word, pass 1's scan and the prefix of the block sums are shared
// with crc32c_put_pack.hip and described in crc32c_pack_layout.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmqcrc_internal.h"
#include "crc32c_pack_layout.h"

namespace bmqcrc {
namespace {

// byte-aligned dword: a GUID array need not be 4-byte aligned
typedef uint32_t u32u __attribute__((aligned(1)));

constexpr uint32_t kDataHeaderBytes = 12, kJournalDwords = 15;

// DataHeader + application data + padding (calcNumDwordsAndPadding: 1..8 bytes)
__device__ __forceinline__ uint64_t record_bytes(uint32_t len)
{
    return ((((uint64_t)len + kDataHeaderBytes) >> 3) + 1) << 3;
}

// Pass 1: the shared scan.
__global__ __launch_bounds__(kPackThreads) void k_rec_count(RecArgs a)
{
    layout_count(a, [&a](uint64_t i, uint64_t so, uint32_t len) {
        unsigned long long b = record_bytes(len);
        if ((b >> 2) > 0x1FFFFFFFull) {
            // 29 bits of DataHeader::messageWords; the record counts for
            // nothing, so that no sum of the scan can pass 2^64
            refuse(a, BMQCRC_REC_KIND_RECORD_TOO_BIG, i);
            b = 0;
        }
        if (!(so <= a.src_bytes && len <= a.src_bytes - so)) {
            refuse(a, BMQCRC_REC_KIND_SRC_RANGE, i);
        }
        return b;
    });
}

// Pass 2: the checks on the totals, then off[i] = where message i's
// application data goes.
__global__ __launch_bounds__(kPackThreads) void k_rec_place(RecArgs a)
{
    __shared__ unsigned long long bpre[kPackBlocks + 1];
    const uint32_t tid = threadIdx.x;
    const uint64_t lo = (uint64_t)blockIdx.x * a.per_block;
    const uint64_t hi = min(lo + a.per_block, a.n);
    // Pass 1's word.  A block that starts late may read what another block of
    // this pass has raised below instead: it then holds of the totals too.
    const bool counted_clean = a.ctr[kRecCtrRefusal] == 0;
    const unsigned long long pieces = block_prefix(a, bpre);
    const unsigned long long all = bpre[a.nblocks];
    const unsigned long long before = bpre[blockIdx.x], after = bpre[blockIdx.x + 1];
    // bytes the DATA file still takes before MessageOffsetDwords overflows
    const unsigned long long room =
        a.data_file_pos <= kRecMaxFileBytes ? kRecMaxFileBytes - a.data_file_pos : 0ull;
    // the same answer in every block: all of it comes from the block sums
    const bool refused = !counted_clean || all > a.dst_bytes || all > room || pieces > 0xFFFFFFFFull;
    if (tid == 0) {
        // Record i ends at Q[i + 1].  The first one to end past a bound lies
        // in the block with before <= bound < after, and is the last message
        // there that still starts at or before the bound.  (Searched whatever
        // pass 1 found: the lowest kind wins in the word itself.)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const unsigned long long bound = k ? room : a.dst_bytes;
            if (before <= bound && bound < after) {
                uint64_t l = lo, h = hi - 1;  // off[lo] = 0: starts at `before`
                while (l < h) {
                    const uint64_t mid = l + (h - l + 1) / 2;
                    if (before + a.off[mid] <= bound) {
                        l = mid;
                    } else {
                        h = mid - 1;
                    }
                }
                refuse(a, k ? BMQCRC_REC_KIND_DATA_FILE_FULL : BMQCRC_REC_KIND_DST_TOO_SMALL, l);
            }
        }
        if (blockIdx.x == 0) {
            if (pieces > 0xFFFFFFFFull) {
                refuse(a, BMQCRC_REC_KIND_TOO_MANY_PIECES, 0);
            }
            a.ctr[kRecCtrTotal] = all;
        }
    }
    __syncthreads();  // the search above reads off[] as pass 1 left it
    if (refused) {
        // past any dst_bytes: the copy kernels refuse the message
        for (uint64_t i = lo + tid; i < hi; i += kPackThreads) {
            a.off[i] = ~0ull;
        }
        return;
    }
    for (uint64_t i = lo + tid; i < hi; i += kPackThreads) {
        const unsigned long long q = a.off[i] + before;
        a.off[i] = q + kDataHeaderBytes;
        if (a.record_offsets) {
            a.record_offsets[i] = q;
        }
    }
    if (tid == 0 && hi == a.n && a.record_offsets) {
        a.record_offsets[a.n] = all;
    }
}

// Step 3.  Thread t of the grid owns dword t % 15 of journal record t / 15,
// then DataHeader dword t % 3 of DATA record t / 3.
__global__ __launch_bounds__(kPackFrameThreads) void k_rec_frame(RecArgs a)
{
    if (a.ctr[kRecCtrRefusal] != 0) {
        return;
    }
    const uint64_t stride = (uint64_t)gridDim.x * kPackFrameThreads;
    const uint64_t t0 = (uint64_t)blockIdx.x * kPackFrameThreads + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t ndw = kJournalDwords * a.n;
    // (n < 2^32: a dword's index needs 36 bits, its message's 32); the
    // divisions in 32 bits whenever the call's indices fit
    const bool narrow = ndw <= 0xFFFFFFFFull;
    for (uint64_t t = t0; t < ndw; t += stride) {
        const uint64_t m = narrow ? (uint32_t)t / kJournalDwords : t / kJournalDwords;
        const uint32_t j = (uint32_t)(t - kJournalDwords * m);
        // What the lane reads, at most two dwords, is fetched before any of it
        // is used: one memory latency per step.  (Each field loading inside
        // its own branch made a wave wait for up to nine loads one after the
        // other; with byte-wise padding stores on top that version took 433
        // against 349 us on 4M x 64 B and 115 against 92 on 1M x 256 B,
        // profiles/r10/records_pack/first_run.)
        const u32u* pa = nullptr;
        const u32u* pb = nullptr;
        if (j == 0 || j == 5) {
            pa = a.ref_counts ? (const u32u*)a.ref_counts + m : nullptr;
            // queue key bytes 0..3 (0 and 1 are used): 5 m + 3 < 5 n
            pb = j == 5 ? (const u32u*)(a.queue_keys + 5 * m) : nullptr;
        } else if (j == 3 || j == 4) {
            // the half of timestamps[m] this dword holds: the high one first
            pa = a.timestamps ? (const u32u*)a.timestamps + 2 * m + (j == 3) : nullptr;
        } else if (j == 6) {
            pa = (const u32u*)(a.queue_keys + 5 * m + 1);  // queue key bytes 1..4
        } else if (j == 8) {
            pa = (const u32u*)(a.off + m);
            pb = pa + 1;
        } else if (j >= 9 && j < 13) {
            pa = (const u32u*)a.guids + 4 * m + (j - 9);
        } else if (j == 13) {
            pa = (const u32u*)a.out + m;
            pb = a.expected ? (const u32u*)a.expected + m : nullptr;
        }
        const uint32_t xa = pa ? *pa : 0u;
        const uint32_t xb = pb ? *pb : 0u;
        const uint64_t seq = a.first_seq + m;
        const uint32_t rc = a.ref_counts ? xa : 1u;  // (dwords 0 and 5)
        uint32_t v;
        bool bad = false;
        if (j == 0) {
            // RecordHeader: type MESSAGE (1) | flags = refcount's low 12 bits,
            // then the 48-bit sequence number
            v = __builtin_bswap32(((0x1000u | (rc & 0xFFFu)) << 16) | (uint32_t)(seq >> 32));
        } else if (j == 1) {
            v = __builtin_bswap32((uint32_t)seq);
        } else if (j == 2) {
            v = __builtin_bswap32(a.lease_id);
        } else if (j < 5) {
            const uint32_t half = j == 3 ? (uint32_t)(a.timestamp >> 32) : (uint32_t)a.timestamp;
            v = __builtin_bswap32(a.timestamps ? xa : half);
        } else if (j == 5) {
            // refcount's high 8 bits, CAT 0, queue key bytes 0 and 1
            v = ((rc >> 12) & 0xFFu) | (xb << 16);
        } else if (j == 6) {
            v = (xa >> 8) | a.key_lo;  // queue key bytes 2..4, file key byte 0
        } else if (j == 7) {
            v = a.key_hi;
        } else if (j == 8) {
            // MessageOffsetDwords: the record's place in the file, in 8-byte units
            const uint64_t app = ((uint64_t)xb << 32) | xa;
            v = __builtin_bswap32((uint32_t)((a.data_file_pos + (app - kDataHeaderBytes)) >> 3));
        } else if (j < 13) {
            v = xa;
        } else if (j == 13) {
            const uint32_t want = a.expected ? xb : xa;
            bad = want != xa;
            v = __builtin_bswap32(want);  // what arrived with the message, as the broker stores
        } else {
            v = 0x6345722Au;  // bytes 2A 72 45 63: RecordHeader magic
        }
        ((uint32_t*)a.journal)[t] = v;
        // the lanes here ascend in t, so the lowest set lane holds the wave's lowest message
        const unsigned long long mask = __ballot(bad);
        if (mask != 0 && lane == (uint32_t)__ffsll(mask) - 1u) {
            atomicAdd(&a.ctr[kRecCtrBad], (unsigned long long)__popcll(mask));
            atomicMax(&a.ctr[kRecCtrFirstBad], ~(unsigned long long)m);
        }
    }
    const uint64_t nhd = 3 * a.n;
    for (uint64_t t = t0; t < nhd; t += stride) {
        const uint64_t m = narrow ? (uint32_t)t / 3u : t / 3;
        const uint32_t j = (uint32_t)(t - 3 * m);
        const uint64_t app = a.off[m];
        const uint32_t len = a.lengths[m];
        const uint32_t flags = j == 1 && a.data_flags ? a.data_flags[m] : 0u;
        const uint32_t bytes = (uint32_t)record_bytes(len);  // at most 2^31 - 8
        uint8_t* rec = a.dst + (app - kDataHeaderBytes);
        uint32_t v = flags << 24;  // dword 1: OptionsWords 0 | flags; dword 2: SchemaId 0, Reserved 0
        if (j == 0) {
            v = __builtin_bswap32((3u << 29) | (bytes >> 2));  // HeaderWords 3 | MessageWords
        } else if (j == 2) {
            // This lane writes the padding: the record's last 1..8 bytes, and
            // the record ends on an 8-byte boundary, so they are two aligned
            // dword stores or at most one store each of 4, 2 and 1 bytes, also
            // aligned -- none touches a payload byte.
            const uint32_t pad = bytes - kDataHeaderBytes - len;
            const uint32_t fill = pad * 0x01010101u;
            uint8_t* e = rec + bytes;
            if (pad == 8) {
                e -= 4;
                *(uint32_t*)e = fill;
            }
            if (pad & 12u) {
                e -= 4;
                *(uint32_t*)e = fill;
            }
            if (pad & 2u) {
                e -= 2;
                *(uint16_t*)e = (uint16_t)fill;
            }
            if (pad & 1u) {
                e[-1] = (uint8_t)fill;
            }
        }
        ((uint32_t*)rec)[j] = v;
    }
}

}  // namespace
}  // namespace bmqcrc

using namespace bmqcrc;

extern "C" int bmqcrc_launch_records_layout(const RecArgs* a, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_rec_count, dim3(a->nblocks), dim3(kPackThreads), 0, s, *a);
    hipLaunchKernelGGL(k_rec_place, dim3(a->nblocks), dim3(kPackThreads), 0, s, *a);
    return hipGetLastError() != hipSuccess;
}

extern "C" int bmqcrc_launch_records_frame(const RecArgs* a, void* stream)
{
    const uint64_t want = (kJournalDwords * a->n + kPackFrameThreads - 1) / kPackFrameThreads;
    const uint32_t blocks = (uint32_t)(want > kPackFrameBlocks ? kPackFrameBlocks : want);
    hipLaunchKernelGGL(k_rec_frame, dim3(blocks), dim3(kPackFrameThreads), 0, (hipStream_t)stream,
                       *a);
    return hipGetLastError() != hipSuccess;
}
