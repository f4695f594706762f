// crc32c_rollover.hip -- MI355X (gfx950) compaction of a device-resident
// partition: the outstanding records of a journal run and their DATA records
// rolled over into a new run and a new DATA window (bmqcrc_partition_rollover,
// ABI 2.18).
//
// The device-side form of FileStore::rolloverImpl's loop over
// writeRolledOverRecord: every kept record's 60 bytes to the next free place of
// the new journal, a MESSAGE record's whole DATA record (DataHeader, options,
// application data, 1..8 padding bytes) to the next free place of the new DATA
// file and its MessageOffsetDwords patched, a QUEUE_OP CREATION / ADDITION
// record's QLIST offset zeroed, one sync point behind the last record.  Which
// record is kept is the caller's keep[], except that in FOLLOW mode a CONFIRM
// record is kept exactly when a kept MESSAGE record has its GUID and queue key:
// an order-free join through a hash of the kept MESSAGE records.  With R[i] the
// DATA record's bytes of a kept MESSAGE record (0 elsewhere), Q its 64-bit
// exclusive prefix and J the exclusive prefix of "kept", record i goes to
// journal_dst + 60 J[i] and its DATA record to dst + Q[i].  Five kernels on one
// stream around the fused copy of crc32c_copy.hip:
//
//   1. k_rov_classify: the grid is nblocks x kPackThreads over contiguous
//      record ranges (layout_split), one record per thread and step, staged
//      through LDS a wave's 64 records at a time (crc32c_journal_stage.h).
//      RecordHeader, record type and queue op of EVERY record; keep[] against
//      the type; the sync point's record; then for a kept MESSAGE record its
//      place in the hash (FOLLOW mode), the data offset and the DATA record, in
//      k_spk_classify's order.  Every record leaves its kind (kRov*), R, header
//      + options bytes, the application data's window offset and length and the
//      stored CRC in the workspace -- an empty message when it is refused, not
//      kept or not a MESSAGE record.  The DATA window is read for kept MESSAGE
//      records only.
//   2. k_rov_count: the CONFIRM records' join (FOLLOW mode: the hash is whole
//      once step 1 has ended), then pass 1 of crc32c_pack_layout.h twice: over R
//      and over "kept".
//   3. k_rov_check: unless step 1 refused, every kept record's end against
//      journal_dst_bytes, every DATA record's end against dst_bytes and against
//      where MessageOffsetDwords stops, and the pieces against the copy's limit.
//   4. k_rov_seal: off[i] becomes where record i's application data goes, Q[i] +
//      header + options, and joff[i] its index in the new run -- or, when
//      anything was refused, off an offset past dst_bytes for EVERY record: the
//      copy kernels then refuse every message, own no piece and write neither
//      dst nor their CRCs.
//   (the payload: bmqcrc_launch_copy over the n slots, as it is)
//   5. k_rov_frame: unless refused, the 15 dwords of every kept record, indexed
//      across the grid so that adjacent lanes load adjacent dwords; DataHeader +
//      options as dwords and the padding as bytes; the sync point; the caller's
//      arrays and the mismatches.
//
// No byte outside [journal, +60 n) and [data, +data_bytes) is loaded: the
// journal is read by record index below n only (the hash holds such indices);
// of the DATA window step 1 reads what data_record (crc32c_journal_stage.h)
// reads of a record it finds inside the window, and the frame reads inside that
// record only.  Every size in the format is a word count, so every position
// in dst is a multiple of 4.  Nothing is stored to dst or journal_dst that
// step 3 has not shown to lie below dst_bytes / journal_dst_bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmqcrc_internal.h"
#include "crc32c_join_key.h"
#include "crc32c_journal_stage.h"
#include "crc32c_pack_layout.h"

namespace bmqcrc {
namespace {

constexpr uint32_t kJournalOpSyncPoint = 2;  // JournalOpType (mqbs_filestoreprotocol.h)
// The hash of the kept MESSAGE records (crc32c_join_key.h).  The join asks for
// existence only.
__device__ __forceinline__ JoinTable join_table(const RovArgs& a)
{
    return {a.gslot, a.gslots, a.journal};
}

// Step 1.
__global__ __launch_bounds__(kPackThreads) void k_rov_classify(RovArgs a)
{
    __shared__ uint32_t recs[kWaves * kWaveDwords];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint64_t lo = (uint64_t)blockIdx.x * a.per_block;
    const uint64_t hi = min(lo + a.per_block, a.n);
    uint32_t* mine = recs + wv * kWaveDwords;
    const uint32_t* d = mine + kJournalRecordDwords * lane;
    const uint64_t end = a.data_bytes;
    for (uint64_t base = lo; base < hi; base += kPackThreads) {
        stage(a.journal, base + 64u * wv, hi, mine, lane);
        __syncthreads();
        const uint64_t r = base + tid;
        if (r < hi) {
            const uint32_t w0 = __builtin_bswap32(d[0]);  // type | flags | sequence number's top
            const uint32_t type = w0 >> 28;
            const bool want = a.keep ? a.keep[r] != 0 : true;
            uint64_t app = 0;
            uint32_t len = 0, rec = 0, hdr = 0, exp = 0;
            uint8_t kind = kRovDrop;
            bool header_ok = false;
            if (!record_header_ok(w0, d[1], d[2], d[14], kRecJournalOp)) {
                refuse(a, BMQCRC_ROV_KIND_RECORD_HEADER, r);
            } else if (type == kRecQueueOp) {
                const uint32_t op = __builtin_bswap32(d[8]);  // QueueOpType: PURGE 1 .. ADDITION 4
                if (op < 1 || op > 4) {
                    refuse(a, BMQCRC_ROV_KIND_RECORD_HEADER, r);
                } else {
                    header_ok = true;
                    if (want) {
                        kind = (op & 1u) ? kRovPlain : kRovQueueUri;  // CREATION 2, ADDITION 4
                    }
                }
            } else if (type == kRecJournalOp) {
                header_ok = true;
                if (a.keep && want) {
                    refuse(a, BMQCRC_ROV_KIND_KEEP_JOURNAL_OP, r);
                }
            } else if (type == kRecConfirm) {
                header_ok = true;
                kind = a.follow ? kRovConfirm : want ? kRovPlain : kRovDrop;
            } else if (type == kRecDeletion) {
                header_ok = true;
                kind = want ? kRovPlain : kRovDrop;
            } else {  // a MESSAGE record
                header_ok = true;
                if (want) {
                    if (a.follow) {
                        join_insert(join_table(a), join_key(d, kMsgGuidDword), r);
                    }
                    uint64_t ow;
                    DataRecord dr;
                    if (!data_window_offset(d[8], a.data_file_pos, end, &ow)) {
                        refuse(a, BMQCRC_ROV_KIND_DATA_OFFSET, r);
                    } else if (!data_record(a.data, end, ow, &dr)) {
                        refuse(a, BMQCRC_ROV_KIND_DATA_RECORD, r);
                    } else {
                        kind = kRovMessage;
                        app = dr.app;
                        len = dr.len;
                        rec = (uint32_t)dr.total;  // at most 2^31 - 4
                        hdr = (uint32_t)dr.hdr;
                        exp = __builtin_bswap32(d[13]);  // MessageRecord @52
                    }
                }
            }
            if (r == a.sync_point && header_ok &&
                !(type == kRecJournalOp && __builtin_bswap32(d[6]) == kJournalOpSyncPoint)) {
                refuse(a, BMQCRC_ROV_KIND_SYNC_POINT, r);
            }
            a.ws_off[r] = app;
            a.ws_len[r] = len;
            a.ws_rec[r] = rec;
            a.ws_hdr[r] = hdr;
            a.ws_exp[r] = exp;
            a.kind[r] = kind;
        }
        __syncthreads();  // this step's LDS reads before the next stage
    }
}

// The records as messages (LayoutView), under one of the two prefixes.
__device__ __forceinline__ LayoutView bytes_view(const RovArgs& a)
{
    return {a.ws_off, a.ws_len, a.n, a.off, a.bsum, a.ctr, a.per_block, a.nblocks};
}

__device__ __forceinline__ LayoutView kept_view(const RovArgs& a)
{
    return {a.ws_off, a.ws_len, a.n, a.joff, a.bsum + 2 * kPackBlocks, a.ctr, a.per_block,
            a.nblocks};
}

// Step 2.  A record is decided, counted and scanned by one and the same thread
// (lo + tid + k kPackThreads in all three loops).
__global__ __launch_bounds__(kPackThreads) void k_rov_count(RovArgs a)
{
    if (a.follow) {
        const uint64_t lo = (uint64_t)blockIdx.x * a.per_block;
        const uint64_t hi = min(lo + a.per_block, a.n);
        for (uint64_t i = lo + threadIdx.x; i < hi; i += kPackThreads) {
            if (a.kind[i] == kRovConfirm) {
                const JoinKey k =
                    join_key(a.journal + (uint64_t)kJournalRecordDwords * i, kCfmGuidDword);
                a.kind[i] = join_find(join_table(a), k) ? kRovPlain : kRovDrop;
            }
        }
    }
    __syncthreads();
    layout_count(bytes_view(a), [&a](uint64_t i, uint64_t, uint32_t) {
        return (unsigned long long)a.ws_rec[i];
    });
    __syncthreads();
    layout_count(kept_view(a), [&a](uint64_t i, uint64_t, uint32_t) {
        return a.kind[i] != kRovDrop ? 1ull : 0ull;
    });
}

// Both block prefixes; returns the pieces of all blocks.  Called by the whole block.
__device__ __forceinline__ unsigned long long both_prefixes(const RovArgs& a,
                                                            unsigned long long* bq,
                                                            unsigned long long* bj)
{
    const unsigned long long pieces = block_prefix(bytes_view(a), bq);
    __syncthreads();  // block_prefix's own LDS words are read up to its return
    block_prefix(kept_view(a), bj);
    return pieces;
}

// Step 3: the records, one per thread and step.
__global__ __launch_bounds__(kPackThreads) void k_rov_check(RovArgs a)
{
    __shared__ unsigned long long bq[kPackBlocks + 1], bj[kPackBlocks + 1];
    // Step 1's word: kinds up to DATA_RECORD.  A higher kind is raised by this
    // pass itself and never replaces one of theirs, so the test gives the same
    // answer in every block whenever it starts.
    const unsigned long long word = a.ctr[kSlotCtrRefusal];
    if (word != 0 && (~word >> 56) <= BMQCRC_ROV_KIND_DATA_RECORD) {
        return;
    }
    const unsigned long long pieces = both_prefixes(a, bq, bj);
    const unsigned long long bytes = bq[a.nblocks], kept = bj[a.nblocks];
    // bytes the new DATA file still takes before MessageOffsetDwords overflows
    const unsigned long long room =
        a.new_data_file_pos <= kRecMaxFileBytes ? kRecMaxFileBytes - a.new_data_file_pos : 0ull;
    const uint64_t lo = (uint64_t)blockIdx.x * a.per_block;
    const uint64_t hi = min(lo + a.per_block, a.n);
    for (uint64_t i = lo + threadIdx.x; i < hi; i += kPackThreads) {
        const uint8_t kind = a.kind[i];
        if (kind == kRovDrop) {
            continue;
        }
        const unsigned long long j = a.joff[i] + bj[blockIdx.x];
        bool small = (unsigned long long)(4 * kJournalRecordDwords) * (j + 1) > a.journal_dst_bytes;
        if (kind == kRovMessage) {
            const unsigned long long e = a.off[i] + bq[blockIdx.x] + a.ws_rec[i];
            small = small || e > a.dst_bytes;
            if (e > room) {
                refuse(a, BMQCRC_ROV_KIND_DATA_FILE_FULL, i);
            }
        }
        if (small) {
            refuse(a, BMQCRC_ROV_KIND_DST_TOO_SMALL, i);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (a.sync_point != kRovNoSyncPoint &&
            (unsigned long long)(4 * kJournalRecordDwords) * (kept + 1) > a.journal_dst_bytes) {
            refuse(a, BMQCRC_ROV_KIND_DST_TOO_SMALL, a.n);
        }
        if (a.new_data_file_pos > kRecMaxFileBytes || bytes > room) {
            refuse(a, BMQCRC_ROV_KIND_DATA_FILE_FULL, a.n);
        }
        if (pieces > 0xFFFFFFFFull) {
            refuse(a, BMQCRC_ROV_KIND_TOO_MANY_PIECES, 0);
        }
        a.ctr[kRovCtrData] = bytes;
        a.ctr[kRovCtrKept] = kept;
    }
}

// Step 4.
__global__ __launch_bounds__(kPackThreads) void k_rov_seal(RovArgs a)
{
    __shared__ unsigned long long bq[kPackBlocks + 1], bj[kPackBlocks + 1];
    const uint32_t tid = threadIdx.x;
    const uint64_t lo = (uint64_t)blockIdx.x * a.per_block;
    const uint64_t hi = min(lo + a.per_block, a.n);
    if (a.ctr[kSlotCtrRefusal] != 0) {
        // past any dst_bytes: the copy kernels refuse the message
        for (uint64_t i = lo + tid; i < hi; i += kPackThreads) {
            a.off[i] = ~0ull;
        }
        return;
    }
    both_prefixes(a, bq, bj);
    const unsigned long long qb = bq[blockIdx.x], jb = bj[blockIdx.x];
    for (uint64_t i = lo + tid; i < hi; i += kPackThreads) {
        a.off[i] = a.off[i] + qb + a.ws_hdr[i];
        a.joff[i] = a.kind[i] != kRovDrop ? a.joff[i] + jb : ~0ull;
    }
}

// Step 5, after the copy.  The word is final: on a refusal the host reads kind
// and index from it, and the kernel leaves.
__global__ __launch_bounds__(kPackFrameThreads) void k_rov_frame(RovArgs a)
{
    if (a.ctr[kSlotCtrRefusal] != 0) {
        return;
    }
    const uint64_t stride = (uint64_t)gridDim.x * kPackFrameThreads;
    const uint64_t t0 = (uint64_t)blockIdx.x * kPackFrameThreads + threadIdx.x;
    // Thread t of the grid owns dword t % 15 of record t / 15 (n < 2^32: a
    // dword's index needs 36 bits); the division in 32 bits whenever the
    // call's indices fit.
    const uint64_t ndw = (uint64_t)kJournalRecordDwords * a.n;
    const bool narrow = ndw <= 0xFFFFFFFFull;
    for (uint64_t t = t0; t < ndw; t += stride) {
        const uint64_t m = narrow ? (uint32_t)t / kJournalRecordDwords : t / kJournalRecordDwords;
        const uint32_t j = (uint32_t)(t - kJournalRecordDwords * m);
        const unsigned long long at = a.joff[m];
        if (at == ~0ull) {
            continue;
        }
        const uint8_t kind = a.kind[m];
        uint32_t v = a.journal[t];
        if (kind == kRovMessage && j == 8) {
            // MessageOffsetDwords: where the DATA record went in the new file
            v = __builtin_bswap32(
                (uint32_t)((a.new_data_file_pos + (a.off[m] - a.ws_hdr[m])) >> 3));
        } else if (kind == kRovQueueUri && j == 9) {
            v = 0;  // queueUriRecordOffsetWords: there is no QLIST file
        }
        a.journal_dst[kJournalRecordDwords * at + j] = v;
    }
    // One record per thread and step: its DATA record's frame and its entries.
    unsigned long long bad = 0, lowest = 0, msgs = 0;
    for (uint64_t i = t0; i < a.n; i += stride) {
        uint32_t crc = 0;
        if (a.kind[i] == kRovMessage) {
            const uint32_t len = a.ws_len[i], hdr = a.ws_hdr[i], rec = a.ws_rec[i];
            const uint32_t* src = (const uint32_t*)(a.data + (a.ws_off[i] - hdr));
            uint8_t* dst = a.dst + (a.off[i] - hdr);
            // The record's last two dwords hold its 1..8 padding bytes (rec >= 8).
            // Every load of a group is issued before the group's first store:
            // the compiler cannot move a load across a store that might alias
            // it, and each one is a trip to memory nobody has touched.
            const uint32_t tail0 = src[(rec >> 2) - 2], tail1 = src[(rec >> 2) - 1];
            crc = a.ws_out[i];
            const uint32_t exp = a.ws_exp[i];
            // DataHeader and options as dwords, four at a time
            for (uint32_t w = 0; w < (hdr >> 2); w += 4) {
                uint32_t v[4];
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) {
                    v[k] = w + k < (hdr >> 2) ? src[w + k] : 0u;
                }
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) {
                    if (w + k < (hdr >> 2)) {
                        ((uint32_t*)dst)[w + k] = v[k];
                    }
                }
            }
            // the padding as bytes, so that no word that holds application
            // data is read and written back
            for (uint32_t b = hdr + len; b < rec; ++b) {
                const uint32_t k = b - (rec - 8);  // 0..7; rec is a multiple of 4
                dst[b] = (uint8_t)((k < 4 ? tail0 : tail1) >> (8 * (k & 3u)));
            }
            ++msgs;
            if (crc != exp) {
                ++bad;
                lowest = max(lowest, ~(unsigned long long)i);
            }
        }
        if (a.new_index) {
            a.new_index[i] = (uint32_t)a.joff[i];  // ~0 when not kept
        }
        if (a.out) {
            a.out[i] = crc;
        }
    }
    if (t0 == 0 && a.sync_point != kRovNoSyncPoint) {
        // the run's sync point restated: its PSN, the new timestamp, the new
        // DATA file's end
        const uint32_t* s = a.journal + kJournalRecordDwords * a.sync_point;
        uint32_t* o = a.journal_dst + kJournalRecordDwords * a.ctr[kRovCtrKept];
        const uint64_t end = a.new_data_file_pos + a.ctr[kRovCtrData];
        o[0] = (s[0] & 0xFFFF0000u) | 0x00000050u;  // bytes: 0x50 JOURNAL_OP, flags 0
        o[1] = s[1];
        o[2] = s[2];
        o[3] = __builtin_bswap32((uint32_t)(a.timestamp >> 32));
        o[4] = __builtin_bswap32((uint32_t)a.timestamp);
        o[5] = 0x01000000u;  // byte 23: SyncPointType REGULAR
        o[6] = __builtin_bswap32(kJournalOpSyncPoint);
        o[7] = s[7];
        o[8] = s[8];
        o[9] = s[9];
        o[10] = s[10];
        o[11] = __builtin_bswap32((uint32_t)(end >> 3));
        o[12] = 0;
        o[13] = 0;
        o[14] = kMagicLE;
    }
    msgs = wave_sum(msgs);
    if ((threadIdx.x & 63u) == 0 && msgs) {
        atomicAdd(&a.ctr[kSlotCtrMsgs], msgs);
    }
    if (bad) {
        atomicAdd(&a.ctr[kSlotCtrBad], bad);
        atomicMax(&a.ctr[kSlotCtrFirstBad], lowest);
    }
}

}  // namespace
}  // namespace bmqcrc

using namespace bmqcrc;

extern "C" int bmqcrc_launch_rollover_layout(const RovArgs* a, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_rov_classify, dim3(a->nblocks), dim3(kPackThreads), 0, s, *a);
    hipLaunchKernelGGL(k_rov_count, dim3(a->nblocks), dim3(kPackThreads), 0, s, *a);
    hipLaunchKernelGGL(k_rov_check, dim3(a->nblocks), dim3(kPackThreads), 0, s, *a);
    hipLaunchKernelGGL(k_rov_seal, dim3(a->nblocks), dim3(kPackThreads), 0, s, *a);
    return hipGetLastError() != hipSuccess;
}

extern "C" int bmqcrc_launch_rollover_frame(const RovArgs* a, void* stream)
{
    const uint64_t work = (uint64_t)kJournalRecordDwords * a->n;
    const uint64_t want = (work + kPackFrameThreads - 1) / kPackFrameThreads;
    const uint32_t blocks = (uint32_t)(want > kPackFrameBlocks ? kPackFrameBlocks : want);
    hipLaunchKernelGGL(k_rov_frame, dim3(blocks), dim3(kPackFrameThreads), 0, (hipStream_t)stream,
                       *a);
    return hipGetLastError() != hipSuccess;
}
