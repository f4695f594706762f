// crc32c_records_unpack.hip -- MI355X (gfx950) walk of device-resident journal
// and DATA records (bmqcrc_message_records_unpack, ABI 2.13; DESIGN.md
// section 15).
//
// The inverse of crc32c_records_pack.hip and the device-side form of the
// MESSAGE-record branch of walk_recovery (bmqcrc_protocol.cpp): given a run of
// 60-byte journal records and a window of the DATA file in HBM it finds every
// selected MessageRecord, checks it and its DataHeader as
// FileStore::recoverMessages does, and yields the per-message arrays the
// packers take.  Journal records lie at fixed positions, so every record is
// independent: the walk is a map, a scan and a scatter.  Three kernels on one
// stream, around the fold of crc32c_kernels.hip:
//
//   1. k_recunp_classify: the grid is nblocks x kPackThreads and block b owns
//      the contiguous records [b per_block, (b + 1) per_block), one record per
//      thread and step, staged through LDS a wave's 64 records at a time
//      (crc32c_journal_stage.h).  The record is checked in the host walk's order --
//      RecordHeader, then for a MESSAGE record GUID and queue key, the data
//      offset, and, when selected, the DATA record -- and the first violation
//      raises the call's refusal word (crc32c_pack_layout.h).  It leaves
//      pre[r] = message flag | BLOCK-LOCAL exclusive prefix of the flags, for
//      a record that takes a slot rec_off / rec_len / rec_flags, and per block
//      the messages and the skipped records in bsum.
//   2. k_recunp_place: every block scans the block sums (block_prefix); more
//      messages than msg_cap is a refusal naming the record that would take
//      slot msg_cap.  Unless refused, record r goes to slot bpre[block] +
//      local prefix: offset, length and stored CRC to the WORKSPACE, which the
//      fold reads, the other fields to the caller's arrays.  The slots no
//      message took -- all of them when anything was refused -- become empty
//      messages (empty_slots of crc32c_unpack_slots.h).
//   (the fold: bmqcrc_launch_batch over the msg_cap slots, when out != NULL)
//   3. k_recunp_publish: unless refused, the workspace's offsets, lengths,
//      stored CRCs and computed CRCs to the caller's arrays, the mismatches
//      counted.
//
// No byte outside [journal, +60 n_records) and [data, +data_bytes) is loaded:
// the journal is read by record index below n_records only; of the DATA window
// step 1 reads what data_record (crc32c_journal_stage.h) reads of a selected
// record it finds inside the window.  Every offset is 64 bits wide: 8 x
// MessageOffsetDwords reaches 2^35, and the sums above add at most 2^31 to it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmqcrc_internal.h"
#include "crc32c_journal_stage.h"
#include "crc32c_pack_layout.h"
#include "crc32c_unpack_slots.h"

namespace bmqcrc {
namespace {

// byte-aligned dword: a GUID or queue-key array need not be 4-byte aligned
typedef uint32_t u32u __attribute__((aligned(1)));

// Step 1.
__global__ __launch_bounds__(kPackThreads) void k_recunp_classify(RecUnpackArgs a)
{
    __shared__ uint32_t recs[kWaves * kWaveDwords];
    __shared__ uint32_t wtot[kWaves];
    __shared__ unsigned long long wskip[kWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint64_t lo = (uint64_t)blockIdx.x * a.per_block;
    const uint64_t hi = min(lo + a.per_block, a.n_records);
    uint32_t* mine = recs + wv * kWaveDwords;
    const uint32_t* d = mine + kJournalRecordDwords * lane;
    const uint64_t end = a.data_bytes;
    uint32_t carry = 0;  // (a block's records are fewer than 2^31)
    unsigned long long skipped = 0;
    for (uint64_t base = lo; base < hi; base += kPackThreads) {
        stage(a.journal, base + 64u * wv, hi, mine, lane);
        __syncthreads();
        const uint64_t r = base + tid;
        bool msg = false;
        if (r < hi) {
            const uint32_t w0 = __builtin_bswap32(d[0]);  // type | flags | sequence number's top
            const uint32_t type = w0 >> 28;
            if (!record_header_ok(w0, d[1], d[2], d[14], kRecAnyType)) {
                refuse(a, BMQCRC_RECUNP_KIND_RECORD_HEADER, r);
            } else if (type == kRecMessage) {
                // GUID @36..51, queue key @22..26
                const bool unset = (d[9] | d[10] | d[11] | d[12]) == 0 ||
                                   ((d[5] >> 16) | (d[6] & 0xFFFFFFu)) == 0;
                uint64_t ow;
                DataRecord dr;
                if (unset) {
                    refuse(a, BMQCRC_RECUNP_KIND_MESSAGE_RECORD, r);
                } else if (!data_window_offset(d[8], a.data_file_pos, end, &ow)) {
                    refuse(a, BMQCRC_RECUNP_KIND_DATA_OFFSET, r);
                } else if (a.select && a.select[r] == 0) {
                    ++skipped;  // no byte of its DATA record is read
                } else if (!data_record(a.data, end, ow, &dr)) {
                    refuse(a, BMQCRC_RECUNP_KIND_DATA_RECORD, r);
                } else {
                    msg = true;
                    a.rec_off[r] = dr.app;
                    a.rec_len[r] = dr.len;
                    a.rec_flags[r] = (uint8_t)dr.h1;
                }
            }
            // (any other type: validated above and skipped, as the host walk skips it)
        }
        const unsigned long long mask = __ballot(msg);
        const uint32_t below = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) {
            wtot[wv] = (uint32_t)__popcll(mask);
        }
        __syncthreads();
        uint32_t woff = 0, tot = 0;
        for (uint32_t w = 0; w < kWaves; ++w) {
            woff += w < wv ? wtot[w] : 0u;
            tot += wtot[w];
        }
        __syncthreads();  // (also orders this step's LDS reads before the next stage)
        if (r < hi) {
            a.pre[r] = (msg ? kRecUnpMsgFlag : 0u) | (carry + woff + below);
        }
        carry += tot;
    }
    skipped = wave_sum(skipped);
    if (lane == 0) {
        wskip[wv] = skipped;
    }
    __syncthreads();
    if (tid == 0) {
        unsigned long long t = 0;
        for (uint32_t w = 0; w < kWaves; ++w) {
            t += wskip[w];
        }
        a.bsum[blockIdx.x] = carry;
        a.bsum[kPackBlocks + blockIdx.x] = t;
    }
}

// Step 2.
__global__ __launch_bounds__(kPackThreads) void k_recunp_place(RecUnpackArgs a)
{
    __shared__ uint32_t recs[kWaves * kWaveDwords];
    __shared__ unsigned long long bpre[kPackBlocks + 1];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint64_t lo = (uint64_t)blockIdx.x * a.per_block;
    const uint64_t hi = min(lo + a.per_block, a.n_records);
    // Step 1's word.  A block that starts late may read TOO_MANY_MESSAGES
    // raised below by another block of this pass instead: then all > msg_cap
    // holds here as well, and `refused` is the same answer in every block.
    const bool classified_clean = a.ctr[kSlotCtrRefusal] == 0;
    const unsigned long long skipped = block_prefix(a, bpre);
    const unsigned long long all = bpre[a.nblocks];
    const unsigned long long before = bpre[blockIdx.x], after = bpre[blockIdx.x + 1];
    const bool refused = !classified_clean || all > a.msg_cap;
    if (blockIdx.x == 0 && tid == 0) {
        a.ctr[kSlotCtrMsgs] = all;
        a.ctr[kRecUnpCtrSkipped] = skipped;
    }
    if (before <= a.msg_cap && a.msg_cap < after) {
        // the record that would take slot msg_cap lies in this block
        for (uint64_t r = lo + tid; r < hi; r += kPackThreads) {
            const uint32_t p = a.pre[r];
            if ((p & kRecUnpMsgFlag) && before + (p & ~kRecUnpMsgFlag) == a.msg_cap) {
                refuse(a, BMQCRC_RECUNP_KIND_TOO_MANY_MESSAGES, r);
            }
        }
    }
    if (!refused) {
        uint32_t* mine = recs + wv * kWaveDwords;
        const uint32_t* d = mine + kJournalRecordDwords * lane;
        for (uint64_t base = lo; base < hi; base += kPackThreads) {
            stage(a.journal, base + 64u * wv, hi, mine, lane);
            __syncthreads();
            const uint64_t r = base + tid;
            const uint32_t p = r < hi ? a.pre[r] : 0u;
            if (p & kRecUnpMsgFlag) {
                const uint64_t i = before + (p & ~kRecUnpMsgFlag);  // < all <= msg_cap
                a.ws_off[i] = a.rec_off[r];
                a.ws_len[i] = a.rec_len[r];
                a.ws_exp[i] = __builtin_bswap32(d[13]);
                if (a.record_index) {
                    a.record_index[i] = (uint32_t)r;
                }
                if (a.queue_keys) {
                    uint8_t* q = a.queue_keys + 5 * i;
                    *(u32u*)q = (d[5] >> 16) | (d[6] << 16);
                    q[4] = (uint8_t)(d[6] >> 16);
                }
                if (a.guids) {
                    u32u* g = (u32u*)(a.guids + 16 * i);
                    g[0] = d[9];
                    g[1] = d[10];
                    g[2] = d[11];
                    g[3] = d[12];
                }
                if (a.data_flags) {
                    a.data_flags[i] = a.rec_flags[r];
                }
                if (a.ref_counts) {
                    // @20 the high 8 bits, the RecordHeader's 12 flag bits the low ones
                    a.ref_counts[i] =
                        ((d[5] & 0xFFu) << 12) | ((__builtin_bswap32(d[0]) >> 16) & 0xFFFu);
                }
                if (a.timestamps) {
                    a.timestamps[i] = ((uint64_t)__builtin_bswap32(d[3]) << 32) |
                                      __builtin_bswap32(d[4]);
                }
            }
            __syncthreads();  // this step's LDS reads before the next stage
        }
    }
    empty_slots(a, refused ? 0 : all, kPackThreads);
}

// Step 3, after the fold.  The loop is k_unpack_publish's: as one function
// behind the early return it cost this kernel two SGPRs (profiles/r14/unpack_slots).
__global__ __launch_bounds__(kUnpackPublishThreads) void k_recunp_publish(RecUnpackArgs a)
{
    if (a.ctr[kSlotCtrRefusal] != 0) {
        return;
    }
    const uint64_t t0 = (uint64_t)blockIdx.x * kUnpackPublishThreads + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * kUnpackPublishThreads;
    const uint64_t n = a.ctr[kSlotCtrMsgs];  // <= msg_cap: k_recunp_place
    unsigned long long bad = 0, lowest = 0;
    for (uint64_t i = t0; i < n; i += stride) {
        const uint32_t exp = a.ws_exp[i];
        a.app_offsets[i] = a.ws_off[i];
        a.lengths[i] = a.ws_len[i];
        if (a.expected) {
            a.expected[i] = exp;
        }
        if (a.out) {
            const uint32_t crc = a.ws_out[i];
            a.out[i] = crc;
            if (crc != exp) {
                ++bad;
                lowest = max(lowest, ~(unsigned long long)i);
            }
        }
    }
    if (bad) {
        atomicAdd(&a.ctr[kSlotCtrBad], bad);
        atomicMax(&a.ctr[kSlotCtrFirstBad], lowest);
    }
}

}  // namespace
}  // namespace bmqcrc

using namespace bmqcrc;

extern "C" int bmqcrc_launch_records_unpack_walk(const RecUnpackArgs* a, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_recunp_classify, dim3(a->nblocks), dim3(kPackThreads), 0, s, *a);
    hipLaunchKernelGGL(k_recunp_place, dim3(a->nblocks), dim3(kPackThreads), 0, s, *a);
    return hipGetLastError() != hipSuccess;
}

extern "C" int bmqcrc_launch_records_unpack_publish(const RecUnpackArgs* a, void* stream)
{
    const uint64_t want = (a->msg_cap + kUnpackPublishThreads - 1) / kUnpackPublishThreads;
    const uint32_t blocks =
        (uint32_t)(want > kUnpackPublishBlocks ? kUnpackPublishBlocks : want < 1 ? 1 : want);
    hipLaunchKernelGGL(k_recunp_publish, dim3(blocks), dim3(kUnpackPublishThreads), 0,
                       (hipStream_t)stream, *a);
    return hipGetLastError() != hipSuccess;
}
