// crc32c_expire_records.hip -- MI355X (gfx950): the messages of a
// device-resident partition whose TTL has run out, turned into the DELETION
// records the primary's garbage collection appends
// (bmqcrc_expire_records_pack, ABI 2.20).
//
// The device-side form of FileBackedStorage::gcExpiredMessages over
// FileStore::writeDeletionRecord.  There is no CRC in this call: no payload
// byte is read.  Nothing persists between calls: which messages a queue still
// holds is derived from the run, as recovery derives it.  With key = (GUID,
// queue key), for a selected MESSAGE record m of the run: live(m) when no
// DELETION record of the run has its key, queue(m) the table entry with its
// queue key, young(m) when it is live, has a queue q and (now - ts(m)) mod 2^64
// <= ttl_seconds[q], front(q) the lowest young record of q, expired(m) when it
// is live, has a queue q and m < front(q).  The reference walks each queue from
// its head and stops at the first message that has not expired; front(q) is
// that message, and every one of these is a reduction that needs no order.
// Six kernels on one stream:
//
//   1. k_exp_classify: the grid is nblocks x kPackThreads over contiguous
//      record ranges (layout_split), one record per thread and step, staged
//      through LDS a wave's 64 records at a time (crc32c_journal_stage.h).  The
//      RecordHeader of EVERY record; every selected MESSAGE record into the hash
//      (crc32c_join_key.h), where one that meets its own key raises
//      DUPLICATE_MESSAGE with the lower record of the two.  The same blocks
//      over contiguous ranges of the queue table: an entry into the queue hash,
//      where an all-zero key, or one that meets its own key (the lower entry of
//      the two), raises QUEUE_KEY.  The lowest of a group always meets another
//      or is met by all of them, whichever was inserted first, so the lowest
//      index is named whatever the interleaving.
//   2. k_exp_join: both hashes are whole.  The run's DELETION records probe the
//      first and raise dead of their message; every selected MESSAGE record
//      probes the second and leaves its queue.
//   3. k_exp_front: dead is whole.  A young message lowers front of its queue
//      with atomicMin, in LDS first when the table fits there.  (One kernel for
//      2 and 3 would read dead while it is written.)
//   4. k_exp_check: front is whole.  Pass 1 of crc32c_pack_layout.h over
//      "expired".
//   5. k_exp_seal: the block prefix: off[r] becomes j (~0 when not expired);
//      every record's end against journal_dst_bytes; the counts, per queue too.
//   6. k_exp_frame (not when size-only): unless refused, the 15 dwords of every
//      written record, indexed across the grid so that adjacent lanes store
//      adjacent dwords, and the caller's arrays.
//
// No byte outside [journal, +60 n_records), select's n_records bytes and the
// table's 5 n_queues and 8 n_queues bytes is loaded: the journal is read by
// record index below n_records only (the hash holds such indices), the table by
// entry below n_queues only (the queue hash holds such entries).  Nothing is
// stored to journal_dst that step 5 has not shown to end at or below
// journal_dst_bytes, and nothing to an output array at or past its n_records or
// n_queues entries.  journal_dst may follow the run in one allocation: the run
// is only read, the destination only written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmqcrc_internal.h"
#include "crc32c_join_key.h"
#include "crc32c_journal_stage.h"
#include "crc32c_pack_layout.h"

namespace bmqcrc {
namespace {

__device__ __forceinline__ JoinTable join_table(const ExpArgs& a)
{
    return {a.gslot, a.gslots, a.journal};
}

// ---- the queue table's hash: a slot holds entry + 1 (0: empty) and no key, a
// probe compares with queue_keys itself.  A power of two of slots, at least
// twice the entries, zeroed before the call; nothing is ever removed.

// A queue key as the join holds one (q0, q1), under the null GUID.
__device__ __forceinline__ JoinKey queue_key(uint32_t q0, uint32_t q1)
{
    return {{0u, 0u, 0u, 0u}, q0, q1};
}

// Entry e's.
__device__ __forceinline__ JoinKey queue_key_of(const ExpArgs& a, uint64_t e)
{
    const uint8_t null_guid[16] = {0};
    return join_key_bytes(null_guid, a.queue_keys + 5 * e);
}

// Entry e, whose key is k, into the table unless its key is there already:
// returns 0 when e took a slot, otherwise entry + 1 of the one that holds it.
__device__ __forceinline__ uint32_t queue_insert(const ExpArgs& a, const JoinKey& k, uint64_t e)
{
    const uint64_t mask = a.qslots - 1;
    uint64_t s = key_hash(k) & mask;
    for (uint64_t step = 0; step < a.qslots; ++step, s = (s + 1) & mask) {
        const uint32_t cur = atomicCAS(&a.qslot[s], 0u, (uint32_t)e + 1u);
        if (cur == 0) {
            return 0;
        }
        if (same_key(k, queue_key_of(a, cur - 1u))) {
            return cur;
        }
    }
    return 0;
}

// Entry + 1 of the one that has this key, 0 when none has.  For a table that
// is whole (or has no slot at all: n_queues 0).
__device__ __forceinline__ uint32_t queue_find(const ExpArgs& a, const JoinKey& k)
{
    const uint64_t mask = a.qslots - 1;
    uint64_t s = key_hash(k) & mask;
    for (uint64_t step = 0; step < a.qslots; ++step, s = (s + 1) & mask) {
        const uint32_t cur = a.qslot[s];
        if (cur == 0) {
            return 0;
        }
        if (same_key(k, queue_key_of(a, cur - 1u))) {
            return cur;
        }
    }
    return 0;
}

// Step 1.
__global__ __launch_bounds__(kPackThreads) void k_exp_classify(ExpArgs a)
{
    __shared__ uint32_t recs[kWaves * kWaveDwords];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    if (blockIdx.x < a.nblocks) {  // (the whole block takes one side)
        const uint64_t lo = (uint64_t)blockIdx.x * a.per_block;
        const uint64_t hi = min(lo + a.per_block, a.n_records);
        uint32_t* mine = recs + wv * kWaveDwords;
        const uint32_t* d = mine + kJournalRecordDwords * lane;
        for (uint64_t base = lo; base < hi; base += kPackThreads) {
            stage(a.journal, base + 64u * wv, hi, mine, lane);
            __syncthreads();
            const uint64_t r = base + tid;
            if (r < hi) {
                const uint32_t w0 = __builtin_bswap32(d[0]);  // type | flags | sequence number's top
                const uint32_t type = w0 >> 28;
                uint8_t kind = kExpOther;
                if (!record_header_ok(w0, d[1], d[2], d[14], kRecJournalOp)) {
                    refuse(a, BMQCRC_EXP_KIND_RECORD_HEADER, r);
                } else if (type == kRecQueueOp) {
                    const uint32_t op = __builtin_bswap32(d[8]);  // QueueOpType: PURGE 1 .. ADDITION 4
                    if (op < 1 || op > 4) {
                        refuse(a, BMQCRC_EXP_KIND_RECORD_HEADER, r);
                    }
                } else if (type == kRecMessage) {
                    if (a.select ? a.select[r] != 0 : true) {
                        kind = kExpMessage;
                        const uint32_t met =
                            join_insert(join_table(a), join_key(d, kMsgGuidDword), r);
                        if (met) {
                            refuse(a, BMQCRC_EXP_KIND_DUPLICATE_MESSAGE,
                                   min(r, (uint64_t)(met - 1u)));
                        }
                    }
                } else if (type == kRecDeletion) {
                    kind = kExpDeletion;
                }
                a.kind[r] = kind;
            }
            __syncthreads();  // this step's LDS reads before the next stage
        }
    }
    if (blockIdx.x < a.qnblocks) {
        const uint64_t lo = (uint64_t)blockIdx.x * a.qper_block;
        const uint64_t hi = min(lo + a.qper_block, a.n_queues);
        for (uint64_t e = lo + tid; e < hi; e += kPackThreads) {
            const JoinKey k = queue_key_of(a, e);
            if ((k.q0 | k.q1) == 0) {
                refuse(a, BMQCRC_EXP_KIND_QUEUE_KEY, e);
            } else {
                const uint32_t met = queue_insert(a, k, e);
                if (met) {
                    refuse(a, BMQCRC_EXP_KIND_QUEUE_KEY, min(e, (uint64_t)(met - 1u)));
                }
            }
        }
    }
}

// Step 2.
__global__ __launch_bounds__(kPackThreads) void k_exp_join(ExpArgs a)
{
    const JoinTable t = join_table(a);
    const uint64_t lo = (uint64_t)blockIdx.x * a.per_block;
    const uint64_t hi = min(lo + a.per_block, a.n_records);
    for (uint64_t r = lo + threadIdx.x; r < hi; r += kPackThreads) {
        const uint8_t kind = a.kind[r];
        const uint32_t* d = a.journal + (uint64_t)kJournalRecordDwords * r;
        if (kind == kExpDeletion) {
            const uint32_t m = join_find(t, join_key_deletion(d));
            if (m) {
                a.dead[m - 1u] = 1;  // whoever stores, stores 1
            }
        } else if (kind == kExpMessage) {
            // bytes 22..26, as join_key takes them
            a.queue[r] = queue_find(a, queue_key(d[5] >> 16, d[6] & 0x00FFFFFFu)) - 1u;  // 0: kExpNone
        }
    }
}

// queue(m) of a live MESSAGE record, kExpNone for every other record and for a
// live one without an entry.
__device__ __forceinline__ uint32_t live_queue(const ExpArgs& a, uint64_t r)
{
    return a.kind[r] == kExpMessage && !a.dead[r] ? a.queue[r] : kExpNone;
}

// Step 3.  A table of at most kExpLdsQueues entries is reduced in LDS first, and
// a block then lowers a queue's front once: the messages of one queue would
// otherwise queue up behind one another at one word of memory.
__global__ __launch_bounds__(kPackThreads) void k_exp_front(ExpArgs a)
{
    __shared__ uint32_t lfront[kExpLdsQueues];
    const bool local = a.n_queues <= kExpLdsQueues;
    if (local) {
        for (uint32_t q = threadIdx.x; q < a.n_queues; q += kPackThreads) {
            lfront[q] = kExpNone;
        }
        __syncthreads();
    }
    const uint64_t lo = (uint64_t)blockIdx.x * a.per_block;
    const uint64_t hi = min(lo + a.per_block, a.n_records);
    for (uint64_t r = lo + threadIdx.x; r < hi; r += kPackThreads) {
        const uint32_t q = live_queue(a, r);
        if (q == kExpNone) {
            continue;
        }
        const uint32_t* d = a.journal + (uint64_t)kJournalRecordDwords * r;
        const uint64_t ts = ((uint64_t)__builtin_bswap32(d[3]) << 32) | __builtin_bswap32(d[4]);
        // unsigned, and it wraps: a timestamp in the future reads as expired
        // (mqbs_filebackedstorage.cpp:809).  A front only ever falls, so a
        // record at or above what it reads has nothing to lower.
        if (a.now - ts <= a.ttl_seconds[q]) {
            if (local) {
                if ((uint32_t)r < lfront[q]) {
                    atomicMin(&lfront[q], (uint32_t)r);
                }
            } else if ((uint32_t)r < a.front[q]) {
                atomicMin(&a.front[q], (uint32_t)r);
            }
        }
    }
    if (local) {
        __syncthreads();
        for (uint32_t q = threadIdx.x; q < a.n_queues; q += kPackThreads) {
            if (lfront[q] != kExpNone) {
                atomicMin(&a.front[q], lfront[q]);
            }
        }
    }
}

// expired(m): for a front that is whole.
__device__ __forceinline__ bool expired(const ExpArgs& a, uint64_t r, uint32_t* q)
{
    *q = live_queue(a, r);
    return *q != kExpNone && (uint32_t)r < a.front[*q];  // kExpNone: every one has expired
}

// The records as messages (LayoutView): the pass reads a source offset and a
// length of every entry, of which this call has neither -- it is handed off and
// queue, n_records entries each, and the pieces it counts from them are not
// used.
__device__ __forceinline__ LayoutView records_view(const ExpArgs& a)
{
    return {a.off, a.queue, a.n_records, a.off, a.bsum, a.ctr, a.per_block, a.nblocks};
}

// Step 4.
__global__ __launch_bounds__(kPackThreads) void k_exp_check(ExpArgs a)
{
    layout_count(records_view(a), [&a](uint64_t r, uint64_t, uint32_t) {
        uint32_t q;
        return expired(a, r, &q) ? 1ull : 0ull;
    });
}

// Step 5.
__global__ __launch_bounds__(kPackThreads) void k_exp_seal(ExpArgs a)
{
    __shared__ unsigned long long bpre[kPackBlocks + 1];
    __shared__ uint32_t lcount[kExpLdsQueues];  // as k_exp_front's lfront
    const bool local = a.n_queues <= kExpLdsQueues;
    if (local) {
        for (uint32_t q = threadIdx.x; q < a.n_queues; q += kPackThreads) {
            lcount[q] = 0;
        }
    }
    block_prefix(records_view(a), bpre);  // (its barriers stand behind the zeroes)
    const unsigned long long before = bpre[blockIdx.x];
    const uint64_t lo = (uint64_t)blockIdx.x * a.per_block;
    const uint64_t hi = min(lo + a.per_block, a.n_records);
    unsigned long long live = 0, no_queue = 0;
    for (uint64_t r = lo + threadIdx.x; r < hi; r += kPackThreads) {
        uint32_t q;
        if (!expired(a, r, &q)) {
            a.off[r] = ~0ull;
            if (a.kind[r] == kExpMessage && !a.dead[r]) {
                ++live;
                no_queue += q == kExpNone ? 1u : 0u;
            }
            continue;
        }
        ++live;
        const unsigned long long j = a.off[r] + before;
        a.off[r] = j;
        if (!a.size_only &&
            (unsigned long long)(4 * kJournalRecordDwords) * (j + 1) > a.journal_dst_bytes) {
            refuse(a, BMQCRC_EXP_KIND_DST_TOO_SMALL, r);
        }
        if (local) {
            atomicAdd(&lcount[q], 1u);
        } else {
            atomicAdd(&a.qcount[q], 1u);
        }
    }
    if (local) {
        __syncthreads();
        for (uint32_t q = threadIdx.x; q < a.n_queues; q += kPackThreads) {
            if (lcount[q]) {
                atomicAdd(&a.qcount[q], lcount[q]);
            }
        }
    }
    live = wave_sum(live);
    no_queue = wave_sum(no_queue);
    if ((threadIdx.x & 63u) == 0) {
        if (live) {
            atomicAdd(&a.ctr[kExpCtrLive], live);
        }
        if (no_queue) {
            atomicAdd(&a.ctr[kExpCtrNoQueue], no_queue);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.ctr[kExpCtrExpired] = bpre[a.nblocks];
    }
}

// Step 6.  The word is final: on a refusal the host reads kind and index from
// it, and the kernel leaves.
__global__ __launch_bounds__(kPackFrameThreads) void k_exp_frame(ExpArgs a)
{
    if (a.ctr[kExpCtrRefusal] != 0) {
        return;
    }
    const uint64_t stride = (uint64_t)gridDim.x * kPackFrameThreads;
    const uint64_t t0 = (uint64_t)blockIdx.x * kPackFrameThreads + threadIdx.x;
    // Thread t of the grid owns dword t % 15 of record t / 15's DELETION record
    // (n_records < 2^32: a dword's index needs 36 bits); the division in 32
    // bits whenever the call's indices fit.
    const uint64_t ndw = (uint64_t)kJournalRecordDwords * a.n_records;
    const bool narrow = ndw <= 0xFFFFFFFFull;
    const uint8_t* bytes = (const uint8_t*)a.journal;
    for (uint64_t t = t0; t < ndw; t += stride) {
        const uint64_t r = narrow ? (uint32_t)t / kJournalRecordDwords : t / kJournalRecordDwords;
        const uint32_t j = (uint32_t)(t - kJournalRecordDwords * r);
        const unsigned long long at = a.off[r];
        if (at == ~0ull) {
            continue;
        }
        uint32_t v;
        if (j < 5) {
            const uint64_t seq = a.first_seq + at;
            v = j == 0   ? (kRecDeletion << 28) | (kDeletionFlagTtl << 16) | (uint32_t)(seq >> 32)
                : j == 1 ? (uint32_t)seq
                : j == 2 ? a.lease_id
                : j == 3 ? (uint32_t)(a.now >> 32)
                         : (uint32_t)a.now;
            v = __builtin_bswap32(v);
        } else if (j == 14) {
            v = kMagicLE;
        } else {
            // bytes 20..55: the queue key at 23 from the MESSAGE record's 22, the
            // GUID at 28 from its 36
            v = 0;
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t p = 4 * j + k;
                uint32_t b = 0;
                if (p >= 23 && p < 28) {
                    b = bytes[4 * kJournalRecordDwords * r + (p - 1)];
                } else if (p >= 28 && p < 44) {
                    b = bytes[4 * kJournalRecordDwords * r + (p + 8)];
                }
                v |= b << (8 * k);
            }
        }
        a.journal_dst[kJournalRecordDwords * at + j] = v;
    }
    for (uint64_t r = t0; r < a.n_records; r += stride) {
        const unsigned long long at = a.off[r];
        if (a.expired) {
            a.expired[r] = at != ~0ull ? 1 : 0;
        }
        if (a.new_index) {
            a.new_index[r] = (uint32_t)at;  // ~0 when not expired
        }
        if (a.select_out) {
            a.select_out[r] = a.kind[r] == kExpMessage && !a.dead[r] && at == ~0ull ? 1 : 0;
        }
    }
    for (uint64_t q = t0; q < a.n_queues; q += stride) {
        if (a.queue_expired) {
            a.queue_expired[q] = a.qcount[q];
        }
        if (a.queue_front) {
            a.queue_front[q] = a.front[q];
        }
    }
}

}  // namespace
}  // namespace bmqcrc

using namespace bmqcrc;

extern "C" int bmqcrc_launch_expire_records_layout(const ExpArgs* a, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    const uint32_t blocks = a->nblocks > a->qnblocks ? a->nblocks : a->qnblocks;
    hipLaunchKernelGGL(k_exp_classify, dim3(blocks), dim3(kPackThreads), 0, s, *a);
    hipLaunchKernelGGL(k_exp_join, dim3(a->nblocks), dim3(kPackThreads), 0, s, *a);
    hipLaunchKernelGGL(k_exp_front, dim3(a->nblocks), dim3(kPackThreads), 0, s, *a);
    hipLaunchKernelGGL(k_exp_check, dim3(a->nblocks), dim3(kPackThreads), 0, s, *a);
    hipLaunchKernelGGL(k_exp_seal, dim3(a->nblocks), dim3(kPackThreads), 0, s, *a);
    return hipGetLastError() != hipSuccess;
}

extern "C" int bmqcrc_launch_expire_records_frame(const ExpArgs* a, void* stream)
{
    const uint64_t units = a->n_records > a->n_queues / kJournalRecordDwords
                               ? a->n_records
                               : a->n_queues / kJournalRecordDwords;
    const uint64_t work = (uint64_t)kJournalRecordDwords * units;
    const uint64_t want = (work + kPackFrameThreads - 1) / kPackFrameThreads;
    const uint32_t blocks = (uint32_t)(want > kPackFrameBlocks ? kPackFrameBlocks : want);
    hipLaunchKernelGGL(k_exp_frame, dim3(blocks ? blocks : 1u), dim3(kPackFrameThreads), 0,
                       (hipStream_t)stream, *a);
    return hipGetLastError() != hipSuccess;
}
