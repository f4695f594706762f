// crc32c_confirm_records.hip -- MI355X (gfx950): a batch of consumer confirms
// turned into the CONFIRM and DELETION records of a device-resident partition
// (bmqcrc_confirm_records_pack, ABI 2.19).
//
// The device-side form of FileBackedStorage::confirm over
// FileStore::writeConfirmRecord and, when a message's count reaches zero,
// FileBackedStorage::remove over FileStore::writeDeletionRecord.  There is no
// CRC in this call: a confirm carries no payload.  Nothing persists between
// calls: the outstanding count of a message is derived from the run, as
// recovery derives it.  With key = (GUID, queue key), for a selected MESSAGE
// record m of the run: dead(m) when a DELETION record of the run has its key,
// had(m) the CONFIRM records of the run with its key whose reason is not
// AUTO_CONFIRMED, left(m) = max(refCount(m) - had(m), 0), c(m) the confirms of
// this call with its key and last(m) the highest of them.  Confirm i with a
// live target m writes one record at journal_dst + 60 j, j the confirms below
// i that have a target: a DELETION record when i == last(m) and c(m) ==
// left(m), a CONFIRM record otherwise.  Every one of these is a reduction that
// needs no order.  Five kernels on one stream:
//
//   1. k_cfm_classify: the grid is nblocks x kPackThreads over contiguous
//      record ranges (layout_split), one record per thread and step, staged
//      through LDS a wave's 64 records at a time (crc32c_journal_stage.h).  The
//      RecordHeader of EVERY record; every selected MESSAGE record into the hash
//      (crc32c_join_key.h), where one that meets its own key raises
//      DUPLICATE_MESSAGE with the lower record of the two -- the lowest record
//      of a group always meets another or is met by all of them, whichever was
//      inserted first, so the lowest index is named whatever the interleaving.
//      Every record leaves its kind (kCfm*) and its refCount.
//   2. k_cfm_join: the hash is whole.  The run's CONFIRM and DELETION records
//      probe it and raise had / dead of their message; the call's confirms
//      probe it, leave their hit and raise c and last.  NULL_KEY and REASON.
//      Neither half reads what the other writes.
//   3. k_cfm_check: had, dead, c and last are whole.  OVER_CONFIRMED, and pass 1
//      of crc32c_pack_layout.h over "has a live target".
//   4. k_cfm_seal: the block prefix: off[i] becomes j (~0 without a target);
//      every record's end against journal_dst_bytes; the counts.
//   5. k_cfm_frame (not when size-only): unless refused, the 15 dwords of every
//      written record, indexed across the grid so that adjacent lanes store
//      adjacent dwords, and the caller's arrays.
//
// No byte outside [journal, +60 n_records) and the n-entry input arrays is
// loaded: the journal is read by record index below n_records only (the hash
// holds such indices).  Nothing is stored to journal_dst that step 4 has not
// shown to end at or below journal_dst_bytes, and nothing to an output array
// at or past its n (left_out: n_records) entries.  journal_dst may follow the
// run in one allocation: the run is only read, the destination only written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmqcrc_internal.h"
#include "crc32c_join_key.h"
#include "crc32c_journal_stage.h"
#include "crc32c_pack_layout.h"

namespace bmqcrc {
namespace {

__device__ __forceinline__ JoinTable join_table(const CfmArgs& a)
{
    return {a.gslot, a.gslots, a.journal};
}

// Step 1.
__global__ __launch_bounds__(kPackThreads) void k_cfm_classify(CfmArgs a)
{
    __shared__ uint32_t recs[kWaves * kWaveDwords];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
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
            const uint32_t type = w0 >> 28, flags = (w0 >> 16) & 0xFFFu;
            uint8_t kind = kCfmOther;
            uint32_t ref = 0;
            if (!record_header_ok(w0, d[1], d[2], d[14], kRecJournalOp)) {
                refuse(a, BMQCRC_CFM_KIND_RECORD_HEADER, r);
            } else if (type == kRecQueueOp) {
                const uint32_t op = __builtin_bswap32(d[8]);  // QueueOpType: PURGE 1 .. ADDITION 4
                if (op < 1 || op > 4) {
                    refuse(a, BMQCRC_CFM_KIND_RECORD_HEADER, r);
                }
            } else if (type == kRecMessage) {
                if (a.select ? a.select[r] != 0 : true) {
                    kind = kCfmMessage;
                    ref = ((d[5] & 0xFFu) << 12) | flags;  // byte 20 above the flags' 12 bits
                    const uint32_t met = join_insert(join_table(a), join_key(d, kMsgGuidDword), r);
                    if (met) {
                        refuse(a, BMQCRC_CFM_KIND_DUPLICATE_MESSAGE, min(r, (uint64_t)(met - 1u)));
                    }
                }
            } else if (type == kRecConfirm) {
                kind = flags == kConfirmReasonAuto ? kCfmOther : kCfmConfirm;
            } else if (type == kRecDeletion) {
                kind = kCfmDeletion;
            }
            a.kind[r] = kind;
            a.ref[r] = ref;
        }
        __syncthreads();  // this step's LDS reads before the next stage
    }
}

// Step 2.
__global__ __launch_bounds__(kPackThreads) void k_cfm_join(CfmArgs a)
{
    const JoinTable t = join_table(a);
    if (blockIdx.x < a.nblocks) {
        const uint64_t lo = (uint64_t)blockIdx.x * a.per_block;
        const uint64_t hi = min(lo + a.per_block, a.n_records);
        for (uint64_t r = lo + threadIdx.x; r < hi; r += kPackThreads) {
            const uint8_t kind = a.kind[r];
            if (kind == kCfmConfirm) {
                const uint32_t m = join_find(
                    t, join_key(a.journal + (uint64_t)kJournalRecordDwords * r, kCfmGuidDword));
                if (m) {
                    atomicAdd(&a.had[m - 1u], 1u);
                }
            } else if (kind == kCfmDeletion) {
                const uint32_t m =
                    join_find(t, join_key_deletion(a.journal + (uint64_t)kJournalRecordDwords * r));
                if (m) {
                    a.dead[m - 1u] = 1;  // whoever stores, stores 1
                }
            }
        }
    }
    if (blockIdx.x < a.cnblocks) {
        const uint64_t lo = (uint64_t)blockIdx.x * a.cper_block;
        const uint64_t hi = min(lo + a.cper_block, a.n);
        for (uint64_t i = lo + threadIdx.x; i < hi; i += kPackThreads) {
            const JoinKey k = join_key_bytes(a.guids + 16 * i, a.queue_keys + 5 * i);
            uint32_t hit = kCfmNone;
            if ((k.g[0] | k.g[1] | k.g[2] | k.g[3]) == 0 || (k.q0 | k.q1) == 0) {
                refuse(a, BMQCRC_CFM_KIND_NULL_KEY, i);
            } else {
                const uint32_t m = join_find(t, k);
                if (m) {
                    hit = m - 1u;
                    atomicAdd(&a.cnt[hit], 1u);
                    atomicMax(&a.last[hit], (uint32_t)i + 1u);
                }
            }
            if (a.reasons && a.reasons[i] > 1) {
                refuse(a, BMQCRC_CFM_KIND_REASON, i);
            }
            a.hit[i] = hit;
        }
    }
}

// left(m) of a selected MESSAGE record that no DELETION record names.
__device__ __forceinline__ uint32_t left_of(const CfmArgs& a, uint32_t m)
{
    const uint32_t ref = a.ref[m], had = a.had[m];
    return ref > had ? ref - had : 0u;
}

// target(i): the live MESSAGE record confirm i names, or kCfmNone.
__device__ __forceinline__ uint32_t target_of(const CfmArgs& a, uint64_t i)
{
    const uint32_t m = a.hit[i];
    return m != kCfmNone && !a.dead[m] ? m : kCfmNone;
}

// The confirms as messages (LayoutView): the pass reads a source offset and a
// length of every entry, of which this call has neither -- it is handed off and
// hit, n entries each, and the pieces it counts from them are not used.
__device__ __forceinline__ LayoutView confirms_view(const CfmArgs& a)
{
    return {a.off, a.hit, a.n, a.off, a.bsum, a.ctr, a.cper_block, a.cnblocks};
}

// Step 3.
__global__ __launch_bounds__(kPackThreads) void k_cfm_check(CfmArgs a)
{
    layout_count(confirms_view(a), [&a](uint64_t i, uint64_t, uint32_t) {
        const uint32_t m = target_of(a, i);
        if (m == kCfmNone) {
            return 0ull;
        }
        if (a.cnt[m] > left_of(a, m)) {
            refuse(a, BMQCRC_CFM_KIND_OVER_CONFIRMED, i);
        }
        return 1ull;
    });
}

// Is confirm i, whose target is m, the one that writes m's DELETION record?
__device__ __forceinline__ bool deletes(const CfmArgs& a, uint64_t i, uint32_t m)
{
    return a.last[m] == (uint32_t)i + 1u && a.cnt[m] == left_of(a, m);
}

// Step 4.
__global__ __launch_bounds__(kPackThreads) void k_cfm_seal(CfmArgs a)
{
    __shared__ unsigned long long bpre[kPackBlocks + 1];
    block_prefix(confirms_view(a), bpre);
    const unsigned long long before = bpre[blockIdx.x];
    const uint64_t lo = (uint64_t)blockIdx.x * a.cper_block;
    const uint64_t hi = min(lo + a.cper_block, a.n);
    unsigned long long deletions = 0, not_found = 0;
    for (uint64_t i = lo + threadIdx.x; i < hi; i += kPackThreads) {
        const uint32_t m = target_of(a, i);
        if (m == kCfmNone) {
            a.off[i] = ~0ull;
            ++not_found;
            continue;
        }
        const unsigned long long j = a.off[i] + before;
        a.off[i] = j;
        if (!a.size_only &&
            (unsigned long long)(4 * kJournalRecordDwords) * (j + 1) > a.journal_dst_bytes) {
            refuse(a, BMQCRC_CFM_KIND_DST_TOO_SMALL, i);
        }
        deletions += deletes(a, i, m) ? 1u : 0u;
    }
    deletions = wave_sum(deletions);
    not_found = wave_sum(not_found);
    if ((threadIdx.x & 63u) == 0) {
        if (deletions) {
            atomicAdd(&a.ctr[kCfmCtrDeletions], deletions);
        }
        if (not_found) {
            atomicAdd(&a.ctr[kCfmCtrNotFound], not_found);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.ctr[kCfmCtrWritten] = bpre[a.cnblocks];
    }
}

// Step 5.  The word is final: on a refusal the host reads kind and index from
// it, and the kernel leaves.
__global__ __launch_bounds__(kPackFrameThreads) void k_cfm_frame(CfmArgs a)
{
    if (a.ctr[kCfmCtrRefusal] != 0) {
        return;
    }
    const uint64_t stride = (uint64_t)gridDim.x * kPackFrameThreads;
    const uint64_t t0 = (uint64_t)blockIdx.x * kPackFrameThreads + threadIdx.x;
    // Thread t of the grid owns dword t % 15 of confirm t / 15's record (n <
    // 2^32: a dword's index needs 36 bits); the division in 32 bits whenever
    // the call's indices fit.
    const uint64_t ndw = (uint64_t)kJournalRecordDwords * a.n;
    const bool narrow = ndw <= 0xFFFFFFFFull;
    for (uint64_t t = t0; t < ndw; t += stride) {
        const uint64_t i = narrow ? (uint32_t)t / kJournalRecordDwords : t / kJournalRecordDwords;
        const uint32_t j = (uint32_t)(t - kJournalRecordDwords * i);
        const unsigned long long at = a.off[i];
        if (at == ~0ull) {
            continue;
        }
        const bool del = deletes(a, i, a.hit[i]);
        uint32_t v;
        if (j < 5) {
            const uint64_t seq = a.first_seq + at;
            const uint64_t ts = a.timestamps ? a.timestamps[i] : a.timestamp;
            const uint32_t reason = !del && a.reasons ? a.reasons[i] : 0u;
            v = j == 0   ? ((del ? kRecDeletion : kRecConfirm) << 28) | (reason << 16) |
                             (uint32_t)(seq >> 32)
                : j == 1 ? (uint32_t)seq
                : j == 2 ? a.lease_id
                : j == 3 ? (uint32_t)(ts >> 32)
                         : (uint32_t)ts;
            v = __builtin_bswap32(v);
        } else if (j == 14) {
            v = kMagicLE;
        } else {
            // bytes 20..55: the queue key, a CONFIRM record's app key, the GUID
            const uint32_t qo = del ? 23u : 22u, go = del ? 28u : 32u;
            v = 0;
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t p = 4 * j + k;
                uint32_t b = 0;
                if (p >= qo && p < qo + 5) {
                    b = a.queue_keys[5 * i + (p - qo)];
                } else if (!del && a.app_keys && p >= 27 && p < 32) {
                    b = a.app_keys[5 * i + (p - 27)];
                } else if (p >= go && p < go + 16) {
                    b = a.guids[16 * i + (p - go)];
                }
                v |= b << (8 * k);
            }
        }
        a.journal_dst[kJournalRecordDwords * at + j] = v;
    }
    for (uint64_t i = t0; i < a.n; i += stride) {
        const uint32_t m = target_of(a, i);
        if (a.status) {
            a.status[i] = m == kCfmNone ? 2 : deletes(a, i, m) ? 1 : 0;
        }
        if (a.target) {
            a.target[i] = m;
        }
        if (a.new_index) {
            a.new_index[i] = (uint32_t)a.off[i];  // ~0 without a target
        }
    }
    if (a.left_out) {
        for (uint64_t r = t0; r < a.n_records; r += stride) {
            // nothing was refused: c(m) <= left(m)
            a.left_out[r] = a.kind[r] == kCfmMessage && !a.dead[r]
                                ? left_of(a, (uint32_t)r) - a.cnt[r]
                                : 0u;
        }
    }
}

}  // namespace
}  // namespace bmqcrc

using namespace bmqcrc;

extern "C" int bmqcrc_launch_confirm_records_layout(const CfmArgs* a, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (a->nblocks) {
        hipLaunchKernelGGL(k_cfm_classify, dim3(a->nblocks), dim3(kPackThreads), 0, s, *a);
    }
    const uint32_t blocks = a->nblocks > a->cnblocks ? a->nblocks : a->cnblocks;
    hipLaunchKernelGGL(k_cfm_join, dim3(blocks), dim3(kPackThreads), 0, s, *a);
    hipLaunchKernelGGL(k_cfm_check, dim3(a->cnblocks), dim3(kPackThreads), 0, s, *a);
    hipLaunchKernelGGL(k_cfm_seal, dim3(a->cnblocks), dim3(kPackThreads), 0, s, *a);
    return hipGetLastError() != hipSuccess;
}

extern "C" int bmqcrc_launch_confirm_records_frame(const CfmArgs* a, void* stream)
{
    const uint64_t units = a->n > a->n_records / kJournalRecordDwords
                               ? a->n
                               : a->n_records / kJournalRecordDwords;
    const uint64_t work = (uint64_t)kJournalRecordDwords * units;
    const uint64_t want = (work + kPackFrameThreads - 1) / kPackFrameThreads;
    const uint32_t blocks = (uint32_t)(want > kPackFrameBlocks ? kPackFrameBlocks : want);
    hipLaunchKernelGGL(k_cfm_frame, dim3(blocks ? blocks : 1u), dim3(kPackFrameThreads), 0,
                       (hipStream_t)stream, *a);
    return hipGetLastError() != hipSuccess;
}
