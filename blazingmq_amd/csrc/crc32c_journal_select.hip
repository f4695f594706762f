// crc32c_journal_select.hip -- MI355X (gfx950) selection of recovery's MESSAGE
// records from a device-resident run of journal records (bmqcrc_journal_select,
// ABI 2.14).
//
// The device-side form of the two backward passes of walk_recovery
// (bmqcrc_protocol.cpp), which carry hash sets from record to record and
// return at the first failure.  Restated, nothing is carried: every table is
// a maximum over record indices, every rule asks only about records above the
// one it judges, and the failure is the failing record with the highest
// index, so each record is judged on its own and the order the blocks run in
// changes nothing.  A word that names a record holds record + 1, 0 meaning
// none: the zeroed workspace is the empty state and atomicMax the reduction.
// Six kernels on one stream behind one memset of the workspace:
//
//   1. k_jsel_scan (nblocks x kPackThreads, records staged through LDS as in
//      crc32c_journal_stage.h): stop, the highest record with type 0, lease id
//      0, sequence number 0 or a wrong magic -- the walk is the records above
//      it -- and the indices of the QueueOp and the JOURNAL_OP records, both
//      rare, appended to two lists a wave at a time.
//   2. k_jsel_queues (one block): over the QueueOp list and queue_keys.  The
//      keys go into an open-addressing table (one 64-bit atomicCAS publishes a
//      key); then, a block barrier between the phases, per key the highest
//      queue DELETION, the highest CREATION above it, and last the first
//      pass's failures, the highest whole-queue PURGE of a live queue and the
//      lowest sync point.  More distinct keys than queue_cap is the refusal.
//   3. k_jsel_build: per record of the walk the PSN checks against the record
//      above and the record's own checks; every eligible DELETION takes a slot
//      of its own in the GUID table (a multimap: one 32-bit atomicCAS from 0
//      stores record + 1, the GUID stays in the journal); every MESSAGE gets
//      its state.
//   4. k_jsel_claim: every eligible MESSAGE walks its GUID's chain to the
//      first empty slot, comparing GUIDs in the journal, for the lowest
//      DELETION above itself, and raises that DELETION's claim to its own
//      index.  A launch of its own: it never meets a half-built table.
//   5. k_jsel_resolve: a MESSAGE that holds the claim of the DELETION it named
//      is the one the reference's set would have removed: skipped.  The others
//      are selected, or fail when their queue is not live.
//   6. k_jsel_finish: select = 0 at and below max(stop, the failing record),
//      the three counts above it, first_record.
//
// No byte outside [journal, +60 n_records) and [queue_keys, +5 n_queue_keys)
// is loaded: records are read by an index below n_records only (r + 1 after
// r + 1 < n_records, a table's entry after it was stored from such an index).
// Every offset is 64 bits wide.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmqcrc_internal.h"
#include "crc32c_journal_stage.h"
#include "crc32c_pack_layout.h"

namespace bmqcrc {
namespace {

typedef unsigned long long u64;

// RecordType, QueueOpType (mqbs_filestoreprotocol.h)
constexpr uint32_t kMessage = 1, kConfirm = 2, kDeletion = 3, kQueueOp = 4, kJournalOp = 5;
constexpr uint32_t kOpPurge = 1, kOpCreation = 2, kOpDeletion = 3, kOpAddition = 4;
// -BMQCRC_RECOVERY_* (bmqcrc_protocol.h, which the kernels do not include)
constexpr uint32_t kLeaseId = 2, kSeqNumber = 3, kQueueOpRecord = 4, kNullQueueKey = 5,
                   kDuplicateQueueKey = 7, kQueueKey = 8, kDataOffset = 11, kSyncPtSubType = 12,
                   kDeletionRecord = 14, kConfirmRecord = 15, kMessageRecord = 16;
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
constexpr u64 kKeyTaken = 1ull << 63;

// A failure of record r: the highest record wins, and a record reports once.
__device__ __forceinline__ void fails(const JselArgs& a, int word, uint64_t r, uint32_t code)
{
    atomicMax(&a.ctr[word], (u64)(r + 1) << 8 | code);
}

// The 5-byte key at bytes 22..26 (QueueOp, MESSAGE, CONFIRM) or 23..27
// (DELETION) of a record, first byte lowest; 0 is the null key.
__device__ __forceinline__ u64 key_at22(const uint32_t* d)
{
    return (u64)((d[5] >> 16) | (d[6] << 16)) | (u64)((d[6] >> 16) & 0xFFu) << 32;
}

__device__ __forceinline__ u64 key_at23(const uint32_t* d)
{
    return (u64)((d[5] >> 24) | (d[6] << 8)) | (u64)(d[6] >> 24) << 32;
}

__device__ __forceinline__ uint64_t key_home(const JselArgs& a, u64 key)
{
    u64 h = key * 0x9E3779B97F4A7C15ull;
    h ^= h >> 29;
    return h & (a.qslots - 1);
}

// The key's slot, or kNoSlot: plain loads, for the kernels after k_jsel_queues.
__device__ __forceinline__ uint32_t key_find(const JselArgs& a, u64 key)
{
    uint64_t s = key_home(a, key);
    for (uint64_t i = 0; i < a.qslots; ++i, s = (s + 1) & (a.qslots - 1)) {
        const u64 v = a.qkey[s];
        if (v == (key | kKeyTaken)) {
            return (uint32_t)s;
        }
        if (v == 0) {
            break;
        }
    }
    return kNoSlot;
}

// All 16 bytes mixed: real GUIDs are counters and timestamps.
__device__ __forceinline__ uint64_t guid_home(const JselArgs& a, uint32_t g0, uint32_t g1,
                                              uint32_t g2, uint32_t g3)
{
    u64 h = ((u64)g1 << 32 | g0) * 0x9E3779B97F4A7C15ull;
    h ^= h >> 32;
    h += ((u64)g3 << 32 | g2) * 0xD6E8FEB86659FD93ull;
    h ^= h >> 32;
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 29;
    return h & (a.gslots - 1);
}

struct Header {
    uint32_t type, lease;
    u64 seq;
};

__device__ __forceinline__ Header header_of(uint32_t d0, uint32_t d1, uint32_t d2)
{
    const uint32_t w0 = __builtin_bswap32(d0);  // type | flags | sequence number's top
    return Header{w0 >> 28, __builtin_bswap32(d2), (u64)(w0 & 0xFFFFu) << 32 | __builtin_bswap32(d1)};
}

// Appends the records of the wave's lanes with `take` to list[], whose length
// is ctr[word]: one atomicAdd per wave.
__device__ __forceinline__ void append(const JselArgs& a, int word, uint32_t* list, bool take,
                                       uint64_t r, uint32_t lane)
{
    const u64 mask = __ballot(take);
    if (mask == 0) {
        return;
    }
    const int leader = __ffsll((long long)mask) - 1;
    u64 base = 0;
    if ((int)lane == leader) {
        base = atomicAdd(&a.ctr[word], (u64)__popcll(mask));
    }
    base = __shfl(base, leader);
    if (take) {
        list[base + __popcll(mask & ((1ull << lane) - 1ull))] = (uint32_t)r;
    }
}

// Step 1.
__global__ __launch_bounds__(kPackThreads) void k_jsel_scan(JselArgs a)
{
    __shared__ uint32_t recs[kWaves * kWaveDwords];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint64_t lo = (uint64_t)blockIdx.x * a.per_block;
    const uint64_t hi = min(lo + a.per_block, a.n_records);
    uint32_t* mine = recs + wv * kWaveDwords;
    const uint32_t* d = mine + kJournalRecordDwords * lane;
    u64 stop = 0;
    for (uint64_t base = lo; base < hi; base += kPackThreads) {
        stage(a.journal, base + 64u * wv, hi, mine, lane);
        __syncthreads();
        const uint64_t r = base + tid;
        uint32_t type = 0;
        if (r < hi) {
            const Header h = header_of(d[0], d[1], d[2]);
            type = h.type;
            if (h.type == 0 || h.lease == 0 || h.seq == 0 || d[14] != kMagicLE) {
                stop = r + 1;  // (r only grows)
                type = 0;
            }
        }
        append(a, kJselCtrQueueOps, a.qlist, type == kQueueOp, r, lane);
        append(a, kJselCtrSyncs, a.slist, type == kJournalOp, r, lane);
        __syncthreads();  // this step's LDS reads before the next stage
    }
    if (stop) {
        atomicMax(&a.ctr[kJselCtrStop], stop);
    }
}

// A load that no earlier load of this block can have left stale in the CU's L1
// (k_jsel_queues reads what its own atomics wrote a phase before).
template <class T>
__device__ __forceinline__ T fresh(const T* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The slot of `key`, published if new; kNoSlot (and the refusal) when the
// table is full.  A key past queue_cap raises the refusal too.
__device__ __forceinline__ uint32_t key_publish(const JselArgs& a, u64 key)
{
    uint64_t s = key_home(a, key);
    for (uint64_t i = 0; i < a.qslots; ++i, s = (s + 1) & (a.qslots - 1)) {
        const u64 old = atomicCAS(&a.qkey[s], 0ull, key | kKeyTaken);
        if (old == 0 && atomicAdd(&a.ctr[kJselCtrKeys], 1ull) >= a.queue_cap) {
            atomicMax(&a.ctr[kJselCtrRefused], 1ull);
        }
        if (old == 0 || old == (key | kKeyTaken)) {
            return (uint32_t)s;
        }
    }
    atomicMax(&a.ctr[kJselCtrRefused], 1ull);
    return kNoSlot;
}

// Step 2.  One block.
__global__ __launch_bounds__(kPackThreads) void k_jsel_queues(JselArgs a)
{
    __shared__ uint32_t first_sync;
    const uint32_t tid = threadIdx.x;
    const u64 stop = a.ctr[kJselCtrStop];
    const u64 nq = a.ctr[kJselCtrQueueOps], ns = a.ctr[kJselCtrSyncs];
    if (tid == 0) {
        first_sync = kNoSlot;
    }
    __syncthreads();
    // the keys; the lowest sync point of the walk
    for (u64 i = tid; i < ns; i += kPackThreads) {
        const uint32_t r = a.slist[i];
        if (r >= stop) {
            atomicMin(&first_sync, r);
        }
    }
    if (a.with_csl) {
        for (u64 i = tid; i < a.n_queue_keys; i += kPackThreads) {
            const uint8_t* k = a.queue_keys + 5 * i;
            const u64 key = (u64)k[0] | (u64)k[1] << 8 | (u64)k[2] << 16 | (u64)k[3] << 24 |
                            (u64)k[4] << 32;
            const uint32_t s = key_publish(a, key);
            if (s != kNoSlot) {
                atomicMax(&a.qcsl[s], 1u);
            }
        }
    }
    for (u64 i = tid; i < nq; i += kPackThreads) {
        const uint32_t r = a.qlist[i];
        const u64 key = key_at22(a.journal + (uint64_t)kJournalRecordDwords * r);
        if (r >= stop && key != 0) {
            key_publish(a, key);
        }
    }
    __syncthreads();
    if (tid == 0) {
        a.ctr[kJselCtrFirstSync] = first_sync == kNoSlot ? 0 : first_sync;
    }
    if (fresh(&a.ctr[kJselCtrRefused])) {
        return;  // (the whole block)
    }
    // per key the highest queue DELETION, then the highest CREATION above it,
    // then the failures and the highest PURGE
    for (int phase = 0; phase < 3; ++phase) {
        for (u64 i = tid; i < nq; i += kPackThreads) {
            const uint32_t r = a.qlist[i];
            if (r < stop) {
                continue;
            }
            const uint32_t* d = a.journal + (uint64_t)kJournalRecordDwords * r;
            const u64 key = key_at22(d);
            const bool whole = (d[6] >> 24) == 0 && d[7] == 0;  // null app key @27..31
            const uint32_t op = __builtin_bswap32(d[8]);
            // a key the table holds: published above
            const uint32_t s = key ? key_publish(a, key) : kNoSlot;
            if (phase == 0) {
                if (key && op == kOpDeletion && whole) {
                    atomicMax(&a.qdel[s], r + 1);
                }
                continue;
            }
            const bool above_del = key && r + 1 > fresh(&a.qdel[s]);
            if (phase == 1) {
                if (op == kOpCreation && above_del) {
                    atomicMax(&a.qtop[s], r + 1);
                }
                continue;
            }
            const bool known = key && fresh(&a.qcsl[s]) != 0;
            const uint32_t top = key ? fresh(&a.qtop[s]) : 0;
            uint32_t code = 0;
            if (op == 0) {
                code = kQueueOpRecord;
            } else if (key == 0) {
                code = kNullQueueKey;
            } else if (op == kOpDeletion) {
                code = a.with_csl && whole && known ? kDeletionRecord : 0;
            } else if ((op == kOpCreation || op == kOpAddition) && above_del) {
                code = a.with_csl ? (known ? 0 : kQueueKey) : (r + 1 < top ? kDuplicateQueueKey : 0);
            }
            if (code) {
                fails(a, kJselCtrFail1, r, code);
            }
            if (op == kOpPurge && whole && above_del && (a.with_csl ? known : top != 0)) {
                atomicMax(&a.qpurge[s], r + 1);
            }
        }
        __syncthreads();
    }
}

// The call stops short: refused, or failed in the first pass.
__device__ __forceinline__ bool nothing_selected(const JselArgs& a)
{
    return a.ctr[kJselCtrRefused] != 0 || a.ctr[kJselCtrFail1] != 0;
}

// Step 3.
__global__ __launch_bounds__(kPackThreads) void k_jsel_build(JselArgs a)
{
    __shared__ uint32_t recs[kWaves * kWaveDwords];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint64_t lo = (uint64_t)blockIdx.x * a.per_block;
    const uint64_t hi = min(lo + a.per_block, a.n_records);
    const bool bail = nothing_selected(a);
    const u64 stop = a.ctr[kJselCtrStop], first_sync = a.ctr[kJselCtrFirstSync];
    uint32_t* mine = recs + wv * kWaveDwords;
    const uint32_t* d = mine + kJournalRecordDwords * lane;
    for (uint64_t base = lo; base < hi; base += kPackThreads) {
        if (bail) {
            if (base + tid < hi) {
                a.state[base + tid] = kJselNone;
            }
            continue;
        }
        stage(a.journal, base + 64u * wv, hi, mine, lane);
        __syncthreads();
        const uint64_t r = base + tid;
        if (r < hi) {
            uint8_t state = kJselNone;
            uint32_t code = 0;
            if (r >= stop) {
                const Header h = header_of(d[0], d[1], d[2]);
                // the record above, which is in the walk too; the write head for the last
                Header up{0, h.lease, h.seq + 1};
                if (r + 1 < a.n_records) {
                    const uint32_t* u = a.journal + kJournalRecordDwords * (r + 1);
                    up = header_of(u[0], u[1], u[2]);
                }
                if (h.lease > up.lease) {
                    code = kLeaseId;
                } else if (h.lease == up.lease &&
                           (r >= first_sync ? h.seq != up.seq - 1 : h.seq > up.seq - 1)) {
                    code = kSeqNumber;
                } else if (h.type == kJournalOp) {
                    const u64 sp_seq = (u64)__builtin_bswap32(d[7]) << 32 | __builtin_bswap32(d[8]);
                    const uint32_t sp_lease = __builtin_bswap32(d[10]);
                    const u64 o = (u64)__builtin_bswap32(d[11]) * 8;
                    code = (d[5] >> 24) == 0                       ? kSyncPtSubType  // @23
                           : o == 0 || o > a.data_file_bytes       ? kDataOffset
                           : sp_lease == 0                         ? kLeaseId
                           : sp_seq == 0                           ? kSeqNumber
                           : sp_lease > h.lease                    ? kLeaseId
                           : sp_lease == h.lease && sp_seq != h.seq ? kSeqNumber
                                                                    : 0;
                } else if (h.type == kQueueOp) {
                    const uint32_t s = key_find(a, key_at22(d));
                    const bool below_del = s != kNoSlot && r + 1 < a.qdel[s];
                    if (!below_del && __builtin_bswap32(d[8]) == kOpAddition && !a.with_csl &&
                        !(s != kNoSlot && a.qtop[s])) {
                        code = kQueueKey;
                    }
                } else if (h.type == kConfirm) {  // GUID @32..47
                    if ((d[8] | d[9] | d[10] | d[11]) == 0 || key_at22(d) == 0) {
                        code = kConfirmRecord;
                    }
                } else if (h.type == kDeletion || h.type == kMessage) {
                    const bool del = h.type == kDeletion;
                    const uint32_t* g = d + (del ? 7 : 9);  // GUID @28..43, @36..51
                    const u64 key = del ? key_at23(d) : key_at22(d);
                    const u64 o = (u64)__builtin_bswap32(d[8]) * 8;  // MessageOffsetDwords
                    if ((g[0] | g[1] | g[2] | g[3]) == 0 || key == 0) {
                        code = del ? kDeletionRecord : kMessageRecord;
                    } else if (!del && (o == 0 || o > a.data_file_bytes)) {
                        code = kDataOffset;
                    } else {
                        const uint32_t s = key_find(a, key);
                        const bool eligible =
                            s == kNoSlot || (r + 1 >= a.qdel[s] && r + 1 >= a.qpurge[s]);
                        if (!del) {
                            const bool live = s != kNoSlot && (a.with_csl ? a.qcsl[s] : a.qtop[s]);
                            state = !eligible ? kJselPurged : live ? kJselLive : kJselDead;
                        } else if (eligible) {
                            // (the table holds 2 n_records slots at least: one is free)
                            uint64_t at = guid_home(a, g[0], g[1], g[2], g[3]);
                            for (uint64_t i = 0; i < a.gslots; ++i, at = (at + 1) & (a.gslots - 1)) {
                                if (atomicCAS(&a.gslot[at], 0u, (uint32_t)r + 1) == 0) {
                                    break;
                                }
                            }
                        }
                    }
                }
                if (code) {
                    fails(a, kJselCtrFail2, r, code);
                }
            }
            a.state[r] = state;
        }
        __syncthreads();  // this step's LDS reads before the next stage
    }
}

// Step 4.
__global__ __launch_bounds__(kPackThreads) void k_jsel_claim(JselArgs a)
{
    const uint64_t lo = (uint64_t)blockIdx.x * a.per_block;
    const uint64_t hi = min(lo + a.per_block, a.n_records);
    for (uint64_t r = lo + threadIdx.x; r < hi; r += kPackThreads) {
        const uint8_t state = a.state[r];
        if (state != kJselLive && state != kJselDead) {
            continue;
        }
        const uint32_t* g = a.journal + kJournalRecordDwords * r + 9;
        const uint32_t g0 = g[0], g1 = g[1], g2 = g[2], g3 = g[3];
        uint32_t lowest = 0;  // record + 1 of the lowest DELETION of this GUID above r
        uint64_t at = guid_home(a, g0, g1, g2, g3);
        for (uint64_t i = 0; i < a.gslots; ++i, at = (at + 1) & (a.gslots - 1)) {
            const uint32_t v = a.gslot[at];
            if (v == 0) {
                break;
            }
            if (v - 1 > r && (lowest == 0 || v < lowest)) {
                const uint32_t* e = a.journal + (uint64_t)kJournalRecordDwords * (v - 1) + 7;
                if (e[0] == g0 && e[1] == g1 && e[2] == g2 && e[3] == g3) {
                    lowest = v;
                }
            }
        }
        a.names[r] = lowest;
        if (lowest) {
            atomicMax(&a.claim[lowest - 1], (uint32_t)r + 1);
        }
    }
}

// Step 5.
__global__ __launch_bounds__(kPackThreads) void k_jsel_resolve(JselArgs a)
{
    const uint64_t lo = (uint64_t)blockIdx.x * a.per_block;
    const uint64_t hi = min(lo + a.per_block, a.n_records);
    for (uint64_t r = lo + threadIdx.x; r < hi; r += kPackThreads) {
        uint8_t state = a.state[r];
        if (state == kJselLive || state == kJselDead) {
            const uint32_t named = a.names[r];
            if (named && a.claim[named - 1] == (uint32_t)r + 1) {
                state = kJselDeleted;
            } else if (state == kJselDead) {
                fails(a, kJselCtrFail2, r, kQueueKey);
                state = kJselNone;
            }
            a.state[r] = state;
        }
        a.select[r] = state == kJselLive;
    }
}

// Step 6.
__global__ __launch_bounds__(kPackThreads) void k_jsel_finish(JselArgs a)
{
    __shared__ u64 total[3];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t lo = (uint64_t)blockIdx.x * a.per_block;
    const uint64_t hi = min(lo + a.per_block, a.n_records);
    const u64 first = nothing_selected(a)
                          ? a.n_records
                          : max(a.ctr[kJselCtrStop], a.ctr[kJselCtrFail2] >> 8);
    u64 selected = 0, deleted = 0, purged = 0;
    for (uint64_t r = lo + threadIdx.x; r < hi; r += kPackThreads) {
        if (r < first) {
            a.select[r] = 0;
            continue;
        }
        const uint8_t state = a.state[r];
        selected += state == kJselLive;
        deleted += state == kJselDeleted;
        purged += state == kJselPurged;
    }
    // one atomic per block and count: thousands of waves adding to one line
    // took longer than the pass itself
    selected = wave_sum(selected);
    deleted = wave_sum(deleted);
    purged = wave_sum(purged);
    if (threadIdx.x < 3) {
        total[threadIdx.x] = 0;
    }
    __syncthreads();
    if (lane == 0) {
        atomicAdd(&total[0], selected);
        atomicAdd(&total[1], deleted);
        atomicAdd(&total[2], purged);
    }
    __syncthreads();
    if (threadIdx.x < 3 && total[threadIdx.x]) {
        atomicAdd(&a.ctr[kJselCtrSelected + threadIdx.x], total[threadIdx.x]);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.ctr[kJselCtrFirst] = first;
    }
}

static_assert(kJselCtrDeleted == kJselCtrSelected + 1 && kJselCtrPurged == kJselCtrSelected + 2,
              "k_jsel_finish: the three counts are adjacent words");

}  // namespace
}  // namespace bmqcrc

using namespace bmqcrc;

extern "C" int bmqcrc_launch_journal_select(const JselArgs* a, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(a->nblocks), block(kPackThreads);
    hipLaunchKernelGGL(k_jsel_scan, grid, block, 0, s, *a);
    hipLaunchKernelGGL(k_jsel_queues, dim3(1), block, 0, s, *a);
    hipLaunchKernelGGL(k_jsel_build, grid, block, 0, s, *a);
    hipLaunchKernelGGL(k_jsel_claim, grid, block, 0, s, *a);
    hipLaunchKernelGGL(k_jsel_resolve, grid, block, 0, s, *a);
    hipLaunchKernelGGL(k_jsel_finish, grid, block, 0, s, *a);
    return hipGetLastError() != hipSuccess;
}
