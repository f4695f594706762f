// crc32c_pending_list.hip -- MI355X (gfx950): which messages of a
// device-resident partition each consumer still has to see, as the lists
// bmqcrc_push_event_pack takes (bmqcrc_pending_records_list, ABI 2.21;
// DESIGN.md section 23).
//
// The device-side form of mqbi::Storage::getIterator(appKey) over the state
// FileBackedStorage::processMessageRecord / processConfirmRecord /
// processDeletionRecord rebuild.  There is no CRC in this call: no payload
// byte is read.  Nothing persists between calls: the journal is the state.
// With key = (GUID, queue key), for a selected MESSAGE record m of the run:
// live(m) when no DELETION record of the run has its key, queue(m) the table
// entry with its queue key, confirmed(m, a) when a is an app of queue(m) with a
// non-null app key and some CONFIRM record of the run has m's key and a's app
// key, pending(m, a) when m is live, a is an app of queue(m), not
// confirmed(m, a) and m >= from_record[a].  list(a) is a's pending records in
// journal order.  Every one of these is a reduction that needs no order, and
// the grouping by app is a stable sort.  On one stream:
//
//   1. k_pnd_classify: the grid's first nblocks blocks over contiguous record
//      ranges (layout_split), one record per thread and step, staged through LDS
//      a wave's 64 records at a time (crc32c_journal_stage.h).  The RecordHeader
//      of EVERY record; every selected MESSAGE record into the hash
//      (crc32c_join_key.h), where one that meets its own key raises
//      DUPLICATE_MESSAGE with the lower record of the two.  All blocks, strided:
//      a table entry into the queue hash (QUEUE_KEY as in the expire call), its
//      app_first range (APP_FIRST) and, once that range is known to lie in
//      [0, n_apps] and to hold at most 32 apps, its app keys against one another
//      (APP_KEY, the lower app of a pair); an app's from_record (FROM_RECORD).
//   2. k_pnd_join: both hashes are whole and every refusal but the last kind is
//      known.  A DELETION record raises dead of its message; a MESSAGE record
//      finds its queue; a CONFIRM record finds its message and its queue, scans
//      the queue's at most 32 app keys and ORs bit `ordinal` into confirmed of
//      the message.  (atomicOr and a store of 1: whoever comes first, the word
//      ends the same.)
//   3. k_pnd_mask: dead and confirmed are whole.  The record's pending_mask;
//      pass 1 of crc32c_pack_layout.h over its popcount; the live counts.
//   4. k_pnd_total: the block sums' total, the pairs of the call -- the one word
//      the host reads, to size what follows.  2^32 pairs or more are refused.
//   5. k_pnd_emit: the block prefix; record m stores a pair (app, m) for every
//      set bit at its prefix position: pairs in journal order, inside a record
//      in ordinal order.
//   6. the grouping, a stable LSD radix sort of the pairs by app over only as
//      many 8-bit digits as n_apps - 1 has.  A pass is k_pnd_hist (a block's
//      digit counts over its contiguous pair range, in LDS), k_pnd_scan (the
//      digit-major 256 x blocks matrix scanned row by row, a block a digit, with
//      the rows' totals, which every scatter block scans for itself) and
//      k_pnd_scatter: a lane's rank among its wave's equal digits is eight
//      ballots and a popcount below the lane, the waves of a block are ordered
//      through per-wave LDS counts, the tiles of a block through a running base.
//      No atomic decides a position, so equal apps keep journal order.
//   7. k_pnd_bounds: per app two lower bounds on the sorted apps give
//      first_pending(a) and |list(a)| (empty apps too); pass 1 over
//      listed(a) = min(|list(a)|, limit[a]).
//   8. k_pnd_check: the block prefix makes list_first; every app's end against
//      list_cap (LIST_TOO_SMALL, the lowest app); the listed total.
//   9. k_pnd_frame (not when size-only): unless refused, sorted pair i of app a
//      has rank r = i - first_pending(a); r < limit[a] stores the three lists at
//      list_first[a] + r, r == limit[a] stores app_next[a]; the per-app and
//      per-record arrays.
//
// No byte outside [journal, +60 n_records), select's n_records bytes and the
// table's arrays at their stated lengths is loaded.  Every probe loop is
// bounded by its table's slots.  The journal is read by a record index below
// n_records only (the hash and the pairs hold such indices), the table by an
// entry below n_queues and an app below n_apps only.  An index taken from the
// caller's app_first is used only after step 1 has shown it in range: step 1
// itself reads app keys only of a range it has just bounded, every later kernel
// returns at once when the refusal word is set (the host launches 5 to 9 only
// after it has read a clean word), so a refused table is never walked -- and
// the app scan is bounded by 32 and by n_apps whatever the table says.  No pair
// is stored at or past n_pairs, what the host sized the workspace for from step
// 4's total, and nothing to an output at or past its stated length.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmqcrc_internal.h"
#include "crc32c_join_key.h"
#include "crc32c_journal_stage.h"
#include "crc32c_pack_layout.h"

namespace bmqcrc {
namespace {

__device__ __forceinline__ JoinTable join_table(const PndArgs& a)
{
    return {a.gslot, a.gslots, a.journal};
}

__device__ __forceinline__ QueueTable queue_table(const PndArgs& a)
{
    return {a.qslot, a.qslots, a.queue_keys};
}

// An app key's five bytes as two words: the first byte, and the other four as
// they lie in memory.  Of a CONFIRM record's dwords (bytes 27..31) ...
struct AppKey {
    uint32_t k0, k1;
};

__device__ __forceinline__ AppKey app_key_confirm(const uint32_t* d)
{
    return {d[6] >> 24, d[7]};
}

// ... and of app e of the table, at any alignment.
__device__ __forceinline__ AppKey app_key_of(const PndArgs& a, uint64_t e)
{
    const uint8_t* p = a.app_keys + 5 * e;
    return {p[0], (uint32_t)p[1] | ((uint32_t)p[2] << 8) | ((uint32_t)p[3] << 16) |
                      ((uint32_t)p[4] << 24)};
}

// The apps [*lo, *lo + return value) of entry q < n_queues: empty unless the
// range lies in [0, n_apps] and holds at most kPndMaxApps.
__device__ __forceinline__ uint32_t apps_of(const PndArgs& a, uint64_t q, uint64_t* lo)
{
    const uint64_t f = a.app_first[q], g = a.app_first[q + 1];
    *lo = f;
    return f <= g && g <= a.n_apps && g - f <= kPndMaxApps ? (uint32_t)(g - f) : 0u;
}

// Step 1.
__global__ __launch_bounds__(kPackThreads) void k_pnd_classify(PndArgs a)
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
                uint8_t kind = kPndOther;
                if (!record_header_ok(w0, d[1], d[2], d[14], kRecJournalOp)) {
                    refuse(a, BMQCRC_PND_KIND_RECORD_HEADER, r);
                } else if (type == kRecQueueOp) {
                    const uint32_t op = __builtin_bswap32(d[8]);  // QueueOpType: PURGE 1 .. ADDITION 4
                    if (op < 1 || op > 4) {
                        refuse(a, BMQCRC_PND_KIND_RECORD_HEADER, r);
                    }
                } else if (type == kRecMessage) {
                    if (a.select ? a.select[r] != 0 : true) {
                        kind = kPndMessage;
                        const uint32_t met =
                            join_insert(join_table(a), join_key(d, kMsgGuidDword), r);
                        if (met) {
                            refuse(a, BMQCRC_PND_KIND_DUPLICATE_MESSAGE,
                                   min(r, (uint64_t)(met - 1u)));
                        }
                    }
                } else if (type == kRecDeletion) {
                    kind = kPndDeletion;
                } else if (type == kRecConfirm) {
                    kind = kPndConfirm;
                }
                a.kind[r] = kind;
            }
            __syncthreads();  // this step's LDS reads before the next stage
        }
    }
    const uint64_t stride = (uint64_t)gridDim.x * kPackThreads;
    const uint64_t t0 = (uint64_t)blockIdx.x * kPackThreads + tid;
    const QueueTable qt = queue_table(a);
    for (uint64_t e = t0; e <= a.n_queues; e += stride) {
        const uint64_t f = a.app_first[e];
        if (e == a.n_queues) {
            if (f != a.n_apps) {
                refuse(a, BMQCRC_PND_KIND_APP_FIRST, e);
            }
            if (e == 0 && f != 0) {
                refuse(a, BMQCRC_PND_KIND_APP_FIRST, 0);
            }
            continue;
        }
        const JoinKey k = table_key_of(qt, e);
        if ((k.q0 | k.q1) == 0) {
            refuse(a, BMQCRC_PND_KIND_QUEUE_KEY, e);
        } else {
            const uint32_t met = table_insert(qt, k, e);
            if (met) {
                refuse(a, BMQCRC_PND_KIND_QUEUE_KEY, min(e, (uint64_t)(met - 1u)));
            }
        }
        const uint64_t g = a.app_first[e + 1];
        if ((e == 0 && f != 0) || f > g || g - f > kPndMaxApps) {
            refuse(a, BMQCRC_PND_KIND_APP_FIRST, e);
        }
        uint64_t lo;
        const uint32_t cnt = apps_of(a, e, &lo);
        for (uint32_t i = 1; i < cnt; ++i) {
            const AppKey x = app_key_of(a, lo + i);
            for (uint32_t j = 0; j < i; ++j) {
                const AppKey y = app_key_of(a, lo + j);
                if (x.k0 == y.k0 && x.k1 == y.k1) {
                    refuse(a, BMQCRC_PND_KIND_APP_KEY, lo + j);
                    break;  // (the lowest j of this i; a lower one of another i raises its own)
                }
            }
        }
    }
    if (a.from_record) {
        for (uint64_t e = t0; e < a.n_apps; e += stride) {
            if (a.from_record[e] > a.n_records) {
                refuse(a, BMQCRC_PND_KIND_FROM_RECORD, e);
            }
        }
    }
}

// Step 2.
__global__ __launch_bounds__(kPackThreads) void k_pnd_join(PndArgs a)
{
    if (a.ctr[kPndCtrRefusal] != 0) {
        return;
    }
    const JoinTable t = join_table(a);
    const QueueTable qt = queue_table(a);
    const uint64_t lo = (uint64_t)blockIdx.x * a.per_block;
    const uint64_t hi = min(lo + a.per_block, a.n_records);
    unsigned long long unknown = 0, not_found = 0;
    for (uint64_t r = lo + threadIdx.x; r < hi; r += kPackThreads) {
        const uint8_t kind = a.kind[r];
        const uint32_t* d = a.journal + (uint64_t)kJournalRecordDwords * r;
        if (kind == kPndDeletion) {
            const uint32_t m = join_find(t, join_key_deletion(d));
            if (m) {
                a.dead[m - 1u] = 1;  // whoever stores, stores 1
            }
        } else if (kind == kPndMessage) {
            // bytes 22..26, as join_key takes them
            a.queue[r] = table_find(qt, table_key(d[5] >> 16, d[6] & 0x00FFFFFFu)) - 1u;  // 0: kPndNone
        } else if (kind == kPndConfirm) {
            const JoinKey k = join_key(d, kCfmGuidDword);
            const uint32_t m = join_find(t, k);
            if (!m) {
                ++not_found;
                continue;
            }
            const AppKey x = app_key_confirm(d);
            if ((x.k0 | x.k1) == 0) {
                continue;  // the null key marks nothing
            }
            const uint32_t q = table_find(qt, table_key(k.q0, k.q1));
            uint32_t bit = 0;
            if (q) {
                uint64_t first;
                const uint32_t cnt = apps_of(a, q - 1u, &first);
                for (uint32_t o = 0; o < cnt; ++o) {
                    const AppKey y = app_key_of(a, first + o);
                    if (x.k0 == y.k0 && x.k1 == y.k1) {
                        bit = 1u << o;
                        break;  // (an app key stands once in a queue)
                    }
                }
            }
            if (bit) {
                atomicOr(&a.confirmed[m - 1u], bit);
            } else {
                ++unknown;
            }
        }
    }
    unknown = wave_sum(unknown);
    not_found = wave_sum(not_found);
    if ((threadIdx.x & 63u) == 0) {
        if (unknown) {
            atomicAdd(&a.ctr[kPndCtrUnknown], unknown);
        }
        if (not_found) {
            atomicAdd(&a.ctr[kPndCtrNotFound], not_found);
        }
    }
}

// The records as messages (LayoutView): the pass reads a source offset and a
// length of every entry, of which this call has neither -- it is handed off and
// queue, n_records entries each, and the pieces it counts from them are not
// used.  (Both loads stay inside the workspace but may read words nothing has
// written yet -- queue of a record that is no MESSAGE record, off before this
// very pass stores it: whatever they hold goes into the unused pieces only, as
// in crc32c_expire_records.hip.)
__device__ __forceinline__ LayoutView records_view(const PndArgs& a)
{
    return {a.off, a.queue, a.n_records, a.off, a.bsum, a.ctr, a.per_block, a.nblocks};
}

// ... and the apps likewise, over aoff and acount.
__device__ __forceinline__ LayoutView apps_view(const PndArgs& a)
{
    return {a.aoff, a.acount, a.n_apps, a.aoff, a.absum, a.ctr, a.aper_block, a.anblocks};
}

// Step 3.
__global__ __launch_bounds__(kPackThreads) void k_pnd_mask(PndArgs a)
{
    if (a.ctr[kPndCtrRefusal] != 0) {
        return;
    }
    unsigned long long live = 0, no_queue = 0;
    layout_count(records_view(a), [&](uint64_t r, uint64_t, uint32_t) {
        uint32_t mask = 0;
        if (a.kind[r] == kPndMessage && !a.dead[r]) {
            ++live;
            const uint32_t q = a.queue[r];
            if (q == kPndNone) {
                ++no_queue;
            } else {
                uint64_t first;
                const uint32_t cnt = apps_of(a, q, &first);
                mask = cnt == 32u ? 0xFFFFFFFFu : (1u << cnt) - 1u;
                mask &= ~a.confirmed[r];
                if (a.from_record) {
                    for (uint32_t o = 0; o < cnt; ++o) {
                        if (r < a.from_record[first + o]) {
                            mask &= ~(1u << o);
                        }
                    }
                }
            }
        }
        a.mask[r] = mask;
        return (unsigned long long)__popc(mask);
    });
    live = wave_sum(live);
    no_queue = wave_sum(no_queue);
    if ((threadIdx.x & 63u) == 0) {
        if (live) {
            atomicAdd(&a.ctr[kPndCtrLive], live);
        }
        if (no_queue) {
            atomicAdd(&a.ctr[kPndCtrNoQueue], no_queue);
        }
    }
}

// Step 4: one block.
__global__ __launch_bounds__(kPackThreads) void k_pnd_total(PndArgs a)
{
    __shared__ unsigned long long bpre[kPackBlocks + 1];
    if (a.ctr[kPndCtrRefusal] != 0) {
        return;
    }
    block_prefix(records_view(a), bpre);
    if (threadIdx.x == 0) {
        a.ctr[kPndCtrPending] = bpre[a.nblocks];
        if (bpre[a.nblocks] > 0xFFFFFFFFull) {
            refuse(a, BMQCRC_PND_KIND_LIST_TOO_SMALL, a.n_apps);
        }
    }
}

// Step 5.
__global__ __launch_bounds__(kPackThreads) void k_pnd_emit(PndArgs a)
{
    __shared__ unsigned long long bpre[kPackBlocks + 1];
    block_prefix(records_view(a), bpre);
    const unsigned long long before = bpre[blockIdx.x];
    const uint64_t lo = (uint64_t)blockIdx.x * a.per_block;
    const uint64_t hi = min(lo + a.per_block, a.n_records);
    for (uint64_t r = lo + threadIdx.x; r < hi; r += kPackThreads) {
        uint32_t mask = a.mask[r];
        if (!mask) {
            continue;
        }
        uint64_t first;
        apps_of(a, a.queue[r], &first);  // (a set bit: the record has a queue, below n_queues)
        unsigned long long at = a.off[r] + before;
        while (mask) {
            const uint32_t o = __ffs(mask) - 1;
            mask &= mask - 1;
            if (at < a.n_pairs) {
                a.key[0][at] = (uint32_t)(first + o);
                a.val[0][at] = (uint32_t)r;
            }
            ++at;
        }
    }
}

// Step 6, first leg: hist[d * snblocks + b] = the pairs of block b's range
// whose digit is d.
__global__ __launch_bounds__(kPackThreads) void k_pnd_hist(PndArgs a, uint32_t pass)
{
    __shared__ uint32_t lh[kPndDigits];
    const uint32_t tid = threadIdx.x;
    if (tid < kPndDigits) {
        lh[tid] = 0;
    }
    __syncthreads();
    const uint32_t* key = a.key[pass & 1u];
    const uint64_t lo = (uint64_t)blockIdx.x * a.sper_block;
    const uint64_t hi = min(lo + a.sper_block, a.n_pairs);
    for (uint64_t i = lo + tid; i < hi; i += kPackThreads) {
        atomicAdd(&lh[(key[i] >> (8u * pass)) & 0xFFu], 1u);  // counts: any order, one sum
    }
    __syncthreads();
    if (tid < kPndDigits) {
        a.hist[(uint64_t)tid * a.snblocks + blockIdx.x] = lh[tid];
    }
}

// Second leg, a block per digit: row d of the matrix becomes its own exclusive
// scan over the blocks, in place, and rowsum[d] the row's total (the pairs of
// the call whose digit is d).  hist[d * snblocks + b] plus the rows before d is
// then where block b's first pair of digit d goes; the scatter adds the rows.
static_assert(kPackBlocks <= kPndDigits, "k_pnd_scan: a row is one entry a thread");

__global__ __launch_bounds__(kPndDigits) void k_pnd_scan(PndArgs a)
{
    __shared__ uint32_t wsum[kPndDigits / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    uint32_t* row = a.hist + (uint64_t)blockIdx.x * a.snblocks;
    const uint32_t v = tid < a.snblocks ? row[tid] : 0u;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d);
        incl += lane >= (uint32_t)d ? o : 0u;
    }
    if (lane == 63) {
        wsum[wv] = incl;
    }
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < kPndDigits / 64; ++w) {
        before += w < wv ? wsum[w] : 0u;
        all += wsum[w];
    }
    if (tid < a.snblocks) {
        row[tid] = before + incl - v;
    }
    if (tid == 0) {
        a.rowsum[blockIdx.x] = all;
    }
}

// Third leg.  Pair i of the block's range goes to base[digit] + the equal
// digits before it in the range: those of earlier tiles (base moves on behind
// every tile), of earlier waves of its tile (wcount, turned into a prefix over
// the waves) and of lower lanes of its wave (the ballots).
__global__ __launch_bounds__(kPackThreads) void k_pnd_scatter(PndArgs a, uint32_t pass)
{
    __shared__ uint32_t base[kPndDigits];
    __shared__ uint32_t wcount[kWaves][kPndDigits];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint32_t* key = a.key[pass & 1u];
    const uint32_t* val = a.val[pass & 1u];
    uint32_t* key_to = a.key[(pass & 1u) ^ 1u];
    uint32_t* val_to = a.val[(pass & 1u) ^ 1u];
    __shared__ unsigned long long wtot[kWaves];
    unsigned long long all;
    const unsigned long long rows =
        tile_scan(tid < kPndDigits ? (unsigned long long)a.rowsum[tid] : 0ull, wtot, &all);
    if (tid < kPndDigits) {
        base[tid] = (uint32_t)rows + a.hist[(uint64_t)tid * a.snblocks + blockIdx.x];
    }
    for (uint32_t j = tid; j < kWaves * kPndDigits; j += kPackThreads) {
        (&wcount[0][0])[j] = 0;
    }
    __syncthreads();
    const uint64_t lo = (uint64_t)blockIdx.x * a.sper_block;
    const uint64_t hi = min(lo + a.sper_block, a.n_pairs);
    for (uint64_t tile = lo; tile < hi; tile += kPackThreads) {
        const uint64_t i = tile + tid;
        const bool valid = i < hi;
        const uint32_t k = valid ? key[i] : 0u;
        const uint32_t v = valid ? val[i] : 0u;
        const uint32_t digit = (k >> (8u * pass)) & 0xFFu;
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (uint32_t bit = 0; bit < 8; ++bit) {
            const bool one = (digit >> bit) & 1u;
            const unsigned long long b = __ballot(one);
            peers &= one ? b : ~b;
        }
        const uint32_t rank = __popcll(peers & ((1ull << lane) - 1ull));
        if (valid && rank == 0) {
            wcount[wv][digit] = __popcll(peers);  // the lowest lane of the digit's lanes: one store
        }
        __syncthreads();
        uint32_t run = 0;
        if (tid < kPndDigits) {
            for (uint32_t w = 0; w < kWaves; ++w) {
                const uint32_t c = wcount[w][tid];
                wcount[w][tid] = run;
                run += c;
            }
        }
        __syncthreads();
        if (valid) {
            const uint64_t at = (uint64_t)base[digit] + wcount[wv][digit] + rank;
            if (at < a.n_pairs) {
                key_to[at] = k;
                val_to[at] = v;
            }
        }
        __syncthreads();
        if (tid < kPndDigits) {
            base[tid] += run;
        }
        for (uint32_t j = tid; j < kWaves * kPndDigits; j += kPackThreads) {
            (&wcount[0][0])[j] = 0;
        }
        __syncthreads();
    }
}

// The first of the n sorted apps that is not below `app`.
__device__ __forceinline__ uint64_t first_not_below(const uint32_t* key, uint64_t n, uint64_t app)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (key[mid] < app) {
            lo = mid + 1;
        } else {
            hi = mid;
        }
    }
    return lo;
}

__device__ __forceinline__ uint32_t limit_of(const PndArgs& a, uint64_t app)
{
    return a.limit ? a.limit[app] : 0xFFFFFFFFu;
}

// Step 7.
__global__ __launch_bounds__(kPackThreads) void k_pnd_bounds(PndArgs a)
{
    const uint32_t* key = a.key[a.passes & 1u];
    layout_count(apps_view(a), [&](uint64_t e, uint64_t, uint32_t) {
        const uint64_t f = first_not_below(key, a.n_pairs, e);
        const uint64_t g = first_not_below(key, a.n_pairs, e + 1);
        a.afirst[e] = (uint32_t)f;
        a.acount[e] = (uint32_t)(g - f);
        return (unsigned long long)min((uint32_t)(g - f), limit_of(a, e));
    });
}

// Step 8.
__global__ __launch_bounds__(kPackThreads) void k_pnd_check(PndArgs a)
{
    __shared__ unsigned long long bpre[kPackBlocks + 1];
    block_prefix(apps_view(a), bpre);
    const unsigned long long before = bpre[blockIdx.x];
    const uint64_t lo = (uint64_t)blockIdx.x * a.aper_block;
    const uint64_t hi = min(lo + a.aper_block, a.n_apps);
    for (uint64_t e = lo + threadIdx.x; e < hi; e += kPackThreads) {
        const unsigned long long at = a.aoff[e] + before;
        a.aoff[e] = at;
        if (!a.size_only && at + min(a.acount[e], limit_of(a, e)) > a.list_cap) {
            refuse(a, BMQCRC_PND_KIND_LIST_TOO_SMALL, e);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.ctr[kPndCtrListed] = bpre[a.anblocks];
    }
}

// Step 9.  The word is final: on a refusal the host reads kind and index from
// it, and the kernel leaves.
__global__ __launch_bounds__(kPackFrameThreads) void k_pnd_frame(PndArgs a)
{
    if (a.ctr[kPndCtrRefusal] != 0) {
        return;
    }
    const uint64_t stride = (uint64_t)gridDim.x * kPackFrameThreads;
    const uint64_t t0 = (uint64_t)blockIdx.x * kPackFrameThreads + threadIdx.x;
    const uint32_t* key = a.key[a.passes & 1u];
    const uint32_t* val = a.val[a.passes & 1u];
    for (uint64_t i = t0; i < a.n_pairs; i += stride) {
        const uint64_t e = key[i];
        if (e >= a.n_apps) {
            continue;
        }
        const uint64_t r = i - a.afirst[e];
        const uint32_t lim = limit_of(a, e);
        if (r < lim) {
            const unsigned long long at = a.aoff[e] + r;
            if (at < a.list_cap) {
                a.records[at] = val[i];
                a.out_queue_ids[at] = a.queue_ids[e];
                if (a.out_sub_ids) {
                    a.out_sub_ids[at] = a.sub_ids[e];
                }
            }
        } else if (r == lim && a.app_next) {
            a.app_next[e] = val[i];
        }
    }
    for (uint64_t e = t0; e <= a.n_apps; e += stride) {
        if (e == a.n_apps) {
            a.list_first[e] = a.ctr[kPndCtrListed];
            continue;
        }
        a.list_first[e] = a.aoff[e];
        if (a.app_pending) {
            a.app_pending[e] = a.acount[e];
        }
        if (a.app_next && a.acount[e] <= limit_of(a, e)) {
            a.app_next[e] = (uint32_t)a.n_records;  // nothing stands beyond the limit
        }
    }
    if (a.pending_mask) {
        for (uint64_t r = t0; r < a.n_records; r += stride) {
            a.pending_mask[r] = a.mask[r];
        }
    }
}

}  // namespace
}  // namespace bmqcrc

using namespace bmqcrc;

extern "C" int bmqcrc_launch_pending_list_masks(const PndArgs* a, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_pnd_classify, dim3(a->cblocks), dim3(kPackThreads), 0, s, *a);
    hipLaunchKernelGGL(k_pnd_join, dim3(a->nblocks), dim3(kPackThreads), 0, s, *a);
    hipLaunchKernelGGL(k_pnd_mask, dim3(a->nblocks), dim3(kPackThreads), 0, s, *a);
    hipLaunchKernelGGL(k_pnd_total, dim3(1), dim3(kPackThreads), 0, s, *a);
    return hipGetLastError() != hipSuccess;
}

extern "C" int bmqcrc_launch_pending_list_lists(const PndArgs* a, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (a->snblocks) {
        hipLaunchKernelGGL(k_pnd_emit, dim3(a->nblocks), dim3(kPackThreads), 0, s, *a);
        for (uint32_t pass = 0; pass < a->passes; ++pass) {
            hipLaunchKernelGGL(k_pnd_hist, dim3(a->snblocks), dim3(kPackThreads), 0, s, *a, pass);
            hipLaunchKernelGGL(k_pnd_scan, dim3(kPndDigits), dim3(kPndDigits), 0, s, *a);
            hipLaunchKernelGGL(k_pnd_scatter, dim3(a->snblocks), dim3(kPackThreads), 0, s, *a,
                               pass);
        }
    }
    if (a->anblocks) {
        hipLaunchKernelGGL(k_pnd_bounds, dim3(a->anblocks), dim3(kPackThreads), 0, s, *a);
        hipLaunchKernelGGL(k_pnd_check, dim3(a->anblocks), dim3(kPackThreads), 0, s, *a);
    }
    if (!a->size_only) {
        const uint64_t units = a->n_pairs > a->n_records ? a->n_pairs : a->n_records;
        const uint64_t work = units > a->n_apps + 1 ? units : a->n_apps + 1;
        const uint64_t want = (work + kPackFrameThreads - 1) / kPackFrameThreads;
        const uint32_t blocks = (uint32_t)(want > kPackFrameBlocks ? kPackFrameBlocks : want);
        hipLaunchKernelGGL(k_pnd_frame, dim3(blocks ? blocks : 1u), dim3(kPackFrameThreads), 0, s,
                           *a);
    }
    return hipGetLastError() != hipSuccess;
}
