// crc32c_storage_apply.hip -- MI355X (gfx950) replica side of replication:
// device-resident STORAGE events applied to a journal run and a DATA window
// (bmqcrc_storage_event_apply, ABI 2.15).
//
// The device-side form of FileStore::processStorageEvent and
// FileStoreUtil::writeMessageRecordImpl: a STORAGE event is an EventHeader and
// a chain of storage messages, each a StorageHeader (12 bytes at least) and a
// 60-byte journal record, a DATA message (type 1) carrying its whole DATA
// record behind that.  The chain is serial inside an event, exactly as a
// PutHeader chain is, so the walks are crc32c_put_unpack.hip's: one wave walks
// one event, the grid strides over the events.  Seven kernels on one stream
// around the fused copy of crc32c_copy.hip:
//
//   1. k_sap_walk<false>: every event validated, its messages counted into
//      first[e]; the first violation of an event raises the call's refusal
//      word (crc32c_pack_layout.h) and leaves its offset in bad_off[e].
//   2. k_sap_scan: first[] becomes the exclusive prefix of the counts, and the
//      lowest event whose last message lies past msg_cap is refused.
//   3. k_sap_walk<true>: the same walk again, now placing: per message the
//      journal record's offset, the application data's offset and length, the
//      DATA record's size R and its header + options size, the bytes after the
//      journal record, type and flags, all to the WORKSPACE.  The slots no
//      message took -- all of them when anything was refused -- become empty
//      messages (empty_slots of crc32c_unpack_slots.h).
//   4. k_sap_count: pass 1 of crc32c_pack_layout.h over R of the msg_cap slots.
//   5. k_sap_check: every block scans the block sums (block_prefix), which
//      makes off[i] the 64-bit prefix Q[i]; then per message the checks that
//      need its predecessor or Q: the journal offset, the sequence of lease
//      ids and sequence numbers, the DATA offset, and whether both
//      destinations hold what is to be written.
//   6. k_sap_seal: off[i] becomes where message i's application data goes,
//      Q[i] + header + options -- or, when anything was refused, an offset
//      past data_dst_bytes for EVERY slot: the copy kernels then refuse every
//      message, own no piece and write neither data_dst nor their CRCs.  (A
//      kernel of its own, because step 5's refusals are found message by
//      message: no block of step 5 knows what another one found.)
//   (the payload: bmqcrc_launch_copy over the msg_cap slots, as it is)
//   7. k_sap_frame: unless refused, the 15 dwords of every journal record,
//      DataHeader + options and the padding bytes of every DATA record, the
//      caller's arrays, the mismatches and the new write head.  On a refusal
//      it names the event, the message and the byte and leaves.
//
// The walk loads no byte it has not shown to lie inside its event: the
// event's bounds are checked against events_bytes first, pos + 12 <= end
// before a StorageHeader, pos + messageWords * 4 <= end before anything behind
// it.  Every later kernel reads `events` only at offsets the walk left in the
// workspace.  Every size in the format is a word count and event offsets are
// multiples of 4, so every position is one and the header copies are dword
// copies.  A step advances by at least 72 bytes, which bounds the loop by the
// event's size.
//
// The walk's DATA-record check states the clauses of data_record
// (crc32c_journal_stage.h) but is not that function: its bound `stop` is the
// end of the storage message inside the event, not of a caller's window, and
// its words come from the wave's LDS ring (Window::need / be32), wave-uniform,
// not from loads of the thread's own.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmqcrc_internal.h"
#include "crc32c_pack_layout.h"
#include "crc32c_unpack_slots.h"

namespace bmqcrc {
namespace {

constexpr uint32_t kWindowDwords = kUnpackWindowBytes / 4;
static_assert(kWindowDwords == 4 * kUnpackWalkThreads, "Window::fetch: four dwords per lane");
constexpr uint64_t kJournalBytes = 4 * kJournalRecordDwords;

// A refusal of event e: the call's word, and the byte it names.
__device__ __forceinline__ void refuse_event(const SapArgs& a, uint32_t kind, uint64_t e,
                                             uint64_t offset)
{
    if (threadIdx.x == 0) {
        a.bad_off[e] = offset;
        refuse(a, kind, e);
    }
}

// A wave's view of its event, as crc32c_put_unpack.hip's Window (that unit's
// kernels stay what they were, so this is a copy): a ring of two 1 KiB chunks
// in LDS covering bytes [cb, cb + 2 KiB) of the events buffer, and the chunk
// behind them on its way into four registers per lane.  The walk moves forward
// only.  A position at most one chunk ahead takes the prefetched chunk into
// the ring and issues the next prefetch; one further ahead -- a long message --
// loads all three afresh.  Only whole dwords inside [ev0, end), the event, are
// ever loaded: a lane whose dword lies outside reads the event's first dword
// instead, which is never used, since the walk checks a position against `end`
// before it looks it up.
struct Window {
    const uint8_t* events;
    uint32_t* ring;     // LDS, 2 * kWindowDwords
    uint64_t ev0, end;  // the event: ev0 + 8 <= end
    uint64_t cb;        // ring chunk `slot` covers [cb, cb + 1 KiB), the other the next KiB
    uint32_t slot;
    uint32_t nx[4];     // [cb + 2 KiB, cb + 3 KiB), in flight

    __device__ __forceinline__ void fetch(uint64_t from, uint32_t (&v)[4]) const
    {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint64_t p = from + 4ull * (threadIdx.x + 64u * j);
            v[j] = *(const uint32_t*)(events + (p + 4 <= end ? p : ev0));
        }
    }
    __device__ __forceinline__ void store(uint32_t s, const uint32_t (&v)[4])
    {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            ring[s * kWindowDwords + threadIdx.x + 64u * j] = v[j];
        }
    }
    __device__ __forceinline__ void reload(uint64_t at)
    {
        uint32_t c0[4], c1[4];
        fetch(at, c0);
        fetch(at + kUnpackWindowBytes, c1);
        fetch(at + 2 * kUnpackWindowBytes, nx);
        __syncthreads();  // (one wave per block: orders the LDS reads before)
        store(0, c0);
        store(1, c1);
        __syncthreads();
        cb = at;
        slot = 0;
    }
    __device__ __forceinline__ void advance()
    {
        __syncthreads();
        store(slot, nx);
        slot ^= 1u;
        cb += kUnpackWindowBytes;
        fetch(cb + 2 * kUnpackWindowBytes, nx);
        __syncthreads();
    }
    // makes [p, p + bytes) readable, p >= cb a multiple of 4, bytes <= 12
    __device__ __forceinline__ void need(uint64_t p, uint32_t bytes)
    {
        if (p + bytes > cb + 2 * kUnpackWindowBytes) {
            if (p + bytes <= cb + 3 * kUnpackWindowBytes) {
                advance();  // (p > cb + 2 KiB - 12: inside the ring's new first chunk)
            } else {
                reload(p);
            }
        }
    }
    // big-endian dword at byte position p of the buffer, made readable before
    __device__ __forceinline__ uint32_t be32(uint64_t p) const
    {
        const uint32_t i =
            ((uint32_t)((p - cb) >> 2) + slot * kWindowDwords) & (2 * kWindowDwords - 1);
        return __builtin_bswap32(__builtin_amdgcn_readfirstlane(ring[i]));
    }
};

// One event, walked by the block's one wave; every value that steers the walk
// is the same in all lanes.  kPlace false: validate and count into first[e].
// kPlace true (the walk refused nothing, first[] is the prefix): place the
// event's first[e + 1] - first[e] messages from slot first[e] on.
template <bool kPlace>
__device__ __forceinline__ void walk_event(const SapArgs& a, uint64_t e, uint32_t* win)
{
    const uint32_t lane = threadIdx.x;
    uint64_t beg = 0, end = a.events_bytes;
    if (a.event_offsets) {
        beg = a.event_offsets[e];
        end = a.event_offsets[e + 1];
    }
    uint64_t slot = 0, limit = ~0ull;  // kPlace: the event's first slot, its messages
    if (kPlace) {
        slot = a.first[e];
        limit = a.first[e + 1] - slot;
        if (limit == 0) {
            return;
        }
    } else if (lane == 0) {
        a.first[e] = 0;
    }
    if (beg > end || end > a.events_bytes || (beg & 3u)) {
        if (!kPlace) {
            refuse_event(a, BMQCRC_SAP_KIND_EVENT_OFFSETS, e, beg);
        }
        return;
    }
    const uint64_t size = end - beg;
    if (size < 8) {
        if (!kPlace) {
            refuse_event(a, BMQCRC_SAP_KIND_EVENT_HEADER, e, beg);
        }
        return;
    }
    Window w;
    w.events = a.events;
    w.ring = win;
    w.ev0 = beg;
    w.end = end;
    w.reload(beg);
    {
        const uint32_t h1 = w.be32(beg + 4);  // bytes 4..7: PV | type, headerWords, ...
        const uint64_t hw = (uint64_t)((h1 >> 16) & 0xFFu) * 4;
        const uint32_t type = (h1 >> 24) & 0x3Fu;
        uint64_t bad = ~0ull;
        if ((w.be32(beg) & 0x7FFFFFFFu) != size) {
            bad = 0;  // EventHeader length differs from the event size
        } else if (type != 8u && type != 10u) {
            bad = 4;  // neither a STORAGE nor a PARTITION_SYNC event
        } else if (hw < 8 || hw > size) {
            bad = 5;  // EventHeader headerWords out of range
        }
        if (bad != ~0ull) {
            if (!kPlace) {
                refuse_event(a, BMQCRC_SAP_KIND_EVENT_HEADER, e, beg + bad);
            }
            return;
        }
        beg += hw;
    }
    uint64_t pos = beg, k = 0;
    // the lane's own message of the current 64
    uint64_t my_jrn = 0, my_app = 0;
    uint32_t my_len = 0, my_rec = 0, my_hdr = 0, my_pay = 0, my_meta = 0;
    // lanes [0, cnt) hold messages slot + k0 ...: store them
    auto flush = [&](uint64_t k0, uint32_t cnt) {
        if (lane < cnt) {
            const uint64_t i = slot + k0 + lane;
            a.ws_off[i] = my_app;
            a.ws_len[i] = my_len;
            a.ws_jrn[i] = my_jrn;
            a.ws_rec[i] = my_rec;
            a.ws_hdr[i] = my_hdr;
            a.ws_pay[i] = my_pay;
            a.ws_meta[i] = my_meta;
            // MessageRecord @52: the CRC the producer computed
            a.ws_exp[i] = (my_meta & 0xFFu) == kSapTypeData
                              ? __builtin_bswap32(*(const uint32_t*)(a.events + my_jrn + 52))
                              : 0u;
        }
    };
    while (pos < end && k < limit) {
        uint32_t kind = 0;
        uint64_t at = pos;
        uint64_t msg = 0, shw = 0, hs = 0, opt = 0, total = 0;
        uint32_t pad = 0, type = 0, w0 = 0;
        if (pos + 12 > end) {
            kind = BMQCRC_SAP_KIND_STORAGE_HEADER;  // truncated StorageHeader
        } else {
            w.need(pos, 12);
            w0 = w.be32(pos);
            const uint32_t w1 = w.be32(pos + 4);
            msg = (uint64_t)(w0 & 0x07FFFFFFu) * 4;
            shw = (uint64_t)((w1 >> 24) & 0xFu) * 4;
            type = (w1 >> 16) & 0xFFu;
            if (shw < 12 || msg < shw || pos + msg > end || type < 1 || type > 6 ||
                msg - shw < kJournalBytes || (w1 & 0xFFFFu) != a.partition_id) {
                kind = BMQCRC_SAP_KIND_STORAGE_HEADER;
            } else if (type == kSapTypeData) {
                const uint64_t jr = pos + shw, dr = jr + kJournalBytes, stop = pos + msg;
                w.need(jr, 4);
                if ((w.be32(jr) >> 28) != 1u) {
                    kind = BMQCRC_SAP_KIND_STORAGE_HEADER;  // not a MESSAGE record
                } else if (dr + 8 > stop) {
                    kind = BMQCRC_SAP_KIND_DATA_RECORD;
                    at = dr;
                } else {
                    w.need(dr, 8);
                    const uint32_t h0 = w.be32(dr), h1 = w.be32(dr + 4);
                    hs = (uint64_t)(h0 >> 29) * 4;
                    total = (uint64_t)(h0 & 0x1FFFFFFFu) * 4;
                    opt = (uint64_t)(h1 >> 8) * 4;
                    bool bad = hs == 0 || total == 0 || hs + opt >= total || dr + total > stop;
                    if (!bad) {
                        w.need(dr + total - 4, 4);  // the dword of the padding byte
                        pad = w.be32(dr + total - 4) & 0xFFu;
                        bad = pad < 1 || pad > 8 || total < hs + opt + pad;
                    }
                    if (bad) {
                        kind = BMQCRC_SAP_KIND_DATA_RECORD;
                        at = dr;
                    }
                }
            }
        }
        if (kind) {
            if (!kPlace) {
                refuse_event(a, kind, e, at);
            }
            break;
        }
        if (kPlace && lane == (uint32_t)(k & 63u)) {
            const bool data = type == kSapTypeData;
            my_jrn = pos + shw;
            my_app = data ? my_jrn + kJournalBytes + hs + opt : 0;
            my_len = data ? (uint32_t)(total - hs - opt - pad) : 0u;
            my_rec = (uint32_t)total;  // at most 2^31 - 4; 0 when not DATA
            my_hdr = (uint32_t)(hs + opt);
            my_pay = (uint32_t)(msg - shw - kJournalBytes);
            my_meta = type | ((w0 >> 27) << 8) | ((uint32_t)shw << 16);
        }
        ++k;
        if (kPlace && (k & 63u) == 0) {
            flush(k - 64, 64);
        }
        pos += msg;
    }
    if (kPlace) {
        if (k & 63u) {
            flush(k & ~63ull, (uint32_t)(k & 63u));
        }
    } else if (lane == 0) {
        a.first[e] = k;
    }
}

// Steps 1 and 3.  The placing grid may be larger than the events: its blocks
// also empty the slots no message took.
template <bool kPlace>
__global__ __launch_bounds__(kUnpackWalkThreads) void k_sap_walk(SapArgs a)
{
    __shared__ uint32_t win[2 * kWindowDwords];
    const bool refused = kPlace && a.ctr[kSlotCtrRefusal] != 0;
    if (!refused) {
        for (uint64_t e = blockIdx.x; e < a.n_events; e += gridDim.x) {
            walk_event<kPlace>(a, e, win);
        }
    }
    if (kPlace) {
        // (first[n_events] <= msg_cap: the scan)
        empty_slots(a, refused ? 0 : a.first[a.n_events], kUnpackWalkThreads);
    }
}

// Step 2: one block, k_unpack_scan's shape.  first[e] = messages of the events
// before e, first[n_events] = of all; a refused event counts the messages in
// front of its violation.
__global__ __launch_bounds__(kUnpackThreads) void k_sap_scan(SapArgs a)
{
    __shared__ unsigned long long wtot[kUnpackThreads / 64];
    const uint32_t tid = threadIdx.x;
    unsigned long long carry = 0;
    for (uint64_t base = 0; base < a.n_events; base += kUnpackThreads) {
        const uint64_t e = base + tid;
        const unsigned long long c = e < a.n_events ? a.first[e] : 0ull;
        unsigned long long tot;
        const unsigned long long before = carry + tile_scan(c, wtot, &tot);
        if (e < a.n_events) {
            a.first[e] = before;
            // the lowest event whose last message does not fit
            if (before <= a.msg_cap && before + c > a.msg_cap) {
                refuse(a, BMQCRC_SAP_KIND_TOO_MANY_MESSAGES, e);
            }
        }
        carry += tot;
    }
    if (tid == 0) {
        a.first[a.n_events] = carry;
    }
}

// Step 4: the shared scan over R; an unused slot, or every slot after a
// refusal, counts for nothing.
__global__ __launch_bounds__(kPackThreads) void k_sap_count(SapArgs a)
{
    const uint64_t used = a.ctr[kSlotCtrRefusal] != 0 ? 0 : a.first[a.n_events];
    const LayoutView v = {a.ws_off, a.ws_len, a.msg_cap,   a.off,
                        a.bsum,   a.ctr,    a.per_block, a.nblocks};
    layout_count(v, [&a, used](uint64_t i, uint64_t, uint32_t) {
        return (unsigned long long)(i < used ? a.ws_rec[i] : 0u);
    });
}

// lease id and sequence number of the journal record at byte `jrn` of events
__device__ __forceinline__ void record_psn(const SapArgs& a, uint64_t jrn, uint32_t* lease,
                                           uint64_t* seq)
{
    const uint32_t* r = (const uint32_t*)(a.events + jrn);
    *seq = ((uint64_t)(__builtin_bswap32(r[0]) & 0xFFFFu) << 32) | __builtin_bswap32(r[1]);
    *lease = __builtin_bswap32(r[2]);
}

// Step 5.
__global__ __launch_bounds__(kPackThreads) void k_sap_check(SapArgs a)
{
    __shared__ unsigned long long bpre[kPackBlocks + 1];
    // The walk's word: kinds up to TOO_MANY_MESSAGES.  A higher kind is raised
    // by this pass itself and never replaces one of the walk's, so the test
    // gives the same answer in every block whenever it starts.
    const unsigned long long word = a.ctr[kSlotCtrRefusal];
    if (word != 0 && (~word >> 56) <= BMQCRC_SAP_KIND_TOO_MANY_MESSAGES) {
        return;
    }
    const uint32_t tid = threadIdx.x;
    const unsigned long long pieces = block_prefix(a, bpre);
    const unsigned long long all = bpre[a.nblocks], before = bpre[blockIdx.x];
    const uint64_t n = a.first[a.n_events];  // <= msg_cap: the scan
    const uint64_t lo = (uint64_t)blockIdx.x * a.per_block;
    const uint64_t hi = min(lo + a.per_block, n);
    const bool journal_fits = kJournalBytes * n <= a.journal_dst_bytes;
    if (blockIdx.x == 0 && tid == 0) {
        a.ctr[kSlotCtrMsgs] = n;
        a.ctr[kSapCtrTotal] = all;
        if (!journal_fits) {
            // the lowest message whose journal record ends past journal_dst
            refuse(a, BMQCRC_SAP_KIND_DST_TOO_SMALL, a.journal_dst_bytes / kJournalBytes);
        }
        if (pieces > 0xFFFFFFFFull) {
            refuse(a, BMQCRC_SAP_KIND_TOO_MANY_PIECES, 0);
        }
    }
    for (uint64_t i = lo + tid; i < hi; i += kPackThreads) {
        const unsigned long long q = a.off[i] + before;
        a.off[i] = q;
        const uint64_t jrn = a.ws_jrn[i];
        const uint32_t meta = a.ws_meta[i];
        // StorageHeader dword 2: the primary's journal offset in words
        const uint32_t jow =
            __builtin_bswap32(*(const uint32_t*)(a.events + jrn - (meta >> 16) + 8));
        uint32_t lease, please = a.lease_id;
        uint64_t seq, pseq = a.seq;
        record_psn(a, jrn, &lease, &seq);
        if (i) {
            record_psn(a, a.ws_jrn[i - 1], &please, &pseq);
        }
        bool bad = 4ull * jow != a.journal_pos + kJournalBytes * i || lease < please ||
                   (lease == please && seq != pseq + 1);
        if ((meta & 0xFFu) == kSapTypeData) {
            // MessageRecord @32: MessageOffsetDwords
            const uint32_t mod = __builtin_bswap32(*(const uint32_t*)(a.events + jrn + 32));
            bad = bad || 8ull * mod != a.data_file_pos + q;
            if (journal_fits && q + a.ws_rec[i] > a.data_dst_bytes) {
                refuse(a, BMQCRC_SAP_KIND_DST_TOO_SMALL, i);
            }
        }
        if (bad) {
            refuse(a, BMQCRC_SAP_KIND_OUT_OF_SYNC, i);
        }
    }
}

// Step 6.
__global__ __launch_bounds__(kPackThreads) void k_sap_seal(SapArgs a)
{
    const bool refused = a.ctr[kSlotCtrRefusal] != 0;
    const uint64_t n = refused ? 0 : a.first[a.n_events];
    const uint64_t stride = (uint64_t)gridDim.x * kPackThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kPackThreads + threadIdx.x; i < a.msg_cap;
         i += stride) {
        // past any data_dst_bytes: the copy kernels refuse the message
        a.off[i] = refused ? ~0ull : i < n ? a.off[i] + a.ws_hdr[i] : 0ull;
    }
}

// Step 7, after the copy.
__global__ __launch_bounds__(kPackFrameThreads) void k_sap_frame(SapArgs a)
{
    const uint64_t t0 = (uint64_t)blockIdx.x * kPackFrameThreads + threadIdx.x;
    const unsigned long long word = a.ctr[kSlotCtrRefusal];
    if (word != 0) {
        if (t0 == 0) {
            const unsigned long long key = ~word;
            const uint32_t kind = (uint32_t)(key >> 56);
            const uint64_t index = key & ((1ull << 56) - 1);
            uint64_t e = index, i = index, offset;
            if (kind <= BMQCRC_SAP_KIND_TOO_MANY_MESSAGES) {
                // the word names the event.  The message: the one the walk
                // stopped at, else the event's first.  (TOO_MANY_MESSAGES
                // names no byte: the event's start)
                const bool stopped = kind == BMQCRC_SAP_KIND_STORAGE_HEADER ||
                                     kind == BMQCRC_SAP_KIND_DATA_RECORD;
                i = a.first[stopped ? e + 1 : e];
                offset = kind != BMQCRC_SAP_KIND_TOO_MANY_MESSAGES ? a.bad_off[e]
                         : a.event_offsets                         ? a.event_offsets[e]
                                                                   : 0ull;
            } else {
                // the word names the message: its event is the one with
                // first[e] <= i < first[e + 1], its byte the StorageHeader's
                uint64_t l = 0, h = a.n_events - 1;
                while (l < h) {
                    const uint64_t mid = l + (h - l) / 2;
                    if (a.first[mid + 1] > i) {
                        h = mid;
                    } else {
                        l = mid + 1;
                    }
                }
                e = l;
                offset = a.ws_jrn[i] - (a.ws_meta[i] >> 16);
            }
            a.ctr[kSapCtrEvent] = e;
            a.ctr[kSapCtrIndex] = i;
            a.ctr[kSapCtrOffset] = offset;
        }
        return;
    }
    const uint64_t stride = (uint64_t)gridDim.x * kPackFrameThreads;
    const uint64_t n = a.first[a.n_events];
    // Thread t of the grid owns dword t % 15 of journal record t / 15
    // (n < 2^32: a dword's index needs 36 bits); the division in 32 bits
    // whenever the call's indices fit.
    const uint64_t ndw = kJournalRecordDwords * n;
    const bool narrow = ndw <= 0xFFFFFFFFull;
    for (uint64_t t = t0; t < ndw; t += stride) {
        const uint64_t m = narrow ? (uint32_t)t / kJournalRecordDwords : t / kJournalRecordDwords;
        const uint32_t j = (uint32_t)(t - kJournalRecordDwords * m);
        ((uint32_t*)a.journal_dst)[t] = *(const uint32_t*)(a.events + a.ws_jrn[m] + 4 * j);
    }
    // One message per thread and step: its DATA record's frame and its entries.
    unsigned long long bad = 0, lowest = 0, data = 0;
    for (uint64_t i = t0; i < n; i += stride) {
        const uint64_t jrn = a.ws_jrn[i];
        const uint32_t meta = a.ws_meta[i], type = meta & 0xFFu;
        const uint32_t len = a.ws_len[i], hdr = a.ws_hdr[i], rec = a.ws_rec[i];
        const uint64_t q = a.off[i] - hdr;
        uint32_t exp = 0, crc = 0;
        if (type == kSapTypeData) {
            const uint8_t* src = a.events + jrn + kJournalBytes;
            uint8_t* dst = a.data_dst + q;
            // DataHeader and options, then the padding: byte stores, so that
            // no word that holds application data is read and written back
            for (uint32_t b = 0; b < hdr; b += 4) {
                *(uint32_t*)(dst + b) = *(const uint32_t*)(src + b);
            }
            for (uint32_t b = hdr + len; b < rec; ++b) {
                dst[b] = src[b];
            }
            exp = a.ws_exp[i];
            crc = a.ws_out[i];
            ++data;
            if (crc != exp) {
                ++bad;
                lowest = max(lowest, ~(unsigned long long)i);
            }
        }
        if (a.types) {
            a.types[i] = (uint8_t)type;
        }
        if (a.flags) {
            a.flags[i] = (uint8_t)(meta >> 8);
        }
        if (a.payload_offsets) {
            a.payload_offsets[i] = jrn + kJournalBytes;
        }
        if (a.payload_lengths) {
            a.payload_lengths[i] = a.ws_pay[i];
        }
        if (a.record_offsets) {
            a.record_offsets[i] = q;
        }
        if (a.lengths) {
            a.lengths[i] = len;
        }
        if (a.expected) {
            a.expected[i] = exp;
        }
        if (a.out) {
            a.out[i] = crc;
        }
        if (i + 1 == n) {
            uint32_t lease;
            uint64_t seq;
            record_psn(a, jrn, &lease, &seq);
            a.ctr[kSapCtrHeadLease] = lease;
            a.ctr[kSapCtrHeadSeq] = seq;
        }
    }
    if (a.event_first) {
        for (uint64_t e = t0; e <= a.n_events; e += stride) {
            a.event_first[e] = a.first[e];
        }
    }
    if (t0 == 0 && a.record_offsets) {
        a.record_offsets[n] = a.ctr[kSapCtrTotal];
    }
    data = wave_sum(data);
    if ((threadIdx.x & 63u) == 0 && data) {
        atomicAdd(&a.ctr[kSapCtrData], data);
    }
    if (bad) {
        atomicAdd(&a.ctr[kSlotCtrBad], bad);
        atomicMax(&a.ctr[kSlotCtrFirstBad], lowest);
    }
}

}  // namespace
}  // namespace bmqcrc

using namespace bmqcrc;

extern "C" int bmqcrc_launch_storage_apply_layout(const SapArgs* a, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    const uint64_t walk = a->n_events < kUnpackWalkBlocks ? a->n_events : kUnpackWalkBlocks;
    // 16 slots per thread at least for the blocks that only empty slots
    const uint64_t fill = a->msg_cap / (16 * kUnpackWalkThreads);
    const uint64_t place = fill < walk ? walk : fill > kUnpackWalkBlocks ? kUnpackWalkBlocks : fill;
    hipLaunchKernelGGL(k_sap_walk<false>, dim3((uint32_t)walk), dim3(kUnpackWalkThreads), 0, s, *a);
    hipLaunchKernelGGL(k_sap_scan, dim3(1), dim3(kUnpackThreads), 0, s, *a);
    hipLaunchKernelGGL(k_sap_walk<true>, dim3((uint32_t)place), dim3(kUnpackWalkThreads), 0, s, *a);
    hipLaunchKernelGGL(k_sap_count, dim3(a->nblocks), dim3(kPackThreads), 0, s, *a);
    hipLaunchKernelGGL(k_sap_check, dim3(a->nblocks), dim3(kPackThreads), 0, s, *a);
    hipLaunchKernelGGL(k_sap_seal, dim3(a->nblocks), dim3(kPackThreads), 0, s, *a);
    return hipGetLastError() != hipSuccess;
}

extern "C" int bmqcrc_launch_storage_apply_frame(const SapArgs* a, void* stream)
{
    const uint64_t want =
        (kJournalRecordDwords * a->msg_cap + kPackFrameThreads - 1) / kPackFrameThreads;
    const uint32_t blocks =
        (uint32_t)(want > kPackFrameBlocks ? kPackFrameBlocks : want < 1 ? 1 : want);
    hipLaunchKernelGGL(k_sap_frame, dim3(blocks), dim3(kPackFrameThreads), 0, (hipStream_t)stream,
                       *a);
    return hipGetLastError() != hipSuccess;
}
