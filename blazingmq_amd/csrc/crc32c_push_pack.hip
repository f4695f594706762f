// crc32c_push_pack.hip -- MI355X (gfx950) delivery to consumers: device-resident
// journal and DATA records packed into PUSH events (bmqcrc_push_event_pack,
// ABI 2.17).
//
// The device-side form of mqba::ClientSession's delivery loop with
// bmqp::PushEventBuilder::packMessage: per message a 32-byte PushHeader, O
// bytes of one sub-queue option (0, 4, 8 or 12, uniform over the call), the
// application data of the DATA record its MESSAGE record names and 1..4 padding
// bytes; per event an 8-byte EventHeader.  Message m is journal record
// records[m] (any order, repeats allowed), so every message is independent: a
// gather, a scan and a scatter.  With L[m] the application data's length,
// B[m] = 32 + O + L[m] + (4 - L[m] % 4) and P its 64-bit exclusive prefix,
// message m's PushHeader lies at 8 (e(m) + 1) + P[m] and event e starts at
// 8 e + P[event_first[e]].  Five kernels on one stream around the fused copy of
// crc32c_copy.hip:
//
//   1. k_ppk_classify: the grid is nblocks x kPackThreads over contiguous
//      message ranges (layout_split), one message per thread and step.  The
//      seven dwords of record records[m] the checks need are gathered straight
//      from memory -- the records of a wave are not contiguous, so the LDS
//      staging of crc32c_journal_stage.h does not fit, and the identity
//      (records == nullptr) takes the same path: one code path, and the journal
//      is 60 bytes a message beside the payload the copy moves.  Record index,
//      RecordHeader and type, data offset, DATA record, in this order; then the
//      flags and the payload cap.  Every message leaves the application data's
//      window offset and length, the stored CRC and CAT | SchemaId |
//      MESSAGE_PROPERTIES in the workspace -- an empty message when refused.
//   2. k_ppk_count: pass 1 of crc32c_pack_layout.h over B, and event_first's
//      shape.
//   3. k_ppk_check: unless step 1 or 2 refused, every event's size against the
//      cap and (with a destination) its end against dst_bytes, and the pieces
//      against the copy's limit; the total.
//   4. k_ppk_seal: off[m] becomes where message m's application data goes,
//      8 (e(m) + 1) + P[m] + 32 + O -- or, when anything was refused, an offset
//      past dst_bytes for EVERY message: the copy kernels then refuse every
//      message, own no piece and write neither dst nor their CRCs.  A size-only
//      call (dst == nullptr) ends here: the kernel writes event_offsets instead
//      and leaves off[] alone.
//   (the payload: bmqcrc_launch_copy over the n messages, as it is)
//   5. k_ppk_frame: unless refused, the 8 + O / 4 dwords of every PushHeader
//      and option, indexed across the grid so that adjacent lanes store
//      adjacent dwords; the padding as bytes; the EventHeaders; the caller's
//      arrays and the mismatches.
//
// No byte outside [journal, +60 n_records) and [data, +data_bytes) is loaded:
// the journal is read by record index below n_records only; of the DATA window
// step 1 reads what data_record (crc32c_journal_stage.h) reads of a record it
// finds inside the window, and the SchemaId word at o + 8 of such a record
// whose header has 3 words or more.  Every size in the format is a word count
// and the padding brings B to a multiple of 4, so every header position in dst
// is a multiple of 4.  Nothing is stored to dst that step 3 has not shown to
// lie below dst_bytes: it checks every event's end.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmqcrc_internal.h"
#include "crc32c_journal_stage.h"
#include "crc32c_pack_layout.h"

namespace bmqcrc {
namespace {

constexpr uint32_t kHeaderDwords = kPushHeaderBytes / 4;  // 8
constexpr uint32_t kFlagOutOfOrder = 4, kFlagProperties = 2;  // PushHeaderFlags
constexpr uint32_t kEventPush = 4;                        // EventType::e_PUSH

// 1..4 bytes, each equal to the count (ProtocolUtil::appendPadding)
__device__ __forceinline__ uint32_t padding(uint32_t len)
{
    return 4u - (len & 3u);
}

// Step 1.
__global__ __launch_bounds__(kPackThreads) void k_ppk_classify(PpkArgs a)
{
    const uint64_t lo = (uint64_t)blockIdx.x * a.per_block;
    const uint64_t hi = min(lo + a.per_block, a.n);
    const uint64_t end = a.data_bytes;
    for (uint64_t m = lo + threadIdx.x; m < hi; m += kPackThreads) {
        const uint64_t r = a.records ? a.records[m] : m;
        uint64_t app = 0;
        uint32_t len = 0, exp = 0, meta = 0;
        bool ok = false;
        if (r >= a.n_records) {
            refuse(a, BMQCRC_PPK_KIND_RECORD_INDEX, m);
        } else {
            const uint32_t* d = a.journal + kJournalRecordDwords * r;
            // all seven in flight together: nothing below depends on another
            const uint32_t d0 = d[0], d1 = d[1], d2 = d[2], d5 = d[5], d8 = d[8], d13 = d[13],
                           d14 = d[14];
            const uint32_t w0 = __builtin_bswap32(d0);  // type | flags | sequence number's top
            uint64_t ow;
            DataRecord dr;
            uint32_t schema = 0;
            if (!record_header_ok(w0, d1, d2, d14, kRecMessage)) {  // type 1 alone
                refuse(a, BMQCRC_PPK_KIND_RECORD, m);
            } else if (!data_window_offset(d8, a.data_file_pos, end, &ow)) {
                refuse(a, BMQCRC_PPK_KIND_DATA_OFFSET, m);
            } else if (!data_record(a.data, end, ow, &dr, [&](uint64_t hs) {
                           // SchemaId: DataHeader bytes 8..9, there from 3 header words on
                           // (12 <= hs < total: inside the record)
                           if (hs >= 12) {
                               schema = *(const uint32_t*)(a.data + ow + 8) & 0xFFFFu;
                           }
                       })) {
                refuse(a, BMQCRC_PPK_KIND_DATA_RECORD, m);
            } else {
                ok = true;
                app = dr.app;
                len = dr.len;
                exp = __builtin_bswap32(d13);  // MessageRecord @52
                // MessageRecord @21: CAT in the low 3 bits
                meta = schema | (((d5 >> 8) & 7u) << kPpkMetaCatShift) |
                       ((dr.h1 & 1u) ? kPpkMetaPropsBit : 0u);
            }
        }
        if (a.flags && (a.flags[m] & ~kFlagOutOfOrder)) {
            refuse(a, BMQCRC_PPK_KIND_FLAGS, m);
        }
        if (ok && len > a.max_payload_bytes) {
            refuse(a, BMQCRC_PPK_KIND_PAYLOAD_TOO_BIG, m);
        }
        a.ws_off[m] = app;
        a.ws_len[m] = len;
        a.ws_exp[m] = exp;
        a.ws_meta[m] = meta;
    }
}

// Step 2: the shared scan over B, then event_first's shape.
__global__ __launch_bounds__(kPackThreads) void k_ppk_count(PpkArgs a)
{
    const LayoutView v = {a.ws_off, a.ws_len, a.n, a.off, a.bsum, a.ctr, a.per_block, a.nblocks};
    const uint32_t lead = kPushHeaderBytes + a.opt_bytes;
    layout_count(v, [lead](uint64_t, uint64_t, uint32_t len) {
        return (unsigned long long)lead + len + padding(len);
    });
    event_first_shape(a, BMQCRC_PPK_KIND_EVENT_FIRST);
}

// Step 3: the events, one per thread.
__global__ __launch_bounds__(kPackThreads) void k_ppk_check(PpkArgs a)
{
    // Steps 1 and 2's word: kinds up to PAYLOAD_TOO_BIG.  A higher kind is
    // raised by this pass itself and never replaces one of theirs, so the test
    // gives the same answer in every block whenever it starts.
    const unsigned long long word = a.ctr[kSlotCtrRefusal];
    if (word != 0 && (~word >> 56) <= BMQCRC_PPK_KIND_PAYLOAD_TOO_BIG) {
        return;
    }
    events_check(a, BMQCRC_PPK_KIND_EVENT_TOO_BIG, BMQCRC_PPK_KIND_DST_TOO_SMALL,
                 BMQCRC_PPK_KIND_TOO_MANY_PIECES, kPpkCtrTotal, true);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.ctr[kSlotCtrMsgs] = a.n;
    }
}

// Step 4.  The word is final.
__global__ __launch_bounds__(kPackThreads) void k_ppk_seal(PpkArgs a)
{
    if (!a.dst) {
        unsigned long long* bpre = shared_bpre();
        // size only: where every event would start, and the total behind the last
        if (a.ctr[kSlotCtrRefusal] != 0 || !a.event_offsets) {
            return;
        }
        block_prefix(a, bpre);
        const unsigned long long all = bpre[a.nblocks];
        const uint64_t stride = (uint64_t)gridDim.x * kPackThreads;
        for (uint64_t e = (uint64_t)blockIdx.x * kPackThreads + threadIdx.x; e <= a.n_events;
             e += stride) {
            const uint64_t f = e == a.n_events ? a.n : a.event_first ? a.event_first[e] : 0;
            const unsigned long long p = f == a.n ? all : a.off[f] + bpre[f / a.per_block];
            a.event_offsets[e] = kEventHeaderBytes * e + p;
        }
        return;
    }
    const uint32_t lead = kPushHeaderBytes + a.opt_bytes;
    seal_offsets(a, [lead](uint64_t) { return lead; });
}

// Step 5, after the copy.  The word is final: on a refusal the host reads kind
// and index from it, and the kernel leaves.
__global__ __launch_bounds__(kPackFrameThreads) void k_ppk_frame(PpkArgs a)
{
    if (a.ctr[kSlotCtrRefusal] != 0) {
        return;
    }
    const uint64_t stride = (uint64_t)gridDim.x * kPackFrameThreads;
    const uint64_t t0 = (uint64_t)blockIdx.x * kPackFrameThreads + threadIdx.x;
    const uint32_t lead = kPushHeaderBytes + a.opt_bytes;
    const uint32_t hdw = lead >> 2;  // 8..11
    // Thread t of the grid owns dword t % hdw of message t / hdw: eight of the
    // PushHeader, then the option's (n < 2^32: a dword's index needs 36 bits);
    // the division in 32 bits whenever the call's indices fit.  A thread's
    // loads all precede its one store.
    const uint64_t ndw = (uint64_t)hdw * a.n;
    const bool narrow = ndw <= 0xFFFFFFFFull;
    for (uint64_t t = t0; t < ndw; t += stride) {
        const uint64_t m = narrow ? (uint32_t)t / hdw : t / hdw;
        const uint32_t j = (uint32_t)(t - hdw * m);
        uint32_t v;
        if (j == 0) {
            // Flags(4) | MessageWords(28): header, option, padded application data in words
            const uint32_t len = a.ws_len[m];
            const uint32_t f = (a.flags ? (uint32_t)a.flags[m] & kFlagOutOfOrder : 0u) |
                               ((a.ws_meta[m] & kPpkMetaPropsBit) ? kFlagProperties : 0u);
            v = __builtin_bswap32((f << 28) | (hdw + ((len + padding(len)) >> 2)));
        } else if (j == 1) {
            // OptionsWords(24) | CAT(3) | HeaderWords(5) = 8
            v = __builtin_bswap32(((a.opt_bytes >> 2) << 8) |
                                  (((a.ws_meta[m] >> kPpkMetaCatShift) & 7u) << 5) |
                                  kHeaderDwords);
        } else if (j == 2) {
            v = __builtin_bswap32((uint32_t)a.queue_ids[m]);
        } else if (j < 7) {
            // the GUID: MessageRecord bytes 36..51
            const uint64_t r = a.records ? a.records[m] : m;
            v = a.journal[kJournalRecordDwords * r + 9 + (j - 3)];
        } else if (j == 7) {
            v = a.ws_meta[m] & 0xFFFFu;  // bytes: SchemaId, two of 0
        } else if (j == 8) {
            // the OptionHeader: Type(6) | Packed(1) | TypeSpecific(4) | Words(21)
            v = a.option_mode == 1   ? (3u << 26) | (1u << 25) | a.rda[m]   // packed SUB_QUEUE_INFOS
                : a.option_mode == 2 ? (1u << 26) | 2u                      // SUB_QUEUE_IDS_OLD
                                     : (3u << 26) | (2u << 21) | 3u;        // SUB_QUEUE_INFOS
            v = __builtin_bswap32(v);
        } else if (j == 9) {
            v = __builtin_bswap32(a.sub_ids[m]);
        } else {
            v = a.rda[m];  // bytes: the RdaInfo, three of 0 (SubQueueInfo)
        }
        ((uint32_t*)(a.dst + (a.off[m] - lead)))[j] = v;
    }
    // One message per thread and step: its padding and its entries.
    unsigned long long bad = 0, lowest = 0;
    for (uint64_t i = t0; i < a.n; i += stride) {
        const uint32_t len = a.ws_len[i], crc = a.ws_out[i], exp = a.ws_exp[i];
        const uint32_t pad = padding(len);
        uint8_t* at = a.dst + a.off[i] + len;
        // as bytes, so that no word that holds application data is read and
        // written back; four of them are a word of their own
        if (pad == 4) {
            *(uint32_t*)at = 0x04040404u;
        } else {
            for (uint32_t b = 0; b < pad; ++b) {
                at[b] = (uint8_t)pad;
            }
        }
        if (a.out) {
            a.out[i] = crc;
        }
        if (a.lengths) {
            a.lengths[i] = len;
        }
        if (crc != exp) {
            ++bad;
            lowest = max(lowest, ~(unsigned long long)i);
        }
    }
    // event e starts 8 + 32 + O bytes before its first message's data
    event_headers(a, [lead](uint64_t) { return lead; }, 0x40u | kEventPush, a.ctr[kPpkCtrTotal]);
    if (bad) {
        atomicAdd(&a.ctr[kSlotCtrBad], bad);
        atomicMax(&a.ctr[kSlotCtrFirstBad], lowest);
    }
}

}  // namespace
}  // namespace bmqcrc

using namespace bmqcrc;

extern "C" int bmqcrc_launch_push_pack_layout(const PpkArgs* a, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    const uint64_t eblocks = (a->n_events + kPackThreads - 1) / kPackThreads;
    const uint32_t check = (uint32_t)(eblocks < 1 ? 1 : eblocks > kPackBlocks ? kPackBlocks : eblocks);
    hipLaunchKernelGGL(k_ppk_classify, dim3(a->nblocks), dim3(kPackThreads), 0, s, *a);
    hipLaunchKernelGGL(k_ppk_count, dim3(a->nblocks), dim3(kPackThreads), 0, s, *a);
    hipLaunchKernelGGL(k_ppk_check, dim3(check), dim3(kPackThreads), 0, s, *a);
    hipLaunchKernelGGL(k_ppk_seal, dim3(a->nblocks), dim3(kPackThreads), 0, s, *a);
    return hipGetLastError() != hipSuccess;
}

extern "C" int bmqcrc_launch_push_pack_frame(const PpkArgs* a, void* stream)
{
    const uint64_t hdw = (kPushHeaderBytes + a->opt_bytes) / 4;
    const uint64_t work = hdw * a->n > a->n_events + 1 ? hdw * a->n : a->n_events + 1;
    const uint64_t want = (work + kPackFrameThreads - 1) / kPackFrameThreads;
    const uint32_t blocks = (uint32_t)(want > kPackFrameBlocks ? kPackFrameBlocks : want);
    hipLaunchKernelGGL(k_ppk_frame, dim3(blocks), dim3(kPackFrameThreads), 0, (hipStream_t)stream,
                       *a);
    return hipGetLastError() != hipSuccess;
}
