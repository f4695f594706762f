// crc32c_storage_pack.hip -- MI355X (gfx950) primary side of replication:
// device-resident journal and DATA records packed into STORAGE events
// (bmqcrc_storage_event_pack, ABI 2.16).
//
// The device-side form of FileStore::replicateRecord with
// bmqp::StorageEventBuilder::packMessage: per record a 12-byte StorageHeader
// and the 60-byte journal record, behind a MESSAGE record its whole DATA record
// (DataHeader, options, application data, 1..8 padding bytes); per event an
// 8-byte EventHeader.  Journal records lie at fixed positions and a MESSAGE
// record names its DATA record, so every record is independent: a map, a scan
// and a scatter.  With R[i] = the DATA record's bytes (0 when not a MESSAGE
// record), B[i] = 12 + 60 + R[i] and P its 64-bit exclusive prefix, message i's
// StorageHeader lies at 8 (e(i) + 1) + P[i] and event e starts at
// 8 e + P[event_first[e]].  Five kernels on one stream around the fused copy of
// crc32c_copy.hip:
//
//   1. k_spk_classify: the grid is nblocks x kPackThreads over contiguous
//      record ranges (layout_split), one record per thread and step, staged
//      through LDS a wave's 64 records at a time (crc32c_journal_stage.h).
//      RecordHeader, record type and queue op, then for a MESSAGE record the
//      data offset and the DATA record, in k_recunp_classify's order; then the
//      payload cap.  Every record leaves its storage message type, R, header +
//      options bytes, the application data's window offset and length and the
//      stored CRC in the workspace -- an empty message when it is refused or
//      not a MESSAGE record.
//   2. k_spk_count: pass 1 of crc32c_pack_layout.h over B, and event_first's
//      shape.  (A kernel of its own: layout_count reads a message's descriptor
//      before it asks for its size, so the descriptors have to be in memory.)
//   3. k_spk_check: unless step 1 or 2 refused (every event_first entry is then
//      a valid index), every event's size against the cap and its end against
//      dst_bytes, and the pieces against the copy's limit.
//   4. k_spk_seal: off[i] becomes where message i's application data goes,
//      8 (e(i) + 1) + P[i] + 72 + header + options -- or, when anything was
//      refused, an offset past dst_bytes for EVERY record: the copy kernels
//      then refuse every message, own no piece and write neither dst nor
//      their CRCs.
//   (the payload: bmqcrc_launch_copy over the n_records slots, as it is)
//   5. k_spk_frame: unless refused, the 18 dwords of every StorageHeader and
//      journal record, indexed across the grid so that adjacent lanes store
//      adjacent dwords; DataHeader + options as dwords and the padding as
//      bytes; the EventHeaders; the caller's arrays and the mismatches.
//
// No byte outside [journal, +60 n_records) and [data, +data_bytes) is loaded:
// the journal is read by record index below n_records only; of the DATA window
// step 1 reads what data_record (crc32c_journal_stage.h) reads of a record it
// finds inside the window, and the frame reads inside that record only.
// Every size in the format is a word count, so every position in dst is a
// multiple of 4.  Nothing is stored to dst that step 3 has not shown to lie
// below dst_bytes: it checks every event's end.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmqcrc_internal.h"
#include "crc32c_journal_stage.h"
#include "crc32c_pack_layout.h"

namespace bmqcrc {
namespace {

constexpr uint32_t kStorageHeaderBytes = 12;
constexpr uint32_t kJournalBytes = 4 * kJournalRecordDwords;
constexpr uint32_t kFrameBytes = kStorageHeaderBytes + kJournalBytes;  // in front of a payload
constexpr uint32_t kFrameDwords = kFrameBytes / 4;                     // 18
// StorageMessageType (bmqp_protocol.h)
constexpr uint32_t kMsgData = 1, kMsgQlist = 2, kMsgConfirm = 3, kMsgDeletion = 4,
                   kMsgJournalOp = 5, kMsgQueueOp = 6;

// Step 1.
__global__ __launch_bounds__(kPackThreads) void k_spk_classify(SpkArgs a)
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
            uint64_t app = 0;
            uint32_t len = 0, rec = 0, hdr = 0, exp = 0, msg = 0;
            if (!record_header_ok(w0, d[1], d[2], d[14], kRecJournalOp)) {
                refuse(a, BMQCRC_SPK_KIND_RECORD_HEADER, r);
            } else if (type == kRecQueueOp) {
                const uint32_t op = __builtin_bswap32(d[8]);  // QueueOpType: PURGE 1 .. ADDITION 4
                if (op < 1 || op > 4) {
                    refuse(a, BMQCRC_SPK_KIND_RECORD_HEADER, r);
                } else {
                    msg = (op & 1u) ? kMsgQueueOp : kMsgQlist;  // CREATION 2 and ADDITION 4: QLIST
                }
            } else if (type == kRecMessage) {
                uint64_t ow;
                DataRecord dr;
                if (!data_window_offset(d[8], a.data_file_pos, end, &ow)) {
                    refuse(a, BMQCRC_SPK_KIND_DATA_OFFSET, r);
                } else if (!data_record(a.data, end, ow, &dr)) {
                    refuse(a, BMQCRC_SPK_KIND_DATA_RECORD, r);
                } else {
                    msg = kMsgData;
                    app = dr.app;
                    len = dr.len;
                    rec = (uint32_t)dr.total;  // at most 2^31 - 4
                    hdr = (uint32_t)dr.hdr;
                    exp = __builtin_bswap32(d[13]);  // MessageRecord @52
                }
            } else {
                msg = type == kRecConfirm ? kMsgConfirm : type == kRecDeletion ? kMsgDeletion
                                                                              : kMsgJournalOp;
            }
            if (msg != 0 && (uint64_t)kJournalBytes + rec > a.max_payload_bytes) {
                refuse(a, BMQCRC_SPK_KIND_PAYLOAD_TOO_BIG, r);
            }
            a.ws_off[r] = app;
            a.ws_len[r] = len;
            a.ws_rec[r] = rec;
            a.ws_hdr[r] = hdr;
            a.ws_exp[r] = exp;
            a.ws_type[r] = (uint8_t)msg;
        }
        __syncthreads();  // this step's LDS reads before the next stage
    }
}

// Step 2: the shared scan over B, then event_first's shape.
__global__ __launch_bounds__(kPackThreads) void k_spk_count(SpkArgs a)
{
    const LayoutView v = {a.ws_off, a.ws_len, a.n, a.off, a.bsum, a.ctr, a.per_block, a.nblocks};
    layout_count(v, [&a](uint64_t i, uint64_t, uint32_t) {
        return (unsigned long long)kFrameBytes + a.ws_rec[i];
    });
    event_first_shape(a, BMQCRC_SPK_KIND_EVENT_FIRST);
}

// Step 3: the events, one per thread.
__global__ __launch_bounds__(kPackThreads) void k_spk_check(SpkArgs a)
{
    // Steps 1 and 2's word: kinds up to PAYLOAD_TOO_BIG.  A higher kind is
    // raised by this pass itself and never replaces one of theirs, so the test
    // gives the same answer in every block whenever it starts.
    const unsigned long long word = a.ctr[kSlotCtrRefusal];
    if (word != 0 && (~word >> 56) <= BMQCRC_SPK_KIND_PAYLOAD_TOO_BIG) {
        return;
    }
    events_check(a, BMQCRC_SPK_KIND_EVENT_TOO_BIG, BMQCRC_SPK_KIND_DST_TOO_SMALL,
                 BMQCRC_SPK_KIND_TOO_MANY_PIECES, kSpkCtrTotal);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.ctr[kSlotCtrMsgs] = a.n;
    }
}

// Step 4: the frame in front of a record's application data is the
// StorageHeader, the journal record, DataHeader and options.
__global__ __launch_bounds__(kPackThreads) void k_spk_seal(SpkArgs a)
{
    seal_offsets(a, [&a](uint64_t i) { return kFrameBytes + a.ws_hdr[i]; });
}

// Step 5, after the copy.  The word is final: on a refusal the host reads kind
// and index from it, and the kernel leaves.
__global__ __launch_bounds__(kPackFrameThreads) void k_spk_frame(SpkArgs a)
{
    if (a.ctr[kSlotCtrRefusal] != 0) {
        return;
    }
    const uint64_t stride = (uint64_t)gridDim.x * kPackFrameThreads;
    const uint64_t t0 = (uint64_t)blockIdx.x * kPackFrameThreads + threadIdx.x;
    // Thread t of the grid owns dword t % 18 of message t / 18: three of the
    // StorageHeader, fifteen of the journal record (n < 2^32 / 15: a dword's
    // index needs 33 bits); the division in 32 bits whenever the call's
    // indices fit.
    const uint64_t ndw = (uint64_t)kFrameDwords * a.n;
    const bool narrow = ndw <= 0xFFFFFFFFull;
    for (uint64_t t = t0; t < ndw; t += stride) {
        const uint64_t m = narrow ? (uint32_t)t / kFrameDwords : t / kFrameDwords;
        const uint32_t j = (uint32_t)(t - kFrameDwords * m);
        uint32_t v;
        if (j == 0) {
            // Flags(5) | MessageWords(27): header, journal record and payload in words
            v = __builtin_bswap32(((a.flags ? (uint32_t)a.flags[m] & 0x1Fu : 0u) << 27) |
                                  (kFrameDwords + (a.ws_rec[m] >> 2)));
        } else if (j == 1) {
            // bytes: Reserved | SPV | HeaderWords 3, MessageType, PartitionId
            v = (a.spv << 4) | 3u | ((uint32_t)a.ws_type[m] << 8) |
                ((a.partition_id >> 8) << 16) | ((a.partition_id & 0xFFu) << 24);
        } else if (j == 2) {
            v = __builtin_bswap32((uint32_t)((a.journal_pos + (uint64_t)kJournalBytes * m) >> 2));
        } else {
            v = a.journal[kJournalRecordDwords * m + (j - 3)];
        }
        ((uint32_t*)(a.dst + (a.off[m] - a.ws_hdr[m] - kFrameBytes)))[j] = v;
    }
    // One record per thread and step: its DATA record's frame and its entries.
    unsigned long long bad = 0, lowest = 0, data = 0;
    for (uint64_t i = t0; i < a.n; i += stride) {
        const uint32_t type = a.ws_type[i];
        uint32_t crc = 0;
        if (type == kMsgData) {
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
            ++data;
            if (crc != exp) {
                ++bad;
                lowest = max(lowest, ~(unsigned long long)i);
            }
        }
        if (a.types) {
            a.types[i] = (uint8_t)type;
        }
        if (a.out) {
            a.out[i] = crc;
        }
    }
    // event e starts 8 + 72 + header + options bytes before its first message's data
    event_headers(a, [&a](uint64_t i) { return kFrameBytes + a.ws_hdr[i]; }, 0x40u | a.event_type,
                  a.ctr[kSpkCtrTotal]);
    data = wave_sum(data);
    if ((threadIdx.x & 63u) == 0 && data) {
        atomicAdd(&a.ctr[kSpkCtrData], data);
    }
    if (bad) {
        atomicAdd(&a.ctr[kSlotCtrBad], bad);
        atomicMax(&a.ctr[kSlotCtrFirstBad], lowest);
    }
}

}  // namespace
}  // namespace bmqcrc

using namespace bmqcrc;

extern "C" int bmqcrc_launch_storage_pack_layout(const SpkArgs* a, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    const uint64_t eblocks = (a->n_events + kPackThreads - 1) / kPackThreads;
    const uint32_t check = (uint32_t)(eblocks < 1 ? 1 : eblocks > kPackBlocks ? kPackBlocks : eblocks);
    hipLaunchKernelGGL(k_spk_classify, dim3(a->nblocks), dim3(kPackThreads), 0, s, *a);
    hipLaunchKernelGGL(k_spk_count, dim3(a->nblocks), dim3(kPackThreads), 0, s, *a);
    hipLaunchKernelGGL(k_spk_check, dim3(check), dim3(kPackThreads), 0, s, *a);
    hipLaunchKernelGGL(k_spk_seal, dim3(a->nblocks), dim3(kPackThreads), 0, s, *a);
    return hipGetLastError() != hipSuccess;
}

extern "C" int bmqcrc_launch_storage_pack_frame(const SpkArgs* a, void* stream)
{
    const uint64_t work = kFrameDwords * a->n > a->n_events + 1 ? kFrameDwords * a->n
                                                                  : a->n_events + 1;
    const uint64_t want = (work + kPackFrameThreads - 1) / kPackFrameThreads;
    const uint32_t blocks = (uint32_t)(want > kPackFrameBlocks ? kPackFrameBlocks : want);
    hipLaunchKernelGGL(k_spk_frame, dim3(blocks), dim3(kPackFrameThreads), 0, (hipStream_t)stream,
                       *a);
    return hipGetLastError() != hipSuccess;
}
