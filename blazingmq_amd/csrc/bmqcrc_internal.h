// bmqcrc_internal.h -- shared between the host dispatcher and the HIP kernels.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bmqcrc {

// One wave owns 64 segments; per round each segment advances one 128-byte
// line (= 32 dwords = one full turn of the 32-word fold ring).
constexpr int kLine = 128;
constexpr int kWaveLanes = 64;
constexpr int kWavesPerBlock = 4;
constexpr int kSlots = 2;                                  // LDS ring depth per wave
constexpr int kSlotBytes = kWaveLanes * kLine;             // 8 KiB per round per wave
constexpr int kLdsBytes = kWavesPerBlock * kSlots * kSlotBytes;  // 64 KiB per block
constexpr int kTabBytes = 8 * 256 * 4;  // remainder-reduction slicing tables (LDS)
constexpr int kXbBytes = 4 * 256 * 4;   // move factors x^(8 b 256^i) (LDS)
constexpr uint32_t kDefaultSegBytes = 16384;
constexpr int kPlanBlock = 1024;
constexpr int kPlanMaxBlocks = 256;  // planner grids: contiguous message ranges
constexpr int kSyncFlags = 16;       // BatchArgs::plan_sync: first arrival flag

constexpr int kBuckets = 16;            // segment size classes: floor(log2(lines))

// Experiment knobs for same-box A/B builds (tools/build_variant.sh
// -DBMQCRC_TUNE_BITS=...); the product is built with 0.  bit0 disables the
// non-temporal LDS-DMA loads, bit1 forces a 1-block/CU k_fold grid, bit3
// forces 2, bit4 always builds the size-class map (no shape prediction),
// bit5 retired, bit7 plans ragged
// batches with the round-2 pair k_plan<true> + k_plan_sort instead of the
// single-pass k_plan_map, bit9 gives planner blocks whole tiles, bit10 keeps
// two 4-wave k_fold blocks per CU with static group shares (round 3's schedule)
// instead of one 8-wave block claiming groups dynamically (A/B), bit11
// launches BMQCRC_F_PLAN batches as the speculative one-segment kernel instead
// of planning them (the cost of speculating on a stream with no history),
// bit12 plans every batch that is planned at all with k_plan_map (round 4)
// instead of the light k_plan when nothing says it is ragged.  bit8 retired.
#ifndef BMQCRC_TUNE_BITS
#define BMQCRC_TUNE_BITS 0u
#endif
constexpr uint32_t kTuneBits = BMQCRC_TUNE_BITS;
// Streams right-aligned at piece granularity when that saves a line or the
// stream is at most this many lines; longer streams otherwise keep a 128-byte
// aligned start, whose lines are whole cache lines (right-aligning every
// stream cost Zipf's k_fold 2.3 %, one line 0.5 %: profiles/r03/ab/ab3_*).
constexpr uint32_t kRightAlignLines = 1u;

struct BatchArgs {
    const uint8_t* arena;      // device
    const uint64_t* offsets;   // device, n
    const uint32_t* lengths;   // device, n
    const uint32_t* seeds;     // device, n, or nullptr (all zero)
    uint32_t* out;             // device, n
    uint32_t* seg_first;       // workspace, n: block-local exclusive prefix of segment counts
    uint32_t* block_sum;       // workspace, 3 * nblocks, per k_plan block: [segments |
                               // messages with != 1 segment | segments per message if equal
                               // for all the block's messages, else ~0]
    uint32_t* seginfo;         // workspace, max_segs: segments in size-class order, one word
                               // each (message, | kSegLast for its last segment)
    uint32_t* firstk;          // workspace, max_segs / 64 + 1: k of each group's first entry
    unsigned long long* gdesc; // workspace, max_segs / 64 + 2 (round 4): (epoch << 32) | message
    uint32_t* grec;            // workspace, 8 words per group (round 6): the prefix record
                               // {epoch, message, lanes, 0} and the suffix record, a long
                               // run's tail and head in the group (k_plan_map)
                               // for a group whose 64 seginfo slots are all full segments of
                               // one message (k_plan_map writes this instead of the 64 entries)
    uint32_t* bhist;           // workspace, kBuckets * nblocks: per-block size-class histogram
    uint64_t n;
    uint64_t max_segs;
    uint64_t per_msg;          // messages per planner block (multiple of kPlanBlock)
    uint32_t seg_bytes;
    uint32_t nblocks;          // planner blocks (<= kPlanMaxBlocks)
    uint32_t whole;            // 1: BMQCRC_F_WHOLE_MESSAGES (one segment per message, no planner)
    uint32_t blocks_per_cu;    // k_fold grid: 1 (large messages) or 2 blocks per CU
    uint32_t tune;             // experiment knobs, fixed at build time (BMQCRC_TUNE_BITS below)
    uint32_t map_planned;      // 1: k_plan builds the size-class histogram and k_plan_sort
                               //    runs before k_fold; 0: skipped (the previous batch on this
                               //    workspace was closed-form) and a ragged batch maps segments
                               //    by binary search instead -- slower, never wrong
    uint32_t* shape_hint;      // host-mapped words or nullptr: k_fold writes [0] kHintIdentity,
                               // kHintClosed or kHintRagged, the host reads it when planning
                               // the next batch; [1] the epoch of the last launch whose
                               // k_plan_map gave its map up (sticky)
    // Speculative single launch (spec = u > 0): the previous batch on this
    // workspace had u segments per message (u = 1, or u dividing 64), so no
    // planner runs and k_fold folds segment k of message m in slot m*u + k
    // (a group holds 64/u whole messages).  A message with another segment
    // count is skipped there and folded by the same wave afterwards, 64
    // segments at a time -- correct for any batch, only slower when the
    // guess was wrong.
    uint32_t spec;
    // Single-pass planner (k_plan_map): [1] the device-side launch tag of
    // graph-captured batches, [2] the epoch of a launch whose map
    // was given up (k_fold then searches seg_first), [3] how many
    // launches gave theirs up, [kSyncFlags + b] block b's arrival flag (the
    // epoch of the launch it last arrived in), then kPlanMaxBlocks x
    // (kBuckets + 3) epoch-tagged words the blocks exchange.  Zeroed once
    // when allocated.
    unsigned long long* plan_sync;
    uint32_t plan_epoch;       // k_plan_map launch tag on this workspace, in [1, 2^31); 0: the
                               // tag is plan_sync[1], advanced on the device (graph capture)
    uint32_t off32;            // 1: 32-bit offsets; the launcher picks the kernels compiled for them
    uint64_t map_wait_ticks;   // k_plan_map's grid-wide wait limit (100 MHz wall clock)
    uint32_t class_desc;       // k_plan_map: size classes in descending order (short schedules)
    // 1: plan this ragged batch with the meeting-free pair k_plan<true> +
    // k_plan_sort instead of k_plan_map (the host does so for a while after
    // a map on this workspace was given up: the GPU is shared, kPairAfterVoid)
    uint32_t pair;
    // set by the launcher: a batch of fewer groups than 4-wave blocks x CUs
    // runs its groups one per block first (group k * gridDim.x + blockIdx.x
    // for claim k) over every CU, instead of filling 4-wave blocks on a
    // quarter of them
    uint32_t spread;
    // BMQCRC_F_OFFSETS32 (ABI 2.8, off32 above): `offsets` points at n
    // uint32_t and message i starts at (uint64_t)offsets32[i] << off_shift
    uint32_t off_shift;
};

// off_shift, appended, fills what was the struct's tail padding, and off32
// (read by the launcher only) the padding after plan_epoch: no field moves,
// and neither do the arguments the compiler places after the struct (grid and
// block sizes), which a larger struct would push on in every kernel, the
// 64-bit ones included.
static_assert(sizeof(BatchArgs) == 200 && offsetof(BatchArgs, plan_epoch) == 168 &&
                  offsetof(BatchArgs, off32) == 172 && offsetof(BatchArgs, map_wait_ticks) == 176 &&
                  offsetof(BatchArgs, spread) == 192 && offsetof(BatchArgs, off_shift) == 196,
              "BatchArgs: kernel argument offsets are fixed");

// Ragged batches planned with the pair after k_fold reports a given-up map
// on the workspace (shape_hint[1] = that launch's epoch), before the
// single-pass planner is tried again.
constexpr uint32_t kPairAfterVoid = 16;

// k_fold groups per wave below which k_plan_map orders the size classes
// largest first: the schedule's tail is then one-line groups instead of a
// row of the largest ones.  Measured on Zipf shards (profiles/r03/ab/
// class_order_*.jsonl, k_fold us, ascending -> descending): 1/16 shard 278 ->
// 272, 1/8 531 -> 525, 1/4 1,036 -> 1,040, 1/2 2,051 -> 2,073, whole 4,082
// -> 4,162; the crossover lies between ~15 and ~30 groups per wave.
constexpr uint64_t kClassDescGroupsPerWave = 24;

constexpr uint32_t kPlanV = 4;  // planner: messages per thread per tile (kPlanBlock * kPlanV)
constexpr uint32_t kSegLast = 0x80000000u;  // seginfo: the entry is its message's last segment

// Ragged batches (map_planned): the single-pass k_plan_map (TUNE bit 7: the
// round-2 pair k_plan<true> + k_plan_sort instead; the pair was kept for
// single-tile blocks until the round-3 planner work made k_plan_map faster
// there too: 19.7 against 24.2 us on the 1/8 Zipf shard,
// profiles/r03/ab/planner_stamps/).
inline bool single_pass_planner(const BatchArgs& a)
{
    return !(a.tune & 128u) && !a.pair;
}

constexpr uint32_t kHintUnknown = 0;
constexpr uint32_t kHintClosed = 1;  // uniform segment counts (> 1); | (u << 8) when u divides 64
constexpr uint32_t kHintRagged = 2;
constexpr uint32_t kHintIdentity = 3;  // one segment per message

// ---- bmqcrc_crc32c_copy (crc32c_copy.hip, ABI 2.9) -------------------------
constexpr int kCopyWaves = 4;                  // k_copy_fold: waves per block
constexpr uint32_t kCopyChunkPieces = 4096;    // a wave's unit of work: 64 KiB of 16-byte pieces
constexpr uint32_t kCopyChunkBytes = 16 * kCopyChunkPieces;
constexpr int kCopyPlanThreads = 1024;         // k_copy_count / k_copy_scan block
constexpr uint32_t kCopyPlanBlocks = 256;      // their grid: contiguous message ranges, at most
// CopyArgs::ctr words
constexpr int kCopyCtrRefused = 0;    // messages refused (out of [src, src+src_bytes) or dst's)
constexpr int kCopyCtrLowestInv = 1;  // ~(lowest refused index), 0: none
constexpr int kCopyCtrOverflow = 2;   // 1: more than 2^32-1 pieces, nothing copied
constexpr int kCopyCtrWords = 4;

struct CopyArgs {
    const uint8_t* src;           // device
    uint64_t src_bytes;
    const uint64_t* src_offsets;  // device, n
    const uint32_t* lengths;      // device, n
    uint8_t* dst;                 // device
    uint64_t dst_bytes;
    const uint64_t* dst_offsets;  // device, n
    const uint32_t* seeds;        // device, n, or nullptr (all zero)
    uint32_t* out;                // device, n
    uint64_t n;
    uint32_t* first;              // workspace, n + 1: exclusive prefix of piece counts
    unsigned long long* bsum;     // workspace, kCopyPlanBlocks: pieces per pre-kernel block
    unsigned long long* ctr;      // workspace, kCopyCtrWords, zeroed before the launch
    uint64_t per_block;           // messages per pre-kernel block (multiple of kCopyPlanThreads)
    uint32_t nblocks;             // pre-kernel blocks (<= kCopyPlanBlocks)
};

// ---- bmqcrc_put_event_pack (crc32c_put_pack.hip, ABI 2.10) -----------------
constexpr int kPackThreads = 1024;         // layout kernels' block
constexpr uint32_t kPackBlocks = 256;      // their grid: contiguous message ranges, at most
constexpr int kPackFrameThreads = 256;     // k_pack_frame: one header dword per thread and step
constexpr uint32_t kPackFrameBlocks = 2048;
// ctr[] word 0 of both packers (crc32c_pack_layout.h raises it):
// ~((kind << 56) | index) of the refusal reported, 0: none
constexpr int kLayoutCtrRefusal = 0;
// PackArgs::ctr words
constexpr int kPackCtrRefusal = kLayoutCtrRefusal;
constexpr int kPackCtrTotal = 1;    // bytes of all events (k_pack_check)
constexpr int kPackCtrWords = 2;
// BMQCRC_PUT_PACK_* of bmqcrc_protocol.h, which the kernels do not include
#define BMQCRC_PACK_KIND_SRC_RANGE 1u
#define BMQCRC_PACK_KIND_EVENT_FIRST 2u
#define BMQCRC_PACK_KIND_EVENT_TOO_BIG 3u
#define BMQCRC_PACK_KIND_DST_TOO_SMALL 4u
#define BMQCRC_PACK_KIND_TOO_MANY_PIECES 5u

struct PackArgs {
    uint64_t src_bytes;
    const uint64_t* src_offsets;   // device, n
    const uint32_t* lengths;       // device, n
    const int32_t* queue_ids;      // device, n
    const uint8_t* guids;          // device, 16 n
    const uint8_t* flags;          // device, n, or nullptr (all zero)
    const uint64_t* event_first;   // device, n_events + 1, or nullptr (one event)
    uint64_t n;
    uint64_t n_events;
    uint64_t max_event_bytes;
    uint8_t* dst;                  // device, 4-byte aligned
    uint64_t dst_bytes;
    uint64_t* event_offsets;       // device, n_events + 1, or nullptr
    const uint32_t* out;           // device, n: the CRCs, final after k_copy_fold
    unsigned long long* off;       // workspace, n: block-local prefix, then data offset in dst
    unsigned long long* bsum;      // workspace, 2 * kPackBlocks: framed bytes | pieces per block
    unsigned long long* ctr;       // workspace, kPackCtrWords, zeroed before the launch
    uint64_t per_block;            // messages per layout block (multiple of kPackThreads)
    uint32_t nblocks;              // layout blocks (<= kPackBlocks)
};

// ---- bmqcrc_message_records_pack (crc32c_records_pack.hip, ABI 2.11) -------
// The layout grid and block are kPackBlocks x kPackThreads, the frame kernel's
// kPackFrameBlocks x kPackFrameThreads.  RecArgs::ctr words
constexpr int kRecCtrRefusal = kLayoutCtrRefusal;
constexpr int kRecCtrTotal = 1;     // bytes of all DATA records (k_rec_place)
constexpr int kRecCtrBad = 2;       // messages whose CRC differs from expected[]
constexpr int kRecCtrFirstBad = 3;  // ~(lowest such message), 0: none
constexpr int kRecCtrWords = 4;
// BMQCRC_REC_PACK_* of bmqcrc_protocol.h, which the kernels do not include
#define BMQCRC_REC_KIND_RECORD_TOO_BIG 1u
#define BMQCRC_REC_KIND_SRC_RANGE 2u
#define BMQCRC_REC_KIND_DST_TOO_SMALL 3u
#define BMQCRC_REC_KIND_DATA_FILE_FULL 4u
#define BMQCRC_REC_KIND_TOO_MANY_PIECES 5u
constexpr uint64_t kRecMaxFileBytes = 8ull * 0xFFFFFFFFull;  // where MessageOffsetDwords stops

struct RecArgs {
    uint64_t src_bytes;
    const uint64_t* src_offsets;   // device, n
    const uint32_t* lengths;       // device, n
    const uint8_t* queue_keys;     // device, 5 n
    const uint8_t* guids;          // device, 16 n
    const uint8_t* data_flags;     // device, n, or nullptr (all zero)
    const uint32_t* ref_counts;    // device, n, or nullptr (all 1)
    const uint64_t* timestamps;    // device, n, or nullptr (all `timestamp`)
    const uint32_t* expected;      // device, n, or nullptr (store the computed CRC)
    uint64_t n;
    uint64_t first_seq;
    uint64_t timestamp;
    uint64_t data_file_pos;        // multiple of 8, > 0
    uint32_t lease_id;
    uint32_t key_lo;               // record bytes 24..27 carry file_key[0] in the top byte
    uint32_t key_hi;               // record bytes 28..31: file_key[1..4], as stored
    uint8_t* dst;                  // device, 8-byte aligned
    uint64_t dst_bytes;
    uint8_t* journal;              // device, 4-byte aligned, 60 n bytes at least
    uint64_t* record_offsets;      // device, n + 1, or nullptr
    const uint32_t* out;           // device, n: the CRCs, final after k_copy_fold
    unsigned long long* off;       // workspace, n: block-local prefix, then data offset in dst
    unsigned long long* bsum;      // workspace, 2 * kPackBlocks: record bytes | pieces per block
    unsigned long long* ctr;       // workspace, kRecCtrWords, zeroed before the launch
    uint64_t per_block;            // messages per layout block (multiple of kPackThreads)
    uint32_t nblocks;              // layout blocks (<= kPackBlocks)
};

// ---- bmqcrc_put_event_unpack (crc32c_put_unpack.hip, ABI 2.12) -------------
constexpr int kUnpackWalkThreads = 64;        // the walks: one wave per block, one event at a time
constexpr uint32_t kUnpackWalkBlocks = 4096;  // their grid, at most: 16 waves per CU
constexpr uint32_t kUnpackWindowBytes = 1024; // a chunk of a wave's window of its event (two in LDS)
constexpr int kUnpackThreads = 1024;          // k_unpack_scan: one block
constexpr int kUnpackPublishThreads = 256;    // k_unpack_publish: one message per thread and step
constexpr uint32_t kUnpackPublishBlocks = 2048;
// ctr[] words of both unpackers (crc32c_unpack_slots.h); the last is the unit's own
constexpr int kSlotCtrRefusal = kLayoutCtrRefusal;
constexpr int kSlotCtrMsgs = 1;      // messages found: PUT events' by k_unpack_publish (0 when
                                     // refused), selected MESSAGE records by k_recunp_place
                                     // (refused or not)
constexpr int kSlotCtrBad = 2;       // slots whose computed CRC differs from the stored one
constexpr int kSlotCtrFirstBad = 3;  // ~(lowest such slot), 0: none
constexpr int kUnpCtrOffset = 4;     // the refused event's bad_off (k_unpack_publish)
constexpr int kRecUnpCtrSkipped = 4; // unselected MESSAGE records (k_recunp_place)
constexpr int kSlotCtrWords = 5;
static_assert(kSlotCtrFirstBad < kUnpCtrOffset && kUnpCtrOffset < kSlotCtrWords &&
                  kSlotCtrFirstBad < kRecUnpCtrSkipped && kRecUnpCtrSkipped < kSlotCtrWords,
              "a unit's own word lies behind the shared ones, inside the array");
// BMQCRC_PUT_UNPACK_* of bmqcrc_protocol.h, which the kernels do not include
#define BMQCRC_UNPACK_KIND_EVENT_OFFSETS 1u
#define BMQCRC_UNPACK_KIND_EVENT_HEADER 2u
#define BMQCRC_UNPACK_KIND_PUT_HEADER 3u
#define BMQCRC_UNPACK_KIND_PADDING 4u
#define BMQCRC_UNPACK_KIND_TOO_MANY_MESSAGES 5u

struct UnpackArgs {
    const uint8_t* events;          // device, 4-byte aligned
    uint64_t events_bytes;
    const uint64_t* event_offsets;  // device, n_events + 1, or nullptr (one event, the buffer)
    uint64_t n_events;
    uint64_t msg_cap;
    uint64_t* app_offsets;          // the caller's arrays (device, msg_cap; event_first n_events
    uint32_t* lengths;              // + 1): written when nothing was refused, and only by
    int32_t* queue_ids;             // k_unpack_place (queue_ids, guids, flags) and
    uint8_t* guids;                 // k_unpack_publish (the others); all but the first two
    uint8_t* flags;                 // may be nullptr
    uint32_t* expected;
    uint32_t* out;                  // nullptr: walk only, ws_out is then unused
    uint64_t* event_first;
    unsigned long long* ws_off;     // workspace, msg_cap: what the fold reads, every slot filled
    uint32_t* ws_len;               // workspace, msg_cap  by k_unpack_place (empty when unused)
    uint32_t* ws_exp;               // workspace, msg_cap: the PutHeader CRCs
    const uint32_t* ws_out;         // workspace, msg_cap: the fold's CRCs
    unsigned long long* first;      // workspace, n_events + 1: counts, then their exclusive prefix
    unsigned long long* bad_off;    // workspace, n_events: the offset an event's refusal names
    unsigned long long* ctr;        // workspace, kSlotCtrWords, zeroed before the launch
};

// ---- bmqcrc_message_records_unpack (crc32c_records_unpack.hip, ABI 2.13) ---
// The classify and place grid and block are kPackBlocks x kPackThreads over
// contiguous record ranges (layout_split), the publish kernel's
// kUnpackPublishBlocks x kUnpackPublishThreads.
constexpr uint32_t kJournalRecordDwords = 15;  // a journal record: 60 bytes
constexpr uint32_t kRecUnpMsgFlag = 0x80000000u;  // RecUnpackArgs::pre: the record takes a slot
// BMQCRC_REC_UNPACK_* of bmqcrc_protocol.h, which the kernels do not include
#define BMQCRC_RECUNP_KIND_RECORD_HEADER 1u
#define BMQCRC_RECUNP_KIND_MESSAGE_RECORD 2u
#define BMQCRC_RECUNP_KIND_DATA_OFFSET 3u
#define BMQCRC_RECUNP_KIND_DATA_RECORD 4u
#define BMQCRC_RECUNP_KIND_TOO_MANY_MESSAGES 5u

struct RecUnpackArgs {
    const uint32_t* journal;        // device, 4-byte aligned: n_records records of 15 dwords
    uint64_t n_records;
    const uint8_t* data;            // device, 8-byte aligned: the DATA-file window
    uint64_t data_bytes;
    uint64_t data_file_pos;         // byte of the DATA file that data[0] stands for
    const uint8_t* select;          // device, n_records, or nullptr (every MESSAGE record)
    uint64_t msg_cap;
    uint32_t* record_index;         // the caller's arrays (device, msg_cap): written when nothing
    uint64_t* app_offsets;          // was refused, and only by k_recunp_place (record_index,
    uint32_t* lengths;              // queue_keys, guids, data_flags, ref_counts, timestamps) and
    uint8_t* queue_keys;            // k_recunp_publish (the others); all but app_offsets and
    uint8_t* guids;                 // lengths may be nullptr
    uint8_t* data_flags;
    uint32_t* ref_counts;
    uint64_t* timestamps;
    uint32_t* expected;
    uint32_t* out;                  // nullptr: walk only, ws_out is then unused
    unsigned long long* ws_off;     // workspace, msg_cap: what the fold reads, every slot filled
    uint32_t* ws_len;               // workspace, msg_cap  by k_recunp_place (empty when unused)
    uint32_t* ws_exp;               // workspace, msg_cap: the stored CRCs
    const uint32_t* ws_out;         // workspace, msg_cap: the fold's CRCs
    uint32_t* pre;                  // workspace, n_records: kRecUnpMsgFlag | block-local prefix
    unsigned long long* rec_off;    // workspace, n_records: application data's offset in `data`,
    uint32_t* rec_len;              // its length and the DataHeader's flags byte, of the records
    uint8_t* rec_flags;             // that take a slot
    unsigned long long* bsum;       // workspace, 2 * kPackBlocks: messages | skipped per block
    unsigned long long* ctr;        // workspace, kSlotCtrWords, zeroed before the launch
    uint64_t per_block;             // records per block (multiple of kPackThreads)
    uint32_t nblocks;               // blocks (<= kPackBlocks)
};

// ---- bmqcrc_journal_select (crc32c_journal_select.hip, ABI 2.14) -----------
// The per-record kernels' grid and block are kPackBlocks x kPackThreads over
// contiguous record ranges (layout_split); k_jsel_queues is one block.  Every
// "record + 1" word below is 0 for "none", so a maximum of them is the highest
// record and a zeroed workspace is the empty state.
// JselArgs::ctr words
constexpr int kJselCtrStop = 0;       // stop + 1: the highest record that is not in the journal
constexpr int kJselCtrFail1 = 1;      // (record + 1) << 8 | -rc of the first pass's failure
constexpr int kJselCtrFail2 = 2;      // ... of the second pass's
constexpr int kJselCtrQueueOps = 3;   // entries of qlist
constexpr int kJselCtrSyncs = 4;      // entries of slist
constexpr int kJselCtrKeys = 5;       // distinct queue keys published
constexpr int kJselCtrRefused = 6;    // 1: more distinct queue keys than queue_cap
constexpr int kJselCtrFirstSync = 7;  // the lowest JOURNAL_OP record of the walk, 0 when none
constexpr int kJselCtrSelected = 8;   // the three counts over [first_record, n_records)
constexpr int kJselCtrDeleted = 9;
constexpr int kJselCtrPurged = 10;
constexpr int kJselCtrFirst = 11;     // first_record
constexpr int kJselCtrWords = 16;
// JselArgs::state values: what a MESSAGE record of the walk came to
constexpr uint8_t kJselNone = 0;      // not a MESSAGE record, not walked, or failed
constexpr uint8_t kJselLive = 1;      // eligible, its queue is live: selected unless a DELETION claims it
constexpr uint8_t kJselPurged = 2;    // below its queue's DELETION or PURGE
constexpr uint8_t kJselDead = 3;      // eligible, its queue is not live: a failure unless claimed
constexpr uint8_t kJselDeleted = 4;   // claimed by a DELETION of its GUID (k_jsel_resolve)

struct JselArgs {
    const uint32_t* journal;       // device, 4-byte aligned: n_records records of 15 dwords
    uint64_t n_records;
    uint64_t data_file_bytes;
    const uint8_t* queue_keys;     // device, 5 n_queue_keys (with_csl only)
    uint64_t n_queue_keys;
    uint64_t queue_cap;
    uint8_t* select;               // device, n_records, out
    uint32_t with_csl;
    // workspace, zeroed before the launch
    unsigned long long* ctr;       // kJselCtrWords
    unsigned long long* qkey;      // qslots: 1 << 63 | the 40-bit key, 0: empty
    uint32_t* qdel;                // qslots: record + 1 of the key's highest queue DELETION
    uint32_t* qtop;                // qslots: ... of its highest CREATION above that
    uint32_t* qpurge;              // qslots: ... of its highest whole-queue PURGE above that, when live
    uint32_t* qcsl;                // qslots: 1: the key is one of queue_keys
    uint32_t* gslot;               // gslots: record + 1 of an eligible DELETION, hashed by its GUID
    uint32_t* claim;               // n_records: at a DELETION, record + 1 of the highest MESSAGE naming it
    // workspace, written before it is read
    uint32_t* qlist;               // n_records: the QueueOp records, in no order
    uint32_t* slist;               // n_records: the JOURNAL_OP records, in no order
    uint32_t* names;               // n_records: at an eligible MESSAGE, record + 1 of the DELETION it names
    uint8_t* state;                // n_records: kJsel*
    uint64_t qslots;               // powers of two
    uint64_t gslots;
    uint64_t per_block;            // records per block (multiple of kPackThreads)
    uint32_t nblocks;              // blocks (<= kPackBlocks)
};

// ---- bmqcrc_storage_event_apply (crc32c_storage_apply.hip, ABI 2.15) -------
// The walks' grid and block are the PUT unpack's (kUnpackWalkBlocks x
// kUnpackWalkThreads, one wave per event), the per-slot layout kernels'
// kPackBlocks x kPackThreads over contiguous slot ranges (layout_split), the
// frame kernel's kPackFrameBlocks x kPackFrameThreads.  SapArgs::ctr words: the
// first four are the unpackers' (kSlotCtr*), behind them the call's own
constexpr int kSapCtrOffset = 4;     // the refusal's byte in `events` (k_sap_frame)
constexpr int kSapCtrEvent = 5;      // the refused event
constexpr int kSapCtrIndex = 6;      // the refused message
constexpr int kSapCtrData = 7;       // DATA messages
constexpr int kSapCtrTotal = 8;      // bytes of all DATA records (k_sap_check)
constexpr int kSapCtrHeadLease = 9;  // the last message's lease id and sequence number
constexpr int kSapCtrHeadSeq = 10;
constexpr int kSapCtrWords = 12;
// BMQCRC_STORAGE_APPLY_* of bmqcrc_protocol.h, which the kernels do not include
#define BMQCRC_SAP_KIND_EVENT_OFFSETS 1u
#define BMQCRC_SAP_KIND_EVENT_HEADER 2u
#define BMQCRC_SAP_KIND_STORAGE_HEADER 3u
#define BMQCRC_SAP_KIND_DATA_RECORD 4u
#define BMQCRC_SAP_KIND_TOO_MANY_MESSAGES 5u
#define BMQCRC_SAP_KIND_OUT_OF_SYNC 6u
#define BMQCRC_SAP_KIND_DST_TOO_SMALL 7u
#define BMQCRC_SAP_KIND_TOO_MANY_PIECES 8u
constexpr uint32_t kSapTypeData = 1;  // StorageMessageType::e_DATA

struct SapArgs {
    const uint8_t* events;          // device, 4-byte aligned
    uint64_t events_bytes;
    const uint64_t* event_offsets;  // device, n_events + 1, or nullptr (one event, the buffer)
    uint64_t n_events;
    uint64_t msg_cap;
    uint64_t journal_pos;           // the replica's state: byte of the journal file that
    uint64_t data_file_pos;         // journal_dst[0] stands for, of the DATA file that data_dst[0]
    uint64_t seq;                   // does, and the write head (lease_id 0: none known)
    uint32_t lease_id;
    uint32_t partition_id;
    uint8_t* journal_dst;           // device, 4-byte aligned
    uint64_t journal_dst_bytes;
    uint8_t* data_dst;              // device, 8-byte aligned
    uint64_t data_dst_bytes;
    uint8_t* types;                 // the caller's arrays (device, msg_cap; record_offsets
    uint8_t* flags;                 // msg_cap + 1, event_first n_events + 1), each may be
    uint64_t* payload_offsets;      // nullptr: written by k_sap_frame, when nothing was
    uint32_t* payload_lengths;      // refused
    uint64_t* record_offsets;
    uint32_t* lengths;
    uint32_t* expected;
    uint32_t* out;
    uint64_t* event_first;
    unsigned long long* ws_off;     // workspace, msg_cap: what the copy reads -- the application
    uint32_t* ws_len;               // data's offset in `events` and length (0 when not DATA) --
    unsigned long long* off;        // and where it goes in data_dst; every slot filled
    uint32_t* ws_exp;               // workspace, msg_cap: the MessageRecords' stored CRCs
    const uint32_t* ws_out;         // workspace, msg_cap: the copy's CRCs
    unsigned long long* ws_jrn;     // workspace, msg_cap: the journal record's offset in `events`,
    uint32_t* ws_rec;               // the DATA record's bytes R, its header + options bytes, the
    uint32_t* ws_hdr;               // bytes after the journal record, and type | flags << 8 |
    uint32_t* ws_pay;               // StorageHeader bytes << 16
    uint32_t* ws_meta;
    unsigned long long* first;      // workspace, n_events + 1: counts, then their exclusive prefix
    unsigned long long* bad_off;    // workspace, n_events: the offset an event's refusal names
    unsigned long long* bsum;       // workspace, 2 * kPackBlocks: record bytes | pieces per block
    unsigned long long* ctr;        // workspace, kSapCtrWords, zeroed before the launch
    uint64_t per_block;             // slots per layout block (multiple of kPackThreads)
    uint32_t nblocks;               // layout blocks (<= kPackBlocks)
};

// ---- bmqcrc_storage_event_pack (crc32c_storage_pack.hip, ABI 2.16) ---------
// The classify, count and seal grid and block are kPackBlocks x kPackThreads
// over contiguous record ranges (layout_split), the check kernel's one event
// per thread, the frame kernel's kPackFrameBlocks x kPackFrameThreads.
// SpkArgs::ctr words: the first four are the unpackers' (kSlotCtr*: the
// refusal, the records, the mismatches and the lowest), behind them the call's
constexpr int kSpkCtrTotal = 4;      // bytes of all events (k_spk_check)
constexpr int kSpkCtrData = 5;       // DATA messages (k_spk_frame)
constexpr int kSpkCtrWords = 6;
// BMQCRC_STORAGE_PACK_* of bmqcrc_protocol.h, which the kernels do not include
#define BMQCRC_SPK_KIND_RECORD_HEADER 1u
#define BMQCRC_SPK_KIND_DATA_OFFSET 2u
#define BMQCRC_SPK_KIND_DATA_RECORD 3u
#define BMQCRC_SPK_KIND_EVENT_FIRST 4u
#define BMQCRC_SPK_KIND_PAYLOAD_TOO_BIG 5u
#define BMQCRC_SPK_KIND_EVENT_TOO_BIG 6u
#define BMQCRC_SPK_KIND_DST_TOO_SMALL 7u
#define BMQCRC_SPK_KIND_TOO_MANY_PIECES 8u

struct SpkArgs {
    const uint32_t* journal;        // device, 4-byte aligned: n records of 15 dwords
    uint64_t n;                     // records = storage messages
    uint64_t journal_pos;           // byte of the journal file that record 0 stands for
    const uint8_t* data;            // device, 8-byte aligned: the DATA-file window
    uint64_t data_bytes;
    uint64_t data_file_pos;         // byte of the DATA file that data[0] stands for
    const uint8_t* flags;           // device, n, or nullptr (all zero)
    const uint64_t* event_first;    // device, n_events + 1, or nullptr (one event)
    uint64_t n_events;
    uint64_t max_event_bytes;
    uint64_t max_payload_bytes;
    uint32_t partition_id;
    uint32_t event_type;            // 8 or 10
    uint32_t spv;                   // StorageProtocolVersion, 2 bits
    uint8_t* dst;                   // device, 4-byte aligned
    uint64_t dst_bytes;
    uint64_t* event_offsets;        // the caller's arrays (device; n_events + 1, n, n), each may
    uint8_t* types;                 // be nullptr: written by k_spk_frame, when nothing was
    uint32_t* out;                  // refused
    unsigned long long* ws_off;     // workspace, n: what the copy reads -- the application data's
    uint32_t* ws_len;               // offset in `data` and length (0 when not a MESSAGE record) --
    unsigned long long* off;        // and where it goes in dst (before: the prefix of B)
    uint32_t* ws_exp;               // workspace, n: the MessageRecords' stored CRCs
    const uint32_t* ws_out;         // workspace, n: the copy's CRCs
    uint32_t* ws_rec;               // workspace, n: the DATA record's bytes R, its header + options
    uint32_t* ws_hdr;               // bytes, and the StorageMessageType (0: the record was
    uint8_t* ws_type;               // refused)
    unsigned long long* bsum;       // workspace, 2 * kPackBlocks: framed bytes | pieces per block
    unsigned long long* ctr;        // workspace, kSpkCtrWords, zeroed before the launch
    uint64_t per_block;             // records per layout block (multiple of kPackThreads)
    uint32_t nblocks;               // layout blocks (<= kPackBlocks)
};

// ---- bmqcrc_push_event_pack (crc32c_push_pack.hip, ABI 2.17) ---------------
// The classify, count and seal grid and block are kPackBlocks x kPackThreads
// over contiguous MESSAGE ranges (layout_split over n, not n_records: a message
// names its record), the check kernel's one event per thread, the frame
// kernel's kPackFrameBlocks x kPackFrameThreads.  PpkArgs::ctr words: the first
// four are the unpackers' (kSlotCtr*), behind them the call's
constexpr int kPpkCtrTotal = 4;      // bytes of all events (k_ppk_check)
constexpr int kPpkCtrWords = 6;      // (one spare: the copy's counters start 16-byte aligned)
constexpr uint32_t kPushHeaderBytes = 32;
// PpkArgs::ws_meta: SchemaId as its two bytes lie in memory | CAT << 16 |
// (DataHeader.flags & 1) << 19
constexpr uint32_t kPpkMetaCatShift = 16, kPpkMetaPropsBit = 1u << 19;
// BMQCRC_PUSH_PACK_* of bmqcrc_protocol.h, which the kernels do not include
#define BMQCRC_PPK_KIND_RECORD_INDEX 1u
#define BMQCRC_PPK_KIND_RECORD 2u
#define BMQCRC_PPK_KIND_DATA_OFFSET 3u
#define BMQCRC_PPK_KIND_DATA_RECORD 4u
#define BMQCRC_PPK_KIND_FLAGS 5u
#define BMQCRC_PPK_KIND_EVENT_FIRST 6u
#define BMQCRC_PPK_KIND_PAYLOAD_TOO_BIG 7u
#define BMQCRC_PPK_KIND_EVENT_TOO_BIG 8u
#define BMQCRC_PPK_KIND_DST_TOO_SMALL 9u
#define BMQCRC_PPK_KIND_TOO_MANY_PIECES 10u

struct PpkArgs {
    const uint32_t* journal;        // device, 4-byte aligned: n_records records of 15 dwords
    uint64_t n_records;
    const uint8_t* data;            // device, 8-byte aligned: the DATA-file window
    uint64_t data_bytes;
    uint64_t data_file_pos;         // byte of the DATA file that data[0] stands for
    const uint32_t* records;        // device, n, or nullptr (message m is record m)
    const int32_t* queue_ids;       // device, n
    const uint8_t* flags;           // device, n, or nullptr (all zero)
    const uint8_t* rda;             // device, n (option modes 1 and 3)
    const uint32_t* sub_ids;        // device, n (option modes 2 and 3)
    uint32_t option_mode;           // 0..3
    uint32_t opt_bytes;             // O: 0, 4, 8 or 12
    const uint64_t* event_first;    // device, n_events + 1, or nullptr (one event)
    uint64_t n;                     // messages
    uint64_t n_events;
    uint64_t max_event_bytes;
    uint64_t max_payload_bytes;
    uint8_t* dst;                   // device, 4-byte aligned; nullptr: size only
    uint64_t dst_bytes;
    uint64_t* event_offsets;        // the caller's arrays (device; n_events + 1, n, n), each may
    uint32_t* out;                  // be nullptr: written by k_ppk_frame (size only: event_offsets
    uint32_t* lengths;              // by k_ppk_seal), when nothing was refused
    unsigned long long* ws_off;     // workspace, n: what the copy reads -- the application data's
    uint32_t* ws_len;               // offset in `data` and length (0 when refused) --
    unsigned long long* off;        // and where it goes in dst (before: the prefix of B)
    uint32_t* ws_exp;               // workspace, n: the MessageRecords' stored CRCs
    const uint32_t* ws_out;         // workspace, n: the copy's CRCs
    uint32_t* ws_meta;              // workspace, n: kPpkMeta*
    unsigned long long* bsum;       // workspace, 2 * kPackBlocks: framed bytes | pieces per block
    unsigned long long* ctr;        // workspace, kPpkCtrWords, zeroed before the launch
    uint64_t per_block;             // messages per layout block (multiple of kPackThreads)
    uint32_t nblocks;               // layout blocks (<= kPackBlocks)
};

// ---- bmqcrc_partition_rollover (crc32c_rollover.hip, ABI 2.18) -------------
// The classify, count, check and seal grid and block are kPackBlocks x
// kPackThreads over contiguous record ranges (layout_split), the frame kernel's
// kPackFrameBlocks x kPackFrameThreads.  RovArgs::ctr words: the first four are
// the unpackers' (kSlotCtr*: the refusal, the kept MESSAGE records, the
// mismatches and the lowest), behind them the call's
constexpr int kRovCtrData = 4;       // bytes of all DATA records rolled (k_rov_check)
constexpr int kRovCtrKept = 5;       // records kept, the sync point not counted (k_rov_check)
constexpr int kRovCtrWords = 6;
constexpr uint64_t kRovNoSyncPoint = ~0ull;  // BMQCRC_ROLLOVER_NO_SYNC_POINT
// RovArgs::kind: what becomes of a record
constexpr uint8_t kRovDrop = 0;      // not kept
constexpr uint8_t kRovPlain = 1;     // kept, copied as it is
constexpr uint8_t kRovMessage = 2;   // kept MESSAGE record: its DATA record goes with it
constexpr uint8_t kRovQueueUri = 3;  // kept QUEUE_OP CREATION / ADDITION: the QLIST offset is zeroed
constexpr uint8_t kRovConfirm = 4;   // CONFIRM record k_rov_count decides by the join (FOLLOW mode)
// BMQCRC_ROLLOVER_* of bmqcrc_protocol.h, which the kernels do not include
#define BMQCRC_ROV_KIND_RECORD_HEADER 1u
#define BMQCRC_ROV_KIND_KEEP_JOURNAL_OP 2u
#define BMQCRC_ROV_KIND_SYNC_POINT 3u
#define BMQCRC_ROV_KIND_DATA_OFFSET 4u
#define BMQCRC_ROV_KIND_DATA_RECORD 5u
#define BMQCRC_ROV_KIND_DST_TOO_SMALL 6u
#define BMQCRC_ROV_KIND_DATA_FILE_FULL 7u
#define BMQCRC_ROV_KIND_TOO_MANY_PIECES 8u

struct RovArgs {
    const uint32_t* journal;        // device, 4-byte aligned: n records of 15 dwords
    uint64_t n;                     // records
    const uint8_t* data;            // device, 8-byte aligned: the DATA-file window
    uint64_t data_bytes;
    uint64_t data_file_pos;         // byte of the DATA file that data[0] stands for
    const uint8_t* keep;            // device, n, or nullptr (every record that may be kept)
    uint32_t follow;                // 1: BMQCRC_ROLLOVER_CONFIRMS_FOLLOW_MESSAGES
    uint64_t sync_point;            // the record restated behind the kept ones, or kRovNoSyncPoint
    uint64_t timestamp;
    uint64_t new_data_file_pos;     // byte of the new DATA file that dst[0] stands for
    uint8_t* dst;                   // device, 8-byte aligned
    uint64_t dst_bytes;
    uint32_t* journal_dst;          // device, 4-byte aligned
    uint64_t journal_dst_bytes;
    uint32_t* new_index;            // the caller's arrays (device, n), each may be nullptr:
    uint32_t* out;                  // written by k_rov_frame, when nothing was refused
    unsigned long long* ws_off;     // workspace, n: what the copy reads -- the application data's
    uint32_t* ws_len;               // offset in `data` and length (0 when not a kept MESSAGE
    unsigned long long* off;        // record) -- and where it goes in dst (before: the prefix of R)
    uint32_t* ws_exp;               // workspace, n: the MessageRecords' stored CRCs
    const uint32_t* ws_out;         // workspace, n: the copy's CRCs
    uint32_t* ws_rec;               // workspace, n: the DATA record's bytes R and its header +
    uint32_t* ws_hdr;               // options bytes
    uint8_t* kind;                  // workspace, n: kRov*
    unsigned long long* joff;       // workspace, n: the prefix of "kept", then the record's index
                                    // in the new run (~0: not kept)
    uint32_t* gslot;                // workspace, gslots, zeroed (FOLLOW mode): record + 1 of a kept
    uint64_t gslots;                // MESSAGE record, hashed by GUID and queue key; a power of two
    unsigned long long* bsum;       // workspace, 4 * kPackBlocks: R bytes | pieces | kept | (unused)
    unsigned long long* ctr;        // workspace, kRovCtrWords, zeroed before the launch
    uint64_t per_block;             // records per layout block (multiple of kPackThreads)
    uint32_t nblocks;               // layout blocks (<= kPackBlocks)
};

// ---- bmqcrc_confirm_records_pack (crc32c_confirm_records.hip, ABI 2.19) ----
// The classify and join grid and block are kPackBlocks x kPackThreads over
// contiguous record ranges (layout_split over n_records), the check and seal
// kernels' the same over contiguous confirm ranges (layout_split over n), the
// frame kernel's kPackFrameBlocks x kPackFrameThreads.  CfmArgs::ctr words
constexpr int kCfmCtrRefusal = kLayoutCtrRefusal;
constexpr int kCfmCtrWritten = 1;    // records written (k_cfm_seal)
constexpr int kCfmCtrDeletions = 2;  // DELETION records among them (k_cfm_seal)
constexpr int kCfmCtrNotFound = 3;   // confirms without a target (k_cfm_seal)
constexpr int kCfmCtrWords = 4;
constexpr uint32_t kCfmNone = 0xFFFFFFFFu;  // no target, no place
// CfmArgs::kind: what the join makes of a record of the run
constexpr uint8_t kCfmOther = 0;
constexpr uint8_t kCfmMessage = 1;   // a selected MESSAGE record: it is in the hash
constexpr uint8_t kCfmConfirm = 2;   // a CONFIRM record whose reason is not AUTO_CONFIRMED
constexpr uint8_t kCfmDeletion = 3;
constexpr uint32_t kConfirmReasonAuto = 2;  // ConfirmReason::e_AUTO_CONFIRMED
// BMQCRC_CONFIRM_PACK_* of bmqcrc_protocol.h, which the kernels do not include
#define BMQCRC_CFM_KIND_RECORD_HEADER 1u
#define BMQCRC_CFM_KIND_DUPLICATE_MESSAGE 2u
#define BMQCRC_CFM_KIND_NULL_KEY 3u
#define BMQCRC_CFM_KIND_REASON 4u
#define BMQCRC_CFM_KIND_OVER_CONFIRMED 5u
#define BMQCRC_CFM_KIND_DST_TOO_SMALL 6u

struct CfmArgs {
    const uint32_t* journal;        // device, 4-byte aligned: n_records records of 15 dwords
    uint64_t n_records;
    const uint8_t* select;          // device, n_records, or nullptr (every MESSAGE record)
    const uint8_t* guids;           // device, 16 n
    const uint8_t* queue_keys;      // device, 5 n
    const uint8_t* app_keys;        // device, 5 n, or nullptr (the null key)
    const uint8_t* reasons;         // device, n, or nullptr (all CONFIRMED)
    const uint64_t* timestamps;     // device, n, or nullptr (all `timestamp`)
    uint64_t n;                     // confirms
    uint64_t first_seq;
    uint64_t timestamp;
    uint32_t lease_id;
    uint32_t size_only;             // 1: journal_dst is null, DST_TOO_SMALL is never raised
    uint32_t* journal_dst;          // device, 4-byte aligned
    uint64_t journal_dst_bytes;
    uint8_t* status;                // the caller's arrays (device; n, n, n, n_records), each may
    uint32_t* target;               // be nullptr: written by k_cfm_frame, when nothing was
    uint32_t* new_index;            // refused
    uint32_t* left_out;
    // workspace, zeroed before the launch
    unsigned long long* ctr;        // kCfmCtrWords
    uint32_t* gslot;                // gslots: record + 1 of a selected MESSAGE record, hashed by
    uint64_t gslots;                // GUID and queue key; a power of two
    uint32_t* had;                  // n_records: CONFIRM records of the run that name the message
    uint32_t* cnt;                  // n_records: c(m), the confirms of this call that name it
    uint32_t* last;                 // n_records: the highest such confirm + 1
    uint8_t* dead;                  // n_records: 1: a DELETION record of the run names it
    // workspace, written before it is read
    uint32_t* ref;                  // n_records: the MESSAGE record's 20-bit refCount
    uint8_t* kind;                  // n_records: kCfm*
    uint32_t* hit;                  // n: the selected MESSAGE record with the confirm's key, live
                                    // or not, or kCfmNone
    unsigned long long* off;        // n: the prefix of "has a target", then the place j
    unsigned long long* bsum;       // 2 * kPackBlocks: records written | (unused) per block
    uint64_t per_block;             // records per block (multiple of kPackThreads)
    uint32_t nblocks;               // blocks over the records (<= kPackBlocks, 0: no record)
    uint32_t cnblocks;              // blocks over the confirms (<= kPackBlocks)
    uint64_t cper_block;            // confirms per block (multiple of kPackThreads)
};

// ---- bmqcrc_expire_records_pack (crc32c_expire_records.hip, ABI 2.20) ------
// The classify grid and block are kPackBlocks x kPackThreads over contiguous
// record ranges (layout_split over n_records) and, in the same blocks, over
// contiguous queue-table ranges (layout_split over n_queues); the join, front,
// check and seal kernels' the same over the records; the frame kernel's
// kPackFrameBlocks x kPackFrameThreads.  ExpArgs::ctr words
constexpr int kExpCtrRefusal = kLayoutCtrRefusal;
constexpr int kExpCtrExpired = 1;   // DELETION records written (k_exp_seal)
constexpr int kExpCtrLive = 2;      // live MESSAGE records (k_exp_seal)
constexpr int kExpCtrNoQueue = 3;   // ... of them without a table entry (k_exp_seal)
constexpr int kExpCtrWords = 4;
constexpr uint32_t kExpNone = 0xFFFFFFFFu;  // no queue, no young message, no place
constexpr uint32_t kExpLdsQueues = 2048;   // a table up to this long is reduced per block in LDS
// ExpArgs::kind: what the join makes of a record of the run
constexpr uint8_t kExpOther = 0;
constexpr uint8_t kExpMessage = 1;   // a selected MESSAGE record: it is in the hash
constexpr uint8_t kExpDeletion = 2;
constexpr uint32_t kDeletionFlagTtl = 2;  // DeletionRecordFlag::e_TTL_EXPIRATION
// BMQCRC_EXPIRE_PACK_* of bmqcrc_protocol.h, which the kernels do not include
#define BMQCRC_EXP_KIND_RECORD_HEADER 1u
#define BMQCRC_EXP_KIND_DUPLICATE_MESSAGE 2u
#define BMQCRC_EXP_KIND_QUEUE_KEY 3u
#define BMQCRC_EXP_KIND_DST_TOO_SMALL 4u

struct ExpArgs {
    const uint32_t* journal;        // device, 4-byte aligned: n_records records of 15 dwords
    uint64_t n_records;
    const uint8_t* select;          // device, n_records, or nullptr (every MESSAGE record)
    const uint8_t* queue_keys;      // device, 5 n_queues
    const uint64_t* ttl_seconds;    // device, n_queues
    uint64_t n_queues;
    uint64_t now;                   // secondsFromEpoch, and every written record's timestamp
    uint64_t first_seq;
    uint32_t lease_id;
    uint32_t size_only;             // 1: journal_dst is null, DST_TOO_SMALL is never raised
    uint32_t* journal_dst;          // device, 4-byte aligned
    uint64_t journal_dst_bytes;
    uint8_t* expired;               // the caller's arrays (device; n_records, n_records,
    uint32_t* new_index;            // n_records, n_queues, n_queues), each may be nullptr:
    uint8_t* select_out;            // written by k_exp_frame, when nothing was refused
    uint32_t* queue_expired;
    uint32_t* queue_front;
    // workspace, zeroed before the launch
    unsigned long long* ctr;        // kExpCtrWords
    uint32_t* gslot;                // gslots: record + 1 of a selected MESSAGE record, hashed by
    uint64_t gslots;                // GUID and queue key; a power of two
    uint32_t* qslot;                // qslots: entry + 1 of the queue table, hashed by its key; a
    uint64_t qslots;                // power of two (0 slots for an empty table)
    uint32_t* qcount;               // n_queues: the queue's expired messages (k_exp_seal)
    uint8_t* dead;                  // n_records: 1: a DELETION record of the run names it
    // workspace, every byte 0xFF before the launch
    uint32_t* front;                // n_queues: front(q), kExpNone without a young message
    // workspace, written before it is read
    uint32_t* queue;                // n_records: a selected MESSAGE record's entry, or kExpNone
    uint8_t* kind;                  // n_records: kExp*
    unsigned long long* off;        // n_records: the prefix of "expired", then the place j (~0:
                                    // not expired)
    unsigned long long* bsum;       // 2 * kPackBlocks: records written | (unused) per block
    uint64_t per_block;             // records per block (multiple of kPackThreads)
    uint32_t nblocks;               // blocks over the records (<= kPackBlocks)
    uint32_t qnblocks;              // blocks over the queue table (<= kPackBlocks, 0: empty)
    uint64_t qper_block;            // entries per block (multiple of kPackThreads)
};

// ---- bmqcrc_pending_records_list (crc32c_pending_list.hip, ABI 2.21) -------
// The classify grid and block are kPackBlocks x kPackThreads over contiguous
// record ranges (layout_split over n_records) and, strided over the grid, the
// queue table's n_queues + 1 app_first entries and the n_apps apps; the join, mask and emit kernels' the same over the records;
// the sort's three legs over contiguous pair ranges (layout_split over
// n_pairs); the bounds and check kernels' over the apps; the frame kernel's
// kPackFrameBlocks x kPackFrameThreads.  PndArgs::ctr words
constexpr int kPndCtrRefusal = kLayoutCtrRefusal;
constexpr int kPndCtrPending = 1;    // pairs (app, message): the sum of |list(a)| (k_pnd_total)
constexpr int kPndCtrLive = 2;       // live MESSAGE records (k_pnd_mask)
constexpr int kPndCtrNoQueue = 3;    // ... of them without a table entry (k_pnd_mask)
constexpr int kPndCtrListed = 4;     // entries a real call writes (k_pnd_check)
constexpr int kPndCtrUnknown = 5;    // CONFIRM records whose app key no app of the queue has (k_pnd_join)
constexpr int kPndCtrNotFound = 6;   // CONFIRM records without a message (k_pnd_join)
constexpr int kPndCtrWords = 8;
constexpr uint32_t kPndNone = 0xFFFFFFFFu;  // no queue
constexpr uint32_t kPndMaxApps = 32;        // apps of one queue: a message's state is one word
constexpr uint32_t kPndDigits = 256;        // the sort's radix: 8 bits a pass
// PndArgs::kind: what the join makes of a record of the run
constexpr uint8_t kPndOther = 0;
constexpr uint8_t kPndMessage = 1;   // a selected MESSAGE record: it is in the hash
constexpr uint8_t kPndDeletion = 2;
constexpr uint8_t kPndConfirm = 3;
// BMQCRC_PENDING_LIST_* of bmqcrc_protocol.h, which the kernels do not include
#define BMQCRC_PND_KIND_RECORD_HEADER 1u
#define BMQCRC_PND_KIND_DUPLICATE_MESSAGE 2u
#define BMQCRC_PND_KIND_QUEUE_KEY 3u
#define BMQCRC_PND_KIND_APP_FIRST 4u
#define BMQCRC_PND_KIND_APP_KEY 5u
#define BMQCRC_PND_KIND_FROM_RECORD 6u
#define BMQCRC_PND_KIND_LIST_TOO_SMALL 7u

struct PndArgs {
    const uint32_t* journal;        // device, 4-byte aligned: n_records records of 15 dwords
    uint64_t n_records;
    const uint8_t* select;          // device, n_records, or nullptr (every MESSAGE record)
    const uint8_t* queue_keys;      // device, 5 n_queues
    const uint64_t* app_first;      // device, n_queues + 1
    uint64_t n_queues;
    const uint8_t* app_keys;        // device, 5 n_apps
    const int32_t* queue_ids;       // device, n_apps
    const uint32_t* sub_ids;        // device, n_apps, or nullptr
    const uint32_t* from_record;    // device, n_apps, or nullptr (all 0)
    const uint32_t* limit;          // device, n_apps, or nullptr (no limit)
    uint64_t n_apps;
    uint32_t size_only;             // 1: records is null, LIST_TOO_SMALL only for 2^32 pairs
    uint32_t passes;                // 8-bit digits of n_apps - 1: the sort's passes
    uint32_t* records;              // the caller's lists (device, list_cap each; out_sub_ids may be
    int32_t* out_queue_ids;         // nullptr) and arrays (n_apps + 1, n_apps, n_apps, n_records,
    uint32_t* out_sub_ids;          // each but list_first may be nullptr): written by k_pnd_frame,
    uint64_t list_cap;              // when nothing was refused
    uint64_t* list_first;
    uint32_t* app_pending;
    uint32_t* app_next;
    uint32_t* pending_mask;
    // workspace, zeroed before the launch
    unsigned long long* ctr;        // kPndCtrWords
    uint32_t* gslot;                // gslots: record + 1 of a selected MESSAGE record, hashed by
    uint64_t gslots;                // GUID and queue key; a power of two
    uint32_t* qslot;                // qslots: entry + 1 of the queue table, hashed by its key; a
    uint64_t qslots;                // power of two (0 slots for an empty table)
    uint32_t* confirmed;            // n_records: bit `ordinal`: a CONFIRM record names the message
                                    // and that app
    uint8_t* dead;                  // n_records: 1: a DELETION record of the run names it
    // workspace, written before it is read
    uint32_t* queue;                // n_records: a selected MESSAGE record's entry, or kPndNone
    uint32_t* mask;                 // n_records: pending_mask
    uint8_t* kind;                  // n_records: kPnd*
    unsigned long long* off;        // n_records: the block-local prefix of popcount(mask)
    unsigned long long* bsum;       // 2 * kPackBlocks: pairs | (unused) per block
    uint64_t per_block;             // records per block (multiple of kPackThreads)
    uint32_t nblocks;               // blocks over the records (<= kPackBlocks)
    uint32_t cblocks;               // k_pnd_classify's grid: nblocks, or what the table's entries
                                    // and apps, strided over, ask for (<= kPackBlocks)
    // ... the sort and what follows it: sized by the host from ctr[kPndCtrPending]
    uint64_t n_pairs;               // what the workspace holds of each of the four arrays below
    uint32_t* key[2];               // n_pairs each: the pair's app, ping and pong
    uint32_t* val[2];               // n_pairs each: the pair's record
    uint32_t* hist;                 // kPndDigits * snblocks: digit-major, the scan's in and out
    uint32_t* rowsum;               // kPndDigits: the pairs of each digit (k_pnd_scan)
    uint64_t sper_block;            // pairs per block (multiple of kPackThreads)
    uint32_t snblocks;              // blocks over the pairs (<= kPackBlocks, 0: no pair)
    uint32_t anblocks;              // blocks over the apps (<= kPackBlocks, 0: no app)
    uint64_t aper_block;            // apps per block (multiple of kPackThreads)
    uint32_t* afirst;               // n_apps: first_pending(a), the app's first sorted pair
    uint32_t* acount;               // n_apps: |list(a)|
    unsigned long long* aoff;       // n_apps: the prefix of listed(a), then list_first[a]
    unsigned long long* absum;      // 2 * kPackBlocks: listed entries | (unused) per block
};

}  // namespace bmqcrc

// Launchers (crc32c_pending_list.hip).  Asynchronous on `stream`: the masks
// decide every refusal but the last kind and count the pairs, which the host
// reads to size the sort's buffers; the lists sort, bound and (unless size-only)
// store.
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_launch_pending_list_masks(const bmqcrc::PndArgs* a, void* stream);
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_launch_pending_list_lists(const bmqcrc::PndArgs* a, void* stream);

// Launchers (crc32c_expire_records.hip).  Asynchronous on `stream`: the layout
// decides everything, the frame stores; a size-only call launches the layout
// alone.
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_launch_expire_records_layout(const bmqcrc::ExpArgs* a, void* stream);
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_launch_expire_records_frame(const bmqcrc::ExpArgs* a, void* stream);

// Launchers (crc32c_confirm_records.hip).  Asynchronous on `stream`: the layout
// decides everything, the frame stores; a size-only call launches the layout
// alone.
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_launch_confirm_records_layout(const bmqcrc::CfmArgs* a, void* stream);
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_launch_confirm_records_frame(const bmqcrc::CfmArgs* a, void* stream);

// Launchers (crc32c_rollover.hip).  Asynchronous on `stream`: the layout
// before bmqcrc_launch_copy (it writes the copy's descriptors), the frame after.
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_launch_rollover_layout(const bmqcrc::RovArgs* a, void* stream);
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_launch_rollover_frame(const bmqcrc::RovArgs* a, void* stream);

// Launchers (crc32c_push_pack.hip).  Asynchronous on `stream`: the layout
// before bmqcrc_launch_copy (it writes the copy's descriptors), the frame after;
// a size-only call (dst nullptr) launches the layout alone.
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_launch_push_pack_layout(const bmqcrc::PpkArgs* a, void* stream);
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_launch_push_pack_frame(const bmqcrc::PpkArgs* a, void* stream);

// Launchers (crc32c_storage_pack.hip).  Asynchronous on `stream`: the layout
// before bmqcrc_launch_copy (it writes the copy's descriptors), the frame after.
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_launch_storage_pack_layout(const bmqcrc::SpkArgs* a, void* stream);
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_launch_storage_pack_frame(const bmqcrc::SpkArgs* a, void* stream);

// Launchers (crc32c_storage_apply.hip).  Asynchronous on `stream`: the layout
// before bmqcrc_launch_copy (it writes the copy's descriptors), the frame after.
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_launch_storage_apply_layout(const bmqcrc::SapArgs* a, void* stream);
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_launch_storage_apply_frame(const bmqcrc::SapArgs* a, void* stream);

// Launcher (crc32c_journal_select.hip): the six kernels, asynchronous on `stream`.
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_launch_journal_select(const bmqcrc::JselArgs* a, void* stream);

// Launchers (crc32c_records_unpack.hip).  Asynchronous on `stream`: the walk
// fills ws_off / ws_len for the fold (bmqcrc_launch_batch), the publish runs
// after it.
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_launch_records_unpack_walk(const bmqcrc::RecUnpackArgs* a, void* stream);
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_launch_records_unpack_publish(const bmqcrc::RecUnpackArgs* a, void* stream);

// Launchers (crc32c_put_unpack.hip).  Asynchronous on `stream`: the walk fills
// ws_off / ws_len for the fold (bmqcrc_launch_batch), the publish runs after it.
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_launch_unpack_walk(const bmqcrc::UnpackArgs* a, void* stream);
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_launch_unpack_publish(const bmqcrc::UnpackArgs* a, void* stream);

// Launchers (crc32c_records_pack.hip).  Asynchronous on `stream`: the layout
// before bmqcrc_launch_copy (it writes the copy's dst_offsets), the frame after.
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_launch_records_layout(const bmqcrc::RecArgs* a, void* stream);
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_launch_records_frame(const bmqcrc::RecArgs* a, void* stream);

// Launchers (crc32c_put_pack.hip).  Asynchronous on `stream`: the layout
// before bmqcrc_launch_copy (it writes the copy's dst_offsets), the frame after.
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_launch_put_layout(const bmqcrc::PackArgs* a, void* stream);
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_launch_put_frame(const bmqcrc::PackArgs* a, void* stream);

// Launchers (crc32c_copy.hip).  Asynchronous on `stream`.
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_launch_copy(const bmqcrc::CopyArgs* a, void* stream,
                                  uint32_t fold_blocks);
// k_copy_fold blocks one CU holds at once: its persistent grid is that times the CUs.
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_copy_occupancy(int* blocks_per_cu);

// Launchers (crc32c_kernels.hip).  All asynchronous on `stream`.
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_launch_batch(const bmqcrc::BatchArgs* a, void* stream, int num_cus,
                                   void* ev_start, void* ev_stop);
// k_plan_map blocks one CU holds at once (hipOccupancyMaxActiveBlocksPerMultiprocessor),
// of the kernel compiled for 64-bit (off32 = 0) or 32-bit offsets.
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_plan_map_occupancy(int off32, int* blocks_per_cu);
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_launch_compare(const uint32_t* got, const uint32_t* expected, uint64_t n,
                                     uint32_t* bad_count, uint32_t* bad_idx, uint32_t bad_cap,
                                     void* stream);
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_launch_blob_combine(const uint32_t* buf_crc, const uint32_t* buf_len,
                                         const uint64_t* msg_first_buf, const uint32_t* seeds,
                                         uint32_t* out, uint64_t n, void* stream);
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_launch_fill(uint8_t* dst, uint64_t nbytes, uint64_t seed, uint64_t begin,
                                  void* stream);
// Ordered mismatch list: pass 0 writes per-block counts to block_cnt, pass 1
// reads the exclusive prefix from block_cnt and writes the mismatching indices
// of ranks [skip, skip + bad_cap) in index order to bad_idx (ascending).
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_launch_compare_ordered(const uint32_t* got, const uint32_t* expected,
                                            uint64_t n, uint32_t* block_cnt, uint32_t nblocks,
                                            uint32_t* bad_idx, uint32_t skip, uint32_t bad_cap,
                                            int pass, void* stream);
// Host-buffer verify with the descriptor walk overlapped (bmqcrc_host.cpp):
// `prepare` runs on the calling thread while the arena is copied to the device
// on a helper thread; it returns 0 and the (offset, length, expected CRC)
// arrays of n messages, or a BMQCRC_E* code with the error already set.
// *offsets32 is null, or the same offsets as uint32_t in units of
// 1 << opts->offset_shift bytes (a walk over a buffer below 4 GiB writes
// both, shift 0): the device is then handed those, 4 bytes per message.
typedef int (*bmqcrc_prepare_fn)(void* ctx, const uint64_t** offsets, const uint32_t** offsets32,
                                 const uint32_t** lengths, const uint32_t** expected, uint64_t* n);
// `bad` receives the lowest min(*n_bad, bad_cap) mismatching indices, like
// bmqcrc_crc32c_verify; *n_written (if non-null) = how many were written.
// With `crcs` non-null the call computes instead of verifying: crcs = the n
// CRCs (expected, n_bad and bad are then unused).  C++ only.
#ifdef __cplusplus
#include <vector>
struct bmqcrc_opts;
__attribute__((visibility("hidden"))) int bmqcrc_verify_host_overlapped(
    const void* arena, uint64_t arena_bytes, bmqcrc_prepare_fn prepare, void* pctx,
    uint64_t* n_bad, std::vector<uint64_t>* bad, uint64_t bad_cap, const bmqcrc_opts* opts,
    std::vector<uint32_t>* crcs = nullptr, uint64_t* n_written = nullptr);
#endif
// Thread-local error message shared by every C-ABI source (bmqcrc_last_error).
extern "C" __attribute__((visibility("hidden"))) int bmqcrc_set_error(int rc, const char* msg);
extern "C" __attribute__((visibility("hidden"))) void bmqcrc_clear_error(void);
