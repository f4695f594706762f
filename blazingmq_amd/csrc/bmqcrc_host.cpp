// bmqcrc_host.cpp -- C ABI implementation (include/bmqcrc.h).
//
// Device context, per-(device, stream) workspaces, host<->device staging and
// multi-GPU sharding around the HIP kernels in crc32c_kernels.hip.  The batch
// path is GPU-only: with no usable device it returns BMQCRC_ENODEV and never
// computes on the CPU.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <initializer_list>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/bmqcrc.h"
#include "../../include/bmqcrc_protocol.h"
#include "bmqcrc_internal.h"

namespace bmqcrc {
uint32_t cpu_crc32c(const void* data, uint32_t length, uint32_t crc);
uint32_t cpu_combine(uint32_t crcA, uint32_t crcB, uint64_t lenB);
}  // namespace bmqcrc

using namespace bmqcrc;

namespace {

thread_local std::string t_err;

int fail(int rc, const std::string& msg)
{
    t_err = msg;
    return rc;
}

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) {                                                             \
            return fail(e_ == hipErrorOutOfMemory ? BMQCRC_ENOMEM : BMQCRC_EIO,             \
                        std::string(#expr ": ") + hipGetErrorString(e_));                   \
        }                                                                                   \
    } while (0)

// Restores the calling thread's current HIP device on scope exit: the library
// selects the device a call targets, and a drop-in must not retarget the
// caller's later HIP/torch work on that thread.
struct DeviceGuard {
    int prev = -1;
    DeviceGuard()
    {
        if (hipGetDevice(&prev) != hipSuccess) {
            prev = -1;
        }
    }
    ~DeviceGuard()
    {
        if (prev >= 0) {
            (void)hipSetDevice(prev);
        }
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

struct DevBuf {
    void* p = nullptr;
    uint64_t bytes = 0;
    bool fresh = false;  // set when ensure() (re)allocated
    int ensure(uint64_t want)
    {
        fresh = false;
        if (want <= bytes) {
            return 0;
        }
        fresh = true;
        if (p) {
            (void)hipFree(p);
            p = nullptr;
            bytes = 0;
        }
        want = std::max<uint64_t>(want, 256);
        HIP_TRY(hipMalloc(&p, want));
        bytes = want;
        return 0;
    }
    ~DevBuf()
    {
        if (p) {
            (void)hipFree(p);
        }
    }
};

// Scratch of one device packer (bmqcrc_put_event_pack,
// bmqcrc_message_records_pack): data offsets, the copy pass's piece prefix,
// the CRCs when the caller wants none, the layout's and the copy pass's block
// sums, and the counters of the layout (ctr_words) followed by the copy
// pass's (kCopyCtrWords); the size of the last pack enqueued (bmqcrc_last_*).
struct PackScratch {
    DevBuf off, first, out, bsum, copy_bsum, ctr;
    uint64_t n = 0;
    bool any = false;
    // (first and copy_bsum are sized by enqueue_copy)
    int ensure(uint64_t n_msgs, int ctr_words, bool need_out)
    {
        int rc;
        if ((rc = ctr.ensure(8 * (ctr_words + kCopyCtrWords))) ||
            (rc = bsum.ensure(8ull * 2 * kPackBlocks)) || (rc = off.ensure(8 * n_msgs))) {
            return rc;
        }
        return need_out ? out.ensure(4 * n_msgs) : 0;
    }
};

// Scratch of one device unpacker (bmqcrc_put_event_unpack,
// bmqcrc_message_records_unpack): per slot the descriptor its fold reads
// (offset 8, length 4), the stored and the computed CRC (4 each); the
// kSlotCtrWords counters; the events or records of the last unpack enqueued
// (bmqcrc_last_*).
struct UnpackScratch {
    DevBuf off, len, exp, out, ctr;
    uint64_t n = 0;
    bool any = false;
    int ensure(uint64_t msg_cap, bool need_out, int ctr_words = kSlotCtrWords)
    {
        const uint64_t slots = std::max<uint64_t>(msg_cap, 1);
        int rc;
        if ((rc = ctr.ensure(8 * ctr_words)) || (rc = off.ensure(8 * slots)) ||
            (rc = len.ensure(4 * slots)) || (rc = exp.ensure(4 * slots))) {
            return rc;
        }
        return need_out ? out.ensure(4 * slots) : 0;
    }
};

struct Ctx;

// Scratch of one device call that copies the slots it found to where its
// layout placed them (bmqcrc_storage_event_apply, bmqcrc_storage_event_pack,
// bmqcrc_push_event_pack, bmqcrc_partition_rollover): an UnpackScratch whose
// counters are followed by the copy pass's (kCopyCtrWords); per slot the
// destination offset (8); the layout's block sums, `prefixes` pairs of
// kPackBlocks; the copy pass's piece prefix (4 a slot) and block sums.
struct SlotCopyScratch : UnpackScratch {
    DevBuf dst, bsum, copy_first, copy_bsum;
    // (copy_first and copy_bsum are sized by enqueue_copy)
    int ensure(uint64_t cap, bool need_out, int ctr_words, uint32_t prefixes = 1)
    {
        int rc;
        if ((rc = UnpackScratch::ensure(cap, need_out, ctr_words + kCopyCtrWords)) ||
            (rc = bsum.ensure(8ull * 2 * prefixes * kPackBlocks))) {
            return rc;
        }
        return dst.ensure(8 * std::max<uint64_t>(cap, 1));
    }
    // A call begins: its counters and the copy pass's zeroed on c's stream, and
    // n_units what bmqcrc_last_* reports the call was given.
    int begin(Ctx& c, int ctr_words, uint64_t n_units);
    // The slots as the copy's n_slots messages, from [src, +src_bytes) to
    // [to, +to_bytes): the descriptors are the workspace's, never the caller's.
    int enqueue_slot_copy(Ctx& c, const void* src, uint64_t src_bytes, void* to, uint64_t to_bytes,
                          uint64_t n_slots, int ctr_words);
};

// Planner + staging scratch for one (device, stream).
struct Workspace {
    std::mutex mu;
    DevBuf seg_first, block_sum, seginfo, firstk, gdesc, grec, bhist, plan_sync;
    uint32_t plan_epoch = 0;  // k_plan_map launches on this workspace (BatchArgs::plan_epoch)
    uint64_t map_wait_ticks = 10000;  // 100 us (bmqcrc_plan_wait)

    // host-pointer staging
    DevBuf arena, offsets, lengths, seeds, out;
    // verify / blobs
    DevBuf expected, vcount, vidx, vblock, buf_crc, first_buf;
    // BMQCRC_F_TIME_KERNEL: event pairs around k_fold not yet reported
    std::vector<std::pair<hipEvent_t, hipEvent_t>> timing, spare;
    // Shape of the last batch planned on this workspace, written by k_fold
    // into host-mapped memory (kHint*): after a closed-form batch the next
    // one skips the size-class histogram and the k_plan_sort launch.  A wrong guess only
    // costs speed (k_fold then maps segments by binary search).
    uint32_t* hint_host = nullptr;
    uint32_t* hint_dev = nullptr;
    // Launch plan of the last batch (bmqcrc_last_launch).
    uint32_t last_kernels = 0, last_spec = 0, last_seg = 0, last_map = 0;
    // Offset form of the last batch (bmqcrc_last_offsets): 64 or 32 bits, and the shift.
    uint32_t last_off_bits = 64, last_off_shift = 0;
    // Given-up planner maps (hint_host[1], written by k_fold): the last epoch
    // seen, and how many more ragged batches take the meeting-free pair.
    uint32_t void_seen = 0, pair_left = 0;
    // bmqcrc_crc32c_copy: its own scratch (piece prefix, block sums, counters)
    // and the size of the last copy enqueued here (bmqcrc_last_copy)
    DevBuf copy_first, copy_bsum, copy_ctr;
    uint64_t copy_n = 0;
    bool copy_any = false;
    // bmqcrc_put_event_pack and bmqcrc_message_records_pack: a set each,
    // because bmqcrc_last_put_pack and bmqcrc_last_records_pack report
    // independently; the events of the last PUT pack
    PackScratch pack, rec;
    uint64_t pack_events = 0;
    // bmqcrc_put_event_unpack and bmqcrc_message_records_unpack: a set each,
    // like the packers'.  Beside it the PUT unpack keeps per event the counts /
    // their prefix and the refusal offset (8 each); the records unpack per
    // record the message flag with the block-local prefix (4), the application
    // data's offset (8), length (4) and DataHeader flags (1), and the block sums
    UnpackScratch unp, runp;
    DevBuf unp_first, unp_bad;
    DevBuf runp_pre, runp_roff, runp_rlen, runp_rflags, runp_bsum;
    // bmqcrc_storage_event_apply, bmqcrc_storage_event_pack,
    // bmqcrc_push_event_pack and bmqcrc_partition_rollover: a set each again,
    // because their bmqcrc_last_* report independently.  Beside it:
    // the apply keeps per event what the PUT unpack keeps, per slot the journal
    // record's offset (8), the DATA record's size, its header + options size,
    // the bytes after the journal record and type | flags (4 each), and the
    // write head the last apply was given
    SlotCopyScratch sap;
    DevBuf sap_first, sap_bad, sap_jrn, sap_rec, sap_hdr, sap_pay, sap_meta;
    uint32_t sap_lease = 0;
    uint64_t sap_seq = 0;
    // the storage pack per record the DATA record's size and its header +
    // options size (4 each) and the message type (1), and the events of the
    // last pack enqueued
    SlotCopyScratch spk;
    DevBuf spk_rec, spk_hdr, spk_type;
    uint64_t spk_events = 0;
    // the push pack per message CAT, SchemaId and the properties flag (4), and
    // the events of the last pack enqueued
    SlotCopyScratch ppk;
    DevBuf ppk_meta;
    uint64_t ppk_events = 0;
    // the rollover per record the DATA record's size and its header + options
    // size (4 each), the kind (1) and the index in the new run (8); in FOLLOW
    // mode the hash of the kept MESSAGE records (8 to 16 a record, a power of
    // two); two pairs of block sums; whether the last rollover enqueued
    // restates a sync point
    SlotCopyScratch rov;
    DevBuf rov_rec, rov_hdr, rov_kind, rov_joff, rov_gslot;
    bool rov_sync = false;
    // bmqcrc_confirm_records_pack: the part of its workspace every call zeroes
    // (the counters; the hash of the selected MESSAGE records, 8 to 16 bytes a
    // record; per record had, c and last, 4 each, and dead, 1), per record the
    // refCount (4) and the kind (1), per confirm the hit (4) and the place (8),
    // the block sums; the confirms and first_seq of the last call enqueued
    DevBuf cfm_zero, cfm_rec, cfm_hit, cfm_off, cfm_bsum;
    uint64_t cfm_n = 0, cfm_first_seq = 0;
    bool cfm_any = false;
    // bmqcrc_expire_records_pack: the part of its workspace every call zeroes
    // (the counters; the hash of the selected MESSAGE records, 8 to 16 bytes a
    // record; the hash of the queue table, 8 to 16 bytes an entry; per entry
    // the expired count, 4; per record dead, 1), per entry front (4, every byte
    // 0xFF before the launch), per record the queue (4), the kind (1) and the
    // place (8), the block sums; the records and first_seq of the last call
    // enqueued
    DevBuf exp_zero, exp_front, exp_rec, exp_off, exp_bsum;
    uint64_t exp_n = 0, exp_first_seq = 0;
    bool exp_any = false;
    // bmqcrc_pending_records_list: the part of its workspace every call zeroes
    // (the counters; the two hashes as the expire call's; per record confirmed,
    // 4, and dead, 1), per record the queue and the mask (4 each), the kind (1)
    // and the prefix (8), the records' and the apps' block sums, per pair (app,
    // message) the app and the record twice (16), the sort's digit counts
    // (256 per block and 256 row totals), per app the list's start (8), its first pair and its
    // length (4 each); the records of the last call enqueued
    DevBuf pnd_zero, pnd_rec, pnd_off, pnd_bsum, pnd_pairs, pnd_hist, pnd_app;
    uint64_t pnd_n = 0;
    bool pnd_any = false;
    // bmqcrc_journal_select: the part of its workspace every call zeroes (the
    // counters, the queue-key and GUID tables, the claims) and the rest (the
    // two record lists, the named DELETIONs, the states); the records of the
    // last select enqueued (bmqcrc_last_journal_select)
    DevBuf jsel_zero, jsel_rec;
    uint64_t jsel_records = 0;
    bool jsel_any = false;
    // Pinned staging ring for gathered host buffers (bmqcrc_crc32c_gather):
    // kGatherSlots chunks of kGatherChunk bytes, each reusable once the event
    // recorded after its H2D copy has completed.
    uint8_t* pin = nullptr;
    hipEvent_t pin_ev[16] = {};
    bool pin_used[16] = {};
    ~Workspace()
    {
        if (hint_host) {
            (void)hipHostFree(hint_host);
        }
        if (pin) {
            (void)hipHostFree(pin);
        }
        for (hipEvent_t e : pin_ev) {
            if (e) {
                (void)hipEventDestroy(e);
            }
        }
        for (auto& v : {timing, spare}) {
            for (auto& e : v) {
                (void)hipEventDestroy(e.first);
                (void)hipEventDestroy(e.second);
            }
        }
    }
};

struct DeviceState {
    int num_cus = 0;
    // k_plan_map blocks the device holds at once (occupancy x CUs, at most
    // kPlanMaxBlocks): its grid never exceeds this, so on an idle GPU every
    // block is resident for the grid-wide meeting (a partitioned or smaller
    // part gets fewer, fuller blocks instead of a wait that must give up)
    // ([1]: of the kernel compiled for 32-bit offsets, which is launched then)
    uint32_t plan_resident[2] = {kPlanMaxBlocks, kPlanMaxBlocks};
    uint32_t copy_blocks = 0;  // k_copy_fold's persistent grid (occupancy x CUs), set on first use
};

std::mutex g_mu;
std::map<std::pair<int, void*>, std::unique_ptr<Workspace>> g_ws;
std::map<int, DeviceState> g_dev;

int device_count_raw()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        return 0;
    }
    return n;
}

int resolve_device(int dev, int* out)
{
    const int n = device_count_raw();
    if (n <= 0) {
        return fail(BMQCRC_ENODEV, "no HIP device available (batch CRC32C runs only on the GPU)");
    }
    if (dev < 0) {
        HIP_TRY(hipGetDevice(&dev));
    }
    if (dev >= n) {
        return fail(BMQCRC_EINVAL, "device ordinal out of range");
    }
    *out = dev;
    return 0;
}

int device_state(int dev, DeviceState** st)
{
    std::lock_guard<std::mutex> g(g_mu);
    DeviceState& s = g_dev[dev];
    if (s.num_cus == 0) {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, dev));
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
            return fail(BMQCRC_ENODEV, std::string("device is ") + prop.gcnArchName +
                                           ", this library is built for gfx950 (MI355X) only");
        }
        HIP_TRY(hipSetDevice(dev));
        for (int off32 = 0; off32 < 2; ++off32) {
            int per = 0;
            if (bmqcrc_plan_map_occupancy(off32, &per) != 0 || per <= 0) {
                return fail(BMQCRC_EIO, "k_plan_map occupancy query failed");
            }
            s.plan_resident[off32] = (uint32_t)std::min<uint64_t>(
                (uint64_t)per * (uint64_t)std::max(prop.multiProcessorCount, 1), kPlanMaxBlocks);
        }
        s.num_cus = prop.multiProcessorCount;
    }
    *st = &s;
    return 0;
}

Workspace* workspace(int dev, void* stream)
{
    std::lock_guard<std::mutex> g(g_mu);
    auto& w = g_ws[std::make_pair(dev, stream)];
    if (!w) {
        w.reset(new Workspace());
    }
    return w.get();
}

uint64_t max_segs_for(uint64_t n, uint64_t arena_bytes, uint32_t seg)
{
    // Sum over messages of ceil(len/seg) <= n + total_len/seg.  For
    // non-overlapping messages total_len <= arena_bytes; segments past this
    // bound (overlapping batches) are resolved by binary search in-kernel.
    return n + arena_bytes / seg + 64;
}

// Contiguous ranges of whole kPlanBlock tiles, at most kPlanMaxBlocks blocks.
// (As many blocks as possible: the planners are latency-bound per block.
// Fewer, fuller blocks -- at least 8 tiles each, so that the 1/8 Zipf shard
// takes the single-pass planner -- traced 36.8 against 26.3 us there,
// profiles/r03/ab/planner_block_sizing/.)
static void split_ranges(uint64_t items, uint64_t* per, uint32_t* blocks,
                         uint32_t max_blocks = kPlanMaxBlocks)
{
    const uint64_t tiles = std::max<uint64_t>((items + kPlanBlock - 1) / kPlanBlock, 1);
    const uint64_t nb = std::min<uint64_t>(
        tiles, std::max<uint32_t>(1u, std::min<uint32_t>(max_blocks, kPlanMaxBlocks)));
    uint64_t tiles_per = (tiles + nb - 1) / nb;
    if (kTuneBits & 512u) {  // A/B: whole planner tiles (kPlanV x kPlanBlock) per block
        tiles_per = (tiles_per + kPlanV - 1) / kPlanV * kPlanV;
    }
    *per = tiles_per * kPlanBlock;
    *blocks = (uint32_t)((tiles + tiles_per - 1) / tiles_per);
}

int plan_ws(Workspace* w, hipStream_t s, uint64_t n, uint64_t arena_bytes, uint32_t seg,
            BatchArgs* a, const DeviceState& st, bool off32 = false)
{
    const int num_cus = st.num_cus;
    const uint64_t max_segs = max_segs_for(n, arena_bytes, seg);
    // k_plan_map's blocks meet grid-wide: never more than the GPU holds
    split_ranges(n, &a->per_msg, &a->nblocks, st.plan_resident[off32 ? 1 : 0]);
    int rc;
    if ((rc = w->seg_first.ensure(4 * std::max<uint64_t>(n, 1))) ||
        (rc = w->block_sum.ensure(12ull * kPlanMaxBlocks)) ||
        (rc = w->seginfo.ensure(4 * max_segs)) ||
        (rc = w->firstk.ensure(4 * (max_segs / 64 + 2))) ||
        (rc = w->gdesc.ensure(8 * (max_segs / 64 + 2))) ||
        (rc = w->grec.ensure(32 * (max_segs / 64 + 2))) ||
        (rc = w->bhist.ensure(4ull * kBuckets * kPlanMaxBlocks)) ||
        (rc = w->plan_sync.ensure(8ull * (kSyncFlags + kPlanMaxBlocks +
                                          kPlanMaxBlocks * (kBuckets + 3))))) {
        return rc;
    }
    if (w->plan_sync.fresh) {  // zero counters, no given-up epoch (stream-ordered)
        HIP_TRY(hipMemsetAsync(w->plan_sync.p, 0, w->plan_sync.bytes, s));
    }
    if (w->grec.fresh) {  // no run record of any epoch either
        HIP_TRY(hipMemsetAsync(w->grec.p, 0, w->grec.bytes, s));
    }
    if (w->gdesc.fresh) {  // no group descriptor of any epoch (epochs start at 1)
        HIP_TRY(hipMemsetAsync(w->gdesc.p, 0, w->gdesc.bytes, s));
    }
    // host tags stay in [1, 2^31): a batch captured into a graph takes its
    // tags from the device instead (0x80000000 | count, k_epoch_advance)
    w->plan_epoch = w->plan_epoch % 0x7fffffffu + 1u;
    a->plan_sync = (unsigned long long*)w->plan_sync.p;
    a->plan_epoch = w->plan_epoch;
    a->map_wait_ticks = w->map_wait_ticks;
    if (!w->hint_host) {
        void* h = nullptr;
        HIP_TRY(hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocPortable |
                                          hipHostMallocCoherent));
        ((volatile uint32_t*)h)[0] = kHintUnknown;
        ((volatile uint32_t*)h)[1] = 0;  // no given-up map yet
        void* d = nullptr;
        const hipError_t e = hipHostGetDevicePointer(&d, h, 0);
        if (e != hipSuccess) {
            (void)hipHostFree(h);
            return fail(BMQCRC_EIO, std::string("hipHostGetDevicePointer: ") + hipGetErrorString(e));
        }
        w->hint_host = (uint32_t*)h;
        w->hint_dev = (uint32_t*)d;
    }
    a->shape_hint = w->hint_dev;
    {
        // expected k_fold groups per wave (max_segs bounds the segments)
        const uint64_t waves = (uint64_t)(num_cus > 0 ? num_cus : 256) * a->blocks_per_cu *
                               kWavesPerBlock;
        a->class_desc = (max_segs / 64) < kClassDescGroupsPerWave * waves ? 1u : 0u;
    }
    // seginfo entries hold 31-bit message indices (bit 31 marks a last
    // segment): larger batches map their segments by binary search
    a->map_planned = n < (1ull << 31) ? 1u : 0u;
    a->seg_first = (uint32_t*)w->seg_first.p;
    a->firstk = (uint32_t*)w->firstk.p;
    a->gdesc = (unsigned long long*)w->gdesc.p;
    a->grec = (uint32_t*)w->grec.p;
    a->block_sum = (uint32_t*)w->block_sum.p;
    a->seginfo = (uint32_t*)w->seginfo.p;
    a->bhist = (uint32_t*)w->bhist.p;
    a->max_segs = max_segs;
    return 0;
}

// 0 = automatic (auto_shape, per batch); otherwise validated here.
int check_seg(uint32_t* seg)
{
    if (*seg == 0) {
        return 0;
    }
    if (*seg % kLine != 0 || *seg < 256 || *seg > (1u << 30)) {
        return fail(BMQCRC_EINVAL, "seg_bytes must be a multiple of 128 in [256, 2^30]");
    }
    return 0;
}

struct Ctx {
    int dev = 0;
    DeviceState* st = nullptr;
    hipStream_t s = nullptr;
    Workspace* w = nullptr;
};

int open_ctx(int dev, void* user_stream, Ctx* c)
{
    int rc = device_state(dev, &c->st);
    if (rc) {
        return rc;
    }
    HIP_TRY(hipSetDevice(dev));
    c->dev = dev;
    c->s = (hipStream_t)user_stream;  // NULL: the device's default (null) stream, as in HIP
    c->w = workspace(dev, user_stream);
    return 0;
}

// The context of (device, stream) as a device call or a query names it, its
// workspace locked until the LockedCtx goes.  with_state false is for the
// queries that only read or set workspace fields: no DeviceState (no gfx950
// check, no occupancy query) and no hipSetDevice, and c->st stays null.
struct LockedCtx : Ctx {
    std::unique_lock<std::mutex> lock;
};

int lock_on(int device, void* stream, bool with_state, LockedCtx* c)
{
    int dev, rc;
    if ((rc = resolve_device(device, &dev))) {
        return rc;
    }
    if (with_state) {
        if ((rc = open_ctx(dev, stream, c))) {
            return rc;
        }
    } else {
        c->dev = dev;
        c->s = (hipStream_t)stream;
        c->w = workspace(dev, stream);
    }
    c->lock = std::unique_lock<std::mutex>(c->w->mu);
    return 0;
}

// A speculative single launch (BatchArgs::spec) is used only when every
// k_fold wave owns at least one group of 64 messages: a message longer than
// one segment is then folded by the wave that met it, and no wave is idle
// while another folds one.
bool spec_eligible(const Ctx& c, uint64_t n, uint32_t blocks_per_cu)
{
    const uint32_t per_cu = (kTuneBits & 2u) ? 1u : (kTuneBits & 8u) ? 2u : blocks_per_cu;
    const uint64_t waves = (uint64_t)(c.st->num_cus > 0 ? c.st->num_cus : 256) * per_cu *
                           kWavesPerBlock;
    return (n + 63) / 64 >= waves;
}

// Enqueue planner + fold on device pointers (caller holds c.w->mu).
// Segment size (when the caller left it at 0) and k_fold blocks per CU, from
// the batch's average message size and total bytes.  Measured on MI355X
// (profiles/r01/sweeps/, profiles/r02/seg_sweep_*.jsonl):
//  * >= 4 GiB of >= 16 KiB messages: 64 KiB segments, one 4-wave block per CU
//    (64k x 64 KiB: 620 us, the fastest shape);
//  * otherwise two blocks per CU; messages averaging >= 16 KiB get 16 KiB
//    segments when that still gives every wave slot a group of 64 (2 GiB of
//    64 KiB messages);
//  * everything else: the longest of 2 KiB, 1 KiB, 512 B, 256 B that gives
//    every wave two groups.  Segments of 4 and 8 KiB are never chosen: a wave
//    whose 64 segments start 4 or 8 KiB apart (uniform messages of those
//    sizes) streams at 0.71-0.75 of the roofline against 0.83-0.84 with
//    2 KiB segments, and Zipf 4M is within 2 % at 2, 4 and 16 KiB.
void auto_shape(uint64_t n, uint64_t arena_bytes, int num_cus, uint32_t* seg,
                uint32_t* blocks_per_cu)
{
    const uint64_t cus = (uint64_t)(num_cus > 0 ? num_cus : 256);
    const uint64_t wave_segs = (uint64_t)kWavesPerBlock * kWaveLanes;  // per block
    const bool large = n > 0 && arena_bytes / n >= kDefaultSegBytes;
    if (large && arena_bytes / (4 * kDefaultSegBytes) >= cus * wave_segs) {
        *blocks_per_cu = 1;
        if (*seg == 0) {
            *seg = 4 * kDefaultSegBytes;
        }
        return;
    }
    *blocks_per_cu = 2;
    if (*seg == 0) {
        const uint64_t slots = cus * 2 * wave_segs;
        if (large && arena_bytes / kDefaultSegBytes >= slots) {
            *seg = kDefaultSegBytes;
            return;
        }
        *seg = 256;
        for (uint32_t s : {2048u, 1024u, 512u}) {
            if (arena_bytes / s >= 2 * slots) {
                *seg = s;
                break;
            }
        }
    }
}

uint64_t max_length(const uint32_t* lengths, uint64_t n)
{
    uint32_t m = 0;
    for (uint64_t i = 0; i < n; ++i) {
        m = std::max(m, lengths[i]);
    }
    return m;
}

uint64_t min_length(const uint32_t* lengths, uint64_t n)
{
    uint32_t m = n ? UINT32_MAX : 0u;
    for (uint64_t i = 0; i < n; ++i) {
        m = std::min(m, lengths[i]);
    }
    return m;
}

// off_shift: with BMQCRC_F_OFFSETS32 in flags, bmqcrc_opts.offset_shift.
// host_max_len: the longest message when the lengths were seen on the host, or
// the caller's declared bound for device lengths (bmqcrc_opts.max_len: a
// message over it is still exact, folded by its wave's second pass)
// (host-buffer calls), UINT64_MAX when they live on the device.
int run_batch(Ctx& c, uint32_t flags, uint32_t seg, const void* arena, uint64_t arena_bytes,
              const uint64_t* offsets, const uint32_t* lengths, const uint32_t* seeds,
              uint32_t* out, uint64_t n, uint64_t host_max_len = UINT64_MAX,
              uint64_t host_min_len = 0, uint32_t off_shift = 0)
{
    Workspace* w = c.w;
    BatchArgs a;
    memset(&a, 0, sizeof(a));
    a.n = n;
    // BMQCRC_F_OFFSETS32: `offsets` points at n uint32_t (device memory)
    a.off32 = (flags & BMQCRC_F_OFFSETS32) ? 1u : 0u;
    a.off_shift = a.off32 ? off_shift : 0u;
    auto_shape(n, arena_bytes, c.st->num_cus, &seg, &a.blocks_per_cu);
    a.seg_bytes = seg;
    a.tune = kTuneBits;
    int rc;
    if (flags & BMQCRC_F_WHOLE_MESSAGES) {
        a.whole = 1;  // identity map over messages: no planner workspace
        a.max_segs = n;
    } else if ((rc = plan_ws(w, c.s, n, arena_bytes, seg, &a, *c.st, a.off32 != 0))) {
        return rc;
    } else if (!(kTuneBits & 16u) && !(flags & BMQCRC_F_PLAN)) {
        const uint32_t hint = __atomic_load_n(w->hint_host, __ATOMIC_RELAXED);
        const uint32_t shape = hint & 0xffu, hint_u = hint >> 8;
        if (shape == kHintClosed || shape == kHintIdentity) {
            a.map_planned = 0;  // last batch was closed-form: predict this one is too
        }
        if (shape == kHintIdentity && spec_eligible(c, n, a.blocks_per_cu)) {
            a.spec = 1;  // ... and one segment per message: one launch, no planner
        } else if (shape == kHintClosed && hint_u >= 2u && hint_u <= 64u && 64u % hint_u == 0u &&
                   (uint64_t)n * hint_u <= 0xFFFFFF00ull) {
            // ... and the same u segments per message, u dividing 64: every
            // group holds 64/u whole messages, so one launch needs no planner
            // and no cross-group combine (a message of another count is folded
            // by its wave's second pass, and the next batch is planned again)
            a.spec = hint_u;
        }
    }
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(c.s, &cap) == hipSuccess &&
                           cap == hipStreamCaptureStatusActive;
    // A captured launch is replayed as recorded: the light planner's "the
    // next batch gets the map" never happens inside a graph, so a capture
    // keeps the map whatever the history
    if (!(kTuneBits & (16u | 4096u)) && !capturing && !a.whole && !a.spec && a.map_planned &&
        w->hint_host &&
        (__atomic_load_n(w->hint_host, __ATOMIC_RELAXED) & 0xffu) != kHintRagged &&
        !(host_max_len != UINT64_MAX && host_max_len > a.seg_bytes &&
          (host_min_len == 0 || (host_min_len - 1) / a.seg_bytes != (host_max_len - 1) / a.seg_bytes))) {
        // Planned with no evidence that the batch is ragged -- no shape
        // history on the stream, or BMQCRC_F_PLAN after a closed-form batch
        // (segment counts seen on the host decide for host batches): the
        // light k_plan (counts and closed forms, no size-class map).  A
        // ragged batch is then folded by searching seg_first, and k_fold
        // records its shape, so the stream's next batch gets the map
        // (planned steps: 1M x 256 B 0.055 against 0.066 ms, 1k x 4 KiB 0.013
        // against 0.017; a ragged first batch 1.09x: Zipf 4.45 against 4.07;
        // profiles/r05/ab/light_planner.jsonl; TUNE bit 12 restores round 4)
        a.map_planned = 0;
    }
    if ((kTuneBits & 2048u) && !a.whole && (flags & BMQCRC_F_PLAN) &&
        spec_eligible(c, n, a.blocks_per_cu)) {
        // A/B only (TUNE bit 11): a batch with no shape history launched as
        // the speculative one-segment kernel instead of being planned (its
        // second pass folds the longer messages); bench.py's planned leg
        // then prices that choice
        a.spec = 1;
    } else if (!a.whole && host_max_len <= a.seg_bytes && !(flags & BMQCRC_F_PLAN)) {
        a.spec = 1;  // known, not guessed: every message is one segment
    } else if (!a.whole && host_min_len > 0 && host_max_len != UINT64_MAX &&
               !(flags & BMQCRC_F_PLAN)) {
        // every length in [min, max] has the same u segments, u dividing 64:
        // the speculative uniform launch, known instead of guessed
        const uint64_t u = (host_max_len - 1) / a.seg_bytes + 1;
        if ((host_min_len - 1) / a.seg_bytes + 1 == u && u >= 2 && u <= 64 && 64 % u == 0 &&
            (uint64_t)n * u <= 0xFFFFFF00ull) {
            a.spec = (uint32_t)u;
        }
    }
    if (!a.whole && !a.spec && a.map_planned && w->hint_host && w->map_wait_ticks != 0) {
        // (a zero limit is the test hook that gives every map up: no switch)
        // a map given up since the last look (k_fold's sticky epoch word):
        // the GPU is shared with other streams or processes, whose resident
        // kernels keep k_plan_map's blocks from meeting, so the next
        // kPairAfterVoid ragged batches here are planned by the pair, which
        // needs no co-residency (Zipf 4M: ~76 against ~54 us)
        const uint32_t voided = __atomic_load_n(w->hint_host + 1, __ATOMIC_RELAXED);
        if (voided != w->void_seen) {
            w->void_seen = voided;
            w->pair_left = kPairAfterVoid;
        }
        if (w->pair_left) {
            a.pair = 1;
            --w->pair_left;
        }
    }
    if (!a.whole && !a.spec && a.map_planned) {
        // inside a graph capture every replay must tag its planner words
        // afresh: the tag then lives on the device (BatchArgs::plan_epoch 0)
        if (capturing) {
            a.plan_epoch = 0;
        }
    }
    a.arena = (const uint8_t*)arena;
    a.offsets = offsets;
    a.lengths = lengths;
    a.seeds = seeds;
    a.out = out;
    void* ev0 = nullptr;
    void* ev1 = nullptr;
    if (flags & BMQCRC_F_TIME_KERNEL) {
        std::pair<hipEvent_t, hipEvent_t> ev;
        if (!w->spare.empty()) {
            ev = w->spare.back();
            w->spare.pop_back();
        } else {
            HIP_TRY(hipEventCreate(&ev.first));
            HIP_TRY(hipEventCreate(&ev.second));
        }
        w->timing.push_back(ev);
        ev0 = (void*)ev.first;
        ev1 = (void*)ev.second;
    }
    if (bmqcrc_launch_batch(&a, (void*)c.s, c.st->num_cus, ev0, ev1) != 0) {
        return fail(BMQCRC_EIO, std::string("kernel launch failed: ") +
                                    hipGetErrorString(hipGetLastError()));
    }
    w->last_spec = a.whole ? 1u : a.spec;
    w->last_seg = a.seg_bytes;
    w->last_kernels = n == 0                 ? 0u
                      : (a.whole || a.spec)  ? 1u
                      : !a.map_planned       ? 2u
                      : single_pass_planner(a) ? 2u
                                             : 3u;
    w->last_map = n != 0 && !a.whole && !a.spec && a.map_planned ? 1u : 0u;
    w->last_off_bits = a.off32 ? 32u : 64u;
    w->last_off_shift = a.off_shift;
    return 0;
}

// Stage host arrays into workspace buffers (async on c.s).
int stage(Ctx& c, DevBuf& buf, const void* host, uint64_t bytes)
{
    int rc = buf.ensure(bytes + 16);
    if (rc) {
        return rc;
    }
    if (bytes) {
        HIP_TRY(hipMemcpyAsync(buf.p, host, bytes, hipMemcpyHostToDevice, c.s));
    }
    return 0;
}

// Bytes of a batch's n offsets: 32-bit ones are staged as they are, 4 bytes each.
uint64_t offsets_bytes(uint32_t flags, uint64_t n)
{
    return ((flags & BMQCRC_F_OFFSETS32) ? 4 : 8) * n;
}

// Where a batch's arrays lie on the device.
struct DevArrays {
    const void* arena;
    const uint64_t* offsets;
    const uint32_t* lengths;
    const uint32_t* seeds;
};

// Stage a host batch's arrays into the workspace (async on c.s; caller holds
// c.w->mu).  arena_staged: the arena's bytes are in c.w->arena already, and
// `arena` is not read.  seeds may be null.
int stage_batch(Ctx& c, uint32_t flags, bool arena_staged, const void* arena,
                uint64_t arena_bytes, const void* offsets, const uint32_t* lengths,
                const uint32_t* seeds, uint64_t n, DevArrays* d)
{
    Workspace* w = c.w;
    int rc;
    if ((!arena_staged && (rc = stage(c, w->arena, arena, arena_bytes))) ||
        (rc = stage(c, w->offsets, offsets, offsets_bytes(flags, n))) ||
        (rc = stage(c, w->lengths, lengths, 4 * n)) ||
        (seeds && (rc = stage(c, w->seeds, seeds, 4 * n)))) {
        return rc;
    }
    d->arena = w->arena.p;
    d->offsets = (const uint64_t*)w->offsets.p;
    d->lengths = (const uint32_t*)w->lengths.p;
    d->seeds = seeds ? (const uint32_t*)w->seeds.p : nullptr;
    return 0;
}

// One fold over host arrays (caller holds c.w->mu): stage them, run_batch,
// copy the n CRCs back to `out` (host) and synchronise.  run_batch is told the
// longest message and, with min_too, the shortest: the two bounds together
// select its speculative uniform launch, so min_too changes which kernel runs.
// (The bounds are taken after the copies are enqueued, while those run.)
int fold_staged(Ctx& c, uint32_t flags, uint32_t seg, bool arena_staged, const void* arena,
                uint64_t arena_bytes, const void* offsets, const uint32_t* lengths,
                const uint32_t* seeds, uint64_t n, bool min_too, uint32_t off_shift,
                uint32_t* out)
{
    DevArrays d;
    int rc;
    if ((rc = stage_batch(c, flags, arena_staged, arena, arena_bytes, offsets, lengths, seeds, n,
                          &d)) ||
        (rc = c.w->out.ensure(4 * n)) ||
        (rc = run_batch(c, flags, seg, d.arena, arena_bytes, d.offsets, d.lengths, d.seeds,
                        (uint32_t*)c.w->out.p, n, max_length(lengths, n),
                        min_too ? min_length(lengths, n) : 0, off_shift))) {
        return rc;
    }
    HIP_TRY(hipMemcpyAsync(out, c.w->out.p, 4 * n, hipMemcpyDeviceToHost, c.s));
    HIP_TRY(hipStreamSynchronize(c.s));
    return 0;
}

// declared_max / declared_min: the caller's bounds on every length of a
// device-resident batch (bmqcrc_opts.max_len / min_len, 0 = none); host
// batches use the lengths they hold.
int batch_one(int dev, void* user_stream, uint32_t flags, uint32_t seg, const void* arena,
              uint64_t arena_bytes, const uint64_t* offsets, const uint32_t* lengths,
              const uint32_t* seeds, uint32_t* out, uint64_t n, uint32_t declared_max = 0,
              uint32_t declared_min = 0, uint32_t off_shift = 0)
{
    Ctx c;
    int rc = open_ctx(dev, user_stream, &c);
    if (rc) {
        return rc;
    }
    Workspace* w = c.w;
    std::lock_guard<std::mutex> g(w->mu);
    const bool dev_ptrs = (flags & BMQCRC_F_DEVICE_PTRS) != 0;
    if (dev_ptrs) {
        if ((rc = run_batch(c, flags, seg, arena, arena_bytes, offsets, lengths, seeds, out, n,
                            declared_max ? (uint64_t)declared_max : UINT64_MAX,
                            declared_max ? std::min(declared_min, declared_max) : 0u,
                            off_shift))) {
            return rc;
        }
        if (!(flags & BMQCRC_F_ASYNC)) {
            HIP_TRY(hipStreamSynchronize(c.s));
        }
        return 0;
    }
    return fold_staged(c, flags, seg, false, arena, arena_bytes, offsets, lengths, seeds, n, true,
                       off_shift, out);
}

// The caller's bmqcrc_opts (null: the defaults) as the current layout, read
// by its struct_size.
void read_opts(const bmqcrc_opts* opts, bmqcrc_opts* o)
{
    memset(o, 0, sizeof(*o));
    o->device = -1;
    if (opts) {
        // struct_size 0 reads only the ABI 2.0 fields: a caller that never set
        // it may be built against any earlier, shorter layout
        // (ABI 2.7: nothing past offsetof(ndevices) is read then, not even to
        // check it -- a 2.0 caller's struct ends there)
        const size_t given = opts->struct_size ? opts->struct_size : offsetof(bmqcrc_opts, ndevices);
        memcpy(o, opts, std::min<size_t>(sizeof(*o), given));
        o->struct_size = sizeof(*o);
    }
}

// offsets32_ok: the entry point takes BMQCRC_F_OFFSETS32 (batch and verify).
int parse_opts(const bmqcrc_opts* opts, bmqcrc_opts* o, uint32_t* seg, int* dev,
               bool offsets32_ok = false)
{
    read_opts(opts, o);
    *seg = o->seg_bytes;
    const uint32_t known = BMQCRC_F_DEVICE_PTRS | BMQCRC_F_ASYNC | BMQCRC_F_TIME_KERNEL |
                           BMQCRC_F_WHOLE_MESSAGES | BMQCRC_F_PLAN | BMQCRC_F_OFFSETS32;
    if (o->flags & ~known) {
        return fail(BMQCRC_EINVAL, "unknown bmqcrc_opts.flags bits");
    }
    // (a caller whose struct ends before offset_shift has 0 from the memset)
    if ((o->flags & BMQCRC_F_OFFSETS32) && !offsets32_ok) {
        return fail(BMQCRC_EINVAL,
                    "BMQCRC_F_OFFSETS32 applies to bmqcrc_crc32c_batch and bmqcrc_crc32c_verify only");
    }
    if (o->offset_shift && !(o->flags & BMQCRC_F_OFFSETS32)) {
        return fail(BMQCRC_EINVAL, "bmqcrc_opts.offset_shift needs BMQCRC_F_OFFSETS32");
    }
    if (o->offset_shift > 7) {
        return fail(BMQCRC_EINVAL, "bmqcrc_opts.offset_shift must be in [0, 7]");
    }
    int rc;
    if ((rc = check_seg(seg)) || (rc = resolve_device(o->device, dev))) {
        return rc;
    }
    return 0;
}

// A host batch's offsets in either form (BMQCRC_F_OFFSETS32: p32, shift),
// read in 64 bits: off << shift.
struct Offsets {
    const uint64_t* p64;
    const uint32_t* p32;
    uint32_t shift;
    uint64_t operator[](uint64_t i) const
    {
        return p32 ? (uint64_t)p32[i] << shift : p64[i];
    }
};

Offsets offsets_of(const bmqcrc_opts& o, const uint64_t* offsets)
{
    if (o.flags & BMQCRC_F_OFFSETS32) {
        return Offsets{nullptr, (const uint32_t*)offsets, o.offset_shift};
    }
    return Offsets{offsets, nullptr, 0u};
}

// Bytes [off, off+len) do not lie inside an arena of arena_bytes.
bool outside(uint64_t off, uint32_t len, uint64_t arena_bytes)
{
    return off > arena_bytes || len > arena_bytes - off;
}

int check_ranges(const Offsets& of, const uint32_t* lengths, uint64_t n, uint64_t arena_bytes)
{
    for (uint64_t i = 0; i < n; ++i) {
        if (outside(of[i], lengths[i], arena_bytes)) {
            return fail(BMQCRC_EINVAL,
                        "message " + std::to_string(i) + " lies outside [arena, arena+arena_bytes)");
        }
    }
    return 0;
}

// Device mismatch-index list of a verify: 4 Mi entries (16 MiB) at most.
constexpr uint64_t kVerifyListCap = 1ull << 22;

// The message arrays of a plain verify call, handed to verify_host_multi as
// an already finished "walk".
struct GivenArrays {
    const uint64_t* off;
    const uint32_t* off32;  // BMQCRC_F_OFFSETS32: the caller's array, `off` is null
    const uint32_t* len;
    const uint32_t* exp;
    uint64_t n;
};

int given_arrays(void* ctx, const uint64_t** off, const uint32_t** off32, const uint32_t** len,
                 const uint32_t** exp, uint64_t* n)
{
    const GivenArrays* g = (const GivenArrays*)ctx;
    *off = g->off;
    *off32 = g->off32;
    *len = g->len;
    *exp = g->exp;
    *n = g->n;
    return 0;
}

// The verify pipeline after the workspace lock: stage (host buffers; the
// arena may already be staged), fold, compare on the device, collect the
// lowest mismatching indices.  With BMQCRC_F_OFFSETS32 in o.flags `offsets`
// points at n uint32_t in units of 1 << o.offset_shift bytes.
int verify_locked(Ctx& c, Workspace* w, const bmqcrc_opts& o, uint32_t seg, bool arena_staged,
                  const void* arena, uint64_t arena_bytes, const uint64_t* offsets,
                  const uint32_t* lengths, const uint32_t* expected, uint64_t n, uint64_t* n_bad,
                  uint64_t* bad_idx, uint64_t bad_cap, uint64_t* n_written)
{
    int rc;
    const bool dev_ptrs = (o.flags & BMQCRC_F_DEVICE_PTRS) != 0;
    // The device list holds at most kVerifyListCap indices (16 MiB), whatever
    // bad_cap is; a longer answer is taken in windows of that size, so exactly
    // min(n_bad, bad_cap) indices are still written.
    const uint64_t want = std::min<uint64_t>(bad_cap, n);
    const uint32_t cap = (uint32_t)std::min<uint64_t>(want, kVerifyListCap);
    if (n_written) {
        *n_written = 0;
    }
    if ((rc = w->out.ensure(4 * n)) || (rc = w->vcount.ensure(4)) ||
        (rc = w->vidx.ensure(4ull * std::max<uint32_t>(cap, 1)))) {
        return rc;
    }
    DevArrays d = {arena, offsets, lengths, nullptr};
    const uint32_t* d_exp = expected;
    if (!dev_ptrs) {
        if ((rc = stage_batch(c, o.flags, arena_staged, arena, arena_bytes, offsets, lengths,
                              nullptr, n, &d)) ||
            (rc = stage(c, w->expected, expected, 4 * n))) {
            return rc;
        }
        d_exp = (const uint32_t*)w->expected.p;
    }
    if ((rc = run_batch(c, o.flags, seg, d.arena, arena_bytes, d.offsets, d.lengths, nullptr,
                        (uint32_t*)w->out.p, n,
                        dev_ptrs ? UINT64_MAX : max_length(lengths, n), 0, o.offset_shift))) {
        return rc;
    }
    HIP_TRY(hipMemsetAsync(w->vcount.p, 0, 4, c.s));
    if (bmqcrc_launch_compare((const uint32_t*)w->out.p, d_exp, n, (uint32_t*)w->vcount.p,
                              (uint32_t*)w->vidx.p, cap, (void*)c.s)) {
        return fail(BMQCRC_EIO, "compare launch failed");
    }
    uint32_t cnt = 0;
    HIP_TRY(hipMemcpyAsync(&cnt, w->vcount.p, 4, hipMemcpyDeviceToHost, c.s));
    HIP_TRY(hipStreamSynchronize(c.s));
    *n_bad = cnt;
    const uint64_t take = std::min<uint64_t>(cnt, want);
    if (take && cnt <= cap) {
        // the single pass kept every mismatch: sort the short list
        std::vector<uint32_t> idx(take);
        HIP_TRY(hipMemcpyAsync(idx.data(), w->vidx.p, 4ull * take, hipMemcpyDeviceToHost, c.s));
        HIP_TRY(hipStreamSynchronize(c.s));
        std::sort(idx.begin(), idx.end());
        for (uint64_t k = 0; k < take; ++k) {
            bad_idx[k] = idx[k];
        }
    } else if (take) {
        // more mismatches than device slots: the single pass kept an arbitrary
        // subset, so rebuild the list in index order, one window at a time
        const uint32_t nb = (uint32_t)std::min<uint64_t>((n + 255) / 256, 4096);
        if ((rc = w->vblock.ensure(4ull * nb))) {
            return rc;
        }
        uint32_t* d_blk = (uint32_t*)w->vblock.p;
        if (bmqcrc_launch_compare_ordered((const uint32_t*)w->out.p, d_exp, n, d_blk, nb,
                                          nullptr, 0, cap, 0, (void*)c.s)) {
            return fail(BMQCRC_EIO, "ordered compare launch failed");
        }
        std::vector<uint32_t> blk(nb);
        HIP_TRY(hipMemcpyAsync(blk.data(), d_blk, 4ull * nb, hipMemcpyDeviceToHost, c.s));
        HIP_TRY(hipStreamSynchronize(c.s));
        uint64_t run = 0;
        for (uint32_t b = 0; b < nb; ++b) {
            const uint32_t k = blk[b];
            blk[b] = (uint32_t)std::min<uint64_t>(run, 0xFFFFFFFFu);
            run += k;
        }
        HIP_TRY(hipMemcpyAsync(d_blk, blk.data(), 4ull * nb, hipMemcpyHostToDevice, c.s));
        std::vector<uint32_t> idx(cap);
        for (uint64_t skip = 0; skip < take; skip += cap) {
            const uint32_t m = (uint32_t)std::min<uint64_t>(cap, take - skip);
            if (bmqcrc_launch_compare_ordered((const uint32_t*)w->out.p, d_exp, n, d_blk, nb,
                                              (uint32_t*)w->vidx.p, (uint32_t)skip, m, 1,
                                              (void*)c.s)) {
                return fail(BMQCRC_EIO, "ordered compare launch failed");
            }
            HIP_TRY(hipMemcpyAsync(idx.data(), w->vidx.p, 4ull * m, hipMemcpyDeviceToHost, c.s));
            HIP_TRY(hipStreamSynchronize(c.s));  // also: blk is read by the async H2D copy
            for (uint32_t k = 0; k < m; ++k) {
                bad_idx[skip + k] = idx[k];
            }
        }
    }
    if (n_written) {
        *n_written = take;
    }
    return 0;
}

// Library-owned stream k of a device (a device listed twice in
// bmqcrc_opts.devices gets two streams, hence two workspaces).
int internal_stream(int dev, int k, hipStream_t* out)
{
    static std::map<std::pair<int, int>, hipStream_t> streams;
    std::lock_guard<std::mutex> g(g_mu);
    hipStream_t& s = streams[std::make_pair(dev, k)];
    if (!s) {
        HIP_TRY(hipSetDevice(dev));
        HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    }
    *out = s;
    return 0;
}

// The device ordinals of a multi-device call, one per entry of `devs`
// (devices == NULL: 0, 1, ...), each below `have`; with no device (have <= 0)
// only their sign is checked, and the caller decides what a missing device
// means.
int device_list(const int* devices, int have, std::vector<int>* devs)
{
    for (size_t d = 0; d < devs->size(); ++d) {
        const int dev = devices ? devices[d] : (int)d;
        if (dev < 0 || (have > 0 && dev >= have)) {
            return fail(BMQCRC_EINVAL, "device ordinal out of range");
        }
        (*devs)[d] = dev;
    }
    return 0;
}

// bmqcrc_verify_host_overlapped over several devices (bmqcrc_opts.ndevices >
// 1): the arena is cut into ndevices contiguous byte ranges; one thread per
// range copies it to its device over that device's PCIe link while the
// calling thread walks the format, then verifies (or computes) the messages
// lying wholly inside its range.  The few messages that straddle a cut are
// gathered into a small arena and done by the first range's thread
// afterwards.  Results are merged in message order: n_bad is the sum, `bad`
// the lowest min(n_bad, bad_cap) indices overall.
int verify_host_multi(const void* arena, uint64_t arena_bytes, bmqcrc_prepare_fn prepare,
                      void* pctx, uint64_t* n_bad, std::vector<uint64_t>* bad, uint64_t bad_cap,
                      const bmqcrc_opts& o, uint32_t seg, std::vector<uint32_t>* crcs,
                      uint64_t* n_written)
{
    const uint32_t nd = o.ndevices;
    if (nd > 64) {
        return fail(BMQCRC_EINVAL, "at most 64 device listings");
    }
    const int have = device_count_raw();
    std::vector<int> devs(nd);
    if (const int drc = device_list(o.devices, have, &devs)) {
        return drc;
    }
    const uint64_t* off64 = nullptr;
    const uint32_t* off32 = nullptr;
    const uint32_t* len = nullptr;
    const uint32_t* exp = nullptr;
    uint64_t n = 0;
    // the messages' offsets in the form `prepare` gives (both: the 32-bit one)
    Offsets off = {nullptr, nullptr, o.offset_shift};
    if (have <= 0) {
        // no usable device: a malformed input is still reported first
        const int prc = prepare(pctx, &off64, &off32, &len, &exp, &n);
        if (prc || n == 0) {
            return prc;
        }
        return fail(BMQCRC_ENODEV, "no HIP device available (batch CRC32C runs only on the GPU)");
    }
    std::vector<uint64_t> cut(nd + 1, arena_bytes);
    cut[0] = 0;
    for (uint32_t d = 1; d < nd; ++d) {
        cut[d] = (arena_bytes / nd * d) & ~127ull;
    }
    std::vector<int> rcs(nd, 0);
    std::vector<std::string> errs(nd);
    std::vector<uint64_t> nb(nd, 0);
    std::vector<std::vector<uint64_t>> bads(nd);
    std::vector<uint32_t> owner;  // per message: its range, or nd (straddles a cut)
    std::mutex mu;
    std::condition_variable cv;
    bool walked = false, walk_ok = false;
    auto slice = [&](uint32_t t) {
        const int dev = devs[t];
        hipStream_t st = nullptr;
        Ctx c;
        int rc = internal_stream(dev, (int)t, &st);
        if (!rc) {
            rc = open_ctx(dev, (void*)st, &c);
        }
        std::unique_lock<std::mutex> lk;
        if (!rc) {
            lk = std::unique_lock<std::mutex>(c.w->mu);
            rc = stage(c, c.w->arena, (const uint8_t*)arena + cut[t], cut[t + 1] - cut[t]);
        }
        if (!rc && hipStreamSynchronize(c.s) != hipSuccess) {
            rc = fail(BMQCRC_EIO, "staging the arena range failed");
        }
        {
            std::unique_lock<std::mutex> wl(mu);
            cv.wait(wl, [&] { return walked; });
        }
        if (rc || !walk_ok) {
            rcs[t] = rc;
            errs[t] = t_err;
            return;
        }
        // this range's messages (and, for range 0, then the straddlers)
        for (uint32_t pass = 0; pass < (t == 0 ? 2u : 1u) && !rc; ++pass) {
            const uint32_t want = pass == 0 ? t : nd;
            std::vector<uint64_t> gi, lo;
            std::vector<uint32_t> ll, le;
            std::vector<uint8_t> packed;
            for (uint64_t i = 0; i < n; ++i) {
                if (owner[i] != want) {
                    continue;
                }
                gi.push_back(i);
                ll.push_back(len[i]);
                le.push_back(exp ? exp[i] : 0u);
                if (pass == 0) {
                    lo.push_back(off[i] - cut[t]);
                } else {
                    lo.push_back(packed.size());
                    packed.insert(packed.end(), (const uint8_t*)arena + off[i],
                                  (const uint8_t*)arena + off[i] + len[i]);
                }
            }
            // The slice keeps the batch's offset form.  A range's offsets
            // stay whole units of the shift from its cut (a multiple of 128);
            // the gathered straddlers sit at any byte, so theirs are bytes.
            bmqcrc_opts so = o;
            std::vector<uint32_t> lo32;
            if (off.p32 && (pass == 0 || packed.size() <= 0xFFFFFFFFull)) {
                so.flags |= BMQCRC_F_OFFSETS32;
                so.offset_shift = pass == 0 ? off.shift : 0u;
                lo32.resize(lo.size());
                for (size_t k = 0; k < lo.size(); ++k) {
                    lo32[k] = (uint32_t)(lo[k] >> so.offset_shift);
                }
            } else {
                so.flags &= ~BMQCRC_F_OFFSETS32;
                so.offset_shift = 0;
            }
            const uint64_t* lop = lo32.empty() ? lo.data() : (const uint64_t*)lo32.data();
            if (gi.empty()) {
                continue;
            }
            const uint64_t m = gi.size();
            const bool staged = pass == 0;
            const void* abase = staged ? (const void*)((const uint8_t*)arena + cut[t])
                                       : (const void*)packed.data();
            const uint64_t abytes = staged ? cut[t + 1] - cut[t] : packed.size();
            if (crcs) {
                std::vector<uint32_t> part(m);
                if ((rc = fold_staged(c, so.flags, seg, staged, abase, abytes, lop, ll.data(),
                                      nullptr, m, false, so.offset_shift, part.data()))) {
                    break;
                }
                for (uint64_t k = 0; k < m; ++k) {
                    (*crcs)[gi[k]] = part[k];
                }
                continue;
            }
            uint64_t nbad = 0, nw = 0;
            std::vector<uint64_t> lb(std::min<uint64_t>(bad_cap, m));
            if ((rc = verify_locked(c, c.w, so, seg, staged, abase, abytes, lop, ll.data(),
                                    le.data(), m, &nbad, lb.data(), lb.size(), &nw))) {
                break;
            }
            nb[t] += nbad;
            for (uint64_t k = 0; k < nw; ++k) {
                bads[t].push_back(gi[lb[k]]);
            }
        }
        rcs[t] = rc;
        errs[t] = t_err;
    };
    std::vector<std::thread> th;
    for (uint32_t t = 0; t < nd; ++t) {
        th.emplace_back(slice, t);
    }
    const int prc = prepare(pctx, &off64, &off32, &len, &exp, &n);
    off.p64 = off64;
    off.p32 = off32;
    int rc = prc;
    if (!rc && n > 0xFFFFFFFFull) {
        rc = fail(BMQCRC_EINVAL, "at most 2^32-1 messages per batch");
    }
    if (!rc) {
        rc = check_ranges(off, len, n, arena_bytes);
    }
    if (!rc) {
        owner.resize(n);
        for (uint64_t i = 0; i < n; ++i) {
            uint32_t t = (uint32_t)(std::upper_bound(cut.begin(), cut.end(), off[i]) - cut.begin());
            t = std::min(t == 0 ? 0u : t - 1u, nd - 1);
            owner[i] = off[i] + len[i] <= cut[t + 1] ? t : nd;
        }
        if (crcs) {
            crcs->assign(n, 0);
        }
    }
    const std::string walk_err = t_err;
    {
        std::lock_guard<std::mutex> wl(mu);
        walked = true;
        walk_ok = rc == 0;
    }
    cv.notify_all();
    for (auto& t : th) {
        t.join();
    }
    if (rc) {  // the walk's error (malformed input) takes precedence
        t_err = walk_err;
        return rc;
    }
    for (uint32_t t = 0; t < nd; ++t) {
        if (rcs[t]) {
            return fail(rcs[t], "device " + std::to_string(devs[t]) + ": " + errs[t]);
        }
    }
    if (crcs) {
        return 0;
    }
    uint64_t total_bad = 0;
    std::vector<uint64_t> all;
    for (uint32_t t = 0; t < nd; ++t) {
        total_bad += nb[t];
        all.insert(all.end(), bads[t].begin(), bads[t].end());
    }
    std::sort(all.begin(), all.end());
    const uint64_t take = std::min<uint64_t>(all.size(), bad_cap);
    bad->assign(std::min(bad_cap, n), 0);
    std::copy(all.begin(), all.begin() + take, bad->begin());
    *n_bad = total_bad;
    if (n_written) {
        *n_written = take;
    }
    return 0;
}

// bmqcrc_crc32c_batch_multi over offsets of either form: a slice's offsets
// keep the batch's form (32-bit ones are rebased in whole units of the shift).
int batch_multi(const void* arena, uint64_t arena_bytes, Offsets offsets, const uint32_t* lengths,
                const uint32_t* seeds, uint32_t* out, uint64_t n, const int* devices, int ndev,
                uint32_t seg_bytes)
{
    if (ndev < 1 || !lengths || !out || !arena) {
        return fail(BMQCRC_EINVAL, "bad arguments");
    }
    uint32_t seg = seg_bytes;
    int rc = check_seg(&seg);
    if (rc) {
        return rc;
    }
    const int have = device_count_raw();
    if (have <= 0) {
        return fail(BMQCRC_ENODEV, "no HIP device available");
    }
    std::vector<int> devs(ndev);
    if ((rc = device_list(devices, have, &devs))) {
        return rc;
    }
    // (its own text and the byte total: not check_ranges)
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (outside(offsets[i], lengths[i], arena_bytes)) {
            return fail(BMQCRC_EINVAL, "message outside arena");
        }
        total += lengths[i];
    }
    // Contiguous byte-balanced message slices; each device gets its own
    // copy of the arena range its slice touches.
    std::vector<uint64_t> cut(ndev + 1, n);
    cut[0] = 0;
    {
        uint64_t acc = 0, i = 0;
        for (int d = 1; d < ndev; ++d) {
            const uint64_t target = total * (uint64_t)d / (uint64_t)ndev;
            while (i < n && acc < target) {
                acc += lengths[i++];
            }
            cut[d] = i;
        }
    }
    std::vector<int> rcs(ndev, 0);
    std::vector<std::string> errs(ndev);
    std::vector<std::thread> th;
    for (int d = 0; d < ndev; ++d) {
        th.emplace_back([&, d]() {
            const uint64_t lo = cut[d], hi = cut[d + 1];
            if (lo >= hi) {
                return;
            }
            uint64_t amin = UINT64_MAX, amax = 0;
            for (uint64_t i = lo; i < hi; ++i) {
                amin = std::min(amin, offsets[i]);
                amax = std::max(amax, offsets[i] + lengths[i]);
            }
            if (amin > amax) {
                amin = amax = 0;
            }
            if (offsets.p32) {
                std::vector<uint32_t> rel32(hi - lo);
                const uint32_t base = (uint32_t)(amin >> offsets.shift);  // amin is one of them
                for (uint64_t i = lo; i < hi; ++i) {
                    rel32[i - lo] = offsets.p32[i] - base;
                }
                rcs[d] = batch_one(devs[d], nullptr, BMQCRC_F_OFFSETS32, seg,
                                   (const uint8_t*)arena + amin, amax - amin,
                                   (const uint64_t*)rel32.data(), lengths + lo,
                                   seeds ? seeds + lo : nullptr, out + lo, hi - lo, 0, 0,
                                   offsets.shift);
                errs[d] = t_err;
                return;
            }
            std::vector<uint64_t> rel(hi - lo);
            for (uint64_t i = lo; i < hi; ++i) {
                rel[i - lo] = offsets[i] - amin;
            }
            rcs[d] = batch_one(devs[d], nullptr, 0, seg, (const uint8_t*)arena + amin, amax - amin,
                               rel.data(), lengths + lo, seeds ? seeds + lo : nullptr, out + lo,
                               hi - lo);
            errs[d] = t_err;
        });
    }
    for (auto& t : th) {
        t.join();
    }
    for (int d = 0; d < ndev; ++d) {
        if (rcs[d]) {
            return fail(rcs[d], "device " + std::to_string(devs[d]) + ": " + errs[d]);
        }
    }
    return 0;
}

}  // namespace

extern "C" int bmqcrc_set_error(int rc, const char* msg)
{
    return fail(rc, msg ? msg : "");
}

extern "C" void bmqcrc_clear_error(void)
{
    t_err.clear();
}

int bmqcrc_verify_host_overlapped(const void* arena, uint64_t arena_bytes,
                                  bmqcrc_prepare_fn prepare, void* pctx, uint64_t* n_bad,
                                  std::vector<uint64_t>* bad, uint64_t bad_cap,
                                  const bmqcrc_opts* opts, std::vector<uint32_t>* crcs,
                                  uint64_t* n_written)
{
    if (n_written) {
        *n_written = 0;
    }
    t_err.clear();
    DeviceGuard keep_device;
    if (!prepare || (!crcs && (!n_bad || !bad)) || (!arena && arena_bytes)) {
        return fail(BMQCRC_EINVAL, "null pointer argument");
    }
    if (n_bad) {
        *n_bad = 0;
    }
    bmqcrc_opts o;
    uint32_t seg;
    int dev = 0, rc;
    const uint64_t* off = nullptr;
    const uint32_t* off32 = nullptr;
    const uint32_t* len = nullptr;
    const uint32_t* exp = nullptr;
    uint64_t n = 0;
    rc = parse_opts(opts, &o, &seg, &dev);
    if (rc && rc != BMQCRC_ENODEV) {
        return rc;
    }
    if (o.flags & (BMQCRC_F_DEVICE_PTRS | BMQCRC_F_ASYNC)) {
        return fail(BMQCRC_EINVAL, "overlapped verify takes host buffers, synchronously");
    }
    if (o.ndevices > 1) {
        return verify_host_multi(arena, arena_bytes, prepare, pctx, n_bad, bad, bad_cap, o, seg,
                                 crcs, n_written);
    }
    Ctx c;
    if (rc || (rc = open_ctx(dev, o.stream, &c))) {
        // no usable device: a malformed input is still reported first
        const std::string why = t_err;
        const int prc = prepare(pctx, &off, &off32, &len, &exp, &n);
        if (prc || n == 0) {  // nothing to verify needs no device
            return prc;
        }
        return fail(rc, why);
    }
    Workspace* w = c.w;
    std::lock_guard<std::mutex> g(w->mu);
    // The arena's H2D copy runs on a helper thread while the caller's walk
    // produces the descriptors on this one (its errors stay in this thread's
    // bmqcrc_last_error).
    int src = 0;
    std::thread copier([&] {
        if (hipSetDevice(dev) != hipSuccess) {
            src = BMQCRC_EIO;
            return;
        }
        src = stage(c, w->arena, arena, arena_bytes);
        if (!src && hipStreamSynchronize(c.s) != hipSuccess) {
            src = BMQCRC_EIO;
        }
    });
    const int prc = prepare(pctx, &off, &off32, &len, &exp, &n);
    copier.join();
    if (prc) {
        return prc;
    }
    if (src) {
        return fail(src, "staging the arena to the device failed");
    }
    if (n == 0) {
        return 0;
    }
    if (n > 0xFFFFFFFFull) {
        return fail(BMQCRC_EINVAL, "at most 2^32-1 messages per batch");
    }
    if ((rc = check_ranges(Offsets{off, off32, 0u}, len, n, arena_bytes))) {
        return rc;
    }
    if (off32) {  // the walk wrote its offsets in 32 bits as well: hand the device those
        o.flags |= BMQCRC_F_OFFSETS32;
        off = (const uint64_t*)off32;
    }
    if (crcs) {  // compute: stage the descriptors, fold, copy the CRCs back
        crcs->assign(n, 0);
        return fold_staged(c, o.flags, seg, true, arena, arena_bytes, off, len, nullptr, n, false,
                           0, crcs->data());
    }
    bad->assign(std::min<uint64_t>(bad_cap, n), 0);
    return verify_locked(c, w, o, seg, true, arena, arena_bytes, off, len, exp, n, n_bad,
                         bad->data(), bad->size(), n_written);
}

extern "C" {

// bmqcrc_crc32c, bmqcrc_crc32c_blob and bmqcrc_combine: crc32c_cpu.cpp

int bmqcrc_crc32c_batch(const void* arena, uint64_t arena_bytes, const uint64_t* offsets,
                        const uint32_t* lengths, const uint32_t* seeds, uint32_t* out,
                        uint64_t n, const bmqcrc_opts* opts)
{
    t_err.clear();
    DeviceGuard keep_device;
    if (n == 0) {
        return 0;
    }
    if (!offsets || !lengths || !out || (!arena && arena_bytes)) {
        return fail(BMQCRC_EINVAL, "null pointer argument");
    }
    if (n > 0xFFFFFFFFull) {
        return fail(BMQCRC_EINVAL, "at most 2^32-1 messages per batch");
    }
    bmqcrc_opts o;
    uint32_t seg;
    int dev, rc;
    if ((rc = parse_opts(opts, &o, &seg, &dev, true))) {
        return rc;
    }
    if (!(o.flags & BMQCRC_F_DEVICE_PTRS) &&
        (rc = check_ranges(offsets_of(o, offsets), lengths, n, arena_bytes))) {
        return rc;  // device arrays are trusted
    }
    if (!(o.flags & BMQCRC_F_DEVICE_PTRS) && o.ndevices > 1) {  // one byte range per device
        if (!(o.flags & BMQCRC_F_OFFSETS32)) {
            return bmqcrc_crc32c_batch_multi(arena, arena_bytes, offsets, lengths, seeds, out, n,
                                             o.devices, (int)o.ndevices, seg);
        }
        return batch_multi(arena, arena_bytes, offsets_of(o, offsets), lengths, seeds, out, n,
                           o.devices, (int)o.ndevices, seg);
    }
    return batch_one(dev, o.stream, o.flags, seg, arena, arena_bytes, offsets, lengths, seeds,
                     out, n, (o.flags & BMQCRC_F_DEVICE_PTRS) ? o.max_len : 0u,
                     (o.flags & BMQCRC_F_DEVICE_PTRS) ? o.min_len : 0u, o.offset_shift);
}

int bmqcrc_crc32c_verify(const void* arena, uint64_t arena_bytes, const uint64_t* offsets,
                         const uint32_t* lengths, const uint32_t* expected, uint64_t n,
                         uint64_t* n_bad, uint64_t* bad_idx, uint64_t bad_cap,
                         const bmqcrc_opts* opts)
{
    t_err.clear();
    DeviceGuard keep_device;
    if (!n_bad) {
        return fail(BMQCRC_EINVAL, "n_bad is required");
    }
    *n_bad = 0;
    if (n == 0) {
        return 0;
    }
    if (!offsets || !lengths || !expected || (!arena && arena_bytes) || (bad_cap && !bad_idx)) {
        return fail(BMQCRC_EINVAL, "null pointer argument");
    }
    if (n > 0xFFFFFFFFull) {
        return fail(BMQCRC_EINVAL, "at most 2^32-1 messages per batch");
    }
    bmqcrc_opts o;
    uint32_t seg;
    int dev, rc;
    if ((rc = parse_opts(opts, &o, &seg, &dev, true))) {
        return rc;
    }
    const bool dev_ptrs = (o.flags & BMQCRC_F_DEVICE_PTRS) != 0;
    const Offsets of = offsets_of(o, offsets);
    if (!dev_ptrs && (rc = check_ranges(of, lengths, n, arena_bytes))) {
        return rc;
    }
    if (!dev_ptrs && o.ndevices > 1) {  // one byte range per device, merged in index order
        GivenArrays ga = {of.p64, of.p32, lengths, expected, n};
        std::vector<uint64_t> bad;
        uint64_t written = 0;
        if ((rc = verify_host_multi(arena, arena_bytes, given_arrays, &ga, n_bad, &bad, bad_cap, o,
                                    seg, nullptr, &written))) {
            return rc;
        }
        std::copy(bad.begin(), bad.begin() + written, bad_idx);
        return 0;
    }
    Ctx c;
    if ((rc = open_ctx(dev, o.stream, &c))) {
        return rc;
    }
    Workspace* w = c.w;
    std::lock_guard<std::mutex> g(w->mu);
    return verify_locked(c, w, o, seg, false, arena, arena_bytes, offsets, lengths, expected, n,
                         n_bad, bad_idx, bad_cap, nullptr);
}

int bmqcrc_crc32c_blobs(const void* arena, uint64_t arena_bytes, const uint64_t* buf_offsets,
                        const uint32_t* buf_lengths, uint64_t nbuf,
                        const uint64_t* msg_first_buf, const uint32_t* seeds, uint32_t* out,
                        uint64_t n, const bmqcrc_opts* opts)
{
    t_err.clear();
    DeviceGuard keep_device;
    if (n == 0) {
        return 0;
    }
    if (!msg_first_buf || !out || (nbuf && (!buf_offsets || !buf_lengths)) ||
        (!arena && arena_bytes)) {
        return fail(BMQCRC_EINVAL, "null pointer argument");
    }
    if (nbuf > 0xFFFFFFFFull || n > 0xFFFFFFFFull) {
        return fail(BMQCRC_EINVAL, "at most 2^32-1 buffers and blobs per call");
    }
    bmqcrc_opts o;
    uint32_t seg;
    int dev, rc;
    if ((rc = parse_opts(opts, &o, &seg, &dev))) {
        return rc;
    }
    const bool dev_ptrs = (o.flags & BMQCRC_F_DEVICE_PTRS) != 0;
    if (!dev_ptrs) {
        if ((rc = check_ranges(Offsets{buf_offsets, nullptr, 0u}, buf_lengths, nbuf,
                               arena_bytes))) {
            return rc;
        }
        for (uint64_t m = 0; m < n; ++m) {
            if (msg_first_buf[m] > msg_first_buf[m + 1] || msg_first_buf[m + 1] > nbuf) {
                return fail(BMQCRC_EINVAL, "msg_first_buf must be non-decreasing and <= nbuf");
            }
        }
    }
    Ctx c;
    if ((rc = open_ctx(dev, o.stream, &c))) {
        return rc;
    }
    Workspace* w = c.w;
    std::lock_guard<std::mutex> g(w->mu);
    if ((rc = w->buf_crc.ensure(4 * std::max<uint64_t>(nbuf, 1)))) {
        return rc;
    }
    // the batch is the nbuf buffers; the seeds are the n blobs', staged apart
    DevArrays d = {arena, buf_offsets, buf_lengths, nullptr};
    const uint64_t* d_first = msg_first_buf;
    const uint32_t* d_seeds = seeds;
    uint32_t* d_out = out;
    if (!dev_ptrs) {
        if ((rc = stage_batch(c, o.flags, false, arena, arena_bytes, buf_offsets, buf_lengths,
                              nullptr, nbuf, &d)) ||
            (rc = stage(c, w->first_buf, msg_first_buf, 8 * (n + 1))) ||
            (seeds && (rc = stage(c, w->seeds, seeds, 4 * n))) || (rc = w->out.ensure(4 * n))) {
            return rc;
        }
        d_first = (const uint64_t*)w->first_buf.p;
        d_seeds = seeds ? (const uint32_t*)w->seeds.p : nullptr;
        d_out = (uint32_t*)w->out.p;
    }
    if (nbuf && (rc = run_batch(c, o.flags, seg, d.arena, arena_bytes, d.offsets, d.lengths,
                                nullptr, (uint32_t*)w->buf_crc.p, nbuf,
                                dev_ptrs ? UINT64_MAX : max_length(buf_lengths, nbuf)))) {
        return rc;
    }
    if (bmqcrc_launch_blob_combine((const uint32_t*)w->buf_crc.p, d.lengths, d_first, d_seeds,
                                   d_out, n, (void*)c.s)) {
        return fail(BMQCRC_EIO, "blob combine launch failed");
    }
    if (!dev_ptrs) {
        HIP_TRY(hipMemcpyAsync(out, d_out, 4 * n, hipMemcpyDeviceToHost, c.s));
        HIP_TRY(hipStreamSynchronize(c.s));
    } else if (!(o.flags & BMQCRC_F_ASYNC)) {
        HIP_TRY(hipStreamSynchronize(c.s));
    }
    return 0;
}

// Scattered host buffers (a bdlbb::Blob's data buffers) -> one contiguous
// device arena, through the workspace's pinned ring: kGatherThreads host
// threads each copy their chunks into pinned slots and enqueue the slot's H2D
// copy at once, so gathering chunk k+1 overlaps the PCIe transfer of chunk k
// (no pageable staging copy, no second host copy).  Message m is then the
// contiguous range of its buffers and the whole batch is one fold launch.
constexpr uint64_t kGatherChunk = 4ull << 20;
constexpr int kGatherSlots = 16;
constexpr int kGatherThreads = 8;

int bmqcrc_crc32c_gather(const void* const* bufs, const uint32_t* buf_lengths, uint64_t nbuf,
                         const uint64_t* msg_first_buf, const uint32_t* seeds, uint32_t* out,
                         uint64_t n, const bmqcrc_opts* opts)
{
    t_err.clear();
    DeviceGuard keep_device;
    if (n == 0) {
        return 0;
    }
    if (!msg_first_buf || !out || (nbuf && (!bufs || !buf_lengths))) {
        return fail(BMQCRC_EINVAL, "null pointer argument");
    }
    if (nbuf > 0xFFFFFFFFull || n > 0xFFFFFFFFull) {
        return fail(BMQCRC_EINVAL, "at most 2^32-1 buffers and messages per call");
    }
    for (uint64_t m = 0; m < n; ++m) {
        if (msg_first_buf[m] > msg_first_buf[m + 1] || msg_first_buf[m + 1] > nbuf) {
            return fail(BMQCRC_EINVAL, "msg_first_buf must be non-decreasing and <= nbuf");
        }
    }
    // Arena layout: buffers [b0, b1) back to back, in order.
    const uint64_t b0 = msg_first_buf[0], b1 = msg_first_buf[n];
    std::vector<uint64_t> boff(b1 - b0 + 1, 0);
    for (uint64_t b = b0; b < b1; ++b) {
        if (buf_lengths[b] && !bufs[b]) {
            return fail(BMQCRC_EINVAL, "buffer " + std::to_string(b) + " is NULL with a length");
        }
        boff[b - b0 + 1] = boff[b - b0] + buf_lengths[b];
    }
    const uint64_t total = boff.back();
    std::vector<uint64_t> moff(n);
    std::vector<uint32_t> mlen(n);
    for (uint64_t m = 0; m < n; ++m) {
        moff[m] = boff[msg_first_buf[m] - b0];
        const uint64_t len = boff[msg_first_buf[m + 1] - b0] - moff[m];
        if (len > 0xFFFFFFFFull) {
            return fail(BMQCRC_EINVAL, "message " + std::to_string(m) + " is longer than 2^32-1");
        }
        mlen[m] = (uint32_t)len;
    }
    // argument errors above are reported before a missing device
    bmqcrc_opts o;
    uint32_t seg;
    int dev, rc;
    if ((rc = parse_opts(opts, &o, &seg, &dev))) {
        return rc;
    }
    if (o.flags & (BMQCRC_F_DEVICE_PTRS | BMQCRC_F_ASYNC)) {
        return fail(BMQCRC_EINVAL, "gather takes host buffers, synchronously");
    }
    Ctx c;
    if ((rc = open_ctx(dev, o.stream, &c))) {
        return rc;
    }
    Workspace* w = c.w;
    std::lock_guard<std::mutex> g(w->mu);
    if ((rc = w->arena.ensure(total + 16))) {
        return rc;
    }
    if (total && !w->pin) {
        void* h = nullptr;
        HIP_TRY(hipHostMalloc(&h, kGatherSlots * kGatherChunk, hipHostMallocPortable));
        w->pin = (uint8_t*)h;
        for (int sl = 0; sl < kGatherSlots; ++sl) {
            HIP_TRY(hipEventCreateWithFlags(&w->pin_ev[sl], hipEventDisableTiming));
        }
    }
    const uint64_t nchunks = (total + kGatherChunk - 1) / kGatherChunk;
    const int nthreads = (int)std::min<uint64_t>(kGatherThreads, nchunks);
    std::vector<int> trc(std::max(nthreads, 1), 0);
    std::vector<std::string> terr(trc.size());
    auto worker = [&](int t) {
        if (hipSetDevice(dev) != hipSuccess) {
            trc[t] = BMQCRC_EIO;
            terr[t] = "hipSetDevice failed in a gather thread";
            return;
        }
        const int per = kGatherSlots / nthreads;  // slots t, t + nthreads, ... are thread t's
        for (uint64_t ch = (uint64_t)t; ch < nchunks; ch += (uint64_t)nthreads) {
            const int sl = t + nthreads * (int)((ch / (uint64_t)nthreads) % (uint64_t)per);
            hipError_t e = hipSuccess;
            if (w->pin_used[sl]) {
                e = hipEventSynchronize(w->pin_ev[sl]);  // the slot's previous copy is done
            }
            const uint64_t lo = ch * kGatherChunk, hi = std::min(total, lo + kGatherChunk);
            uint8_t* dst = w->pin + (uint64_t)sl * kGatherChunk;
            size_t k = (size_t)(std::upper_bound(boff.begin(), boff.end(), lo) - boff.begin()) - 1;
            for (uint64_t pos = lo; e == hipSuccess && pos < hi;) {
                if (boff[k + 1] <= pos) {
                    ++k;  // empty buffers and buffers that end at pos
                    continue;
                }
                const uint64_t take = std::min(hi, boff[k + 1]) - pos;
                memcpy(dst + (pos - lo), (const uint8_t*)bufs[b0 + k] + (pos - boff[k]), take);
                pos += take;
            }
            if (e == hipSuccess) {
                e = hipMemcpyAsync((uint8_t*)w->arena.p + lo, dst, hi - lo, hipMemcpyHostToDevice,
                                   c.s);
            }
            if (e == hipSuccess) {
                e = hipEventRecord(w->pin_ev[sl], c.s);
            }
            if (e != hipSuccess) {
                trc[t] = e == hipErrorOutOfMemory ? BMQCRC_ENOMEM : BMQCRC_EIO;
                terr[t] = std::string("gather staging: ") + hipGetErrorString(e);
                return;
            }
            w->pin_used[sl] = true;
        }
    };
    if (nthreads == 1) {
        worker(0);
    } else if (nthreads > 1) {
        std::vector<std::thread> th;
        for (int t = 0; t < nthreads; ++t) {
            th.emplace_back(worker, t);
        }
        for (auto& t : th) {
            t.join();
        }
    }
    for (size_t t = 0; t < trc.size(); ++t) {
        if (trc[t]) {
            (void)hipStreamSynchronize(c.s);  // no copy may still read a slot we hand back
            return fail(trc[t], terr[t]);
        }
    }
    // the ring has put the arena on the device
    return fold_staged(c, o.flags, seg, true, nullptr, total, moff.data(), mlen.data(), seeds, n,
                       false, 0, out);
}

int bmqcrc_crc32c_batch_multi(const void* arena, uint64_t arena_bytes, const uint64_t* offsets,
                              const uint32_t* lengths, const uint32_t* seeds, uint32_t* out,
                              uint64_t n, const int* devices, int ndev, uint32_t seg_bytes)
{
    t_err.clear();
    if (n == 0) {
        return 0;
    }
    if (!offsets) {
        return fail(BMQCRC_EINVAL, "bad arguments");
    }
    return batch_multi(arena, arena_bytes, Offsets{offsets, nullptr, 0u}, lengths, seeds, out, n,
                       devices, ndev, seg_bytes);
}

int bmqcrc_reserve(int device, void* stream, uint64_t n_msgs, uint64_t arena_bytes,
                   uint32_t seg_bytes)
{
    t_err.clear();
    DeviceGuard keep_device;
    LockedCtx c;
    int rc;
    if ((rc = check_seg(&seg_bytes)) || (rc = lock_on(device, stream, true, &c))) {
        return rc;
    }
    BatchArgs a;
    memset(&a, 0, sizeof(a));
    auto_shape(n_msgs, arena_bytes, c.st->num_cus, &seg_bytes, &a.blocks_per_cu);  // as the batch call will
    return plan_ws(c.w, c.s, n_msgs, arena_bytes, seg_bytes, &a, *c.st);
}

int bmqcrc_fill_synthetic(void* dev_dst, uint64_t nbytes, uint64_t seed, uint64_t begin,
                          const bmqcrc_opts* opts)
{
    t_err.clear();
    DeviceGuard keep_device;
    if (opts && (opts->flags & BMQCRC_F_OFFSETS32)) {
        return fail(BMQCRC_EINVAL,
                    "BMQCRC_F_OFFSETS32 applies to bmqcrc_crc32c_batch and bmqcrc_crc32c_verify only");
    }
    int dev, rc;
    if ((rc = resolve_device(opts ? opts->device : -1, &dev))) {
        return rc;
    }
    if (((uintptr_t)dev_dst & 7u) || (begin & 7u)) {
        return fail(BMQCRC_EINVAL, "destination and begin must be 8-byte aligned");
    }
    DeviceState* st = nullptr;
    if ((rc = device_state(dev, &st))) {
        return rc;
    }
    HIP_TRY(hipSetDevice(dev));
    hipStream_t s = opts ? (hipStream_t)opts->stream : nullptr;
    if (bmqcrc_launch_fill((uint8_t*)dev_dst, nbytes, seed, begin, (void*)s)) {
        return fail(BMQCRC_EIO, "fill launch failed");
    }
    if (!(opts && (opts->flags & BMQCRC_F_ASYNC))) {
        HIP_TRY(hipStreamSynchronize(s));
    }
    return 0;
}

int bmqcrc_kernel_timing(int device, void* stream, double* total_ms, uint32_t* count)
{
    t_err.clear();
    DeviceGuard keep_device;
    LockedCtx c;
    int rc;
    if ((rc = lock_on(device, stream, false, &c))) {
        return rc;
    }
    HIP_TRY(hipSetDevice(c.dev));  // for the event calls below
    Workspace* w = c.w;
    double tot = 0;
    uint32_t cnt = 0;
    for (auto& e : w->timing) {
        HIP_TRY(hipEventSynchronize(e.second));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, e.first, e.second));
        tot += ms;
        ++cnt;
        w->spare.push_back(e);
    }
    w->timing.clear();
    if (total_ms) {
        *total_ms = tot;
    }
    if (count) {
        *count = cnt;
    }
    return 0;
}

}  // extern "C"

// ---- the calls that take device pointers only: the fused copy, the packers --
namespace {

// Their bmqcrc_opts, with `call` naming the entry point in the refusals.
// Answers without a device: the call's own argument checks follow it, and
// only then the device lookup.
int device_call_opts(const bmqcrc_opts* opts, const std::string& call, bmqcrc_opts* o)
{
    read_opts(opts, o);
    static const struct {
        uint32_t bit;
        const char* name;
    } refused[] = {{BMQCRC_F_TIME_KERNEL, "BMQCRC_F_TIME_KERNEL"},
                   {BMQCRC_F_WHOLE_MESSAGES, "BMQCRC_F_WHOLE_MESSAGES"},
                   {BMQCRC_F_PLAN, "BMQCRC_F_PLAN"},
                   {BMQCRC_F_OFFSETS32, "BMQCRC_F_OFFSETS32"}};
    for (const auto& r : refused) {
        if (o->flags & r.bit) {
            return fail(BMQCRC_EINVAL, std::string(r.name) + " does not apply to " + call);
        }
    }
    if (o->flags & ~(BMQCRC_F_DEVICE_PTRS | BMQCRC_F_ASYNC)) {
        return fail(BMQCRC_EINVAL, "unknown bmqcrc_opts.flags bits");
    }
    if (!(o->flags & BMQCRC_F_DEVICE_PTRS)) {
        return fail(BMQCRC_EINVAL,
                    call + " takes device pointers only: BMQCRC_F_DEVICE_PTRS is required");
    }
    if (o->ndevices > 1) {
        return fail(BMQCRC_EINVAL, call + " runs on one device: ndevices > 1");
    }
    return 0;
}

// `what` names the kernel ("copy", "put-pack layout") whose launch call failed.
int launch_failed(const char* what)
{
    return fail(BMQCRC_EIO, std::string(what) + " launch failed: " +
                                hipGetErrorString(hipGetLastError()));
}

// The first required pointer that is null, by its name in the call's struct.
struct NamedNull {
    bool null;
    const char* name;
};

int refuse_null(std::initializer_list<NamedNull> args)
{
    for (const NamedNull& a : args) {
        if (a.null) {
            return fail(BMQCRC_EINVAL, std::string("null pointer argument: ") + a.name);
        }
    }
    return 0;
}

// Two byte ranges, neither empty, share a byte.
bool overlaps(uintptr_t a, uint64_t a_bytes, uintptr_t b, uint64_t b_bytes)
{
    return a_bytes && b_bytes && a < b + b_bytes && b < a + a_bytes;
}

// A refusal counter as the kernels leave it: 0 when nothing was refused,
// otherwise the complement of (kind << 56 | index).
void refusal_of(unsigned long long ctr, uint32_t* kind, uint64_t* index)
{
    const unsigned long long key = ctr ? ~ctr : 0;
    *kind = (uint32_t)(key >> 56);
    *index = key & ((1ull << 56) - 1);
}

// The refusal `kind` of a device call in words: what[kind] is its text,
// with %llu for the index and, where the text has a second, for the offset,
// and where it has a third, for the message.
template <size_t K>
int refused(const char* const (&what)[K], uint32_t kind, uint64_t index, uint64_t offset = 0,
            uint64_t message = 0)
{
    char buf[256];
    snprintf(buf, sizeof(buf), what[kind < K ? kind : 0], (unsigned long long)index,
             (unsigned long long)offset, (unsigned long long)message);
    return fail(BMQCRC_EINVAL, std::string(buf) + ": nothing was written");
}

static_assert(kCopyPlanThreads == kPackThreads && kCopyPlanBlocks == kPackBlocks,
              "layout_split: the copy's and the packers' pre-kernels share one grid split");

// Contiguous message ranges of whole kPackThreads tiles for at most
// kPackBlocks blocks (n > 0).
void layout_split(uint64_t n, uint64_t* per_block, uint32_t* nblocks)
{
    const uint64_t tiles = (n + kPackThreads - 1) / kPackThreads;
    const uint64_t nb = std::min<uint64_t>(tiles, kPackBlocks);
    const uint64_t tiles_per = (tiles + nb - 1) / nb;
    *per_block = tiles_per * kPackThreads;
    *nblocks = (uint32_t)((tiles + tiles_per - 1) / tiles_per);
}

// Counters of the copy last enqueued on c's workspace, after everything
// enqueued on its stream (w->mu held).
static int copy_result(Ctx& c, unsigned long long (&ctr)[kCopyCtrWords])
{
    HIP_TRY(hipMemcpyAsync(ctr, c.w->copy_ctr.p, sizeof(ctr), hipMemcpyDeviceToHost, c.s));
    HIP_TRY(hipStreamSynchronize(c.s));
    return 0;
}

// Enqueue one fused copy + CRC on c.s (caller holds c.w->mu): `a` carries the
// caller's arrays and n; the scratch (piece prefix, block sums, kCopyCtrWords
// counters at `ctr`, zeroed here) is the calling entry point's own, so that
// bmqcrc_crc32c_copy and bmqcrc_put_event_pack keep separate records.
static int enqueue_copy(Ctx& c, CopyArgs a, DevBuf& first, DevBuf& bsum, void* ctr)
{
    int rc;
    if ((rc = bsum.ensure(8ull * kCopyPlanBlocks)) || (rc = first.ensure(4 * (a.n + 1)))) {
        return rc;
    }
    {
        std::lock_guard<std::mutex> gd(g_mu);  // DeviceState is shared by the device's streams
        if (c.st->copy_blocks == 0) {
            int per = 0;
            if (bmqcrc_copy_occupancy(&per) != 0 || per <= 0) {
                return fail(BMQCRC_EIO, "k_copy_fold occupancy query failed");
            }
            c.st->copy_blocks = (uint32_t)per * (uint32_t)std::max(c.st->num_cus, 1);
        }
    }
    HIP_TRY(hipMemsetAsync(ctr, 0, 8 * kCopyCtrWords, c.s));
    if (a.n) {
        a.first = (uint32_t*)first.p;
        a.bsum = (unsigned long long*)bsum.p;
        a.ctr = (unsigned long long*)ctr;
        layout_split(a.n, &a.per_block, &a.nblocks);
        if (bmqcrc_launch_copy(&a, (void*)c.s, c.st->copy_blocks)) {
            return launch_failed("copy");
        }
    }
    return 0;
}

// The payload pass of a packer: the messages of `a` (PackArgs or RecArgs)
// copied from `src` to where the layout placed them (a.off), their CRCs to
// a.out, the copy's counters behind the layout's ctr_words.
template <class Args>
int enqueue_payload(Ctx& c, PackScratch& s, int ctr_words, const void* src, const Args& a)
{
    CopyArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.src = (const uint8_t*)src;
    ca.src_bytes = a.src_bytes;
    ca.src_offsets = a.src_offsets;
    ca.lengths = a.lengths;
    ca.dst = a.dst;
    ca.dst_bytes = a.dst_bytes;
    ca.dst_offsets = (const uint64_t*)a.off;
    ca.out = (uint32_t*)a.out;
    ca.n = a.n;
    return enqueue_copy(c, ca, s.first, s.copy_bsum, a.ctr + ctr_words);
}

// The copy pass behind a layout that refused nothing, from its counters `cc`:
// the layout placed every message inside the destination, so the copy pass has
// nothing to refuse.
int copy_pass_clean(const unsigned long long* cc, const char* call)
{
    if (cc[kCopyCtrRefused] || cc[kCopyCtrOverflow]) {
        return fail(BMQCRC_EIO, std::string(call) + ": the copy pass refused a message the "
                                                    "layout had placed (internal error)");
    }
    return 0;
}

int SlotCopyScratch::begin(Ctx& c, int ctr_words, uint64_t n_units)
{
    HIP_TRY(hipMemsetAsync(ctr.p, 0, 8 * (ctr_words + kCopyCtrWords), c.s));
    n = n_units;
    any = true;
    return 0;
}

int SlotCopyScratch::enqueue_slot_copy(Ctx& c, const void* src, uint64_t src_bytes, void* to,
                                       uint64_t to_bytes, uint64_t n_slots, int ctr_words)
{
    CopyArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.src = (const uint8_t*)src;
    ca.src_bytes = src_bytes;
    ca.src_offsets = (const uint64_t*)off.p;
    ca.lengths = (const uint32_t*)len.p;
    ca.dst = (uint8_t*)to;
    ca.dst_bytes = to_bytes;
    ca.dst_offsets = (const uint64_t*)dst.p;
    ca.out = (uint32_t*)out.p;
    ca.n = n_slots;
    return enqueue_copy(c, ca, copy_first, copy_bsum, (unsigned long long*)ctr.p + ctr_words);
}

// Counters of the pack last enqueued on `s`, after everything enqueued on c's
// stream (w->mu held): ctr[] receives the layout's ctr_words and the copy
// pass's kCopyCtrWords, kind and index the refusal (kind 0: nothing refused).
int pack_counters(Ctx& c, const PackScratch& s, int ctr_words, const char* call,
                  unsigned long long* ctr, uint32_t* kind, uint64_t* index)
{
    HIP_TRY(hipMemcpyAsync(ctr, s.ctr.p, 8 * (ctr_words + kCopyCtrWords), hipMemcpyDeviceToHost,
                           c.s));
    HIP_TRY(hipStreamSynchronize(c.s));
    refusal_of(ctr[kLayoutCtrRefusal], kind, index);
    return *kind ? 0 : copy_pass_clean(ctr + ctr_words, call);
}

// The struct_size / reserved preamble of a call that takes its arguments in a
// struct P, `name`d in the texts.  Answers before the options are read.
template <class P>
int check_struct(const P* p, const char* name, uint64_t reserved2 = 0,
                 const char* reserved_text = ".reserved must be 0")
{
    if (!p || p->struct_size != sizeof(P)) {
        return fail(BMQCRC_EINVAL,
                    std::string(name) + ".struct_size must be sizeof(" + name + ")");
    }
    return p->reserved || reserved2 ? fail(BMQCRC_EINVAL, std::string(name) + reserved_text) : 0;
}

// The first of `outs` (null ones skipped) that shares a byte with one of `ins`.
struct NamedRange {
    const void* at;
    uint64_t bytes;
    const char* name;
};

int refuse_overlap(std::initializer_list<NamedRange> outs, std::initializer_list<NamedRange> ins)
{
    for (const NamedRange& a : outs) {
        for (const NamedRange& b : ins) {
            if (a.at && overlaps((uintptr_t)a.at, a.bytes, (uintptr_t)b.at, b.bytes)) {
                return fail(BMQCRC_EINVAL, std::string(a.name) + " overlaps " + b.name);
            }
        }
    }
    return 0;
}

// The fold of an unpacker over its scratch's descriptors, which the placing
// kernel filled for every slot: never over the caller's arrays.
int fold_slots(Ctx& c, const UnpackScratch& s, const void* window, uint64_t window_bytes,
               uint64_t cap)
{
    return run_batch(c, BMQCRC_F_DEVICE_PTRS | BMQCRC_F_PLAN, 0, window, window_bytes,
                     (const uint64_t*)s.off.p, (const uint32_t*)s.len.p, nullptr,
                     (uint32_t*)s.out.p, cap);
}

// Counters of the unpack last enqueued on `s`, after everything enqueued on
// c's stream (w->mu held), into ctr[] and what both results (R) share: the
// refusal (its index to *index), otherwise the messages, the mismatches and
// the lowest of them.  All zeros when there was none.
template <class R, size_t W>
int slot_counters(Ctx& c, const UnpackScratch& s, unsigned long long (&ctr)[W], R* r,
                  uint64_t* index)
{
    memset(r, 0, sizeof(*r));
    memset(ctr, 0, sizeof(ctr));
    if (!s.any) {
        return 0;
    }
    HIP_TRY(hipMemcpyAsync(ctr, s.ctr.p, sizeof(ctr), hipMemcpyDeviceToHost, c.s));
    HIP_TRY(hipStreamSynchronize(c.s));
    if (ctr[kSlotCtrRefusal]) {
        refusal_of(ctr[kSlotCtrRefusal], &r->refused_kind, index);
        return 0;
    }
    r->n_msgs = ctr[kSlotCtrMsgs];
    r->n_bad = ctr[kSlotCtrBad];
    r->first_bad = r->n_bad ? ~ctr[kSlotCtrFirstBad] : r->n_msgs;
    return 0;
}

// The end of a device call: unless asynchronous, the result `read` gives for
// c's workspace, copied out when the caller wants it.  *r is zeros, no
// refusal, after an asynchronous call.
template <class R, class Read>
int sync_result(Ctx& c, const bmqcrc_opts& o, Read read, R* result, R* r)
{
    memset(r, 0, sizeof(*r));
    int rc = 0;
    if (!(o.flags & BMQCRC_F_ASYNC) && !(rc = read(c, r)) && result) {
        *result = *r;
    }
    return rc;
}

// ... and, for a result that names its refusal by kind and index alone, the
// refusal's text and code.
template <class R, class Read, size_t K>
int sync_result_or_refusal(Ctx& c, const bmqcrc_opts& o, Read read, R* result,
                           const char* const (&what)[K])
{
    R r;
    const int rc = sync_result(c, o, read, result, &r);
    return rc ? rc : r.refused_kind ? refused(what, r.refused_kind, r.refused_index) : 0;
}

// The body of a bmqcrc_last_*: the result `read` gives for the stream's workspace.
template <class R, class Read>
int last_result(int device, void* stream, Read read, R* result)
{
    t_err.clear();
    DeviceGuard keep_device;
    LockedCtx c;
    int rc;
    R r;
    if ((rc = lock_on(device, stream, true, &c)) || (rc = read(c, &r))) {
        return rc;
    }
    if (result) {
        *result = r;
    }
    return 0;
}

}  // namespace

extern "C" {

int bmqcrc_crc32c_copy(const void* src, uint64_t src_bytes, const uint64_t* src_offsets,
                       const uint32_t* lengths, void* dst, uint64_t dst_bytes,
                       const uint64_t* dst_offsets, const uint32_t* seeds, uint32_t* out,
                       uint64_t n, const bmqcrc_opts* opts)
{
    t_err.clear();
    DeviceGuard keep_device;
    // every refusal below answers before the device lookup (no GPU needed)
    bmqcrc_opts o;
    int rc;
    if ((rc = device_call_opts(opts, "bmqcrc_crc32c_copy", &o))) {
        return rc;
    }
    if (n > 0xFFFFFFFFull) {
        return fail(BMQCRC_EINVAL, "at most 2^32-1 messages per batch");
    }
    if (n && (!src_offsets || !lengths || !dst_offsets || !out || (!src && src_bytes) ||
              (!dst && dst_bytes))) {
        return fail(BMQCRC_EINVAL, "null pointer argument");
    }
    LockedCtx c;
    if ((rc = lock_on(o.device, o.stream, true, &c))) {
        return rc;
    }
    Workspace* w = c.w;
    if ((rc = w->copy_ctr.ensure(8 * kCopyCtrWords))) {
        return rc;
    }
    CopyArgs a;
    memset(&a, 0, sizeof(a));
    a.src = (const uint8_t*)src;
    a.src_bytes = src_bytes;
    a.src_offsets = src_offsets;
    a.lengths = lengths;
    a.dst = (uint8_t*)dst;
    a.dst_bytes = dst_bytes;
    a.dst_offsets = dst_offsets;
    a.seeds = seeds;
    a.out = out;
    a.n = n;
    w->copy_n = n;
    w->copy_any = true;
    if ((rc = enqueue_copy(c, a, w->copy_first, w->copy_bsum, w->copy_ctr.p))) {
        return rc;
    }
    if (o.flags & BMQCRC_F_ASYNC) {
        return 0;
    }
    unsigned long long ctr[kCopyCtrWords];
    if ((rc = copy_result(c, ctr))) {
        return rc;
    }
    if (ctr[kCopyCtrOverflow]) {
        return fail(BMQCRC_EINVAL, "more than 2^32-1 16-byte pieces in one copy call: nothing copied");
    }
    if (ctr[kCopyCtrRefused]) {
        return fail(BMQCRC_EINVAL,
                    "message " + std::to_string(~ctr[kCopyCtrLowestInv]) + " lies outside [src, src+"
                    "src_bytes) or [dst, dst+dst_bytes): refused (" +
                        std::to_string(ctr[kCopyCtrRefused]) + " in all), the others were copied");
    }
    return 0;
}

int bmqcrc_last_copy(int device, void* stream, uint64_t* n_msgs, uint64_t* n_refused,
                     uint64_t* first_refused)
{
    t_err.clear();
    DeviceGuard keep_device;
    LockedCtx c;
    int rc;
    if ((rc = lock_on(device, stream, true, &c))) {
        return rc;
    }
    unsigned long long ctr[kCopyCtrWords] = {};
    if (c.w->copy_any && (rc = copy_result(c, ctr))) {
        return rc;
    }
    if (ctr[kCopyCtrOverflow]) {
        return fail(BMQCRC_EINVAL, "more than 2^32-1 16-byte pieces in one copy call: nothing copied");
    }
    if (n_msgs) {
        *n_msgs = c.w->copy_n;
    }
    if (n_refused) {
        *n_refused = ctr[kCopyCtrRefused];
    }
    if (first_refused) {
        *first_refused = ctr[kCopyCtrRefused] ? ~ctr[kCopyCtrLowestInv] : c.w->copy_n;
    }
    return 0;
}

static_assert(BMQCRC_PUT_PACK_SRC_RANGE == BMQCRC_PACK_KIND_SRC_RANGE &&
                  BMQCRC_PUT_PACK_EVENT_FIRST == BMQCRC_PACK_KIND_EVENT_FIRST &&
                  BMQCRC_PUT_PACK_EVENT_TOO_BIG == BMQCRC_PACK_KIND_EVENT_TOO_BIG &&
                  BMQCRC_PUT_PACK_DST_TOO_SMALL == BMQCRC_PACK_KIND_DST_TOO_SMALL &&
                  BMQCRC_PUT_PACK_TOO_MANY_PIECES == BMQCRC_PACK_KIND_TOO_MANY_PIECES,
              "the kernels' refusal kinds are the public ones");

constexpr uint64_t kPutMaxSizeSoft = 66ull << 20;              // PutHeader::k_MAX_SIZE_SOFT
constexpr uint64_t kPutMaxEventBytes = ((1ull << 28) - 1) * 4;  // 28 bits of MessageWords

// Counters of the pack last enqueued on c's workspace, after everything
// enqueued on its stream (w->mu held): kind 0 = nothing refused.
static int pack_result(Ctx& c, uint32_t* kind, uint64_t* index, uint64_t* total)
{
    unsigned long long ctr[kPackCtrWords + kCopyCtrWords];
    const int rc =
        pack_counters(c, c.w->pack, kPackCtrWords, "bmqcrc_put_event_pack", ctr, kind, index);
    *total = rc || *kind ? 0 : ctr[kPackCtrTotal];
    return rc;
}

static const char* const kPackRefusals[6] = {
    "", "BMQCRC_PUT_PACK_SRC_RANGE: message %llu lies outside [src, src+src_bytes)",
    "BMQCRC_PUT_PACK_EVENT_FIRST: event_first[%llu] breaks 0 = first < ... < last = n",
    "BMQCRC_PUT_PACK_EVENT_TOO_BIG: event %llu is longer than max_event_bytes",
    "BMQCRC_PUT_PACK_DST_TOO_SMALL: event %llu ends past dst_bytes",
    "BMQCRC_PUT_PACK_TOO_MANY_PIECES: more than 2^32-1 16-byte pieces of payload in one "
    "call (index %llu)"};

int bmqcrc_put_event_pack(const bmqcrc_put_pack* p, uint64_t* total_bytes, const bmqcrc_opts* opts)
{
    t_err.clear();
    DeviceGuard keep_device;
    // every refusal below answers before the device lookup (no GPU needed)
    bmqcrc_opts o;
    int rc;
    if ((rc = check_struct(p, "bmqcrc_put_pack")) ||
        (rc = device_call_opts(opts, "bmqcrc_put_event_pack", &o))) {
        return rc;
    }
    const uint64_t n = p->n;
    if (n > 0xFFFFFFFFull) {
        return fail(BMQCRC_EINVAL, "at most 2^32-1 messages per call");
    }
    if (n && (rc = refuse_null({{!p->src_offsets, "src_offsets"},
                                {!p->lengths, "lengths"},
                                {!p->queue_ids, "queue_ids"},
                                {!p->guids, "guids"},
                                {!p->dst, "dst"},
                                {!p->src && p->src_bytes, "src"}}))) {
        return rc;
    }
    if ((uintptr_t)p->dst & 3u) {
        return fail(BMQCRC_EINVAL, "dst must be 4-byte aligned");
    }
    if (overlaps((uintptr_t)p->src, p->src_bytes, (uintptr_t)p->dst, p->dst_bytes)) {
        return fail(BMQCRC_EINVAL, "[dst, dst+dst_bytes) overlaps [src, src+src_bytes)");
    }
    if (p->max_event_bytes > kPutMaxEventBytes) {
        return fail(BMQCRC_EINVAL, "max_event_bytes above (2^28-1)*4: MessageWords would overflow");
    }
    if (!p->event_first && p->n_events != 1) {
        return fail(BMQCRC_EINVAL, "event_first == NULL means one event: n_events must be 1");
    }
    if (n && (p->n_events < 1 || p->n_events > n)) {
        return fail(BMQCRC_EINVAL, "n_events must lie in [1, n]: no event is empty");
    }
    LockedCtx c;
    if ((rc = lock_on(o.device, o.stream, true, &c))) {
        return rc;
    }
    Workspace* w = c.w;
    if ((rc = w->pack.ensure(n, kPackCtrWords, !p->out))) {
        return rc;
    }
    HIP_TRY(hipMemsetAsync(w->pack.ctr.p, 0, 8 * kPackCtrWords, c.s));
    PackArgs a;
    memset(&a, 0, sizeof(a));
    a.src_bytes = p->src_bytes;
    a.src_offsets = p->src_offsets;
    a.lengths = p->lengths;
    a.queue_ids = p->queue_ids;
    a.guids = p->guids;
    a.flags = p->flags;
    a.event_first = p->event_first;
    a.n = n;
    a.n_events = n ? p->n_events : 0;
    a.max_event_bytes = p->max_event_bytes ? p->max_event_bytes : kPutMaxSizeSoft;
    a.dst = (uint8_t*)p->dst;
    a.dst_bytes = p->dst_bytes;
    a.event_offsets = p->event_offsets;
    a.out = p->out ? p->out : (uint32_t*)w->pack.out.p;
    a.off = (unsigned long long*)w->pack.off.p;
    a.bsum = (unsigned long long*)w->pack.bsum.p;
    a.ctr = (unsigned long long*)w->pack.ctr.p;
    if (n) {
        layout_split(n, &a.per_block, &a.nblocks);
        if (bmqcrc_launch_put_layout(&a, (void*)c.s)) {
            return launch_failed("put-pack layout");
        }
    }
    if ((rc = enqueue_payload(c, w->pack, kPackCtrWords, p->src, a))) {
        return rc;
    }
    if (n && bmqcrc_launch_put_frame(&a, (void*)c.s)) {
        return launch_failed("put-pack frame");
    }
    w->pack.n = n;
    w->pack_events = a.n_events;
    w->pack.any = true;
    if (o.flags & BMQCRC_F_ASYNC) {
        return 0;
    }
    uint32_t kind;
    uint64_t index, total;
    if ((rc = pack_result(c, &kind, &index, &total))) {
        return rc;
    }
    if (total_bytes) {
        *total_bytes = total;
    }
    return kind ? refused(kPackRefusals, kind, index) : 0;
}

int bmqcrc_last_put_pack(int device, void* stream, uint64_t* n_msgs, uint64_t* n_events,
                         uint64_t* total_bytes, uint32_t* refused_kind, uint64_t* refused_index)
{
    t_err.clear();
    DeviceGuard keep_device;
    LockedCtx c;
    int rc;
    uint32_t kind = 0;
    uint64_t index = 0, total = 0;
    if ((rc = lock_on(device, stream, true, &c)) ||
        (c.w->pack.any && (rc = pack_result(c, &kind, &index, &total)))) {
        return rc;
    }
    if (n_msgs) {
        *n_msgs = c.w->pack.n;
    }
    if (n_events) {
        *n_events = c.w->pack_events;
    }
    if (total_bytes) {
        *total_bytes = total;
    }
    if (refused_kind) {
        *refused_kind = kind;
    }
    if (refused_index) {
        *refused_index = index;
    }
    return 0;
}

static_assert(BMQCRC_REC_PACK_RECORD_TOO_BIG == BMQCRC_REC_KIND_RECORD_TOO_BIG &&
                  BMQCRC_REC_PACK_SRC_RANGE == BMQCRC_REC_KIND_SRC_RANGE &&
                  BMQCRC_REC_PACK_DST_TOO_SMALL == BMQCRC_REC_KIND_DST_TOO_SMALL &&
                  BMQCRC_REC_PACK_DATA_FILE_FULL == BMQCRC_REC_KIND_DATA_FILE_FULL &&
                  BMQCRC_REC_PACK_TOO_MANY_PIECES == BMQCRC_REC_KIND_TOO_MANY_PIECES,
              "the kernels' refusal kinds are the public ones");

constexpr uint64_t kJournalRecordBytes = 60;       // FileStoreProtocol::k_JOURNAL_RECORD_SIZE
constexpr uint64_t kMaxSeqNum = (1ull << 48) - 1;  // RecordHeader: 48 bits of sequence number

// Result of the records pack last enqueued on c's workspace, after everything
// enqueued on its stream (w->mu held); zeros when there was none.
static int records_result(Ctx& c, bmqcrc_records_result* r)
{
    memset(r, 0, sizeof(*r));
    if (!c.w->rec.any) {
        return 0;
    }
    unsigned long long ctr[kRecCtrWords + kCopyCtrWords];
    const int rc = pack_counters(c, c.w->rec, kRecCtrWords, "bmqcrc_message_records_pack", ctr,
                                 &r->refused_kind, &r->refused_index);
    if (rc) {
        return rc;
    }
    r->n_msgs = c.w->rec.n;
    r->first_bad = r->n_msgs;
    if (r->refused_kind) {
        return 0;
    }
    r->data_bytes = r->n_msgs ? ctr[kRecCtrTotal] : 0;
    r->journal_bytes = kJournalRecordBytes * r->n_msgs;
    r->n_bad = ctr[kRecCtrBad];
    if (r->n_bad) {
        r->first_bad = ~ctr[kRecCtrFirstBad];
    }
    return 0;
}

static const char* const kRecordsRefusals[6] = {
    "", "BMQCRC_REC_PACK_RECORD_TOO_BIG: message %llu makes a record above 2^29-1 words",
    "BMQCRC_REC_PACK_SRC_RANGE: message %llu lies outside [src, src+src_bytes)",
    "BMQCRC_REC_PACK_DST_TOO_SMALL: the record of message %llu ends past dst_bytes",
    "BMQCRC_REC_PACK_DATA_FILE_FULL: the record of message %llu ends past 8*(2^32-1) bytes "
    "of DATA file, where MessageOffsetDwords stops",
    "BMQCRC_REC_PACK_TOO_MANY_PIECES: more than 2^32-1 16-byte pieces of payload in one "
    "call (index %llu)"};

int bmqcrc_message_records_pack(const bmqcrc_records_pack* p, bmqcrc_records_result* result,
                                const bmqcrc_opts* opts)
{
    t_err.clear();
    DeviceGuard keep_device;
    // every refusal below answers before the device lookup (no GPU needed)
    bmqcrc_opts o;
    int rc;
    if ((rc = check_struct(p, "bmqcrc_records_pack")) ||
        (rc = device_call_opts(opts, "bmqcrc_message_records_pack", &o))) {
        return rc;
    }
    const uint64_t n = p->n;
    if (n > 0xFFFFFFFFull) {
        return fail(BMQCRC_EINVAL, "at most 2^32-1 messages per call");
    }
    if (n && (rc = refuse_null({{!p->src_offsets, "src_offsets"},
                                {!p->lengths, "lengths"},
                                {!p->queue_keys, "queue_keys"},
                                {!p->guids, "guids"},
                                {!p->dst, "dst"},
                                {!p->journal_dst, "journal_dst"},
                                {!p->src && p->src_bytes, "src"}}))) {
        return rc;
    }
    if ((uintptr_t)p->dst & 7u) {
        return fail(BMQCRC_EINVAL, "dst must be 8-byte aligned");
    }
    if ((uintptr_t)p->journal_dst & 3u) {
        return fail(BMQCRC_EINVAL, "journal_dst must be 4-byte aligned");
    }
    if (p->data_file_pos == 0 || (p->data_file_pos & 7u)) {
        return fail(BMQCRC_EINVAL, "data_file_pos must be a multiple of 8 and not 0 (recovery "
                                   "treats a MessageOffsetDwords of 0 as invalid)");
    }
    if (p->lease_id == 0) {
        return fail(BMQCRC_EINVAL, "lease_id must not be 0");
    }
    if (p->first_seq == 0 || p->first_seq > kMaxSeqNum ||
        (n && n - 1 > kMaxSeqNum - p->first_seq)) {
        return fail(BMQCRC_EINVAL, "first_seq must not be 0, and first_seq + n - 1 at most 2^48-1");
    }
    if (kJournalRecordBytes * n > p->journal_bytes) {
        return fail(BMQCRC_EINVAL, "journal_bytes is below 60 n");
    }
    {
        const struct {
            uintptr_t at;
            uint64_t bytes;
            const char* name;
        } r[] = {{(uintptr_t)p->src, p->src_bytes, "[src, src+src_bytes)"},
                 {(uintptr_t)p->dst, p->dst_bytes, "[dst, dst+dst_bytes)"},
                 {(uintptr_t)p->journal_dst, p->journal_bytes,
                  "[journal_dst, journal_dst+journal_bytes)"}};
        for (int i = 1; i < 3; ++i) {
            for (int j = 0; j < i; ++j) {
                if (overlaps(r[i].at, r[i].bytes, r[j].at, r[j].bytes)) {
                    return fail(BMQCRC_EINVAL, std::string(r[i].name) + " overlaps " + r[j].name);
                }
            }
        }
    }
    LockedCtx c;
    if ((rc = lock_on(o.device, o.stream, true, &c))) {
        return rc;
    }
    Workspace* w = c.w;
    if ((rc = w->rec.ensure(n, kRecCtrWords, !p->out))) {
        return rc;
    }
    HIP_TRY(hipMemsetAsync(w->rec.ctr.p, 0, 8 * kRecCtrWords, c.s));
    RecArgs a;
    memset(&a, 0, sizeof(a));
    a.src_bytes = p->src_bytes;
    a.src_offsets = p->src_offsets;
    a.lengths = p->lengths;
    a.queue_keys = p->queue_keys;
    a.guids = p->guids;
    a.data_flags = p->data_flags;
    a.ref_counts = p->ref_counts;
    a.timestamps = p->timestamps;
    a.expected = p->expected;
    a.n = n;
    a.first_seq = p->first_seq;
    a.timestamp = p->timestamp;
    a.data_file_pos = p->data_file_pos;
    a.lease_id = p->lease_id;
    const uint8_t* fk = p->file_key;
    a.key_lo = (uint32_t)fk[0] << 24;
    a.key_hi = (uint32_t)fk[1] | ((uint32_t)fk[2] << 8) | ((uint32_t)fk[3] << 16) |
               ((uint32_t)fk[4] << 24);
    a.dst = (uint8_t*)p->dst;
    a.dst_bytes = p->dst_bytes;
    a.journal = (uint8_t*)p->journal_dst;
    a.record_offsets = p->record_offsets;
    a.out = p->out ? p->out : (uint32_t*)w->rec.out.p;
    a.off = (unsigned long long*)w->rec.off.p;
    a.bsum = (unsigned long long*)w->rec.bsum.p;
    a.ctr = (unsigned long long*)w->rec.ctr.p;
    if (n) {
        layout_split(n, &a.per_block, &a.nblocks);
        if (bmqcrc_launch_records_layout(&a, (void*)c.s)) {
            return launch_failed("records-pack layout");
        }
    }
    if ((rc = enqueue_payload(c, w->rec, kRecCtrWords, p->src, a))) {
        return rc;
    }
    if (n && bmqcrc_launch_records_frame(&a, (void*)c.s)) {
        return launch_failed("records-pack frame");
    }
    w->rec.n = n;
    w->rec.any = true;
    bmqcrc_records_result r;
    if ((rc = sync_result(c, o, records_result, result, &r))) {
        return rc;
    }
    return r.refused_kind ? refused(kRecordsRefusals, r.refused_kind, r.refused_index) : 0;
}

int bmqcrc_last_records_pack(int device, void* stream, bmqcrc_records_result* result)
{
    return last_result(device, stream, records_result, result);
}

static_assert(BMQCRC_PUT_UNPACK_EVENT_OFFSETS == BMQCRC_UNPACK_KIND_EVENT_OFFSETS &&
                  BMQCRC_PUT_UNPACK_EVENT_HEADER == BMQCRC_UNPACK_KIND_EVENT_HEADER &&
                  BMQCRC_PUT_UNPACK_PUT_HEADER == BMQCRC_UNPACK_KIND_PUT_HEADER &&
                  BMQCRC_PUT_UNPACK_PADDING == BMQCRC_UNPACK_KIND_PADDING &&
                  BMQCRC_PUT_UNPACK_TOO_MANY_MESSAGES == BMQCRC_UNPACK_KIND_TOO_MANY_MESSAGES,
              "the kernels' refusal kinds are the public ones");

// Result of the unpack last enqueued on c's workspace, after everything
// enqueued on its stream (w->mu held); zeros when there was none.
static int unpack_result(Ctx& c, bmqcrc_put_unpack_result* r)
{
    unsigned long long ctr[kSlotCtrWords];
    const int rc = slot_counters(c, c.w->unp, ctr, r, &r->refused_event);
    if (!rc) {
        r->n_events = c.w->unp.n;
        r->refused_offset = r->refused_kind ? ctr[kUnpCtrOffset] : 0;
    }
    return rc;
}

static const char* const kUnpackRefusals[6] = {
    "", "BMQCRC_PUT_UNPACK_EVENT_OFFSETS: event_offsets[%llu] is above its successor, no "
        "multiple of 4, or the event ends past events_bytes (offset %llu)",
    "BMQCRC_PUT_UNPACK_EVENT_HEADER: event %llu has a malformed EventHeader (offset %llu)",
    "BMQCRC_PUT_UNPACK_PUT_HEADER: event %llu has a truncated or inconsistent PutHeader "
    "(offset %llu)",
    "BMQCRC_PUT_UNPACK_PADDING: event %llu has invalid PUT message padding (offset %llu)",
    "BMQCRC_PUT_UNPACK_TOO_MANY_MESSAGES: the messages of event %llu do not fit msg_cap "
    "(offset %llu)"};

int bmqcrc_put_event_unpack(const bmqcrc_put_unpack* p, bmqcrc_put_unpack_result* result,
                            const bmqcrc_opts* opts)
{
    t_err.clear();
    DeviceGuard keep_device;
    // every refusal below answers before the device lookup (no GPU needed)
    bmqcrc_opts o;
    int rc;
    if ((rc = check_struct(p, "bmqcrc_put_unpack")) ||
        (rc = device_call_opts(opts, "bmqcrc_put_event_unpack", &o))) {
        return rc;
    }
    if ((rc = refuse_null({{!p->events, "events"},
                           {!p->app_offsets, "app_offsets"},
                           {!p->lengths, "lengths"}}))) {
        return rc;
    }
    if ((uintptr_t)p->events & 3u) {
        return fail(BMQCRC_EINVAL, "events must be 4-byte aligned");
    }
    if (!p->event_offsets && p->n_events != 1) {
        return fail(BMQCRC_EINVAL, "event_offsets == NULL means one event: n_events must be 1");
    }
    if (p->n_events > 0xFFFFFFFFull || p->msg_cap > 0xFFFFFFFFull) {
        return fail(BMQCRC_EINVAL, "n_events and msg_cap must be below 2^32");
    }
    const uint64_t cap = p->msg_cap;
    if ((rc = refuse_overlap({{p->app_offsets, 8 * cap, "app_offsets"},
                              {p->lengths, 4 * cap, "lengths"},
                              {p->queue_ids, 4 * cap, "queue_ids"},
                              {p->guids, 16 * cap, "guids"},
                              {p->flags, cap, "flags"},
                              {p->expected, 4 * cap, "expected"},
                              {p->out, 4 * cap, "out"},
                              {p->event_first, 8 * (p->n_events + 1), "event_first"}},
                             {{p->events, p->events_bytes, "[events, events+events_bytes)"}}))) {
        return rc;
    }
    LockedCtx c;
    if ((rc = lock_on(o.device, o.stream, true, &c))) {
        return rc;
    }
    Workspace* w = c.w;
    UnpackScratch& s = w->unp;
    if ((rc = s.ensure(cap, p->out != nullptr)) ||
        (rc = w->unp_first.ensure(8 * (p->n_events + 1))) ||
        (rc = w->unp_bad.ensure(8 * std::max<uint64_t>(p->n_events, 1)))) {
        return rc;
    }
    HIP_TRY(hipMemsetAsync(s.ctr.p, 0, 8 * kSlotCtrWords, c.s));
    s.n = p->n_events;
    s.any = true;
    if (p->n_events) {
        UnpackArgs a;
        memset(&a, 0, sizeof(a));
        a.events = (const uint8_t*)p->events;
        a.events_bytes = p->events_bytes;
        a.event_offsets = p->event_offsets;
        a.n_events = p->n_events;
        a.msg_cap = cap;
        a.app_offsets = p->app_offsets;
        a.lengths = p->lengths;
        a.queue_ids = p->queue_ids;
        a.guids = p->guids;
        a.flags = p->flags;
        a.expected = p->expected;
        a.out = p->out;
        a.event_first = p->event_first;
        a.ws_off = (unsigned long long*)s.off.p;
        a.ws_len = (uint32_t*)s.len.p;
        a.ws_exp = (uint32_t*)s.exp.p;
        a.ws_out = (const uint32_t*)s.out.p;
        a.first = (unsigned long long*)w->unp_first.p;
        a.bad_off = (unsigned long long*)w->unp_bad.p;
        a.ctr = (unsigned long long*)s.ctr.p;
        if (bmqcrc_launch_unpack_walk(&a, (void*)c.s)) {
            return launch_failed("put-unpack walk");
        }
        if (p->out && (rc = fold_slots(c, s, p->events, p->events_bytes, cap))) {
            return rc;
        }
        if (bmqcrc_launch_unpack_publish(&a, (void*)c.s)) {
            return launch_failed("put-unpack publish");
        }
    }
    bmqcrc_put_unpack_result r;
    if ((rc = sync_result(c, o, unpack_result, result, &r))) {
        return rc;
    }
    return r.refused_kind
               ? refused(kUnpackRefusals, r.refused_kind, r.refused_event, r.refused_offset)
               : 0;
}

int bmqcrc_last_put_unpack(int device, void* stream, bmqcrc_put_unpack_result* result)
{
    return last_result(device, stream, unpack_result, result);
}

static_assert(BMQCRC_REC_UNPACK_RECORD_HEADER == BMQCRC_RECUNP_KIND_RECORD_HEADER &&
                  BMQCRC_REC_UNPACK_MESSAGE_RECORD == BMQCRC_RECUNP_KIND_MESSAGE_RECORD &&
                  BMQCRC_REC_UNPACK_DATA_OFFSET == BMQCRC_RECUNP_KIND_DATA_OFFSET &&
                  BMQCRC_REC_UNPACK_DATA_RECORD == BMQCRC_RECUNP_KIND_DATA_RECORD &&
                  BMQCRC_REC_UNPACK_TOO_MANY_MESSAGES == BMQCRC_RECUNP_KIND_TOO_MANY_MESSAGES,
              "the kernels' refusal kinds are the public ones");
static_assert(kJournalRecordBytes == 4 * kJournalRecordDwords, "a journal record is 15 dwords");

// Result of the records unpack last enqueued on c's workspace, after
// everything enqueued on its stream (w->mu held); zeros when there was none.
static int records_unpack_result(Ctx& c, bmqcrc_records_unpack_result* r)
{
    unsigned long long ctr[kSlotCtrWords];
    const int rc = slot_counters(c, c.w->runp, ctr, r, &r->refused_index);
    if (!rc) {
        r->n_records = c.w->runp.n;
        r->n_skipped = r->refused_kind ? 0 : ctr[kRecUnpCtrSkipped];
    }
    return rc;
}

static const char* const kRecordsUnpackRefusals[6] = {
    "", "BMQCRC_REC_UNPACK_RECORD_HEADER: record %llu has type 0, lease id 0, sequence number 0 "
        "or a wrong magic",
    "BMQCRC_REC_UNPACK_MESSAGE_RECORD: MESSAGE record %llu has a null GUID or queue key",
    "BMQCRC_REC_UNPACK_DATA_OFFSET: MESSAGE record %llu points at offset 0 or outside "
    "[data_file_pos, data_file_pos+data_bytes]",
    "BMQCRC_REC_UNPACK_DATA_RECORD: MESSAGE record %llu points at a malformed DATA record",
    "BMQCRC_REC_UNPACK_TOO_MANY_MESSAGES: the message of record %llu does not fit msg_cap"};

int bmqcrc_message_records_unpack(const bmqcrc_records_unpack* p,
                                  bmqcrc_records_unpack_result* result, const bmqcrc_opts* opts)
{
    t_err.clear();
    DeviceGuard keep_device;
    // every refusal below answers before the device lookup (no GPU needed)
    bmqcrc_opts o;
    int rc;
    if ((rc = check_struct(p, "bmqcrc_records_unpack")) ||
        (rc = device_call_opts(opts, "bmqcrc_message_records_unpack", &o))) {
        return rc;
    }
    if ((rc = refuse_null({{!p->journal, "journal"},
                           {!p->data, "data"},
                           {!p->app_offsets, "app_offsets"},
                           {!p->lengths, "lengths"}}))) {
        return rc;
    }
    if ((uintptr_t)p->journal & 3u) {
        return fail(BMQCRC_EINVAL, "journal must be 4-byte aligned");
    }
    if ((uintptr_t)p->data & 7u) {
        return fail(BMQCRC_EINVAL, "data must be 8-byte aligned");
    }
    if (p->data_file_pos & 7u) {
        return fail(BMQCRC_EINVAL, "data_file_pos must be a multiple of 8");
    }
    if (p->n_records > 0xFFFFFFFFull || p->msg_cap > 0xFFFFFFFFull) {
        return fail(BMQCRC_EINVAL, "n_records and msg_cap must be below 2^32");
    }
    if (kJournalRecordBytes * p->n_records > p->journal_bytes) {
        return fail(BMQCRC_EINVAL, "journal_bytes is below 60 n_records");
    }
    const uint64_t n = p->n_records, cap = p->msg_cap;
    if ((rc = refuse_overlap({{p->record_index, 4 * cap, "record_index"},
                              {p->app_offsets, 8 * cap, "app_offsets"},
                              {p->lengths, 4 * cap, "lengths"},
                              {p->queue_keys, 5 * cap, "queue_keys"},
                              {p->guids, 16 * cap, "guids"},
                              {p->data_flags, cap, "data_flags"},
                              {p->ref_counts, 4 * cap, "ref_counts"},
                              {p->timestamps, 8 * cap, "timestamps"},
                              {p->expected, 4 * cap, "expected"},
                              {p->out, 4 * cap, "out"}},
                             {{p->journal, p->journal_bytes, "[journal, journal+journal_bytes)"},
                              {p->data, p->data_bytes, "[data, data+data_bytes)"}}))) {
        return rc;
    }
    LockedCtx c;
    if ((rc = lock_on(o.device, o.stream, true, &c))) {
        return rc;
    }
    Workspace* w = c.w;
    UnpackScratch& s = w->runp;
    const uint64_t recs = std::max<uint64_t>(n, 1);
    if ((rc = s.ensure(cap, p->out != nullptr)) ||
        (rc = w->runp_bsum.ensure(8ull * 2 * kPackBlocks)) || (rc = w->runp_pre.ensure(4 * recs)) ||
        (rc = w->runp_roff.ensure(8 * recs)) || (rc = w->runp_rlen.ensure(4 * recs)) ||
        (rc = w->runp_rflags.ensure(recs))) {
        return rc;
    }
    HIP_TRY(hipMemsetAsync(s.ctr.p, 0, 8 * kSlotCtrWords, c.s));
    s.n = n;
    s.any = true;
    if (n) {
        RecUnpackArgs a;
        memset(&a, 0, sizeof(a));
        a.journal = (const uint32_t*)p->journal;
        a.n_records = n;
        a.data = (const uint8_t*)p->data;
        a.data_bytes = p->data_bytes;
        a.data_file_pos = p->data_file_pos;
        a.select = p->select;
        a.msg_cap = cap;
        a.record_index = p->record_index;
        a.app_offsets = p->app_offsets;
        a.lengths = p->lengths;
        a.queue_keys = p->queue_keys;
        a.guids = p->guids;
        a.data_flags = p->data_flags;
        a.ref_counts = p->ref_counts;
        a.timestamps = p->timestamps;
        a.expected = p->expected;
        a.out = p->out;
        a.ws_off = (unsigned long long*)s.off.p;
        a.ws_len = (uint32_t*)s.len.p;
        a.ws_exp = (uint32_t*)s.exp.p;
        a.ws_out = (const uint32_t*)s.out.p;
        a.pre = (uint32_t*)w->runp_pre.p;
        a.rec_off = (unsigned long long*)w->runp_roff.p;
        a.rec_len = (uint32_t*)w->runp_rlen.p;
        a.rec_flags = (uint8_t*)w->runp_rflags.p;
        a.bsum = (unsigned long long*)w->runp_bsum.p;
        a.ctr = (unsigned long long*)s.ctr.p;
        layout_split(n, &a.per_block, &a.nblocks);
        if (bmqcrc_launch_records_unpack_walk(&a, (void*)c.s)) {
            return launch_failed("records-unpack walk");
        }
        if (p->out && (rc = fold_slots(c, s, p->data, p->data_bytes, cap))) {
            return rc;
        }
        if (bmqcrc_launch_records_unpack_publish(&a, (void*)c.s)) {
            return launch_failed("records-unpack publish");
        }
    }
    bmqcrc_records_unpack_result r;
    if ((rc = sync_result(c, o, records_unpack_result, result, &r))) {
        return rc;
    }
    return r.refused_kind ? refused(kRecordsUnpackRefusals, r.refused_kind, r.refused_index) : 0;
}

int bmqcrc_last_records_unpack(int device, void* stream, bmqcrc_records_unpack_result* result)
{
    return last_result(device, stream, records_unpack_result, result);
}

// Result of the journal select last enqueued on c's workspace, after
// everything enqueued on its stream (w->mu held); zeros when there was none.
static int journal_select_result(Ctx& c, bmqcrc_journal_select_result* r)
{
    memset(r, 0, sizeof(*r));
    if (!c.w->jsel_any) {
        return 0;
    }
    unsigned long long ctr[kJselCtrWords] = {0};
    const uint64_t n = c.w->jsel_records;
    if (n) {
        HIP_TRY(hipMemcpyAsync(ctr, c.w->jsel_zero.p, sizeof(ctr), hipMemcpyDeviceToHost, c.s));
    }
    HIP_TRY(hipStreamSynchronize(c.s));
    r->n_records = n;
    r->first_record = ctr[kJselCtrFirst];
    r->n_selected = ctr[kJselCtrSelected];
    r->n_deleted = ctr[kJselCtrDeleted];
    r->n_purged = ctr[kJselCtrPurged];
    r->error_record = n;
    if (ctr[kJselCtrRefused]) {
        r->refused_kind = BMQCRC_JSEL_TOO_MANY_QUEUES;
        return 0;
    }
    const unsigned long long failure =
        ctr[kJselCtrFail1] ? ctr[kJselCtrFail1] : ctr[kJselCtrFail2];
    if (failure) {
        r->recovery_rc = -(int32_t)(failure & 0xFFu);
        r->error_record = (failure >> 8) - 1;
    }
    return 0;
}

static uint64_t pow2_at_least(uint64_t v)
{
    uint64_t p = 64;
    while (p < v) {
        p <<= 1;
    }
    return p;
}

int bmqcrc_journal_select(const bmqcrc_journal_select_args* p, bmqcrc_journal_select_result* result,
                          const bmqcrc_opts* opts)
{
    t_err.clear();
    DeviceGuard keep_device;
    // every refusal below answers before the device lookup (no GPU needed)
    bmqcrc_opts o;
    int rc;
    if ((rc = check_struct(p, "bmqcrc_journal_select_args", p ? p->reserved2 : 0,
                           ".reserved and reserved2 must be 0")) ||
        (rc = device_call_opts(opts, "bmqcrc_journal_select", &o))) {
        return rc;
    }
    const struct {
        bool bad;
        const char* what;
    } checks[] = {{!p->journal, "null pointer argument: journal"},
                  {!p->select, "null pointer argument: select"},
                  {p->n_queue_keys && !p->queue_keys, "null pointer argument: queue_keys"},
                  {((uintptr_t)p->journal & 3u) != 0, "journal must be 4-byte aligned"},
                  {p->n_records > 0xFFFFFFFFull, "n_records must be below 2^32"},
                  {p->journal_bytes != kJournalRecordBytes * p->n_records,
                   "journal_bytes must be 60 n_records"},
                  {p->queue_cap == 0, "queue_cap must not be 0"}};
    for (const auto& k : checks) {
        if (k.bad) {
            return fail(BMQCRC_EINVAL, std::string("bmqcrc_journal_select: ") + k.what);
        }
    }
    LockedCtx c;
    if ((rc = lock_on(o.device, o.stream, true, &c))) {
        return rc;
    }
    Workspace* w = c.w;
    const uint64_t n = p->n_records;
    const uint64_t nkeys = p->with_csl ? p->n_queue_keys : 0;
    w->jsel_records = n;
    w->jsel_any = true;
    if (n) {
        // no more distinct keys than QueueOp records and queue_keys together
        const uint64_t qslots = pow2_at_least(2 * std::min(p->queue_cap, n + nkeys));
        const uint64_t gslots = pow2_at_least(2 * n);
        const uint64_t zero_bytes = 8ull * kJselCtrWords + 24 * qslots + 4 * gslots + 4 * n;
        if ((rc = w->jsel_zero.ensure(zero_bytes)) || (rc = w->jsel_rec.ensure(13 * n))) {
            return rc;
        }
        HIP_TRY(hipMemsetAsync(w->jsel_zero.p, 0, zero_bytes, c.s));
        JselArgs a;
        memset(&a, 0, sizeof(a));
        a.journal = (const uint32_t*)p->journal;
        a.n_records = n;
        a.data_file_bytes = p->data_file_bytes;
        a.queue_keys = p->queue_keys;
        a.n_queue_keys = nkeys;
        a.queue_cap = p->queue_cap;
        a.select = p->select;
        a.with_csl = p->with_csl != 0;
        a.ctr = (unsigned long long*)w->jsel_zero.p;
        a.qkey = a.ctr + kJselCtrWords;
        a.qdel = (uint32_t*)(a.qkey + qslots);
        a.qtop = a.qdel + qslots;
        a.qpurge = a.qtop + qslots;
        a.qcsl = a.qpurge + qslots;
        a.gslot = a.qcsl + qslots;
        a.claim = a.gslot + gslots;
        a.qlist = (uint32_t*)w->jsel_rec.p;
        a.slist = a.qlist + n;
        a.names = a.slist + n;
        a.state = (uint8_t*)(a.names + n);
        a.qslots = qslots;
        a.gslots = gslots;
        layout_split(n, &a.per_block, &a.nblocks);
        if (bmqcrc_launch_journal_select(&a, (void*)c.s)) {
            return launch_failed("journal-select");
        }
    }
    bmqcrc_journal_select_result r;
    if ((rc = sync_result(c, o, journal_select_result, result, &r))) {
        return rc;
    }
    return r.refused_kind
               ? fail(BMQCRC_EINVAL, "BMQCRC_JSEL_TOO_MANY_QUEUES: the journal's QueueOp records "
                                     "and queue_keys hold more distinct queue keys than queue_cap: "
                                     "nothing was selected")
               : 0;
}

int bmqcrc_last_journal_select(int device, void* stream, bmqcrc_journal_select_result* result)
{
    return last_result(device, stream, journal_select_result, result);
}

static_assert(BMQCRC_STORAGE_APPLY_EVENT_OFFSETS == BMQCRC_SAP_KIND_EVENT_OFFSETS &&
                  BMQCRC_STORAGE_APPLY_EVENT_HEADER == BMQCRC_SAP_KIND_EVENT_HEADER &&
                  BMQCRC_STORAGE_APPLY_STORAGE_HEADER == BMQCRC_SAP_KIND_STORAGE_HEADER &&
                  BMQCRC_STORAGE_APPLY_DATA_RECORD == BMQCRC_SAP_KIND_DATA_RECORD &&
                  BMQCRC_STORAGE_APPLY_TOO_MANY_MESSAGES == BMQCRC_SAP_KIND_TOO_MANY_MESSAGES &&
                  BMQCRC_STORAGE_APPLY_OUT_OF_SYNC == BMQCRC_SAP_KIND_OUT_OF_SYNC &&
                  BMQCRC_STORAGE_APPLY_DST_TOO_SMALL == BMQCRC_SAP_KIND_DST_TOO_SMALL &&
                  BMQCRC_STORAGE_APPLY_TOO_MANY_PIECES == BMQCRC_SAP_KIND_TOO_MANY_PIECES,
              "the kernels' refusal kinds are the public ones");

// Result of the storage apply last enqueued on c's workspace, after
// everything enqueued on its stream (w->mu held); zeros when there was none.
static int storage_apply_result(Ctx& c, bmqcrc_storage_apply_result* r)
{
    unsigned long long ctr[kSapCtrWords + kCopyCtrWords];
    const int rc = slot_counters(c, c.w->sap, ctr, r, &r->refused_event);
    if (rc || !c.w->sap.any) {
        return rc;
    }
    r->n_events = c.w->sap.n;
    if (r->refused_kind) {
        r->refused_event = ctr[kSapCtrEvent];
        r->refused_index = ctr[kSapCtrIndex];
        r->refused_offset = ctr[kSapCtrOffset];
        return 0;
    }
    if (int bad = copy_pass_clean(ctr + kSapCtrWords, "bmqcrc_storage_event_apply")) {
        return bad;
    }
    r->n_data = ctr[kSapCtrData];
    r->journal_bytes = kJournalRecordBytes * r->n_msgs;
    r->data_bytes = ctr[kSapCtrTotal];
    r->head_lease_id = r->n_msgs ? (uint32_t)ctr[kSapCtrHeadLease] : c.w->sap_lease;
    r->head_seq = r->n_msgs ? ctr[kSapCtrHeadSeq] : c.w->sap_seq;
    return 0;
}

static const char* const kStorageApplyRefusals[9] = {
    "", "BMQCRC_STORAGE_APPLY_EVENT_OFFSETS: event_offsets[%llu] is above its successor, no "
        "multiple of 4, or the event ends past events_bytes (offset %llu, message %llu)",
    "BMQCRC_STORAGE_APPLY_EVENT_HEADER: event %llu has a malformed EventHeader (offset %llu, "
    "message %llu)",
    "BMQCRC_STORAGE_APPLY_STORAGE_HEADER: event %llu has a truncated or inconsistent "
    "StorageHeader, or one of another partition (offset %llu, message %llu)",
    "BMQCRC_STORAGE_APPLY_DATA_RECORD: event %llu has a DATA message with a malformed DATA "
    "record (offset %llu, message %llu)",
    "BMQCRC_STORAGE_APPLY_TOO_MANY_MESSAGES: the messages of event %llu do not fit msg_cap "
    "(offset %llu, message %llu)",
    "BMQCRC_STORAGE_APPLY_OUT_OF_SYNC: event %llu has a message that does not continue the "
    "journal, the DATA file or the sequence numbers (offset %llu, message %llu)",
    "BMQCRC_STORAGE_APPLY_DST_TOO_SMALL: event %llu has the first message that ends past "
    "journal_dst_bytes or data_dst_bytes (offset %llu, message %llu)",
    "BMQCRC_STORAGE_APPLY_TOO_MANY_PIECES: more than 2^32-1 16-byte pieces of application data "
    "in one call (event %llu, offset %llu, message %llu)"};

int bmqcrc_storage_event_apply(const bmqcrc_storage_apply* p, bmqcrc_storage_apply_result* result,
                               const bmqcrc_opts* opts)
{
    t_err.clear();
    DeviceGuard keep_device;
    // every refusal below answers before the device lookup (no GPU needed)
    bmqcrc_opts o;
    int rc;
    if ((rc = check_struct(p, "bmqcrc_storage_apply")) ||
        (rc = device_call_opts(opts, "bmqcrc_storage_event_apply", &o))) {
        return rc;
    }
    if ((rc = refuse_null({{!p->events, "events"},
                           {!p->journal_dst, "journal_dst"},
                           {!p->data_dst, "data_dst"}}))) {
        return rc;
    }
    const struct {
        bool bad;
        const char* what;
    } checks[] = {
        {((uintptr_t)p->events & 3u) != 0, "events must be 4-byte aligned"},
        {((uintptr_t)p->journal_dst & 3u) != 0, "journal_dst must be 4-byte aligned"},
        {((uintptr_t)p->data_dst & 7u) != 0, "data_dst must be 8-byte aligned"},
        {!p->event_offsets && p->n_events != 1,
         "event_offsets == NULL means one event: n_events must be 1"},
        {p->n_events > 0xFFFFFFFFull || p->msg_cap > 0xFFFFFFFFull,
         "n_events and msg_cap must be below 2^32"},
        {p->journal_pos == 0 || (p->journal_pos & 3u),
         "journal_pos must be a multiple of 4 and not 0 (a journal begins with its file headers)"},
        {p->data_file_pos == 0 || (p->data_file_pos & 7u),
         "data_file_pos must be a multiple of 8 and not 0 (recovery treats a MessageOffsetDwords "
         "of 0 as invalid)"},
        {p->partition_id > 0xFFFFu, "partition_id must be at most 65535"},
        {p->lease_id == 0 && p->seq != 0,
         "lease_id == 0 means no write head is known: seq must be 0"}};
    for (const auto& k : checks) {
        if (k.bad) {
            return fail(BMQCRC_EINVAL, k.what);
        }
    }
    const uint64_t cap = p->msg_cap;
    const NamedRange events = {p->events, p->events_bytes, "[events, events+events_bytes)"};
    const NamedRange journal = {p->journal_dst, p->journal_dst_bytes,
                                "[journal_dst, journal_dst+journal_dst_bytes)"};
    const NamedRange data = {p->data_dst, p->data_dst_bytes, "[data_dst, data_dst+data_dst_bytes)"};
    if ((rc = refuse_overlap({journal, data}, {events})) ||
        (rc = refuse_overlap({data}, {journal})) ||
        (rc = refuse_overlap({{p->types, cap, "types"},
                              {p->flags, cap, "flags"},
                              {p->payload_offsets, 8 * cap, "payload_offsets"},
                              {p->payload_lengths, 4 * cap, "payload_lengths"},
                              {p->record_offsets, 8 * (cap + 1), "record_offsets"},
                              {p->lengths, 4 * cap, "lengths"},
                              {p->expected, 4 * cap, "expected"},
                              {p->out, 4 * cap, "out"},
                              {p->event_first, 8 * (p->n_events + 1), "event_first"}},
                             {events, journal, data}))) {
        return rc;
    }
    LockedCtx c;
    if ((rc = lock_on(o.device, o.stream, true, &c))) {
        return rc;
    }
    Workspace* w = c.w;
    SlotCopyScratch& s = w->sap;
    const uint64_t slots = std::max<uint64_t>(cap, 1);
    if ((rc = s.ensure(cap, true, kSapCtrWords)) ||
        (rc = w->sap_first.ensure(8 * (p->n_events + 1))) ||
        (rc = w->sap_bad.ensure(8 * std::max<uint64_t>(p->n_events, 1))) ||
        (rc = w->sap_jrn.ensure(8 * slots)) || (rc = w->sap_rec.ensure(4 * slots)) ||
        (rc = w->sap_hdr.ensure(4 * slots)) || (rc = w->sap_pay.ensure(4 * slots)) ||
        (rc = w->sap_meta.ensure(4 * slots)) || (rc = s.begin(c, kSapCtrWords, p->n_events))) {
        return rc;
    }
    w->sap_lease = p->lease_id;
    w->sap_seq = p->seq;
    if (p->n_events) {
        SapArgs a;
        memset(&a, 0, sizeof(a));
        a.events = (const uint8_t*)p->events;
        a.events_bytes = p->events_bytes;
        a.event_offsets = p->event_offsets;
        a.n_events = p->n_events;
        a.msg_cap = cap;
        a.journal_pos = p->journal_pos;
        a.data_file_pos = p->data_file_pos;
        a.seq = p->seq;
        a.lease_id = p->lease_id;
        a.partition_id = p->partition_id;
        a.journal_dst = (uint8_t*)p->journal_dst;
        a.journal_dst_bytes = p->journal_dst_bytes;
        a.data_dst = (uint8_t*)p->data_dst;
        a.data_dst_bytes = p->data_dst_bytes;
        a.types = p->types;
        a.flags = p->flags;
        a.payload_offsets = p->payload_offsets;
        a.payload_lengths = p->payload_lengths;
        a.record_offsets = p->record_offsets;
        a.lengths = p->lengths;
        a.expected = p->expected;
        a.out = p->out;
        a.event_first = p->event_first;
        a.ws_off = (unsigned long long*)s.off.p;
        a.ws_len = (uint32_t*)s.len.p;
        a.off = (unsigned long long*)s.dst.p;
        a.ws_exp = (uint32_t*)s.exp.p;
        a.ws_out = (const uint32_t*)s.out.p;
        a.ws_jrn = (unsigned long long*)w->sap_jrn.p;
        a.ws_rec = (uint32_t*)w->sap_rec.p;
        a.ws_hdr = (uint32_t*)w->sap_hdr.p;
        a.ws_pay = (uint32_t*)w->sap_pay.p;
        a.ws_meta = (uint32_t*)w->sap_meta.p;
        a.first = (unsigned long long*)w->sap_first.p;
        a.bad_off = (unsigned long long*)w->sap_bad.p;
        a.bsum = (unsigned long long*)s.bsum.p;
        a.ctr = (unsigned long long*)s.ctr.p;
        layout_split(slots, &a.per_block, &a.nblocks);
        if (bmqcrc_launch_storage_apply_layout(&a, (void*)c.s)) {
            return launch_failed("storage-apply layout");
        }
        if ((rc = s.enqueue_slot_copy(c, a.events, a.events_bytes, a.data_dst, a.data_dst_bytes, cap,
                                      kSapCtrWords))) {
            return rc;
        }
        if (bmqcrc_launch_storage_apply_frame(&a, (void*)c.s)) {
            return launch_failed("storage-apply frame");
        }
    }
    bmqcrc_storage_apply_result r;
    if ((rc = sync_result(c, o, storage_apply_result, result, &r))) {
        return rc;
    }
    return r.refused_kind ? refused(kStorageApplyRefusals, r.refused_kind, r.refused_event,
                                    r.refused_offset, r.refused_index)
                          : 0;
}

int bmqcrc_last_storage_apply(int device, void* stream, bmqcrc_storage_apply_result* result)
{
    return last_result(device, stream, storage_apply_result, result);
}

static_assert(BMQCRC_STORAGE_PACK_RECORD_HEADER == BMQCRC_SPK_KIND_RECORD_HEADER &&
                  BMQCRC_STORAGE_PACK_DATA_OFFSET == BMQCRC_SPK_KIND_DATA_OFFSET &&
                  BMQCRC_STORAGE_PACK_DATA_RECORD == BMQCRC_SPK_KIND_DATA_RECORD &&
                  BMQCRC_STORAGE_PACK_EVENT_FIRST == BMQCRC_SPK_KIND_EVENT_FIRST &&
                  BMQCRC_STORAGE_PACK_PAYLOAD_TOO_BIG == BMQCRC_SPK_KIND_PAYLOAD_TOO_BIG &&
                  BMQCRC_STORAGE_PACK_EVENT_TOO_BIG == BMQCRC_SPK_KIND_EVENT_TOO_BIG &&
                  BMQCRC_STORAGE_PACK_DST_TOO_SMALL == BMQCRC_SPK_KIND_DST_TOO_SMALL &&
                  BMQCRC_STORAGE_PACK_TOO_MANY_PIECES == BMQCRC_SPK_KIND_TOO_MANY_PIECES,
              "the kernels' refusal kinds are the public ones");

constexpr uint64_t kStorageMaxEventSoft = 512ull << 20;    // EventHeader::k_MAX_SIZE_SOFT
constexpr uint64_t kStorageMaxEventBytes = (1ull << 31) - 1;  // 31 bits of Length
constexpr uint64_t kStorageMaxPayloadSoft = 65ull << 20;   // StorageHeader::k_MAX_PAYLOAD_SIZE_SOFT
constexpr uint64_t kStorageMaxPayloadBytes = 4 * ((1ull << 27) - 1) - 12;  // 27 bits of MessageWords
constexpr uint64_t kJournalMaxBytes = 4 * 0xFFFFFFFFull;   // where JournalOffsetWords stops

// Result of the storage pack last enqueued on c's workspace, after everything
// enqueued on its stream (w->mu held); zeros when there was none.
static int storage_pack_result(Ctx& c, bmqcrc_storage_pack_result* r)
{
    unsigned long long ctr[kSpkCtrWords + kCopyCtrWords];
    const int rc = slot_counters(c, c.w->spk, ctr, r, &r->refused_index);
    if (rc || !c.w->spk.any) {
        return rc;
    }
    r->n_events = c.w->spk_events;
    if (r->refused_kind) {
        return 0;
    }
    if (int bad = copy_pass_clean(ctr + kSpkCtrWords, "bmqcrc_storage_event_pack")) {
        return bad;
    }
    r->n_data = ctr[kSpkCtrData];
    r->total_bytes = ctr[kSpkCtrTotal];
    return 0;
}

static const char* const kStoragePackRefusals[9] = {
    "", "BMQCRC_STORAGE_PACK_RECORD_HEADER: record %llu has type 0 or above 5, lease id 0, "
        "sequence number 0, a wrong magic or a QueueOpType outside 1..4",
    "BMQCRC_STORAGE_PACK_DATA_OFFSET: MESSAGE record %llu points at offset 0 or outside "
    "[data_file_pos, data_file_pos+data_bytes]",
    "BMQCRC_STORAGE_PACK_DATA_RECORD: MESSAGE record %llu points at a malformed DATA record",
    "BMQCRC_STORAGE_PACK_EVENT_FIRST: event_first[%llu] breaks 0 = first < ... < last = n_records",
    "BMQCRC_STORAGE_PACK_PAYLOAD_TOO_BIG: the journal and DATA record of record %llu are longer "
    "than max_payload_bytes",
    "BMQCRC_STORAGE_PACK_EVENT_TOO_BIG: event %llu is longer than max_event_bytes",
    "BMQCRC_STORAGE_PACK_DST_TOO_SMALL: event %llu ends past dst_bytes",
    "BMQCRC_STORAGE_PACK_TOO_MANY_PIECES: more than 2^32-1 16-byte pieces of application data "
    "in one call (index %llu)"};

int bmqcrc_storage_event_pack(const bmqcrc_storage_pack* p, bmqcrc_storage_pack_result* result,
                              const bmqcrc_opts* opts)
{
    t_err.clear();
    DeviceGuard keep_device;
    // every refusal below answers before the device lookup (no GPU needed)
    bmqcrc_opts o;
    int rc;
    if ((rc = check_struct(p, "bmqcrc_storage_pack", p ? p->reserved2 : 0,
                           ".reserved and reserved2 must be 0")) ||
        (rc = device_call_opts(opts, "bmqcrc_storage_event_pack", &o))) {
        return rc;
    }
    if ((rc = refuse_null({{!p->journal, "journal"}, {!p->data, "data"}, {!p->dst, "dst"}}))) {
        return rc;
    }
    const uint64_t n = p->n_records;
    const struct {
        bool bad;
        const char* what;
    } checks[] = {
        {((uintptr_t)p->journal & 3u) != 0, "journal must be 4-byte aligned"},
        {((uintptr_t)p->data & 7u) != 0, "data must be 8-byte aligned"},
        {((uintptr_t)p->dst & 3u) != 0, "dst must be 4-byte aligned"},
        {n > 0xFFFFFFFFull || p->journal_bytes != kJournalRecordBytes * n,
         "journal_bytes must be 60 n_records"},
        {!p->event_first && p->n_events != 1,
         "event_first == NULL means one event: n_events must be 1"},
        {n && (p->n_events < 1 || p->n_events > n),
         "n_events must lie in [1, n_records]: no event is empty"},
        {p->journal_pos == 0 || (p->journal_pos & 3u),
         "journal_pos must be a multiple of 4 and not 0 (a journal begins with its file headers)"},
        {p->journal_pos > kJournalMaxBytes ||
             kJournalRecordBytes * n > kJournalMaxBytes - p->journal_pos,
         "journal_pos + 60 n_records above 4 (2^32-1): JournalOffsetWords would overflow"},
        {(p->data_file_pos & 7u) != 0, "data_file_pos must be a multiple of 8"},
        {p->partition_id > 0xFFFFu, "partition_id must be at most 65535"},
        {p->event_type != 0 && p->event_type != 8 && p->event_type != 10,
         "event_type must be 8 (STORAGE), 10 (PARTITION_SYNC) or 0 (STORAGE)"},
        {p->storage_protocol_version > 3, "storage_protocol_version must be at most 3"},
        {p->max_event_bytes > kStorageMaxEventBytes,
         "max_event_bytes above 2^31-1: the EventHeader's length would overflow"},
        {p->max_payload_bytes > kStorageMaxPayloadBytes,
         "max_payload_bytes above 4 (2^27-1) - 12: MessageWords would overflow"}};
    for (const auto& k : checks) {
        if (k.bad) {
            return fail(BMQCRC_EINVAL, k.what);
        }
    }
    const uint64_t entries = 8 * (p->n_events + 1);
    const NamedRange journal = {p->journal, p->journal_bytes, "[journal, journal+journal_bytes)"};
    const NamedRange data = {p->data, p->data_bytes, "[data, data+data_bytes)"};
    const NamedRange flags = {p->flags, p->flags ? n : 0, "flags"};
    const NamedRange first = {p->event_first, p->event_first ? entries : 0, "event_first"};
    const NamedRange dst = {p->dst, p->dst_bytes, "[dst, dst+dst_bytes)"};
    const NamedRange offsets = {p->event_offsets, entries, "event_offsets"};
    const NamedRange types = {p->types, n, "types"};
    const NamedRange out = {p->out, 4 * n, "out"};
    if ((rc = refuse_overlap({dst, offsets, types, out}, {journal, data, flags, first})) ||
        (rc = refuse_overlap({offsets, types, out}, {dst})) ||
        (rc = refuse_overlap({types, out}, {offsets})) || (rc = refuse_overlap({out}, {types}))) {
        return rc;
    }
    LockedCtx c;
    if ((rc = lock_on(o.device, o.stream, true, &c))) {
        return rc;
    }
    Workspace* w = c.w;
    SlotCopyScratch& s = w->spk;
    const uint64_t recs = std::max<uint64_t>(n, 1);
    if ((rc = s.ensure(n, true, kSpkCtrWords)) || (rc = w->spk_rec.ensure(4 * recs)) ||
        (rc = w->spk_hdr.ensure(4 * recs)) || (rc = w->spk_type.ensure(recs)) ||
        (rc = s.begin(c, kSpkCtrWords, n))) {
        return rc;
    }
    w->spk_events = n ? p->n_events : 0;
    if (n) {
        SpkArgs a;
        memset(&a, 0, sizeof(a));
        a.journal = (const uint32_t*)p->journal;
        a.n = n;
        a.journal_pos = p->journal_pos;
        a.data = (const uint8_t*)p->data;
        a.data_bytes = p->data_bytes;
        a.data_file_pos = p->data_file_pos;
        a.flags = p->flags;
        a.event_first = p->event_first;
        a.n_events = p->n_events;
        a.max_event_bytes = p->max_event_bytes ? p->max_event_bytes : kStorageMaxEventSoft;
        a.max_payload_bytes = p->max_payload_bytes ? p->max_payload_bytes : kStorageMaxPayloadSoft;
        a.partition_id = p->partition_id;
        a.event_type = p->event_type ? p->event_type : 8u;
        a.spv = p->storage_protocol_version;
        a.dst = (uint8_t*)p->dst;
        a.dst_bytes = p->dst_bytes;
        a.event_offsets = p->event_offsets;
        a.types = p->types;
        a.out = p->out;
        a.ws_off = (unsigned long long*)s.off.p;
        a.ws_len = (uint32_t*)s.len.p;
        a.off = (unsigned long long*)s.dst.p;
        a.ws_exp = (uint32_t*)s.exp.p;
        a.ws_out = (const uint32_t*)s.out.p;
        a.ws_rec = (uint32_t*)w->spk_rec.p;
        a.ws_hdr = (uint32_t*)w->spk_hdr.p;
        a.ws_type = (uint8_t*)w->spk_type.p;
        a.bsum = (unsigned long long*)s.bsum.p;
        a.ctr = (unsigned long long*)s.ctr.p;
        layout_split(n, &a.per_block, &a.nblocks);
        if (bmqcrc_launch_storage_pack_layout(&a, (void*)c.s)) {
            return launch_failed("storage-pack layout");
        }
        if ((rc = s.enqueue_slot_copy(c, a.data, a.data_bytes, a.dst, a.dst_bytes, n,
                                      kSpkCtrWords))) {
            return rc;
        }
        if (bmqcrc_launch_storage_pack_frame(&a, (void*)c.s)) {
            return launch_failed("storage-pack frame");
        }
    }
    return sync_result_or_refusal(c, o, storage_pack_result, result, kStoragePackRefusals);
}

int bmqcrc_last_storage_pack(int device, void* stream, bmqcrc_storage_pack_result* result)
{
    return last_result(device, stream, storage_pack_result, result);
}

static_assert(BMQCRC_PUSH_PACK_RECORD_INDEX == BMQCRC_PPK_KIND_RECORD_INDEX &&
                  BMQCRC_PUSH_PACK_RECORD == BMQCRC_PPK_KIND_RECORD &&
                  BMQCRC_PUSH_PACK_DATA_OFFSET == BMQCRC_PPK_KIND_DATA_OFFSET &&
                  BMQCRC_PUSH_PACK_DATA_RECORD == BMQCRC_PPK_KIND_DATA_RECORD &&
                  BMQCRC_PUSH_PACK_FLAGS == BMQCRC_PPK_KIND_FLAGS &&
                  BMQCRC_PUSH_PACK_EVENT_FIRST == BMQCRC_PPK_KIND_EVENT_FIRST &&
                  BMQCRC_PUSH_PACK_PAYLOAD_TOO_BIG == BMQCRC_PPK_KIND_PAYLOAD_TOO_BIG &&
                  BMQCRC_PUSH_PACK_EVENT_TOO_BIG == BMQCRC_PPK_KIND_EVENT_TOO_BIG &&
                  BMQCRC_PUSH_PACK_DST_TOO_SMALL == BMQCRC_PPK_KIND_DST_TOO_SMALL &&
                  BMQCRC_PUSH_PACK_TOO_MANY_PIECES == BMQCRC_PPK_KIND_TOO_MANY_PIECES,
              "the kernels' refusal kinds are the public ones");

constexpr uint64_t kPushMaxPayloadSoft = 64ull << 20;  // PushHeader::k_MAX_PAYLOAD_SIZE_SOFT
// 28 bits of MessageWords: the PushHeader, the longest option and the padding beside it
constexpr uint64_t kPushMaxPayloadBytes = 4 * ((1ull << 28) - 1) - kPushHeaderBytes - 12 - 4;

// Result of the push pack last enqueued on c's workspace, after everything
// enqueued on its stream (w->mu held); zeros when there was none.
static int push_pack_result(Ctx& c, bmqcrc_push_pack_result* r)
{
    unsigned long long ctr[kPpkCtrWords + kCopyCtrWords];
    const int rc = slot_counters(c, c.w->ppk, ctr, r, &r->refused_index);
    if (rc || !c.w->ppk.any) {
        return rc;
    }
    r->n_events = c.w->ppk_events;
    if (r->refused_kind) {
        return 0;
    }
    if (int bad = copy_pass_clean(ctr + kPpkCtrWords, "bmqcrc_push_event_pack")) {
        return bad;
    }
    r->total_bytes = ctr[kPpkCtrTotal];
    return 0;
}

static const char* const kPushPackRefusals[11] = {
    "", "BMQCRC_PUSH_PACK_RECORD_INDEX: records[%llu] is not below n_records",
    "BMQCRC_PUSH_PACK_RECORD: the record of message %llu is not a MESSAGE record or has type 0, "
    "lease id 0, sequence number 0 or a wrong magic",
    "BMQCRC_PUSH_PACK_DATA_OFFSET: the record of message %llu points at offset 0 or outside "
    "[data_file_pos, data_file_pos+data_bytes]",
    "BMQCRC_PUSH_PACK_DATA_RECORD: the record of message %llu points at a malformed DATA record",
    "BMQCRC_PUSH_PACK_FLAGS: flags[%llu] has a bit other than e_OUT_OF_ORDER (4)",
    "BMQCRC_PUSH_PACK_EVENT_FIRST: event_first[%llu] breaks 0 = first < ... < last = n",
    "BMQCRC_PUSH_PACK_PAYLOAD_TOO_BIG: the application data of message %llu is longer than "
    "max_payload_bytes",
    "BMQCRC_PUSH_PACK_EVENT_TOO_BIG: event %llu is longer than max_event_bytes",
    "BMQCRC_PUSH_PACK_DST_TOO_SMALL: event %llu ends past dst_bytes",
    "BMQCRC_PUSH_PACK_TOO_MANY_PIECES: more than 2^32-1 16-byte pieces of application data "
    "in one call (index %llu)"};

int bmqcrc_push_event_pack(const bmqcrc_push_pack* p, bmqcrc_push_pack_result* result,
                           const bmqcrc_opts* opts)
{
    t_err.clear();
    DeviceGuard keep_device;
    // every refusal below answers before the device lookup (no GPU needed)
    bmqcrc_opts o;
    int rc;
    if ((rc = check_struct(p, "bmqcrc_push_pack", p ? p->reserved2 : 0,
                           ".reserved and reserved2 must be 0")) ||
        (rc = device_call_opts(opts, "bmqcrc_push_event_pack", &o))) {
        return rc;
    }
    if ((rc = refuse_null({{!p->journal, "journal"}, {!p->data, "data"},
                           {!p->queue_ids, "queue_ids"}}))) {
        return rc;
    }
    const uint64_t n = p->n, nrec = p->n_records;
    const uint32_t mode = p->option_mode;
    const bool wants_rda = mode == BMQCRC_PUSH_OPTION_PACKED_RDA ||
                           mode == BMQCRC_PUSH_OPTION_SUB_QUEUE_INFO;
    const bool wants_sub = mode == BMQCRC_PUSH_OPTION_SUB_QUEUE_ID ||
                           mode == BMQCRC_PUSH_OPTION_SUB_QUEUE_INFO;
    const struct {
        bool bad;
        const char* what;
    } checks[] = {
        {!p->dst && p->dst_bytes != 0, "dst == NULL is the size-only call: dst_bytes must be 0"},
        {((uintptr_t)p->journal & 3u) != 0, "journal must be 4-byte aligned"},
        {((uintptr_t)p->data & 7u) != 0, "data must be 8-byte aligned"},
        {((uintptr_t)p->dst & 3u) != 0, "dst must be 4-byte aligned"},
        {nrec > 0xFFFFFFFFull || p->journal_bytes != kJournalRecordBytes * nrec,
         "journal_bytes must be 60 n_records"},
        {n > 0xFFFFFFFFull, "n must be below 2^32"},
        {!p->records && n != nrec, "records == NULL means message m is record m: n must be n_records"},
        {!p->event_first && p->n_events != 1,
         "event_first == NULL means one event: n_events must be 1"},
        {n && (p->n_events < 1 || p->n_events > n),
         "n_events must lie in [1, n]: no event is empty"},
        {(p->data_file_pos & 7u) != 0, "data_file_pos must be a multiple of 8"},
        {mode > BMQCRC_PUSH_OPTION_SUB_QUEUE_INFO, "option_mode must be at most 3"},
        {wants_rda != (p->rda != nullptr),
         "rda is required in option modes 1 and 3 and must be NULL in modes 0 and 2"},
        {wants_sub != (p->sub_ids != nullptr),
         "sub_ids is required in option modes 2 and 3 and must be NULL in modes 0 and 1"},
        {p->max_event_bytes > kStorageMaxEventBytes,
         "max_event_bytes above 2^31-1: the EventHeader's length would overflow"},
        {p->max_payload_bytes > kPushMaxPayloadBytes,
         "max_payload_bytes above 4 (2^28-1) - 48: MessageWords would overflow"}};
    for (const auto& k : checks) {
        if (k.bad) {
            return fail(BMQCRC_EINVAL, k.what);
        }
    }
    const uint64_t entries = 8 * (p->n_events + 1);
    const NamedRange journal = {p->journal, p->journal_bytes, "[journal, journal+journal_bytes)"};
    const NamedRange data = {p->data, p->data_bytes, "[data, data+data_bytes)"};
    const NamedRange records = {p->records, p->records ? 4 * n : 0, "records"};
    const NamedRange queue_ids = {p->queue_ids, 4 * n, "queue_ids"};
    const NamedRange flags = {p->flags, p->flags ? n : 0, "flags"};
    const NamedRange rda = {p->rda, p->rda ? n : 0, "rda"};
    const NamedRange sub_ids = {p->sub_ids, p->sub_ids ? 4 * n : 0, "sub_ids"};
    const NamedRange first = {p->event_first, p->event_first ? entries : 0, "event_first"};
    const NamedRange dst = {p->dst, p->dst_bytes, "[dst, dst+dst_bytes)"};
    const NamedRange offsets = {p->event_offsets, entries, "event_offsets"};
    const NamedRange out = {p->out, 4 * n, "out"};
    const NamedRange lengths = {p->lengths, 4 * n, "lengths"};
    if ((rc = refuse_overlap({dst, offsets, out, lengths},
                             {journal, data, records, queue_ids, flags, rda, sub_ids, first})) ||
        (rc = refuse_overlap({offsets, out, lengths}, {dst})) ||
        (rc = refuse_overlap({out, lengths}, {offsets})) ||
        (rc = refuse_overlap({lengths}, {out}))) {
        return rc;
    }
    LockedCtx c;
    if ((rc = lock_on(o.device, o.stream, true, &c))) {
        return rc;
    }
    Workspace* w = c.w;
    SlotCopyScratch& s = w->ppk;
    const bool size_only = !p->dst;
    if ((rc = s.ensure(n, !size_only, kPpkCtrWords)) ||
        (rc = w->ppk_meta.ensure(4 * std::max<uint64_t>(n, 1))) ||
        (rc = s.begin(c, kPpkCtrWords, n))) {
        return rc;
    }
    w->ppk_events = n ? p->n_events : 0;
    if (n) {
        PpkArgs a;
        memset(&a, 0, sizeof(a));
        a.journal = (const uint32_t*)p->journal;
        a.n_records = nrec;
        a.data = (const uint8_t*)p->data;
        a.data_bytes = p->data_bytes;
        a.data_file_pos = p->data_file_pos;
        a.records = p->records;
        a.queue_ids = p->queue_ids;
        a.flags = p->flags;
        a.rda = p->rda;
        a.sub_ids = p->sub_ids;
        a.option_mode = mode;
        a.opt_bytes = 4 * mode;  // 0, 4, 8, 12
        a.event_first = p->event_first;
        a.n = n;
        a.n_events = p->n_events;
        a.max_event_bytes = p->max_event_bytes ? p->max_event_bytes : kStorageMaxEventSoft;
        a.max_payload_bytes = p->max_payload_bytes ? p->max_payload_bytes : kPushMaxPayloadSoft;
        a.dst = (uint8_t*)p->dst;
        a.dst_bytes = p->dst_bytes;
        a.event_offsets = p->event_offsets;
        a.out = p->out;
        a.lengths = p->lengths;
        a.ws_off = (unsigned long long*)s.off.p;
        a.ws_len = (uint32_t*)s.len.p;
        a.off = (unsigned long long*)s.dst.p;
        a.ws_exp = (uint32_t*)s.exp.p;
        a.ws_out = (const uint32_t*)s.out.p;
        a.ws_meta = (uint32_t*)w->ppk_meta.p;
        a.bsum = (unsigned long long*)s.bsum.p;
        a.ctr = (unsigned long long*)s.ctr.p;
        layout_split(n, &a.per_block, &a.nblocks);
        if (bmqcrc_launch_push_pack_layout(&a, (void*)c.s)) {
            return launch_failed("push-pack layout");
        }
        if (!size_only) {
            if ((rc = s.enqueue_slot_copy(c, a.data, a.data_bytes, a.dst, a.dst_bytes, n,
                                          kPpkCtrWords))) {
                return rc;
            }
            if (bmqcrc_launch_push_pack_frame(&a, (void*)c.s)) {
                return launch_failed("push-pack frame");
            }
        }
    }
    return sync_result_or_refusal(c, o, push_pack_result, result, kPushPackRefusals);
}

int bmqcrc_last_push_pack(int device, void* stream, bmqcrc_push_pack_result* result)
{
    return last_result(device, stream, push_pack_result, result);
}

static_assert(BMQCRC_ROLLOVER_RECORD_HEADER == BMQCRC_ROV_KIND_RECORD_HEADER &&
                  BMQCRC_ROLLOVER_KEEP_JOURNAL_OP == BMQCRC_ROV_KIND_KEEP_JOURNAL_OP &&
                  BMQCRC_ROLLOVER_SYNC_POINT == BMQCRC_ROV_KIND_SYNC_POINT &&
                  BMQCRC_ROLLOVER_DATA_OFFSET == BMQCRC_ROV_KIND_DATA_OFFSET &&
                  BMQCRC_ROLLOVER_DATA_RECORD == BMQCRC_ROV_KIND_DATA_RECORD &&
                  BMQCRC_ROLLOVER_DST_TOO_SMALL == BMQCRC_ROV_KIND_DST_TOO_SMALL &&
                  BMQCRC_ROLLOVER_DATA_FILE_FULL == BMQCRC_ROV_KIND_DATA_FILE_FULL &&
                  BMQCRC_ROLLOVER_TOO_MANY_PIECES == BMQCRC_ROV_KIND_TOO_MANY_PIECES &&
                  BMQCRC_ROLLOVER_NO_SYNC_POINT == kRovNoSyncPoint,
              "the kernels' refusal kinds are the public ones");

// Result of the rollover last enqueued on c's workspace, after everything
// enqueued on its stream (w->mu held); zeros when there was none.
static int rollover_result(Ctx& c, bmqcrc_rollover_result* r)
{
    const SlotCopyScratch& s = c.w->rov;
    unsigned long long ctr[kRovCtrWords + kCopyCtrWords];
    memset(r, 0, sizeof(*r));
    if (!s.any) {
        return 0;
    }
    HIP_TRY(hipMemcpyAsync(ctr, s.ctr.p, sizeof(ctr), hipMemcpyDeviceToHost, c.s));
    HIP_TRY(hipStreamSynchronize(c.s));
    r->n_records = s.n;
    if (ctr[kSlotCtrRefusal]) {
        refusal_of(ctr[kSlotCtrRefusal], &r->refused_kind, &r->refused_index);
        return 0;
    }
    if (int bad = copy_pass_clean(ctr + kRovCtrWords, "bmqcrc_partition_rollover")) {
        return bad;
    }
    r->n_kept = ctr[kRovCtrKept];
    r->n_messages = ctr[kSlotCtrMsgs];
    r->journal_bytes = kJournalRecordBytes * (r->n_kept + (c.w->rov_sync ? 1 : 0));
    r->data_bytes = ctr[kRovCtrData];
    r->n_bad = ctr[kSlotCtrBad];
    r->first_bad = r->n_bad ? ~ctr[kSlotCtrFirstBad] : r->n_records;
    return 0;
}

static const char* const kRolloverRefusals[9] = {
    "", "BMQCRC_ROLLOVER_RECORD_HEADER: record %llu has type 0 or above 5, lease id 0, "
        "sequence number 0, a wrong magic or a QueueOpType outside 1..4",
    "BMQCRC_ROLLOVER_KEEP_JOURNAL_OP: keep[%llu] is set on a JOURNAL_OP record, which is never "
    "rolled",
    "BMQCRC_ROLLOVER_SYNC_POINT: record %llu (sync_point) is not a JOURNAL_OP SYNCPOINT record",
    "BMQCRC_ROLLOVER_DATA_OFFSET: kept MESSAGE record %llu points at offset 0 or outside "
    "[data_file_pos, data_file_pos+data_bytes]",
    "BMQCRC_ROLLOVER_DATA_RECORD: kept MESSAGE record %llu points at a malformed DATA record",
    "BMQCRC_ROLLOVER_DST_TOO_SMALL: the DATA record of record %llu ends past dst_bytes or its "
    "journal record past journal_dst_bytes (n_records: the sync point)",
    "BMQCRC_ROLLOVER_DATA_FILE_FULL: the DATA record of record %llu ends past 8*(2^32-1) bytes "
    "of the new DATA file, where MessageOffsetDwords stops (n_records: new_data_file_pos itself)",
    "BMQCRC_ROLLOVER_TOO_MANY_PIECES: more than 2^32-1 16-byte pieces of application data "
    "in one call (index %llu)"};

int bmqcrc_partition_rollover(const bmqcrc_rollover* p, bmqcrc_rollover_result* result,
                              const bmqcrc_opts* opts)
{
    t_err.clear();
    DeviceGuard keep_device;
    // every refusal below answers before the device lookup (no GPU needed)
    bmqcrc_opts o;
    int rc;
    if ((rc = check_struct(p, "bmqcrc_rollover", p ? p->reserved2 : 0,
                           ".reserved and reserved2 must be 0")) ||
        (rc = device_call_opts(opts, "bmqcrc_partition_rollover", &o))) {
        return rc;
    }
    if ((rc = refuse_null({{!p->journal, "journal"},
                           {!p->data, "data"},
                           {!p->dst, "dst"},
                           {!p->journal_dst, "journal_dst"}}))) {
        return rc;
    }
    const uint64_t n = p->n_records;
    const bool with_sync = p->sync_point != BMQCRC_ROLLOVER_NO_SYNC_POINT;
    const struct {
        bool bad;
        const char* what;
    } checks[] = {
        {((uintptr_t)p->journal & 3u) != 0, "journal must be 4-byte aligned"},
        {((uintptr_t)p->data & 7u) != 0, "data must be 8-byte aligned"},
        {((uintptr_t)p->dst & 7u) != 0, "dst must be 8-byte aligned"},
        {((uintptr_t)p->journal_dst & 3u) != 0, "journal_dst must be 4-byte aligned"},
        {((uintptr_t)p->new_index & 3u) != 0, "new_index must be 4-byte aligned"},
        {((uintptr_t)p->out & 3u) != 0, "out must be 4-byte aligned"},
        {n > 0xFFFFFFFFull, "n_records must be below 2^32"},
        {p->journal_bytes != kJournalRecordBytes * n, "journal_bytes must be 60 n_records"},
        {(p->data_file_pos & 7u) != 0, "data_file_pos must be a multiple of 8"},
        {p->new_data_file_pos == 0 || (p->new_data_file_pos & 7u) != 0,
         "new_data_file_pos must be a multiple of 8 and not 0 (a DATA file begins with its file "
         "headers)"},
        {p->confirm_mode > BMQCRC_ROLLOVER_CONFIRMS_FOLLOW_MESSAGES,
         "confirm_mode must be at most 1"},
        {with_sync && p->sync_point >= n,
         "sync_point must be a record of the run or BMQCRC_ROLLOVER_NO_SYNC_POINT"}};
    for (const auto& k : checks) {
        if (k.bad) {
            return fail(BMQCRC_EINVAL, k.what);
        }
    }
    const NamedRange journal = {p->journal, p->journal_bytes, "[journal, journal+journal_bytes)"};
    const NamedRange data = {p->data, p->data_bytes, "[data, data+data_bytes)"};
    const NamedRange keep = {p->keep, p->keep ? n : 0, "keep"};
    const NamedRange dst = {p->dst, p->dst_bytes, "[dst, dst+dst_bytes)"};
    const NamedRange jdst = {p->journal_dst, p->journal_dst_bytes,
                             "[journal_dst, journal_dst+journal_dst_bytes)"};
    const NamedRange index = {p->new_index, 4 * n, "new_index"};
    const NamedRange out = {p->out, 4 * n, "out"};
    if ((rc = refuse_overlap({dst, jdst, index, out}, {journal, data, keep})) ||
        (rc = refuse_overlap({jdst, index, out}, {dst})) ||
        (rc = refuse_overlap({index, out}, {jdst})) || (rc = refuse_overlap({out}, {index}))) {
        return rc;
    }
    LockedCtx c;
    if ((rc = lock_on(o.device, o.stream, true, &c))) {
        return rc;
    }
    Workspace* w = c.w;
    SlotCopyScratch& s = w->rov;
    const uint64_t recs = std::max<uint64_t>(n, 1);
    const bool follow = p->confirm_mode == BMQCRC_ROLLOVER_CONFIRMS_FOLLOW_MESSAGES;
    // the hash: a power of two, at least twice the records, so that a walk ends
    uint64_t gslots = 64;
    while (gslots < 2 * recs) {
        gslots <<= 1;
    }
    if ((rc = s.ensure(n, true, kRovCtrWords, 2)) || (rc = w->rov_rec.ensure(4 * recs)) ||
        (rc = w->rov_hdr.ensure(4 * recs)) || (rc = w->rov_kind.ensure(recs)) ||
        (rc = w->rov_joff.ensure(8 * recs)) ||
        (follow && n && (rc = w->rov_gslot.ensure(4 * gslots))) ||
        (rc = s.begin(c, kRovCtrWords, n))) {
        return rc;
    }
    w->rov_sync = with_sync;
    if (n) {
        if (follow) {
            HIP_TRY(hipMemsetAsync(w->rov_gslot.p, 0, 4 * gslots, c.s));
        }
        RovArgs a;
        memset(&a, 0, sizeof(a));
        a.journal = (const uint32_t*)p->journal;
        a.n = n;
        a.data = (const uint8_t*)p->data;
        a.data_bytes = p->data_bytes;
        a.data_file_pos = p->data_file_pos;
        a.keep = p->keep;
        a.follow = follow ? 1u : 0u;
        a.sync_point = p->sync_point;
        a.timestamp = p->timestamp;
        a.new_data_file_pos = p->new_data_file_pos;
        a.dst = (uint8_t*)p->dst;
        a.dst_bytes = p->dst_bytes;
        a.journal_dst = (uint32_t*)p->journal_dst;
        a.journal_dst_bytes = p->journal_dst_bytes;
        a.new_index = p->new_index;
        a.out = p->out;
        a.ws_off = (unsigned long long*)s.off.p;
        a.ws_len = (uint32_t*)s.len.p;
        a.off = (unsigned long long*)s.dst.p;
        a.ws_exp = (uint32_t*)s.exp.p;
        a.ws_out = (const uint32_t*)s.out.p;
        a.ws_rec = (uint32_t*)w->rov_rec.p;
        a.ws_hdr = (uint32_t*)w->rov_hdr.p;
        a.kind = (uint8_t*)w->rov_kind.p;
        a.joff = (unsigned long long*)w->rov_joff.p;
        a.gslot = follow ? (uint32_t*)w->rov_gslot.p : nullptr;
        a.gslots = gslots;
        a.bsum = (unsigned long long*)s.bsum.p;
        a.ctr = (unsigned long long*)s.ctr.p;
        layout_split(n, &a.per_block, &a.nblocks);
        if (bmqcrc_launch_rollover_layout(&a, (void*)c.s)) {
            return launch_failed("rollover layout");
        }
        if ((rc = s.enqueue_slot_copy(c, a.data, a.data_bytes, a.dst, a.dst_bytes, n,
                                      kRovCtrWords))) {
            return rc;
        }
        if (bmqcrc_launch_rollover_frame(&a, (void*)c.s)) {
            return launch_failed("rollover frame");
        }
    }
    return sync_result_or_refusal(c, o, rollover_result, result, kRolloverRefusals);
}

int bmqcrc_last_rollover(int device, void* stream, bmqcrc_rollover_result* result)
{
    return last_result(device, stream, rollover_result, result);
}

static_assert(BMQCRC_CONFIRM_PACK_RECORD_HEADER == BMQCRC_CFM_KIND_RECORD_HEADER &&
                  BMQCRC_CONFIRM_PACK_DUPLICATE_MESSAGE == BMQCRC_CFM_KIND_DUPLICATE_MESSAGE &&
                  BMQCRC_CONFIRM_PACK_NULL_KEY == BMQCRC_CFM_KIND_NULL_KEY &&
                  BMQCRC_CONFIRM_PACK_REASON == BMQCRC_CFM_KIND_REASON &&
                  BMQCRC_CONFIRM_PACK_OVER_CONFIRMED == BMQCRC_CFM_KIND_OVER_CONFIRMED &&
                  BMQCRC_CONFIRM_PACK_DST_TOO_SMALL == BMQCRC_CFM_KIND_DST_TOO_SMALL,
              "the kernels' refusal kinds are the public ones");

// Result of the confirm pack last enqueued on c's workspace, after everything
// enqueued on its stream (w->mu held); zeros when there was none.
static int confirm_records_result(Ctx& c, bmqcrc_confirm_pack_result* r)
{
    memset(r, 0, sizeof(*r));
    if (!c.w->cfm_any) {
        return 0;
    }
    unsigned long long ctr[kCfmCtrWords] = {0};
    r->n_confirms = c.w->cfm_n;
    if (r->n_confirms) {
        HIP_TRY(hipMemcpyAsync(ctr, c.w->cfm_zero.p, sizeof(ctr), hipMemcpyDeviceToHost, c.s));
    }
    HIP_TRY(hipStreamSynchronize(c.s));
    if (ctr[kCfmCtrRefusal]) {
        refusal_of(ctr[kCfmCtrRefusal], &r->refused_kind, &r->refused_index);
        return 0;
    }
    r->n_written = ctr[kCfmCtrWritten];
    r->n_deletions = ctr[kCfmCtrDeletions];
    r->n_confirm_records = r->n_written - r->n_deletions;
    r->n_not_found = ctr[kCfmCtrNotFound];
    r->journal_bytes = kJournalRecordBytes * r->n_written;
    r->next_seq = c.w->cfm_first_seq + r->n_written;
    return 0;
}

static const char* const kConfirmPackRefusals[7] = {
    "", "BMQCRC_CONFIRM_PACK_RECORD_HEADER: record %llu has type 0 or above 5, lease id 0, "
        "sequence number 0, a wrong magic or a QueueOpType outside 1..4",
    "BMQCRC_CONFIRM_PACK_DUPLICATE_MESSAGE: selected MESSAGE record %llu shares its GUID and "
    "queue key with another selected MESSAGE record",
    "BMQCRC_CONFIRM_PACK_NULL_KEY: the GUID or the queue key of confirm %llu is all zero",
    "BMQCRC_CONFIRM_PACK_REASON: reasons[%llu] is neither 0 (CONFIRMED) nor 1 (REJECTED)",
    "BMQCRC_CONFIRM_PACK_OVER_CONFIRMED: the message of confirm %llu is confirmed more often "
    "in this call than it has references left",
    "BMQCRC_CONFIRM_PACK_DST_TOO_SMALL: the record of confirm %llu ends past journal_dst_bytes"};

int bmqcrc_confirm_records_pack(const bmqcrc_confirm_pack* p, bmqcrc_confirm_pack_result* result,
                                const bmqcrc_opts* opts)
{
    t_err.clear();
    DeviceGuard keep_device;
    // every refusal below answers before the device lookup (no GPU needed)
    bmqcrc_opts o;
    int rc;
    if ((rc = check_struct(p, "bmqcrc_confirm_pack", p ? p->reserved2 : 0,
                           ".reserved and reserved2 must be 0")) ||
        (rc = device_call_opts(opts, "bmqcrc_confirm_records_pack", &o))) {
        return rc;
    }
    if ((rc = refuse_null({{!p->journal, "journal"},
                           {!p->guids, "guids"},
                           {!p->queue_keys, "queue_keys"},
                           {!p->journal_dst && p->journal_dst_bytes != 0,
                            "journal_dst (with journal_dst_bytes != 0)"}}))) {
        return rc;
    }
    const uint64_t n = p->n, nrec = p->n_records;
    const struct {
        bool bad;
        const char* what;
    } checks[] = {
        {((uintptr_t)p->journal & 3u) != 0, "journal must be 4-byte aligned"},
        {((uintptr_t)p->journal_dst & 3u) != 0, "journal_dst must be 4-byte aligned"},
        {((uintptr_t)p->timestamps & 7u) != 0, "timestamps must be 8-byte aligned"},
        {((uintptr_t)p->target & 3u) != 0, "target must be 4-byte aligned"},
        {((uintptr_t)p->new_index & 3u) != 0, "new_index must be 4-byte aligned"},
        {((uintptr_t)p->left_out & 3u) != 0, "left_out must be 4-byte aligned"},
        {nrec > 0xFFFFFFFFull, "n_records must be below 2^32"},
        {n > 0xFFFFFFFFull, "n must be below 2^32"},
        {p->journal_bytes != kJournalRecordBytes * nrec, "journal_bytes must be 60 n_records"},
        {p->lease_id == 0, "lease_id must not be 0"},
        {p->first_seq == 0 || p->first_seq > kMaxSeqNum || n > kMaxSeqNum - p->first_seq,
         "first_seq must not be 0, and first_seq + n at most 2^48-1"}};
    for (const auto& k : checks) {
        if (k.bad) {
            return fail(BMQCRC_EINVAL, k.what);
        }
    }
    const NamedRange journal = {p->journal, p->journal_bytes, "[journal, journal+journal_bytes)"};
    const NamedRange select = {p->select, p->select ? nrec : 0, "select"};
    const NamedRange guids = {p->guids, 16 * n, "guids"};
    const NamedRange qkeys = {p->queue_keys, 5 * n, "queue_keys"};
    const NamedRange akeys = {p->app_keys, p->app_keys ? 5 * n : 0, "app_keys"};
    const NamedRange reasons = {p->reasons, p->reasons ? n : 0, "reasons"};
    const NamedRange stamps = {p->timestamps, p->timestamps ? 8 * n : 0, "timestamps"};
    const NamedRange jdst = {p->journal_dst, p->journal_dst_bytes,
                             "[journal_dst, journal_dst+journal_dst_bytes)"};
    const NamedRange status = {p->status, n, "status"};
    const NamedRange target = {p->target, 4 * n, "target"};
    const NamedRange index = {p->new_index, 4 * n, "new_index"};
    const NamedRange left = {p->left_out, 4 * nrec, "left_out"};
    if ((rc = refuse_overlap({jdst, status, target, index, left},
                             {journal, select, guids, qkeys, akeys, reasons, stamps})) ||
        (rc = refuse_overlap({status, target, index, left}, {jdst})) ||
        (rc = refuse_overlap({target, index, left}, {status})) ||
        (rc = refuse_overlap({index, left}, {target})) || (rc = refuse_overlap({left}, {index}))) {
        return rc;
    }
    LockedCtx c;
    if ((rc = lock_on(o.device, o.stream, true, &c))) {
        return rc;
    }
    Workspace* w = c.w;
    w->cfm_n = n;
    w->cfm_first_seq = p->first_seq;
    w->cfm_any = true;
    if (n) {
        // the hash: a power of two, at least twice the records, so that a walk ends
        const uint64_t gslots = pow2_at_least(2 * nrec);
        const uint64_t zero_bytes = 8ull * kCfmCtrWords + 4 * gslots + 13 * nrec;
        if ((rc = w->cfm_zero.ensure(zero_bytes)) ||
            (rc = w->cfm_rec.ensure(5 * std::max<uint64_t>(nrec, 1))) ||
            (rc = w->cfm_hit.ensure(4 * n)) || (rc = w->cfm_off.ensure(8 * n)) ||
            (rc = w->cfm_bsum.ensure(8ull * 2 * kPackBlocks))) {
            return rc;
        }
        HIP_TRY(hipMemsetAsync(w->cfm_zero.p, 0, zero_bytes, c.s));
        CfmArgs a;
        memset(&a, 0, sizeof(a));
        a.journal = (const uint32_t*)p->journal;
        a.n_records = nrec;
        a.select = p->select;
        a.guids = p->guids;
        a.queue_keys = p->queue_keys;
        a.app_keys = p->app_keys;
        a.reasons = p->reasons;
        a.timestamps = p->timestamps;
        a.n = n;
        a.first_seq = p->first_seq;
        a.timestamp = p->timestamp;
        a.lease_id = p->lease_id;
        a.size_only = p->journal_dst ? 0u : 1u;
        a.journal_dst = (uint32_t*)p->journal_dst;
        a.journal_dst_bytes = p->journal_dst_bytes;
        a.status = p->status;
        a.target = p->target;
        a.new_index = p->new_index;
        a.left_out = p->left_out;
        a.ctr = (unsigned long long*)w->cfm_zero.p;
        a.gslot = (uint32_t*)(a.ctr + kCfmCtrWords);
        a.gslots = gslots;
        a.had = a.gslot + gslots;
        a.cnt = a.had + nrec;
        a.last = a.cnt + nrec;
        a.dead = (uint8_t*)(a.last + nrec);
        a.ref = (uint32_t*)w->cfm_rec.p;
        a.kind = (uint8_t*)(a.ref + nrec);
        a.hit = (uint32_t*)w->cfm_hit.p;
        a.off = (unsigned long long*)w->cfm_off.p;
        a.bsum = (unsigned long long*)w->cfm_bsum.p;
        if (nrec) {
            layout_split(nrec, &a.per_block, &a.nblocks);
        }
        layout_split(n, &a.cper_block, &a.cnblocks);
        if (bmqcrc_launch_confirm_records_layout(&a, (void*)c.s)) {
            return launch_failed("confirm-records layout");
        }
        if (!a.size_only && bmqcrc_launch_confirm_records_frame(&a, (void*)c.s)) {
            return launch_failed("confirm-records frame");
        }
    }
    return sync_result_or_refusal(c, o, confirm_records_result, result, kConfirmPackRefusals);
}

int bmqcrc_last_confirm_records(int device, void* stream, bmqcrc_confirm_pack_result* result)
{
    return last_result(device, stream, confirm_records_result, result);
}

static_assert(BMQCRC_EXPIRE_PACK_RECORD_HEADER == BMQCRC_EXP_KIND_RECORD_HEADER &&
                  BMQCRC_EXPIRE_PACK_DUPLICATE_MESSAGE == BMQCRC_EXP_KIND_DUPLICATE_MESSAGE &&
                  BMQCRC_EXPIRE_PACK_QUEUE_KEY == BMQCRC_EXP_KIND_QUEUE_KEY &&
                  BMQCRC_EXPIRE_PACK_DST_TOO_SMALL == BMQCRC_EXP_KIND_DST_TOO_SMALL,
              "the kernels' refusal kinds are the public ones");

// Result of the expire pack last enqueued on c's workspace, after everything
// enqueued on its stream (w->mu held); zeros when there was none.
static int expire_records_result(Ctx& c, bmqcrc_expire_pack_result* r)
{
    memset(r, 0, sizeof(*r));
    if (!c.w->exp_any) {
        return 0;
    }
    unsigned long long ctr[kExpCtrWords] = {0};
    r->n_records = c.w->exp_n;
    if (r->n_records) {
        HIP_TRY(hipMemcpyAsync(ctr, c.w->exp_zero.p, sizeof(ctr), hipMemcpyDeviceToHost, c.s));
    }
    HIP_TRY(hipStreamSynchronize(c.s));
    if (ctr[kExpCtrRefusal]) {
        refusal_of(ctr[kExpCtrRefusal], &r->refused_kind, &r->refused_index);
        return 0;
    }
    r->n_live = ctr[kExpCtrLive];
    r->n_expired = ctr[kExpCtrExpired];
    r->n_no_queue = ctr[kExpCtrNoQueue];
    r->journal_bytes = kJournalRecordBytes * r->n_expired;
    r->next_seq = c.w->exp_first_seq + r->n_expired;
    return 0;
}

static const char* const kExpirePackRefusals[5] = {
    "", "BMQCRC_EXPIRE_PACK_RECORD_HEADER: record %llu has type 0 or above 5, lease id 0, "
        "sequence number 0, a wrong magic or a QueueOpType outside 1..4",
    "BMQCRC_EXPIRE_PACK_DUPLICATE_MESSAGE: selected MESSAGE record %llu shares its GUID and "
    "queue key with another selected MESSAGE record",
    "BMQCRC_EXPIRE_PACK_QUEUE_KEY: queue_keys entry %llu is all zero or stands in the table twice",
    "BMQCRC_EXPIRE_PACK_DST_TOO_SMALL: the DELETION record of MESSAGE record %llu ends past "
    "journal_dst_bytes"};

int bmqcrc_expire_records_pack(const bmqcrc_expire_pack* p, bmqcrc_expire_pack_result* result,
                               const bmqcrc_opts* opts)
{
    t_err.clear();
    DeviceGuard keep_device;
    // every refusal below answers before the device lookup (no GPU needed)
    bmqcrc_opts o;
    int rc;
    if ((rc = check_struct(p, "bmqcrc_expire_pack", p ? p->reserved2 : 0,
                           ".reserved and reserved2 must be 0")) ||
        (rc = device_call_opts(opts, "bmqcrc_expire_records_pack", &o))) {
        return rc;
    }
    if ((rc = refuse_null({{!p->journal, "journal"},
                           {!p->queue_keys && p->n_queues != 0, "queue_keys (with n_queues != 0)"},
                           {!p->ttl_seconds && p->n_queues != 0,
                            "ttl_seconds (with n_queues != 0)"},
                           {!p->journal_dst && p->journal_dst_bytes != 0,
                            "journal_dst (with journal_dst_bytes != 0)"}}))) {
        return rc;
    }
    const uint64_t nrec = p->n_records, nq = p->n_queues;
    const struct {
        bool bad;
        const char* what;
    } checks[] = {
        {((uintptr_t)p->journal & 3u) != 0, "journal must be 4-byte aligned"},
        {((uintptr_t)p->journal_dst & 3u) != 0, "journal_dst must be 4-byte aligned"},
        {((uintptr_t)p->ttl_seconds & 7u) != 0, "ttl_seconds must be 8-byte aligned"},
        {((uintptr_t)p->new_index & 3u) != 0, "new_index must be 4-byte aligned"},
        {((uintptr_t)p->queue_expired & 3u) != 0, "queue_expired must be 4-byte aligned"},
        {((uintptr_t)p->queue_front & 3u) != 0, "queue_front must be 4-byte aligned"},
        {nrec > 0xFFFFFFFFull, "n_records must be below 2^32"},
        {nq > 0xFFFFFFFFull, "n_queues must be below 2^32"},
        {p->journal_bytes != kJournalRecordBytes * nrec, "journal_bytes must be 60 n_records"},
        {p->lease_id == 0, "lease_id must not be 0"},
        {p->first_seq == 0 || p->first_seq > kMaxSeqNum || nrec > kMaxSeqNum - p->first_seq,
         "first_seq must not be 0, and first_seq + n_records at most 2^48-1"}};
    for (const auto& k : checks) {
        if (k.bad) {
            return fail(BMQCRC_EINVAL, k.what);
        }
    }
    const NamedRange journal = {p->journal, p->journal_bytes, "[journal, journal+journal_bytes)"};
    const NamedRange select = {p->select, p->select ? nrec : 0, "select"};
    const NamedRange qkeys = {p->queue_keys, 5 * nq, "queue_keys"};
    const NamedRange ttls = {p->ttl_seconds, 8 * nq, "ttl_seconds"};
    const NamedRange jdst = {p->journal_dst, p->journal_dst_bytes,
                             "[journal_dst, journal_dst+journal_dst_bytes)"};
    const NamedRange expired = {p->expired, nrec, "expired"};
    const NamedRange index = {p->new_index, 4 * nrec, "new_index"};
    const NamedRange selout = {p->select_out, nrec, "select_out"};
    const NamedRange qexp = {p->queue_expired, 4 * nq, "queue_expired"};
    const NamedRange qfront = {p->queue_front, 4 * nq, "queue_front"};
    if ((rc = refuse_overlap({jdst, expired, index, selout, qexp, qfront},
                             {journal, select, qkeys, ttls})) ||
        (rc = refuse_overlap({expired, index, selout, qexp, qfront}, {jdst})) ||
        (rc = refuse_overlap({index, selout, qexp, qfront}, {expired})) ||
        (rc = refuse_overlap({selout, qexp, qfront}, {index})) ||
        (rc = refuse_overlap({qexp, qfront}, {selout})) ||
        (rc = refuse_overlap({qfront}, {qexp}))) {
        return rc;
    }
    LockedCtx c;
    if ((rc = lock_on(o.device, o.stream, true, &c))) {
        return rc;
    }
    Workspace* w = c.w;
    w->exp_n = nrec;
    w->exp_first_seq = p->first_seq;
    w->exp_any = true;
    if (nrec) {
        // the hashes: a power of two, at least twice what they hold, so that a walk ends
        const uint64_t gslots = pow2_at_least(2 * nrec);
        const uint64_t qslots = nq ? pow2_at_least(2 * nq) : 0;
        const uint64_t zero_bytes = 8ull * kExpCtrWords + 4 * gslots + 4 * qslots + 4 * nq + nrec;
        if ((rc = w->exp_zero.ensure(zero_bytes)) ||
            (rc = w->exp_front.ensure(4 * std::max<uint64_t>(nq, 1))) ||
            (rc = w->exp_rec.ensure(5 * nrec)) || (rc = w->exp_off.ensure(8 * nrec)) ||
            (rc = w->exp_bsum.ensure(8ull * 2 * kPackBlocks))) {
            return rc;
        }
        HIP_TRY(hipMemsetAsync(w->exp_zero.p, 0, zero_bytes, c.s));
        if (nq) {
            HIP_TRY(hipMemsetAsync(w->exp_front.p, 0xFF, 4 * nq, c.s));  // kExpNone
        }
        ExpArgs a;
        memset(&a, 0, sizeof(a));
        a.journal = (const uint32_t*)p->journal;
        a.n_records = nrec;
        a.select = p->select;
        a.queue_keys = p->queue_keys;
        a.ttl_seconds = p->ttl_seconds;
        a.n_queues = nq;
        a.now = p->now;
        a.first_seq = p->first_seq;
        a.lease_id = p->lease_id;
        a.size_only = p->journal_dst ? 0u : 1u;
        a.journal_dst = (uint32_t*)p->journal_dst;
        a.journal_dst_bytes = p->journal_dst_bytes;
        a.expired = p->expired;
        a.new_index = p->new_index;
        a.select_out = p->select_out;
        a.queue_expired = p->queue_expired;
        a.queue_front = p->queue_front;
        a.ctr = (unsigned long long*)w->exp_zero.p;
        a.gslot = (uint32_t*)(a.ctr + kExpCtrWords);
        a.gslots = gslots;
        a.qslot = a.gslot + gslots;
        a.qslots = qslots;
        a.qcount = a.qslot + qslots;
        a.dead = (uint8_t*)(a.qcount + nq);
        a.front = (uint32_t*)w->exp_front.p;
        a.queue = (uint32_t*)w->exp_rec.p;
        a.kind = (uint8_t*)(a.queue + nrec);
        a.off = (unsigned long long*)w->exp_off.p;
        a.bsum = (unsigned long long*)w->exp_bsum.p;
        layout_split(nrec, &a.per_block, &a.nblocks);
        if (nq) {
            layout_split(nq, &a.qper_block, &a.qnblocks);
        }
        if (bmqcrc_launch_expire_records_layout(&a, (void*)c.s)) {
            return launch_failed("expire-records layout");
        }
        if (!a.size_only && bmqcrc_launch_expire_records_frame(&a, (void*)c.s)) {
            return launch_failed("expire-records frame");
        }
    }
    return sync_result_or_refusal(c, o, expire_records_result, result, kExpirePackRefusals);
}

int bmqcrc_last_expire_records(int device, void* stream, bmqcrc_expire_pack_result* result)
{
    return last_result(device, stream, expire_records_result, result);
}

static_assert(BMQCRC_PENDING_LIST_RECORD_HEADER == BMQCRC_PND_KIND_RECORD_HEADER &&
                  BMQCRC_PENDING_LIST_DUPLICATE_MESSAGE == BMQCRC_PND_KIND_DUPLICATE_MESSAGE &&
                  BMQCRC_PENDING_LIST_QUEUE_KEY == BMQCRC_PND_KIND_QUEUE_KEY &&
                  BMQCRC_PENDING_LIST_APP_FIRST == BMQCRC_PND_KIND_APP_FIRST &&
                  BMQCRC_PENDING_LIST_APP_KEY == BMQCRC_PND_KIND_APP_KEY &&
                  BMQCRC_PENDING_LIST_FROM_RECORD == BMQCRC_PND_KIND_FROM_RECORD &&
                  BMQCRC_PENDING_LIST_LIST_TOO_SMALL == BMQCRC_PND_KIND_LIST_TOO_SMALL,
              "the kernels' refusal kinds are the public ones");

// Result of the pending list last enqueued on c's workspace, after everything
// enqueued on its stream (w->mu held); zeros when there was none.
static int pending_list_result(Ctx& c, bmqcrc_pending_list_result* r)
{
    memset(r, 0, sizeof(*r));
    if (!c.w->pnd_any) {
        return 0;
    }
    unsigned long long ctr[kPndCtrWords] = {0};
    r->n_records = c.w->pnd_n;
    if (r->n_records) {
        HIP_TRY(hipMemcpyAsync(ctr, c.w->pnd_zero.p, sizeof(ctr), hipMemcpyDeviceToHost, c.s));
    }
    HIP_TRY(hipStreamSynchronize(c.s));
    if (ctr[kPndCtrRefusal]) {
        refusal_of(ctr[kPndCtrRefusal], &r->refused_kind, &r->refused_index);
        return 0;
    }
    r->n_live = ctr[kPndCtrLive];
    r->n_no_queue = ctr[kPndCtrNoQueue];
    r->n_pending = ctr[kPndCtrPending];
    r->n_listed = ctr[kPndCtrListed];
    r->n_unknown_confirms = ctr[kPndCtrUnknown];
    r->n_not_found = ctr[kPndCtrNotFound];
    return 0;
}

static const char* const kPendingListRefusals[8] = {
    "", "BMQCRC_PENDING_LIST_RECORD_HEADER: record %llu has type 0 or above 5, lease id 0, "
        "sequence number 0, a wrong magic or a QueueOpType outside 1..4",
    "BMQCRC_PENDING_LIST_DUPLICATE_MESSAGE: selected MESSAGE record %llu shares its GUID and "
    "queue key with another selected MESSAGE record",
    "BMQCRC_PENDING_LIST_QUEUE_KEY: queue_keys entry %llu is all zero or stands in the table twice",
    "BMQCRC_PENDING_LIST_APP_FIRST: app_first entry %llu does not start at 0, falls, spans more "
    "than 32 apps or does not end at n_apps",
    "BMQCRC_PENDING_LIST_APP_KEY: app %llu shares its app key with another app of its queue",
    "BMQCRC_PENDING_LIST_FROM_RECORD: from_record of app %llu is above n_records",
    "BMQCRC_PENDING_LIST_LIST_TOO_SMALL: the listed entries of app %llu end past list_cap (app "
    "n_apps: 2^32 pending entries or more)"};

int bmqcrc_pending_records_list(const bmqcrc_pending_list* p, bmqcrc_pending_list_result* result,
                                const bmqcrc_opts* opts)
{
    t_err.clear();
    DeviceGuard keep_device;
    // every refusal below answers before the device lookup (no GPU needed)
    bmqcrc_opts o;
    int rc;
    if ((rc = check_struct(p, "bmqcrc_pending_list")) ||
        (rc = device_call_opts(opts, "bmqcrc_pending_records_list", &o))) {
        return rc;
    }
    const bool size_only = !p->records;
    if ((rc = refuse_null({{!p->journal, "journal"},
                           {!p->app_first, "app_first"},
                           {!p->queue_keys && p->n_queues != 0, "queue_keys (with n_queues != 0)"},
                           {!p->app_keys && p->n_apps != 0, "app_keys (with n_apps != 0)"},
                           {!p->queue_ids && p->n_apps != 0, "queue_ids (with n_apps != 0)"},
                           {size_only && p->list_cap != 0, "records (with list_cap != 0)"},
                           {!size_only && !p->out_queue_ids, "out_queue_ids (with records)"},
                           {!size_only && !p->list_first, "list_first (with records)"},
                           {p->out_sub_ids && !p->sub_ids, "sub_ids (with out_sub_ids)"}}))) {
        return rc;
    }
    const uint64_t nrec = p->n_records, nq = p->n_queues, na = p->n_apps, cap = p->list_cap;
    const struct {
        bool bad;
        const char* what;
    } checks[] = {
        {((uintptr_t)p->journal & 3u) != 0, "journal must be 4-byte aligned"},
        {((uintptr_t)p->app_first & 7u) != 0, "app_first must be 8-byte aligned"},
        {((uintptr_t)p->queue_ids & 3u) != 0, "queue_ids must be 4-byte aligned"},
        {((uintptr_t)p->sub_ids & 3u) != 0, "sub_ids must be 4-byte aligned"},
        {((uintptr_t)p->from_record & 3u) != 0, "from_record must be 4-byte aligned"},
        {((uintptr_t)p->limit & 3u) != 0, "limit must be 4-byte aligned"},
        {((uintptr_t)p->records & 3u) != 0, "records must be 4-byte aligned"},
        {((uintptr_t)p->out_queue_ids & 3u) != 0, "out_queue_ids must be 4-byte aligned"},
        {((uintptr_t)p->out_sub_ids & 3u) != 0, "out_sub_ids must be 4-byte aligned"},
        {((uintptr_t)p->list_first & 7u) != 0, "list_first must be 8-byte aligned"},
        {((uintptr_t)p->app_pending & 3u) != 0, "app_pending must be 4-byte aligned"},
        {((uintptr_t)p->app_next & 3u) != 0, "app_next must be 4-byte aligned"},
        {((uintptr_t)p->pending_mask & 3u) != 0, "pending_mask must be 4-byte aligned"},
        {nrec > 0xFFFFFFFFull, "n_records must be below 2^32"},
        {nq > 0xFFFFFFFFull, "n_queues must be below 2^32"},
        {na > 0xFFFFFFFFull, "n_apps must be below 2^32"},
        {p->journal_bytes != kJournalRecordBytes * nrec, "journal_bytes must be 60 n_records"},
        {cap > (1ull << 60), "list_cap must be at most 2^60"}};
    for (const auto& k : checks) {
        if (k.bad) {
            return fail(BMQCRC_EINVAL, k.what);
        }
    }
    const NamedRange journal = {p->journal, p->journal_bytes, "[journal, journal+journal_bytes)"};
    const NamedRange select = {p->select, p->select ? nrec : 0, "select"};
    const NamedRange qkeys = {p->queue_keys, 5 * nq, "queue_keys"};
    const NamedRange afirst = {p->app_first, 8 * (nq + 1), "app_first"};
    const NamedRange akeys = {p->app_keys, 5 * na, "app_keys"};
    const NamedRange qids = {p->queue_ids, 4 * na, "queue_ids"};
    const NamedRange sids = {p->sub_ids, p->sub_ids ? 4 * na : 0, "sub_ids"};
    const NamedRange from = {p->from_record, p->from_record ? 4 * na : 0, "from_record"};
    const NamedRange limit = {p->limit, p->limit ? 4 * na : 0, "limit"};
    const NamedRange recs = {p->records, 4 * cap, "records"};
    const NamedRange oqids = {p->out_queue_ids, 4 * cap, "out_queue_ids"};
    const NamedRange osids = {p->out_sub_ids, 4 * cap, "out_sub_ids"};
    const NamedRange lfirst = {p->list_first, 8 * (na + 1), "list_first"};
    const NamedRange apend = {p->app_pending, 4 * na, "app_pending"};
    const NamedRange anext = {p->app_next, 4 * na, "app_next"};
    const NamedRange pmask = {p->pending_mask, 4 * nrec, "pending_mask"};
    if ((rc = refuse_overlap({recs, oqids, osids, lfirst, apend, anext, pmask},
                             {journal, select, qkeys, afirst, akeys, qids, sids, from, limit})) ||
        (rc = refuse_overlap({oqids, osids, lfirst, apend, anext, pmask}, {recs})) ||
        (rc = refuse_overlap({osids, lfirst, apend, anext, pmask}, {oqids})) ||
        (rc = refuse_overlap({lfirst, apend, anext, pmask}, {osids})) ||
        (rc = refuse_overlap({apend, anext, pmask}, {lfirst})) ||
        (rc = refuse_overlap({anext, pmask}, {apend})) ||
        (rc = refuse_overlap({pmask}, {anext}))) {
        return rc;
    }
    LockedCtx c;
    if ((rc = lock_on(o.device, o.stream, true, &c))) {
        return rc;
    }
    Workspace* w = c.w;
    // (a call that fails below leaves no record: its counters would be a half-run's)
    w->pnd_any = false;
    if (nrec) {
        // the hashes: a power of two, at least twice what they hold, so that a walk ends
        const uint64_t gslots = pow2_at_least(2 * nrec);
        const uint64_t qslots = nq ? pow2_at_least(2 * nq) : 0;
        const uint64_t zero_bytes = 8ull * kPndCtrWords + 4 * gslots + 4 * qslots + 5 * nrec;
        if ((rc = w->pnd_zero.ensure(zero_bytes)) || (rc = w->pnd_rec.ensure(9 * nrec)) ||
            (rc = w->pnd_off.ensure(8 * nrec)) ||
            (rc = w->pnd_bsum.ensure(8ull * 4 * kPackBlocks)) ||
            (rc = w->pnd_hist.ensure(4ull * kPndDigits * (kPackBlocks + 1))) ||
            (rc = w->pnd_app.ensure(16 * std::max<uint64_t>(na, 1)))) {
            return rc;
        }
        HIP_TRY(hipMemsetAsync(w->pnd_zero.p, 0, zero_bytes, c.s));
        PndArgs a;
        memset(&a, 0, sizeof(a));
        a.journal = (const uint32_t*)p->journal;
        a.n_records = nrec;
        a.select = p->select;
        a.queue_keys = p->queue_keys;
        a.app_first = p->app_first;
        a.n_queues = nq;
        a.app_keys = p->app_keys;
        a.queue_ids = p->queue_ids;
        a.sub_ids = p->sub_ids;
        a.from_record = p->from_record;
        a.limit = p->limit;
        a.n_apps = na;
        a.size_only = size_only ? 1u : 0u;
        for (uint64_t v = na ? na - 1 : 0; v; v >>= 8) {
            ++a.passes;
        }
        a.records = p->records;
        a.out_queue_ids = p->out_queue_ids;
        a.out_sub_ids = p->out_sub_ids;
        a.list_cap = cap;
        a.list_first = p->list_first;
        a.app_pending = p->app_pending;
        a.app_next = p->app_next;
        a.pending_mask = p->pending_mask;
        a.ctr = (unsigned long long*)w->pnd_zero.p;
        a.gslot = (uint32_t*)(a.ctr + kPndCtrWords);
        a.gslots = gslots;
        a.qslot = a.gslot + gslots;
        a.qslots = qslots;
        a.confirmed = a.qslot + qslots;
        a.dead = (uint8_t*)(a.confirmed + nrec);
        a.queue = (uint32_t*)w->pnd_rec.p;
        a.mask = a.queue + nrec;
        a.kind = (uint8_t*)(a.mask + nrec);
        a.off = (unsigned long long*)w->pnd_off.p;
        a.bsum = (unsigned long long*)w->pnd_bsum.p;
        a.absum = a.bsum + 2 * kPackBlocks;
        layout_split(nrec, &a.per_block, &a.nblocks);
        const uint64_t table = std::max(nq + 1, na);
        a.cblocks = std::max<uint32_t>(
            a.nblocks, (uint32_t)std::min<uint64_t>((table + kPackThreads - 1) / kPackThreads,
                                                    kPackBlocks));
        if (bmqcrc_launch_pending_list_masks(&a, (void*)c.s)) {
            return launch_failed("pending-list masks");
        }
        // the one word the sort's buffers are sized from (and the refusals so far:
        // nothing more is launched over a refused table)
        unsigned long long ctr[kPndCtrWords] = {0};
        HIP_TRY(hipMemcpyAsync(ctr, a.ctr, sizeof(ctr), hipMemcpyDeviceToHost, c.s));
        HIP_TRY(hipStreamSynchronize(c.s));
        if (!ctr[kPndCtrRefusal]) {
            const uint64_t np = ctr[kPndCtrPending];  // below 2^32, or it was refused
            if ((rc = w->pnd_pairs.ensure(16 * std::max<uint64_t>(np, 1)))) {
                return rc;
            }
            a.n_pairs = np;
            a.key[0] = (uint32_t*)w->pnd_pairs.p;
            a.key[1] = a.key[0] + np;
            a.val[0] = a.key[1] + np;
            a.val[1] = a.val[0] + np;
            a.hist = (uint32_t*)w->pnd_hist.p;
            a.rowsum = a.hist + (uint64_t)kPndDigits * kPackBlocks;
            if (np) {
                layout_split(np, &a.sper_block, &a.snblocks);
            }
            a.aoff = (unsigned long long*)w->pnd_app.p;
            a.afirst = (uint32_t*)(a.aoff + na);
            a.acount = a.afirst + na;
            if (na) {
                layout_split(na, &a.aper_block, &a.anblocks);
            }
            if (bmqcrc_launch_pending_list_lists(&a, (void*)c.s)) {
                return launch_failed("pending-list lists");
            }
        }
    }
    w->pnd_n = nrec;
    w->pnd_any = true;
    return sync_result_or_refusal(c, o, pending_list_result, result, kPendingListRefusals);
}

int bmqcrc_last_pending_records(int device, void* stream, bmqcrc_pending_list_result* result)
{
    return last_result(device, stream, pending_list_result, result);
}

int bmqcrc_last_launch(int device, void* stream, uint32_t* kernels, uint32_t* spec,
                       uint32_t* seg_bytes)
{
    t_err.clear();
    DeviceGuard keep_device;
    LockedCtx c;
    int rc;
    if ((rc = lock_on(device, stream, false, &c))) {
        return rc;
    }
    Workspace* w = c.w;
    if (kernels) {
        *kernels = w->last_kernels;
    }
    if (spec) {
        *spec = w->last_spec;
    }
    if (seg_bytes) {
        *seg_bytes = w->last_seg;
    }
    return 0;
}

int bmqcrc_last_plan(int device, void* stream, uint32_t* map)
{
    t_err.clear();
    DeviceGuard keep_device;
    LockedCtx c;
    int rc;
    if ((rc = lock_on(device, stream, false, &c))) {
        return rc;
    }
    Workspace* w = c.w;
    if (map) {
        *map = w->last_map;
    }
    return 0;
}

int bmqcrc_last_offsets(int device, void* stream, uint32_t* bits, uint32_t* shift)
{
    t_err.clear();
    DeviceGuard keep_device;
    LockedCtx c;
    int rc;
    if ((rc = lock_on(device, stream, false, &c))) {
        return rc;
    }
    Workspace* w = c.w;
    if (bits) {
        *bits = w->last_off_bits;
    }
    if (shift) {
        *shift = w->last_off_shift;
    }
    return 0;
}

int bmqcrc_forget_shape(int device, void* stream)
{
    t_err.clear();
    DeviceGuard keep_device;
    LockedCtx c;
    int rc;
    if ((rc = lock_on(device, stream, false, &c))) {
        return rc;
    }
    Workspace* w = c.w;
    if (w->hint_host) {
        __atomic_store_n(w->hint_host, kHintUnknown, __ATOMIC_RELAXED);
    }
    return 0;
}

int bmqcrc_plan_wait(int device, void* stream, uint64_t wait_us, uint64_t* voided)
{
    t_err.clear();
    DeviceGuard keep_device;
    LockedCtx c;
    int rc;
    if ((rc = lock_on(device, stream, true, &c))) {
        return rc;
    }
    Workspace* w = c.w;
    w->map_wait_ticks = wait_us > (UINT64_MAX / 100) ? UINT64_MAX : wait_us * 100;
    if (voided) {
        // k_plan_map counts its launches that gave up their map (plan_sync[3])
        unsigned long long n = 0;
        if (w->plan_sync.p) {  // after the work already enqueued on this stream
            HIP_TRY(hipMemcpyAsync(&n, (const uint8_t*)w->plan_sync.p + 24, 8,
                                   hipMemcpyDeviceToHost, (hipStream_t)stream));
            HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        }
        *voided = n;
    }
    return 0;
}

int bmqcrc_host_register(void* host, uint64_t bytes, int device, void** dev_ptr)
{
    t_err.clear();
    DeviceGuard keep_device;
    if (!host || !bytes || !dev_ptr) {
        return fail(BMQCRC_EINVAL, "host, bytes and dev_ptr are required");
    }
    int dev, rc;
    DeviceState* st = nullptr;
    if ((rc = resolve_device(device, &dev)) || (rc = device_state(dev, &st))) {
        return rc;
    }
    HIP_TRY(hipSetDevice(dev));
    HIP_TRY(hipHostRegister(host, bytes, hipHostRegisterMapped | hipHostRegisterPortable));
    void* d = nullptr;
    const hipError_t e = hipHostGetDevicePointer(&d, host, 0);
    if (e != hipSuccess) {
        (void)hipHostUnregister(host);
        return fail(BMQCRC_EIO, std::string("hipHostGetDevicePointer: ") + hipGetErrorString(e));
    }
    *dev_ptr = d;
    return 0;
}

int bmqcrc_host_unregister(void* host)
{
    t_err.clear();
    if (!host) {
        return fail(BMQCRC_EINVAL, "null host pointer");
    }
    if (device_count_raw() <= 0) {
        return fail(BMQCRC_ENODEV, "no HIP device available");
    }
    HIP_TRY(hipHostUnregister(host));
    return 0;
}

int bmqcrc_device_count(void)
{
    return device_count_raw();
}

const char* bmqcrc_last_error(void)
{
    return t_err.c_str();
}

// Host fallbacks of the C++ spellings (bmqcrc.h).  A fault (EIO) is never
// silent: the first one in the process is printed with its HIP error.
static std::atomic<uint64_t> g_fallbacks{0};
static std::atomic<int32_t> g_fallback_rc{0};
static std::atomic<bool> g_eio_reported{false};

void bmqcrc_note_host_fallback(int32_t rc)
{
    g_fallbacks.fetch_add(1, std::memory_order_relaxed);
    g_fallback_rc.store(rc, std::memory_order_relaxed);
    if (rc == BMQCRC_EIO && !g_eio_reported.exchange(true)) {
        fprintf(stderr,
                "libbmqcrc: GPU batch failed with BMQCRC_EIO (%s); finishing on the host "
                "(bmqcrc_host_fallbacks counts every such call)\n",
                t_err.c_str());
    }
}

uint64_t bmqcrc_host_fallbacks(int32_t* last_rc)
{
    if (last_rc) {
        *last_rc = g_fallback_rc.load(std::memory_order_relaxed);
    }
    return g_fallbacks.load(std::memory_order_relaxed);
}

uint32_t bmqcrc_version(void)
{
    return (2u << 16) | 21u;
}

}  // extern "C"
