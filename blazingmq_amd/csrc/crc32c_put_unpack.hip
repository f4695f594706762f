// crc32c_put_unpack.hip -- MI355X (gfx950) walk of device-resident PUT events
// (bmqcrc_put_event_unpack, ABI 2.12).
//
// The inverse of crc32c_put_pack.hip and the device-side form of
// walk_put_event (bmqcrc_protocol.cpp): given PUT events in HBM it finds every
// message and yields the per-message arrays the packers take.  The chain of
// PutHeaders is serial inside an event, so the parallelism is across events:
// one wave walks one event, the grid strides over the events.  Four kernels on
// one stream, around the fold of crc32c_kernels.hip:
//
//   1. k_unpack_walk<false>: every event validated with the host walk's checks
//      in the host walk's order, its messages counted into first[e]; the first
//      violation of an event raises the call's refusal word
//      (crc32c_pack_layout.h) and leaves its offset in bad_off[e].
//   2. k_unpack_scan: first[] becomes the exclusive prefix of the counts
//      (tile_scan of crc32c_pack_layout.h), and the lowest event whose last
//      message lies past msg_cap is refused.
//   3. k_unpack_walk<true>: the same walk again, now placing: after every 64
//      messages the 64 lanes fetch their own message's queue id, GUID and CRC
//      and store coalesced.  Offsets and lengths go to the WORKSPACE, which
//      the fold reads; the slots no message took -- all of them when anything
//      was refused -- become empty messages (empty_slots of
//      crc32c_unpack_slots.h).
//   (the fold: bmqcrc_launch_batch over the msg_cap slots, when out != NULL)
//   4. k_unpack_publish: unless refused, the workspace's offsets, lengths,
//      header CRCs and computed CRCs to the caller's arrays, the mismatches
//      counted.
//
// The walk loads no byte it has not shown to lie inside its event: the
// event's bounds are checked against events_bytes first, pos + 8 <= end before
// a header, pos + msg <= end before the padding byte.  The header words and
// the padding byte are read through a window of the event in LDS (struct
// Window: two 1 KiB chunks per wave and a third prefetched into registers), so
// several small messages cost one trip to memory and that trip overlaps the
// walk of the chunk before.  A step advances by at least 36 bytes (headerWords
// >= 8 and header + options < messageWords), which bounds the loop by the
// event's size.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmqcrc_internal.h"
#include "crc32c_pack_layout.h"
#include "crc32c_unpack_slots.h"

namespace bmqcrc {
namespace {

// byte-aligned dword: a GUID array need not be 4-byte aligned
typedef uint32_t u32u __attribute__((aligned(1)));

constexpr uint32_t kWindowDwords = kUnpackWindowBytes / 4;
static_assert(kWindowDwords == 4 * kUnpackWalkThreads, "Window::fetch: four dwords per lane");

// A refusal of event e: the call's word, and the byte the host walk would name.
__device__ __forceinline__ void refuse_event(const UnpackArgs& a, uint32_t kind, uint64_t e,
                                             uint64_t offset)
{
    if (threadIdx.x == 0) {
        a.bad_off[e] = offset;
        refuse(a, kind, e);
    }
}

// A wave's view of its event: a ring of two 1 KiB chunks in LDS covering
// bytes [cb, cb + 2 KiB) of the events buffer, and the chunk behind them on
// its way into four registers per lane.  The walk moves forward only.  A
// position at most one chunk ahead takes the prefetched chunk into the ring
// (advance: its loads were issued a chunk's walk ago) and issues the next
// prefetch; one further ahead -- a long message -- loads all three afresh
// (reload: one trip to memory).  Only whole dwords inside [ev0, end), the
// event, are ever loaded: a lane whose dword lies outside reads the event's
// first dword instead, so that the four loads are unconditional and in flight
// together and nothing waits for a prefetch before its chunk is needed; that
// dword is never used, since the walk checks a position against `end` before
// it looks it up.
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
    // makes [p, p + bytes) readable, p >= cb, bytes <= 8
    __device__ __forceinline__ void need(uint64_t p, uint32_t bytes)
    {
        if (p + bytes > cb + 2 * kUnpackWindowBytes) {
            if (p + bytes <= cb + 3 * kUnpackWindowBytes) {
                advance();  // (p > cb + 2 KiB - 8: inside the ring's new first chunk)
            } else {
                reload(p);
            }
        }
    }
    // big-endian dword at byte position p of the buffer, made readable before
    __device__ __forceinline__ uint32_t be32(uint64_t p) const
    {
        const uint32_t i = ((uint32_t)((p - cb) >> 2) + slot * kWindowDwords) & (2 * kWindowDwords - 1);
        return __builtin_bswap32(__builtin_amdgcn_readfirstlane(ring[i]));
    }
};

// One event, walked by the block's one wave; every value that steers the walk
// is the same in all lanes.  kPlace false: validate and count into first[e].
// kPlace true (the call refused nothing, first[] is the prefix): place the
// event's first[e + 1] - first[e] messages from slot first[e] on.
template <bool kPlace>
__device__ __forceinline__ void walk_event(const UnpackArgs& a, uint64_t e, uint32_t* win)
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
            refuse_event(a, BMQCRC_UNPACK_KIND_EVENT_OFFSETS, e, beg);
        }
        return;
    }
    const uint64_t size = end - beg;
    if (size < 8) {
        if (!kPlace) {
            refuse_event(a, BMQCRC_UNPACK_KIND_EVENT_HEADER, e, beg);
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
        uint64_t bad = ~0ull;
        if ((w.be32(beg) & 0x7FFFFFFFu) != size) {
            bad = 0;  // EventHeader length differs from the event size
        } else if (((h1 >> 24) & 0x3Fu) != 2u) {
            bad = 4;  // not a PUT event
        } else if (hw < 8 || hw > size) {
            bad = 5;  // EventHeader headerWords out of range
        }
        if (bad != ~0ull) {
            if (!kPlace) {
                refuse_event(a, BMQCRC_UNPACK_KIND_EVENT_HEADER, e, beg + bad);
            }
            return;
        }
        beg += hw;
    }
    uint64_t pos = beg, k = 0;
    // the lane's own message of the current 64: header, data, length, flags
    uint64_t my_hdr = 0, my_app = 0;
    uint32_t my_len = 0, my_flags = 0;
    // lanes [0, cnt) hold messages slot + k0 ...: fetch the fields and store
    auto flush = [&](uint64_t k0, uint32_t cnt) {
        if (lane < cnt) {
            const uint64_t i = slot + k0 + lane;
            const uint32_t* h = (const uint32_t*)(a.events + my_hdr);
            a.ws_off[i] = my_app;
            a.ws_len[i] = my_len;
            a.ws_exp[i] = __builtin_bswap32(h[7]);
            if (a.queue_ids) {
                a.queue_ids[i] = (int32_t)__builtin_bswap32(h[2]);
            }
            if (a.guids) {
                u32u* g = (u32u*)(a.guids + 16 * i);
                g[0] = h[3];
                g[1] = h[4];
                g[2] = h[5];
                g[3] = h[6];
            }
            if (a.flags) {
                a.flags[i] = (uint8_t)my_flags;
            }
        }
    };
    while (pos < end && k < limit) {
        uint32_t kind = 0;
        uint64_t at = pos;
        uint64_t msg = 0, skip = 0;
        uint32_t pad = 0, w0 = 0;
        if (pos + 8 > end) {
            kind = BMQCRC_UNPACK_KIND_PUT_HEADER;  // truncated PutHeader
        } else {
            w.need(pos, 8);
            w0 = w.be32(pos);
            const uint32_t w1 = w.be32(pos + 4);
            msg = (uint64_t)(w0 & 0x0FFFFFFFu) * 4;
            const uint64_t hdr = (uint64_t)(w1 & 0x1Fu) * 4;
            skip = hdr + (uint64_t)(w1 >> 8) * 4;  // header + options
            if (hdr < 32 || msg == 0 || pos + msg > end || skip >= msg) {
                kind = BMQCRC_UNPACK_KIND_PUT_HEADER;
            } else {
                const uint64_t last = pos + msg - 4;  // the dword of the padding byte
                w.need(last, 4);  // (a reload starts there: the next header is its neighbour)
                pad = w.be32(last) & 0xFFu;
                if (pad < 1 || pad > 4 || skip + pad > msg) {
                    kind = BMQCRC_UNPACK_KIND_PADDING;
                    at = pos + msg - 1;
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
            my_hdr = pos;
            my_app = pos + skip;
            my_len = (uint32_t)(msg - skip - pad);
            my_flags = w0 >> 28;
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
__global__ __launch_bounds__(kUnpackWalkThreads) void k_unpack_walk(UnpackArgs a)
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

// Step 2: one block.  first[e] = messages of the events before e, first[n_events] = of all.
__global__ __launch_bounds__(kUnpackThreads) void k_unpack_scan(UnpackArgs a)
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
                refuse(a, BMQCRC_UNPACK_KIND_TOO_MANY_MESSAGES, e);
            }
        }
        carry += tot;
    }
    if (tid == 0) {
        a.first[a.n_events] = carry;
    }
}

// Step 4, after the fold.
__global__ __launch_bounds__(kUnpackPublishThreads) void k_unpack_publish(UnpackArgs a)
{
    const uint64_t t0 = (uint64_t)blockIdx.x * kUnpackPublishThreads + threadIdx.x;
    const unsigned long long word = a.ctr[kSlotCtrRefusal];
    if (word != 0) {
        if (t0 == 0) {
            const unsigned long long key = ~word;
            const uint64_t e = key & ((1ull << 56) - 1);
            // (TOO_MANY_MESSAGES names no byte: the event's start)
            a.ctr[kUnpCtrOffset] =
                (key >> 56) != BMQCRC_UNPACK_KIND_TOO_MANY_MESSAGES ? a.bad_off[e]
                : a.event_offsets                                   ? a.event_offsets[e]
                                                                    : 0ull;
        }
        return;
    }
    const uint64_t stride = (uint64_t)gridDim.x * kUnpackPublishThreads;
    const uint64_t n = a.first[a.n_events];
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
    if (a.event_first) {
        for (uint64_t e = t0; e <= a.n_events; e += stride) {
            a.event_first[e] = a.first[e];
        }
    }
    if (t0 == 0) {
        a.ctr[kSlotCtrMsgs] = n;
    }
    if (bad) {
        atomicAdd(&a.ctr[kSlotCtrBad], bad);
        atomicMax(&a.ctr[kSlotCtrFirstBad], lowest);
    }
}

}  // namespace
}  // namespace bmqcrc

using namespace bmqcrc;

extern "C" int bmqcrc_launch_unpack_walk(const UnpackArgs* a, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    const uint64_t walk = a->n_events < kUnpackWalkBlocks ? a->n_events : kUnpackWalkBlocks;
    // 16 slots per thread at least for the blocks that only empty slots
    const uint64_t fill = a->msg_cap / (16 * kUnpackWalkThreads);
    const uint64_t place = fill < walk ? walk : fill > kUnpackWalkBlocks ? kUnpackWalkBlocks : fill;
    hipLaunchKernelGGL(k_unpack_walk<false>, dim3((uint32_t)walk), dim3(kUnpackWalkThreads), 0, s,
                       *a);
    hipLaunchKernelGGL(k_unpack_scan, dim3(1), dim3(kUnpackThreads), 0, s, *a);
    hipLaunchKernelGGL(k_unpack_walk<true>, dim3((uint32_t)place), dim3(kUnpackWalkThreads), 0, s,
                       *a);
    return hipGetLastError() != hipSuccess;
}

extern "C" int bmqcrc_launch_unpack_publish(const UnpackArgs* a, void* stream)
{
    const uint64_t work = a->msg_cap > a->n_events + 1 ? a->msg_cap : a->n_events + 1;
    const uint64_t want = (work + kUnpackPublishThreads - 1) / kUnpackPublishThreads;
    const uint32_t blocks = (uint32_t)(want > kUnpackPublishBlocks ? kUnpackPublishBlocks : want);
    hipLaunchKernelGGL(k_unpack_publish, dim3(blocks), dim3(kUnpackPublishThreads), 0,
                       (hipStream_t)stream, *a);
    return hipGetLastError() != hipSuccess;
}
