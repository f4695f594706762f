// k_plan_map_body.inc -- the body of k_plan_map (crc32c_kernels.hip), included
// once per offset form with `constexpr bool O32` in scope.
//
// Why not a template like the other kernels: as an instantiation (any
// linkage a template gets) the 64-bit kernel came out of the compiler with
// its second half scheduled and register-allocated differently from the
// same body in a plain function -- four more instructions, no change in the
// source it compiles.  This file's kernels are sensitive to exactly that
// (DESIGN.md appendix A), so the 64-bit k_plan_map stays a plain kernel and
// the 32-bit one shares its text this way.
// Only that goal justifies a body without a scope of its own: with another
// compiler version, try `template <bool O32>` on k_plan_map again
// (tools/asm_diff_kernels.py tells) and fold this file back in.
    using Quad = QuadT<O32>;
    PLAN_STAMP(0)
    __shared__ uint32_t wsum[40];
    __shared__ uint32_t sh[4];
    __shared__ uint32_t hist[kBuckets];
    __shared__ uint32_t run[kBuckets];
    __shared__ uint32_t part[2][2][kBuckets];  // per wave: class totals / prefix, block words
    __shared__ unsigned long long segs64;
    __shared__ uint32_t go;
    __shared__ PlanTail tail;
    __shared__ uint32_t sruns[kPlanBlock / 64][64 * kPlanV];  // per wave: short-run ends
    __shared__ uint32_t slong[kPlanBlock / 64][2][64 * kPlanV];  // per wave: long runs' starts, lengths
    __shared__ uint32_t smark[kPlanBlock / 64][64];             // per wave: item-run starts in a chunk
    const uint32_t nb = a.nblocks, ep = launch_epoch(a), bid = blockIdx.x;
    load_tail<O32>(a, min((uint64_t)bid * a.per_msg + a.per_msg, a.n), true, &tail);
    // epoch-tagged words the blocks exchange (plan_sync after the flags),
    // laid out for coalesced reads: [c * kPlanMaxBlocks + b] histograms,
    // [kTagWords + i * kPlanMaxBlocks + b] block words
    unsigned long long* const tags = a.plan_sync + kSyncFlags + kPlanMaxBlocks;
    constexpr uint32_t kTagWords = kPlanMaxBlocks * kBuckets;
    // mark this launch's map given up (one thread): k_fold folds every
    // message whole; the first block to give up counts the launch
    auto give_up = [&]() {
        if (__hip_atomic_exchange(&a.plan_sync[2], (unsigned long long)ep, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT) != ep) {
            __hip_atomic_fetch_add(&a.plan_sync[3], 1ull, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    unsigned long long* const sync = a.plan_sync;
    if (threadIdx.x == 0) {
        sh[1] = 0;            // messages with != 1 segment
        sh[2] = 0xffffffffu;  // min segments per message
        sh[3] = 0;            // max segments per message
        segs64 = 0;
    }
    if (threadIdx.x < kBuckets) {
        hist[threadIdx.x] = 0;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    constexpr uint64_t kTile = (uint64_t)kPlanBlock * kPlanV;
    const uint64_t lo = (uint64_t)bid * a.per_msg;
    const uint64_t hi = min(lo + a.per_msg, a.n);
    const uint32_t ntiles = hi > lo ? (uint32_t)((hi - lo + kTile - 1) / kTile) : 0u;
    const uint32_t seg = a.seg_bytes;
    const uint32_t seg_shift = (seg & (seg - 1u)) == 0 ? (uint32_t)__builtin_ctz(seg) : 0u;
    const uint32_t c_full = size_class(seg >> 7);
    const bool one_tile = ntiles <= 1u;
    auto segments = [&](uint32_t len) {
        return len ? (seg_shift ? ((len - 1u) >> seg_shift) : (len - 1u) / seg) + 1u : 0u;
    };

    // Thread t of tile [base, base + kTile) owns messages base + 4t .. base + 4t + 3.
    auto load = [&](uint32_t t) {
        return load_quad<O32>(a, lo + (uint64_t)t * kTile + (uint64_t)threadIdx.x * kPlanV, hi);
    };
    // seg_first (the block-local prefix from run0) and out[] for one tile
    auto tile_words = [&](uint64_t base, const uint32_t (&L)[kPlanV], uint32_t run0,
                          bool write_sf) {
        uint32_t ns[kPlanV];
#pragma unroll
        for (uint32_t v = 0; v < kPlanV; ++v) {
            ns[v] = segments(L[v]);
        }
        store_quad(a, base + (uint64_t)threadIdx.x * kPlanV, hi, L, ns, run0, write_sf);
    };
    // Phase 1.  The first kMapRegTiles tiles are loaded at once (all in
    // flight together) and keep their lengths, classes and prefix in
    // registers, deferring their writes; later tiles load one ahead and
    // write as k_plan does.
    uint32_t Lr[kMapRegTiles][kPlanV], Cr[kMapRegTiles], R0[kMapRegTiles];
    uint32_t full = 0, carry = 0, mn = 0xffffffffu, mx = 0, non1 = 0;
    uint64_t mine64 = 0;
    Quad rq[kMapRegTiles];
#pragma unroll
    for (uint32_t t = 0; t < kMapRegTiles; ++t) {
        rq[t] = load(t);  // unguarded: a tile past the range loads the zero line
    }
    auto count_tile = [&](uint32_t t, const Quad& q, uint32_t (&L)[kPlanV], uint32_t& cls,
                          uint32_t& run0, bool defer) {
        const uint64_t base = lo + (uint64_t)t * kTile;
        uint64_t O[kPlanV];
        unpack_quad<O32>(a, q, base + (uint64_t)threadIdx.x * kPlanV, hi, &tail, L, O);
        if (t == 0) {
            PLAN_STAMP_LANDED(1)
        }
        cls = 0;
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t v = 0; v < kPlanV; ++v) {
            uint32_t c;
            const uint32_t ns = msg_segments(a, O[v], L[v], seg_shift, &c);
            full += ns ? ns - 1u : 0u;
            if (c < (uint32_t)kBuckets) {
                atomicAdd(&hist[c], 1u);
            }
            cls |= c << (8u * v);  // kBuckets (no segment) fits a byte
            const uint64_t i = base + (uint64_t)threadIdx.x * kPlanV + v;
            if (i < hi) {
                mn = min(mn, ns);
                mx = max(mx, ns);
                non1 += ns != 1u ? 1u : 0u;
            }
            sum += ns;
        }
        mine64 += sum;
        uint32_t excl;
        const uint32_t tot = block_scan(sum, &excl, wsum);
        run0 = carry + excl;
        carry += tot;
        if (!defer) {
            tile_words(base, L, run0, true);
        }
        if (t == 0) {
            PLAN_STAMP(2)
        }
    };
#pragma unroll
    for (uint32_t t = 0; t < kMapRegTiles; ++t) {
        if (t < ntiles) {
            count_tile(t, rq[t], Lr[t], Cr[t], R0[t], true);
        }
    }
    if (ntiles > kMapRegTiles) {
        Quad nq = load(kMapRegTiles);
        for (uint32_t t = kMapRegTiles; t < ntiles; ++t) {
            const Quad q = nq;
            if (t + 1u < ntiles) {
                nq = load(t + 1u);  // the next tile in flight during this one
            }
            uint32_t L[kPlanV], c, r0;
            count_tile(t, q, L, c, r0, false);
        }
    }
    // wave reductions by DPP (the bpermute butterflies were a 6-deep chain
    // of LDS round trips per value)
    mn = wave_min(mn);
    mx = wave_max(mx);
    non1 = wave_sum(non1);
    full = wave_sum(full);
    mine64 = wave_sum64(mine64);
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&sh[2], mn);
        atomicMax(&sh[3], mx);
        atomicAdd(&sh[1], non1);
        atomicAdd(&segs64, (unsigned long long)mine64);
        if (full) {
            atomicAdd(&hist[c_full], full);
        }
    }
    __syncthreads();
    // a single-tile block whose messages all have the same segment count
    // leaves seg_first to the consumers (seg_first_g), as in k_plan
    const bool write_sf = !one_tile || sh[2] != sh[3];
    // the register tiles' deferred writes: out[], and seg_first when there
    // is no map to use
    auto deferred = [&](bool sf) {
#pragma unroll
        for (uint32_t t = 0; t < kMapRegTiles; ++t) {
            if (t < ntiles) {
                tile_words(lo + (uint64_t)t * kTile, Lr[t], R0[t], sf && write_sf);
            }
        }
    };
    // Publish the block words and the histogram, then arrive and wait.
    PLAN_STAMP(3)
    if (threadIdx.x < 64) {
        // Wave 0 publishes the block words and the histogram as
        // device-scope 64-bit stores, each word tagged with this launch's
        // epoch (they write through to memory, visible on every XCD once
        // complete), waits for them, then arrives: one flag word per block,
        // set to the epoch.  The readers load everything with device-scope
        // loads and check every word's tag, reading a stale one again, so no
        // visibility order is assumed between the flag and the words and
        // neither side needs an agent-scope fence (an L2 write-back /
        // invalidate: ~3 us of the wait, profiles/r03/ab/planner_stamps/).
        // No shared counter -- 256 atomics on one word serialize at the
        // memory side (11-16 us measured,
        // profiles/r03/ab/planner_phases_counter_wait/) -- and no reset: a
        // word of an older launch holds an older epoch.
        const unsigned long long tagv = (unsigned long long)ep << 32;
        if (lane < kBuckets) {
            __hip_atomic_store(&tags[lane * kPlanMaxBlocks + bid], tagv | hist[lane],
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (lane < 3) {
            const uint32_t wv = lane == 0   ? (segs64 > kSegLimit ? 0xffffffffu : carry)
                                : lane == 1 ? sh[1]
                                            : (sh[2] == sh[3] ? sh[2] : 0xffffffffu);
            __hip_atomic_store(&tags[kTagWords + lane * kPlanMaxBlocks + bid], tagv | wv,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            a.block_sum[lane * nb + bid] = wv;  // for k_fold (the next launch)
        }
        // round 4: no separate flag.  The poll reads each block's tagged
        // third block word (published beside its histogram, in no particular
        // order: the tag check below re-reads any word still stale), so the
        // wait for the stores' completion and the flag's own store and
        // visibility latency are gone from the meeting.
        const unsigned long long* const arrive = tags + kTagWords + 2u * kPlanMaxBlocks;
        constexpr int kArriveShift = 32;
        const uint64_t t0 = wall_clock64();
        uint32_t ok = 1u;
        static_assert(kPlanMaxBlocks <= 4 * 64, "four flags per lane");
        // a zero limit gives the map up before the first poll (the test hook
        // of bmqcrc_plan_wait(0): every such launch takes the fallback)
        bool waiting = a.map_wait_ticks != 0;
        if (!waiting) {
            ok = 0u;
            if (lane == 0) {
                give_up();
            }
        }
        while (waiting) {
            // all four loads in flight at once (a short-circuit chain made
            // them four round trips per poll), plus the launch's give-up word:
            // a block arriving after another gave the map up leaves at once
            // instead of waiting out its own limit
            unsigned long long f[4];
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t b = (uint32_t)lane + 64u * k;
                f[k] = b < nb ? __hip_atomic_load(&arrive[b], __ATOMIC_RELAXED,
                                                  __HIP_MEMORY_SCOPE_AGENT) >> kArriveShift
                              : (unsigned long long)ep;
            }
            const unsigned long long gone =
                __hip_atomic_load(&sync[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const bool mine = f[0] == ep && f[1] == ep && f[2] == ep && f[3] == ep;
            if (__ballot(!mine) == 0) {
                break;
            }
            if (gone == (unsigned long long)ep) {
                ok = 0u;  // another block gave this launch's map up
                break;
            }
            if (wall_clock64() - t0 >= a.map_wait_ticks) {
                ok = 0u;  // not all blocks running: give up the map, keep correctness
                if (lane == 0) {
                    give_up();
                }
                break;
            }
            __builtin_amdgcn_s_sleep(2);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (lane == 0) {
            go = ok;
        }
    }
    __syncthreads();
    PLAN_STAMP(4)
    // false: no map for k_fold (given up, or a closed form / past capacity
    // below); it then searches seg_first, and multi-segment messages
    // XOR-combine into out[] -- both written by deferred() in every path
    bool map = go != 0;
    // Batch shape and size from every block's words (closed-form batches
    // and those past seginfo's capacity or 32-bit indices need no map), and
    // this block's slice of every class (k_plan_sort's class-major order):
    // every load goes out at once, each wave reduces its share by DPP, and
    // one LDS exchange combines the waves.  Wave c sums class c over all
    // blocks (lane l: blocks l + 64 k); the block words are in waves 0-3.
    static_assert(kPlanBlock / 64 == kBuckets && kPlanMaxBlocks <= 4 * 64,
                  "one wave per size class, four blocks per lane");
    const uint32_t cw = threadIdx.x >> 6;
    const uint32_t j = threadIdx.x;
    uint32_t u0 = 0;
    if (map) {  // block-uniform (go is in LDS)
        const uint64_t t1 = wall_clock64();
        auto tagged = [&](const unsigned long long* p, uint32_t& val, bool& stale) {
            const unsigned long long x = __hip_atomic_load(p, __ATOMIC_RELAXED,
                                                           __HIP_MEMORY_SCOPE_AGENT);
            stale = stale || (uint32_t)(x >> 32) != ep;
            val = (uint32_t)x;
        };
        while (true) {
            bool stale = false;
            uint32_t hb[4], v = 0, nn = 0, u;
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t b = (uint32_t)lane + 64u * k;
                hb[k] = 0u;
                if (b < nb) {
                    tagged(&tags[cw * kPlanMaxBlocks + b], hb[k], stale);
                }
            }
            tagged(&tags[kTagWords + 2u * kPlanMaxBlocks], u0, stale);
            u = u0;
            if (j < nb) {
                tagged(&tags[kTagWords + j], v, stale);
                tagged(&tags[kTagWords + kPlanMaxBlocks + j], nn, stale);
                tagged(&tags[kTagWords + 2u * kPlanMaxBlocks + j], u, stale);
            }
            uint32_t tot = 0, pre = 0;
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                tot += hb[k];
                pre += (uint32_t)lane + 64u * k < bid ? hb[k] : 0u;
            }
            tot = wave_sum(tot);
            pre = wave_sum(pre);
            // (a block over the limit stores ~0: its wave's sum passes any capacity)
            const uint64_t segs = wave_sum64(v);
            const bool w_ragged = __ballot(nn != 0u) != 0, w_mixed = __ballot(u != u0) != 0;
            const bool w_stale = __ballot(stale) != 0;
            if (lane == 0) {
                part[0][0][cw] = tot;
                part[1][0][cw] = pre;
                part[0][1][cw] = (uint32_t)min(segs, (uint64_t)0xffffffffu);
                part[1][1][cw] = (w_ragged ? 1u : 0u) | (w_mixed ? 2u : 0u) | (w_stale ? 4u : 0u) |
                                 ((threadIdx.x == 0 && wall_clock64() - t1 >= a.map_wait_ticks)
                                      ? 8u : 0u);
            }
            __syncthreads();
            uint32_t f = 0;
#pragma unroll
            for (uint32_t w = 0; w < (uint32_t)kBuckets; ++w) {
                f |= part[1][1][w];
            }
            if (!(f & 4u)) {
                break;
            }
            // a word not yet visible: read again, within the same time limit
            if (f & 8u) {
                if (threadIdx.x == 0) {
                    give_up();
                }
                map = false;
                break;
            }
            __syncthreads();  // part[] read by all before the next round
        }
    }
    if (map) {
        uint32_t flags = 0;
        unsigned long long all = 0;
#pragma unroll
        for (uint32_t w = 0; w < (uint32_t)kBuckets; ++w) {
            flags |= part[1][1][w];
            all += part[0][1][w];
        }
        const bool ragged = flags & 1u, mixed = flags & 2u;
        if (!ragged || (!mixed && u0 != 0xffffffffu)) {
            map = false;  // identity or uniform: k_fold uses closed forms
        } else {
            // past seginfo's capacity: k_fold searches seg_first (or folds
            // whole messages past 32-bit segment indices)
            map = all <= min((unsigned long long)a.max_segs, (unsigned long long)kSegLimit);
        }
        if (threadIdx.x < kBuckets) {
            uint32_t acc = 0;
            const bool desc = a.class_desc;
            for (uint32_t c = 0; c < (uint32_t)kBuckets; ++c) {
                acc += (desc ? c > threadIdx.x : c < threadIdx.x) ? part[0][0][c] : 0u;
            }
            run[threadIdx.x] = acc + part[1][0][threadIdx.x];
        }
    }
    // seg_first in every path: should another block give the map up after
    // this one saw every arrival (its timer ran out between two polls),
    // k_fold searches seg_first for every segment of the batch (16 MB of
    // stores on Zipf 4M; round 3 skipped them and fell back to one lane per
    // message, a cliff of up to the longest message per wave).
    deferred(true);
    PLAN_STAMP(5)
    if (!map) {
        return;
    }
    __syncthreads();  // run[]
    PLAN_STAMP(6)
    // Phase 2: (message, k) of every segment.
    auto write_tile = [&](uint32_t t, const uint32_t (&L)[kPlanV], uint32_t cls) {
        const uint64_t base = lo + (uint64_t)t * kTile;
        // Full segments: one claim per wave for all its runs, short ones
        // (at most kMapShortRun segments) first, then long ones; each kind
        // in (lane, v) order.  The wave writes the short runs' range
        // together, 64 consecutive entries per store: slot j finds its run
        // by a binary search over the runs' ends, staged in LDS.  (Each lane
        // writing its own runs issued up to 4 kShortRun scattered stores per
        // tile: 16 of the planner's 58 us on Zipf 4M,
        // profiles/r03/ab/planner_stamps/sk1_component_skips.jsonl.)
        // Each long run is written by the whole wave, coalesced.
        uint32_t nf[kPlanV], ns_all = 0, nl_all = 0;
#pragma unroll
        for (uint32_t v = 0; v < kPlanV; ++v) {
            const uint32_t nseg = segments(L[v]);
            nf[v] = nseg ? nseg - 1u : 0u;
            ns_all += nf[v] <= kMapShortRun ? nf[v] : 0u;
            nl_all += nf[v] > kMapShortRun ? nf[v] : 0u;
        }
        const uint32_t xs = wave_incl_scan(ns_all), xl = wave_incl_scan(nl_all);
        const uint32_t ts = (uint32_t)__builtin_amdgcn_readlane((int)xs, 63);
        const uint32_t tl = (uint32_t)__builtin_amdgcn_readlane((int)xl, 63);
        if (ts + tl) {
            uint32_t pos = 0;
            if (lane == 0) {
                pos = atomicAdd(&run[c_full], ts + tl);
            }
            pos = (uint32_t)__builtin_amdgcn_readfirstlane((int)pos);
            const uint32_t w = threadIdx.x >> 6;
            const uint64_t wbase = base + (uint64_t)(threadIdx.x & ~63u) * kPlanV;
            if (ts) {
                uint32_t e = xs - ns_all, ends[kPlanV];
#pragma unroll
                for (uint32_t v = 0; v < kPlanV; ++v) {
                    e += nf[v] <= kMapShortRun ? nf[v] : 0u;
                    ends[v] = e;
                }
                *(u32x4*)&sruns[w][lane * kPlanV] = u32x4{ends[0], ends[1], ends[2], ends[3]};
                for (uint32_t j = (uint32_t)lane; j < ts; j += 64u) {
                    uint32_t q = 0;  // runs ending at or before j
#pragma unroll
                    for (uint32_t st = 32u * kPlanV; st; st >>= 1) {
                        q += sruns[w][q + st - 1u] <= j ? st : 0u;
                    }
                    const uint32_t k = j - (q ? sruns[w][q - 1u] : 0u);
                    put_full(a, pos + j, (uint32_t)(wbase + q), k);
                }
            }
            uint64_t longs = 0;
#pragma unroll
            for (uint32_t v = 0; v < kPlanV; ++v) {
                longs |= __ballot(nf[v] > kMapShortRun);
            }
            const uint32_t lpos = pos + ts + (xl - nl_all);
            if (longs) {
                // Every long run of the wave at once: its head and tail
                // entries (the partial groups at either end) are one list of
                // items over the wave, its whole groups another, each walked
                // 64 items per store.  (Run by run, a wave issued two to four
                // partly filled stores per run, and the long runs' stores
                // were 5.3 of the 1/8 shard's 21.5 us planner,
                // profiles/r05/ab/planner/phase_stamps_fullrun_split.jsonl.)
                // An item finds its run by a mark at the run's first item and
                // a max-scan over the wave (run indices grow with their
                // items); a wave's LDS operations complete in order, so
                // marks, reads and clearing need no barrier.  The shard's
                // planner 21.6 -> 20.7 us traced, the whole batch flat
                // (profiles/r05/ab/planner/long_flat_ab.jsonl): the bytes
                // stored, not the store count, are what remains.
                uint32_t atv[kPlanV], nv[kPlanV], ni[kPlanV], ng[kPlanV];
                uint32_t p = lpos;
#pragma unroll
                for (uint32_t v = 0; v < kPlanV; ++v) {
                    const uint32_t n = nf[v] > kMapShortRun ? nf[v] : 0u;
                    const uint32_t gf = (p + 63u) >> 6, ge = (p + n) >> 6;
                    const bool whole = gf < ge;
                    atv[v] = p;
                    nv[v] = n;
                    // entries only for a run inside one group touching
                    // neither of its ends; a run's head (the group's
                    // last lanes) and tail (its first lanes) are records
                    const bool inner = n && (p >> 6) == ((p + n - 1u) >> 6) && (p & 63u) &&
                                       ((p + n) & 63u);
                    ni[v] = inner ? n : 0u;
                    ng[v] = whole ? ge - gf : 0u;
                    p += n;
                }
                *(u32x4*)&slong[w][0][lane * kPlanV] = u32x4{atv[0], atv[1], atv[2], atv[3]};
                *(u32x4*)&slong[w][1][lane * kPlanV] = u32x4{nv[0], nv[1], nv[2], nv[3]};
                // Run records (round 6): a long run's partial groups
                // are described per group, not per slot -- its head
                // (lanes ho..63 of group at/64) by the group's suffix
                // record, its tail (lanes 0..te-1 of the last group) by
                // the prefix record and firstk; each side of a group has
                // one owner (the run covering lane 63, or lane 0).
                // Round 5 wrote up to 63 + 63 entries per long run, ~3 MB
                // on Zipf's 1/8 shard: 5.3 of its planner's 20.7 us
                // (profiles/r05/ab/planner/phase_stamps_fullrun_split.jsonl).
#pragma unroll
                for (uint32_t v = 0; v < kPlanV; ++v) {
                    const uint32_t at = atv[v], n = nv[v];
                    if (n == 0u) {
                        continue;
                    }
                    const uint32_t hb = at >> 6, tb = (at + n - 1u) >> 6;
                    const uint32_t ho = at & 63u, te = (at + n) & 63u;
                    const uint32_t msg = (uint32_t)(wbase + (uint32_t)lane * kPlanV + v);
                    if (ho != 0u && (hb < tb || te == 0u)) {
                        *(u32x4*)&a.grec[8u * hb + 4u] = u32x4{ep, msg, 64u - ho, 0u};
                    }
                    if (te != 0u && (hb < tb || ho == 0u)) {
                        *(u32x4*)&a.grec[8u * tb] = u32x4{ep, msg, te, 0u};
                        a.firstk[tb] = 64u * tb - at;
                    }
                }
                auto flat = [&](const uint32_t (&cnt)[kPlanV], auto&& body) {
                    const uint32_t mine = cnt[0] + cnt[1] + cnt[2] + cnt[3];
                    const uint32_t x = wave_incl_scan(mine);
                    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
                    uint32_t s0 = x - mine, st[kPlanV];
#pragma unroll
                    for (uint32_t v = 0; v < kPlanV; ++v) {
                        st[v] = cnt[v] ? s0 : 0xffffffffu;
                        s0 += cnt[v];
                    }
                    *(u32x4*)&sruns[w][lane * kPlanV] = u32x4{st[0], st[1], st[2], st[3]};
                    smark[w][lane] = 0u;
                    uint32_t open = 0u;
                    for (uint32_t j0 = 0; j0 < total; j0 += 64u) {
#pragma unroll
                        for (uint32_t v = 0; v < kPlanV; ++v) {
                            if (st[v] - j0 < 64u) {
                                smark[w][st[v] - j0] = (uint32_t)lane * kPlanV + v + 1u;
                            }
                        }
                        uint32_t o = smark[w][lane];
                        smark[w][lane] = 0u;
                        o = max(wave_incl_max(o), open);
                        open = (uint32_t)__builtin_amdgcn_readlane((int)o, 63);
                        const uint32_t j = j0 + (uint32_t)lane;
                        if (j < total) {
                            const uint32_t q = o - 1u;  // o >= 1: a run's items start at 0
                            body(q, j - sruns[w][q]);
                        }
                    }
                };
                flat(ni, [&](uint32_t q, uint32_t e) {
                    const uint32_t at = slong[w][0][q], n = slong[w][1][q];
                    const uint32_t gf = (at + 63u) >> 6, ge = (at + n) >> 6;
                    const uint32_t h = gf < ge ? 64u * gf - at : n;
                    const uint32_t slot = e < h ? at + e : 64u * ge + (e - h);
                    put_full(a, slot, (uint32_t)(wbase + q), slot - at);
                });
                flat(ng, [&](uint32_t q, uint32_t e) {
                    const uint32_t at = slong[w][0][q];
                    const uint32_t g = ((at + 63u) >> 6) + e;
                    a.gdesc[g] = (unsigned long long)ep << 32 | (uint32_t)(wbase + q);
                    a.firstk[g] = 64u * g - at;
                });
            }
        }
        // last (or only) segments: one returning LDS atomic per message
#pragma unroll
        for (uint32_t v = 0; v < kPlanV; ++v) {
            const uint32_t c = (cls >> (8u * v)) & 0xffu;
            if (c < (uint32_t)kBuckets) {
                const uint64_t i = base + (uint64_t)threadIdx.x * kPlanV + v;
                put_last(a, atomicAdd(&run[c], 1u), (uint32_t)i);
            }
        }
    };
#pragma unroll
    for (uint32_t t = 0; t < kMapRegTiles; ++t) {
        if (t < ntiles) {
            write_tile(t, Lr[t], Cr[t]);
        }
    }
    for (uint32_t t = kMapRegTiles; t < ntiles; ++t) {
        uint32_t L[kPlanV];
        uint64_t O[kPlanV];
        unpack_quad<O32>(a, load(t), lo + (uint64_t)t * kTile + (uint64_t)threadIdx.x * kPlanV, hi,
                         &tail, L, O);
        uint32_t cls = 0;
#pragma unroll
        for (uint32_t v = 0; v < kPlanV; ++v) {
            uint32_t c;
            (void)msg_segments(a, O[v], L[v], seg_shift, &c);
            cls |= c << (8u * v);
        }
        write_tile(t, L, cls);
    }
    __syncthreads();
    PLAN_STAMP(7)
