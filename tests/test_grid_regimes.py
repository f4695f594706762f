"""The sizes at which the device calls' shared grids change what they run, and
the sizes the large GPU tests use to get there (no GPU needed).

Every device call splits its units -- messages, records, confirms -- with
layout_split (bmqcrc_host.cpp): at most kPackBlocks blocks of whole
kPackThreads tiles each.  A frame kernel of kPackFrameBlocks x
kPackFrameThreads threads then strides over 15 dwords per unit and over the
units.  Above certain sizes the same code runs loops it never enters below:

  A  15 n > frame grid     the frame kernels' dword loop takes a second step
  B  more than 64 blocks   block_prefix's cross-wave leg (before += wsum[0][w])
  C  kPackBlocks blocks    the whole layout grid, one tile each
  D  per_block > one tile  stage()'s second tile, layout_count's carry from tile
                           to tile inside a block
  E  n > frame grid        the frame kernels' per-unit loops take a second step

The two walkers, bmqcrc_put_event_unpack and bmqcrc_storage_event_apply, walk
one event per wave on a grid of at most kUnpackWalkBlocks blocks, scan the
events' message counts in one block of kUnpackThreads, and publish (frame) on a
grid of kUnpackPublishBlocks x kUnpackPublishThreads (the frame grid) threads:

  F  n_events > 4,096      a walk block's second event, in both walks
  G  n_events > 1,024      the scan's second tile
  H  place > walk          placing blocks that walk no event and only empty slots
  I  n > 524,288           the second message step of publish / frame
  J  n_events + 1 > 524,288  the second step of the event_first loop

The apply also splits its layout grid by msg_cap, not by the messages found,
so A to D hold for it taken over msg_cap.

`layout_split` is restated here and the constants are read from the text
of bmqcrc_internal.h, so a changed constant fails this file instead of letting
test_gpu_rollover.py, test_gpu_confirm_records.py, test_gpu_copy.py,
test_gpu_put_pack.py, test_gpu_records_pack.py, test_gpu_storage_pack.py,
test_gpu_push_pack.py, test_gpu_put_unpack.py and test_gpu_storage_apply.py
(with pack_pool.py and record_pool.py, their inputs), which import the sizes
and event splits below, quietly stop reaching their regimes."""
import collections
import os
import re

import numpy as np
import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                      "blazingmq_amd", "csrc", "bmqcrc_internal.h")

N_WAVES = 65537 + 1024          # A and B: 66 blocks of one tile
N_FULL = 262144                 # C (A and B too): 256 blocks of one tile
N_TILES = 256 * 1024 + 1025     # D: 129 blocks of two tiles
N_FRAME = 524289                # E: 171 blocks of three tiles; unit 524,288 is frame thread 0's
N_FEW = 40000                   # A alone: 40 blocks of one tile, one wave of block sums
RECORD_DWORDS = 15              # kJournalRecordDwords: a journal record is 60 bytes

Regime = collections.namedtuple(
    "Regime", "nblocks per_block dwords_past_grid units_past_grid cross_wave")


PACK_CONSTANTS = ("kPackThreads", "kPackBlocks", "kPackFrameThreads", "kPackFrameBlocks",
                  "kJournalRecordDwords")
WALK_CONSTANTS = ("kUnpackWalkThreads", "kUnpackWalkBlocks", "kUnpackThreads",
                  "kUnpackPublishThreads", "kUnpackPublishBlocks")


def constants(names=PACK_CONSTANTS):
    """kPackThreads, kPackBlocks, kPackFrameThreads, kPackFrameBlocks and
    kJournalRecordDwords (or `names`) as bmqcrc_internal.h spells them."""
    with open(HEADER) as f:
        text = f.read()
    found = {}
    for name in names:
        m = re.findall(r"constexpr (?:int|uint32_t) %s = (\d+);" % name, text)
        assert len(m) == 1, (name, m)
        found[name] = int(m[0])
    return found


def layout_split(n, threads, blocks):
    """(per_block, nblocks) as bmqcrc_host.cpp's layout_split gives them, n > 0."""
    tiles = (n + threads - 1) // threads
    nb = min(tiles, blocks)
    tiles_per = (tiles + nb - 1) // nb
    return tiles_per * threads, (tiles + tiles_per - 1) // tiles_per


def regime(n):
    """What a call over n units runs, by today's header."""
    k = constants()
    per_block, nblocks = layout_split(n, k["kPackThreads"], k["kPackBlocks"])
    grid = k["kPackFrameThreads"] * k["kPackFrameBlocks"]
    return Regime(nblocks, per_block, k["kJournalRecordDwords"] * n > grid, n > grid,
                  nblocks > 64)


def test_the_constants_the_sizes_were_derived_from():
    assert constants() == dict(kPackThreads=1024, kPackBlocks=256, kPackFrameThreads=256,
                               kPackFrameBlocks=2048, kJournalRecordDwords=RECORD_DWORDS)


@pytest.mark.parametrize("n,want", [
    (N_FEW, Regime(40, 1024, True, False, False)),
    (N_WAVES, Regime(66, 1024, True, False, True)),
    (N_FULL, Regime(256, 1024, True, False, True)),
    (N_TILES, Regime(129, 2048, True, False, True)),
    (N_FRAME, Regime(171, 3072, True, True, True)),
], ids=["N_FEW", "N_WAVES", "N_FULL", "N_TILES", "N_FRAME"])
def test_each_size_reaches_the_regime_it_claims(n, want):
    assert regime(n) == want


def test_the_first_size_of_every_regime():
    # A: 15 n > 524,288
    assert not regime(34952).dwords_past_grid and regime(34953).dwords_past_grid
    # B: a 65th block, whose sum lies in the second wave of block_prefix
    assert regime(65536) == Regime(64, 1024, True, False, False)
    assert regime(65537) == Regime(65, 1024, True, False, True)
    # C and D: the last size with one tile per block, the first with two
    assert regime(N_FULL - 1023)[:2] == (256, 1024)
    assert regime(N_FULL)[:2] == (256, 1024)
    assert regime(N_FULL + 1)[:2] == (129, 2048)
    # E: unit 524,288 is the first that a frame thread reaches in its second step
    assert not regime(N_FRAME - 1).units_past_grid and regime(N_FRAME).units_past_grid
    assert regime(N_FRAME - 1)[:2] == (256, 2048) and regime(N_FRAME)[:2] == (171, 3072)


def test_every_block_of_the_large_sizes_owns_units():
    # no empty block, and the last block ends the call: a refusal "in the last
    # record of the last block" is record n - 1 of block nblocks - 1
    for n in (N_FEW, N_WAVES, N_FULL, N_TILES, N_FRAME):
        r = regime(n)
        assert (r.nblocks - 1) * r.per_block < n <= r.nblocks * r.per_block


def seal_events():
    """kSealEvents as crc32c_pack_layout.h spells it."""
    with open(os.path.join(os.path.dirname(HEADER), "crc32c_pack_layout.h")) as f:
        m = re.findall(r"constexpr uint32_t kSealEvents = (\d+);", f.read())
    assert len(m) == 1, m
    return int(m[0])


def steps(entries, threads):
    """Steps of a grid-stride loop of `threads` threads over `entries` entries."""
    return (entries + threads - 1) // threads


def test_what_the_put_and_record_packers_reach():
    # test_gpu_put_pack.py and test_gpu_records_pack.py: their frame kernels
    # stride over 9 and 3 dwords per message, not 15
    k = constants()
    grid = k["kPackFrameThreads"] * k["kPackFrameBlocks"]
    assert steps(9 * 58254, grid) == 1 and steps(9 * 58255, grid) == 2      # PutHeader
    assert steps(3 * 174762, grid) == 1 and steps(3 * 174763, grid) == 2    # DataHeader
    for n in (N_WAVES, N_FULL, N_TILES, N_FRAME):
        assert steps(9 * n, grid) >= 2, n
    assert steps(3 * N_WAVES, grid) == 1 and steps(3 * N_FULL, grid) == 2
    # one event per message at N_FRAME: event_first's N_FRAME + 1 entries over
    # the layout grid, the events over k_pack_check's grid, the EventHeaders
    # over the frame grid
    r = regime(N_FRAME)
    assert steps(N_FRAME + 1, r.nblocks * k["kPackThreads"]) == 3
    assert steps(N_FRAME, k["kPackBlocks"] * k["kPackThreads"]) == 3
    assert steps(N_FULL, k["kPackBlocks"] * k["kPackThreads"]) == 1
    assert steps(N_FRAME + 1, grid) == 2 and steps(N_FRAME - 1, grid) == 1
    # seal_offsets at N_TILES: a block of single-message events is past the
    # events it searches in LDS, a block of 3-message events is not
    per_block = regime(N_TILES).per_block
    assert seal_events() == 1024
    assert per_block - 1 >= seal_events() > (per_block + 2) // 3 + 1


def test_what_the_storage_and_push_packers_reach():
    # test_gpu_storage_pack.py and test_gpu_push_pack.py: their frame kernels
    # stride over 18 dwords per record and over 8..11 per message
    k = constants()
    grid = k["kPackFrameThreads"] * k["kPackFrameBlocks"]
    assert steps(18 * 29127, grid) == 1 and steps(18 * 29128, grid) == 2    # StorageHeader + record
    assert steps(8 * 65536, grid) == 1 and steps(8 * 65537, grid) == 2      # PushHeader alone
    assert steps(11 * 47662, grid) == 1 and steps(11 * 47663, grid) == 2    # with a SubQueueInfo
    for n in (N_WAVES, N_FULL, N_TILES, N_FRAME):
        assert steps(18 * n, grid) >= 2 and steps(8 * n, grid) >= 2, n
    # the per-unit loops of both, and k_ppk_seal's size-only loop over
    # n_events + 1 entries of the layout grid
    assert steps(N_TILES, grid) == 1 and steps(N_FRAME, grid) == 2
    r = regime(N_FRAME)
    assert steps(N_FRAME + 1, r.nblocks * k["kPackThreads"]) == 3
    r = regime(N_TILES)
    assert steps(N_TILES // 3 + 2, r.nblocks * k["kPackThreads"]) == 1


def event_of(first, i):
    """Last e with first[e] <= i, as crc32c_pack_layout.h's event_of finds it."""
    lo, hi = 0, len(first) - 2
    while lo < hi:
        mid = lo + (hi - lo + 1) // 2
        if first[mid] <= i:
            lo = mid
        else:
            hi = mid - 1
    return lo


def seal_range(first, n, per_block, block):
    """(e1 - e0, staged) of seal_offsets for a block that owns units."""
    lo, hi = block * per_block, min((block + 1) * per_block, n)
    e0, e1 = event_of(first, lo), event_of(first, hi - 1)
    return e1 - e0, e0 != e1 and e1 - e0 < seal_events()


SEAL_BLOCK = 85      # the block whose first message is an event of its own in boundary_split


def events_of_3(n):
    return list(range(0, n, 3)) + [n]


def boundary_split(n, per_block, block=SEAL_BLOCK):
    """event_first of events of 3 but for one event of 1, the first message of
    `block`; the last event takes the remainder."""
    cut = block * per_block
    assert cut % 3 == 0 and cut + 1 < n
    return list(range(0, cut, 3)) + list(range(cut, cut + 1)) + list(range(cut + 1, n, 3)) + [n]


def test_the_seal_stages_a_block_of_exactly_its_array_and_no_more():
    r = regime(N_FRAME)
    assert r.per_block == 3072 == 3 * seal_events() and 0 < SEAL_BLOCK < r.nblocks - 1 == 170
    full = range(r.nblocks - 1)         # the last block owns 2,049 units
    first = events_of_3(N_FRAME)
    for b in full:      # e1 - e0 + 1 entries staged: every LDS entry used
        assert seal_range(first, N_FRAME, r.per_block, b) == (seal_events() - 1, True), b
    first = boundary_split(N_FRAME, r.per_block)
    assert first[0] == 0 and first[-1] == N_FRAME and all(a < b for a, b in zip(first, first[1:]))
    assert first.count(SEAL_BLOCK * r.per_block) == first.count(SEAL_BLOCK * r.per_block + 1) == 1
    for b in full:
        want = (seal_events() - 1, True) if b < SEAL_BLOCK else (seal_events(), False)
        assert seal_range(first, N_FRAME, r.per_block, b) == want, b
    assert seal_range(first, N_FRAME, r.per_block, r.nblocks - 1) == (683, True)
    # and with an event per unit at N_TILES the last block's 1,025 units lie in
    # exactly kSealEvents + 1 events: not staged either
    r = regime(N_TILES)
    assert seal_range(range(N_TILES + 1), N_TILES, r.per_block, r.nblocks - 1) == (
        seal_events(), False)
    assert seal_range(range(N_TILES + 1), N_TILES, r.per_block, 0) == (r.per_block - 1, False)


# ---- the walkers: bmqcrc_put_event_unpack and bmqcrc_storage_event_apply ---------

RAGGED_SIZES = (1, 63, 64, 65, 130, 7)      # the lane edges of a wave's 64-message flush
EMPTY_RUN_AT, EMPTY_RUN = 300, 65           # events 300..364 of RAGGED hold no message
SECOND_STEP = 4096                          # the first event of walk block 0's second step

Walk = collections.namedtuple(
    "Walk", "walk place second_event scan_tiles idle_placing msgs_past_grid first_past_grid")


def ones(n):
    """event_first of one unit per event."""
    return np.arange(n + 1, dtype=np.int64)


def ragged(n, empties=True):
    """event_first of n units in events whose sizes cycle through RAGGED_SIZES
    (the last takes what is left).  With `empties`, events of no unit: the
    first of all and the last of all, EMPTY_RUN in a row from event
    EMPTY_RUN_AT on (the middle one, with fewer events) and, where there are
    that many events, event SECOND_STEP."""
    sizes = np.tile(np.array(RAGGED_SIZES, np.int64), n // sum(RAGGED_SIZES) + 1)
    ends = np.cumsum(sizes)
    k = int(np.searchsorted(ends, n))
    sizes = sizes[:k + 1].copy()
    sizes[k] = n - (int(ends[k - 1]) if k else 0)
    if empties:
        sizes = np.insert(sizes, 0, 0)
        sizes = np.insert(sizes, [min(EMPTY_RUN_AT, sizes.size // 2)] * EMPTY_RUN, 0)
        if sizes.size > SECOND_STEP:
            sizes = np.insert(sizes, SECOND_STEP, 0)
        sizes = np.append(sizes, 0)
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def cap_inside_the_third_tile(first):
    """(event, msg_cap) for TOO_MANY_MESSAGES from the scan's third tile: the
    first 130-message event from event 2,748 on, and 30 messages into it."""
    e = 2748 + int(np.argmax(np.diff(first)[2748:] == 130))
    return e, int(first[e]) + 30


def walk_grids(n_events, msg_cap):
    """(walk, place) blocks as bmqcrc_launch_unpack_walk and
    bmqcrc_launch_storage_apply_layout give them, n_events > 0."""
    k = constants(WALK_CONSTANTS)
    walk = min(n_events, k["kUnpackWalkBlocks"])
    fill = msg_cap // (16 * k["kUnpackWalkThreads"])
    return walk, max(walk, min(fill, k["kUnpackWalkBlocks"]))


def publish_threads(n_events, msg_cap):
    """Threads of k_unpack_publish's grid (bmqcrc_launch_unpack_publish)."""
    k = constants(WALK_CONSTANTS)
    blocks = min(steps(max(msg_cap, n_events + 1), k["kUnpackPublishThreads"]),
                 k["kUnpackPublishBlocks"])
    return blocks * k["kUnpackPublishThreads"]


def apply_frame_threads(msg_cap):
    """Threads of k_sap_frame's grid (bmqcrc_launch_storage_apply_frame)."""
    k = constants()
    blocks = min(max(steps(k["kJournalRecordDwords"] * msg_cap, k["kPackFrameThreads"]), 1),
                 k["kPackFrameBlocks"])
    return blocks * k["kPackFrameThreads"]


def walk_regime(first, msg_cap=None):
    """What either walker runs over the events `first` (an event_first), by
    today's header; msg_cap None: the message count."""
    n_events, n = len(first) - 1, int(first[-1])
    cap = n if msg_cap is None else msg_cap
    walk, place = walk_grids(n_events, cap)
    k = constants(WALK_CONSTANTS)
    return Walk(walk, place, n_events > walk, steps(n_events, k["kUnpackThreads"]),
                place > walk, n > publish_threads(n_events, cap),
                n_events + 1 > publish_threads(n_events, cap))


def test_the_walkers_constants_and_grids():
    assert constants(WALK_CONSTANTS) == dict(
        kUnpackWalkThreads=64, kUnpackWalkBlocks=4096, kUnpackThreads=1024,
        kUnpackPublishThreads=256, kUnpackPublishBlocks=2048)
    # walk = min(n_events, 4096), place = max(walk, min(msg_cap // 1024, 4096))
    assert walk_grids(1, 1) == (1, 1) and walk_grids(257, 526593 + 300000) == (257, 807)
    assert walk_grids(4096, 5000) == (4096, 4096) and walk_grids(5000, 5000) == (4096, 4096)
    assert walk_grids(3, 4096 * 1024 - 1) == (3, 4095)
    assert walk_grids(3, 1 << 40) == (3, 4096)
    # both frame grids are full long before the sizes below, and as large as
    # the packers' frame grid: regimes A and E hold for the apply as they stand
    grid = 2048 * 256
    assert publish_threads(1, 1) == 256 and publish_threads(5000, 3) == 5120
    assert publish_threads(10, grid - 255) == grid == publish_threads(10, 1 << 40)
    assert apply_frame_threads(0) == 256 and apply_frame_threads(17) == 256
    assert apply_frame_threads(34935) == grid - 256 and apply_frame_threads(34936) == grid
    k = constants()
    assert grid == k["kPackFrameThreads"] * k["kPackFrameBlocks"]
    # what the two older large cases run: 257 events never leave the first step
    old = walk_regime(2049 * np.arange(258), 526593 + 300000)
    assert old == Walk(257, 807, False, 1, True, True, False)
    assert walk_regime(np.arange(5001)) == Walk(4096, 4096, True, 5, False, False, False)


def test_the_event_splits():
    assert sum(RAGGED_SIZES) == 330 and set(RAGGED_SIZES) >= {1, 63, 64, 65, 130}
    for n in (1, 64, 329, 330, 331):
        assert np.array_equal(ones(n), range(n + 1))
        assert ragged(n, empties=False).tolist() == [
            x for x in (0, 1, 64, 128, 193, 323, 330, 331) if x < n] + [n]
    for n in (4101, N_WAVES, N_FULL, N_TILES, N_FRAME):
        plain, first = ragged(n, empties=False), ragged(n)
        for f in (plain, first):
            assert f[0] == 0 and f[-1] == n and bool((np.diff(f) >= 0).all())
        sizes = np.diff(plain)
        assert bool((sizes > 0).all())
        assert sizes[:-1].tolist() == list(RAGGED_SIZES * (n // 330 + 1))[:sizes.size - 1]
        assert 0 < sizes[-1] <= RAGGED_SIZES[(sizes.size - 1) % 6]
        # the empties: first, last, the run and (with enough events) event 4,096
        empty = np.flatnonzero(np.diff(first) == 0)
        run_at = min(EMPTY_RUN_AT, plain.size // 2)
        want = [0] + list(range(run_at, run_at + EMPTY_RUN)) + \
            ([SECOND_STEP] if plain.size + EMPTY_RUN > SECOND_STEP else []) + \
            [first.size - 2]
        assert empty.tolist() == want, n
        assert np.array_equal(np.diff(first)[np.diff(first) > 0], sizes)
    assert ragged(N_TILES).size - 1 > SECOND_STEP + 3
    # event 4,099, a walk block's second event, holds messages
    assert np.diff(ragged(N_TILES))[SECOND_STEP:SECOND_STEP + 4].tolist()[0] == 0
    assert np.diff(ragged(N_TILES))[SECOND_STEP + 1:SECOND_STEP + 5].tolist() == [130, 7, 1, 63]


@pytest.mark.parametrize("name,first,cap,want", [
    # RAGGED with its empties: about 1,200 events at N_WAVES, 9,500 at N_FRAME
    ("waves", ragged(N_WAVES), None, Walk(1278, 1278, False, 2, False, False, False)),
    ("full", ragged(N_FULL), None, Walk(4096, 4096, True, 5, False, False, False)),
    ("tiles", ragged(N_TILES), None, Walk(4096, 4096, True, 5, False, False, False)),
    ("frame", ragged(N_FRAME), None, Walk(4096, 4096, True, 10, False, True, False)),
    ("frame-ones", ones(N_FRAME), None, Walk(4096, 4096, True, 513, False, True, True)),
    ("tiles-ones", ones(N_TILES), None, Walk(4096, 4096, True, 258, False, False, False)),
    # H needs msg_cap // 1,024 above the event count: none of these splits
    # reaches it under the caps the GPU cases use (the older uniform cases of
    # 257 events, above, do)
    ("waves-wide", ragged(N_WAVES), N_WAVES + 300000, Walk(1278, 1278, False, 2, False, False,
                                                            False)),
    ("waves-cap-tiles", ragged(N_WAVES), N_TILES, Walk(1278, 1278, False, 2, False, False,
                                                        False)),
    ("waves-cap-frame", ragged(N_WAVES), N_FRAME, Walk(1278, 1278, False, 2, False, False,
                                                        False)),
], ids=lambda v: v if isinstance(v, str) else "")
def test_what_each_split_reaches(name, first, cap, want):
    got = walk_regime(first, cap)
    assert got == want, got


def test_msg_cap_splits_the_applys_layout_grid():
    # layout_split(msg_cap): at N_WAVES messages the checks' lo / hi follow the
    # split of another size, and the blocks behind the 66th own no message
    assert regime(N_WAVES + 300000)[:2] == (179, 2048)
    assert regime(N_TILES)[:2] == (129, 2048) and regime(N_FRAME)[:2] == (171, 3072)
    assert steps(N_WAVES, 2048) == 33 < 129 and steps(N_WAVES, 3072) == 22 < 171
    assert regime(N_FRAME + 300000)[:2] == (202, 4096)
    # TOO_MANY_MESSAGES from the scan's 513th tile, and from its third
    assert steps(N_FRAME, 1024) == 513 and (N_FRAME - 1) // 1024 == 512
    first = ragged(N_TILES)
    e, cap = cap_inside_the_third_tile(first)
    assert 2048 <= e < 3072 and first[e + 1] - first[e] == 130
    assert first[e] < cap < first[e + 1] - 1
    assert int(np.searchsorted(first, cap, side="right")) - 1 == e


def test_layout_split_below_one_grid_of_tiles():
    # what the older tests run at: their sizes stay in the first regime
    assert layout_split(1, 1024, 256) == (1024, 1)
    assert layout_split(1025, 1024, 256) == (1024, 2)
    assert layout_split(3000, 1024, 256) == (1024, 3)
    assert not regime(3000).dwords_past_grid
