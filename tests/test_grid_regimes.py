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

`layout_split` is restated here and the four constants are read from the text
of bmqcrc_internal.h, so a changed constant fails this file instead of letting
test_gpu_rollover.py, test_gpu_confirm_records.py, test_gpu_copy.py,
test_gpu_put_pack.py, test_gpu_records_pack.py, test_gpu_storage_pack.py and
test_gpu_push_pack.py (with pack_pool.py and record_pool.py, their inputs),
which import the sizes below, quietly stop reaching their regimes."""
import collections
import os
import re

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


def constants():
    """kPackThreads, kPackBlocks, kPackFrameThreads, kPackFrameBlocks and
    kJournalRecordDwords as bmqcrc_internal.h spells them."""
    with open(HEADER) as f:
        text = f.read()
    found = {}
    for name in ("kPackThreads", "kPackBlocks", "kPackFrameThreads", "kPackFrameBlocks",
                 "kJournalRecordDwords"):
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


def test_layout_split_below_one_grid_of_tiles():
    # what the older tests run at: their sizes stay in the first regime
    assert layout_split(1, 1024, 256) == (1024, 1)
    assert layout_split(1025, 1024, 256) == (1024, 2)
    assert layout_split(3000, 1024, 256) == (1024, 3)
    assert not regime(3000).dwords_past_grid
