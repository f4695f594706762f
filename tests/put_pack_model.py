"""The PUT-event packer's layout restated in numpy, and its oracle (shared by
test_put_pack_model.py and test_gpu_put_pack.py; not a test module).

B[i] = 36 + lengths[i] + pad(lengths[i]), P = its 64-bit exclusive prefix,
e(i) = the event of message i:

    message i's header   at 8 (e(i) + 1) + P[i]
    event e              at 8 e + P[event_first[e]]
    event e's length     8 + P[event_first[e+1]] - P[event_first[e]]
"""
import numpy as np

from blazingmq_amd import Crc32c
from blazingmq_amd.put_event import PutEventBuilder

HDR, EVT = 36, 8


def pad_of(lens):
    return 4 - np.asarray(lens, np.int64) % 4


def layout(lens, event_first=None):
    """(header offset of every message, event offsets with the total last)."""
    lens = np.asarray(lens, np.int64)
    n = lens.size
    ef = np.array([0, n], np.int64) if event_first is None else np.asarray(event_first, np.int64)
    B = HDR + lens + pad_of(lens)
    P = np.concatenate([[0], np.cumsum(B)]).astype(np.int64)
    e = np.searchsorted(ef, np.arange(n), side="right") - 1
    hdr = EVT * (e + 1) + P[:n]
    ev = EVT * np.arange(ef.size) + P[ef]
    return hdr, ev


def model_bytes(src, soff, lens, qids, guids, flags, event_first, crcs):
    """The packed bytes from the formulas alone (no PutEventBuilder)."""
    lens = np.asarray(lens, np.int64)
    hdr, ev = layout(lens, event_first)
    img = np.zeros(int(ev[-1]), np.uint8)
    for e in range(ev.size - 1):
        at = int(ev[e])
        img[at:at + 4] = np.frombuffer(int(ev[e + 1] - ev[e]).to_bytes(4, "big"), np.uint8)
        img[at + 4:at + 8] = [(1 << 6) | 2, 2, 0, 0]
    for i in range(lens.size):
        h, ln = int(hdr[i]), int(lens[i])
        pad = 4 - ln % 4
        words = (HDR + ln + pad) // 4
        f = int(flags[i]) & 0xF if flags is not None else 0
        head = ((f << 28) | words).to_bytes(4, "big") + (9).to_bytes(4, "big") + \
            int(qids[i]).to_bytes(4, "big", signed=True) + bytes(guids[i]) + \
            int(crcs[i]).to_bytes(4, "big") + bytes(4)
        img[h:h + HDR] = np.frombuffer(head, np.uint8)
        img[h + HDR:h + HDR + ln] = src[int(soff[i]):int(soff[i]) + ln]
        img[h + HDR + ln:h + HDR + ln + pad] = pad
    return img


def oracle_events(src, soff, lens, qids, guids, flags, event_first, events=None):
    """PutEventBuilder(defer_crc=False), one builder per event: the list of
    finalized events (only those in `events` when given)."""
    n = len(lens)
    ef = [0, n] if event_first is None else [int(x) for x in event_first]
    out = []
    for e in (range(len(ef) - 1) if events is None else events):
        b = PutEventBuilder(defer_crc=False)
        for i in range(ef[e], ef[e + 1]):
            so, ln = int(soff[i]), int(lens[i])
            b.pack_message(src[so:so + ln].tobytes(), queue_id=int(qids[i]),
                           guid=bytes(guids[i]), flags=int(flags[i]) if flags is not None else 0)
        out.append(b.finalize())
    return out


def host_crcs(src, soff, lens):
    return np.array([Crc32c.calculate(src[int(s):int(s) + int(l)].tobytes())
                     for s, l in zip(soff, lens)], np.uint32)


def random_meta(rng, n):
    """(queue ids with negatives, guids (n, 16), flags 0..15)."""
    qids = rng.integers(-2**31, 2**31, size=n, dtype=np.int64).astype(np.int32)
    guids = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    flags = rng.integers(0, 16, size=n, dtype=np.uint8)
    return qids, guids, flags


# ---- the same bytes without a Python loop per message --------------------------

def be_bytes(a, width):
    """The low `width` bytes of every entry of `a`, big-endian: (n, width) uint8."""
    a = np.ascontiguousarray(np.asarray(a).astype(np.uint64).astype(">u8"))
    return a.view(np.uint8).reshape(-1, 8)[:, 8 - width:]


def byte_runs(starts, counts):
    """(owner, position) of every byte of the runs [starts[k], starts[k] +
    counts[k]): the index of the run it belongs to and where it lies."""
    counts = np.asarray(counts, np.int64)
    owner = np.repeat(np.arange(counts.size), counts)
    first = np.cumsum(counts) - counts  # of each run, among all runs' bytes
    within = np.arange(int(counts.sum()), dtype=np.int64) - first[owner]
    return owner, np.asarray(starts, np.int64)[owner] + within


def scatter_frames(img, at, frames):
    """img[at[k]:at[k] + w] = frames[k] for (n, w) uint8 frames; every at[k] and
    w are multiples of 4, so whole dwords are scattered."""
    frames = np.ascontiguousarray(frames, np.uint8)
    w = frames.shape[1] // 4
    assert frames.shape[1] % 4 == 0 and img.size % 4 == 0 and np.all(np.asarray(at) % 4 == 0)
    img.view(np.uint32)[(np.asarray(at, np.int64) // 4)[:, None] + np.arange(w)] = \
        frames.view(np.uint32).reshape(-1, w)


def place_payload(img, src, soff, lens, app, pad):
    """Message i's application data at img[app[i]:] by one gather from src, and
    its pad[i] padding bytes, each equal to their count, by one scatter."""
    lens = np.asarray(lens, np.int64)
    owner, to = byte_runs(app, lens)
    img[to] = np.asarray(src)[byte_runs(soff, lens)[1]]
    owner, to = byte_runs(np.asarray(app, np.int64) + lens, pad)
    img[to] = np.asarray(pad)[owner]


def model_bytes_fast(src, soff, lens, qids, guids, flags, event_first, crcs):
    """model_bytes in numpy alone: the EventHeaders from layout(), the PutHeaders
    as an (n, 36) array scattered to its offsets, the payload by one gather, the
    padding by one scatter."""
    lens = np.asarray(lens, np.int64)
    n = lens.size
    hdr, ev = layout(lens, event_first)
    img = np.zeros(int(ev[-1]), np.uint8)
    heads = np.zeros((ev.size - 1, EVT), np.uint8)
    heads[:, 0:4] = be_bytes(np.diff(ev), 4)
    heads[:, 4:8] = [(1 << 6) | 2, 2, 0, 0]
    scatter_frames(img, ev[:-1], heads)
    pad = pad_of(lens)
    f = np.asarray(flags, np.int64) & 0xF if flags is not None else np.zeros(n, np.int64)
    frames = np.zeros((n, HDR), np.uint8)
    frames[:, 0:4] = be_bytes((f << 28) | ((HDR + lens + pad) // 4), 4)
    frames[:, 4:8] = be_bytes(np.full(n, 9), 4)
    frames[:, 8:12] = be_bytes(np.asarray(qids, np.int64) & 0xFFFFFFFF, 4)
    frames[:, 12:28] = np.asarray(guids, np.uint8).reshape(n, 16)
    frames[:, 28:32] = be_bytes(crcs, 4)
    scatter_frames(img, hdr, frames)
    place_payload(img, src, soff, lens, hdr + HDR, pad)
    return img


def pool_crcs(src, pool_offsets, pool_lengths):
    """The CRC of every distinct source range, once."""
    return host_crcs(src, pool_offsets, pool_lengths)


def pooled_crcs(pool_crc, index):
    """Message i's CRC when its source range is pair index[i] of the pool."""
    return np.asarray(pool_crc, np.uint32)[np.asarray(index, np.int64)]
