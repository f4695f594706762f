"""Buffers at a chosen base-pointer phase, for the tests that hand the library
pointers which are not the start of an allocation.

A fresh torch allocation starts at a multiple of 256 bytes or more, so a test
that passes `torch.from_numpy(a).to(device)` only ever runs with the low bits
of its base pointers zero.  `place` puts an array into a longer allocation
instead, `lead = 256 + phase` bytes behind a 256-byte boundary:

    view = place(a, phase, device)         view.data_ptr() % 256 == phase
    ... the call under test ...
    check_margins(view)

At least MARGIN bytes of the allocation lie in front of the view and MARGIN
behind it, all filled with SENTINEL; `check_margins` fails if one of them
changed -- a store rounded down to an aligned piece in front of a buffer, or
one that runs past its end.  `place` itself asserts where the allocation and
the view start, so a test built on it cannot run at phase 0 unnoticed.

This is a plain module (not a conftest): import it from the tests."""
import numpy as np

MARGIN = 256        # bytes in front of lead's phase part and behind the view (>= 128 each)
SENTINEL = 0xD7
_TORCH = {"uint8": "uint8", "int8": "int8", "int32": "int32", "uint32": "int32",
          "int64": "int64", "uint64": "int64"}


def place(a, phase, device, sentinel=SENTINEL):
    """`a` (uint8, int32, uint32, int64 or uint64 numpy array, any shape; the
    unsigned 32- and 64-bit ones become the int32 / int64 tensors the library's
    wrappers read as unsigned) as a contiguous tensor on `device` whose first
    byte lies `256 + phase` bytes into an allocation that starts on a 256-byte
    boundary.  `phase` is in bytes, in [0, 256), a multiple of the element
    size: arrays move by whole elements."""
    import torch
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:   # (torch warns about a read-only array)
        a = a.copy()
    if a.dtype.name not in _TORCH:
        raise TypeError("place takes 8-bit, 32-bit and 64-bit integer arrays, not %s" % a.dtype)
    phase = int(phase)
    if not 0 <= phase < 256 or phase % a.itemsize:
        raise ValueError("phase %d is not a multiple of the %d-byte element below 256"
                         % (phase, a.itemsize))
    lead, nbytes = MARGIN + phase, a.nbytes
    total = lead + nbytes + MARGIN
    # (a host allocation may start anywhere: cut the 256-aligned part out of it)
    raw = torch.empty(total + 256, dtype=torch.uint8, device=device)
    skip = -raw.data_ptr() % 256
    alloc = raw[skip:skip + total]
    alloc.fill_(sentinel)
    body = alloc[lead:lead + nbytes]
    if nbytes:
        body.copy_(torch.from_numpy(a.reshape(-1).view(np.uint8)))
    view = body.view(getattr(torch, _TORCH[a.dtype.name])).reshape(a.shape)
    assert alloc.data_ptr() % 256 == 0, alloc.data_ptr()
    if nbytes:      # (an empty tensor has no address)
        assert view.data_ptr() == alloc.data_ptr() + lead
        assert view.data_ptr() % 128 == phase % 128 and view.data_ptr() % 256 == phase
    assert view.is_contiguous() and view.numel() == a.size
    assert lead >= 128 and total - lead - nbytes >= 128
    view._placed = (alloc, lead, nbytes, sentinel)
    return view


def filled(count, dtype, value, phase, device, sentinel=SENTINEL):
    """An output array of `count` elements of numpy `dtype`, every one `value`
    (the caller's canary), placed like `place` does."""
    fill = np.array([value], np.uint64).astype(dtype)
    return place(np.repeat(fill, count), phase, device, sentinel)


class Placer:
    """The buffers of one call, placed by name: `phases` maps every pointer
    the call takes to its phase (a pointer it does not name is a KeyError, so
    none is left at the start of an allocation by oversight)."""

    def __init__(self, device, phases):
        self.device, self.phases, self.views = device, dict(phases), {}

    def put(self, name, a):
        v = place(a, self.phases[name], self.device)
        assert v.numel() == 0 or phase_of(v) == self.phases[name], name
        self.views[name] = v
        return v

    def fill(self, name, count, dtype, value):
        return self.put(name, np.repeat(np.array([value], np.uint64).astype(dtype), count))

    def check(self):
        for name, v in self.views.items():
            try:
                check_margins(v)
            except AssertionError as e:
                raise AssertionError("%s: %s" % (name, e)) from None


def phase_of(view):
    """The view's base pointer modulo 256."""
    return view.data_ptr() % 256


def margins(view):
    """(bytes in front, bytes behind) of a placed view, as numpy arrays."""
    alloc, lead, nbytes, _ = view._placed
    return alloc[:lead].cpu().numpy(), alloc[lead + nbytes:].cpu().numpy()


def check_margins(*views):
    """Both sentinel margins of every placed view are as `place` left them."""
    for k, view in enumerate(views):
        sentinel = view._placed[3]
        for side, m in zip(("in front of", "behind"), margins(view)):
            bad = np.nonzero(m != sentinel)[0]
            assert bad.size == 0, "view %d: %d bytes changed %s it, the first at margin byte %d" \
                % (k, bad.size, side, int(bad[0]))
