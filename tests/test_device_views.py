"""tests/device_views.py on host tensors: the phases it promises, the margins
it lays out, and that its margin check notices a write into either of them."""
import numpy as np
import pytest

import device_views as V


@pytest.mark.parametrize("dtype,phases", [
    (np.uint8, [0, 1, 3, 4, 8, 12, 15, 16, 17, 63, 64, 65, 100, 127, 128, 129, 255]),
    (np.int32, [0, 4, 8, 12, 60, 124, 132]),
    (np.uint32, [4, 8, 12, 252]),
    (np.int64, [0, 8, 24, 72, 120, 136]),
    (np.uint64, [8, 248])])
def test_phases_contents_and_margins(dtype, phases):
    import torch
    rng = np.random.default_rng(1)
    for phase in phases:
        a = rng.integers(0, 1 << 31, size=37).astype(dtype)
        v = V.place(a, phase, "cpu")
        alloc, lead, nbytes, sentinel = v._placed
        assert alloc.data_ptr() % 256 == 0
        assert v.data_ptr() == alloc.data_ptr() + 256 + phase
        assert v.data_ptr() % 128 == phase % 128 and V.phase_of(v) == phase
        assert v.is_contiguous() and v.device.type == "cpu"
        assert v.dtype == {1: torch.uint8, 4: torch.int32, 8: torch.int64}[a.itemsize]
        assert np.array_equal(v.numpy().view(dtype), a)
        front, back = V.margins(v)
        assert front.size == lead >= 128 and back.size >= 128
        assert nbytes == a.nbytes and lead + nbytes + back.size == alloc.numel()
        assert (front == sentinel).all() and (back == sentinel).all()
        V.check_margins(v)


def test_shapes_empty_arrays_and_read_only_input():
    a = np.arange(48, dtype=np.uint8).reshape(3, 16)
    a.setflags(write=False)
    v = V.place(a, 3, "cpu")
    assert tuple(v.shape) == (3, 16) and np.array_equal(v.numpy(), a)
    e = V.place(np.zeros(0, np.int64), 8, "cpu")
    assert e.numel() == 0
    V.check_margins(v, e)
    f = V.filled(5, np.uint32, 0x5A5A5A5A, 12, "cpu")
    assert V.phase_of(f) == 12 and f.numpy().view(np.uint32).tolist() == [0x5A5A5A5A] * 5
    g = V.filled(2, np.uint64, 0x5A5A5A5A5A5A5A5A, 8, "cpu")
    assert g.numpy().view(np.uint64).tolist() == [0x5A5A5A5A5A5A5A5A] * 2


@pytest.mark.parametrize("dtype,phase", [(np.int32, 1), (np.uint32, 6), (np.int64, 4),
                                         (np.uint8, -1), (np.uint8, 256)])
def test_a_phase_that_is_no_whole_element_is_refused(dtype, phase):
    with pytest.raises(ValueError):
        V.place(np.zeros(4, dtype), phase, "cpu")
    with pytest.raises(TypeError):
        V.place(np.zeros(4, np.float32), 0, "cpu")


@pytest.mark.parametrize("where", ["last byte in front", "first byte behind", "first byte of all",
                                   "last byte of all"])
def test_the_margin_check_fails_after_a_planted_write(where):
    v = V.place(np.arange(100, dtype=np.uint8), 5, "cpu")
    alloc, lead, nbytes, sentinel = v._placed
    at = {"last byte in front": lead - 1, "first byte behind": lead + nbytes,
          "first byte of all": 0, "last byte of all": alloc.numel() - 1}[where]
    V.check_margins(v)
    alloc[at] = sentinel ^ 0xFF
    with pytest.raises(AssertionError, match="in front of" if at < lead else "behind"):
        V.check_margins(v)
    alloc[at] = sentinel
    V.check_margins(v)
    v[0] = 77                       # a write inside the view is not the margins' business
    V.check_margins(v)
