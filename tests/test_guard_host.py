"""The guard-band helper of the device tests (tests/gpu_guard.py) on CPU tensors: a write into a band is reported with its offset, an
untouched buffer passes.  Without this a broken helper would make every test built on it vacuous."""
import pytest
import torch

from gpu_guard import BAND, guard, guard_slice


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
@pytest.mark.parametrize("offset", [0, 1, 3])
def test_guard_reports_a_write_into_either_band(dtype, offset):
    n = 37
    g = guard(n, dtype, "cpu", offset=offset)
    size = g.payload.element_size()
    assert g.payload.shape == (n,) and g.payload.dtype == dtype and bool(torch.isnan(g.payload).all())
    assert (g.payload.data_ptr() - offset * size) % 256 == 0 and g.start >= BAND + offset and g.raw.numel() - g.start - n >= BAND
    g.check()
    g.payload.fill_(1.5)                                    # the payload is the caller's: writing all of it changes no band
    g.check()
    whole = g.raw.view(dtype)
    for where, off in ((g.start - 1, -1), (g.start + n, n), (0, -g.start), (g.raw.numel() - 1, g.raw.numel() - 1 - g.start)):
        keep = g.raw[where].clone()
        whole[where] = 0.25                                 # a torch write through the float view of the same storage
        with pytest.raises(AssertionError, match=r"payload offset %d \(" % off):
            g.check("band")
        g.raw[where] = keep
        g.check()
    # a one-bit change (the sign of one band element) is a change
    g.raw[g.start + n + 5] ^= g.raw.new_tensor(-1 << (8 * size - 1))
    with pytest.raises(AssertionError, match="payload offset %d" % (n + 5)):
        g.check()


def test_guard_pattern_differs_from_element_to_element():
    for dtype in (torch.float32, torch.bfloat16, torch.float64):
        g = guard(5, dtype, "cpu")
        band = g.raw[:g.start]
        assert band.unique().numel() > band.numel() // 2 and not bool((band == 0).any())


def test_guard_keeps_caller_data_and_payload_snapshot():
    data = torch.arange(24, dtype=torch.float32)
    g = guard(24, torch.float32, "cpu", fill=data, shape=(2, 12))
    assert torch.equal(g.payload, data.view(2, 12))
    bits = g.bits()
    assert g.untouched(bits)
    g.payload[1, 3] = -7.0
    assert not g.untouched(bits)
    g.check()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_guard_slice_is_a_channel_range_between_band_channels(dtype):
    C, V = 3, 5 * 7 * 9                                     # odd V: the slice starts element-aligned only
    g = guard_slice(C, V, dtype, "cpu")
    assert g.payload.shape == (C, V) and g.c0 >= 1 and g.c0 * V >= BAND and g.c_total == 2 * g.c0 + C
    size = g.payload.element_size()
    assert (g.payload.data_ptr() - g.c0 * V * size) % 256 == 0 and g.payload.data_ptr() % 16 == (g.c0 * V * size) % 16
    g.check()
    buf = g.raw[g.start - g.c0 * V:g.start + (g.c0 + C) * V].view(dtype).view(g.c_total, V)
    assert bool(torch.isnan(buf[g.c0:g.c0 + C]).all())
    buf[g.c0 - 1, V - 1] = 2.0                               # the last voxel of the neighbouring channel in front
    with pytest.raises(AssertionError, match=r"payload offset -1 \("):
        g.check()
    g = guard_slice(C, V, dtype, "cpu", fill=torch.ones(C, V))
    buf = g.raw[g.start - g.c0 * V:g.start + (g.c0 + C) * V].view(dtype).view(g.c_total, V)
    buf[g.c0 + C, 0] = 2.0                                   # the first voxel of the channel behind
    with pytest.raises(AssertionError, match=r"payload offset %d \(" % (C * V)):
        g.check()
