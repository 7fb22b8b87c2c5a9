"""The guarded-buffer helper of the buffer-contract tests (tests/guarded.py) can fail: a byte written just outside the payload
is reported, a byte written inside it is not, and the views are what a kernel would get from torch."""
import numpy as np
import pytest
import torch

import guarded as gd

SHAPES = [((1,), torch.float32), ((3, 17, 3), torch.float32), ((5,), torch.uint8), ((7, 2), torch.int32), ((2, 3), torch.float64),
          ((4, 1, 2), torch.uint64 if hasattr(torch, "uint64") else torch.int64), ((0, 4), torch.float32)]


@pytest.mark.parametrize("shape,dtype", SHAPES)
@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_view_is_what_was_asked_for(shape, dtype, fill):
    view, parent = gd.guarded(shape, dtype, "cpu", fill, guard_bytes=1000)   # a guard size that is no multiple of 256
    assert view.is_contiguous() and view.dtype == dtype and tuple(view.shape) == shape
    off, n = gd.span(parent)
    assert off % 256 == 0 and off >= 1000 and parent.numel() - off - n >= 1000
    assert n == view.numel() * view.element_size()
    assert view.numel() == 0 or view.data_ptr() == parent.data_ptr() + off
    assert bool((parent[off:off + n] == fill).all())
    assert bool((parent[:off] == gd.GUARD_BYTE).all()) and bool((parent[off + n:] == gd.GUARD_BYTE).all())
    assert gd.guards_intact(parent)
    if dtype == torch.float32 and view.numel():
        assert bool(torch.isnan(view).all()) if fill == 0xFF else bool((view == 0).all())
    if dtype == torch.int32 and fill == 0xFF:
        assert bool((view == -1).all())


def test_default_guard_is_256_kib_on_both_sides():
    view, parent = gd.guarded((3,), torch.float32, "cpu", 0)
    off, n = gd.span(parent)
    assert off == 256 * 1024 and parent.numel() == 2 * 256 * 1024 + 12


@pytest.mark.parametrize("where", ["before", "after", "first_guard_byte", "last_guard_byte"])
def test_a_write_outside_the_payload_is_reported(where):
    view, parent = gd.guarded((3, 5), torch.float32, "cpu", 0xFF, guard_bytes=4096)
    off, n = gd.span(parent)
    snap = gd.snapshot(parent)
    at = {"before": off - 1, "after": off + n, "first_guard_byte": 0, "last_guard_byte": parent.numel() - 1}[where]
    parent[at] = 0
    assert not gd.guards_intact(parent)
    assert not gd.unchanged(parent, snap)
    parent[at] = gd.GUARD_BYTE
    assert gd.guards_intact(parent) and gd.unchanged(parent, snap)


def test_a_write_with_the_fill_byte_of_the_payload_is_reported_too():
    view, parent = gd.guarded((4,), torch.int32, "cpu", 0x00, guard_bytes=512)
    off, n = gd.span(parent)
    parent[off + n] = 0x00
    assert not gd.guards_intact(parent)


def test_a_write_inside_the_payload_is_not_a_guard_violation_but_changes_a_const_input():
    a = np.arange(12, dtype=np.float32).reshape(3, 4)
    view, parent = gd.from_array(a, "cpu", guard_bytes=512)
    assert np.array_equal(view.numpy(), a) and view.is_contiguous() and view.dtype == torch.float32
    off, n = gd.span(parent)
    snap = gd.snapshot(parent)
    assert gd.unchanged(parent, snap)
    parent[off] ^= 0xFF                   # first byte of the payload
    parent[off + n - 1] ^= 0xFF           # last byte of the payload
    assert gd.guards_intact(parent)
    assert not gd.unchanged(parent, snap)
    view[1, 2] = 99.0                      # through the view: the same memory
    assert gd.guards_intact(parent) and parent[off:off + n].view(torch.float32)[6] == 99.0


def test_from_array_keeps_dtype_and_bits():
    for a in (np.array([1, 0, 255], np.uint8), np.array([[-1, 7]], np.int32), np.array([np.nan, -0.0, 1e-40], np.float32),
              np.array([2.5], np.float64)):
        view, parent = gd.from_array(a, "cpu", guard_bytes=256)
        assert np.array_equal(gd.bits(view), a.view(gd.bits(view).dtype)) and tuple(view.shape) == a.shape
        assert gd.guards_intact(parent)


def test_bits_tells_nan_payloads_apart():
    a = torch.tensor(np.array([0x7FC00000, 0x7FC00001, 0xFFFFFFFF], np.uint32).view(np.float32))
    assert gd.bits(a).tolist() == [0x7FC00000, 0x7FC00001, 0xFFFFFFFF]
