"""Guarded device (or host) buffers: what a kernel writes OUTSIDE the array it was handed, and what it reads before writing.

A plain `torch.empty(shape)` is rounded up to 512 bytes by the caching allocator and sits between other recycled blocks: a
kernel that stores a few rows past the end of its output lands in that rounding and no comparison of the output sees it.
`guarded()` puts the array inside one larger uint8 allocation with GUARD_BYTE on both sides and a chosen byte pattern in the
payload, so that

  * a store before or behind the array changes a guard byte         -> guards_intact(parent) is False
  * a store into a `const` input changes the allocation             -> unchanged(parent, snapshot) is False
  * a load of scratch or output memory the kernel never wrote shows as a result that differs between two fills
    (0x00 and 0xFF: NaN as a float, -1 as an integer), and an element the kernel leaves alone still holds its fill.

The payload starts at a multiple of 256 bytes inside the allocation (torch's allocations are at least as aligned on the
device), so the kernel sees the alignment it would get from torch: only the surroundings change.

Guard size.  The default of 256 KiB per side is above the largest block ONE workgroup of this library stores: a 256-sample
chunk of the fit's workspace, 256 rows of 112 floats (112 KiB) for h1 and rho*dh1 and of 16 * 14 floats (224 KiB) for
rho*de at F = 220 (csrc/onf_x32_impl.h, csrc/onf_wgrad.hip); an ONF output tile is 256 rows of 4 floats.  A workgroup that
runs a whole tile past its array therefore still lands inside the guard.
"""
import numpy as np
import torch

GUARD_BYTE = 0xA5
ALIGN = 256


def _round_up(n, m):
    return (n + m - 1) // m * m


def guarded(shape, dtype, device, fill_byte, guard_bytes=256 * 1024):
    """(view, parent): `view` is a contiguous tensor of `shape` / `dtype` whose bytes are all `fill_byte`, inside the uint8
    allocation `parent`, with at least `guard_bytes` of GUARD_BYTE in front of it and behind it."""
    if isinstance(shape, int):
        shape = (shape,)
    shape = tuple(int(s) for s in shape)
    itemsize = torch.empty(0, dtype=dtype).element_size()
    nbytes = itemsize * int(np.prod(shape, dtype=np.int64))
    front = _round_up(max(int(guard_bytes), 1), ALIGN)
    parent = torch.full((front + nbytes + int(guard_bytes),), GUARD_BYTE, dtype=torch.uint8, device=device)
    payload = parent[front:front + nbytes]
    payload.fill_(int(fill_byte))
    view = payload.view(dtype).view(shape)
    assert view.is_contiguous() and view.dtype == dtype and tuple(view.shape) == shape
    parent._guard_span = (front, nbytes)
    return view, parent


def from_array(a, device, guard_bytes=256 * 1024):
    """(view, parent) with the payload holding the numpy array (or tensor) `a`: for inputs and in/out state."""
    t = torch.from_numpy(np.array(a, order="C")) if isinstance(a, np.ndarray) else torch.as_tensor(a)   # np.array copies: a
    # read-only array (a cached case) is fine
    view, parent = guarded(tuple(t.shape), t.dtype, device, 0, guard_bytes)
    view.copy_(t)
    return view, parent


def span(parent):
    """(offset, size) in bytes of the payload inside `parent`."""
    return parent._guard_span


def guards_intact(parent):
    """True iff every byte in front of and behind the payload still holds GUARD_BYTE."""
    off, n = parent._guard_span
    return bool((parent[:off] == GUARD_BYTE).all()) and bool((parent[off + n:] == GUARD_BYTE).all())


def snapshot(parent):
    """A copy of the whole allocation, taken before the call, for unchanged()."""
    return parent.clone()


def unchanged(parent, snap):
    """True iff the whole allocation (guards and payload) equals its snapshot byte for byte: a `const` input."""
    return torch.equal(parent, snap)


def bits(t):
    """The elements of a tensor as a numpy array of unsigned integers of the same width (NaN payloads compare like numbers)."""
    a = t.detach().cpu().contiguous().numpy()
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
