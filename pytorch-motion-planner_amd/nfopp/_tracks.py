"""What the entries on timed tracks share on the host side (conflicts.py, schedule.py, time_profile.py): the layout check of a
tracks tensor, its device pointer, the device check of a call, and one value per row."""
import numpy as np
import torch

from . import _lib


def check_tracks(t, name):
    """[B, K, >= 2] fp32 with K >= 1 whose last two dimensions are contiguous and whose tracks follow each other without a
    gap: what the kernel indexes by.  -> (B, K, row stride in floats)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a tensor" % name)
    if t.dim() != 3 or t.shape[1] < 1 or t.shape[2] < 2:
        raise ValueError("%s must be [B, K, >= 2] with K >= 1, got %s" % (name, tuple(t.shape)))
    if t.dtype != torch.float32:
        raise ValueError("%s must be float32, got %s" % (name, t.dtype))
    b, k, _ = t.shape
    sb, sk, sx = t.stride()
    row = sk if k > 1 else (sb if b > 1 else t.shape[2])      # the stride of a dimension of size 1 says nothing
    if b > 0 and (sx != 1 or row < 2 or (k > 1 and b > 1 and sb != k * sk)):
        raise ValueError("%s must be laid out as rows of x, y, ... that follow each other (strides (K * S, S, 1) with S >= 2), "
                         "got strides %s for shape %s" % (name, tuple(t.stride()), tuple(t.shape)))
    return b, k, int(row)


def hip_device(caller, name, tracks, other_name=None, other=None):
    """The device of a call on `tracks` and, when given, `other`: both HIP tensors on one device."""
    if not tracks.is_cuda or (other is not None and not other.is_cuda):
        raise _lib.NfoppError("%s needs HIP tensors (there is no CPU path)" % caller)
    if other is not None and other.device != tracks.device:
        raise _lib.NfoppError("%s is on %s, %s on %s" % (other_name, other.device, name, tracks.device))
    return tracks.device


def raw_ptr(t):
    """Device pointer of a tracks tensor that `check_tracks` and `hip_device` accepted (it may be a strided view, which
    `_lib.ptr` refuses)."""
    dev = _lib._current_device()
    if t.device.index != dev:
        _lib.require_current_device(t.device.index, dev)
    return t.data_ptr() or None


def per_row(v, batch, device, name):
    """None, a number, an array or a tensor -> None or a [B] fp32 device tensor (a tensor is not copied to the host).  `name`
    is what the value is called in the error: a radius, a speed."""
    if v is None:
        return None
    if isinstance(v, torch.Tensor):
        v = v.to(device=device, dtype=torch.float32).reshape(-1)
    else:
        v = torch.from_numpy(np.array(v, np.float32).reshape(-1)).to(device)
    if v.numel() not in (1, batch):
        raise ValueError("%s must be a number or [B] = [%d], got %d values" % (name, batch, v.numel()))
    return v.expand(batch).contiguous()
