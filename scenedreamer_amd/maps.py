"""Depth and opacity maps of a frame (csrc/maps.hip through sdn_depth_maps / sdn_depth_quantise): the tail of the reference's
second inference loop, Generator.inference_givenstyle_depth (imaginaire/generators/scenedreamer.py:636-851), on the two per-sample
arrays the field kernels already deliver through the aux protocol (fused.field_render / fused.field_exact, aux={}): the compositing of
:816, the crop of :821-823, the normalisation over the pixels that hit something of :835-841 and the 8-bit values of :844.

All arithmetic is specified to the bit: tests/depth_maps_ref.py restates it in numpy and tests/test_depth_maps_gpu.py compares with ==.
Everything runs on the current stream and nothing synchronises with the host.  There is no CPU substitute: without the library every
call raises."""
import numpy as np
import torch

from . import capi

NO_HIT = (0x7F800000, 0)      # the range pair of a frame in which no pixel hit anything


def _check(t, name, dtype):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise RuntimeError(f"{name} must be a contiguous CUDA {dtype} tensor")


def depth_maps(weights, sample_depth, rows, cols, crop=0, opacity=True, n_workgroups=0):
    """weights, sample_depth: f32 [rows*cols, ns] in the window's row-major ray order (the aux arrays "weights" and "depth").
    Returns (depth f32 [H,W], opacity f32 [H,W] or None, range int32[2]) with H, W = rows - 2 crop, cols - 2 crop:
    depth = the products w[s] * z[s] accumulated in f64 for s ascending, rounded to f32 once; opacity = the same sum of w[s];
    range = the f32 BIT PATTERNS (uint32 values in an int32 tensor, which is how PyTorch can hold them) of the smallest and the largest
    depth that is > 0 and finite, (0x7F800000, 0) = NO_HIT when there is none."""
    _check(weights, "weights", torch.float32)
    _check(sample_depth, "sample_depth", torch.float32)
    rows, cols, crop = int(rows), int(cols), int(crop)
    if weights.dim() != 2 or weights.shape != sample_depth.shape or weights.device != sample_depth.device or weights.shape[0] != rows * cols:
        raise RuntimeError(f"weights and sample_depth must both be [{rows * cols}, ns] on one device, got {tuple(weights.shape)} and "
                           f"{tuple(sample_depth.shape)}")
    if crop < 0 or 2 * crop >= rows or 2 * crop >= cols:
        raise RuntimeError(f"a crop of {crop} leaves nothing of {rows} x {cols}")
    H, W = rows - 2 * crop, cols - 2 * crop
    dev = weights.device
    depth = torch.empty((H, W), dtype=torch.float32, device=dev)
    opac = torch.empty((H, W), dtype=torch.float32, device=dev) if opacity else None
    rng = torch.empty(2, dtype=torch.int32, device=dev)          # (initialised by the entry itself)
    with torch.cuda.device(dev):
        rc = capi.lib().sdn_depth_maps(weights.data_ptr(), sample_depth.data_ptr(), rows, cols, int(weights.shape[1]), crop, depth.data_ptr(),
                                       opac.data_ptr() if opac is not None else None, rng.data_ptr(), int(n_workgroups), capi.current_stream(dev))
    capi.check(rc, "sdn_depth_maps")
    return depth, opac, rng


def quantise(depth, rng, bits=8, n_workgroups=0):
    """depth f32 [...], rng int32[2] (the pair of depth_maps, or metric_range) -> uint8 (bits = 8) or uint16 (bits = 16) of depth's
    shape: rint((d - lo) / (hi - lo) * (2^bits - 1)) clamped, 0 when hi == lo, 2^bits - 1 where d is not a positive finite number.
    With depth_maps' own pair and bits = 8 these are the pixels of the reference's depth/%05d.png."""
    _check(depth, "depth", torch.float32)
    _check(rng, "rng", torch.int32)
    if rng.numel() != 2 or rng.device != depth.device:
        raise RuntimeError("rng must hold two 32-bit elements on depth's device")
    if bits not in (8, 16):
        raise RuntimeError(f"bits must be 8 or 16, got {bits!r}")
    out = torch.empty(depth.shape, dtype=torch.uint8 if bits == 8 else torch.uint16, device=depth.device)
    with torch.cuda.device(depth.device):
        rc = capi.lib().sdn_depth_quantise(depth.data_ptr(), depth.numel(), rng.data_ptr(), int(bits), out.data_ptr(), int(n_workgroups),
                                           capi.current_stream(depth.device))
    capi.check(rc, "sdn_depth_quantise")
    return out


def metric_range(depth_max, device):
    """The pair (0, depth_max) for `quantise`: a depth in world units that is comparable across frames, which the reference's
    per-frame normalisation is not.  Depths beyond depth_max are clamped to it."""
    depth_max = np.float32(depth_max)
    if not (np.isfinite(depth_max) and depth_max > 0):
        raise ValueError(f"depth_max must be a positive finite number, got {depth_max!r}")
    return torch.from_numpy(np.array([0.0, depth_max], np.float32).view(np.int32)).to(device)


def range_values(rng):
    """The pair as floats (lo, hi), or None for NO_HIT.  Synchronises: a convenience for tests and tools."""
    lo, hi = (int(v) & 0xFFFFFFFF for v in rng.cpu().tolist())
    if hi == 0:
        return None
    return tuple(float(v) for v in np.array([lo, hi], np.uint32).view(np.float32))
