"""CPU emulation of the accumulation the fp32 MFMA convolution performs (csrc/cnn_f32.hip), shared by tests/test_cnn_f32_cpu.py
and tests/test_cnn_f32_gpu.py.

v_mfma_f32_32x32x2_f32 is bit for bit a k-ordered fmaf chain.  `chain_conv` restates such a chain as
acc = fl32(fl64(acc) + fl64(x) * fl64(w)) -- the product of two f32 values is exact in f64, so one step differs from fmaf only by
the double rounding of the sum -- over the products of a convolution in tap-major order (ky, kx, then the input channels), cut
into segments of `segment` products: every segment starts from zero and the segments' partial sums are added in f32, in order."""
import numpy as np
import torch


def chain_conv(x, w, segment):
    """x f32 [1,C,H,W], w f32 [O,C,k,k] (k = 1 or 3, zero padding k // 2) -> f32 [1,O,H,W]."""
    x = np.asarray(x, dtype=np.float32)
    w = np.asarray(w, dtype=np.float32)
    _, C, H, W = x.shape
    O, _, k, _ = w.shape
    pad = k // 2
    xp = np.zeros((C, H + 2 * pad, W + 2 * pad), np.float32)
    xp[:, pad:pad + H, pad:pad + W] = x[0]
    total = np.zeros((H * W, O), np.float32)
    acc = np.zeros((H * W, O), np.float32)
    n = 0
    for ky in range(k):
        for kx in range(k):
            xs = xp[:, ky:ky + H, kx:kx + W].reshape(C, H * W).astype(np.float64)       # [C, P]
            wt = w[:, :, ky, kx].astype(np.float64)                                      # [O, C]
            for c in range(C):
                acc = (acc.astype(np.float64) + xs[c][:, None] * wt[:, c][None, :]).astype(np.float32)
                n += 1
                if n % segment == 0:
                    total = total + acc         # f32 + f32, rounded once
                    acc = np.zeros_like(acc)
    if n % segment:
        total = total + acc
    return torch.from_numpy(np.ascontiguousarray(total.T.reshape(1, O, H, W)))


def resolution_rows():
    """The cnn_mode resolution table: (path taken, Renderer.exact_cnn resolved, explicit cnn_mode) -> the CNN that runs."""
    return (
        # the defaults: nothing set
        ("fused", "torch", None, "mfma"),
        ("exact", "torch", None, "torch"),
        ("unfused", "torch", None, "torch"),
        # exact_cnn decides on the exact path only, asked for directly or adopted through Renderer.fallback = "exact"
        ("exact", "f32", None, "f32"),
        ("fused", "f32", None, "mfma"),
        ("unfused", "f32", None, "torch"),
        # an explicit cnn_mode wins on every path
        ("exact", "torch", "f32", "f32"),
        ("exact", "f32", "torch", "torch"),
        ("exact", "f32", "mfma", "mfma"),
        ("fused", "torch", "f32", "f32"),
        ("fused", "f32", "torch", "torch"),
        ("unfused", "torch", "f32", "f32"),
        ("unfused", "f32", "mfma", "mfma"),
    )
