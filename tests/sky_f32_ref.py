"""CPU restatements of what the fp32 sky kernel computes (csrc/sky_f32.hip), shared by tests/test_sky_f32_cpu.py and
tests/test_sky_f32_gpu.py: the k-ordered fmaf chain of every layer, the order in which the frame mean is added, the bound that
order is held to, and the sky-mode resolution table.

v_mfma_f32_32x32x2_f32 is bit for bit a k-ordered fmaf chain.  `chain_linear` restates such a chain as
acc = fl32(fl64(acc) + fl64(w) * fl64(x)) -- the product of two f32 values is exact in f64, so one step differs from fmaf only by
the double rounding of the sum (tests/cnn_f32_ref.py)."""
import numpy as np
import torch

U = 2.0 ** -24      # unit roundoff of f32


def chain_linear(x, W, bias):
    """x f32 [n,K], W f32 [O,K], bias f32 [O] -> f32 [n,O]: one chain over k = 0 .. K - 1 from zero, then + bias in f32."""
    x = np.asarray(x, dtype=np.float32)
    W = np.asarray(W, dtype=np.float32)
    acc = np.zeros((x.shape[0], W.shape[0]), np.float32)
    x64, w64 = x.astype(np.float64), W.astype(np.float64)
    for k in range(x.shape[1]):
        acc = (acc.astype(np.float64) + x64[:, k][:, None] * w64[:, k][None, :]).astype(np.float32)
    return acc + np.asarray(bias, dtype=np.float32)[None, :]


def _lrelu(v):
    return np.where(v > 0, v, np.float32(0.2) * v).astype(np.float32)        # x > 0 ? x : 0.2f * x


def chain_sky_mlp(fold, pe):
    """SKYMLP.forward on encoded rows pe f32 [n,33] with every layer a k-ordered chain; fold = oracle/split_ref.py fold_sky_mlp
    (f32): w1, b1 (fc1.bias + fc_z_a(z)), hidden, bias, wc, bc.  Returns f32 [n,64]."""
    n = lambda t: np.asarray(t, dtype=np.float32)
    a = _lrelu(chain_linear(n(pe), n(fold["w1"]), n(fold["b1"])))
    for W, b in zip(fold["hidden"], fold["bias"]):
        a = _lrelu(chain_linear(a, n(W), n(b)))
    return torch.from_numpy(chain_linear(a, n(fold["wc"]), n(fold["bc"])))


def tree_mean(sky_c):
    """The kernel's frame mean of sky_c f32 [n,64]: every 32-ray tile (the last one padded with zeros) added in f32 as a depth-5
    tree of neighbours, the tiles' sums added in f64, one division and one rounding to f32.  Returns f32 [64]."""
    v = np.asarray(sky_c, dtype=np.float32)
    n = v.shape[0]
    pad = (-n) % 32
    if pad:
        v = np.concatenate([v, np.zeros((pad, v.shape[1]), np.float32)])
    t = v.reshape(-1, 32, v.shape[1])
    for _ in range(5):
        t = t[:, 0::2] + t[:, 1::2]           # f32 + f32, rounded once
        assert t.dtype == np.float32
    return torch.from_numpy((t[:, 0].astype(np.float64).sum(axis=0) / n).astype(np.float32))


def mean_bound(sky_c):
    """Per feature: a depth-5 f32 tree, then f64, then one rounding errs by at most 5 u mean|x| + u |mean|; 8 u mean|x| covers the
    second-order terms.  f64 [64]."""
    return 8 * U * torch.as_tensor(sky_c).double().abs().mean(dim=0)


def check_mean(avg, sky_c):
    """|avg - f64 mean of sky_c| <= mean_bound(sky_c), per feature; returns the largest ratio."""
    c = torch.as_tensor(sky_c).double()
    err = (torch.as_tensor(avg).double().reshape(-1) - c.mean(dim=0)).abs()
    bound = mean_bound(c)
    assert bool((err <= bound).all()), (float((err / bound).max()), int((err > bound).sum()))
    return float((err / bound).max())


def resolution_rows():
    """The sky-mode resolution table: (path taken, Renderer.exact_sky resolved) -> the sky MLP that runs."""
    return (
        # the defaults: nothing set
        ("fused", "torch", "fused"),
        ("exact", "torch", "torch"),
        ("unfused", "torch", "torch"),
        # exact_sky decides on the exact path only, asked for directly or adopted through Renderer.fallback = "exact"
        ("exact", "f32", "f32"),
        ("fused", "f32", "fused"),
        ("unfused", "f32", "torch"),
    )
