"""CPU restatement of the fixed orders of csrc/world_f32.hip (the world encoder and the style MLP), shared by
tests/test_world_f32_cpu.py and tests/test_world_f32_gpu.py, with the library references they are measured against.

v_mfma_f32_32x32x2_f32 is bit for bit a k-ordered fmaf chain; a chain step is restated as acc = fl32(fl64(acc) + fl64(w) * fl64(x))
(the product of two f32 values is exact in f64, so a step differs from fmaf only by the double rounding of the sum).
  conv / head layers: per tap one chain from zero over the input channels in ascending order; the nine tap sums added in f32 in
                      the order ky, kx to a total that starts at zero; the head adds its bias in f32 after that.
  tail:               per channel the rows added in row order in f64, / P in f64, rounded to f32; fc1 / fc2 accumulate in f64 in k
                      order, are rounded to f32 and get their bias in f32; LeakyReLU; tanh in f64, rounded to f32.
  style MLP:          sum of squares in f64 in k order, sqrt rounded to f32, max(., 1e-12), an f32 division; every output
                      accumulated in f64 in k order, + bias in f64, rounded to f32 once, LeakyReLU in f32.
Activations are NCHW tensors here; `rows` / `nchw` convert to and from the kernels' channels-last rows."""
import numpy as np
import torch
import torch.nn.functional as F

PAIRS = tuple((c, c * s, s) for c in (16, 32, 64, 128, 256) for s in (1, 2))       # (cin, cout, stride): the five SRTConvBlocks
CONV_NAMES = tuple(f"conv_blocks.{i}.layers.{k}" for i in range(5) for k in (0, 2))
LAYER_NAMES = ("head",) + CONV_NAMES
YARD_HW = (70, 52)      # spatial sizes 35x26 -> 18x13 -> 9x7 -> 5x4 -> 3x2 -> 2x1: every layer has >= 1024 output values


def T(w, name, dtype=torch.float32):
    return torch.as_tensor(np.asarray(w["world_encoder." + name]), dtype=dtype)


def half(v):
    return (v - 1) // 2 + 1


def rows(x):
    """NCHW [1,C,H,W] -> channels-last rows [H*W, C]."""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def nchw(r, hw):
    return r.reshape(1, hw[0], hw[1], -1).permute(0, 3, 1, 2).contiguous()


# --------------------------------------------------------------------------- inputs

def maps(hw, seed=0):
    """height f32 [1,1,H,W] uniform in [0,1), semantic f32 [1,11,H,W] one-hot of uniform random classes."""
    rng = np.random.default_rng(1201 + seed)
    h = rng.random((1, 1) + tuple(hw)).astype(np.float32)
    cls = rng.integers(0, 11, size=tuple(hw))
    s = np.zeros((1, 11) + tuple(hw), np.float32)
    np.put_along_axis(s[0], cls[None], 1.0, axis=0)
    return torch.from_numpy(h), torch.from_numpy(s)


def styles(seeds):
    """style codes f32 [len(seeds),128], standard normal, one generator per seed."""
    return torch.from_numpy(np.stack([np.random.default_rng(1301 + s).standard_normal(128).astype(np.float32) for s in seeds]))


# --------------------------------------------------------------------------- the restated orders

def chain_conv(x, w, stride=1, bias=None):
    """The kernel's order: x f32 [1,C,H,W], w f32 [O,C,3,3], zero padding 1 -> f32 [1,O,Ho,Wo] (before any activation)."""
    x = np.asarray(x, dtype=np.float32)
    w = np.asarray(w, dtype=np.float32)
    _, C, H, W = x.shape
    O = w.shape[0]
    Ho, Wo = (half(H), half(W)) if stride == 2 else (H, W)
    xp = np.zeros((C, H + 2, W + 2), np.float32)
    xp[:, 1:1 + H, 1:1 + W] = x[0]
    # taps [9, C, P] and weights [9, C, O] in f64; the nine chains advance together, one input channel per step
    xs = np.stack([xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride].reshape(C, Ho * Wo)
                   for ky in range(3) for kx in range(3)]).astype(np.float64)
    wt = np.stack([w[:, :, ky, kx].T for ky in range(3) for kx in range(3)]).astype(np.float64)
    acc = np.zeros((9, Ho * Wo, O), np.float32)
    for c in range(C):
        acc = (acc.astype(np.float64) + xs[:, c, :, None] * wt[:, c, None, :]).astype(np.float32)
    total = np.zeros((Ho * Wo, O), np.float32)
    for t in range(9):
        total = total + acc[t]            # f32 + f32, rounded once
    if bias is not None:
        total = total + np.asarray(bias, np.float32)[None, :]
    return torch.from_numpy(np.ascontiguousarray(total.T.reshape(1, O, Ho, Wo)))


def lrelu32(x):
    return torch.where(x > 0, x, x * np.float32(0.2))


def chain_layer(w, name, x, sem=None):
    """One layer in the kernel's order, activation included.  "head": x = height map, sem = semantic map -> [1,16,Ho,Wo]."""
    if name == "head":
        h = chain_conv(x, T(w, "hconv_head.weight"), 2, T(w, "hconv_head.bias"))
        s = chain_conv(sem, T(w, "sconv_head.weight"), 2, T(w, "sconv_head.bias"))
        return lrelu32(torch.cat([h, s], dim=1))
    stride = PAIRS[CONV_NAMES.index(name)][2]
    return torch.relu(chain_conv(x, T(w, name + ".weight"), stride))


def lib_layer(w, name, x, sem=None, dtype=torch.float64):
    """The same layer by F.conv2d in `dtype` (the reference's own arithmetic: fp64 = the truth, fp32 = the yardstick E32)."""
    act = lambda v: F.leaky_relu(v, 0.2)
    if name == "head":
        h = act(F.conv2d(x.to(dtype), T(w, "hconv_head.weight", dtype), T(w, "hconv_head.bias", dtype), stride=2, padding=1))
        s = act(F.conv2d(sem.to(dtype), T(w, "sconv_head.weight", dtype), T(w, "sconv_head.bias", dtype), stride=2, padding=1))
        return torch.cat([h, s], dim=1)
    stride = PAIRS[CONV_NAMES.index(name)][2]
    return act(F.relu(F.conv2d(x.to(dtype), T(w, name + ".weight", dtype), None, stride=stride, padding=1)))


def lib_tail(w, last, dtype=torch.float64):
    """layers.py:51-54 on the last layer's NCHW output (or rows [P,512] / [B,P,512]): (pooled [..,512], global_enc [..,2])."""
    x = last.to(dtype)
    if x.dim() == 4:
        x = x.permute(0, 2, 3, 1).reshape(x.shape[0], -1, x.shape[1])
    elif x.dim() == 2:
        x = x[None]
    pooled = torch.mean(x, dim=1)
    cond = F.leaky_relu(F.linear(pooled, T(w, "fc1.weight", dtype), T(w, "fc1.bias", dtype)), 0.2)
    return pooled, torch.tanh(F.linear(cond, T(w, "fc2.weight", dtype), T(w, "fc2.bias", dtype)))


def lib_encode(w, hm, sm, dtype=torch.float64):
    """The whole network by the library in `dtype`: {layer name: NCHW activation, "pooled": [1,512], "global_enc": [1,2]}."""
    out = {"head": lib_layer(w, "head", hm, sm, dtype)}
    x = out["head"]
    for name in CONV_NAMES:
        x = out[name] = lib_layer(w, name, x, dtype=dtype)
    out["pooled"], out["global_enc"] = lib_tail(w, x, dtype)
    return out


def lib_style(w, style, dtype=torch.float64):
    """StyleMLP.forward (gancraft_base.py:113-126) by F.normalize / F.linear in `dtype`: style [n,128] -> z [n,256]."""
    z = F.normalize(torch.as_tensor(np.asarray(style), dtype=dtype).reshape(-1, 128), p=2, dim=-1)
    for n in [f"style_net.fc_layers.{i}" for i in range(5)] + ["style_net.fc_out"]:
        z = F.leaky_relu(F.linear(z, torch.as_tensor(np.asarray(w[n + ".weight"]), dtype=dtype), torch.as_tensor(np.asarray(w[n + ".bias"]), dtype=dtype)), 0.2)
    return z


def chain_tail(w, r):
    """The tail kernel's order on rows f32 [P,512]: (pooled f32 [512], global_enc f32 [2])."""
    r = np.asarray(r, np.float32).astype(np.float64)
    s = np.zeros(512, np.float64)
    for p in range(r.shape[0]):
        s = s + r[p]
    pooled = (s / np.float64(r.shape[0])).astype(np.float32)

    def fc(x, wt, b):
        wt = np.asarray(wt, np.float32).astype(np.float64)
        acc = np.zeros(wt.shape[0], np.float64)
        for k in range(wt.shape[1]):
            acc = acc + wt[:, k] * np.float64(x[k])
        return acc.astype(np.float32) + np.asarray(b, np.float32)

    h = fc(pooled, T(w, "fc1.weight"), T(w, "fc1.bias"))
    h = np.where(h > 0, h, np.float32(0.2) * h).astype(np.float32)
    g = fc(h, T(w, "fc2.weight"), T(w, "fc2.bias"))
    return torch.from_numpy(pooled), torch.from_numpy(np.tanh(g.astype(np.float64)).astype(np.float32))


def chain_encode(w, hm, sm):
    """The whole network in the kernels' orders (CPU, slow at the deep layers: use small maps)."""
    out = {"head": chain_layer(w, "head", hm, sm)}
    x = out["head"]
    for name in CONV_NAMES:
        x = out[name] = chain_layer(w, name, x)
    out["pooled"], out["global_enc"] = chain_tail(w, rows(x))
    return out


def style_ref(w, style):
    """The style kernel's order: style f32 [n,128] -> z f32 [n,256]."""
    s = np.asarray(style, np.float32).reshape(-1, 128)
    ss = np.zeros(s.shape[0], np.float64)
    for k in range(128):
        ss = ss + s[:, k].astype(np.float64) ** 2
    denom = np.maximum(np.sqrt(ss).astype(np.float32), np.float32(1e-12))
    x = (s / denom[:, None]).astype(np.float32)
    for n in [f"style_net.fc_layers.{i}" for i in range(5)] + ["style_net.fc_out"]:
        wt = np.asarray(w[n + ".weight"], np.float32).astype(np.float64)
        b = np.asarray(w[n + ".bias"], np.float32).astype(np.float64)
        acc = np.zeros((x.shape[0], wt.shape[0]), np.float64)
        for k in range(wt.shape[1]):
            acc = acc + x[:, k, None].astype(np.float64) * wt[None, :, k]
        y = (acc + b[None, :]).astype(np.float32)
        x = np.where(y > 0, y, np.float32(0.2) * y).astype(np.float32)
    return torch.from_numpy(x)


# --------------------------------------------------------------------------- the knobs

def resolution_rows():
    """(attribute, environment variable's value or None) -> what runs; the same table for exact_world and exact_style."""
    return (
        (None, None, "torch"),          # the default
        ("f32", None, "f32"),
        ("torch", None, "torch"),
        (None, "f32", "f32"),           # the environment supplies it when the attribute is unset
        (None, "torch", "torch"),
        ("torch", "f32", "torch"),      # the attribute wins
        ("f32", "torch", "f32"),
    )
