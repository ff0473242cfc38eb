"""CPU emulation of the f16-split MFMA arithmetic (TEST INFRASTRUCTURE ONLY; plain torch on the CPU, no GPU calls).

Every product W.X of the render MLP, the sky MLP and the render CNN is evaluated on the GPU as a sum of f16 x f16 MFMA
terms with f32 accumulation:  hh = Whi.Xhi,  lh = Wlo.Xhi,  hl = Whi.Xlo  (lo = f16(x - hi)).  f16 x f16 products are
exact in f32, so fp32 matmuls of the split operands reproduce the kernels' products; only the ORDER of the f32 additions
differs (the tests allow a factor 4 for it, the allowance tests/test_exact_rung_gpu.py uses).

Two layers of functions:

  split / mm / conv / T3, LH, HL, T1     the term emulation itself (tools/precision_study.py imports these; `ROUND` is that
                                         study's switch and keeps its default, round-toward-zero).
  render_mlp / sky_mlp / render_cnn / conv_layer / composite
                                         the networks as THIS PROJECT'S KERNELS evaluate them, with a per-layer term set
                                         (`cfg`: layer name -> tuple of terms; None = all three everywhere).

What the network emulations match, read off the kernels (csrc/mlp_layers.h, mlp_pack.hip, field.hip, sky.hip, cnn.hip,
cnn_ends.hip), because it changes the error:
  * hi is rounded to NEAREST, for weights (the packers' `(_Float16)v`) and for activations (split8 / act_stage /
    planes_kernel / the conv epilogue: v_cvt_pk_f16_f32);
  * the register-resident chains (render MLP, sky MLP, the CNN's chained tail) carry a' = 1.5 y + |y| = LeakyReLU(y) / 0.4
    as ONE fma, and the consuming layer's packed weights are f32(W * 0.4f); the density head is an f32 dot product of a'
    with f32(fc_sigma.weight * 0.4f) -- it has no split terms, so it takes no part in the defect list;
  * the render MLP's trunk fc_1 .. fc_4, every layer of the sky MLP and every layer of the CNN's chained tail are packed
    times 2^TRUNK_SHIFT (so that the lo halves of the weights leave f16's subnormal range) and the factor is taken out again
    in the bias fma y = acc * 2^-shift + b; the render MLP's fc_5, fc_6, fc_out_c and conv_kernel's weights carry no shift;
  * the render MLP's output layer fc_out_c seeds the accumulator with the bias;
  * the render CNN's activations travel as f16 hi / lo planes: a stored activation IS hi + lo (2^-22 relative), and a
    residual read back from planes is f32(hi) + f32(lo); conv_kernel's own LeakyReLU is max(v, 0.2 v), its fused conv4
    projection an f32 dot product (no split); the chained tail (`chain=True`) evaluates conv4 as a 3-term layer;
  * compositing (`composite`): volum_rendering_relu, the sky-only mask, the sky blend, clamp and sum, in the dtype of its
    arguments throughout (oracle/field_ref.py's volum_rendering_relu holds a `.float()`, so its fp64 evaluation is not fp64).
Deliberately NOT matched: the order of the f32 additions inside the MFMA and across k-steps / terms; fma contraction of
the FiLM and residual adds in the conv epilogue; the kernels' fast exponential (__expf) and tanhf / sinf / cosf
implementations; block-scaled fp6 terms (colour_terms = 6, hidden_terms = 6) and the 1-term CNN rungs, whose loss is
intentional.
"""
import numpy as np
import torch
import torch.nn.functional as F

from . import field_ref as FR

ROUND = {"x": "rtz", "w": "rtz"}     # tools/precision_study.py's switch: rtz (v_cvt_pkrtz_f16_f32) or rtn (v_cvt_pk_f16_f32)

ACT_SCALE = np.float32(0.4)          # mlp_layers.h ACT_SCALE
TRUNK_SHIFT = 8                      # mlp_layers.h SDN_TRUNK_SHIFT (sdn_field_trunk_shift())


def split(x, mode="rtz"):
    h = x.to(torch.float16)
    if mode == "rtz":
        over = h.float().abs() > x.abs()
        hv = h.view(torch.int16)
        hv = torch.where(over, hv - 1, hv)          # sign-magnitude: one step toward zero
        h = hv.view(torch.float16)
    hi = h.float()
    lo = (x - hi).to(torch.float16).float()
    return hi, lo


def mm(x, W, terms, rx=None, rw=None):
    """x [..., K], W [N, K] -> x W^T with the given subset of split terms ('f32' = exact).  rx / rw: how hi is rounded for
    the activations / the weights (None: ROUND)."""
    if terms == "f32":
        return x @ W.t()
    xh, xl = split(x, rx or ROUND["x"])
    Wh, Wl = split(W, rw or ROUND["w"])
    y = xh @ Wh.t()
    if "lh" in terms:
        y = y + xh @ Wl.t()
    if "hl" in terms:
        y = y + xl @ Wh.t()
    if "ll" in terms:
        y = y + xl @ Wl.t()
    return y


def conv(v, W, pad, terms, rx=None, rw=None):
    """v [N,C,H,W], W [O,C,k,k] -> conv2d without bias, the products as in mm."""
    if terms == "f32":
        return F.conv2d(v, W, None, padding=pad)
    vh, vl = split(v, rx or ROUND["x"])
    Wh, Wl = split(W, rw or ROUND["w"])
    y = F.conv2d(vh, Wh, None, padding=pad)
    if "lh" in terms:
        y = y + F.conv2d(vh, Wl, None, padding=pad)
    if "hl" in terms:
        y = y + F.conv2d(vl, Wh, None, padding=pad)
    return y


T3, LH, HL, T1 = ("hh", "lh", "hl"), ("hh", "lh"), ("hh", "hl"), ("hh",)

# layers that are evaluated as split products (fc_sigma is an f32 dot product in the kernel)
MLP_LAYERS = ["fc_1", "fc_2", "fc_3", "fc_4", "fc_5", "fc_6", "fc_out_c"]
MLP_FEEDS = {"sigma": ["fc_1", "fc_2", "fc_3", "fc_4"], "colour": MLP_LAYERS}
SKY_LAYERS = ["fc1", "fc2", "fc3", "fc4", "fc5", "fc_out_c"]
CNN_LAYERS = ["conv1", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b", "conv4"]


def intact(layers):
    return {n: T3 for n in layers}


def single_defects(layers, feeds=None):
    """Every configuration that differs from all-3-term in exactly ONE layer by exactly ONE dropped correction term:
    yields (layer, dropped term, cfg).  feeds: restrict the defects to these layers (the ones that reach the output)."""
    for n in (feeds if feeds is not None else layers):
        for dropped, kept in (("lh", HL), ("hl", LH)):
            yield n, dropped, dict(intact(layers), **{n: kept})


def _rtn(x, W, terms):
    return mm(x, W, terms, "rtn", "rtn")


def _act(y):
    """a' = fma(y, 1.5, |y|) = LeakyReLU_0.2(y) / 0.4, one rounding (act_stage, stage 2)."""
    yd = y.double()
    return (1.5 * yd + yd.abs()).float()


# --------------------------------------------------------------------------- render MLP

def fold_render_mlp(w, z, dtype=torch.float32):
    """The per-style constants of LightningMLP as Renderer.set_style_code folds them (renderer.fold_render_net), on the CPU."""
    Tn = lambda n: FR.T(w, "render_net." + n, dtype)
    z = torch.as_tensor(np.asarray(z), dtype=dtype).reshape(1, -1)
    hidden, beta = [], []
    for i in (2, 3, 4, 5, 6):
        alpha = F.linear(z, Tn(f"fc_{i}.weight_alpha"), Tn(f"fc_{i}.bias_alpha"))
        beta.append(F.linear(z, Tn(f"fc_{i}.weight_beta"), Tn(f"fc_{i}.bias_beta"))[0])
        hidden.append(Tn(f"fc_{i}.weight") * alpha)
    return dict(w1=Tn("fc_1.weight"), label_bias=Tn("fc_m_a.weight").t() + Tn("fc_1.bias")[None, :], hidden=hidden, beta=beta,
                w_sigma=Tn("fc_sigma.weight").reshape(-1), b_sigma=Tn("fc_sigma.bias").reshape(-1)[0],
                wc=Tn("fc_out_c.weight"), bc=Tn("fc_out_c.bias"))


def render_mlp(fold, x, label, cfg=None, trunk_shift=TRUNK_SHIFT):
    """sdn_render_mlp / the MLP of sdn_field_mlp with colour_terms = 3.  fold: fold_render_mlp (f32) or the Renderer's own
    folded tensors in that layout; x f32 [n,128]; label int64 [n] -> (sigma [n], c [n,64])."""
    cfg = cfg or intact(MLP_LAYERS)
    S = np.float32(2.0 ** trunk_shift)
    k = np.float32(1.0) / S
    y = _rtn(x, fold["w1"] * S, cfg["fc_1"]) * k + fold["label_bias"][label]
    a = _act(y)
    sigma = None
    for i, (W, b) in enumerate(zip(fold["hidden"], fold["beta"])):
        Wp = W * ACT_SCALE
        if i < 3:
            y = _rtn(a, Wp * S, cfg[f"fc_{i + 2}"]) * k + b
        else:
            y = _rtn(a, Wp, cfg[f"fc_{i + 2}"]) + b
        a = _act(y)
        if i == 2:      # the density head reads fc_4's scaled activation
            sigma = a @ (fold["w_sigma"] * ACT_SCALE) + fold["b_sigma"]
    c = fold["bc"] + _rtn(a, fold["wc"] * ACT_SCALE, cfg["fc_out_c"])
    return sigma, c


def render_mlp_ref(w, x, z, label, dtype):
    """oracle/field_ref.py's LightningMLP on rows: x [n,128], z [1,256], label int64 [n] -> (sigma [n], c [n,64]) in dtype."""
    onehot = torch.zeros(x.shape[0], 12, dtype=dtype)
    onehot.scatter_(-1, label.reshape(-1, 1), 1.0)
    z = torch.as_tensor(np.asarray(z), dtype=dtype).reshape(1, -1)
    s, c = FR.render_mlp(w, x.to(dtype)[None, None, None], z, onehot[None, None, None], dtype=dtype)
    return s.reshape(-1), c.reshape(-1, 64)


# --------------------------------------------------------------------------- sky MLP

def fold_sky_mlp(w, z, dtype=torch.float32):
    Tn = lambda n: FR.T(w, "sky_net." + n, dtype)
    z = torch.as_tensor(np.asarray(z), dtype=dtype).reshape(1, -1)
    return dict(w1=Tn("fc1.weight"), b1=Tn("fc1.bias") + F.linear(z, Tn("fc_z_a.weight"))[0],
                hidden=[Tn(f"fc{i}.weight") for i in (2, 3, 4, 5)], bias=[Tn(f"fc{i}.bias") for i in (2, 3, 4, 5)],
                wc=Tn("fc_out_c.weight"), bc=Tn("fc_out_c.bias"))


def sky_mlp(fold, x, cfg=None, shift=TRUNK_SHIFT):
    """sdn_sky_mlp with hidden_terms = 3 on positional-encoded rows x f32 [n,33] -> [n,64]."""
    cfg = cfg or intact(SKY_LAYERS)
    S = np.float32(2.0 ** shift)
    k = np.float32(1.0) / S
    a = _act(_rtn(x, fold["w1"] * S, cfg["fc1"]) * k + fold["b1"])
    for i, (W, b) in enumerate(zip(fold["hidden"], fold["bias"])):
        a = _act(_rtn(a, W * ACT_SCALE * S, cfg[f"fc{i + 2}"]) * k + b)
    return _rtn(a, fold["wc"] * ACT_SCALE * S, cfg["fc_out_c"]) * k + fold["bc"]


def sky_mlp_ref(w, x, z, dtype):
    z = torch.as_tensor(np.asarray(z), dtype=dtype).reshape(1, -1)
    return FR.sky_mlp(w, x.to(dtype)[None], z, dtype)[0]


# --------------------------------------------------------------------------- render CNN

def planes(v):
    """What an activation is once it is stored as f16 hi / lo planes: hi + lo."""
    hi, lo = split(v, "rtn")
    return hi + lo


def _lrelu(v):
    return torch.maximum(v, np.float32(0.2) * v) if v.dtype == torch.float32 else F.leaky_relu(v, 0.2)


def conv_layer(x, W, terms=T3, bias=None, resid=None, mod=None, proj=None, to_planes=False):
    """One sdn_conv launch with its epilogue: LeakyReLU((resid + conv(x) + bias) * (mod_w + 1) + mod_b), then optionally
    tanh(proj_w . y + proj_b).  x [1,C,H,W]: the DECODED input planes (hi + lo), so the layer's input rounding is no part of
    its error; W [256,C,k,k]; resid [1,256,H,W] (fp32 rows, or decoded planes); mod = (mod_w [256], mod_b [256]);
    proj = (proj_w [3,256], proj_b [3]).  terms = 'f32': the same graph in x's dtype with exact products (the fp32 yardstick
    in float32, the truth in float64).  Returns y [1,256,H,W] (to_planes: as the stored hi + lo), or the image [1,3,H,W]."""
    pad = W.shape[-1] // 2
    v = conv(x, W, pad, terms, "rtn", "rtn")
    if bias is not None:
        v = v + bias[None, :, None, None]
    if resid is not None:
        v = resid + v
    if mod is not None:
        v = v * (mod[0][None, :, None, None] + 1) + mod[1][None, :, None, None]
    v = _lrelu(v)
    if proj is not None:
        return torch.tanh(F.conv2d(v, proj[0][:, :, None, None], proj[1]))
    return planes(v) if to_planes and terms != "f32" else v


def render_cnn(w, net_out, z, cfg=None, chain=True, memo=None):
    """MfmaCNN(renderer, 3): net_out [1,h,w,64] f32 -> image [1,3,h,w].  chain: the head / tail kernels of cnn_ends.hip
    (conv4 as a 3-term layer on the 0.4-scaled activation) or conv_kernel launches throughout (conv4 as conv4b's f32
    projection: cfg['conv4'] is then unused).  memo: a dict shared between calls on the SAME inputs; layers in front of the
    first non-intact one are taken from it."""
    cfg = cfg or intact(CNN_LAYERS)
    Tn = lambda n: FR.T(w, "denoiser." + n)
    bias = lambda n: Tn(n + ".bias") if f"denoiser.{n}.bias" in w else None
    zt = torch.as_tensor(np.asarray(z), dtype=torch.float32).reshape(1, -1)
    a = [c[0] for c in torch.chunk(F.linear(zt, Tn("fc_z_cond.weight"), Tn("fc_z_cond.bias")), 4, dim=-1)]
    state = {"clean": memo is not None}

    def layer(n, fn):
        clean = state["clean"] and cfg[n] == T3
        state["clean"] = clean
        if clean and (n, chain) in memo:
            return memo[(n, chain)]
        out = fn()
        if clean:
            memo[(n, chain)] = out
        return out
    x = torch.as_tensor(net_out, dtype=torch.float32).permute(0, 3, 1, 2).contiguous()
    # head: the rows are split in registers (head_kernel) or stored as planes first (planes_kernel): the same hi / lo either way
    y = layer("conv1", lambda: conv_layer(x, Tn("conv1.weight"), cfg["conv1"], bias("conv1"), to_planes=True))
    t = layer("conv2a", lambda: conv_layer(y, Tn("conv2a.weight"), cfg["conv2a"], bias("conv2a"), to_planes=True))
    y = layer("conv2b", lambda: conv_layer(t, Tn("conv2b.weight"), cfg["conv2b"], bias("conv2b"), resid=y, mod=(a[0], a[1]), to_planes=True))
    t = layer("conv3a", lambda: conv_layer(y, Tn("conv3a.weight"), cfg["conv3a"], bias("conv3a"), to_planes=True))
    y = layer("conv3b", lambda: conv_layer(t, Tn("conv3b.weight"), cfg["conv3b"], bias("conv3b"), resid=y, mod=(a[2], a[3]), to_planes=True))
    if not chain:
        t = conv_layer(y, Tn("conv4a.weight"), cfg["conv4a"], bias("conv4a"), to_planes=True)
        return conv_layer(t, Tn("conv4b.weight"), cfg["conv4b"], bias("conv4b"), resid=y,
                          proj=(Tn("conv4.weight").reshape(3, 256), Tn("conv4.bias")))
    return chain_tail(y, Tn("conv4a.weight"), bias("conv4a"), Tn("conv4b.weight"), bias("conv4b"), Tn("conv4.weight"), Tn("conv4.bias"),
                      {n: cfg[n] for n in ("conv4a", "conv4b", "conv4")})


def chain_tail(y, w4a, b4a, w4b, b4b, w4, b4, cfg=None, dtype=None, shift=TRUNK_SHIFT):
    """sdn_conv_chain: tanh(conv4(LeakyReLU(y + conv4b(LeakyReLU(conv4a(y)))))) on the decoded planes y [1,256,H,W] -> [1,3,H,W].
    dtype = torch.float32 / torch.float64: the plain graph in that type (yardstick / truth)."""
    rows = y.permute(0, 2, 3, 1).reshape(-1, 256)
    w4a, w4b, w4 = w4a.reshape(256, 256), w4b.reshape(256, 256), w4.reshape(3, 256)
    if dtype is not None:
        r = rows.to(dtype)
        t = F.leaky_relu(F.linear(r, w4a.to(dtype), b4a.to(dtype)), 0.2)
        t = F.leaky_relu(r + F.linear(t, w4b.to(dtype), b4b.to(dtype)), 0.2)
        out = torch.tanh(F.linear(t, w4.to(dtype), b4.to(dtype)))
    else:
        cfg = cfg or intact(("conv4a", "conv4b", "conv4"))
        S = np.float32(2.0 ** shift)
        k = np.float32(1.0) / S
        a = _act(_rtn(rows, w4a * S, cfg["conv4a"]) * k + b4a)
        a = _act((_rtn(a, w4b * ACT_SCALE * S, cfg["conv4b"]) * k + b4b) + rows)
        out = torch.tanh(_rtn(a, w4 * ACT_SCALE * S, cfg["conv4"]) * k + b4)
    return out.reshape(1, y.shape[2], y.shape[3], 3).permute(0, 3, 1, 2).contiguous()


def head(x_rows, w1, b1, hw, cfg=T3, dtype=None):
    """sdn_conv_head: LeakyReLU(conv1(x) + bias) for rows x [h*w,64] -> [1,256,h,w] (emulation: as the stored planes)."""
    if dtype is not None:
        y = F.leaky_relu(F.linear(x_rows.to(dtype), w1.reshape(256, 64).to(dtype), b1.to(dtype)), 0.2)
    else:
        y = planes(_lrelu(_rtn(x_rows, w1.reshape(256, 64), cfg) + b1))
    return y.reshape(1, hw[0], hw[1], 256).permute(0, 3, 1, 2).contiguous()


# --------------------------------------------------------------------------- compositing

def volum_rendering_relu(sigma, dists, dim):
    """mc_utils.py:154-161 in the dtype of its arguments (oracle/field_ref.py's follows the reference's `.float()`)."""
    free_energy = F.relu(sigma) * dists
    return (1 - torch.exp(-free_energy)) * torch.exp(-FR.cumsum_exclusive(free_energy, dim=dim))


def composite(sigma, colour, dists, sky_only, nosky, sky_c, sky_avg):
    """The compositing of Generator._forward_perpix (oracle/field_ref.py forward_perpix, scenedreamer.py:373-413) per ray, in
    the dtype of `sigma` throughout: sigma [R,ns], colour [R,ns,64], dists [R,ns] (new_dists * dists_scale), sky_only / nosky
    bool [R], sky_c [R,64], sky_avg [64] -> net_out [R,64]."""
    dt = sigma.dtype
    weights = volum_rendering_relu(sigma, dists.to(dt), dim=-1) * torch.logical_not(sky_only).to(dt)[:, None]        # :373-376
    total = weights.sum(dim=-1, keepdim=True)
    m = nosky.to(dt)[:, None]
    sky = sky_c.to(dt) * (1.0 - m) + sky_avg.to(dt).reshape(1, -1) * m   # :401
    rgbs = torch.clamp(colour, -1, 1) + 1
    rgbs_sky = torch.clamp(sky, -1, 1) + 1
    return (weights[..., None] * rgbs).sum(dim=1) + (1.0 - total) * rgbs_sky - 1
