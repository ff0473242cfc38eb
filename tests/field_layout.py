"""Shared by the arithmetic tests (tests/test_split_ref_cpu.py, tests/test_arithmetic_gpu.py, tests/test_encode_edges_gpu.py)
and tests/test_fused_gpu.py: the MFMA kernels' operand layouts decoded on the host, the fixed inputs of the arithmetic tests and
the rules they apply (check / check_fp32: 4 x E3, 4 x E32) -- one place, so that the CPU test that qualifies the yardstick
and the GPU tests that apply it cannot drift apart."""
import json
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# --------------------------------------------------------------------------- operand layouts

def decode_encode_buffers(buf, n_rays, ns):
    """The buffers sdn_field_encode wrote (fused.encode), un-permuted: feat f32 [n_rays, S, 16, 8] (hi + lo of the MLP's B
    fragments: the value to 2^-22), dist f32 [n_rays, S], label u8 [n_rays, S], with S = 4 * ceil(ns / 4) sample SLOTS -- the
    slots past `ns` are the padding of the last 4-sample pass.
    Layout: tile = 8 rays, pass = 4 samples; lane = h * 32 + 4 * ray_in_tile + sample_in_pass holds, in k-step s, the 8
    channels of level 2 s + h."""
    nch = (ns + 3) // 4
    ntile = (n_rays + 7) // 8
    fh = buf["feat"].cpu().numpy().view(np.float16)[:ntile * nch * 8 * 64 * 16].reshape(ntile, nch, 8, 64, 2, 8).astype(np.float32)
    feat = fh[..., 0, :] + fh[..., 1, :]                                   # [tile, pass, s, lane, 8]
    feat = feat.reshape(ntile, nch, 8, 2, 8, 4, 8)                         # [tile, pass, s, h, ray, sample, c]
    feat = feat.transpose(0, 4, 1, 5, 2, 3, 6).reshape(ntile * 8, nch * 4, 16, 8)
    per = lambda t: t.cpu().numpy()[:ntile * nch * 32].reshape(ntile, nch, 8, 4).transpose(0, 2, 1, 3).reshape(ntile * 8, nch * 4)
    return np.ascontiguousarray(feat[:n_rays]), np.ascontiguousarray(per(buf["dist"])[:n_rays]), np.ascontiguousarray(per(buf["label"])[:n_rays])


def plane_index(H, W, Hb, Wb):
    """Flat pixel index of frame pixel (y, x) inside a padded Hb x Wb plane: (y + 1, x + 1)."""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return ((yy + 1) * Wb + (xx + 1)).reshape(-1)


def decode_planes(hi, lo, H, W, Hb, Wb, C=256):
    """f16 planes [C/16 chunks][Hb*Wb][16] (torch tensors, any device; lo may be None) -> (hi, lo) f32 [H*W, C] rows of the
    frame, and whether every border / out-of-frame pixel of the given planes is zero."""
    idx = plane_index(H, W, Hb, Wb)
    outside = np.ones(Hb * Wb, bool)
    outside[idx] = False
    rows, clean = [], True
    for p in (hi, lo):
        if p is None:
            rows.append(None)
            continue
        a = p.cpu().numpy().view(np.float16)[:(C // 16) * Hb * Wb * 16].reshape(C // 16, Hb * Wb, 16)
        clean = clean and not a[:, outside].any()
        rows.append(np.ascontiguousarray(a[:, idx].transpose(1, 0, 2).reshape(H * W, C).astype(np.float32)))
    return rows[0], rows[1], clean


# --------------------------------------------------------------------------- fixed inputs

def style_code():
    """The intermediate style code z [1,256] of the goldens."""
    return np.load(os.path.join(GOLDEN, "style_globalenc.npz"))["z"].astype(np.float32)


MLP_ROWS = (1537, 33, 1)      # 1537: the last 32-row group and the last 256-row block are ragged


def mlp_rows(n=1537):
    """x f32 [n,128] with |x| <= 0.3 and labels int64 [n] in which all 12 classes occur (n >= 12)."""
    rng = np.random.default_rng(1101)
    x = rng.uniform(-0.3, 0.3, size=(1537, 128)).astype(np.float32)
    lab = rng.permutation(1537) % 12
    return torch.from_numpy(x[:n].copy()), torch.from_numpy(lab[:n].astype(np.int64))


def sky_dirs(n=1001):
    """Unit ray directions f32 [n,3]."""
    rng = np.random.default_rng(1102)
    d = rng.normal(size=(n, 3))
    return torch.from_numpy((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32))


CNN_HW = (21, 37)


def cnn_net_out(hw=CNN_HW):
    """A net_out-like tensor f32 [1,h,w,64] in [-1, 1]."""
    rng = np.random.default_rng(1103)
    return torch.from_numpy(rng.uniform(-1, 1, size=(1, hw[0], hw[1], 64)).astype(np.float32))


CONV_FRAMES = ((1, 1), (3, 2), (9, 33), (37, 53))

# One sdn_conv launch per case: (name, denoiser layer whose weights are used, frame, epilogue).  Epilogue keys: bias,
# resid ("rows" = fp32 rows, "planes" = hi / lo planes, updated in place when out == "planes"), mod, proj (conv4 + tanh),
# out ("f32" rows, "planes", "img"), hi_only (the GPU test repeats the launch with out_lo = NULL: the hi plane must be the same
# bits -- an f16 plane on its own is 2^-12 coarse and cannot be held to an arithmetic bound).  Every frame size and every
# epilogue occurs for a 3x3 and for a 1x1 layer; the plane-to-plane combinations the render CNN launches are among them.
CONV_CASES = (
    ("3x3 bias -> f32 rows", "conv2a", (1, 1), dict(bias=True, out="f32")),
    ("3x3 bias + fp32-row residual -> f32 rows", "conv2a", (3, 2), dict(bias=True, resid="rows", out="f32")),
    ("3x3 plane residual in place + FiLM -> planes", "conv2b", (9, 33), dict(resid="planes", mod=True, out="planes")),
    ("3x3 bias -> planes", "conv2a", (37, 53), dict(bias=True, out="planes", hi_only=True)),
    ("3x3 bias + plane residual, conv4 + tanh -> image", "conv3b", (9, 33), dict(bias=True, resid="planes", proj=True, out="img")),
    ("1x1 bias + plane residual, conv4 + tanh -> image", "conv4b", (1, 1), dict(bias=True, resid="planes", proj=True, out="img")),
    ("1x1 bias -> planes", "conv4a", (3, 2), dict(bias=True, out="planes", hi_only=True)),
    ("1x1 fp32-row residual + FiLM -> f32 rows", "conv4a", (9, 33), dict(resid="rows", mod=True, out="f32")),
    ("1x1 bias + plane residual, conv4 + tanh -> image", "conv4b", (37, 53), dict(bias=True, resid="planes", proj=True, out="img")),
)


def conv_inputs(hw, cin=256):
    """Inputs of one convolution layer on an h x w frame: x f32 [h*w, cin] (the activation that goes through
    sdn_conv_planes_from_f32), resid f32 [h*w, 256], FiLM vectors mod_w, mod_b f32 [256] and a bias f32 [256] for the layers
    the reference gives none."""
    rng = np.random.default_rng(1104 + 1000 * hw[0] + hw[1])
    n = hw[0] * hw[1]
    f = lambda *s, k=1.0: torch.from_numpy((k * rng.normal(size=s)).astype(np.float32))
    return dict(x=f(n, cin, k=0.5), resid=f(n, 256, k=0.5), mod_w=f(256, k=0.2), mod_b=f(256, k=0.2), bias=f(256, k=0.1))


def rows_to_nchw(rows, hw):
    return rows.reshape(1, hw[0], hw[1], -1).permute(0, 3, 1, 2).contiguous()


def nchw_to_rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def conv_case_eval(w, layer, hw, ep, inp, x_rows, resid_rows, how):
    """One CONV_CASES launch on the CPU.  x_rows / resid_rows: the values the kernel reads (decoded planes where it reads
    planes).  how: a term tuple (oracle/split_ref.py: the emulated kernel), "f32" (the fp32 yardstick) or "f64" (the truth).
    Returns rows [h*w, 256], or the image [3, h*w] for out == "img"."""
    from oracle import field_ref as FR
    from oracle import split_ref as SR
    ref = how in ("f32", "f64")
    dt = torch.float64 if how == "f64" else torch.float32
    W = FR.T(w, f"denoiser.{layer}.weight", dt)
    bias = inp["bias"].to(dt) if ep.get("bias") else None
    resid = rows_to_nchw(resid_rows.to(dt), hw) if ep.get("resid") else None
    mod = (inp["mod_w"].to(dt), inp["mod_b"].to(dt)) if ep.get("mod") else None
    proj = (FR.T(w, "denoiser.conv4.weight", dt).reshape(3, 256), FR.T(w, "denoiser.conv4.bias", dt)) if ep.get("proj") else None
    y = SR.conv_layer(rows_to_nchw(x_rows.to(dt), hw), W, "f32" if ref else how, bias, resid, mod, proj)
    if ep["out"] == "img":
        return y.reshape(3, -1)
    if not ref and ep["out"] == "planes":
        y = SR.planes(y)
    return nchw_to_rows(y)


def sky_encoded(dirs):
    """voxlib.positional_encoding(dirs, 5, incl_orig) by the CPU oracle: f32 [n,3] -> [n,33], SKYMLP.forward's argument."""
    from oracle import field_ref as FR
    from oracle import oracle as O
    O.build()
    return FR.positional_encoding(dirs[None, :, None, :].contiguous(), 5, True).reshape(-1, 33)


def max_err(a, truth):
    return float((torch.as_tensor(a).double() - truth).abs().max())


# A maximum over a handful of values is a single draw at the 1-ulp level, not a yardstick: frames of fewer than 256 pixels
# (1x1: 3 image values) are held to the E3 / E32 of the SAME layer and epilogue on the 9 x 33 frame.
YARD_HW = (9, 33)


def yard_frame(hw):
    return hw if hw[0] * hw[1] >= 256 else YARD_HW


def conv_case_yardstick(w, layer, ep):
    """(E3, E32) of a CONV_CASES layer + epilogue on the YARD_HW frame (inputs as the planes kernel stores them, emulated on the CPU)."""
    from oracle import split_ref as SR
    inp = conv_inputs(YARD_HW)
    x = SR.planes(inp["x"])
    resid = SR.planes(inp["resid"]) if ep.get("resid") == "planes" else inp["resid"]
    ev = lambda how: conv_case_eval(w, layer, YARD_HW, ep, inp, x, resid, how)
    truth = ev("f64")
    return max_err(ev(SR.T3), truth), max_err(ev("f32"), truth)


def head_yardstick(w):
    from oracle import field_ref as FR
    from oracle import split_ref as SR
    x = conv_inputs(YARD_HW, 64)["x"]
    hd = lambda **k: SR.head(x, FR.T(w, "denoiser.conv1.weight"), FR.T(w, "denoiser.conv1.bias"), YARD_HW, **k)
    truth = hd(dtype=torch.float64)
    return max_err(hd(), truth), max_err(hd(dtype=torch.float32), truth)


def chain_args(w, y_rows, hw):
    from oracle import field_ref as FR
    Tn = lambda n: FR.T(w, "denoiser." + n)
    return (rows_to_nchw(y_rows, hw), Tn("conv4a.weight"), Tn("conv4a.bias"), Tn("conv4b.weight"), Tn("conv4b.bias"), Tn("conv4.weight"), Tn("conv4.bias"))


def chain_yardstick(w):
    from oracle import split_ref as SR
    args = chain_args(w, SR.planes(conv_inputs(YARD_HW)["x"]), YARD_HW)
    truth = SR.chain_tail(*args, dtype=torch.float64)
    return max_err(SR.chain_tail(*args), truth), max_err(SR.chain_tail(*args, dtype=torch.float32), truth)


# --------------------------------------------------------------------------- the bounds of the arithmetic tests

FACTOR = 4.0          # the summation-order allowance of tests/test_exact_rung_gpu.py
RECORD = {}           # name -> the figures check / check_fp32 printed


def record_file_fixture():
    """A module-scoped autouse fixture that writes RECORD to $SDN_ARITH_RECORD (if set) when the module's tests are done."""
    @pytest.fixture(scope="module", autouse=True)
    def _record_file():
        yield
        path = os.environ.get("SDN_ARITH_RECORD")
        if path:
            with open(path, "w") as f:
                json.dump(RECORD, f, indent=1, sort_keys=True)
    return _record_file


def check(name, got, truth, emu, yard, factor=FACTOR, scale=None):
    """max |got - T| <= factor x E3; prints and records kernel/E3 and kernel/E32.  scale: (E3, E32) measured elsewhere (a larger
    frame of the same layer) where the case's own values are too few to be a yardstick.  E3 <= 8 x E32 is asserted here too: the
    emulation runs on tensors the code under test folded, and a wrong fold must not move the kernel and its yardstick together."""
    e = max_err(got, truth)
    e3, e32 = scale if scale is not None else (max_err(emu, truth), max_err(yard, truth))
    RECORD[name] = dict(kernel=e, E3=e3, E32=e32, kernel_over_E3=e / e3, kernel_over_E32=e / e32)
    if scale is not None:
        RECORD[name]["yardstick_frame"] = "%dx%d" % YARD_HW
    print(f"{name:72s} kernel {e:.2e}  E3 {e3:.2e}  E32 {e32:.2e}  kernel/E3 {e / e3:5.2f}  kernel/E32 {e / e32:5.2f}")
    assert e3 <= 8 * e32, (name, e3, e32)
    assert e <= factor * e3, (name, e, e3)


def check_fp32(name, got, truth, yard, factor=FACTOR):
    """An fp32 kernel: max |got - T| <= factor x E32, the error of the reference's own fp32 arithmetic."""
    e, e32 = max_err(got, truth), max_err(yard, truth)
    RECORD[name] = dict(kernel=e, E32=e32, kernel_over_E32=e / e32)
    print(f"{name:72s} kernel {e:.2e}  E32 {e32:.2e}  kernel/E32 {e / e32:5.2f}")
    assert e <= factor * e32, (name, e, e32)


def fold_from(R):
    """The folded render-MLP constants the kernels were given (oracle/split_ref.py fold_render_mlp's layout), on the CPU."""
    c = lambda t: t.detach().float().cpu()
    w = R.w
    return dict(w1=c(w["render_net.fc_1.weight"]), label_bias=c(R.label_bias), hidden=[c(R.mod[i][0]) for i in (2, 3, 4, 5, 6)],
                beta=[c(R.mod[i][1]) for i in (2, 3, 4, 5, 6)], w_sigma=c(w["render_net.fc_sigma.weight"]).reshape(-1),
                b_sigma=c(w["render_net.fc_sigma.bias"]).reshape(-1)[0], wc=c(w["render_net.fc_out_c.weight"]),
                bc=c(w["render_net.fc_out_c.bias"]))


def two_kernel_field(R, vid, d2, rd, ori, ns):
    """sdn_field_encode -> sdn_field_mlp (colour_terms = 3, term_eps = 0: the caller sets them) on the rays vid [n,M] / d2 [2,n,M] /
    rd [n,3] (GPU) from the camera origin `ori` (CPU), and what the MLP kernel was given: returns net_out [n,64] (GPU) and a dict of
    CPU tensors -- feat [n,ns,128], dist [n,ns], label [n,ns], sky_only / nosky [n], sky_c [n,64], sky_avg [64] -- plus the ray
    arrays for the one-kernel forms.  The sky inputs are fused.sky_fused's on the same directions."""
    from scenedreamer_amd import fused
    n = vid.shape[0]
    with torch.no_grad():
        sky_c, sky_avg = fused.sky_fused(R, rd)
        buf = fused.encode(R, vid, d2, rd, ori, ns)
        net_out = fused.mlp_from(R, buf, sky_c, sky_avg.reshape(-1), n, ns)
        torch.cuda.synchronize()
    feat, dist, label = decode_encode_buffers(buf, n, ns)
    flags = buf["rayflag"].cpu().numpy()
    sky_only = torch.from_numpy((flags & 1).astype(bool))
    feat = torch.from_numpy(feat[:, :ns].reshape(n, ns, 128).copy())
    feat[sky_only] = 0.0            # rays that hit nothing: the kernel gathers no features for them and gives them weight 0
    given = dict(feat=feat, dist=torch.from_numpy(dist[:, :ns].copy()), label=torch.from_numpy(label[:, :ns].astype(np.int64)),
                 sky_only=sky_only, nosky=torch.from_numpy(((flags >> 1) & 1).astype(bool)), sky_c=sky_c.cpu(), sky_avg=sky_avg.reshape(-1).cpu())
    return net_out, given, (vid, d2, rd, ori, sky_c, sky_avg)


def field_references(R, weights, given):
    """fp64 truth, emulated 3-term MLP + fp32 compositing, fp32 MLP + fp32 compositing -- on exactly the values the kernel read."""
    from oracle import split_ref as SR
    n, ns = given["dist"].shape
    x, lab = given["feat"].reshape(n * ns, 128), given["label"].reshape(-1)
    z = R.z.cpu().numpy()
    comp = lambda s, c, dt: SR.composite(s.reshape(n, ns), c.reshape(n, ns, 64), given["dist"].to(dt), given["sky_only"], given["nosky"],
                                         given["sky_c"].to(dt), given["sky_avg"].to(dt))
    truth = comp(*SR.render_mlp_ref(weights, x, z, lab, torch.float64), torch.float64)
    yard = comp(*SR.render_mlp_ref(weights, x, z, lab, torch.float32), torch.float32)
    emu = comp(*SR.render_mlp(fold_from(R), x, lab), torch.float32)
    return truth, emu, yard
