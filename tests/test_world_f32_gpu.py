"""The fixed-order world encoder and style MLP on the MI355X (csrc/world_f32.hip: sdn_wenc_*_f32, sdn_style_mlp_f32,
fused.world_exact / style_exact, Renderer.exact_world / exact_style, modules.ConditionalHashGrid / StyleMLP with sdn_exact): the
arithmetic against fp64 in units of the error E32 of the library's own fp32 arithmetic (tests/field_layout.py: 4 x E32;
tests/test_world_f32_cpu.py qualifies the orders that bound asks for), edges, the launch shape and the position in the frame with no
tolerance, fp32's range with no tolerance, the renderer, another process, and the module surface.  Every arithmetic check prints its
kernel/E32 ratio; SDN_ARITH_RECORD=<file> collects them as JSON."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import field_layout as FL
import world_f32_ref as WR

pytestmark = pytest.mark.gpu

RECORD = FL.RECORD
_record_file = FL.record_file_fixture()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-3          # the tolerance of tests/test_exact_rung_gpu.py
HW, NS = (72, 104), 24
ENV = ("SDN_EXACT_WORLD", "SDN_EXACT_STYLE", "SDN_WORLD_EXACT", "SDN_STYLE_EXACT", "SDN_EXACT_SKY", "SDN_EXACT_CNN")
NAN = float("nan")


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _backend(w):
    """What fused.world_exact / style_exact expect of a renderer: `w` (the encoders' parameters on the GPU) and `dev`."""
    return types.SimpleNamespace(dev=_dev(), w={k: torch.as_tensor(np.asarray(v)).to(_dev()) for k, v in w.items()
                                                if k.startswith(("world_encoder.", "style_net."))})


@pytest.fixture(scope="module")
def backend(weights_full):
    return _backend(weights_full)


@pytest.fixture(scope="module")
def gpu_weights(weights_full):
    """The whole weight set on the GPU, once: Renderer(...) takes device tensors as they are."""
    return {k: torch.as_tensor(np.asarray(v)).to(_dev()) for k, v in weights_full.items()}


@pytest.fixture(scope="module")
def yard(weights_full):
    """The (70, 52) maps and the library's whole network on them in fp64 and fp32: computed once, never modified."""
    hm, sm = WR.maps(WR.YARD_HW, 0)
    t64, t32 = WR.lib_encode(weights_full, hm, sm, torch.float64), WR.lib_encode(weights_full, hm, sm, torch.float32)
    e32 = {n: FL.max_err(t32[n], t64[n]) for n in t64}
    return types.SimpleNamespace(hm=hm, sm=sm, t64=t64, t32=t32, e32=e32)


def _guarded(n):
    return torch.full((n + 64,), NAN, dtype=torch.float32, device=_dev())


def _unguard(buf, n, what):
    torch.cuda.synchronize()
    assert torch.isnan(buf[n:]).all(), f"{what}: the floats behind the last row were written"
    return buf[:n]


def _head(B, hm, sm, wg=0):
    """sdn_wenc_head_f32 through the C entry, 64 NaN guard floats behind the last row: rows [Ho*Wo,16] and (Ho, Wo)."""
    from scenedreamer_amd import capi, fused
    wx = getattr(B, "_fused_world_f32", None) or fused.prepare_world_exact(B)
    hm, sm = hm.to(B.dev).contiguous(), sm.to(B.dev).contiguous()
    H, W = hm.shape[2:]
    ho, wo = WR.half(H), WR.half(W)
    buf = _guarded(ho * wo * 16)
    capi.check(capi.lib().sdn_wenc_head_f32(hm.data_ptr(), sm.data_ptr(), *[t.data_ptr() for t in wx["head"]], buf.data_ptr(), H, W, wg,
                                            capi.current_stream(B.dev)), "sdn_wenc_head_f32")
    return _unguard(buf, ho * wo * 16, "head").view(ho * wo, 16), (ho, wo)


def _conv(B, name, x_rows, hw, wg=0):
    """sdn_wenc_conv_f32 for layer `name` through the C entry on rows [H*W,cin] (GPU), guarded: rows [Ho*Wo,cout] and (Ho, Wo)."""
    from scenedreamer_amd import capi, fused
    wx = getattr(B, "_fused_world_f32", None) or fused.prepare_world_exact(B)
    i = WR.CONV_NAMES.index(name)
    cin, cout, stride = WR.PAIRS[i]
    x_rows = x_rows.contiguous()
    assert tuple(x_rows.shape) == (hw[0] * hw[1], cin) and x_rows.is_cuda
    ho, wo = (WR.half(hw[0]), WR.half(hw[1])) if stride == 2 else hw
    buf = _guarded(ho * wo * cout)
    capi.check(capi.lib().sdn_wenc_conv_f32(x_rows.data_ptr(), cin, cout, stride, wx["packed"][i].data_ptr(), buf.data_ptr(), hw[0], hw[1], wg,
                                            capi.current_stream(B.dev)), "sdn_wenc_conv_f32")
    return _unguard(buf, ho * wo * cout, name).view(ho * wo, cout), (ho, wo)


def _tail(B, r, pooled=True):
    from scenedreamer_amd import capi, fused
    wx = getattr(B, "_fused_world_f32", None) or fused.prepare_world_exact(B)
    r = r.contiguous()
    pb, gb = torch.full((512 + 64,), NAN, device=B.dev), torch.full((2 + 64,), NAN, device=B.dev)
    capi.check(capi.lib().sdn_wenc_tail_f32(r.data_ptr(), r.shape[0], *[t.data_ptr() for t in wx["tail"]], pb.data_ptr() if pooled else None,
                                            gb.data_ptr(), capi.current_stream(B.dev)), "sdn_wenc_tail_f32")
    g = _unguard(gb, 2, "global_enc")
    assert torch.isnan(pb[512:]).all() and (pooled or torch.isnan(pb).all())
    return pb[:512], g.view(1, 2)


def _by_entries(B, hm, sm, wg=0):
    """The whole encode through the C entries, every output guarded: {layer: rows, "pooled", "global_enc"}."""
    out = {}
    x, hw = _head(B, hm, sm, wg)
    out["head"] = x
    for name in WR.CONV_NAMES:
        x, hw = _conv(B, name, x, hw, wg)
        out[name] = x
    out["pooled"], out["global_enc"] = _tail(B, x)
    return out


# ----------------------------------------------------------------------------------------------------- 1 - 4: arithmetic

def test_each_layer_in_isolation_against_fp64(backend, weights_full, yard):
    """1. On the (70, 52) maps (35x26 -> 18x13 -> 9x7 -> 5x4 -> 3x2 -> 2x1: every stride-2 layer meets an odd extent, every layer has
    >= 1024 output values), each layer on the f32-rounded fp64 activation of the layer before: within 4 x E32 of F.conv2d in fp64, E32
    = F.conv2d in fp32 on the same input."""
    x, sem, hw = yard.hm, yard.sm, None
    for name in WR.LAYER_NAMES:
        truth = WR.lib_layer(weights_full, name, x, sem, torch.float64)
        yd = WR.lib_layer(weights_full, name, x, sem, torch.float32)
        if name == "head":
            got, hw = _head(backend, x, sem)
        else:
            got, hw = _conv(backend, name, WR.rows(x).to(backend.dev), hw)
        assert truth.numel() >= 1024 and tuple(truth.shape[2:]) == tuple(hw) and torch.isfinite(got).all()
        FL.check_fp32(f"sdn_wenc f32 {name} in isolation, 70x52 maps", got.cpu(), WR.rows(truth), WR.rows(yd))
        x, sem = yard.t64[name].to(torch.float32), None
        hw = tuple(x.shape[2:])


def test_whole_encode_on_the_scene(backend, weights_full, scene256):
    """2. fused.world_exact on scene256's 256 x 256 maps: every layer's rows and `pooled` within 4 x E32 of the fp64 network, E32 from
    the fp32 network at the same layer; everything finite."""
    from scenedreamer_amd import fused
    hm, sm = scene256.current_height_map.float(), scene256.current_semantic_map.float()
    t64, t32 = WR.lib_encode(weights_full, hm, sm, torch.float64), WR.lib_encode(weights_full, hm, sm, torch.float32)
    genc, lay = fused.world_exact(backend, hm, sm, layers=True)
    torch.cuda.synchronize()
    assert tuple(genc.shape) == (1, 2) and torch.isfinite(genc).all() and sorted(lay) == sorted(WR.LAYER_NAMES + ("pooled",))
    for name in WR.LAYER_NAMES:
        assert torch.isfinite(lay[name]).all()
        FL.check_fp32(f"world_exact {name}, scene256", lay[name].cpu(), WR.rows(t64[name]), WR.rows(t32[name]))
    FL.check_fp32("world_exact pooled, scene256", lay["pooled"].cpu(), t64["pooled"][0], t32["pooled"][0])
    e = FL.max_err(genc.cpu(), t64["global_enc"])
    print(f"world_exact global_enc, scene256: {genc.cpu().numpy().tolist()}  |kernel - fp64| {e:.2e} (two values: no yardstick; see test 4)")
    assert e < 1e-5


def _tail_inputs():
    rng = np.random.default_rng(1231)
    return torch.from_numpy(np.maximum(rng.normal(0.3, 0.5, size=(128, 6, 512)), 0).astype(np.float32))     # ReLU outputs


def test_tail_in_isolation(backend, weights_full):
    """3. 128 seeded inputs [6][512] -> 256 global_enc values: max error against fp64 <= 4 x the E32 of the same population
    (torch.mean / F.linear / tanh in fp32); `pooled` is optional and likewise held."""
    r = _tail_inputs()
    p64, g64 = WR.lib_tail(weights_full, r, torch.float64)
    p32, g32 = WR.lib_tail(weights_full, r, torch.float32)
    rg = r.to(backend.dev)
    got = [_tail(backend, rg[i], pooled=(i % 2 == 0)) for i in range(128)]
    g = torch.cat([t[1] for t in got]).cpu()
    assert tuple(g.shape) == (128, 2) and torch.isfinite(g).all()
    FL.check_fp32("sdn_wenc_tail_f32 global_enc, 128 x [6][512]", g, g64, g32)
    FL.check_fp32("sdn_wenc_tail_f32 pooled, 64 x [6][512]", torch.stack([got[i][0] for i in range(0, 128, 2)]).cpu(), p64[0::2], p32[0::2])
    # and the restated order gives the kernel's bits for pooled (f64 sums of f32 values, one rounding)
    assert torch.equal(got[0][0].cpu(), WR.chain_tail(weights_full, r[0])[0])


def test_global_enc_of_the_whole_encode(backend, weights_full):
    """4. The 128 map pairs maps((12, 10), s) as ONE population of 256 values: the kernel's max error against
    field_ref.world_encoder(float64) <= 4 x the fp32 oracle's max error on that population (two values from one scene are a single
    draw, not a yardstick: field_layout.yard_frame's rule)."""
    from oracle import field_ref as FR
    from scenedreamer_amd import fused
    got, t64, t32 = [], [], []
    for s in range(128):
        hm, sm = WR.maps((12, 10), s)
        got.append(fused.world_exact(backend, hm, sm))
        t64.append(FR.world_encoder(weights_full, hm, sm, torch.float64))
        t32.append(FR.world_encoder(weights_full, hm, sm, torch.float32))
    got = torch.cat(got).cpu()
    assert tuple(got.shape) == (128, 2) and torch.isfinite(got).all()
    FL.check_fp32("world_exact global_enc, 128 x maps((12, 10), s)", got, torch.cat(t64), torch.cat(t32))


# ----------------------------------------------------------------------------------------------------- 5: edges

@pytest.mark.parametrize("hw", [(1, 1), (2, 3), (33, 1)], ids=str)
def test_edges(backend, weights_full, yard, hw):
    """5. Maps of one pixel, of less than a wave's pixels and of one column: every layer runs through the C entries with NaN guard
    floats behind its last row (nothing is written there), is finite and equals fused.world_exact's bits; against the fp64 network
    each layer is within 4 x E32 -- its own where it has >= 256 values, else the same layer's on the (70, 52) maps."""
    from scenedreamer_amd import fused
    hm, sm = WR.maps(hw, 7)
    t64, t32 = WR.lib_encode(weights_full, hm, sm, torch.float64), WR.lib_encode(weights_full, hm, sm, torch.float32)
    out = _by_entries(backend, hm, sm)
    genc, lay = fused.world_exact(backend, hm, sm, layers=True)
    assert torch.equal(genc, out["global_enc"]) and torch.isfinite(genc).all()
    for name in WR.LAYER_NAMES + ("pooled",):
        truth = WR.rows(t64[name]) if name != "pooled" else t64[name][0]
        assert torch.equal(lay[name], out[name].view(lay[name].shape)) and torch.isfinite(out[name]).all(), name
        assert tuple(out[name].shape) == tuple(truth.shape), name
        e = FL.max_err(out[name].cpu(), truth)
        e32 = FL.max_err(t32[name], t64[name]) if truth.numel() >= 256 else yard.e32[name]
        RECORD[f"world_exact {name}, {hw[0]}x{hw[1]} maps"] = dict(kernel=e, E32=e32, kernel_over_E32=e / e32, values=truth.numel())
        print(f"{name:24s} {hw} values {truth.numel():6d}  kernel {e:.2e}  E32 {e32:.2e}  kernel/E32 {e / e32:5.2f}")
        assert e <= FL.FACTOR * e32, (name, e, e32)


# ----------------------------------------------------------------------------------------------------- 6: launch shape and position

def test_launch_shape_is_a_schedule(backend, yard):
    """6a. n_workgroups = 0, 1 and 2 (the grid-stride loops: one workgroup walks every pixel group) give the same bits for every layer's
    rows and for global_enc, and so does a second call."""
    from scenedreamer_amd import fused
    g0, l0 = fused.world_exact(backend, yard.hm, yard.sm, layers=True)
    for wg in (0, 1, 2):
        g, l = fused.world_exact(backend, yard.hm, yard.sm, layers=True, n_workgroups=wg)
        assert torch.equal(g, g0), wg
        for name in l0:
            assert torch.equal(l[name], l0[name]), (wg, name)
    assert torch.equal(fused.world_exact(backend, yard.hm, yard.sm), g0)
    by = _by_entries(backend, yard.hm, yard.sm, 1)
    assert all(torch.equal(by[n].view(l0[n].shape), l0[n]) for n in l0) and torch.equal(by["global_enc"], g0)


@pytest.mark.parametrize("name", ["conv_blocks.1.layers.0", "conv_blocks.1.layers.2"])
def test_position_in_the_frame(backend, name):
    """6b. A pixel's value depends on its 3x3 neighbourhood only, not on where it lies: the layer (stride 1, stride 2) on a crop of its
    input at an even offset equals the matching window of the whole layer's output, bit for bit, one output pixel in from the
    crop's edges."""
    cin, cout, stride = WR.PAIRS[WR.CONV_NAMES.index(name)]
    H, W, y0, x0, hc, wc = 21, 150, 4, 6, 13, 139           # 3150 pixels: 25 pixel groups; the crop: 1807 pixels, 15 groups
    rng = np.random.default_rng(1261)
    x = torch.from_numpy(rng.normal(size=(H, W, cin)).astype(np.float32)).to(backend.dev)
    whole, (ho, wo) = _conv(backend, name, x.reshape(H * W, cin), (H, W))
    crop, (hco, wco) = _conv(backend, name, x[y0:y0 + hc, x0:x0 + wc].reshape(hc * wc, cin), (hc, wc))
    whole, crop = whole.view(ho, wo, cout), crop.view(hco, wco, cout)
    oy, ox = y0 // stride, x0 // stride
    assert float(whole.abs().max()) > 0
    assert torch.equal(crop[1:-1, 1:-1], whole[oy + 1:oy + hco - 1, ox + 1:ox + wco - 1])


@pytest.mark.parametrize("pair", [0, 1, 9], ids=lambda i: "%dx%d" % WR.PAIRS[i][:2])
def test_packed_stream_holds_every_weight_once(backend, weights_full, pair):
    """The pack kernel against the layout world_f32.hip's header states: float4 ((tap * NB + ib) * cin / 8 + kq) * 64 + lane holds in
    element e W[32 ib + (lane & 31)][8 kq + 2 e + (lane >> 5)][tap]; rows >= cout (COUT = 16: the upper half of its block) are zeros."""
    from scenedreamer_amd import fused
    wx = getattr(backend, "_fused_world_f32", None) or fused.prepare_world_exact(backend)
    cin, cout, _ = WR.PAIRS[pair]
    nb = (cout + 31) // 32
    w = np.zeros((32 * nb, cin, 9), np.float32)
    w[:cout] = np.asarray(weights_full[f"world_encoder.{WR.CONV_NAMES[pair]}.weight"], np.float32).reshape(cout, cin, 9)
    tap, ib, kq, lane, e = np.meshgrid(np.arange(9), np.arange(nb), np.arange(cin // 8), np.arange(64), np.arange(4), indexing="ij")
    want = w[32 * ib + (lane & 31), 8 * kq + 2 * e + (lane >> 5), tap].reshape(-1)
    got = wx["packed"][pair].view(torch.float32).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)
    assert np.count_nonzero(got) == np.count_nonzero(w[:cout]) and got.size == 9 * cin * 32 * nb


# ----------------------------------------------------------------------------------------------------- 7: range

def test_range_is_fp32s_with_no_tolerance(weights_full, backend, yard):
    """7. ReLU and LeakyReLU are positively homogeneous and a power of two scales fp32 exactly: conv_blocks.0.layers.0.weight x 2^10
    and layers.2.weight x 2^-10 are the same function bit for bit from conv_blocks.0.layers.2 on; so are style_net.fc_layers.0
    (weight and bias) x 2^10 and fc_layers.1.weight x 2^-10."""
    from scenedreamer_amd import fused
    w = dict(weights_full)
    g = np.float32(2.0 ** 10)
    w["world_encoder.conv_blocks.0.layers.0.weight"] = weights_full["world_encoder.conv_blocks.0.layers.0.weight"] * g
    w["world_encoder.conv_blocks.0.layers.2.weight"] = weights_full["world_encoder.conv_blocks.0.layers.2.weight"] / g
    w["style_net.fc_layers.0.weight"] = weights_full["style_net.fc_layers.0.weight"] * g
    w["style_net.fc_layers.0.bias"] = weights_full["style_net.fc_layers.0.bias"] * g
    w["style_net.fc_layers.1.weight"] = weights_full["style_net.fc_layers.1.weight"] / g
    big = _backend(w)
    g0, l0 = fused.world_exact(backend, yard.hm, yard.sm, layers=True)
    g1, l1 = fused.world_exact(big, yard.hm, yard.sm, layers=True)
    assert torch.equal(l1["conv_blocks.0.layers.0"], l0["conv_blocks.0.layers.0"] * float(g)) and float(l0["conv_blocks.0.layers.0"].max()) > 0
    for name in WR.CONV_NAMES[1:] + ("pooled",):
        assert torch.equal(l1[name], l0[name]), name
    assert torch.equal(g1, g0)
    s = WR.styles(range(8))
    z0, z1 = fused.style_exact(backend, s), fused.style_exact(big, s)
    assert torch.isfinite(z0).all() and float(z0.abs().max()) > 0 and torch.equal(z0, z1)


# ----------------------------------------------------------------------------------------------------- 8: style

def test_style_exact(backend, weights_full):
    """8. fused.style_exact on 8 seeded styles in one call (2048 values) within 4 x E32 of field_ref.style_mlp; row i of the batch is
    the one-style call's, bit for bit."""
    from oracle import field_ref as FR
    from scenedreamer_amd import fused
    s = WR.styles(range(8))
    z = fused.style_exact(backend, s)
    assert tuple(z.shape) == (8, 256) and torch.isfinite(z).all()
    FL.check_fp32("sdn_style_mlp_f32, 8 styles", z.cpu(), FR.style_mlp(weights_full, s, torch.float64), FR.style_mlp(weights_full, s, torch.float32))
    for i in range(8):
        assert torch.equal(fused.style_exact(backend, s[i:i + 1])[0], z[i]), i
    assert torch.equal(fused.style_exact(backend, s[3])[0], z[3])          # a [128] vector is one style


# ----------------------------------------------------------------------------------------------------- 9: the renderer

def test_renderer(gpu_weights, backend, scene256):
    """9. The default Renderer is what it was (two instances agree bit for bit, `encoders` says "torch"); with exact_world = exact_style
    = "f32" global_enc is fused.world_exact's and z is style_exact's (two instances agree), both within 1e-5 of the library's, and the
    frames of modes "fused" and "exact" are within 1e-3 of the default renderer's; resetting the attributes and encoding again gives
    back the first frames bit for bit."""
    from scenedreamer_amd import camera, fused, synth
    from scenedreamer_amd.renderer import Renderer
    style = synth.make_style(8888)
    pose = camera.eval_camera_poses(scene256, maxstep=8)[5]
    D, D2 = Renderer(gpu_weights, scene256, "cuda"), Renderer(gpu_weights, scene256, "cuda")
    D.set_style(style)
    D2.set_style(style)
    assert torch.equal(D.global_enc, D2.global_enc) and torch.equal(D.z, D2.z)
    assert D.encoders == {"world": "torch", "style": "torch"} and D.exact_world is None and D.exact_style is None
    first = {m: D.render_frame(pose, HW, NS, mode=m) for m in ("fused", "exact")}
    genc_t, z_t = D.global_enc.clone(), D.z.clone()

    X = Renderer(gpu_weights, scene256, "cuda", exact_world="f32", exact_style="f32")          # the constructor's keywords
    assert X.encoders == {"world": "f32", "style": None}
    X.set_style(style)
    assert X.encoders == {"world": "f32", "style": "f32"}
    D2.exact_world = D2.exact_style = "f32"          # ... or the attributes, and encoding again
    D2.set_scene(scene256)
    D2.set_style(style)
    want_g = fused.world_exact(backend, scene256.current_height_map, scene256.current_semantic_map)
    want_z = fused.style_exact(backend, torch.as_tensor(style))
    for r in (X, D2):
        assert torch.equal(r.global_enc, want_g) and torch.equal(r.z, want_z) and tuple(r.z.shape) == (1, 256)
    dg, dz = float((X.global_enc - genc_t).abs().max()), float((X.z - z_t).abs().max())
    print(f"exact_world / exact_style = 'f32' vs the library: global_enc max abs diff {dg:.3e}, z max abs diff {dz:.3e} (max|z| {float(z_t.abs().max()):.3f})")
    assert dg < 1e-5 and dz <= 1e-5 * float(z_t.abs().max())

    D.exact_world = D.exact_style = "f32"
    D.set_scene(scene256)
    D.set_style(style)
    assert torch.equal(D.global_enc, want_g) and torch.equal(D.z, want_z) and D.encoders == {"world": "f32", "style": "f32"}
    for m in ("fused", "exact"):
        img = D.render_frame(pose, HW, NS, mode=m)
        err = float((img - first[m]).abs().max())
        print(f"mode={m!r} with the f32 encoders vs the default renderer's frame: max abs diff {err:.3e}")
        assert tuple(img.shape) == (1, 3) + HW and torch.isfinite(img).all() and err < TOL
    D.exact_world = D.exact_style = None
    D.set_scene(scene256)
    D.set_style(style)
    assert D.encoders == {"world": "torch", "style": "torch"} and torch.equal(D.global_enc, genc_t) and torch.equal(D.z, z_t)
    for m in ("fused", "exact"):
        assert torch.equal(D.render_frame(pose, HW, NS, mode=m), first[m]), m
    D.exact_world = "fast"
    with pytest.raises(ValueError, match="exact_world"):
        D.set_scene(scene256)


# ----------------------------------------------------------------------------------------------------- 10: another process

CHILD = """
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import types, numpy as np, torch
import world_f32_ref as WR
from scenedreamer_amd import fused, synth
w = synth.make_weights(0, with_embeddings=False)
dev = torch.device("cuda", torch.cuda.current_device())
B = types.SimpleNamespace(dev=dev, w={{k: torch.as_tensor(np.asarray(v)).to(dev) for k, v in w.items() if k.startswith(("world_encoder.", "style_net."))}})
hm, sm = WR.maps(WR.YARD_HW, 0)
g, lay = fused.world_exact(B, hm, sm, layers=True)
z = fused.style_exact(B, WR.styles(range(8)))
torch.cuda.synchronize()
print("GENC", g.cpu().numpy().tobytes().hex())
print("LAST", lay["conv_blocks.4.layers.2"].cpu().numpy().tobytes().hex())
print("Z", z.cpu().numpy().tobytes().hex())
"""


def test_another_process_gives_the_same_bits(backend, yard):
    """10. One fresh child process computes world_exact and style_exact on the same inputs: the bytes are this process's."""
    from scenedreamer_amd import fused
    g, lay = fused.world_exact(backend, yard.hm, yard.sm, layers=True)
    z = fused.style_exact(backend, WR.styles(range(8)))
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = dict(line.split(" ", 1) for line in r.stdout.splitlines() if line.split(" ", 1)[0] in ("GENC", "LAST", "Z"))
    assert got["GENC"] == g.cpu().numpy().tobytes().hex()
    assert got["LAST"] == lay["conv_blocks.4.layers.2"].cpu().numpy().tobytes().hex()
    assert got["Z"] == z.cpu().numpy().tobytes().hex()


# ----------------------------------------------------------------------------------------------------- 11: module surface

def _load(net, weights, pre):
    net.load_state_dict({k[len(pre):]: torch.as_tensor(np.asarray(v)) for k, v in weights.items() if k.startswith(pre)})
    net = net.cuda().eval()
    for prm in net.parameters():
        prm.requires_grad_(False)
    return net


class ConditionalHashGrid(torch.nn.Module):
    """A locally defined class named like the reference's (its structure, this file's own forward) for make_fast."""

    def __init__(self):
        super().__init__()
        from scenedreamer_amd import modules
        self.sconv_head = torch.nn.Conv2d(11, 8, 3, stride=2, padding=1)
        self.hconv_head = torch.nn.Conv2d(1, 8, 3, stride=2, padding=1)
        self.conv_blocks = torch.nn.Sequential(*[modules.SRTConvBlock(16 << i) for i in range(5)])
        self.fc1, self.fc2, self.act = torch.nn.Linear(512, 16), torch.nn.Linear(16, 2), torch.nn.LeakyReLU(0.2)

    def forward(self, height_map, semantic_map):
        x = torch.cat([self.act(self.hconv_head(height_map)), self.act(self.sconv_head(semantic_map))], dim=1)
        for layer in self.conv_blocks:
            x = self.act(layer(x))
        x = x.permute(0, 2, 3, 1)
        return torch.tanh(self.fc2(self.act(self.fc1(torch.mean(x.reshape(x.shape[0], -1, x.shape[-1]), dim=1)))))


class StyleMLP(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.normalize_input = self.output_act = True
        self.fc_layers = torch.nn.ModuleList([torch.nn.Linear(128 if i == 0 else 256, 256) for i in range(5)])
        self.fc_out, self.act = torch.nn.Linear(256, 256), torch.nn.LeakyReLU(0.2)

    def forward(self, z):
        z = torch.nn.functional.normalize(z, p=2, dim=-1)
        for layer in self.fc_layers:
            z = self.act(layer(z))
        return self.act(self.fc_out(z))


def test_module_surface(backend, weights_full, yard):
    """11. modules.ConditionalHashGrid / StyleMLP loaded from the synthetic weights: with sdn_exact = True the bits of world_exact /
    style_exact; without the flag the call IS the composite forward's (counted: the library's own bits are not repeatable from call
    to call, which is what the kernels are for).  make_fast on a locally defined class named like the reference's behaves the same."""
    from scenedreamer_amd import fused, modules
    hm, sm = yard.hm.cuda(), yard.sm.cuda()
    s = WR.styles(range(8)).cuda()
    want_g, want_z = fused.world_exact(backend, hm, sm), fused.style_exact(backend, s)
    for wcls, scls, sargs in ((modules.ConditionalHashGrid, modules.StyleMLP, (128, 256)),
                              (modules.make_fast(ConditionalHashGrid), modules.make_fast(StyleMLP), ())):
        assert modules.is_native(wcls) and modules.is_native(scls)
        net, sty = _load(wcls(), weights_full, "world_encoder."), _load(scls(*sargs), weights_full, "style_net.")
        calls = []
        for m in (net, sty):          # count the composite forward's calls: the library's bits do not repeat from call to call (MIOpen)
            m._forward_composite = (lambda f: lambda *a: (calls.append(f), f(*a))[1])(m._forward_composite)
        with torch.no_grad():
            g0, z0 = net(hm, sm), sty(s)
            assert len(calls) == 2          # without the flag the forward IS the composite one
            net.sdn_exact = sty.sdn_exact = True
            g1, z1 = net(hm, sm), sty(s)
        assert len(calls) == 2 and net.__dict__.get("_sdn_composite_reason") is None and sty.__dict__.get("_sdn_composite_reason") is None
        assert torch.equal(g1, want_g) and torch.equal(z1, want_z)
        assert float((g1 - g0).abs().max()) < 1e-5 and float((z1 - z0).abs().max()) <= 1e-5 * float(z0.abs().max())
        del net.sdn_exact, sty.sdn_exact
        with torch.no_grad():
            g2, z2 = net(hm, sm), sty(s)
            assert len(calls) == 4 and float((g2 - g0).abs().max()) < 1e-5 and float((z2 - z0).abs().max()) <= 1e-5 * float(z0.abs().max())
            # a call the kernels do not serve goes to the composite forward, with the reason recorded
            net.sdn_exact = True
            two = net(hm.repeat(2, 1, 1, 1), sm.repeat(2, 1, 1, 1))
        assert tuple(two.shape) == (2, 2) and "batch 1" in net.__dict__["_sdn_composite_reason"]
