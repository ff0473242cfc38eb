"""The fp32 field kernel's FIELD_AUX instantiation and stochastic sampling on the MI355X (csrc/field_f32.hip:
sdn_field_render_f32_aux, fused.field_exact(u=, aux=), the drop-in binding's exact route): the plain launch is unchanged, the
eleven other return values of Generator._forward_perpix against the sampling op, their own recomposition, the f16 AUX kernel and
the reference goldens; independence of ray order and window; range with no tolerance; the training-time draw; the bound method
on a holder that has no reference method to fall back to."""
import ctypes
import json

import numpy as np
import pytest
import torch

from conftest import bits, golden

pytestmark = pytest.mark.gpu

TOL = 1e-3          # the tolerance of tests/test_render_gpu.py
KEYS = ("weights", "depth", "sigma", "colour", "sky_blended", "nosky")


def _scaled_weights(weights_full, g):
    """fc_1 (weight, bias, fc_m_a) x g and fc_2.weight / g: the same function bit for bit when g is a power of two
    (tests/test_exact_rung_gpu.py), outside the packed f16 stream's range for g = 2^10."""
    w = dict(weights_full)
    for k in ("render_net.fc_1.weight", "render_net.fc_1.bias", "render_net.fc_m_a.weight"):
        w[k] = torch.as_tensor(np.asarray(w[k])) * g
    w["render_net.fc_2.weight"] = torch.as_tensor(np.asarray(w["render_net.fc_2.weight"])) * (1.0 / g)
    return w


@pytest.fixture(scope="module")
def renderer(weights_full, scene256):
    from scenedreamer_amd import synth
    from scenedreamer_amd.renderer import Renderer
    r = Renderer(weights_full, scene256, "cuda")
    r.set_style(synth.make_style(8888))
    return r


@pytest.fixture(scope="module")
def big(weights_full, scene256):
    from scenedreamer_amd import synth
    from scenedreamer_amd.renderer import Renderer
    r = Renderer(_scaled_weights(weights_full, 2.0 ** 10), scene256, "cuda")
    r.set_style(synth.make_style(8888))
    return r


class Case:
    """The rays of one frame (the padded frame of `hw`), a window over them and a sample count."""

    def __init__(self, R, scene256, hw, ns, crop):
        from scenedreamer_amd import camera, fused
        self.pose = camera.eval_camera_poses(scene256, maxstep=8)[5]
        self.ns = ns
        with torch.no_grad():
            vid, d2, rd, (H0, W0) = R.cast_rays(self.pose, hw)
            n = H0 * W0
            self.H0, self.W0, self.M = H0, W0, R.M
            self.vid, self.d2, self.rd = vid.view(n, R.M), d2.view(2, n, R.M), rd.view(n, 3)
            self.sky_c = R.sky_features(self.rd)
            self.sky_avg = self.sky_c.mean(dim=0, keepdim=True)
        self.ori = torch.as_tensor(self.pose[0], dtype=torch.float32)
        self.o = crop
        self.win = fused.Window.crop(H0, W0, crop)
        self.h, self.w = H0 - 2 * crop, W0 - 2 * crop

    def crop(self, per_ray):
        """Rows of a frame-wide per-ray array [H0 * W0, ...] at the window's pixels, row-major."""
        v = per_ray.reshape(self.H0, self.W0, *per_ray.shape[1:])
        o = self.o
        v = v[o:self.H0 - o, o:self.W0 - o] if o else v
        return v.reshape(self.h * self.w, *per_ray.shape[1:])

    def run(self, R, aux=None, u=None, win=None, **kw):
        from scenedreamer_amd import fused
        with torch.no_grad():
            return fused.field_exact(R, self.vid, self.d2, self.rd, self.ori, self.sky_c, self.sky_avg, self.ns, window=win or self.win,
                                     u=u, aux=aux, **kw)

    def depth(self, R, u=None, division="reciprocal"):
        """rand_depth of the window's rays from the stand-alone sampling op, after the NaN / inf -> 0 replacement."""
        from scenedreamer_amd import ops
        o = self.o
        d2 = self.d2.view(2, self.H0, self.W0, self.M)[:, o:self.H0 - o, o:self.W0 - o]
        d, _, _ = ops.sample_depth_batched(d2.reshape(1, 2, self.h, self.w, self.M, 1).contiguous(), self.ns + 1, deterministic=u is None, use_box_boundaries=False, sample_depth=R.sample_depth,
                                           rand=u.view(1, self.h, self.w, self.ns + 1, 1) if u is not None else None, division=division)
        d = d.view(self.h * self.w, self.ns)
        return torch.where(torch.isnan(d) | torch.isinf(d), torch.zeros_like(d), d)


@pytest.fixture(scope="module")
def cases(renderer, scene256):
    """"frame": a whole 48 x 64 frame (padded: 78 x 94 rays), ns = 12.  "ragged": the cropped window of
    test_plumbing_is_bit_exact, 69 x 85 rays of the 61 x 77 frame -- neither side a multiple of the 8 x 4 block -- with ns = 10, so
    that the last pass carries 2 padding samples.  Each with its plain launch and its launch with all six aux outputs."""
    from scenedreamer_amd import synth
    renderer.set_style(synth.make_style(8888))
    out = {}
    for name, hw, ns, crop in (("frame", (48, 64), 12, 0), ("ragged", (61, 77), 10, renderer.pad // 2 - 4)):
        c = Case(renderer, scene256, hw, ns, crop)
        hit = float((c.crop(c.vid)[:, 0] != 0).float().mean())
        assert 0.2 < hit < 1.0, f"{hit:.2f} of the rays hit the scene: the frame must show both scene and sky"
        c.plain = c.run(renderer)
        c.aux = dict.fromkeys(KEYS)
        c.with_aux = c.run(renderer, aux=c.aux)
        out[name] = c
    assert (out["ragged"].h, out["ragged"].w) == (69, 85)
    assert out["ragged"].win.host(0, out["ragged"].win.n_rays, True)[5] == 2 and out["frame"].win.n_rays == 78 * 94
    return out


def _rowmajor(win):
    """A copy of `win` whose launches take the row-major ray order."""
    from scenedreamer_amd import fused
    w = fused.Window(win.n_src, win.pitch, win.first, win.rows, win.cols)
    w.blocked = lambda *a, **k: False
    assert w.host(0, w.n_rays, True)[5] == 0
    return w


def test_new_entry_without_aux_and_u_is_the_old_launch(renderer, cases):
    """1. sdn_field_render_f32_aux(aux = NULL, u = NULL) == sdn_field_render_f32, on the ragged window (blocked == 2)."""
    from scenedreamer_amd import capi, fused
    c = cases["ragged"]
    R = renderer
    sc = R._fused_scene or fused.prepare_scene(R)
    st = getattr(R, "_fused_style_f32", None) or fused.prepare_style_f32(R)
    n = c.win.n_rays
    lin = fused._lin(R, c.ns)
    ori = np.asarray(c.ori.numpy(), np.float32)
    sky_avg = c.sky_avg.reshape(-1).contiguous()
    out = torch.full((n, 64), float("nan"), device="cuda")
    for aux in (None, ctypes.byref(capi.FieldAux())):        # (a struct with no pointer set selects the same instantiation)
        out.fill_(float("nan"))
        rc = capi.lib().sdn_field_render_f32_aux(c.vid.data_ptr(), c.d2.data_ptr(), c.rd.data_ptr(), sc["lut"].data_ptr(), sc["table3"].data_ptr(),
                                                 sc["T"], sc["scales"].data_ptr(), sc["genc"].ctypes.data, ori.ctypes.data, sc["dims"].ctypes.data,
                                                 lin.data_ptr(), None, n, R.M, c.ns, R.sample_depth, R.dists_scale, st["packed"].data_ptr(),
                                                 st["consts"].data_ptr(), c.sky_c.data_ptr(), sky_avg.data_ptr(), out.data_ptr(), 0,
                                                 c.win.host(0, n, True), None, 0, aux, capi.current_stream(R.dev))
        capi.check(rc, "sdn_field_render_f32_aux")
        assert torch.isfinite(out).all() and torch.equal(out, c.plain)


@pytest.mark.parametrize("name", ["frame", "ragged"])
def test_aux_outputs(renderer, cases, name):
    """2. What the six arrays must be, whatever the MLP computes: depth from the shared placement function, weights a sub-unit
    partition that is zero where nothing is hit, net_out recomposed from them, the sky blend a pure selection."""
    c = cases[name]
    n, ns = c.win.n_rays, c.ns
    a = c.aux
    assert [tuple(a[k].shape) for k in KEYS] == [(n, ns), (n, ns), (n, ns), (n, ns, 64), (n, 64), (n,)] and a["nosky"].dtype == torch.uint8
    assert all(bool(torch.isfinite(a[k].float()).all()) for k in KEYS)
    # another compilation of the same arithmetic (the project's bound for the f16 pair, tests/test_dropin_gpu.py)
    d = float((c.with_aux - c.plain).abs().max())
    print(f"{name}: net_out with aux vs without: max abs {d:.3e}")
    assert d <= 2e-6
    assert torch.equal(a["depth"], c.depth(renderer))
    vid = c.crop(c.vid)
    hit = vid[:, 0] != 0
    w = a["weights"]
    assert float(w[~hit].abs().max()) == 0.0 and bool((w >= 0).all()) and float(w.sum(dim=1).max()) <= 1.0 + 1e-5
    assert int(hit.sum()) > 100 and float(w[hit].sum(dim=1).max()) > 0.05
    skyb, nosky = a["sky_blended"], a["nosky"].bool()
    recomposed = (w[:, :, None] * (a["colour"].clamp(-1, 1) + 1)).sum(dim=1) + (1 - w.sum(dim=1, keepdim=True)) * (skyb.clamp(-1, 1) + 1) - 1
    e = float((recomposed - c.with_aux).abs().max())
    print(f"{name}: net_out recomposed from the per-sample outputs: max abs {e:.3e}")
    assert e <= 1e-5
    sky_c = c.crop(c.sky_c)
    assert 0 < int(nosky.sum()) < n
    assert torch.equal(skyb[nosky], c.sky_avg.reshape(1, 64).expand(int(nosky.sum()), 64)) and torch.equal(skyb[~nosky], sky_c[~nosky])
    assert bool(nosky[vid[:, -1] != 0].all())
    two = {}                 # (an empty dict asks for weights + depth only)
    no2 = c.run(renderer, aux=two)
    assert sorted(two) == ["depth", "weights"] and torch.equal(two["weights"], w) and torch.equal(two["depth"], a["depth"])
    assert torch.equal(no2, c.with_aux)


def test_ray_order_and_window_change_no_bit(renderer, cases):
    """3. out_row, the one index that can go wrong: 8 x 4 blocks (blocked == 2) against row-major over the ragged window, and the
    cropped window against the same pixels of a launch over the whole frame."""
    from scenedreamer_amd import fused
    c = cases["ragged"]
    rm = dict.fromkeys(KEYS)
    no = c.run(renderer, aux=rm, win=_rowmajor(c.win))
    assert torch.equal(no, c.with_aux)
    for k in KEYS:
        assert torch.equal(rm[k], c.aux[k]), k
    whole = dict.fromkeys(KEYS)
    full_win = fused.Window.crop(c.H0, c.W0, 0)
    no = c.run(renderer, aux=whole, win=full_win)
    assert full_win.host(0, full_win.n_rays, True)[5] == 2 and tuple(no.shape) == (c.H0 * c.W0, 64)
    assert torch.equal(c.crop(no), c.with_aux)
    for k in KEYS:
        assert torch.equal(c.crop(whole[k]), c.aux[k]), k


@pytest.mark.parametrize("name", ["frame", "ragged"])
def test_against_the_f16_aux_kernel(renderer, cases, name):
    """4. On weights the f16 stream accepts: what comes from shared device functions and pure selections is the same bits, what
    comes out of the MLP agrees within the tolerance both kernels are held to."""
    from scenedreamer_amd import fused
    c = cases[name]
    f16 = dict.fromkeys(KEYS)
    with torch.no_grad():
        no16 = fused.field_render(renderer, c.vid, c.d2, c.rd, c.ori, c.sky_c, c.sky_avg, c.ns, window=c.win, aux=f16)
    for k in ("depth", "nosky", "sky_blended"):
        assert torch.equal(f16[k], c.aux[k]), k
    ew, en = float((f16["weights"] - c.aux["weights"]).abs().max()), float((no16 - c.with_aux).abs().max())
    print(f"{name}: fp32 AUX vs f16 AUX: weights max abs {ew:.3e}, net_out max abs {en:.3e}")
    assert ew <= TOL and en <= TOL


def _golden_inputs(g):
    M = g["voxel_id"].shape[-2]
    vid = torch.from_numpy(g["voxel_id"]).cuda().reshape(-1, M)
    d2 = torch.from_numpy(g["depth2"]).cuda().reshape(2, -1, M)
    rd = torch.from_numpy(g["raydirs"]).cuda().reshape(-1, 3)
    return vid, d2, rd, torch.from_numpy(g["cam_ori"]), torch.from_numpy(g["sky_avg"]).cuda().reshape(1, 64)


class golden_scene:
    """The renderer with a golden's style code and global_enc, restored on exit."""

    def __init__(self, R, g):
        self.R, self.g = R, g

    def __enter__(self):
        self.z, self.ge = self.R.z, self.R.global_enc
        self.R.set_style_code(self.g["z"])
        self.R.global_enc = torch.from_numpy(self.g["global_enc"]).cuda()
        self.R._fused_scene = None

    def __exit__(self, *exc):
        self.R.set_style_code(self.z)
        self.R.global_enc = self.ge
        self.R._fused_scene = None


def _q99_max(e):
    e = e.flatten()
    return float(e.kthvalue(max(1, int(0.99 * e.numel()))).values), float(e.max())


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_against_reference_goldens(renderer, tag):
    """5. Against what the unmodified reference recorded (CPU run): the weight sums, the sample depths bit for bit, and the density
    per sample in the measure |d| / (1 + |ref|) with the f16 AUX kernel's error on the same golden, in the same run, as yardstick:
    both kernels share the encode stage, so the feature-induced part -- which the density head amplifies -- is common to them and
    the factor 2 covers the MLP's different rounding.
    Measured on one MI355X (profiles/exact_aux_arithmetic.json), fp32 | f16, 0.99 quantile and maximum: field_a 3.03e-5 / 1.49e-4 |
    3.29e-5 / 1.65e-4; field_b 2.93e-5 / 1.38e-4 | 3.04e-5 / 1.40e-4; field_c 1.95e-5 / 1.04e-4 | 2.16e-5 / 1.38e-4 -- the fp32 kernel
    at 0.75 - 0.99 x the f16 kernel's figures.  All four are printed on every run."""
    from scenedreamer_amd import fused
    g = golden(f"field_{tag}.npz")
    vid, d2, rd, ori, sky_avg = _golden_inputs(g)
    ns = int(g["num_samples"])
    n = vid.shape[0]
    with golden_scene(renderer, g), torch.no_grad():
        sky_c = renderer.sky_features(rd)
        a32, a16 = dict.fromkeys(KEYS), dict.fromkeys(KEYS)
        no = fused.field_exact(renderer, vid, d2, rd, ori, sky_c, sky_avg, ns, aux=a32)
        fused.field_render(renderer, vid, d2, rd, ori, sky_c, sky_avg, ns, aux=a16)
    assert float(np.abs(no.cpu().numpy().reshape(g["net_out"].shape) - g["net_out"]).max()) < TOL
    tw = float(np.abs(a32["weights"].sum(dim=1).cpu().numpy() - g["total_weights"].reshape(n)).max())
    print(f"field_{tag}: sum of weights vs total_weights: max abs {tw:.3e}")
    assert tw <= TOL
    # the sampling op reproduces the reference's CPU depths bit for bit (test_sample_depth_op_matches_reference_golden); so must this
    np.testing.assert_array_equal(bits(a32["depth"].cpu().numpy()), bits(g["rand_depth"].reshape(n, ns)))
    ref = torch.from_numpy(g["sigma"].reshape(n, ns)).cuda()
    q32, m32 = _q99_max((a32["sigma"] - ref).abs() / (1 + ref.abs()))
    q16, m16 = _q99_max((a16["sigma"] - ref).abs() / (1 + ref.abs()))
    print("EXACT_AUX_ARITHMETIC " + json.dumps({"golden": f"field_{tag}", "measure": "|sigma - ref| / (1 + |ref|)", "fp32_q99": q32, "fp32_max": m32,
                                                "f16_q99": q16, "f16_max": m16}))
    assert q32 <= 2 * q16 and m32 <= 2 * m16, (q32, q16, m32, m16)


def test_range_beyond_f16_changes_no_bit(renderer, big, cases):
    """6. Range, no tolerance: the weights rescaled by 2^10 / 2^-10 are the same function bit for bit and outside the f16 stream."""
    from scenedreamer_amd import fused
    c = cases["frame"]
    with pytest.raises(fused.TrunkRangeError):
        fused.prepare_style(big)
    fused.prepare_style(renderer)
    b = dict.fromkeys(KEYS)
    no = c.run(big, aux=b)
    assert torch.equal(no, c.with_aux)
    for k in KEYS:
        assert torch.equal(b[k], c.aux[k]), k


def test_stochastic_sampling_against_the_oracle(renderer, weights_full, lut):
    """7a. field_exact(u=) on golden b against the CPU oracle evaluated with the same draw."""
    from oracle import field_ref as FR
    from scenedreamer_amd import fused
    g = golden("field_b.npz")
    hp, wp = g["net_out"].shape[1:3]
    ns = int(g["num_samples"])
    torch.manual_seed(5)
    u = torch.rand([1, hp, wp, ns + 1, 1], dtype=torch.float32)
    orig = FR.sample_depth_batched
    FR.sample_depth_batched = lambda d2, nsamples, sd: orig(d2, nsamples, sd, rand=u)
    try:
        ref = FR.forward_perpix(weights_full, lut, tuple(int(v) for v in renderer.voxel_dims), g["voxel_id"], g["depth2"], g["raydirs"],
                                g["cam_ori"][None], g["z"], g["global_enc"], ns, sky_avg=g["sky_avg"])
    finally:
        FR.sample_depth_batched = orig
    vid, d2, rd, ori, sky_avg = _golden_inputs(g)
    with golden_scene(renderer, g), torch.no_grad():
        sky_c = renderer.sky_features(rd)
        no = fused.field_exact(renderer, vid, d2, rd, ori, sky_c, sky_avg, ns, u=u.reshape(-1, ns + 1).cuda().contiguous())
    err = float(np.abs(no.view(1, hp, wp, 64).cpu().numpy() - ref.numpy()).max())
    det = float(np.abs(ref.numpy() - g["net_out"]).max())
    print(f"stochastic sampling, fp32 kernel vs oracle: max abs err {err:.2e} (stochastic vs deterministic output differs by {det:.2e})")
    assert err < 1e-3 and det > 1e-3


def test_stochastic_depths_and_rows_of_u(renderer, cases):
    """7b. The depths under a draw are the sampling op's for both division forms, and row r of u belongs to pixel r of the window."""
    from scenedreamer_amd import fused
    c = cases["ragged"]
    ns = c.ns
    torch.manual_seed(9)
    u_full = torch.rand(c.H0 * c.W0, ns + 1, device="cuda")
    u = c.crop(u_full).contiguous()
    outs = {}
    for division in ("reciprocal", "ieee"):
        a = dict.fromkeys(KEYS)
        no = c.run(renderer, aux=a, u=u, division=division)
        assert torch.equal(a["depth"], c.depth(renderer, u, division)), division
        outs[division] = (no, a)
    assert not torch.equal(outs["reciprocal"][1]["depth"], c.aux["depth"])
    no, a = outs["reciprocal"]
    whole = dict.fromkeys(KEYS)
    no_w = c.run(renderer, aux=whole, u=u_full, win=fused.Window.crop(c.H0, c.W0, 0))
    assert torch.equal(c.crop(no_w), no)
    for k in KEYS:
        assert torch.equal(c.crop(whole[k]), a[k]), k
    # without aux the draw goes through the plain instantiation: another compilation of the same arithmetic
    assert float((c.run(renderer, u=u) - no).abs().max()) <= 2e-6


# ---- 8. the drop-in route, without the reference's tree ---------------------------------------------------------------------------
def _call_args(c, R):
    """Generator._forward_perpix's arguments for the rays of case `c` (the whole frame)."""
    H0, W0, M = c.H0, c.W0, c.M
    return (None, c.vid.view(1, H0, W0, M, 1), c.d2.view(1, 2, H0, W0, M, 1), c.rd.view(1, H0, W0, 1, 3), c.ori.cuda().reshape(1, 3),
            R.z.reshape(1, -1), R.global_enc.reshape(1, 2))


def test_dropin_exact_route_serves_a_refused_style(big, weights_full, scene256, cases, monkeypatch):
    from perpix_host import PerpixHost, ReferenceMethodCalled
    from scenedreamer_amd import dropin, fused, ops
    monkeypatch.delenv("SDN_PERPIX_EXACT", raising=False)
    c = cases["frame"]
    H0, W0, ns = c.H0, c.W0, c.ns
    G = PerpixHost(_scaled_weights(weights_full, 2.0 ** 10), scene256, ns)
    args = _call_args(c, big)
    b = dropin.binding(G)
    assert b.exact is False
    # the default: the refused style is handed to the reference's method, as before
    with pytest.raises(ReferenceMethodCalled):
        G._forward_perpix(*args)
    assert b.stats["perpix_reference"] == 1 and b.stats["perpix_exact"] == 0 and b.stats["perpix_fast"] == 0
    assert list(b.stats["why"]) == ["trunk weights outside the packed f16 range"]
    # exact="refused": served by the fp32 kernel
    dropin.binding(G, exact="refused")
    before = dict(b.stats)
    out = G._forward_perpix(*args)
    assert b.stats["perpix_exact"] == before["perpix_exact"] + 1 and b.stats["perpix_reference"] == before["perpix_reference"]
    assert b.stats["perpix_fast"] == 0
    assert len(out) == 12 and all(o is None for o in out[1:]) and tuple(out[0].shape) == (1, H0, W0, 64)
    with torch.no_grad():
        sky_c, sky_avg = fused.sky_exact(big, c.rd)
        want = fused.field_exact(big, c.vid, c.d2, c.rd, args[4], sky_c, sky_avg, ns)
        want_aux = dict.fromkeys(KEYS)
        want_a = fused.field_exact(big, c.vid, c.d2, c.rd, args[4], sky_c, sky_avg, ns, aux=want_aux)
    assert torch.equal(out[0].reshape(-1, 64), want)
    # ... with all twelve return values
    dropin.binding(G, aux=True)
    before = dict(b.stats)
    out = G._forward_perpix(*args)
    assert b.stats["perpix_exact"] == before["perpix_exact"] + 1 and b.stats["perpix_reference"] == before["perpix_reference"]
    shapes = dict(zip(dropin.PERPIX_OUTPUTS, ((1, H0, W0, 64), (1, H0, W0, ns, 1), (1, H0, W0, ns, 1), (1, H0, W0, 1, 1), (1, H0, W0, ns, 1),
                                              (1, H0, W0, ns, 1), (1, H0, W0, ns, 64), (1, H0, W0, 1, 64), (1, H0, W0, 1, 1), (1, H0, W0, 1, 1),
                                              (1, H0, W0, 1, 1), (1, H0, W0, ns, 1))))
    assert len(out) == 12 and all(o is not None for o in out)
    assert {k: tuple(o.shape) for k, o in zip(dropin.PERPIX_OUTPUTS, out)} == shapes
    assert torch.equal(out[0].reshape(-1, 64), want_a)
    for i, k in ((2, "weights"), (4, "depth"), (5, "sigma"), (6, "colour"), (7, "sky_blended")):
        assert torch.equal(out[i].reshape(want_aux[k].shape), want_aux[k]), k
    assert torch.equal(out[8].reshape(-1), want_aux["nosky"].float()) and out[11].dtype == torch.int64
    # ... and with the training-time draw: the binding draws like the reference (mc_utils.py:121), the kernel places by it
    G.coarse_deterministic_sampling = False
    torch.manual_seed(21)
    out = G._forward_perpix(*args)
    torch.manual_seed(21)
    u = torch.rand([1, H0, W0, ns + 1, 1], dtype=torch.float32, device="cuda")
    depth, _, _ = ops.sample_depth_batched(args[2], ns + 1, deterministic=False, use_box_boundaries=False, sample_depth=G.sample_depth, rand=u)
    depth = torch.where(torch.isnan(depth) | torch.isinf(depth), torch.zeros_like(depth), depth)
    assert torch.equal(out[4], depth) and not torch.equal(out[4].reshape(-1, ns), want_aux["depth"])
    assert b.stats["perpix_exact"] == before["perpix_exact"] + 2 and b.stats["perpix_reference"] == before["perpix_reference"]


def test_dropin_exact_true_serves_every_style(renderer, weights_full, scene256, cases, monkeypatch):
    from perpix_host import PerpixHost
    from scenedreamer_amd import dropin, synth
    monkeypatch.delenv("SDN_PERPIX_EXACT", raising=False)
    renderer.set_style(synth.make_style(8888))
    c = cases["frame"]
    G = PerpixHost(weights_full, scene256, c.ns)
    args = _call_args(c, renderer)
    b = dropin.binding(G)
    fast = G._forward_perpix(*args)[0]
    assert b.stats["perpix_fast"] == 1 and b.stats["perpix_exact"] == 0
    dropin.binding(G, exact=True)
    exact = G._forward_perpix(*args)[0]
    assert b.stats["perpix_fast"] == 1 and b.stats["perpix_exact"] == 1 and b.stats["perpix_reference"] == 0
    e = float((exact - fast).abs().max())
    print(f"binding exact=True vs the fast route on in-range weights: net_out max abs {e:.3e}")
    assert tuple(exact.shape) == (1, c.H0, c.W0, 64) and e <= TOL and not torch.equal(exact, fast)


def test_dropin_exact_route_tiles_in_place_and_coalesced(big, weights_full, scene256, cases, monkeypatch):
    """A tile of a frame whose sky pre-pass is at hand (scenedreamer.py:592-616): the exact route evaluates the frame once through
    device addresses + a window (frame_field), or -- coalesce off -- the tile in place; both are the tile's pixels of field_exact
    on the whole frame."""
    from perpix_host import PerpixHost
    from scenedreamer_amd import dropin, fused, ops
    monkeypatch.delenv("SDN_PERPIX_EXACT", raising=False)
    c = cases["frame"]
    H0, W0, ns = c.H0, c.W0, c.ns
    G = PerpixHost(_scaled_weights(weights_full, 2.0 ** 10), scene256, ns)
    _, vid, d2, rd, cam, z, ge = _call_args(c, big)
    with torch.no_grad():        # the frame-wide sky pre-pass of inference_givenstyle
        sky_in = ops.positional_encoding(rd.expand(-1, -1, -1, 1, -1).contiguous(), 5, -1, True)
        G.sky_avg = torch.mean(G.sky_net(sky_in, z), dim=[1, 2], keepdim=True)
    last = G.sky_net.__dict__["_sdn_last_frame"]
    with torch.no_grad():
        want = fused.field_exact(big, c.vid, c.d2, c.rd, cam, last["sky_c"], G.sky_avg, ns, window=fused.Window.crop(H0, W0, 0))
        # (device addresses + a window are the tensors' own launch)
        addr = fused.field_exact(big, c.vid.data_ptr(), c.d2.data_ptr(), c.rd.data_ptr(), cam, last["sky_c"].data_ptr(), G.sky_avg, ns,
                                 window=fused.Window.crop(H0, W0, 0))
    assert torch.equal(addr, want)
    want = want.view(H0, W0, 64)
    b = dropin.binding(G, exact="refused")
    y0, x0, h, w = 5, 7, 40, 50
    tile = (None, vid[:, y0:y0 + h, x0:x0 + w], d2[:, :, y0:y0 + h, x0:x0 + w], rd[:, y0:y0 + h, x0:x0 + w], cam, z, ge)
    out = G._forward_perpix(*tile)
    assert b.stats["perpix_exact"] == 1 and b.stats["frames_coalesced"] == 1 and b.stats["tiles_from_frame"] == 1 and b.stats["tiles_in_place"] == 1
    assert tuple(out[0].shape) == (1, h, w, 64) and torch.equal(out[0][0], want[y0:y0 + h, x0:x0 + w])
    out = G._forward_perpix(*tile)        # the frame's next tile is a view of the same evaluation
    assert b.stats["frames_coalesced"] == 1 and b.stats["tiles_from_frame"] == 2 and torch.equal(out[0][0], want[y0:y0 + h, x0:x0 + w])
    b.coalesce = False
    out = G._forward_perpix(*tile)
    assert b.stats["perpix_exact"] == 3 and b.stats["tiles_in_place"] == 3 and b.stats["tiles_from_frame"] == 2 and b.stats["tiles_copied"] == 0
    assert b.stats["perpix_reference"] == 0 and torch.equal(out[0][0], want[y0:y0 + h, x0:x0 + w])
