"""The fp32 field rung on the MI355X (csrc/field_f32.hip: sdn_field_render_f32 / sdn_render_mlp_f32, fused.field_exact,
Renderer mode "exact", Renderer.fallback, LightningMLPNative.sdn_exact): arithmetic against fp64, range with no tolerance,
parity with the reference goldens and the CPU oracle, bit-exact plumbing, the fallback switch, the module surface."""
import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

TOL = 1e-3          # the tolerance of tests/test_render_gpu.py
HW, NS = (72, 104), 24


@pytest.fixture(scope="module")
def renderer(weights_full, scene256):
    from scenedreamer_amd import synth
    from scenedreamer_amd.renderer import Renderer
    r = Renderer(weights_full, scene256, "cuda")
    r.set_style(synth.make_style(8888))
    return r


def _pose(scene256, i):
    from scenedreamer_amd import camera
    return camera.eval_camera_poses(scene256, maxstep=8)[i]


def _inputs(g, dev="cuda"):
    M = g["voxel_id"].shape[-2]
    vid = torch.from_numpy(g["voxel_id"]).to(dev).reshape(-1, M)
    d2 = torch.from_numpy(g["depth2"]).to(dev).reshape(2, -1, M)
    rd = torch.from_numpy(g["raydirs"]).to(dev).reshape(-1, 3)
    ori = torch.from_numpy(g["cam_ori"]).to(dev)
    sky_avg = torch.from_numpy(g["sky_avg"]).to(dev).reshape(1, 64)
    return vid, d2, rd, ori, sky_avg


def _golden_mlp_case(tag, weights_full, scene256, lut):
    """Features / labels of golden `tag` from the CPU oracle, fp64 truth and the reference's own fp32 arithmetic on them."""
    from oracle import field_ref as FR
    g = golden(f"field_{tag}.npz")
    _, aux = FR.forward_perpix(weights_full, lut, scene256.voxel_t.shape, g["voxel_id"], g["depth2"], g["raydirs"],
                               g["cam_ori"][None], g["z"], g["global_enc"], int(g["num_samples"]), sky_avg=g["sky_avg"], return_aux=True)
    x = aux["feature_in"].to(torch.float32)                                   # [1,h,w,ns,128]
    reduced = torch.as_tensor(lut, dtype=torch.long)[torch.as_tensor(g["voxel_id"]).long()]
    reduced[reduced == 0] = 3
    lab = torch.gather(reduced, -2, aux["new_idx"]).long()                    # [1,h,w,ns,1]
    onehot = torch.zeros(list(lab.shape[:-1]) + [12], dtype=torch.float32)
    onehot.scatter_(-1, lab, 1.0)
    z = torch.as_tensor(g["z"], dtype=torch.float32)
    s64, c64 = FR.render_mlp(weights_full, x.double(), z.double(), onehot.double(), dtype=torch.float64)
    s32, c32 = FR.render_mlp(weights_full, x, z, onehot, dtype=torch.float32)
    return g, x, lab.reshape(-1).to(torch.uint8), onehot, (s64.reshape(-1), c64.reshape(-1, 64)), (s32.reshape(-1), c32.reshape(-1, 64))


def _check_against_fp64(name, sigma, c, truth, yard):
    """Condition 1: max |new - fp64| <= 4 x max |reference fp32 - fp64|, separately for sigma and c."""
    for what, new, t, y in (("sigma", sigma, truth[0], yard[0]), ("c", c, truth[1], yard[1])):
        e_new = float((new.double().cpu() - t).abs().max())
        e_ref = float((y.double() - t).abs().max())
        print(f"{name} {what}: fp32 MFMA kernel vs fp64 {e_new:.3e}; reference fp32 (CPU) vs fp64 {e_ref:.3e}; ratio {e_new / e_ref:.2f}")
        assert e_new <= 4 * e_ref, (name, what, e_new, e_ref)


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_raw_mlp_is_fp32_accurate(renderer, weights_full, scene256, lut, tag):
    """1. The arithmetic, isolated: sdn_render_mlp_f32 on the goldens' features against an fp64 evaluation, measured in units of
    the error of the reference's own fp32 arithmetic (the CPU's BLAS).  The MFMA is a strictly sequential 256-term fmaf chain, BLAS
    sums in blocks: a sequential chain emulated on the CPU gave 1.0 - 1.8 x the BLAS error on these inputs, so the bound is 4 x --
    a single plain f16 operand anywhere in the trunk is 2^13 times coarser."""
    from scenedreamer_amd import fused
    g, x, lab, _, truth, yard = _golden_mlp_case(tag, weights_full, scene256, lut)
    renderer.set_style_code(g["z"])
    sigma, c = fused.render_mlp_exact(renderer, x.reshape(-1, 128).cuda(), lab.cuda())
    _check_against_fp64(f"field_{tag}", sigma, c, truth, yard)


def _scaled_weights(weights_full, g):
    w = dict(weights_full)
    for k in ("render_net.fc_1.weight", "render_net.fc_1.bias", "render_net.fc_m_a.weight"):
        w[k] = torch.as_tensor(np.asarray(w[k])) * g
    w["render_net.fc_2.weight"] = torch.as_tensor(np.asarray(w["render_net.fc_2.weight"])) * (1.0 / g)
    return w


def test_range_beyond_f16_is_bit_exact(renderer, weights_full, scene256, lut):
    """2. Range, with no tolerance.  LeakyReLU is positively homogeneous and a power of two scales fp32 exactly: fc_1 (weight,
    bias, fc_m_a) x 2^10 and fc_2.weight x 2^-10 are the same function bit for bit.  The f16 stream refuses those weights
    (TrunkRangeError); the fp32 kernel must render the same bits as with the original ones -- which no f16-operand kernel can."""
    from scenedreamer_amd import fused, synth
    from scenedreamer_amd.renderer import Renderer
    G = 2.0 ** 10
    big = Renderer(_scaled_weights(weights_full, G), scene256, "cuda")
    big.set_style(synth.make_style(8888))
    renderer.set_style(synth.make_style(8888))
    with pytest.raises(fused.TrunkRangeError):
        fused.prepare_style(big)
    fused.prepare_style(renderer)           # ... while the original weights are inside the f16 stream's range
    pose = _pose(scene256, 5)
    vid = renderer.cast_rays(pose, HW)[0]
    hit = float((vid.reshape(-1, renderer.M)[:, 0] != 0).float().mean())
    assert hit > 0.2, f"only {hit:.2f} of the rays hit the scene: the frame shows nothing"
    a = renderer.render_frame(pose, HW, NS, mode="exact", cnn=False)
    b = big.render_frame(pose, HW, NS, mode="exact", cnn=False)
    assert a.shape == b.shape and torch.isfinite(a).all()
    assert torch.equal(a, b)
    # the same for the MLP as an op, on the features of a golden
    g, x, lab, *_ = _golden_mlp_case("a", weights_full, scene256, lut)
    renderer.set_style_code(g["z"])
    big.set_style_code(g["z"])
    xs, ls = x.reshape(-1, 128).cuda(), lab.cuda()
    s0, c0 = fused.render_mlp_exact(renderer, xs, ls)
    s1, c1 = fused.render_mlp_exact(big, xs, ls)
    assert torch.equal(s0, s1) and torch.equal(c0, c1)


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_field_exact_matches_reference_golden(renderer, tag):
    """3a. field_exact on the goldens recorded from the unmodified reference: net_out and, through render_cnn, the image."""
    from scenedreamer_amd import fused
    g = golden(f"field_{tag}.npz")
    vid, d2, rd, ori, sky_avg = _inputs(g)
    ns = int(g["num_samples"])
    renderer.set_style_code(g["z"])
    ge = renderer.global_enc
    try:
        renderer.global_enc = torch.from_numpy(g["global_enc"]).cuda()
        renderer._fused_scene = None
        with torch.no_grad():
            sky_c = renderer.sky_features(rd)
            no = fused.field_exact(renderer, vid, d2, rd, ori, sky_c, sky_avg, ns)
            hp, wp = g["net_out"].shape[1:3]
            no = no.view(1, hp, wp, 64)
            img = renderer.render_cnn(no)
    finally:
        renderer.global_enc = ge
        renderer._fused_scene = None
    err = np.abs(no.cpu().numpy() - g["net_out"])
    ierr = np.abs(img.cpu().numpy() - g["image"])
    print(f"field_{tag}: net_out max abs err {err.max():.3e}, image max abs err {ierr.max():.3e}")
    assert err.max() < TOL, f"net_out max abs err {err.max():.3e}"
    assert ierr.max() < TOL, f"image max abs err {ierr.max():.3e}"


def test_field_exact_vs_fp32_op_sequence(renderer, scene256):
    """3b. On a rendered frame: field_exact against the fp32 op sequence with the kernel's sample placement (calibrate_one's twin),
    inside the bound the fused path is held to."""
    from scenedreamer_amd import fused, synth
    from scenedreamer_amd import renderer as rmod
    renderer.set_style(synth.make_style(8888))
    pose = _pose(scene256, 5)
    with torch.no_grad():
        vid, d2, rd, cam_res = renderer.cast_rays(pose, HW)
        n = cam_res[0] * cam_res[1]
        vid, d2, rd = vid.view(n, renderer.M), d2.view(2, n, renderer.M), rd.view(n, 3)
        sky_c = renderer.sky_features(rd)
        sky_avg = sky_c.mean(dim=0, keepdim=True)
        ori = torch.as_tensor(pose[0], dtype=torch.float32)
        a = fused.field_exact(renderer, vid, d2, rd, ori, sky_c, sky_avg, NS)
        b = renderer.field_unfused(vid, d2, rd, ori.cuda(), sky_c, sky_avg, NS, placement="kernel")
    err = float((a - b).abs().max())
    print(f"field_exact vs field_unfused(placement='kernel'): max abs {err:.3e} over {a.numel()} values")
    assert err <= rmod.FIELD_AUTO_BOUND


def test_full_frame_equals_reference_tiling(renderer, weights_full, scene256, lut):
    """4. A whole frame in mode "exact" against the reference's tile loop evaluated by the CPU oracle."""
    from oracle import field_ref as FR
    from scenedreamer_amd import synth
    renderer.set_style(synth.make_style(8888))
    pose = _pose(scene256, 2)
    hw = (140, 150)
    img = renderer.render_frame(pose, hw, 12, mode="exact")
    ref = FR.render_frame_tiled(weights_full, lut, scene256.voxel_t.numpy(), (pose[0].numpy(), pose[1].numpy(), pose[2].numpy(), pose[3]),
                                hw, 12, renderer.z.cpu().numpy(), renderer.global_enc.cpu().numpy())
    assert tuple(img.shape) == (1, 3, 140, 150)
    err = np.abs(img.cpu().numpy() - ref.numpy())
    print(f"mode='exact' frame vs CPU oracle: image max abs err {err.max():.3e}")
    assert err.max() < TOL, f"image max abs err {err.max():.3e}"


def test_plumbing_is_bit_exact(renderer, scene256):
    """5. Trajectory loop == single frames, calls repeat, the minimal apron is the inner window of the reference apron, and the
    8 x 4-block ray order equals the row-major one on a window whose sides are not multiples of 8 / 4."""
    from scenedreamer_amd import fused, synth
    renderer.set_style(synth.make_style(8888))
    p = _pose(scene256, 5)
    one = renderer.render_frame(p, HW, NS, mode="exact")
    assert tuple(one.shape) == (1, 3) + HW
    assert torch.equal(one, renderer.render_frame(p, HW, NS, mode="exact"))
    frames = list(renderer.render_frames([p, p], HW, NS, mode="exact"))
    assert len(frames) == 2 and all(torch.equal(f, one) for f in frames)
    # apron: the comparison stops in front of the PyTorch CNN (its algorithm choice may depend on the image size)
    hw = (61, 77)
    a = renderer.render_frame(p, hw, 12, mode="exact", cnn=False, apron="minimal")
    b = renderer.render_frame(p, hw, 12, mode="exact", cnn=False, apron="reference")
    o = (b.shape[1] - a.shape[1]) // 2
    assert o == renderer.pad // 2 - 4 and a.shape[1] == hw[0] + 8 and a.shape[2] == hw[1] + 8
    assert a.shape[1] % 4 != 0 and a.shape[2] % 8 != 0           # a ragged window for the blocked order
    assert torch.equal(a, b[:, o:-o, o:-o])
    # blocked 2 (what field_exact passes) vs row-major (blocked 0) over the same window
    with torch.no_grad():
        vid, d2, rd, cam_res = renderer.cast_rays(p, hw)
        n = cam_res[0] * cam_res[1]
        vid, d2, rd = vid.view(n, renderer.M), d2.view(2, n, renderer.M), rd.view(n, 3)
        sky_c = renderer.sky_features(rd)
        sky_avg = sky_c.mean(dim=0, keepdim=True)
        win = fused.Window.crop(cam_res[0], cam_res[1], o)
        ori = torch.as_tensor(p[0], dtype=torch.float32)
        blocked = fused.field_exact(renderer, vid, d2, rd, ori, sky_c, sky_avg, 12, window=win)
        assert win.host(0, win.n_rays, True)[5] == 2
        try:
            win.blocked = lambda *a_, **k_: False
            assert win.host(0, win.n_rays, True)[5] == 0
            rowmajor = fused.field_exact(renderer, vid, d2, rd, ori, sky_c, sky_avg, 12, window=win)
        finally:
            del win.blocked
    assert torch.equal(blocked, rowmajor)
    assert torch.equal(blocked.view(a.shape), a)


def test_fallback_switch(weights_full, scene256, monkeypatch):
    """6. Renderer.fallback decides what a closed gate selects; the default is unchanged."""
    from scenedreamer_amd import synth
    from scenedreamer_amd import renderer as rmod
    from scenedreamer_amd.renderer import Renderer
    monkeypatch.setattr(rmod, "FIELD_AUTO_BOUND", 1e-9)
    p = _pose(scene256, 5)
    hw = (48, 64)
    R = Renderer(weights_full, scene256, "cuda")
    R.set_style(synth.make_style(8888))
    R.fallback = "exact"
    img = R.render_frame(p, hw, 12, mode="fused")
    assert R.field_gate["path"] == "exact" and R.field_falls_back()
    assert torch.equal(img, R.render_frame(p, hw, 12, mode="exact"))
    assert all(torch.equal(f, img) for f in R.render_frames([p, p], hw, 12, mode="fused"))
    D = Renderer(weights_full, scene256, "cuda")
    D.set_style(synth.make_style(8888))
    img = D.render_frame(p, hw, 12, mode="fused")
    assert D.field_gate["path"] == "unfused" and D.field_falls_back()
    assert torch.equal(img, D.render_frame(p, hw, 12, mode="unfused"))


def test_module_surface(weights_full, scene256, lut):
    """7. LightningMLPNative with sdn_exact: the call is served by sdn_render_mlp_f32 (same bits as the direct call) and meets
    condition 1; with the option set a style outside the f16 stream's range is served natively too."""
    from scenedreamer_amd import fused
    from scenedreamer_amd.renderer import Renderer
    g, x, lab, onehot, truth, yard = _golden_mlp_case("b", weights_full, scene256, lut)
    net = _native_render_net(weights_full)
    z = torch.as_tensor(g["z"], dtype=torch.float32).cuda().reshape(1, -1)
    net.sdn_exact = True
    sigma, c = net(x.cuda(), None, z, onehot.cuda())
    assert net.__dict__.get("_sdn_composite_reason") is None
    R = Renderer(weights_full, scene256, "cuda")
    R.set_style_code(g["z"])
    s0, c0 = fused.render_mlp_exact(R, x.reshape(-1, 128).cuda(), lab.cuda())
    assert torch.equal(sigma.reshape(-1), s0) and torch.equal(c.reshape(-1, 64), c0)
    _check_against_fp64("module field_b", sigma.reshape(-1), c.reshape(-1, 64), truth, yard)
    # out-of-range weights: natively, not by _forward_composite
    big = _native_render_net(_scaled_weights(weights_full, 2.0 ** 10))
    big.sdn_exact = True
    s1, c1 = big(x.cuda(), None, z, onehot.cuda())
    assert big.__dict__.get("_sdn_composite_reason") is None
    assert torch.equal(s1.reshape(-1), s0) and torch.equal(c1.reshape(-1, 64), c0)


def _native_render_net(weights):
    """modules.LightningMLP (the reference's constructor and parameters, this package's native forward) loaded with `weights`."""
    from scenedreamer_amd import modules
    net = modules.LightningMLP(128, 256, 0, mask_dim=12, out_channels_s=1, out_channels_c=64)
    pre = "render_net."
    net.load_state_dict({k[len(pre):]: torch.as_tensor(np.asarray(v)) for k, v in weights.items() if k.startswith(pre)})
    net = net.cuda().eval()
    for p in net.parameters():
        p.requires_grad_(False)
    return net
