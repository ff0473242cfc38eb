"""The fp32 sky MLP on the MI355X (csrc/sky_f32.hip: sdn_sky_mlp_f32, fused.sky_exact, Renderer.exact_sky, SKYMLPNative.sdn_exact):
the arithmetic against fp64 in units of the error E32 of the reference's own fp32 arithmetic (tests/field_layout.py: 4 x E32;
tests/test_sky_f32_cpu.py qualifies the summation order that bound asks for), the frame mean against its own bound
(tests/sky_f32_ref.py), both input forms, ragged sizes and the grid-stride loop, fp32's range with no tolerance, frames, and the
module surface.  Every arithmetic check prints its kernel/E32 ratio; SDN_ARITH_RECORD=<file> collects them as JSON."""
import types

import numpy as np
import pytest
import torch

import field_layout as FL
import sky_f32_ref as SF

pytestmark = pytest.mark.gpu

RECORD = FL.RECORD
_record_file = FL.record_file_fixture()
TOL = 1e-3          # the tolerance of tests/test_exact_rung_gpu.py
HW, NS = (72, 104), 24
SIZES = (1, 31, 32, 33, 127, 129, 1001)


@pytest.fixture(scope="module")
def renderer(weights_full, scene256):
    from scenedreamer_amd.renderer import Renderer
    r = Renderer(weights_full, scene256, "cuda")
    r.set_style_code(FL.style_code())
    return r


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    for k in ("SDN_EXACT_SKY", "SDN_SKY_EXACT", "SDN_EXACT_CNN"):
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def dirs():
    return FL.sky_dirs().cuda()


@pytest.fixture(scope="module")
def full(renderer, dirs):
    """fused.sky_exact on the 1001 directions, once: (sky_c, sky_avg)."""
    from scenedreamer_amd import fused
    renderer.set_style_code(FL.style_code())
    c, a = fused.sky_exact(renderer, dirs)
    torch.cuda.synchronize()
    return c.clone(), a.clone()


def _pose(scene256, i):
    from scenedreamer_amd import camera
    return camera.eval_camera_poses(scene256, maxstep=8)[i]


# ----------------------------------------------------------------------------------------------------- arithmetic

@pytest.mark.parametrize("encoded", [0, 1])
def test_sky_exact_against_fp64(renderer, weights_full, dirs, encoded):
    """1. fused.sky_exact on the 1001 unit directions, the encoding evaluated inside the kernel (encoded = 0) or handed in as the CPU
    oracle's rows (encoded = 1): sky_c within 4 x E32 of SKYMLP in fp64 on the oracle's encoding; sky_avg within 8 u mean|x| of the
    f64 mean of the kernel's own sky_c."""
    from oracle import split_ref as SR
    from scenedreamer_amd import fused
    renderer.set_style_code(FL.style_code())
    pe = FL.sky_encoded(FL.sky_dirs())
    z = renderer.z.cpu().numpy()
    truth = SR.sky_mlp_ref(weights_full, pe, z, torch.float64)
    yard = SR.sky_mlp_ref(weights_full, pe, z, torch.float32)
    sky_c, avg = fused.sky_exact(renderer, pe.cuda() if encoded else dirs, encoded=bool(encoded))
    torch.cuda.synchronize()
    assert tuple(sky_c.shape) == (1001, 64) and tuple(avg.shape) == (1, 64) and torch.isfinite(sky_c).all()
    FL.check_fp32(f"sdn_sky_mlp_f32 sky_c, encoded={encoded}", sky_c.cpu(), truth, yard)
    worst = SF.check_mean(avg.cpu(), sky_c.cpu())
    e = FL.max_err(avg.reshape(-1).cpu(), truth.mean(dim=0))
    e32 = FL.max_err(yard.mean(dim=0), truth.mean(dim=0))
    RECORD[f"sdn_sky_mlp_f32 sky_avg, encoded={encoded}"] = dict(kernel=e, E32=e32, kernel_over_E32=e / e32, fraction_of_mean_bound=worst)
    print(f"{'sdn_sky_mlp_f32 sky_avg, encoded=%d' % encoded:72s} kernel {e:.2e}  E32 {e32:.2e}  kernel/E32 {e / e32:5.2f}  "
          f"vs its own f64 mean: {worst:.3f} of 8 u mean|x|")


def test_both_input_forms_give_the_same_bits(renderer, dirs, full):
    """2. Ray directions encoded inside the kernel == the rows of ops.positional_encoding handed in."""
    from scenedreamer_amd import fused, ops
    renderer.set_style_code(FL.style_code())
    pe = ops.positional_encoding(dirs, 5, -1, True)
    assert tuple(pe.shape) == (1001, 33)
    c1, a1 = fused.sky_exact(renderer, pe, encoded=True)
    assert torch.equal(full[0], c1) and torch.equal(full[1], a1)


# ----------------------------------------------------------------------------------------------------- sizes, grid, guard, counter

def _launch(R, rd, n_workgroups=0, counter=None):
    """sdn_sky_mlp_f32 through the C entry on rd [n,3]: sky_c with 64 guard floats behind row n - 1, sky_avg."""
    from scenedreamer_amd import capi, fused
    lib = capi.lib()
    sk = getattr(R, "_fused_sky_f32", None) or fused.prepare_sky_exact(R)
    n = rd.shape[0]
    buf = torch.full((n * 64 + 64,), float("nan"), device=R.dev)
    part = torch.empty((lib.sdn_sky_f32_partial_rows(n, n_workgroups), 64), dtype=torch.float64, device=R.dev)
    avg = torch.full((64,), float("nan"), device=R.dev)
    rc = lib.sdn_sky_mlp_f32(rd.data_ptr(), sk["packed"].data_ptr(), sk["consts"].data_ptr(), buf.data_ptr(), part.data_ptr(), n, n_workgroups,
                             avg.data_ptr(), counter.data_ptr(), 0, capi.current_stream(R.dev))
    capi.check(rc, "sdn_sky_mlp_f32")
    torch.cuda.synchronize()
    assert torch.isnan(buf[n * 64:]).all(), "the floats behind the last row were written"
    return buf[:n * 64].view(n, 64), avg


@pytest.mark.parametrize("n,wg", [(n, 0) for n in SIZES] + [(1001, 2)], ids=lambda v: str(v))
def test_ragged_sizes_and_the_grid_stride_loop(renderer, dirs, full, n, wg):
    """3. A ray's features depend on its direction only: row r of a launch over the first n directions equals, bit for bit, row r of
    the 1001-ray launch -- for one ray, a ragged tile, a whole tile, a tile and one ray, ragged 128-ray groups, and 1001 rays on TWO
    workgroups (8 groups: four trips through the group loop each).  Nothing is written behind row n - 1, sky_avg is within its bound
    of the launch's own f64 mean, and a second launch on the same counter gives the same bits (the kernel resets it)."""
    renderer.set_style_code(FL.style_code())
    rd = dirs[:n].contiguous()
    counter = torch.zeros(1, dtype=torch.int32, device=renderer.dev)
    c, a = _launch(renderer, rd, wg, counter)
    assert torch.equal(c, full[0][:n])
    assert torch.isfinite(a).all()
    SF.check_mean(a.cpu(), c.cpu())
    assert int(counter) == 0
    c2, a2 = _launch(renderer, rd, wg, counter)
    assert torch.equal(c, c2) and torch.equal(a, a2)
    if n == 1001:
        # the launch shape is a schedule: the mean of 2 workgroups' rows and of 8 workgroups' rows agree to the f64 sums' rounding
        assert float((a - full[1].reshape(-1)).abs().max()) <= float(SF.mean_bound(c.cpu()).max())


# ----------------------------------------------------------------------------------------------------- range

def _scaled(w, g):
    out = dict(w)
    for k in ("sky_net.fc1.weight", "sky_net.fc1.bias", "sky_net.fc_z_a.weight"):
        out[k] = w[k] * g
    out["sky_net.fc2.weight"] = w["sky_net.fc2.weight"] * (1.0 / g)
    return out


def test_range_beyond_f16_is_bit_exact(renderer, dirs, full):
    """4. Range, with no tolerance.  LeakyReLU is positively homogeneous and a power of two scales fp32 exactly: fc1 (weight, bias,
    fc_z_a) x 2^10 and fc2.weight x 2^-10 are the same function bit for bit.  The f16 stream refuses those weights (TrunkRangeError:
    max|fc1.weight| = 0.827 here, times 2^18 far beyond 65504) and accepts the original ones; the fp32 kernel returns the same bits
    for both sets."""
    from scenedreamer_amd import fused
    from scenedreamer_amd.renderer import fold_sky_net
    renderer.set_style_code(FL.style_code())
    big = types.SimpleNamespace(w=_scaled(renderer.w, 2.0 ** 10), dev=renderer.dev)
    fold_sky_net(big, renderer.z)
    assert float(big.w["sky_net.fc1.weight"].abs().max()) * 2.0 ** 8 > 65504
    with pytest.raises(fused.TrunkRangeError):
        fused.prepare_sky(big)
    fused.prepare_sky(renderer)           # ... while the original weights are inside the f16 stream's range
    c, a = fused.sky_exact(big, dirs)
    assert torch.isfinite(c).all() and float(c.abs().max()) > 0
    assert torch.equal(c, full[0]) and torch.equal(a, full[1])


# ----------------------------------------------------------------------------------------------------- frames

@pytest.fixture(scope="module")
def frame_renderer(weights_full, scene256):
    from scenedreamer_amd import synth
    from scenedreamer_amd.renderer import Renderer
    r = Renderer(weights_full, scene256, "cuda")
    r.set_style(synth.make_style(8888))
    return r


def test_frames_with_the_f32_sky(frame_renderer, scene256):
    """5a. render_frame(mode="exact") with exact_sky = "f32": finite, repeats bit for bit, equals the trajectory loop's frames; its
    sky is fused.sky_exact's; with the attribute unset -- and on "unfused" whatever it is -- the tensors are what they were."""
    from scenedreamer_amd import fused
    R = frame_renderer
    p = _pose(scene256, 5)
    assert R.exact_sky is None
    default = R.render_frame(p, HW, NS, mode="exact")
    unfused = R.render_frame(p, HW, NS, mode="unfused")
    no_default = R.render_frame(p, HW, NS, mode="exact", cnn=False)
    R.exact_sky = "f32"
    try:
        one = R.render_frame(p, HW, NS, mode="exact")
        assert tuple(one.shape) == (1, 3) + HW and torch.isfinite(one).all()
        assert torch.equal(one, R.render_frame(p, HW, NS, mode="exact"))
        frames = list(R.render_frames([p, p], HW, NS, mode="exact"))
        assert len(frames) == 2 and all(torch.equal(f, one) for f in frames)
        # the frame IS the field on sky_exact's features
        no = R.render_frame(p, HW, NS, mode="exact", cnn=False)
        with torch.no_grad():
            vid, d2, rd, (Hp, Wp) = R.cast_rays(p, HW)
            n = Hp * Wp
            vid, d2, rd = vid.view(n, R.M), d2.view(2, n, R.M), rd.view(n, 3)
            sky_c, sky_avg = fused.sky_exact(R, rd)
            o = R.pad // 2 - 4
            byhand = fused.field_exact(R, vid, d2, rd, torch.as_tensor(p[0], dtype=torch.float32), sky_c, sky_avg, NS,
                                       window=fused.Window.crop(Hp, Wp, o))
        assert torch.equal(no.reshape(-1, 64), byhand)
        assert not torch.equal(no, no_default)          # (two summation orders: the kernel did run)
        assert float((no - no_default).abs().max()) < 1e-4
        assert torch.equal(unfused, R.render_frame(p, HW, NS, mode="unfused"))          # "unfused" stays on PyTorch
        assert "sky MLP: f32-input MFMA" in R.compute_dtype("exact")
    finally:
        R.exact_sky = None
    assert torch.equal(default, R.render_frame(p, HW, NS, mode="exact"))
    assert torch.equal(no_default, R.render_frame(p, HW, NS, mode="exact", cnn=False))
    R.exact_sky = "fast"
    try:
        with pytest.raises(ValueError, match="exact_sky"):
            R.render_frame(p, HW, NS, mode="exact")
    finally:
        R.exact_sky = None


def test_full_frame_equals_reference_tiling(frame_renderer, weights_full, scene256, lut):
    """5b. A whole (140, 150) frame at 12 samples in mode "exact" with the fp32 sky against the reference's tile loop evaluated by the
    CPU oracle: tolerance and case of tests/test_exact_rung_gpu.py."""
    from oracle import field_ref as FR
    R = frame_renderer
    pose = _pose(scene256, 2)
    hw = (140, 150)
    R.exact_sky = "f32"
    try:
        img = R.render_frame(pose, hw, 12, mode="exact")
    finally:
        R.exact_sky = None
    ref = FR.render_frame_tiled(weights_full, lut, scene256.voxel_t.numpy(), (pose[0].numpy(), pose[1].numpy(), pose[2].numpy(), pose[3]),
                                hw, 12, R.z.cpu().numpy(), R.global_enc.cpu().numpy())
    assert tuple(img.shape) == (1, 3, 140, 150)
    err = np.abs(img.cpu().numpy() - ref.numpy())
    print(f"mode='exact', exact_sky='f32' frame vs CPU oracle: image max abs err {err.max():.3e}")
    assert err.max() < TOL, f"image max abs err {err.max():.3e}"


def test_whole_frame_native_equals_a_window_of_itself(frame_renderer, scene256):
    """5c. exact_sky = "f32" and exact_cnn = "f32": no PyTorch network op in the frame.  The image is F32CNN on the frame's net_out,
    and a window of that net_out gives the same image bits 4 pixels in from its edges (the CNN's own position test, on a frame)."""
    R = frame_renderer
    p = _pose(scene256, 5)
    R.exact_sky, R.exact_cnn = "f32", "f32"
    try:
        img = R.render_frame(p, HW, NS, mode="exact")
        no = R.render_frame(p, HW, NS, mode="exact", cnn=False)
        s = R.compute_dtype("exact")
    finally:
        R.exact_sky = R.exact_cnn = None
    assert "PyTorch" not in s
    assert tuple(no.shape) == (1, HW[0] + 8, HW[1] + 8, 64)
    cnn = R.f32_cnn()
    whole = cnn(no)
    assert torch.equal(img, whole[:, :, 4:-4, 4:-4])
    sub = cnn(no[:, 5:67, 7:98].contiguous())
    assert torch.equal(whole[:, :, 9:63, 11:94], sub[:, :, 4:-4, 4:-4])


def test_closed_gate_with_fallback_exact_takes_the_f32_sky(weights_full, scene256, monkeypatch):
    """5d. fallback = "exact", exact_sky = "f32" and a closed field gate (forced as in tests/test_exact_rung_gpu.py): the frame is the
    exact path's with the fp32 sky kernel; with fallback "unfused" the attribute changes nothing."""
    from scenedreamer_amd import synth
    from scenedreamer_amd import renderer as rmod
    from scenedreamer_amd.renderer import Renderer
    monkeypatch.setattr(rmod, "FIELD_AUTO_BOUND", 1e-9)
    p = _pose(scene256, 5)
    hw = (48, 64)
    R = Renderer(weights_full, scene256, "cuda")
    R.set_style(synth.make_style(8888))
    R.fallback, R.exact_sky = "exact", "f32"
    no = R.render_frame(p, hw, 12, mode="fused", cnn=False)
    assert R.field_gate["path"] == "exact" and R.field_falls_back()
    assert torch.equal(no, R.render_frame(p, hw, 12, mode="exact", cnn=False))
    img = R.render_frame(p, hw, 12, mode="fused")
    assert torch.equal(img, R.render_frame(p, hw, 12, mode="exact"))
    assert all(torch.equal(f, img) for f in R.render_frames([p, p], hw, 12, mode="fused"))
    R.exact_sky = None
    assert not torch.equal(no, R.render_frame(p, hw, 12, mode="exact", cnn=False))          # (the PyTorch sky: another summation order)
    D = Renderer(weights_full, scene256, "cuda")
    D.set_style(synth.make_style(8888))
    D.exact_sky = "f32"                       # fallback stays "unfused": all of it on PyTorch
    img = D.render_frame(p, hw, 12, mode="fused")
    assert D.field_gate["path"] == "unfused"
    assert torch.equal(img, D.render_frame(p, hw, 12, mode="unfused"))
    D.exact_sky = None
    assert torch.equal(img, D.render_frame(p, hw, 12, mode="unfused"))


def test_bands_equal_the_frame(frame_renderer, scene256):
    """5e. band_prepare / band_finish over two bands with exact_sky = "f32" (the kernel runs without sky_avg; the band's f64 sky_sum is
    taken from sky_c): the bands' net_out rows equal the single frame's within 1e-3 -- not bit for bit, the two means are added in
    different orders -- and so do the image rows."""
    R = frame_renderer
    p = _pose(scene256, 5)
    H, W = HW
    R.exact_sky = "f32"
    keep = R._run_cnn
    try:
        no = R.render_frame(p, HW, NS, mode="exact", cnn=False)[:, 4:-4, 4:-4]
        img = R.render_frame(p, HW, NS, mode="exact")
        hds = [R.band_prepare(p, HW, r0, r1, mode="exact") for r0, r1 in ((0, 40), (40, H))]
        assert all(h["sky_sum"].dtype == torch.float64 for h in hds)
        tot = (sum(h["sky_sum"] for h in hds) / sum(h["sky_cnt"] for h in hds)).to(torch.float32).reshape(1, 64)
        band_img = torch.cat([R.band_finish(h, tot, NS) for h in hds], dim=2)
        R._run_cnn = lambda mode, x: x.permute(0, 3, 1, 2)          # band_finish's net_out, cropped by the band's halo like an image
        band_no = torch.cat([R.band_finish(h, tot, NS) for h in hds], dim=2).permute(0, 2, 3, 1)
    finally:
        R._run_cnn = keep
        R.exact_sky = None
    assert tuple(band_no.shape) == tuple(no.shape) == (1, H, W, 64) and tuple(band_img.shape) == tuple(img.shape)
    e_no, e_img = float((band_no - no).abs().max()), float((band_img - img).abs().max())
    print(f"two bands vs the frame, exact_sky='f32': net_out max abs diff {e_no:.3e}, image max abs diff {e_img:.3e}")
    assert e_no <= TOL and e_img <= TOL


# ----------------------------------------------------------------------------------------------------- module surface

def _native_sky_net(weights):
    from scenedreamer_amd import modules
    net = modules.SKYMLP(33, 256, out_channels_c=64)
    pre = "sky_net."
    net.load_state_dict({k[len(pre):]: torch.as_tensor(np.asarray(v)) for k, v in weights.items() if k.startswith(pre)})
    net = net.cuda().eval()
    for prm in net.parameters():
        prm.requires_grad_(False)
    return net


def test_module_surface(renderer, weights_full, dirs, full):
    """6. modules.SKYMLP with sdn_exact = True is served by sdn_sky_mlp_f32 in both input forms (the same bits as fused.sky_exact);
    with weights outside the f16 stream's range it is served natively too, with the same bits; without the flag the call is what
    it was."""
    from scenedreamer_amd import ops
    z = torch.from_numpy(FL.style_code()).cuda().reshape(1, -1)
    net = _native_sky_net(weights_full)
    tagged = ops.positional_encoding(dirs[None], 5, -1, True)          # [1,1001,33], tagged with its source: encoded in the kernel
    plain = tagged.clone()                                             # the same rows, no tag: handed in
    before = net(plain, z)
    assert net.__dict__.get("_sdn_composite_reason") is None
    net.sdn_exact = True
    a, b = net(tagged, z), net(plain, z)
    assert net.__dict__.get("_sdn_composite_reason") is None and tuple(a.shape) == (1, 1001, 64)
    assert torch.equal(a[0], full[0]) and torch.equal(b[0], full[0])
    del net.sdn_exact
    assert torch.equal(before, net(plain, z))
    assert not torch.equal(before, a)          # (the f16 kernel's answer, as before)
    # out-of-range weights: natively, not by _forward_composite, and no TrunkRangeError
    w = {k: torch.as_tensor(np.asarray(v)) for k, v in weights_full.items() if k.startswith("sky_net.")}
    big = _native_sky_net(_scaled(w, 2.0 ** 10))
    big.sdn_exact = True
    c = big(plain, z)
    assert big.__dict__.get("_sdn_composite_reason") is None
    assert torch.equal(c[0], full[0])
