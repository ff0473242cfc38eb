"""Depth and opacity maps on the MI355X: the two kernels of csrc/maps.hip against their numpy restatement (tests/depth_maps_ref.py)
with ==, then the maps through Renderer.render_frame in its three modes, render_frames, and the command line."""
import os

import numpy as np
import pytest
import torch

import depth_maps_ref as ref
from conftest import bits

pytestmark = pytest.mark.gpu

HW, NS = (48, 64), 12          # the small frame of tests/test_exact_aux_gpu.py
ALL = ("depth", "opacity", "range", "depth_u8", "weights", "sample_depth")


def _u32(rng):
    """the int32[2] tensor of maps.depth_maps as uint32 numpy"""
    return rng.cpu().numpy().view(np.uint32)


# ---- 5. the kernels against the restatement ----------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1, 0), (5, 7, 3, 1), (9, 70, 24, 2), (33, 65, 40, 0), (4, 64, 5, 0)]          # rows, cols, ns, crop


def _check_against_ref(w, z, rows, cols, crop, n_workgroups=0):
    from scenedreamer_amd import maps
    d, o, r = maps.depth_maps(torch.from_numpy(w).cuda(), torch.from_numpy(z).cuda(), rows, cols, crop, n_workgroups=n_workgroups)
    u8, u16 = maps.quantise(d, r, 8, n_workgroups=n_workgroups), maps.quantise(d, r, 16, n_workgroups=n_workgroups)
    want_d, want_o = ref.composite(w, z, rows, cols, crop)
    want_r = ref.value_range(want_d)
    assert tuple(d.shape) == tuple(o.shape) == want_d.shape == (rows - 2 * crop, cols - 2 * crop)
    assert np.array_equal(bits(d.cpu().numpy()), bits(want_d)) and np.array_equal(bits(o.cpu().numpy()), bits(want_o))
    assert np.array_equal(_u32(r), want_r), (_u32(r), want_r)
    assert u8.dtype == torch.uint8 and np.array_equal(u8.cpu().numpy(), ref.quantise(want_d, want_r, 8))
    assert u16.dtype == torch.uint16 and np.array_equal(u16.cpu().numpy(), ref.quantise(want_d, want_r, 16))
    return d, o, r, u8, u16


@pytest.mark.parametrize("rows,cols,ns,crop", SHAPES)
def test_kernels_equal_the_restatement(rows, cols, ns, crop):
    w, z = ref.synthetic(rows, cols, ns, seed=rows * 1000 + cols)
    if rows * cols >= 4:
        dm, _ = ref.composite(w, z, rows, cols, 0)
        assert np.isnan(dm).any() and (dm < 0).any() and (dm == 0).any() and (dm > 0).any()      # the synthetic frame has every kind of ray
    outs = [_check_against_ref(w, z, rows, cols, crop, nwg) for nwg in (0, 1, 2, 7)]
    for other in outs[1:]:                      # the launch shape changes no bit
        for a, b in zip(outs[0], other):
            assert np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8))


def test_an_unaligned_base_takes_the_scalar_loads():
    """num_samples % 4 == 0 on a base address that is not 16-byte aligned: the float4 form does not apply, the result is the same."""
    from scenedreamer_amd import maps
    rows, cols, ns = 6, 10, 8
    w, z = ref.synthetic(rows, cols, ns, seed=5)
    hold_w, hold_z = torch.zeros(rows * cols * ns + 1, device="cuda"), torch.zeros(rows * cols * ns + 1, device="cuda")
    wv, zv = hold_w[1:].view(rows * cols, ns), hold_z[1:].view(rows * cols, ns)
    wv.copy_(torch.from_numpy(w))
    zv.copy_(torch.from_numpy(z))
    assert wv.data_ptr() % 16 == 4 and wv.is_contiguous()
    d, o, r = maps.depth_maps(wv, zv, rows, cols, 1)
    want_d, want_o = ref.composite(w, z, rows, cols, 1)
    assert np.array_equal(bits(d.cpu().numpy()), bits(want_d)) and np.array_equal(bits(o.cpu().numpy()), bits(want_o))
    assert np.array_equal(_u32(r), ref.value_range(want_d))


def test_range_is_reinitialised_on_reused_buffers_and_opacity_is_optional():
    from scenedreamer_amd import capi, maps
    rows, cols, ns = 9, 11, 6
    w1, z1 = ref.synthetic(rows, cols, ns, seed=1)
    w2, z2 = ref.synthetic(rows, cols, ns, seed=2)
    # a range strictly inside the first one: weights that add up to one per ray, depths of 200 .. 203
    z2 = (np.abs(z2) * np.float32(0.01) + np.float32(200)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        w2 = np.where(w2.sum(axis=1, keepdims=True) > 0, w2 / w2.sum(axis=1, keepdims=True), w2).astype(np.float32)
    d = torch.empty(rows * cols, device="cuda")
    rng = torch.full((2,), 12345, dtype=torch.int32, device="cuda")            # garbage: the entry initialises the pair itself
    got = []
    for w, z in ((w1, z1), (w2, z2)):
        wt, zt = torch.from_numpy(w).cuda(), torch.from_numpy(z).cuda()
        capi.check(capi.lib().sdn_depth_maps(wt.data_ptr(), zt.data_ptr(), rows, cols, ns, 0, d.data_ptr(), None, rng.data_ptr(), 3,
                                             capi.current_stream(d.device)), "sdn_depth_maps")
        want, _ = ref.composite(w, z, rows, cols, 0)
        assert np.array_equal(bits(d.cpu().numpy().reshape(rows, cols)), bits(want))
        assert np.array_equal(_u32(rng), ref.value_range(want))
        got.append(_u32(rng).copy())
    assert got[1][0] > got[0][0] and got[1][1] < got[0][1]                     # neither end is left over from the first call
    dd, oo, _ = maps.depth_maps(torch.from_numpy(w1).cuda(), torch.from_numpy(z1).cuda(), rows, cols, 0, opacity=False)
    assert oo is None and np.array_equal(bits(dd.cpu().numpy()), bits(ref.composite(w1, z1, rows, cols, 0)[0]))


def test_on_a_side_stream():
    from scenedreamer_amd import maps
    rows, cols, ns, crop = 12, 20, 12, 2
    w, z = ref.synthetic(rows, cols, ns, seed=9)
    wt, zt = torch.from_numpy(w).cuda(), torch.from_numpy(z).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d, o, r = maps.depth_maps(wt, zt, rows, cols, crop)
        u8 = maps.quantise(d, r, 8)
    s.synchronize()
    want, want_o = ref.composite(w, z, rows, cols, crop)
    assert np.array_equal(bits(d.cpu().numpy()), bits(want)) and np.array_equal(bits(o.cpu().numpy()), bits(want_o))
    assert np.array_equal(u8.cpu().numpy(), ref.quantise(want, ref.value_range(want), 8))


def test_frames_without_a_range():
    from scenedreamer_amd import maps
    rows, cols, ns = 5, 9, 4
    g = np.random.default_rng(4)
    z = (g.random((rows * cols, ns), dtype=np.float32) * 50 + 1).astype(np.float32)
    # nothing positive: zero rays, a negative one and a NaN one
    w = np.zeros((rows * cols, ns), np.float32)
    w[3], w[7, 1] = -0.25, np.nan
    d, o, r, u8, u16 = _check_against_ref(w, z, rows, cols, 0)
    assert tuple(int(v) for v in _u32(r)) == ref.NO_HIT == maps.NO_HIT and maps.range_values(r) is None
    assert bool((u8 == 255).all()) and bool((u16.cpu().numpy() == 65535).all())
    # one positive pixel: hi == lo -> 0 there
    w[11] = 0.125
    d, o, r, u8, u16 = _check_against_ref(w, z, rows, cols, 0)
    lo, hi = _u32(r)
    assert lo == hi and maps.range_values(r)[0] == float(d.view(-1)[11])
    assert int(u8.view(-1)[11]) == 0 and int((u8 == 255).sum()) == rows * cols - 1 and int(u16.cpu().numpy().reshape(-1)[11]) == 0
    # a frame of equal positives
    w = np.full((rows * cols, ns), 0.25, np.float32)
    z = np.full((rows * cols, ns), 3.0, np.float32)
    d, o, r, u8, u16 = _check_against_ref(w, z, rows, cols, 1)
    assert _u32(r)[0] == _u32(r)[1] and bool((u8 == 0).all()) and bool((u16.cpu().numpy() == 0).all()) and float(d.max()) == 3.0 * 0.25 * ns


def test_metric_range_16_bits():
    from scenedreamer_amd import maps
    rows, cols, ns = 7, 33, 12
    w, z = ref.synthetic(rows, cols, ns, seed=21)
    w = (w * np.random.default_rng(22).random((rows * cols, 1), dtype=np.float32)).astype(np.float32)      # depths from ~0 to > 1000
    d, _, r = maps.depth_maps(torch.from_numpy(w).cuda(), torch.from_numpy(z).cuda(), rows, cols, 0)
    want, _ = ref.composite(w, z, rows, cols, 0)
    depth_max = 200.0
    assert np.nanmax(want) > 2 * depth_max > 0                                  # some values are beyond depth_max: clamped
    metric = maps.metric_range(depth_max, "cuda")
    assert _u32(metric).view(np.float32).tolist() == [0.0, depth_max]
    for nbits, top in ((16, 65535), (8, 255)):
        got = maps.quantise(d, metric, nbits).cpu().numpy()
        assert np.array_equal(got, ref.quantise(want, _u32(metric), nbits))
        assert np.all(got[want >= depth_max] == top) and np.all(got[~(want > 0)] == top) and got.min() < top // 4
    with pytest.raises(ValueError):
        maps.metric_range(0.0, "cuda")
    with pytest.raises(RuntimeError):
        maps.quantise(d, metric, 12)


# ---- 6. through the renderer ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def renderer(weights_full, scene256):
    from scenedreamer_amd import synth
    from scenedreamer_amd.renderer import Renderer
    r = Renderer(weights_full, scene256, "cuda")
    r.set_style(synth.make_style(8888))
    return r


@pytest.fixture(scope="module")
def poses(scene256):
    from scenedreamer_amd import camera
    return camera.eval_camera_poses(scene256, maxstep=8)


def _restated(m):
    rows, cols, crop = m["window"]
    w, z = m["weights"].cpu().numpy(), m["sample_depth"].cpu().numpy()
    assert w.shape == z.shape == (rows * cols, NS)
    d, o = ref.composite(w, z, rows, cols, crop)
    r = ref.value_range(d)
    return d, o, r, ref.quantise(d, r, 8)


@pytest.mark.parametrize("mode", ["fused", "exact", "unfused"])
def test_render_frame_maps(renderer, poses, mode):
    R, pose = renderer, poses[5]
    try:
        R.set_precision(term_eps=0.0)           # every sample evaluated: the launch with per-sample outputs is then the same evaluation
        before = R.render_frame(pose, HW, NS, mode=mode, cnn=False)
        m = dict.fromkeys(ALL)
        with_maps = R.render_frame(pose, HW, NS, mode=mode, cnn=False, maps=m)
        after = R.render_frame(pose, HW, NS, mode=mode, cnn=False)
    finally:
        R.set_precision()
    assert sorted(m) == sorted(ALL + ("window",))
    rows, cols, crop = m["window"]
    assert (rows - 2 * crop, cols - 2 * crop) == HW == tuple(m["depth"].shape) == tuple(m["opacity"].shape) == tuple(m["depth_u8"].shape)
    # the maps are the restatement of this call's own per-sample arrays: pins the window, the order and the crop
    d, o, r, u8 = _restated(m)
    assert np.array_equal(bits(m["depth"].cpu().numpy()), bits(d)) and np.array_equal(bits(m["opacity"].cpu().numpy()), bits(o))
    assert np.array_equal(_u32(m["range"]), r) and np.array_equal(m["depth_u8"].cpu().numpy(), u8)
    depth, opacity = m["depth"], m["opacity"]
    assert bool(torch.isfinite(depth).all()) and float(opacity.min()) >= 0 and float(opacity.max()) <= 1 + 1e-5
    assert torch.equal(depth > 0, opacity > 0)
    hit = float((depth > 0).float().mean())
    print(f"{mode}: {hit:.2f} of the pixels hit the scene; depth {float(depth[depth > 0].min()):.3f} .. {float(depth.max()):.3f}")
    assert 0.2 < hit < 1.0
    # the frame itself: within the project's bound for the instantiation with per-sample outputs; a default call is untouched
    diff = float((with_maps - before).abs().max())
    print(f"{mode}: net_out with maps vs without: max abs {diff:.3e}")
    assert with_maps.shape == before.shape and diff <= 2e-6
    assert torch.equal(after, before)
    # an empty dict stands for depth, opacity and depth_u8
    e = {}
    R.render_frame(pose, HW, NS, mode=mode, cnn=False, maps=e)
    assert sorted(e) == ["depth", "depth_u8", "opacity", "window"]
    if mode != "fused":         # (fused: early termination is off for the launch with maps, so it is the launch above)
        assert torch.equal(e["depth"], depth) and torch.equal(e["opacity"], opacity) and torch.equal(e["depth_u8"], m["depth_u8"])
    with pytest.raises(ValueError, match="unknown keys"):
        R.render_frame(pose, HW, NS, mode=mode, cnn=False, maps={"disparity": None})


@pytest.mark.parametrize("mode", ["exact", "fused"])
def test_maps_and_the_apron(renderer, poses, mode):
    """The per-ray bits of the fp32 kernel do not depend on the window (include/sdnative.h): the maps of the minimal and of the
    reference apron are the same.  The f16 kernel's are printed."""
    R, pose = renderer, poses[5]
    a, b = dict.fromkeys(ALL), dict.fromkeys(ALL)
    R.render_frame(pose, HW, NS, mode=mode, maps=a, apron="minimal")
    R.render_frame(pose, HW, NS, mode=mode, maps=b, apron="reference")
    assert a["window"] == (HW[0] + 8, HW[1] + 8, 4) and b["window"] == (HW[0] + 30, HW[1] + 30, 15)
    dd = float((a["depth"] - b["depth"]).abs().max())
    print(f"{mode}: depth with the minimal vs the reference apron: max abs {dd:.3e}")
    if mode == "exact":
        for k in ("depth", "opacity", "depth_u8", "range"):
            assert torch.equal(a[k], b[k]), k
    for m in (a, b):
        d, o, r, u8 = _restated(m)
        assert np.array_equal(bits(m["depth"].cpu().numpy()), bits(d)) and np.array_equal(m["depth_u8"].cpu().numpy(), u8)


# ---- 7. the trajectory loop ----------------------------------------------------------------------------------------------------------
def test_render_frames_with_maps(renderer, poses):
    R = renderer
    three = [poses[i] for i in (2, 5, 6)]
    calls = []

    def factory():
        calls.append(dict.fromkeys(("depth", "opacity", "depth_u8", "range")))
        return calls[-1]

    got = list(R.render_frames(three, HW, NS, mode="fused", maps=factory))
    by_template = list(R.render_frames(three, HW, NS, mode="fused", maps={}))
    assert len(got) == len(by_template) == len(calls) == 3
    for pose, (img, m), made, (img_t, m_t) in zip(three, got, calls, by_template):
        assert m is made
        want = dict.fromkeys(("depth", "opacity", "depth_u8", "range"))
        want_img = R.render_frame(pose, HW, NS, mode="fused", maps=want)
        assert torch.equal(img, want_img) and torch.equal(img_t, want_img) and tuple(img.shape) == (1, 3) + HW
        for k in ("depth", "opacity", "depth_u8", "range"):
            assert torch.equal(m[k], want[k]), k
        assert sorted(m_t) == ["depth", "depth_u8", "opacity", "window"] and torch.equal(m_t["depth_u8"], want["depth_u8"])
    assert not torch.equal(got[0][1]["depth"], got[1][1]["depth"])
    # without maps the generator yields images, as before
    plain = list(R.render_frames(three[:1], HW, NS, mode="fused"))
    assert isinstance(plain[0], torch.Tensor) and tuple(plain[0].shape) == (1, 3) + HW


# ---- 8. the command line -------------------------------------------------------------------------------------------------------------
def test_cli_writes_the_depth_directory(tmp_path, weights_full, scene256):
    """Six frames through the command line in --mode exact, with and without --depth-maps u8.  The four networks beside the field run
    on their fixed-order fp32 kernels (--exact-cnn / -world / -style / -sky f32): with the render CNN on the library's convolutions the
    two runs' RGB files differed in one of two sessions (frame 00004, one of six), because the library's solver choice is not
    reproducible from call to call (renderer.py says so of the world encoder) -- with the kernels nothing between the scene and the
    PNG depends on a library, and the comparison below is of the launch with per-sample outputs against the plain launch alone."""
    from PIL import Image
    from scenedreamer_amd import camera, cli, synth
    from scenedreamer_amd.renderer import Renderer
    hw, ns, n = (72, 104), 12, 6
    common = ["--scene_size", "256", "--cam_maxstep", str(n), "--resolution_hw", str(hw[0]), str(hw[1]), "--num_samples", str(ns),
              "--mode", "exact", "--exact-cnn", "f32", "--exact-world", "f32", "--exact-style", "f32", "--exact-sky", "f32",
              "--video-backend", "mjpeg"]
    on, off = str(tmp_path / "on"), str(tmp_path / "off")
    cli.main(["--output_dir", on, "--depth-maps", "u8"] + common)
    cli.main(["--output_dir", off] + common)
    names = [f"{i:05d}.png" for i in range(n)]
    assert sorted(os.listdir(os.path.join(on, "depth"))) == names and not os.path.exists(os.path.join(off, "depth"))
    for name in names:         # the image does not change with the maps (the fp32 kernel's per-ray bits)
        a, b = (open(os.path.join(d, "rgb_render", name), "rb").read() for d in (on, off))
        assert a == b, name
    R = Renderer(weights_full, scene256, "cuda", exact_world="f32", exact_style="f32")
    R.exact_cnn = R.exact_sky = "f32"
    R.set_style(synth.make_style(8888))
    poses = camera.eval_camera_poses(scene256, maxstep=n, pattern=4, cam_ang=72)      # the command line's defaults
    assert len(poses) == n
    for i, name in enumerate(names):
        im = Image.open(os.path.join(on, "depth", name))
        m = {"depth_u8": None}
        R.render_frame(poses[i], hw, ns, mode="exact", maps=m)
        assert im.mode == "L" and im.size == (hw[1], hw[0])
        assert np.array_equal(np.asarray(im), m["depth_u8"].cpu().numpy()), name
