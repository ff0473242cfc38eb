"""The fp32 render CNN on the MI355X (csrc/cnn_f32.hip: sdn_conv_f32, cnn.F32CNN, Renderer.exact_cnn / cnn_mode = "f32",
RenderCNNNative.sdn_exact): every layer and epilogue against fp64 in units of the error E32 of the reference's own fp32 arithmetic
(tests/field_layout.py: 4 x E32; tests/test_cnn_f32_cpu.py qualifies the summation order that bound asks for), the whole CNN, the
independence of a pixel's bits from its position and from the frame, fp32's range with no tolerance, and the plumbing.
Every check prints its kernel/E32 ratio; SDN_ARITH_RECORD=<file> collects them as JSON (none recorded yet: the tests were written
with no MI355X at hand)."""
import contextlib
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import field_layout as FL

pytestmark = pytest.mark.gpu

RECORD = FL.RECORD
_record_file = FL.record_file_fixture()
HW, NS = (72, 104), 24          # the renderer tests: the setup of tests/test_exact_rung_gpu.py


def _check32(name, got, truth, yard=None, e32=None):
    """max |got - T| <= 4 x E32 (FL.check_fp32), with E32 measured elsewhere (`e32`) where the case's own values are too few."""
    if e32 is None:
        return FL.check_fp32(name, got, truth, yard)
    e = FL.max_err(got, truth)
    RECORD[name] = dict(kernel=e, E32=e32, kernel_over_E32=e / e32, yardstick_frame="%dx%d" % FL.YARD_HW)
    print(f"{name:72s} kernel {e:.2e}  E32 {e32:.2e}  kernel/E32 {e / e32:5.2f}   (E32 of the {FL.YARD_HW[0]}x{FL.YARD_HW[1]} frame)")
    assert e <= FL.FACTOR * e32, (name, e, e32)


@pytest.fixture(scope="module")
def renderer(weights_full, scene256):
    from scenedreamer_amd.renderer import Renderer
    r = Renderer(weights_full, scene256, "cuda")
    r.set_style_code(FL.style_code())
    return r


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    monkeypatch.delenv("SDN_EXACT_CNN", raising=False)
    monkeypatch.delenv("SDN_CNN_EXACT", raising=False)


# ----------------------------------------------------------------------------------------------------- one layer at a time

EP_ROWS = dict(bias=True, out="f32")                                   # bias -> rows
EP_FILM = dict(bias=True, resid="rows", mod=True, out="f32")           # bias + residual + FiLM, IN PLACE (out_rows = resid)
EP_PROJ = dict(bias=True, resid="rows", proj=True, out="img")          # bias + residual, conv4 -> raw, tanh -> img; no rows
LAYER_CASES = tuple(
    (layer, cin, hw, ep)
    for layer, cin, eps in (("conv1", 64, (EP_ROWS, EP_ROWS, EP_ROWS, EP_ROWS)),
                            ("conv2a", 256, (EP_ROWS, EP_FILM, EP_PROJ, EP_ROWS)),
                            ("conv3b", 256, (EP_PROJ, EP_ROWS, EP_FILM, EP_PROJ)),
                            ("conv4a", 256, (EP_FILM, EP_PROJ, EP_ROWS, EP_FILM)),
                            ("conv4b", 256, (EP_ROWS, EP_FILM, EP_PROJ, EP_PROJ)))
    for hw, ep in zip(FL.CONV_FRAMES, eps))
_EP_NAME = {id(EP_ROWS): "bias -> rows", id(EP_FILM): "bias + residual + FiLM in place", id(EP_PROJ): "bias + residual, conv4 -> raw, img"}
_EP_ID = {id(EP_ROWS): "rows", id(EP_FILM): "film-in-place", id(EP_PROJ): "proj"}


def _case_id(c):
    return f"{c[0]}-{c[2][0]}x{c[2][1]}-{_EP_ID[id(c[3])]}"


def _eval_case(w, layer, cin, hw, ep, how):
    """(rows [h*w,256] or img [3,h*w], raw [3,h*w] or None) of one launch on the CPU: FL.conv_case_eval, and conv4 before the tanh."""
    from oracle import field_ref as FR
    inp = FL.conv_inputs(hw, cin)
    res = FL.conv_case_eval(w, layer, hw, ep, inp, inp["x"], inp["resid"], how)
    raw = None
    if ep.get("proj"):
        dt = torch.float64 if how == "f64" else torch.float32
        v = FL.conv_case_eval(w, layer, hw, dict(ep, proj=False, out="f32"), inp, inp["x"], inp["resid"], how)
        raw = F.conv2d(FL.rows_to_nchw(v.to(dt), hw), FR.T(w, "denoiser.conv4.weight", dt).reshape(3, 256, 1, 1),
                       FR.T(w, "denoiser.conv4.bias", dt)).reshape(3, -1)
    return res, raw


_YARD = {}


def _yard_e32(w, layer, cin, ep):
    """E32 of the same layer and epilogue on the 9 x 33 frame: (rows or img, raw)."""
    key = (layer, id(ep))
    if key not in _YARD:
        (t, traw), (y, yraw) = _eval_case(w, layer, cin, FL.YARD_HW, ep, "f64"), _eval_case(w, layer, cin, FL.YARD_HW, ep, "f32")
        _YARD[key] = (FL.max_err(y, t), FL.max_err(yraw, traw) if traw is not None else None)
    return _YARD[key]


class _Conv:
    """sdn_conv_f32 launches with the weights of a denoiser layer, packed once."""

    def __init__(self, R):
        from scenedreamer_amd import capi
        self.R, self.lib, self.capi, self.packed = R, capi.lib(), capi, {}

    def weights(self, layer, cin, taps):
        if layer not in self.packed:
            wt = self.R.w[f"denoiser.{layer}.weight"].contiguous()
            buf = torch.empty(self.lib.sdn_conv_f32_packed_weight_bytes(cin, taps), dtype=torch.uint8, device=self.R.dev)
            self.capi.check(self.lib.sdn_conv_pack_weights_f32(wt.data_ptr(), cin, taps, buf.data_ptr(), self.capi.current_stream(self.R.dev)),
                            "sdn_conv_pack_weights_f32")
            self.packed[layer] = buf
        return self.packed[layer]

    def __call__(self, layer, x, hw, bias=None, resid=None, mod=None, out=None, proj=None, img=None, raw=None, n_workgroups=0):
        taps = self.R.w[f"denoiser.{layer}.weight"].shape[-1] ** 2
        cin = x.shape[1]
        p = lambda t: t.data_ptr() if t is not None else None
        rc = self.lib.sdn_conv_f32(x.data_ptr(), cin, taps, self.weights(layer, cin, taps).data_ptr(), p(bias), p(resid),
                                   p(mod[0]) if mod else None, p(mod[1]) if mod else None, p(out), p(proj[0]) if proj else None,
                                   p(proj[1]) if proj else None, p(img), p(raw), hw[0], hw[1], n_workgroups, self.capi.current_stream(self.R.dev))
        self.capi.check(rc, "sdn_conv_f32")
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def conv(renderer):
    return _Conv(renderer)


@pytest.mark.parametrize("case", LAYER_CASES, ids=_case_id)
def test_layer_against_fp64(renderer, conv, weights_full, case):
    """1. sdn_conv_f32, one launch at a time: conv1 (1x1, 64 channels), conv2a / conv3b (3x3) and conv4a / conv4b (1x1) on 1x1, 3x2,
    9x33 and 37x53 frames; every epilogue for a 3x3 and for a 1x1 layer.  Truth and yardstick are the same graph in fp64 and in fp32
    on the same f32 rows; the 1x1 and 3x2 frames are held to the E32 of the 9x33 frame (tests/field_layout.py yard_frame).  One fmaf
    chain per tap predicts 1.0 - 1.5 x E32; a kernel with ONE chain over a 3x3 layer's 2304 products would measure about 6.5."""
    layer, cin, hw, ep = case
    n = hw[0] * hw[1]
    dev = renderer.dev
    inp = FL.conv_inputs(hw, cin)
    g = {k: v.to(dev) for k, v in inp.items()}
    name = f"sdn_conv_f32 {layer} {hw[0]}x{hw[1]}: {_EP_NAME[id(ep)]}"
    (truth, truth_raw), (yard, yard_raw) = _eval_case(weights_full, layer, cin, hw, ep, "f64"), _eval_case(weights_full, layer, cin, hw, ep, "f32")
    small = FL.yard_frame(hw) != hw
    e32, e32_raw = _yard_e32(weights_full, layer, cin, ep) if small else (None, None)
    guard = torch.full((n * 256 + 256,), float("nan"), device=dev)          # what follows the rows stays untouched
    if ep is EP_ROWS:
        conv(layer, g["x"], hw, bias=g["bias"], out=guard)
    elif ep is EP_FILM:
        guard[:n * 256] = g["resid"].reshape(-1)
        conv(layer, g["x"], hw, bias=g["bias"], resid=guard, mod=(g["mod_w"], g["mod_b"]), out=guard)          # in place
    else:
        w4 = renderer.w["denoiser.conv4.weight"].reshape(3, 256).contiguous()
        b4 = renderer.w["denoiser.conv4.bias"].contiguous()
        img = torch.full((3 * n + 8,), float("nan"), device=dev)
        raw = torch.full((3 * n + 8,), float("nan"), device=dev)
        conv(layer, g["x"], hw, bias=g["bias"], resid=g["resid"], proj=(w4, b4), img=img, raw=raw)
        assert torch.isnan(img[3 * n:]).all() and torch.isnan(raw[3 * n:]).all()
        _check32(name + " [img]", img[:3 * n].view(3, n).cpu(), truth, yard, e32)
        _check32(name + " [raw]", raw[:3 * n].view(3, n).cpu(), truth_raw, yard_raw, e32_raw)
        assert float((torch.tanh(raw[:3 * n]) - img[:3 * n]).abs().max()) <= 2.0 ** -22          # img IS tanh(raw)
        only = torch.empty(3 * n, device=dev)                                # either output alone: the same bits
        conv(layer, g["x"], hw, bias=g["bias"], resid=g["resid"], proj=(w4, b4), img=only)
        assert torch.equal(only, img[:3 * n])
        conv(layer, g["x"], hw, bias=g["bias"], resid=g["resid"], proj=(w4, b4), raw=only)
        assert torch.equal(only, raw[:3 * n])
        return
    assert torch.isnan(guard[n * 256:]).all()
    _check32(name, guard[:n * 256].view(n, 256).cpu(), truth, yard, e32)


def test_launch_shape_changes_no_bit(renderer, conv):
    """The grid is a schedule, not arithmetic: 1 workgroup, 3 workgroups (groups per workgroup not equal) and the default give the
    same bits -- on a frame whose last 128-pixel group and last 32-pixel group are ragged."""
    hw = (37, 53)
    n = hw[0] * hw[1]
    assert n % 128 != 0 and n % 32 != 0
    g = {k: v.to(renderer.dev) for k, v in FL.conv_inputs(hw).items()}
    outs = []
    for wg in (0, 1, 3):
        o = torch.empty(n, 256, device=renderer.dev)
        conv("conv3b", g["x"], hw, bias=g["bias"], resid=g["resid"], mod=(g["mod_w"], g["mod_b"]), out=o, n_workgroups=wg)
        outs.append(o)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_3x3_in_place_is_refused(renderer, conv):
    from scenedreamer_amd import capi
    x = FL.conv_inputs((3, 2))["x"].to(renderer.dev)
    with pytest.raises(Exception, match="cannot write the rows it reads"):
        conv("conv2a", x, (3, 2), out=x)
    y = x.clone()
    conv("conv4a", y, (3, 2), out=y)                 # a 1x1 layer may: a pixel's input is read only by the lanes that write it
    z = torch.empty_like(x)
    conv("conv4a", x, (3, 2), out=z)
    assert torch.equal(y, z)
    assert capi.lib().sdn_abi_version() == 5


# ----------------------------------------------------------------------------------------------------- the whole CNN

@contextlib.contextmanager
def _no_tanh():
    """oracle/field_ref.py render_cnn with its last step removed: conv4's output, RenderCNN.forward's own return value."""
    keep = torch.tanh
    torch.tanh = lambda v: v
    try:
        yield
    finally:
        torch.tanh = keep


_CNN_REF = {}


def _cnn_refs(weights, net_out, z, key):
    """(img, raw) of FR.render_cnn in fp64 and in fp32, computed once per input."""
    from oracle import field_ref as FR
    if key not in _CNN_REF:
        out = {}
        for dt in (torch.float64, torch.float32):
            with _no_tanh():
                raw = FR.render_cnn(weights, net_out, z, dtype=dt)
            out[dt] = (torch.tanh(raw), raw)
        _CNN_REF[key] = out
    return _CNN_REF[key][torch.float64], _CNN_REF[key][torch.float32]


def _f32cnn(R):
    from scenedreamer_amd.cnn import F32CNN
    return F32CNN(R)


@pytest.mark.parametrize("hw", [(21, 37), (37, 53)], ids=lambda hw: "%dx%d" % hw)
def test_whole_cnn_against_fp64(renderer, weights_full, hw):
    """2. cnn.F32CNN (7 launches) against oracle/field_ref.py render_cnn in fp64: img and raw within 4 x E32 (the per-tap chain
    emulated on the CPU predicts 1.1 - 1.2)."""
    no = FL.cnn_net_out(hw)
    (t_img, t_raw), (y_img, y_raw) = _cnn_refs(weights_full, no, FL.style_code(), hw)
    renderer.set_style_code(FL.style_code())
    cnn = _f32cnn(renderer)
    raw = torch.full((1, 3) + hw, float("nan"), device=renderer.dev)
    timers = {}
    img = cnn(no.to(renderer.dev), raw=raw, timers=timers)
    torch.cuda.synchronize()
    assert tuple(img.shape) == (1, 3) + hw and list(timers) == list(cnn.FLOP_PER_PIXEL) and sum(cnn.FLOP_PER_PIXEL.values()) == 5015040
    _check32(f"F32CNN {hw[0]}x{hw[1]} [img]", img.cpu(), t_img, y_img)
    _check32(f"F32CNN {hw[0]}x{hw[1]} [raw]", raw.cpu(), t_raw, y_raw)
    assert torch.equal(img, cnn(no.to(renderer.dev)))          # again, without raw and timers: the same bits


def test_position_independence(renderer, conv):
    """3. A pixel's bits depend on its neighbourhood only.  The image of the 37 x 53 frame on rows 9 .. 26, columns 11 .. 43 equals
    the image of net_out[:, 5:31, 7:48] on its interior 4 pixels in from every edge (four 3x3 layers); the window's origin is a
    multiple of no tile size, its pixels sit in other lanes, waves and workgroups.  The same for one 3x3 layer, interior 1 pixel."""
    renderer.set_style_code(FL.style_code())
    no = FL.cnn_net_out((37, 53)).to(renderer.dev)
    cnn = _f32cnn(renderer)
    full = cnn(no)
    sub = cnn(no[:, 5:31, 7:48].contiguous())
    assert tuple(sub.shape) == (1, 3, 26, 41)
    assert torch.equal(full[:, :, 9:27, 11:44], sub[:, :, 4:-4, 4:-4])
    assert not torch.equal(full[:, :, 8:28, 10:45], sub[:, :, 3:-3, 3:-3])      # (one pixel further out the zero padding shows)
    g = {k: v.to(renderer.dev) for k, v in FL.conv_inputs((37, 53)).items()}
    a = torch.empty(37 * 53, 256, device=renderer.dev)
    conv("conv2a", g["x"], (37, 53), bias=g["bias"], out=a)
    xs = g["x"].view(37, 53, 256)[5:31, 7:48].reshape(-1, 256).contiguous()
    b = torch.empty(26 * 41, 256, device=renderer.dev)
    conv("conv2a", xs, (26, 41), bias=g["bias"], out=b)
    assert torch.equal(a.view(37, 53, 256)[6:30, 8:47], b.view(26, 41, 256)[1:-1, 1:-1])


def test_range_is_bit_exact(renderer):
    """4. fp32's range, with no tolerance: conv2a (weight, bias) x 2^20 and conv2b.weight x 2^-20 are the same function -- LeakyReLU
    is positively homogeneous, a power of two scales every fp32 product exactly -- and must give the same image bits.  (The f16
    kernels cannot hold 2^20 times these weights at all.)"""
    renderer.set_style_code(FL.style_code())
    no = FL.cnn_net_out((21, 37)).to(renderer.dev)
    w = dict(renderer.w)
    w["denoiser.conv2a.weight"] = w["denoiser.conv2a.weight"] * 2.0 ** 20
    w["denoiser.conv2a.bias"] = w["denoiser.conv2a.bias"] * 2.0 ** 20
    w["denoiser.conv2b.weight"] = w["denoiser.conv2b.weight"] * 2.0 ** -20
    assert float(w["denoiser.conv2a.weight"].abs().max()) > 65504 / 256          # outside what MfmaCNN's 2^8-scaled stream holds
    big = types.SimpleNamespace(w=w, dev=renderer.dev, cnn_adapt=renderer.cnn_adapt)
    a, b = _f32cnn(renderer)(no), _f32cnn(big)(no)
    assert torch.isfinite(a).all() and float(a.abs().max()) > 0
    assert torch.equal(a, b)


# ----------------------------------------------------------------------------------------------------- renderer

def _pose(scene256, i):
    from scenedreamer_amd import camera
    return camera.eval_camera_poses(scene256, maxstep=8)[i]


def test_renderer_routes_to_the_kernel(weights_full, scene256):
    """5. render_frame(mode="exact", cnn_mode="f32") is F32CNN on the frame's net_out, cropped; within 4 x E32 of fp64 on that
    net_out; Renderer.exact_cnn = "f32" is the same bits as the explicit cnn_mode; unset, the image is the PyTorch CNN's, as before;
    the trajectory loop equals single frames."""
    from scenedreamer_amd import synth
    from scenedreamer_amd.renderer import Renderer
    R = Renderer(weights_full, scene256, "cuda")
    R.set_style(synth.make_style(8888))
    p = _pose(scene256, 5)
    assert R.exact_cnn is None
    default = R.render_frame(p, HW, NS, mode="exact")
    assert torch.equal(default, R.render_frame(p, HW, NS, mode="exact", cnn_mode="torch"))
    img = R.render_frame(p, HW, NS, mode="exact", cnn_mode="f32")
    no = R.render_frame(p, HW, NS, mode="exact", cnn=False)
    c = (no.shape[1] - HW[0]) // 2
    assert tuple(img.shape) == (1, 3) + HW and c == 4
    whole = R.f32_cnn()(no)
    assert torch.equal(img, whole[:, :, c:-c, c:-c])
    assert not torch.equal(img, default)          # (two summation orders: the kernel did run)
    (t_img, _), (y_img, _) = _cnn_refs(weights_full, no.cpu(), R.z.cpu().numpy(), "frame")
    _check32(f"render_frame(mode='exact', cnn_mode='f32') {no.shape[1]}x{no.shape[2]} [img]", whole.cpu(), t_img, y_img)
    R.exact_cnn = "f32"
    assert torch.equal(img, R.render_frame(p, HW, NS, mode="exact"))
    assert torch.equal(default, R.render_frame(p, HW, NS, mode="exact", cnn_mode="torch"))       # the explicit choice wins
    frames = list(R.render_frames([p, p], HW, NS, mode="exact"))
    assert len(frames) == 2 and all(torch.equal(f, img) for f in frames)
    R.exact_cnn = "fast"
    with pytest.raises(ValueError, match="exact_cnn"):
        R.render_frame(p, HW, NS, mode="exact")
    R.exact_cnn = None
    assert torch.equal(default, R.render_frame(p, HW, NS, mode="exact"))
    frames = list(R.render_frames([p, p], HW, NS, mode="exact", cnn_mode="f32"))
    assert all(torch.equal(f, img) for f in frames)


def test_closed_gate_with_fallback_exact_routes_to_the_kernel(weights_full, scene256, monkeypatch):
    """5b. fallback = "exact", exact_cnn = "f32" and a closed field gate (forced as in tests/test_exact_rung_gpu.py
    test_fallback_switch): the frame is the exact path's with the fp32 CNN kernel; "unfused" stays on PyTorch."""
    from scenedreamer_amd import synth
    from scenedreamer_amd import renderer as rmod
    from scenedreamer_amd.renderer import Renderer
    monkeypatch.setattr(rmod, "FIELD_AUTO_BOUND", 1e-9)
    p = _pose(scene256, 5)
    hw = (48, 64)
    R = Renderer(weights_full, scene256, "cuda")
    R.set_style(synth.make_style(8888))
    R.fallback, R.exact_cnn = "exact", "f32"
    img = R.render_frame(p, hw, 12, mode="fused")
    assert R.field_gate["path"] == "exact" and R.field_falls_back()
    no = R.render_frame(p, hw, 12, mode="exact", cnn=False)
    assert torch.equal(img, R.f32_cnn()(no)[:, :, 4:-4, 4:-4])
    assert torch.equal(img, R.render_frame(p, hw, 12, mode="exact", cnn_mode="f32"))
    assert all(torch.equal(f, img) for f in R.render_frames([p, p], hw, 12, mode="fused"))
    assert torch.equal(R.render_frame(p, hw, 12, mode="fused", cnn_mode="torch"), R.render_frame(p, hw, 12, mode="exact", cnn_mode="torch"))
    D = Renderer(weights_full, scene256, "cuda")
    D.set_style(synth.make_style(8888))
    D.exact_cnn = "f32"                       # fallback stays "unfused": all of it on PyTorch
    img = D.render_frame(p, hw, 12, mode="fused")
    assert D.field_gate["path"] == "unfused"
    assert torch.equal(img, D.render_frame(p, hw, 12, mode="unfused"))
    D.exact_cnn = None
    assert torch.equal(img, D.render_frame(p, hw, 12, mode="unfused"))


# ----------------------------------------------------------------------------------------------------- module surface

def test_module_surface(renderer, weights_full):
    """6. modules.RenderCNN with sdn_exact = True is served by F32CNN (the same bits as the direct call) and returns conv4's output
    within rule 2's bound; without the flag the call is what it was."""
    from scenedreamer_amd import modules
    hw = (21, 37)
    net = modules.RenderCNN(64, 256)
    pre = "denoiser."
    net.load_state_dict({k[len(pre):]: torch.as_tensor(np.asarray(v)) for k, v in weights_full.items() if k.startswith(pre)})
    net = net.cuda().eval()
    for prm in net.parameters():
        prm.requires_grad_(False)
    no = FL.cnn_net_out(hw)
    x = no.permute(0, 3, 1, 2).contiguous().cuda()
    z = torch.from_numpy(FL.style_code()).cuda().reshape(1, -1)
    before = net(x, z)
    assert net.__dict__.get("_sdn_composite_reason") is None
    net.sdn_exact = True
    raw = net(x, z)
    assert net.__dict__.get("_sdn_composite_reason") is None and tuple(raw.shape) == (1, 3) + hw
    (_, t_raw), (_, y_raw) = _cnn_refs(weights_full, no, FL.style_code(), hw)
    _check32(f"RenderCNN.sdn_exact {hw[0]}x{hw[1]} [raw]", raw.cpu(), t_raw, y_raw)
    renderer.set_style_code(FL.style_code())
    direct = torch.empty_like(raw)
    _f32cnn(renderer)(no.cuda(), raw=direct)
    assert torch.equal(raw, direct)
    del net.sdn_exact
    after = net(x, z)
    assert torch.equal(before, after)
    assert not torch.equal(before, raw)          # (the f16 kernels' answer, as before)
