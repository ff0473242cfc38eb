"""The arithmetic of every f16-split MFMA kernel on the MI355X against fp64.

Every product of the render MLP, the sky MLP and the render CNN is the 3-term f16 split Whi.Xhi + Wlo.Xhi + Whi.Xlo with f32
accumulation.  oracle/split_ref.py emulates that scheme on the CPU; tests/test_split_ref_cpu.py shows that on the inputs used
here the intact scheme's error E3 (against fp64) is within 8 x the error E32 of plain fp32 arithmetic, and that dropping ONE
correction term in ONE layer costs at least 16 x E3.  The bound here is

        max |kernel - T|  <=  4 x E3

with T the fp64 truth from this repository's oracle on the CPU and E3 computed in the same test on the same inputs (4 = the
summation-order allowance of tests/test_exact_rung_gpu.py): every single defect is at least 4 x outside it.  Every test prints
kernel/E3 and kernel/E32; SDN_ARITH_RECORD=<file> collects them as JSON (profiles/split_arithmetic.json)."""
import ctypes

import numpy as np
import pytest
import torch

import field_layout as FL

pytestmark = pytest.mark.gpu

FACTOR = FL.FACTOR
RECORD = FL.RECORD
_record_file = FL.record_file_fixture()
_check, _check_fp32 = FL.check, FL.check_fp32


def _lossy(name, got, truth, yard):
    """The intentionally lossy forms: no bound, their kernel/E32 ratio for the record."""
    e, e32 = FL.max_err(got, truth), FL.max_err(yard, truth)
    RECORD[name] = dict(kernel=e, E32=e32, kernel_over_E32=e / e32)
    print(f"{name:72s} kernel {e:.2e}  E32 {e32:.2e}  kernel/E32 {e / e32:7.1f}   (lossy by design: not bounded)")


def _renderer(weights, scene):
    from scenedreamer_amd.renderer import Renderer
    r = Renderer(weights, scene, "cuda")
    r.set_style_code(FL.style_code())
    return r


@pytest.fixture(scope="module")
def renderer(weights_full, scene256):
    return _renderer(weights_full, scene256)


_fold_from = FL.fold_from


# ----------------------------------------------------------------------------------------------------- render MLP as an op

def _render_mlp(R, x, lab, ct=3, n_workgroups=0, ticket=True):
    from scenedreamer_amd import capi, fused
    st = R._fused_style or fused.prepare_style(R)
    n = x.shape[0]
    sigma = torch.full((n,), float("nan"), device=R.dev)
    c = torch.full((n, 64), float("nan"), device=R.dev)
    tk = torch.zeros(2, dtype=torch.int32, device=R.dev)
    with torch.cuda.device(R.dev):
        capi.check(capi.lib().sdn_render_mlp(x.data_ptr(), lab.data_ptr(), st["packed_mx" if ct == 6 else "packed"].data_ptr(),
                                             st["consts"].data_ptr(), sigma.data_ptr(), c.data_ptr(), n, ct, n_workgroups,
                                             tk.data_ptr() if ticket else None, capi.current_stream(R.dev)), "sdn_render_mlp")
    torch.cuda.synchronize()
    assert int(tk.abs().sum()) == 0          # the launch leaves the ticket at zero
    return sigma, c


@pytest.fixture(scope="module")
def mlp_case(renderer, weights_full):
    from oracle import split_ref as SR
    x, lab = FL.mlp_rows()
    z = renderer.z.cpu().numpy()
    truth = SR.render_mlp_ref(weights_full, x, z, lab, torch.float64)
    yard = SR.render_mlp_ref(weights_full, x, z, lab, torch.float32)
    emu = SR.render_mlp(_fold_from(renderer), x, lab)
    whole = _render_mlp(renderer, x.cuda().contiguous(), lab.to(torch.uint8).cuda().contiguous())
    return x, lab, truth, emu, yard, whole


@pytest.mark.parametrize("n", FL.MLP_ROWS)
def test_render_mlp_against_fp64(renderer, mlp_case, n):
    """sdn_render_mlp, colour_terms = 3: 1537 rows (the last 32-row group and the last 256-row block are ragged), 33 rows, 1 row;
    all 12 labels, |x| <= 0.3; sigma and colour bounded separately.  E3 is a maximum over rows -- the emulation's error on one
    row is a single draw, not a yardstick -- so the 33- and 1-row launches (the first rows of the same set) are held to the E3 of
    the whole set, and, rows being independent, must reproduce the bits the 1537-row launch gave those rows.  The same bits for
    n_workgroups 0 / 1 / 7 and with or without the ticket counter, as the header promises."""
    x, lab, truth, emu, yard, whole = mlp_case
    assert n == 1 or set(lab[:n].tolist()) == set(range(12))
    xg, lg = x[:n].cuda().contiguous(), lab[:n].to(torch.uint8).cuda().contiguous()
    sigma, c = _render_mlp(renderer, xg, lg)
    assert torch.isfinite(sigma).all() and torch.isfinite(c).all()
    if n == FL.MLP_ROWS[0]:
        _check(f"sdn_render_mlp sigma, {n} rows", sigma.cpu(), truth[0], emu[0], yard[0])
        _check(f"sdn_render_mlp colour, {n} rows", c.cpu(), truth[1], emu[1], yard[1])
    else:
        assert torch.equal(sigma, whole[0][:n]) and torch.equal(c, whole[1][:n])
        for i, (what, got) in enumerate((("sigma", sigma), ("colour", c))):
            e, e3 = FL.max_err(got.cpu(), truth[i][:n]), FL.max_err(emu[i], truth[i])
            print(f"sdn_render_mlp {what}, {n} rows: kernel {e:.2e}, E3 of the {FL.MLP_ROWS[0]}-row set {e3:.2e}, ratio {e / e3:.2f}")
            RECORD[f"sdn_render_mlp {what}, {n} rows"] = dict(kernel=e, E3_of_whole_set=e3, kernel_over_E3=e / e3)
            assert e <= FACTOR * e3, (what, n, e, e3)
    for nwg in (0, 1, 7):
        for ticket in (False, True):
            s2, c2 = _render_mlp(renderer, xg, lg, n_workgroups=nwg, ticket=ticket)
            assert torch.equal(s2, sigma) and torch.equal(c2, c), (nwg, ticket)
    if n == FL.MLP_ROWS[0]:
        s6, c6 = _render_mlp(renderer, xg, lg, ct=6)
        assert torch.equal(s6, sigma)              # the fp6 corrections live in the colour layers only
        _lossy("sdn_render_mlp colour, colour_terms=6 (fp6 corrections)", c6.cpu(), truth[1][:n], yard[1][:n])


# ----------------------------------------------------------------------------------------------------- sky MLP

@pytest.mark.parametrize("encoded", [0, 1])
def test_sky_mlp_against_fp64(renderer, weights_full, encoded):
    """sdn_sky_mlp, hidden_terms = 3, on 1001 unit directions: the positional encoding evaluated inside the kernel (encoded = 0)
    or handed in (encoded = 1); the truth is SKYMLP in fp64 on the CPU oracle's encoding.  sky_avg, the frame mean the kernel
    finishes itself, against the fp64 mean: its yardstick is the fp32 mean's error (errors of the packed WEIGHTS are common to
    all rays and do not average out, so this is the sharpest test of the weights' lo halves)."""
    from oracle import split_ref as SR
    from scenedreamer_amd import fused
    d = FL.sky_dirs()
    pe = FL.sky_encoded(d)
    z = renderer.z.cpu().numpy()
    truth = SR.sky_mlp_ref(weights_full, pe, z, torch.float64)
    yard = SR.sky_mlp_ref(weights_full, pe, z, torch.float32)
    c = lambda t: t.detach().float().cpu()
    w = renderer.w
    fold = dict(w1=c(w["sky_net.fc1.weight"]), b1=c(w["sky_net.fc1.bias"] + renderer.sky_z.reshape(-1)),
                hidden=[c(w[f"sky_net.fc{i}.weight"]) for i in (2, 3, 4, 5)], bias=[c(w[f"sky_net.fc{i}.bias"]) for i in (2, 3, 4, 5)],
                wc=c(w["sky_net.fc_out_c.weight"]), bc=c(w["sky_net.fc_out_c.bias"]))
    emu = SR.sky_mlp(fold, pe)
    renderer.sky_terms = 3
    try:
        sky_c, avg = fused.sky_fused(renderer, (pe if encoded else d).cuda(), encoded=bool(encoded))
        torch.cuda.synchronize()
        _check(f"sdn_sky_mlp sky_c, encoded={encoded}", sky_c.cpu(), truth, emu, yard)
        e = FL.max_err(avg.reshape(-1).cpu(), truth.mean(dim=0))
        e32 = FL.max_err(yard.mean(dim=0), truth.mean(dim=0))
        e3 = FL.max_err(emu.mean(dim=0), truth.mean(dim=0))
        RECORD[f"sdn_sky_mlp sky_avg, encoded={encoded}"] = dict(kernel=e, E3=e3, E32=e32, kernel_over_E3=e / e3, kernel_over_E32=e / e32)
        print(f"{'sdn_sky_mlp sky_avg, encoded=%d' % encoded:72s} kernel {e:.2e}  E3 {e3:.2e}  E32 {e32:.2e}  kernel/E32 {e / e32:5.2f}")
        assert e <= FACTOR * e32, (e, e32)
        if not encoded:
            renderer.sky_terms = 6
            c6, _ = fused.sky_fused(renderer, d.cuda())
            _lossy("sdn_sky_mlp sky_c, hidden_terms=6 (fp6 corrections)", c6.cpu(), truth, yard)
    finally:
        renderer.sky_terms = None


# ----------------------------------------------------------------------------------------------------- convolutions

class _Conv:
    """The C ABI of the render CNN's kernels on torch tensors."""

    def __init__(self, R):
        from scenedreamer_amd import capi
        self.R, self.capi, self.lib = R, capi, capi.lib()
        self.packed = {}

    def dims(self, H, W):
        hb, wb = ctypes.c_int(), ctypes.c_int()
        self.lib.sdn_conv_plane_dims(H, W, ctypes.byref(hb), ctypes.byref(wb))
        return hb.value, wb.value

    def zeros(self, H, W, C=256):
        hb, wb = self.dims(H, W)
        mk = lambda: torch.zeros(hb * wb * C, dtype=torch.float16, device=self.R.dev)
        return mk(), mk()

    def planes(self, rows, H, W):
        """sdn_conv_planes_from_f32 into zero-filled planes; asserts hi + lo == x and a clean border."""
        C = rows.shape[1]
        hi, lo = self.zeros(H, W, C)
        x = rows.cuda().contiguous()
        self.capi.check(self.lib.sdn_conv_planes_from_f32(x.data_ptr(), C, hi.data_ptr(), lo.data_ptr(), H, W,
                                                          self.capi.current_stream(self.R.dev)), "sdn_conv_planes_from_f32")
        torch.cuda.synchronize()
        dec = self.decode(hi, lo, H, W, C)
        # hi + lo == x to 2^-22 relative; lo is an f16, whose subnormal quantum 2^-24 is the floor for |x| < 1/8
        d = (dec.double() - rows.double()).abs()
        assert bool((d <= torch.clamp(rows.double().abs() * 2.0 ** -22, min=2.0 ** -25)).all()), float(d.max())
        return hi, lo, dec

    def decode(self, hi, lo, H, W, C=256):
        hb, wb = self.dims(H, W)
        h, l, clean = FL.decode_planes(hi, lo, H, W, hb, wb, C)
        assert clean, "a border / out-of-frame pixel of a plane is not zero"
        return torch.from_numpy(h + l if l is not None else h)

    def weights(self, layer, cin, taps, terms=3):
        if (layer, terms) not in self.packed:
            wt = self.R.w[f"denoiser.{layer}.weight"].contiguous()
            buf = torch.empty(self.lib.sdn_conv_packed_weight_bytes(cin, taps, terms), dtype=torch.uint8, device=self.R.dev)
            self.capi.check(self.lib.sdn_conv_pack_weights(wt.data_ptr(), cin, taps, terms, buf.data_ptr(),
                                                           self.capi.current_stream(self.R.dev)), "sdn_conv_pack_weights")
            self.packed[(layer, terms)] = buf
        return self.packed[(layer, terms)]

    def conv(self, src, layer, H, W, bias=None, resid=None, resid_planes=None, mod=None, dst=None, out32=None, proj=None, img=None):
        p = lambda t: t.data_ptr() if t is not None else None
        wt = self.R.w[f"denoiser.{layer}.weight"]
        cin, taps = wt.shape[1], wt.shape[2] * wt.shape[3]
        self.capi.check(self.lib.sdn_conv(src[0].data_ptr(), src[1].data_ptr(), cin, taps, 3, self.weights(layer, cin, taps).data_ptr(),
                                          p(bias), p(resid), p(resid_planes[0]) if resid_planes else None,
                                          p(resid_planes[1]) if resid_planes else None, p(mod[0]) if mod else None,
                                          p(mod[1]) if mod else None, p(dst[0]) if dst else None, p(dst[1]) if dst else None,
                                          p(out32), p(proj[0]) if proj else None, p(proj[1]) if proj else None, p(img), H, W, 0,
                                          self.capi.current_stream(self.R.dev)), "sdn_conv")
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def conv(renderer):
    return _Conv(renderer)


@pytest.mark.parametrize("case", FL.CONV_CASES, ids=[f"{c[1]}-{c[2][0]}x{c[2][1]}-{c[3]['out']}" for c in FL.CONV_CASES])
def test_conv_layer_against_fp64(renderer, conv, weights_full, case):
    """sdn_conv, one layer at a time, terms = 3: a 3x3 and a 1x1 layer on 1x1, 3x2, 9x33 and 37x53 frames, every epilogue at
    least once (tests/field_layout.py CONV_CASES).  The inputs go through sdn_conv_planes_from_f32; the truth convolves the
    DECODED planes, so the input rounding is no part of the error, and E3 is emulated the same way (for the 1x1 and 3x2 frames
    on the 9x33 frame of the same layer and epilogue: a maximum over a few values is a draw, not a yardstick).  The planes themselves:
    hi + lo == x to 2^-22, border and out-of-frame pixels zero before and after the launch, inputs untouched."""
    from oracle import split_ref as SR
    name, layer, (H, W), ep = case
    inp = FL.conv_inputs((H, W))
    dev = lambda t: t.cuda().contiguous()
    xh, xl, x_dec = conv.planes(inp["x"], H, W)
    resid_rows, rp, r32 = inp["resid"], None, None
    if ep.get("resid") == "planes":
        rh, rl, resid_rows = conv.planes(inp["resid"], H, W)
        rp = (rh, rl)
    elif ep.get("resid") == "rows":
        r32 = dev(inp["resid"])
    bias = dev(inp["bias"]) if ep.get("bias") else None
    mod = (dev(inp["mod_w"]), dev(inp["mod_b"])) if ep.get("mod") else None
    proj = (renderer.w["denoiser.conv4.weight"].reshape(3, 256).contiguous(), renderer.w["denoiser.conv4.bias"].contiguous()) if ep.get("proj") else None
    out32 = torch.full((H * W, 256), float("nan"), device="cuda") if ep["out"] == "f32" else None
    img = torch.full((3, H * W), float("nan"), device="cuda") if ep["out"] == "img" else None
    dst = None
    if ep["out"] == "planes":
        dst = rp if rp is not None else conv.zeros(H, W)          # a plane residual is updated in place
    conv.conv((xh, xl), layer, H, W, bias=bias, resid=r32, resid_planes=rp, mod=mod, dst=dst, out32=out32, proj=proj, img=img)
    got = out32.cpu() if out32 is not None else img.cpu() if img is not None else conv.decode(dst[0], dst[1], H, W)
    assert torch.isfinite(got).all()
    assert torch.equal(conv.decode(xh, xl, H, W), x_dec)           # the input planes (and their border) are as they were
    ev = lambda how: FL.conv_case_eval(weights_full, layer, (H, W), ep, inp, x_dec, resid_rows, how)
    scale = FL.conv_case_yardstick(weights_full, layer, ep) if FL.yard_frame((H, W)) != (H, W) else None
    _check(f"sdn_conv {name} ({layer}, {H}x{W})", got, ev("f64"), ev(SR.T3), ev("f32"), scale=scale)
    if ep.get("hi_only"):       # out_lo = NULL (every consumer 1-term): the hi plane is the same bits, nothing else is written
        hi2, _ = conv.zeros(H, W)
        conv.conv((xh, xl), layer, H, W, bias=bias, resid=r32, resid_planes=rp, mod=mod, dst=(hi2, None))
        assert torch.equal(hi2, dst[0])
        conv.decode(hi2, None, H, W)


@pytest.mark.parametrize("hw", FL.CONV_FRAMES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_conv_head_and_chain_against_fp64(renderer, conv, weights_full, hw):
    """sdn_conv_head (net_out rows -> conv1 -> LeakyReLU -> planes) and sdn_conv_chain (conv4a -> conv4b + y -> conv4 -> tanh,
    register-resident) against the fp64 restatement of their layer chains, on the frames of the single-layer test.  The 1x1 and
    3x2 frames (3 and 18 image values) are held to the E3 of the 9x33 frame: tests/field_layout.py yard_frame."""
    from oracle import field_ref as FR
    from oracle import split_ref as SR
    from scenedreamer_amd import capi
    from scenedreamer_amd.cnn import MfmaCNN
    H, W = hw
    m = MfmaCNN(renderer, 3, chain=True)
    assert m.chain
    Tn = lambda n: FR.T(weights_full, "denoiser." + n)
    lib, st = capi.lib(), capi.current_stream(renderer.dev)
    # head
    x = FL.conv_inputs(hw, 64)["x"]
    yh, yl = conv.zeros(H, W)
    xg = x.cuda().contiguous()
    capi.check(lib.sdn_conv_head(xg.data_ptr(), m.head_packed.data_ptr(), m.head_bias.data_ptr(), yh.data_ptr(), yl.data_ptr(), H, W, 0, st),
               "sdn_conv_head")
    torch.cuda.synchronize()
    got = FL.rows_to_nchw(conv.decode(yh, yl, H, W), hw)
    hd = lambda **k: SR.head(x, Tn("conv1.weight"), Tn("conv1.bias"), hw, **k)
    small = FL.yard_frame(hw) != hw
    _check(f"sdn_conv_head {H}x{W}", got, hd(dtype=torch.float64), hd(), hd(dtype=torch.float32),
           scale=FL.head_yardstick(weights_full) if small else None)
    # chain
    ih, il, y_dec = conv.planes(FL.conv_inputs(hw)["x"], H, W)
    img = torch.full((3, H * W), float("nan"), device="cuda")
    raw = torch.full((3, H * W), float("nan"), device="cuda")
    capi.check(lib.sdn_conv_chain(ih.data_ptr(), il.data_ptr(), m.chain_packed.data_ptr(), m.chain_consts.data_ptr(), img.data_ptr(),
                                  raw.data_ptr(), H, W, 0, st), "sdn_conv_chain")
    torch.cuda.synchronize()
    assert torch.equal(torch.tanh(raw), img) or float((torch.tanh(raw) - img).abs().max()) < 1e-6
    args = (FL.rows_to_nchw(y_dec, hw), Tn("conv4a.weight"), Tn("conv4a.bias"), Tn("conv4b.weight"), Tn("conv4b.bias"), Tn("conv4.weight"), Tn("conv4.bias"))
    _check(f"sdn_conv_chain {H}x{W}", img.cpu().reshape(1, 3, H, W), SR.chain_tail(*args, dtype=torch.float64), SR.chain_tail(*args),
           SR.chain_tail(*args, dtype=torch.float32), scale=FL.chain_yardstick(weights_full) if small else None)


@pytest.mark.parametrize("chain", [True, False])
def test_mfma_cnn_against_fp64(renderer, weights_full, chain):
    """The whole MfmaCNN(renderer, 3) at 21 x 37, chained head / tail and conv_kernel launches throughout, against RenderCNN in fp64."""
    from oracle import field_ref as FR
    from oracle import split_ref as SR
    from scenedreamer_amd.cnn import MfmaCNN
    no = FL.cnn_net_out()
    z = renderer.z.cpu().numpy()
    truth = FR.render_cnn(weights_full, no, z, torch.float64)
    yard = FR.render_cnn(weights_full, no, z, torch.float32)
    emu = SR.render_cnn(weights_full, no, z, None, chain)
    m = MfmaCNN(renderer, 3, chain=chain)
    assert m.chain == chain
    img = m(no.cuda())
    torch.cuda.synchronize()
    _check(f"MfmaCNN(terms3x3=3, chain={chain}) image {FL.CNN_HW[0]}x{FL.CNN_HW[1]}", img.cpu(), truth, emu, yard)
    if chain:
        _lossy("MfmaCNN(terms3x3=1) image (one product in the 3x3 layers)", MfmaCNN(renderer, 1, chain=True)(no.cuda()).cpu(), truth, yard)
        _lossy("MfmaCNN(terms3x3='1133') image (ladder rung)", MfmaCNN(renderer, "1133", chain=True)(no.cuda()).cpu(), truth, yard)


# ----------------------------------------------------------------------------------------------------- field MLP + compositing

FIELD_HW = (10, 26)         # + the 30-pixel apron: 40 x 56 rays
REGIMES = ("default", "surface", "fog")


@pytest.fixture(scope="module")
def regimes(renderer, weights_full, scene256):
    """Three density regimes, built the way tests/test_config_parity_gpu.py builds them: the synthetic default (about half the
    samples have sigma <= 0), surface-like (fc_sigma.bias + 4000: the transmittance underflows within a few samples) and fog
    (synth.fog_weights: sigma = 6 +- 0.65, no weight exactly zero)."""
    from scenedreamer_amd import synth
    made = {"default": (renderer, weights_full)}

    def get(name):
        if name not in made:
            if name == "surface":
                w2 = dict(weights_full)
                w2["render_net.fc_sigma.bias"] = np.asarray(weights_full["render_net.fc_sigma.bias"]) + np.float32(4000.0)
            else:
                w2 = synth.fog_weights(weights_full)
            made[name] = (_renderer(w2, scene256), w2)
        return made[name]
    return get


def _rays(R, scene):
    from scenedreamer_amd import camera
    pose = camera.eval_camera_poses(scene, maxstep=8)[5]
    with torch.no_grad():
        vid, d2, rd, (H0, W0) = R.cast_rays(pose, FIELD_HW)
    n = H0 * W0
    assert (H0, W0) == (40, 56)
    return pose, vid.view(n, R.M).contiguous(), d2.view(2, n, R.M).contiguous(), rd.view(n, 3).contiguous()


def _two_kernel_field(R, scene, ns):
    """FL.two_kernel_field on the small frame's rays."""
    pose, vid, d2, rd = _rays(R, scene)
    return FL.two_kernel_field(R, vid, d2, rd, torch.as_tensor(pose[0], dtype=torch.float32), ns)


_field_references = FL.field_references


@pytest.fixture(scope="module")
def field_cases():
    return {}


def _field_case(cache, regimes, scene, regime, ns):
    if (regime, ns) not in cache:
        R, w = regimes(regime)
        R.set_precision(colour_terms=3, term_eps=0.0)
        R.field_single_kernel = False
        try:
            net_out, given, rays = _two_kernel_field(R, scene, ns)
        finally:
            R.field_single_kernel = None
            R.set_precision()
        cache[(regime, ns)] = (net_out, given, rays, _field_references(R, w, given))
    return cache[(regime, ns)]


@pytest.mark.parametrize("ns", [10, 24])
@pytest.mark.parametrize("regime", REGIMES)
def test_field_mlp_and_compositing_against_fp64(regimes, field_cases, scene256, regime, ns):
    """sdn_field_mlp isolated: the encode buffers are read back (features as hi + lo, dist, label, rayflag) and the MLP and the
    compositing (volume rendering, sky-only mask, sky blend, clamp, sum) are evaluated in fp64 on exactly those values, with the
    kernel's sky_c and sky_avg as given inputs.  Three density regimes; num_samples 10 leaves two padded slots in the last
    4-sample pass.  At least 20 % of the rays hit something, so the case cannot pass on sky alone."""
    net_out, given, _, (truth, emu, yard) = _field_case(field_cases, regimes, scene256, regime, ns)
    hit = 1.0 - float(given["sky_only"].float().mean())
    assert hit >= 0.2, f"only {hit:.2f} of the rays hit the scene"
    assert torch.isfinite(net_out).all()
    print(f"{100 * hit:.0f} % of the rays hit")
    _check(f"sdn_field_mlp net_out, {regime} density, num_samples={ns}", net_out.cpu(), truth, emu, yard)


@pytest.mark.parametrize("ns", [1, 5, 10])
def test_ragged_sample_counts_through_the_one_kernel_forms(regimes, field_cases, weights_full, lut, scene256, ns):
    """num_samples 1, 5, 10 (no multiple of four: the last 4-sample pass has padded slots).  fused.field_fused as ONE kernel must
    produce the bits of the two-kernel sequence (which is held to the fp64 bound above, here also at 1 and 5 samples);
    fused.field_exact (the fp32 rung) must stay within 4 x the fp32 yardstick of the fp64 truth -- the oracle's forward_perpix
    in float64, whose sample placement is the kernel's (the sample distances are compared bit for bit)."""
    from oracle import field_ref as FR
    from oracle import split_ref as SR
    from scenedreamer_amd import fused
    R, w = regimes("default")
    net_out, given, (vid, d2, rd, ori, sky_c, sky_avg), (truth, emu, yard) = _field_case(field_cases, regimes, scene256, "default", ns)
    _check(f"sdn_field_mlp net_out, default density, num_samples={ns}", net_out.cpu(), truth, emu, yard)
    R.set_precision(colour_terms=3, term_eps=0.0)
    R.field_single_kernel = True
    try:
        with torch.no_grad():
            one = fused.field_fused(R, vid, d2, rd, ori, sky_c, sky_avg, ns)
            exact = fused.field_exact(R, vid, d2, rd, ori, sky_c, sky_avg, ns)
            torch.cuda.synchronize()
    finally:
        R.field_single_kernel = None
        R.set_precision()
    assert torch.equal(one, net_out)
    # the oracle's forward_perpix on the same rays, in fp32 and in fp64, with the kernel's sky features as the given sky
    n = vid.shape[0]
    M = R.M
    args = (w, lut, scene256.voxel_t.shape, vid.cpu().numpy().reshape(1, 40, 56, M, 1), d2.cpu().numpy().reshape(1, 2, 40, 56, M, 1),
            rd.cpu().numpy().reshape(1, 40, 56, 1, 3), ori.numpy()[None], R.z.cpu().numpy(), R.global_enc.cpu().numpy(), ns)
    # the kernel's sky features as the given sky; the volume rendering in the dtype of the evaluation (the oracle's own drops to
    # float32 inside: no fp64 truth)
    kw = dict(sky_avg=given["sky_avg"].reshape(1, 1, 1, 1, 64), sky_c=given["sky_c"].reshape(1, 40, 56, 1, 64),
              volume_rendering=SR.volum_rendering_relu)
    f32, aux = FR.forward_perpix(*args, return_aux=True, **kw)
    f64 = FR.forward_perpix(*args, dtype=torch.float64, **kw)
    # ... and on the features the kernels gathered (the collapsed 3-D table), the arithmetic alone
    feat = given["feat"].reshape(1, 40, 56, ns, 128)
    k32 = FR.forward_perpix(*args, feature_in=feat, **kw)
    k64 = FR.forward_perpix(*args, feature_in=feat, dtype=torch.float64, **kw)
    hitting = ~given["sky_only"]
    ref_dist = (aux["new_dists"].reshape(n, ns) * np.float32(0.25))[hitting]
    assert torch.equal(ref_dist.view(torch.int32), given["dist"][hitting].view(torch.int32))         # the kernel's placement IS the oracle's
    ex = exact.cpu()
    _check_fp32(f"field_exact net_out, num_samples={ns}, vs forward_perpix fp64 (oracle features)", ex, f64.reshape(n, 64), f32.reshape(n, 64))
    _check_fp32(f"field_exact net_out, num_samples={ns}, vs forward_perpix fp64 (kernel features)", ex, k64.reshape(n, 64), k32.reshape(n, 64))
