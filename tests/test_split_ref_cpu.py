"""The yardstick of tests/test_arithmetic_gpu.py, qualified without a GPU.  oracle/split_ref.py emulates the 3-term f16 split
of every MFMA kernel on the CPU; the GPU tests bound each kernel by 4 x E3, the emulated intact scheme's own error against
fp64.  That bound means something only if, on the very inputs the GPU tests use (tests/field_layout.py),

    E3 <= 8 x E32          the intact scheme is "as close to fp64 as fp32 is" (README), and
    Edef >= 16 x E3        the CHEAPEST single defect -- one correction term (Wlo.Xhi or Whi.Xlo) dropped in one layer --
                           is at least 4 x outside the GPU bound,

with T the fp64 truth (oracle/field_ref.py in float64), E32 / E3 / Edef the max abs error against T of the fp32 reference
arithmetic / the emulated intact scheme / the best single-defect configuration.  These are conditions on the inputs, not
measurements: if an input set fails them, the inputs change, not the factors."""
import pytest
import torch

import field_layout as FL

E3_OVER_E32, EDEF_OVER_E3 = 8.0, 16.0


def _report(name, e32, e3, defects):
    """defects: [(error, layer, dropped term)]"""
    edef, layer, term = min(defects)
    print(f"{name:58s} E32 {e32:.2e}  E3 {e3:.2e}  E3/E32 {e3 / e32:5.2f}  Edef/E3 {edef / e3:7.1f} (cheapest: {layer} without {term})")
    assert e3 <= E3_OVER_E32 * e32, (name, e3, e32)
    assert edef >= EDEF_OVER_E3 * e3, (name, layer, term, edef, e3)


@pytest.fixture(scope="module")
def z():
    return FL.style_code()


def test_render_mlp_sigma_and_colour(weights_full, z):
    """sdn_render_mlp's inputs (1537 rows, all 12 labels, |x| <= 0.3), sigma and colour separately.  The colour layers do not
    feed sigma and the density head is an f32 dot product in the kernel: the defect list of sigma is fc_1 .. fc_4."""
    from oracle import split_ref as SR
    x, lab = FL.mlp_rows()
    assert set(lab.tolist()) == set(range(12)) and float(x.abs().max()) <= 0.3
    truth = SR.render_mlp_ref(weights_full, x, z, lab, torch.float64)
    yard = SR.render_mlp_ref(weights_full, x, z, lab, torch.float32)
    fold = SR.fold_render_mlp(weights_full, z)
    got = SR.render_mlp(fold, x, lab)
    runs = [(n, d, SR.render_mlp(fold, x, lab, cfg)) for n, d, cfg in SR.single_defects(SR.MLP_LAYERS)]
    for i, what in enumerate(("sigma", "colour")):
        feeds = SR.MLP_FEEDS[what]
        _report(f"LightningMLP {what} (|.| <= {float(truth[i].abs().max()):.3g})", FL.max_err(yard[i], truth[i]), FL.max_err(got[i], truth[i]),
                [(FL.max_err(out[i], truth[i]), n, d) for n, d, out in runs if n in feeds])
    # the layers that do not feed sigma leave it untouched, bit for bit: the list above skips nothing that matters
    assert all(torch.equal(out[0], got[0]) for n, _, out in runs if n not in SR.MLP_FEEDS["sigma"])


def test_sky_mlp(weights_full, z):
    from oracle import split_ref as SR
    pe = FL.sky_encoded(FL.sky_dirs())
    truth = SR.sky_mlp_ref(weights_full, pe, z, torch.float64)
    yard = SR.sky_mlp_ref(weights_full, pe, z, torch.float32)
    fold = SR.fold_sky_mlp(weights_full, z)
    got = SR.sky_mlp(fold, pe)
    _report(f"SKYMLP (|y| <= {float(truth.abs().max()):.3g})", FL.max_err(yard, truth), FL.max_err(got, truth),
            [(FL.max_err(SR.sky_mlp(fold, pe, cfg), truth), n, d) for n, d, cfg in SR.single_defects(SR.SKY_LAYERS)])
    # the frame mean (sky_avg): errors of the packed WEIGHTS are the same for every ray and do not average out, so the mean is
    # the sharpest test of the weights' lo halves; the GPU test bounds it by 4 x the fp32 yardstick of the mean
    e32m, e3m = FL.max_err(yard.mean(dim=0), truth.mean(dim=0)), FL.max_err(got.mean(dim=0), truth.mean(dim=0))
    print(f"{'SKYMLP frame mean':58s} E32 {e32m:.2e}  E3 {e3m:.2e}  E3/E32 {e3m / e32m:5.2f}")
    assert e3m <= 4 * e32m, (e3m, e32m)


@pytest.mark.parametrize("chain", [True, False])
def test_render_cnn_image(weights_full, z, chain):
    """MfmaCNN(renderer, 3) at 21 x 37, with the chained head / tail kernels and as conv_kernel launches throughout (conv4 is then
    the f32 projection of conv4b's epilogue: no split terms, no defect)."""
    from oracle import field_ref as FR
    from oracle import split_ref as SR
    no = FL.cnn_net_out()
    truth = FR.render_cnn(weights_full, no, z, torch.float64)
    yard = FR.render_cnn(weights_full, no, z, torch.float32)
    memo = {}
    got = SR.render_cnn(weights_full, no, z, None, chain, memo)
    layers = SR.CNN_LAYERS if chain else SR.CNN_LAYERS[:-1]
    _report(f"RenderCNN image {FL.CNN_HW[0]}x{FL.CNN_HW[1]}, chain={chain}", FL.max_err(yard, truth), FL.max_err(got, truth),
            [(FL.max_err(SR.render_cnn(weights_full, no, z, cfg, chain, memo), truth), n, d) for n, d, cfg in SR.single_defects(SR.CNN_LAYERS, layers)])


@pytest.mark.parametrize("case", FL.CONV_CASES, ids=[f"{c[1]}-{c[2][0]}x{c[2][1]}-{c[3]['out']}" for c in FL.CONV_CASES])
def test_conv_layer(weights_full, case):
    """Every single-layer case of the GPU test (3x3 and 1x1, each frame size, each epilogue).  Frames of fewer than 256 pixels take
    E3 and E32 from the 9x33 frame of the same layer and epilogue, as the GPU test does; their defects are their own."""
    from oracle import split_ref as SR
    name, layer, hw, ep = case
    inp = FL.conv_inputs(hw)
    x = SR.planes(inp["x"])
    resid = SR.planes(inp["resid"]) if ep.get("resid") == "planes" else inp["resid"]
    ev = lambda how: FL.conv_case_eval(weights_full, layer, hw, ep, inp, x, resid, how)
    truth = ev("f64")
    e3, e32 = FL.conv_case_yardstick(weights_full, layer, ep) if FL.yard_frame(hw) != hw else (FL.max_err(ev(SR.T3), truth), FL.max_err(ev("f32"), truth))
    _report(f"{name} ({layer}, {hw[0]}x{hw[1]})", e32, e3,
            [(FL.max_err(ev(SR.LH), truth), layer, "hl"), (FL.max_err(ev(SR.HL), truth), layer, "lh")])


def test_chain_and_head(weights_full):
    """sdn_conv_head and sdn_conv_chain on the frames of the GPU test."""
    from oracle import field_ref as FR
    from oracle import split_ref as SR
    Tn = lambda n: FR.T(weights_full, "denoiser." + n)
    for hw in FL.CONV_FRAMES:
        x = FL.conv_inputs(hw, 64)["x"]
        truth = SR.head(x, Tn("conv1.weight"), Tn("conv1.bias"), hw, dtype=torch.float64)
        ev = lambda t: SR.head(x, Tn("conv1.weight"), Tn("conv1.bias"), hw, t)
        small = FL.yard_frame(hw) != hw
        e3, e32 = FL.head_yardstick(weights_full) if small else (FL.max_err(ev(SR.T3), truth),
                                                                  FL.max_err(SR.head(x, Tn("conv1.weight"), Tn("conv1.bias"), hw, dtype=torch.float32), truth))
        _report(f"conv head {hw[0]}x{hw[1]}", e32, e3, [(FL.max_err(ev(SR.LH), truth), "conv1", "hl"), (FL.max_err(ev(SR.HL), truth), "conv1", "lh")])
        y = FL.rows_to_nchw(SR.planes(FL.conv_inputs(hw)["x"]), hw)
        args = (y, Tn("conv4a.weight"), Tn("conv4a.bias"), Tn("conv4b.weight"), Tn("conv4b.bias"), Tn("conv4.weight"), Tn("conv4.bias"))
        truth = SR.chain_tail(*args, dtype=torch.float64)
        layers = ("conv4a", "conv4b", "conv4")
        e3, e32 = FL.chain_yardstick(weights_full) if small else (FL.max_err(SR.chain_tail(*args), truth),
                                                                   FL.max_err(SR.chain_tail(*args, dtype=torch.float32), truth))
        _report(f"conv chain {hw[0]}x{hw[1]}", e32, e3, [(FL.max_err(SR.chain_tail(*args, cfg), truth), n, d) for n, d, cfg in SR.single_defects(layers)])


def test_single_defect_generator():
    from oracle import split_ref as SR
    cfgs = list(SR.single_defects(SR.MLP_LAYERS))
    assert len(cfgs) == 2 * len(SR.MLP_LAYERS) and len({(n, d) for n, d, _ in cfgs}) == len(cfgs)
    for n, d, cfg in cfgs:
        assert set(cfg) == set(SR.MLP_LAYERS) and d in ("lh", "hl")
        assert [k for k in cfg if cfg[k] != SR.T3] == [n] and set(SR.T3) - set(cfg[n]) == {d}
    assert [n for n, _, _ in SR.single_defects(SR.MLP_LAYERS, SR.MLP_FEEDS["sigma"])] == [l for l in SR.MLP_FEEDS["sigma"] for _ in range(2)]


def test_composite_restates_the_oracle(weights_full):
    """split_ref.composite in float32 is the compositing of oracle/field_ref.py's forward_perpix, bit for bit; in float64 it
    stays float64 (the oracle's volum_rendering_relu drops to float32 inside)."""
    from oracle import field_ref as FR
    from oracle import split_ref as SR
    g = torch.Generator().manual_seed(5)
    R, ns = 37, 10
    sigma = torch.randn(R, ns, generator=g) * 20 - 4
    colour = torch.randn(R, ns, 64, generator=g) * 1.5
    dists = torch.rand(R, ns, generator=g) * 0.03
    sky_c, sky_avg = torch.randn(R, 64, generator=g), torch.randn(64, generator=g)
    sky_only, nosky = torch.rand(R, generator=g) < 0.2, torch.rand(R, generator=g) < 0.5
    got = SR.composite(sigma, colour, dists, sky_only, nosky, sky_c, sky_avg)
    w = FR.volum_rendering_relu(sigma[..., None], dists[..., None], dim=-2) * torch.logical_not(sky_only).float()[:, None, None]
    m = nosky.float()[:, None]
    sky = sky_c * (1.0 - m) + sky_avg[None] * m
    want = torch.sum(w * (torch.clamp(colour, -1, 1) + 1), dim=-2) + (1.0 - w.sum(dim=-2)) * (torch.clamp(sky, -1, 1) + 1) - 1
    assert torch.equal(got, want)
    d = SR.composite(sigma.double(), colour.double(), dists.double(), sky_only, nosky, sky_c.double(), sky_avg.double())
    assert d.dtype == torch.float64 and 0 < float((d - got.double()).abs().max()) < 1e-5


def test_shifted_streams_refuse_weights_outside_f16():
    """fused.check_trunk_range guards every stream that is packed times 2^shift (field trunk, sky MLP, render CNN tail): weights
    that would leave f16's range there raise TrunkRangeError naming the stream; the plain layer counts in full, the layers that
    consume the 0.4-scaled activation times 0.4."""
    from scenedreamer_amd import fused
    w1, wh = torch.full((4, 4), 0.5), [torch.full((4, 4), 0.3)]
    assert fused.check_trunk_range(w1, wh, 8, "sky MLP") == 0.5
    assert abs(fused.check_trunk_range(w1 * 0.1, [wh[0] * 100], 8, "sky MLP") - 12.0) < 1e-5
    with pytest.raises(fused.TrunkRangeError, match="sky MLP"):
        fused.check_trunk_range(w1 * 256, wh, 8, "sky MLP")                # 128 * 2^8 = 32768: at the headroom
    with pytest.raises(fused.TrunkRangeError, match="render CNN tail"):
        fused.check_trunk_range(w1, [wh[0] * 1100], 8, "render CNN tail")   # 0.4 * 330 = 132
    with pytest.raises(fused.TrunkRangeError):
        fused.check_trunk_range(w1 * float("nan"), wh, 8)
    fused.check_trunk_range(w1 * 255, wh, 8, "sky MLP")
