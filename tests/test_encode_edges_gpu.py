"""Sample placement and the encode stage (csrc/field_enc.h) on the MI355X at every box count and edge.

The inputs are the edge-case ray sets of tests/encode_edges.py -- M = 1, 2, 3, 6, 7, 8 boxes per ray, 1 .. 79 samples, ties on
box boundaries, zero-length / NaN / infinite boxes, coordinates exactly on and one step outside the grid's faces --, which
tests/test_encode_edges_cpu.py qualifies without a GPU (coverage, single-defect sensitivity, oracle == unmodified reference).
Every discrete decision (box index, label, sky_only / nosky, out-of-range) and every depth and distance is held bit for bit
against oracle/field_ref.py; features to the 5e-6 of tests/test_fused_gpu.py; the MLP / compositing kernels behind the stage
to the 4 x E3 / 4 x E32 rules of tests/test_arithmetic_gpu.py (tests/field_layout.py check / check_fp32)."""
import numpy as np
import pytest
import torch

import encode_edges as EE
import field_layout as FL
from conftest import bits

pytestmark = pytest.mark.gpu

IDS = [f"M{M}-ns{ns}" for M, ns in EE.CASES]
_record_file = FL.record_file_fixture()


@pytest.fixture(scope="module")
def sets():
    made = {}

    def get(M, ns):
        if (M, ns) not in made:
            made[(M, ns)] = EE.rays(M, ns)
        return made[(M, ns)]
    return get


@pytest.fixture(scope="module")
def renderers(weights_full, scene256):
    """One Renderer per box count M (they share the weights on the device)."""
    from scenedreamer_amd.renderer import Renderer
    assert tuple(scene256.voxel_t.shape) == EE.VOXEL_DIMS
    wdev = {k: torch.as_tensor(np.asarray(v)).cuda() for k, v in weights_full.items()}
    made = {}

    def get(M):
        if M not in made:
            made[M] = Renderer(wdev, scene256, "cuda", num_blocks_early_stop=M)
            made[M].set_style_code(FL.style_code())
            assert made[M].M == M and made[M].sample_depth == EE.SAMPLE_DEPTH and made[M].dists_scale == EE.DISTS_SCALE
        return made[M]
    return get


def _dev(E):
    return (torch.from_numpy(E.voxel_id).cuda().contiguous(), torch.from_numpy(E.depth2).cuda().contiguous(),
            torch.from_numpy(E.raydirs).cuda().contiguous(), torch.from_numpy(E.cam_ori))


# ----------------------------------------------------------------------------------------------------- sdn_sample_depth

@pytest.mark.parametrize("case", EE.CASES, ids=IDS)
def test_sample_depth_op_on_the_edge_set(sets, case):
    """ops.sample_depth_batched, deterministic and stochastic (a given draw, division="ieee": the CPU reference's form), against
    the oracle: box indices equal, depths and distances bit for bit (NaN positions included)."""
    from scenedreamer_amd import ops
    E = sets(*case)
    d2 = torch.from_numpy(E.depth2.reshape(1, 2, 1, E.n, E.M, 1)).cuda()
    u = EE.stratified_u(E.n, E.ns)
    for rand in (None, u):
        kw = dict(deterministic=True) if rand is None else dict(deterministic=False, division="ieee",
                                                                rand=torch.from_numpy(rand).reshape(1, 1, E.n, E.ns + 1, 1).cuda())
        depth, dist, idx = ops.sample_depth_batched(d2, E.ns + 1, use_box_boundaries=False, sample_depth=EE.SAMPLE_DEPTH, **kw)
        assert tuple(depth.shape) == (1, 1, E.n, E.ns, 1) and idx.dtype == torch.int64
        ref = EE.oracle_placement(E, rand)
        np.testing.assert_array_equal(idx.cpu().numpy().reshape(E.n, E.ns), ref[2])
        np.testing.assert_array_equal(bits(depth.cpu().numpy().reshape(E.n, E.ns)), bits(ref[0]))
        np.testing.assert_array_equal(bits(dist.cpu().numpy().reshape(E.n, E.ns)), bits(ref[1]))


def test_eighty_samples_are_refused(sets, renderers):
    from scenedreamer_amd import fused
    E = sets(6, 24)
    vid, d2, rd, ori = _dev(E)
    with pytest.raises(RuntimeError, match="at most 79"):
        fused.encode(renderers(6), vid, d2, rd, ori, 80)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------- sdn_field_encode

def _check_encode(R, E, weights, lut, u=None, global_enc=None, name=""):
    """fused.encode on the set against forward_perpix's aux: labels, distances (bits; padding slots exactly 0), ray flags,
    features of hit rays within 5e-6 (tests/test_fused_gpu.py test_encode_matches_oracle's bound), exactly 0 where the oracle's
    are (out-of-range samples).  Returns the fraction of out-of-range samples among the hit rays."""
    from scenedreamer_amd import fused
    vid, d2, rd, ori = _dev(E)
    genc = R.global_enc.cpu().numpy() if global_enc is None else global_enc
    kw = {} if u is None else dict(u=torch.from_numpy(u).cuda().contiguous(), division="ieee")
    buf = fused.encode(R, vid, d2, rd, ori, E.ns, **kw)
    torch.cuda.synchronize()
    _, aux = EE.oracle_field(weights, lut, E, R.z.cpu().numpy(), genc, rand=u)
    n, ns = E.n, E.ns
    feat, dist, label = FL.decode_encode_buffers(buf, n, ns)
    ref_idx = aux["new_idx"].numpy().reshape(n, ns)
    red = np.asarray(lut)[E.voxel_id]
    red[red == 0] = 3
    np.testing.assert_array_equal(label[:, :ns], np.take_along_axis(red, ref_idx, axis=1))
    ref_dist = (aux["new_dists"].numpy().reshape(n, ns) * np.float32(EE.DISTS_SCALE)).astype(np.float32)
    np.testing.assert_array_equal(bits(dist[:, :ns]), bits(ref_dist))
    assert not dist[:, ns:].view(np.int32).any(), "a padding slot's distance is not +0"
    flags = buf["rayflag"].cpu().numpy()
    sky_only = aux["sky_only"].numpy().reshape(-1)
    np.testing.assert_array_equal((flags & 1).astype(bool), sky_only)
    np.testing.assert_array_equal(((flags >> 1) & 1).astype(bool), aux["nosky"].numpy().reshape(-1))
    assert not (flags >> 2).any()
    # rays that hit nothing get weight 0 (scenedreamer.py:376): the kernel neither gathers nor (for a tile of 8 such rays) writes
    # their features
    hit = ~sky_only
    ref_feat = aux["feature_in"].numpy().reshape(n, ns, 16, 8)[hit]
    got = feat[:, :ns][hit]
    e = float(np.abs(got - ref_feat).max())
    zero = ~ref_feat.reshape(ref_feat.shape[0], ns, 128).any(axis=-1)
    print(f"{name}: {n} rays, {int(hit.sum())} hit, features max abs err {e:.2e}, {100 * zero.mean():.1f} % of their samples out of range")
    np.testing.assert_allclose(got, ref_feat, rtol=0, atol=5e-6)
    assert not np.abs(got[zero]).any(), "a feature of an out-of-range sample is not 0"
    return float(zero.mean())


@pytest.mark.parametrize("case", EE.CASES, ids=IDS)
def test_encode_on_the_edge_set(sets, renderers, weights_full, lut, case):
    M, ns = case
    oob = _check_encode(renderers(M), sets(M, ns), weights_full, lut, name=f"encode M={M} ns={ns}")
    assert 0 < oob < 0.5


def test_encode_on_the_edge_set_with_stochastic_sampling(sets, renderers, weights_full, lut):
    """M = 8 with a given stratified draw u (division="ieee": the oracle runs on the CPU)."""
    E = sets(8, 24)
    _check_encode(renderers(8), E, weights_full, lut, u=EE.stratified_u(E.n, E.ns, seed=1), name="encode M=8 ns=24 stochastic")


# ----------------------------------------------------------------------------------------------------- global_enc

def _genc_with_whole_level0_position():
    """A global_enc value (other than 0) whose level-0 grid position ((g + 1) / 2 * 15 + 0.5, one fp32 rounding per operation)
    has fractional part exactly 0: searched around the values (2 k + 1) / 15 - 1."""
    one, two = np.float32(1), np.float32(2)
    for k in (1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13):
        g = np.float32((2 * k + 1) / 15 - 1)
        for _ in range(64):
            g = np.nextafter(g, np.float32(-2))
        for _ in range(128):
            pos = np.float32(np.float32(np.float32(np.float32(g + one) / two) * np.float32(15)) + np.float32(0.5))
            if pos == np.float32(k + 1):
                return float(g)
            g = np.nextafter(g, np.float32(2))
    raise AssertionError("no such value")


# (1.0000001, 0) is the float 1 + 2^-23: (g + 1) / 2 rounds to exactly 1.0 in fp32 -- inside, for the reference as for the
# kernels; 1.0000002 = 1 + 2^-22 is the first value above 1 that is out of range, -1.0000001 the first below -1.
GENC = ((-1.0, -1.0), (1.0, 1.0), (-1.0, 1.0), (0.0, 0.0), (_genc_with_whole_level0_position(), 0.3), (1.0000001, 0.0),
        (1.0000002, 0.0), (0.3, -1.0000001))
GENC_OUT_OF_RANGE = {(1.0000002, 0.0), (0.3, -1.0000001)}


@pytest.mark.parametrize("genc", GENC, ids=lambda g: f"{g[0]:.9g}_{g[1]:.9g}")
def test_global_enc_edges(sets, renderers, weights_full, lut, genc):
    """The table collapse (sdn_field_collapse_table) at global_enc's edges, M = 6: +-1 (grid coordinate 0 / 1), a whole grid
    position, just inside and just outside the range.  Encode features against the oracle's 5-D lookup; out of range: every
    feature exactly 0 (the oracle's are, too) and the whole field still matches forward_perpix (_check_field's rules)."""
    R, E = renderers(6), sets(6, 24)
    g = np.asarray([genc], np.float32)
    x01 = (g + np.float32(1)) / np.float32(2)
    out = bool(((x01 < 0) | (x01 > 1)).any())
    assert out == (genc in GENC_OUT_OF_RANGE)
    keep = R.global_enc
    R.global_enc = torch.from_numpy(g).cuda()
    R._fused_scene = None
    try:
        oob = _check_encode(R, E, weights_full, lut, global_enc=g, name=f"global_enc {genc}")
        assert (oob == 1.0) == out
        if out:
            _check_field(R, E, weights_full, lut, g, f"edge rays M=6 num_samples=24, global_enc {genc} (out of range)")
    finally:
        R.global_enc = keep
        R._fused_scene = None


# ----------------------------------------------------------------------------------------------------- the kernels behind the stage

def _check_field(R, E, weights, lut, global_enc, name):
    """The rules of tests/test_arithmetic_gpu.py on a ray set: encode -> mlp (colour_terms = 3, term_eps = 0) within 4 x E3 of fp64
    on exactly the values the MLP kernel read; fused.field_fused as ONE kernel the same bits; fused.field_exact within 4 x E32 of
    forward_perpix in float64 (on the oracle's features and on the kernels').  The sky inputs are fused.sky_fused's on the same
    directions."""
    from oracle import split_ref as SR
    from scenedreamer_amd import fused
    vid, d2, rd, ori = _dev(E)
    n, ns = E.n, E.ns
    R.set_precision(colour_terms=3, term_eps=0.0)
    try:
        R.field_single_kernel = False
        net_out, given, (_, _, _, _, sky_c, sky_avg) = FL.two_kernel_field(R, vid, d2, rd, ori, ns)
        R.field_single_kernel = True
        with torch.no_grad():
            one = fused.field_fused(R, vid, d2, rd, ori, sky_c, sky_avg, ns)
            exact = fused.field_exact(R, vid, d2, rd, ori, sky_c, sky_avg, ns)
            torch.cuda.synchronize()
    finally:
        R.field_single_kernel = None
        R.set_precision()
    assert torch.isfinite(net_out).all() and torch.isfinite(exact).all()
    assert 1.0 - float(given["sky_only"].float().mean()) >= 0.2
    truth, emu, yard = FL.field_references(R, weights, given)
    FL.check(f"{name}: sdn_field_mlp net_out", net_out.cpu(), truth, emu, yard)
    assert torch.equal(one, net_out)
    kw = dict(sky_avg=given["sky_avg"].reshape(1, 1, 1, 1, 64), sky_c=given["sky_c"].reshape(1, 1, n, 1, 64), volume_rendering=SR.volum_rendering_relu)
    args = (weights, lut, E, R.z.cpu().numpy(), global_enc)
    f32, aux = EE.oracle_field(*args, **kw)
    f64, _ = EE.oracle_field(*args, dtype=torch.float64, **kw)
    feat = given["feat"].reshape(1, 1, n, ns, 128)
    k32, _ = EE.oracle_field(*args, feature_in=feat, **kw)
    k64, _ = EE.oracle_field(*args, feature_in=feat, dtype=torch.float64, **kw)
    ref_dist = aux["new_dists"].reshape(n, ns) * np.float32(EE.DISTS_SCALE)
    assert torch.equal(ref_dist.view(torch.int32), given["dist"].view(torch.int32))         # the kernel's placement IS the oracle's
    ex = exact.cpu()
    FL.check_fp32(f"{name}: field_exact vs forward_perpix fp64 (oracle features)", ex, f64.reshape(n, 64), f32.reshape(n, 64))
    FL.check_fp32(f"{name}: field_exact vs forward_perpix fp64 (kernel features)", ex, k64.reshape(n, 64), k32.reshape(n, 64))


FIELD_CASES = tuple((M, 6) for M in EE.MS) + ((2, 79), (8, 24))


@pytest.mark.parametrize("case", FIELD_CASES, ids=lambda c: f"M{c[0]}-ns{c[1]}")
def test_field_kernels_on_the_edge_set(sets, renderers, weights_full, lut, case):
    """The MLP / compositing kernels behind the encode stage on the edge rays, for each M (_check_field)."""
    M, ns = case
    R = renderers(M)
    _check_field(R, sets(M, ns), weights_full, lut, R.global_enc.cpu().numpy(), f"edge rays M={M} num_samples={ns}")
