"""The edge-case ray sets of tests/encode_edges.py, qualified without a GPU: before a kernel sees them,

  * the oracle's own output on them contains every edge the GPU tests rely on (coverage: conditions on the inputs, not
    measurements -- if a set fails one, the generator changes, not the condition);
  * every single-line defect of the placement / the ground test / the out-of-range test changes a discrete output or the bits
    of a depth or distance on them (so a kernel with that defect cannot pass tests/test_encode_edges_gpu.py);
  * the oracle's placement IS the unmodified reference's on them, bit for bit (needs_reference)."""
import inspect
import textwrap
import types

import numpy as np
import pytest
import torch

import encode_edges as EE
from conftest import bits

IDS = [f"M{M}-ns{ns}" for M, ns in EE.CASES]


@pytest.fixture(scope="module")
def sets():
    return {c: EE.rays(*c) for c in EE.CASES}


def _world(E, depth):
    """scenedreamer.py:350-354 on the oracle's raw depths: NaN / inf -> 0, then raydirs * depth + cam_ori in fp32."""
    bad = np.isnan(depth) | np.isinf(depth)
    d0 = np.where(bad, np.float32(0), depth).astype(np.float32)
    return (E.raydirs[:, None, :] * d0[:, :, None]).astype(np.float32) + E.cam_ori, bad


def _labels(E, idx, lut):
    red = np.asarray(lut)[E.voxel_id]
    red[red == 0] = 3
    return np.take_along_axis(red, np.minimum(idx, E.M - 1), axis=1)


@pytest.mark.parametrize("case", EE.CASES, ids=IDS)
def test_edge_set_covers_what_it_claims(sets, lut, case):
    M, ns = case
    E = sets[case]
    assert E.n % 8 and E.n % 32 and 100 <= E.n <= 400
    depth, dist, idx = EE.oracle_placement(E)
    mid, accu = EE.placement_internals(E)
    assert (idx == (mid[:, :, None] > accu[:, None, :]).sum(-1)).all()        # the internals are the oracle's
    hit = E.voxel_id[:, 0] != 0
    assert hit.mean() >= 0.20 and (~hit).mean() >= 0.05
    assert idx.max() == M - 1
    for k in range(M):
        assert (idx[hit] == k).mean() >= 0.01, f"box {k} is taken by {(idx[hit] == k).mean():.4f} of the samples"
    # an exact tie mid == accu[k] below the last prefix (M = 1 has one prefix, the total: a tie needs a zero-length ray there)
    ties = (mid[:, :, None] == accu[:, None, :])[hit]
    assert ties[:, :, :max(M - 1, 1)].any()
    if M >= 2:
        tie_rays = np.char.startswith(E.tag.astype(str), "tie_")
        t = mid[tie_rays][:, :, None] == accu[tie_rays][:, None, :M - 1]
        assert t.any(axis=(1, 2)).all()                                       # every constructed tie IS one ...
        s, k = np.nonzero(t.any(axis=0))[0][0], np.nonzero(t.any(axis=0))[1][0]
        r = np.nonzero(t[:, s, k])[0][0]
        assert idx[tie_rays][r, s] <= k                                       # ... and the sample stays in the lower box
    world, bad = _world(E, depth)
    assert bad[hit].any() and not bad[hit].all()                              # a depth of a HIT ray replaced by 0
    x, oob, gnd = EE.decisions(world, E.voxel_dims)
    wx = world[..., 0]
    assert (wx == 1.0).any() and (wx == np.nextafter(np.float32(1), np.float32(2))).any()
    for a in range(3):
        for v in (0.0, 1.0, EE.BELOW_ZERO, EE.ABOVE_ONE):
            assert (x[hit][..., a] == np.float32(v)).any(), (a, v)
    assert oob[hit].any() and (~oob[hit]).mean() > 0.5
    nosky = (E.voxel_id[:, -1] != 0) | gnd.any(axis=1)
    assert nosky[hit].any() and gnd[hit].any() and (~gnd[hit].any(axis=1)).any()
    assert M == 1 or (~nosky[hit]).any()                                      # (M = 1: a hit ray's only box is its last)
    lab = _labels(E, idx, lut)
    want = set(np.asarray(lut).tolist()) - {0}
    assert set(lab.reshape(-1).tolist()) == want, "a reduced label is missing"
    assert E.voxel_id.max() == EE.F32_MAX_ID == len(lut) - 1
    # the total depth below, at and far above sample_depth
    tot = accu[:, -1]
    assert (tot[hit] < 3).any() and (tot == 3).any() and (tot > 1e3).any() and np.isinf(tot).any()


@pytest.mark.parametrize("case", [(3, 6), (8, 24), (1, 24), (2, 79)], ids=lambda c: f"M{c[0]}-ns{c[1]}")
def test_decisions_helper_is_the_oracles(sets, weights_full, lut, case):
    """encode_edges.decisions (grid coordinates, out-of-range, ground) restates in numpy what forward_perpix and the C oracle's
    grid encoder decide: the same world coordinates, features exactly zero where (and only where) it says out-of-range, the
    same nosky flag."""
    import field_layout as FL
    E = sets[case]
    _, aux = EE.oracle_field(weights_full, lut, E, FL.style_code(), np.zeros((1, 2), np.float32))
    depth, _, idx = EE.oracle_placement(E)
    world, _ = _world(E, depth)
    assert np.array_equal(bits(aux["worldcoord2"].numpy().reshape(E.n, E.ns, 3)), bits(world))
    assert np.array_equal(aux["new_idx"].numpy().reshape(E.n, E.ns), idx)
    x, oob, gnd = EE.decisions(world, E.voxel_dims, np.zeros(2, np.float32))
    zero = ~aux["feature_in"].numpy().reshape(E.n, E.ns, 128).any(axis=-1)
    assert np.array_equal(zero, oob)
    nosky = (E.voxel_id[:, -1] != 0) | gnd.any(axis=1)
    assert np.array_equal(aux["nosky"].numpy().reshape(-1), nosky)
    assert np.array_equal(aux["sky_only"].numpy().reshape(-1), E.voxel_id[:, 0] == 0)


# --------------------------------------------------------------------------- single-defect sensitivity

def _mutant(fn, old, new):
    """`fn` with ONE line of its source changed (old -> new, which must occur exactly once), compiled in a copy of its module."""
    src = textwrap.dedent(inspect.getsource(fn))
    assert src.count(old) == 1, (fn.__name__, old, src.count(old))
    env = dict(vars(inspect.getmodule(fn)))
    exec(compile(src.replace(old, new), f"<{fn.__name__}: {old} -> {new}>", "exec"), env)
    return env[fn.__name__]


def _subset(E, keep):
    return types.SimpleNamespace(voxel_id=E.voxel_id[keep], depth2=E.depth2[:, keep], raydirs=E.raydirs[keep], cam_ori=E.cam_ori,
                                 tag=E.tag[keep], voxel_dims=E.voxel_dims, M=E.M, ns=E.ns, n=int(keep.sum()))


def _placement_differs(E, old, new, rand=None):
    from oracle import field_ref as FR
    a = EE.oracle_placement(E, rand)
    b = EE.oracle_placement(E, rand, fn=_mutant(FR.sample_depth_batched, old, new))
    return (not np.array_equal(a[2], b[2])) or (not np.array_equal(bits(a[0]), bits(b[0]))) or (not np.array_equal(bits(a[1]), bits(b[1])))


# (what, old line, new line, smallest M at which the defect can show at all)
PLACEMENT_MUTANTS = (
    # M = 1: the only prefix is the total, and a midpoint is below the total unless the total is zero
    (">= for > in the box count", "midpoints.unsqueeze(-3) > accu_depth", "midpoints.unsqueeze(-3) >= accu_depth", 2),
    # the float32 sum of TWO floats is the rounded exact sum, which is also what the double accumulation rounds to
    ("prefix sum carried in float32", "accu_depth = torch.cumsum(dists, dim=-2)",
     "accu_depth = torch.from_numpy(np.cumsum(dists.numpy(), axis=-2, dtype=np.float32))", 3),
    ("sample_depth clamp dropped", "total_depth = torch.clamp(total_depth, None, sample_depth)", "total_depth = total_depth + 0", 1),
    ("NaN box lengths not zeroed", "dists[torch.isnan(dists)] = 0", "pass", 1),
    ("head taken from box idx - 1", "heads = torch.gather(depth_deltas, -2, idx)",
     "heads = torch.gather(depth_deltas, -2, (idx - 1).clamp(min=0))", 2),
)


@pytest.mark.parametrize("case", EE.CASES, ids=IDS)
@pytest.mark.parametrize("mutant", PLACEMENT_MUTANTS, ids=lambda m: m[0].replace(" ", "_"))
def test_placement_defects_show_on_the_edge_set(sets, mutant, case):
    what, old, new, m_min = mutant
    E = sets[case]
    if what.startswith(">="):
        # on a ray whose total depth is zero (sky-only rays, a single zero-length box) EVERY midpoint equals EVERY prefix: the
        # defect counts M boxes there and the reference's gather raises.  The defect has to show without those rays.
        E = _subset(E, EE.placement_internals(E)[1][:, -1] > 0)
    differs = _placement_differs(E, old, new)
    assert differs == (E.M >= m_min), what


@pytest.mark.parametrize("case", EE.CASES, ids=IDS)
def test_stratified_division_defect_shows_on_the_edge_set(sets, case):
    """rand * (1 / n) for rand / n in the stochastic branch: 1 ulp apart -- unless n = num_samples + 1 is a power of two, where
    the two are the same operation."""
    E = sets[case]
    n = E.ns + 1
    differs = _placement_differs(E, "rand_samples = rand_samples / nsamples", "rand_samples = rand_samples * (1.0 / nsamples)",
                                 rand=EE.stratified_u(E.n, E.ns))
    assert differs == (n & (n - 1) != 0)


@pytest.mark.parametrize("case", EE.CASES, ids=IDS)
def test_ground_and_range_defects_show_on_the_edge_set(sets, weights_full, lut, case):
    """`<` for `<=` in is_gnd (forward_perpix itself, one line changed: the nosky flag moves); `<=` / `>=` for the strict
    out-of-range tests (encode_edges.decisions, which test_decisions_helper_is_the_oracles ties to the C oracle).
    M = 1: nosky = (id[0] != 0) or is_gnd, and a ray with id[0] == 0 hits nothing -- all its samples sit at the camera: the
    ground test cannot reach the flag there, it shows from M = 2 on."""
    import field_layout as FL
    from oracle import field_ref as FR
    E = sets[case]
    zeros = dict(feature_in=torch.zeros(1, 1, E.n, E.ns, 128), sky_c=torch.zeros(1, 1, E.n, 1, 64), sky_avg=torch.zeros(1, 1, 1, 1, 64))
    args = (weights_full, lut, E, FL.style_code(), np.zeros((1, 2), np.float32))
    a = EE.oracle_field(*args, **zeros)[1]["nosky"]
    b = EE.oracle_field(*args, fn=_mutant(FR.forward_perpix, "<= 1.0).any(", "< 1.0).any("), **zeros)[1]["nosky"]
    assert (not torch.equal(a, b)) == (E.M >= 2)
    world, _ = _world(E, EE.oracle_placement(E)[0])
    oob = EE.decisions(world, E.voxel_dims)[1]
    for old, new in (("(x < 0)", "(x <= 0)"), ("(x > 1)", "(x >= 1)")):
        assert not np.array_equal(_mutant(EE.decisions, old, new)(world, E.voxel_dims)[1], oob), (old, new)


# --------------------------------------------------------------------------- the oracle is the reference on these inputs

@pytest.mark.needs_reference
@pytest.mark.parametrize("case", EE.CASES, ids=IDS)
def test_oracle_placement_is_the_references_on_the_edge_set(sets, case):
    """The UNMODIFIED mc_utils.sample_depth_batched (CPU, use_box_boundaries=False), deterministic and with a given torch.rand
    draw, against oracle/field_ref.py's: box indices equal, depths and distances bit for bit, NaN positions included."""
    from unittest import mock

    from oracle import ref_harness as RH
    RH.install("oracle")
    from imaginaire.model_utils.gancraft import mc_utils
    E = sets[case]
    d2 = torch.from_numpy(EE.oracle_shapes(E)[1])
    u = EE.stratified_u(E.n, E.ns)
    for rand in (None, u):
        r = None if rand is None else torch.from_numpy(rand).reshape(1, 1, E.n, E.ns + 1, 1)
        with mock.patch.object(torch, "rand", lambda *a, **k: r.clone()):
            ref = mc_utils.sample_depth_batched(d2.clone(), E.ns + 1, deterministic=rand is None, use_box_boundaries=False,
                                                sample_depth=EE.SAMPLE_DEPTH)
        got = EE.oracle_placement(E, rand)
        assert np.array_equal(ref[2].reshape(E.n, E.ns).numpy(), got[2])
        assert np.array_equal(bits(ref[0].reshape(E.n, E.ns).numpy()), bits(got[0]))
        assert np.array_equal(bits(ref[1].reshape(E.n, E.ns).numpy()), bits(got[1]))
