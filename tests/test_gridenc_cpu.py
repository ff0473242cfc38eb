"""tests/gridenc_ref.py earns its place: the fp64 model of the hash-grid encoder agrees with the CPU oracle (values to fp32
rounding, the discrete part exactly), the cases contain the edge rows they claim, every defect knob moves the model by more than
the bound tests/test_gridenc_gpu.py applies (so that test would see the defect in a kernel), and the exact scatter cases are
exact.  No GPU."""
import numpy as np
import pytest

import gridenc_ref as G

ALL = [("case",) + c for c in G.CASES] + list(G.EXTRA)


def _get(key):
    return G.case(*key[1:]) if key[0] == "case" else G.extra(key)


def _id(key):
    return "-".join(str(int(k)) if isinstance(k, (bool, np.bool_)) else str(k) for k in key)


@pytest.fixture(scope="module")
def fwd(oracle):
    """key -> (model features, model dy_dx, oracle features, oracle dy_dx), computed once."""
    memo = {}

    def get(key):
        if key not in memo:
            c = _get(key)
            memo[key] = G.model(c.x, c.emb, *c.args(), want_dy=True) + oracle.grid_encode_fwd(c.x, c.emb, c.offs, c.S, c.H, True, c.gridtype, c.align)
        return memo[key]
    return get


def test_offsets_are_the_modules():
    from scenedreamer_amd.gridencoder import level_offsets
    for a in ((5, 2, 512, 4, 12, False), (2, 2, 512, 4, 12, True), (5, 1, 1, 8, 12, True), (2, 40, 1, 9, 12, False), (3, 3, 1, 9, 8, True)):
        np.testing.assert_array_equal(G.level_offsets(*a), level_offsets(*a))


@pytest.mark.parametrize("key", ALL, ids=_id)
def test_model_agrees_with_oracle(fwd, key):
    """Features and dy_dx: within what fp32 arithmetic can differ from fp64 on these sizes (gridenc_ref.fwd_bound); a wrong cell,
    row or weight is 1e-1.  Out-of-range rows are zero in both."""
    c = _get(key)
    m_out, m_dy, o_out, o_dy = fwd(key)
    scale_max = max(s for s, _ in G.levels(c.L, c.S, c.H))
    b_out, b_dy = G.fwd_bound(c.D, scale_max, 0.5)
    e_out, e_dy = np.abs(o_out - m_out).max(), np.abs(o_dy - m_dy).max()
    print(f"{c.name:28s} E32 features {e_out:.2e} (bound {b_out:.2e})  dy_dx {e_dy:.2e} (bound {b_dy:.2e})")
    assert 0 < e_out <= b_out and 0 < e_dy <= b_dy
    oob = G.out_of_range(c.x)
    assert not m_out[:, oob].any() and not m_dy[oob].any() and not o_out[:, oob].any() and not o_dy[oob].any()
    assert m_out[:, ~oob].any(axis=2).all()


@pytest.mark.parametrize("key", [k for k in ALL if k[0] != "case" or k[2] in (1, 8)], ids=_id)
def test_discrete_model_is_the_oracles(oracle, key):
    """Cell indices and table rows of every corner, on the edge rows and a few random ones, against oracle.grid_index."""
    c = _get(key)
    edge = sorted(i for v in c.classes.values() for i in v[:2])
    pick = np.array(edge[:: max(1, len(edge) // 24)] + [0, c.B - 1])
    for l in sorted({0, c.L - 1}):
        pg, rows, oob = G.corner_rows(c.x[pick], c.offs, c.S, c.H, c.gridtype, c.align, l)
        np.testing.assert_array_equal(oob, ((c.x[pick] < 0) | (c.x[pick] > 1)).any(1))
        scale, res = oracle.level_params(l, c.S, c.H)
        T = int(c.offs[l + 1] - c.offs[l])
        for i in range(len(pick)):
            if oob[i]:
                continue
            pos = c.x[pick[i]] * np.float32(scale) + np.float32(0.0 if c.align else 0.5)
            np.testing.assert_array_equal(pg[i], np.floor(pos).astype(np.int64))
            for idx in range(1 << c.D):
                pgl = [int(pg[i, d]) + ((idx >> d) & 1) for d in range(c.D)]
                assert oracle.grid_index(c.D, c.C, c.gridtype, c.align, T, res, pgl) == rows[i, idx] * c.C


@pytest.mark.parametrize("key", [k for k in ALL if k[0] != "case" or k[2] in (1, 4)], ids=_id)
def test_bwd_model_agrees_with_oracle(oracle, fwd, key):
    """grad_grid and grad_inputs against the oracle (fp32 contributions summed in double; fp32 chain): the bounds of the GPU test."""
    c = _get(key)
    o_dy = fwd(key)[3]
    r = G.bwd_model(c.x, c.grad, *c.args(), dy_dx=o_dy)
    gg, gi = oracle.grid_encode_bwd(c.grad, c.x, c.emb.shape, c.offs, c.S, c.H, o_dy, c.gridtype, c.align)
    assert (np.abs(gg - r["grad_grid"]) <= G.grid_grad_bound(r, c.D)).all()
    assert (np.abs(gi - r["grad_inputs"]) <= G.input_grad_bound(r, c.L, c.C)).all()
    assert (gg[r["n"] == 0] == 0).all() and (r["n"] == 0).any() and (r["n"] > 1).any()
    assert not gi[G.out_of_range(c.x)].any()


@pytest.mark.parametrize("key", ALL, ids=_id)
def test_cases_contain_their_edge_rows(key):
    c = _get(key)
    assert c.B % 64 != 0 and c.x.dtype == np.float32 and not np.isnan(c.x).any()
    oob = G.out_of_range(c.x)
    for name in ("zero", "negzero", "one", "below_one", "denormal"):
        assert len(c.classes[name]) >= 2 and not oob[c.classes[name]].any(), name
    x = c.x
    assert (x[c.classes["zero"][0]] == 0).all() and not np.signbit(x[c.classes["zero"][0]]).any()
    assert np.signbit(x[c.classes["negzero"][0]]).all() and (x[c.classes["negzero"][0]] == 0).all()
    assert (x[c.classes["one"][0]] == 1).all() and (x[c.classes["below_one"][0]] == np.float32(1) - np.float32(2.0 ** -24)).all()
    assert (x[c.classes["denormal"][0]].view(np.uint32) == 1).all()
    assert (x[c.classes["oob:above_one"]].view(np.uint32) == 0x3F800001).any(1).all() and oob[c.classes["oob:above_one"]].all()
    assert (x[c.classes["oob:neg_denormal"]].view(np.uint32) == 0x80000001).any(1).all() and oob[c.classes["oob:neg_denormal"]].all()
    for d in range(c.D):                    # exactly coordinate d is out of range, once on each side
        rows = x[c.classes["oob:dim%d" % d]]
        bad = (rows < 0) | (rows > 1)
        assert bad[:, d].all() and bad.sum() == len(rows) == 2 and (rows[:, d] < 0).any() and (rows[:, d] > 1).any()
    for i in np.flatnonzero(oob):           # an in-range sample in the same 4-lane quad (and so in the same wave)
        q = np.arange(i // 4 * 4, min(i // 4 * 4 + 4, c.B))
        assert (~oob[q]).any()
    scales = {}
    for l, (scale, _) in enumerate(G.levels(c.L, c.S, c.H)):
        scales.setdefault(scale, l)
    for scale, l in scales.items():         # per level: pos exactly on a cell boundary, just under and just over one
        rows = np.array(sum((c.classes["boundary:L%d:%s" % (l, k)] for k in ("on", "under", "over", "all")), []))
        assert not oob[rows].any()
        _, frac = G.place(x[rows], scale, c.align)
        ulp = np.spacing(np.float32(max(scale, 1.0)))
        assert (frac == 0).any() and (frac >= 1 - 8 * ulp).any() and ((frac > 0) & (frac <= 8 * ulp)).any(), (l, scale)


def _separable(key, defect):
    """Whether `defect` CAN change the result of a case, from what the defect is."""
    c = _get(key)
    overflow = key[0] != "many_levels"        # CASES' level 1 and STRIDE_EQ overflow their table; MANY_LEVELS is dense
    if defect == "contract":                  # with align_corners the offset is 0.0: x * scale + 0 rounds once either way; and
        return not c.align and key[0] != "many_levels"      # MANY_LEVELS' scale is 8: x * 8 is exact, one rounding either way
    if defect == "prime4":                    # the fifth prime multiplies the fifth coordinate of a HASHED level
        return c.D == 5 and c.gridtype == 0 and overflow
    if defect == "stride_lt":                 # needs a stride that EQUALS the table size: STRIDE_EQ's fifth (4096).  There `<`
        return key == ("stride_eq", 0)        # drops pos_grid[4] * 4096, a multiple of the size (no change after `% size`), and
    #                                         # leaves stride at 4096 = size: "not overflowed", so the hash grid is not hashed --
    #                                         # the TILED form cannot show it, in any configuration
    if defect == "hash_tiled":                # hashing where the grid is tiled: a tiled level that overflows
        return c.gridtype == 1 and overflow
    if defect == "side_swap":                 # the side enters the stride walk only: a level that is hashed does not use it, and
        return key != ("stride_eq", 0)        # STRIDE_EQ's single level overflows with either side
    return True                               # oob_ge: every case has x == 1.0 rows


def test_every_defect_moves_the_model_beyond_the_gpu_bound(fwd):
    """For every case and knob: max |model(defect) - model| over the features > 4 x E32 of that case (the GPU test's bound, E32 =
    the oracle's fp32 error on the same inputs) exactly where the defect can act at all (_separable), and == 0 elsewhere."""
    missed, ghost, closest = [], [], {}
    for key in ALL:
        c = _get(key)
        m_out, _, o_out, _ = fwd(key)
        bound = 4 * np.abs(o_out - m_out).max()
        for defect in G.DEFECTS:
            moved = np.abs(G.model(c.x, c.emb, *c.args(), defect=defect) - m_out).max()
            if _separable(key, defect):
                closest[defect] = min(closest.get(defect, np.inf), moved / bound)
                if not moved > bound:
                    missed.append((c.name, defect, moved, bound))
            elif moved != 0:
                ghost.append((c.name, defect, moved))
    for d in G.DEFECTS:
        print(f"{d:12s} smallest movement / (4 x E32) over the cases where it can act: {closest[d]:.1f}")
    assert not missed, missed
    assert not ghost, ghost
    assert set(closest) == set(G.DEFECTS)


@pytest.mark.parametrize("identical", [False, True])
@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("D,C", G.DC)
def test_exact_scatter_cases_are_exact(oracle, D, C, align, identical):
    """The builder's own asserts (fractions 0 / 0.5, integer sums below the format's limit) ran; both oracles and the fp64 model
    give the same integer table, heavy collisions included."""
    for dtype in ("f16", "f32"):
        e = G.exact_scatter_case(D, C, align, dtype, identical)
        assert e.A.max() <= e.limit and e.n.max() >= (257 if identical else 8) and np.abs(e.expected).max() >= 8
        assert G.out_of_range(e.x).any() != identical
        shape = (int(e.offs[-1]), C)
        g32, _ = oracle.grid_encode_bwd(e.grad, e.x, shape, e.offs, e.S, e.H, None, 0, align)
        g16, _ = oracle.grid_encode_bwd_f16(e.grad.astype(np.float16), e.x, shape, e.offs, e.S, e.H, None, 0, align)
        np.testing.assert_array_equal(g32.astype(np.float64), e.expected)
        np.testing.assert_array_equal(g16.astype(np.float64), e.expected)
        if C == 1:                                # neighbouring rows (one 32-bit word in the f16 table) both written
            both = (e.n[0::2] > 0) & (e.n[1::2] > 0)
            assert both.any()
