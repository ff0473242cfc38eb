"""The hash-grid encoder's kernels (csrc/gridenc.hip) on the MI355X, every instantiation, against the fp64 model of
tests/gridenc_ref.py (qualified by tests/test_gridenc_cpu.py): the f32 forward of BOTH kernels -- the quad-cooperative one that
runs without dy_dx and the one-lane one that runs with it -- within 4 x E32 (tests/field_layout.py: E32 = the CPU oracle's own fp32
error on the same inputs), bit-identical rows whatever the launch shape, f16 tables bit for bit, the table gradient exactly on
configurations whose sums are exact in any order, and on general values within the recursive-summation bound.  Everything goes
through scenedreamer_amd.ops -> ctypes -> the C ABI.  Each arithmetic check prints its ratio; SDN_ARITH_RECORD=<file> collects
them as JSON (profiles/gridenc_arithmetic.json)."""
import numpy as np
import pytest
import torch

import field_layout as FL
import gridenc_ref as G

pytestmark = pytest.mark.gpu

RECORD = FL.RECORD
_record_file = FL.record_file_fixture()
ALL = [("case",) + c for c in G.CASES] + list(G.EXTRA)


def _get(key):
    return G.case(*key[1:]) if key[0] == "case" else G.extra(key)


def _id(key):
    return "-".join(str(int(k)) if isinstance(k, (bool, np.bool_)) else str(k) for k in key)


@pytest.fixture(scope="module")
def ops():
    from scenedreamer_amd import capi, ops
    capi.lib()
    assert torch.cuda.is_available()
    return ops


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _forward(ops, c, x, emb, with_dy):
    """ops.grid_encode_forward on x [B,D] (GPU) with the table emb (GPU, f32 or f16) of configuration c: (out [L,B,C], dy_dx).
    with_dy = False and an f32 table is the quad kernel; anything else the one-lane kernel."""
    B = x.shape[0]
    out = torch.full((c.L, B, c.C), 7.0, device="cuda", dtype=emb.dtype)
    dy = torch.full((B, c.L * c.D * c.C) if with_dy else (1,), 7.0, device="cuda", dtype=emb.dtype)
    ops.grid_encode_forward(x, emb, _cuda(c.offs), out, B, c.D, c.C, c.L, c.S, c.H, with_dy, dy, c.gridtype, c.align)
    torch.cuda.synchronize()
    return out.cpu().numpy(), (dy.cpu().numpy() if with_dy else None)


def _backward(ops, c, x, grad, shape, dy=None):
    """ops.grid_encode_backward: (grad_embeddings, grad_inputs | None) as numpy; the dtype is grad's."""
    B = x.shape[0]
    gg = torch.zeros(shape, device="cuda", dtype=grad.dtype)
    gi = torch.zeros((B, c.D) if dy is not None else (1,), device="cuda", dtype=grad.dtype)
    dd = dy if dy is not None else torch.zeros(1, device="cuda", dtype=grad.dtype)
    ops.grid_encode_backward(grad, x, torch.empty(shape, device="cuda", dtype=grad.dtype), _cuda(c.offs), gg, B, c.D, c.C, c.L, c.S,
                             c.H, dy is not None, dd, gi, c.gridtype, c.align)
    torch.cuda.synchronize()
    return gg.cpu().numpy(), (gi.cpu().numpy() if dy is not None else None)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint16)


# ----------------------------------------------------------------------------------------------------- forward, f32

@pytest.mark.parametrize("key", ALL, ids=_id)
def test_forward_f32_both_kernels_against_fp64(ops, oracle, key):
    """Quad kernel (no dy_dx) and one-lane kernel (with dy_dx): features and dy_dx within 4 x E32 of the fp64 model; out-of-range
    rows exactly zero; the rows at 0.0, -0.0, 1.0, just under 1.0 and the smallest denormal are NOT zero rows."""
    c = _get(key)
    truth, truth_dy = (torch.from_numpy(t) for t in G.model(c.x, c.emb, *c.args(), want_dy=True))
    yard, yard_dy = oracle.grid_encode_fwd(c.x, c.emb, c.offs, c.S, c.H, True, c.gridtype, c.align)
    x, emb = _cuda(c.x), _cuda(c.emb)
    quad, _ = _forward(ops, c, x, emb, False)
    lane, dy = _forward(ops, c, x, emb, True)
    oob = G.out_of_range(c.x)
    inside = sum((c.classes[k] for k in ("zero", "negzero", "one", "below_one", "denormal")), [])
    assert oob.any() and not oob[inside].any()
    for name, got in (("quad", quad), ("one-lane", lane)):
        assert not _bits(got[:, oob]).any(), name
        assert got[:, inside].any(axis=2).all(), name
        FL.check_fp32(f"grid fwd {c.name}: {name} features", got, truth, yard)
    assert not _bits(dy[oob]).any()
    assert dy[inside].any(axis=1).all()
    FL.check_fp32(f"grid fwd {c.name}: one-lane dy_dx", dy, truth_dy, yard_dy)


@pytest.mark.parametrize("i", range(len(G.DC)), ids=["D%d-C%d" % dc for dc in G.DC])
def test_forward_rows_do_not_depend_on_the_launch(ops, i):
    """The first k rows alone (k = 1: one live quad; 3, 63 .. 65: dead quads and lanes around a wave; 255, 257: the last partial
    workgroup) and the whole set behind 37 out-of-range rows (every row in another lane, quad and workgroup): each row has the
    bits it has in the full launch, in both kernels, dy_dx included."""
    D, C = G.DC[i]
    c = G.case(D, C, *G.FORMS[(i + i // 4) % 4])
    x, emb = _cuda(c.x), _cuda(c.emb)
    quad, _ = _forward(ops, c, x, emb, False)
    lane, dy = _forward(ops, c, x, emb, True)
    for k in (1, 3, 63, 64, 65, 255, 257, 777):
        xk = x[:k].contiguous()
        q, _ = _forward(ops, c, xk, emb, False)
        l, d = _forward(ops, c, xk, emb, True)
        np.testing.assert_array_equal(_bits(q), _bits(quad[:, :k]), err_msg=f"quad k={k}")
        np.testing.assert_array_equal(_bits(l), _bits(lane[:, :k]), err_msg=f"one-lane k={k}")
        np.testing.assert_array_equal(_bits(d), _bits(dy[:k]), err_msg=f"dy_dx k={k}")
    front = torch.full((37, D), 1.5, device="cuda")
    front[::2, 0] = -0.5
    xs = torch.cat([front, x]).contiguous()
    q, _ = _forward(ops, c, xs, emb, False)
    l, d = _forward(ops, c, xs, emb, True)
    assert not _bits(q[:, :37]).any() and not _bits(l[:, :37]).any() and not _bits(d[:37]).any()
    np.testing.assert_array_equal(_bits(q[:, 37:]), _bits(quad))
    np.testing.assert_array_equal(_bits(l[:, 37:]), _bits(lane))
    np.testing.assert_array_equal(_bits(d[37:]), _bits(dy))


# ----------------------------------------------------------------------------------------------------- forward, f16

@pytest.mark.parametrize("D,C", G.DC)
def test_forward_f16_tables_bit_exact(ops, oracle, D, C):
    """scalar_t = at::Half on every (D, C) and all four (gridtype, align_corners) forms, edge rows included: features and dy_dx
    equal the oracle's sequential half evaluation bit for bit."""
    for gridtype, align in G.FORMS:
        c = G.case(D, C, gridtype, align, B=301)
        emb16 = c.emb.astype(np.float16)
        out, dy = _forward(ops, c, _cuda(c.x), _cuda(emb16), True)
        ref, ref_dy = oracle.grid_encode_fwd_f16(c.x, emb16, c.offs, c.S, c.H, True, gridtype, align)
        np.testing.assert_array_equal(_bits(out), _bits(ref), err_msg=c.name)
        np.testing.assert_array_equal(_bits(dy), _bits(ref_dy), err_msg=c.name)
        out2, _ = _forward(ops, c, _cuda(c.x), _cuda(emb16), False)
        np.testing.assert_array_equal(_bits(out2), _bits(ref), err_msg=c.name + " without dy_dx")


# ----------------------------------------------------------------------------------------------------- table gradient

@pytest.mark.parametrize("D,C", G.DC)
def test_table_gradient_exact_in_any_order(ops, D, C):
    """gridenc_ref.exact_scatter_case: every contribution and partial sum is an integer the format holds exactly, so the atomics'
    order cannot matter and grad_embeddings must EQUAL the integer table: no lost compare-and-swap update (C = 1 half: two rows per
    32-bit word), no wrong half of the word, no dropped packed add, no wrong row -- under 300 rows colliding in 256-row tables
    and under 257 lanes hitting the same entries."""
    for align in (False, True):
        for dtype in ("f32", "f16"):
            for identical in (False, True):
                e = G.exact_scatter_case(D, C, align, dtype, identical)
                tdt = torch.float32 if dtype == "f32" else torch.float16
                gg, _ = _backward(ops, e, _cuda(e.x), _cuda(e.grad).to(tdt), (int(e.offs[-1]), C))
                np.testing.assert_array_equal(gg.astype(np.float64), e.expected,
                                              err_msg=f"D{D} C{C} align={align} {dtype} identical={identical}")


@pytest.mark.parametrize("D,C", G.DC)
def test_gradients_general_values(ops, oracle, D, C):
    """Random grad on the CASES inputs, all four forms.  f32: every table entry within (n + D + 2) 2^-24 A of the fp64 sum (n
    contributions of total magnitude A: the recursive-summation bound, any order), untouched entries exactly zero; grad_inputs
    (from the kernel's own dy_dx) within (L C + 2) 2^-24 A_in, out-of-range rows exactly zero.  f16: grad_inputs equal to the
    oracle's sequential half evaluation bit for bit."""
    for gridtype, align in G.FORMS:
        c = G.case(D, C, gridtype, align)
        x, oob = _cuda(c.x), G.out_of_range(c.x)
        shape = (int(c.offs[-1]), C)
        _, dy = _forward(ops, c, x, _cuda(c.emb), True)
        gg, gi = _backward(ops, c, x, _cuda(c.grad), shape, _cuda(dy))
        r = G.bwd_model(c.x, c.grad, *c.args(), dy_dx=dy)
        for what, got, want, bound in (("grad_embeddings", gg, r["grad_grid"], G.grid_grad_bound(r, D)),
                                       ("grad_inputs", gi, r["grad_inputs"], G.input_grad_bound(r, c.L, C))):
            err = np.abs(got - want)
            ratio = float((err / bound).max())
            name = f"grid bwd {c.name}: {what}"
            RECORD[name] = dict(kernel=float(err.max()), kernel_over_bound=ratio)
            print(f"{name:72s} max err {err.max():.2e}  largest err / bound {ratio:.3f}")
            assert (err <= bound).all(), name
        assert (r["n"] == 0).any() and not _bits(gg[r["n"] == 0]).any()
        assert not _bits(gi[oob]).any()

        emb16, grad16 = c.emb.astype(np.float16), c.grad.astype(np.float16)
        _, dy16 = _forward(ops, c, x, _cuda(emb16), True)
        gg16, gi16 = _backward(ops, c, x, _cuda(grad16), shape, _cuda(dy16))
        _, ref_gi = oracle.grid_encode_bwd_f16(grad16, c.x, shape, c.offs, c.S, c.H, dy16, gridtype, align)
        np.testing.assert_array_equal(_bits(gi16), _bits(ref_gi), err_msg=c.name)
        assert not _bits(gg16[r["n"] == 0]).any() and np.isfinite(gg16.astype(np.float32)).all()


def test_empty_batch_writes_nothing(ops):
    """B == 0: no launch, no error, no byte written -- forward (both kernels, f32 and f16) and backward."""
    c = G.case(3, 2, 0, False)
    x = _cuda(c.x[:4])
    for dt in (torch.float32, torch.float16):
        emb = _cuda(c.emb).to(dt)
        for with_dy in (False, True):
            out = torch.full((c.L, 4, c.C), 7.0, device="cuda", dtype=dt)
            dy = torch.full((4, c.L * c.D * c.C), 7.0, device="cuda", dtype=dt)
            ops.grid_encode_forward(x[:0], emb, _cuda(c.offs), out, 0, c.D, c.C, c.L, c.S, c.H, with_dy, dy, 0, False)
            torch.cuda.synchronize()
            assert (out == 7).all() and (dy == 7).all()
        gg, gi = torch.full_like(emb, 7.0), torch.full((4, c.D), 7.0, device="cuda", dtype=dt)
        grad = torch.ones(c.L, 4, c.C, device="cuda", dtype=dt)
        ops.grid_encode_backward(grad[:, :0].contiguous(), x[:0], emb, _cuda(c.offs), gg, 0, c.D, c.C, c.L, c.S, c.H, True,
                                 torch.ones(4, c.L * c.D * c.C, device="cuda", dtype=dt), gi, 0, False)
        torch.cuda.synchronize()
        assert (gg == 7).all() and (gi == 7).all()


# ----------------------------------------------------------------------------------------------------- module surface

def _module(c):
    from scenedreamer_amd.gridencoder import GridEncoder
    enc = GridEncoder(input_dim=c.D, num_levels=c.L, level_dim=c.C, per_level_scale=512, base_resolution=c.H, log2_hashmap_size=12,
                      gridtype="tiled" if c.gridtype else "hash", align_corners=c.align).cuda()
    np.testing.assert_array_equal(enc.offsets.cpu().numpy(), c.offs)
    enc.embeddings.data.copy_(_cuda(c.emb))
    xin = (c.x * np.float32(2) - np.float32(1)).astype(np.float32)            # the module maps [-1, 1] -> [0, 1] itself
    return enc, xin, ((xin + np.float32(1)) / np.float32(2)).astype(np.float32)


@pytest.mark.parametrize("D,gridtype,align", [(2, 1, False), (4, 1, False), (2, 0, True), (4, 0, True), (2, 1, True), (4, 1, True)])
def test_module_inference_tiled_and_aligned(ops, oracle, D, gridtype, align):
    """GridEncoder(gridtype="tiled") / (align_corners=True), inputs without requires_grad (the quad kernel): [B, L*C] within
    4 x E32 of the fp64 model."""
    c = G.case(D, 2, gridtype, align)
    enc, xin, x01 = _module(c)
    y = enc(_cuda(xin).reshape(7, 111, D))
    assert y.shape == (7, 111, c.L * c.C) and enc.gridtype_id == gridtype and enc.align_corners == align
    got = y.detach().cpu().numpy().reshape(c.B, c.L, c.C).transpose(1, 0, 2)
    truth = torch.from_numpy(G.model(x01, c.emb, *c.args()))
    yard = oracle.grid_encode_fwd(x01, c.emb, c.offs, c.S, c.H, False, gridtype, align)
    FL.check_fp32(f"GridEncoder {c.name}: inference", got, truth, yard)


def test_module_backward(ops, oracle):
    """One backward() through GridEncoder (tiled, align_corners, D = 4): embeddings.grad within the table-gradient bound of
    bwd_model; inputs.grad = 0.5 x grad_inputs (the module's [-1, 1] -> [0, 1] map), within the chain's bound plus what the
    kernel's dy_dx may differ from the model's by (4 x E32 of dy_dx, the forward test's bound) times sum |grad|."""
    c = G.case(4, 2, 1, True)
    enc, xin, x01 = _module(c)
    xt = _cuda(xin).requires_grad_(True)
    y = enc(xt)
    g = c.grad.transpose(1, 0, 2).reshape(c.B, c.L * c.C)
    y.backward(_cuda(g))
    truth_dy = G.model(x01, c.emb, *c.args(), want_dy=True)[1]
    yard_dy = oracle.grid_encode_fwd(x01, c.emb, c.offs, c.S, c.H, True, c.gridtype, c.align)[1]
    r = G.bwd_model(x01, c.grad, *c.args(), dy_dx=truth_dy)
    assert (np.abs(enc.embeddings.grad.cpu().numpy() - r["grad_grid"]) <= G.grid_grad_bound(r, c.D)).all()
    slack = FL.FACTOR * np.abs(yard_dy - truth_dy).max() * np.abs(c.grad).sum(axis=(0, 2))[:, None]
    assert (np.abs(xt.grad.cpu().numpy() * 2.0 - r["grad_inputs"]) <= G.input_grad_bound(r, c.L, c.C) + slack).all()
    assert not xt.grad.cpu().numpy()[G.out_of_range(x01)].any()
