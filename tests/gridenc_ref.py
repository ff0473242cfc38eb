"""fp64 reference of the hash-grid encoder (csrc/gridenc.hip) and the inputs of its tests: tests/test_gridenc_cpu.py qualifies
both against the CPU oracle, tests/test_gridenc_gpu.py applies them to the kernels.  numpy only: no GPU, no reference tree.

The model.  What the op DEFINES in f32 is taken in f32, exactly: the level constants (oracle.level_params), the grid position
pos = fl(fl(x * scale) + off) (two roundings), its floor and fraction, the stride walk (`<=`), the hash (only for gridtype 0 and
only when the walk overflowed), `% size`, and the out-of-range test `x < 0 || x > 1`.  What the op COMPUTES from those -- corner
weights, blends, dy_dx, gradients -- is evaluated in float64.  `defect=` turns one of those definitions into a plausible wrong one;
tests/test_gridenc_cpu.py shows that each moves the result by more than the GPU test's bound, i.e. that the GPU test would see it.

No NaN inputs anywhere: the oracle's `(uint32_t)floorf(NaN)` is undefined in C, so there is nothing to compare a kernel with."""
import numpy as np

F32, F64, U64 = np.float32, np.float64, np.uint64
M32 = U64(0xFFFFFFFF)
PRIMES = (1, 2654435761, 805459861, 3674653429, 2097192037, 1434869437, 2165219737)
DEFECTS = ("contract", "oob_ge", "stride_lt", "side_swap", "hash_tiled", "prime4")
U = 2.0 ** -24           # unit roundoff of f32


def _oracle():
    from oracle import oracle as O
    O.build()
    return O


def level_offsets(D, L, per_level_scale, H, log2_T, align):
    """Row offsets of every level's table, as GridEncoder lays them out (tests/test_gridenc_cpu.py compares the two)."""
    offs, off = [0], 0
    for i in range(L):
        res = int(np.ceil(H * per_level_scale ** i))
        rows = min(2 ** log2_T, (res if align else res + 1) ** D)
        off += int(np.ceil(rows / 8) * 8)
        offs.append(off)
    return np.asarray(offs, np.int32)


def levels(L, S, H):
    """[(scale as a Python float holding the f32 value, resolution)] per level, from the oracle (libm's exp2f)."""
    O = _oracle()
    return [O.level_params(l, S, H) for l in range(L)]


def out_of_range(x, defect=None):
    x = np.asarray(x, F32)
    return ((x < 0) | ((x >= 1) if defect == "oob_ge" else (x > 1))).any(axis=1)


def place(x, scale, align, defect=None):
    """pos_grid int64 [B,D] and the fraction f32 [B,D] of in-range coordinates x f32 [B,D] on a level."""
    x = np.asarray(x, F32)
    sc, off = F32(scale), F32(0.0 if align else 0.5)
    if defect == "contract":
        pos = (x.astype(F64) * F64(sc) + F64(off)).astype(F32)         # one rounding: what an FMA gives
    else:
        pos = (x * sc).astype(F32) + off                              # two roundings
    assert pos.dtype == F32
    pg = np.floor(pos)
    return pg.astype(np.int64), (pos - pg).astype(F32)


def row_index(pgl, gridtype, align, T, res, defect=None):
    """get_grid_index / C for corner coordinates pgl int64 [B,D] in a T-row table; uint32 arithmetic as in the op."""
    D = pgl.shape[1]
    side = res if align else res + 1
    if defect == "side_swap":
        side = res + 1 if align else res
    p = pgl.astype(U64)
    stride, idx = 1, np.zeros(pgl.shape[0], U64)
    for d in range(D):
        if (stride < T) if defect == "stride_lt" else (stride <= T):
            idx = (idx + p[:, d] * U64(stride)) & M32
            stride = (stride * side) & 0xFFFFFFFF
    if (gridtype == 0 or defect == "hash_tiled") and stride > T:
        primes = list(PRIMES)
        if defect == "prime4":
            primes[4] = PRIMES[5]
        idx = np.zeros(pgl.shape[0], U64)
        for d in range(D):
            idx ^= (p[:, d] * U64(primes[d])) & M32
    return (idx % U64(T)).astype(np.int64)


def _corners(x, scale, res, T, gridtype, align, defect):
    """Yields (rows int64 [B], factors f64 [B,D]) per corner in the op's order; the weight is the product of the factors."""
    pg, frac = place(x, scale, align, defect)
    f = frac.astype(F64)
    D = x.shape[1]
    for idx in range(1 << D):
        bit = np.array([(idx >> d) & 1 for d in range(D)], np.int64)
        yield idx, row_index(pg + bit, gridtype, align, T, res, defect), np.where(bit.astype(bool), f, 1.0 - f)


def model(x, emb, offs, S, H, gridtype, align, want_dy=False, defect=None):
    """features f64 [L,B,C] (and dy_dx f64 [B, L*D*C]) of the encoder on x [B,D], emb [rows,C], offs int32 [L+1]."""
    x = np.ascontiguousarray(x, F32)
    e = np.asarray(emb, F64)
    B, D = x.shape
    C, L = e.shape[1], len(offs) - 1
    oob = out_of_range(x, defect)
    xin = np.where(oob[:, None], F32(0), x)
    out = np.zeros((L, B, C), F64)
    dy = np.zeros((B, L, D, C), F64) if want_dy else None
    for l, (scale, res) in enumerate(levels(L, S, H)):
        T = int(offs[l + 1] - offs[l])
        for idx, rows, fac in _corners(xin, scale, res, T, gridtype, align, defect):
            v = e[int(offs[l]) + rows]
            out[l] += fac.prod(axis=1)[:, None] * v
            if want_dy:
                for gd in range(D):
                    wo = np.delete(fac, gd, axis=1).prod(axis=1) * scale
                    dy[:, l, gd] += (wo if (idx >> gd) & 1 else -wo)[:, None] * v
    out[:, oob] = 0
    if want_dy:
        dy[oob] = 0
        return out, dy.reshape(B, L * D * C)
    return out


def corner_rows(x, offs, S, H, gridtype, align, level):
    """The discrete model on one level, for comparison with oracle.grid_index: pos_grid int64 [B,D], rows int64 [B, 2^D]
    (within the level's table) and the out-of-range mask.  Out-of-range rows are placed as x = 0."""
    x = np.ascontiguousarray(x, F32)
    oob = out_of_range(x)
    xin = np.where(oob[:, None], F32(0), x)
    scale, res = levels(len(offs) - 1, S, H)[level]
    T = int(offs[level + 1] - offs[level])
    pg, _ = place(xin, scale, align)
    return pg, np.stack([r for _, r, _ in _corners(xin, scale, res, T, gridtype, align, None)], axis=1), oob


def bwd_model(x, grad, offs, S, H, gridtype, align, dy_dx=None):
    """The backward pass in float64.  grad [L,B,C]; dy_dx [B, L*D*C] or None.  Returns a dict:
    grad_grid f64 [rows,C]; n int64 [rows]: how many (sample, corner) contributions an entry receives; A f64 [rows,C]: the sum of
    their magnitudes |w g|; and, for a given dy_dx, grad_inputs f64 [B,D] with A_in = sum |g dy| per element."""
    x = np.ascontiguousarray(x, F32)
    g = np.asarray(grad, F64)
    L, B, C = g.shape
    D = x.shape[1]
    keep = ~out_of_range(x)
    xin = x[keep]
    gg, A, n = np.zeros((int(offs[-1]), C), F64), np.zeros((int(offs[-1]), C), F64), np.zeros(int(offs[-1]), np.int64)
    for l, (scale, res) in enumerate(levels(L, S, H)):
        T = int(offs[l + 1] - offs[l])
        for _, rows, fac in _corners(xin, scale, res, T, gridtype, align, None):
            c = fac.prod(axis=1)[:, None] * g[l][keep]
            np.add.at(gg, int(offs[l]) + rows, c)
            np.add.at(A, int(offs[l]) + rows, np.abs(c))
            np.add.at(n, int(offs[l]) + rows, 1)
    r = dict(grad_grid=gg, n=n, A=A)
    if dy_dx is not None:
        t = g.transpose(1, 0, 2)[:, :, None, :] * np.asarray(dy_dx, F64).reshape(B, L, D, C)     # [B,L,D,C]
        r["grad_inputs"], r["A_in"] = t.sum(axis=(1, 3)), np.abs(t).sum(axis=(1, 3))
    return r


TINY = 2.0 ** -149      # one f32 operation that underflows is off by at most half of this, whatever the size of its result


def grid_grad_bound(r, D):
    """|fp32 table gradient - grad_grid| per entry, for ANY order of the additions: (n + D + 2) U A -- the recursive-summation
    bound over the entry's n contributions, each carrying the roundings of its weight -- plus the same count of underflows: the
    denormal and boundary rows give contributions far below 2^-126, where a rounding is absolute, not relative."""
    k = r["n"][:, None] + D + 2
    return k * U * r["A"] + k * TINY


def input_grad_bound(r, L, C):
    """|fp32 grad_inputs - grad_inputs| per element: a chain of L C products and sums."""
    return (L * C + 2) * U * r["A_in"] + (L * C + 2) * TINY


def fwd_bound(D, scale_max, emb_max):
    """What fp32 arithmetic in ANY summation order can differ from the fp64 model by (first order in U): per corner D roundings of
    `1 - frac`, D multiplies (the weight and w * v), and 2^D additions of terms whose weights sum to 1.  (features, dy_dx)."""
    return (2 * D + 2 ** D) * U * emb_max, (2 * D + 1 + 2 ** (D - 1)) * U * scale_max * 2 * emb_max


# --------------------------------------------------------------------------------------------------------------------- inputs

def _nudge(v, k):
    """The f32 k ulps from v (k may be negative)."""
    v = F32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, F32(2.0 if k > 0 else -2.0))
    return v


def boundary_values(scale, align, cells):
    """[(n, k, x)]: the f32 neighbours (k = -3 .. 3 ulp) of (n - off) / scale that lie in [0, 1]: pos on, just under and just over
    the boundary of cell n."""
    off = 0.0 if align else 0.5
    vals = []
    for n in cells:
        c = F32((n - off) / scale)
        for k in range(-3, 4):
            v = _nudge(c, k)
            if 0 <= v <= 1:
                vals.append((n, k, v))
    return vals


def boundary_cells(scale):
    """Cells of a level at whose boundary rows are placed: the first, one in the middle, the last, and every power of two from 4 up
    (where pos changes binade, so that x * scale and x * scale + off round on different grids: the only place two roundings and
    one can differ by a whole ulp of pos)."""
    top = int(np.ceil(scale))
    return sorted({1, 2, top // 2 + 1, top} | {2 ** k for k in range(2, 12) if 2 ** k <= top})


class Case:
    """One configuration with its inputs.  `classes`: edge class -> row indices of x."""

    def __init__(self, name, D, C, L, per_level_scale, H, log2_T, gridtype, align, B, seed):
        self.name, self.D, self.C, self.L, self.H, self.gridtype, self.align, self.B = name, D, C, L, H, gridtype, align, B
        self.S = float(F32(np.log2(per_level_scale)))
        self.offs = level_offsets(D, L, per_level_scale, H, log2_T, align)
        rng = np.random.default_rng(seed)
        self.emb = (rng.random((int(self.offs[-1]), C), dtype=F32) - F32(0.5))      # differs per channel
        self.x, self.classes = self._inputs(rng)
        self.grad = rng.standard_normal((L, B, C)).astype(F32)

    def _inputs(self, rng):
        D, B = self.D, self.B
        rows, cls = [], []

        def add(name, row):
            rows.append(np.asarray(row, F32))
            cls.append(name)

        rnd = lambda: rng.random(D, dtype=F32)
        one = lambda d, v: np.concatenate([rnd()[:d], [F32(v)], rnd()[d + 1:]]).astype(F32)
        below1, above1, tiny = np.nextafter(F32(1), F32(0)), np.nextafter(F32(1), F32(2)), np.nextafter(F32(0), F32(1))
        for name, v in (("zero", 0.0), ("negzero", -0.0), ("one", 1.0), ("below_one", below1), ("denormal", tiny)):
            add(name, np.full(D, v, F32))                       # in range
            add(name, one(len(rows) % D, v))
        for name, v in (("above_one", above1), ("neg_denormal", -tiny)):
            add("oob:" + name, one(len(rows) % D, v))           # out of range
            add("oob:" + name, np.full(D, v, F32))
        for d in range(D):                                       # one out-of-range coordinate in each dimension in turn
            add("oob:dim%d" % d, one(d, -0.25))
            add("oob:dim%d" % d, one(d, 1.5))
        seen = set()
        for l, (scale, _) in enumerate(levels(self.L, self.S, self.H)):
            if scale in seen:                                    # MANY_LEVELS: forty equal levels
                continue
            seen.add(scale)
            vals = boundary_values(scale, self.align, boundary_cells(scale))
            for i, (n, k, v) in enumerate(vals):
                add("boundary:L%d:%s" % (l, "on" if k == 0 else "under" if k < 0 else "over"), one(i % D, v))
            for _ in range(8):                                   # every coordinate on or next to a boundary
                add("boundary:L%d:all" % l, [vals[j][2] for j in rng.integers(0, len(vals), D)])
        assert len(rows) <= B * 2 // 3, (len(rows), B)
        x = rng.random((B, D), dtype=F32)
        step = next(s for s in (5, 7, 3, 11) if np.gcd(s, B) == 1)      # spread: every edge row has random rows in its wave and its
        at = (np.arange(len(rows)) * step + 1) % B                       # 4-lane quad, the out-of-range ones in-range neighbours
        x[at] = np.stack(rows)
        classes = {}
        for name, i in zip(cls, at):
            classes.setdefault(name, []).append(int(i))
        return np.ascontiguousarray(x), classes

    def args(self):
        """(offs, S, H, gridtype, align) as model / bwd_model / the oracle take them after x, emb."""
        return self.offs, self.S, self.H, self.gridtype, self.align


FORMS = ((0, False), (1, False), (0, True), (1, True))       # (gridtype, align_corners)
DC = tuple((D, C) for D in (2, 3, 4, 5) for C in (1, 2, 4, 8))
_CACHE = {}


def case(D, C, gridtype, align, B=777):
    """Two levels, H = 4, per-level scale 512, 2^12 rows: level 0 (scale 3) is dense for every D, level 1 (scale 2047) overflows
    the table and is hashed / wrapped; one ulp of pos is 1.2e-4 there."""
    key = (D, C, gridtype, align, B)
    if key not in _CACHE:
        name = "D%d C%d %s%s B%d" % (D, C, "tiled" if gridtype else "hash", " align" if align else "", B)
        _CACHE[key] = Case(name, D, C, 2, 512, 4, 12, gridtype, align, B, 7000 + 100 * D + 10 * C + 2 * gridtype + int(align))
    return _CACHE[key]


CASES = tuple((D, C, gt, al) for (D, C) in DC for (gt, al) in FORMS)


def stride_eq(gridtype):
    """One level, D = 5, H = 8, align_corners: strides 1, 8, 64, 512, 4096 -- the last EQUALS the table size, the only place the
    stride walk's `<=` differs from `<`."""
    key = ("stride_eq", gridtype)
    if key not in _CACHE:
        c = Case("STRIDE_EQ " + ("tiled" if gridtype else "hash"), 5, 4, 1, 1, 8, 12, gridtype, True, 777, 7900 + gridtype)
        assert c.offs[-1] == 4096 and levels(1, c.S, 8)[0] == (7.0, 8)
        _CACHE[key] = c
    return _CACHE[key]


def many_levels():
    """Forty levels (more than the 32 the host hands the kernels as a table: the in-kernel level formula runs) of scale exactly 8
    (S = 0: exp2f(0) == 1 on the host and on the device)."""
    if "many" not in _CACHE:
        c = Case("MANY_LEVELS", 2, 2, 40, 1, 9, 12, 0, False, 777, 7950)
        assert all(lv == (8.0, 9) for lv in levels(40, c.S, 9))
        _CACHE["many"] = c
    return _CACHE["many"]


EXTRA = (("stride_eq", 0), ("stride_eq", 1), ("many_levels",))


def extra(key):
    return stride_eq(key[1]) if key[0] == "stride_eq" else many_levels()


# ------------------------------------------------------------------------------------------------------- the exact scatter

class ExactScatter:
    pass


def exact_scatter_case(D, C, align, dtype, identical=False):
    """A backward case whose every contribution and every partial sum is an integer below the format's exact-integer limit, so
    that the table gradient is THE SAME for every order of the atomics: S = 0, H = 9 (scale 8), three levels of 2^8 rows, hashed;
    x = m / 16 puts every fraction on 0 or 0.5, i.e. every weight on 0 or 2^-k (k <= D); grad = small integers x 2^D.
    identical = False: 300 random rows (m = 17 is out of range) into 256-row tables: heavy collisions, and for C = 1 neighbouring
    rows share a 32-bit word.  identical = True: 257 copies of one row: every lane of a wave hits the same entries.
    dtype "f16" / "f32".  Asserts sum |contribution| <= 2048 (f16) / 2^24 (f32) per entry: exactness is shown, not assumed."""
    key = ("exact", D, C, align, dtype, identical)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(8000 + 100 * D + 10 * C + int(align) + (5 if identical else 0))
    e = ExactScatter()
    e.D, e.C, e.L, e.H, e.S, e.gridtype, e.align, e.dtype = D, C, 3, 9, 0.0, 0, align, dtype
    e.offs = level_offsets(D, 3, 1, 9, 8, align)
    if identical:
        e.B = 257
        for _ in range(64):       # every fraction 0.5 (all 2^D corners carry 2^-D); two of the corners in one 32-bit word of a
            m1 = 2 * rng.integers(0, 8, (1, D)) + int(align)          # C = 1 half table (rows 2k and 2k + 1)
            n1 = bwd_model(m1.astype(F32) / F32(16), np.ones((3, 1, C)), e.offs, e.S, e.H, 0, align)["n"]
            if ((n1[0::2] > 0) & (n1[1::2] > 0)).any():
                break
        else:
            raise AssertionError("no row whose corners share a word")
        m = np.tile(m1, (e.B, 1))
        ints = rng.choice([-1, 1, 1], size=(3, e.B, C))
    else:
        e.B = 300
        m = rng.integers(0, 18, (e.B, D))
        ints = rng.integers(-1, 2, size=(3, e.B, C))
    e.x = np.ascontiguousarray(m.astype(F32) / F32(16))
    e.grad = (ints * 2 ** D).astype(F32)
    for scale, res in levels(3, e.S, 9):
        assert (scale, res) == (8.0, 9)
        _, frac = place(np.where(out_of_range(e.x)[:, None], F32(0), e.x), scale, align)
        assert np.isin(frac, (0.0, 0.5)).all()
    r = bwd_model(e.x, e.grad, e.offs, e.S, e.H, 0, align)
    e.expected, e.n, e.A = r["grad_grid"], r["n"], r["A"]
    assert (e.expected == np.rint(e.expected)).all() and (e.A == np.rint(e.A)).all()
    e.limit = 2048 if dtype == "f16" else 2 ** 24
    assert e.A.max() <= e.limit, (D, C, align, dtype, identical, e.A.max())
    assert (np.abs(e.grad) <= e.limit).all()
    _CACHE[key] = e
    return e
