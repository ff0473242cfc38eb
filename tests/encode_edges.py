"""Edge-case rays for the encode stage (csrc/field_enc.h): sample placement, world / grid coordinates, the ground and sky
flags, the label select chain.  Shared by tests/test_encode_edges_cpu.py (which shows on the oracle's own output that the
set contains what it claims) and tests/test_encode_edges_gpu.py (which runs the kernels on it).

The rays are not ray-marched: they are built class by class (the tag of every ray names its class), for any box count M and any
sample count, on scene256's voxel extent and one camera origin whose coordinates are powers of two -- with axis-aligned
directions a world coordinate is then `origin +- depth`, one rounding, and can be steered onto a given float."""
import types

import numpy as np
import torch

SAMPLE_DEPTH = 3.0
DISTS_SCALE = 0.25
VOXEL_DIMS = (195, 256, 256)            # synth.make_scene(256, 3407).voxel_t.shape (the GPU tests assert it)
CAM_ORI = (2.0, 128.0, 64.0)
F32_MAX_ID = 679                        # the largest id of the 680-entry label table

# (M, num_samples) of the GPU tests: every M with 6 and 24 samples, M = 2 and 8 with every sample count
MS = (1, 2, 3, 6, 7, 8)
SAMPLES = (1, 3, 4, 6, 24, 79)
CASES = tuple((M, ns) for M in MS for ns in (6, 24)) + tuple((M, ns) for M in (2, 8) for ns in (1, 3, 4, 79))

f32 = np.float32
NAN = f32("nan")
INF = f32("inf")


def lin_points(ns, stochastic=False):
    """The stratified positions of ns samples (ns + 1 points), as the reference makes them: mc_utils.py:120 / :125."""
    return torch.linspace(0, 1, ns + 3)[1:-1].numpy() if not stochastic else torch.linspace(0, 1, ns + 2)[:-1].numpy()


def det_midpoints(ns, total):
    """Midpoints of the deterministic samples of a ray whose clamped total depth is `total`, in the reference's fp32 operations."""
    s = lin_points(ns) * f32(total)
    return ((s[1:] + s[:-1]) / f32(2)).astype(f32)


def normalise(wc, delim):
    """World coordinate -> grid coordinate in [0, 1]: scenedreamer.py:300 then grid.py:144, one fp32 rounding per operation."""
    n = (np.asarray(wc, f32) / f32(delim)).astype(f32)
    n = (n * f32(2)).astype(f32)
    n = (n - f32(1)).astype(f32)
    n = (n + f32(1)).astype(f32)
    return (n / f32(2)).astype(f32)


BELOW_ZERO = f32(-2.0 ** -24)           # the first values outside [0, 1] that op sequence can yield: (-1 - 2^-23 + 1) / 2 and
ABOVE_ONE = np.nextafter(f32(1), f32(2))  # (1 + 2^-22 + 1) / 2


def _ulp(x):
    return np.nextafter(f32(abs(x)), INF) - f32(abs(x))


class _Set:
    def __init__(self, M, rng, ids):
        self.M, self.rng, self.ids = M, rng, ids
        self.t, self.t2, self.id, self.d, self.tag = [], [], [], [], []

    def unit(self, up=True):
        d = self.rng.normal(size=3)
        d /= np.linalg.norm(d)
        if up:
            d[0] = abs(d[0])            # world x grows along the ray: no sample at or below x = 1 (the camera is at x = 2)
        return d.astype(f32)

    def some_ids(self, k):
        return [int(v) for v in self.rng.choice(self.ids, size=k)]

    def add(self, tag, t, t2, ids=None, d=None):
        """Boxes t / t2 (at most M; the rest NaN with id 0), ids (default: random non-zero ones), direction (default: random)."""
        k = len(t)
        assert k == len(t2) <= self.M
        ids = self.some_ids(k) if ids is None else list(ids)
        pad = self.M - k
        self.t.append(np.asarray(list(t) + [NAN] * pad, f32))
        self.t2.append(np.asarray(list(t2) + [NAN] * pad, f32))
        self.id.append(np.asarray(ids + [0] * pad, np.int32))
        self.d.append(self.unit() if d is None else np.asarray(d, f32))
        self.tag.append(tag)

    def chain(self, t0, lengths, gaps):
        """Boxes of the given lengths, the first at t0, separated by the given gaps."""
        t, t2, at = [], [], f32(t0)
        for i, ln in enumerate(lengths):
            if i:
                at = f32(at + f32(gaps[i - 1]))
            t.append(at)
            at = f32(at + f32(ln))
            t2.append(at)
        return t, t2


def _box_for_depth(ns, target, j=None):
    """A single box [t0, t0 + L] whose deterministic sample j lands on depth `target` EXACTLY: fl(t0 + mid_j) == target with
    fl((t0 + L) - t0) == L (so the total depth, and with it mid_j, is what was planned).  Searched, then verified."""
    target = f32(target)
    for L in (2.0, 1.0, 0.5, 3.0, 1.5, 2.5, 0.25, 0.75, 0.125):
        mids = det_midpoints(ns, min(L, SAMPLE_DEPTH))
        for jj in ([j] if j is not None else list(range(ns - 1, -1, -1))):
            t0 = f32(np.float64(target) - np.float64(mids[jj]))
            for _ in range(4):
                for cand in (t0, np.nextafter(t0, INF), np.nextafter(t0, -INF)):
                    t2 = f32(cand + f32(L))
                    if cand >= 0 and f32(cand + mids[jj]) == target and f32(t2 - cand) == f32(L):
                        return cand, t2, jj
                t0 = np.nextafter(t0, INF)
    raise AssertionError(f"no box puts a sample of {ns} at depth {target!r}")


def _straddle(ori, delim, low):
    """Two adjacent float depths along an axis (direction -1 for the low face, +1 for the high face) whose world coordinate
    origin -+ depth is the last one inside the grid and the first one outside it (normalised == BELOW_ZERO / ABOVE_ONE)."""
    base = f32(ori) if low else f32(delim - ori)
    k = np.arange(0, 4096, dtype=np.float64)
    depth = (np.float64(base) + k * np.float64(_ulp(base))).astype(f32)
    wc = (f32(ori) - depth).astype(f32) if low else (f32(ori) + depth).astype(f32)
    x = normalise(wc, delim)
    out = x < 0 if low else x > 1
    first = int(np.argmax(out))
    assert out[first] and first > 0 and not out[first - 1] and x[first] == (BELOW_ZERO if low else ABOVE_ONE)
    return depth[first - 1], depth[first]


def rays(M, num_samples, seed=0, lut=None):
    """Edge rays for M boxes per ray and `num_samples` samples: a namespace with voxel_id i32 [n,M], depth2 f32 [2,n,M],
    raydirs f32 [n,3], cam_ori f32 [3], tag (object [n]: the class of every ray), voxel_dims, M, ns.
    lut: the 680-entry block id -> reduced label table (default: the project's), for ids that span every label."""
    ns = int(num_samples)
    assert 1 <= M <= 8 and 1 <= ns <= 79
    if lut is None:
        from scenedreamer_amd.renderer import load_label_lut
        lut = load_label_lut()["lut"]
    lut = np.asarray(lut)
    rng = np.random.default_rng(7000 + 100 * M + ns + 10007 * seed)
    per_label = [int(np.nonzero(lut == r)[0][np.nonzero(lut == r)[0] > 0][0]) for r in sorted(set(lut.tolist()))
                 if (np.nonzero(lut == r)[0] > 0).any()]
    S = _Set(M, rng, np.asarray(per_label + [F32_MAX_ID]))
    U = lambda a, b, k=None: rng.uniform(a, b, size=k)
    X, Y, Z = (1, 0, 0), (0, 1, 0), (0, 0, 1)
    neg = lambda a: tuple(-v for v in a)

    # 1. 0 .. M valid boxes, the trailing ones NaN with id 0 (none valid: the ray hits nothing, `sky_only`)
    for k in range(M + 1):
        for _ in range(3 if k else 20):
            S.add(f"valid{k}", *S.chain(U(3, 20), U(0.3, 1.5, k), U(0.1, 1.0, max(k - 1, 0))))
    # 2. short boxes with gaps: all M boxes inside sample_depth, evenly and with one dominant box, so that every index is taken
    for _ in range(6):
        S.add("short", *S.chain(U(3, 20), U(0.6, 1.0, M) * (2.9 / M), U(0.05, 2.0, M - 1)))
    for jdom in range(M):
        for _ in range(6):
            ln = U(0.5, 1.0, M) * (0.6 / M)
            ln[jdom] = U(1.5, 2.2)
            S.add(f"short_dom{jdom}", *S.chain(U(3, 20), ln, U(0.05, 2.0, M - 1)))
    # 3. zero-length boxes: the first, a middle one, the last
    for pos in sorted({0, M // 2, M - 1}):
        for _ in range(2):
            ln = U(0.6, 1.0, M) * (2.9 / M)
            ln[pos] = 0.0
            S.add(f"zero_len{pos}", *S.chain(U(3, 20), ln, U(0.05, 2.0, M - 1)))
    # 4. total depth below, exactly at and far above sample_depth (dyadic lengths from a dyadic start: the sums are exact)
    two = M >= 2
    S.add("total_below", *S.chain(4.0, [0.5, 0.75] if two else [1.25], [1.0]))
    S.add("total_below", *S.chain(U(3, 20), U(0.2, 0.9, min(M, 3)), U(0.1, 1.0, min(M, 3) - 1)))
    S.add("total_equal", *S.chain(4.0, [1.0, 2.0] if two else [3.0], [0.5]))
    S.add("total_equal", *S.chain(8.0, [0.5, 1.25, 1.25][:M] if M >= 3 else ([1.75, 1.25] if two else [3.0]), [0.25, 0.5]))
    S.add("total_above", *S.chain(4.0, [4.0, 1e4] if two else [1e4], [1.0]))
    S.add("total_above", *S.chain(U(3, 20), U(2.0, 5.0, min(M, 3)), U(0.1, 1.0, min(M, 3) - 1)))
    # ... and, below it, with box lengths of different binades (boxes at 0, 1, 2: the lengths keep their low bits, where the
    # lengths of boxes tens of units away are multiples of 2^-20 and every float32 sum of them is exact): the double-accumulated
    # prefix sum and a float32 one round differently here
    if M >= 3:
        kept = 0
        for i in range(4000):
            a = [f32(U(0.05, 0.5)), f32(U(0.1, 0.9)), f32(U(0.1, 0.9))]
            ln = [a[0], f32(f32(f32(1) + a[1]) - f32(1)), f32(f32(f32(2) + a[2]) - f32(2))]      # as t2 - t will give them
            differs = f32(f32(ln[0] + ln[1]) + ln[2]) != f32(np.float64(ln[0]) + np.float64(ln[1]) + np.float64(ln[2]))
            if i < 4 or (differs and kept < 4):
                S.add("fine_lengths", [0.0, 1.0, 2.0], [a[0], f32(f32(1) + a[1]), f32(f32(2) + a[2])])
                kept += bool(differs and i >= 4)
        assert kept == 4
    # 5. ties: a midpoint that equals a prefix sum exactly (the reference's `>` is strict: the sample stays in the lower box)
    if two:
        # the total clamped to sample_depth: mid_j is fixed, box 0 = [0, mid_j] ends exactly there
        m3 = det_midpoints(ns, SAMPLE_DEPTH)
        for j in sorted({0, ns // 2, ns - 1}):
            S.add("tie_clamped", [0.0, f32(m3[j] + f32(1.0))], [m3[j], f32(m3[j] + f32(5.0))])
        # the total unclamped (a power of two, so that total * lin is exact): box 0 = [0, mid_j], box 1 makes up the total
        found = 0
        for T in (1.0, 2.0, 0.5):
            mT = det_midpoints(ns, T)
            for j in range(ns):
                l1 = f32(f32(T) - mT[j])
                t1 = f32(2 * T)
                if f32(np.float64(mT[j]) + np.float64(l1)) == f32(T) and f32(f32(t1 + l1) - t1) == l1 and found < 3:
                    S.add("tie_unclamped", [0.0, t1], [mT[j], f32(t1 + l1)])
                    found += 1
        # prefix sum of TWO boxes (M >= 3): 0.25 + (mid_j - 0.25), third box long
        if M >= 3:
            for j in range(ns):
                l1 = f32(m3[j] - f32(0.25))
                if l1 > 0 and f32(np.float64(f32(0.25)) + np.float64(l1)) == m3[j] and f32(f32(1.0 + l1) - f32(1.0)) == l1:
                    S.add("tie_second", [0.0, 1.0, 8.0], [0.25, f32(1.0 + l1), 16.0])
                    break
    # 6. the camera inside a box, infinite and huge depths, heads that overflow or are NaN (the depth is then replaced by 0)
    S.add("t0_zero", [0.0], [1.5])
    S.add("t2_inf", [2.0] + ([9.0] if two else []), [INF] + ([9.5] if two else []))
    S.add("huge", [1e30], [f32(1e30) + 8 * _ulp(1e30)])
    S.add("head_inf", [INF], [INF])
    if two:
        S.add("head_overflow", [-3e38, 3e38], [-3e38, f32(3e38) + _ulp(3e38)])
        S.add("head_nan", [INF, 2.0], [INF, 3.0])
    # 7. a NaN box between two valid ones (its id zero, and non-zero)
    if M >= 3:
        S.add("nan_middle", [4.0, NAN, 7.0], [5.0, NAN, 11.0], ids=S.some_ids(1) + [0] + S.some_ids(1))
        S.add("nan_middle", [4.0, NAN, 7.0], [4.5, NAN, 7.5], ids=S.some_ids(3))
    # 8. the last box: id != 0 against id == 0 (valid boxes throughout), and ids of every reduced label + the table's largest
    for _ in range(3):
        S.add("last_id_set", *S.chain(U(3, 20), U(0.6, 1.0, M) * (2.9 / M), U(0.05, 1.0, M - 1)))
        S.add("last_id_zero", *S.chain(U(3, 20), U(0.6, 1.0, M) * (2.9 / M), U(0.05, 1.0, M - 1)), ids=S.some_ids(M - 1) + [0])
    pool = per_label + [F32_MAX_ID]
    for i in range(0, len(pool), max(M, 1)):
        ids = pool[i:i + M]
        S.add("labels", *S.chain(U(3, 20), U(0.6, 1.0, len(ids)) * (2.9 / len(ids)), U(0.05, 1.0, len(ids) - 1)), ids=ids)
    # 9. axis-aligned rays onto exact coordinates (one box; for M >= 2 the last id is 0, so `nosky` is the ground test alone)
    t0, t2, _ = _box_for_depth(ns, 1.0, ns - 1)                         # world x == 1.0 at the LAST sample, above it before
    S.add("wx_one", [t0], [t2], d=neg(X))
    t0, t2, _ = _box_for_depth(ns, f32(1) - f32(2.0 ** -23), ns - 1)     # ... and the next float above 1.0 there
    assert f32(f32(CAM_ORI[0]) - (f32(1) - f32(2.0 ** -23))) == np.nextafter(f32(1), f32(2))
    S.add("wx_above_one", [t0], [t2], d=neg(X))
    for a, axis in enumerate((X, Y, Z)):
        o, dl = CAM_ORI[a], VOXEL_DIMS[a]
        t0, t2, _ = _box_for_depth(ns, o)
        S.add(f"norm_zero{a}", [t0], [t2], d=neg(axis))                 # world == 0: normalised == 0.0
        t0, t2, _ = _box_for_depth(ns, dl - o)
        S.add(f"norm_one{a}", [t0], [t2], d=axis)                       # world == delim: normalised == 1.0
        for low in (True, False):
            for which, depth in zip(("in", "out"), _straddle(o, dl, low)):
                t0, t2, _ = _box_for_depth(ns, depth)
                S.add(f"norm_{'low' if low else 'high'}_{which}{a}", [t0], [t2], d=neg(axis) if low else axis)
    # 10. ordinary random rays (a fifth of them descend below x = 1)
    n_rand = 64
    for i in range(n_rand):
        k = int(rng.integers(1, M + 1))
        d = S.unit(up=i % 5 != 0)
        S.add("random", *S.chain(U(1, 25), U(0.05, 2.0, k), U(0.05, 1.5, max(k - 1, 0))), d=d)
    while len(S.tag) % 8 != 5:          # neither a whole number of 8-ray tiles nor of 32-ray groups
        S.add("random", *S.chain(U(1, 25), U(0.05, 2.0, 1), []))

    return types.SimpleNamespace(
        voxel_id=np.stack(S.id), depth2=np.stack([np.stack(S.t), np.stack(S.t2)]), raydirs=np.stack(S.d),
        cam_ori=np.asarray(CAM_ORI, f32), tag=np.asarray(S.tag, object), voxel_dims=VOXEL_DIMS, M=M, ns=ns, n=len(S.tag))


def stratified_u(n, ns, seed=0):
    """The torch.rand draw of the stochastic branch for n rays: f32 [n, ns + 1] in [0, 1)."""
    return np.random.default_rng(9000 + seed).random((n, ns + 1), dtype=f32)


# --------------------------------------------------------------------------- the oracle on a ray set

def oracle_shapes(E):
    """The ray set in forward_perpix's shapes: voxel_id [1,1,n,M,1], depth2 [1,2,1,n,M,1], raydirs [1,1,n,1,3], cam_ori [1,3]."""
    n, M = E.n, E.M
    return (E.voxel_id.reshape(1, 1, n, M, 1), E.depth2.reshape(1, 2, 1, n, M, 1), E.raydirs.reshape(1, 1, n, 1, 3), E.cam_ori[None])


def oracle_placement(E, rand=None, fn=None):
    """FR.sample_depth_batched (or `fn`, a mutant of it) on the set: depth, dist f32 [n, ns] and idx i64 [n, ns], raw."""
    from oracle import field_ref as FR
    d2 = torch.from_numpy(oracle_shapes(E)[1]).clone()
    r = None if rand is None else torch.as_tensor(rand).reshape(1, 1, E.n, E.ns + 1, 1)
    depth, dist, idx = (fn or FR.sample_depth_batched)(d2, E.ns + 1, SAMPLE_DEPTH, r)
    return depth.reshape(E.n, E.ns).numpy(), dist.reshape(E.n, E.ns).numpy(), idx.reshape(E.n, E.ns).numpy()


def placement_internals(E):
    """(mid [n, ns], accu [n, M]) of the deterministic placement: the first lines of mc_utils.sample_depth_batched, for the
    tie condition (the caller checks them against the oracle's idx)."""
    d2 = torch.from_numpy(E.depth2)
    dists = d2[1] - d2[0]
    dists[torch.isnan(dists)] = 0
    accu = torch.cumsum(dists, dim=-1)
    total = torch.clamp(accu[:, -1:], None, SAMPLE_DEPTH)
    s = torch.from_numpy(lin_points(E.ns))[None, :] * total
    return ((s[:, 1:] + s[:, :-1]) / 2).numpy(), accu.numpy()


def decisions(world, voxel_dims, global_enc=None):
    """What the encode stage decides per sample from its world coordinate [.., 3]: the grid coordinates x [.., 3] (`normalise`),
    out-of-range (strictly outside [0, 1] in any of the dimensions -- global_enc's two included: gridencoder.cu's test) and
    the ground test (scenedreamer.py:380)."""
    world = np.asarray(world, f32)
    x = np.stack([normalise(world[..., a], voxel_dims[a]) for a in range(3)], axis=-1)
    oob = ((x < 0) | (x > 1)).any(axis=-1)
    if global_enc is not None:
        g = ((np.asarray(global_enc, f32).reshape(2) + f32(1)) / f32(2)).astype(f32)
        oob = oob | bool(((g < 0) | (g > 1)).any())
    gnd = world[..., 0] <= 1.0
    return x, oob, gnd


def oracle_field(weights, lut, E, z, global_enc, dtype=torch.float32, rand=None, fn=None, **kw):
    """FR.forward_perpix (or `fn`, a mutant) on the set with return_aux.  rand: the stochastic draw [n, ns + 1], handed to the
    oracle's sample_depth_batched the way tests/test_fused_gpu.py does."""
    from oracle import field_ref as FR
    orig = FR.sample_depth_batched
    if rand is not None:
        r = torch.as_tensor(rand).reshape(1, 1, E.n, E.ns + 1, 1)
        FR.sample_depth_batched = lambda d2, nsamples, sd: orig(d2, nsamples, sd, rand=r)
    try:
        return (fn or FR.forward_perpix)(weights, lut, E.voxel_dims, *oracle_shapes(E), z, global_enc, E.ns,
                                         sample_depth=SAMPLE_DEPTH, dists_scale=DISTS_SCALE, dtype=dtype, return_aux=True, **kw)
    finally:
        FR.sample_depth_batched = orig
