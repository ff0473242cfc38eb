"""The arithmetic of csrc/maps.hip restated in numpy: what sdn_depth_maps and sdn_depth_quantise must produce, bit for bit.

  composite   per kept ray acc = 0.0 (f64); for s ascending acc += f64(w[s]) * f64(z[s]) (the product is exact in f64);
              (float32)acc, one rounding.  opacity: the same over w[s] alone.
  value_range the f32 bit patterns of the smallest and largest composite value that is > 0 and finite; (0x7F800000, 0) if none.
  quantise    d > 0 and finite: t = (d - lo) / (hi - lo) in float32, 0 when hi == lo, clamped to [0, 1] (NaN -> 0);
              rint(t * (2^bits - 1)), ties to even.  Everything else: 2^bits - 1."""
import numpy as np

NO_HIT = (0x7F800000, 0)


def composite(weights, sample_depth, rows, cols, crop=0):
    """weights, sample_depth f32 [rows*cols, ns] -> (depth f32 [H,W], opacity f32 [H,W])"""
    w = np.ascontiguousarray(weights, np.float32).reshape(rows, cols, -1)
    z = np.ascontiguousarray(sample_depth, np.float32).reshape(rows, cols, -1)
    if crop:
        w, z = w[crop:rows - crop, crop:cols - crop], z[crop:rows - crop, crop:cols - crop]
    w, z = w.astype(np.float64), z.astype(np.float64)
    acc = np.zeros(w.shape[:2], np.float64)
    op = np.zeros(w.shape[:2], np.float64)
    with np.errstate(all="ignore"):
        for s in range(w.shape[2]):
            acc = acc + w[:, :, s] * z[:, :, s]
            op = op + w[:, :, s]
        return acc.astype(np.float32), op.astype(np.float32)


def _hit(depth):
    with np.errstate(invalid="ignore"):
        return (depth > 0) & np.isfinite(depth)


def value_range(depth):
    """-> uint32[2]: bit patterns of (min, max) over the positive finite values"""
    d = np.asarray(depth, np.float32)
    v = d[_hit(d)]
    if v.size == 0:
        return np.array(NO_HIT, np.uint32)
    return np.array([v.min(), v.max()], np.float32).view(np.uint32)


def quantise(depth, rng_bits, bits=8):
    d = np.asarray(depth, np.float32)
    lo, hi = np.asarray(rng_bits).astype(np.uint32).view(np.float32)
    top = np.float32(2 ** bits - 1)
    with np.errstate(all="ignore"):
        if hi == lo:
            t = np.zeros_like(d)
        else:
            t = (d - lo) / (hi - lo)                    # float32 subtract, float32 IEEE divide
        assert t.dtype == np.float32
        t = np.where(t > 0, t, np.float32(0))           # NaN -> 0
        t = np.where(t < 1, t, np.float32(1))
        v = np.rint(t * top)
        assert v.dtype == np.float32
    v = np.where(_hit(d), v, top)
    return v.astype(np.uint8 if bits == 8 else np.uint16)


def synthetic(rows, cols, ns, seed):
    """The arrays of the GPU test: weights in [0,1) with whole rays zero, depths up to 300, one ray with a negative sum and one NaN
    weight (where the frame has room for them)."""
    g = np.random.default_rng(seed)
    n = rows * cols
    w = g.random((n, ns), dtype=np.float32)
    z = (g.random((n, ns), dtype=np.float32) * np.float32(300)).astype(np.float32)
    w[g.random(n) < 0.3] = 0                              # rays that hit nothing
    if n >= 4:
        w[n // 2] = g.random(ns, dtype=np.float32)
        z[n // 2] = -np.abs(z[n // 2]) - 1                # a negative sum
        w[n // 3] = g.random(ns, dtype=np.float32)
        w[n // 3, ns // 2] = np.nan                       # a NaN weight
    return w, z
