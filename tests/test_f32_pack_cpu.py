"""Qualifies tests/f32_pack_layout.py, the numpy restatement of the three packed fp32 streams (layout: csrc/mlp_f32.h), without a GPU:
read back lane by lane the way the header says the MFMA reads it, and multiplied with the B operand each kernel feeds at that
k-step, a stream gives W @ x; it holds every weight exactly once and zeros elsewhere.  The data are random integers in [-8, 8] as
f64: every product and every partial sum is an integer far below 2^53, so both sides are exact and compared with ==."""
import numpy as np
import pytest

import f32_pack_layout as PL

COLS = 5


def _ints(rng, *shape):
    return rng.integers(-8, 9, size=shape).astype(np.float64)


def _mlp(rng, k1, n_hidden):
    return _ints(rng, 256, k1), [_ints(rng, 256, 256) for _ in range(n_hidden)], _ints(rng, 64, 256)


def test_field_stream_read_as_the_kernel_reads_it_is_the_layers_product():
    rng = np.random.default_rng(1)
    w1, wh, wc = _mlp(rng, 128, 5)
    s = PL.field_stream(w1, wh, wc)
    assert s.shape == (PL.FIELD_CHUNKS * PL.CHUNK_FLOATS,)
    x1, xs, xo = _ints(rng, 128, COLS), [_ints(rng, 256, COLS) for _ in range(5)], _ints(rng, 256, COLS)
    # fc_1's B operand: chunk c, k-step kk, lane half h = feature 16 s + 8 h + ch of level pair s = 2 c + kk / 8, channel ch = kk % 8
    B1 = [np.stack([np.stack([x1[16 * (2 * c + kk // 8) + 8 * h + kk % 8] for h in range(2)]) for kk in range(16)]) for c in range(4)]
    got = PL.mlp_layers_product(s, 4, B1, 5, xs, xo)
    want = [w1 @ x1] + [W @ x for W, x in zip(wh, xs)] + [wc @ xo]
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(g, w)


def test_sky_stream_read_as_the_kernel_reads_it_is_the_layers_product():
    rng = np.random.default_rng(2)
    w1, wh, wc = _mlp(rng, 33, 4)
    s = PL.sky_stream(w1, wh, wc)
    assert s.shape == (PL.SKY_CHUNKS * PL.CHUNK_FLOATS,)
    x1, xs, xo = _ints(rng, 33, COLS), [_ints(rng, 256, COLS) for _ in range(4)], _ints(rng, 256, COLS)
    # fc1's B operand: k-step t of chunk c, lane half h = encoded element 2 (16 c + t) + h; zero from element 33 on.  The padding
    # is fed as ones here, so that a weight in a padding place would show.
    pad = np.concatenate([x1, np.ones((31, COLS))])
    B1 = [np.stack([np.stack([pad[2 * (16 * c + t) + h] for h in range(2)]) for t in range(16)]) for c in range(2)]
    got = PL.mlp_layers_product(s, 2, B1, 4, xs, xo)
    want = [w1 @ x1] + [W @ x for W, x in zip(wh, xs)] + [wc @ xo]
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(g, w)


@pytest.mark.parametrize("taps,cin", PL.CONV_SHAPES)
def test_conv_stream_read_as_the_kernel_reads_it_is_the_convolution(taps, cin):
    rng = np.random.default_rng(3)
    kh = 3 if taps == 9 else 1
    w = _ints(rng, 256, cin, kh, kh)
    s = PL.conv_stream(w)
    nb = cin // 32
    assert s.shape == (taps * nb * PL.CHUNK_FLOATS,) == (256 * cin * taps,)
    x = _ints(rng, taps, cin, COLS)          # per tap: the 32 pixels' neighbour at that tap, here COLS columns
    # the B operand of chunk (tap, blk): k-step kk, lane half h = input channel 32 blk + 16 h + kk of the tap's pixel
    got = sum(PL.mfma(PL.read_chunk8(s, tap * nb + blk), np.stack([np.stack([x[tap, 32 * blk + 16 * h + kk] for h in range(2)]) for kk in range(16)]))
              for tap in range(taps) for blk in range(nb))
    want = sum(w[:, :, tap // kh, tap % kh] @ x[tap] for tap in range(taps))
    assert np.array_equal(got, want)


def test_every_weight_once_and_zeros_elsewhere():
    w1, *wh, wc = PL.position_weights([(256, 128)] + [(256, 256)] * 5 + [(64, 256)])
    s = PL.field_stream(w1, wh, wc)
    assert s.dtype == np.float32 and np.array_equal(np.sort(s), np.sort(np.concatenate([t.reshape(-1) for t in (w1, *wh, wc)])))
    w1, *wh, wc = PL.position_weights([(256, 33)] + [(256, 256)] * 4 + [(64, 256)])
    s = PL.sky_stream(w1, wh, wc)
    ws = np.concatenate([t.reshape(-1) for t in (w1, *wh, wc)])
    assert np.count_nonzero(s == 0) == 256 * 31 and np.array_equal(np.sort(s[s != 0]), np.sort(ws))      # fc1's padding to K = 64
    assert not s[:2 * PL.CHUNK_FLOATS].reshape(2, 16, -1)[1, 1:].any()          # ... all of chunk 1 behind its first k-step
    for taps, cin in PL.CONV_SHAPES:
        kh = 3 if taps == 9 else 1
        w, = PL.position_weights([(256, cin, kh, kh)])
        s = PL.conv_stream(w)
        assert float(w.max()) == 256 * cin * taps < 2 ** 24 and np.array_equal(np.sort(s), w.reshape(-1))
