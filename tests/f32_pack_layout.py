"""The three packed fp32 weight streams of the exact rung in numpy, written from the layout comment of csrc/mlp_f32.h (not from the
pack kernels): field_stream / sky_stream / conv_stream place every weight, read_chunk8 / read_chunk2 read a chunk back the way a
lane of the MFMA does.  tests/test_f32_pack_cpu.py qualifies the one against the other and against W @ x;
tests/test_f32_pack_gpu.py holds the pack kernels to the streams."""
import numpy as np

CHUNK_FLOATS = 8192          # 32 KiB
FIELD_CHUNKS, SKY_CHUNKS = 4 + 5 * 8 + 2, 2 + 4 * 8 + 2
CONV_SHAPES = ((9, 256), (1, 256), (1, 64))          # (taps, cin)


def kmap(r, h):
    """Channel (inside its block of 32) that accumulator register r of lane half h holds = k of k-step r of that input block."""
    return 8 * (r // 4) + 4 * h + r % 4


# ------------------------------------------------------------------------------------------------- writers: weight -> place
def chunk8(W, k_of):
    """16 k-steps x [blocks 0-3 | blocks 4-7][lane][4 blocks] of W [256, K]; k_of(kk, h) = the column that lane half h multiplies
    in k-step kk, or None for a zero (padding)."""
    out = np.zeros((16, 2, 64, 4), W.dtype)
    for kk in range(16):
        for h in range(2):
            k = k_of(kk, h)
            if k is not None:          # lane (h, j) of block ib = 4 half + e holds W[32 ib + j][k]
                out[kk, :, 32 * h:32 * h + 32, :] = W[:, k].reshape(2, 4, 32).transpose(0, 2, 1)
    return out.reshape(-1)


def chunk2(W, k_of):
    """64 k-steps x [lane][2 blocks] of W [64, K]."""
    out = np.zeros((64, 64, 2), W.dtype)
    for kk in range(64):
        for h in range(2):
            out[kk, 32 * h:32 * h + 32, :] = W[:, k_of(kk, h)].reshape(2, 32).T
    return out.reshape(-1)


def _hidden_and_out(wh, wc):
    chunks = [chunk8(W, lambda kk, h, b=b: 32 * b + kmap(kk, h)) for W in wh for b in range(8)]
    return chunks + [chunk2(wc, lambda kk, h, C=C: 32 * (4 * C + kk // 16) + kmap(kk % 16, h)) for C in range(2)]


def field_stream(w1, wh, wc):
    """w1 [256,128], wh 5 x [256,256], wc [64,256] -> 46 chunks: fc_1 (4) | fc_2 .. fc_6 | fc_out_c."""
    assert w1.shape == (256, 128) and len(wh) == 5
    first = [chunk8(w1, lambda kk, h, c=c: 16 * (2 * c + kk // 8) + 8 * h + kk % 8) for c in range(4)]
    return np.concatenate(first + _hidden_and_out(wh, wc))


def sky_stream(w1, wh, wc):
    """w1 [256,33], wh 4 x [256,256], wc [64,256] -> 36 chunks: fc1, K = 33 zero-padded to 64 (2) | fc2 .. fc5 | fc_out_c."""
    assert w1.shape == (256, 33) and len(wh) == 4
    k1 = lambda c: lambda kk, h: (2 * (16 * c + kk) + h) if 2 * (16 * c + kk) + h < 33 else None
    return np.concatenate([chunk8(w1, k1(c)) for c in range(2)] + _hidden_and_out(wh, wc))


def conv_stream(w_oihw):
    """[256, cin, kh, kw] -> taps x cin / 32 chunks: chunk tap * (cin / 32) + blk, tap = (ky, kx) row-major."""
    cout, cin, kh, kw = w_oihw.shape
    assert cout == 256 and (kh * kw, cin) in CONV_SHAPES
    return np.concatenate([chunk8(w_oihw[:, :, tap // kw, tap % kw], lambda kk, h, blk=blk: 32 * blk + 16 * h + kk)
                           for tap in range(kh * kw) for blk in range(cin // 32)])


# ------------------------------------------------------------------------------------------------- readers: place -> A operand
def read_chunk8(stream, c):
    """A[kk][ib][h][j]: what lane (h, j) feeds the MFMA of block ib in k-step kk of 8-block chunk c -- float
    512 kk + 256 (ib / 4) + 4 lane + ib % 4 of the chunk, lane = 32 h + j."""
    kk, ib, h, j = np.ix_(range(16), range(8), range(2), range(32))
    return stream[c * CHUNK_FLOATS + 512 * kk + 256 * (ib // 4) + 4 * (32 * h + j) + ib % 4]


def read_chunk2(stream, c):
    """A[kk][ib][h][j] of 2-block chunk c: float 128 kk + 2 lane + ib."""
    kk, ib, h, j = np.ix_(range(64), range(2), range(2), range(32))
    return stream[c * CHUNK_FLOATS + 128 * kk + 2 * (32 * h + j) + ib]


def mfma(A, B):
    """sum over k-steps and the two lane halves (the MFMA's K = 2) of A[kk][ib][h][i] B[kk][h][col] -> [32 ib + i][col]."""
    out = np.einsum("kbhi,khc->bic", A, B)
    return out.reshape(-1, B.shape[-1])


def registers(x):
    """Activations x [256, cols] as the accumulators hold them: [block b][register r][lane half h][col] = channel 32 b + kmap(r, h)."""
    return np.stack([np.stack([np.stack([x[32 * b + kmap(r, h)] for h in range(2)]) for r in range(16)]) for b in range(8)])


def mlp_layers_product(stream, first_chunks, first_B, n_hidden, xs, x_out):
    """The products an MLP kernel forms from `stream`: the first layer on first_B (one B [16][2][cols] per chunk), hidden layer l on
    xs[l], fc_out_c on x_out -- each input fed as the kernel feeds it, register r of block b in k-step r of chunk b."""
    outs = [sum(mfma(read_chunk8(stream, c), first_B[c]) for c in range(first_chunks))]
    for l in range(n_hidden):
        R = registers(xs[l])
        outs.append(sum(mfma(read_chunk8(stream, first_chunks + 8 * l + b), R[b]) for b in range(8)))
    R = registers(x_out).reshape(2, 64, 2, -1)          # chunk C: k-step kk = register kk % 16 of block 4 C + kk / 16
    c0 = first_chunks + 8 * n_hidden
    outs.append(sum(mfma(read_chunk2(stream, c0 + C), R[C]) for C in range(2)))
    return outs


def position_weights(shapes):
    """One f32 matrix per shape whose entries are distinct integers below 2^24 that name their own place:
    1 + layer * 2^17 + row * K + k (1 + the flat index for a single tensor)."""
    out = []
    for layer, shp in enumerate(shapes):
        n = int(np.prod(shp))
        assert n <= 1 << 17 or len(shapes) == 1
        out.append((1 + layer * (1 << 17) + np.arange(n)).astype(np.float32).reshape(shp))
    assert float(out[-1].max()) < 2 ** 24
    return out
