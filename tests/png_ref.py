"""numpy restatement of the PNG encoder's specification (csrc/png.hip's contract), written from the PNG specification and RFC 1950 /
1951: 8-bit RGB, the five filters with bpp = 3, per-row tokens (literals and distance-1 matches only), one dynamic-Huffman deflate
block per frame, the zlib wrapper with Adler-32.  encode() returns the file, the zlib stream, the filtered stream F, the filter types
and the code lengths.

The two choices the format leaves to the builder, restated from the comment at the top of png.hip:

LENGTHS (huff_lengths, used for the literal/length code with a limit of 15 and for the code-length code with a limit of 7).
  The used symbols (count > 0) are sorted ascending by (count, symbol).  A Huffman tree is built with two queues, the sorted leaves
  and the internal nodes in the order they are made: each step takes the two smallest fronts, the leaf queue winning a tie against
  the internal queue, and appends their sum.  n[d] = number of leaves at depth min(d, limit).  While sum n[d] 2^(limit - d) exceeds
  2^limit: n[limit] -= 1; the largest d < limit with n[d] > 0 gives n[d] -= 1, n[d + 1] += 2.  The sorted symbols then receive the
  lengths from the longest down: the first n[limit] symbols get `limit`, the next n[limit - 1] get limit - 1, and so on.  A single
  used symbol gets length 1.  Codes are canonical (RFC 1951 3.2.2).
HEADER.  HLIT = max(257, 1 + the largest used literal/length symbol) - 257, HDIST = 0, HCLEN = 15 (all 19 code-length-code lengths
  are sent).  The HLIT + 257 literal/length lengths and the one distance length (1) are each sent as their own code-length symbol
  0 .. 15: symbols 16 - 18 are never used."""
import struct
import zlib

import numpy as np

import jpeg_ref

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}
MODES = (0, 1, 2, 3, 4, 5)
HEADER_MAX_BITS = 17 + 3 * 19 + 7 * 287


def length_symbol(n):
    """match length 3 .. 258 -> (symbol, extra value, extra bits)"""
    for k in range(28, -1, -1):
        if n >= LEN_BASE[k]:
            return 257 + k, n - LEN_BASE[k], LEN_EXTRA[k]
    raise ValueError(n)


# ---- filters --------------------------------------------------------------------------------------------------------------------------
def filter_candidates(img):
    """int64 [5, H, 3W]: the filtered bytes of every row under each of the five types."""
    H, W, _ = img.shape
    x = img.reshape(H, 3 * W).astype(np.int64)
    a = np.zeros_like(x)
    a[:, 3:] = x[:, :-3]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, 3:] = x[:-1, :-3]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([x, x - a, x - b, x - (a + b) // 2, x - paeth]) & 255


def scores(cand):
    """int64 [5, H]: sum over the row of b < 128 ? b : 256 - b"""
    return np.where(cand < 128, cand, 256 - cand).sum(-1)


def filtered(img, mode):
    """(F uint8 [H, 1 + 3W], types int64 [H])"""
    cand = filter_candidates(img)
    H = img.shape[0]
    types = np.full(H, mode, np.int64) if mode < 5 else np.argmin(scores(cand), axis=0)      # argmin: the first (smallest) minimum
    rows = cand[types, np.arange(H)]
    return np.concatenate([types[:, None], rows], 1).astype(np.uint8), types


# ---- tokens ---------------------------------------------------------------------------------------------------------------------------
def row_tokens(row):
    """[(symbol, extra value, extra bits)] of one row of F; a match is followed by its distance code by the packer."""
    r = [int(v) for v in row[1:]]
    out = [(int(row[0]), 0, 0)]
    n, k = len(r), 0
    while k < n:
        out.append((r[k], 0, 0))                    # r[k] != r[k - 1] or k == 0: a literal
        k += 1
        run = 0
        while k + run < n and r[k + run] == r[k + run - 1]:
            run += 1
        rest = run
        while rest > 0:
            piece = min(258, rest)
            if piece >= 3:
                out.append(length_symbol(piece))
            else:
                out.extend([(r[k], 0, 0)] * piece)
            rest -= piece
        k += run
    return out


# ---- Huffman --------------------------------------------------------------------------------------------------------------------------
def huff_lengths(counts, limit):
    n_sym = len(counts)
    order = sorted((s for s in range(n_sym) if counts[s] > 0), key=lambda s: (counts[s], s))
    n = len(order)
    lengths = [0] * n_sym
    if n == 0:
        return lengths
    if n == 1:
        lengths[order[0]] = 1
        return lengths
    w = [counts[s] for s in order]
    parent = [0] * (2 * n - 1)
    li, ii = 0, n
    for ni in range(n, 2 * n - 1):
        pick = []
        for _ in range(2):
            if li < n and (ii >= len(w) or w[li] <= w[ii]):
                pick.append(li)
                li += 1
            else:
                pick.append(ii)
                ii += 1
        w.append(w[pick[0]] + w[pick[1]])
        parent[pick[0]] = parent[pick[1]] = ni
    num = [0] * (limit + 1)
    for leaf in range(n):
        d, x = 0, leaf
        while x != 2 * n - 2:
            x = parent[x]
            d += 1
        num[min(d, limit)] += 1
    total = sum(num[d] << (limit - d) for d in range(1, limit + 1))
    while total > 1 << limit:
        num[limit] -= 1
        for d in range(limit - 1, 0, -1):
            if num[d]:
                num[d] -= 1
                num[d + 1] += 2
                break
        total -= 1
    k = 0
    for d in range(limit, 0, -1):
        for _ in range(num[d]):
            lengths[order[k]] = d
            k += 1
    assert k == n
    return lengths


def canonical_codes(lengths):
    """symbol -> code (RFC 1951 3.2.2), most significant bit first"""
    count = [0] * 17
    for n in lengths:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    codes = [0] * len(lengths)
    for s, n in enumerate(lengths):
        if n:
            codes[s] = nxt[n]
            nxt[n] += 1
    return codes


def kraft(lengths):
    """sum 2^-len in units of 2^-15"""
    return sum(1 << (15 - n) for n in lengths if n)


def _reverse(code, n):
    return int(format(code, f"0{n}b")[::-1], 2) if n else 0


class _Bits:
    """LSB-first bit string (RFC 1951 3.1.1): values as given, Huffman codes reversed by the caller"""

    def __init__(self):
        self.values, self.lengths = [], []

    def put(self, value, n):
        self.values.append(value)
        self.lengths.append(n)

    def to_bytes(self):
        v, n = np.array(self.values, np.int64), np.array(self.lengths, np.int64)
        bits = (v[:, None] >> np.arange(32)[None, :]) & 1
        keep = np.arange(32)[None, :] < n[:, None]
        return np.packbits(bits[keep].astype(np.uint8), bitorder="little").tobytes(), int(n.sum())


def adler32(data):
    """RFC 1950, restated: A = 1 + sum of the bytes, B = sum of the successive values of A, both mod 65521"""
    d = np.frombuffer(data, np.uint8).astype(np.int64)
    n = len(d)
    a = (1 + int(d.sum())) % 65521
    b = (n + int((d * np.arange(n, 0, -1)).sum())) % 65521
    return (b << 16) | a


def deflate(F):
    """(zlib stream, literal/length lengths, code-length-code lengths) of the filtered stream F [H, 1 + 3W]"""
    tokens = [t for row in F for t in row_tokens(row)]
    hist = [0] * 286
    for s, _, _ in tokens:
        hist[s] += 1
    hist[256] = 1
    ll = huff_lengths(hist, 15)
    ll_codes = canonical_codes(ll)
    nlit = max(257, 1 + max(s for s in range(286) if hist[s]))
    seq = ll[:nlit] + [1]                           # + the distance code: one symbol of length 1
    cl_hist = [0] * 19
    for v in seq:
        cl_hist[v] += 1
    cl = huff_lengths(cl_hist, 7)
    cl_codes = canonical_codes(cl)
    out = _Bits()
    out.put(1, 1)                                   # BFINAL
    out.put(2, 2)                                   # BTYPE = 10
    out.put(nlit - 257, 5)
    out.put(0, 5)
    out.put(15, 4)
    for s in CL_ORDER:
        out.put(cl[s], 3)
    for v in seq:
        out.put(_reverse(cl_codes[v], cl[v]), cl[v])
    assert sum(out.lengths) <= HEADER_MAX_BITS
    for s, extra, nextra in tokens:
        out.put(_reverse(ll_codes[s], ll[s]), ll[s])
        if s > 256:
            out.put(extra, nextra)
            out.put(0, 1)                           # distance 1: symbol 0, the code "0", no extra bits
    out.put(_reverse(ll_codes[256], ll[256]), ll[256])
    body, _ = out.to_bytes()
    return b"\x78\x01" + body + struct.pack(">I", adler32(F.tobytes())), ll, cl


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def file(H, W, stream):
    """signature, IHDR (8 bit, colour type 2, no interlace), one IDAT, IEND"""
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) + _chunk(b"IDAT", stream) +
            _chunk(b"IEND", b""))


def encode(img, filter_mode=5):
    """uint8 [H,W,3] -> dict(file, stream, F, types, ll, cl)"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3 and 0 <= filter_mode <= 5
    F, types = filtered(img, filter_mode)
    stream, ll, cl = deflate(F)
    return dict(file=file(img.shape[0], img.shape[1], stream), stream=stream, F=F, types=types, ll=ll, cl=cl)


def stream_bound(H, W):
    """sdn_png_stream_bound restated: 15 bits per position of F and for the end-of-block code, the longest header, rounded up to a
    byte, + 2 (zlib header) + 4 (Adler-32), rounded up to a multiple of 4"""
    return ((15 * (H * (1 + 3 * W) + 1) + HEADER_MAX_BITS + 7) // 8 + 6 + 3) // 4 * 4


# ---- the image set --------------------------------------------------------------------------------------------------------------------
RUN_BYTES = (2, 3, 4, 258, 259, 260, 261, 262, 517, 518)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def _filters_image():
    """Nine rows of 3 x 24 bytes: rows 0, 2, 4, 6, 8 are made for None (tied with Up on row 0), Up, Avg, Paeth and Sub."""
    W = 24
    rng = np.random.default_rng(11)
    x = np.zeros((9, 3 * W), np.int64)
    x[0] = (np.arange(3 * W) // 3 % 2) * 2                         # 0 0 0 2 2 2 0 0 0 ...: None = Up < Sub = Paeth
    for r in (1, 3, 5, 7):
        x[r] = rng.integers(0, 256, 3 * W)
    x[2] = x[1]
    x[6, :3] = (31, 207, 118)                                       # not the pixel above: the predictor then moves between a, b and c
    for j in range(3 * W):
        x[4, j] = ((x[4, j - 3] if j >= 3 else 0) + x[3, j]) // 2
        if j >= 3:
            x[6, j] = _paeth(x[6, j - 3], x[5, j], x[5, j - 3])
    x[8, :3] = (90, 140, 200)
    for j in range(3, 3 * W):
        x[8, j] = (x[8, j - 3] + 1) & 255
    return x.reshape(9, W, 3).astype(np.uint8)


def _runs_image():
    """One row per entry of RUN_BYTES: that many equal bytes from the start of the row, then bytes without a repeat.  Under filter None
    the rows hold e-runs of 1, 2, 3, 257 .. 261, 516 and 517 positions: below and at the shortest match, around one full piece with
    remainders of 0, 1, 2 and 3, and two pieces with remainders of 0 and 1."""
    W = 174                                                         # 522 bytes
    x = np.zeros((len(RUN_BYTES), 3 * W), np.uint8)
    for i, n in enumerate(RUN_BYTES):
        x[i, :n] = 40 + i
        x[i, n:] = 1 + (np.arange(3 * W - n) % 2) * 2               # 1 3 1 3 ...
    return x.reshape(len(RUN_BYTES), W, 3)


def _skewed_image():
    """89 x 66: under filter None the frame's histogram is the Fibonacci numbers 1, 1, 2, 3, ... 4181 and one larger count (symbol 256
    gives one 1, the 89 filter bytes give the 89), so the unlimited tree is 19 deep and the limit of 15 acts.  No two neighbouring bytes
    are equal, so no match changes the counts."""
    fib = [1, 1]
    while len(fib) < 19:
        fib.append(fib[-1] + fib[-2])
    left = {10 * i + 5: n for i, n in enumerate(fib[1:]) if n != 89}            # value -> count; the first 1 is symbol 256's
    left[250] = 89 * 66 * 3 - sum(left.values())
    assert left[250] >= fib[-1] + fib[-2]
    seq, last = [], -1
    for _ in range(89 * 66 * 3):                                                # the most frequent remaining value that is not the last
        v = max((v for v in left if v != last and left[v] > 0), key=lambda v: (left[v], v))
        left[v] -= 1
        seq.append(v)
        last = v
    return np.array(seq, np.uint8).reshape(89, 66, 3)


def images():
    """name -> uint8 [H,W,3] (fixed seeds)"""
    out = dict(jpeg_ref.images())
    out["column"] = np.random.default_rng(5).integers(0, 256, (33, 1, 3), dtype=np.uint8)
    out["row"] = np.random.default_rng(6).integers(0, 256, (1, 70, 3), dtype=np.uint8)
    wide = np.clip(jpeg_ref._smooth(3, 341) + np.random.default_rng(7).integers(-3, 4, (3, 341, 3)), 0, 255).astype(np.uint8)
    wide[1, 100:300] = wide[1, 100]                                 # a run across the 1024-byte boundary of the row
    out["wide"] = wide
    out["runs"] = _runs_image()
    out["grey86"] = np.full((5, 86, 3), 128, np.uint8)
    out["filters"] = _filters_image()
    out["skewed"] = _skewed_image()
    out["two_values"] = np.where(np.random.default_rng(8).integers(0, 2, (12, 20, 3)) == 1, 200, 7).astype(np.uint8)
    return out
