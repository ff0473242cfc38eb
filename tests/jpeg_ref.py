"""numpy restatement of the JPEG encoder's specification (csrc/jpeg.hip's contract), int64, written from the specification:
baseline sequential DCT, 8 bit, three components, 4:4:4, Annex K tables, restart intervals.  encode() returns the file, the scan
and the coverage counters of the entropy coder.  The Huffman tables are read from a file Pillow writes (they are data of the
standard; scenedreamer_amd/jpeg.py holds its own copy, pinned to the same source by tests/test_jpeg_cpu.py)."""
import functools
import io
import struct

import numpy as np
from PIL import Image

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
                   49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# ITU-T T.81 Annex K.1, natural order (= what Pillow writes at quality 50, where the scaling is 100 %)
QBASE = np.array([
    [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
    [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32],
    dtype=np.int64)

T = np.array([[np.rint(8192 * ((1 / np.sqrt(2)) if k == 0 else 1.0) / 2 * np.cos((2 * n + 1) * k * np.pi / 16)) for n in range(8)]
              for k in range(8)]).astype(np.int64)
# the committed table of 64 integers
assert T.tolist() == [[2896] * 8, [4017, 3406, 2276, 799, -799, -2276, -3406, -4017], [3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784],
                      [3406, -799, -4017, -2276, 2276, 4017, 799, -3406], [2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896],
                      [2276, -4017, 799, 3406, -3406, -799, 4017, -2276], [1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567],
                      [799, -2276, 3406, -4017, 4017, -3406, 2276, -799]]


def segments(data):
    """[(marker, payload, offset)] of the segments before the scan, then ("scan", bytes between SOS and EOI)."""
    assert data[:2] == b"\xff\xd8"
    out, pos = [], 2
    while True:
        assert data[pos] == 0xFF, pos
        m = data[pos + 1]
        n = struct.unpack(">H", data[pos + 2:pos + 4])[0]
        out.append((m, data[pos + 4:pos + 2 + n], pos))
        pos += 2 + n
        if m == 0xDA:
            assert data[-2:] == b"\xff\xd9"
            out.append(("scan", data[pos:-2], pos))
            return out


@functools.lru_cache(None)
def pillow_tables(quality=50):
    """({(class, id): (BITS, HUFFVAL)}, {id: 64 entries in zigzag order}) of a file Pillow writes without `optimize`."""
    buf = io.BytesIO()
    Image.fromarray(np.zeros((8, 8, 3), np.uint8), "RGB").save(buf, format="JPEG", quality=quality, subsampling=0)
    dht, dqt = {}, {}
    for m, seg, _ in segments(buf.getvalue()):
        p = 0
        while m == 0xC4 and p < len(seg):
            n = sum(seg[p + 1:p + 17])
            dht[(seg[p] >> 4, seg[p] & 15)] = (tuple(seg[p + 1:p + 17]), tuple(seg[p + 17:p + 17 + n]))
            p += 17 + n
        while m == 0xDB and p < len(seg):
            assert seg[p] >> 4 == 0
            dqt[seg[p] & 15] = tuple(seg[p + 1:p + 65])
            p += 65
    return dht, dqt


def quant_tables(quality):
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((QBASE * s + 50) // 100, 1, 255)


def canonical_codes(bits, vals):
    """symbol -> (code, length), assigned canonically (Annex C)."""
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return codes


def coefficients(rgb, quality):
    """int64 [bh, bw, 3, 64]: quantised coefficients in zigzag order."""
    H, W, _ = rgb.shape
    bh, bw = -(-H // 8), -(-W // 8)
    p = np.pad(rgb, ((0, 8 * bh - H), (0, 8 * bw - W), (0, 0)), mode="edge").astype(np.int64)
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    X = np.clip(np.stack([Y, Cb, Cr]), 0, 255) - 128                            # [3, 8bh, 8bw]
    X = X.reshape(3, bh, 8, bw, 8).transpose(1, 3, 0, 2, 4)                     # [bh, bw, 3, y, x]
    P = np.einsum("ky,...yx->...kx", T, X)
    P1 = (P + 512) >> 10
    Q = np.einsum("...kx,lx->...kl", P1, T)
    assert np.abs(Q).max() < 2 ** 31
    q = quant_tables(quality)[[0, 1, 1]].reshape(3, 8, 8)
    a = np.abs(Q)
    v = (a + (q << 15)) // (q << 16)
    v = np.where(Q < 0, -v, v)
    return v.reshape(bh, bw, 3, 64)[..., ZIGZAG]


def header(H, W, quality, Ri):
    dht, _ = pillow_tables()
    q = quant_tables(quality)
    seg = lambda m, payload: bytes([0xFF, m]) + struct.pack(">H", len(payload) + 2) + payload
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0" + bytes([1, 1, 0]) + struct.pack(">HH", 1, 1) + bytes([0, 0]))
    for t in (0, 1):
        out += seg(0xDB, bytes([t]) + bytes(int(x) for x in q[t][ZIGZAG]))
    out += seg(0xC0, bytes([8]) + struct.pack(">HH", H, W) + bytes([3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc, th in ((0, 0), (1, 0), (0, 1), (1, 1)):
        bits, vals = dht[(tc, th)]
        out += seg(0xC4, bytes([tc << 4 | th]) + bytes(bits) + bytes(vals))
    out += seg(0xDD, struct.pack(">H", Ri))
    out += seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def encode(rgb, quality, restart_mcus=None):
    """(file bytes, scan bytes, counters) for a uint8 [H,W,3] array."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    H, W, _ = rgb.shape
    co = coefficients(rgb, quality)
    bh, bw = co.shape[:2]
    n = bh * bw
    Ri = bw if restart_mcus is None else int(restart_mcus)
    assert 1 <= Ri <= 65535 and 1 <= quality <= 100
    co = co.reshape(n, 3, 64).tolist()
    dht, _ = pillow_tables()
    dc_codes = [canonical_codes(*dht[(0, t)]) for t in (0, 1)]
    ac_codes = [canonical_codes(*dht[(1, t)]) for t in (0, 1)]
    cnt = dict(zrl=0, no_eob=0, stuffed=0, max_ac_cat=0, max_dc_cat=0, max_interval_blocks=0, intervals=0)
    scan = bytearray()
    n_int = -(-n // Ri)
    cnt["intervals"] = n_int
    for s in range(n_int):
        acc, nbits = 0, 0                  # the interval's bit string as one integer

        def put(code, length):
            nonlocal acc, nbits
            acc = (acc << length) | code
            nbits += length

        def magnitude(v, cat):
            return (v - 1 if v < 0 else v) & ((1 << cat) - 1)

        pred = [0, 0, 0]
        mcus = range(s * Ri, min(n, (s + 1) * Ri))
        cnt["max_interval_blocks"] = max(cnt["max_interval_blocks"], 3 * len(mcus))
        for m in mcus:
            for c in range(3):
                blk, t = co[m][c], min(c, 1)
                diff = blk[0] - pred[c]
                pred[c] = blk[0]
                cat = abs(diff).bit_length()
                cnt["max_dc_cat"] = max(cnt["max_dc_cat"], cat)
                put(*dc_codes[t][cat])
                put(magnitude(diff, cat), cat)
                run = 0
                for k in range(1, 64):
                    v = blk[k]
                    if v == 0:
                        run += 1
                        continue
                    while run >= 16:
                        put(*ac_codes[t][0xF0])
                        cnt["zrl"] += 1
                        run -= 16
                    cat = abs(v).bit_length()
                    cnt["max_ac_cat"] = max(cnt["max_ac_cat"], cat)
                    put(*ac_codes[t][run * 16 + cat])
                    put(magnitude(v, cat), cat)
                    run = 0
                if blk[63] == 0:
                    put(*ac_codes[t][0x00])
                else:
                    cnt["no_eob"] += 1
        pad = -nbits % 8
        put((1 << pad) - 1, pad)
        raw = acc.to_bytes(nbits // 8, "big")
        cnt["stuffed"] += raw.count(0xFF)
        scan += raw.replace(b"\xff", b"\xff\x00")
        if s + 1 < n_int:
            scan += bytes([0xFF, 0xD0 + s % 8])
    scan = bytes(scan)
    return header(H, W, quality, Ri) + scan + b"\xff\xd9", scan, cnt


# ---- the image set ------------------------------------------------------------------------------------------------------------------
def _smooth(H, W):
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    r = 128 + 100 * np.sin(xx / 9.0) * np.cos(yy / 7.0)
    g = (xx * 3 + yy * 5) % 256                                     # the modular ramp: sharp edges in a smooth image
    b = 128 + 90 * np.cos((xx + 2 * yy) / 13.0)
    return np.stack([r, g, b], -1)


def images():
    """name -> uint8 [H,W,3] (fixed seeds)."""
    out = {}
    out["pixel"] = np.array([[[200, 30, 90]]], np.uint8)
    out["constant"] = np.full((8, 8, 3), (17, 130, 250), np.uint8)
    out["noise"] = np.random.default_rng(1).integers(0, 256, (33, 70, 3), dtype=np.uint8)
    yy, xx = np.meshgrid(np.arange(16), np.arange(24), indexing="ij")
    out["checker"] = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, -1)
    dots = np.zeros((24, 40, 3), np.uint8)
    rng = np.random.default_rng(2)
    dots[rng.integers(0, 24, 12), rng.integers(0, 40, 12)] = 255
    dots[8:16, 8:16] = 255                                          # one white block beside black ones: DC category 11
    out["dots"] = dots
    out["smooth"] = np.clip(_smooth(40, 200), 0, 255).astype(np.uint8)
    noise = np.random.default_rng(3).integers(-6, 7, (64, 96, 3))
    out["smooth_noise"] = np.clip(_smooth(64, 96) + noise, 0, 255).astype(np.uint8)
    return out


QUALITIES = (50, 92, 100)


def intervals_of(img):
    """restart_mcus of the cases: 1, 5, one MCU row (None: the default), larger than the frame's MCU count."""
    bh, bw = -(-img.shape[0] // 8), -(-img.shape[1] // 8)
    return (1, 5, None, bh * bw + 3)
