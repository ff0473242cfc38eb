"""The PNG encoder's specification and host code without a GPU: tests/png_ref.py (the numpy restatement the GPU bytes are held to in
tests/test_png_gpu.py) is qualified against zlib's inflate and Pillow's decoder, its choices are recomputed by brute force, its size
is held to zlib's own run-length strategy, and the file framing, the C ABI entries, the FrameWriter backend and the CLI flag are
checked.

    python tests/test_png_cpu.py        # rewrites profiles/png_gpu.md, the table SIZE_RATIO below was taken from"""
import ctypes
import io
import os
import sys
import zlib

import numpy as np
import pytest

import png_ref as PR

ENTRIES = ("sdn_png_stream_bound", "sdn_png_workspace_bytes", "sdn_png_encode")

# Largest ratio over the six filter modes of the restatement's stream against zlib.compressobj(9, DEFLATED, 15, 9, Z_RLE) on the same
# F, measured on the CPU (profiles/png_gpu.md).  The test allows + 0.02: zlib versions split blocks differently; it is not room for a
# worse code.  The small images are dominated by the block header (no symbols 16 - 18: about 100 bytes).
SIZE_RATIO = {
    "pixel": 4.250, "constant": 1.778, "noise": 1.006, "checker": 1.141, "dots": 1.838, "smooth": 1.003, "smooth_noise": 1.003,
    "column": 1.098, "row": 1.203, "wide": 1.017, "runs": 1.051, "grey86": 2.222, "filters": 1.018, "skewed": 1.003, "two_values": 1.173,
}


@pytest.fixture(scope="module")
def images():
    return PR.images()


@pytest.fixture(scope="module")
def encoded(images):
    """(image name, filter_mode) -> png_ref.encode's record, computed once for the module."""
    return {(name, m): PR.encode(img, m) for name, img in images.items() for m in PR.MODES}


def _zlib_rle(F):
    co = zlib.compressobj(9, zlib.DEFLATED, 15, 9, zlib.Z_RLE)
    return co.compress(F.tobytes()) + co.flush()


def ratio_table(images, encoded):
    """[(name, shape, {mode: (ours, zlib's)})]"""
    return [(name, img.shape, {m: (len(encoded[(name, m)]["stream"]), len(_zlib_rle(encoded[(name, m)]["F"]))) for m in PR.MODES})
            for name, img in images.items()]


def test_image_set_holds_what_the_issue_lists(images):
    assert set(__import__("jpeg_ref").images()) <= set(images)
    assert images["column"].shape == (33, 1, 3) and images["row"].shape == (1, 70, 3) and images["wide"].shape == (3, 341, 3)
    assert images["grey86"].shape[1] == 86 and len(np.unique(images["grey86"])) == 1
    assert len(np.unique(images["two_values"])) == 2


def test_inflate_returns_the_filtered_stream_and_pillow_the_pixels(images, encoded):
    from PIL import Image
    for (name, m), e in encoded.items():
        img = images[name]
        assert e["F"].shape == (img.shape[0], 1 + 3 * img.shape[1])
        assert e["stream"][:2] == b"\x78\x01"
        assert zlib.decompress(e["stream"]) == e["F"].tobytes(), (name, m)
        assert (m == 5 or (e["types"] == m).all()) and (e["F"][:, 0] == e["types"]).all()
        im = Image.open(io.BytesIO(e["file"]))
        assert im.mode == "RGB" and im.size == (img.shape[1], img.shape[0]), (name, m)
        assert np.array_equal(np.asarray(im), img), (name, m)
        Image.open(io.BytesIO(e["file"])).verify()          # the CRCs


def _filter_row_slow(cur, prior, t):
    """One row, byte by byte, from the PNG specification's text."""
    out = []
    for j, x in enumerate(cur):
        a = cur[j - 3] if j >= 3 else 0
        b = prior[j] if prior is not None else 0
        c = prior[j - 3] if (prior is not None and j >= 3) else 0
        if t == 4:
            p = a + b - c
            pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
            pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
        else:
            pred = (0, a, b, (a + b) // 2)[t]
        out.append((x - pred) % 256)
    return out


def test_filters_and_the_adaptive_choice_equal_a_brute_force_recomputation(images, encoded):
    for name, img in images.items():
        rows = img.reshape(img.shape[0], -1).astype(int).tolist()
        chosen = []
        for y, cur in enumerate(rows):
            prior = rows[y - 1] if y else None
            cands = [_filter_row_slow(cur, prior, t) for t in range(5)]
            for t in range(5):
                assert encoded[(name, t)]["F"][y, 1:].tolist() == cands[t], (name, t, y)
            sums = [sum(b if b < 128 else 256 - b for b in cand) for cand in cands]
            best = min(range(5), key=lambda t: (sums[t], t))
            chosen.append(best)
            assert encoded[(name, 5)]["F"][y].tolist() == [best] + cands[best], (name, y)
        assert encoded[(name, 5)]["types"].tolist() == chosen, name


def test_filters_image_lets_every_type_win_and_holds_a_tie(images, encoded):
    img = images["filters"]
    types = encoded[("filters", 5)]["types"].tolist()
    assert set(types) == {0, 1, 2, 3, 4}
    s = PR.scores(PR.filter_candidates(img))                # [5, H]
    tied = [y for y in range(img.shape[0]) if (s[:, y] == s[:, y].min()).sum() > 1]
    assert tied and all(types[y] == int(np.flatnonzero(s[:, y] == s[:, y].min())[0]) for y in tied)
    assert 0 in tied and types[0] == 0 and s[0, 0] == s[2, 0]   # row 0: Up equals None, None wins


def test_run_edges_become_the_pieces_the_format_states(images, encoded):
    F = encoded[("runs", 0)]["F"]
    for row, n in zip(F, PR.RUN_BYTES):
        toks = PR.row_tokens(row)
        run = n - 1                                         # e-true positions
        lengths = [PR.LEN_BASE[s - 257] + x for s, x, _ in toks if s > 256]
        want = [258] * (run // 258) + ([run % 258] if run % 258 >= 3 else [])
        assert lengths == want, (n, lengths)
        literals = sum(1 for s, _, _ in toks if s < 256)
        assert literals == 1 + len(row[1:]) - sum(want), n      # the filter byte + every position no match covers
    g = PR.row_tokens(encoded[("grey86", 0)]["F"][0])
    assert g == [(0, 0, 0), (128, 0, 0), PR.length_symbol(257)]
    for n in range(3, 259):
        s, x, nx = PR.length_symbol(n)
        assert PR.LEN_BASE[s - 257] + x == n and 0 <= x < (1 << nx) and (n < 258 or s == 285)


def test_codes_are_complete_and_within_their_limits(encoded):
    deepest = 0
    for key, e in encoded.items():
        assert len(e["ll"]) == 286 and max(e["ll"]) <= 15 and PR.kraft(e["ll"]) == 1 << 15, key
        assert e["ll"][256] > 0
        assert len(e["cl"]) == 19 and max(e["cl"]) <= 7 and PR.kraft(e["cl"]) == 1 << 15 and e["cl"][16:] == [0, 0, 0], key
        deepest = max(deepest, max(e["ll"]))
    assert max(encoded[("skewed", 0)]["ll"]) == 15                              # ... and the limit is reached in the set
    assert min(sum(1 for n in e["ll"] if n) for e in encoded.values()) <= 4     # the degenerate tree is in the set
    # the limit itself: Fibonacci counts make an unlimited tree deeper than 15 (and than 7)
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    for counts, limit in ((fib + [0] * 246, 15), (fib[:19], 7), ([3, 1] + [0] * 17, 7), ([0, 5], 7)):
        ll = PR.huff_lengths(counts, limit)
        used = [n for n in ll if n]
        assert max(used) == min(limit, max(used)) and (len(used) == 1 or PR.kraft(ll) == 1 << 15)
        order = sorted((s for s in range(len(counts)) if counts[s]), key=lambda s: (counts[s], s))
        assert all(ll[a] >= ll[b] for a, b in zip(order, order[1:]))            # a rarer symbol never has the shorter code
    assert max(PR.huff_lengths(fib + [0] * 246, 15)) == 15 and max(PR.huff_lengths(fib[:19], 7)) == 7


def test_size_against_zlib_run_length_strategy(images, encoded):
    table = ratio_table(images, encoded)
    assert {name for name, _, _ in table} == set(SIZE_RATIO) == set(images)      # no image is left out
    for name, shape, per_mode in table:
        worst = max(ours / theirs for ours, theirs in per_mode.values())
        print(f"{name} {shape}: worst ratio {worst:.3f} (recorded {SIZE_RATIO[name]:.3f})")
        assert worst <= SIZE_RATIO[name] + 0.02, (name, worst)


def test_adler_and_file_framing(encoded, images):
    from scenedreamer_amd import png
    for (name, m), e in encoded.items():
        assert int.from_bytes(e["stream"][-4:], "big") == zlib.adler32(e["F"].tobytes()), (name, m)
        H, W, _ = images[name].shape
        assert png.file(H, W, e["stream"]) == e["file"]
    assert [png.filter_mode(k) for k in ("none", "sub", "up", "average", "paeth", "adaptive", 3)] == [0, 1, 2, 3, 4, 5, 3]
    for bad in ("best", 6, -1, None, True):
        with pytest.raises(ValueError):
            png.filter_mode(bad)
    for bad in ((0, 8), (8, 65536)):
        with pytest.raises(ValueError):
            png.file(*bad, b"")


def test_entries_are_exported_declared_and_sized(encoded, images):
    from scenedreamer_amd import capi
    lib = capi.lib()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in capi.declared_symbols()
    assert lib.sdn_abi_version() == 5
    for (name, m), e in encoded.items():
        H, W, _ = images[name].shape
        bound = lib.sdn_png_stream_bound(H, W)
        assert bound == PR.stream_bound(H, W) and bound % 4 == 0
        assert len(e["stream"]) <= bound, (name, m)
    sizes = [(1, 1), (1, 2), (2, 2), (33, 70), (34, 70), (34, 71), (540, 960), (2160, 3840), (2160, 3841), (4000, 7000)]
    for fn in (lib.sdn_png_stream_bound, lib.sdn_png_workspace_bytes):
        vals = [fn(h, w) for h, w in sizes]
        assert all(v > 0 for v in vals) and all(a <= b for a, b in zip(vals, vals[1:])), vals    # monotone in H and W
    assert lib.sdn_png_workspace_bytes(33, 70) >= 3 * 33 * (1 + 3 * 70)
    assert lib.sdn_png_workspace_bytes(2160, 3840) < 2 ** 27
    for bad in ((0, 8), (8, 0), (-1, 8), (65536, 8), (8, 65536), (40000, 40000)):
        assert lib.sdn_png_stream_bound(*bad) == 0 and lib.sdn_png_workspace_bytes(*bad) == 0, bad


def test_argument_validation_without_a_gpu():
    """Rejected before any launch with -2 and a message: filter_mode outside 0 .. 5, H or W outside 1 .. 65535, a null pointer on a
    non-empty frame, a frame whose bit count does not fit 32 bits."""
    from scenedreamer_amd import capi
    lib = capi.lib()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)
    msg = lambda: lib.sdn_last_error().decode()
    for m in (-1, 6, 100):
        assert lib.sdn_png_encode(p, 8, 8, m, p, p, p, 0, None) == -2 and "filter_mode must be 0 .. 5" in msg()
    for k in range(4):
        ptrs = [p, p, p, p]
        ptrs[k] = None
        assert lib.sdn_png_encode(ptrs[0], 8, 8, 5, ptrs[1], ptrs[2], ptrs[3], 0, None) == -2 and "null pointer" in msg()
    for hw in ((65536, 8), (8, 65536), (-1, 8), (8, -2)):
        assert lib.sdn_png_encode(p, hw[0], hw[1], 5, p, p, p, 0, None) == -2 and "H and W must be 1 .. 65535" in msg()
    assert lib.sdn_png_encode(p, 40000, 40000, 5, p, p, p, 0, None) == -2 and "too large" in msg()
    assert lib.sdn_png_encode(None, 0, 8, 5, None, None, None, 0, None) == 0            # an empty frame is a no-op
    assert lib.sdn_png_encode(None, 8, 0, 0, None, None, None, 0, None) == 0


def test_encoder_has_no_cpu_substitute():
    import torch
    from scenedreamer_amd import ops, png
    with pytest.raises(ValueError, match="no CPU substitute"):
        png.PngEncoder(8, 8, device="cpu")
    z = torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.png_encode(z, 5, z, z, torch.zeros(1, dtype=torch.int32))


def test_frame_writer_gpu_backend_rejects_cpu_images_and_other_formats(tmp_path):
    import torch
    from scenedreamer_amd.output import FrameWriter
    w = FrameWriter(str(tmp_path / "png"), png_backend="gpu")
    with pytest.raises(ValueError, match='png_backend="gpu"'):
        w.submit(torch.zeros(1, 3, 8, 8), 0)
    w.close()
    assert w.frames_done == 0 and os.listdir(tmp_path / "png") == []
    with pytest.raises(ValueError, match='fmt must be "png"'):
        FrameWriter(str(tmp_path / "npy"), fmt="npy", png_backend="gpu")
    with pytest.raises(ValueError, match="png_backend"):
        FrameWriter(str(tmp_path / "x"), png_backend="zopfli")
    # the default is the Pillow pool, and a CPU image is still fine with it
    w = FrameWriter(str(tmp_path / "cpu"))
    assert not w.gpu_png
    w.submit(torch.zeros(1, 3, 8, 8), 0)
    w.close()
    assert w.frames_done == 1


def test_cli_flag():
    from scenedreamer_amd import cli
    ap = cli.build_parser()
    assert ap.parse_args(["--output_dir", "x"]).png_backend == "pillow"
    assert ap.parse_args(["--output_dir", "x", "--png-backend", "gpu"]).png_backend == "gpu"
    with pytest.raises(SystemExit):
        ap.parse_args(["--output_dir", "x", "--png-backend", "zopfli"])


def _write_table():
    images = PR.images()
    encoded = {(name, m): PR.encode(img, m) for name, img in images.items() for m in PR.MODES}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ["# PNG encoder: stream size against zlib's run-length strategy (CPU, the restatement)", "",
             "`tests/png_ref.py`'s zlib stream against `zlib.compressobj(9, DEFLATED, 15, 9, Z_RLE)` on the same filtered stream F, per image",
             f"of the test set and per `filter_mode` (bytes ours / zlib's; zlib {zlib.ZLIB_RUNTIME_VERSION}).  The GPU's bytes equal the",
             "restatement's (`tests/test_png_gpu.py`), so these are the GPU's sizes too.  `tests/test_png_cpu.py` asserts the last column",
             "+ 0.02.  The block header always lists every code length by itself (no symbols 16 - 18), about 100 bytes that zlib's",
             "header does not spend: that is the whole difference on the small images.", "",
             "| image | H x W | " + " | ".join(f"mode {m}" for m in PR.MODES) + " | worst ratio |", "|---|---|" + "---|" * 7]
    for name, shape, per_mode in ratio_table(images, encoded):
        worst = max(o / z for o, z in per_mode.values())
        lines.append(f"| {name} | {shape[0]} x {shape[1]} | " + " | ".join(f"{o} / {z}" for o, z in per_mode.values()) + f" | {worst:.3f} |")
        print(f'    "{name}": {worst:.3f},')
    with open(os.path.join(root, "profiles", "png_gpu.md"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    _write_table()
