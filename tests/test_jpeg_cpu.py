"""The JPEG encoder's specification and host code without a GPU: tests/jpeg_ref.py (the numpy restatement the GPU bytes are held
to in tests/test_jpeg_gpu.py) is qualified against Pillow's decoder and encoder, the standard tables of scenedreamer_amd/jpeg.py
are pinned to the ones Pillow writes, and the header, the C ABI entries, mp4.append_encoded and the FrameWriter backend are checked."""
import ctypes
import io
import os
import struct

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_ref as JR

ENTRIES = ("sdn_jpeg_scan_bound", "sdn_jpeg_workspace_bytes", "sdn_jpeg_encode_scan")


@pytest.fixture(scope="module")
def encoded():
    """(image name, quality, restart_mcus) -> (file, scan, counters), computed once for the module."""
    out = {}
    for name, img in JR.images().items():
        for q in JR.QUALITIES:
            for ri in JR.intervals_of(img):
                out[(name, q, ri)] = JR.encode(img, q, ri)
    return out


def _pillow_mae(img, quality):
    buf = io.BytesIO()
    Image.fromarray(img, "RGB").save(buf, format="JPEG", quality=quality, subsampling=0)
    dec = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB")).astype(np.int64)
    return float(np.abs(dec - img.astype(np.int64)).mean())


def test_pillow_decodes_every_case_within_the_error_of_its_own_encoder(encoded):
    """Decodability and decoded-image error: mean absolute error against the source <= 1.05 x Pillow's own encoder at the same
    quality with subsampling=0, plus 0.02 grey levels."""
    imgs = JR.images()
    worst = 0.0
    for (name, q, ri), (data, _, _) in encoded.items():
        img = imgs[name]
        im = Image.open(io.BytesIO(data))
        im.load()
        assert im.mode == "RGB" and im.size == (img.shape[1], img.shape[0]), (name, q, ri)
        mae = float(np.abs(np.asarray(im).astype(np.int64) - img.astype(np.int64)).mean())
        ref = _pillow_mae(img, q)
        print(f"{name} q={q} Ri={ri}: mae {mae:.4f} pillow {ref:.4f}")
        assert mae <= 1.05 * ref + 0.02, (name, q, ri, mae, ref)
        worst = max(worst, mae / ref if ref > 0 else 0.0)
    print("largest ratio", worst)


def test_interval_length_does_not_change_the_decoded_image(encoded):
    imgs = JR.images()
    for name, img in imgs.items():
        for q in JR.QUALITIES:
            dec = [np.asarray(Image.open(io.BytesIO(encoded[(name, q, ri)][0])).convert("RGB")) for ri in JR.intervals_of(img)]
            for d in dec[1:]:
                np.testing.assert_array_equal(d, dec[0])


def test_image_set_covers_every_path_of_the_entropy_coder(encoded):
    cnts = [c for _, _, c in encoded.values()]
    assert sum(c["zrl"] for c in cnts) >= 1
    assert sum(c["no_eob"] for c in cnts) >= 1
    assert sum(c["stuffed"] for c in cnts) >= 1
    assert max(c["max_ac_cat"] for c in cnts) == 10
    assert max(c["max_dc_cat"] for c in cnts) == 11
    assert max(c["max_interval_blocks"] for c in cnts) > 64
    assert max(c["intervals"] for c in cnts) > 8                                  # the RST index wraps
    # per image, what it is in the set for
    at = lambda name, q, key: max(encoded[(name, q, ri)][2][key] for ri in JR.intervals_of(JR.images()[name]))
    assert at("checker", 100, "max_ac_cat") == 10 and at("dots", 100, "max_dc_cat") == 11
    assert at("smooth", 50, "zrl") >= 1 and at("smooth", 100, "zrl") >= 1 and encoded[("smooth", 92, None)][2]["max_interval_blocks"] == 75
    assert at("smooth_noise", 92, "zrl") >= 1 and at("smooth_noise", 100, "no_eob") >= 1
    assert at("noise", 92, "stuffed") >= 1
    assert all(c["max_ac_cat"] == 0 for (n, _, _), (_, _, c) in encoded.items() if n == "constant")


def test_standard_tables_equal_pillows():
    from scenedreamer_amd import jpeg
    dht, _ = JR.pillow_tables(50)
    assert set(dht) == set(jpeg.HUFFMAN)
    for key, (bits, vals) in dht.items():
        assert jpeg.HUFFMAN[key] == (bits, vals), key
    for q in (1, 25, 50, 75, 92, 100):
        _, dqt = JR.pillow_tables(q)
        ours = jpeg.quant_tables(q)
        for t in (0, 1):
            assert tuple(ours[t][z] for z in jpeg.ZIGZAG) == dqt[t], (q, t)
            assert tuple(int(x) for x in JR.quant_tables(q)[t]) == ours[t], (q, t)
    # the segments themselves, byte for byte
    buf = io.BytesIO()
    Image.fromarray(np.zeros((8, 8, 3), np.uint8), "RGB").save(buf, format="JPEG", quality=92, subsampling=0)
    theirs = b"".join(seg for m, seg, _ in JR.segments(buf.getvalue()) if m == 0xC4)
    ours = b"".join(seg for m, seg, _ in JR.segments(jpeg.header(8, 8, 92, 1) + jpeg.EOI) if m == 0xC4)
    assert ours == theirs


def test_header_parses_back():
    from scenedreamer_amd import jpeg
    for (H, W, q, ri) in ((1, 1, 50, 1), (33, 70, 92, 9), (2160, 3840, 100, 65535)):
        hdr = jpeg.header(H, W, q, ri)
        assert hdr == JR.header(H, W, q, ri)
        segs = JR.segments(hdr + jpeg.EOI)
        assert [m for m, _, _ in segs] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA, "scan"]
        assert segs[-1][1] == b"" and segs[-1][2] == len(hdr)                    # lengths consistent: the walk ends at the scan
        assert segs[0][1] == b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00"
        assert [s[0] for _, s, _ in segs[1:3]] == [0, 1] and all(len(s) == 65 for _, s, _ in segs[1:3])
        assert segs[3][1] == bytes([8]) + struct.pack(">HH", H, W) + bytes([3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
        assert [s[0] for _, s, _ in segs[4:8]] == [0x00, 0x10, 0x01, 0x11]
        assert struct.unpack(">H", segs[8][1])[0] == ri
        assert segs[9][1] == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    for bad in ((8, 8, 0, 1), (8, 8, 101, 1), (8, 8, 92, 0), (8, 8, 92, 65536), (0, 8, 92, 1), (8, 65536, 92, 1)):
        with pytest.raises(ValueError):
            jpeg.header(*bad)


def test_entries_are_exported_declared_and_sized(encoded):
    from scenedreamer_amd import capi
    lib = capi.lib()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in capi.declared_symbols()
    assert lib.sdn_abi_version() == 5
    imgs = JR.images()
    for (name, q, ri), (_, scan, _) in encoded.items():
        H, W, _ = imgs[name].shape
        bw, bh = -(-W // 8), -(-H // 8)
        r = bw if ri is None else ri
        bound = lib.sdn_jpeg_scan_bound(H, W, r)
        assert bound == 1248 * bw * bh + 3 * -(-bw * bh // r)
        assert len(scan) <= bound, (name, q, ri)
        assert lib.sdn_jpeg_workspace_bytes(H, W, r) >= bw * bh * (3 * 64 * 2 + 3 * 208)
    assert lib.sdn_jpeg_workspace_bytes(2160, 3840, 480) < 2 ** 28
    for bad in ((0, 8, 1), (8, 0, 1), (65536, 8, 1), (8, 8, 0), (8, 8, 65536), (40000, 40000, 1)):
        assert lib.sdn_jpeg_scan_bound(*bad) == 0 and lib.sdn_jpeg_workspace_bytes(*bad) == 0, bad


def test_argument_validation_without_a_gpu():
    """Rejected before any launch with -2 and a message: quality outside 1 .. 100, restart_mcus outside 1 .. 65535, a null pointer
    on a non-empty frame."""
    from scenedreamer_amd import capi
    lib = capi.lib()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)
    msg = lambda: lib.sdn_last_error().decode()
    for q in (0, -3, 101):
        assert lib.sdn_jpeg_encode_scan(p, 8, 8, q, 1, p, p, p, 0, None) == -2 and "quality must be 1 .. 100" in msg()
    for ri in (0, -1, 65536):
        assert lib.sdn_jpeg_encode_scan(p, 8, 8, 92, ri, p, p, p, 0, None) == -2 and "restart_mcus must be 1 .. 65535" in msg()
    for k in range(4):
        ptrs = [p, p, p, p]
        ptrs[k] = None
        assert lib.sdn_jpeg_encode_scan(ptrs[0], 8, 8, 92, 1, ptrs[1], ptrs[2], ptrs[3], 0, None) == -2 and "null pointer" in msg()
    assert lib.sdn_jpeg_encode_scan(p, 65536, 8, 92, 1, p, p, p, 0, None) == -2 and "H and W" in msg()
    assert lib.sdn_jpeg_encode_scan(p, 40000, 40000, 92, 1, p, p, p, 0, None) == -2 and "too large" in msg()
    assert lib.sdn_jpeg_encode_scan(None, 0, 8, 92, 1, None, None, None, 0, None) == 0           # an empty frame is a no-op


def test_encoder_has_no_cpu_substitute():
    from scenedreamer_amd import jpeg, ops
    with pytest.raises(ValueError, match="no CPU substitute"):
        jpeg.JpegEncoder(8, 8, device="cpu")
    z = torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.jpeg_encode_scan(z, 92, 1, z, z, torch.zeros(1, dtype=torch.int32))


def test_append_encoded_roundtrip(tmp_path, encoded):
    from scenedreamer_amd.mp4 import Mp4MjpegWriter, read_frames
    img = JR.images()["smooth_noise"]
    files = [encoded[("smooth_noise", q, None)][0] for q in JR.QUALITIES]
    w = Mp4MjpegWriter(str(tmp_path / "a.mp4"), fps=10)
    for f in files:
        w.append_encoded(f, img.shape[1], img.shape[0])
    with pytest.raises(ValueError, match="frame size changed"):
        w.append_encoded(files[0], img.shape[1] + 8, img.shape[0])
    w.close()
    fps, frames = read_frames(str(tmp_path / "a.mp4"))
    assert fps == 10 and len(frames) == 3
    for f, got in zip(files, frames):
        np.testing.assert_array_equal(got, np.asarray(Image.open(io.BytesIO(f)).convert("RGB")))
    raw = open(tmp_path / "a.mp4", "rb").read()
    assert all(f in raw for f in files)
    # append and append_encoded share the bookkeeping: a Pillow-encoded frame after GPU-style samples lands in the same index
    w = Mp4MjpegWriter(str(tmp_path / "b.mp4"), fps=10)
    w.append_encoded(files[0], img.shape[1], img.shape[0])
    w.append(img)
    with pytest.raises(ValueError, match="frame size changed"):
        w.append(img[:8])
    w.close()
    assert len(read_frames(str(tmp_path / "b.mp4"))[1]) == 2


def test_frame_writer_gpu_backend_rejects_cpu_images(tmp_path):
    from scenedreamer_amd.output import FrameWriter
    w = FrameWriter(None, video_path=str(tmp_path / "v.mp4"), video_backend="mjpeg-gpu")
    with pytest.raises(ValueError, match="mjpeg-gpu"):
        w.submit(torch.zeros(1, 3, 8, 8), 0)
    w.close()
    assert w.frames_done == 0


def test_auto_backend_resolves_as_before(tmp_path, monkeypatch):
    """"auto" is imageio where it opens, else the Pillow-encoding MJPEG writer: never the GPU backend."""
    from scenedreamer_amd import output
    from scenedreamer_amd.mp4 import Mp4MjpegWriter

    def no_imageio(path, fps):
        raise ImportError("imageio")

    monkeypatch.setattr(output, "_ImageioVideo", no_imageio)
    v = output.open_video(str(tmp_path / "a.mp4"), 10, "auto")
    assert type(v) is Mp4MjpegWriter
    v.close()
    with pytest.raises(ImportError):
        output.open_video(str(tmp_path / "b.mp4"), 10, "imageio")
    w = output.FrameWriter(None, video_path=str(tmp_path / "c.mp4"))
    assert not w.gpu_video and type(w.video) is Mp4MjpegWriter
    w.submit(torch.zeros(1, 3, 8, 8), 0)                                          # a CPU image is still fine with "auto"
    w.close()
    assert w.frames_done == 1

    class Sentinel:
        def __init__(self, path, fps):
            pass

        def close(self):
            pass

    monkeypatch.setattr(output, "_ImageioVideo", Sentinel)
    assert type(output.open_video(str(tmp_path / "d.mp4"), 10, "auto")) is Sentinel
    w = output.FrameWriter(None, video_path=str(tmp_path / "e.mp4"), video_backend="auto")
    assert not w.gpu_video and type(w.video) is Sentinel
    w.close()


def test_cli_flag():
    from scenedreamer_amd import cli
    ap = cli.build_parser()
    assert ap.parse_args(["--output_dir", "x"]).video_backend == "auto"
    assert ap.parse_args(["--output_dir", "x", "--video-backend", "mjpeg-gpu"]).video_backend == "mjpeg-gpu"
    with pytest.raises(SystemExit):
        ap.parse_args(["--output_dir", "x", "--video-backend", "h265"])
