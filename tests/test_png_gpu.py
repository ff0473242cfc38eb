"""The PNG encoder on the MI355X (csrc/png.hip through scenedreamer_amd/png.py): the file's bytes equal tests/png_ref.py's with ==
for every image and filter mode that tests/test_png_cpu.py qualifies, whatever the launch shape, the history of the encoder's buffers
and the stream; and the frame pipeline with png_backend="gpu" delivers those bytes in every %05d.png while the Pillow path keeps its
own."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_ref as JR
import png_ref as PR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def images():
    return PR.images()


@pytest.fixture(scope="module")
def ref_files(images):
    """(image name, filter_mode) -> the restatement's file, computed once."""
    return {(name, m): PR.encode(img, m)["file"] for name, img in images.items() for m in PR.MODES}


def _first_difference(a, b):
    n = min(len(a), len(b))
    d = [i for i in range(n) if a[i] != b[i]]
    return f"lengths {len(a)} / {len(b)}, first difference at byte {d[0] if d else n}"


@pytest.mark.parametrize("name", list(PR.images()))
def test_bytes_equal_the_restatement(images, ref_files, name):
    from scenedreamer_amd import png
    img = images[name]
    dev = torch.from_numpy(img).cuda()
    for m in PR.MODES:
        got = png.PngEncoder(img.shape[0], img.shape[1], filter=m).encode_to_bytes(dev)
        want = ref_files[(name, m)]
        assert got == want, (name, m, _first_difference(got, want))


def test_launch_shape_does_not_reach_the_bytes(images, ref_files):
    from scenedreamer_amd import png
    for name, m in (("smooth", 5), ("noise", 3), ("runs", 0), ("wide", 4)):
        img = images[name]
        dev = torch.from_numpy(img).cuda()
        want = ref_files[(name, m)]
        for wg in (0, 1, 2, 7):
            got = png.PngEncoder(img.shape[0], img.shape[1], filter=m, n_workgroups=wg).encode_to_bytes(dev)
            assert got == want, (name, m, wg, _first_difference(got, want))


def test_an_encoder_can_be_used_again(ref_files):
    """A second call gives the same bytes (a histogram or a stream buffer that was not zeroed again would keep the first call's
    counts or bits), and so does a call after a frame of larger entropy."""
    from scenedreamer_amd import png
    smooth = np.clip(JR._smooth(33, 70), 0, 255).astype(np.uint8)
    noise = PR.images()["noise"]
    assert smooth.shape == noise.shape
    want = PR.encode(smooth, 5)["file"]
    enc = png.PngEncoder(33, 70)
    s, n = torch.from_numpy(smooth).cuda(), torch.from_numpy(noise).cuda()
    assert enc.encode_to_bytes(s) == want
    assert enc.encode_to_bytes(s) == want
    big = enc.encode_to_bytes(n)
    assert big == ref_files[("noise", 5)] and len(big) > len(want)
    assert enc.encode_to_bytes(s) == want


def test_two_frames_on_a_side_stream_without_host_synchronisation(images, ref_files):
    from scenedreamer_amd import png
    a, b = images["smooth_noise"], np.ascontiguousarray(images["smooth_noise"][::-1, ::-1])
    want = [ref_files[("smooth_noise", 5)], PR.encode(b, 5)["file"]]
    encs = [png.PngEncoder(64, 96), png.PngEncoder(64, 96)]
    devs = [torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        outs = [e.encode(d) for e, d in zip(encs, devs)]          # both enqueued before anything is read
    side.synchronize()
    for (zstream, nbytes), w in zip(outs, want):
        n = int(nbytes.item())
        assert png.file(64, 96, zstream[:n].cpu().numpy().tobytes()) == w


@pytest.fixture(scope="module")
def small_frames(weights_full, scene256):
    from scenedreamer_amd import camera, synth
    from scenedreamer_amd.renderer import Renderer
    R = Renderer(weights_full, scene256, "cuda")
    R.set_style(synth.make_style(8888))
    poses = camera.eval_camera_poses(scene256, maxstep=8)
    return [R.render_frame(poses[i], (72, 104), 12, mode="fused").clone() for i in (2, 3, 5)]


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def test_frame_writer_end_to_end(small_frames, tmp_path):
    from scenedreamer_amd.mp4 import read_frames
    from scenedreamer_amd.output import FrameWriter, to_uint8_hwc
    pix = [to_uint8_hwc(f).cpu().numpy() for f in small_frames]
    want = {f"{i:05d}.png": PR.encode(p, 5)["file"] for i, p in enumerate(pix)}

    def run(name, **kw):
        w = FrameWriter(str(tmp_path / name), **kw)
        for i, f in enumerate(small_frames):
            w.submit(f, i)
        w.close()
        assert w.frames_done == 3
        return _files(tmp_path / name)

    got = run("gpu", png_backend="gpu")
    assert got == want                                              # the restatement's file, byte for byte
    for i, p in enumerate(pix):
        np.testing.assert_array_equal(np.asarray(Image.open(io.BytesIO(got[f"{i:05d}.png"]))), p)
    # the Pillow path keeps its bytes: the same files as a writer constructed without the new arguments
    plain = run("plain")
    assert run("pillow", png_backend="pillow", png_slots=1) == plain and plain != want
    for i, p in enumerate(pix):
        buf = io.BytesIO()
        Image.fromarray(p, "RGB").save(buf, format="PNG", compress_level=4)
        assert plain[f"{i:05d}.png"] == buf.getvalue()
    # both GPU encoders: both outputs, and the raw frame is never copied
    assert run("both", png_backend="gpu", video_path=str(tmp_path / "both.mp4"), video_backend="mjpeg-gpu") == want
    fps, frames = read_frames(str(tmp_path / "both.mp4"))
    assert fps == 10 and len(frames) == 3
    for p, f in zip(pix, frames):                                   # the video samples are what tests/test_jpeg_gpu.py holds them to
        np.testing.assert_array_equal(f, np.asarray(Image.open(io.BytesIO(JR.encode(p, 92, None)[0])).convert("RGB")))
    # a CPU video backend beside the GPU PNG: the raw frame is still copied, for the video thread only
    assert run("cpu_video", png_backend="gpu", video_path=str(tmp_path / "cpu.mp4"), video_backend="mjpeg") == want
    assert len(read_frames(str(tmp_path / "cpu.mp4"))[1]) == 3
    assert run("one_slot", png_backend="gpu", png_slots=1, png_threads=1) == want
    assert run("forced", png_backend="gpu", png_filter="paeth") == {n: PR.encode(p, 4)["file"] for n, p in zip(want, pix)}


def test_trajectory_to_gpu_encoded_png_keeps_pace(weights_full, tmp_path):
    """tests/test_jpeg_gpu.py::test_trajectory_to_png_and_gpu_encoded_mp4_keeps_pace with the PNG backends: 16 pipelined 960 x 540
    frames to PNG + GPU-encoded MP4, delivered (files closed) at more than half the render-only rate.  The three rates are printed
    (README.md has the figures of one run)."""
    import time

    from scenedreamer_amd import camera, synth
    from scenedreamer_amd.output import FrameWriter, to_uint8_hwc
    from scenedreamer_amd.renderer import Renderer
    scene = synth.make_scene(2048, 3407, device="cuda")
    R = Renderer(weights_full, scene, "cuda")
    R.set_style(synth.make_style(8888))
    poses = camera.eval_camera_poses(scene, maxstep=40)
    sel = [poses[(3 * i) % 40] for i in range(16)]
    for _ in R.render_frames(sel[:3], (540, 960), 24, mode="fused"):     # warm-up
        pass
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in R.render_frames(sel, (540, 960), 24, mode="fused"):
        pass
    torch.cuda.synchronize()
    render_fps = len(sel) / (time.perf_counter() - t0)
    rates, keep, sizes = {}, {}, {}
    for backend in ("gpu", "pillow"):
        w = FrameWriter(str(tmp_path / backend), fmt="png", video_path=str(tmp_path / (backend + ".mp4")), fps=10, video_backend="mjpeg-gpu",
                        png_backend=backend)
        t0 = time.perf_counter()
        for i, img in enumerate(R.render_frames(sel, (540, 960), 24, mode="fused")):
            w.submit(img, i)
            if i == 9 and backend == "gpu":
                keep[i] = to_uint8_hwc(img).cpu().numpy()
        w.close()
        rates[backend] = len(sel) / (time.perf_counter() - t0)
        assert w.frames_done == len(sel)
        sizes[backend] = sum(os.path.getsize(tmp_path / backend / n) for n in os.listdir(tmp_path / backend)) / len(sel)
    print(f"render only {render_fps:.1f} frames/s, delivered as PNG + GPU-encoded MP4: png_backend gpu {rates['gpu']:.1f} frames/s "
          f"({sizes['gpu'] / 1e3:.0f} kB per file), pillow {rates['pillow']:.1f} frames/s ({sizes['pillow'] / 1e3:.0f} kB per file)")
    assert sorted(os.listdir(tmp_path / "gpu")) == [f"{i:05d}.png" for i in range(len(sel))]
    np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / "gpu" / "00009.png")), keep[9])
    Image.open(tmp_path / "gpu" / "00009.png").verify()
    assert rates["gpu"] > 0.5 * render_fps
