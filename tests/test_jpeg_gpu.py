"""The JPEG encoder on the MI355X (csrc/jpeg.hip through scenedreamer_amd/jpeg.py): the bytes equal tests/jpeg_ref.py's with ==
for every image, quality and restart interval that tests/test_jpeg_cpu.py qualifies, whatever the launch shape, the history of
the encoder's buffers and the stream; and the frame pipeline with video_backend="mjpeg-gpu" delivers those bytes in the MP4 while
the PNG path is untouched."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_ref as JR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def images():
    return JR.images()


@pytest.fixture(scope="module")
def ref_files(images):
    """(image name, quality, restart_mcus) -> the restatement's file, computed once."""
    return {(name, q, ri): JR.encode(img, q, ri)[0] for name, img in images.items() for q in JR.QUALITIES for ri in JR.intervals_of(img)}


def _first_difference(a, b):
    n = min(len(a), len(b))
    d = [i for i in range(n) if a[i] != b[i]]
    return f"lengths {len(a)} / {len(b)}, first difference at byte {d[0] if d else n}"


@pytest.mark.parametrize("name", list(JR.images()))
def test_bytes_equal_the_restatement(images, ref_files, name):
    from scenedreamer_amd import jpeg
    img = images[name]
    dev = torch.from_numpy(img).cuda()
    for q in JR.QUALITIES:
        for ri in JR.intervals_of(img):
            enc = jpeg.JpegEncoder(img.shape[0], img.shape[1], quality=q, restart_mcus=ri)
            got = enc.encode_to_bytes(dev)
            want = ref_files[(name, q, ri)]
            assert got == want, (name, q, ri, _first_difference(got, want))


def test_launch_shape_does_not_reach_the_bytes(images, ref_files):
    from scenedreamer_amd import jpeg
    for name, q, ri in (("smooth", 100, None), ("noise", 92, 5), ("smooth_noise", 92, 1), ("dots", 100, 18)):
        img = images[name]
        dev = torch.from_numpy(img).cuda()
        want = ref_files[(name, q, ri)]
        for wg in (0, 1, 2, 7):
            got = jpeg.JpegEncoder(img.shape[0], img.shape[1], quality=q, restart_mcus=ri, n_workgroups=wg).encode_to_bytes(dev)
            assert got == want, (name, q, ri, wg, _first_difference(got, want))


def test_an_encoder_can_be_used_again(ref_files):
    """A second call gives the same bytes (a buffer that was not zeroed again would keep the first call's bits), and so does
    a call after a frame of larger entropy."""
    from scenedreamer_amd import jpeg
    smooth = np.clip(JR._smooth(33, 70), 0, 255).astype(np.uint8)
    noise = JR.images()["noise"]
    assert smooth.shape == noise.shape
    want = JR.encode(smooth, 92, 5)[0]
    enc = jpeg.JpegEncoder(33, 70, quality=92, restart_mcus=5)
    s, n = torch.from_numpy(smooth).cuda(), torch.from_numpy(noise).cuda()
    assert enc.encode_to_bytes(s) == want
    assert enc.encode_to_bytes(s) == want
    big = enc.encode_to_bytes(n)
    assert big == ref_files[("noise", 92, 5)] and len(big) > len(want)
    assert enc.encode_to_bytes(s) == want


def test_two_frames_on_a_side_stream_without_host_synchronisation(images, ref_files):
    from scenedreamer_amd import jpeg
    a, b = images["smooth_noise"], np.ascontiguousarray(images["smooth_noise"][::-1, ::-1])
    want = [ref_files[("smooth_noise", 92, None)], JR.encode(b, 92, None)[0]]
    encs = [jpeg.JpegEncoder(64, 96), jpeg.JpegEncoder(64, 96)]
    devs = [torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        outs = [e.encode(d) for e, d in zip(encs, devs)]          # both enqueued before anything is read
    side.synchronize()
    for (scan, nbytes), e, w in zip(outs, encs, want):
        n = int(nbytes.item())
        assert e.header + scan[:n].cpu().numpy().tobytes() + jpeg.EOI == w


@pytest.fixture(scope="module")
def small_frames(weights_full, scene256):
    from scenedreamer_amd import camera, synth
    from scenedreamer_amd.renderer import Renderer
    R = Renderer(weights_full, scene256, "cuda")
    R.set_style(synth.make_style(8888))
    poses = camera.eval_camera_poses(scene256, maxstep=8)
    return [R.render_frame(poses[i], (72, 104), 12, mode="fused").clone() for i in (2, 3, 5)]


def test_frame_writer_end_to_end(small_frames, tmp_path):
    from scenedreamer_amd.mp4 import read_frames
    from scenedreamer_amd.output import FrameWriter, to_uint8_hwc
    pix = [to_uint8_hwc(f).cpu().numpy() for f in small_frames]
    w = FrameWriter(str(tmp_path / "png"), video_path=str(tmp_path / "gpu.mp4"), video_backend="mjpeg-gpu")
    for i, f in enumerate(small_frames):
        w.submit(f, i)
    w.close()
    assert w.frames_done == 3
    fps, frames = read_frames(str(tmp_path / "gpu.mp4"))
    assert fps == 10 and len(frames) == 3
    raw = open(tmp_path / "gpu.mp4", "rb").read()
    for p, got in zip(pix, frames):
        want = JR.encode(p, 92, None)[0]
        assert want in raw                                         # the sample is the restatement's file, byte for byte
        np.testing.assert_array_equal(got, np.asarray(Image.open(io.BytesIO(want)).convert("RGB")))
    for i, p in enumerate(pix):
        np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / "png" / f"{i:05d}.png")), p)
    w2 = FrameWriter(str(tmp_path / "png2"), video_path=str(tmp_path / "cpu.mp4"), video_backend="mjpeg")
    for i, f in enumerate(small_frames):
        w2.submit(f, i)
    w2.close()
    for i in range(3):
        name = f"{i:05d}.png"
        assert open(tmp_path / "png" / name, "rb").read() == open(tmp_path / "png2" / name, "rb").read()


def test_video_only(small_frames, tmp_path):
    from scenedreamer_amd.mp4 import read_frames
    from scenedreamer_amd.output import FrameWriter, to_uint8_hwc
    w = FrameWriter(None, video_path=str(tmp_path / "v.mp4"), video_backend="mjpeg-gpu", video_slots=1)
    order = [0, 1, 2, 0, 2]
    for i, k in enumerate(order):
        w.submit(small_frames[k], i)
    w.close()
    assert w.frames_done == len(order) and not os.path.exists(tmp_path / "png")
    _, frames = read_frames(str(tmp_path / "v.mp4"))
    assert len(frames) == len(order)
    for k, got in zip(order, frames):
        want = JR.encode(to_uint8_hwc(small_frames[k]).cpu().numpy(), 92, None)[0]
        np.testing.assert_array_equal(got, np.asarray(Image.open(io.BytesIO(want)).convert("RGB")))


def test_trajectory_to_png_and_gpu_encoded_mp4_keeps_pace(weights_full, tmp_path):
    """tests/test_fullsize_gpu.py::test_trajectory_to_png_and_mp4_keeps_pace with the GPU backend: 16 pipelined 960 x 540 frames
    to PNG + MP4, delivered (files closed) at more than half the render-only rate.  Both backends' rates are printed (one run on
    one MI355X: render only 55.6, GPU-encoded 47.2, Pillow-encoded 46.9 frames/s -- the PNG pool is the slower consumer there)."""
    import time

    from scenedreamer_amd import camera, synth
    from scenedreamer_amd.mp4 import read_frames
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
    rates, keep = {}, {}
    for backend in ("mjpeg-gpu", "mjpeg"):
        w = FrameWriter(str(tmp_path / backend), fmt="png", video_path=str(tmp_path / (backend + ".mp4")), fps=10, video_backend=backend)
        t0 = time.perf_counter()
        for i, img in enumerate(R.render_frames(sel, (540, 960), 24, mode="fused")):
            w.submit(img, i)
            if i == 9 and backend == "mjpeg-gpu":
                keep[i] = to_uint8_hwc(img).cpu().numpy()
        w.close()
        rates[backend] = len(sel) / (time.perf_counter() - t0)
        assert w.frames_done == len(sel)
    print(f"render only {render_fps:.1f} frames/s, delivered as PNG + MP4: GPU-encoded {rates['mjpeg-gpu']:.1f} frames/s, "
          f"Pillow-encoded {rates['mjpeg']:.1f} frames/s")
    np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / "mjpeg-gpu" / "00009.png")), keep[9])
    fps, frames = read_frames(str(tmp_path / "mjpeg-gpu.mp4"))
    assert fps == 10 and len(frames) == len(sel)
    assert np.abs(frames[9].astype(np.int32) - keep[9].astype(np.int32)).mean() < 4.0      # JPEG
    assert rates["mjpeg-gpu"] > 0.5 * render_fps
