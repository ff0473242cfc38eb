"""Timing record of the GPU JPEG encoder (csrc/jpeg.hip, scenedreamer_amd/jpeg.py) against Pillow's encoder on one host thread.

    python tools/jpeg_timing.py [--out profiles/jpeg_gpu.json] [--no-render]

Frames: 540 x 960 and 2160 x 3840.  The pattern frames are a smooth sinusoid with a modular ramp plus +-6 noise; the rendered
540 x 960 frame comes from the renderer on the 2048^2 synthetic scene, and its 2160 x 3840 form is that frame enlarged four
times (bicubic) -- smoother than a frame rendered at that size.  Per frame: the median of 10 runs after 3 warm-ups of
`JpegEncoder.encode` between two HIP events, of `Image.save(format="JPEG", quality=92, subsampling=0)` on this thread, and of the
device-to-pinned-host copies each path needs (the raw frame; the 4-byte length and the scan), with the bytes each moves."""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RUNS, WARMUP = 10, 3


def pattern(H, W, seed=3):
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    r = 128 + 100 * np.sin(xx / 9.0) * np.cos(yy / 7.0)
    g = (xx * 3 + yy * 5) % 256
    b = 128 + 90 * np.cos((xx + 2 * yy) / 13.0)
    noise = np.random.default_rng(seed).integers(-6, 7, (H, W, 3))
    return np.clip(np.stack([r, g, b], -1) + noise, 0, 255).astype(np.uint8)


def rendered():
    from scenedreamer_amd import camera, synth
    from scenedreamer_amd.output import to_uint8_hwc
    from scenedreamer_amd.renderer import Renderer
    scene = synth.make_scene(2048, 3407, device="cuda")
    R = Renderer(synth.make_weights(0), scene, "cuda")
    R.set_style(synth.make_style(8888))
    img = R.render_frame(camera.eval_camera_poses(scene, maxstep=40)[9], (540, 960), 24, mode="fused")
    big = torch.nn.functional.interpolate(img, scale_factor=4, mode="bicubic", align_corners=False).clamp_(-1, 1)
    return to_uint8_hwc(img).cpu().numpy(), to_uint8_hwc(big).cpu().numpy()


def gpu_ms(fn):
    """Median over RUNS of the time between two events around fn() on the current stream, after WARMUP calls."""
    out = []
    for i in range(WARMUP + RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= WARMUP:
            out.append(a.elapsed_time(b))
    return statistics.median(out)


def measure(name, frame, quality=92):
    from scenedreamer_amd import jpeg
    H, W, _ = frame.shape
    dev = torch.from_numpy(frame).cuda()
    enc = jpeg.JpegEncoder(H, W, quality=quality)
    data = enc.encode_to_bytes(dev)
    n = len(data) - len(enc.header) - 2
    raw_host = torch.empty(dev.shape, dtype=torch.uint8, pin_memory=True)
    scan_host = torch.empty(n, dtype=torch.uint8, pin_memory=True)
    len_host = torch.empty(1, dtype=torch.int32, pin_memory=True)

    def copy_encoded():
        len_host.copy_(enc.nbytes, non_blocking=True)
        scan_host.copy_(enc.scan[:n], non_blocking=True)

    rec = {"frame": name, "H": H, "W": W, "quality": quality, "restart_mcus": enc.restart_mcus,
           "gpu_encode_ms": gpu_ms(lambda: enc.encode(dev)),
           "d2h_raw_ms": gpu_ms(lambda: raw_host.copy_(dev, non_blocking=True)),
           "d2h_encoded_ms": gpu_ms(copy_encoded),
           "pcie_bytes_raw": int(dev.numel()), "pcie_bytes_encoded": n + 4, "gpu_file_bytes": len(data),
           "workspace_bytes": int(enc.workspace.numel()), "scan_buffer_bytes": int(enc.scan.numel())}
    dec = np.asarray(Image.open(io.BytesIO(data)).convert("RGB")).astype(np.int64)
    rec["gpu_decoded_mae"] = float(np.abs(dec - frame.astype(np.int64)).mean())
    times, size = [], 0
    pil = Image.fromarray(frame, "RGB")
    for i in range(WARMUP + RUNS):
        buf = io.BytesIO()
        t0 = time.perf_counter()
        pil.save(buf, format="JPEG", quality=quality, subsampling=0)
        if i >= WARMUP:
            times.append((time.perf_counter() - t0) * 1e3)
        size = buf.tell()
    dec = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB")).astype(np.int64)
    rec.update(pillow_encode_ms=statistics.median(times), pillow_file_bytes=size,
               pillow_decoded_mae=float(np.abs(dec - frame.astype(np.int64)).mean()))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "jpeg_gpu.json"))
    ap.add_argument("--no-render", action="store_true", help="pattern frames only")
    args = ap.parse_args()
    frames = [("pattern 540x960", pattern(540, 960)), ("pattern 2160x3840", pattern(2160, 3840))]
    if not args.no_render:
        small, big = rendered()
        frames += [("rendered 540x960", small), ("rendered 540x960 enlarged to 2160x3840", big)]
    rec = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "warmup": WARMUP,
           "host_threads_for_pillow": 1, "frames": [measure(n, f) for n, f in frames]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
