"""Timing record of the GPU PNG encoder (csrc/png.hip, scenedreamer_amd/png.py) against Pillow's encoder on one host thread.

    python tools/png_timing.py [--out profiles/png_gpu.json] [--no-render] [--small-only]
    python tools/png_timing.py --out profiles/png_gpu.json --merge-kernel-stats kernel_stats.csv      # no GPU needed

Frames: 540 x 960 and 2160 x 3840.  The pattern frames are a smooth sinusoid with a modular ramp plus +-6 noise; the rendered
540 x 960 frame comes from the renderer on the 2048^2 synthetic scene, and its 2160 x 3840 form is that frame enlarged four
times (bicubic) -- smoother than a frame rendered at that size.  Per frame: the median of 10 runs after 3 warm-ups of
`PngEncoder.encode` between two HIP events, of `Image.save(format="PNG", compress_level=4)` on this thread, and of the
device-to-pinned-host copies each path needs (the raw frame; the 4-byte length and the stream), with the bytes each moves, the file
sizes, and the sizes of the workspace and of one stream buffer (a FrameWriter slot).
--merge-kernel-stats: the kernel statistics of a `rocprofv3 --kernel-trace --stats -- python tools/png_timing.py --small-only` run (a
run of its own: the timings above are not taken under the profiler); the average time of every png_* and scan_* kernel is added to the
record that --out names, and nothing is measured."""
import argparse
import csv
import io
import json
import os
import statistics
import sys
import time
import zlib

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from jpeg_timing import gpu_ms, pattern, rendered  # noqa: E402  (the same frames as the JPEG record)

RUNS, WARMUP = 10, 3


def measure(name, frame):
    from scenedreamer_amd import png
    H, W, _ = frame.shape
    dev = torch.from_numpy(frame).cuda()
    enc = png.PngEncoder(H, W)
    data = enc.encode_to_bytes(dev)
    n = int(enc.nbytes.item())
    raw_host = torch.empty(dev.shape, dtype=torch.uint8, pin_memory=True)
    z_host = torch.empty(n, dtype=torch.uint8, pin_memory=True)
    len_host = torch.empty(1, dtype=torch.int32, pin_memory=True)

    def copy_encoded():
        len_host.copy_(enc.nbytes, non_blocking=True)
        z_host.copy_(enc.zstream[:n], non_blocking=True)

    rec = {"frame": name, "H": H, "W": W, "filter": "adaptive",
           "gpu_encode_ms": gpu_ms(lambda: enc.encode(dev)),
           "d2h_raw_ms": gpu_ms(lambda: raw_host.copy_(dev, non_blocking=True)),
           "d2h_encoded_ms": gpu_ms(copy_encoded),
           "pcie_bytes_raw": int(dev.numel()), "pcie_bytes_encoded": n + 4, "gpu_file_bytes": len(data),
           "workspace_bytes": int(enc.workspace.numel()), "stream_buffer_bytes": int(enc.zstream.numel())}
    rec["gpu_decodes_pixel_exact"] = bool(np.array_equal(np.asarray(Image.open(io.BytesIO(data))), frame))
    t0 = time.perf_counter()
    zlib.crc32(data)
    rec["host_crc32_ms"] = (time.perf_counter() - t0) * 1e3
    times, size = [], 0
    pil = Image.fromarray(frame, "RGB")
    for i in range(WARMUP + RUNS):
        buf = io.BytesIO()
        t0 = time.perf_counter()
        pil.save(buf, format="PNG", compress_level=4)
        if i >= WARMUP:
            times.append((time.perf_counter() - t0) * 1e3)
        size = buf.tell()
    rec.update(pillow_encode_ms=statistics.median(times), pillow_file_bytes=size, size_ratio_gpu_over_pillow=len(data) / size)
    return rec


def kernel_stats(path):
    """name -> average microseconds of the png_* / scan_* kernels in rocprofv3's kernel statistics"""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            avg = row.get("AverageNs") or row.get("Average") or row.get("AverageNs ")
            if avg and ("png_" in name or "scan_" in name):
                short = name.replace("(anonymous namespace)::", "").split("(")[0]
                out[short] = {"avg_us": float(avg) / 1e3, "calls": int(float(row.get("Calls", 0) or 0))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "png_gpu.json"))
    ap.add_argument("--no-render", action="store_true", help="pattern frames only")
    ap.add_argument("--small-only", action="store_true", help="the 540 x 960 pattern frame only (for a run under the profiler)")
    ap.add_argument("--merge-kernel-stats", default="", help="rocprofv3 kernel statistics (csv) of a separate --small-only run")
    args = ap.parse_args()
    if args.merge_kernel_stats:
        rec = json.load(open(args.out))
        rec["kernels_under_rocprofv3_540x960"] = kernel_stats(args.merge_kernel_stats)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
        print(json.dumps(rec["kernels_under_rocprofv3_540x960"]))
        return
    frames = [("pattern 540x960", pattern(540, 960))]
    if not args.small_only:
        frames.append(("pattern 2160x3840", pattern(2160, 3840)))
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
