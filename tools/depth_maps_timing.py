"""Timing record of the depth / opacity map kernels (csrc/maps.hip, scenedreamer_amd/maps.py).

    python tools/depth_maps_timing.py [--out profiles/depth_maps.json]

One process, HIP events, medians of 10 after 3 warm-ups, at 540 x 960 with 24 samples on the frame's window (the minimal apron:
548 x 968 rays, crop 4) of the 2048^2 synthetic scene:
  * sdn_depth_maps and sdn_depth_quantise against their traffic floor -- the bytes their shapes imply (both per-sample arrays read
    once, the maps written once) over the HBM peak of 8.0 TB/s;
  * the same maps by the PyTorch expression of the reference (scenedreamer.py:816, :821-823, :835-841) on the same arrays;
  * Renderer.render_frame(mode="fused") with and without maps on the same commit."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RUNS, WARMUP = 10, 3
HBM_PEAK_GBPS = 8000.0
HW, NS = (540, 960), 24


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


def torch_maps(w, z, rows, cols, crop):
    """The reference's expression on the window's arrays: composite, crop, normalise over the hits, 8-bit values."""
    d = torch.sum(w * z, -1).view(rows, cols)[crop:rows - crop, crop:cols - crop]
    o = torch.sum(w, -1).view(rows, cols)[crop:rows - crop, crop:cols - crop]
    hit = d > 0
    big = torch.where(hit, d, torch.full_like(d, float("inf"))).min()
    top = torch.where(hit, d, torch.zeros_like(d)).max()
    t = torch.where(hit, (d - big) / (top - big), torch.ones_like(d))
    return d, o, torch.round(t * 255).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "depth_maps.json"))
    args = ap.parse_args()
    from scenedreamer_amd import camera, maps, synth
    from scenedreamer_amd.renderer import Renderer
    scene = synth.make_scene(2048, 3407, device="cuda")
    R = Renderer(synth.make_weights(0), scene, "cuda")
    R.set_style(synth.make_style(8888))
    pose = camera.eval_camera_poses(scene, maxstep=40)[9]
    m = dict.fromkeys(("depth", "opacity", "depth_u8", "range", "weights", "sample_depth"))
    R.render_frame(pose, HW, NS, mode="fused", maps=m)
    rows, cols, crop = m["window"]
    w, z = m["weights"], m["sample_depth"]
    n_in, n_out = rows * cols, HW[0] * HW[1]
    bytes_maps = 2 * n_in * NS * 4 + 2 * n_out * 4                  # (the cropped rays' rows are not read: an upper bound within 3 %)
    rec = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "warmup": WARMUP, "frame_hw": list(HW), "num_samples": NS,
           "window": [rows, cols, crop], "hbm_peak_gbps": HBM_PEAK_GBPS,
           "hit_fraction": float((m["depth"] > 0).float().mean())}
    ms = gpu_ms(lambda: maps.depth_maps(w, z, rows, cols, crop))
    rec["sdn_depth_maps"] = {"ms": ms, "bytes": bytes_maps, "floor_ms": bytes_maps / (HBM_PEAK_GBPS * 1e6), "gbps": bytes_maps / ms / 1e6}
    d, _, rng = maps.depth_maps(w, z, rows, cols, crop)
    for bits in (8, 16):
        b = n_out * 4 + n_out * bits // 8
        ms = gpu_ms(lambda: maps.quantise(d, rng, bits))
        rec[f"sdn_depth_quantise_{bits}"] = {"ms": ms, "bytes": b, "floor_ms": b / (HBM_PEAK_GBPS * 1e6), "gbps": b / ms / 1e6}
    rec["torch_expression_ms"] = gpu_ms(lambda: torch_maps(w, z, rows, cols, crop))
    td, _, tu8 = torch_maps(w, z, rows, cols, crop)
    rec["torch_vs_kernel"] = {"depth_max_abs": float((td - m["depth"]).abs().max()), "u8_pixels_differ": int((tu8 != m["depth_u8"]).sum())}
    rec["render_frame_fused_ms"] = gpu_ms(lambda: R.render_frame(pose, HW, NS, mode="fused"))
    rec["render_frame_fused_with_maps_ms"] = gpu_ms(lambda: R.render_frame(pose, HW, NS, mode="fused", maps={}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
