#!/usr/bin/env python
"""Headline benchmark: rendered frames/s at 960x540, 24 samples/ray, scene_size 2048 (BASELINE.json).

    python bench.py --gpus 1 --steps 20 --warmup 3
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One "step" = every rank renders ONE complete frame of the reference's pattern-0 camera orbit
(ray casting on the padded 570x990 frame -> sky MLP -> per-sample hash-grid + render MLP + volume
rendering -> render CNN -> 540x960 image), synthetic scene / random-init weights of the reference's
shapes (no checkpoint is available offline).  Frames are independent, so ranks shard the trajectory
with no data-path collective (weak scaling: K frames per rank); RCCL is only used before the timed
region to broadcast the scene volume / weights / style code from rank 0.

Other BASELINE.json configurations are one command each:
    --config 3                     1920x1080, 40 samples/ray, one GPU
    --config 4   (with --gpus 8)   960x540x24, cam_maxstep=256: all 256 frames of the orbit sharded over the ranks
    --config 5   (with --gpus 8)   3840x2160x40, ONE frame per step rendered tile-parallel (row bands) by all ranks;
                                   the only exchange is the all_reduce of the frame-wide sky mean ("scaling": "strong")
(--bench-mode frames|tile-parallel, --cam-maxstep, --height/--width/--samples give the same control by hand.)

`--gpus N` (N > 1) as a PLAIN command (no WORLD_SIZE in the environment) re-executes itself under
`python -m torch.distributed.run --nproc-per-node N`; the world size must equal --gpus, and with the RCCL backend N GPUs
must be visible -- anything else stops with an error instead of reporting a smaller job.

A plain run sets up, warms up, times the --steps frames and prints the result line: the headline (`value` frames/s,
`ms_per_step`, `dtype`, the per-frame spread) and nothing that needs launches of its own.  --full adds everything else
that is measured outside the timed region (the records listed below); --dump-outputs DIR writes the image of the last
timed frame as DIR/image.npy (float32 [1, 3, H, W]; rank r > 0: image_rank<r>.npy) for comparing two builds output for
output -- the scene, weights and style are seeded, so the inputs are the same in every run with the same arguments.

Output: stdout carries exactly ONE line, the last one, <= 6 KB of JSON (scenedreamer_amd/benchline.py: `compact`): the driver
contract's keys and, with --full, numeric `roofline` (dominant kernel: the field MLP) / `roofline_grid_sampler` /
`roofline_cnn` / `roofline_rvip` / `roofline_sky`, at N=1 `cpu_baseline` (the unmodified reference on the host cores) and
`precision`, and one number each for the unmodified reference loop on the fast shims, configs 3 / 5 on this GPU, the fp32
rung, the no-skip floor (fog weights), colour skipping off, and the per-style one-off costs.  The FULL record (gates,
per-tile errors, per-launch tables, the prose that explains each figure) is written to `bench_detail.json` next to this file
(or $SDN_BENCH_DETAIL).  Everything else that would reach stdout (library chatter, the reference loop's own prints) is sent
to stderr at file-descriptor level.  --only dropin|other prints just that record.
"""
import argparse
import json
import os
import sys
import time

# Host threads for the cpu_baseline leg: both OpenMP runtimes in the process (PyTorch's and the C oracle's) read
# OMP_NUM_THREADS at load time as their MAXIMUM; cpu_baseline() then calibrates the thread count that scales best
# (on the 256-thread GPU host two runtimes spinning 256 threads each made the oracle 10x SLOWER than 8 cores:
# passive waiting + a calibrated count instead of "all of them").
CPU_THREADS_MAX = int(os.environ.get("SDN_CPU_THREADS", min(os.cpu_count() or 1, 128)))
os.environ.setdefault("OMP_NUM_THREADS", str(CPU_THREADS_MAX))
os.environ.setdefault("OMP_WAIT_POLICY", "passive")

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")   # the per-scene world-encoder convolutions: no exhaustive MIOpen search

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0          # MI355X_MICROARCH.md: 8 TB/s HBM3E spec
BYTES_PER_SAMPLE_UNFUSED = 16916  # 16384 gather + 20 coords in + 512 features out
BYTES_PER_SAMPLE_FUSED = 16404    # 16384 gather + 20 coords in


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None,
                    help="timed frames per rank (default 10; --config 4: 256 / N, --config 5: 6)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--full", action="store_true",
                    help="also run every record measured outside the timed region (roofline / per-kernel timing, other apron, "
                         "delivered rate, CPU baseline and precision, floor / style-cost records, other configs, drop-in loop)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the image of the last timed frame to DIR/image.npy (float32)")
    ap.add_argument("--mode", default=os.environ.get("SDN_BENCH_MODE", "auto"), choices=["auto", "fused", "unfused", "dropin"],
                    help="fused / unfused: which per-pixel path this package's frame loop uses; dropin = --only dropin (the UNMODIFIED "
                         "reference generator's inference_givenstyle loop on install_shims(fast=True))")
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--samples", type=int, default=24)
    ap.add_argument("--scene-size", type=int, default=2048)
    ap.add_argument("--apron", default="minimal", choices=["minimal", "reference"],
                    help="field/CNN evaluated on the 4-px apron the image can depend on (the same image), or on the "
                         "reference's full 15-px apron")
    ap.add_argument("--no-overlap", action="store_true", help="do not cast the next frame's rays on a second stream")
    ap.add_argument("--no-extras", action="store_true",
                    help="skip the untimed extra loops (other apron setting, delivered rate): for the very large configs")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--profile", action="store_true",
                    help="for rocprofv3 --kernel-trace runs: only launches of the benchmark configuration (no other-apron / "
                         "delivered-rate loops, no stand-alone kernel timing, no CPU baseline), so that the trace's average "
                         "duration of a kernel is the average over the same launches the roofline record uses")
    ap.add_argument("--cpu-budget-s", type=float, default=25.0)
    ap.add_argument("--cam-maxstep", type=int, default=40, help="poses of the pattern-0 orbit (reference cam_maxstep)")
    ap.add_argument("--pose-stride", type=int, default=2, help="frame f uses pose (stride * f) %% cam_maxstep")
    ap.add_argument("--bench-mode", default="frames", choices=["frames", "tile-parallel"],
                    help="frames: every rank renders whole frames (frame f -> rank f %% N); tile-parallel: every step is ONE "
                         "frame whose row bands are rendered by the N ranks (BASELINE config 5)")
    ap.add_argument("--volume", default="compact", choices=["compact", "int32"],
                    help="scene volume the rays walk: uint8 palette indices + int32 palette (scene.py, 4x smaller, what the "
                         "ranks receive; voxel ids come out identical) or the reference's int32 block ids")
    ap.add_argument("--field", default=None, choices=["one-kernel", "two-kernel"],
                    help="fused path: sample placement + hash-grid lookup + MLP + compositing as ONE kernel (default) or as "
                         "encode_kernel -> feature buffer in HBM -> mlp_kernel (the round-1/2 form, kept for A/B runs)")
    ap.add_argument("--backend", default=os.environ.get("SDN_DIST_BACKEND", "nccl"), choices=["nccl", "gloo"],
                    help="torch.distributed backend for --gpus N > 1: nccl (= RCCL over xGMI, one GPU per rank: the production path) "
                         "or gloo (collectives staged through host memory by scenedreamer_amd.dist; lets N ranks share one GPU, "
                         "which is how this script's multi-rank path is exercised on a one-GPU box -- timings are then meaningless)")
    ap.add_argument("--config", type=int, default=None, choices=[2, 3, 4, 5],
                    help="BASELINE.json configs[i-1]: sets resolution / samples / cam_maxstep / bench mode / steps")
    ap.add_argument("--only", default=None, choices=["dropin", "other"],
                    help="print only that extra record (JSON line): `dropin` = the unmodified reference generator's inference loop on "
                         "the fast shims; `other` = BASELINE configs 3 and 5 on one GPU")
    ap.add_argument("--no-dropin", action="store_true", help="skip the `dropin` record")
    ap.add_argument("--no-other-configs", action="store_true", help="skip the `other_configs` record")
    ap.add_argument("--dropin-frames", type=int, default=12, help="frames of the reference's loop per tile size in the `dropin` record")
    args = ap.parse_args()
    if args.mode == "dropin":
        args.mode, args.only = "auto", "dropin"
    if args.profile:     # the roofline record of the traced launches is what a --profile run is for
        args.full = True
        args.no_extras = args.no_cpu_baseline = args.no_dropin = args.no_other_configs = True
        os.environ.setdefault("SDN_FIELD_GATE", "0")    # no calibration launches in the trace (scenedreamer_amd.renderer.FIELD_GATE)
    if not args.full:
        args.no_extras = args.no_cpu_baseline = args.no_dropin = args.no_other_configs = True
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.config == 3:
        args.height, args.width, args.samples, args.no_extras = 1080, 1920, 40, True
    elif args.config == 4:     # the whole 256-pose orbit, sharded: K = 256 / N frames per rank
        args.cam_maxstep, args.pose_stride = 256, 1
        if args.steps is None:
            args.steps = max(1, 256 // world)
    elif args.config == 5:
        args.height, args.width, args.samples, args.bench_mode, args.no_extras = 2160, 3840, 40, "tile-parallel", True
        if args.steps is None:
            args.steps = 6
    if args.steps is None:
        args.steps = 10
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


def dump_outputs(dirname, arrays, limit):
    """--dump-outputs: every array as DIR/<name>.npy in float32.  One larger than `limit` bytes is thinned to every s-th row
    and column (the smallest s that fits: the same sample in every run) and saved as <name>_stride<s>.npy."""
    os.makedirs(dirname, exist_ok=True)
    for name, t in arrays.items():
        a = t.detach().float().cpu().numpy()
        s = 1
        while a[..., ::s, ::s].nbytes > limit:
            s += 1
        if s > 1:
            a, name = np.ascontiguousarray(a[..., ::s, ::s]), f"{name}_stride{s}"
        np.save(os.path.join(dirname, name + ".npy"), a)


def cpu_baseline(args, weights, scene, z, genc):
    """The reference path as the CPU oracle executes it (reference-literal tiling, fp32): oracle/sdn_oracle.c (pinned bit
    for bit on the reference's own .cu sources compiled for the host, tests/test_ref_pin_cpu.py) for the three native
    ops + oracle/field_ref.py (bit-identical to the imported reference Python on the goldens) for the Python layers.

    Bounded sample of THIS workload: the benchmark scene and resolution, one pose; ray casting and the sky
    pre-pass over the whole padded frame (as the reference does per frame) + 4 of the reference's 128-px tiles (two
    frame corners incl. a ragged edge tile, the centre, one more interior tile); frames/s = 1 / (frame-wide part +
    tile part x tile-rays of the frame / tile-rays sampled).  The thread count is calibrated first (8..128): the one
    that renders a small tile fastest is used and reported as `cores`."""
    from oracle import field_ref as FR
    from oracle import oracle as O
    from scenedreamer_amd import camera, synth
    from scenedreamer_amd.camera import tile_grid
    from scenedreamer_amd.renderer import load_label_lut
    lut = load_label_lut()["lut"]
    vox = scene.voxel_t.cpu().numpy()          # (a compact scene expands to the reference's int32 ids here)
    # z / global_enc: the per-trajectory codes (computed once per style / scene, not per frame) as the renderer holds them
    all_poses = camera.eval_camera_poses(scene, maxstep=40)
    pose = all_poses[8]
    p = (pose[0].numpy(), pose[1].numpy(), pose[2].numpy(), pose[3])
    hw = (args.height, args.width)

    def set_threads(n):
        torch.set_num_threads(n)
        O.set_num_threads(n)

    # ---- calibration: one small reference tile per candidate thread count --------------------------------------
    cal = {}
    for n in [c for c in (8, 16, 32, 64, 128) if c <= CPU_THREADS_MAX] or [CPU_THREADS_MAX]:
        set_threads(n)
        t0 = time.time()
        FR.render_frame_tiled(weights, lut, vox, p, (66, 66), args.samples, z, genc)
        cal[n] = time.time() - t0
    cores = min(cal, key=cal.get)
    set_threads(cores)
    # ---- the sample -----------------------------------------------------------------------------------------------
    tiles_all, nh, nw = tile_grid([hw[0] + 30, hw[1] + 30], 30)
    frame_tile_rays = sum((a[1] - a[0]) * (a[3] - a[2]) for a in tiles_all)
    picks = list(dict.fromkeys([(0, 0), (nh - 1, nw - 1), (nh // 2, nw // 2), (min(1, nh - 1), max(0, nw - 2))]))
    kind, why_port = "port", None
    try:    # the UNMODIFIED reference (staged Python tree + its native sources compiled for the host), when it travelled here
        t_frame, t_tiles, got = _reference_tiles(weights, scene, vox, pose, hw, args.samples, z, genc, picks)
        kind = "reference"
    except Exception as e:  # noqa: BLE001 -- the staged reference is optional: the port (pinned on it bit for bit) is the fallback
        why_port = f"{type(e).__name__}: {e}"
        t0 = time.time()
        FR.render_frame_tiled(weights, lut, vox, p, hw, args.samples, z, genc, tiles=[])       # frame-wide part only
        t_frame = time.time() - t0
        t0 = time.time()
        got = FR.render_frame_tiled(weights, lut, vox, p, hw, args.samples, z, genc, tiles=picks)
        t_tiles = time.time() - t0 - t_frame
    sampled = sum((im.shape[2] + 30) * (im.shape[3] + 30) for (_, _, im) in got.values())
    fps_a = 1.0 / (t_frame + t_tiles * frame_tile_rays / sampled)
    cpu_baseline.tiles, cpu_baseline.pose = got, pose       # the CPU pixels: main() measures the GPU path's error on them
    # a second pose (the work per frame is pose dependent: more ground -> more samples the MLP is evaluated on): two tiles of it
    pose_b = all_poses[26]
    picks_b = picks[1:3] if len(picks) >= 3 else picks[:1]
    per_pose = {"8": fps_a}
    cpu_baseline.more = []
    try:
        if kind == "reference":
            tf_b, tt_b, got_b = _reference_tiles(weights, scene, vox, pose_b, hw, args.samples, z, genc, picks_b)
        else:
            pb = (pose_b[0].numpy(), pose_b[1].numpy(), pose_b[2].numpy(), pose_b[3])
            t0 = time.time()
            FR.render_frame_tiled(weights, lut, vox, pb, hw, args.samples, z, genc, tiles=[])
            tf_b = time.time() - t0
            t0 = time.time()
            got_b = FR.render_frame_tiled(weights, lut, vox, pb, hw, args.samples, z, genc, tiles=picks_b)
            tt_b = time.time() - t0 - tf_b
        sampled_b = sum((im.shape[2] + 30) * (im.shape[3] + 30) for (_, _, im) in got_b.values())
        per_pose["26"] = 1.0 / (tf_b + tt_b * frame_tile_rays / sampled_b)
        cpu_baseline.more = [(pose_b, got_b)]
        t_frame, t_tiles, sampled = t_frame + tf_b, t_tiles + tt_b, sampled + sampled_b
    except Exception as e:  # noqa: BLE001 -- the second pose is extra evidence: the first one stands on its own
        per_pose["26"] = f"not measured ({type(e).__name__}: {e})"
    rates = [v for v in per_pose.values() if isinstance(v, float)]
    fps = len(rates) / sum(1.0 / v for v in rates)          # frames / total time over the poses
    what = ("the UNMODIFIED reference: imaginaire Generator._forward_perpix / _forward_global / sky_net from the staged Python tree "
            "(oracle/_ref/pytree.zip) on its own voxlib / gridencoder sources compiled for the host (oracle/_ref/nofma/*.so); the "
            "per-frame body of inference_givenstyle (scenedreamer.py:573-628) is restated around them because the method hard-codes "
            "device 'cuda'" if kind == "reference" else
            "oracle/sdn_oracle.c == the reference's .cu sources compiled for the host (bit for bit) + oracle/field_ref.py == the "
            "reference's Python layers on the goldens" + (f"; the staged reference itself was not usable here ({why_port})" if why_port else ""))
    return {"value": fps, "unit": "frames/s", "cores": cores, "kind": kind,
            "sample": f"{args.width}x{args.height}, {args.samples} samples/ray, scene_size {args.scene_size}: ray casting + sky "
                      f"pre-pass of the whole padded frame + {len(picks)} (pose 8) and {len(picks_b)} (pose 26 of the 40-pose orbit) of the "
                      f"reference's {nh * nw} tiles per frame: {t_frame:.2f} s frame-wide + {t_tiles:.2f} s for {sampled} tile-rays in all, each "
                      f"pose extrapolated to its {frame_tile_rays} tile-rays; value = 2 frames / the two extrapolated frame times",
            "sample_short": f"whole-frame ray cast + sky + {len(picks)}+{len(picks_b)} of {nh * nw} tiles/frame, poses 8, 26; extrapolated to a frame",
            "frames_per_s_by_pose": per_pose,
            "thread_calibration_s": {str(k): round(v, 3) for k, v in cal.items()}, "host_cpus": os.cpu_count(),
            "implementation": what}


def _reference_tiles(weights, scene, vox, pose, hw, ns, z, genc, picks, pad=30, tile=128):
    """(seconds for the frame-wide part, seconds for the picked tiles, {(ih, iw): (row0, col0, image tile)}) with the unmodified
    reference on CPU tensors: oracle/ref_harness.install("ref") puts the reference's own native sources (compiled for the
    host) under the unmodified imaginaire Generator.  The statements below are the per-frame body of inference_givenstyle
    (scenedreamer.py:573-628) with its calls unchanged."""
    from oracle import ref_harness as RH
    from oracle import ref_native
    if not (RH.available() and ref_native.available()):
        raise RuntimeError("oracle/_ref (staged reference) is not present")
    RH.install("ref")
    import voxlib
    from scenedreamer_amd.synth import Scene
    sc = Scene()          # the voxel handle the generator reads (CPU tensors; int32 volume)
    sc.voxel_t, sc.heightmap = torch.from_numpy(vox), scene.heightmap
    sc.current_height_map, sc.current_semantic_map = scene.current_height_map.cpu(), scene.current_semantic_map.cpu()
    sc.trans_mat, sc.sample_size = scene.trans_mat, scene.sample_size
    G, _ = RH.build_generator(weights, sc)
    RH.set_inference_overrides(G, ns, list(hw), pad)
    zt, gt = torch.as_tensor(z, dtype=torch.float32).reshape(1, -1), torch.as_tensor(genc, dtype=torch.float32).reshape(1, -1)
    cam_ori, cam_dir, cam_up, cam_f = pose
    got = {}
    with torch.no_grad():
        t0 = time.time()
        f = cam_f * (hw[1] - 1)
        c = [(G.cam_res[0] - 1) / 2, (G.cam_res[1] - 1) / 2]
        vid, d2, rd = voxlib.ray_voxel_intersection_perspective(G.voxel.voxel_t, cam_ori, cam_dir, cam_up, f, c, G.cam_res, G.num_blocks_early_stop)
        vid, d2, rd = vid.unsqueeze(0), d2.unsqueeze(0), rd.unsqueeze(0)
        sky_in = voxlib.positional_encoding(rd.expand(-1, -1, -1, 1, -1).contiguous(), G.pe_params_sky[0], -1, G.pe_params_sky[1])
        G.sky_avg = torch.mean(G.sky_net(sky_in, zt), dim=[1, 2], keepdim=True)
        t_frame = time.time() - t0
        t0 = time.time()
        for ih, iw in picks:
            h0, h1 = ih * tile, min(ih * tile + tile + pad, G.cam_res[0])
            w0, w1 = iw * tile, min(iw * tile + tile + pad, G.cam_res[1])
            out = G._forward_perpix(G.blk_feats, vid[:, h0:h1, w0:w1], d2[:, :, h0:h1, w0:w1].clone(), rd[:, h0:h1, w0:w1],
                                    torch.as_tensor(cam_ori, dtype=torch.float32).reshape(1, 3), zt, gt)
            img, _ = G._forward_global(out[0], zt)
            got[(ih, iw)] = (h0, w0, img[:, :, pad // 2:-pad // 2, pad // 2:-pad // 2])
        t_tiles = time.time() - t0
    return t_frame, t_tiles, got


def dropin_record(args, weights, scene, dev, oracle_tiles=None):
    """The UNMODIFIED reference generator -- imaginaire.generators.scenedreamer.Generator.inference_givenstyle, its own frame loop
    (scenedreamer.py:479-632) -- on `scenedreamer_amd.install_shims(fast=True)`: voxlib / gridencoder served by the HIP ops, its
    LightningMLP / SKYMLP / RenderCNN classes and its _forward_perpix / _forward_global methods bound to the fused kernels from
    outside (scenedreamer_amd/dropin.py).  Needs the reference's Python tree at run time: /root/reference in the build container,
    the staged archive oracle/_ref/pytree.zip (unchanged files, oracle/build_ref.stage_pytree) on the GPU box; the loader
    (oracle/ref_harness) only locates / unpacks it and supplies the cv2 / imageio stand-ins this image lacks -- nothing of the CPU
    oracle runs here.  Frames/s are taken between the completion times of the loop's own frames (after its device -> host copy
    and uint8 conversion; PNG / MP4 encoders are no-ops: host-side file encoding is excluded, as for the headline)."""
    import tempfile
    try:
        from oracle import ref_harness as RH
    except ImportError as e:
        return {"skipped": f"oracle/ref_harness not importable: {e}"}
    if not RH.available():
        return {"skipped": "the reference's Python tree is not on this machine (neither /root/reference nor oracle/_ref/pytree.zip)"}
    from scenedreamer_amd import dropin, synth
    RH.install("hip-fast")
    import cv2
    import imageio
    stamps = []

    class _Writer:
        def append_data(self, rgb):
            stamps.append(time.perf_counter())

        def close(self):
            pass

    cv2.__dict__["imwrite"] = lambda path, img, params=None: True
    cv2.__dict__["IMWRITE_PNG_COMPRESSION"] = 16
    imageio.__dict__["get_writer"] = lambda path, fps=10: _Writer()
    sc = synth.Scene()
    sc.voxel_t = scene.voxel_t.to(dev)                    # the int32 volume the reference's generator holds (pcg_gen.py:173)
    sc.heightmap, sc.trans_mat, sc.sample_size = scene.heightmap, scene.trans_mat, scene.sample_size
    sc.current_height_map, sc.current_semantic_map = scene.current_height_map.to(dev), scene.current_semantic_map.to(dev)
    G, _ = RH.build_generator(weights, sc)
    G = G.to(dev).eval()
    for prm in G.parameters():
        prm.requires_grad = False                          # inference.py:63-64
    v = G.voxel
    v.voxel_t, v.current_height_map, v.current_semantic_map = sc.voxel_t, sc.current_height_map, sc.current_semantic_map
    style = torch.from_numpy(np.asarray(synth.make_style(8888))).to(dev)
    hw = [args.height, args.width]
    out = {"what": "imaginaire.generators.scenedreamer.Generator.inference_givenstyle, unmodified, on install_shims(fast=True)",
           "workload": f"{args.width}x{args.height}, num_samples={args.samples}, scene_size={args.scene_size}, camera_mode 0, "
                       f"cam_maxstep={args.dropin_frames}", "runs": [],
           "timing": "frames/s = (frames - 1) / (completion of the last - completion of the first frame), each completion taken "
                     "when the loop hands the frame to its video writer (after its own D2H copy + uint8 conversion); the first "
                     "call with 3 frames is the warm-up; PNG / MP4 encoders are no-ops"}
    with tempfile.TemporaryDirectory() as tmp, torch.no_grad():
        for tile, coalesce in ((128, True), (128, False), (1024, True)):
            dropin.binding(G).coalesce = coalesce
            kw = dict(camera_mode=0, num_samples=args.samples, tile_size=tile, resolution_hw=hw, cam_ang=72)
            G.inference_givenstyle(style, os.path.join(tmp, f"warm{tile}"), cam_maxstep=3, **kw)
            torch.cuda.synchronize()
            b = dropin.binding(G)
            before = {k: v for k, v in b.stats.items() if k != "why"}
            del stamps[:]
            t0 = time.perf_counter()
            G.inference_givenstyle(style, os.path.join(tmp, f"run{tile}"), cam_maxstep=args.dropin_frames, **kw)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            n = len(stamps)
            fps = (n - 1) / (stamps[-1] - stamps[0]) if n > 1 else None
            tiles = ((hw[0] + tile - 1) // tile) * ((hw[1] + tile - 1) // tile)
            out["runs"].append({"tile_size": tile, "tiles_per_frame": tiles, "frame_evaluated_once_for_its_tiles": bool(coalesce and tiles > 1),
                                "frames": n, "frames_per_s": fps,
                                "ms_per_frame": 1000.0 / fps if fps else None, "whole_call_s": t1 - t0,
                                "note": (("the reference's default tiling (inference.py passes no tile_size)" +
                                          ("; the binding evaluates the whole frame when its first tile arrives and serves the 40 tiles as views"
                                           if coalesce else "; every tile evaluated by its own field / CNN launches (binding.coalesce = False)"))
                                         if tile == 128 else
                                         "tile_size >= frame -- an argument of the unmodified method: one _forward_perpix / "
                                         "_forward_global call per frame"),
                                "calls": {k: v - before[k] for k, v in b.stats.items() if k != "why"}, "reference_path_reasons": dict(b.stats["why"])})
        # ---- the loop's OWN pixels (float, before its uint8 conversion) of one frame -- frame 8 of the 40-step orbit, default tiling,
        #      the frame evaluated once for its 40 tiles -- against this package's renderer ON THE CAMERA THE LOOP USED: the generator's
        #      voxel handle computes the poses on the GPU (its trans_mat is a buffer of the module: camctl.py:9-60), an ulp away from the
        #      host poses the CPU baseline rendered, and the random-init field is chaotic in such an ulp at ~20 rays per frame
        #      (profiles/r05_dropin_vs_renderer_camera_ulp.txt) -- so the CPU tiles of cpu_baseline are not comparable pixel for pixel.
        #      The renderer against the CPU oracle: `precision.max_abs_err`; this loop against the oracle on its own camera:
        #      tests/test_dropin_gpu.py::test_unmodified_loop_at_the_headline_config_against_oracle_tiles (3.8e-4).
        try:
            import sys as _sys
            from scenedreamer_amd.renderer import Renderer
            b = dropin.binding(G)
            b.coalesce = True
            got, cams = [], []
            b.on_frame = lambda fr: got.append(fr["img"].clone() if len(got) == 8 else None)
            vox_mod = _sys.modules["imaginaire.generators.scenedreamer"].voxlib
            rvip = vox_mod.ray_voxel_intersection_perspective

            def rec_rvip(voxel_t, cam_ori, cam_dir, cam_up, cam_f, cam_c, img_dims, max_samples):
                cams.append((torch.as_tensor(cam_ori).detach().cpu().float(), torch.as_tensor(cam_dir).detach().cpu().float(),
                             torch.as_tensor(cam_up).detach().cpu().float(), float(cam_f) / (hw[1] - 1)))
                return rvip(voxel_t, cam_ori, cam_dir, cam_up, cam_f, cam_c, img_dims, max_samples)
            vox_mod.ray_voxel_intersection_perspective = rec_rvip
            try:
                G.inference_givenstyle(style, os.path.join(tmp, "err"), cam_maxstep=40, camera_mode=0, num_samples=args.samples, tile_size=128,
                                       resolution_hw=hw, cam_ang=72)
            finally:
                b.on_frame = None
                vox_mod.ray_voxel_intersection_perspective = rvip
            if len(got) == 40 and got[8] is not None and len(cams) == 40:
                Rc = Renderer(weights, sc, dev)
                Rc.set_style(synth.make_style(8888))
                mine = Rc.render_frame(cams[8], tuple(hw), args.samples, mode="fused", apron="reference")
                c = (got[8].shape[2] - hw[0]) // 2
                e = (got[8][:, :, c:c + hw[0], c:c + hw[1]] - mine).abs()
                out["max_abs_diff_vs_renderer"] = float(e.max())
                out["max_abs_diff_where"] = ("whole frame 8 of the 40-step orbit: the unmodified loop's float image (tile_size 128, frame evaluated once) vs "
                                             "Renderer.render_frame on the camera the loop's ray caster received; the loop's sky MLP runs 3-term where the "
                                             "renderer's gate chose f16 + fp6 (<= 1e-4 on sky_c); loop vs CPU oracle: tests/test_dropin_gpu.py (3.8e-4, bound 1e-3)")
                del Rc
        except Exception as ex:  # noqa: BLE001 -- an extra figure must not cost the record
            out["max_abs_diff_vs_renderer"] = f"not measured ({type(ex).__name__}: {ex})"
    out["cnn_gate"] = b.B.cnn_calibration
    try:
        from scenedreamer_amd import modules as _modules
        out["sky_gate"] = getattr(_modules._backend(G.sky_net), "sky_gate", None)
    except Exception:  # noqa: BLE001
        out["sky_gate"] = None
    del G
    torch.cuda.empty_cache()
    return out


def other_configs(args, R, weights, scene, poses, dev):
    """BASELINE configs 3 (1920x1080x40) and 5 (3840x2160x40; on ONE GPU: the tile-parallel path with a single band) on the
    benchmark scene: a few frames each, after the headline's timed region, + the max abs error of one tile of the
    reference's tile grid against the CPU oracle (reference-literal evaluation of that tile)."""
    from oracle import field_ref as FR
    from scenedreamer_amd import dist as sdist
    from scenedreamer_amd.camera import tile_grid
    from scenedreamer_amd.renderer import load_label_lut
    lut = load_label_lut()["lut"]
    vox = scene.voxel_t.cpu().numpy()
    z, genc = R.z.cpu().numpy(), R.global_enc.cpu().numpy()
    torch.set_num_threads(min(CPU_THREADS_MAX, 64))
    recs = []
    for cfg, hw, ns, frames in ((3, (1080, 1920), 40, 3), (5, (2160, 3840), 40, 2)):
        sel = [poses[(7 * k + 3) % len(poses)] for k in range(frames + 1)]
        probe = {}
        torch.cuda.synchronize()
        if cfg == 3:
            it = R.render_frames(sel, hw, ns, mode="fused", probe=probe)
            imgs = []
            for k, im in enumerate(it):
                if k == 0:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                imgs.append(im if k == frames else None)
            torch.cuda.synchronize()
            ms = 1000.0 * (time.perf_counter() - t0) / frames
            last = imgs[-1]
            field_ms = float(np.mean([a.elapsed_time(b) for a, b in probe["mlp_kernel"][1:]])) if probe.get("mlp_kernel") else None
            B, hit, ev = R.field_work(sel[1:], hw, ns, "minimal")
            flop = ev["evaluated_samples"] * (754176 - 294912) + ev.get("colour_samples", ev["evaluated_samples"]) * 294912
            field_frac = (flop / (field_ms * 1e-3) / 1e12 / 2500.0) if field_ms else None
            how = "render_frames (pipelined trajectory loop, minimal apron), 1 warm-up frame"
        else:
            sdist.render_frame_tile_parallel(R, sel[0], hw, ns, mode="fused")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(frames):
                last = sdist.render_frame_tile_parallel(R, sel[k + 1], hw, ns, mode="fused")
            torch.cuda.synchronize()
            ms = 1000.0 * (time.perf_counter() - t0) / frames
            field_ms = field_frac = None
            how = "dist.render_frame_tile_parallel with ONE band (the 8-GPU path of config 5 on one GPU), reference apron, 1 warm-up frame"
        pose = sel[-1]
        tiles_all, nh, nw = tile_grid([hw[0] + 30, hw[1] + 30], 30)
        pick = (nh // 2, nw // 2)
        t_cpu = time.time()
        ref = FR.render_frame_tiled(weights, lut, vox, (pose[0].numpy(), pose[1].numpy(), pose[2].numpy(), pose[3]), hw, ns, z, genc,
                                    tiles=[pick])
        r0, c0, tile = ref[pick]
        err = float((last[:, :, r0:r0 + tile.shape[2], c0:c0 + tile.shape[3]].cpu() - tile).abs().max())
        recs.append({"baseline_config": cfg, "workload": f"{hw[1]}x{hw[0]}, num_samples={ns}, scene_size={args.scene_size}", "frames": frames,
                     "ms_per_frame": ms, "frames_per_s": 1000.0 / ms, "field_kernel_ms": field_ms, "field_frac": field_frac, "how": how,
                     "max_abs_err_tile": err, "tile": f"{pick} of the reference's {nh}x{nw} tile grid vs the CPU oracle "
                                                      f"({time.time() - t_cpu:.1f} s of CPU incl. the frame-wide ray casting / sky pre-pass)",
                     "precision_gates": {"cnn": R.cnn_calibration, "field": {k: v for k, v in (R.field_gate or {}).items() if k != "measurements"}}})
    return recs


def early_termination_record(args, R, weights, scene, poses, hw, mode):
    """The north star's "wavefront ballots for early termination" measured: frames/s of the trajectory loop with the default
    term_eps and with 0, on the benchmark weights (random-init: densities are low, few rays become opaque) and on an
    opaque-surface variant of them (density-head bias + 4000: every hit ray is opaque after its first samples -- what a
    trained checkpoint's terrain looks like to the ray), outside the timed region."""
    from scenedreamer_amd import fused
    from scenedreamer_amd.renderer import Renderer
    default = float(fused.TERM_EPS_DEFAULT)
    sel = [poses[(2 * k) % len(poses)] for k in range(8)]

    def ms_per_frame(Rx, eps):
        saved = getattr(Rx, "term_eps", None)
        Rx.term_eps = eps
        try:
            for _ in Rx.render_frames(sel[:2], hw, args.samples, mode=mode, apron=args.apron):
                pass
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in Rx.render_frames(sel, hw, args.samples, mode=mode, apron=args.apron):
                pass
            torch.cuda.synchronize()
            ms = 1000.0 * (time.perf_counter() - t0) / len(sel)
            _, _, ev = Rx.field_work(sel[:3], hw, args.samples, args.apron)
        finally:
            Rx.term_eps = saved
        return ms, ev
    rec = {"default_eps": default, "bound_on_net_out_change": 2 * default, "frames": len(sel)}
    opaque = dict(weights)
    opaque["render_net.fc_sigma.bias"] = np.asarray(weights["render_net.fc_sigma.bias"]) + 4000.0
    Ro = Renderer(opaque, scene, R.dev)
    Ro.set_style_code(R.z)
    Ro.field_gate, Ro.cnn_calibration = {"path": "fused", "max_abs_err_vs_fp32": 0.0}, dict(R.cnn_calibration or {"terms3x3": 1, "pixels": 1 << 30,
                                                                                                   "max_abs_diff_1term_vs_3term": 0.0, "bound": 0.0})
    for name, Rx in (("benchmark_weights", R), ("opaque_surface_weights", Ro)):
        on, ev_on = ms_per_frame(Rx, default)
        off, _ = ms_per_frame(Rx, 0.0)
        rec[name] = {"ms_per_frame_term_on": on, "ms_per_frame_term_off": off, "speedup": off / on,
                     "passes_skipped_frac": ev_on["passes_skipped_by_termination"] / max(1.0, ev_on["passes_of_visited_groups"])}
    del Ro
    return rec


def _trajectory_ms(Rx, sel, hw, ns, mode, apron, warm=2):
    """ms per frame of the pipelined trajectory loop over `sel` (after `warm` untimed frames of the same loop)."""
    for _ in Rx.render_frames(sel[:warm], hw, ns, mode=mode, apron=apron):
        pass
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in Rx.render_frames(sel, hw, ns, mode=mode, apron=apron):
        pass
    torch.cuda.synchronize()
    return 1000.0 * (time.perf_counter() - t0) / len(sel)


def floor_record(args, R, weights, scene, poses, hw, mode):
    """The regime in which the field kernel can remove NOTHING: `synth.fog_weights` (density 6 +- 0.65 at
    every sample: no ray terminates, no sample has weight zero, all 24 colours of every hit ray are composited) on the DENSEST
    pose of the orbit (most rays that hit), 8 frames of the pipelined loop.  The record also carries the style's calibration
    (image error of the fused path against the fp32 op sequence on these weights) and the kernel's own pass counters, which
    must show 0 terminated / 0 colour-skipped passes."""
    from scenedreamer_amd import synth
    from scenedreamer_amd.renderer import Renderer
    with torch.no_grad():
        hits = [float((R.cast_rays(p, hw)[0][..., 0] != 0).float().mean()) for p in poses]
    dense = int(np.argmax(hits))
    Rf = Renderer(synth.fog_weights(weights), scene, R.dev)
    Rf.set_style_code(R.z)
    sel = [poses[dense]] * 8
    ms = _trajectory_ms(Rf, sel, hw, args.samples, mode, args.apron)
    _, _, ev = Rf.field_work(sel[:1], hw, args.samples, args.apron)
    ms_bench = _trajectory_ms(R, sel, hw, args.samples, mode, args.apron)      # the benchmark weights on the same pose
    rec = {"frames_per_s": 1000.0 / ms, "ms_per_frame": ms, "pose": dense, "ray_hit_fraction": hits[dense],
           "benchmark_weights_same_pose_frames_per_s": 1000.0 / ms_bench,
           "passes_skipped_by_termination": ev["passes_skipped_by_termination"],
           "colour_branch_skipped_fraction": 1.0 - ev["colour_samples"] / max(1.0, ev["evaluated_samples"]),
           "evaluated_samples": ev["evaluated_samples"],
           "max_abs_err_vs_fp32": (Rf.field_gate or {}).get("image_err_vs_fp32"), "net_out_err_vs_fp32": (Rf.field_gate or {}).get("max_abs_err_vs_fp32"),
           "cnn_terms3x3": (Rf.cnn_calibration or {}).get("terms3x3"), "path": (Rf.field_gate or {}).get("path"),
           "weights": "synth.fog_weights: fc_sigma x 0.03 + 6 (sigma > 0 everywhere, final transmittance > term_eps)"}
    del Rf
    return rec


def style_cost_record(args, weights, scene, poses, hw, mode, dev):
    """What a NEW style costs before and with its first frames, in a warm process: the reference calls
    style_net once per inference_givenstyle and ships 40 frames per call (scenedreamer.py:570, configs/scenedreamer_inference.yaml).
    trajectory40: set_style + the 40 poses of the orbit through render_frames, everything included (fold, weight packing,
    calibration, frames), wall clock to the completion of the last frame; first_frame_ms: to the completion of frame 0.
    A second fresh style gives the components: style_setup_ms (style MLP + fold + pack of field / sky / CNN weights),
    calibration_ms (calibrate_style as the trajectory loop calls it)."""
    from scenedreamer_amd import fused, synth
    from scenedreamer_amd.renderer import Renderer
    R2 = Renderer(weights, scene, dev)
    fused.prepare_scene(R2)                 # per SCENE (collapsed table), not per style
    R2.set_style(synth.make_style(8888))    # (warm-up style: this renderer's buffers, streams, CNN planes)
    for _ in R2.render_frames(poses[:2], hw, args.samples, mode=mode, apron=args.apron):      # buffers / streams of this renderer
        pass
    torch.cuda.synchronize()
    orbit = [poses[k % len(poses)] for k in range(40)]
    t0 = time.perf_counter()
    R2.set_style(synth.make_style(8888))     # (the benchmark's style: the field's work is content dependent; everything per-style is redone)
    first = None
    for k, im in enumerate(R2.render_frames(orbit, hw, args.samples, mode=mode, apron=args.apron)):
        if k == 0:
            torch.cuda.synchronize()
            first = time.perf_counter() - t0
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    rec = {"trajectory40_frames_per_s": len(orbit) / total, "trajectory40_s": total, "first_frame_ms": 1000.0 * first,
           "steady_frames_per_s_after_first": (len(orbit) - 1) / (total - first),
           "adopted": {"cnn": (R2.cnn_calibration or {}).get("terms3x3"), "path": (R2.field_gate or {}).get("path"),
                       "calibration_poses": ((R2.field_gate or {}).get("measurements") or {}).get("poses", 1)}}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    R2.set_style(synth.make_style(8888))
    fused.prepare_style(R2)
    fused.prepare_sky(R2)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    R2.calibrate_style(orbit[0], hw, args.samples, more_poses=orbit[20:21])
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    rec.update(style_setup_ms=1000.0 * (t1 - t0), calibration_ms=1000.0 * (t2 - t1))
    del R2
    return rec


def rvip_roofline(R, poses, hw):
    """SURVEY 8(d) record of the ray marcher: algorithmic bytes = 4 B x DDA steps of the reference's cell-by-cell loop
    (ray_voxel_intersection.cu:115-229; counted by the measurement build of the same kernel, sdn_rvip_debug_counts, WITHOUT the
    occupancy grid) + 84 B per ray of output, over the kernel's duration (HIP events on the launch stream, product kernel with
    empty-space skipping), against the HBM peak.  Latency / divergence bound: the fraction is small by construction."""
    from scenedreamer_amd import ops
    from scenedreamer_amd.camera import frame_intrinsics
    sel = list(poses)[:6]
    steps = reads = jumps = rays = 0
    ms = []
    with torch.no_grad():
        for pose in sel:
            f, c, cam_res = frame_intrinsics(pose[3], hw, R.pad)
            ref = ops.rvip_step_counts(R.volume, pose[0], pose[1], pose[2], f, c, cam_res, R.M, accelerate=False, palette=R.palette)
            got = ops.rvip_step_counts(R.volume, pose[0], pose[1], pose[2], f, c, cam_res, R.M, accelerate=True, palette=R.palette)
            steps += ref["iterations"]; reads += got["volume_reads"]; jumps += got["block_jumps"]; rays += ref["rays"]
            R.cast_rays(pose, hw)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            R.cast_rays(pose, hw)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
    k = len(sel)
    alg = (4.0 * steps + 84.0 * rays) / k
    t = float(np.mean(ms))
    return {"bound": "hbm", "kernel": "rvip_kernel (exact DDA + exact empty-space skipping" + (", uint8 volume)" if R.palette is not None else ", int32 volume)"),
            "achieved": alg / (t * 1e-3) / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": alg / (t * 1e-3) / 1e9 / HBM_PEAK_GBPS,
            "traffic": None, "avg_launch_ms": t, "rays_per_launch": rays / k, "reference_dda_steps_per_launch": steps / k,
            "reference_dda_steps_per_ray": steps / max(1, rays), "algorithmic_bytes_per_launch": alg,
            "volume_reads_per_launch_this_kernel": reads / k, "empty_block_jumps_per_launch": jumps / k,
            "bytes_per_volume_read": 1 if R.palette is not None else 4,
            "timing": f"HIP events around a stand-alone launch per pose ({k} poses of the timed region), outside the timed region",
            "note": "algorithmic = 4 B x the reference's DDA steps + 84 B/ray (SURVEY 8d); this kernel skips empty 8x16x16 blocks and, on "
                    "the compact volume, reads 1 B per visited cell, so it moves far fewer bytes than that; the walk is latency / "
                    "divergence bound, not bandwidth bound"}


def sustained_ceiling(roof):
    """roofline.peak_sustained: what the part sustains on the field MLP's own instruction mix, measured IN THIS RUN by the
    micro-kernel tools/mlp_shape_ubench (one 256 -> 256 layer in the kernel's shape: 4 waves / CU, 32 samples per wave,
    v_mfma_f32_32x32x16_f16 3-term split on random f16 operands, fragments from the LDS ring): with ONLY the MFMAs and their
    fragment reads in the loop it is the ceiling of any schedule of this arithmetic (the part lowers its clock under this load);
    `frac_of_sustained` divides the kernel's achieved rate by that ceiling scaled to the kernel's instruction mix."""
    import subprocess
    exe = os.path.join(ROOT, "tools", "mlp_shape_ubench")
    if not os.path.exists(exe):
        roof["peak_sustained"] = {"skipped": "tools/mlp_shape_ubench is not built (python -c 'import __graft_entry__ as g; g.build()')"}
        return
    r = subprocess.run([exe, "--ceiling"], capture_output=True, text=True, timeout=120)
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("{")), None)
    if r.returncode != 0 or line is None:
        roof["peak_sustained"] = {"skipped": f"micro-kernel failed (rc {r.returncode}): {r.stderr[-300:]}"}
        return
    u = json.loads(line)
    issued = roof.get("issued_over_algorithmic") or 3.0
    # the higher of the two loops: with ONLY MFMAs + fragment reads the part draws more power and clocks lower (1.4 - 1.5 GHz) than with
    # the activation work interleaved (2.0 - 2.2 GHz), so on some boxes the complete layer loop is the faster one
    ceil3 = max(u["mfma_and_fragment_reads_only"]["tflops_algorithmic_3term"], u["whole_layer_loop"]["tflops_algorithmic_3term"])
    mix = ceil3 * 3.0 / issued
    roof["peak_sustained"] = {"value": mix, "unit": "TFLOP/s algorithmic", "three_term_layer": ceil3, "micro_kernel": u,
                              "note": "ceiling for THIS kernel's mix = 3-term ceiling x 3 / issued_over_algorithmic (the fp6-corrected colour "
                                      "layers issue fewer MFMA slots per product); nominal peak 2500 TFLOP/s is what `frac` divides by"}
    roof["frac_of_sustained"] = roof["achieved"] / mix


def _single_kernel(R):
    from scenedreamer_amd import fused
    return fused.single_kernel(R) and fused.precision_profile(R)[0] != 2


def fused_eps(R):
    from scenedreamer_amd import fused
    return fused.precision_profile(R)[1]


def self_launch(args):
    """`python bench.py --gpus N` without a launcher: become `python -m torch.distributed.run --nproc-per-node N bench.py ...`."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.stderr.write(f"[bench] --gpus {args.gpus} without WORLD_SIZE: re-executing under torch.distributed.run on port {port}\n")
    sys.stderr.flush()
    os.execv(sys.executable, cmd)


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)
    from scenedreamer_amd import benchline
    guard = benchline.StdoutGuard()      # from here on stdout belongs to the one JSON line; everything else lands on stderr
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch with --nproc-per-node {args.gpus} (or run "
                         f"`python bench.py --gpus {args.gpus}` without a launcher)")
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    assert torch.cuda.is_available(), "bench.py needs an MI355X"
    ndev = torch.cuda.device_count()
    if world > ndev and args.backend == "nccl":
        raise SystemExit(f"rank {rank}: {world} ranks but only {ndev} GPU(s) visible (RCCL needs one GPU per rank; --backend gloo shares GPUs)")
    torch.cuda.set_device(local % ndev)
    dev = torch.device("cuda", local % ndev)
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group(args.backend, init_method="env://")

    from scenedreamer_amd import camera, capi, synth
    from scenedreamer_amd import dist as sdist
    from scenedreamer_amd.renderer import Renderer
    capi.lib()  # hard requirement: no fallback

    mode = args.mode
    if mode == "auto":
        try:
            from scenedreamer_amd import fused  # noqa: F401
            mode = "fused"
        except ImportError:
            mode = "unfused"

    # ---- scene / weights / style: built on rank 0, broadcast over RCCL ----------------------------
    t_setup = time.time()
    scene = synth.make_scene(args.scene_size, 3407, device=dev) if rank == 0 or world == 1 else None
    weights = synth.make_weights(0) if rank == 0 or world == 1 else None
    style = synth.make_style(8888) if rank == 0 or world == 1 else None
    bstats = {}
    if world > 1:
        t_b = time.time()
        scene, weights, style = sdist.broadcast_state(scene, weights, style, dev, src=0, stats=bstats,
                                                      compact=args.volume == "compact")
        torch.cuda.synchronize()
        bstats["broadcast_s"] = time.time() - t_b
    elif args.volume == "compact":
        from scenedreamer_amd import scene as scene_mod
        scene = scene_mod.to_compact(scene)
    R = Renderer(weights, scene, dev)
    R.set_style(style)
    if args.field is not None:
        R.field_single_kernel = args.field == "one-kernel"
    maxstep = args.cam_maxstep
    poses = camera.eval_camera_poses(scene, maxstep=maxstep)
    # global frame f uses pose (stride * f) % maxstep (default: every 2nd pose of the 40-pose orbit)
    order = [(args.pose_stride * i) % maxstep for i in range(maxstep)]
    tile_parallel = args.bench_mode == "tile-parallel"
    if tile_parallel:
        # strong scaling inside a frame: step k = global frame k, every rank renders its row band of it
        frame_pose = lambda k: poses[order[k % len(order)]]
    else:
        # weak scaling: step k renders global frames k*world .. k*world+world-1, rank r takes frame k*world + r
        frame_pose = lambda k: poses[order[sdist.shard_frames(range(k * world, (k + 1) * world), rank, world)[0] % len(order)]]
    hw = (args.height, args.width)
    setup_s = time.time() - t_setup
    if args.only:       # just one of the extra records (one GPU)
        assert world == 1, "--only runs on one GPU"
        if args.only == "dropin":
            guard.emit(json.dumps({"dropin": dropin_record(args, weights, scene, dev)}))
        else:
            R.render_frame(poses[0], hw, args.samples, mode=mode)      # (the style's precision gates, as the headline run has them)
            guard.emit(json.dumps({"other_configs": other_configs(args, R, weights, scene, poses, dev)}))
        return

    def barrier():
        if world > 1:
            import torch.distributed as dist
            dist.barrier()

    if world > 1 and mode == "fused":
        # one decision of the render CNN's precision gate for the whole job (every rank renders the same frame; MAX over ranks)
        # (the trajectory loop's policy: the first pose of the timed trajectory + its middle pose, MAX-combined, then over the ranks)
        sdist.agree_precision(R, frame_pose(0), hw, args.samples,
                              more_poses=() if tile_parallel else (frame_pose(max(1, (args.warmup + args.steps) // 2)),))

    def render_one(pz):
        if tile_parallel:     # bands cut by the static row-cost model x the measured feedback of the frames before (dist.rebalance_scale)
            return sdist.render_frame_tile_parallel(R, pz, hw, args.samples, mode=mode, balance="feedback", stats={})
        return R.render_frame(pz, hw, args.samples, mode=mode, apron=args.apron)

    pipelined = not (args.no_overlap or mode != "fused" or tile_parallel)
    if pipelined and args.warmup:
        # the warm-up frames take the SAME code path as the timed ones (the two-stream trajectory loop): its one-time costs --
        # the side stream, the second set of ray / sky buffers, allocator growth -- belong to the warm-up, not to frame 1 of K
        for _ in R.render_frames([frame_pose(k) for k in range(args.warmup)], hw, args.samples, mode=mode, apron=args.apron):
            pass
    else:
        for k in range(args.warmup):
            render_one(frame_pose(k))
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    t0 = time.perf_counter()
    marks[0].record()
    timed_poses = [frame_pose(args.warmup + k) for k in range(args.steps)]
    probe = {}   # (start, end) events around the mlp_kernel / encode_kernel launches of the timed region, on their own streams
    if not pipelined:
        frames = (render_one(pz) for pz in timed_poses)
    else:   # all K frames are cast, evaluated and finished inside the timed region; frame k+1's ray casting runs beside frame k
        frames = R.render_frames(timed_poses, hw, args.samples, mode=mode, apron=args.apron, probe=probe)
    for k, img in enumerate(frames):
        marks[k + 1].record()       # no sync: per-frame device times for the p10 / p50 / p90 spread (DDA work is pose dependent)
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        import torch.distributed as dist
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        sdist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs and img is not None:       # (tile-parallel: only rank 0 receives the stitched image)
        dump_outputs(args.dump_outputs, {"image" if rank == 0 else f"image_rank{rank}": img}, (64 << 20) // world)

    tp_stats = None
    if tile_parallel and args.full:       # one more frame, outside the timed region, with per-rank device timing of the bands
        tp_stats = {}
        sdist.render_frame_tile_parallel(R, frame_pose(args.warmup), hw, args.samples, mode=mode, balance="feedback", stats=tp_stats)
        barrier()
    frame_ms = sorted(marks[k].elapsed_time(marks[k + 1]) for k in range(args.steps))
    pct = lambda q: frame_ms[min(len(frame_ms) - 1, int(round(q * (len(frame_ms) - 1))))]

    # ---- delivered rate: frame in host memory as uint8 HWC (async D2H, PNG/MP4 encoding excluded), outside the timed region
    from scenedreamer_amd.output import to_uint8_hwc
    if tile_parallel:
        args.no_extras = True
    n_del = 0 if args.no_extras else min(args.steps, 10)
    pinned = [torch.empty((hw[0], hw[1], 3), dtype=torch.uint8).pin_memory() for _ in range(2 if n_del else 0)]
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    if n_del and pipelined:     # the path that is timed above (render_frames), every frame converted and copied to pinned host memory
        for k, im in enumerate(R.render_frames([frame_pose(args.warmup + k) for k in range(n_del)], hw, args.samples, mode=mode, apron=args.apron)):
            pinned[k & 1].copy_(to_uint8_hwc(im), non_blocking=True)
    else:
        for k in range(n_del):
            im = R.render_frame(frame_pose(args.warmup + k), hw, args.samples, mode=mode, apron=args.apron)
            pinned[k & 1].copy_(to_uint8_hwc(im), non_blocking=True)
    torch.cuda.synchronize()
    delivered_fps = n_del / (time.perf_counter() - t2) if n_del else None

    # ---- per-stage breakdown + roofline of the dominant kernel (outside the timed region) ----------
    stages = {}
    for k in range(0 if tile_parallel or not args.full else min(args.steps, 5)):
        R.render_frame(frame_pose(args.warmup + k), hw, args.samples, mode=mode, timers=stages, apron=args.apron)
    stage_ms = {k: float(np.mean(v)) for k, v in stages.items()}
    # the same frames with the other apron setting (outside the timed region; reported for transparency)
    other = "reference" if args.apron == "minimal" else "minimal"
    n_other = 0 if args.no_extras else min(args.steps, 8)
    for k in range(2 if n_other else 0):
        R.render_frame(frame_pose(k), hw, args.samples, mode=mode, apron=other)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for k in range(n_other):
        R.render_frame(frame_pose(args.warmup + k), hw, args.samples, mode=mode, apron=other)
    torch.cuda.synchronize()
    other_ms = 1000.0 * (time.perf_counter() - t1) / n_other if n_other else None
    roof_cnn = roof_sky = None
    if tile_parallel or not args.full:     # (tile-parallel: no per-kernel records on this rank's band, 1/N of the frame)
        roof, roof_grid = None, None
    elif probe.get("mlp_kernel"):
        # the launches of the timed region itself: average duration from HIP events recorded around every launch on the
        # stream it went to (main stream: mlp_kernel; side stream: encode_kernel), work averaged over the same poses
        ms_of = lambda k: float(np.mean([a.elapsed_time(b) for a, b in probe[k]]))
        B, hit, ev = R.field_work(timed_poses, hw, args.samples, args.apron)
        one_kernel = "encode_kernel" not in probe      # field_kernel: lookup + MLP in one launch, no separate encode launch
        alone = None
        if one_kernel or not args.profile:             # stand-alone launches of encode_kernel / mlp_kernel, outside the timed region
            alone = R.measure_roofline(frame_pose(args.warmup), hw, args.samples, mode)
        if one_kernel:
            roof, roof_grid = R.roofline_records(
                B, alone[1]["avg_launch_ms"] * B / alone[1]["samples_per_launch"], ms_of("mlp_kernel"), hit, ev,
                "the encode stage (collapsed 3-D table: 4096 B/sample actually gathered) -- in the timed region it runs INSIDE "
                "field_kernel; timed here as encode_kernel (the same device functions) alone, outside the timed region",
                timing=f"field_kernel: HIP events around each of the {len(probe['mlp_kernel'])} launches of the timed region on the "
                       "main stream; grid sampler: 5 back-to-back stand-alone launches of encode_kernel on the whole padded frame, "
                       "scaled to the samples of a timed launch", field_kernel=True)
        else:
            roof, roof_grid = R.roofline_records(
                B, ms_of("encode_kernel"), ms_of("mlp_kernel"), hit, ev,
                "encode_kernel (collapsed 3-D table: 4096 B/sample actually gathered)",
                timing=f"HIP events around each of the {len(probe['mlp_kernel'])} launches of the timed region, on the launch stream "
                       "(mlp_kernel: main; encode_kernel: side stream, where it shares the GPU with the previous frame's "
                       "mlp_kernel / conv_kernel -- its stand-alone duration is `standalone_ms`)")
        # render CNN (5 015 040 FLOP per pixel of the evaluated frame): its six launches share the GPU with the
        # next frame's sky MLP / sample encode on the side stream in the timed region; `stage_ms.cnn` is the same CNN alone
        px = (hw[0] + 8) * (hw[1] + 8) if args.apron == "minimal" else (hw[0] + 30) * (hw[1] + 30)
        ms_cnn = ms_of("render_cnn")
        t3 = (R.cnn_calibration or {}).get("terms3x3") or getattr(R, "cnn_terms3x3", None) or os.environ.get("SDN_CNN_TERMS")
        roof_cnn = {"bound": "mfma", "kernel": f"head_kernel + conv_kernel<9> x 4 + chain_kernel (RenderCNN; conv1 and the conv4a -> conv4b -> conv4 "
                                               f"chain 3-term f16, 3x3 layers {t3}-term f16)",
                    "precision_gate": R.cnn_calibration,
                    "pixels": px, "algorithmic_flop_per_pixel": 5015040, "avg_ms_in_timed_region": ms_cnn,
                    "achieved": px * 5015040 / (ms_cnn * 1e-3) / 1e12, "peak": 2500.0, "unit": "TFLOP/s",
                    "frac": px * 5015040 / (ms_cnn * 1e-3) / 1e12 / 2500.0,
                    "alone_ms": stage_ms.get("cnn"),
                    "frac_alone": (px * 5015040 / (stage_ms["cnn"] * 1e-3) / 1e12 / 2500.0) if stage_ms.get("cnn") else None,
                    "timing": "HIP events around the CNN of every timed frame on the main stream"}
        # ---- per-launch records of the kernels the three records above do not break down: the render CNN's six launches and the
        #      sky MLP, each ALONE on the GPU (5 repetitions on the evaluated frame, outside the timed region)
        try:
            Hc, Wc = (hw[0] + 8, hw[1] + 8) if args.apron == "minimal" else (hw[0] + 30, hw[1] + 30)
            xin = torch.rand(1, Hc, Wc, 64, device=dev) * 2 - 1
            cnn = R.mfma_cnn(xin)
            cnn(xin)
            tm = {}
            for _ in range(5):
                cnn(xin, timers=tm)
            torch.cuda.synchronize()
            per = {}
            for name, fl in cnn.FLOP_PER_PIXEL.items():
                ms_k = float(np.mean([a.elapsed_time(b) for a, b in tm[name]]))
                t_k = cnn.terms.get(name.split(" ")[0], 3)
                per[name] = {"avg_launch_ms": ms_k, "algorithmic_flop_per_pixel": fl, "achieved": Hc * Wc * fl / (ms_k * 1e-3) / 1e12,
                             "frac": Hc * Wc * fl / (ms_k * 1e-3) / 1e12 / 2500.0, "f16_products_per_algorithmic_product": t_k}
            roof_cnn["per_launch_alone"] = {"pixels": Hc * Wc, "unit": "TFLOP/s", "peak": 2500.0, "bound": "mfma", "kernels": per,
                                            "timing": "HIP events between the launches, 5 repetitions, nothing else on the GPU; an event between two launches opens a "
                                                      "gap of ~0.05 - 0.1 ms that is inside these figures (their sum exceeds `alone_ms`): the pure kernel "
                                                      "durations are rocprof's, profiles/r05_kernel_stats.md"}
            n_sky = (hw[0] + 30) * (hw[1] + 30)
            from scenedreamer_amd import fused as _fused
            from scenedreamer_amd.renderer import _time_ms
            rd_sky = torch.nn.functional.normalize(torch.randn(n_sky, 3, device=dev), dim=-1)
            ms_sky = _time_ms(lambda: _fused.sky_fused(R, rd_sky), 5)
            roof_sky = {"bound": "mfma", "kernel": f"sky_kernel (SKYMLP on every ray of the padded frame + the frame mean; hidden layers "
                                                   f"{'f16 + MX-fp6 corrections' if _fused.sky_terms(R) == 6 else '3-term f16'})",
                        "rays": n_sky, "algorithmic_flop_per_ray": 573952, "avg_launch_ms": ms_sky,
                        "achieved": n_sky * 573952 / (ms_sky * 1e-3) / 1e12, "peak": 2500.0, "unit": "TFLOP/s",
                        "frac": n_sky * 573952 / (ms_sky * 1e-3) / 1e12 / 2500.0,
                        "timing": "5 stand-alone launches, nothing else on the GPU (in the timed region it runs beside the previous frame's CNN)"}
        except Exception as ex:  # noqa: BLE001 -- extra records must not cost the headline line
            roof_sky = {"error": f"{type(ex).__name__}: {ex}"}
        if one_kernel:   # the MLP stage by itself (mlp_kernel on pre-encoded features: the same layers without the encode stage)
            roof["mlp_stage_alone"] = {"kernel": "mlp_kernel (stand-alone launches on pre-encoded features, outside the timed region)",
                                       "avg_launch_ms": alone[0]["avg_launch_ms"], "achieved": alone[0]["achieved"],
                                       "frac": alone[0]["frac"], "samples_evaluated": alone[0]["samples_evaluated"]}
        if alone is not None:
            roof["standalone_ms"], roof_grid["standalone_ms"] = alone[0]["avg_launch_ms"], alone[1]["avg_launch_ms"]
            roof["standalone_note"] = roof_grid["standalone_note"] = (
                "standalone_ms: 5 back-to-back launches of "
                + ("mlp_kernel (the MLP stage alone, features pre-encoded) / encode_kernel" if one_kernel else "the kernel")
                + f" alone on the whole padded frame ({alone[0]['samples_per_launch']} samples), outside the timed region")
    else:
        roof, roof_grid = R.measure_roofline(frame_pose(args.warmup), hw, args.samples, mode)
    roof_rvip = None
    if rank == 0 and not tile_parallel and args.full:
        roof_rvip = rvip_roofline(R, timed_poses, hw)
        if roof is not None and roof.get("bound") == "mfma" and not args.profile:
            sustained_ceiling(roof)
    early = None
    if rank == 0 and world == 1 and mode == "fused" and not tile_parallel and not args.no_extras:
        early = early_termination_record(args, R, weights, scene, poses, hw, mode)

    floor = style_cost = skip_off_fps = None
    if rank == 0 and world == 1 and mode == "fused" and not tile_parallel and not args.no_extras:
        try:
            floor = floor_record(args, R, weights, scene, poses, hw, mode)
        except Exception as ex:  # noqa: BLE001 -- an extra record must not cost the headline line
            floor = {"error": f"{type(ex).__name__}: {ex}"}
        try:        # the timed region's poses with colour-branch skipping off (bit-identical images; tests/test_fused_gpu.py)
            R.colour_skip = False
            skip_off_fps = 1000.0 / _trajectory_ms(R, timed_poses, hw, args.samples, mode, args.apron)
        except Exception as ex:  # noqa: BLE001
            sys.stderr.write(f"[bench] colour_skip_off: {type(ex).__name__}: {ex}\n")
        finally:
            R.colour_skip = None
        try:
            style_cost = style_cost_record(args, weights, scene, poses, hw, mode, dev)
        except Exception as ex:  # noqa: BLE001
            style_cost = {"error": f"{type(ex).__name__}: {ex}"}

    # config 4 is the whole orbit split over the ranks (K = 256 / N each); an explicit --steps other than that K times part of it
    partial_orbit = args.config == 4 and args.steps != max(1, maxstep // world)
    if rank == 0:
        fps = (1 if tile_parallel else world) * args.steps / elapsed
        out = {
            # BASELINE.json's metric verbatim ("...; HBM GB/s": value = frames/s, the grid sampler's GB/s is in roofline_grid_sampler)
            "metric": f"rendered frames/sec @{args.width}\u00d7{args.height}, {args.samples} samples/ray, scene_size {args.scene_size}; HBM GB/s",
            "value": fps, "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1000.0 * elapsed / args.steps, "higher_is_better": True,
            # config 5: one frame split over the ranks; config 4: the 256 frames of the orbit split over the ranks (K = 256 / N per rank):
            # both fixed total work = strong.  Default (and what the driver's SCALE run is): every rank renders K frames = weak.
            "scaling": "strong" if (tile_parallel or (args.config == 4 and not partial_orbit)) else "weak",
            "vs_baseline": None, "dtype": R.compute_dtype(mode), "data": "synthetic",
            "config": {"workload": f"{args.width}x{args.height}, num_samples={args.samples}, "
                                   f"scene_size={args.scene_size}, cam pattern 0 (pose stride {args.pose_stride} of {maxstep} poses), "
                                   + ("1 frame per step, row bands over the ranks (tile-parallel)" if tile_parallel
                                      else "1 frame per rank per step")
                                   + (f", {args.steps * world} of the {maxstep} orbit frames" if partial_orbit else ""),
                       "baseline_config": None if partial_orbit else args.config or (2 if (hw, args.samples, args.scene_size) == ((540, 960), 24, 2048) else None),
                       "path": mode, "apron": ("minimal" if mode == "fused" else "reference") if tile_parallel else args.apron,
                       "bands": ({"rows": tp_stats.get("bands"), "band_ms": tp_stats.get("band_ms"), "imbalance_max_over_mean": tp_stats.get("imbalance"),
                                  "cut": "equal estimated work (dist.balanced_row_bands on a 1/16-resolution ray cast)" if world > 1 else "one band",
                                  "timing": "device events around each rank's own band work in one extra frame after the timed region"}
                                 if tp_stats else None),
                       "field": ("one kernel (field_kernel: sample placement + hash-grid lookup + MLP + compositing)"
                                 if mode == "fused" and _single_kernel(R) else "encode_kernel -> HBM -> mlp_kernel") if mode == "fused" else None,
                       "ray_casting_overlap": not (args.no_overlap or mode != "fused"),
                       "scene_volume": ("uint8 palette indices" if getattr(scene, "voxel_u8", None) is not None else "int32 block ids"),
                       "padded_rays": (hw[0] + 30) * (hw[1] + 30),
                       "field_rays": (hw[0] + 8) * (hw[1] + 8) if (args.apron == "minimal" and mode == "fused") else (hw[0] + 30) * (hw[1] + 30),
                       "samples_per_frame": ((hw[0] + 8) * (hw[1] + 8) if (args.apron == "minimal" and mode == "fused") else (hw[0] + 30) * (hw[1] + 30)) * args.samples,
                       "parallelism": f"row bands x{world}" if tile_parallel else f"frames x{world}",
                       "dist_backend": (args.backend + (f", {world} ranks on {ndev} GPU(s)" if world > ndev else "")) if world > 1 else None,
                       "apron_note": "ray casting and the sky MLP always cover the reference's padded frame (15-px apron); "
                                     "'minimal' evaluates the field MLP and the CNN on the 4-px apron that can reach a kept "
                                     "pixel -- the same image: bit-identical with term_eps = 0, within the early-termination bound (2 eps = 1e-4 on net_out each) otherwise "
                                     "(tests/test_render_gpu.py, test_fullsize_gpu.py)"},
            "frame_ms_p10_p50_p90": [pct(0.1), pct(0.5), pct(0.9)], "delivered_frames_per_s_uint8_host": delivered_fps,
            "stage_ms": stage_ms, "setup_s": setup_s, "broadcast": bstats or None, f"ms_per_step_apron_{other}": other_ms,
            "roofline": roof, "roofline_grid_sampler": roof_grid, "roofline_cnn": roof_cnn, "roofline_rvip": roof_rvip,
            "roofline_sky": roof_sky,
            "early_termination": early,
            "floor": floor, "colour_skip_off_frames_per_s": skip_off_fps, "style_cost": style_cost,
        }
        gates = {"cnn": getattr(R, "cnn_calibration", None),
                 "field": {k: v for k, v in (getattr(R, "field_gate", None) or {}).items() if k != "measurements"} or None,
                 "colour_terms": (getattr(R, "field_gate", None) or {}).get("colour"), "sky": (getattr(R, "field_gate", None) or {}).get("sky")}
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args, weights, scene, R.z.cpu().numpy(), R.global_enc.cpu().numpy())
            # a reduced-precision internal path is named (`dtype`) together with its MEASURED max-abs error:
            # the same pose through the timed path (pipelined render_frames, this volume, this apron) against the
            # oracle's pixels of the tiles the CPU baseline has just rendered
            if tile_parallel:
                gpu_img = render_one(cpu_baseline.pose)
            elif mode == "fused" and not args.no_overlap:
                gpu_img = [im.clone() for im in R.render_frames([cpu_baseline.pose] * 2, hw, args.samples, mode=mode, apron=args.apron)][1]
            else:
                gpu_img = R.render_frame(cpu_baseline.pose, hw, args.samples, mode=mode, apron=args.apron)
            gpu_img = gpu_img.cpu().numpy()
            errs = {t: float(np.abs(gpu_img[:, :, r0:r0 + im.shape[2], c0:c0 + im.shape[3]] - im.numpy()).max())
                    for t, (r0, c0, im) in cpu_baseline.tiles.items()}
            for pz_b, tiles_b in getattr(cpu_baseline, "more", []):      # the second pose of the CPU leg, through render_frame
                img_b = R.render_frame(pz_b, hw, args.samples, mode=mode, apron=args.apron).cpu().numpy()
                errs.update({(f"pose26:{t[0]}", t[1]): float(np.abs(img_b[:, :, r0:r0 + im.shape[2], c0:c0 + im.shape[3]] - im.numpy()).max())
                             for t, (r0, c0, im) in tiles_b.items()})
            out["precision"] = {"max_abs_err": max(errs.values()), "bound": 1e-3, "quantity": "image (tanh output, range [-1, 1])",
                                "gates": gates,
                                "per_tile": {f"{t[0]},{t[1]}": e for t, e in errs.items()},
                                "where_measured": f"{len(errs)} tiles of the reference's tile grid ({sum(im.shape[2] * im.shape[3] for _, _, im in cpu_baseline.tiles.values())} "
                                                  f"of {hw[0] * hw[1]} pixels of pose 8, + the tiles of pose 26), poses 8 and 26 of the 40-pose orbit, this run's GPU path vs the fp32 CPU "
                                                  f"run named in cpu_baseline (kind: {out['cpu_baseline']['kind']}); one whole frame (40 of 40 "
                                                  "tiles) and configs 3 / 5 against the oracle: tests/test_config_parity_gpu.py"}
        if "precision" not in out:
            out["precision"] = {"gates": gates, "max_abs_err": None,
                                "note": "per-style gates only: the error against the CPU run is measured with the cpu_baseline leg"}
        if world == 1 and mode == "fused" and not tile_parallel and not args.no_extras:
            # north star: "within 1e-3 vs the reference CUDA path".  Its nearest stand-in on this box: the reference's op sequence
            # in fp32 on the GPU -- sample placement by PyTorch ops on a GPU tensor (mc_utils.py:82-151: torch.cumsum accumulates
            # in float32 there, in double on the CPU the oracle follows), this package's drop-in grid op, torch fp32 MLP / conv2d.
            # One whole frame, reference apron, outside the timed region.
            try:
                pz = frame_pose(args.warmup)
                a = R.render_frame(pz, hw, args.samples, mode="fused", apron=args.apron)
                b = R.render_frame(pz, hw, args.samples, mode="unfused", cnn_mode="torch")
                torch.cuda.synchronize()
                t_fb = time.perf_counter()
                for _ in range(2):
                    R.render_frame(pz, hw, args.samples, mode="unfused", cnn_mode="torch")
                torch.cuda.synchronize()
                # what a style pays when calibrate_style rejects the MFMA path (gain-scaled weights in tests/test_precision_gates_gpu.py):
                # the fp32 op sequence below the HIP ray marcher / grid op is PyTorch (rocBLAS addmm, MIOpen conv2d), not a HIP rung
                out["fallback_fp32_path_frames_per_s"] = 2.0 / (time.perf_counter() - t_fb)
                e = (a - b).abs()
                out["precision"]["vs_gpu_placement_fp32_path"] = {
                    "max_abs_diff": float(e.max()), "fraction_above_1e-4": float((e > 1e-4).float().mean()), "pixels": int(e[0, 0].numel()),
                    "what": "fused HIP frame vs Renderer.render_frame(mode='unfused', cnn_mode='torch'): torch-op sample placement on the GPU "
                            "(float32 cumsum, as the reference's CUDA path places samples), HIP grid op, fp32 torch MLP and convolutions; "
                            "also asserted < 1e-3 at 960x540 and 1920x1080 in tests/test_fullsize_gpu.py"}
            except Exception as ex:  # noqa: BLE001 -- an extra record must not cost the headline line
                out["precision"]["vs_gpu_placement_fp32_path"] = {"error": f"{type(ex).__name__}: {ex}"}
        if world == 1 and mode == "fused" and not tile_parallel:
            if not args.no_other_configs and (hw, args.samples, args.scene_size) == ((540, 960), 24, 2048):
                try:
                    out["other_configs"] = other_configs(args, R, weights, scene, poses, dev)
                except Exception as e:  # noqa: BLE001 -- an extra record must not cost the headline line
                    out["other_configs"] = {"error": f"{type(e).__name__}: {e}"}
            if not args.no_dropin:
                del R
                torch.cuda.empty_cache()
                try:
                    out["dropin"] = dropin_record(args, weights, scene, dev, getattr(cpu_baseline, "tiles", None))
                except Exception as e:  # noqa: BLE001
                    out["dropin"] = {"error": f"{type(e).__name__}: {e}"}
        # the full record -> bench_detail.json; its numeric extract (<= 6 KB, benchline.compact) -> the one stdout line
        detail_path = os.environ.get("SDN_BENCH_DETAIL") or os.path.join(ROOT, "bench_detail.json")
        try:
            with open(detail_path, "w") as f:
                json.dump(out, f, indent=1, default=str)
        except OSError as e:
            sys.stderr.write(f"[bench] could not write {detail_path}: {e}\n")
            detail_path = None
        guard.emit(benchline.line(out, detail_path))
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
