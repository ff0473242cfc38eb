"""Trajectory renderer with the reference's inference.py / inference_givenstyle interface
(inference.py:18-32, configs/scenedreamer_inference.yaml:1-17):

    python -m scenedreamer_amd.cli --output_dir out --seed 8888 [--checkpoint scenedreamer_released.pt]
        [--camera_mode 4 --cam_maxstep 40 --resolution_hw 540 960 --num_samples 40 --cam_ang 72 --scene_size 2048]
        [--video-backend auto|imageio|mjpeg|mjpeg-gpu]     # mjpeg-gpu: the video's JPEG frames are encoded on the GPU
        [--png-backend pillow|gpu]                         # gpu: the PNG frames are filtered and deflated on the GPU
        [--depth-maps off|u8|u16 [--depth-max D]]          # also <output_dir>/depth/%05d.png (inference_givenstyle_depth)
        [--scene world.npz]     # a saved reference world: voxel_t, heightmap, current_height_map, current_semantic_map, trans_mat
    python -m torch.distributed.run --nproc-per-node N ... -m scenedreamer_amd.cli ...     # frames sharded over GPUs

Without --checkpoint (none is available offline) a seeded synthetic scene and random-init weights of the reference's
shapes are used.  Outputs as the reference writes them (scenedreamer.py:557-564, :629-632): <output_dir>/rgb_render/%05d.png,
semantic_map.png, height_map.png, style.npy and, on a single rank, <output_dir>/rgb_render.mp4 at 10 fps -- all by a
background writer."""
import argparse
import os

import numpy as np
import torch


def build_parser():
    ap = _Parser()
    ap.add_argument("--output_dir", required=True)
    ap.add_argument("--seed", type=int, default=8888)
    ap.add_argument("--checkpoint", default="")
    ap.add_argument("--camera_mode", type=int, default=4)
    ap.add_argument("--cam_maxstep", type=int, default=40)
    ap.add_argument("--resolution_hw", type=int, nargs=2, default=[540, 960])
    ap.add_argument("--num_samples", type=int, default=40)
    ap.add_argument("--cam_ang", type=float, default=72)
    ap.add_argument("--scene_size", type=int, default=2048)
    ap.add_argument("--scene", default="", help="npz with the fields of the reference's voxel handle (pcg_gen.py:161-174)")
    ap.add_argument("--mode", default="fused", choices=["fused", "unfused", "exact"],
                    help="fused: MFMA kernels behind the per-style precision gates; unfused: the reference's fp32 op sequence on "
                         "PyTorch; exact: that sequence with the field on the fp32 MFMA kernel (no calibration, any weight range)")
    ap.add_argument("--exact-cnn", dest="exact_cnn", default=None, choices=["torch", "f32"],
                    help="render CNN of the exact path (--mode exact, or a closed gate with Renderer.fallback = 'exact'): torch = the "
                         "reference's F.conv2d sequence (default; SDN_EXACT_CNN when not given); f32 = the fp32 MFMA kernel "
                         "(fixed summation order, any weight range).  Every rank of a job must be given the same value")
    ap.add_argument("--exact-world", dest="exact_world", default=None, choices=["torch", "f32"],
                    help="world encoder (global_enc, once per scene, in every --mode): torch = the reference's F.conv2d sequence "
                         "(default; SDN_EXACT_WORLD when not given); f32 = the fixed-order fp32 kernels (no library solver choice "
                         "between the maps and global_enc).  Every rank of a job must be given the same value")
    ap.add_argument("--exact-style", dest="exact_style", default=None, choices=["torch", "f32"],
                    help="style MLP (z, once per style, in every --mode): torch = the reference's F.linear sequence (default; "
                         "SDN_EXACT_STYLE when not given); f32 = the fixed-order kernel (f64 accumulation in k order).  Every rank of "
                         "a job must be given the same value")
    ap.add_argument("--exact-sky", dest="exact_sky", default=None, choices=["torch", "f32"],
                    help="sky MLP of the exact path (--mode exact, or a closed gate with Renderer.fallback = 'exact'): torch = the "
                         "reference's F.linear sequence and a library mean (default; SDN_EXACT_SKY when not given); f32 = the fp32 MFMA "
                         "kernel (fixed summation order, any weight range).  Every rank of a job must be given the same value")
    ap.add_argument("--video-backend", dest="video_backend", default="auto", choices=["auto", "imageio", "mjpeg", "mjpeg-gpu"],
                    help="writer of rgb_render.mp4 (single rank only): auto = imageio's H.264 where imageio is importable, else mjpeg; "
                         "mjpeg = Motion-JPEG encoded by Pillow on one host thread; mjpeg-gpu = the same container with every frame "
                         "encoded on the GPU (quality 92, 4:4:4), so that only the encoded bytes cross PCIe")
    ap.add_argument("--png-backend", dest="png_backend", default="pillow", choices=["pillow", "gpu"],
                    help="encoder of rgb_render/%%05d.png: pillow = zlib at compress_level 4 on a pool of host threads; gpu = the "
                         "filters, one dynamic-Huffman deflate block and the Adler-32 on the GPU (lossless, the same pixels; larger "
                         "files where the image repeats at a distance), so that only the encoded bytes cross PCIe")
    ap.add_argument("--depth-maps", dest="depth_maps", default="off", choices=["off", "u8", "u16"],
                    help="also write <output_dir>/depth/%%05d.png per frame (the reference's inference_givenstyle_depth): off = none "
                         "(default; the run is what it was); u8 = the reference's 8-bit values, normalised per frame over the pixels "
                         "that hit something; u16 = 16-bit depth in world units scaled by --depth-max, comparable across frames")
    ap.add_argument("--depth-max", dest="depth_max", type=float, default=None,
                    help="depth that maps to 65535 with --depth-maps u16 (larger depths are clamped); required with u16")
    return ap


class _Parser(argparse.ArgumentParser):
    """The flags that depend on each other are checked where the arguments are parsed, so every user of build_parser() gets the
    same errors as the command line."""

    def parse_args(self, args=None, namespace=None):
        ns = super().parse_args(args, namespace)
        if ns.depth_maps == "u16" and ns.depth_max is None:
            self.error("--depth-maps u16 needs --depth-max")
        if ns.depth_max is not None and not ns.depth_max > 0:
            self.error("--depth-max must be a positive number")
        return ns


def main(argv=None):
    args = build_parser().parse_args(argv)

    world, rank, local = (int(os.environ.get(k, d)) for k, d in (("WORLD_SIZE", 1), ("RANK", 0), ("LOCAL_RANK", 0)))
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", init_method="env://")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    from . import camera, synth
    from . import dist as sdist
    from .output import FrameWriter, write_scene_maps
    from .renderer import Renderer

    scene = weights = style = None
    if rank == 0:
        if args.scene:
            z = np.load(args.scene)
            scene = synth.Scene()
            scene.voxel_t = torch.from_numpy(z["voxel_t"].astype(np.int32)).to(dev)
            scene.heightmap = torch.from_numpy(z["heightmap"])
            scene.current_height_map = torch.from_numpy(z["current_height_map"].astype(np.float32)).to(dev)
            scene.current_semantic_map = torch.from_numpy(z["current_semantic_map"].astype(np.float32)).to(dev)
            scene.trans_mat = torch.from_numpy(z["trans_mat"].astype(np.float32))
            scene.sample_size = int(scene.voxel_t.shape[1])
        else:
            scene = synth.make_scene(args.scene_size, 3407, device=dev)
        if args.checkpoint:
            ck = torch.load(args.checkpoint, map_location="cpu")      # inference.py:57-61 ("module." prefix)
            weights = {k[len("module."):] if k.startswith("module.") else k: v for k, v in ck["net_G"].items()}
        else:
            weights = synth.make_weights(0)
        style = synth.make_style(args.seed)                           # inference.py:81-82
    if world > 1:
        scene, weights, style = sdist.broadcast_state(scene, weights, style, dev, src=0)
    R = Renderer(weights, scene, dev, exact_world=args.exact_world, exact_style=args.exact_style)
    R.set_style(style)
    if args.exact_cnn is not None:
        R.exact_cnn = args.exact_cnn
    if args.exact_sky is not None:
        R.exact_sky = args.exact_sky
    poses = camera.eval_camera_poses(scene, maxstep=args.cam_maxstep, pattern=args.camera_mode, cam_ang=args.cam_ang)
    if world > 1 and args.mode == "fused":     # one decision of the render CNN's precision gate for all ranks
        sdist.agree_cnn_precision(R, poses[0], tuple(args.resolution_hw), args.num_samples)
    out = os.path.join(args.output_dir, "rgb_render")
    # (a sharded job writes PNGs from every rank; the video needs the frames in one place, so only a single rank writes it)
    writer = FrameWriter(out, video_path=(out + ".mp4") if world == 1 else None, fps=10, video_backend=args.video_backend,
                         png_backend=args.png_backend)
    if rank == 0:
        write_scene_maps(out, scene)                                  # scenedreamer.py:562-563
        np.save(os.path.join(out, "style.npy"), np.asarray(style))    # scenedreamer.py:564
    mine = sdist.shard_frames(range(len(poses)), rank, world)
    hw = tuple(args.resolution_hw)
    if args.depth_maps != "off":
        return _render_with_depth(args, R, poses, mine, hw, writer, rank, world, dev)
    if args.mode == "fused":     # next frame's ray casting on a second stream beside the current frame
        frames = R.render_frames([poses[f] for f in mine], hw, args.num_samples, mode="fused")
    else:
        frames = (R.render_frame(poses[f], hw, args.num_samples, mode=args.mode) for f in mine)
    for f, img in zip(mine, frames):
        print(f"[rank {rank}] Rendering frame {f}", flush=True)
        writer.submit(img, f)
    writer.close()
    _leave(world)


def _render_with_depth(args, R, poses, mine, hw, writer, rank, world, dev):
    """The loop of main with --depth-maps u8 | u16: every frame also yields its depth map, written to <output_dir>/depth/%05d.png
    (the reference's directory, scenedreamer.py:720, :844) by every rank for its own frames."""
    from . import maps as M
    from .output import MapWriter
    bits = 8 if args.depth_maps == "u8" else 16
    depth_writer = MapWriter(os.path.join(args.output_dir, "depth"), bits=bits)
    metric = M.metric_range(args.depth_max, dev) if bits == 16 else None
    want = ("depth_u8",) if bits == 8 else ("depth",)
    if args.mode == "fused":
        frames = R.render_frames([poses[f] for f in mine], hw, args.num_samples, mode="fused", maps=dict.fromkeys(want))
    else:
        def one(f):
            m = dict.fromkeys(want)
            return R.render_frame(poses[f], hw, args.num_samples, mode=args.mode, maps=m), m
        frames = (one(f) for f in mine)
    for f, (img, m) in zip(mine, frames):
        print(f"[rank {rank}] Rendering frame {f}", flush=True)
        writer.submit(img, f)
        depth_writer.submit(m["depth_u8"] if bits == 8 else M.quantise(m["depth"], metric, 16), f)
    writer.close()
    depth_writer.close()
    _leave(world)


def _leave(world):
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
