#!/usr/bin/env python
"""Times the fp32 field rung against the PyTorch fp32 op sequence it replaces, at the benchmark configuration (960x540, 24 samples,
scene 2048, pose 0 of pattern 0, synthetic weights, style 8888), and writes profiles/exact_rung_timing.json.

    python tools/exact_rung_timing.py [--reps 10] [--warmup 3] [--out profiles/exact_rung_timing.json] [--only cnn]

Six comparisons, each inside ONE process on one device (devices differ by up to 20 %):
  field   fused.field_exact  vs  Renderer.field_unfused over the rays of the same (minimal-apron) window
  frame   render_frame(mode="exact")  vs  render_frame(mode="unfused")
  cnn     cnn.F32CNN (csrc/cnn_f32.hip)  vs  Renderer.render_cnn (PyTorch) on the same 548 x 968 net_out, and
          render_frame(mode="exact") with exact_cnn = "f32" vs "torch"; the kernel's per-launch times, and its time against the
          matrix-issue floor of the CNN: pixels x 5 015 040 FLOP / (1 024 SIMDs x 64 FLOP per clock x the clock)
  sky     fused.sky_exact (csrc/sky_f32.hip)  vs  Renderer.sky_features + .mean() (PyTorch) on the rays of the same 548 x 968 frame
          (the minimal-apron frame's ray count; sky_c and the frame mean on both sides), and the kernel's time against its
          matrix-issue floor: 128-ray groups x 4 waves x chunks issued (fc1's padding included) x 128 MFMAs x 64 cycles / 1 024
          SIMDs / the clock
  world   fused.world_exact (csrc/world_f32.hip)  vs  Renderer._world_encoder_torch (the F.conv2d sequence of set_scene, with the
          deterministic-algorithm flags it sets) on the 2048 x 2048 benchmark scene's maps, resident on the device on both sides
  style   fused.style_exact  vs  Renderer._style_mlp_torch (the F.linear sequence of set_style) on style 8888
          (both run once per scene / per style, not per frame: no time here is a gate, the two kernels stand on their fixed order)
--only STEP runs one comparison and replaces only its key in an existing record.
Every figure is the median of `reps` HIP-event timings after `warmup` runs, the two sides interleaved; `faster` is true when the
gain exceeds the spread (max - min) of either side.  The field kernel's time is also set against its matrix-issue floor: evaluated
32-sample tiles x 5 888 MFMAs x 64 cycles / 1 024 SIMDs / the clock.
Each comparison runs as a child process under its own `timeout`; the first failure ends the run (nothing more is started)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HW, NS, SCENE = (540, 960), 24, 2048
MFMA_PER_TILE_PASS, MFMA_CYCLES, SIMDS, CLOCK_GHZ = 5888, 64, 1024, 2.4     # the clock: the part's maximum, so the fraction is a lower bound
STEP_TIMEOUT_S = {"field": 420, "frame": 420, "cnn": 420, "sky": 300, "world": 300, "style": 300}
SKY_CHUNKS, MFMA_PER_CHUNK = 2 + 4 * 8 + 2, 128      # csrc/sky_f32.hip: fc1 padded to K = 64 (2 chunks) | fc2 .. fc5 | fc_out_c
SKY_FLOP_PER_RAY = 2 * (33 * 256 + 4 * 256 * 256 + 256 * 64)
CNN_FLOP_PER_PIXEL, F32_FLOP_PER_CLOCK_PER_SIMD = 5015040, 64


def _setup():
    import torch
    sys.path.insert(0, ROOT)
    from scenedreamer_amd import camera, synth
    from scenedreamer_amd.renderer import Renderer
    dev = torch.device("cuda:0")
    scene = synth.make_scene(SCENE, 3407, device=dev)
    R = Renderer(synth.make_weights(0), scene, dev)
    R.set_style(synth.make_style(8888))
    pose = camera.eval_camera_poses(scene, maxstep=40)[0]
    return torch, R, pose


def _time_pair(torch, a, b, reps, warmup):
    """[ms] of a() and b(), interleaved, HIP events on the current stream."""
    for _ in range(warmup):
        a()
        b()
    torch.cuda.synchronize()
    out = ([], [])
    for _ in range(reps):
        for fn, sink in ((a, out[0]), (b, out[1])):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            sink.append(e0.elapsed_time(e1))
    return out


def _summary(new, old):
    s = lambda v: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread_ms=max(v) - min(v), runs_ms=[round(x, 3) for x in v])
    n, o = s(new), s(old)
    gain = o["median_ms"] - n["median_ms"]
    return n, o, dict(gain_ms=gain, speedup=o["median_ms"] / n["median_ms"], faster=bool(gain > max(n["spread_ms"], o["spread_ms"])))


def step_field(reps, warmup):
    torch, R, pose = _setup()
    from scenedreamer_amd import fused
    from scenedreamer_amd.precision import CNN_HALO
    with torch.no_grad():
        vid, d2, rd, (Hp, Wp) = R.cast_rays(pose, HW)
        n = Hp * Wp
        vid, d2, rd = vid.view(n, R.M), d2.view(2, n, R.M), rd.view(n, 3)
        sky_c = R.sky_features(rd)
        sky_avg = sky_c.mean(dim=0, keepdim=True)
        o = R.pad // 2 - CNN_HALO
        win = fused.Window.crop(Hp, Wp, o)
        rows, cols = Hp - 2 * o, Wp - 2 * o
        cut = lambda t: t.view(Hp, Wp, -1)[o:o + rows, o:o + cols].reshape(rows * cols, -1).contiguous()
        vid_w, rd_w, sky_w = cut(vid), cut(rd), cut(sky_c)
        d2_w = torch.stack([cut(d2[0]), cut(d2[1])]).contiguous()
        ori = torch.as_tensor(pose[0], dtype=torch.float32)
        ori_dev = ori.to(R.dev)
        chunk = 1 << 16

        def exact():
            return fused.field_exact(R, vid, d2, rd, ori, sky_c, sky_avg, NS, window=win)

        def unfused():
            return torch.cat([R.field_unfused(vid_w[r:r + chunk], d2_w[:, r:r + chunk], rd_w[r:r + chunk], ori_dev, sky_w[r:r + chunk],
                                              sky_avg, NS) for r in range(0, rows * cols, chunk)])

        diff = float((exact() - unfused()).abs().max())
        new, old = _time_pair(torch, exact, unfused, reps, warmup)
        hit = win.groups((vid_w[:, 0] != 0), ragged=True).any(dim=1)
        tiles = int(hit.sum()) * 4 * (-(-NS // 4))
    n_, o_, cmp_ = _summary(new, old)
    floor_ms = tiles * MFMA_PER_TILE_PASS * MFMA_CYCLES / SIMDS / (CLOCK_GHZ * 1e6)
    return dict(window=[rows, cols], rays=rows * cols, max_abs_diff_net_out=diff, field_exact=n_, field_unfused=o_, **cmp_,
                evaluated_tile_passes=tiles, evaluated_samples=tiles * 32, matrix_floor_ms=floor_ms, clock_ghz_assumed=CLOCK_GHZ,
                matrix_issue_fraction=floor_ms / n_["median_ms"])


def step_frame(reps, warmup):
    torch, R, pose = _setup()
    exact = lambda: R.render_frame(pose, HW, NS, mode="exact")
    unfused = lambda: R.render_frame(pose, HW, NS, mode="unfused")
    diff = float((exact() - unfused()).abs().max())
    new, old = _time_pair(torch, exact, unfused, reps, warmup)
    n_, o_, cmp_ = _summary(new, old)
    return dict(max_abs_diff_image=diff, render_frame_exact=n_, render_frame_unfused=o_, **cmp_,
                frames_per_s_exact=1e3 / n_["median_ms"], frames_per_s_unfused=1e3 / o_["median_ms"])


def step_cnn(reps, warmup):
    torch, R, pose = _setup()
    from scenedreamer_amd.cnn import F32CNN
    with torch.no_grad():
        net_out = R.render_frame(pose, HW, NS, mode="exact", cnn=False)          # [1, 548, 968, 64]: the minimal apron
        _, Hc, Wc, _ = net_out.shape
        k = R.f32_cnn()
        new_fn, old_fn = (lambda: k(net_out)), (lambda: R.render_cnn(net_out))
        diff = float((new_fn() - old_fn()).abs().max())
        new, old = _time_pair(torch, new_fn, old_fn, reps, warmup)
        timers = {}
        for _ in range(reps):
            k(net_out, timers=timers)
        torch.cuda.synchronize()
        launches = {}
        for name, evs in timers.items():
            ms = statistics.median(a.elapsed_time(b) for a, b in evs)
            fl = F32CNN.FLOP_PER_PIXEL[name] * Hc * Wc
            launches[name] = dict(median_ms=ms, gflop=fl / 1e9, tflops=fl / ms / 1e9,
                                  matrix_floor_ms=fl / (SIMDS * F32_FLOP_PER_CLOCK_PER_SIMD * CLOCK_GHZ * 1e6))
        n_, o_, cmp_ = _summary(new, old)
        floor_ms = Hc * Wc * CNN_FLOP_PER_PIXEL / (SIMDS * F32_FLOP_PER_CLOCK_PER_SIMD * CLOCK_GHZ * 1e6)

        def frame(which):
            R.exact_cnn = which
            return R.render_frame(pose, HW, NS, mode="exact")
        fdiff = float((frame("f32") - frame("torch")).abs().max())
        fnew, fold = _time_pair(torch, lambda: frame("f32"), lambda: frame("torch"), reps, warmup)
        fn_, fo_, fcmp = _summary(fnew, fold)
    return dict(net_out=[Hc, Wc], pixels=Hc * Wc, flop_per_pixel=CNN_FLOP_PER_PIXEL, max_abs_diff_image=diff, f32cnn=n_, render_cnn_torch=o_, **cmp_,
                launches=launches, matrix_floor_ms=floor_ms, clock_ghz_assumed=CLOCK_GHZ, matrix_issue_fraction=floor_ms / n_["median_ms"],
                frame=dict(max_abs_diff_image=fdiff, render_frame_exact_cnn_f32=fn_, render_frame_exact_cnn_torch=fo_, **fcmp))


def step_sky(reps, warmup):
    torch, R, pose = _setup()
    from scenedreamer_amd import fused
    from scenedreamer_amd.precision import CNN_HALO
    with torch.no_grad():
        _, _, rd, (Hp, Wp) = R.cast_rays(pose, HW)
        o = R.pad // 2 - CNN_HALO
        rows, cols = Hp - 2 * o, Wp - 2 * o                                 # 548 x 968
        rd = rd.view(Hp, Wp, 3)[o:o + rows, o:o + cols].reshape(rows * cols, 3).contiguous()
        n = rd.shape[0]

        def exact():
            return fused.sky_exact(R, rd)

        def torch_seq():
            c = R.sky_features(rd)
            return c, c.mean(dim=0, keepdim=True)

        (c0, a0), (c1, a1) = exact(), torch_seq()
        diff_c, diff_avg = float((c0 - c1).abs().max()), float((a0 - a1).abs().max())
        new, old = _time_pair(torch, exact, torch_seq, reps, warmup)
    n_, o_, cmp_ = _summary(new, old)
    groups = -(-n // 128)
    rounds = -(-groups // min(groups, 256))          # a workgroup's trips through the group loop: the launch is as long as the longest
    mfma_per_wave = SKY_CHUNKS * MFMA_PER_CHUNK
    floor_ms = groups * 4 * mfma_per_wave * MFMA_CYCLES / SIMDS / (CLOCK_GHZ * 1e6)
    return dict(frame=[rows, cols], rays=n, flop_per_ray=SKY_FLOP_PER_RAY, max_abs_diff_sky_c=diff_c, max_abs_diff_sky_avg=diff_avg,
                sky_exact=n_, sky_features_torch=o_, **cmp_, ratio_kernel_over_torch=n_["median_ms"] / o_["median_ms"],
                groups_of_128_rays=groups, chunks_per_group=SKY_CHUNKS, mfma_per_wave_and_group=mfma_per_wave,
                fc1_padding_fraction_of_issue=(2 * MFMA_PER_CHUNK - 17 * 8) / mfma_per_wave, rounds_of_256_workgroups=rounds,
                matrix_floor_ms=floor_ms, matrix_floor_ms_whole_rounds=rounds * mfma_per_wave * MFMA_CYCLES / (CLOCK_GHZ * 1e6),
                clock_ghz_assumed=CLOCK_GHZ, matrix_issue_fraction=floor_ms / n_["median_ms"],
                tflops=n * SKY_FLOP_PER_RAY / n_["median_ms"] / 1e9)


def step_world(reps, warmup):
    torch, R, _ = _setup()
    import types
    from scenedreamer_amd import fused
    with torch.no_grad():
        hm = R.scene.current_height_map.to(R.dev, torch.float32).contiguous()
        sm = R.scene.current_semantic_map.to(R.dev, torch.float32).contiguous()
        on_dev = types.SimpleNamespace(current_height_map=hm, current_semantic_map=sm)
        new_fn, old_fn = (lambda: fused.world_exact(R, hm, sm)), (lambda: R._world_encoder_torch(on_dev))
        g_new, g_old = new_fn(), old_fn()
        diff = float((g_new - g_old).abs().max())
        same = bool(torch.equal(new_fn(), g_new))
        new, old = _time_pair(torch, new_fn, old_fn, reps, warmup)
    n_, o_, cmp_ = _summary(new, old)
    return dict(maps=list(hm.shape[2:]), global_enc=g_new.reshape(-1).tolist(), max_abs_diff_global_enc=diff, repeats_bit_for_bit=same,
                world_exact=n_, world_encoder_torch=o_, **cmp_, ratio_kernel_over_torch=n_["median_ms"] / o_["median_ms"])


def step_style(reps, warmup):
    torch, R, _ = _setup()
    sys.path.insert(0, ROOT)
    from scenedreamer_amd import fused, synth
    with torch.no_grad():
        style = torch.as_tensor(synth.make_style(8888)).to(R.dev)
        new_fn, old_fn = (lambda: fused.style_exact(R, style)), (lambda: R._style_mlp_torch(style))
        z_new, z_old = new_fn(), old_fn()
        diff = float((z_new - z_old).abs().max())
        new, old = _time_pair(torch, new_fn, old_fn, reps, warmup)
    n_, o_, cmp_ = _summary(new, old)
    return dict(styles=1, max_abs_diff_z=diff, max_abs_z=float(z_old.abs().max()), style_exact=n_, style_mlp_torch=o_, **cmp_,
                ratio_kernel_over_torch=n_["median_ms"] / o_["median_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_rung_timing.json"))
    ap.add_argument("--step", choices=["field", "frame", "cnn", "sky", "world", "style"], help="(internal) run one comparison in this process and print its JSON")
    ap.add_argument("--only", choices=["field", "frame", "cnn", "sky", "world", "style"], help="run this comparison only; the other keys of an existing --out file are kept")
    args = ap.parse_args()
    if args.step:
        res = {"field": step_field, "frame": step_frame, "cnn": step_cnn, "sky": step_sky, "world": step_world, "style": step_style}[args.step](args.reps, args.warmup)
        print("RESULT " + json.dumps(res))
        return 0
    if args.reps < 10 or args.warmup < 3:
        print("note: the comparison is defined on >= 10 timings after >= 3 warm-up runs", file=sys.stderr)
    rec = dict(config=dict(resolution_hw=list(HW), num_samples=NS, scene_size=SCENE, pose="pattern 0, pose 0 of maxstep 40", weights="synth.make_weights(0)",
                           style=8888, reps=args.reps, warmup=args.warmup, timing="HIP events, sides interleaved, one process per comparison"))
    if args.only and os.path.exists(args.out):
        with open(args.out) as f:
            rec = {**json.load(f), "config": rec["config"]}
    for step in ((args.only,) if args.only else ("field", "frame", "cnn", "sky", "world", "style")):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps),
               "--warmup", str(args.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"step {step} failed with exit status {r.returncode}; nothing more is started\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            return 1
        rec[step] = json.loads(line[-1][len("RESULT "):])
        print(step, json.dumps({k: v for k, v in rec[step].items() if not isinstance(v, dict)}), flush=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
