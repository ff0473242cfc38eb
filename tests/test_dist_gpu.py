"""The GPU-side multi-rank paths executed under world_size 2 on ONE MI355X: two processes share cuda:0 and talk over gloo
(device tensors are staged through host memory by scenedreamer_amd.dist -- RCCL needs one GPU per rank, which a one-GPU box
cannot give; the NCCL/RCCL route differs only in the transport of the same collectives).  Exercised with the REAL
Renderer: the compact uint8 scene volume broadcast into device memory with its integrity check, frames of a trajectory
sharded f -> rank f % 2, and one frame rendered tile-parallel (row bands, all_reduce of the frame-wide sky sums, strips
gathered on rank 0).  Everything must equal what a single process renders from the same state."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

HW, NS, SCENE, FRAMES, TP_POSE = (96, 136), 12, 256, 4, 5


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _state():
    from scenedreamer_amd import synth
    return synth.make_scene(SCENE, 3407, device="cuda"), synth.make_weights(0), synth.make_style(8888)


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from scenedreamer_amd import camera
        from scenedreamer_amd import dist as sdist
        from scenedreamer_amd.renderer import Renderer
        dev = torch.device("cuda", 0)
        scene, weights, style = _state() if rank == 0 else (None, None, None)
        stats = {}
        sc, w, st = sdist.broadcast_state(scene, weights, style, dev, src=0, compact=True, stats=stats)
        assert getattr(sc, "voxel_u8", None) is not None and sc.voxel_u8.is_cuda and sc.voxel_u8.dtype == torch.uint8
        R = Renderer(w, sc, dev)
        R.set_style(st)
        poses = camera.eval_camera_poses(sc, maxstep=8)
        cal = sdist.agree_cnn_precision(R, poses[0], HW, NS)
        mine = sdist.shard_frames(range(FRAMES), rank, world)
        imgs = {f: im.clone().cpu().numpy() for f, im in zip(mine, R.render_frames([poses[f] for f in mine], HW, NS, mode="fused"))}
        tp = sdist.render_frame_tile_parallel(R, poses[TP_POSE], HW, NS, mode="fused")
        q.put((rank, imgs, None if tp is None else tp.cpu().numpy(), stats["scene_volume_bytes"], cal))
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_equal_single_process():
    from scenedreamer_amd import camera
    from scenedreamer_amd import dist as sdist
    from scenedreamer_amd import scene as scene_mod
    from scenedreamer_amd.renderer import Renderer
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    # the single-process reference, meanwhile, from the same synthetic state
    scene, weights, style = _state()
    R = Renderer(weights, scene_mod.to_compact(scene), "cuda")
    R.set_style(style)
    poses = camera.eval_camera_poses(scene, maxstep=8)
    cal = sdist.agree_cnn_precision(R, poses[0], HW, NS)                # (no process group here: the local decision)
    single = [R.render_frame(poses[f], HW, NS, mode="fused").cpu().numpy() for f in range(FRAMES)]
    tp_single = R.render_frame(poses[TP_POSE], HW, NS, mode="fused").cpu().numpy()
    res = sorted((q.get(timeout=600) for _ in range(world)), key=lambda r: r[0])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    assert res[0][3] == res[1][3] == scene.voxel_t.numel()                  # one byte per cell travelled, not four
    assert res[0][4]["terms3x3"] == res[1][4]["terms3x3"] == cal["terms3x3"] and res[0][4]["agreed_over_ranks"] == 2
    got = {}
    for _, imgs, _, _, _ in res:
        got.update(imgs)
    assert sorted(got) == list(range(FRAMES)) and sorted(res[0][1]) == [0, 2] and sorted(res[1][1]) == [1, 3]
    for f in range(FRAMES):
        np.testing.assert_array_equal(got[f], single[f])                    # sharded frames: the same bits
    assert res[1][2] is None and res[0][2].shape == tp_single.shape
    # row bands vs full frame: only the summation order of the sky mean differs (~1e-7 on net_out); with 1-term 3x3 layers
    # that can flip an f16 rounding in the CNN, so the bound is the CNN's own error level (test_row_bands_equal_full_frame)
    d = float(np.abs(res[0][2] - tp_single).max())
    print(f"tile-parallel over 2 ranks vs single process: max abs diff {d:.2e} (CNN 3x3 terms {cal['terms3x3']})")
    assert d < (5e-4 if cal["terms3x3"] != 3 else 1e-6)


def _worker8(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from scenedreamer_amd import camera
        from scenedreamer_amd import dist as sdist
        from scenedreamer_amd.renderer import Renderer
        dev = torch.device("cuda", 0)
        scene, weights, style = _state() if rank == 0 else (None, None, None)
        sc, w, st = sdist.broadcast_state(scene, weights, style, dev, src=0, compact=True)
        R = Renderer(w, sc, dev)
        R.set_style(st)
        poses = camera.eval_camera_poses(sc, maxstep=8)
        gates = sdist.agree_precision(R, poses[0], HW, NS)
        mine = sdist.shard_frames(range(8), rank, world)
        imgs = {f: im.clone().cpu().numpy() for f, im in zip(mine, R.render_frames([poses[f] for f in mine], HW, NS, mode="fused"))}
        stats = {}
        tp = sdist.render_frame_tile_parallel(R, poses[TP_POSE], HW, NS, mode="fused", stats=stats)
        q.put((rank, imgs, None if tp is None else tp.cpu().numpy(), stats, {k: (v or {}).get("agreed_over_ranks") for k, v in gates.items()}))
    finally:
        dist.destroy_process_group()


def test_eight_ranks_on_one_gpu_equal_single_process():
    """The shapes the 8-GPU node will run -- 8 ranks: state broadcast (a table whose size is not a multiple of 8 included),
    job-wide precision gates, frames f -> rank f % 8, and ONE frame as 8 work-balanced row bands with the minimal apron --
    with 8 processes sharing this box's GPU over gloo.  Sharded frames equal a single process bit for bit; the banded frame
    equals the full frame to the CNN's error level; the bands tile the frame and follow the per-row work estimate."""
    from scenedreamer_amd import camera
    from scenedreamer_amd import dist as sdist
    from scenedreamer_amd import scene as scene_mod
    from scenedreamer_amd.renderer import Renderer
    world, port = 8, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker8, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    scene, weights, style = _state()
    R = Renderer(weights, scene_mod.to_compact(scene), "cuda")
    R.set_style(style)
    poses = camera.eval_camera_poses(scene, maxstep=8)
    sdist.agree_precision(R, poses[0], HW, NS)
    single = [R.render_frame(poses[f], HW, NS, mode="fused").cpu().numpy() for f in range(8)]
    tp_single = R.render_frame(poses[TP_POSE], HW, NS, mode="fused").cpu().numpy()
    costs = R.row_costs(poses[TP_POSE], HW)
    res = sorted((q.get(timeout=900) for _ in range(world)), key=lambda r: r[0])
    for p in procs:
        p.join(180)
        assert p.exitcode == 0
    for r, imgs, tp, stats, agreed in res:
        assert sorted(imgs) == [r] and agreed == {"cnn": 8, "field": 8}
        np.testing.assert_array_equal(imgs[r], single[r])
        assert (tp is None) == (r != 0)
        assert stats["bands"] == res[0][3]["bands"] and len(stats["band_ms"]) == 8 and min(stats["band_ms"]) > 0
    bands = res[0][3]["bands"]
    assert bands == sdist.balanced_row_bands(costs, 8) and bands[0][0] == 0 and bands[-1][1] == HW[0]
    assert all(a[1] == b[0] for a, b in zip(bands, bands[1:])) and all(b - a >= sdist.MIN_BAND_ROWS for a, b in bands)
    d = float(np.abs(res[0][2] - tp_single).max())
    print(f"tile-parallel over 8 ranks (bands {bands}, band_ms {[round(x, 2) for x in res[0][3]['band_ms']]}) vs single process: max abs diff {d:.2e}")
    assert d < 5e-4


def test_bench_py_self_launches_for_gpus_n():
    """`python bench.py --gpus 2 ...` as a PLAIN command (no launcher, no WORLD_SIZE): it re-executes itself under
    torch.distributed.run and reports n_gpus 2; a WORLD_SIZE that contradicts --gpus is an error, not a smaller job."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    bench = [sys.executable, os.path.join(root, "bench.py")]
    small = ["--steps", "2", "--warmup", "1", "--scene-size", "256", "--height", "96", "--width", "136", "--samples", "12", "--no-extras"]
    r = subprocess.run(bench + ["--gpus", "2", "--backend", "gloo"] + small, capture_output=True, text=True, timeout=600, cwd=root, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0])["n_gpus"] == 2
    bad = subprocess.run(bench + ["--gpus", "4", "--backend", "gloo"] + small, capture_output=True, text=True, timeout=120, cwd=root,
                         env=dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"))
    assert bad.returncode != 0 and "--gpus 4 but WORLD_SIZE=1" in bad.stderr
    if torch.cuda.device_count() == 1:          # RCCL: one GPU per rank, or an error -- never a silently smaller job
        nccl = subprocess.run(bench + ["--gpus", "2", "--backend", "nccl"] + small, capture_output=True, text=True, timeout=300, cwd=root, env=env)
        assert nccl.returncode != 0 and "only 1 GPU(s) visible" in nccl.stderr


def _nccl_worker(port, q):
    """world_size 1 on the RCCL backend: no peer to talk to, but every collective dist.py issues is dispatched to RCCL with the
    dtypes it uses -- an op or dtype the backend does not implement raises here instead of on the first multi-GPU job."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        from scenedreamer_amd import dist as sdist
        dev = torch.device("cuda", 0)
        done = []
        for dt in (torch.uint8, torch.int32, torch.int64, torch.float32):          # volume, ids / palette, heightmap, weights
            t = (torch.arange(1 << 12, device=dev) % 251).to(dt)
            assert sdist._scatter_supported(t) and not sdist._host_staged(t)
            mine = torch.empty_like(t)
            dist.scatter(mine, [t.clone()], src=0)
            outs = [torch.empty_like(t)]
            dist.all_gather(outs, mine)
            dist.broadcast(t, 0)
            assert torch.equal(outs[0], t)
            done.append(str(dt))
        sums = torch.tensor([3, -5, 1 << 40], dtype=torch.int64, device=dev)
        lo, hi = sums.clone(), sums.clone()
        sdist.all_reduce(lo, op=dist.ReduceOp.MIN)
        sdist.all_reduce(hi, op=dist.ReduceOp.MAX)
        assert torch.equal(lo, hi)
        red = torch.arange(65, dtype=torch.float64, device=dev)
        sdist.all_reduce(red)                                                       # the sky sums of the tile-parallel frame
        got = sdist.gather(torch.ones(1, 3, 8, 16, device=dev), dst=0)              # its image strips
        assert len(got) == 1 and float(got[0].sum()) == 3 * 8 * 16
        meta = [[("name", (2, 3), "float32")]]
        dist.broadcast_object_list(meta, src=0)
        dist.barrier()
        # the whole broadcast of a (small) state through the production entry point
        from scenedreamer_amd import synth
        sc, w, st = sdist.broadcast_state(synth.make_scene(64, 11, device=dev), synth.make_weights(0, grid_log2_hashmap=10),
                                          synth.make_style(8888), dev, src=0, compact=True)
        assert sc.voxel_u8.is_cuda and all(v.is_cuda for v in w.values())
        q.put(("ok", done))
    except Exception as e:  # noqa: BLE001 -- reported to the parent, which fails the test with the message
        q.put(("error", f"{type(e).__name__}: {e}"))
    finally:
        dist.destroy_process_group()


def test_rccl_backend_accepts_every_collective_dist_uses():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_nccl_worker, args=(_free_port(), q))
    p.start()
    status, info = q.get(timeout=300)
    p.join(60)
    assert status == "ok", info
    assert len(info) == 4 and p.exitcode == 0


@pytest.mark.parametrize("bench_mode", ["frames", "tile-parallel"])
def test_bench_py_multi_rank_path_two_ranks_on_one_gpu(bench_mode):
    """bench.py exactly as the driver launches it for N > 1 (`python -m torch.distributed.run --nproc-per-node N ... bench.py
    --gpus N`), with two ranks sharing the box's one GPU over gloo (`--backend gloo`; the production backend is RCCL with one
    GPU per rank): state broadcast, the job-wide CNN precision decision, sharded / tile-parallel frames, barriers, MAX over
    ranks of the elapsed time, ONE JSON line from rank 0.  Small workload: the numbers mean nothing, the path is what is run."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--backend", "gloo", "--scene-size", "256", "--height", "96", "--width", "136", "--samples", "12", "--no-extras",
           "--bench-mode", bench_mode, "--full"]
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        detail_path = os.path.join(tmp, "detail.json")
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root, env=dict(os.environ, SDN_BENCH_DETAIL=detail_path))
        assert r.returncode == 0, r.stderr[-3000:]
        full = json.load(open(detail_path))          # the full record (bench_detail.json); stdout carries its compact extract
    assert r.stdout.count("\n") == 1 and len(r.stdout) < 6144, r.stdout[-2000:]          # ONE line, nothing else, small
    d = json.loads(r.stdout)
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["value"] > 0 and d["unit"] == "frames/s"
    assert d["scaling"] == ("strong" if bench_mode == "tile-parallel" else "weak")
    assert d["config"]["dist_backend"].startswith("gloo, 2 ranks on 1 GPU")
    assert d["config"]["parallelism"] == ("row bands x2" if bench_mode == "tile-parallel" else "frames x2")
    if bench_mode == "tile-parallel":
        b = full["config"]["bands"]
        assert len(b["rows"]) == 2 and b["rows"][0][0] == 0 and b["rows"][1][1] == 96 and len(b["band_ms"]) == 2 and b["imbalance_max_over_mean"] >= 1.0
        assert len(d["band_ms"]) == 2 and d["imbalance"] >= 1.0
    if bench_mode == "frames":
        assert full["broadcast"]["scene_volume_bytes"] > 0 and "cpu_baseline" not in d      # compact volume; no CPU leg at N > 1
        assert d["broadcast_s"] > 0


def test_bench_py_single_gpu_stdout_is_one_small_json_line():
    """The failure of round 5, end to end: `bench.py` with EVERY leg on (CPU baseline, floor / style-cost records, the unmodified
    reference loop with its own "Rendering frame ..." prints, early-termination record) must leave exactly one line on stdout --
    parseable, below the 6 KB limit, carrying `roofline` and (when the CPU leg ran) `cpu_baseline` -- and the full record in the
    detail file.  Small workload: the numbers mean nothing, the plumbing is what is run."""
    import json
    import subprocess
    import sys
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as tmp:
        detail_path = os.path.join(tmp, "detail.json")
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--scene-size", "256",
               "--height", "96", "--width", "136", "--samples", "12", "--dropin-frames", "3", "--cpu-budget-s", "5", "--full"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root,
                           env=dict(os.environ, SDN_BENCH_DETAIL=detail_path, SDN_CPU_THREADS="16"))
        assert r.returncode == 0, r.stderr[-3000:]
        full = json.load(open(detail_path))
    assert r.stdout.endswith("\n") and r.stdout.count("\n") == 1 and len(r.stdout.encode()) < 6144, r.stdout[-1500:]
    d = json.loads(r.stdout)
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 2 and d["value"] > 0 and d["unit"] == "frames/s" and d["higher_is_better"] is True
    assert abs(d["ms_per_step"] * d["value"] - 1000.0) < 1.0                              # one frame per step
    roof = d["roofline"]
    assert roof["bound"] == "mfma" and 0 < roof["frac"] < 1 and abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3 and roof["avg_launch_ms"] > 0
    assert d["cpu_baseline"]["kind"] in ("reference", "port") and d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["cores"] >= 1
    assert d["precision"]["max_abs_err"] < d["precision"]["bound"] == 1e-3
    for k in ("floor_frames_per_s", "colour_skip_off_frames_per_s", "style_setup_ms", "calibration_ms", "first_frame_ms", "trajectory40_frames_per_s"):
        assert d[k] > 0, k
    if "skipped" not in (full.get("dropin") or {}):
        assert d["dropin_frames_per_s"] > 0
        assert "Rendering frame" in r.stderr and "Rendering frame" not in r.stdout      # the reference loop's prints went to stderr
    # the detail file is the full record: everything on the line is in it, plus what the line leaves out
    assert full["value"] == pytest.approx(d["value"], rel=1e-4) and "gates" in full["precision"] and "timing" in full["roofline"]
    assert (full["floor"]["passes_skipped_by_termination"], full["floor"]["colour_branch_skipped_fraction"]) == (0.0, 0.0)


def test_bench_py_plain_run_times_steps_and_dumps_the_last_frame():
    """A plain run (no --full) is the headline alone: --steps timed frames, the result line's head keys, none of the records
    that --full measures outside the timed region.  --dump-outputs writes the LAST timed frame: the image of orbit frame
    warmup + steps - 1 as bench.py's loop renders it in this process, for two different --steps.  A config-4 run with an
    explicit --steps that does not cover the orbit is not labelled as config 4."""
    import json
    import subprocess
    import sys
    import tempfile
    from scenedreamer_amd import camera, synth
    from scenedreamer_amd import scene as scene_mod
    from scenedreamer_amd.renderer import Renderer
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hw, ns, warmup = (96, 136), 12, 1
    small = ["--scene-size", "256", "--height", str(hw[0]), "--width", str(hw[1]), "--samples", str(ns)]

    def bench(tmp, *args):
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", *small, *args]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root,
                           env=dict(os.environ, SDN_BENCH_DETAIL=os.path.join(tmp, "detail.json")))
        assert r.returncode == 0, r.stderr[-3000:]
        assert r.stdout.count("\n") == 1, r.stdout[-1500:]
        return json.loads(r.stdout)

    dumped, lines = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for steps in (3, 4):
            out = os.path.join(tmp, f"out{steps}")
            lines[steps] = bench(tmp, "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", out)
            assert os.listdir(out) == ["image.npy"]
            dumped[steps] = np.load(os.path.join(out, "image.npy"))
        c4 = bench(tmp, "--config", "4", "--steps", "2", "--warmup", "1")
        c4_workload = json.load(open(os.path.join(tmp, "detail.json")))["config"]["workload"]     # (the line cuts it to 120 characters)
    for steps, d in lines.items():
        assert d["steps"] == steps and d["warmup"] == warmup and d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"]
        assert len(d["frame_ms_p10_p50_p90"]) == 3 and d["value"] > 0 and d["ms_per_step"] > 0
        assert d["roofline"] is None and not d.get("stage_ms")
        assert not {"cpu_baseline", "roofline_rvip", "roofline_cnn", "floor_frames_per_s", "dropin_frames_per_s"} & set(d)
    assert c4["steps"] == 2 and c4["scaling"] == "weak" and "baseline_config" not in c4["config"]
    assert c4_workload.endswith(", 2 of the 256 orbit frames"), c4_workload

    # bench.py's renderer and loop for the same arguments: compact volume, seeded weights / style, frame k = orbit pose 2k of 40,
    # the warm-up frames and then the timed trajectory through render_frames (a fresh renderer per run, as each run is a process)
    dev = torch.device("cuda", 0)
    scene = scene_mod.to_compact(synth.make_scene(256, 3407, device=dev))
    weights = synth.make_weights(0)
    poses = camera.eval_camera_poses(scene, maxstep=40)
    pose = lambda k: poses[(2 * k) % 40]
    for steps, img in dumped.items():
        R = Renderer(weights, scene, dev)
        R.set_style(synth.make_style(8888))
        for _ in R.render_frames([pose(k) for k in range(warmup)], hw, ns, mode="fused", apron="minimal"):
            pass
        frames = [im.clone() for im in R.render_frames([pose(warmup + k) for k in range(steps)], hw, ns, mode="fused", apron="minimal")]
        last, before = frames[-1].cpu().numpy(), frames[-2].cpu().numpy()
        assert img.dtype == np.float32 and img.shape == (1, 3) + hw and np.isfinite(img).all()
        err_last, err_before = float(np.abs(img - last).max()), float(np.abs(img - before).max())
        print(f"--steps {steps}: dump vs last timed frame {err_last:.2e}, vs the frame before it {err_before:.2e}")
        assert err_last < 1e-4 < err_before
