"""Roofline records of the dominant kernels, as bench.py reports them: work per launch, achieved rates, and the HBM traffic of the
newest committed PMC profile.  Plain functions of a renderer `R` (renderer.Renderer keeps the public names as delegations)."""
import json
import os

import torch

from . import build, fused, ops
from .timing import _time_ms

L2_PEAK_GBPS = 34500.0   # MI355X_MICROARCH.md: 4 MiB per XCD, ~34.5 TB/s aggregate
PMC_PROFILES = ("r06_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json", "r01_pmc_traffic.json")   # newest first


def measure_roofline(R, pose, resolution_hw, num_samples, mode, hbm_peak_gbps=8000.0, mfma_peak_tflops=2500.0):
    """Roofline records, timed with events on the launch stream (PyTorch's current stream).
    Algorithmic work per sample: SURVEY.md 8(d) -- 754 176 FLOP (render MLP), 16 404 B (grid gather, fused)
    / 16 916 B (un-fused).  Returns (dominant-kernel record, grid-sampler record)."""
    with torch.no_grad():
        vid, d2, rd, cam_res = R.cast_rays(pose, resolution_hw)
        n_rays = cam_res[0] * cam_res[1]
        vid, d2, rd = R.flat_rays(vid, d2, rd)
        cam_ori = torch.as_tensor(pose[0], dtype=torch.float32).to(R.dev)
        if mode == "unfused":
            n = min(n_rays, 1 << 16)
            depth, _, _ = R.place_samples(d2[:, :n], num_samples)
            depth = torch.nan_to_num(depth, nan=0.0, posinf=0.0, neginf=0.0)
            wc = rd[:n, None, :] * depth[:, :, None] + cam_ori
            delim = torch.tensor([float(v) for v in R.voxel_dims], device=R.dev)
            x5 = torch.cat([wc / delim * 2 - 1, R.global_enc[:, None, :].expand(n, num_samples, 2)], dim=-1)
            x5 = ((x5 + 1) / 2).reshape(-1, 5).contiguous()
            B = x5.shape[0]
            feats = torch.empty(R.grid_L, B, 8, device=R.dev)
            dummy = torch.empty(1, device=R.dev)
            w = R.w
            ms = _time_ms(lambda: ops.grid_encode_forward(x5, w["hash_encoder.embeddings"], w["hash_encoder.offsets"],
                                                          feats, B, 5, 8, R.grid_L, R.grid_S, 16, False, dummy,
                                                          0, False))
            achieved = B * 16916 / (ms * 1e-3) / 1e9
            # 32 corner rows x 32 B x 16 levels per sample really are requested, but from a 268 MB table whose coarse levels
            # stay in L2 / Infinity Cache: the rate is an on-die gather rate, bounded by the aggregate L2 bandwidth -- not
            # by HBM (dividing it by the HBM peak gave a "fraction" above 1)
            grid = {"bound": "l2", "kernel": "grid_fwd_quad_kernel<5,8> (drop-in GridEncoder.forward, 32-corner 5-D gather)", "achieved": achieved,
                    "peak": L2_PEAK_GBPS, "unit": "GB/s", "frac": achieved / L2_PEAK_GBPS, "traffic": None,
                    "effective_over_hbm_peak": achieved / hbm_peak_gbps,
                    "samples_per_launch": B, "algorithmic_bytes_per_sample": 16916, "avg_launch_ms": ms,
                    "note": "achieved = samples x 16 916 B (SURVEY 8(d), un-fused) / launch time: L2-level gather rate; peak = "
                            "aggregate L2 bandwidth (MI355X_MICROARCH.md: 34.5 TB/s); DRAM traffic not profiled for this kernel"}
            return grid, grid
        sky_c, sky_avg = R.sky(rd, "torch")
        B, ms_enc, per_sample, kernel = fused.time_encode_kernel(R, vid, d2, rd, cam_ori, num_samples)
        _, ms_mlp, hit, ev = fused.time_mlp_kernel(R, vid, d2, rd, cam_ori, sky_c, sky_avg, num_samples)
    return R.roofline_records(B, ms_enc, ms_mlp, hit, ev, kernel, hbm_peak_gbps, mfma_peak_tflops,
                              "HIP events around 5 back-to-back launches of each kernel on the whole padded frame, "
                              "outside the timed region")


def field_work(R, poses, resolution_hw, num_samples, apron="minimal"):
    """What the field kernel of the fused frame loop processes for these poses, averaged per frame (outside any timed
    region): samples per launch, fraction of rays that hit something, and the samples the kernel EVALUATES -- it visits only
    32-ray groups with a hit, and with early termination on (the default) it drops a group's remaining passes once all its
    rays are opaque: the executed passes are then counted by launching the kernel once per pose with a `passes` buffer."""
    o = R.apron_offset(apron)
    nch = -(-num_samples // 4)
    eps = fused.precision_profile(R)[1]
    B = hits = groups = evald = skipped = coloured = 0.0
    with torch.no_grad():
        for pose in poses:
            vid, d2, rd, (H0, W0) = R.cast_rays(pose, resolution_hw)
            hit = (vid.view(H0, W0, R.M)[o:H0 - o, o:W0 - o, 0] != 0).reshape(-1)
            n = hit.numel()
            g = fused.Window.crop(H0, W0, o).groups(hit, ragged=True).any(dim=1)          # the 32-ray groups as the launch forms them
            B += n * num_samples
            hits += float(hit.float().mean())
            groups += float(g.float().mean())
            if (eps > 0 or fused.colour_skip(R)) and fused.single_kernel(R):
                v, d, r = R.flat_rays(vid, d2, rd)
                sky_c, sky_avg = R.sky(r, "fused")
                win = fused.Window.crop(H0, W0, o)
                pa = torch.zeros(win.n_groups(ragged=True), dtype=torch.uint8, device=R.dev)
                cp = torch.zeros_like(pa)
                fused.field_render(R, v, d, r, torch.as_tensor(pose[0], dtype=torch.float32), sky_c, sky_avg, num_samples,
                                   passes=pa, window=win, colour_passes=cp)
                executed = int(pa.sum(dtype=torch.int64))
                evald += executed * 128
                coloured += int(cp.sum(dtype=torch.int64)) * 128
                skipped += int((pa > 0).sum()) * nch - executed
            else:
                evald += int(g.sum()) * 32 * nch * 4
                coloured += int(g.sum()) * 32 * nch * 4
    k = max(1, len(poses))
    return B / k, hits / k, dict(group_hit_fraction=groups / k, evaluated_samples=evald / k, passes_skipped_by_termination=skipped / k,
                                 passes_of_visited_groups=(evald / 128 + skipped) / k, colour_samples=coloured / k)


def roofline_records(R, B, ms_enc, ms_mlp, hit, ev, kernel, hbm_peak_gbps=8000.0, mfma_peak_tflops=2500.0, timing="",
                     field_kernel=False):
    """(field-MLP record, grid-sampler record) from per-launch work (B samples, hit fraction, evaluated samples in
    `ev`) and average launch durations.  field_kernel: ms_mlp is the duration of the single-kernel field (its launches
    contain the encode stage as well: the MLP's algorithmic FLOPs are divided by the WHOLE launch time)."""
    traffic, traffic_src = _profiled_traffic()
    ct, eps = fused.precision_profile(R)
    # ---- grid sampler (encode_kernel).  SURVEY 8(d): effective gather bandwidth = samples x 16 404 B / time.  The
    # gathers are served on-die (collapsed table: 8 x 32 B per level instead of 32 x 32 B, L2 / Infinity-Cache
    # hits), so that figure exceeds the HBM peak many times over: HBM does not bound this kernel, the L2-level
    # gather rate does.  All three rates are reported; `frac` is against the bound that applies (aggregate L2).
    n_gather = B * hit                                   # samples of rays that hit something: the others issue no gathers
    eff = B * 16404 / (ms_enc * 1e-3) / 1e9              # SURVEY 8(d) definition, every sample of the frame
    coll = n_gather * (4096 + 20 + 512) / (ms_enc * 1e-3) / 1e9   # bytes the kernel really moves at L2 level
    dram = traffic.get("encode_kernel")
    grid = {"bound": "l2", "kernel": kernel, "achieved": coll, "peak": L2_PEAK_GBPS, "unit": "GB/s",
            "frac": coll / L2_PEAK_GBPS, "avg_launch_ms": ms_enc, "samples_per_launch": B, "timing": timing,
            "samples_with_gathers": n_gather,
            "effective_GBps": eff, "effective_bytes_per_sample": 16404, "effective_over_hbm_peak": eff / hbm_peak_gbps,
            "collapsed_GBps": coll, "collapsed_bytes_per_sample": 4096 + 20 + 512,
            "dram_GBps_from_profile": (dram / (ms_enc * 1e-3) / 1e9) if dram else None,
            "dram_frac_of_hbm_peak_from_profile": (dram / (ms_enc * 1e-3) / 1e9 / hbm_peak_gbps) if dram else None,
            "traffic": dram, "traffic_source": traffic_src,
            "note": "effective = SURVEY 8(d): samples x 16 404 B (reference's 32-corner 5-D gather) / launch time -- "
                    "served on-die, hence far above the 8 TB/s HBM peak; collapsed = what this kernel moves at L2 level "
                    "(8 corners x 32 B x 16 levels + 20 B coords + 512 B feature write, only for rays that hit); "
                    "dram = FETCH+WRITE bytes of the PMC profile named in traffic_source / launch time (mostly the "
                    "feature write); peak = aggregate L2 bandwidth (MI355X_MICROARCH.md: 34.5 TB/s)"}
    # ---- field MLP.  Algorithmic FLOPs are counted on the samples the kernel EVALUATES (it skips 32-ray groups that
    # hit nothing and the passes early termination removes): samples of skipped groups are not work done.
    n_eval = ev["evaluated_samples"]
    # ... and the colour branch (fc_5, fc_6, fc_out_c: 294 912 of the 754 176 FLOP) only on the passes that ran it: passes whose
    # 128 samples all have volume-rendering weight exactly zero skip it (field.hip), and work not done is not counted
    n_col = ev.get("colour_samples", n_eval)
    flop_launch = n_eval * (754176 - 294912) + n_col * 294912
    ach_m = flop_launch / (ms_mlp * 1e-3) / 1e12
    # MFMA issue slots per pass / algorithmic (one f16 MFMA per product tile): 2208 for the 3-term split everywhere;
    # colour layers 2-term: 2 x 128 fewer; colour layers f16 + fp6: 2 x (384 - 192) fewer (an fp6 K = 64 MFMA takes the
    # issue time of one K = 16 f16 MFMA)
    issued = (2208 - (256 if ct == 2 else 384 if ct == 6 else 0)) / 736.0
    colour = {2: "2-term", 3: "3-term", 6: "f16 + MX-fp6 corrections"}[ct]
    name = ("field_kernel = mlp_kernel<FUSED>: sample placement + collapsed hash-grid lookup + MLP + compositing in ONE launch"
            if field_kernel else "mlp_kernel")
    mlp = {"bound": "mfma", "kernel": f"{name} (f16 MFMA, 3-term split, colour layers {colour}, f32 accumulate)",
           "achieved": ach_m, "peak": mfma_peak_tflops, "unit": "TFLOP/s", "frac": ach_m / mfma_peak_tflops,
           "traffic": traffic.get("field_kernel (mlp_kernel<0, 6, 1>)" if field_kernel else "mlp_kernel"), "traffic_source": traffic_src,
           "samples_per_launch": B, "samples_evaluated": n_eval, "algorithmic_flop_per_sample": 754176,
           "samples_with_colour_branch": n_col, "colour_branch_flop_per_sample": 294912, "algorithmic_flop_per_launch": flop_launch,
           "colour_passes_skipped_fraction": 1.0 - n_col / max(n_eval, 1.0),
           "achieved_counting_skipped_colour_branch": n_eval * 754176 / (ms_mlp * 1e-3) / 1e12,
           "frac_counting_skipped_colour_branch": n_eval * 754176 / (ms_mlp * 1e-3) / 1e12 / mfma_peak_tflops,
           "accounting": "`achieved` / `frac` count the FLOPs the launch EXECUTES; `*_counting_skipped_colour_branch` is SURVEY 8(d)'s "
                         "754 176 FLOP x every sample the launch finishes (a skipped colour branch is a finished sample: its colour is "
                         "multiplied by a weight that is exactly zero) -- the figure comparable with earlier rounds' `frac`",
           "avg_launch_ms": ms_mlp, "ray_hit_fraction": hit, "group_hit_fraction": ev["group_hit_fraction"],
           "early_termination_eps": eps, "passes_skipped_by_termination": ev["passes_skipped_by_termination"],
           "issued_over_algorithmic": issued, "issued_frac_of_peak": ach_m * issued / mfma_peak_tflops,
           "timing": timing,
           "achieved_counting_skipped_samples": B * 754176 / (ms_mlp * 1e-3) / 1e12,
           "note": ("the launch ALSO contains the encode stage of its samples (sample placement + 8-corner gathers of 16 levels, "
                    "the work of the former encode_kernel): its time is in the denominator, its bytes are not in the numerator; "
                    if field_kernel else "") +
                   "achieved = (samples evaluated x 459 264 FLOP of trunk + density head + samples whose pass ran the colour branch x "
                   "294 912 FLOP) / launch time (skipped sky groups, terminated passes and skipped colour branches are not "
                   "counted as work); the kernel issues `issued_over_algorithmic` MFMA slots per algorithmic product (hi*hi + "
                   "lo*hi + hi*lo: plain f16 misses the 1e-3 bound 17x; in the colour layers the two corrections run as "
                   "block-scaled fp6 at 4x the rate); traffic = HBM bytes per launch from the "
                   "PMC profile named in traffic_source (a separate rocprofv3 --pmc run, not this process)"}
    return mlp, grid


def _profiled_traffic():
    """(HBM bytes per launch by kernel, source label) from the newest committed PMC profile: bench.py cannot run rocprofv3 on
    itself, so `traffic` in the roofline records is NOT measured in the bench process -- the label says so.  A profile is
    used only if it was taken on THESE kernel sources: tools/pmc_traffic.py stores the digest of csrc/*.hip + the header
    (build._digest(), the same value as lib/libsdnative.stamp) and a profile whose digest differs from the current
    sources' -- or that predates the digest field -- yields no traffic figure and a label that says why."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cur = build._digest()
    why = None
    for name in PMC_PROFILES:
        try:
            with open(os.path.join(root, "profiles", name)) as f:
                d = json.load(f)
            per = {k: v["traffic"] for k, v in d["per_launch_bytes"].items()}
        except (OSError, KeyError, ValueError):
            continue
        if d.get("csrc_digest") != cur:
            why = why or (f"profiles/{name} is STALE (taken at build {d.get('commit', 'unrecorded')}, kernel-source digest "
                          f"{str(d.get('csrc_digest'))[:12]} != current {cur[:12]}): no traffic figure reported")
            continue
        return (per, f"profiles/{name} (rocprofv3 --pmc passes of tools/frame_once.py, build {d.get('commit', 'unrecorded')}, "
                     f"kernel-source digest {cur[:12]} = this build; not measured in this run)")
    return {}, why
