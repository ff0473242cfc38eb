"""The per-style precision gates: what the reduced-precision choices of the fused path cost for the current weights and style,
measured against the fp32 op sequence, and the decisions that follow.  Plain functions of a renderer `R` (renderer.Renderer keeps
the public names as delegations; cnn_window_gate also serves modules.Backend through PrecisionState.mfma_cnn).  The bounds are
read from precision.py at call time."""
import os
import time
import warnings

import torch
import torch.nn.functional as F

from . import fused
from . import precision as P
from .cnn import CNN_LADDER, form_key


def calibrate_style(R, pose, resolution_hw, num_samples, more_poses=()):
    """calibrate_one on `pose` and on every pose of `more_poses` (the trajectory loop adds the middle pose of the trajectory:
    the errors depend on what the camera sees), the measurements combined with MAX, then adopt_precision -- the decision a
    multi-rank job reaches by reducing the same measurements over its ranks (dist.agree_precision)."""
    meas = R.calibrate_one(pose, resolution_hw, num_samples)
    for p2 in more_poses:
        m2 = R.calibrate_one(p2, resolution_hw, num_samples)
        for k, v in m2.items():
            if isinstance(v, dict):
                meas[k] = {kk: max(vv, meas[k].get(kk, vv)) if isinstance(vv, float) else vv for kk, vv in v.items()}
            elif isinstance(v, float):
                meas[k] = max(v, meas.get(k, v))
        meas["poses"] = meas.get("poses", 1) + 1
    return R.adopt_precision(meas)


def calibrate_one(R, pose, resolution_hw, num_samples, crop_px=None):
    """Measure END TO END, for the CURRENT weights and style, what the reduced-precision choices of the fused path cost, and
    decide.  A window of one frame (`pose`) is rendered by the reference's op sequence in fp32 (field_unfused + render_cnn:
    PyTorch fp32 + the drop-in HIP ops -- the path the CPU-oracle tests validate; samples placed by the fused kernel's own
    device function, see field_unfused) and by the candidates; the cheapest candidate inside the bounds is adopted:

      colour layers fc_5 / fc_6: f16 + MX-fp6 corrections (colour_terms 6) if net_out stays within COLOUR_AUTO_BOUND of the
        3-term evaluation, else the 3-term split;
      the fused field (3-term f16 split, f32 accumulate): net_out against the fp32 net_out, bound FIELD_AUTO_BOUND -- above
        it the style is served by the fp32 op sequence (`path: "unfused"`): slow, but inside the tolerance;
      render CNN 3x3 layers: the cheapest rung of cnn.CNN_LADDER -- all four layers ONE f16 product; conv3b 3-term ("1113");
        conv3a + conv3b 3-term ("1133"); all 3-term -- whose image stays within CNN_AUTO_BOUND of the 3-term image AND whose
        MEASURED total error against the fp32 image (field error included) stays within IMAGE_AUTO_BOUND; if not even the
        3-term image is within IMAGE_AUTO_BOUND, the fp32 path.

    The window (round 6; `crop_px`, default CAL_CROP = 256 output pixels square, 0 = the whole frame as in rounds 4-5): the fp32
    twin of a whole 960x540x24 frame is 0.25 s of GPU time per pose -- with two poses more than half of a 40-frame trajectory
    (0.72 s).  The field is evaluated per ray and the CNN's receptive radius is 4 px, so any window of the frame is a valid
    sample of both; the window is put where the frame's content changes most from pixel to pixel (box sum of first-hit block-id
    changes and depth steps, straight from the ray caster's output: silhouettes and material boundaries, where net_out -- and
    with it the f16 rounding of the one-product 3x3 layers -- varies most).  A maximum over 1/8 of the pixels under-estimates
    the frame's (extreme-value growth ~ sqrt(2 ln N): 1.08 here), so every window-measured maximum is charged times
    CAL_CROP_FACTOR = 1.15 before it meets a bound (`raw` keeps the measured values).  The fused sky MLP runs on every ray of
    the padded frame (its frame mean needs them), its fp32 twin on the window's rays.

    The errors depend on the loaded weights (the density head amplifies hidden-activation error; 3x3 gains compound over
    four layers): tests/test_precision_gates_gpu.py scales them until every gate closes.  Explicit settings (set_precision,
    SDN_MLP_COLOUR_TERMS, SDN_CNN_TERMS) are measured but not overridden.  Returns the measurements; calibrate_style turns
    them into the records `field_gate`, `cnn_calibration` (bench.py writes both to bench_detail.json)."""
    H, W = resolution_hw
    if H * W > P.CAL_MAX_PIXELS:
        f = (P.CAL_MAX_PIXELS / float(H * W)) ** 0.5
        H, W = max(8, int(H * f)), max(8, int(W * f))
    if crop_px is None:
        crop_px = int(os.environ.get("SDN_CAL_CROP", P.CAL_CROP))
    crop = R.pad // 2
    phases, _t = {}, [None]

    def tick(name):          # SDN_CAL_TIMING=1: wall clock per phase (synchronised) -> meas["timing_ms"] (tools/cal_timing.py)
        if os.environ.get("SDN_CAL_TIMING"):
            torch.cuda.synchronize()
            now = time.perf_counter()
            if _t[0] is not None and name:
                phases[name] = phases.get(name, 0.0) + 1000.0 * (now - _t[0])
            _t[0] = now
    with torch.no_grad():
        tick(None)
        vid, d2, rd, (H0, W0) = R.cast_rays(pose, (H, W))
        vid, d2, rd = R.flat_rays(vid, d2, rd)
        ori = torch.as_tensor(pose[0], dtype=torch.float32).reshape(3)
        tick("cast rays")
        inner = (lambda im: im[:, :, crop:-crop, crop:-crop]) if crop else (lambda im: im)
        # ---- the window: where the frame's content changes most from pixel to pixel -- silhouettes, material boundaries, depth
        #      steps of the first hit (from the ray caster's output: no field evaluation needed) -- is where net_out varies most
        explicit_ct = R.explicit_colour_terms()
        saved = R.colour_terms
        Hc, Wc, r0, c0 = H0, W0, 0, 0
        windowed = bool(crop_px) and (H0 > crop_px + R.pad + 32 or W0 > crop_px + R.pad + 32)
        if windowed:
            Hc, Wc = min(H0, crop_px + R.pad), min(W0, crop_px + R.pad)
            v0 = vid[:, 0].view(H0, W0)
            t0 = torch.nan_to_num(d2[0][:, 0], nan=-64.0).view(H0, W0)
            g = torch.zeros(H0, W0, device=R.dev)
            g[1:] += (v0[1:] != v0[:-1]).float() + ((t0[1:] - t0[:-1]).abs() > 1.0).float()
            g[:, 1:] += (v0[:, 1:] != v0[:, :-1]).float() + ((t0[:, 1:] - t0[:, :-1]).abs() > 1.0).float()
            g += 1e-3 * (v0 != 0).float()           # (ties: prefer ground to sky)
            r0, c0 = _busiest_window(g, Hc, Wc)
            del g
        tick("window choice")
        nc = Hc * Wc
        cut = lambda t, last: t.view(H0, W0, last)[r0:r0 + Hc, c0:c0 + Wc].reshape(nc, last).contiguous()
        if windowed:
            vid_c, rd_c = cut(vid, R.M), cut(rd, 3)
            d2_c = torch.stack([cut(d2[0], R.M), cut(d2[1], R.M)]).contiguous()
        else:
            vid_c, rd_c, d2_c = vid, rd, d2
        # ---- the sky MLP: hidden layers as f16 + fp6 corrections if its features stay within SKY_AUTO_BOUND of the fp32 ones.
        #      The fused forms run on every ray of the padded frame (the frame mean needs them; 0.8 ms each); the fp32 twin on the
        #      window's rays, its frame mean taken from the 3-term evaluation (4e-6 per feature before averaging 564 k of them)
        ori_dev = ori.to(R.dev)
        explicit_sky = R.explicit_sky_terms()
        sky32_c = R.sky_features(rd_c)
        R.sky_terms_auto = None
        sky_c, sky_avg = fused.sky_fused(R, rd)
        savg32 = sky_avg.reshape(1, 64) if (windowed and fused.sky_terms(R) == 3) else None
        cut_sky = (lambda t: cut(t, 64)) if windowed else (lambda t: t)
        k_ev = P.CAL_CROP_FACTOR if windowed else 1.0       # window maxima are charged with the extreme-value factor
        sky_err = {fused.sky_terms(R): float((cut_sky(sky_c) - sky32_c).abs().max()) * k_ev}
        if explicit_sky is None:
            R.sky_terms_auto = 6
            c6, a6 = fused.sky_fused(R, rd)
            sky_err[6] = float((cut_sky(c6) - sky32_c).abs().max()) * k_ev
            if sky_err[6] <= P.SKY_AUTO_BOUND:
                sky_c, sky_avg = c6, a6
            else:
                R.sky_terms_auto = None
        if savg32 is None:      # whole frame (or an explicit fp6 sky): the fp32 mean over every ray
            savg32 = (sky32_c if not windowed else R.sky_features(rd)).mean(dim=0, keepdim=True)
        skyc_c = cut_sky(sky_c)
        tick("sky (fp32 twin on the window, 2 fused forms on the frame)")
        # ---- the fp32 twin of the window
        ref_no = torch.cat([R.field_unfused(vid_c[r:r + P.CAL_CHUNK], d2_c[:, r:r + P.CAL_CHUNK].contiguous(), rd_c[r:r + P.CAL_CHUNK], ori_dev,
                                            sky32_c[r:r + P.CAL_CHUNK], savg32, num_samples, placement="kernel")
                            for r in range(0, nc, P.CAL_CHUNK)], dim=0)
        tick("fp32 field twin")
        ref_img = inner(R.render_cnn(ref_no.view(1, Hc, Wc, 64)))
        tick("fp32 CNN twin")
        # ---- the fused field on the window's rays
        no = {}
        try:
            for ct in ((explicit_ct,) if explicit_ct is not None else (6, 3)):
                R.colour_terms = ct
                no[ct] = fused.field_fused(R, vid_c, d2_c, rd_c, ori, skyc_c, sky_avg, num_samples)
        finally:
            R.colour_terms = saved
        raw = {"field_err": {ct: float((v - ref_no).abs().max()) for ct, v in no.items()}}
        meas = {"field_err": {ct: e * k_ev for ct, e in raw["field_err"].items()}, "sky_err": sky_err, "explicit_sky": explicit_sky}
        if explicit_ct is None:
            raw["colour_diff"] = float((no[6] - no[3]).abs().max())
            meas["colour_diff"] = raw["colour_diff"] * k_ev
        ct = explicit_ct if explicit_ct is not None else (6 if meas["colour_diff"] <= P.COLOUR_AUTO_BOUND else 3)
        tick("fused field, 2 colour forms")
        # ---- the render CNN on the chosen field's output
        explicit_t = R.explicit_cnn_terms()       # "1", "3" or a per-layer form like "1113"
        x = no[ct].view(1, Hc, Wc, 64)
        if explicit_t is not None:
            explicit_t = form_key(explicit_t)
        # (every rung is measured, whichever is adopted: adopt_precision must be a function of `meas` alone, so that the ranks of
        #  a multi-GPU job can reduce the measurements and reach the same decision)
        imgs = {t: inner(R._cnn_form(t)(x)).clone() for t in ((explicit_t,) if explicit_t is not None else CNN_LADDER)}
        raw["image_err"] = {t: float((im - ref_img).abs().max()) for t, im in imgs.items()}
        meas["image_err"] = {t: e * k_ev for t, e in raw["image_err"].items()}
        if explicit_t is None:
            raw["cnn_diffs"] = {t: float((imgs[t] - imgs[3]).abs().max()) for t in CNN_LADDER if t != 3}
            meas["cnn_diffs"] = {t: e * k_ev for t, e in raw["cnn_diffs"].items()}
            meas["cnn_diff"] = meas["cnn_diffs"][1]
        tick("MFMA CNN rungs")
        if windowed:        # (a window's activation planes are not the frame's: drop them, the packed weights stay)
            R._drop_cnn_planes(Hc, Wc)
    meas.update(explicit_colour=explicit_ct, explicit_cnn=explicit_t, pixels=int((Hc - 2 * crop) * (Wc - 2 * crop)), rays=int(nc), samples_per_ray=int(num_samples),
                frame=f"{W}x{H} (+{R.pad}-px apron), {num_samples} samples/ray" +
                      (f"; window {Wc - 2 * crop}x{Hc - 2 * crop} at ({r0},{c0}), maxima x {P.CAL_CROP_FACTOR}" if windowed else ""),
                window=([r0, c0, Hc, Wc] if windowed else None), raw=raw if windowed else None)
    if phases:
        meas["timing_ms"] = phases
    return meas


def adopt_precision(R, meas):
    """Decisions that follow from calibrate_style's measurements (a pure function of `meas` plus R.fallback and R.cnn_auto_bound:
    dist.agree_precision reduces the measurements over the ranks with MAX and lets every rank adopt the same ones)."""
    ect, et = meas["explicit_colour"], meas["explicit_cnn"]
    ct = ect if ect is not None else (6 if meas["colour_diff"] <= P.COLOUR_AUTO_BOUND else 3)
    ferr = meas["field_err"][ct]
    path = "fused" if ferr <= P.FIELD_AUTO_BOUND else R._fallback_mode()
    bound = float(R.cnn_auto_bound or P.CNN_AUTO_BOUND)
    ierr = meas["image_err"]
    cal = None
    if et is None:
        diffs = dict(meas.get("cnn_diffs") or {1: meas["cnn_diff"]})
        t = 3
        for cand in CNN_LADDER:         # cheapest first
            if cand != 3 and cand in diffs and cand in ierr and diffs[cand] <= bound and ierr[cand] <= P.IMAGE_AUTO_BOUND:
                t = cand
                break
        if t == 3 and ierr[3] > P.IMAGE_AUTO_BOUND:
            path = R._fallback_mode()
        cal = {"terms3x3": t, "max_abs_diff_1term_vs_3term": meas["cnn_diff"], "bound": bound,
               "max_abs_diff_vs_3term": {str(k): v for k, v in diffs.items()},
               "image_err_vs_fp32": {("1-term" if k == 1 else "3-term" if k == 3 else str(k)): v for k, v in ierr.items()},
               "image_bound": P.IMAGE_AUTO_BOUND, "ladder": [str(k) for k in CNN_LADDER],
               "pixels": P.CNN_CAL_PIXELS, "pixels_measured": meas["pixels"], "calls": 1, "frame": meas["frame"], "measured": "end to end (calibrate_style)"}
    R.field_gate = {
        "path": path, "max_abs_err_vs_fp32": ferr, "bound": P.FIELD_AUTO_BOUND, "quantity": "net_out (per-ray feature, range [-1, 1])",
        "colour": ({"terms": ct, "set_explicitly": True} if ect is not None else
                   {"terms": ct, "max_abs_diff_fp6_vs_3term": meas["colour_diff"], "bound": P.COLOUR_AUTO_BOUND}),
        "image_err_vs_fp32": ierr[et if et is not None else cal["terms3x3"]], "image_bound": P.IMAGE_AUTO_BOUND,
        "sky": {"hidden_terms": (meas.get("explicit_sky") or (6 if meas.get("sky_err", {}).get(6, 1.0) <= P.SKY_AUTO_BOUND else 3)),
                "max_abs_err_vs_fp32": meas.get("sky_err"), "bound": P.SKY_AUTO_BOUND, "set_explicitly": meas.get("explicit_sky") is not None},
        "rays": meas["rays"], "samples_per_ray": meas["samples_per_ray"], "frame": meas["frame"], "measurements": meas}
    R.colour_terms_auto = ct if ect is None else None
    if "sky_err" in meas:
        R.sky_terms_auto = 6 if (meas.get("explicit_sky") is None and meas["sky_err"].get(6, 1.0) <= P.SKY_AUTO_BOUND) else None
    if cal is not None:
        R.cnn_calibration = cal
        R._drop_other_cnn_planes(cal["terms3x3"])
    return R.field_gate


def recheck_cnn(R, net_out):
    """Once per style, on a LATER frame than the ones calibrate_style saw (the trajectory loop passes its last frame's
    net_out [1,Hp,Wp,64]): the adopted 3x3 rung against the 3-term form on the window where this frame's net_out varies
    most, maximum charged like calibrate_one's.  Two calibration poses decide for a whole trajectory and the margins are thin
    by construction (a style may adopt a rung at 4.97e-4 against 5e-4): if the later pose disagrees, warn and step up the
    ladder for the rest of the style.  ~1.5 ms + one host read, once per style."""
    cal = R.cnn_calibration
    if (not cal or cal.get("recheck") is not None or cal["terms3x3"] == 3 or R.explicit_cnn_terms() is not None
            or os.environ.get("SDN_CNN_RECHECK", "1") == "0"):
        return None
    bound = float(cal.get("bound") or P.CNN_AUTO_BOUND)
    _, Hp, Wp, _ = net_out.shape
    side = P.CAL_CROP + 2 * P.CNN_HALO
    Hc, Wc = min(Hp, side), min(Wp, side)
    with torch.no_grad():
        v = net_out[0]
        g = torch.zeros(Hp, Wp, device=net_out.device)
        g[1:] += (v[1:] - v[:-1]).abs().sum(dim=-1)
        g[:, 1:] += (v[:, 1:] - v[:, :-1]).abs().sum(dim=-1)
        r0, c0 = _busiest_window(g, Hc, Wc)
        x = net_out[:, r0:r0 + Hc, c0:c0 + Wc].contiguous()
        ref3 = R._cnn_form(3)(x).clone()
        ladder = list(CNN_LADDER)
        start = ladder.index(form_key(cal["terms3x3"]))
        seen = {}
        adopted = 3
        for cand in ladder[start:]:
            if cand == 3:
                break
            seen[str(cand)] = float((R._cnn_form(cand)(x) - ref3).abs().max()) * P.CAL_CROP_FACTOR
            if seen[str(cand)] <= bound:
                adopted = cand
                break
        R._drop_cnn_planes(Hc, Wc)      # the window's planes are not the frame's
    cal["recheck"] = {"window": [r0, c0, Hc, Wc], "max_abs_diff_vs_3term_charged": seen, "bound": bound, "adopted_before": cal["terms3x3"],
                      "adopted_after": adopted}
    if adopted != cal["terms3x3"]:
        warnings.warn(f"render CNN: rung {cal['terms3x3']} adopted on the calibration poses measures {seen} > {bound:g} on a later frame of the "
                      f"style; stepping up to {adopted}")
        cal["terms3x3"] = adopted
    return cal["recheck"]


def cnn_window_gate(R, net_out):
    """The render CNN's gate where no fp32 twin is at hand (see PrecisionState.mfma_cnn): every net_out presented until
    CNN_CAL_PIXELS pixels of the style have been seen (one 960x540 frame; the first ~20 tiles of the reference's tiled loop) goes
    through the 3-term form AND every cheaper rung of cnn.CNN_LADDER that has not failed yet.  The cheapest rung is used whose
    every comparison so far stayed inside the bound AND inside the image budget left by the field's own measured error
    (field_gate); a rung that violates either once is out for the style.  Updates and returns R.cnn_calibration."""
    cal = R.cnn_calibration
    get = R._cnn_form
    bound = float(R.cnn_auto_bound or P.CNN_AUTO_BOUND)
    fg = R.field_gate
    field_err = float(fg["max_abs_err_vs_fp32"]) if fg else P.FIELD_NOMINAL_ERR
    worst = dict(cal["max_abs_diff_vs_3term"]) if cal else {}
    fits = lambda v: v <= bound and field_err + v <= P.IMAGE_BUDGET
    with torch.no_grad():
        ref3 = get(3)(net_out)
        for cand in CNN_LADDER:
            if cand != 3 and fits(worst.get(str(cand), 0.0)):
                worst[str(cand)] = max(worst.get(str(cand), 0.0), float((ref3 - get(cand)(net_out)).abs().max()))
    t = next((cand for cand in CNN_LADDER if cand != 3 and fits(worst.get(str(cand), float("inf")))), 3)
    px = int(net_out.shape[1] * net_out.shape[2])
    cal = R.cnn_calibration = {
        "terms3x3": t, "max_abs_diff_1term_vs_3term": worst.get("1"), "max_abs_diff_vs_3term": worst, "bound": bound,
        "ladder": [str(k) for k in CNN_LADDER],
        "field_err_charged": field_err, "image_budget": P.IMAGE_BUDGET, "pixels": (cal["pixels"] if cal else 0) + px,
        "calls": (cal["calls"] if cal else 0) + 1,
        "frame": f"first {(cal['calls'] if cal else 0) + 1} net_out(s) of the style, {(cal['pixels'] if cal else 0) + px} px "
                 f"(window {P.CNN_CAL_PIXELS} px)"}
    if t == 3 or cal["pixels"] >= P.CNN_CAL_PIXELS:
        R._drop_other_cnn_planes(t)
    return cal


def _busiest_window(g, Hc, Wc, stride=8):
    """(row, column) of the Hc x Wc window of the score map g [H, W] with the largest sum, on a grid of `stride` pixels: box sums from
    a summed-area table (a pooling kernel with a 286 x 286 window took 34 ms of a 75-ms calibration; this takes 0.3)."""
    H, W = g.shape
    sat = F.pad(g.double().cumsum(0).cumsum(1), (1, 0, 1, 0))
    ys = torch.arange(0, H - Hc + 1, stride, device=g.device)
    xs = torch.arange(0, W - Wc + 1, stride, device=g.device)
    box = sat[ys + Hc][:, xs + Wc] - sat[ys][:, xs + Wc] - sat[ys + Hc][:, xs] + sat[ys][:, xs]
    k = int(box.argmax())
    return int(ys[k // xs.numel()]), int(xs[k % xs.numel()])
