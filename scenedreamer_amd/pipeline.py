"""The trajectory loop of the renderer (Renderer.render_frames): frames software-pipelined over two (optionally three) streams."""
import os

import torch

from . import fused
from . import precision as P
from .camera import frame_intrinsics

RECHECK_MIN_FRAMES = 2     # trajectories at least this long re-check the adopted CNN rung on their last frame (Renderer.recheck_cnn)
FRONT_DEFAULT = "early"
CNN_STREAM_DEFAULT = "0"   # render CNN of frame i on its own stream beside the field kernel of frame i+1 (see render_frames)


def render_frames(R, poses, resolution_hw=(540, 960), num_samples=24, mode="fused", apron="minimal", probe=None, **kw):
    """Generator over the frames of a trajectory, software-pipelined over two streams: the front half of frame i+1
    (ray casting, sky MLP, sample encode) is issued on a second stream while the back half of frame i (field MLP, render
    CNN) runs.  rvip_kernel (20 registers, no LDS) co-resides with the one-workgroup-per-CU MFMA kernels; the sky and
    encode kernels fill the CUs that idle at the tails and launch boundaries of the MFMA kernels.  Images are bit-identical
    to render_frame (tests/test_fullsize_gpu.py).
    probe: optional dict; gets lists of (start, end) timing events around the dominant kernels' launches, recorded on the
    stream they are launched on ("mlp_kernel": main stream, "encode_kernel": side stream) -- bench.py's roofline record is
    computed from the launches of the timed region itself."""
    poses = list(poses)
    if not poses:
        return
    main = torch.cuda.current_stream(R.dev)
    side = R._side_stream
    if side is None:
        side = R._side_stream = torch.cuda.Stream(R.dev)
    if mode == "fused":
        if R.field_gate is None and P.FIELD_GATE:
            R.calibrate_style(poses[0], resolution_hw, num_samples, more_poses=poses[len(poses) // 2:len(poses) // 2 + 1] if len(poses) > 2 else ())
        if R.field_falls_back():
            mode = R.field_gate["path"]       # "unfused" or "exact" (Renderer.fallback): every frame of the trajectory the same
    f0, c0, cam_res = frame_intrinsics(poses[0][3], resolution_hw, R.pad)
    crop = R.pad // 2
    o = R.apron_offset(apron)
    Hp, Wp = cam_res[0] - 2 * o, cam_res[1] - 2 * o
    one = mode == "fused" and fused.single_kernel(R) and fused.precision_profile(R)[0] != 2   # lookup + MLP in ONE kernel
    deep = mode == "fused" and not kw and (one or fused.single_chunk(Hp * Wp, num_samples))

    def front(pose, slot):
        start = torch.cuda.Event()
        start.record(main)                      # everything of the frame that used this slot before has been enqueued
        with torch.cuda.stream(side), torch.no_grad():
            side.wait_event(start)
            vid, d2, rd, res = R.cast_rays(pose, resolution_hw)
            out = (vid, d2, rd, res)
            if deep:
                H0, W0 = res
                vid, d2, rd = R.flat_rays(vid, d2, rd)
                sky_c, sky_avg = R.sky(rd, "fused")     # (deep is the fused path: always the f16-split sky kernel)
                win = fused.Window.crop(H0, W0, o)      # the kernels read the frame-wide arrays through the window
                if one:     # the field kernel gathers for itself: the front half is ray casting + sky MLP only
                    out = ((vid, d2, rd), sky_c, sky_avg, win)
                    keep = (vid, d2, rd, sky_c, sky_avg)
                else:
                    if probe is not None:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(side)
                    buf = fused.encode(R, vid, d2, rd, torch.as_tensor(pose[0], dtype=torch.float32), num_samples,
                                       fused._buffers(R, win.n_rays, num_samples, slot), window=win)
                    if probe is not None:
                        e1.record(side)
                        probe.setdefault("encode_kernel", []).append((e0, e1))
                    out = (buf, sky_c, sky_avg, win)
                    keep = (sky_c, sky_avg)     # vid / d2 / rd are only read on the side stream (by encode)
            else:
                keep = out[:3]
            done = torch.cuda.Event()
            done.record(side)
        for t in keep:
            t.record_stream(main)               # allocated on the side stream, consumed on the main stream
        return out, done

    # (Issuing the next front half only behind this frame's MLP was measured: mlp_kernel 16.2 -> 15.8 ms without the ray caster
    # beside its start, but the frame 22.4 -> 22.8 ms, because the ray caster then lands in the CNN phase too.)
    # where the next frame's front half (ray casting + sky MLP [+ encode]) is released: "early" = as soon as the previous
    # frame's CNN has been enqueued, i.e. beside this frame's field kernel; "late" = behind this frame's field kernel, i.e. beside
    # its CNN.  (SDN_FRONT=late|early; measured in DESIGN.md section 6.)
    late = deep and os.environ.get("SDN_FRONT", FRONT_DEFAULT) == "late"
    # The render CNN of frame i on a THIRD stream, beside the field kernel of frame i+1 (SDN_CNN_STREAM=1): both are one-workgroup-
    # per-CU kernels, so they cannot share a CU, but the CNN's six dependent launches leave CUs idle at every launch boundary
    # and the field kernel's persistent workgroups retire over the length of a 32-ray group -- with both in flight whichever has
    # workgroups ready takes the idle CUs.  The image of frame i is handed out one iteration later (after the field kernel of
    # frame i+1 has been enqueued), so the consumer's wait for it does not order the main stream behind the CNN.
    cnn_side = deep and os.environ.get("SDN_CNN_STREAM", CNN_STREAM_DEFAULT) == "1" and R.field_gate is not None
    cstream = None
    if cnn_side:
        cstream = R._cnn_stream
        if cstream is None:
            cstream = R._cnn_stream = torch.cuda.Stream(R.dev)
    pending = None          # (image, its completion event) of the previous frame
    nxt = front(poses[0], 0)
    try:
        for i, pose in enumerate(poses):
            cur, done = nxt
            if not late:
                nxt = front(poses[i + 1], (i + 1) & 1) if i + 1 < len(poses) else None
            main.wait_event(done)
            if not deep:
                yield R.render_frame(pose, resolution_hw, num_samples, mode=mode, apron=apron, _precast=cur, **kw)
                continue
            buf, sky_c, sky_avg, win = cur
            with torch.no_grad():
                if probe is not None:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(main)
                if one:
                    net_out = fused.field_render(R, *buf, torch.as_tensor(pose[0], dtype=torch.float32), sky_c, sky_avg, num_samples,
                                                 window=win).view(1, Hp, Wp, 64)
                else:
                    net_out = fused.mlp_from(R, buf, sky_c, sky_avg.reshape(-1), win.n_rays, num_samples, window=win).view(1, Hp, Wp, 64)
                if probe is not None:
                    e1.record(main)
                    probe.setdefault("mlp_kernel", []).append((e0, e1))
                if late:
                    nxt = front(poses[i + 1], (i + 1) & 1) if i + 1 < len(poses) else None
                c = crop - o
                if cnn_side:
                    f_done = torch.cuda.Event()
                    f_done.record(main)
                    net_out.record_stream(cstream)              # allocated on the main stream, read on the CNN stream
                    with torch.cuda.stream(cstream):
                        cstream.wait_event(f_done)
                        cnn = R.mfma_cnn(net_out)            # (decided by calibrate_style: no calibration launches here)
                        if probe is not None:
                            c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            c0.record(cstream)
                        img = cnn(net_out)
                        if probe is not None:
                            c1.record(cstream)
                            probe.setdefault("render_cnn", []).append((c0, c1))
                        c_done = torch.cuda.Event()
                        c_done.record(cstream)
                    img.record_stream(main)                     # allocated on the CNN stream, consumed on the main stream
                    if pending is not None:
                        main.wait_event(pending[1])
                        yield pending[0]
                    pending = (img[:, :, c:-c, c:-c] if c else img, c_done)
                    continue
                cnn = R.mfma_cnn(net_out)         # (first frame of a style: calibrates the 3x3 precision, see mfma_cnn)
                if probe is not None:
                    c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    c0.record(main)
                img = cnn(net_out)
                if probe is not None:
                    c1.record(main)
                    probe.setdefault("render_cnn", []).append((c0, c1))
                if i == len(poses) - 1 and len(poses) >= RECHECK_MIN_FRAMES:
                    R.recheck_cnn(net_out)        # (once per style: the adopted 3x3 rung on a pose the calibration did not see)
                yield img[:, :, c:-c, c:-c] if c else img
        if pending is not None:
            last, pending = pending, None
            main.wait_event(last[1])
            yield last[0]
    finally:
        if pending is not None:      # the consumer stopped early: the main stream still has to be ordered behind the CNN stream's work
            main.wait_event(pending[1])
