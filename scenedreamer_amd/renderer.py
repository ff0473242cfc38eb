"""Frame renderer: the host-side mirror of Generator.inference_givenstyle's per-frame body
(imaginaire/generators/scenedreamer.py:573-628) on top of libsdnative.

Two interchangeable per-pixel paths produce net_out [1, Hp, Wp, 64] for the padded frame:

  * "unfused": the reference's op sequence -- voxlib.ray_voxel_intersection_perspective ->
    sample placement -> GridEncoder.forward -> render MLP -> volume rendering -- with the three
    native ops served by the drop-in HIP kernels and everything else by PyTorch ops on the GPU
    (exactly what the unmodified reference generator does when our shim modules are installed);
  * "fused": sample placement, hash-grid lookup, MLP and compositing inside libsdnative's field
    kernels (see csrc/field.hip), selected with mode="fused".

Differences from the reference's loop that do not change the result: every ray is evaluated once on
the full padded frame instead of in 40 overlapping 158-px tiles (the per-pixel field has no spatial
coupling), and the render CNN runs once on the padded frame and is cropped by pad/2 afterwards (its
receptive radius of 4 px is smaller than the 15-px crop, gancraft_base.py:180-190).  Per-style
constants (W * alpha, beta of every ModLinear; the label-bias table replacing the one-hot matmul)
are folded once per style code instead of once per tile.
"""
import json
import os
import sys
import types
import warnings

import numpy as np
import torch
import torch.nn.functional as F

from . import calibration, fused, ops, pipeline, roofline
from . import precision as P
from .calibration import _busiest_window    # noqa: F401  (tests name it here)
from .camera import frame_intrinsics
from .precision import PrecisionState, resolve_cnn_mode, resolve_sky_mode    # noqa: F401  (callers name the two functions here)
from .timing import _Stamps, _time_ms    # noqa: F401  (bench.py and tools/ import _time_ms from here)

MISS_COST = 0.2            # row_costs: cost of a ray that hits nothing relative to one that does (ray casting + sky MLP + CNN vs + field)
_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
MAP_OUTPUTS = ("depth", "opacity", "depth_u8", "range", "weights", "sample_depth")      # keys of render_frame's `maps`
MAP_DEFAULT = ("depth", "opacity", "depth_u8")                                          # ... and what an empty dict stands for


class _BoundsLiveInPrecision(types.ModuleType):
    """The bounds were this module's before they moved to precision.py, and callers still read -- and tests still patch -- them
    here.  A re-export would be a second binding that a patch does not carry to the code; this module forwards reads and writes
    of those names instead, so each bound keeps exactly one binding, in precision.py."""
    _BOUNDS = frozenset(n for n in vars(P) if n.isupper())

    def __getattr__(self, name):
        if name in self._BOUNDS:
            return getattr(P, name)
        raise AttributeError(f"module {self.__name__!r} has no attribute {name!r}")

    def __setattr__(self, name, value):
        if name in self._BOUNDS:
            setattr(P, name, value)
        else:
            super().__setattr__(name, value)


sys.modules[__name__].__class__ = _BoundsLiveInPrecision


def load_label_lut():
    """minecraft block id -> reduced label (12 classes), mc_lbl_reduction.py:36-43 (data file)."""
    return json.load(open(os.path.join(_DATA, "mc2reduced.json")))


def _lrelu(x):
    return F.leaky_relu(x, 0.2)


# ---- per-style constants of the three networks.  `R` is a Renderer or any object with `w` (the reference's parameter names ->
# ---- device tensors), e.g. the module-level backends of modules.py that read a live nn.Module's parameters.
def fold_render_net(R, z):
    """LightningMLP for one style code z [1, style_dim]: ModLinear with N = 1 is a plain layer W' = W * alpha (per input
    channel) with bias beta (layers.py:247-269); one-hot(label) @ fc_m_a^T + fc_1.bias is a row lookup in a [12, 256] table
    (use_seg = False: every row is fc_1.bias)."""
    w = R.w
    with torch.no_grad():
        R.mod = {}
        for i in (2, 3, 4, 5, 6):
            n = f"render_net.fc_{i}"
            alpha = F.linear(z, w[n + ".weight_alpha"], w[n + ".bias_alpha"])       # [1, in]
            beta = F.linear(z, w[n + ".weight_beta"], w[n + ".bias_beta"])          # [1, out]
            R.mod[i] = ((w[n + ".weight"] * alpha).contiguous(), beta[0].contiguous())
        b1 = w["render_net.fc_1.bias"][None, :]
        if "render_net.fc_m_a.weight" in w:
            R.label_bias = (w["render_net.fc_m_a.weight"].t() + b1).contiguous()
        else:
            R.label_bias = b1.expand(12, -1).contiguous()
    R._fused_style = None
    R._fused_style_f32 = None


def fold_sky_net(R, z):
    """SKYMLP: the style term fc_z_a(z) [1, 256] joins fc1's bias (gancraft_base.py:158-162)."""
    with torch.no_grad():
        R.sky_z = F.linear(z, R.w["sky_net.fc_z_a.weight"])
    R._fused_sky = None
    R._fused_sky_f32 = None


def fold_denoiser(R, z):
    """RenderCNN: the four FiLM vectors fc_z_cond(z) [1, 1024] (gancraft_base.py:203-204)."""
    with torch.no_grad():
        R.cnn_adapt = F.linear(z, R.w["denoiser.fc_z_cond.weight"], R.w["denoiser.fc_z_cond.bias"])
    R.cnn_calibration = None      # the FiLM vectors changed: the render CNN's precision gate is re-evaluated


class Renderer(PrecisionState):
    """(The precision knobs, the per-style decisions, their resolvers and the render CNN's forms: precision.PrecisionState.)"""

    def __init__(self, weights, scene, device="cuda", num_blocks_early_stop=6, sample_depth=3.0, dists_scale=0.25,
                 pad=30, exact_world=None, exact_style=None):
        # (the two encoder knobs of precision.PrecisionState, as keywords: set_scene below already runs the world encoder)
        if exact_world is not None:
            self.exact_world = exact_world
        if exact_style is not None:
            self.exact_style = exact_style
        self.dev = torch.device(device)
        if self.dev.type == "cuda" and self.dev.index is None:      # "cuda" -> "cuda:<current>": tensor.device carries the index
            self.dev = torch.device("cuda", torch.cuda.current_device())
        self.w = {k: (v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))).to(self.dev)
                  for k, v in weights.items()}
        lut = load_label_lut()
        t = torch.tensor(lut["lut"], dtype=torch.long)
        t[t == lut["ignore_id"]] = lut["dirt_id"]  # mc2reduced(ign2dirt=True), mc_utils.py:241-246
        self.lut = t.to(self.dev)
        self.M = num_blocks_early_stop
        self.sample_depth = float(sample_depth)
        self.dists_scale = float(dists_scale)
        self.pad = pad
        offs = self.w["hash_encoder.offsets"]
        self.grid_L = offs.numel() - 1
        self.grid_S = float(np.log2(np.exp2(np.log2(2048 / 16) / (self.grid_L - 1))))
        self.timings = {}
        self.set_scene(scene)

    # ------------------------------------------------------------------ once per scene / style
    def set_scene(self, scene):
        self.scene = scene
        # compact scenes (scene.CompactScene: uint8 palette indices + int32 palette, 4x smaller) are walked as they are;
        # the reference's int32 volume otherwise.  `volume` is what the ray marcher gets, `voxel_dims` its extent.
        self.palette = None
        if getattr(scene, "voxel_u8", None) is not None:
            self.volume = scene.voxel_u8.to(self.dev)
            self.palette = scene.palette.to(self.dev).contiguous()
            self.max_block_id = int(self.palette.max())
        else:
            self.volume = scene.voxel_t.to(self.dev)
            self.max_block_id = int(self.volume.max()) if self.volume.numel() else 0
            if self.volume.numel() and int(self.volume.min()) < 0:
                raise RuntimeError("negative block id in the scene volume")
        self.voxel_dims = tuple(int(v) for v in self.volume.shape)
        if self.volume.is_cuda:
            ops.voxel_occupancy(self.volume)   # built here, on the caller's stream, before any side-stream ray casting
        world = self._exact_world_mode()
        with torch.no_grad():
            if world == "f32":      # the fixed-order kernels (csrc/world_f32.hip): no library between the maps and global_enc
                self.global_enc = fused.world_exact(self, scene.current_height_map, scene.current_semantic_map)
            else:
                self.global_enc = self._world_encoder_torch(scene)
        self._ran("world", world)
        self._fused_scene = None
        self.reset_gates()               # (the collapsed table changes with global_enc; the CNN's record and forms stay)

    def _world_encoder_torch(self, scene):
        """ConditionalHashGrid.forward (layers.py:40-55) as the reference's op sequence on the libraries."""
        w = self.w
        # (deterministic convolution algorithms: global_enc feeds every sample of every frame, and every rank of a sharded
        # trajectory computes it for itself -- MIOpen's default solver choice is not reproducible from call to call)
        with torch.no_grad(), warnings.catch_warnings(), \
                torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
            warnings.simplefilter("ignore")
            h = _lrelu(F.conv2d(scene.current_height_map.to(self.dev), w["world_encoder.hconv_head.weight"],
                                w["world_encoder.hconv_head.bias"], stride=2, padding=1))
            s = _lrelu(F.conv2d(scene.current_semantic_map.to(self.dev), w["world_encoder.sconv_head.weight"],
                                w["world_encoder.sconv_head.bias"], stride=2, padding=1))
            x = torch.cat([h, s], dim=1)
            for i in range(5):
                x = F.relu(F.conv2d(x, w[f"world_encoder.conv_blocks.{i}.layers.0.weight"], None, stride=1, padding=1))
                x = F.relu(F.conv2d(x, w[f"world_encoder.conv_blocks.{i}.layers.2.weight"], None, stride=2, padding=1))
                x = _lrelu(x)
            x = x.permute(0, 2, 3, 1)
            x = x.reshape(x.shape[0], -1, x.shape[-1]).mean(dim=1)
            x = _lrelu(F.linear(x, w["world_encoder.fc1.weight"], w["world_encoder.fc1.bias"]))
            return torch.tanh(F.linear(x, w["world_encoder.fc2.weight"], w["world_encoder.fc2.bias"]))

    def _style_mlp_torch(self, style):
        """StyleMLP.forward (gancraft_base.py:113-126) as the reference's op sequence on the libraries."""
        w = self.w
        with torch.no_grad():
            z = F.normalize(torch.as_tensor(style, dtype=torch.float32, device=self.dev), p=2, dim=-1)
            for i in range(5):
                z = _lrelu(F.linear(z, w[f"style_net.fc_layers.{i}.weight"], w[f"style_net.fc_layers.{i}.bias"]))
            return _lrelu(F.linear(z, w["style_net.fc_out.weight"], w["style_net.fc_out.bias"]))

    def set_style(self, style):
        how = self._exact_style_mode()
        with torch.no_grad():
            # "f32": the fixed-order kernel (csrc/world_f32.hip) -- f64 accumulation in k order, no library
            z = fused.style_exact(self, style) if how == "f32" else self._style_mlp_torch(style)
        self._ran("style", how)
        self.set_style_code(z)

    def set_style_code(self, z):
        """Fold an intermediate style code z [1,256] (= style_net(style)) into per-style constants."""
        with torch.no_grad():
            z = torch.as_tensor(z, dtype=torch.float32, device=self.dev).reshape(1, -1)
            self.z = z
            fold_render_net(self, z)
            fold_sky_net(self, z)
            fold_denoiser(self, z)
        self.reset_gates()               # the per-style gates are re-evaluated (the CNN's: fold_denoiser dropped its record)

    # ------------------------------------------------------------------ stages
    def cast_rays(self, pose, resolution_hw):
        cam_ori, cam_dir, cam_up, cam_f = pose
        f, c, cam_res = frame_intrinsics(cam_f, resolution_hw, self.pad)
        vid, d2, rd = ops.ray_voxel_intersection_perspective(self.volume, cam_ori, cam_dir, cam_up, f, c, cam_res,
                                                             self.M, palette=self.palette)
        return vid, d2, rd, cam_res

    def flat_rays(self, vid, d2, rd):
        """A ray-cast result as the per-ray stages take it: voxel ids [n, M], depths [2, n, M], ray directions [n, 3]."""
        n = rd.numel() // 3
        return vid.view(n, self.M), d2.view(2, n, self.M), rd.view(n, 3)

    def apron_offset(self, apron, mode="fused", minimal=True):
        """Rows / columns of the padded frame's border that the field and the CNN skip: the reference's apron is pad / 2 = 15 px,
        only CNN_HALO = 4 px of it can reach a kept pixel (see render_frame).  0 for apron="reference", for the un-fused path
        (it always evaluates everything), and where the caller says the minimal apron does not apply (`minimal` False)."""
        crop = self.pad // 2
        return crop - P.CNN_HALO if (minimal and mode in ("fused", "exact") and apron == "minimal" and crop > P.CNN_HALO) else 0

    def sky(self, rd, sky_mode, mean=True):
        """(sky_c [n, 64], sky_avg [1, 64]) by the sky MLP `sky_mode` (_resolve_sky_mode).  mean=False: a caller that owns only
        part of the frame's rays takes no mean from "f32" and "torch" (sky_avg None; the f16-split kernel always finishes one)."""
        if sky_mode == "fused":
            return fused.sky_fused(self, rd)
        if sky_mode == "f32":
            return fused.sky_exact(self, rd, mean=mean)
        sky_c = self.sky_features(rd)
        return sky_c, (sky_c.mean(dim=0, keepdim=True) if mean else None)    # full-frame mean, scenedreamer.py:592-598

    @property
    def voxel_t(self):
        """The int32 block-id volume (expanded on demand for a compact scene)."""
        return self.volume if self.palette is None else self.scene.voxel_t

    def sky_features(self, raydirs):
        """sky_net(PE(raydirs)) for every ray: [R,3] -> [R,64] (scenedreamer.py:368-370, gancraft_base.py:150-169)."""
        w = self.w
        pe = ops.positional_encoding(raydirs.contiguous(), 5, -1, True)
        y = _lrelu(F.linear(pe, w["sky_net.fc1.weight"], w["sky_net.fc1.bias"]) + self.sky_z)
        for i in (2, 3, 4, 5):
            y = _lrelu(F.linear(y, w[f"sky_net.fc{i}.weight"], w[f"sky_net.fc{i}.bias"]))
        return F.linear(y, w["sky_net.fc_out_c.weight"], w["sky_net.fc_out_c.bias"])

    def place_samples(self, depth2, ns):
        """sample_depth_batched, deterministic, no box boundaries (mc_utils.py:82-151).
        depth2 [2,R,M] -> depth [R,ns], dists [R,ns], box index [R,ns]."""
        t, t2 = depth2[0], depth2[1]
        d = t2 - t
        d = torch.where(torch.isnan(d), torch.zeros_like(d), d)
        accu = torch.cumsum(d, dim=-1)
        total = accu[:, -1:].clamp(max=self.sample_depth)
        lin = torch.linspace(0, 1, ns + 3)[1:-1].to(self.dev)   # nsamples = ns+1 stratified points
        s = lin[None, :] * total
        mid = (s[:, 1:] + s[:, :-1]) / 2
        nd = s[:, 1:] - s[:, :-1]
        idx = (mid[:, None, :] > accu[:, :, None]).sum(dim=1)
        gaps = torch.cumsum(t[:, 1:] - t2[:, :-1], dim=-1)
        heads = torch.cat([t[:, :1], gaps + t[:, :1]], dim=-1)
        depth = torch.gather(heads, 1, idx) + mid
        return depth, nd, idx

    def field_unfused(self, voxel_id, depth2, raydirs, cam_ori, sky_c, sky_avg, ns, placement="torch", aux=None):
        """Per-ray feature net_out [R,64] from [R,M] intersections (scenedreamer.py:313-430).
        aux: None, or a dict that receives "weights" and "depth" [R,ns] (scenedreamer.py:373-376, :346-352), the two per-sample
        arrays of the fused kernels' aux protocol.
        placement: "torch" = sample placement by PyTorch ops on the GPU, what the unmodified reference does on the op shims
        (torch.cumsum accumulates in float32 on the GPU, in double on the CPU: the two reference paths place some samples 1 ulp
        apart, which the fine grid levels and the density head turn into net_out differences of a few 1e-4 at isolated rays);
        "kernel" = placement by sdn_sample_depth, the device function the fused kernel uses (the CPU reference's arithmetic) -- the
        fp32 twin calibrate_style compares with, so that what it measures is the reduced-precision ARITHMETIC of the fused path
        and not the reference's own placement chaos."""
        w = self.w
        if placement == "kernel":
            R_ = depth2.shape[1]
            depth, nd, idx = ops.sample_depth_batched(depth2.reshape(2, R_, 1, self.M, 1).unsqueeze(0).contiguous(), ns + 1, deterministic=True,
                                                      use_box_boundaries=False, sample_depth=self.sample_depth)
            depth, nd, idx = depth.reshape(R_, ns), nd.reshape(R_, ns), idx.reshape(R_, ns).clamp(max=self.M - 1)
        else:
            depth, nd, idx = self.place_samples(depth2, ns)
        depth = torch.where(torch.isnan(depth) | torch.isinf(depth), torch.zeros_like(depth), depth)
        wc = raydirs[:, None, :] * depth[:, :, None] + cam_ori[None, None, :]
        lab = torch.gather(self.lut[voxel_id.long()], 1, idx)
        delim = torch.tensor([float(v) for v in self.voxel_dims], device=self.dev)
        n = wc / delim * 2 - 1
        x5 = torch.cat([n, self.global_enc[:, None, :].expand(n.shape[0], n.shape[1], 2)], dim=-1)
        x5 = ((x5 + 1) / 2).reshape(-1, 5).contiguous()           # GridEncoder.forward, grid.py:144
        B = x5.shape[0]
        feats = torch.empty(self.grid_L, B, 8, device=self.dev)
        ops.grid_encode_forward(x5, w["hash_encoder.embeddings"], w["hash_encoder.offsets"], feats, B, 5, 8,
                                self.grid_L, self.grid_S, 16, False, torch.empty(1, device=self.dev), 0, False)
        feats = feats.permute(1, 0, 2).reshape(B, self.grid_L * 8)
        f = _lrelu(F.linear(feats, w["render_net.fc_1.weight"]) + self.label_bias[lab.reshape(-1)])
        for i in (2, 3, 4):
            f = _lrelu(torch.addmm(self.mod[i][1], f, self.mod[i][0].t()))
        sigma = F.linear(f, w["render_net.fc_sigma.weight"], w["render_net.fc_sigma.bias"]).reshape(-1, ns)
        for i in (5, 6):
            f = _lrelu(torch.addmm(self.mod[i][1], f, self.mod[i][0].t()))
        color = F.linear(f, w["render_net.fc_out_c.weight"], w["render_net.fc_out_c.bias"]).reshape(-1, ns, 64)
        # volum_rendering_relu (mc_utils.py:154-161) + compositing (scenedreamer.py:373-413)
        fe = F.relu(sigma) * (nd * self.dists_scale)
        # exclusive cumsum as roll(cumsum) with a zero head (mc_utils.py:75-79)
        excl = torch.cat([torch.zeros_like(fe[:, :1]), torch.cumsum(fe, dim=-1)[:, :-1]], dim=-1)
        wts = (1 - torch.exp(-fe)) * torch.exp(-excl)
        sky_only = voxel_id[:, :1] == 0
        wts = wts * (~sky_only).float()
        if aux is not None:
            aux["weights"], aux["depth"] = wts, depth
        T = wts.sum(dim=-1, keepdim=True)
        is_gnd = (wc[:, :, 0] <= 1.0).any(dim=-1, keepdim=True)
        nosky = ((voxel_id[:, -1:] != 0) | is_gnd).float()
        sky = sky_c * (1.0 - nosky) + sky_avg * nosky
        rgb = torch.clamp(color, -1, 1) + 1
        rgb_sky = torch.clamp(sky, -1, 1) + 1
        return (wts[:, :, None] * rgb).sum(dim=1) + (1.0 - T) * rgb_sky - 1

    def render_cnn(self, net_out):
        """_forward_global + RenderCNN (gancraft_base.py:588-603, :202-225): [1,Hp,Wp,64] -> [1,3,Hp,Wp]."""
        w = self.w
        a = torch.chunk(self.cnn_adapt, 4, dim=-1)
        mod = lambda v, s, b: v * (s[..., None, None] + 1) + b[..., None, None]
        cv = lambda v, n, p: F.conv2d(v, w[f"denoiser.{n}.weight"], w.get(f"denoiser.{n}.bias"), padding=p)
        x = net_out.permute(0, 3, 1, 2).contiguous()
        y = _lrelu(cv(x, "conv1", 0))
        y = y + cv(_lrelu(cv(y, "conv2a", 1)), "conv2b", 1)
        y = _lrelu(mod(y, a[0], a[1]))
        y = y + cv(_lrelu(cv(y, "conv3a", 1)), "conv3b", 1)
        y = _lrelu(mod(y, a[2], a[3]))
        y = y + cv(_lrelu(cv(y, "conv4a", 0)), "conv4b", 0)
        y = _lrelu(y)
        return torch.tanh(cv(y, "conv4", 0))

    def _run_cnn(self, cnn_mode, net_out):
        if cnn_mode == "mfma":
            return self.mfma_cnn(net_out)(net_out)
        if cnn_mode == "f32":
            return self.f32_cnn()(net_out)
        return self.render_cnn(net_out)

    # ------------------------------------------------------------------ per-style precision gates (calibration.py)
    def calibrate_style(self, pose, resolution_hw, num_samples, more_poses=()):
        return calibration.calibrate_style(self, pose, resolution_hw, num_samples, more_poses)

    def calibrate_one(self, pose, resolution_hw, num_samples, crop_px=None):
        return calibration.calibrate_one(self, pose, resolution_hw, num_samples, crop_px)

    def adopt_precision(self, meas):
        return calibration.adopt_precision(self, meas)

    def recheck_cnn(self, net_out):
        return calibration.recheck_cnn(self, net_out)

    # ------------------------------------------------------------------ measurement (roofline.py)
    def measure_roofline(self, pose, resolution_hw, num_samples, mode, hbm_peak_gbps=8000.0, mfma_peak_tflops=2500.0):
        return roofline.measure_roofline(self, pose, resolution_hw, num_samples, mode, hbm_peak_gbps, mfma_peak_tflops)

    def field_work(self, poses, resolution_hw, num_samples, apron="minimal"):
        return roofline.field_work(self, poses, resolution_hw, num_samples, apron)

    def roofline_records(self, B, ms_enc, ms_mlp, hit, ev, kernel, hbm_peak_gbps=8000.0, mfma_peak_tflops=2500.0, timing="",
                         field_kernel=False):
        return roofline.roofline_records(self, B, ms_enc, ms_mlp, hit, ev, kernel, hbm_peak_gbps, mfma_peak_tflops, timing, field_kernel)

    def compute_dtype(self, mode):
        if mode == "unfused":
            return "f32"
        if mode == "exact":
            sky, cnn = self._exact_sky_mode(), self._exact_cnn_mode()
            if sky == "torch" and cnn == "torch":
                return "f32 (field: hash grid + f32-input MFMA with f32 accumulate; sky MLP and render CNN: PyTorch)"
            native = "f32-input MFMA with f32 accumulate"
            return (f"f32 (field: hash grid + {native}; sky MLP: {native if sky == 'f32' else 'PyTorch'}; "
                    f"render CNN: {native if cnn == 'f32' else 'PyTorch'})")
        ct, _ = fused.precision_profile(self)
        cal = self.cnn_calibration
        t3 = self.explicit_cnn_terms()      # (printed as it was given, not as cnn.form_key reads it)
        if t3 is None:
            t3 = (f"{cal['terms3x3']}-term (auto: 1-term vs 3-term image differed by {cal['max_abs_diff_1term_vs_3term']:.1e} <= "
                  f"{cal['bound']:.0e} on the style's first frame)" if cal and cal["terms3x3"] == 1 else
                  f"3-term (auto: the 1-term form differed by {cal['max_abs_diff_1term_vs_3term']:.1e} > {cal['bound']:.0e})" if cal and cal["terms3x3"] == 3
                  else f"per layer (conv2a, conv2b, conv3a, conv3b) = {cal['terms3x3']} terms (auto: the cheapest rung inside the gate; "
                       f"all-1-term differed by {cal['max_abs_diff_1term_vs_3term']:.1e} > {cal['bound']:.0e})" if cal
                  else "auto (1-term if within 5e-4 of the 3-term image, not yet calibrated)")
        else:
            t3 = f"{t3}-term (set explicitly)"
        eps = fused.precision_profile(self)[1]
        return (f"f32 (hash grid) + f16 MFMA with f32 accumulate{f' (early ray termination at transmittance {eps:g})' if eps > 0 else ''}: field/sky MLP 3-term split"
                f"{' (colour layers 2-term)' if ct == 2 else ' (colour layers: f16 Whi.Xhi + MX-fp6 corrections)' if ct == 6 else ''}"
                f"{' (sky hidden layers: f16 + MX-fp6 corrections)' if fused.sky_terms(self) == 6 else ''}"
                f", render CNN 1x1 3-term / 3x3 {t3}")

    # ------------------------------------------------------------------ row bands (tile-parallel single frame)
    def row_costs(self, pose, resolution_hw, scale=4):
        """Relative cost of every OUTPUT row of the frame, for cutting it into bands of equal work (dist.balanced_row_bands):
        the field kernel visits only rays that hit something (sky rows cost almost nothing there), every ray costs ray casting,
        sky MLP and CNN.  Estimated from a 1/scale-resolution ray cast of the padded frame (1/16 of the rays; deterministic and
        bit-identical on every rank, so all ranks cut the same bands without talking): cost(row) = hits(row) + MISS_COST * width.
        The result is kept per (pose, resolution): a trajectory that is rendered again -- or the stats frame of bench.py -- pays
        the low-resolution ray cast and its device -> host read once."""
        cam_ori, cam_dir, cam_up, cam_f = pose
        H, W = resolution_hw
        key = (tuple(np.asarray(cam_ori, np.float64).reshape(-1).tolist()), tuple(np.asarray(cam_dir, np.float64).reshape(-1).tolist()),
               tuple(np.asarray(cam_up, np.float64).reshape(-1).tolist()), float(cam_f), int(H), int(W), int(scale), id(self.volume))
        cache = self._cache("_row_cost_cache")
        if key in cache:
            return cache[key]
        f, c, cam_res = frame_intrinsics(cam_f, resolution_hw, self.pad)
        Hq, Wq = -(-cam_res[0] // scale), -(-cam_res[1] // scale)
        off = (scale - 1) / 2.0
        with torch.no_grad():
            vid, _, _ = ops.ray_voxel_intersection_perspective(self.volume, cam_ori, cam_dir, cam_up, f / scale,
                                                               [(c[0] - off) / scale, (c[1] - off) / scale], [Hq, Wq], 1, palette=self.palette)
            hits_q = (vid.view(Hq, Wq) != 0).sum(dim=1).cpu().numpy().astype(np.float64) * scale      # hits per padded row, estimated
        pad_rows = np.minimum(np.arange(H) + self.pad // 2, cam_res[0] - 1)       # the padded row at the centre of output row r's apron
        while len(cache) >= 512:
            cache.pop(next(iter(cache)))
        cache[key] = hits_q[pad_rows // scale] + MISS_COST * cam_res[1]
        return cache[key]

    def band_prepare(self, pose, resolution_hw, row0, row1, mode="fused", apron="minimal"):
        """Cast the rays needed for output rows [row0,row1) and evaluate the sky MLP on them.  Returns a handle with the band's
        share of the frame-wide sky sum (sky_avg is the mean over ALL rays of the padded frame, scenedreamer.py:592-598: every
        padded row is owned by exactly one band).
        apron: the reference's tiles carry 15 px of apron per side (pad / 2); only CNN_HALO = 4 px can reach a kept pixel.
        "minimal" (fused mode): the band casts padded rows [row0 + 11, row1 + 19) -- the first / last band additionally the
        frame's top / bottom rows, which only the sky mean needs -- and evaluates the field and the CNN on its 4-px apron;
        "reference": padded rows [row0, row1 + 30), everything evaluated (the un-fused path always does)."""
        cam_ori, cam_dir, cam_up, cam_f = pose
        H, W = resolution_hw
        f, c, cam_res = frame_intrinsics(cam_f, resolution_hw, self.pad)
        Wp = cam_res[1]
        crop = self.pad // 2
        o = self.apron_offset(apron, mode)
        # padded rows this band casts / owns for the sky sum / evaluates the field on
        p0 = 0 if row0 == 0 else row0 + o
        p1 = cam_res[0] if row1 == H else row1 + self.pad - o
        own0 = 0 if row0 == 0 else row0 + crop
        own1 = cam_res[0] if row1 == H else row1 + crop
        if o == 0:                       # reference apron: the ownership of rounds 2-3 (rows [row0, row1) + the trailing pad)
            p0, own0, own1 = row0, row0, (cam_res[0] if row1 == H else row1)
        e0, e1 = row0 + o, row1 + self.pad - o
        # same rays as the full frame: ndc_y = c0 - row_global = (c0 - p0) - row_local, exact in float32
        vid, d2, rd = ops.ray_voxel_intersection_perspective(self.volume, cam_ori, cam_dir, cam_up, f, [c[0] - p0, c[1]],
                                                             [p1 - p0, Wp], self.M, palette=self.palette)
        vid, d2, rd = self.flat_rays(vid, d2, rd)
        with torch.no_grad():
            sky_c, _ = self.sky(rd, self._resolve_sky_mode(mode), mean=False)      # (the band owns only part of the frame's rays)
            sky_sum = sky_c[(own0 - p0) * Wp:(own1 - p0) * Wp].sum(dim=0, dtype=torch.float64)
        return dict(vid=vid, d2=d2, rd=rd, sky_c=sky_c, sky_sum=sky_sum, sky_cnt=(own1 - own0) * Wp, cast_rows=(p1 - p0), Wp=Wp,
                    rows=(e1 - e0), cols=Wp - 2 * o, first=(e0 - p0) * Wp + o, halo=crop - o,
                    cam_ori=(torch.as_tensor(cam_ori, dtype=torch.float32) if mode in ("fused", "exact")
                             else torch.as_tensor(cam_ori, dtype=torch.float32).to(self.dev)), mode=mode)

    def band_finish(self, hd, sky_avg, num_samples, cnn_mode=None):
        """Field + CNN for a prepared band given the frame-wide sky_avg [1,64]; returns image rows [1,3,row1-row0,W]."""
        mode = hd["mode"]
        with torch.no_grad():
            sky_avg = sky_avg.to(torch.float32).reshape(1, 64)
            full = hd["rows"] == hd["cast_rows"] and hd["cols"] == hd["Wp"]
            if mode == "fused" and self.field_falls_back():      # (the job-wide decision of dist.agree_precision)
                mode = self.field_gate["path"]
                if mode == "unfused":
                    hd["cam_ori"] = hd["cam_ori"].to(self.dev)
            if mode in ("fused", "exact"):
                win = None if full else fused.Window(hd["cast_rows"] * hd["Wp"], hd["Wp"], hd["first"], hd["rows"], hd["cols"])
                field = fused.field_fused if mode == "fused" else fused.field_exact
                net_out = field(self, hd["vid"], hd["d2"], hd["rd"], hd["cam_ori"], hd["sky_c"], sky_avg, num_samples, window=win)
            else:
                vid, d2, rd, sky_c = hd["vid"], hd["d2"], hd["rd"], hd["sky_c"]
                if not full:             # (a fused band that fell back: cut the evaluated window out of the cast block)
                    y0, x0 = divmod(hd["first"], hd["Wp"])
                    cut = lambda t: t.view(hd["cast_rows"], hd["Wp"], -1)[y0:y0 + hd["rows"], x0:x0 + hd["cols"]].reshape(hd["rows"] * hd["cols"], -1)
                    vid, rd, sky_c = cut(vid), cut(rd), cut(sky_c)
                    d2 = torch.stack([cut(d2[0]), cut(d2[1])])
                net_out = self.field_unfused(vid.contiguous(), d2.contiguous(), rd.contiguous(), hd["cam_ori"], sky_c.contiguous(), sky_avg,
                                             num_samples)
            net_out = net_out.view(1, hd["rows"], hd["cols"], 64)
            img = self._run_cnn(self._resolve_cnn_mode(mode, cnn_mode), net_out)
            p = hd["halo"]
            return img[:, :, p:-p, p:-p] if p else img

    # ------------------------------------------------------------------ frame
    def render_frame(self, pose, resolution_hw=(540, 960), num_samples=24, mode="unfused", cnn=True,
                     ray_chunk=1 << 16, timers=None, cnn_mode=None, apron="minimal", _precast=None, maps=None):
        """One frame of the trajectory.  Returns image [1,3,H,W] (or net_out [1,Hp,Wp,64] if cnn=False).

        apron: the reference evaluates every ray of the frame padded by 15 px per side (its tile scheme,
        scenedreamer.py:573-628) and crops the image afterwards.  Only CNN_HALO = 4 px of that apron can reach a kept
        pixel (RenderCNN has four 3x3 convolutions, gancraft_base.py:175-225; their zero padding at the padded frame's
        border is 15 px away).  "minimal" (fused path, default) evaluates the field and the CNN on the 4-px apron; the
        sky MLP still sees every ray of the padded frame, because its frame mean does (scenedreamer.py:592-598).  The
        image is bit-identical to "reference" (full apron) when every sample is evaluated (term_eps = 0); with early ray
        termination (the default) the 32-ray groups that stop together differ between the two windows, and the images agree
        to the termination bound (each net_out within 2 eps = 1e-4 of the untruncated one) -- tests/test_render_gpu.py.

        maps: None (the call it always was: same launches, same bits), or a dict in the style of the field kernels' aux protocol --
        its keys name what the frame should also produce, the dict receives the tensors; an empty dict = "depth", "opacity" and
        "depth_u8" (a callable is called for the dict: render_frames' per-frame form).  What the reference's second loop writes next
        to the image (inference_givenstyle_depth, scenedreamer.py:812-844), made by csrc/maps.hip (scenedreamer_amd/maps.py):
          "depth" f32 [H,W]: sum over the samples of weight x sample depth (:816), cropped like the image;
          "opacity" f32 [H,W]: sum of the weights;
          "depth_u8" uint8 [H,W]: the pixels of the reference's depth/%05d.png (:835-844);
          "range" int32[2]: the f32 bit patterns of the smallest / largest positive depth, (0x7F800000, 0) if nothing was hit;
          "weights" / "sample_depth" f32 [window rays, ns]: the per-sample arrays the maps were made from, and
          "window" (always set): (rows, cols, crop) of those arrays -- the crop is the image's, pad // 2 - apron offset.
        The per-sample arrays come from the field launch itself: "fused" launches fused.field_render(aux={}) on the frame's window
        (for that launch early termination is off and no 32-ray group is skipped, as the aux protocol says; colour_terms 2 has no
        such launch and raises), "exact" fused.field_exact(aux={}), "unfused" field_unfused(aux={}) per ray chunk."""
        if callable(maps):
            maps = maps()
        if maps is not None:
            unknown = set(maps) - set(MAP_OUTPUTS) - {"window"}
            if unknown:
                raise ValueError(f"maps: unknown keys {sorted(unknown)}; known: {list(MAP_OUTPUTS)}")
        ev = _Stamps(timers)
        with torch.no_grad():
            ev.mark("start")
            if _precast is None:
                vid, d2, rd, cam_res = self.cast_rays(pose, resolution_hw)
            else:
                vid, d2, rd, cam_res = _precast
            ev.mark("rvip")
            Hp, Wp = cam_res
            R = Hp * Wp
            vid, d2, rd = self.flat_rays(vid, d2, rd)
            # host value for the fused path (its C entry points take host floats): a device copy here and the .cpu() that
            # would undo it are two host<->device synchronisations per frame, each draining the launch queue
            cam_ori = torch.as_tensor(pose[0], dtype=torch.float32)
            if mode not in ("fused", "exact", "unfused"):
                raise ValueError(mode)
            if mode == "unfused":
                cam_ori = cam_ori.to(self.dev)
            if mode == "fused":
                # per-style precision gates (once per style; a host synchronisation on the style's first frame) -- before the sky
                # MLP of this frame, whose hidden-layer form is one of the decisions
                if self.field_gate is None and P.FIELD_GATE:
                    self.calibrate_style(pose, resolution_hw, num_samples)
                if self.field_falls_back():      # this style / these weights are outside the fused path's tolerance: the fp32 op
                    mode = self.field_gate["path"]       # sequence, all of it (sky MLP and CNN included), or with the field on the
                    if mode == "unfused":                # fp32 MFMA kernel ("exact", Renderer.fallback)
                        cam_ori = cam_ori.to(self.dev)
            cnn_mode = self._resolve_cnn_mode(mode, cnn_mode)      # (validated before any work is done)
            sky_c, sky_avg = self.sky(rd, self._resolve_sky_mode(mode))
            ev.mark("sky")
            crop = self.pad // 2
            window = None
            if mode != "unfused":
                # rows / columns of the padded frame that cannot influence the cropped image are not evaluated: the field
                # kernels read the frame-wide ray arrays through a window (no strided-slice copies).  "fused" with cnn=False
                # takes the whole padded frame, as a window too (its launch takes the 8 x 4-pixel ray blocks); "exact" keeps the
                # minimal apron also then: nothing in that kernel depends on which rays share a launch
                o = self.apron_offset(apron, mode, minimal=cnn or mode == "exact")
                window = fused.Window.crop(Hp, Wp, o)
                Hp, Wp, crop = Hp - 2 * o, Wp - 2 * o, crop - o
            aux = {} if maps is not None else None      # (an empty dict: "weights" + "depth")
            if mode == "unfused":
                outs, auxes = [], []
                for r0 in range(0, R, ray_chunk):
                    r1 = min(r0 + ray_chunk, R)
                    if aux is not None:
                        auxes.append({})
                    outs.append(self.field_unfused(vid[r0:r1], d2[:, r0:r1], rd[r0:r1], cam_ori, sky_c[r0:r1],
                                                   sky_avg, num_samples, **({"aux": auxes[-1]} if aux is not None else {})))
                net_out = torch.cat(outs, dim=0)
                if aux is not None:
                    aux = {k: torch.cat([a[k] for a in auxes], dim=0).contiguous() for k in ("weights", "depth")}
            elif mode == "fused" and aux is not None:
                net_out = fused.field_render(self, vid.contiguous(), d2.contiguous(), rd.contiguous(), cam_ori, sky_c, sky_avg, num_samples,
                                             window=window, aux=aux)
            elif mode == "fused":
                net_out = fused.field_fused(self, vid, d2, rd, cam_ori, sky_c, sky_avg, num_samples, window=window)
            else:
                net_out = fused.field_exact(self, vid, d2, rd, cam_ori, sky_c, sky_avg, num_samples, window=window, aux=aux)
            net_out = net_out.view(1, Hp, Wp, 64)
            if maps is not None:
                self._fill_maps(maps, aux["weights"], aux["depth"], Hp, Wp, crop)
            ev.mark("field")
            if not cnn:
                ev.done()
                return net_out
            img = self._run_cnn(cnn_mode, net_out)
            if crop:
                img = img[:, :, crop:-crop, crop:-crop]
            ev.mark("cnn")
            ev.done()
            return img

    def _fill_maps(self, maps, weights, sample_depth, rows, cols, crop):
        """render_frame's `maps` dict from the per-sample arrays of its field launch (scenedreamer_amd/maps.py, current stream)."""
        from . import maps as M
        want = (set(maps) - {"window"}) or set(MAP_DEFAULT)
        depth, opacity, rng = M.depth_maps(weights, sample_depth, rows, cols, crop, opacity="opacity" in want)
        made = {"depth": depth, "opacity": opacity, "range": rng, "weights": weights, "sample_depth": sample_depth}
        if "depth_u8" in want:
            made["depth_u8"] = M.quantise(depth, rng, 8)
        for k in want:
            maps[k] = made[k]
        maps["window"] = (rows, cols, crop)

    def render_frames(self, poses, *args, maps=None, **kw):
        """The frames of a trajectory, software-pipelined over two streams (a generator): pipeline.render_frames.
        maps: None, or what every frame should produce next to its image (render_frame's `maps`): a dict whose keys are copied into a
        fresh dict per frame, or a callable that returns that fresh dict.  The generator then yields (image, maps dict) pairs.
        Frames rendered with maps leave the deep pipelined path: the next frame's ray casting still runs on the side stream, the
        rest of each frame is render_frame's own sequence (the field launch with its per-sample outputs, then the map kernels)."""
        if maps is None:
            return pipeline.render_frames(self, poses, *args, **kw)
        return self._frames_with_maps(poses, maps, args, kw)

    def _frames_with_maps(self, poses, maps, args, kw):
        fresh = maps if callable(maps) else (lambda: dict.fromkeys(k for k in maps if k != "window"))
        made = []

        def per_frame():
            made.append(fresh())
            return made[-1]

        for img in pipeline.render_frames(self, poses, *args, maps=per_frame, **kw):
            yield img, made.pop()
