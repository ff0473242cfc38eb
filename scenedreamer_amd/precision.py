"""The precision state of a renderer: the knobs a caller sets, the per-style decisions the calibration reaches, the caches
that hang off both, and the bounds the decisions are held to.  `PrecisionState` is the base of renderer.Renderer and
modules.Backend -- what fused.*, cnn.MfmaCNN and calibration.* expect of either.

Every knob resolves the same way -- explicit attribute, else its environment variable, else the per-style decision, else
the default -- and each resolver below is the only place that reads its environment variable.  The bounds are read from
this module at call time (`precision.FIELD_AUTO_BOUND`): tests patch them here."""
import os

from .cnn import F32CNN, MfmaCNN, form_key

EXACT_CNN_MODES = ("torch", "f32")
EXACT_SKY_MODES = ("torch", "f32")
EXACT_WORLD_MODES = ("torch", "f32")
EXACT_STYLE_MODES = ("torch", "f32")
CNN_MODES = ("mfma", "torch", "f32")

CNN_AUTO_BOUND = 5e-4   # mfma_cnn: largest image difference (max abs) at which the 1-term 3x3 convolutions are accepted
CNN_CAL_PIXELS = 400_000   # ... measured on every net_out of a style until this many pixels have been compared
IMAGE_BUDGET = 8e-4        # ... and only while (field error charged) + (that difference) stays below this (north star: 1e-3)
FIELD_NOMINAL_ERR = 2e-4   # field error charged to the budget when no field_gate was measured (goldens: 1.0 - 1.6e-4)
# calibrate_style (the renderer's end-to-end gates; the north star's tolerance is 1e-3 abs on radiance and on the image):
COLOUR_AUTO_BOUND = 1e-4   # largest net_out difference fp6-corrected vs 3-term colour layers (goldens: 4e-5)
FIELD_AUTO_BOUND = 1e-3    # largest net_out error of the fused field vs the fp32 op sequence, whole frame: the north star's radiance
                           # tolerance itself.  Measured on the synthetic weights (tools/dbg_field_err.py): max over the 36 M values of
                           # a 960x540 frame 5 - 6e-5 (rms 4e-6) without early termination, 9e-5 with the default term_eps -- since the
                           # trunk weights are packed times 2^8 (mlp_layers.h TRUNK_SHIFT; before that 5.6 - 8.2e-4, profiles/
                           # r04_gate_survey.jsonl: the lo halves of the split sat in f16's subnormal range, ~20 significant bits, and
                           # the density head sums ~2e3 x its result in cancelling terms).  The kernel's sigma is now as close to an
                           # fp64 evaluation as PyTorch's fp32 one is (1e-4 both).
IMAGE_AUTO_BOUND = 8e-4    # largest image error of the whole fused path vs the fp32 path, whole frame
SKY_AUTO_BOUND = 2e-4      # largest sky_c error (vs PyTorch fp32) at which the sky MLP's hidden layers run as f16 + fp6 corrections
CAL_MAX_PIXELS = 1 << 22   # frames above this many pixels (1920x1080 is below: calibrated at its own resolution) are calibrated at a reduced resolution (same pose)
CAL_CHUNK = 1 << 16        # rays per launch group of the fp32 field
CAL_CROP = 256             # calibrate_one: side of the window (output pixels) the fp32 twin and the candidates are evaluated on (0: whole frame)
CAL_CROP_FACTOR = 1.15     # ... and what a maximum measured on that window is multiplied by before it meets a bound
FIELD_GATE = os.environ.get("SDN_FIELD_GATE", "1") != "0"   # (0: no field calibration -- kernel timing experiments only)
CNN_HALO = 4   # receptive-field radius of RenderCNN: four 3x3 convolutions (conv2a, conv2b, conv3a, conv3b)

# Early ray termination is ON by default: a 32-ray group stops sampling once the transmittance of every one of its rays is below
# this (wavefront ballots, field.hip).  It moves net_out by at most 2 x eps = 1e-4 of the 1e-3 tolerance (typically far less: the
# bound assumes all of the remaining mass sits in the skipped samples); the renderer's per-style calibration measures the path
# WITH it, so the charge is inside the measured error.  On the synthetic benchmark weights it removes 2 - 6 % of the field
# kernel's passes, on an opaque-surface weight set 5 of 6 (tests/test_render_gpu.py, bench.py `early_termination`).
TERM_EPS_DEFAULT = "5e-5"
SINGLE_KERNEL_DEFAULT = "1"   # same frame time as the two-kernel sequence (A/B), without its 10.8 GB/frame of HBM hand-off


def _env_flag(name, default):
    return os.environ.get(name, default) not in ("0", "", "false")


def resolve_cnn_mode(path, cnn_mode=None, exact_cnn="torch"):
    """Which render CNN runs: path = the path actually taken ("fused"; "exact" / "unfused", asked for or adopted by a closed gate
    through Renderer.fallback), cnn_mode = the caller's explicit choice or None, exact_cnn = Renderer.exact_cnn resolved.
    Returns "mfma" (cnn.MfmaCNN), "f32" (cnn.F32CNN) or "torch" (Renderer.render_cnn)."""
    if path not in ("fused", "exact", "unfused"):
        raise ValueError(path)
    if exact_cnn not in EXACT_CNN_MODES:
        raise ValueError(f"exact_cnn must be 'torch' or 'f32', not {exact_cnn!r}")
    if cnn_mode is not None:
        if cnn_mode not in CNN_MODES:
            raise ValueError(f"cnn_mode must be one of {CNN_MODES} or None, not {cnn_mode!r}")
        return cnn_mode
    if path == "fused":
        return "mfma"
    return exact_cnn if path == "exact" else "torch"


def resolve_sky_mode(path, exact_sky="torch"):
    """Which sky MLP runs: path = the path actually taken ("fused"; "exact" / "unfused", asked for or adopted by a closed gate through
    Renderer.fallback), exact_sky = Renderer.exact_sky resolved.  Returns "fused" (fused.sky_fused, the f16-split kernel), "f32"
    (fused.sky_exact, the fp32 MFMA kernel) or "torch" (Renderer.sky_features + mean)."""
    if path not in ("fused", "exact", "unfused"):
        raise ValueError(path)
    if exact_sky not in EXACT_SKY_MODES:
        raise ValueError(f"exact_sky must be 'torch' or 'f32', not {exact_sky!r}")
    if path == "fused":
        return "fused"
    return exact_sky if path == "exact" else "torch"


class PrecisionState:
    # ---- the knobs: None = "not set explicitly" (the environment variable, else the per-style decision, else the default)
    cnn_terms3x3 = None         # f16 product terms of the four 3x3 convolutions (set_precision; SDN_CNN_TERMS)
    colour_terms = None         # products of the colour layers fc_5 / fc_6 (set_precision; SDN_MLP_COLOUR_TERMS)
    term_eps = None             # early ray termination threshold (set_precision; SDN_TERM_EPS)
    sky_terms = None            # products of the sky MLP's hidden layers (SDN_SKY_TERMS)
    field_single_kernel = None  # the field as one kernel or as encode + mlp (SDN_FIELD_SINGLE_KERNEL)
    colour_skip = None          # skip the colour branch of passes with all-zero weights (SDN_COLOUR_SKIP)
    cnn_auto_bound = None       # overrides CNN_AUTO_BOUND for this renderer
    # What a closed precision gate selects (adopt_precision): "unfused" = the reference's fp32 op sequence on PyTorch, field, sky
    # MLP and CNN; "exact" = the same with the field on the fp32 MFMA kernel (fused.field_exact).  Every rank of a distributed job
    # must be given the same value (dist.agree_precision).
    fallback = "unfused"
    # The render CNN of the "exact" path (asked for directly, or adopted through fallback = "exact"): "torch" = render_cnn, the
    # reference's F.conv2d sequence (default); "f32" = cnn.F32CNN, the fp32 MFMA kernel (csrc/cnn_f32.hip).  None = the environment
    # variable SDN_EXACT_CNN, else "torch".  An explicit cnn_mode overrides it; "unfused" stays on PyTorch.  Like `fallback`, every
    # rank of a distributed job must be given the same value: the two differ by fp32 rounding.
    exact_cnn = None
    # The sky MLP of the "exact" path, the twin of exact_cnn: "torch" = sky_features + a library mean (default); "f32" =
    # fused.sky_exact, the fp32 MFMA kernel (csrc/sky_f32.hip) with the frame mean finished inside it.  None = the environment
    # variable SDN_EXACT_SKY, else "torch".  "fused" keeps sky_fused, "unfused" stays on PyTorch.  Every rank of a distributed job
    # must be given the same value: the two differ by fp32 rounding.
    exact_sky = None
    # The two networks upstream of every frame: the world encoder of set_scene (global_enc) and the style MLP of set_style (z).
    # "torch" = the reference's F.conv2d / F.linear sequence on the libraries (default); "f32" = fused.world_exact / fused.style_exact,
    # the fixed-order kernels of csrc/world_f32.hip.  None = the environment variable SDN_EXACT_WORLD / SDN_EXACT_STYLE, else "torch".
    # Unlike exact_cnn and exact_sky these two apply in set_scene and set_style WHATEVER mode later renders: the encoders run before
    # a mode exists.  Setting the attribute takes effect at the next set_scene / set_style (Renderer takes both as constructor
    # keywords, because its __init__ already calls set_scene).  Every rank of a distributed job must be given the same value.
    exact_world = None
    exact_style = None
    encoders = None             # what ran: {"world": "torch" | "f32", "style": "torch" | "f32" | None} (set_scene, set_style)
    # ---- the per-style decisions (calibration.py; forgotten by reset_gates)
    field_gate = None           # the record of calibrate_style: path, measured errors, colour and sky forms
    cnn_calibration = None      # the record of the render CNN's 3x3 rung (calibrate_style, or the windowed gate of mfma_cnn)
    colour_terms_auto = None
    sky_terms_auto = None
    # ---- caches, created on first use (dicts through _cache)
    _mfma_cnns = None           # form key -> cnn.MfmaCNN, "f32" -> cnn.F32CNN
    _fused_scene = _fused_style = _fused_style_f32 = _fused_sky = _fused_sky_f32 = None      # fused.prepare_*
    _fused_lin = _fused_buf = None
    _fused_world_f32 = None     # fused.prepare_world_exact: the world encoder's packed convolution weights
    _row_cost_cache = None
    _side_stream = _cnn_stream = None

    def _cache(self, name):
        """The dict cache `name` declared above, created on first use."""
        d = getattr(self, name)
        if d is None:
            d = {}
            setattr(self, name, d)
        return d

    # ------------------------------------------------------------------ one resolver per knob
    def explicit_colour_terms(self):
        """colour_terms, else SDN_MLP_COLOUR_TERMS, else None (the calibration decides)."""
        if self.colour_terms is None and "SDN_MLP_COLOUR_TERMS" in os.environ:
            return int(os.environ["SDN_MLP_COLOUR_TERMS"])
        return self.colour_terms

    def resolved_colour_terms(self):
        """... else the per-style decision of calibrate_style (6 unless the fp6 corrections cost more than its bound), else 6."""
        ct = self.explicit_colour_terms()
        return ct if ct is not None else (self.colour_terms_auto or 6)

    def explicit_cnn_terms(self):
        """cnn_terms3x3, else SDN_CNN_TERMS as its text ("1", "3" or a per-layer form like "1113": cnn.form_key reads all of them),
        else None (the calibration decides)."""
        if self.cnn_terms3x3 is None:
            return os.environ.get("SDN_CNN_TERMS")
        return self.cnn_terms3x3

    def explicit_sky_terms(self):
        """sky_terms, else SDN_SKY_TERMS, else None (the calibration decides)."""
        if self.sky_terms is None and "SDN_SKY_TERMS" in os.environ:
            return int(os.environ["SDN_SKY_TERMS"])
        return self.sky_terms

    def resolved_sky_terms(self):
        """... else the per-style decision (`sky_terms_auto`), else 3."""
        return self.explicit_sky_terms() or self.sky_terms_auto or 3

    def resolved_term_eps(self):
        return self.term_eps if self.term_eps is not None else float(os.environ.get("SDN_TERM_EPS", TERM_EPS_DEFAULT))

    def resolved_single_kernel(self):
        v = self.field_single_kernel
        return bool(v if v is not None else _env_flag("SDN_FIELD_SINGLE_KERNEL", SINGLE_KERNEL_DEFAULT))

    def resolved_colour_skip(self):
        v = self.colour_skip
        return bool(v if v is not None else _env_flag("SDN_COLOUR_SKIP", "1"))

    def _fallback_mode(self):
        if self.fallback not in ("unfused", "exact"):
            raise ValueError(f"Renderer.fallback must be 'unfused' or 'exact', not {self.fallback!r}")
        return self.fallback

    def _exact_cnn_mode(self):
        v = self.exact_cnn if self.exact_cnn is not None else os.environ.get("SDN_EXACT_CNN", "torch")
        if v not in EXACT_CNN_MODES:
            raise ValueError(f"Renderer.exact_cnn (or SDN_EXACT_CNN) must be 'torch' or 'f32', not {v!r}")
        return v

    def _exact_sky_mode(self):
        v = self.exact_sky if self.exact_sky is not None else os.environ.get("SDN_EXACT_SKY", "torch")
        if v not in EXACT_SKY_MODES:
            raise ValueError(f"Renderer.exact_sky (or SDN_EXACT_SKY) must be 'torch' or 'f32', not {v!r}")
        return v

    def _exact_world_mode(self):
        """The world encoder set_scene runs: "torch" or "f32" -- in every render mode (it runs before a mode exists)."""
        v = self.exact_world if self.exact_world is not None else os.environ.get("SDN_EXACT_WORLD", "torch")
        if v not in EXACT_WORLD_MODES:
            raise ValueError(f"Renderer.exact_world (or SDN_EXACT_WORLD) must be 'torch' or 'f32', not {v!r}")
        return v

    def _exact_style_mode(self):
        """The style MLP set_style runs: "torch" or "f32" -- in every render mode (it runs before a mode exists)."""
        v = self.exact_style if self.exact_style is not None else os.environ.get("SDN_EXACT_STYLE", "torch")
        if v not in EXACT_STYLE_MODES:
            raise ValueError(f"Renderer.exact_style (or SDN_EXACT_STYLE) must be 'torch' or 'f32', not {v!r}")
        return v

    def _ran(self, which, how):
        """Record in `encoders` which implementation of the world encoder / style MLP produced the current global_enc / z."""
        e = dict(self.encoders or {"world": None, "style": None})
        e[which] = how
        self.encoders = e

    def _resolve_cnn_mode(self, path, cnn_mode):
        """Which render CNN runs on `path` (the path actually taken: "fused", "exact" or "unfused")."""
        return resolve_cnn_mode(path, cnn_mode, self._exact_cnn_mode() if (cnn_mode is None and path == "exact") else "torch")

    def _resolve_sky_mode(self, path):
        """Which sky MLP runs on `path` (the path actually taken: "fused", "exact" or "unfused")."""
        return resolve_sky_mode(path, self._exact_sky_mode() if path == "exact" else "torch")

    def field_falls_back(self):
        g = self.field_gate
        return bool(g) and g.get("path") in ("unfused", "exact")

    # ------------------------------------------------------------------ forgetting decisions
    def reset_gates(self, cnn=False, cnn_forms=False):
        """Forget the per-style decisions of the field and the sky MLP (field_gate, colour_terms_auto, sky_terms_auto): they are
        measured for one scene (the collapsed table changes with global_enc), one style and one precision profile.
        cnn: the render CNN's record too.  A scene change leaves it alone (the CNN never sees the scene's tables); a style change
        drops it through fold_denoiser, with the FiLM vectors; set_precision and dist.agree_precision start every gate afresh.
        cnn_forms: also the cache of packed CNN forms (set_precision only: a new profile may not want any of them)."""
        self.field_gate = None
        self.colour_terms_auto = None
        self.sky_terms_auto = None
        if cnn:
            self.cnn_calibration = None
        if cnn_forms:
            self._mfma_cnns = None

    def set_precision(self, cnn_terms3x3=None, colour_terms=None, term_eps=None):
        """Precision profile of the MFMA kernels (None = the default of the environment / library):
        cnn_terms3x3: f16 product terms of the four 3x3 convolutions: 1, 3, a per-layer form like "1113" (cnn.CNN_LADDER), or
                      None = "auto" (the cheapest rung of the ladder that passes the per-style calibration -- see mfma_cnn);
        colour_terms: products of the colour layers fc_5 / fc_6: 6 (default: f16 + fp6 corrections), 3 or 2 (fused.precision_profile);
        term_eps: early ray termination threshold on the transmittance, 0 = off (default)."""
        self.cnn_terms3x3, self.colour_terms, self.term_eps = cnn_terms3x3, colour_terms, term_eps
        self.reset_gates(cnn=True, cnn_forms=True)

    # ------------------------------------------------------------------ the render CNN's forms
    def _cnn_form(self, terms3x3):
        cache = self._cache("_mfma_cnns")
        terms3x3 = form_key(terms3x3)
        if terms3x3 not in cache:
            cache[terms3x3] = MfmaCNN(self, terms3x3)
        return cache[terms3x3]

    def f32_cnn(self):
        """The fp32 MFMA render CNN (cnn.F32CNN), cached beside the f16 forms (the same events drop it)."""
        cache = self._cache("_mfma_cnns")
        if "f32" not in cache:
            cache["f32"] = F32CNN(self)
        return cache["f32"]

    def _drop_other_cnn_planes(self, keep):
        """The forms not chosen keep their packed weights (9 MB each), not their activation planes (1.2 GB at 960x540)."""
        for k, c in (self._mfma_cnns or {}).items():
            if k != keep:
                c._planes.clear()

    def _drop_cnn_planes(self, H, W):
        """A window's activation planes are not the frame's: drop them, the packed weights stay."""
        for c in (self._mfma_cnns or {}).values():
            c._planes.pop((H, W), None)

    def mfma_cnn(self, net_out):
        """The MFMA render CNN (cnn.MfmaCNN) for the current precision profile.

        The four 3x3 convolutions can run as ONE f16 product (operands rounded to nearest: a third of the MFMAs, 2.9 ms
        instead of 7.3 ms per 960x540 frame) or as the 3-term f16 split (agrees with the fp32 CNN to < 2e-5).  The 1-term form
        is LOSSY -- its error grows with the activations' magnitude, i.e. it depends on the loaded weights and the style -- so
        it is not a blind default.  Who decides (cnn_terms3x3 = None, "auto"):
          * Renderer.calibrate_style, end to end, on the style's first frame (the record `cnn_calibration` then says
            `measured: end to end`): 1-term only if its image is within CNN_AUTO_BOUND of the 3-term image AND within
            IMAGE_AUTO_BOUND of the fp32 image;
          * where no fp32 twin is at hand (modules.Backend: the drop-in binding; bands rendered without dist.agree_precision), the
            windowed gate (calibration.cnn_window_gate): every net_out presented until CNN_CAL_PIXELS pixels of the style have
            been seen goes through both forms; the 1-term image is used while every comparison stayed within CNN_AUTO_BOUND and
            the charged field error plus that difference within IMAGE_BUDGET; the first violation closes the gate for the style.
        An explicit cnn_terms3x3 (set_precision, or SDN_CNN_TERMS in the environment) bypasses the gate."""
        want = self.explicit_cnn_terms()
        if want is not None:
            return self._cnn_form(want)
        cal = self.cnn_calibration
        if cal is None or (cal["terms3x3"] != 3 and cal["pixels"] < CNN_CAL_PIXELS):
            from .calibration import cnn_window_gate      # (calibration imports fused, fused imports this module)
            cal = cnn_window_gate(self, net_out)
        return self._cnn_form(cal["terms3x3"])
