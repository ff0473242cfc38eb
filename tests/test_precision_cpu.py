"""The single home of the precision state (scenedreamer_amd/precision.py): every resolver's precedence, and what each of the four
reset callers forgets.  No GPU, no library: attributes and environment variables only."""
import types

import pytest
import torch


def _objects():
    """A Renderer nobody initialised, a drop-in Backend, and a Backend nobody initialised (nothing set at all)."""
    from scenedreamer_amd import modules
    from scenedreamer_amd.renderer import Renderer
    return [object.__new__(Renderer), modules.Backend(), modules.Backend.__new__(modules.Backend)]


def _rows():
    from scenedreamer_amd import fused
    from scenedreamer_amd.precision import TERM_EPS_DEFAULT
    # resolver, attribute, (value, resolved), environment variable, (text, resolved), decision attribute, (value, resolved), default
    return [
        (lambda o: fused.precision_profile(o)[0], "colour_terms", (3, 3), "SDN_MLP_COLOUR_TERMS", ("2", 2), "colour_terms_auto", (3, 3), 6),
        (lambda o: fused.precision_profile(o)[1], "term_eps", (0.0, 0.0), "SDN_TERM_EPS", ("1e-3", 1e-3), None, None, float(TERM_EPS_DEFAULT)),
        (fused.sky_terms, "sky_terms", (6, 6), "SDN_SKY_TERMS", ("3", 3), "sky_terms_auto", (6, 6), 3),
        (fused.single_kernel, "field_single_kernel", (True, True), "SDN_FIELD_SINGLE_KERNEL", ("0", False), None, None, True),
        (fused.colour_skip, "colour_skip", (True, True), "SDN_COLOUR_SKIP", ("false", False), None, None, True),
        (lambda o: o._exact_cnn_mode(), "exact_cnn", ("torch", "torch"), "SDN_EXACT_CNN", ("f32", "f32"), None, None, "torch"),
        (lambda o: o._exact_sky_mode(), "exact_sky", ("torch", "torch"), "SDN_EXACT_SKY", ("f32", "f32"), None, None, "torch"),
        (lambda o: o._fallback_mode(), "fallback", ("exact", "exact"), None, None, None, None, "unfused"),
        (lambda o: o.explicit_cnn_terms(), "cnn_terms3x3", (3, 3), "SDN_CNN_TERMS", ("1113", "1113"), None, None, None),
        (lambda o: o.explicit_colour_terms(), "colour_terms", (3, 3), "SDN_MLP_COLOUR_TERMS", ("2", 2), None, None, None),
        (lambda o: o.explicit_sky_terms(), "sky_terms", (6, 6), "SDN_SKY_TERMS", ("3", 3), None, None, None),
    ]


ENV = ("SDN_MLP_COLOUR_TERMS", "SDN_TERM_EPS", "SDN_SKY_TERMS", "SDN_FIELD_SINGLE_KERNEL", "SDN_COLOUR_SKIP", "SDN_EXACT_CNN", "SDN_EXACT_SKY",
       "SDN_CNN_TERMS")


@pytest.mark.parametrize("row", range(11))
def test_resolver_precedence(monkeypatch, row):
    """Explicit attribute > environment variable > per-style decision > default, the same on a Renderer and on a Backend."""
    resolve, attr, attr_v, env, env_v, auto, auto_v, default = _rows()[row]
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for o in _objects():
        assert resolve(o) == default
        if auto:
            setattr(o, auto, auto_v[0])
            assert resolve(o) == auto_v[1] != default
        if env:
            monkeypatch.setenv(env, env_v[0])
            assert resolve(o) == env_v[1] and (not auto or env_v[1] != auto_v[1])
        setattr(o, attr, attr_v[0])
        assert resolve(o) == attr_v[1] and (not env or attr_v[1] != env_v[1])
        if env:
            monkeypatch.delenv(env)
            assert resolve(o) == attr_v[1]


def test_the_explicit_resolvers_ignore_the_decisions(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for o in _objects():
        o.colour_terms_auto, o.sky_terms_auto, o.cnn_calibration = 3, 6, {"terms3x3": 1}
        assert o.explicit_colour_terms() is None and o.explicit_sky_terms() is None and o.explicit_cnn_terms() is None


def test_validation_messages(monkeypatch):
    for o in _objects():
        monkeypatch.setenv("SDN_EXACT_CNN", "fp32")
        with pytest.raises(ValueError, match=r"Renderer.exact_cnn \(or SDN_EXACT_CNN\) must be 'torch' or 'f32', not 'fp32'"):
            o._exact_cnn_mode()
        monkeypatch.delenv("SDN_EXACT_CNN")
        o.exact_sky = "fused"
        with pytest.raises(ValueError, match=r"Renderer.exact_sky \(or SDN_EXACT_SKY\) must be 'torch' or 'f32', not 'fused'"):
            o._exact_sky_mode()
        o.fallback = "torch"
        with pytest.raises(ValueError, match="Renderer.fallback must be 'unfused' or 'exact', not 'torch'"):
            o._fallback_mode()


# --------------------------------------------------------------------------------------------------------- resets
DECISIONS = ("field_gate", "colour_terms_auto", "sky_terms_auto", "cnn_calibration")


def _decided(o):
    o.field_gate, o.colour_terms_auto, o.sky_terms_auto, o.cnn_calibration = {"path": "fused"}, 3, 6, {"terms3x3": 1}
    o._mfma_cnns = {1: object()}
    return o


def _survivors(o):
    return {k for k in DECISIONS if getattr(o, k) is not None} | ({"forms"} if o._mfma_cnns else set())


def _zero_weights():
    """The parameters set_scene and set_style_code read, all zero, in the reference's shapes (views of one zero: nothing to fill)."""
    z = lambda *shape: torch.zeros(1).expand(*shape)
    w = {"world_encoder.sconv_head.weight": z(8, 11, 3, 3), "world_encoder.sconv_head.bias": z(8),
         "world_encoder.hconv_head.weight": z(8, 1, 3, 3), "world_encoder.hconv_head.bias": z(8),
         "world_encoder.fc1.weight": z(16, 512), "world_encoder.fc1.bias": z(16), "world_encoder.fc2.weight": z(2, 16), "world_encoder.fc2.bias": z(2),
         "render_net.fc_1.bias": z(256), "sky_net.fc_z_a.weight": z(256, 256),
         "denoiser.fc_z_cond.weight": z(1024, 256), "denoiser.fc_z_cond.bias": z(1024)}
    for i in range(5):
        c = 16 << i
        w[f"world_encoder.conv_blocks.{i}.layers.0.weight"] = z(c, c, 3, 3)
        w[f"world_encoder.conv_blocks.{i}.layers.2.weight"] = z(2 * c, c, 3, 3)
    for i in (2, 3, 4, 5, 6):
        n = f"render_net.fc_{i}"
        w.update({n + ".weight": z(256, 256), n + ".weight_alpha": z(256, 256), n + ".bias_alpha": z(256), n + ".weight_beta": z(256, 256),
                  n + ".bias_beta": z(256)})
    return w


@pytest.fixture(scope="module")
def renderer():
    from scenedreamer_amd.renderer import Renderer
    R = object.__new__(Renderer)
    R.dev, R.w = torch.device("cpu"), _zero_weights()
    return R


def test_a_scene_change_keeps_the_cnn_record_and_forms(renderer):
    scene = types.SimpleNamespace(voxel_t=torch.zeros((4, 8, 8), dtype=torch.int32), current_height_map=torch.zeros(1, 1, 4, 4),
                                  current_semantic_map=torch.zeros(1, 11, 4, 4))
    _decided(renderer).set_scene(scene)
    assert _survivors(renderer) == {"cnn_calibration", "forms"}


def test_a_style_change_keeps_the_cnn_forms_only(renderer):
    _decided(renderer).set_style_code(torch.zeros(1, 256))
    assert _survivors(renderer) == {"forms"}          # (cnn_calibration: dropped by fold_denoiser, with the FiLM vectors)


def test_set_precision_forgets_everything():
    for o in _objects():
        _decided(o).set_precision(cnn_terms3x3=3)
        assert _survivors(o) == set() and o.cnn_terms3x3 == 3 and o.colour_terms is None and o.term_eps is None


def test_agree_precision_keeps_the_cnn_forms_only(renderer):
    from scenedreamer_amd import dist
    seen = []

    def calibrate_style(pose, hw, ns, more_poses=()):
        seen.append(_survivors(renderer))
        renderer.field_gate = {"measurements": {}}
        return renderer.field_gate
    _decided(renderer).calibrate_style = calibrate_style
    try:
        dist.agree_precision(renderer, None, (8, 8), 4)
    finally:
        del renderer.calibrate_style
    assert seen == [{"forms"}]


def test_a_backend_is_not_a_renderer():
    from scenedreamer_amd import modules
    B = modules.Backend()
    assert not any(hasattr(B, name) for name in ("set_scene", "render_frame", "band_prepare"))
    assert all(hasattr(B, name) for name in ("set_precision", "mfma_cnn", "f32_cnn", "_cnn_form", "_drop_other_cnn_planes"))
