"""The fp32 field rung without a GPU: argument checks of its C entry points (before any launch), the fallback switch of
Renderer.adopt_precision on a fixed measurement record, the command line."""
import ctypes

import pytest

from scenedreamer_amd import capi

SDN_ERR_INVALID, SDN_ERR_UNSUPPORTED = -1, -2


def _codes():
    """(SDN_ERR_INVALID, SDN_ERR_UNSUPPORTED) as include/sdnative.h defines them."""
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sdnative.h")).read()
    val = lambda n: int(re.search(rf"\b{n}\s*=?\s*(-?\d+)", hdr).group(1))
    return val("SDN_ERR_INVALID"), val("SDN_ERR_UNSUPPORTED")


def _msg(lib):
    return lib.sdn_last_error().decode()


def test_entry_points_are_exported_and_sized():
    lib = capi.lib()
    assert lib.sdn_abi_version() == 5
    # every weight once, as f32: fc_1 + 5 hidden layers + fc_out_c
    assert lib.sdn_field_f32_packed_weight_bytes() == 4 * (256 * 128 + 5 * 256 * 256 + 64 * 256)
    assert lib.sdn_field_f32_consts_floats() == lib.sdn_field_consts_floats()


def test_pack_and_raw_mlp_reject_bad_arguments():
    lib = capi.lib()
    inv, _ = _codes()
    p = ctypes.c_void_p(64)          # never dereferenced: every check below fails before a launch
    five = (ctypes.c_void_p * 5)(64, 64, 64, 64, 64)
    assert lib.sdn_field_pack_weights_f32(None, five, p, p, None) == inv and "null pointer" in _msg(lib)
    assert lib.sdn_field_pack_weights_f32(p, five, p, None, None) == inv
    hole = (ctypes.c_void_p * 5)(64, 64, None, 64, 64)
    assert lib.sdn_field_pack_weights_f32(p, hole, p, p, None) == inv and "null hidden weight" in _msg(lib)
    assert lib.sdn_render_mlp_f32(None, p, p, p, p, p, 32, 0, None) == inv and "sdn_render_mlp_f32: null pointer" in _msg(lib)
    assert lib.sdn_render_mlp_f32(p, p, p, p, p, None, 32, 0, None) == inv
    assert lib.sdn_render_mlp_f32(p, p, p, p, p, p, 0, 0, None) == inv and "n_rows" in _msg(lib)
    assert lib.sdn_render_mlp_f32(p, p, p, p, p, p, 1 << 31, 0, None) == inv


def _render_args(**over):
    p = ctypes.c_void_p(64)
    f3 = (ctypes.c_float * 3)(0, 0, 0)
    f2 = (ctypes.c_float * 2)(0, 0)
    a = dict(voxel_id=p, depth2=p, raydirs=p, lut=p, table3=p, table_rows=1 << 19, scales=p, genc=f2, ori=f3, dims=f3, lin=p, u=None,
             n_rays=64, max_blocks=6, num_samples=24, sample_depth=3.0, dists_scale=0.25, packed=p, consts=p, sky_c=p, sky_avg=p,
             net_out=p, n_workgroups=0, window=None, ori_dev=None, stream=None)
    a.update(over)
    return list(a.values())


def test_field_render_f32_rejects_bad_arguments():
    lib = capi.lib()
    inv, unsup = _codes()
    call = lambda **kw: lib.sdn_field_render_f32(*_render_args(**kw))
    for name in ("voxel_id", "depth2", "raydirs", "lut", "table3", "scales", "genc", "dims", "lin", "packed", "consts", "sky_c", "net_out"):
        assert call(**{name: None}) == inv, name
        assert "sdn_field_render_f32: null pointer" in _msg(lib), name
    assert call(u=ctypes.c_void_p(64)) == unsup and "deterministic sampling only" in _msg(lib)
    assert call(n_rays=0) == inv and "empty frame" in _msg(lib)
    assert call(n_rays=-5) == inv
    assert call(num_samples=0) == inv
    assert call(num_samples=80) == unsup and "at most 79 samples" in _msg(lib)
    assert call(max_blocks=9) == unsup and "max_blocks" in _msg(lib)
    assert call(table_rows=1000) == inv and "power of two" in _msg(lib)
    # windows: outside the source rays; a blocked order over part of a window
    w6 = ctypes.c_int32 * 6
    assert call(window=w6(64, 8, 0, 8, 0, 0), n_rays=72) == inv and "reaches outside" in _msg(lib)
    assert call(window=w6(640, 10, 0, 9, 3, 2), n_rays=63) == inv and "blocked ray order" in _msg(lib)
    assert call(window=w6(0, 8, 0, 8, 0, 0)) == inv and "bad ray window" in _msg(lib)


MEAS = dict(explicit_colour=None, explicit_cnn=None, explicit_sky=None, colour_diff=4e-5, field_err={3: 5e-3, 6: 5e-3},
            image_err={1: 9e-4, 3: 2e-4}, cnn_diff=9e-4, cnn_diffs={1: 9e-4}, sky_err={3: 1e-5, 6: 1e-4}, pixels=1000, rays=2000,
            samples_per_ray=24, frame="fixed")


def _adopt(fallback=None):
    from scenedreamer_amd.renderer import Renderer
    R = Renderer.__new__(Renderer)          # adopt_precision is a function of `meas` and of `fallback` alone
    if fallback is not None:
        R.fallback = fallback
    import copy
    return R, R.adopt_precision(copy.deepcopy(MEAS))


def test_adopt_precision_routes_a_closed_gate_by_fallback():
    D, d = _adopt()
    assert D.fallback == "unfused" and d["path"] == "unfused" and D.field_falls_back()
    E, e = _adopt("exact")
    assert e["path"] == "exact" and E.field_falls_back()
    assert {k: v for k, v in d.items() if k != "path"} == {k: v for k, v in e.items() if k != "path"}
    assert D.cnn_calibration == E.cnn_calibration
    # an open gate is "fused" whatever the fallback
    import copy
    ok = copy.deepcopy(MEAS)
    ok["field_err"] = {3: 5e-5, 6: 6e-5}
    from scenedreamer_amd.renderer import Renderer
    for fb in ("unfused", "exact"):
        R = Renderer.__new__(Renderer)
        R.fallback = fb
        assert R.adopt_precision(copy.deepcopy(ok))["path"] == "fused" and not R.field_falls_back()
    R.fallback = "torch"
    with pytest.raises(ValueError):
        R.adopt_precision(copy.deepcopy(MEAS))


def test_cli_accepts_mode_exact():
    from scenedreamer_amd import cli
    ap = cli.build_parser()
    assert ap.parse_args(["--output_dir", "o", "--mode", "exact"]).mode == "exact"
    assert ap.parse_args(["--output_dir", "o"]).mode == "fused"
    with pytest.raises(SystemExit):
        ap.parse_args(["--output_dir", "o", "--mode", "f32"])
