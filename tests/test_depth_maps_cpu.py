"""Depth and opacity maps without a GPU: the two C entry points' argument checks (before any launch), the numpy restatement of
csrc/maps.hip (tests/depth_maps_ref.py) qualified on arrays built from the three reference goldens, output.MapWriter on CPU tensors,
the command line."""
import ctypes
import os

import numpy as np
import pytest
import torch

import depth_maps_ref as ref
from conftest import golden

INV = -1          # SDN_ERR_INVALID (include/sdnative.h)


def _msg(lib):
    return lib.sdn_last_error().decode()


@pytest.fixture(autouse=True, scope="module")
def _the_entries_exist():
    """Everything below is about sdn_depth_maps / sdn_depth_quantise -- also the restatement, which is only worth qualifying as the
    statement of what those two compute."""
    from scenedreamer_amd import capi
    assert {"sdn_depth_maps", "sdn_depth_quantise"} <= set(capi.declared_symbols()), "this library has no depth-map entry points"


# ---- 1. the C boundary ----------------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported_and_the_abi_is_5():
    from scenedreamer_amd import capi
    lib = capi.lib()
    assert lib.sdn_abi_version() == 5
    assert {"sdn_depth_maps", "sdn_depth_quantise"} <= set(capi.declared_symbols())
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sdnative.h")).read()
    assert "int sdn_depth_maps(" in hdr and "int sdn_depth_quantise(" in hdr and "scenedreamer.py:816" in hdr


def _maps_args(**over):
    p = ctypes.c_void_p(64)          # never dereferenced: every check below fails before a launch
    a = dict(weights=p, sample_depth=p, rows=8, cols=8, num_samples=4, crop=1, depth_map=p, opacity=p, range_bits=p, n_workgroups=0, stream=None)
    a.update(over)
    return list(a.values())


def test_depth_maps_rejects_bad_arguments():
    from scenedreamer_amd import capi
    lib = capi.lib()
    call = lambda **kw: lib.sdn_depth_maps(*_maps_args(**kw))
    for name in ("weights", "sample_depth", "depth_map", "range_bits"):
        assert call(**{name: None}) == INV and "sdn_depth_maps: null pointer" in _msg(lib), name
    for kw in (dict(rows=0), dict(cols=0), dict(rows=-3)):
        assert call(**kw) == INV and "rows and cols must be >= 1" in _msg(lib), kw
    assert call(num_samples=0) == INV and "num_samples must be >= 1" in _msg(lib)
    assert call(crop=-1) == INV and "crop must be >= 0" in _msg(lib)
    for kw in (dict(crop=4), dict(rows=2, crop=1), dict(cols=6, crop=3), dict(crop=1 << 30)):
        assert call(**kw) == INV and "leaves nothing" in _msg(lib), kw
    assert call(rows=1 << 16, cols=1 << 15, crop=0) == INV and "beyond int32" in _msg(lib)
    assert call(rows=1 << 12, cols=1 << 12, num_samples=128, crop=0) == INV and "beyond int32" in _msg(lib)


def test_depth_quantise_rejects_bad_arguments():
    from scenedreamer_amd import capi
    lib = capi.lib()
    p = ctypes.c_void_p(64)
    q = lib.sdn_depth_quantise
    assert q(None, 16, p, 8, p, 0, None) == INV and "sdn_depth_quantise: null pointer" in _msg(lib)
    assert q(p, 16, None, 8, p, 0, None) == INV and "null pointer" in _msg(lib)
    assert q(p, 16, p, 8, None, 0, None) == INV and "null pointer" in _msg(lib)
    for n in (0, -1):
        assert q(p, n, p, 8, p, 0, None) == INV and "n must be >= 1" in _msg(lib)
    assert q(p, 1 << 31, p, 8, p, 0, None) == INV and "beyond int32" in _msg(lib)
    for bits in (0, 1, 7, 9, 12, 32, -8):
        assert q(p, 16, p, bits, p, 0, None) == INV and "bits must be 8 or 16" in _msg(lib), bits


# ---- 2. the restatement on the goldens -------------------------------------------------------------------------------------------------
def _golden_arrays(tag):
    """(weights f32 [n,ns], depth f32 [n,ns], H, W) of golden `tag`: the volume-rendering weights (mc_utils.py:154-161) evaluated in
    float64 from the recorded `sigma` and `rand_depth` -- the distance of sample s is depth[s+1] - depth[s], the last one repeated,
    times dists_scale = 0.25; rays that hit nothing (voxel_id[..., 0] == 0) have weight zero (scenedreamer.py:373-376) -- and cast to
    float32; the depths after the NaN / inf -> 0 replacement (scenedreamer.py:346-352)."""
    g = golden(f"field_{tag}.npz")
    ns = int(g["num_samples"])
    H, W = g["net_out"].shape[1:3]
    sig = g["sigma"].reshape(-1, ns).astype(np.float64)
    z = g["rand_depth"].reshape(-1, ns)
    z = np.where(np.isfinite(z), z, 0).astype(np.float32)
    d = np.diff(z.astype(np.float64), axis=1)
    d = np.concatenate([d, d[:, -1:]], axis=1)
    fe = np.maximum(sig, 0) * d * 0.25
    excl = np.concatenate([np.zeros_like(fe[:, :1]), np.cumsum(fe, axis=1)[:, :-1]], axis=1)
    w = (1 - np.exp(-fe)) * np.exp(-excl)
    w[g["voxel_id"].reshape(-1, g["voxel_id"].shape[-2])[:, 0] == 0] = 0
    return w.astype(np.float32), z, H, W


@pytest.fixture(scope="module", params=["a", "b", "c"])
def case(request):
    w, z, H, W = _golden_arrays(request.param)
    depth, opacity = ref.composite(w, z, H, W)
    t_depth = torch.sum(torch.from_numpy(w) * torch.from_numpy(z), -1).reshape(H, W)      # scenedreamer.py:816 in float32
    return dict(tag=request.param, w=w, z=z, H=H, W=W, depth=depth, opacity=opacity, torch_depth=t_depth)


def test_restated_depth_is_no_worse_than_torch_sum(case):
    """Against the float64 sum of the exact products.  Measured on these arrays (restatement | torch.sum in float32):
    field_a 7.6e-6 | 2.7e-5, field_b 7.5e-6 | 3.1e-5, field_c 7.3e-6 | 1.4e-5."""
    exact = (case["w"].astype(np.float64) * case["z"].astype(np.float64)).sum(axis=1).reshape(case["H"], case["W"])
    e_ref = float(np.abs(case["depth"] - exact).max())
    e_torch = float(np.abs(case["torch_depth"].numpy() - exact).max())
    print(f"field_{case['tag']}: restated depth vs fp64 {e_ref:.2e}; torch.sum float32 vs fp64 {e_torch:.2e}")
    assert int((case["depth"] > 0).sum()) > 500 and int((case["depth"] == 0).sum()) > 100        # scene and sky
    assert e_ref <= e_torch
    assert float(case["opacity"].max()) <= 1 + 1e-5 and np.array_equal(case["depth"] > 0, case["opacity"] > 0)


def _reference_u8(depth):
    """scenedreamer.py:835-841 on a float32 tensor, then `* 255` (:844) and round-half-even."""
    fake = depth.clone()
    mmask = fake > 0
    tmp = fake[mmask]
    tmp = (tmp - tmp.min()) / (tmp.max() - tmp.min())
    fake[~mmask] = 1
    fake[mmask] = tmp
    return torch.round(fake * 255).to(torch.uint8).numpy()


def test_restated_u8_is_the_reference_expression(case):
    depth = case["depth"]
    rng = ref.value_range(depth)
    assert rng.dtype == np.uint32 and tuple(rng.view(np.float32)) == (depth[depth > 0].min(), depth.max())
    u8 = ref.quantise(depth, rng, 8)
    assert u8.dtype == np.uint8 and np.array_equal(u8, _reference_u8(torch.from_numpy(depth)))
    assert u8.min() == 0 and u8.max() == 255 and np.all(u8[depth <= 0] == 255)


def test_u8_of_torch_depth_and_restated_depth_agree(case):
    t = case["torch_depth"].numpy()
    a, b = ref.quantise(t, ref.value_range(t), 8), ref.quantise(case["depth"], ref.value_range(case["depth"]), 8)
    n = int((a != b).sum())
    print(f"field_{case['tag']}: depth_u8 from torch's depth vs the restated depth: {n} of {a.size} pixels differ")
    assert n == 0


def test_restatement_edge_rules():
    d = np.array([[np.nan, -1.0, 0.0, np.inf], [2.0, 2.0, 2.0, 2.0]], np.float32)
    rng = ref.value_range(d)
    assert tuple(rng.view(np.float32)) == (2.0, 2.0)
    assert ref.quantise(d, rng, 8).tolist() == [[255] * 4, [0] * 4]                                # hi == lo -> 0
    none = np.array([[0.0, -3.0, np.nan]], np.float32)
    assert tuple(int(v) for v in ref.value_range(none)) == ref.NO_HIT
    assert ref.quantise(none, ref.value_range(none), 16).tolist() == [[65535] * 3]
    metric = np.array([0.0, 100.0], np.float32).view(np.uint32)
    assert ref.quantise(np.array([50.0, 100.0, 250.0, 1e-3], np.float32), metric, 16).tolist() == [32768, 65535, 65535, 1]
    # ties go to even: 0.5 / 255 * 255 and 1.5 / 255 * 255 in float32 are exactly 0.5 and 1.5
    half = np.array([0.5, 1.5, 2.5], np.float32)
    assert ((half / np.float32(255)) * np.float32(255)).tolist() == [0.5, 1.5, 2.5]
    assert ref.quantise(half, np.array([0.0, 255.0], np.float32).view(np.uint32), 8).tolist() == [0, 2, 2]


# ---- 3. MapWriter ----------------------------------------------------------------------------------------------------------------------
def test_map_writer_round_trip_and_errors(tmp_path):
    from PIL import Image
    from scenedreamer_amd.output import MapWriter
    g = np.random.default_rng(3)
    a8 = g.integers(0, 256, (9, 13), dtype=np.uint8)
    a16 = g.integers(0, 65536, (9, 13), dtype=np.uint16)
    a16[0, :3] = (0, 255, 65535)
    for bits, arr, mode in ((8, a8, "L"), (16, a16, "I;16")):
        w = MapWriter(str(tmp_path / f"d{bits}"), bits=bits)
        w.submit(torch.from_numpy(arr), 0)
        w.submit(torch.from_numpy(arr.T.copy()).t(), 7)          # a non-contiguous view
        w.close()
        assert w.maps_done == 2 and sorted(os.listdir(tmp_path / f"d{bits}")) == ["00000.png", "00007.png"]
        for name in ("00000.png", "00007.png"):
            im = Image.open(tmp_path / f"d{bits}" / name)
            assert im.mode == mode and im.size == (13, 9) and np.array_equal(np.asarray(im), arr)
    with pytest.raises(ValueError):
        MapWriter(str(tmp_path / "bad"), bits=12)
    w = MapWriter(str(tmp_path / "d8"), bits=8)
    with pytest.raises(ValueError):
        w.submit(torch.from_numpy(a16), 1)                       # the wrong element type
    w.close()
    # a worker's error comes back from close()
    w = MapWriter(str(tmp_path / "gone"), bits=8)
    os.rmdir(tmp_path / "gone")
    w.submit(torch.from_numpy(a8), 0)
    with pytest.raises(OSError):
        w.close()


# ---- 4. the command line ---------------------------------------------------------------------------------------------------------------
def test_cli_depth_flags(capsys):
    from scenedreamer_amd import cli
    ap = cli.build_parser()
    d = ap.parse_args(["--output_dir", "o"])
    assert d.depth_maps == "off" and d.depth_max is None
    assert ap.parse_args(["--output_dir", "o", "--depth-maps", "u8"]).depth_maps == "u8"
    a = ap.parse_args(["--output_dir", "o", "--depth-maps", "u16", "--depth-max", "120.5"])
    assert a.depth_maps == "u16" and a.depth_max == 120.5
    for bad in (["--depth-maps", "u16"], ["--depth-maps", "u12"], ["--depth-maps", "u16", "--depth-max", "0"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["--output_dir", "o"] + bad)
    assert "--depth-max" in capsys.readouterr().err


def test_band_parallel_frames_refuse_maps():
    from scenedreamer_amd import dist as sdist
    with pytest.raises(ValueError, match="band-parallel"):
        sdist.render_frame_tile_parallel(None, None, (8, 8), 4, maps={})
