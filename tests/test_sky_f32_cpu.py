"""Host side of the fp32 sky MLP (csrc/sky_f32.hip, fused.sky_exact, Renderer.exact_sky): the entry points, the argument checks that
fail before a launch, the sky-mode resolution, and the two qualifiers the GPU test leans on -- a k-ordered fmaf chain through all
six layers is within 2 x E32 of fp64 (so the kernel is held to the project's 4 x E32), and the kernel's order of adding the frame
mean is within 8 u mean|x| of the f64 mean."""
import ctypes
import os
import re

import pytest
import torch

import field_layout as FL
import sky_f32_ref as SF
from scenedreamer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sdn_sky_f32_packed_weight_bytes", "sdn_sky_pack_weights_f32", "sdn_sky_f32_partial_rows", "sdn_sky_mlp_f32")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdnative.h")).read(), flags=re.S)


def _invalid():
    hdr = open(os.path.join(ROOT, "include", "sdnative.h")).read()
    return int(re.search(r"\bSDN_ERR_INVALID\s*=?\s*(-?\d+)", hdr).group(1))


def _msg(lib):
    lib.sdn_last_error.restype = ctypes.c_char_p
    return lib.sdn_last_error().decode()


def test_entry_points_are_exported_declared_and_sized():
    lib = capi.lib()
    hdr = _header()
    for name in ENTRIES:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(rf"\b{name}\s*\(", hdr), f"{name} is not declared in include/sdnative.h"
        assert name in capi.declared_symbols()
    assert lib.sdn_abi_version() == capi.ABI_VERSION == 5          # the entries are additive
    assert lib.sdn_sky_f32_packed_weight_bytes() >= 4 * (33 * 256 + 4 * 256 * 256 + 64 * 256)      # every weight once
    assert lib.sdn_sky_f32_packed_weight_bytes() % 32768 == 0                                      # whole 32 KiB chunks
    rows = lib.sdn_sky_f32_partial_rows
    assert rows(1, 1) == 4 and rows(0, 4) == 0
    sizes, grids = (1, 31, 32, 33, 128, 129, 1001, 530464), (1, 2, 3, 64, 256, 1024)
    for n in sizes:
        for g in grids:
            assert rows(n, g) > 0 and rows(n, g) % 4 == 0
            assert rows(n, g) <= 4 * g and rows(n, g) <= 4 * -(-n // 128)          # a workgroup takes 128 rays at a time
    for g in grids:          # monotone in the ray count ...
        assert all(rows(a, g) <= rows(b, g) for a, b in zip(sizes, sizes[1:]))
    for n in sizes:          # ... and in the workgroup count
        assert all(rows(n, a) <= rows(n, b) for a, b in zip(grids, grids[1:]))
    assert rows(530464, 0) == rows(530464, 256) == 1024          # n_workgroups <= 0: 256


def test_bad_arguments_fail_before_a_launch():
    lib = capi.lib()
    inv = _invalid()
    p, q = ctypes.c_void_p(64), ctypes.c_void_p(128)          # never dereferenced
    ptrs = (ctypes.c_void_p * 4)(64, 64, 64, 64)
    assert lib.sdn_sky_pack_weights_f32(None, ptrs, p, p, None) == inv and "null pointer" in _msg(lib)
    assert lib.sdn_sky_pack_weights_f32(p, (ctypes.c_void_p * 4)(64, 64, None, 64), p, p, None) == inv and "null hidden weight" in _msg(lib)
    call = lambda **kw: lib.sdn_sky_mlp_f32(*{**dict(raydirs=p, packed=p, consts=p, sky_c=q, sky_partial=q, n_rays=100, n_workgroups=0,
                                                     sky_avg=q, counter=q, encoded=0, stream=None), **kw}.values())
    assert call(raydirs=None) == inv and "sdn_sky_mlp_f32" in _msg(lib)
    assert call(packed=None) == inv and call(consts=None) == inv and call(sky_c=None) == inv and call(sky_partial=None) == inv
    assert call(n_rays=0) == inv and call(n_rays=-5) == inv
    assert call(counter=None) == inv and "go together" in _msg(lib)
    assert call(sky_avg=None) == inv and "go together" in _msg(lib)
    assert call(encoded=2) == inv and "encoded" in _msg(lib)


def test_exact_sky_is_validated(monkeypatch):
    from scenedreamer_amd.renderer import Renderer
    monkeypatch.delenv("SDN_EXACT_SKY", raising=False)
    r = Renderer.__new__(Renderer)
    assert Renderer.exact_sky is None and r._exact_sky_mode() == "torch"          # the default
    r.exact_sky = "f32"
    assert r._exact_sky_mode() == "f32"
    for bad in ("fused", "F32", "", 3):
        r.exact_sky = bad
        with pytest.raises(ValueError, match="exact_sky"):
            r._exact_sky_mode()
        with pytest.raises(ValueError, match="exact_sky"):
            r._resolve_sky_mode("exact")
        assert r._resolve_sky_mode("fused") == "fused" and r._resolve_sky_mode("unfused") == "torch"      # (read on the exact path only)
    r.exact_sky = None
    monkeypatch.setenv("SDN_EXACT_SKY", "f32")          # the environment supplies it when the attribute is unset
    assert r._exact_sky_mode() == "f32" and r._resolve_sky_mode("exact") == "f32"
    r.exact_sky = "torch"                                # the attribute wins
    assert r._exact_sky_mode() == "torch" and r._resolve_sky_mode("exact") == "torch"
    r.exact_sky = None
    monkeypatch.setenv("SDN_EXACT_SKY", "fast")
    with pytest.raises(ValueError, match="SDN_EXACT_SKY"):
        r._exact_sky_mode()


@pytest.mark.parametrize("path,exact_sky,runs", SF.resolution_rows())
@pytest.mark.parametrize("via", ["attribute", "environment"])
def test_sky_mode_resolution(path, exact_sky, runs, via, monkeypatch):
    from scenedreamer_amd import renderer as rmod
    assert rmod.resolve_sky_mode(path, exact_sky) == runs
    r = rmod.Renderer.__new__(rmod.Renderer)
    if via == "attribute":
        monkeypatch.setenv("SDN_EXACT_SKY", "torch" if exact_sky == "f32" else "f32")      # (the attribute wins over it)
        r.exact_sky = exact_sky
    else:
        monkeypatch.setenv("SDN_EXACT_SKY", exact_sky)
    assert r._resolve_sky_mode(path) == runs


def test_sky_mode_resolution_rejects_unknown_values():
    from scenedreamer_amd import renderer as rmod
    assert rmod.resolve_sky_mode("exact") == "torch" and rmod.resolve_sky_mode("fused") == "fused"      # the default row
    with pytest.raises(ValueError):
        rmod.resolve_sky_mode("exact", "fused")
    with pytest.raises(ValueError):
        rmod.resolve_sky_mode("exact", None)
    with pytest.raises(ValueError):
        rmod.resolve_sky_mode("tiled")


def test_precision_string_names_what_runs(monkeypatch):
    from scenedreamer_amd.renderer import Renderer
    monkeypatch.delenv("SDN_EXACT_SKY", raising=False)
    monkeypatch.delenv("SDN_EXACT_CNN", raising=False)
    r = Renderer.__new__(Renderer)
    default = r.compute_dtype("exact")
    assert default == "f32 (field: hash grid + f32-input MFMA with f32 accumulate; sky MLP and render CNN: PyTorch)"      # as it was
    r.exact_sky = "f32"
    s = r.compute_dtype("exact")
    assert "sky MLP: f32-input MFMA" in s and "render CNN: PyTorch" in s
    r.exact_cnn = "f32"
    s = r.compute_dtype("exact")
    assert "sky MLP: f32-input MFMA" in s and "render CNN: f32-input MFMA" in s and "PyTorch" not in s
    r.exact_sky = None
    s = r.compute_dtype("exact")
    assert "sky MLP: PyTorch" in s and "render CNN: f32-input MFMA" in s
    assert r.compute_dtype("unfused") == "f32"


def test_cli_has_the_switch():
    from scenedreamer_amd import cli
    ap = cli.build_parser()
    assert ap.parse_args(["--output_dir", "x"]).exact_sky is None
    assert ap.parse_args(["--output_dir", "x", "--exact-sky", "f32"]).exact_sky == "f32"
    with pytest.raises(SystemExit):
        ap.parse_args(["--output_dir", "x", "--exact-sky", "fused"])


def test_sky_cache_is_dropped_with_the_f16_one():
    """_fused_sky_f32 is invalidated wherever _fused_sky is: a new style code, a module backend that moved to another device."""
    import types
    from scenedreamer_amd import modules, renderer
    ns = types.SimpleNamespace(w={"sky_net.fc_z_a.weight": torch.zeros(256, 8)}, _fused_sky=object(), _fused_sky_f32=object())
    renderer.fold_sky_net(ns, torch.ones(1, 8))
    assert ns._fused_sky is None and ns._fused_sky_f32 is None and tuple(ns.sky_z.shape) == (1, 256)
    b = modules.Backend()
    assert b._fused_sky is None and b._fused_sky_f32 is None
    b.bind("sky_net.", torch.nn.Linear(3, 2))
    b._fused_sky, b._fused_sky_f32 = object(), object()
    b.bind("sky_net.", torch.nn.Linear(3, 2, device="meta"))
    assert b._fused_sky is None and b._fused_sky_f32 is None


@pytest.fixture(scope="module")
def sky_case(weights_full):
    """The arithmetic tests' sky inputs, evaluated once: encoded rows, fp64 truth, E32, the k-ordered chain."""
    from oracle import split_ref as SR
    pe = FL.sky_encoded(FL.sky_dirs())
    z = FL.style_code()
    truth = SR.sky_mlp_ref(weights_full, pe, z, torch.float64)
    e32 = FL.max_err(SR.sky_mlp_ref(weights_full, pe, z, torch.float32), truth)
    chain = SF.chain_sky_mlp(SR.fold_sky_mlp(weights_full, z), pe)
    return pe, truth, e32, chain


def test_summation_order_is_qualified(sky_case):
    """A k-ordered chain acc = fl32(fl64(acc) + fl64(w) fl64(x)) through all six layers -- what the MFMA computes, up to the order
    of k inside a layer -- on the 1001 directions of the arithmetic tests stays within 2 x E32 of fp64, E32 being the error of the
    reference's own fp32 arithmetic (measured with a numpy encoding: chain 1.53e-6, E32 1.66e-6, ratio 0.92).  Holding the kernel
    to FL.FACTOR = 4 x E32 therefore leaves room for its k order and for nothing coarser than fp32."""
    pe, truth, e32, chain = sky_case
    assert tuple(pe.shape) == (1001, 33) and tuple(chain.shape) == (1001, 64)
    e = FL.max_err(chain, truth)
    print(f"sky MLP, 1001 directions: E32 {e32:.3e}; k-ordered chain {e:.3e} = {e / e32:.2f} x E32")
    assert e32 > 0 and e <= 2 * e32, (e, e32)
    assert FL.FACTOR == 4.0


def test_mean_order_is_within_its_bound(sky_case):
    """A depth-5 f32 tree over 32 values, then f64, then one rounding errs by at most 5 u mean|x| + u |mean| per feature (u = 2^-24):
    the restatement of the kernel's order is held to 8 u mean|x| against the f64 mean of the same sky_c, n = 1001 (the last tile is
    ragged).  An all-f32 running sum over the 1001 rows is not inside it by construction; the tree's own error is not zero."""
    _, _, _, chain = sky_case
    avg = SF.tree_mean(chain)
    assert avg.dtype == torch.float32 and tuple(avg.shape) == (64,)
    worst = SF.check_mean(avg, chain)
    print(f"tree_mean vs f64 mean, n = 1001: worst feature at {worst:.3f} of the bound 8 u mean|x|")
    # the bound is a bound on THIS order, not a tautology: a mean that is off by one part in 2^16 is outside it
    with pytest.raises(AssertionError):
        SF.check_mean(avg * (1 + 2.0 ** -16), chain)
    # and for sizes that are one tile, less than one, and whole tiles
    for n in (1, 31, 32, 33, 128):
        SF.check_mean(SF.tree_mean(chain[:n]), chain[:n])
