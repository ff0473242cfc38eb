"""Host side of the fp32 render CNN (csrc/cnn_f32.hip, cnn.F32CNN, Renderer.exact_cnn): the entry points, the argument checks that
fail before a launch, the cnn_mode resolution, and the qualifier of the kernel's summation order -- one fmaf chain over a 3x3
layer's 2304 products is outside the 4 x E32 rule, one chain per tap is inside it."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import cnn_f32_ref as CR
import field_layout as FL
from scenedreamer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sdn_conv_f32_packed_weight_bytes", "sdn_conv_pack_weights_f32", "sdn_conv_f32")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdnative.h")).read(), flags=re.S)


def _codes():
    hdr = open(os.path.join(ROOT, "include", "sdnative.h")).read()
    val = lambda n: int(re.search(rf"\b{n}\s*=?\s*(-?\d+)", hdr).group(1))
    return val("SDN_ERR_INVALID"), val("SDN_ERR_UNSUPPORTED")


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
    for cin, taps in ((64, 1), (256, 1), (256, 9)):
        assert lib.sdn_conv_f32_packed_weight_bytes(cin, taps) == 256 * cin * taps * 4       # every weight once
    assert lib.sdn_conv_f32_packed_weight_bytes(64, 9) == 0 and lib.sdn_conv_f32_packed_weight_bytes(128, 1) == 0
    assert lib.sdn_abi_version() == capi.ABI_VERSION == 5          # the entries are additive


def test_bad_arguments_fail_before_a_launch():
    lib = capi.lib()
    inv, unsup = _codes()
    p, q = ctypes.c_void_p(64), ctypes.c_void_p(128)          # never dereferenced
    assert lib.sdn_conv_pack_weights_f32(p, 64, 9, p, None) == unsup and "unsupported (cin, taps) = (64, 9)" in _msg(lib)
    assert lib.sdn_conv_pack_weights_f32(None, 256, 9, p, None) == inv and "null pointer" in _msg(lib)
    call = lambda **kw: lib.sdn_conv_f32(*{**dict(in_rows=p, cin=256, taps=9, packed=p, bias=None, resid=None, mod_w=None, mod_b=None,
                                                   out_rows=q, proj_w=None, proj_b=None, out_img=None, out_raw=None, H=4, W=4,
                                                   n_workgroups=0, stream=None), **kw}.values())
    assert call(cin=128) == unsup and "unsupported (cin, taps) = (128, 9)" in _msg(lib)
    assert call(taps=4) == unsup
    assert call(cin=64) == unsup                              # 3x3 on 64 channels
    assert call(in_rows=None) == inv and "sdn_conv_f32: null pointer" in _msg(lib)
    assert call(packed=None) == inv
    assert call(H=0) == inv and "H * W" in _msg(lib)
    assert call(mod_w=p) == inv and "go together" in _msg(lib)
    assert call(proj_w=p) == inv
    assert call(out_img=p) == inv and "need proj_w" in _msg(lib)
    assert call(out_rows=None) == inv and "no output" in _msg(lib)
    assert call(out_rows=p) == unsup and "cannot write the rows it reads" in _msg(lib)       # taps == 9, out_rows == in_rows


def test_exact_cnn_is_validated(monkeypatch):
    from scenedreamer_amd.renderer import Renderer
    monkeypatch.delenv("SDN_EXACT_CNN", raising=False)
    r = Renderer.__new__(Renderer)
    assert Renderer.exact_cnn is None and r._exact_cnn_mode() == "torch"          # the default
    r.exact_cnn = "f32"
    assert r._exact_cnn_mode() == "f32"
    for bad in ("mfma", "F32", "", 3):
        r.exact_cnn = bad
        with pytest.raises(ValueError, match="exact_cnn"):
            r._exact_cnn_mode()
        with pytest.raises(ValueError, match="exact_cnn"):
            r._resolve_cnn_mode("exact", None)
    r.exact_cnn = None
    monkeypatch.setenv("SDN_EXACT_CNN", "f32")          # the environment supplies it when the attribute is unset
    assert r._exact_cnn_mode() == "f32" and r._resolve_cnn_mode("exact", None) == "f32"
    r.exact_cnn = "torch"
    assert r._exact_cnn_mode() == "torch"
    r.exact_cnn = None
    monkeypatch.setenv("SDN_EXACT_CNN", "fast")
    with pytest.raises(ValueError, match="SDN_EXACT_CNN"):
        r._exact_cnn_mode()


@pytest.mark.parametrize("path,exact_cnn,cnn_mode,runs", CR.resolution_rows())
def test_cnn_mode_resolution(path, exact_cnn, cnn_mode, runs, monkeypatch):
    from scenedreamer_amd import renderer as rmod
    assert rmod.resolve_cnn_mode(path, cnn_mode, exact_cnn) == runs
    monkeypatch.delenv("SDN_EXACT_CNN", raising=False)
    r = rmod.Renderer.__new__(rmod.Renderer)
    r.exact_cnn = exact_cnn
    assert r._resolve_cnn_mode(path, cnn_mode) == runs


def test_cnn_mode_resolution_rejects_unknown_values():
    from scenedreamer_amd import renderer as rmod
    assert rmod.resolve_cnn_mode("exact") == "torch" and rmod.resolve_cnn_mode("fused") == "mfma"      # the default row
    with pytest.raises(ValueError):
        rmod.resolve_cnn_mode("exact", "fp32")
    with pytest.raises(ValueError):
        rmod.resolve_cnn_mode("exact", None, "mfma")
    with pytest.raises(ValueError):
        rmod.resolve_cnn_mode("tiled")


def test_cli_has_the_switch():
    from scenedreamer_amd import cli
    ap = cli.build_parser()
    assert ap.parse_args(["--output_dir", "x"]).exact_cnn is None
    assert ap.parse_args(["--output_dir", "x", "--exact-cnn", "f32"]).exact_cnn == "f32"
    with pytest.raises(SystemExit):
        ap.parse_args(["--output_dir", "x", "--exact-cnn", "mfma"])


@pytest.mark.parametrize("layer", ["conv2a", "conv3b"])
def test_chain_length_qualifier(weights_full, layer):
    """Why the kernel keeps a second accumulator set.  On conv_inputs((9, 33)), against F.conv2d in fp64 and in units of the error
    E32 of F.conv2d in fp32: ONE fmaf chain over the 2304 products of a 3x3 layer is outside the 4 x E32 rule the fp32 kernels are
    held to (measured 6.4 - 6.8), a chain per tap (256 products, the nine partial sums added in f32) is within 2 x E32 (measured
    1.2 - 1.5)."""
    from oracle import field_ref as FR
    hw = (9, 33)
    x = FL.rows_to_nchw(FL.conv_inputs(hw)["x"], hw)
    w = FR.T(weights_full, f"denoiser.{layer}.weight")
    truth = F.conv2d(x.double(), w.double(), padding=1)
    e32 = FL.max_err(F.conv2d(x, w, padding=1), truth)
    one = FL.max_err(CR.chain_conv(x, w, 2304), truth)
    per_tap = FL.max_err(CR.chain_conv(x, w, 256), truth)
    print(f"{layer} 9x33: E32 {e32:.3e}; one 2304-chain {one / e32:.2f} x E32; per-tap chains {per_tap / e32:.2f} x E32")
    assert one > 4 * e32, (one, e32)
    assert per_tap <= 2 * e32, (per_tap, e32)


def test_chain_emulation_is_a_convolution(weights_full):
    """The emulation itself: with a segment of one product it is a plain f32 sum of exact products, and at any segment length it
    agrees with F.conv2d to rounding -- taps, padding and channel order are right."""
    from oracle import field_ref as FR
    hw = (3, 2)
    x = FL.rows_to_nchw(FL.conv_inputs(hw)["x"], hw)
    w = FR.T(weights_full, "denoiser.conv2a.weight")
    truth = F.conv2d(x.double(), w.double(), padding=1)
    for seg in (1, 256, 2304):
        assert FL.max_err(CR.chain_conv(x, w, seg), truth) < 1e-5 * float(truth.abs().max())
    w1 = FR.T(weights_full, "denoiser.conv4a.weight")
    assert FL.max_err(CR.chain_conv(x, w1, 256), F.conv2d(x.double(), w1.double())) < 1e-5 * float(truth.abs().max())
