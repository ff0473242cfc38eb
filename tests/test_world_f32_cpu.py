"""Host side of the fixed-order world encoder and style MLP (csrc/world_f32.hip, fused.world_exact / style_exact,
Renderer.exact_world / exact_style): the entry points, the argument checks that fail before a launch, the two knobs, the restatement
of the kernels' orders (tests/world_f32_ref.py) against the network, and the qualifier of those orders."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import field_layout as FL
import world_f32_ref as WR
from scenedreamer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sdn_wenc_f32_packed_weight_bytes", "sdn_wenc_pack_weights_f32", "sdn_wenc_head_f32", "sdn_wenc_conv_f32", "sdn_wenc_tail_f32",
           "sdn_style_mlp_f32")


@pytest.fixture(scope="module")
def weights():
    """The synthetic weights without the hash table (the encoders' are the same arrays as weights_full's: seeded by name)."""
    from scenedreamer_amd import synth
    return synth.make_weights(0, with_embeddings=False)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdnative.h")).read(), flags=re.S)


def _codes():
    hdr = open(os.path.join(ROOT, "include", "sdnative.h")).read()
    val = lambda n: int(re.search(rf"\b{n}\s*=?\s*(-?\d+)", hdr).group(1))
    return val("SDN_ERR_INVALID"), val("SDN_ERR_UNSUPPORTED")


def _msg(lib):
    lib.sdn_last_error.restype = ctypes.c_char_p
    return lib.sdn_last_error().decode()


# ----------------------------------------------------------------------------------------------------- 1, 2: the C ABI

def test_entry_points_are_exported_declared_and_sized():
    lib = capi.lib()
    hdr = _header()
    for name in ENTRIES:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(rf"\b{name}\s*\(", hdr), f"{name} is not declared in include/sdnative.h"
        assert name in capi.declared_symbols()
    for cin, cout, _ in WR.PAIRS:
        n = lib.sdn_wenc_f32_packed_weight_bytes(cin, cout)
        assert n >= 4 * 9 * cin * cout and n % 16 == 0, (cin, cout, n)
        assert n == 4 * 9 * cin * max(cout, 32)             # every weight once; COUT 16 is a 32-block with a zero upper half
    for cin, cout in ((64, 256), (8, 16), (16, 64), (32, 16), (512, 512), (0, 0), (48, 48)):
        assert lib.sdn_wenc_f32_packed_weight_bytes(cin, cout) == 0, (cin, cout)
    assert lib.sdn_abi_version() == capi.ABI_VERSION == 5          # the entries are additive


def test_bad_arguments_fail_before_a_launch():
    lib = capi.lib()
    inv, unsup = _codes()
    p, q = ctypes.c_void_p(64), ctypes.c_void_p(128)          # never dereferenced
    assert lib.sdn_wenc_pack_weights_f32(p, 64, 256, p, None) == unsup and "unsupported (cin, cout) = (64, 256)" in _msg(lib)
    assert lib.sdn_wenc_pack_weights_f32(None, 16, 16, p, None) == inv and "null pointer" in _msg(lib)
    assert lib.sdn_wenc_pack_weights_f32(p, 16, 16, None, None) == inv

    head = lambda **kw: lib.sdn_wenc_head_f32(*{**dict(height=p, semantic=p, wh=p, bh=p, ws=p, bs=p, out_rows=q, H=4, W=4, n_workgroups=0,
                                                       stream=None), **kw}.values())
    for k in ("height", "semantic", "wh", "bh", "ws", "bs", "out_rows"):
        assert head(**{k: None}) == inv and "sdn_wenc_head_f32: null pointer" in _msg(lib), k
    assert head(H=0) == inv and "H * W" in _msg(lib)
    assert head(W=-3) == inv
    assert head(H=1 << 16, W=1 << 15) == inv and "H * W" in _msg(lib)          # 2^31

    conv = lambda **kw: lib.sdn_wenc_conv_f32(*{**dict(in_rows=p, cin=16, cout=16, stride=1, packed=p, out_rows=q, H=4, W=4, n_workgroups=0,
                                                       stream=None), **kw}.values())
    assert conv(cout=64) == unsup and "unsupported (cin, cout, stride) = (16, 64, 1)" in _msg(lib)
    assert conv(stride=2) == unsup and conv(cout=32) == unsup and conv(cin=8, cout=8) == unsup and conv(stride=0) == unsup
    assert conv(cin=512, cout=512) == unsup
    for k in ("in_rows", "packed", "out_rows"):
        assert conv(**{k: None}) == inv and "sdn_wenc_conv_f32: null pointer" in _msg(lib), k
    assert conv(H=0) == inv and "H * W" in _msg(lib)
    assert conv(H=1 << 16, W=1 << 15) == inv
    assert conv(out_rows=p) == unsup and "cannot write the rows it reads" in _msg(lib)

    tail = lambda **kw: lib.sdn_wenc_tail_f32(*{**dict(rows=p, P=3, fc1_w=p, fc1_b=p, fc2_w=p, fc2_b=p, pooled=None, global_enc=q, stream=None),
                                                **kw}.values())
    for k in ("rows", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "global_enc"):
        assert tail(**{k: None}) == inv and "sdn_wenc_tail_f32: null pointer" in _msg(lib), k
    assert tail(P=0) == inv and "P must be >= 1" in _msg(lib)

    six = (ctypes.c_void_p * 6)(*[64] * 6)
    holed = (ctypes.c_void_p * 6)(64, 64, None, 64, 64, 64)
    assert lib.sdn_style_mlp_f32(None, six, six, q, 1, None) == inv and "sdn_style_mlp_f32: null pointer" in _msg(lib)
    assert lib.sdn_style_mlp_f32(p, None, six, q, 1, None) == inv and lib.sdn_style_mlp_f32(p, six, None, q, 1, None) == inv
    assert lib.sdn_style_mlp_f32(p, six, six, None, 1, None) == inv
    assert lib.sdn_style_mlp_f32(p, six, six, q, 0, None) == inv and "n must be >= 1" in _msg(lib)
    assert lib.sdn_style_mlp_f32(p, holed, six, q, 1, None) == inv and "null layer pointer" in _msg(lib)
    assert lib.sdn_style_mlp_f32(p, six, holed, q, 1, None) == inv


# ----------------------------------------------------------------------------------------------------- 3: the knobs

@pytest.mark.parametrize("knob,env", [("exact_world", "SDN_EXACT_WORLD"), ("exact_style", "SDN_EXACT_STYLE")])
def test_knobs_are_validated(monkeypatch, knob, env):
    from scenedreamer_amd.renderer import Renderer
    mode = lambda r: getattr(r, f"_{knob}_mode")()
    for attr, envval, runs in WR.resolution_rows():
        r = Renderer.__new__(Renderer)
        monkeypatch.delenv(env, raising=False)
        if envval is not None:
            monkeypatch.setenv(env, envval)
        if attr is not None:
            setattr(r, knob, attr)
        assert mode(r) == runs, (attr, envval)
    monkeypatch.delenv(env, raising=False)
    r = Renderer.__new__(Renderer)
    assert getattr(Renderer, knob) is None and Renderer.encoders is None
    for bad in ("mfma", "F32", "", 3):
        setattr(r, knob, bad)
        with pytest.raises(ValueError, match=knob):
            mode(r)
    setattr(r, knob, None)
    monkeypatch.setenv(env, "fast")
    with pytest.raises(ValueError, match=env):
        mode(r)


def test_constructor_keywords_and_cli_switches():
    import inspect
    from scenedreamer_amd import cli
    from scenedreamer_amd.renderer import Renderer
    sig = inspect.signature(Renderer.__init__).parameters
    assert sig["exact_world"].default is None and sig["exact_style"].default is None
    with pytest.raises(ValueError, match="exact_world"):          # validated before anything is computed with it
        r = Renderer.__new__(Renderer)
        r.exact_world = "fast"
        r._exact_world_mode()
    ap = cli.build_parser()
    a = ap.parse_args(["--output_dir", "x"])
    assert a.exact_world is None and a.exact_style is None
    a = ap.parse_args(["--output_dir", "x", "--exact-world", "f32", "--exact-style", "f32"])
    assert a.exact_world == "f32" and a.exact_style == "f32"
    assert ap.parse_args(["--output_dir", "x", "--exact-style", "torch"]).exact_style == "torch"
    for sw in ("--exact-world", "--exact-style"):
        with pytest.raises(SystemExit):
            ap.parse_args(["--output_dir", "x", sw, "mfma"])


def test_module_classes_load_the_state_dict_and_default_to_the_composite_forward(weights):
    """modules.ConditionalHashGrid / StyleMLP carry the reference's parameter names; without sdn_exact (and on the CPU even with it)
    the forward is the composite one, which is the network."""
    from oracle import field_ref as FR
    from scenedreamer_amd import modules
    net = modules.ConditionalHashGrid()
    net.load_state_dict({k[len("world_encoder."):]: torch.as_tensor(np.asarray(v)) for k, v in weights.items() if k.startswith("world_encoder.")})
    sty = modules.StyleMLP(128, 256)
    sty.load_state_dict({k[len("style_net."):]: torch.as_tensor(np.asarray(v)) for k, v in weights.items() if k.startswith("style_net.")})
    hm, sm = WR.maps((12, 10), 0)
    s = WR.styles([0, 1])
    with torch.no_grad():
        g, z = net(hm, sm), sty(s)
        assert FL.max_err(g, FR.world_encoder(weights, hm, sm, torch.float64)) < 1e-5
        assert FL.max_err(z, FR.style_mlp(weights, s, torch.float64)) < 1e-4
        net.sdn_exact = sty.sdn_exact = True          # CPU tensors: served by the composite forward, with the reason recorded
        assert torch.equal(net(hm, sm), g) and torch.equal(sty(s), z)
    assert "CUDA" in net.__dict__["_sdn_composite_reason"] and "CUDA" in sty.__dict__["_sdn_composite_reason"]
    assert modules.is_native(net) and modules.is_native(sty)


# ----------------------------------------------------------------------------------------------------- 4: the restatement is the network

def test_restatement_is_the_network(weights):
    from oracle import field_ref as FR
    hm, sm = WR.maps((12, 10), 0)
    enc = WR.lib_encode(weights, hm, sm, torch.float64)
    assert FL.max_err(enc["global_enc"], FR.world_encoder(weights, hm, sm, torch.float64)) <= 1e-12
    s = WR.styles(range(4))
    truth = FR.style_mlp(weights, s, torch.float64)
    assert FL.max_err(WR.lib_style(weights, s, torch.float64), truth) <= 1e-12
    assert FL.max_err(WR.style_ref(weights, s), truth) <= 1e-5 * float(truth.abs().max())
    # the kernels' orders, end to end, are the same function to fp32 rounding
    ch = WR.chain_encode(weights, hm, sm)
    for name in WR.LAYER_NAMES + ("pooled", "global_enc"):
        assert ch[name].numel() == enc[name].numel() and tuple(ch[name].shape[-1:]) == tuple(enc[name].shape[-1:]), name
        assert FL.max_err(ch[name].reshape(enc[name].shape), enc[name])<= 1e-5 * max(float(enc[name].abs().max()), 1.0), name


@pytest.mark.parametrize("hw", [(5, 4), (1, 1)])
@pytest.mark.parametrize("stride", [1, 2])
def test_chain_conv_is_a_convolution(weights, hw, stride):
    """Taps, padding, stride and channel order of the emulation: it agrees with F.conv2d to rounding."""
    rng = np.random.default_rng(1251 + 10 * hw[0] + stride)
    x = torch.from_numpy(rng.normal(size=(1, 32) + hw).astype(np.float32))
    w = WR.T(weights, f"conv_blocks.1.layers.{0 if stride == 1 else 2}.weight")
    truth = F.conv2d(x.double(), w.double(), stride=stride, padding=1)
    got = WR.chain_conv(x, w, stride)
    assert tuple(got.shape) == tuple(truth.shape) == (1, w.shape[0], WR.half(hw[0]) if stride == 2 else hw[0], WR.half(hw[1]) if stride == 2 else hw[1])
    assert FL.max_err(got, truth) <= 1e-5 * float(truth.abs().max())


# ----------------------------------------------------------------------------------------------------- 5: the order qualifier

def test_order_qualifier(weights):
    """Why the orders are what they are.  On the (70, 52) maps, every layer in isolation (its input the f32-rounded fp64 activation
    of the layer before) with per-tap chains is within 2 x E32 of fp64, E32 = the error of F.conv2d in fp32 on the same input
    (measured: at most 1.29); the style MLP with f64 accumulation is within 1 x E32 on 8 seeded styles (measured: 0.25 - 0.37)."""
    from oracle import field_ref as FR
    hm, sm = WR.maps(WR.YARD_HW, 0)
    truth = WR.lib_encode(weights, hm, sm, torch.float64)
    x, sem = hm, sm
    for name in WR.LAYER_NAMES:
        t = WR.lib_layer(weights, name, x, sem, torch.float64)
        e32 = FL.max_err(WR.lib_layer(weights, name, x, sem, torch.float32), t)
        e = FL.max_err(WR.chain_layer(weights, name, x, sem), t)
        print(f"{name:24s} {tuple(t.shape)} E32 {e32:.3e}  per-tap chains {e / e32:.2f} x E32")
        assert t.numel() >= 1024 and e <= 2 * e32, (name, e, e32)
        x, sem = truth[name].to(torch.float32), None
    s = WR.styles(range(8))
    t = FR.style_mlp(weights, s, torch.float64)
    e32 = FL.max_err(FR.style_mlp(weights, s, torch.float32), t)
    e = FL.max_err(WR.style_ref(weights, s), t)
    print(f"style MLP, 8 styles: E32 {e32:.3e}  f64 accumulation {e / e32:.2f} x E32")
    assert e <= e32, (e, e32)
