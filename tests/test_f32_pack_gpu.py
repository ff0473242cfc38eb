"""The three fp32 pack kernels on the MI355X (sdn_field_pack_weights_f32, sdn_sky_pack_weights_f32, sdn_conv_pack_weights_f32)
against tests/f32_pack_layout.py, the numpy restatement of the layout comment in csrc/mlp_f32.h that tests/test_f32_pack_cpu.py
qualifies.  Every weight is a distinct integer below 2^24 that names its own place, so the packed stream is compared with
torch.equal: a weight in a wrong place, a missing one or a stray one is a mismatch."""
import ctypes

import pytest
import torch

import f32_pack_layout as PL
from scenedreamer_amd import capi

pytestmark = pytest.mark.gpu


def _packed(n_bytes, call):
    out = torch.full((n_bytes // 4,), -1.0, device="cuda")
    capi.check(call(out.data_ptr(), capi.current_stream(out.device)), "pack")
    torch.cuda.synchronize()
    return out.cpu()


def _mlp_pack(entry, n_bytes, mats):
    dev = [torch.from_numpy(m).cuda() for m in mats]
    w1, *wh, wc = dev
    ptrs = (ctypes.c_void_p * len(wh))(*[t.data_ptr() for t in wh])
    return _packed(n_bytes, lambda out, st: entry(w1.data_ptr(), ptrs, wc.data_ptr(), out, st))


def test_field_stream():
    lib = capi.lib()
    assert lib.sdn_field_f32_packed_weight_bytes() == 4 * PL.FIELD_CHUNKS * PL.CHUNK_FLOATS
    mats = PL.position_weights([(256, 128)] + [(256, 256)] * 5 + [(64, 256)])
    got = _mlp_pack(lib.sdn_field_pack_weights_f32, lib.sdn_field_f32_packed_weight_bytes(), mats)
    assert torch.equal(got, torch.from_numpy(PL.field_stream(mats[0], mats[1:6], mats[6])))


def test_sky_stream():
    lib = capi.lib()
    assert lib.sdn_sky_f32_packed_weight_bytes() == 4 * PL.SKY_CHUNKS * PL.CHUNK_FLOATS
    mats = PL.position_weights([(256, 33)] + [(256, 256)] * 4 + [(64, 256)])
    got = _mlp_pack(lib.sdn_sky_pack_weights_f32, lib.sdn_sky_f32_packed_weight_bytes(), mats)
    assert torch.equal(got, torch.from_numpy(PL.sky_stream(mats[0], mats[1:5], mats[5])))


@pytest.mark.parametrize("taps,cin", PL.CONV_SHAPES)
def test_conv_stream(taps, cin):
    lib = capi.lib()
    kh = 3 if taps == 9 else 1
    assert lib.sdn_conv_f32_packed_weight_bytes(cin, taps) == 4 * 256 * cin * taps
    w, = PL.position_weights([(256, cin, kh, kh)])
    wd = torch.from_numpy(w).cuda()
    got = _packed(4 * 256 * cin * taps, lambda out, st: lib.sdn_conv_pack_weights_f32(wd.data_ptr(), cin, taps, out, st))
    assert torch.equal(got, torch.from_numpy(PL.conv_stream(w)))
