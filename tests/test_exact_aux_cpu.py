"""sdn_field_render_f32_aux and the drop-in binding's exact switch without a GPU: the entry is exported, its argument checks
answer before any launch (the pointers below are never dereferenced), GeneratorBinding.exact parses its argument and
SDN_PERPIX_EXACT."""
import ctypes

import pytest

from scenedreamer_amd import capi

NAME = "sdn_field_render_f32_aux"
W6 = ctypes.c_int32 * 6


def _codes():
    """(SDN_ERR_INVALID, SDN_ERR_UNSUPPORTED) as include/sdnative.h defines them."""
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sdnative.h")).read()
    val = lambda n: int(re.search(rf"\b{n}\s*=?\s*(-?\d+)", hdr).group(1))
    return val("SDN_ERR_INVALID"), val("SDN_ERR_UNSUPPORTED")


def _msg(lib):
    return lib.sdn_last_error().decode()


def _args(**over):
    p = ctypes.c_void_p(64)
    f3 = (ctypes.c_float * 3)(0, 0, 0)
    f2 = (ctypes.c_float * 2)(0, 0)
    a = dict(voxel_id=p, depth2=p, raydirs=p, lut=p, table3=p, table_rows=1 << 19, scales=p, genc=f2, ori=f3, dims=f3, lin=p, u=None,
             n_rays=64, max_blocks=6, num_samples=24, sample_depth=3.0, dists_scale=0.25, packed=p, consts=p, sky_c=p, sky_avg=p,
             net_out=p, n_workgroups=0, window=None, ori_dev=None, strat_division=0, aux=None, stream=None)
    a.update(over)
    return list(a.values())


def _call(**kw):
    return capi.lib().sdn_field_render_f32_aux(*_args(**kw))


def test_entry_is_exported_and_the_abi_version_stays():
    lib = capi.lib()
    assert lib.sdn_abi_version() == 5 == capi.ABI_VERSION
    assert NAME in capi.declared_symbols() and callable(getattr(lib, NAME))
    # the same leading arguments as sdn_field_render_f32, then strat_division and aux in front of the stream
    a, b = capi._SIGNATURES["sdn_field_render_f32"][1], capi._SIGNATURES[NAME][1]
    assert b[:len(a) - 1] == a[:-1] and b[len(a) - 1:] == [ctypes.c_int32, capi.c_p, capi.c_p]


def test_required_pointers():
    lib = capi.lib()
    inv, _ = _codes()
    for name in ("voxel_id", "depth2", "raydirs", "lut", "table3", "scales", "genc", "dims", "lin", "packed", "consts", "sky_c", "net_out"):
        assert _call(**{name: None}) == inv, name
        assert f"{NAME}: null pointer" in _msg(lib), (name, _msg(lib))
    # the shared checks name the entry that was called
    assert _call(n_rays=0) == inv and f"{NAME}: empty frame" in _msg(lib)
    assert lib.sdn_field_render_f32(*_args(n_rays=0)[:25], None) == inv and "sdn_field_render_f32: empty frame" in _msg(lib)


def test_stochastic_sampling_is_accepted():
    lib = capi.lib()
    inv, unsup = _codes()
    u = ctypes.c_void_p(64)
    # sdn_field_render_f32 refuses u_dev outright ...
    assert lib.sdn_field_render_f32(*_args(u=u)[:25], None) == unsup and "deterministic sampling only" in _msg(lib)
    # ... the new entry goes on to the checks behind that point (a later argument is bad, so nothing launches)
    assert _call(u=u, table_rows=1000) == inv
    assert "power of two" in _msg(lib) and "deterministic sampling only" not in _msg(lib)
    for div in (0, 1):
        assert _call(u=u, strat_division=div, max_blocks=9) == unsup and "max_blocks" in _msg(lib)
    assert _call(u=u, strat_division=2) == inv and "strat_division" in _msg(lib)
    assert _call(strat_division=2) == inv and _call(strat_division=-1) == inv
    # the blocked == 2 ray order has no rows of u: INVALID, ragged window or whole blocks
    assert _call(u=u, window=W6(640, 10, 0, 9, 0, 2), n_rays=63) == inv and "blocked == 2" in _msg(lib)
    assert _call(u=u, window=W6(640, 16, 0, 16, 0, 2), n_rays=64) == inv and "blocked == 2" in _msg(lib)
    # (without u the same window passes that check: the next bad argument answers)
    assert _call(window=W6(640, 10, 0, 9, 0, 2), n_rays=63, table_rows=1000) == inv and "power of two" in _msg(lib)


def test_aux_without_colour_skipping_fields():
    lib = capi.lib()
    inv, unsup = _codes()
    p = 64
    assert _call(aux=ctypes.byref(capi.FieldAux(weights=p, colour_passes=p))) == unsup and "colour" in _msg(lib) and NAME in _msg(lib)
    assert _call(aux=ctypes.byref(capi.FieldAux(flags=capi.FIELD_NO_COLOUR_SKIP))) == unsup and NAME in _msg(lib)
    # the six outputs are accepted (a later argument is bad, so nothing launches)
    full = capi.FieldAux(weights=p, depth=p, sigma=p, colour=p, sky_blended=p, nosky=p)
    assert _call(aux=ctypes.byref(full), num_samples=80) == unsup and "at most 79 samples" in _msg(lib)
    assert _call(aux=ctypes.byref(capi.FieldAux()), n_rays=-1) == inv


def test_binding_exact_parsing(monkeypatch):
    from scenedreamer_amd import dropin
    monkeypatch.delenv("SDN_PERPIX_EXACT", raising=False)
    assert dropin.GeneratorBinding().exact is False
    assert "perpix_exact" in dropin.GeneratorBinding().stats and dropin.GeneratorBinding().stats["perpix_exact"] == 0
    for given, want in ((False, False), (True, True), ("refused", "refused"), ("1", True), ("0", False), ("", False)):
        got = dropin.GeneratorBinding(exact=given).exact
        assert got == want and type(got) is type(want) and dropin.parse_exact(given) == want
    for env, want in (("refused", "refused"), ("1", True), ("0", False)):
        monkeypatch.setenv("SDN_PERPIX_EXACT", env)
        assert dropin.GeneratorBinding().exact == want
        assert dropin.GeneratorBinding(exact=False).exact is False           # an argument outranks the environment
    monkeypatch.setenv("SDN_PERPIX_EXACT", "sometimes")
    with pytest.raises(ValueError):
        dropin.GeneratorBinding()
    monkeypatch.delenv("SDN_PERPIX_EXACT")
    for bad in ("exact", 2, "refuse"):
        with pytest.raises(ValueError):
            dropin.parse_exact(bad)

    class Holder:
        pass
    G = Holder()
    b = dropin.binding(G)
    assert b.exact is False and dropin.binding(G, exact="refused") is b and b.exact == "refused"
    assert dropin.binding(G).exact == "refused"                              # None leaves it as it is
    assert dropin.binding(G, exact=True).exact is True and dropin.binding(G, exact=False).exact is False
