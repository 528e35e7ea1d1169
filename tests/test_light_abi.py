"""Direct lighting's C-ABI surface (include/rtr.h, rtr_types.h): the layouts of rtr_light_params and RtrRadiance, the RTR_LIGHT_* bits,
and the seven entry points exported by the product library and its test build.  No GPU needed."""
import ctypes as C
import os
import re

from realtimeraytracer_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rtr_light_slots", "rtr_light_rays_async", "rtr_light_rays", "rtr_shade_hits_async", "rtr_shade_hits", "rtr_tonemap_pack_async",
       "rtr_tonemap_pack")
INVALID = -1


def _fields(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for typ, names in re.findall(r"(float|uint32_t)\s+([^;]+);", body):
        for n in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", n)
            out.append((m.group(1), int(m.group(2) or 1)))
    return out


def test_light_params_layout():
    S = A.rtr_light_params
    assert C.sizeof(S) == 32
    names = ("numAreaLights", "numShadowRays", "frame", "width", "spp", "outputs", "_pad")
    assert [(n, getattr(S, n).offset) for n in names] == [("numAreaLights", 0), ("numShadowRays", 4), ("frame", 8), ("width", 12),
                                                        ("spp", 16), ("outputs", 20), ("_pad", 24)]
    text = open(os.path.join(ROOT, "include", "rtr.h")).read()
    assert _fields(text, "rtr_light_params") == [(n, C.sizeof(t) // 4) for n, t in S._fields_]


def test_radiance_layout():
    S = A.RtrRadiance
    assert C.sizeof(S) == 48
    names = ("shadowed", "kind", "unshadowed", "_r0", "analytic", "_r1")
    assert [(n, getattr(S, n).offset) for n in names] == [("shadowed", 0), ("kind", 12), ("unshadowed", 16), ("_r0", 28), ("analytic", 32),
                                                        ("_r1", 44)]
    # three 16-B stores: every record boundary the kernel writes is a field boundary
    assert [getattr(S, n).offset for n in ("shadowed", "unshadowed", "analytic")] == [0, 16, 32]
    text = open(os.path.join(ROOT, "include", "rtr_types.h")).read()
    assert "static_assert(sizeof(RtrRadiance) == 48" in text
    assert _fields(text, "RtrRadiance") == [(n, C.sizeof(t) // 4) for n, t in S._fields_]


def test_output_bits_match_the_header_and_no_surface_kind_was_added():
    text = open(os.path.join(ROOT, "include", "rtr.h")).read()
    vals = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define RTR_LIGHT_(\w+)\s+(\d+)u", text)}
    assert vals == {"SHADOWED": A.LIGHT_SHADOWED, "UNSHADOWED": A.LIGHT_UNSHADOWED, "ANALYTIC": A.LIGHT_ANALYTIC} == \
        {"SHADOWED": 1, "UNSHADOWED": 2, "ANALYTIC": 4}
    types = open(os.path.join(ROOT, "include", "rtr_types.h")).read()
    assert sorted(re.findall(r"#define RTR_SURFACE_(\w+)", types + text)) == ["INVALID", "LIGHT", "MISS", "OBJECT"]


def test_abi_version_unchanged():
    assert A.hip_lib().rtr_abi_version() == 3


def test_light_symbols_are_exported():
    text = open(os.path.join(ROOT, "include", "rtr.h")).read()
    for lib in (C.CDLL(A.LIB_HIP_PATH), C.CDLL(A.LIB_HIP_HOOKS_PATH)):
        for n in NEW:
            assert hasattr(lib, n), n
            assert n in A.RTR_SYMBOLS
            assert re.search(r"\b%s\(" % n, text), n


def test_arguments_are_checked_before_any_device_is_touched():
    lib = A.hip_lib()
    p = A.rtr_light_params(0, 3, 0, 16, 1, A.LIGHT_SHADOWED)
    q = C.c_uint32(0)
    for call in (lambda: lib.rtr_light_slots(None, C.byref(p), C.byref(q)),
                 lambda: lib.rtr_light_rays_async(None, None, None, None, 1, C.byref(p), None, None),
                 lambda: lib.rtr_light_rays(None, None, None, None, 0, None, None, None),
                 lambda: lib.rtr_shade_hits_async(None, None, None, None, 1, C.byref(p), None, None, None),
                 lambda: lib.rtr_shade_hits(None, None, None, None, 0, None, None, None, None),
                 lambda: lib.rtr_tonemap_pack_async(None, None, 48, 1, None),
                 lambda: lib.rtr_tonemap_pack(None, None, 48, 0, None)):
        assert call() == INVALID
        assert b"null" in lib.rtr_last_error()


def test_which_refusal_wins_under_two_faults():
    """the lighting calls look at their handles and params before any array or value; rtr_tonemap_pack at its context, then the stride,
    then the arrays; rtr_light_slots at its output before the scene"""
    lib = A.hip_lib()
    err = lib.rtr_last_error
    bad = A.rtr_light_params(0, 0, 0, 0, 0, 8)          # numShadowRays 0, width and spp 0, unknown output bits
    odd = A.VP(0x1002)
    q = C.c_uint32(0)
    assert lib.rtr_light_slots(None, None, None) == INVALID and err() == b"rtr_light_slots: slotsPerHit is null"
    assert lib.rtr_light_slots(None, C.byref(bad), C.byref(q)) == INVALID and err() == b"rtr_light_slots: null scene or params"
    for name in ("rtr_light_rays_async", "rtr_light_rays"):
        assert getattr(lib, name)(None, None, odd, None, 4, C.byref(bad), odd, None) == INVALID
        assert err() == name.encode() + b": null context, scene or params"
    for name in ("rtr_shade_hits_async", "rtr_shade_hits"):
        assert getattr(lib, name)(None, None, odd, None, 4, C.byref(bad), odd, None, odd) == INVALID
        assert err() == name.encode() + b": null context, scene or params"
    for name in ("rtr_tonemap_pack_async", "rtr_tonemap_pack"):
        assert getattr(lib, name)(None, odd, 7, 4, None) == INVALID and err() == b"rtr_tonemap_pack: null context"
