"""Hit surfaces' C-ABI surface (include/rtr.h, rtr_types.h): the layout of RtrSurface, the RTR_SURFACE_* kinds, and the two entry points
exported by the product library and its test build.  No GPU needed."""
import ctypes as C
import os
import re

from realtimeraytracer_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rtr_hit_surfaces_async", "rtr_hit_surfaces")


def test_surface_layout():
    S = A.RtrSurface
    assert C.sizeof(S) == 80
    names = ("position", "kind", "normal", "objectIndex", "geomNormal", "metallic", "color", "roughness", "uv", "_reserved")
    assert [(n, getattr(S, n).offset) for n in names] == [("position", 0), ("kind", 12), ("normal", 16), ("objectIndex", 28),
                                                        ("geomNormal", 32), ("metallic", 44), ("color", 48), ("roughness", 60),
                                                        ("uv", 64), ("_reserved", 72)]
    # five 16-B stores: every record boundary the kernel writes is a field boundary
    assert [getattr(S, n).offset for n in ("position", "normal", "geomNormal", "color", "uv")] == [0, 16, 32, 48, 64]


def test_static_assert_in_the_header():
    text = open(os.path.join(ROOT, "include", "rtr_types.h")).read()
    assert "static_assert(sizeof(RtrSurface) == 80" in text
    body = re.search(r"typedef struct RtrSurface \{(.*?)\} RtrSurface;", text, re.S).group(1)
    fields = re.findall(r"(float|uint32_t)\s+(\w+)(?:\[(\d)\])?;", body)
    assert [(n, int(k or 1)) for _, n, k in fields] == [(n, C.sizeof(t) // 4) for n, t in A.RtrSurface._fields_]


def test_kind_values_match_the_header():
    text = open(os.path.join(ROOT, "include", "rtr_types.h")).read()
    vals = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define RTR_SURFACE_(\w+)\s+(\d+)u", text)}
    assert vals == {"MISS": A.SURFACE_MISS, "OBJECT": A.SURFACE_OBJECT, "LIGHT": A.SURFACE_LIGHT, "INVALID": A.SURFACE_INVALID} == \
        {"MISS": 0, "OBJECT": 1, "LIGHT": 2, "INVALID": 3}


def test_abi_version_unchanged():
    assert A.hip_lib().rtr_abi_version() == 3


def test_surface_symbols_are_exported():
    for lib in (C.CDLL(A.LIB_HIP_PATH), C.CDLL(A.LIB_HIP_HOOKS_PATH)):
        for n in NEW:
            assert hasattr(lib, n), n
            assert n in A.RTR_SYMBOLS


def test_arguments_are_checked_before_any_device_is_touched():
    lib = A.hip_lib()
    assert lib.rtr_hit_surfaces_async(None, None, None, None, 1, None) == -1
    assert b"null" in lib.rtr_last_error()
    assert lib.rtr_hit_surfaces(None, None, None, None, 0, None) == -1


def test_the_handles_come_before_the_arrays():
    lib = A.hip_lib()
    for name in NEW:                          # a null and a misaligned array beside the null handles: the handles' message wins
        assert getattr(lib, name)(None, None, None, A.VP(0x1008), 4, A.VP(0x1004)) == -1
        assert lib.rtr_last_error() == name.encode() + b": null context or scene"
