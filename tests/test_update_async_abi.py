"""The enqueued vertex update's C-ABI surface (rtr_scene_prepare_async_updates, rtr_scene_update_vertices_async,
rtr_scene_update_status, rtr_update_status) — what needs no device: the header declares the entry points and the struct, the product
and the test library export them, _abi.py binds them with the header's argument lists, the struct is 32 bytes on both sides, the ABI
version is still 3, and the refusals that come before any device work."""
import ctypes as C
import os
import re
import subprocess

from realtimeraytracer_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1

VP, u32 = A.VP, A.u32
EXPECTED = {
    "rtr_scene_prepare_async_updates": ("rtr_scene* scene", [VP]),
    "rtr_scene_update_vertices_async": ("rtr_scene* scene, const rtr_vertex_range* ranges, uint32_t numRanges, uint32_t positionStride, uint32_t normalStride",
                                        [VP, C.POINTER(A.rtr_vertex_range), u32, u32, u32]),
    "rtr_scene_update_status": ("rtr_scene* scene, rtr_update_status* out", [VP, C.POINTER(A.rtr_update_status)]),
}


def _raw_header():
    return open(os.path.join(ROOT, "include", "rtr.h")).read()


def _header():
    return re.sub(r"/\*.*?\*/", "", _raw_header(), flags=re.S)


def _norm(params):
    return [re.sub(r"\s+", " ", p).strip() for p in params.split(",")]


def test_the_entry_points_are_declared_exported_and_bound():
    text = _header()
    for path in (A.LIB_HIP_PATH, A.LIB_HIP_HOOKS_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        for n in EXPECTED:
            assert n in exported, f"{os.path.basename(path)} does not export {n}"
    for n, (params, argtypes) in EXPECTED.items():
        m = re.search(r"\bint\s+" + n + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{n} is not declared in include/rtr.h"
        assert _norm(m.group(1)) == _norm(params), f"{n}: the header's parameters are {_norm(m.group(1))}"
        assert n in A.RTR_SYMBOLS, f"{n} is not bound in _abi.RTR_SYMBOLS"
        res, args = A.RTR_SYMBOLS[n]
        assert res is C.c_int and list(args) == argtypes, f"{n}: bound as {args}"
    # new symbols only: no layout and no kernel changed
    assert A.hip_lib().rtr_abi_version() == 3
    assert re.search(r"#define\s+RTR_ABI_VERSION\s+3\b", _raw_header())


def test_the_struct():
    text = _header()
    m = re.search(r"typedef\s+struct\s+rtr_update_status\s*\{(.*?)\}\s*rtr_update_status\s*;", text, flags=re.S)
    assert m, "rtr_update_status is not declared in include/rtr.h"
    assert re.sub(r"\s+", " ", m.group(1)).strip() == "uint64_t enqueued, refused; uint32_t firstRefusedUpdate, firstBadVertex; uint32_t _pad[2];"
    assert "static_assert(sizeof(rtr_update_status) == 32" in text
    T = A.rtr_update_status
    assert C.sizeof(T) == 32
    assert [f[0] for f in T._fields_] == ["enqueued", "refused", "firstRefusedUpdate", "firstBadVertex", "_pad"]
    assert (T.enqueued.offset, T.refused.offset, T.firstRefusedUpdate.offset, T.firstBadVertex.offset) == (0, 8, 16, 20)


def test_the_refusals_that_need_no_device():
    lib = A.hip_lib()
    st = A.rtr_update_status()
    one = (A.rtr_vertex_range * 1)(A.rtr_vertex_range(0, 0, None, None))
    assert lib.rtr_scene_prepare_async_updates(None) == INVALID
    assert b"rtr_scene_prepare_async_updates" in lib.rtr_last_error() and b"null scene" in lib.rtr_last_error()
    assert lib.rtr_scene_update_vertices_async(None, one, 1, 12, 12) == INVALID
    assert b"rtr_scene_update_vertices_async" in lib.rtr_last_error() and b"null scene" in lib.rtr_last_error()
    assert lib.rtr_scene_update_status(None, C.byref(st)) == INVALID
    assert b"rtr_scene_update_status" in lib.rtr_last_error() and b"null" in lib.rtr_last_error()
    # a handle that is never looked into: these refusals come before anything of the scene is read
    fake = C.create_string_buffer(16)
    scene = C.cast(fake, VP)
    assert lib.rtr_scene_update_vertices_async(scene, None, 1, 12, 12) == INVALID
    assert b"null ranges" in lib.rtr_last_error()
    assert lib.rtr_scene_update_vertices_async(scene, one, 0, 12, 12) == INVALID
    assert b"null ranges" in lib.rtr_last_error()
    for stride in (0, 8, 14):
        assert lib.rtr_scene_update_vertices_async(scene, one, 1, stride, 12) == INVALID
        assert b"positionStride" in lib.rtr_last_error() and b"rtr_scene_update_vertices_async" in lib.rtr_last_error()
    assert lib.rtr_scene_update_status(scene, None) == INVALID
