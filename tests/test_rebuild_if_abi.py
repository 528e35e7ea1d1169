"""The rebuild policy's C-ABI surface (rtr_scene_prepare_async_rebuild_if, rtr_scene_rebuild_if_async, rtr_scene_rebuild_if_status) —
what needs no device: the header declares the entry points with the agreed parameter lists, the product and the test library export
them, _abi.py binds them with the header's argument lists (a c_double for rebuildAbove), rtr_rebuild_if_status is 48 bytes with the
agreed offsets, rtr_update_status keeps its text, the ABI version is still 3, and the refusals that come before anything of the scene
is read."""
import ctypes as C
import os
import re
import subprocess

from realtimeraytracer_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1

VP, u32 = A.VP, A.u32
EXPECTED = {
    "rtr_scene_prepare_async_rebuild_if": ("rtr_scene* scene", lambda: [VP]),
    "rtr_scene_rebuild_if_async": ("rtr_scene* scene, uint32_t buildFlags, double rebuildAbove", lambda: [VP, u32, C.c_double]),
    "rtr_scene_rebuild_if_status": ("rtr_scene* scene, rtr_rebuild_if_status* out", lambda: [VP, C.POINTER(A.rtr_rebuild_if_status)]),
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
        assert res is C.c_int and list(args) == argtypes(), f"{n}: bound as {args}"
    # the documentation follows the declaration of rtr_scene_rebuild_async
    raw = _raw_header()
    assert raw.index("rtr_scene_rebuild_async(rtr_scene* scene, uint32_t buildFlags);") < raw.index("typedef struct rtr_rebuild_if_status")
    # new symbols only: no layout changed
    assert A.hip_lib().rtr_abi_version() == 3
    assert re.search(r"#define\s+RTR_ABI_VERSION\s+3\b", raw)


def test_the_policy_struct_layout():
    text = _header()
    m = re.search(r"typedef\s+struct\s+rtr_rebuild_if_status\s*\{(.*?)\}\s*rtr_rebuild_if_status\s*;", text, flags=re.S)
    assert m, "rtr_rebuild_if_status is not declared in include/rtr.h"
    assert re.sub(r"\s+", " ", m.group(1)).strip() == ("uint64_t evaluated; uint64_t rebuilt; double builtSah; double lastSah; "
                                                        "uint32_t lastDecision; uint32_t _pad[3];")
    assert "static_assert(sizeof(rtr_rebuild_if_status) == 48" in text
    T = A.rtr_rebuild_if_status
    assert C.sizeof(T) == 48
    assert [f[0] for f in T._fields_] == ["evaluated", "rebuilt", "builtSah", "lastSah", "lastDecision", "_pad"]
    assert (T.evaluated.offset, T.rebuilt.offset, T.builtSah.offset, T.lastSah.offset, T.lastDecision.offset) == (0, 8, 16, 24, 32)
    assert T._fields_[2][1] is C.c_double and T._fields_[3][1] is C.c_double


def test_the_update_status_struct_keeps_its_text_and_layout():
    text = _header()
    m = re.search(r"typedef\s+struct\s+rtr_update_status\s*\{(.*?)\}\s*rtr_update_status\s*;", text, flags=re.S)
    assert m, "rtr_update_status is not declared in include/rtr.h"
    assert re.sub(r"\s+", " ", m.group(1)).strip() == "uint64_t enqueued, refused; uint32_t firstRefusedUpdate, firstBadVertex; uint32_t _pad[2];"
    assert "static_assert(sizeof(rtr_update_status) == 32" in text
    assert C.sizeof(A.rtr_update_status) == 32
    # nothing was put in front of it: its comment still says what the word carries for a refused rebuild
    before = _raw_header().split("typedef struct rtr_update_status")[0][-1500:]
    assert re.search(r"refused\s+rebuild\s+firstBadVertex\s+carries\s+the\s+DEPTH", re.sub(r"\s*\n\s*\*\s*", " ", before))
    assert "rebuild_if" not in before


def test_one_function_for_the_cost():
    """the arithmetic lives in kernels/rtr_tree_sah.h, and both sides include it"""
    k = os.path.join(ROOT, "realtimeraytracer_amd", "csrc")
    head = open(os.path.join(k, "kernels", "rtr_tree_sah.h")).read()
    assert re.search(r"RTR_HD\s+double\s+rtr_tree_sah\s*\(", head)
    for f in ("rtr_api.cpp", os.path.join("kernels", "rtr_bvh.hip")):
        src = open(os.path.join(k, f)).read()
        assert '#include "' + ("kernels/" if f == "rtr_api.cpp" else "") + 'rtr_tree_sah.h"' in src and "rtr_tree_sah(" in src, f


def test_the_refusals_that_need_no_device():
    lib = A.hip_lib()
    nan, inf = float("nan"), float("inf")
    st = A.rtr_rebuild_if_status()
    for call, who in ((lambda: lib.rtr_scene_prepare_async_rebuild_if(None), b"rtr_scene_prepare_async_rebuild_if"),
                      (lambda: lib.rtr_scene_rebuild_if_async(None, 1, 1.0), b"rtr_scene_rebuild_if_async"),
                      (lambda: lib.rtr_scene_rebuild_if_async(None, 0, nan), b"rtr_scene_rebuild_if_async"),
                      (lambda: lib.rtr_scene_rebuild_if_status(None, C.byref(st)), b"rtr_scene_rebuild_if_status")):
        assert call() == INVALID
        assert who in lib.rtr_last_error() and b"null scene" in lib.rtr_last_error(), lib.rtr_last_error()
    # a handle that is never looked into
    fake = C.create_string_buffer(16)
    scene = C.cast(fake, VP)
    assert lib.rtr_scene_rebuild_if_status(scene, None) == INVALID
    assert b"rtr_scene_rebuild_if_status" in lib.rtr_last_error() and b"null out" in lib.rtr_last_error()
    # the flags are checked before anything of the scene is read, and before rebuildAbove
    for flags in (0, 2, 3, 0xffffffff):
        for above in (1.0, nan):
            assert lib.rtr_scene_rebuild_if_async(scene, flags, above) == INVALID
            err = lib.rtr_last_error()
            assert b"rtr_scene_rebuild_if_async" in err and b"buildFlags" in err and b"rebuildAbove" not in err, err
    assert b"RTR_BUILD_HOST_SAH" in (lib.rtr_scene_rebuild_if_async(scene, 0, 1.0), lib.rtr_last_error())[1]
    # so is rebuildAbove
    for above in (nan, -1.0, -inf):
        assert lib.rtr_scene_rebuild_if_async(scene, 1, above) == INVALID
        err = lib.rtr_last_error()
        assert b"rtr_scene_rebuild_if_async" in err and b"rebuildAbove" in err, err
