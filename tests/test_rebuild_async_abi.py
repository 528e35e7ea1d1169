"""The enqueued rebuild's C-ABI surface (rtr_scene_prepare_async_rebuild, rtr_scene_rebuild_async) — what needs no device: the header
declares the entry points with the agreed parameter lists, the product and the test library export them, _abi.py binds them with the
header's argument lists, rtr_update_status keeps its text and its 32 bytes, the ABI version is still 3, and the refusals that come
before anything of the scene is read."""
import ctypes as C
import os
import re
import subprocess

from realtimeraytracer_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1

VP, u32 = A.VP, A.u32
EXPECTED = {
    "rtr_scene_prepare_async_rebuild": ("rtr_scene* scene", [VP]),
    "rtr_scene_rebuild_async": ("rtr_scene* scene, uint32_t buildFlags", [VP, u32]),
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
    # new symbols only: no layout changed
    assert A.hip_lib().rtr_abi_version() == 3
    assert re.search(r"#define\s+RTR_ABI_VERSION\s+3\b", _raw_header())


def test_the_status_struct_keeps_its_text_and_layout():
    text = _header()
    m = re.search(r"typedef\s+struct\s+rtr_update_status\s*\{(.*?)\}\s*rtr_update_status\s*;", text, flags=re.S)
    assert m, "rtr_update_status is not declared in include/rtr.h"
    assert re.sub(r"\s+", " ", m.group(1)).strip() == "uint64_t enqueued, refused; uint32_t firstRefusedUpdate, firstBadVertex; uint32_t _pad[2];"
    assert "static_assert(sizeof(rtr_update_status) == 32" in text
    T = A.rtr_update_status
    assert C.sizeof(T) == 32
    assert [f[0] for f in T._fields_] == ["enqueued", "refused", "firstRefusedUpdate", "firstBadVertex", "_pad"]
    assert (T.enqueued.offset, T.refused.offset, T.firstRefusedUpdate.offset, T.firstBadVertex.offset) == (0, 8, 16, 20)
    # the struct's comment says what the word carries for a refused rebuild
    before = _raw_header().split("typedef struct rtr_update_status")[0][-1500:]
    assert re.search(r"refused\s+rebuild\s+firstBadVertex\s+carries\s+the\s+DEPTH", re.sub(r"\s*\n\s*\*\s*", " ", before))


def test_the_refusals_that_need_no_device():
    lib = A.hip_lib()
    for fn, who in ((lib.rtr_scene_prepare_async_rebuild, b"rtr_scene_prepare_async_rebuild"),):
        assert fn(None) == INVALID
        assert who in lib.rtr_last_error() and b"null scene" in lib.rtr_last_error()
    for flags in (0, 1, 2):
        assert lib.rtr_scene_rebuild_async(None, flags) == INVALID
        assert b"rtr_scene_rebuild_async" in lib.rtr_last_error() and b"null scene" in lib.rtr_last_error()
    # a handle that is never looked into: the flags are checked before anything of the scene is read
    fake = C.create_string_buffer(16)
    scene = C.cast(fake, VP)
    for flags in (0, 2, 3, 0xffffffff):
        assert lib.rtr_scene_rebuild_async(scene, flags) == INVALID
        err = lib.rtr_last_error()
        assert b"rtr_scene_rebuild_async" in err and b"buildFlags" in err, err
    assert b"RTR_BUILD_HOST_SAH" in (lib.rtr_scene_rebuild_async(scene, 0), lib.rtr_last_error())[1]
