"""The enqueued instance update's C-ABI surface (rtr_scene_update_instances_async, rtr_scene_export_instances) — what needs no device:
the header declares the entry points with the agreed parameter lists, the product and the test library export them, _abi.py binds them
with the header's argument lists, rtr_update_status keeps its 32 bytes and fields, the ABI version is still 3, and the refusals that
come before anything of the scene is read."""
import ctypes as C
import os
import re
import subprocess

from realtimeraytracer_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1

VP, u32 = A.VP, A.u32
EXPECTED = {
    "rtr_scene_update_instances_async": ("rtr_scene* scene, const void* transforms, uint32_t transformStride, uint32_t firstInstance, uint32_t numInstances, "
                                         "const RtrAreaLightInfo* lights, uint32_t numLights",
                                         [VP, VP, u32, u32, u32, C.POINTER(A.RtrAreaLightInfo), u32]),
    "rtr_scene_export_instances": ("const rtr_scene* scene, RtrInstance* out, size_t bytes", [VP, C.POINTER(A.RtrInstance), C.c_size_t]),
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


def test_the_status_struct_keeps_its_layout():
    text = _header()
    m = re.search(r"typedef\s+struct\s+rtr_update_status\s*\{(.*?)\}\s*rtr_update_status\s*;", text, flags=re.S)
    assert m, "rtr_update_status is not declared in include/rtr.h"
    assert re.sub(r"\s+", " ", m.group(1)).strip() == "uint64_t enqueued, refused; uint32_t firstRefusedUpdate, firstBadVertex; uint32_t _pad[2];"
    T = A.rtr_update_status
    assert C.sizeof(T) == 32
    assert [f[0] for f in T._fields_] == ["enqueued", "refused", "firstRefusedUpdate", "firstBadVertex", "_pad"]
    assert (T.enqueued.offset, T.refused.offset, T.firstRefusedUpdate.offset, T.firstBadVertex.offset) == (0, 8, 16, 20)
    assert C.sizeof(A.RtrInstance) == 64 and A.RtrInstance.transform.offset == 16 and C.sizeof(A.RtrAreaLightInfo) == 96


def test_the_refusals_that_need_no_device():
    lib = A.hip_lib()
    who = b"rtr_scene_update_instances_async"
    data = C.create_string_buffer(256)          # never read: every call below is refused on its arguments alone
    base = (C.addressof(data) + 15) & ~15
    tr = VP(base)
    lights = C.cast(VP(base + 64), C.POINTER(A.RtrAreaLightInfo))

    def refused(*args):
        assert lib.rtr_scene_update_instances_async(*args) == INVALID
        err = lib.rtr_last_error()
        assert who in err, err
        return err

    assert b"null scene" in refused(None, tr, 48, 0, 1, None, 0)
    # a handle that is never looked into: these refusals come before anything of the scene is read
    fake = C.create_string_buffer(16)
    scene = C.cast(fake, VP)
    assert b"null transforms and null lights" in refused(scene, None, 48, 0, 0, None, 0)
    for stride in (0, 44, 50):
        assert b"transformStride" in refused(scene, tr, stride, 0, 1, None, 0)
    assert b"aligned" in refused(scene, VP(base | 2), 48, 0, 1, None, 0)
    assert b"aligned" in refused(scene, tr, 48, 0, 1, C.cast(VP((base + 64) | 2), C.POINTER(A.RtrAreaLightInfo)), 1)
    assert b"null transforms with numInstances 1" in refused(scene, None, 48, 0, 1, lights, 1)
    assert b"numInstances 0" in refused(scene, tr, 48, 0, 0, lights, 1)

    out = (A.RtrInstance * 1)()
    assert lib.rtr_scene_export_instances(None, out, C.sizeof(out)) == INVALID
    assert b"rtr_scene_export_instances" in lib.rtr_last_error() and b"null" in lib.rtr_last_error()
