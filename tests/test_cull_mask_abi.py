"""The instance cull masks' C-ABI surface (rtr_scene_set/get_instance_masks, rtr_trace_rays_masked[_async],
rtr_trace_occlusion_masked[_async]) — what needs no device: the header declares the six entry points, the product and the test library
export them, _abi.py binds them with the header's argument lists, the ABI version stays 3, the argument errors that come before any
device work, and the records every builder writes still carry nothing but bit 0 in their flags word: the default mask 0xff is stored as
its complement, 0, so a scene whose masks were never set has the bytes it always had."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1

VP, u32 = A.VP, A.u32
# name -> the header's parameter list, as the ctypes _abi.py must bind it with
EXPECTED = {
    "rtr_scene_set_instance_masks": ("rtr_scene* scene, const uint8_t* masks, uint32_t numInstances", [VP, VP, u32]),
    "rtr_scene_get_instance_masks": ("const rtr_scene* scene, uint8_t* masks, uint32_t numInstances", [VP, VP, u32]),
    "rtr_trace_rays_masked_async": ("rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const uint8_t* rayMasks, uint32_t numRays, "
                                    "uint32_t flags, uint32_t cullMask, RtrHit* hits, uint8_t* occluded", [VP, VP, VP, VP, u32, u32, u32, VP, VP]),
    "rtr_trace_rays_masked": ("rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const uint8_t* rayMasks, uint32_t numRays, "
                              "uint32_t flags, uint32_t cullMask, RtrHit* hits, uint8_t* occluded, rtr_query_stats* stats",
                              [VP, VP, VP, VP, u32, u32, u32, VP, VP, C.POINTER(A.rtr_query_stats)]),
    "rtr_trace_occlusion_masked_async": ("rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const int32_t* startLeaves, "
                                         "const uint8_t* rayMasks, uint32_t numRays, uint32_t flags, uint32_t cullMask, void* scratch, "
                                         "size_t scratchBytes, uint8_t* occluded", [VP, VP, VP, VP, VP, u32, u32, u32, VP, C.c_size_t, VP]),
    "rtr_trace_occlusion_masked": ("rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const int32_t* startLeaves, "
                                   "const uint8_t* rayMasks, uint32_t numRays, uint32_t flags, uint32_t cullMask, void* scratch, "
                                   "size_t scratchBytes, uint8_t* occluded, rtr_query_stats* stats",
                                   [VP, VP, VP, VP, VP, u32, u32, u32, VP, C.c_size_t, VP, C.POINTER(A.rtr_query_stats)]),
}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtr.h")).read(), flags=re.S)


def _norm(params):
    return [re.sub(r"\s+", " ", p).strip() for p in params.split(",")]


def test_the_six_entry_points_are_declared_exported_and_bound():
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
        assert len(args) == len(_norm(params))
    assert A.hip_lib().rtr_abi_version() == 3
    assert re.search(r"#define\s+RTR_ABI_VERSION\s+3\b", open(os.path.join(ROOT, "include", "rtr.h")).read())
    for f in ("set_instance_masks", "instance_masks"):
        assert callable(getattr(api.Scene, f))


def test_python_layer_takes_the_mask_arguments():
    import inspect
    for fn in (api.trace_rays, api.trace_occlusion):
        p = inspect.signature(fn).parameters
        assert p["cull_mask"].default is None and p["ray_masks"].default is None
    assert inspect.signature(api.direct_light).parameters["shadow_cull_mask"].default is None


def test_argument_errors_that_need_no_device():
    lib = A.hip_lib()
    fake = A.VP(0x1000)
    assert lib.rtr_scene_set_instance_masks(None, fake, 1) == INVALID
    assert b"rtr_scene_set_instance_masks" in lib.rtr_last_error() and b"null" in lib.rtr_last_error()
    assert lib.rtr_scene_get_instance_masks(None, fake, 1) == INVALID
    assert b"rtr_scene_get_instance_masks" in lib.rtr_last_error()
    assert lib.rtr_trace_rays_masked(None, None, fake, None, 64, 0, 0xff, fake, None, None) == INVALID
    assert b"rtr_trace_rays_masked" in lib.rtr_last_error() and b"null context or scene" in lib.rtr_last_error()
    assert lib.rtr_trace_rays_masked_async(None, None, fake, None, 64, 0, 0xff, fake, None) == INVALID
    assert b"rtr_trace_rays_masked_async" in lib.rtr_last_error()
    assert lib.rtr_trace_occlusion_masked(None, None, fake, None, None, 64, 0, 0xff, fake, 1 << 20, fake, None) == INVALID
    assert b"rtr_trace_occlusion_masked" in lib.rtr_last_error()
    assert lib.rtr_trace_occlusion_masked_async(None, None, fake, None, None, 64, 0, 0xff, fake, 1 << 20, fake) == INVALID
    assert b"rtr_trace_occlusion_masked_async" in lib.rtr_last_error()


def test_the_types_header_names_the_mask_bits():
    text = open(os.path.join(ROOT, "include", "rtr_types.h")).read()
    assert re.search(r"#define\s+RTR_TRI_MASK_SHIFT\s+8u\b", text)
    assert re.search(r"#define\s+RTR_TRI_MASK_BITS\s+\(0xffu\s*<<\s*RTR_TRI_MASK_SHIFT\)", text)


@pytest.mark.parametrize("workload", ["cornell_box", "bunny_class", "sponza_class", "sponza_mixed", "textured_room"])
def test_host_built_records_carry_only_bit_0(scene_cache, workload):
    """default bytes unchanged: every builder writes flags in {0, 1}; the complement of the default mask 0xff is 0"""
    if workload == "bunny_class":
        s = scenes.bunny_class(64, 64, subdiv=3)
    else:
        s = getattr(scenes, workload)(64, 36)
    st, nodes, tris = api.host_build_bvh(s.desc)
    raw = np.frombuffer(tris, dtype=np.uint32).reshape(-1, 12)
    assert len(raw) == max(st.numTriangles, 1)
    assert not (raw[:, 11] & ~np.uint32(1)).any(), f"{workload}: flags beyond bit 0 in a freshly built scene"
    if workload in ("sponza_mixed", "textured_room"):
        assert (raw[:, 11] & 1).any(), "the workload holds alpha-tested triangles"
    wide = api.host_build_bvh_wide(s.desc)
    raw_w = np.frombuffer(wide[1], dtype=np.uint32).reshape(-1, 12)
    assert (raw_w == raw).all()
