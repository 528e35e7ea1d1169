"""The binned queue build for one sample per pixel, k_shadow_gen_oct<true> (kernels/rtr_kernels.hip), is built for eight waves per
SIMD: at most 64 VGPRs and NO private segment — a spilled dword is a vector-memory round trip on the chain the kernel already waits
on, which is why it stayed at seven waves until spp == 1 became a compile-time property.  The figures are the loaded code object's own
(hipFuncGetAttributes, through librtr_hip_test.so's rtr_test_gen_oct_attributes): registers, scratch and LDS, nothing else."""
import ctypes as C

import pytest

from realtimeraytracer_amd import _abi as A

pytestmark = pytest.mark.gpu


def _attributes(single):
    lib = A.hip_lib_with_hooks()
    fn = lib.rtr_test_gen_oct_attributes
    fn.argtypes, fn.restype = [C.c_int, C.POINTER(C.c_uint32)], C.c_int
    out = (C.c_uint32 * 4)()
    assert fn(single, out) == 0, lib.rtr_last_error()
    return {"vgprs": out[0], "scratch": out[1], "lds": out[2], "block": out[3]}


def test_the_one_sample_queue_build_has_no_scratch_at_eight_waves(gpu_ctx):
    a = _attributes(1)
    print("k_shadow_gen_oct<true>:", a)
    assert a["scratch"] == 0, f"k_shadow_gen_oct<true> has a private segment of {a['scratch']} bytes per lane"
    assert a["vgprs"] <= 64, f"k_shadow_gen_oct<true> takes {a['vgprs']} VGPRs: more than eight waves per SIMD have"
    assert a["block"] >= 512
    assert 4 * a["lds"] <= 160 * 1024, "four workgroups per CU (eight waves per SIMD) must fit the CU's LDS"


def test_the_product_library_exports_no_such_hook(gpu_ctx):
    assert not hasattr(A.hip_lib(), "rtr_test_gen_oct_attributes")
    b = _attributes(0)                     # spp > 1: today's cap of seven waves; it spills nothing either
    print("k_shadow_gen_oct<false>:", b)
    assert b["scratch"] == 0 and b["vgprs"] <= 72
