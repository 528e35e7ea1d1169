"""The culling ray flags of the ray queries (RTR_QUERY_CULL_BACK_FACING / FRONT_FACING / OPAQUE / NO_OPAQUE) — what needs no device:
the header's four constants with Vulkan's bit values, _abi.py's copies, the ABI version, the Python keywords and the combinations the
Python layer refuses, the records of fresh scenes (a mirrored instance included: the mirrored bit is NOT in them), and the soundness
of the witness the GPU tests rely on: the float32 restatement of rtr_mt_intersect (tests/ray_flags_witness.py), whose determinant
decides facing, gives the bits of oracle_mt, and its opacity-map verdict agrees with the float64 witness."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api, scenes

import ray_flags_witness as W
from witness import Witness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F3 = A.f32 * 3
VALUES = {"CULL_BACK_FACING": 0x10, "CULL_FRONT_FACING": 0x20, "CULL_OPAQUE": 0x40, "CULL_NO_OPAQUE": 0x80}


def test_the_header_defines_the_four_flags_with_vulkans_values():
    text = open(os.path.join(ROOT, "include", "rtr.h")).read()
    for name, value in VALUES.items():
        m = re.search(r"#define\s+RTR_QUERY_" + name + r"\s+(0x[0-9a-fA-F]+)u\b", text)
        assert m and int(m.group(1), 16) == value, f"RTR_QUERY_{name}"
        assert getattr(A, "QUERY_" + name) == value
    assert (A.QUERY_CLOSEST, A.QUERY_ANY, A.QUERY_OPAQUE) == (0, 1, 2)
    assert re.search(r"#define\s+RTR_ABI_VERSION\s+3\b", text)
    assert A.hip_lib().rtr_abi_version() == 3


def test_python_layer_takes_the_flags_and_refuses_what_vulkan_forbids():
    for fn in (api.trace_rays, api.trace_occlusion):
        assert inspect.signature(fn).parameters["ray_flags"].default == 0
    assert inspect.signature(api.direct_light).parameters["shadow_ray_flags"].default == 0
    both = A.QUERY_CULL_BACK_FACING | A.QUERY_CULL_FRONT_FACING
    bad = [dict(ray_flags=both), dict(ray_flags=A.QUERY_CULL_OPAQUE | A.QUERY_CULL_NO_OPAQUE),
           dict(ray_flags=A.QUERY_CULL_OPAQUE, opaque=True), dict(ray_flags=A.QUERY_CULL_NO_OPAQUE, opaque=True),
           dict(ray_flags=A.QUERY_CULL_NO_OPAQUE | A.QUERY_OPAQUE), dict(ray_flags=both | A.QUERY_CULL_OPAQUE), dict(ray_flags=-1)]
    for kw in bad:                          # refused before the scene or the rays are looked at
        with pytest.raises(ValueError):
            api.trace_rays(None, None, **kw)
        with pytest.raises(ValueError):
            api.trace_occlusion(None, None, **kw)
    for f in (both, A.QUERY_CULL_OPAQUE | A.QUERY_CULL_NO_OPAQUE):
        with pytest.raises(ValueError):
            api.direct_light(None, None, shadow_ray_flags=f)


def test_flag_errors_that_need_no_device():
    """the null checks come first; with them out of the way the flags are checked before any device work — covered on the device"""
    lib = A.hip_lib()
    fake = A.VP(0x1000)
    assert lib.rtr_trace_rays(None, None, fake, 64, A.QUERY_CULL_BACK_FACING, fake, None, None) == -1
    assert b"null context or scene" in lib.rtr_last_error()


def _mirrored_copy(s, pick):
    """the instances of s.desc with instance `pick`'s x axis negated (first column of its 3x3), as a ctypes array"""
    n = s.desc.numInstances
    arr = (A.RtrInstance * n)(*[A.RtrInstance.from_buffer_copy(s.desc.instances[i]) for i in range(n)])
    for r in range(3):
        arr[pick].transform[4 * r] = -arr[pick].transform[4 * r]
    return arr


@pytest.mark.parametrize("workload", ["cornell_box", "sponza_mixed", "textured_room"])
def test_records_of_fresh_scenes_carry_only_bit_0_mirrored_or_not(scene_cache, workload):
    s = getattr(scenes, workload)(64, 36)
    before = W.mirrored_by_custom(s.desc)              # some workloads hold mirrored instances already
    pick = next(i for i in range(s.desc.numInstances)
                if s.desc.instances[i].customIndex >= s.num_lights and not before[s.desc.instances[i].customIndex])
    arr = _mirrored_copy(s, pick)
    old = C.cast(s.desc.instances, C.POINTER(A.RtrInstance))         # the pointer's value: a field read aliases the field
    plain = np.frombuffer(api.host_build_bvh(s.desc)[2], dtype=np.uint32).reshape(-1, 12).copy()
    s.desc.instances = arr
    try:
        assert W.mirrored_by_custom(s.desc).sum() == before.sum() + 1
        raw = np.frombuffer(api.host_build_bvh(s.desc)[2], dtype=np.uint32).reshape(-1, 12).copy()
    finally:
        s.desc.instances = old
    assert (W.mirrored_by_custom(s.desc) == before).all()
    assert not (raw[:, 11] & ~np.uint32(1)).any(), "a mirrored instance must not show in the flags word"
    assert not (plain[:, 11] & ~np.uint32(1)).any()
    assert np.array_equal(np.sort(raw[:, 11]), np.sort(plain[:, 11]))


def test_fma32_is_a_correctly_rounded_fma():
    """against exact rational arithmetic, on operands that provoke double rounding (a product that sits next to a tie)"""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (-(a.astype(np.float64) * b).astype(np.float32) * np.float32(1.0 + 2.0 ** -12)).astype(np.float32)     # heavy cancellation
    c[::3] = rng.standard_normal(len(c[::3])).astype(np.float32) * np.float32(1e-3)
    # ties: a * b = 1 + 2^-24 + 2^-46 exactly; adding c = 2^-60 must round up from the tie
    a[:2] = np.float32(1.0 + 2.0 ** -23); b[:2] = np.float32(1.0 - 2.0 ** -24); c[0] = np.float32(2.0 ** -60); c[1] = np.float32(-2.0 ** -60)
    got = W.fma32(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo, hi = np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))
        e = abs(exact - Fraction(float(g)))
        assert e <= abs(exact - Fraction(float(lo))) and e <= abs(exact - Fraction(float(hi))), (x, y, z, g)
        if e == abs(exact - Fraction(float(lo))) or e == abs(exact - Fraction(float(hi))):          # a tie: to even
            assert (np.float32(g).view(np.uint32) & 1) == 0, (x, y, z, g)


@pytest.mark.parametrize("workload", ["cornell_box", "textured_room"])
def test_the_float32_restatement_gives_oracle_mts_bits(oracle, scene_cache, workload):
    """t, u and v rebuilt by the chain that gives the determinant a, against oracle_mt, for every (ray, record) pair oracle_mt
    accepts — and the restatement accepts exactly those"""
    s = getattr(scenes, workload)(64, 36)
    st, nodes, tris = api.host_build_bvh(s.desc)
    raw = np.frombuffer(tris, dtype=np.uint32).reshape(-1, 12)
    flt = raw.view(np.float32)
    lo, hi = np.array(st.boundsMin[:], np.float32), np.array(st.boundsMax[:], np.float32)
    rng = np.random.default_rng(17)
    L = oracle.lib()
    tuv = (A.f32 * 3)()
    accepted = 0
    signs = set()
    for k in range(40):
        o = (lo + (hi - lo) * rng.uniform(0.05, 0.95, 3)).astype(np.float32)
        j = rng.integers(0, len(flt))                      # aimed at a record, so that some are hit
        b = rng.uniform(0.0, 0.5, 2)
        d = (flt[j, 0:3] + flt[j, 4:7] * np.float32(b[0]) + flt[j, 8:11] * np.float32(b[1]) - o).astype(np.float32)
        tmin = np.float32(0.001)
        ok, t, u, v, a = W.mt32(o, d, flt[:, 0:3], flt[:, 4:7], flt[:, 8:11], tmin)
        o32, d32 = F3(*o), F3(*d)
        for i in range(len(flt)):
            ref = L.oracle_mt(o32, d32, F3(*flt[i, 0:3]), F3(*flt[i, 4:7]), F3(*flt[i, 8:11]), float(tmin), tuv)
            assert bool(ref) == bool(ok[i]), (k, i)
            if ref:
                accepted += 1
                got = np.array([t[i], u[i], v[i]], np.float32).view(np.uint32)
                exp = np.array([tuv[0], tuv[1], tuv[2]], np.float32).view(np.uint32)
                assert (got == exp).all(), (k, i, got, exp)
                assert abs(a[i]) >= W.EPS
                signs.add(bool(a[i] > 0))
    assert accepted >= 40 and signs == {True, False}


def test_the_float32_opacity_verdict_agrees_with_the_float64_witness(scene_cache):
    s = scenes.textured_room(64, 36)
    w64 = Witness(s.desc)
    w32 = W.AlphaWitness(s.desc)
    tested = np.nonzero(w64.alpha)[0]
    assert len(tested)
    rng = np.random.default_rng(5)
    verdicts = set()
    close = 0
    for ti in tested[rng.integers(0, len(tested), 300)]:
        bu, bv = rng.uniform(0, 1, 2)
        if bu + bv > 1:
            bu, bv = 1 - bu, 1 - bv
        c, p = int(w64.cust[ti]), int(w64.prim[ti])
        t32 = w32.texel(c, p, bu, bv)
        oi = w64.objects[c - w64.numLights]
        tri = w64.idx[oi.indexOffset + 3 * p: oi.indexOffset + 3 * p + 3].astype(np.int64) + oi.vertexOffset
        uv = w64.verts[tri, 8:10]
        b32u, b32v = np.float64(np.float32(bu)), np.float64(np.float32(bv))
        uu = uv[0, 0] * (1 - b32u - b32v) + uv[1, 0] * b32u + uv[2, 0] * b32v
        vv = uv[0, 1] * (1 - b32u - b32v) + uv[1, 1] * b32u + uv[2, 1] * b32v
        t64 = Witness.sample(w64.textures[oi.opacityIndex], np.array([uu]), np.array([vv]))[0, 0]
        assert abs(float(t32) - t64) < 2e-3, (c, p, bu, bv, t32, t64)          # a texel-coordinate rounding moves the filter weights
        if abs(t64 - 0.9) > 4e-3:
            assert w32.passes(c, p, bu, bv) == (not t64 < 0.9)
            verdicts.add(not t64 < 0.9)
        else:
            close += 1
    assert verdicts == {True, False} and close < 100
