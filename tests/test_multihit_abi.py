"""The multi-hit ray query (rtr_trace_rays_multi) — what needs no device: the header's constant and prototypes, the exported symbols and
_abi.py's bindings, the ABI version, the null checks, the Python signature and the arguments the Python layer refuses; and the soundness
of the witness the GPU tests rely on (tests/multihit_witness.py): first_k on hand-written candidate lists, the layered scene's hit
counts, which are known by construction, and the vectorised float32 restatement against oracle_mt's list."""
import inspect
import os
import re

import numpy as np
import pytest

from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api

import multihit_witness as M
import ray_flags_witness as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
MISS = M.MISS


def test_the_header_defines_the_constant_and_both_prototypes():
    text = open(os.path.join(ROOT, "include", "rtr.h")).read()
    m = re.search(r"#define\s+RTR_MULTIHIT_MAX\s+8u\b", text)
    assert m and A.MULTIHIT_MAX == 8
    flat = re.sub(r"\s+", " ", text)
    args = (r"\(rtr_ctx\* ctx, const rtr_scene\* scene, const RtrRay\* rays, const uint8_t\* rayMasks, uint32_t numRays, uint32_t maxHits, "
            r"uint32_t flags, uint32_t cullMask, const RtrHit\* after, RtrHit\* hits, uint32_t\* counts")
    assert re.search(r"int rtr_trace_rays_multi_async" + args + r"\);", flat)
    assert re.search(r"int rtr_trace_rays_multi" + args + r", rtr_query_stats\* stats\);", flat)
    assert re.search(r"#define\s+RTR_ABI_VERSION\s+3\b", text)


def test_the_library_exports_both_symbols_and_abi_binds_them():
    lib = A.hip_lib()
    assert lib.rtr_abi_version() == 3
    for name, nargs in (("rtr_trace_rays_multi_async", 11), ("rtr_trace_rays_multi", 12)):
        assert name in A.RTR_SYMBOLS and len(A.RTR_SYMBOLS[name][1]) == nargs
        fn = getattr(lib, name)
        assert fn.restype is A.RTR_SYMBOLS[name][0] and list(fn.argtypes) == A.RTR_SYMBOLS[name][1]


def test_null_context_or_scene_is_refused_with_the_existing_message():
    lib = A.hip_lib()
    fake = A.VP(0x1000)
    assert lib.rtr_trace_rays_multi(None, None, fake, None, 64, 4, 0, 0xff, None, fake, None, None) == -1
    assert b"rtr_trace_rays_multi: null context or scene" in lib.rtr_last_error()
    assert lib.rtr_trace_rays_multi_async(None, fake, fake, None, 64, 4, 0, 0xff, None, fake, None) == -1
    assert b"rtr_trace_rays_multi_async: null context or scene" in lib.rtr_last_error()


def test_the_handles_come_before_every_other_fault():
    lib = A.hip_lib()
    odd = A.VP(0x1002)                        # maxHits 0, RTR_QUERY_ANY, a cull mask above 8 bits, null and misaligned arrays beside the null handles
    assert lib.rtr_trace_rays_multi(None, None, None, None, 64, 0, 1, 0x100, odd, odd, odd, None) == -1
    assert lib.rtr_last_error() == b"rtr_trace_rays_multi: null context or scene"
    assert lib.rtr_trace_rays_multi_async(None, None, None, None, 64, 0, 1, 0x100, odd, odd, odd) == -1
    assert lib.rtr_last_error() == b"rtr_trace_rays_multi_async: null context or scene"


def test_python_signature_defaults_and_value_errors():
    sig = inspect.signature(api.trace_rays_multi)
    assert list(sig.parameters) == ["scene", "rays", "max_hits", "after", "opaque", "ray_flags", "cull_mask", "ray_masks", "collect_stats", "ctx",
                                    "asynchronous"]
    defaults = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == {"after": None, "opaque": False, "ray_flags": 0, "cull_mask": None, "ray_masks": None, "collect_stats": False, "ctx": None,
                        "asynchronous": False}
    for field in ("hits", "counts", "t", "u", "v", "custom_index", "primitive_id", "last", "stats"):
        assert hasattr(api.MultiHitResult, field), field
    both = A.QUERY_CULL_BACK_FACING | A.QUERY_CULL_FRONT_FACING
    bad = [dict(max_hits=0), dict(max_hits=9), dict(max_hits=-1), dict(max_hits=4, ray_flags=A.QUERY_ANY), dict(max_hits=4, ray_flags=both),
           dict(max_hits=4, ray_flags=A.QUERY_CULL_OPAQUE | A.QUERY_CULL_NO_OPAQUE), dict(max_hits=4, ray_flags=A.QUERY_CULL_OPAQUE, opaque=True),
           dict(max_hits=1, ray_flags=A.QUERY_CULL_NO_OPAQUE | A.QUERY_OPAQUE)]
    for kw in bad:                          # refused before the scene or the rays are looked at
        with pytest.raises(ValueError):
            api.trace_rays_multi(None, None, **kw)
    # last: the last slot of every ray, contiguous, numpy or not
    r = api.MultiHitResult()
    r.hits = np.arange(3 * 4 * 8, dtype=np.int32).reshape(3, 4, 8)
    assert r.last.shape == (3, 8) and r.last.flags["C_CONTIGUOUS"] and (r.last == r.hits[:, 3, :]).all()


# ---- first_k on hand-written candidate lists -----------------------------------------------------------------------------------------
def _one_ray(cands, front=None, bit0=None, ok=None, tmax=50.0):
    ts, cs, ps = zip(*cands) if cands else ((), (), ())
    n = len(ts)
    us = [F32(0.125 * (i + 1)) for i in range(n)]
    vs = [F32(0.0625 * (i + 1)) for i in range(n)]
    rays = np.zeros((1, 8), F32)
    rays[0, 6], rays[0, 7] = 1.0, tmax
    classes = [(front or [True] * n, bit0 or [False] * n, ok or [True] * n)]
    return [(list(map(F32, ts)), us, vs, list(cs), list(ps))], classes, rays


def _keys(hits, counts):
    h = hits[0]
    return [(float(h[j, 0:1].view(F32)[0]), int(h[j, 3]), int(h[j, 4])) for j in range(int(counts[0]))]


def _is_miss(rec, tmax):
    return (rec == np.array([np.array([tmax], F32).view(np.uint32)[0], 0, 0, MISS, MISS, 0, 0, 0], np.uint32)).all()


# storage order is not key order: a tie group of four at t = 2 (customIndex, then primitiveId decide), one hit before, two behind
TIES = [(2.0, 7, 1), (3.0, 0, 0), (2.0, 3, 9), (1.0, 9, 9), (2.0, 7, 0), (2.0, 12, 0), (2.5, 1, 1)]
SORTED = [(1.0, 9, 9), (2.0, 3, 9), (2.0, 7, 0), (2.0, 7, 1), (2.0, 12, 0), (2.5, 1, 1), (3.0, 0, 0)]


def test_first_k_cuts_a_tie_group_in_the_middle():
    cands, classes, rays = _one_ray(TIES)
    for k in range(1, 9):
        hits, counts = M.first_k(cands, classes, rays, k, 0)
        assert hits.shape == (1, k, 8) and counts[0] == min(k, 7)
        assert _keys(hits, counts) == SORTED[:k]
        for j in range(int(counts[0]), k):
            assert _is_miss(hits[0, j], 50.0)
    hits, _ = M.first_k(cands, classes, rays, 3, 0)              # u, v travel with their record: (2, 7, 0) was written fifth
    assert hits[0, 2, 1:3].view(F32).tolist() == [0.125 * 5, 0.0625 * 5] and not hits[0, :, 5:].any()


def test_first_k_resumes_strictly_behind_after_inside_a_tie_group():
    cands, classes, rays = _one_ray(TIES)
    first, _ = M.first_k(cands, classes, rays, 3, 0)
    after = first[:, 2, :]                                       # (2, 7, 0): two members of its tie group are still to come
    hits, counts = M.first_k(cands, classes, rays, 3, 0, after=after)
    assert _keys(hits, counts) == SORTED[3:6]
    hits, counts = M.first_k(cands, classes, rays, 3, 0, after=hits[:, 2, :])
    assert _keys(hits, counts) == SORTED[6:] and counts[0] == 1 and _is_miss(hits[0, 1], 50.0) and _is_miss(hits[0, 2], 50.0)
    # chained for every K: each record exactly once
    for k in range(1, 9):
        seen, after = [], None
        for _ in range(10):
            hits, counts = M.first_k(cands, classes, rays, k, 0, after=after)
            if counts[0] == 0:
                break
            seen += _keys(hits, counts)
            after = hits[:, k - 1, :]
        assert seen == SORTED, k
    # an after record that is no member of the set still cuts by its key
    rec = np.zeros((1, 8), np.uint32)
    rec[0, 0], rec[0, 3], rec[0, 4] = np.array([2.0], F32).view(np.uint32)[0], 7, 0xfffffffe
    hits, counts = M.first_k(cands, classes, rays, 8, 0, after=rec)
    assert _keys(hits, counts) == SORTED[4:]


def test_first_k_an_exhausted_after_and_fewer_than_k():
    cands, classes, rays = _one_ray(TIES[:2], tmax=77.0)
    hits, counts = M.first_k(cands, classes, rays, 5, 0)
    assert counts[0] == 2 and _keys(hits, counts) == [(2.0, 7, 1), (3.0, 0, 0)]
    assert all(_is_miss(hits[0, j], 77.0) for j in range(2, 5))
    again, counts = M.first_k(cands, classes, rays, 5, 0, after=hits[:, 4, :])      # the last slot is a miss record: exhausted
    assert counts[0] == 0 and all(_is_miss(again[0, j], 77.0) for j in range(5))
    empty, classes0, rays0 = _one_ray([])
    hits, counts = M.first_k(empty, classes0, rays0, 2, 0)
    assert counts[0] == 0 and _is_miss(hits[0, 0], 50.0) and _is_miss(hits[0, 1], 50.0)
    nan = rays0.copy()
    nan[0, 7] = np.nan                                          # a miss reports the ray's own tmax BITS
    hits, _ = M.first_k(empty, classes0, nan, 1, 0)
    assert hits[0, 0, 0] == nan[0, 7:8].view(np.uint32)[0]


def test_first_k_filters_by_masks_and_flags_before_it_sorts():
    cand = [(1.0, 0, 0), (2.0, 1, 0), (3.0, 2, 0), (4.0, 3, 0), (5.0, 4, 0)]
    front = [True, False, True, False, True]
    bit0 = [False, True, True, False, False]
    ok = [True, True, False, True, True]                          # record 2 fails the opacity map
    cands, classes, rays = _one_ray(cand, front, bit0, ok)

    def customs(flags, **kw):
        hits, counts = M.first_k(cands, classes, rays, 8, flags, **kw)
        return [c for _, c, _ in _keys(hits, counts)]

    assert customs(0) == [0, 1, 3, 4]
    assert customs(W.OPAQUE) == [0, 1, 2, 3, 4]
    assert customs(W.BACK) == [0, 4] and customs(W.FRONT) == [1, 3]
    assert customs(W.CULL_OPAQUE) == [1] and customs(W.CULL_NO_OPAQUE) == [0, 3, 4]
    assert customs(W.FRONT | W.OPAQUE) == [1, 3] and customs(W.BACK | W.CULL_NO_OPAQUE) == [0, 4]
    masks = np.array([0x01, 0x02, 0x04, 0x03, 0x80], np.int64)
    assert customs(W.OPAQUE, custom_masks=masks, ray_masks=0x03) == [0, 1, 3]
    assert customs(W.OPAQUE, custom_masks=masks, ray_masks=0x00) == [] and customs(W.OPAQUE, ray_masks=0) == []
    hits, counts = M.first_k(cands, classes, rays, 2, W.OPAQUE, custom_masks=masks, ray_masks=np.array([0x86]))
    assert [c for _, c, _ in _keys(hits, counts)] == [1, 2]      # the slice comes after the filter


# ---- the layered scene: hit counts known by construction -----------------------------------------------------------------------------
def test_the_layered_scene_has_the_hit_counts_it_was_built_for(oracle, scene_cache):
    from test_gpu_cull_masks import all_hits
    from test_gpu_occlusion import mixed_rays
    desc, keep = M.layered_scene()
    st, nodes, tris = api.host_build_bvh(desc)
    raw = np.frombuffer(tris, dtype=np.uint32).reshape(-1, 12)
    assert len(raw) == 32 and sorted(set(raw[:, 3].tolist())) == list(range(16)) and not (raw[:, 11] & 1).any()
    flt = raw.view(F32)
    z = {int(c): float(flt[raw[:, 3] == c, 2][0]) for c in range(16)}
    assert [z[c] for c in range(12)] == [0.25 * c for c in range(12)] and [z[12 + j] for j in range(4)] == [z[3 + j] for j in range(4)]
    rays, kinds = M.layered_rays(st, mixed_rays)
    assert rays.shape == (256 + 256 + 64 + 256, 8)
    bvh = (nodes, tris)
    cands = all_hits(oracle, bvh, rays)
    n = np.array([len(c[0]) for c in cands])
    for kind in (0, 1):
        inside = M.grid_inside(rays[kinds == kind])
        assert inside.sum() == M.INSIDE and (~inside).sum() == 256 - M.INSIDE >= 100
        assert (n[kinds == kind][inside] >= 16).all() and (n[kinds == kind][~inside] == 0).all()
        off = inside & (rays[kinds == kind][:, 0] != rays[kinds == kind][:, 1])
        assert (n[kinds == kind][off] == 16).all(), "a through ray off the diagonal meets every instance once"
    assert (n[kinds == 2] == 32).all(), "a ray through the shared edge meets both triangles of every layer"
    for k in np.nonzero(kinds == 2)[0][:8]:                      # the two triangles of a layer tie in t, and so do the bit copies
        ts = np.array(cands[k][0], F32)
        assert sorted(set(ts.tolist())) == [1.0 + 0.25 * i for i in range(12)]
        assert [int((ts == F32(1.0 + 0.25 * i)).sum()) for i in range(12)] == [2, 2, 2, 4, 4, 4, 4, 2, 2, 2, 2, 2]
    assert 0 < (n[kinds == 3] > 0).sum() < 256
    # the vectorised float32 restatement lists what oracle_mt lists
    pick = np.concatenate([np.nonzero(kinds == k)[0][::7] for k in range(4)])
    for a, b in zip(M.all_hits32(bvh, rays[pick]), (cands[k] for k in pick)):
        ka = sorted(zip(np.array(a[0], F32).view(np.uint32).tolist(), a[3], a[4], np.array(a[1], F32).view(np.uint32).tolist(),
                        np.array(a[2], F32).view(np.uint32).tolist()))
        kb = sorted(zip(np.array(b[0], F32).view(np.uint32).tolist(), b[3], b[4], np.array(b[1], F32).view(np.uint32).tolist(),
                        np.array(b[2], F32).view(np.uint32).tolist()))
        assert ka == kb


def test_fma32_fast_gives_fma32s_bits():
    rng = np.random.default_rng(11)
    n = 20000
    a = rng.standard_normal(n).astype(F32)
    b = rng.standard_normal(n).astype(F32)
    c = (-(a.astype(np.float64) * b).astype(F32) * F32(1.0 + 2.0 ** -12)).astype(F32)            # heavy cancellation
    c[::3] = rng.standard_normal(len(c[::3])).astype(F32) * F32(1e-3)
    # a * b = 1 + 2^-24 + 2^-46 exactly: the float64 sum with c = +-2^-60 sits on a float32 midpoint and must not be rounded twice
    a[:2] = F32(1.0 + 2.0 ** -23); b[:2] = F32(1.0 - 2.0 ** -24); c[0] = F32(2.0 ** -60); c[1] = F32(-2.0 ** -60)
    a[2:6] = [1e-30, 1e30, 0.0, np.inf]; b[2:6] = [1e-30, 1e30, 5.0, 1.0]; c[2:6] = [1e-45, 1.0, 0.0, 1.0]    # subnormal, overflow, zero, inf
    assert (M.fma32_fast(a, b, c).view(np.uint32) == W.fma32(a, b, c).view(np.uint32)).all()
