"""The test-side witness of the multi-hit query (rtr_trace_rays_multi; tests/test_multihit_abi.py, tests/test_gpu_multihit.py).

  accepted, first_k     "the first K hits" as a sort and a slice of a list the tests already own: test_gpu_cull_masks.all_hits' candidates
                        (every record oracle_mt accepts), classed by ray_flags_witness.classify and filtered exactly as
                        ray_flags_witness.filtered filters them, sorted by (t, customIndex, primitiveId), cut behind `after` (strictly
                        greater keys only; a miss record there exhausts the ray), sliced, padded with the ray's miss record
  layered_scene, layered_rays
                        a scene whose hit counts are known by construction: one unit quad (2 triangles) in 16 instances — 12 layers
                        z = 0.25 i, exact in float32, and 4 bit copies of layers 3..6 under other customIndices: exact ties in t
  fma32_fast, all_hits32
                        every accepted record of a ray by the float32 restatement of rtr_mt_intersect (ray_flags_witness.mt32, held to
                        oracle_mt's bits by test_ray_flags_abi.py), vectorised over the records: for the rays that graze the 2^19
                        coplanar triangles of test_gpu_query._deep_scene, where no float64 prefilter is conservative and one ctypes
                        call per (ray, record) pair is out of reach"""
import ctypes as C

import numpy as np

from realtimeraytracer_amd import _abi as A

import ray_flags_witness as W

F32 = np.float32
MISS = 0xFFFFFFFF


def accepted(cands, classes, rays, flags, custom_masks=None, ray_masks=0xff):
    """per ray: the sorted list of ((t, customIndex, primitiveId), u, v) of the candidates that survive the instance masks (by
    customIndex; None: 0xff), the rays' masks and flags (RTR_QUERY_OPAQUE and the four culling flags) — ray_flags_witness.filtered's
    filter, every survivor kept"""
    n = len(rays)
    ray_masks = np.broadcast_to(np.asarray(ray_masks, np.int64), (n,))
    out = []
    for k, ((ts, us, vs, cs, ps), (front, bit0, ok)) in enumerate(zip(cands, classes)):
        keep = []
        for tt, uu, vv, c, p, fr, b0, al in zip(ts, us, vs, cs, ps, front, bit0, ok):
            if custom_masks is not None and not (custom_masks[c] & ray_masks[k]):
                continue
            if custom_masks is None and not ray_masks[k]:
                continue
            nonopaque = b0 and not (flags & W.OPAQUE)
            if (flags & W.CULL_OPAQUE and not nonopaque) or (flags & W.CULL_NO_OPAQUE and nonopaque):
                continue
            if (flags & W.FRONT and fr) or (flags & W.BACK and not fr):
                continue
            if nonopaque and not al:
                continue
            keep.append(((F32(tt), int(c), int(p)), F32(uu), F32(vv)))
        keep.sort(key=lambda e: e[0])
        out.append(keep)
    return out


def after_key(rec):
    """(t, customIndex, primitiveId) of an RtrHit record given as 8 32-bit words, or None for a miss record (the ray is exhausted)"""
    w = np.asarray(rec).view(np.uint32)
    if int(w[3]) == MISS:
        return None
    return (w[0:1].view(F32)[0], int(w[3]), int(w[4]))


def first_k(cands, classes, rays, k, flags, custom_masks=None, ray_masks=0xff, after=None):
    """the expected (N, k, 8) uint32 RtrHit records and (N,) counts of rtr_trace_rays_multi(maxHits = k): the k smallest accepted
    members whose key is strictly greater than after[ray]'s (after: (N, 8) records or None), then the ray's miss record"""
    n = len(rays)
    hits = np.zeros((n, k, 8), np.uint32)
    hits[:, :, 0] = np.ascontiguousarray(rays[:, 7]).view(np.uint32)[:, None]
    hits[:, :, 3] = MISS
    hits[:, :, 4] = MISS
    counts = np.zeros(n, np.int64)
    for r, lst in enumerate(accepted(cands, classes, rays, flags, custom_masks, ray_masks)):
        if after is not None:
            key = after_key(after[r])
            lst = [] if key is None else [e for e in lst if e[0] > key]
        for j, ((t, c, p), u, v) in enumerate(lst[:k]):
            hits[r, j, 0:3] = np.array([t, u, v], F32).view(np.uint32)
            hits[r, j, 3], hits[r, j, 4] = c, p
        counts[r] = min(k, len(lst))
    return hits, counts


def trivial_classes(cands):
    """classes for scenes without alpha-tested geometry queried without facing flags: nothing the filter reads matters"""
    return [([True] * len(c[0]), [False] * len(c[0]), [True] * len(c[0])) for c in cands]


# ---- the layered scene ---------------------------------------------------------------------------------------------------------------
LAYERS, COPIES, FIRST_COPIED = 12, 4, 3


def layered_scene():
    """(desc, keep): 16 instances of one quad in z = 0 over [-0.5, 0.5]^2 (triangles (0, 1, 2), (0, 2, 3): the shared edge is the
    diagonal y = x).  Instance i < 12 is translated to z = 0.25 i; instance 12 + j carries the transform of instance 3 + j bit for bit.
    customIndex = the instance's number; 32 triangles in all."""
    V = np.zeros((4, 12), F32)
    V[:, 0:3] = [[-0.5, -0.5, 0.0], [0.5, -0.5, 0.0], [0.5, 0.5, 0.0], [-0.5, 0.5, 0.0]]
    V[:, 6] = 1.0                       # the normal: floats 4..6 of the 48-B vertex
    V[:, 8:10] = V[:, 0:2] + F32(0.5)
    idx = np.array([0, 1, 2, 0, 2, 3], np.uint32)
    n = LAYERS + COPIES
    meshes = (A.RtrMesh * 1)()
    meshes[0].vertexOffset, meshes[0].indexOffset, meshes[0].vertexCount, meshes[0].indexCount, meshes[0].isOpaque = 0, 0, 4, 6, 1
    inst = (A.RtrInstance * n)()
    for i in range(n):
        inst[i].meshIndex, inst[i].customIndex = 0, i
        layer = i if i < LAYERS else FIRST_COPIED + (i - LAYERS)
        for k, val in enumerate((1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0.25 * layer)):
            inst[i].transform[k] = float(val)
    objs = (A.RtrObjectInfo * n)()
    for o in objs:
        o.vertexOffset, o.indexOffset = 0, 0
        o.color[0] = o.color[1] = o.color[2] = 0.8
    d = A.rtr_scene_desc()
    d.vertices = V.ctypes.data_as(C.POINTER(A.RtrVertex)); d.numVertices = len(V)
    d.indices = idx.ctypes.data_as(C.POINTER(A.u32)); d.numIndices = len(idx)
    d.meshes, d.numMeshes = meshes, 1
    d.instances, d.numInstances = inst, n
    d.objects, d.numObjects = objs, n
    d.skyColor[0] = d.skyColor[1] = d.skyColor[2] = 0.5
    return d, (V, idx, meshes, inst, objs)


GRID = 16
INSIDE = 12 * 12                  # grid points with |x|, |y| < 0.5: 12 of the 16 per axis


def layered_rays(st, mixed_rays):
    """(rays, kinds): 256 +z rays on a 16 x 16 grid over [-0.6, 0.6]^2 from z = -1 (kind 0), the same grid from z = 4 looking back
    (kind 1), 64 +z rays through points ON the diagonal, exact in float32 (kind 2), 256 oblique rays of test_gpu_occlusion.mixed_rays
    (kind 3).  st: the scene's stats (bounds)."""
    g = np.linspace(-0.6, 0.6, GRID).astype(F32)
    gx, gy = np.meshgrid(g, g)
    up = np.zeros((GRID * GRID, 8), F32)
    up[:, 0], up[:, 1], up[:, 2], up[:, 6], up[:, 7] = gx.ravel(), gy.ravel(), -1.0, 1.0, 100.0
    down = up.copy()
    down[:, 2], down[:, 6] = 4.0, -1.0
    x = (np.arange(64, dtype=np.float64) + 0.5) / 64.0 - 0.5            # multiples of 2^-7: exact
    diag = np.zeros((64, 8), F32)
    diag[:, 0], diag[:, 1], diag[:, 2], diag[:, 6], diag[:, 7] = x, x, -1.0, 1.0, 100.0
    size = float(np.linalg.norm(np.array(st.boundsMax[:]) - np.array(st.boundsMin[:])))
    obl = mixed_rays(st, 256, 5, size)
    rays = np.concatenate([up, down, diag, obl]).astype(F32)
    kinds = np.repeat(np.arange(4), [len(up), len(down), len(diag), len(obl)])
    return rays, kinds


def grid_inside(rays):
    """of grid rays: does the ray pass through the quads' interior?"""
    return (np.abs(rays[:, 0]) < 0.5) & (np.abs(rays[:, 1]) < 0.5)


# ---- every accepted record by the float32 restatement, vectorised over the records ---------------------------------------------------
def fma32_fast(a, b, c):
    """ray_flags_witness.fma32's value, cheaper on long arrays: the float64 sum of the exact product and c, rounded to float32.  That
    double rounding differs from the single one only where the float64 sum sits exactly on a float32 midpoint (its low 29 significand
    bits are 1 followed by zeros); those elements — and those outside float32's normal range, where the midpoints lie elsewhere — are
    redone by fma32."""
    a, b, c = (np.atleast_1d(np.asarray(x, F32)) for x in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        s = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
        r = s.astype(F32)
        mag = np.abs(s)
    redo = ((s.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)) | ~(mag >= 2.0 ** -125) | ~(mag < 2.0 ** 127)
    redo &= s != 0
    if redo.any():
        r[redo] = W.fma32(a[redo], b[redo], c[redo])
    return r


def _dot(a, b):
    return fma32_fast(a[..., 2], b[..., 2], fma32_fast(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))


def _cross(a, b):
    return np.stack([fma32_fast(a[..., 1], b[..., 2], -(a[..., 2] * b[..., 1])),
                     fma32_fast(a[..., 2], b[..., 0], -(a[..., 0] * b[..., 2])),
                     fma32_fast(a[..., 0], b[..., 1], -(a[..., 1] * b[..., 0]))], axis=-1)


def all_hits32(bvh, rays, threads=8):
    """test_gpu_cull_masks.all_hits' list — per ray (t, u, v, customIndex, primitiveId) of every record rtr_mt_intersect accepts with
    t < tmax — from ray_flags_witness.mt32's operations, in two stages: the determinant and u for every record, the rest for those whose
    u passed.  The rays are shared among a few threads (numpy drops the interpreter lock inside its loops)."""
    from concurrent.futures import ThreadPoolExecutor
    raw = np.frombuffer(bvh[1], dtype=np.uint32).reshape(-1, 12)
    flt = raw.view(F32)
    v0, e1, e2 = flt[:, 0:3], flt[:, 4:7], flt[:, 8:11]

    def one(r):
        tmin, tmax = r[3], r[7]
        got = ([], [], [], [], [])
        if tmax > tmin and np.isfinite(r[[0, 1, 2, 4, 5, 6]]).all() and r[4:7].any():
            o, d = r[0:3], r[4:7]
            with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
                h = _cross(np.broadcast_to(d, e2.shape), e2)
                a = _dot(e1, h)
                f = F32(1.0) / a
                s = o - v0
                u = f * _dot(s, h)
                js = np.nonzero(~(np.abs(a) < W.EPS) & ~((u < 0) | (u > 1)))[0]
            if len(js):
                ok, t, uu, vv, _ = W.mt32(o, d, v0[js], e1[js], e2[js], tmin)
                assert (uu.view(np.uint32) == u[js].view(np.uint32)).all()
                for i in np.nonzero(ok & (t < tmax))[0]:
                    for lst, x in zip(got, (t[i], uu[i], vv[i], int(raw[js[i], 3]), int(raw[js[i], 7]))):
                        lst.append(x)
        return got

    with ThreadPoolExecutor(max(1, int(threads))) as pool:
        return list(pool.map(one, rays))
