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
                        call per (ray, record) pair is out of reach
  tie_stack_scene, tie_stack_rays, tiny_scenes, tiny_rays
                        the constructions of tests/test_gpu_multihit_edges.py, held to their design by tests/test_multihit_edges_abi.py:
                        ties of 20 and 40 records on one t (more than any K), rays for each of the nine compiled walks, windows whose
                        tmin / tmax sit on a layer, and trees of 1, 2, 8 and 9 triangles
  tail_rays             which rays of a launch k_multihit abandoned to k_multihit_tail"""
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


def first_k(cands, classes, rays, k, flags, custom_masks=None, ray_masks=0xff, after=None, lists=None):
    """the expected (N, k, 8) uint32 RtrHit records and (N,) counts of rtr_trace_rays_multi(maxHits = k): the k smallest accepted
    members whose key is strictly greater than after[ray]'s (after: (N, 8) records or None), then the ray's miss record.
    lists: accepted(cands, classes, rays, flags, custom_masks, ray_masks) where the caller has it already (a chain asks once per link)"""
    n = len(rays)
    hits = np.zeros((n, k, 8), np.uint32)
    hits[:, :, 0] = np.ascontiguousarray(rays[:, 7]).view(np.uint32)[:, None]
    hits[:, :, 3] = MISS
    hits[:, :, 4] = MISS
    counts = np.zeros(n, np.int64)
    for r, lst in enumerate(accepted(cands, classes, rays, flags, custom_masks, ray_masks) if lists is None else lists):
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


def _instanced_scene(positions, idx, zs, customs):
    """(desc, keep): one mesh in z = 0 (positions (n, 3), triangles idx), one instance per entry of zs translated to that z — instances of
    equal z carry one transform bit for bit — under the customIndices given"""
    V = np.zeros((len(positions), 12), F32)
    V[:, 0:3] = positions
    V[:, 6] = 1.0                       # the normal: floats 4..6 of the 48-B vertex
    V[:, 8:10] = V[:, 0:2] + F32(0.5)
    idx = np.array(idx, np.uint32)
    n = len(zs)
    meshes = (A.RtrMesh * 1)()
    meshes[0].vertexOffset, meshes[0].indexOffset, meshes[0].vertexCount, meshes[0].indexCount, meshes[0].isOpaque = 0, 0, len(V), len(idx), 1
    inst = (A.RtrInstance * n)()
    for i in range(n):
        inst[i].meshIndex, inst[i].customIndex = 0, int(customs[i])
        for k, val in enumerate((1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, zs[i])):
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


QUAD = ([[-0.5, -0.5, 0.0], [0.5, -0.5, 0.0], [0.5, 0.5, 0.0], [-0.5, 0.5, 0.0]], [0, 1, 2, 0, 2, 3])


def layered_scene():
    """(desc, keep): 16 instances of one quad in z = 0 over [-0.5, 0.5]^2 (triangles (0, 1, 2), (0, 2, 3): the shared edge is the
    diagonal y = x).  Instance i < 12 is translated to z = 0.25 i; instance 12 + j carries the transform of instance 3 + j bit for bit.
    customIndex = the instance's number; 32 triangles in all."""
    n = LAYERS + COPIES
    return _instanced_scene(*QUAD, [0.25 * (i if i < LAYERS else FIRST_COPIED + (i - LAYERS)) for i in range(n)], range(n))


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


# ---- the tie stack: more than K records on one t -------------------------------------------------------------------------------------
TIE_DEPTH = 20
TIE_Z, SINGLE_Z = (0.5, 1.0), (0.0, 0.25, 0.75, 1.25)
TIE_STACK_Z = [0.0, 0.25] + [0.5] * TIE_DEPTH + [0.75] + [1.0] * TIE_DEPTH + [1.25]      # per instance, in instance order
UP_Z, DOWN_Z = -1.0, 4.0              # where the grid rays start: t = z - UP_Z going up, DOWN_Z - z coming down, exact in float32
KIND_UP, KIND_DOWN, KIND_DIAG, KIND_SIGNS, KIND_WINDOW = range(5)
SIGNS_FIRST = 2 * GRID * GRID + 64    # group (c) starts on a multiple of 64: each of its nine runs of 64 rays is one wave of a launch
# group (d): (tmin, tmax) as the z of the layer the bound sits on, None: the bound of the grid ray
WINDOWS = [(0.5, None), (1.0, None), (None, 0.5), (None, 1.0), (0.5, 1.0), (0.25, 1.25), (0.5, 0.5), (0.75, 0.75)]
WINDOW_PICK = slice(3, None, 8)       # 32 rays of each grid: columns 3 and 11 (inside in x), every row (four of them outside in y)


def tie_stack_scene():
    """(desc, keep): the layered scene's quad in 44 instances — 20 carry one transform bit for bit at z = 0.5, 20 more at z = 1.0,
    single layers at z = 0, 0.25, 0.75, 1.25.  Every customIndex is distinct: a fixed seeded permutation of the instance order, so
    storage order and id order disagree.  88 triangles: enough for both builders."""
    return _instanced_scene(*QUAD, TIE_STACK_Z, np.random.default_rng(20).permutation(len(TIE_STACK_Z)))


def sign_pattern(rays):
    """bit 0, 1, 2: the x, y, z component of the direction is negative (the octant the timed kernels dispatch on)"""
    return (rays[:, 4] < 0) * 1 + (rays[:, 5] < 0) * 2 + (rays[:, 6] < 0) * 4


def tie_stack_rays():
    """(rays, kinds) for the tie stack:
      KIND_UP, KIND_DOWN  (a) layered_rays' 16 x 16 grid over [-0.6, 0.6]^2 from z = -1 looking up and from z = 4 looking down;
      KIND_DIAG           (b) 64 +z rays through points ON the shared diagonal, exact in float32;
      KIND_SIGNS          (c) from ray SIGNS_FIRST on: for each of the eight direction-sign patterns p = 0 .. 7 (sign_pattern) 64 oblique
                          rays of that pattern, no component zero, then 64 rays of patterns k mod 8; all through the quads' interior;
      KIND_WINDOW         (d) for each of WINDOWS, the WINDOW_PICK rays of the up grid and of the down grid with tmin, tmax on layers"""
    g = np.linspace(-0.6, 0.6, GRID).astype(F32)
    gx, gy = np.meshgrid(g, g)
    up = np.zeros((GRID * GRID, 8), F32)
    up[:, 0], up[:, 1], up[:, 2], up[:, 6], up[:, 7] = gx.ravel(), gy.ravel(), UP_Z, 1.0, 100.0
    down = up.copy()
    down[:, 2], down[:, 6] = DOWN_Z, -1.0
    x = (np.arange(64, dtype=np.float64) + 0.5) / 64.0 - 0.5            # multiples of 2^-7: exact
    diag = np.zeros((64, 8), F32)
    diag[:, 0], diag[:, 1], diag[:, 2], diag[:, 6], diag[:, 7] = x, x, UP_Z, 1.0, 100.0
    rng = np.random.default_rng(77)
    pattern = np.concatenate([np.repeat(np.arange(8), 64), np.arange(64) % 8])
    n = len(pattern)
    target = np.concatenate([rng.uniform(-0.3, 0.3, (n, 2)), np.full((n, 1), 0.625)], 1)      # mid-way through the stack
    d = np.concatenate([rng.uniform(0.02, 0.12, (n, 2)), np.ones((n, 1))], 1)                 # at most 0.075 sideways on the way out
    d *= np.where((pattern[:, None] >> np.arange(3)) & 1, -1.0, 1.0)
    signs = np.zeros((n, 8), F32)
    signs[:, 0:3], signs[:, 4:7], signs[:, 7] = target - 2.0 * d, d, 100.0
    wins = []
    for zmin, zmax in WINDOWS:
        for src, t_of in ((up, lambda z: z - UP_Z), (down, lambda z: DOWN_Z - z)):
            w = src[WINDOW_PICK].copy()
            lo, hi = (zmin, zmax) if src is up else (zmax, zmin)         # coming down, the far layer is the lower one
            if lo is not None:
                w[:, 3] = t_of(lo)
            if hi is not None:
                w[:, 7] = t_of(hi)
            wins.append(w)
    parts = [up, down, diag, signs, np.concatenate(wins)]
    assert len(up) + len(down) + len(diag) == SIGNS_FIRST and SIGNS_FIRST % 64 == 0
    return np.concatenate(parts).astype(F32), np.repeat(np.arange(5), [len(p) for p in parts])


# ---- tiny trees ----------------------------------------------------------------------------------------------------------------------
TRIANGLE = ([[-0.5, -0.5, 0.0], [0.5, -0.5, 0.0], [0.0, 0.5, 0.0]], [0, 1, 2])
TINY_Z, TINY_BEHIND_Z = 1.0, 1.5


def tiny_scenes():
    """{number of triangles: (desc, keep)} for 1, 2, 8 and 9 triangles: bit copies of one triangle in z = 1 under distinct customIndices
    (a seeded permutation: storage order is not id order), all tied in t; the 9-triangle scene adds one triangle behind the tie, in
    z = 1.5, under the SMALLEST customIndex.  Up to 8 records fit one leaf; 9 do not."""
    out = {}
    for n in (1, 2, 8, 9):
        tied = min(n, 8)
        customs = (np.random.default_rng(n).permutation(tied) + (n - tied)).tolist() + [0] * (n - tied)
        out[n] = _instanced_scene(*TRIANGLE, [TINY_Z] * tied + [TINY_BEHIND_Z] * (n - tied), customs)
    return out


def tiny_rays():
    """rays for the tiny scenes: a 7 x 7 grid over [-0.6, 0.6]^2 looking up from z = -1 and down from z = 3 (through the triangle and
    past it), +z rays through points ON each of the three edges and on the three corners (exact in float32), rays that run ALONG the
    bottom edge inside the triangles' planes (parallel: no hit, but the leaf is reached), and rays far outside the bounds"""
    g = np.linspace(-0.6, 0.6, 7).astype(F32)
    gx, gy = np.meshgrid(g, g)
    up = np.zeros((49, 8), F32)
    up[:, 0], up[:, 1], up[:, 2], up[:, 6], up[:, 7] = gx.ravel(), gy.ravel(), -1.0, 1.0, 100.0
    down = up.copy()
    down[:, 2], down[:, 6] = 3.0, -1.0
    s = np.arange(9, dtype=np.float64) / 8.0                             # 0 .. 1 in eighths: the corners included
    a, b, c = (np.array(v[:2]) for v in TRIANGLE[0])
    pts = np.concatenate([a + s[:, None] * (b - a), b + s[:, None] * (c - b), c + s[:, None] * (a - c)])
    edge = np.zeros((len(pts), 8), F32)
    edge[:, 0:2], edge[:, 2], edge[:, 6], edge[:, 7] = pts, -1.0, 1.0, 100.0
    along = np.zeros((4, 8), F32)
    along[:, 7] = 100.0
    along[0, 0:3], along[0, 4] = (-2.0, -0.5, TINY_Z), 1.0
    along[1, 0:3], along[1, 4] = (2.0, -0.5, TINY_Z), -1.0
    along[2, 0:3], along[2, 4] = (-2.0, -0.5, TINY_BEHIND_Z), 1.0
    along[3, 0:3], along[3, 4:6] = (1.5, -2.5, TINY_Z), (-0.5, 1.0)        # the edge (0.5, -0.5) -> (0, 0.5), from two edge lengths before it
    away = np.zeros((4, 8), F32)
    away[:, 7] = 100.0
    away[:, 0:3] = [[5.0, 5.0, -1.0], [-5.0, 0.0, -1.0], [0.0, 0.0, 5.0], [0.0, 0.0, -1.0]]
    away[:, 4:7] = [[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0]]      # beside, beside, behind looking away, in front looking away
    return np.concatenate([up, down, edge, along, away]).astype(F32)


# ---- which rays of a launch took the tail kernel -------------------------------------------------------------------------------------
def tail_rays(tail_count, n, cap=64, first_groups=32):
    """indices of up to `cap` rays that k_multihit abandoned.  tail_count(idx) launches the rays idx alone, counting form, and returns
    stats.tailRays: a group whose tailRays equals its size holds only such rays (a lone deep ray walks for a tenth of a second, so the
    groups are halved, not the rays asked one by one)"""
    tail = []

    def collect(idx):
        if len(tail) >= cap or not len(idx):
            return
        c = tail_count(idx)
        if c == len(idx):
            tail.extend(int(i) for i in idx)
        elif c:
            collect(idx[:len(idx) // 2]); collect(idx[len(idx) // 2:])

    for first in range(0, n, first_groups):
        collect(np.arange(first, min(first + first_groups, n)))
    return tail[:cap]
