"""Shapes for the launch-shape tests of the ray queries (tests/test_gpu_occlusion_shapes.py, tests/test_gpu_query_shapes.py), held to
the source's constants by tests/test_shape_constants.py.  No tests in here.

  EDGES                 ray counts on both sides of every constant that cuts a query launch up: the wave (64), the any-hit batch
                        (occlusion_batch: 256, and 512 from BIG_BATCH_FROM rays on), the queue build's lane count (kOccGenBlock) and its
                        chunk (kOcclusionGenRays), two chunks, and nine chunks plus one ray — every blockIdx.x % kQueueRegions and one twice
  soup_scene            216 triangles, one per cell of a 6 x 6 x 6 lattice, in three instances (triangle index % 3)
  targeted_rays         rays aimed at the inside of a triangle from an octant the caller names per ray; about half stop short of it
  kill                  the ways a ray is dead before any walk
  layout                a ray set laid out by octant as a selection (with repeats) from a master set: an answer is a function of the ray
                        alone, so the expected answers are the master's, selected the same way
  Reference             both references of a ray set — multihit_witness.all_hits32 (float32, bit-exact) and witness.ray_hits (float64, with
                        its `ambiguous` flag) — and the conditions under which they are a reference at all"""
import ctypes as C

import numpy as np

from realtimeraytracer_amd import _abi as A

import multihit_witness as MW
import ray_flags_witness as RW
import witness

F32 = np.float32
MISS = 0xFFFFFFFF

WAVE = 64
BATCH, BIG_BATCH, BIG_BATCH_FROM = 256, 512, 100 << 20      # occlusion_batch(n)
GEN_BLOCK, GEN_RAYS = 512, 4096                             # kOccGenBlock, kOcclusionGenRays
REGIONS = 8                                                 # kQueueRegions
EDGES = (1, 2, WAVE - 1, WAVE, WAVE + 1, BATCH - 1, BATCH, BATCH + 1, GEN_BLOCK - 1, GEN_BLOCK, GEN_BLOCK + 1,
         GEN_RAYS - 1, GEN_RAYS, GEN_RAYS + 1, 2 * GEN_RAYS - 1, 2 * GEN_RAYS + 1, (REGIONS + 1) * GEN_RAYS + 1)
MASTER = EDGES[-1]

LIGHT_BLOCK, LIGHT_STAGED_SLOTS, LIGHT_STAGED_LDS = 64, 31, 64 << 10     # kLightRaysBlock, kLightStagedSlots, kLightStagedLds

AMBIGUOUS_CAP = 0.005
OCCLUDED_SHARE = (0.3, 0.7)


def occlusion_list_stride(n):
    """occlusion_list_stride(n) of kernels/rtr_query.h"""
    return n // BATCH // REGIONS + (n + GEN_RAYS - 1) // GEN_RAYS + 1


def worst_list_length(n, batch=BATCH):
    """the most batches one of the 64 lists can be handed by a launch of n rays: every chunk all of one octant, and the list served first
    by every workgroup's rotation"""
    total, left = 0, n
    while left > 0:
        ln = min(left, GEN_RAYS)
        nb = -(-ln // batch)
        total += -(-nb // REGIONS)
        left -= ln
    return total


def hinted_stage_fits(q):
    """does the hinted k_light_rays stage Q slots per hit: 64 lanes x ((2Q + 1) pieces of 16 B + (Q | 1) hint words)"""
    return q <= LIGHT_STAGED_SLOTS and LIGHT_BLOCK * ((2 * q + 1) * 16 + (q | 1) * 4) <= LIGHT_STAGED_LDS


# ---- the scene ------------------------------------------------------------------------------------------------------------------------
LATTICE = 6
NUM_TRIS = LATTICE ** 3
NUM_INSTANCES = 3


def soup_corners():
    """(216, 3, 3) float32 corners: centres 2 (i, j, k) + 1 + U(-0.3, 0.3)^3, v0 = c - 0.5 a - 0.5 b, v1 = v0 + 1.4 a, v2 = v0 + 1.4 b
    with a, b random unit vectors"""
    rng = np.random.default_rng(1)
    g = np.arange(LATTICE, dtype=np.float64)
    c = 2.0 * np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + 1.0 + rng.uniform(-0.3, 0.3, (NUM_TRIS, 3))
    a, b = rng.normal(size=(NUM_TRIS, 3)), rng.normal(size=(NUM_TRIS, 3))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    v0 = c - 0.5 * a - 0.5 * b
    return np.stack([v0, v0 + 1.4 * a, v0 + 1.4 * b], 1).astype(F32)


def soup_scene():
    """(desc, keep): the soup as three meshes in three instances with identity transforms and customIndex 0, 1, 2 — triangle t is
    primitive t // 3 of instance t % 3.  All opaque, no lights."""
    corners = soup_corners()
    parts = [corners[m::NUM_INSTANCES].reshape(-1, 3) for m in range(NUM_INSTANCES)]
    V = np.zeros((3 * NUM_TRIS, 12), F32)
    V[:, 0:3] = np.concatenate(parts)
    V[:, 6] = 1.0
    idx = np.concatenate([np.arange(len(p), dtype=np.uint32) for p in parts])
    n = NUM_INSTANCES
    meshes, inst, objs = (A.RtrMesh * n)(), (A.RtrInstance * n)(), (A.RtrObjectInfo * n)()
    at = 0
    for m in range(n):
        k = len(parts[m])
        meshes[m].vertexOffset, meshes[m].indexOffset, meshes[m].vertexCount, meshes[m].indexCount, meshes[m].isOpaque = at, at, k, k, 1
        inst[m].meshIndex, inst[m].customIndex = m, m
        for j, val in enumerate((1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)):
            inst[m].transform[j] = float(val)
        objs[m].vertexOffset, objs[m].indexOffset = at, at
        objs[m].color[0] = objs[m].color[1] = objs[m].color[2] = 0.8
        at += k
    d = A.rtr_scene_desc()
    d.vertices = V.ctypes.data_as(C.POINTER(A.RtrVertex)); d.numVertices = len(V)
    d.indices = idx.ctypes.data_as(C.POINTER(A.u32)); d.numIndices = len(idx)
    d.meshes, d.numMeshes = meshes, n
    d.instances, d.numInstances = inst, n
    d.objects, d.numObjects = objs, n
    d.skyColor[0] = d.skyColor[1] = d.skyColor[2] = 0.5
    return d, (V, idx, meshes, inst, objs)


def records(tris):
    """(raw uint32 (T, 12), the same as float32) of exported triangle records: v0, customIndex, e1, primitiveId, e2, flags"""
    raw = np.frombuffer(tris, dtype=np.uint32).reshape(-1, 12)
    return raw, raw.view(F32)


# ---- rays -----------------------------------------------------------------------------------------------------------------------------
def targeted_rays(octants, seed, corners=None):
    """one ray per entry of octants (bit 0, 1, 2: the x, y, z component of the direction is negative): aimed at the point (u, v) ~
    U(0.15, 0.35)^2 of a random triangle, direction | N(0, 1)^3 | + 0.2 normalised and signed by the octant, from L ~ U(2, 6) before the
    point, tmin = 0.001, tmax = 1.5 L or 0.5 L with equal odds"""
    corners = soup_corners() if corners is None else corners
    octants = np.asarray(octants, np.int64)
    n = len(octants)
    rng = np.random.default_rng(seed)
    k = rng.integers(0, len(corners), n)
    uv = rng.uniform(0.15, 0.35, (n, 2))
    c = corners[k].astype(np.float64)
    p = c[:, 0] + (c[:, 1] - c[:, 0]) * uv[:, :1] + (c[:, 2] - c[:, 0]) * uv[:, 1:]
    d = np.abs(rng.normal(size=(n, 3))) + 0.2
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= np.where((octants[:, None] >> np.arange(3)) & 1, -1.0, 1.0)
    L = rng.uniform(2.0, 6.0, n)
    far = rng.uniform(0.0, 1.0, n) < 0.5
    r = np.zeros((n, 8), F32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = p - L[:, None] * d, 0.001, d, np.where(far, 1.5, 0.5) * L
    return r


def octant_of(rays):
    return MW.sign_pattern(rays)


DEAD_KINDS = ("null", "zero_direction", "nan_origin", "inf_direction", "tmax_eq_tmin", "tmax_lt_tmin")


def kill(rays, rows, kind):
    """make rays[rows] dead in place: the null ray, a zero direction, a NaN origin word, an infinite direction word, an empty interval
    (tmax == tmin) or a reversed one.  kind "mixed": the kinds in turn."""
    rows = np.arange(len(rays))[rows]
    if kind == "mixed":
        for j, k in enumerate(DEAD_KINDS):
            kill(rays, rows[j::len(DEAD_KINDS)], k)
    elif kind == "null":
        rays[rows] = 0.0
    elif kind == "zero_direction":
        rays[rows, 4:7] = 0.0
    elif kind == "nan_origin":
        rays[rows, rows % 3] = np.nan
    elif kind == "inf_direction":
        rays[rows, 4 + rows % 3] = np.where(rows % 2, np.inf, -np.inf).astype(F32)
    elif kind == "tmax_eq_tmin":
        rays[rows, 7] = rays[rows, 3]
    elif kind == "tmax_lt_tmin":
        rays[rows, 7] = rays[rows, 3] - F32(0.5)
    else:
        raise ValueError(kind)
    return rays


def well_formed(rays):
    """the rays the counting forms count: origin and direction finite, direction not zero (an empty interval is counted)"""
    return np.isfinite(rays[:, [0, 1, 2, 4, 5, 6]]).all(1) & (rays[:, 4:7] != 0).any(1)


def layout(master_octants, want):
    """indices into the master set that give ray i the octant want[i] (-1: any ray; the caller kills those): the master's rays of that
    octant in order, again from the first when they run out"""
    want = np.asarray(want, np.int64)
    out = np.arange(len(want)) % len(master_octants)
    for o in range(8):
        pool = np.nonzero(master_octants == o)[0]
        at = np.nonzero(want == o)[0]
        out[at] = pool[np.arange(len(at)) % len(pool)]
    return out


def runs(n, length):
    """octants in runs of `length` rays: 0 .. 7 and over again"""
    return np.arange(n) // length % 8


def chunk_counts(n, octant, count, rest):
    """per 4096-ray chunk exactly `count` rays of `octant`, spread through the chunk, and the others of `rest`"""
    want = np.full(n, rest, np.int64)
    for first in range(0, n, GEN_RAYS):
        ln = min(GEN_RAYS, n - first)
        c = min(count, ln)
        want[first + (np.arange(c) * ln) // c] = octant
        assert int((want[first:first + ln] == octant).sum()) == c
    return want


# ---- the references -------------------------------------------------------------------------------------------------------------------
def all_hits32_batched(tris, rays, chunk=1024):
    """multihit_witness.all_hits32's lists, computed for `chunk` rays at a time: the same float32 operations (its _cross and _dot for the
    determinant and u of every (ray, record) pair, ray_flags_witness.mt32 for the pairs whose u passed) on arrays over the pairs instead
    of over one ray's records.  all_hits32 spends a millisecond of interpreter per ray, which 36 865 rays cannot afford; Reference holds
    this function to it, list for list and bit for bit, on a sample of every ray set."""
    raw, flt = records(tris)
    v0, e1, e2 = flt[:, 0:3], flt[:, 4:7], flt[:, 8:11]
    out = [([], [], [], [], []) for _ in range(len(rays))]
    live = np.nonzero((rays[:, 7] > rays[:, 3]) & well_formed(rays))[0]
    for lo in range(0, len(live), chunk):
        rows = live[lo:lo + chunk]
        o, d = rays[rows, None, 0:3], rays[rows, None, 4:7]
        shape = (len(rows),) + e2.shape
        with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
            h = MW._cross(np.broadcast_to(d, shape), np.broadcast_to(e2, shape))
            a = MW._dot(np.broadcast_to(e1, shape), h).reshape(shape[:2])
            f = F32(1.0) / a
            s = o - v0[None]
            u = f * MW._dot(s, h).reshape(shape[:2])
            ri, js = np.nonzero(~(np.abs(a) < RW.EPS) & ~((u < 0) | (u > 1)))
        if not len(ri):
            continue
        r = rows[ri]
        ok, t, uu, vv, _ = RW.mt32(rays[r, 0:3], rays[r, 4:7], v0[js], e1[js], e2[js], rays[r, 3])
        assert (uu.view(np.uint32) == u[ri, js].view(np.uint32)).all()
        for i in np.nonzero(ok & (t < rays[r, 7]))[0]:
            for lst, x in zip(out[r[i]], (t[i], uu[i], vv[i], int(raw[js[i], 3]), int(raw[js[i], 7]))):
                lst.append(x)
    return out


def same_lists(a, b):
    return len(a) == len(b) and all(
        [np.asarray(x[k], np.float32).view(np.uint32).tolist() for k in range(3)] + [list(x[3]), list(x[4])]
        == [np.asarray(y[k], np.float32).view(np.uint32).tolist() for k in range(3)] + [list(y[3]), list(y[4])] for x, y in zip(a, b))


class Reference:
    """Both references of a ray set over exported triangle records.
      cands, lists      (a) multihit_witness.all_hits32's candidates and their sorted lists (multihit_witness.accepted)
      hits, occluded    (a)'s closest-hit RtrHit records ((N, 8) uint32; a miss: t = tmax, ids -1) and occlusion bytes
      best, ambiguous   (b) witness.ray_hits' closest record (row of the export, -1: none) and its `ambiguous` flag
    check() asserts what makes them a reference: few ambiguous rays, agreement on the others, a balanced occluded share."""

    def __init__(self, tris, rays, threads=8):
        self.rays = rays
        raw, flt = records(tris)
        self.raw = raw
        self.cands = all_hits32_batched(tris, rays)
        sample = np.unique(np.concatenate([np.arange(min(len(rays), 192)), np.arange(len(rays))[::max(1, len(rays) // 192)]]))
        assert same_lists([self.cands[i] for i in sample], MW.all_hits32((None, tris), rays[sample], threads=threads)), \
            "all_hits32_batched is not multihit_witness.all_hits32"
        self.lists = MW.accepted(self.cands, MW.trivial_classes(self.cands), rays, 0)
        self.hits, cnt = MW.first_k(None, None, rays, 1, 0, lists=self.lists)
        self.hits = self.hits[:, 0, :]
        self.occluded = (cnt > 0).astype(np.uint8)
        v0, e1, e2 = (flt[:, a:a + 3].astype(np.float64) for a in (0, 4, 8))
        self.best, _, _, _, _, amb, ties = witness.ray_hits(v0, v0 + e1, v0 + e2, rays)
        self.ambiguous = (amb | (ties > 1)) & well_formed(rays)      # a malformed ray has one answer in any arithmetic: a miss
        row = {(int(c), int(p)): j for j, (c, p) in enumerate(zip(raw[:, 3], raw[:, 7]))}
        self.rows = np.array([row[(int(c), int(p))] if int(c) != MISS else -1 for c, p in self.hits[:, 3:5]], np.int64)

    def first_k(self, k, n=None):
        n = len(self.rays) if n is None else n
        return MW.first_k(None, None, self.rays[:n], k, 0, lists=self.lists[:n])

    def describe(self, n=None):
        n = len(self.rays) if n is None else n
        return f"reference over {n} rays: ambiguous share {self.ambiguous[:n].mean():.5f}, occluded share {self.occluded[:n].mean():.3f}"

    def check(self, n=None):
        """the conditions on the first n rays; the occluded share only from 63 rays on (of one or two rays it is 0, 0.5 or 1).
        Returns describe(n), for the failure messages of what is compared against this reference."""
        n = len(self.rays) if n is None else n
        what = self.describe(n)
        amb = self.ambiguous[:n]
        assert amb.mean() <= AMBIGUOUS_CAP, what
        bad = ~amb & (self.rows[:n] != self.best[:n])
        assert not bad.any(), f"{what}: the float32 and float64 references disagree on unambiguous rays {np.nonzero(bad)[0][:8].tolist()}"
        if n >= WAVE - 1:
            assert OCCLUDED_SHARE[0] <= self.occluded[:n].mean() <= OCCLUDED_SHARE[1], what
        return what


# ---- what the test files share --------------------------------------------------------------------------------------------------------
def assert_same_bytes(got, exp, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.dtype == np.uint8 and got.shape == exp.shape, f"{what}: {got.dtype} {got.shape}"
    assert set(np.unique(got).tolist()) <= {0, 1}, f"{what}: bytes other than 0 and 1: {np.unique(got).tolist()}"
    bad = got != exp
    if bad.any():
        k = np.nonzero(bad)[0][:8]
        raise AssertionError(f"{what}: {int(bad.sum())} of {len(got)} rays differ; first {k.tolist()}: got {got[k].tolist()} expected {exp[k].tolist()}")


class World:
    """the soup on a context, MASTER targeted rays with uniformly drawn octants, and their Reference, made once for a session"""

    def __init__(self, ctx):
        import torch
        from realtimeraytracer_amd import api
        self.desc, self.keep = soup_scene()
        self.scene = api.Scene(ctx, self.desc)
        self.octants = np.random.default_rng(2).integers(0, 8, MASTER)
        self.rays = targeted_rays(self.octants, 3)
        assert (octant_of(self.rays) == self.octants).all()
        self.rays_t = torch.from_numpy(self.rays).cuda()
        self.ref = Reference(self.scene.export_bvh()[1], self.rays)
        self.ref.check()


_WORLDS = {}


def world(ctx):
    if id(ctx) not in _WORLDS:
        _WORLDS[id(ctx)] = (ctx, World(ctx))
    return _WORLDS[id(ctx)][1]
