"""MIS at a path vertex (rtr_mis_pick_weights, rtr_emitter_hits) on the device, in the Cornell box with three lights of 2 + 1 + 2
triangles, the middle one two-sided.
  * pick side: every RtrMisSample is made of what the picked ray, rtr_hit_surfaces, the exported light table and the host forms of
    include/rtr_mis.h give, word for word; the weights are (float)Ttot / (float)P * wPick; picks without a ray give zeros;
  * bounce side: the device's RtrEmitter records equal rtr_host_emitter_hits' word for word, on constructed rays that reach every rule
    and on the bounce rays of a camera frame;
  * nothing is written behind an output;
  * api.path_trace_mis: path_trace_picked's bytes without bounces, its mean with one, the plain loop's bytes when compacted, and
    path_trace / path_trace_picked are the loops they were."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api, host, scenes

pytestmark = pytest.mark.gpu

NS = 3
W = H = 64
GUARD = 0x5A5A5A5A
SIZES = [1, 63, 64, 65, 257, W * H]


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _bits(x):
    return np.ascontiguousarray(_np(x)).view(np.uint32)


def _i32(x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).cuda()


def _f32(x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.float32)).cuda()


def _box_scene(directory, lights, width=W, height=H, back_seen_quad=False):
    """the Cornell box with the given lights: (triangles 1 or 2, two-sided, x) each, below the ceiling, facing down.  back_seen_quad: one
    more quad, 345 x 345 at z = 150 between the camera and the lights, about a quarter of the frame, whose vertex normals point AWAY
    from the camera (+z, towards the back wall): every camera hit on it has dot(N, V) < 0, a face seen from behind its vertex normals,
    and the three lights are in its normals' hemisphere.  Roughness 1, metallic 0.5: both lobes of the bounce carry weight.
    back_seen_quad="full": the same quad 757 x 757, which fills the frame."""
    tri = os.path.join(directory, "mis_light_triangle.obj")
    if not os.path.exists(tri):
        with open(tri, "w") as f:
            f.write("v -0.5 -0.5 0\nv 0.5 -0.5 0\nv 0 0.5 0\nf 1 2 3\n")
    quad = os.path.join(directory, "mis_back_seen_quad_full.obj" if back_seen_quad == "full" else "mis_back_seen_quad.obj")
    if back_seen_quad and not os.path.exists(quad):
        x0, x1, y0, y1 = (-100.5, 656.5, -105.5, 651.5) if back_seen_quad == "full" else (105.5, 450.5, 100.5, 445.5)
        with open(quad, "w") as f:
            f.write(f"v {x0} {y0} 150\nv {x1} {y0} 150\nv {x1} {y1} 150\nv {x0} {y1} 150\nvn 0 0 1\nf 1//1 2//1 3//1\nf 1//1 3//1 4//1\n")
    obj, mtldir = scenes.write_cornell(None)
    hs = host.HostScene()
    for k, (tris, two_sided, x) in enumerate(lights):
        light = hs.addAreaLight(20.0 - 5.0 * k, (1.0, 0.85 - 0.2 * k, 0.6 + 0.1 * k), two_sided, True, tri if tris == 1 else None)
        light.move((x, 540.0, 279.5)).scale((130.0, 105.0, 1.0)).rotate((90.0, 0.0, 0.0))
    if back_seen_quad:
        hs.addObject(quad).setColor((0.8, 0.6, 0.4)).setSpecular(0.0).setMetallic(0.5)          # roughness is 1 - specular
    hs.addObjMtlPair(obj, mtldir)
    hs.setSky((0.5, 0.7, 1.0))
    hs.build()
    pos = (278.0, 273.0, -800.0)
    cam = host.Camera(40.0, pos, (278.0, 273.0, 0.0), (0.0, 1.0, 0.0), width, height)
    return scenes.SceneSetup("cornell_lights", hs, cam, pos, width, height)


THREE_LIGHTS = [(2, False, 150.0), (1, True, 278.0), (2, False, 410.0)]


class World:
    """the scene, its camera hits and their surfaces, the exported light table: computed once, never changed"""
    def __init__(self, ctx, directory, back_seen_quad=False):
        self.s = _box_scene(directory, THREE_LIGHTS, back_seen_quad=back_seen_quad)
        self.scene = api.Scene(ctx, self.s.desc)
        self.rays = api.camera_rays(ctx, self.s.camera, W, H, 1)
        self.hits = api.trace_rays(self.scene, self.rays).hits
        self.surf = api.hit_surfaces(self.scene, self.rays, self.hits)
        self.rec, self.first = self.scene.export_light_tris()
        self.lights = [self.s.desc.lights[i] for i in range(self.s.num_lights)]
        self.frame = 5

    def params(self, area_lights=3):
        return api.make_light_params(area_lights, NS, self.frame, W, 1, A.LIGHT_SHADOWED)


@pytest.fixture(scope="module")
def world(gpu_ctx, scene_cache):
    wd = World(gpu_ctx, scene_cache)
    yield wd
    wd.scene.close()


@pytest.fixture(scope="module")
def world_behind(gpu_ctx, scene_cache):
    """the same box with the quad that is seen from behind its vertex normals"""
    wd = World(gpu_ctx, scene_cache, back_seen_quad=True)
    yield wd
    wd.scene.close()


def test_the_back_seen_scene_is_seen_from_behind(world_behind):
    """at least 10 % of the camera hits have dot(normal, origin - position) < 0 in rtr_hit_surfaces' records, all of them objects with
    both lobes on: the scene cannot quietly stop covering the case the tests below are there for"""
    wd = world_behind
    raw = _np(wd.surf.raw)
    kind = _bits(raw)[:, 3]
    nov = np.sum(raw[:, 4:7].astype(np.float64) * (_np(wd.rays)[:, 0:3].astype(np.float64) - raw[:, 0:3]), axis=1)
    behind = (kind == A.SURFACE_OBJECT) & (nov < 0.0)
    print(f"{100.0 * behind.mean():.1f} % of the {len(raw)} camera hits are seen from behind the shading normal")
    assert behind.mean() >= 0.10
    assert (raw[behind, 11] == 0.5).all() and (raw[behind, 15] == 1.0).all() and (raw[behind, 6] > 0.99).all()


def test_the_exported_light_table(world):
    rec, first = world.rec, world.first
    assert rec.shape == (5, 16) and first.tolist() == [0, 2, 3]
    assert [int(l.numTriangles) for l in world.lights] == [2, 1, 2] and [int(l.isTwoSided) for l in world.lights] == [0, 1, 0]
    p0, p1, p2 = rec[:, 0:3].astype(np.float64), rec[:, 4:7].astype(np.float64), rec[:, 8:11].astype(np.float64)
    n = np.cross(p2 - p1, p0 - p1)
    area = 0.5 * np.linalg.norm(n, axis=1)
    assert np.allclose(rec[:, 3], area, rtol=1e-5) and np.allclose(rec[:, 7], 1.0 / (0.7 * area), rtol=1e-5)
    assert np.allclose(rec[:, 12:15], n / (2 * area)[:, None], atol=1e-5) and (rec[[0, 1, 3, 4], 13] < -0.99).all(), "the one-sided lights face down"
    assert np.allclose(p0[:, 1], 540.0, atol=1e-3)
    lib = world.scene.lib
    count = C.c_uint32(0)
    buf = np.full((4, 16), 7.0, np.float32)
    assert lib.rtr_scene_export_light_tris(world.scene.h, buf.ctypes.data_as(A.VP), 4, None, C.byref(count)) == -1
    assert count.value == 5 and (buf == 7.0).all()
    assert lib.rtr_last_error().decode() == "rtr_scene_export_light_tris: capacity 4 light triangles, 5 are needed"
    assert lib.rtr_scene_export_light_tris(world.scene.h, None, 9, None, C.byref(count)) == -1 and count.value == 5


# ---- 5. the pick side ----------------------------------------------------------------------------------------------------------------
def _raw_pick_weights(ctx, wd, off, n, p, pick, mis, seeds, slots, samples):
    """rtr_mis_pick_weights straight through the C ABI on hits off ... off + n of the frame, guard words behind both outputs"""
    out = torch.full((n * int(pick.numPicks) + 16,), GUARD, dtype=torch.int32, device="cuda")
    rec = torch.full((n * int(pick.numPicks) + 2, 8), GUARD, dtype=torch.int32, device="cuda") if samples else None
    sl = None if slots is None else _i32(slots)
    torch.cuda.synchronize()
    rc = ctx.lib.rtr_mis_pick_weights(ctx.h, wd.scene.h, A.VP(wd.rays.data_ptr() + 32 * off), A.VP(wd.hits.data_ptr() + 32 * off), n, C.byref(p), C.byref(pick),
                                      C.byref(mis), A.VP(seeds.data_ptr() + 4 * off),
                                      A.VP(sl.data_ptr()) if sl is not None else None, A.VP(out.data_ptr()), A.VP(rec.data_ptr()) if samples else None)
    assert rc == 0, ctx.lib.rtr_last_error().decode()
    P = int(pick.numPicks)
    o = _bits(out)
    assert (o[n * P:] == GUARD).all(), "written behind outWeights"
    if not samples:
        return o[:n * P].reshape(n, P), None
    r = _bits(rec)
    assert (r[n * P:] == GUARD).all(), "written behind outSamples"
    return o[:n * P].reshape(n, P), r[:n * P].reshape(n, P, 8)


def _fma32(a, b, c):
    """fma of float32 arrays through float64: the product is exact there, the sum is rounded to 53 bits and then to 24"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


@pytest.mark.parametrize("picks", [1, 2, 30])
@pytest.mark.parametrize("handed_in", [False, True])
def test_pick_weights_are_made_of_the_public_parts(gpu_ctx, world, picks, handed_in):
    _pick_weights_are_made_of_the_public_parts(gpu_ctx, world, picks, handed_in, SIZES)


@pytest.mark.parametrize("picks", [1, 2])
def test_pick_weights_are_made_of_the_public_parts_seen_from_behind(gpu_ctx, world_behind, picks):
    """the same on the frame whose middle is seen from behind the shading normal: bouncePdf is rtr_host_bounce_pdf there too"""
    _pick_weights_are_made_of_the_public_parts(gpu_ctx, world_behind, picks, False, [1, 65, W * H])


def _pick_weights_are_made_of_the_public_parts(gpu_ctx, wd, picks, handed_in, sizes):
    p, pick, mis = wd.params(), api.make_pick_params(picks, 2), api.make_mis_params(picks, 3, NS)
    tris, area_slots = 5, 5 * NS
    full = W * H
    slots_in = None
    if handed_in:
        rng = np.random.default_rng(picks)
        slots_in = rng.integers(0, area_slots, size=(full, picks), dtype=np.uint64).astype(np.uint32)
        slots_in[rng.random((full, picks)) < 0.1] = A.PICK_NONE
        slots_in[rng.random((full, picks)) < 0.1] = area_slots + 3
        slots_in[0, 0] = area_slots                                     # the first slot past the area slots
    k = np.arange(full, dtype=np.uint64)
    seeds = _i32((((k % W) * 733 + (k // W) * 1933) & 0xffffffff).astype(np.uint32))      # the pixels' own, explicit: a part of the frame keeps its seeds
    pr, used = api.light_rays_picked(wd.scene, wd.rays, wd.hits, p, pick, seeds=seeds, slots=None if slots_in is None else _i32(slots_in))
    pr, used = _np(pr).reshape(full, picks + 1, 8)[:, :picks], _bits(used).reshape(full, picks)
    if handed_in:
        assert (used == slots_in).all()
    kind = _bits(wd.surf.raw)[:, 3]
    assert (kind == A.SURFACE_OBJECT).sum() > 1000 and (kind != A.SURFACE_OBJECT).sum() > 10, "the frame has objects and other hits"
    default = np.float32(tris) / np.float32(picks)
    for n in sizes:
        off = 0 if n == full else 32 * W + 5          # the parts start in the middle of the frame, where the box is
        part = slice(off, off + n)
        w, smp = _raw_pick_weights(gpu_ctx, wd, off, n, p, pick, mis, seeds, None if slots_in is None else slots_in[part], True)
        w2, none = _raw_pick_weights(gpu_ctx, wd, off, n, p, pick, mis, seeds, None if slots_in is None else slots_in[part], False)
        assert none is None and (w == w2).all(), "the weights depend on whether the samples are asked for"
        s = smp.view(np.float32)
        ray = pr[part]
        has_ray = _bits(ray).any(axis=2)
        # a pick without a ray, a hit that is not an object: a zero weight and a zero record
        assert not has_ray[kind[part] != A.SURFACE_OBJECT].any()
        assert not w[~has_ray].any() and not smp[~has_ray].any()
        if n == full:
            assert has_ray.sum() > 500 * picks and (~has_ray[kind == A.SURFACE_OBJECT]).any()
        k, q = np.nonzero(has_ray)
        assert len(k) > 0 or (n == 1 and picks == 1), "no pick of this part of the frame sends a ray"
        if len(k) == 0:
            continue
        rec = s[k, q]
        t = used[off + k, q] // NS
        d = ray[k, q, 4:7]
        assert (_bits(rec[:, 4] - np.float32(0.5)) == _bits(ray[k, q, 7])).all(), "dist - 0.5 is not the picked ray's tmax"
        want_pb = api.host_bounce_pdf(_np(wd.rays)[off + k], _np(wd.surf.raw)[off + k], d)
        assert (_bits(rec[:, 1]) == _bits(want_pb)).all(), "bouncePdf is not rtr_host_bounce_pdf of the hit's surface and the picked direction"
        assert (_bits(rec[:, 5]) == _bits(wd.rec[t, 3])).all() and (smp[k, q, 6] == t).all() and not smp[k, q, 7].any(), "area, lightTri"
        # cosLight = rtr_dot(n_t, -dir) = fma(nz, -dz, fma(ny, -dy, nx * -dx)).  numpy has no fused multiply-add: the float64 stand-in
        # rounds each fma twice (53 bits, then 24), which now and then lands on the neighbouring float: within 4 ulp, and the share of
        # exact matches is printed
        nt = wd.rec[t, 12:15]
        cos = _fma32(nt[:, 2], -d[:, 2], _fma32(nt[:, 1], -d[:, 1], nt[:, 0] * -d[:, 0]))
        ulps = np.abs(rec[:, 3].astype(np.float64) - cos.astype(np.float64)) / np.spacing(np.abs(cos)).astype(np.float64)
        assert ulps.max() <= 4.0, f"cosLight is {ulps.max()} ulp from dot(n_t, -dir)"
        want, _ = api.host_mis_weights(rec[:, 1], rec[:, 4], rec[:, 3], rec[:, 5], tris, picks)
        assert (_bits(rec[:, 0]) == _bits(want[:, 0])).all() and (_bits(rec[:, 2]) == _bits(want[:, 2])).all(), "lightPdf, wPick are not rtr_host_mis_weights' of the record"
        assert (w[k, q] == _bits(default * rec[:, 2])).all(), "the weight is not (float)Ttot / (float)P * wPick"
        assert np.isfinite(s[..., :6]).all()
        if n == full:
            print(f"P {picks} handed in {handed_in}: {len(k)} picks with a ray, wPick {rec[:, 2].min():.3f} ... {rec[:, 2].max():.3f}, cosLight exact for "
                  f"{100.0 * (ulps == 0).mean():.2f} %")
            assert rec[:, 2].min() < 0.999 and rec[:, 2].max() > 0.5


def test_mis_pick_weights_wrapper_and_refusals(gpu_ctx, world):
    wd = world
    p, pick, mis = wd.params(), api.make_pick_params(2, 1), api.make_mis_params(2, 3, NS)
    lr, slots = api.light_rays_picked(wd.scene, wd.rays, wd.hits, p, pick)
    w, smp = api.mis_pick_weights(wd.scene, wd.rays, wd.hits, p, pick, mis, slots, samples=True)
    assert tuple(w.shape) == (W * H, 2) and tuple(smp.shape) == (W * H, 2, 8)
    drawn = api.mis_pick_weights(wd.scene, wd.rays, wd.hits, p, pick, mis, None)
    assert torch.equal(w, drawn), "slots=None does not draw the slots light_rays_picked draws"
    wn = api.mis_pick_weights(wd.scene, _np(wd.rays), _np(wd.hits), p, pick, mis, _np(slots))
    assert isinstance(wn, np.ndarray) and (_bits(wn) == _bits(w)).all()
    diffuse = api.mis_pick_weights(wd.scene, wd.rays, wd.hits, p, pick, api.make_mis_params(2, 3, NS, lobes=A.BOUNCE_DIFFUSE), slots)
    assert not torch.equal(diffuse, w)
    with pytest.raises(api.RtrError, match="rtr_mis_pick_weights: numAreaLights 4 > scene lights 3"):
        api.mis_pick_weights(wd.scene, wd.rays, wd.hits, wd.params(4), pick, api.make_mis_params(2, 4, NS), slots)
    # the weights go where shade_hits_picked and direct_light take them
    occ = api.trace_rays(wd.scene, lr, any_hit=True).occluded
    a = api.shade_hits_picked(wd.scene, wd.rays, wd.hits, p, pick, slots, occ, weights=w)
    b = api.direct_light(wd.scene, wd.rays, wd.hits, p, picks=2, pick_depth=1, pick_weights=w)
    c = api.direct_light(wd.scene, wd.rays, wd.hits, p, picks=2, pick_depth=1, pick_weights=w, max_ray_bytes=1000 * 3 * 32)
    assert (_bits(a.raw) == _bits(b.raw)).all() and (_bits(a.raw) == _bits(c.raw)).all()
    assert not (_bits(a.raw) == _bits(api.direct_light(wd.scene, wd.rays, wd.hits, p, picks=2, pick_depth=1).raw)).all()


# ---- 6. the bounce side --------------------------------------------------------------------------------------------------------------
def _raw_emitter(ctx, wd, rays, hits, surf, bounce, n, mis):
    out = torch.full((n + 2, 8), GUARD, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = ctx.lib.rtr_emitter_hits(ctx.h, wd.scene.h, A.VP(rays.data_ptr()), A.VP(hits.data_ptr()), A.VP(surf.data_ptr()), A.VP(bounce.data_ptr()), n, C.byref(mis),
                                  A.VP(out.data_ptr()))
    assert rc == 0, ctx.lib.rtr_last_error().decode()
    o = _bits(out)
    assert (o[n:] == GUARD).all(), "written behind out"
    return o[:n]


def _interior_points(rec, m=64):
    """m fixed points of the triangle, each at least 0.05 (barycentric) from every edge"""
    k = np.arange(m)
    u = 0.05 + 0.85 * ((k * 0.6180339887) % 1.0)
    v = 0.05 + 0.85 * ((k * 0.7548776662) % 1.0)
    fold = u + v > 0.95
    u, v = np.where(fold, 0.95 - u + 0.05, u), np.where(fold, 0.95 - v + 0.05, v)
    u, v = np.clip(u, 0.05, 0.9), np.clip(v, 0.05, 0.9)
    scale = np.where(u + v > 0.95, 0.95 / (u + v), 1.0)
    u, v = u * scale, v * scale
    p0, p1, p2 = rec[0:3].astype(np.float64), rec[4:7].astype(np.float64), rec[8:11].astype(np.float64)
    return p0 + (p1 - p0) * u[:, None] + (p2 - p0) * v[:, None]


def _constructed(wd, case):
    """hand-made object surfaces under (or above) each light and rays from them to 64 points of each light triangle ->
    (rays, the same rays before any word was spoilt, surfaces, bounce records, expected light, expected triangle) as numpy"""
    rays, clean, surf, bnc, want_l, want_t = [], [], [], [], [], []
    for l, light in enumerate(wd.lights):
        for ti in range(int(light.numTriangles)):
            t = int(wd.first[l]) + ti
            pts = _interior_points(wd.rec[t])
            m = len(pts)
            centre = wd.rec[t, [0, 4, 8]].mean(), wd.rec[t, [2, 6, 10]].mean()
            if case == "behind":         # above the lights, looking down at their backs
                x = np.stack([np.full(m, centre[0]) + np.linspace(-20, 20, m), np.full(m, 546.0), np.full(m, centre[1]) + np.linspace(15, -15, m)], axis=1)
                N = np.tile([0.0, -1.0, 0.0], (m, 1))
            elif case == "grazing":      # 3 below the lights' plane and far to the side: |cosLight| of about 0.01
                x = np.stack([np.full(m, 30.0 if centre[0] > 278.0 else 526.0), np.full(m, 537.0), np.linspace(200.0, 360.0, m)], axis=1)
                N = np.tile([0.0, 1.0, 0.0], (m, 1))
            else:
                x = np.stack([np.full(m, centre[0]) + np.linspace(-60, 60, m), np.linspace(360.0, 500.0, m), np.full(m, centre[1]) + np.linspace(40, -40, m)], axis=1)
                N = np.tile([0.0, 1.0, 0.0], (m, 1))
            s = np.zeros((m, 20), np.float32)
            s[:, 0:3], s[:, 4:7], s[:, 8:11] = x, N, N
            s.view(np.uint32)[:, 3] = A.SURFACE_OBJECT
            s[:, 12:15], s[:, 11], s[:, 15] = (0.7, 0.6, 0.5), 0.25, 0.35
            o = s[:, 0:3].astype(np.float64) + 0.01 * N
            d = pts - o
            d /= np.linalg.norm(d, axis=1)[:, None]
            r = np.zeros((m, 8), np.float32)
            r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, 0.001, d * (1.0 + 0.5 * (np.arange(m) % 3))[:, None], 10000.0       # not all normalised
            view = np.zeros((m, 8), np.float32)                         # the ray that found the vertex: from along its normal, tilted
            view[:, 0:3] = s[:, 0:3] + (N + [0.3, 0.0, 0.2]) * 50.0
            b = np.zeros((m, 8), np.float32)
            b[:, 3] = api.host_bounce_pdf(view, s, d.astype(np.float32))
            b[:, 0:3] = 0.5
            clean.append(r.copy())
            if case == "pb0":
                b[::2, 3] = 0.0
            if case == "nan":
                s[0::4, 5] = np.nan
                b[1::4, 3] = np.nan
                r[2::4, 0] = np.inf
            rays.append(r); surf.append(s); bnc.append(b)
            want_l += [l] * m
            want_t += [ti] * m
    return np.concatenate(rays), np.concatenate(clean), np.concatenate(surf), np.concatenate(bnc), np.array(want_l), np.array(want_t)


@pytest.mark.parametrize("case", ["below", "grazing", "behind", "unsampled", "pb0", "nan"])
def test_emitter_hits_on_constructed_rays(gpu_ctx, world, case):
    wd = world
    rays, clean, surf, bnc, want_l, want_t = _constructed(wd, case)
    area_lights = 2 if case == "unsampled" else 3
    mis = api.make_mis_params(2, area_lights, NS)
    dr, ds, db = _f32(rays), _f32(surf), _f32(bnc)
    hits = api.trace_rays(wd.scene, _f32(clean)).hits                  # the query sees the rays as constructed; a record may hold a spoilt word
    hw = _bits(hits)
    # by construction every ray ends on its light: no case drops out silently
    assert (hw[:, 3] == want_l).all() and (hw[:, 4] == want_t).all(), f"{((hw[:, 3] != want_l) | (hw[:, 4] != want_t)).sum()} rays do not end on their light triangle"
    n = len(rays)
    assert n == 5 * 64
    got = _raw_emitter(gpu_ctx, wd, dr, hits, ds, db, n, mis)
    want = api.host_emitter_hits(rays, _np(hits), surf, bnc, wd.rec, wd.first, wd.lights, mis)
    assert (got == _bits(want.raw)).all(), f"{(got != _bits(want.raw)).any(axis=1).sum()} of {n} records differ from rtr_host_emitter_hits'"
    g = got.view(np.float32)
    assert np.isfinite(g[:, :6]).all()
    counts = got[:, 7] == A.SURFACE_LIGHT
    zero = ~got.any(axis=1)
    assert (counts | zero).all()
    two_sided = want_l == 1
    if case in ("below", "grazing", "unsampled"):
        assert counts.all() and (g[:, 0:3] > 0).all() and (got[:, 6] == wd.first[want_l] + want_t).all()
        sampled = want_l < area_lights
        assert ((g[sampled, 3] > 0) & (g[sampled, 3] < 1)).all() and (g[sampled, 4] > 0).all()
        assert (g[~sampled, 3] == 1.0).all() and (g[~sampled, 4] == 0.0).all(), "a light nobody picks from is the bounce's alone"
        assert (~sampled).sum() == (128 if case == "unsampled" else 0)
    if case == "grazing":
        cos = np.abs(np.sum(wd.rec[wd.first[want_l] + want_t, 12:15] * (rays[:, 4:7] / np.linalg.norm(rays[:, 4:7], axis=1)[:, None]), axis=1))
        assert cos.max() < 0.03, "the rays do not graze the lights"
    if case == "behind":
        assert zero[~two_sided].all() and counts[two_sided].all(), "a one-sided light counts from behind, or a two-sided one does not"
    if case == "pb0":
        assert zero[0::2].all() and counts[1::2].all()
    if case == "nan":
        k = np.arange(n)
        assert zero[k % 4 != 3].all() and counts[k % 4 == 3].all()
    dev = api.emitter_hits(wd.scene, dr, hits, ds, db, mis)
    assert (_bits(dev.raw) == got).all() and (_bits(dev.kind) == got[:, 7]).all() and (_bits(dev.w_bounce) == got[:, 3]).all()


def test_emitter_hits_on_the_bounce_rays_of_a_frame(gpu_ctx, world):
    _emitter_hits_on_the_bounce_rays_of_a_frame(gpu_ctx, world)


def test_emitter_hits_on_the_bounce_rays_of_a_frame_seen_from_behind(gpu_ctx, world_behind):
    _emitter_hits_on_the_bounce_rays_of_a_frame(gpu_ctx, world_behind)


def test_bounce_rays_of_a_frame_seen_from_behind_equal_the_hosts(gpu_ctx, world_behind):
    """rtr_bounce_rays on the camera hits of the back-seen frame: rays and RtrBounce words equal rtr_host_bounce_rays', for every lobe
    mask, and the quad's hits have live records that leave on the normal's side"""
    wd = world_behind
    raw = _np(wd.surf.raw)
    behind = np.sum(raw[:, 4:7].astype(np.float64) * (_np(wd.rays)[:, 0:3].astype(np.float64) - raw[:, 0:3]), axis=1) < 0.0
    for lobes in (A.BOUNCE_DIFFUSE, A.BOUNCE_SPECULAR, A.BOUNCE_DIFFUSE | A.BOUNCE_SPECULAR):
        p = api.make_bounce_params(frame=wd.frame, depth=0, width=W, spp=1, lobes=lobes)
        dev = api.bounce_rays(gpu_ctx, wd.rays, wd.surf, p)
        want = api.host_bounce_rays(_np(wd.rays), raw, p, None)
        assert (_bits(dev.rays) == _bits(want.rays)).all() and (_bits(dev.raw) == _bits(want.raw)).all(), f"lobes {lobes}: the device differs from the host"
        live = behind & (want.lobe != 0)
        # (the specular lobe alone is nearly always dead at a view this far behind the normal: its half vectors are on the far side)
        assert live.sum() > (100 if lobes & A.BOUNCE_DIFFUSE else 0) and (np.sum(want.rays[live, 4:7] * raw[live, 4:7], axis=1) > 0).all()
        pdf = api.host_bounce_pdf(_np(wd.rays)[live], raw[live], want.rays[live, 4:7], lobes)
        assert (_bits(pdf) == _bits(want.pdf[live])).all(), "rtr_host_bounce_pdf of the drawn direction is not RtrBounce::pdf"


def _emitter_hits_on_the_bounce_rays_of_a_frame(gpu_ctx, wd):
    mis = api.make_mis_params(1, 3, NS)
    b = api.bounce_rays(gpu_ctx, wd.rays, wd.surf, api.make_bounce_params(frame=wd.frame, depth=0, width=W, spp=1))
    hits = api.trace_rays(wd.scene, b.rays).hits
    dead = ~_bits(b.rays).any(axis=1)
    met = _bits(hits)[:, 3] < 3
    assert dead.sum() > 10 and met.sum() > 20, "the frame has dead paths and bounce rays that meet a light"
    for n in SIZES:
        got = _raw_emitter(gpu_ctx, wd, b.rays, hits, wd.surf.raw, b.raw, n, mis)
        want = api.host_emitter_hits(_np(b.rays)[:n], _np(hits)[:n], _np(wd.surf.raw)[:n], _np(b.raw)[:n], wd.rec, wd.first, wd.lights, mis)
        assert (got == _bits(want.raw)).all(), f"{n} rays: {(got != _bits(want.raw)).any(axis=1).sum()} records differ from rtr_host_emitter_hits'"
        assert not got[dead[:n]].any() and not got[~met[:n]].any()
        assert np.isfinite(got.view(np.float32)[:, :6]).all()
    counts = got[:, 7] == A.SURFACE_LIGHT
    assert counts.sum() > 10 and counts.sum() <= met.sum()
    numpy_in = api.emitter_hits(wd.scene, _np(b.rays), _np(hits), _np(wd.surf.raw), _np(b.raw), mis)
    assert isinstance(numpy_in.raw, np.ndarray) and (_bits(numpy_in.raw) == got).all()
    with pytest.raises(api.RtrError, match="rtr_emitter_hits: numAreaLights 4 > scene lights 3"):
        api.emitter_hits(wd.scene, b.rays, hits, wd.surf, b, api.make_mis_params(1, 4, NS))


# ---- 7. api.path_trace_mis -----------------------------------------------------------------------------------------------------------
def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _written_out(scene, ctx, rays, lp, bounces, picks=None, pick_from=1):
    """path_trace's (picks None) and path_trace_picked's loop from the public parts -> per_depth"""
    n = rays.shape[0]
    k = torch.arange(n, device=rays.device, dtype=torch.int64) // int(lp.spp)
    base = api._wrap32((k % int(lp.width)) * 733 + (k // int(lp.width)) * 1933)
    T, r, out = torch.ones((n, 3), dtype=torch.float32, device=rays.device), rays, []
    for d in range(bounces + 1):
        q = api.trace_rays(scene, r)
        sd = None if d == 0 else api._wrap32(base.to(torch.int64) + d * api.PATH_SEED_STEP)
        kw = dict(picks=picks, pick_depth=d) if picks is not None and d >= pick_from else {}
        lit = api.direct_light(scene, r, q, lp, seeds=sd, **kw)
        rad = lit.shadowed
        if d >= 1:
            rad = torch.where((lit.kind == A.SURFACE_LIGHT).unsqueeze(1), torch.zeros_like(rad), rad)
        out.append(T * rad)
        if d == bounces:
            break
        b = api.bounce_rays(ctx, r, api.hit_surfaces(scene, r, q), api.make_bounce_params(frame=lp.frame, depth=d, width=lp.width, spp=lp.spp))
        T, r = T * b.weight, b.rays
    return out


def test_path_trace_mis_against_the_other_loops(gpu_ctx, world):
    wd = world
    lp = api.make_light_params(3, NS, 4, W, 1)
    # without bounces there is no MIS vertex: path_trace_picked's bytes
    for pick_from in (0, 1):
        a = api.path_trace_mis(wd.scene, wd.rays, lp, 0, light_picks=2, pick_from=pick_from)
        b = api.path_trace_picked(wd.scene, wd.rays, lp, 0, light_picks=2, pick_from=pick_from)
        assert torch.equal(a.radiance, b.radiance) and len(a.per_depth) == 1
    # path_trace and path_trace_picked are the loops they were
    plain, picked = api.path_trace(wd.scene, wd.rays, lp, 2), api.path_trace_picked(wd.scene, wd.rays, lp, 2, light_picks=1)
    for got, want in ((plain, _written_out(wd.scene, gpu_ctx, wd.rays, lp, 2)), (picked, _written_out(wd.scene, gpu_ctx, wd.rays, lp, 2, picks=1))):
        assert len(got.per_depth) == 3 and all(_same(g, w) for g, w in zip(got.per_depth, want))
    # the MIS loop: the camera vertex keeps the full loops (pick_from=1), vertex 1 is a MIS vertex, vertex 2 counts the lights its ray meets
    mis = api.path_trace_mis(wd.scene, wd.rays, lp, 2, light_picks=1)
    assert _same(mis.per_depth[0], picked.per_depth[0]) and torch.isfinite(mis.radiance).all()
    assert not _same(mis.per_depth[1], picked.per_depth[1]) and not _same(mis.per_depth[2], picked.per_depth[2])
    q1 = api.trace_rays(wd.scene, api.bounce_rays(gpu_ctx, wd.rays, wd.surf, api.make_bounce_params(frame=4, depth=0, width=W, spp=1)).rays).hits
    on_light = torch.from_numpy((_bits(q1)[:, 3] < 3)).cuda()
    assert on_light.sum() > 20 and not mis.per_depth[1][on_light].any(), "vertex 0 took the full loops: its bounce ray counts no light"
    both = api.path_trace_mis(wd.scene, wd.rays, lp, 1, light_picks=1, pick_from=0)
    assert (both.per_depth[1][on_light] != 0).any(), "with pick_from=0 a bounce ray that meets a light counts"
    # compaction without roulette changes nothing
    for bounces, pick_from in ((3, 0), (3, 1)):
        a = api.path_trace_mis(wd.scene, wd.rays, lp, bounces, light_picks=2, pick_from=pick_from)
        b = api.path_trace_mis(wd.scene, wd.rays, lp, bounces, light_picks=2, pick_from=pick_from, compact=True)
        assert torch.equal(a.radiance, b.radiance) and all(torch.equal(x, y) for x, y in zip(a.per_depth, b.per_depth))
        assert b.live[0] == W * H and 0 < b.live[3] < b.live[1] < b.live[0]
    r = api.path_trace_mis(wd.scene, wd.rays, lp, 3, light_picks=1, pick_from=0, compact=True, roulette_from=1)
    assert torch.isfinite(r.radiance).all() and r.live[3] < b.live[3]


def _paired_means(gpu_ctx, s):
    """-> (difference of the image sums MIS - picked per frame over frames 0 ... 63, printed summary)"""
    scene = api.Scene(gpu_ctx, s.desc)
    rays = api.camera_rays(gpu_ctx, s.camera, 32, 32, 1)
    sums = {"picked": [], "mis": []}
    acc = {k: [torch.zeros((32 * 32, 3), dtype=torch.float64, device="cuda") for _ in range(2)] for k in sums}
    for f in range(64):
        lp = api.make_light_params(3, NS, f, 32, 1)
        for name, fn in (("picked", api.path_trace_picked), ("mis", api.path_trace_mis)):
            rad = fn(scene, rays, lp, 1, light_picks=1, pick_from=0).radiance.double()
            sums[name].append(float(rad.sum()))
            acc[name][0] += rad
            acc[name][1] += rad * rad
    scene.close()
    picked, mis = np.array(sums["picked"]), np.array(sums["mis"])
    assert np.isfinite(picked).all() and np.isfinite(mis).all() and picked.mean() > 0
    diff = mis - picked
    se = diff.std(ddof=1) / np.sqrt(64)
    dev = diff.mean() / se
    var = {k: float(((acc[k][1] - acc[k][0] ** 2 / 64) / 63).mean()) for k in acc}
    print(f"image sum of radiance: picked {picked.mean():.4f}, MIS {mis.mean():.4f}, difference {diff.mean():+.4f} +- {se:.4f}: {dev:+.2f} standard errors; "
          f"variance of the sum picked {picked.var(ddof=1):.4f}, MIS {mis.var(ddof=1):.4f}; mean per-pixel variance picked {var['picked']:.5f}, MIS {var['mis']:.5f}")
    return dev


def test_path_trace_mis_has_the_picked_loops_mean(gpu_ctx, scene_cache):
    """bounces=1, pick_from=0, light_picks=1 on a 32x32 frame over frames 0 ... 63: the image sum of radiance has path_trace_picked's
    mean within 5 standard errors of the difference (the two take the same picks and bounce directions in a frame, so the difference is
    taken per frame).  The variances of the image sum and the mean per-pixel variance are printed, not asserted."""
    assert abs(_paired_means(gpu_ctx, _box_scene(scene_cache, THREE_LIGHTS, 32, 32))) <= 5.0


def test_path_trace_mis_has_the_picked_loops_mean_seen_from_behind(gpu_ctx, scene_cache):
    """The same with a quad that is seen from behind its vertex normals (roughness 1, metallic 0.5) and fills the frame: 70 % of the
    camera hits are on it.  MIS weighs by the bounce's density; where that is not the density the directions are drawn from, its mean
    leaves the picked loop's.  Read +0.30 standard errors here (+1.9 +- 6.4 of 4426), and +6.46 (+50.1 +- 7.8 of 4855, 1 % high) with
    the build before rtr_bounce_sample dropped half vectors on the far side of the view.  With the quad over a fifth of the frame, as the
    other tests of this file have it, the rest of the box carries the noise (+- 92 of 6651) and the two builds read -0.18 and -0.05: the
    quad had to cover the frame for the test to tell them apart."""
    assert abs(_paired_means(gpu_ctx, _box_scene(scene_cache, THREE_LIGHTS, 32, 32, back_seen_quad="full"))) <= 5.0
