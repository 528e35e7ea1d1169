"""Hit surfaces (rtr_hit_surfaces) on the device.  The kernel runs the renderer's own surface fetch for caller hits, so:
  * against an independent float64 restatement (tests/witness.py's scene loader: vertices, transforms, texture sampler), fed the SAME
    hits, every field is within 1e-5 of the operands' magnitude (+ 1e-6), and kind / objectIndex are exact;
  * the renderer's normal and position images are exactly write_pixel's packing of `normal` and `position` at every object pixel;
  * moved instances, misses, light hits, ids out of range, and the plumbing (empty calls, bad pointers, streams, numpy)."""

import numpy as np
import pytest
import torch

from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api, scenes
from witness import Witness, normalize

pytestmark = pytest.mark.gpu

MISS = 0xffffffff
EPS32 = 2.0 ** -24
RTOL, ATOL = 1e-5, 1e-6


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def random_rays(lo, hi, n, seed):
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    o = lo + (hi - lo) * rng.uniform(-0.2, 1.2, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, 0.001, d, 10000.0
    return r


def tri_counts(w):
    """what a hit's primitiveId may be, per customIndex"""
    return np.array([w.lights[c].numTriangles if c < w.numLights else w.meshes[w.instances[c].meshIndex].indexCount // 3
                     for c in range(len(w.instances))], np.int64)


def _tex_slack(img, coord_err):
    """how far an fp32 bilinear lookup may sit from the float64 one when its coordinate is off by coord_err: fma(frac(u), W, -0.5)
    rounds once (<= W * 2^-24), plus coord_err texels' worth of W; neighbouring texels differ by at most 1"""
    H, W = img.shape[:2]
    return 2.0 * (EPS32 + coord_err) * max(W, H) + 8 * EPS32


class Expect:
    """the witness's surface for each hit: values and, per field, the bound the fp32 result must keep"""

    def __init__(self, w, rays, hits):
        n = len(rays)
        self.n = n
        cu = hits[:, 3].astype(np.int64) & 0xffffffff
        pr = hits[:, 4].astype(np.int64) & 0xffffffff
        u = hits[:, 1].view(np.float32).astype(np.float64)
        v = hits[:, 2].view(np.float32).astype(np.float64)
        d = rays[:, 4:7].astype(np.float64)
        counts = tri_counts(w)
        ninst = len(counts)
        valid = (cu < ninst) & (pr < counts[np.minimum(cu, max(ninst - 1, 0))]) if ninst else np.zeros(n, bool)
        self.kind = np.full(n, A.SURFACE_INVALID, np.int64)
        self.kind[cu == MISS] = A.SURFACE_MISS
        self.kind[valid & (cu < w.numLights)] = A.SURFACE_LIGHT
        self.kind[valid & (cu >= w.numLights)] = A.SURFACE_OBJECT
        self.index = np.full(n, MISS, np.int64)
        self.index[self.kind == A.SURFACE_LIGHT] = cu[self.kind == A.SURFACE_LIGHT]
        self.index[self.kind == A.SURFACE_OBJECT] = cu[self.kind == A.SURFACE_OBJECT] - w.numLights
        z3 = lambda: np.zeros((n, 3))                                   # noqa: E731
        self.val = {"position": z3(), "normal": z3(), "geom_normal": z3(), "color": z3(), "uv": np.zeros((n, 2)),
                    "roughness": np.zeros(n), "metallic": np.zeros(n)}
        self.bound = {k: np.full(n, ATOL) for k in self.val}
        self.tex_uv = {}
        b0, b1, b2 = 1.0 - u - v, u, v
        # misses: the sky in the ray's direction (miss.rmiss:15-27)
        m = np.nonzero(self.kind == A.SURFACE_MISS)[0]
        if len(m):
            if w.hdri is not None:
                dd = normalize(d[m])
                hu = np.arctan2(dd[:, 2], dd[:, 0]) / (2 * 3.14159265) + 0.5
                hv = 1.0 - np.arccos(np.clip(dd[:, 1], -1, 1)) / 3.14159265
                sky = np.power(w.sample(w.hdri, hu, hv)[:, :3], 2.2)
                slack = 2.2 * _tex_slack(w.hdri, 1e-6)                   # rtr_atan2 <= 6e-7 rad = 1e-7 turn, rtr_acos <= 7e-7 rad = 2.3e-7 of pi (test_math_contract.py): inside 1e-6
            else:
                sky, slack = np.broadcast_to(w.sky, (len(m), 3)), 0.0
            self.val["color"][m] = sky
            self.bound["color"][m] = RTOL * np.abs(sky).max(1) + ATOL + slack
        # light hits: the light's colour, the hit on its world-space triangle
        for li in np.unique(cu[self.kind == A.SURFACE_LIGHT]):
            L = w.lights[li]
            sel = np.nonzero((self.kind == A.SURFACE_LIGHT) & (cu == li))[0]
            T = np.array(L.transform[:], np.float64).reshape(4, 4).T
            j = w.idx[(L.indexOffset + 3 * pr[sel])[:, None] + np.arange(3)].astype(np.int64) + L.vertexOffset
            P = w.verts[j, 0:3] @ T[:3, :3].T + T[:3, 3]                              # (s, 3 corners, 3)
            self.val["color"][sel] = np.array(L.color[:3], np.float64)
            self.val["position"][sel] = P[:, 0] * b0[sel, None] + P[:, 1] * b1[sel, None] + P[:, 2] * b2[sel, None]
            ln = np.cross(P[:, 2] - P[:, 1], P[:, 0] - P[:, 1])
            self.val["normal"][sel] = self.val["geom_normal"][sel] = normalize(ln)
            pmax = np.linalg.norm(P, axis=2).max(1)
            self.bound["position"][sel] = RTOL * pmax + ATOL
            emax = np.maximum(np.linalg.norm(P[:, 2] - P[:, 1], axis=1), np.linalg.norm(P[:, 0] - P[:, 1], axis=1))
            cond = 2 * pmax * emax / np.linalg.norm(ln, axis=1)
            self.bound["normal"][sel] = self.bound["geom_normal"][sel] = RTOL * cond + ATOL
        # objects: closesthit.rchit:53-106
        for ci in np.unique(cu[self.kind == A.SURFACE_OBJECT]):
            sel = np.nonzero((self.kind == A.SURFACE_OBJECT) & (cu == ci))[0]
            oi = w.objects[ci - w.numLights]
            tri = w.idx[(oi.indexOffset + 3 * pr[sel])[:, None] + np.arange(3)].astype(np.int64) + oi.vertexOffset
            vv = w.verts[tri]                                                            # (s, 3, 12)
            wt = np.stack([b0[sel], b1[sel], b2[sel]], 1)[:, :, None]
            M, N = w.xform[ci], w.nmat[ci]
            condN = np.linalg.cond(N)
            lp = np.sum(vv[:, :, 0:3] * wt, 1)
            self.val["position"][sel] = lp @ M[:, :3].T + M[:, 3]
            corners = vv[:, :, 0:3] @ np.abs(M[:, :3]).T + np.abs(M[:, 3])
            self.bound["position"][sel] = RTOL * np.abs(corners).max((1, 2)) * 3 + ATOL
            p0, p1, p2 = vv[:, 0, 0:3], vv[:, 1, 0:3], vv[:, 2, 0:3]
            g = np.cross(p1 - p0, p2 - p0)
            gn = normalize(normalize(g) @ N.T)
            pmax = np.linalg.norm(vv[:, :, 0:3], axis=2).max(1)
            emax = np.maximum(np.linalg.norm(p1 - p0, axis=1), np.linalg.norm(p2 - p0, axis=1))
            condG = (2 * pmax * emax / np.linalg.norm(g, axis=1)) * condN
            self.val["geom_normal"][sel] = gn
            self.bound["geom_normal"][sel] = RTOL * condG + ATOL
            ns = np.sum(vv[:, :, 4:7] * wt, 1)
            zero = np.sum(ns * ns, 1) <= 0
            with np.errstate(invalid="ignore", divide="ignore"):
                nn = normalize(normalize(ns) @ N.T)
                condS = np.sum(np.abs(wt[:, :, 0]) * np.linalg.norm(vv[:, :, 4:7], axis=2), 1) / np.linalg.norm(ns, axis=1) * condN
            nn = np.where(zero[:, None], gn, nn)
            flip = zero & (np.sum(nn * d[sel], 1) > 0)
            self.val["normal"][sel] = np.where(flip[:, None], -nn, nn)
            self.bound["normal"][sel] = RTOL * np.where(zero, condG, condS) + ATOL
            uv = np.sum(vv[:, :, 8:10] * wt, 1)
            self.val["uv"][sel] = uv
            self.bound["uv"][sel] = RTOL * np.sum(np.abs(wt[:, :, 0])[:, :, None] * np.abs(vv[:, :, 8:10]), 1).max(1) + ATOL
            col = np.broadcast_to(np.array(oi.color[:3], np.float64), (len(sel), 3))
            rough, metal = np.full(len(sel), oi.specular, np.float64), np.full(len(sel), oi.metallic, np.float64)
            # the maps are read at the kernel's own uv (checked above against the witness's): what is compared is the sampler, not
            # the fp32 rounding of uv, which a texture magnifies W-fold
            self.tex_uv[ci] = (sel, oi)
            self.val["color"][sel] = np.power(col, 2.2)
            self.val["roughness"][sel] = 1.0 - rough
            self.val["metallic"][sel] = metal
            for k in ("color", "roughness", "metallic"):
                self.bound[k][sel] = RTOL * np.abs(self.val[k][sel]).reshape(len(sel), -1).max(1) + ATOL
        self._w = w

    def resample_maps(self, got_uv):
        """colour / specular / metallic maps sampled in float64 at the kernel's uv"""
        w = self._w
        for ci, (sel, oi) in self.tex_uv.items():
            uu, vv = got_uv[sel, 0].astype(np.float64), got_uv[sel, 1].astype(np.float64)
            maps = (("color", oi.usesColorMap, oi.colorIndex), ("roughness", oi.usesSpecularMap, oi.specularIndex),
                    ("metallic", oi.usesMetallicMap, oi.metallicIndex))
            for field, uses, ti in maps:
                if not uses:
                    continue
                img = w.textures[ti]
                s = w.sample(img, uu, vv)
                if field == "color":
                    val, slack = np.power(s[:, :3], 2.2), 2.2 * _tex_slack(img, 0.0)
                elif field == "roughness":
                    val, slack = 1.0 - s[:, 0], _tex_slack(img, 0.0)
                else:
                    val, slack = s[:, 0], _tex_slack(img, 0.0)
                self.val[field][sel] = val
                self.bound[field][sel] = RTOL * np.abs(val).reshape(len(sel), -1).max(1) + ATOL + slack


def assert_surfaces(res, exp, what):
    kind, index = _np(res.kind).astype(np.int64), _np(res.object_index).astype(np.int64) & 0xffffffff
    bad = (kind != exp.kind) | (index != exp.index)
    if bad.any():
        k = np.nonzero(bad)[0][:5]
        raise AssertionError(f"{what}: {int(bad.sum())} kinds / indices differ; first {k.tolist()}: gpu {kind[k].tolist()} {index[k].tolist()} "
                             f"expected {exp.kind[k].tolist()} {exp.index[k].tolist()}")
    exp.resample_maps(_np(res.uv))
    for f in ("position", "normal", "geom_normal", "color", "uv", "roughness", "metallic"):
        g = _np(getattr(res, f)).astype(np.float64).reshape(exp.n, -1)
        e = exp.val[f].reshape(exp.n, -1)
        err = np.abs(g - e).max(1)
        bad = ~(err <= exp.bound[f])
        if bad.any():
            k = np.nonzero(bad)[0][:5]
            raise AssertionError(f"{what}: {int(bad.sum())} of {exp.n} hits differ in {f}; first {k.tolist()}: kind {exp.kind[k].tolist()} "
                                 f"gpu {g[k].tolist()} expected {e[k].tolist()} bound {exp.bound[f][k].tolist()}")
    raw = _np(res.raw).view(np.uint32)
    assert (raw[:, 18:20] == 0).all(), f"{what}: reserved words"
    off = (exp.kind == A.SURFACE_MISS) | (exp.kind == A.SURFACE_INVALID)
    assert (raw[off][:, [0, 1, 2, 4, 5, 6, 8, 9, 10, 11, 15, 16, 17]] == 0).all(), f"{what}: geometry of a miss / invalid hit is not 0"
    assert (raw[exp.kind == A.SURFACE_INVALID][:, 12:15] == 0).all(), f"{what}: colour of an invalid hit is not 0"


def _setup(case):
    if case == "cornell_box":
        return scenes.cornell_box(128, 128), 128, 128
    if case == "textured_room":
        return scenes.textured_room(160, 100), 160, 100
    return scenes.sponza_mixed(160, 90), 160, 90


# ---- 1. the witness, fed the same hits --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cornell_box", "textured_room", "sponza_mixed"])
def test_surfaces_equal_the_float64_witness(gpu_ctx, scene_cache, case):
    s, w, h = _setup(case)
    scene = api.Scene(gpu_ctx, s.desc)
    st = scene.stats()
    rays = torch.cat([api.camera_rays(gpu_ctx, s.camera, w, h, 1),
                      torch.from_numpy(random_rays(st.boundsMin[:], st.boundsMax[:], 20000, seed=31)).cuda()])
    q = api.trace_rays(scene, rays)
    res = api.hit_surfaces(scene, rays, q)
    assert res.raw.shape == (len(rays), 20) and res.raw.device.type == "cuda"
    exp = Expect(Witness(s.desc), rays.cpu().numpy(), q.hits.cpu().numpy())
    assert_surfaces(res, exp, case)
    kinds = set(np.unique(exp.kind).tolist())
    assert {A.SURFACE_OBJECT, A.SURFACE_MISS} <= kinds and A.SURFACE_INVALID not in kinds
    if case == "textured_room":
        ois = [s.desc.objects[i] for i in range(s.desc.numObjects)]
        assert any(o.usesColorMap for o in ois) and s.desc.hdri


# ---- 2. the renderer's own images, bit for bit -------------------------------------------------------------------------------------
def _fma32(a, b, c):
    return (a.astype(np.float64) * b + c).astype(np.float32)


def _normalize32(x):
    """rtr_normalize: v * (1 / sqrt(fma(z, z, fma(y, y, x * x)))) in fp32"""
    x = x.astype(np.float32)
    d = _fma32(x[:, 2], x[:, 2], _fma32(x[:, 1], x[:, 1], x[:, 0] * x[:, 0]))
    inv = np.float32(1.0) / np.sqrt(d)
    return x * inv[:, None]


@pytest.mark.parametrize("case", ["cornell_box", "textured_room"])
def test_normal_and_position_images_equal_the_renderer(gpu_ctx, oracle, scene_cache, case):
    s, w, h = _setup(case)
    scene = api.Scene(gpu_ctx, s.desc)
    images = A.IMAGES_FRAMEBUFFER | A.IMG_BIT(A.IMAGE_NORMAL) | A.IMG_BIT(A.IMAGE_POSITION)
    frame = api.Frame(gpu_ctx, w, h, images)
    api.render(scene, s.camera, s.scene_info(0), api.make_params(w, h, spp=1, images=images), frame)
    nimg, pimg = frame.download(A.IMAGE_NORMAL).reshape(-1), frame.download(A.IMAGE_POSITION).reshape(-1)
    rays = api.camera_rays(gpu_ctx, s.camera, w, h, 1)
    res = api.hit_surfaces(scene, rays, api.trace_rays(scene, rays))
    kind = _np(res.kind)
    obj = np.nonzero(kind == A.SURFACE_OBJECT)[0]
    assert len(obj) > 0.3 * w * h
    one = np.float32(1.0)
    n = _normalize32((np.float32(0.0) + _np(res.normal)[obj]) / one)          # write_pixel: normalize(avgNormal / spp), avgNormal = 0 + n
    p = (np.float32(0.0) + _np(res.position)[obj]) / one
    pack = oracle.lib().oracle_pack_bgra8
    npk = np.array([pack(*map(float, r)) for r in n], np.uint32)
    ppk = np.array([pack(*map(float, r)) for r in p], np.uint32)
    dn, dp = int((npk != nimg[obj]).sum()), int((ppk != pimg[obj]).sum())
    assert dn == 0 and dp == 0, f"{case}: {dn} normal and {dp} position pixels differ of {len(obj)}"


# ---- 3. moved instances ----------------------------------------------------------------------------------------------------------
def test_surfaces_follow_moved_instances(gpu_ctx, scene_cache):
    s = scenes.cornell_box(64, 64)
    scene = api.Scene(gpu_ctx, s.desc)
    st = scene.stats()
    rays = torch.from_numpy(random_rays(st.boundsMin[:], st.boundsMax[:], 20000, seed=41)).cuda()
    inst = (A.RtrInstance * s.desc.numInstances)(*[A.RtrInstance.from_buffer_copy(s.desc.instances[i]) for i in range(s.desc.numInstances)])
    for k, i in enumerate(inst):
        if i.customIndex >= s.num_lights:
            i.transform[3] += 40.0 * (k % 3)
            i.transform[7] -= 25.0 * (k % 2)
            if k % 2:                                        # a rotation too, so that the normals must follow
                c, sn = np.cos(0.3), np.sin(0.3)
                for r in range(3):
                    a, b = i.transform[4 * r + 0], i.transform[4 * r + 2]
                    i.transform[4 * r + 0], i.transform[4 * r + 2] = c * a + sn * b, -sn * a + c * b
    before = api.hit_surfaces(scene, rays, api.trace_rays(scene, rays))
    scene.update_instances(list(inst))
    q = api.trace_rays(scene, rays)
    res = api.hit_surfaces(scene, rays, q)
    moved = A.rtr_scene_desc.from_buffer_copy(s.desc)
    moved.instances = inst
    exp = Expect(Witness(moved), rays.cpu().numpy(), q.hits.cpu().numpy())
    assert_surfaces(res, exp, "after update_instances")
    assert (exp.kind == A.SURFACE_OBJECT).mean() > 0.05
    assert not torch.equal(before.normal, res.normal)


# ---- 4. edge cases ---------------------------------------------------------------------------------------------------------------
def _hits(rows):
    """(N, 8) int32 RtrHit records from (u, v, customIndex, primitiveId) rows"""
    h = np.zeros((len(rows), 8), np.int32)
    for k, (u, v, c, p) in enumerate(rows):
        h[k, 0] = np.float32(1.0).view(np.int32)
        h[k, 1], h[k, 2] = np.float32(u).view(np.int32), np.float32(v).view(np.int32)
        h[k, 3], h[k, 4] = np.uint32(c).view(np.int32), np.uint32(p).view(np.int32)
    return h


def test_misses_give_the_sky(gpu_ctx, scene_cache):
    for s, hdri in ((scenes.textured_room(64, 40), True), (scenes.cornell_box(64, 64), False)):
        assert bool(s.desc.hdri) == hdri
        scene = api.Scene(gpu_ctx, s.desc)
        rng = np.random.default_rng(5)
        rays = np.zeros((4096, 8), np.float32)
        d = rng.normal(size=(4096, 3))
        rays[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
        rays[:, 7] = 1.0
        hits = _hits([(0.0, 0.0, MISS, MISS)] * 4096)
        res = api.hit_surfaces(scene, rays, hits)                     # numpy in, numpy out
        assert isinstance(res.color, np.ndarray) and (res.kind == A.SURFACE_MISS).all()
        exp = Expect(Witness(s.desc), rays, hits)
        assert_surfaces(res, exp, "misses")
        if not hdri:
            assert (res.color == res.color[0]).all()                 # skyLinear itself, for every direction
        else:
            assert len(np.unique(res.color[:, 0])) > 100             # the HDRI, looked up per direction


def test_light_hits_give_the_light_colour(gpu_ctx, scene_cache):
    s = scenes.cornell_box(64, 64)
    assert s.num_lights >= 1
    scene = api.Scene(gpu_ctx, s.desc)
    w = Witness(s.desc)
    rows = [(u, v, 0, p) for p in range(w.lights[0].numTriangles) for u, v in ((0.2, 0.3), (0.0, 0.0), (0.5, 0.5), (0.0, 1.0))]
    hits = _hits(rows)
    rays = np.zeros((len(rows), 8), np.float32)
    rays[:, 5], rays[:, 7] = 1.0, 10000.0
    res = api.hit_surfaces(scene, torch.from_numpy(rays).cuda(), torch.from_numpy(hits).cuda())
    assert (_np(res.kind) == A.SURFACE_LIGHT).all() and (_np(res.object_index) == 0).all()
    assert (_np(res.color) == np.array(s.desc.lights[0].color[:3], np.float32)).all()
    assert_surfaces(res, Expect(w, rays, hits), "light hits")


def test_ids_out_of_range_are_invalid(gpu_ctx, scene_cache):
    """the range check: ids one past the end give INVALID with zeros (and nothing out of range is read)"""
    s = scenes.cornell_box(64, 64)
    scene = api.Scene(gpu_ctx, s.desc)
    w = Witness(s.desc)
    counts = tri_counts(w)
    ninst = len(counts)
    obj = s.num_lights
    rows = [(0.2, 0.2, ninst, 0), (0.2, 0.2, 0xfffffffe, 0), (0.2, 0.2, obj, counts[obj]), (0.2, 0.2, 0, counts[0]),
            (0.2, 0.2, obj, 0xfffffffe), (0.2, 0.2, obj, counts[obj] - 1), (0.2, 0.2, 0, counts[0] - 1), (0.0, 0.0, MISS, 0)]
    hits = _hits(rows)
    rays = np.zeros((len(rows), 8), np.float32)
    rays[:, 6], rays[:, 7] = 1.0, 10000.0
    res = api.hit_surfaces(scene, rays, hits)
    assert res.kind.tolist() == [A.SURFACE_INVALID] * 5 + [A.SURFACE_OBJECT, A.SURFACE_LIGHT, A.SURFACE_MISS]
    assert (res.raw[:5] == 0).sum() == 5 * 18                      # all 18 floats and reserved words of an invalid hit are 0
    assert (res.object_index[:5] == -1).all()
    assert_surfaces(res, Expect(w, rays, hits), "ids out of range")


def test_plumbing(gpu_ctx, scene_cache):
    s = scenes.cornell_box(64, 64)
    scene = api.Scene(gpu_ctx, s.desc)
    lib, ctx = gpu_ctx.lib, gpu_ctx.h
    rays = api.camera_rays(gpu_ctx, s.camera, 8, 8, 1)
    q = api.trace_rays(scene, rays)
    out = torch.empty((64, 20), dtype=torch.float32, device="cuda")
    rp, hp, op = A.VP(rays.data_ptr()), A.VP(q.hits.data_ptr()), A.VP(out.data_ptr())
    INVALID = -1
    # numRays == 0 does nothing, whatever the pointers
    out.fill_(7.0)
    assert lib.rtr_hit_surfaces(ctx, scene.h, None, None, 0, None) == 0
    assert lib.rtr_hit_surfaces_async(ctx, scene.h, None, None, 0, None) == 0
    e = api.hit_surfaces(scene, rays[:0], q.hits[:0])
    assert e.raw.shape == (0, 20)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # null or unaligned pointers
    for args in ((None, hp, op), (rp, None, op), (rp, hp, None), (A.VP(rays.data_ptr() + 4), hp, op), (rp, A.VP(q.hits.data_ptr() + 8), op),
                 (rp, hp, A.VP(out.data_ptr() + 4))):
        assert lib.rtr_hit_surfaces(ctx, scene.h, *args[:2], 64, args[2]) == INVALID
        assert lib.rtr_hit_surfaces_async(ctx, scene.h, *args[:2], 64, args[2]) == INVALID
    assert b"16-B aligned" in lib.rtr_last_error()
    assert lib.rtr_hit_surfaces(None, scene.h, rp, hp, 64, op) == INVALID
    assert lib.rtr_hit_surfaces(ctx, None, rp, hp, 64, op) == INVALID
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert lib.rtr_hit_surfaces(ctx, scene.h, rp, hp, 64, op) == 0
    assert torch.equal(out.view(torch.int32), api.hit_surfaces(scene, rays, q).raw.view(torch.int32))
    # the Python layer refuses before anything is launched
    for bad_r, bad_h in ((rays[:, :7].contiguous(), q.hits), (rays.double(), q.hits), (rays.cpu(), q.hits), (rays, q.hits.float()),
                         (rays, q.hits[:10]), (rays.cpu().numpy(), q.hits), (rays, q.hits.t().contiguous().t())):
        with pytest.raises(ValueError):
            api.hit_surfaces(scene, bad_r, bad_h)
    with pytest.raises(ValueError):
        api.hit_surfaces(scene, rays, api.trace_rays(scene, rays, any_hit=True))
    # numpy in, numpy out, from a numpy query's result
    qn = api.trace_rays(scene, rays.cpu().numpy())
    rn = api.hit_surfaces(scene, rays.cpu().numpy(), qn)
    assert isinstance(rn.position, np.ndarray) and rn.raw.dtype == np.float32
    assert (rn.raw.view(np.uint32) == out.cpu().numpy().view(np.uint32)).all()


def test_asynchronous_surfaces_on_torchs_stream(scene_cache):
    s = scenes.cornell_box(128, 128)
    ctx = api.Context(0)
    scene = api.Scene(ctx, s.desc)
    rays0 = api.camera_rays(ctx, s.camera, 128, 128, 1)
    ref = api.hit_surfaces(scene, rays0, api.trace_rays(scene, rays0)).raw.clone()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx.set_stream(stream.cuda_stream)
        rays = api.camera_rays(ctx, s.camera, 128, 128, 1) * 1.0          # torch work on the stream between the calls
        q = api.trace_rays(scene, rays, asynchronous=True)
        r = api.hit_surfaces(scene, rays, q, asynchronous=True)
        got = r.raw.view(torch.int32) + 0                                  # consumed on the same stream, no host join in between
        stream.synchronize()
        assert torch.equal(got, ref.view(torch.int32))
        ctx.set_stream(None)
    with pytest.raises(ValueError):
        api.hit_surfaces(scene, rays, q, asynchronous=True)               # the context is no longer on torch's current stream
    scene.close(); ctx.close()
