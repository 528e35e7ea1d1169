"""Power-proportional light picks on the device (include/rtr_power.h).
  * Scene.export_light_power() equals host_light_power of export_light_tris(), word for word, on the one-triangle box, the three-lights
    box with unequal intensities and scales, and mesh lights whose triangle count crosses the scan's chunk size;
  * the drawn slots and weights equal rtr_host_pick_slots_power's word for word at the launch-shape edges, for P = 1, 2 and 30, with
    pixel seeds and explicit seeds, nothing written behind the outputs;
  * rtr_mis_pick_weights_power's and rtr_emitter_hits_power's records equal the host forms bit for bit on camera hits and random-ray hits;
  * after update_lights, update_instances and update_vertices_async the exported table is the host table of the new light triangles, and
    a scene without a table goes through the same calls as before;
  * direct_light_power has the full loops' mean, path_trace_power with equal-power lights has path_trace_mis's, and the picks do not
    change which paths live."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import shape_cases as SC
from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api, host, scenes
from test_gpu_surfaces import random_rays

pytestmark = pytest.mark.gpu

NS = 3
W = H = 128
GUARD = 0x5A5A5A5A
BLOCK = 256                                # kPowerBlock: the workgroup of k_pick_slots_power, and shape_cases.BATCH
SIZES = (1, SC.WAVE - 1, SC.WAVE, SC.WAVE + 1, BLOCK - 1, BLOCK, BLOCK + 1)
CHUNK = A.POWER_SCAN_CHUNK


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _bits(x):
    return np.ascontiguousarray(_np(x)).view(np.uint32)


def _i32(x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).cuda()


def _strip(path, tris):
    """a strip of `tris` triangles of growing width (so that their areas, and with them their powers, differ)"""
    with open(path, "w") as f:
        x = 0.0
        for i in range(tris + 2):
            f.write(f"v {x / tris - 0.5:.6f} {(i & 1) - 0.5:.1f} 0\n")
            x += 0.25 + 1.5 * ((i * 7) % 11) / 11.0
        for i in range(tris):
            f.write(f"f {i + 1} {i + 2} {i + 3}\n")


def _box(directory, lights):
    """the Cornell box with the given lights below the ceiling, facing down: (mesh, intensity, two-sided, x, (scale x, scale y)) each;
    mesh: 1 (a triangle), 2 (the quad) or a triangle count (a strip)"""
    tri = os.path.join(directory, "power_light_triangle.obj")
    if not os.path.exists(tri):
        with open(tri, "w") as f:
            f.write("v -0.5 -0.5 0\nv 0.5 -0.5 0\nv 0 0.5 0\nf 1 2 3\n")
    obj, mtldir = scenes.write_cornell(None)
    hs = host.HostScene()
    for k, (mesh, intensity, two_sided, x, scale) in enumerate(lights):
        path = tri if mesh == 1 else None
        if mesh > 2:
            path = os.path.join(directory, f"power_light_strip_{mesh}.obj")
            _strip(path, mesh)
        light = hs.addAreaLight(intensity, (1.0, 0.85 - 0.2 * k, 0.6 + 0.1 * k), two_sided, True, path)
        light.move((x, 540.0, 279.5)).scale((scale[0], scale[1], 1.0)).rotate((90.0, 0.0, 0.0))
    hs.addObjMtlPair(obj, mtldir)
    hs.setSky((0.5, 0.7, 1.0))
    hs.build()
    pos = (278.0, 273.0, -800.0)
    cam = host.Camera(40.0, pos, (278.0, 273.0, 0.0), (0.0, 1.0, 0.0), W, H)
    return scenes.SceneSetup("cornell_power", hs, cam, pos, W, H)


ONE = [(1, 20.0, False, 278.0, (130.0, 105.0))]
UNEQUAL = [(2, 40.0, False, 150.0, (150.0, 120.0)), (1, 0.5, True, 278.0, (60.0, 45.0)), (2, 6.0, False, 410.0, (100.0, 130.0))]


class World:
    """one scene with its camera hits (seeds: the pixels'), random-ray hits (explicit seeds), surfaces and light table: computed once"""
    def __init__(self, ctx, s, n_random=6000):
        self.s = s
        self.scene = api.Scene(ctx, s.desc)
        st = self.scene.stats()
        lo, hi = np.array(st.boundsMin[:], np.float64), np.array(st.boundsMax[:], np.float64)
        cam = api.camera_rays(ctx, s.camera, W, H, 1)
        rnd = torch.from_numpy(random_rays(lo + 0.25 * (hi - lo), hi - 0.25 * (hi - lo), n_random, seed=41)).cuda()
        rnd_seeds = np.random.default_rng(7).integers(0, 2 ** 32, n_random, dtype=np.uint64).astype(np.uint32)
        self.inputs = {"camera": (cam, api.trace_rays(self.scene, cam).hits, None), "random": (rnd, api.trace_rays(self.scene, rnd).hits, rnd_seeds)}
        self.frame = 5
        self.lights = [s.desc.lights[i] for i in range(s.num_lights)]
        self.rec, self.first = self.scene.export_light_tris()
        self.w, self.cdf = api.host_light_power(self.rec, self.first, self.lights)

    def params(self, kind, area_lights=None, ns=NS):
        return api.make_light_params(self.s.num_lights if area_lights is None else area_lights, ns, self.frame, W if kind == "camera" else 0, 1, A.LIGHT_SHADOWED)

    def tris(self, area_lights=None):
        return sum(int(l.numTriangles) for l in self.lights[:self.s.num_lights if area_lights is None else area_lights])

    def seeds(self, kind):
        sd = self.inputs[kind][2]
        return None if sd is None else _i32(sd)


@pytest.fixture(scope="module")
def worlds(gpu_ctx, scene_cache):
    made = {}

    def get(case):
        if case not in made:
            made[case] = World(gpu_ctx, _box(scene_cache, {"one": ONE, "unequal": UNEQUAL}[case]))
        return made[case]
    yield get
    for wd in made.values():
        wd.scene.close()


# ---- 1. the table ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["one", "unequal"])
def test_the_exported_table_is_the_hosts(worlds, case):
    wd = worlds(case)
    w, cdf = wd.scene.export_light_power()
    assert w.tolist() == wd.w.tolist() and cdf.tolist() == wd.cdf.tolist()
    assert w.max() == A.POWER_SCALE and (case == "one" or len(set(w.tolist())) > 2), f"the powers are not unequal: {w}"
    wd.scene.prepare_light_power()           # a second build is a no-op
    assert wd.scene.export_light_power()[1].tolist() == cdf.tolist()
    lib, count = wd.scene.lib, C.c_uint32(0)
    buf = np.full(len(w), 7, np.uint64)
    assert lib.rtr_scene_export_light_power(wd.scene.h, None, buf.ctypes.data_as(A.VP), len(w), C.byref(count)) == -1 and count.value == len(w)
    assert lib.rtr_scene_export_light_power(wd.scene.h, buf.ctypes.data_as(A.VP), buf.ctypes.data_as(A.VP), len(w) - 1, C.byref(count)) == -1
    assert lib.rtr_last_error().decode() == f"rtr_scene_export_light_power: capacity {len(w) - 1} light triangles, {len(w)} are needed" and (buf == 7).all()


@pytest.mark.parametrize("tris", [CHUNK - 1, CHUNK, CHUNK + 1])
def test_a_mesh_light_across_the_scans_chunk(gpu_ctx, scene_cache, tris):
    """one strip light of chunk - 1, chunk and chunk + 1 triangles: the scan's one pass is not full, exactly full, and followed by a
    second that takes the carry of the first; the draws over the table are the host's"""
    s = _box(scene_cache, [(tris, 11.0, True, 278.0, (400.0, 90.0))])
    scene = api.Scene(gpu_ctx, s.desc)
    try:
        lights = [s.desc.lights[0]]
        rec, first = scene.export_light_tris()
        assert rec.shape[0] == tris
        w, cdf = scene.export_light_power()
        hw, hc = api.host_light_power(rec, first, lights)
        assert w.tolist() == hw.tolist() and cdf.tolist() == hc.tolist()
        assert len(set(w.tolist())) > 8 and w.all() and int(cdf[-1]) == int(w.astype(np.uint64).sum())
        n, pick, p = 600, api.make_pick_params(2, 1), api.make_light_params(1, NS, 3, 40, 1)
        slots, weights = api.pick_slots_power(scene, n, p, pick)
        hs_, hw_ = api.host_pick_slots_power(hc, tris, None, n, p, pick)
        assert (_bits(slots) == hs_).all() and (_bits(weights) == _bits(hw_)).all()
        assert len(np.unique(hs_ // NS)) > 50
    finally:
        scene.close()


# ---- 2. the drawn slots and weights are the host's -------------------------------------------------------------------------------------------
def _raw_pick_slots(ctx, wd, kind, n, p, pick):
    """rtr_pick_slots_power straight through the C ABI on the first n hits, guard words behind both outputs"""
    P = int(pick.numPicks)
    out_slots = torch.full((n * P + 16,), GUARD, dtype=torch.int32, device="cuda")
    out_weights = torch.full((n * P + 16,), GUARD, dtype=torch.int32, device="cuda")
    seeds = wd.seeds(kind)
    torch.cuda.synchronize()
    rc = ctx.lib.rtr_pick_slots_power(ctx.h, wd.scene.h, n, C.byref(p), C.byref(pick), A.VP(seeds.data_ptr()) if seeds is not None else None,
                                      A.VP(out_slots.data_ptr()), A.VP(out_weights.data_ptr()))
    assert rc == 0, ctx.lib.rtr_last_error().decode()
    s, w = _bits(out_slots), _bits(out_weights)
    assert (s[n * P:] == GUARD).all() and (w[n * P:] == GUARD).all(), "written behind an output"
    return s[:n * P].reshape(n, P), w[:n * P].reshape(n, P)


@pytest.mark.parametrize("case", ["one", "unequal"])
@pytest.mark.parametrize("kind", ["camera", "random"])
def test_drawn_slots_and_weights_equal_the_hosts(gpu_ctx, worlds, case, kind):
    wd = worlds(case)
    sd = wd.inputs[kind][2]
    for area_lights in sorted({wd.s.num_lights, 1}):
        tris = wd.tris(area_lights)
        for n in SIZES:
            for P in (1, 2, 30):
                pick, p = api.make_pick_params(P, P % 3), wd.params(kind, area_lights)
                slots, weights = _raw_pick_slots(gpu_ctx, wd, kind, n, p, pick)
                hs_, hw_ = api.host_pick_slots_power(wd.cdf, tris, None if sd is None else sd[:n], n, p, pick)
                what = f"{case} {kind}: {area_lights} lights, {n} hits, {P} picks"
                assert (slots == hs_).all(), f"{what}: {(slots != hs_).sum()} slots differ from the host's"
                assert (weights == _bits(hw_)).all(), f"{what}: {(weights != _bits(hw_)).sum()} weights differ from the host's"
                assert (slots < tris * NS).all()


def test_the_wrapper_and_the_refusals_that_need_a_scene(gpu_ctx, worlds):
    wd = worlds("unequal")
    pick = api.make_pick_params(2)
    sd = wd.inputs["random"][2][:100]
    slots, weights = api.pick_slots_power(wd.scene, 100, wd.params("random"), pick, seeds=_i32(sd))
    ns_, nw_ = api.pick_slots_power(wd.scene, 100, wd.params("random"), pick, seeds=sd)          # numpy in, numpy out
    assert isinstance(ns_, np.ndarray) and ns_.dtype == np.uint32 and (_bits(slots) == ns_).all() and (_bits(weights) == _bits(nw_)).all()
    empty = api.pick_slots_power(wd.scene, 0, wd.params("camera"), pick)
    assert tuple(empty[0].shape) == (0, 2) and tuple(empty[1].shape) == (0, 2)
    # numAreaLights 0: nothing to pick from
    s0, w0 = api.pick_slots_power(wd.scene, 70, wd.params("camera", 0), pick)
    assert (_bits(s0) == A.PICK_NONE).all() and not _bits(w0).any()
    with pytest.raises(api.RtrError, match="rtr_pick_slots_power: numAreaLights 4 > scene lights 3"):
        api.pick_slots_power(wd.scene, 10, wd.params("camera", 4), pick)
    rays, hits, _ = wd.inputs["camera"]
    with pytest.raises(api.RtrError, match="rtr_mis_pick_weights_power: numAreaLights 4 > scene lights 3"):
        api.mis_pick_weights_power(wd.scene, rays[:10], hits[:10], wd.params("camera", 4), pick, api.make_mis_params(2, 4, NS), _i32(np.zeros((10, 2), np.uint32)))
    with pytest.raises(api.RtrError, match="rtr_emitter_hits_power: numAreaLights 4 > scene lights 3"):
        surf = api.hit_surfaces(wd.scene, rays[:10], hits[:10])
        b = api.bounce_rays(gpu_ctx, rays[:10], surf, api.make_bounce_params(width=W))
        api.emitter_hits_power(wd.scene, rays[:10], hits[:10], surf, b, api.make_mis_params(2, 4, NS))


# ---- 3. the MIS kernels' power forms -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["one", "unequal"])
@pytest.mark.parametrize("kind", ["camera", "random"])
@pytest.mark.parametrize("picks", [1, 2, 30])
def test_mis_pick_weights_power_equals_the_host_form(gpu_ctx, worlds, case, kind, picks):
    """the device's RtrMisSample records give the numbers the pick was weighed with (pb, dist, cosLight, area, lightTri); the host form of
    those numbers gives the device's lightPdf, wPick and weight bit for bit"""
    wd = worlds(case)
    rays, hits, sd = wd.inputs[kind]
    total, n = int(rays.shape[0]), 2 * BLOCK + 1
    # 513 hits spread over the whole set (the first rows of a frame see the ceiling, which no light reaches), each with the seed it
    # has there: the pixel's, handed in
    rows = np.linspace(0, total - 1, n).astype(np.int64)
    if sd is None:
        sd = ((rows % W) * 733 + (rows // W) * 1933).astype(np.uint32)
    else:
        sd = sd[rows]
    rows = torch.from_numpy(rows).cuda()
    rays, hits, seeds = rays[rows].contiguous(), hits[rows].contiguous(), _i32(sd)
    area_lights = wd.s.num_lights if picks != 2 else 1
    p, pick, tris = wd.params("random", area_lights), api.make_pick_params(picks, 1), wd.tris(area_lights)
    mis = api.make_mis_params(picks, area_lights, NS)
    slots, wpow = api.pick_slots_power(wd.scene, n, p, pick, seeds=seeds)
    out = torch.full((n * picks + 16,), GUARD, dtype=torch.int32, device="cuda")
    rec = torch.full((n * picks + 2, 8), GUARD, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = gpu_ctx.lib.rtr_mis_pick_weights_power(gpu_ctx.h, wd.scene.h, A.VP(rays.data_ptr()), A.VP(hits.data_ptr()), n, C.byref(p), C.byref(pick), C.byref(mis),
                                                A.VP(seeds.data_ptr()), A.VP(slots.data_ptr()), A.VP(out.data_ptr()),
                                                A.VP(rec.data_ptr()))
    assert rc == 0, gpu_ctx.lib.rtr_last_error().decode()
    o, r = _bits(out), _bits(rec)
    assert (o[n * picks:] == GUARD).all() and (r[n * picks:] == GUARD).all(), "written behind an output"
    wt, smp = o[:n * picks], r[:n * picks]
    f = smp.view(np.float32)
    live = smp.any(axis=1)
    assert live.sum() > n * picks // 10, "few picks send a ray"
    assert not wt[~live].any()
    assert (smp[live, 6] == _bits(slots).reshape(-1)[live] // NS).all(), "lightTri is not the slot's triangle"
    hs_, hwb, hwt = api.host_mis_weights_power(f[live, 1], f[live, 4], f[live, 3], f[live, 5], smp[live, 6], wd.cdf, tris, picks)
    assert (_bits(hs_)[:, :7] == smp[live, :7]).all(), f"{(_bits(hs_)[:, :7] != smp[live, :7]).any(axis=1).sum()} records differ from the host form's"
    assert (_bits(hwt) == wt[live]).all(), "the weights differ from the host form's"
    both = api.mis_pick_weights_power(wd.scene, rays, hits, p, pick, mis, slots, seeds=seeds, samples=True)
    assert (_bits(both[0]).reshape(-1) == wt).all() and (_bits(both[1]).reshape(-1, 8) == smp).all()
    # the uniform form on the same inputs is the function it was: its own host form of its own numbers (tests/test_gpu_mis.py holds the rest)
    uw, us = api.mis_pick_weights(wd.scene, rays, hits, p, pick, mis, slots, seeds=seeds, samples=True)
    us = _bits(us).reshape(-1, 8)
    uf, ulive = us.view(np.float32), us.any(axis=1)
    assert (ulive == live).all()
    hu, _ = api.host_mis_weights(uf[ulive, 1], uf[ulive, 4], uf[ulive, 3], uf[ulive, 5], tris, picks)
    assert (_bits(hu)[:, :6] == us[ulive, :6]).all()
    assert (_bits(uw).reshape(-1)[ulive] == _bits((np.float32(tris) / np.float32(picks)) * hu[:, 2])).all()


@pytest.mark.parametrize("case", ["one", "unequal"])
@pytest.mark.parametrize("kind", ["camera", "random"])
def test_emitter_hits_power_equals_the_host_form(gpu_ctx, worlds, case, kind):
    wd = worlds(case)
    rays, hits, _ = wd.inputs[kind]
    seeds = wd.seeds(kind)
    surf = api.hit_surfaces(wd.scene, rays, hits)
    b = api.bounce_rays(gpu_ctx, rays, surf, api.make_bounce_params(frame=wd.frame, depth=0, width=W if kind == "camera" else 0, spp=1), seeds=seeds)
    bh = api.trace_rays(wd.scene, b.rays).hits
    met = _bits(bh)[:, 3] < wd.s.num_lights
    assert met.sum() > 3, "hardly a bounce ray meets a light"
    total = int(rays.shape[0])
    for area_lights, picks in ((wd.s.num_lights, 1), (1, 2), (wd.s.num_lights, 30)):
        mis = api.make_mis_params(picks, area_lights, NS)
        for n in (1, SC.WAVE + 1, BLOCK - 1, BLOCK, BLOCK + 1, total):
            out = torch.full((n + 2, 8), GUARD, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            rc = gpu_ctx.lib.rtr_emitter_hits_power(gpu_ctx.h, wd.scene.h, A.VP(b.rays.data_ptr()), A.VP(bh.data_ptr()), A.VP(surf.raw.data_ptr()),
                                                    A.VP(b.raw.data_ptr()), n, C.byref(mis), A.VP(out.data_ptr()))
            assert rc == 0, gpu_ctx.lib.rtr_last_error().decode()
            got = _bits(out)
            assert (got[n:] == GUARD).all(), "written behind out"
            want = api.host_emitter_hits_power(_np(b.rays)[:n], _np(bh)[:n], _np(surf.raw)[:n], _np(b.raw)[:n], wd.rec, wd.first, wd.lights, wd.cdf, mis)
            assert (got[:n] == _bits(want.raw)).all(), f"{n} rays: {(got[:n] != _bits(want.raw)).any(axis=1).sum()} records differ from the host form's"
            assert not got[:n][~met[:n]].any()
        counts = got[:total, 7] == A.SURFACE_LIGHT
        assert counts.sum() > 0
        # a light the picks cannot reach is the bounce's alone
        far = counts & (_bits(bh)[:, 3] >= area_lights)
        assert (got[:total][far, 3] == _bits(np.float32(1.0))).all()
        # the uniform form on the same inputs equals its own host form, as before
        u = api.emitter_hits(wd.scene, b.rays, bh, surf, b, mis)
        hu = api.host_emitter_hits(_np(b.rays), _np(bh), _np(surf.raw), _np(b.raw), wd.rec, wd.first, wd.lights, mis)
        assert (_bits(u.raw) == _bits(hu.raw)).all()


# ---- 4. the table follows the lights ---------------------------------------------------------------------------------------------------
def _copies(s):
    lights = [A.RtrAreaLightInfo.from_buffer_copy(s.desc.lights[i]) for i in range(s.num_lights)]
    inst = [A.RtrInstance.from_buffer_copy(s.desc.instances[i]) for i in range(s.desc.numInstances)]
    return lights, inst


def _scaled(lights, inst, l, k):
    """light l and its instance with the linear part of the transform times k (the light's is column-major 4 x 4, the instance's row-major 3 x 4)"""
    for c in range(3):
        for r in range(3):
            lights[l].transform[c * 4 + r] *= k
    for i in inst:
        if i.customIndex == l:
            for r in range(3):
                for c in range(3):
                    i.transform[r * 4 + c] *= k


def _assert_current(scene, lights, what):
    rec, first = scene.export_light_tris()
    w, cdf = scene.export_light_power()
    hw, hc = api.host_light_power(rec, first, lights)
    assert w.tolist() == hw.tolist() and cdf.tolist() == hc.tolist(), f"{what}: the table is not the host table of the new light triangles"
    return w


@pytest.mark.parametrize("prepared", [True, False])
def test_the_table_follows_the_updates(gpu_ctx, scene_cache, prepared):
    """prepared: the scene has a power table before the updates, which then remake it; else the same calls run on a scene without one
    (they launch what they launched before), and the table made afterwards is current all the same"""
    s = _box(scene_cache, UNEQUAL)
    scene, twin = api.Scene(gpu_ctx, s.desc), api.Scene(gpu_ctx, s.desc)
    try:
        lights, inst = _copies(s)
        if prepared:
            scene.prepare_light_power()
            w0 = _assert_current(scene, lights, "at the start")
        # an intensity change
        lights[1].intensity = 80.0
        lights[2].color[0] = 0.1
        scene.update_lights(lights); twin.update_lights(lights)
        if prepared:
            w1 = _assert_current(scene, lights, "update_lights")
            assert w1[2] > w0[2] and w1[3] < w0[3] and w1[0] == A.POWER_SCALE, "the middle light gained, the third lost, the first is still the strongest"
        # a scaled light
        _scaled(lights, inst, 0, 0.5)
        scene.update_instances(inst, lights); twin.update_instances(inst, lights)
        if prepared:
            w2 = _assert_current(scene, lights, "update_instances")
            assert w2[0] < w1[0] and w2[2] == A.POWER_SCALE, "at a quarter of its area the first light is weaker than the middle one"
        # the vertices of a light's mesh, enqueued
        scene.prepare_async_updates(); twin.prepare_async_updates()
        v0 = int(lights[2].vertexOffset)
        pos = scene.export_vertices(raw=True)[v0:v0 + 4, 0:3].copy()
        pos[:, 0:2] *= np.float32(1.5)
        dev = torch.from_numpy(np.ascontiguousarray(pos)).cuda()
        torch.cuda.synchronize()
        scene.update_vertices_async([(v0, dev)]); twin.update_vertices_async([(v0, dev)])
        assert scene.update_status().refused == 0
        w3 = _assert_current(scene, lights, "update_vertices_async")
        if prepared:
            assert w3[3] > w2[3], "the third light grew"
        # a refused update rebuilds the same table from unchanged data
        bad = dev.clone()
        bad[1, 1] = float("nan")
        scene.update_vertices_async([(v0, bad)])
        assert scene.update_status().refused == 1
        assert _assert_current(scene, lights, "a refused update").tolist() == w3.tolist()
        # the scene's other tables went the way they go without a power table
        assert scene.export_light_tris()[0].tobytes() == twin.export_light_tris()[0].tobytes()
        assert bytes(scene.export_bvh()[0]) == bytes(twin.export_bvh()[0])
    finally:
        scene.close(); twin.close()


# ---- 5. the composed routes --------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_direct_light_power_is_the_composed_route(gpu_ctx, worlds):
    wd = worlds("unequal")
    for kind in ("camera", "random"):
        rays, hits, _ = wd.inputs[kind]
        p, pick, seeds = wd.params(kind), api.make_pick_params(2, 3), wd.seeds(kind)
        n = int(rays.shape[0])
        sl, w = api.pick_slots_power(wd.scene, n, p, pick, seeds=seeds)
        lr, sl2 = api.light_rays_picked(wd.scene, rays, hits, p, pick, seeds=seeds, slots=sl)
        assert _same(sl, sl2)
        occ = api.trace_rays(wd.scene, lr, any_hit=True).occluded
        want = api.shade_hits_picked(wd.scene, rays, hits, p, pick, sl, occ, weights=w, seeds=seeds)
        for kw in (dict(), dict(max_ray_bytes=1000 * 3 * 32), dict(occlusion="queued")):
            got = api.direct_light_power(wd.scene, rays, hits, p, picks=2, pick_depth=3, seeds=seeds, **kw)
            assert (_bits(got.raw) == _bits(want.raw)).all(), f"{kind} {kw}"
        mis = api.make_mis_params(2, wd.s.num_lights, NS)
        wm = api.mis_pick_weights_power(wd.scene, rays, hits, p, pick, mis, sl, seeds=seeds)
        want = api.shade_hits_picked(wd.scene, rays, hits, p, pick, sl, occ, weights=wm, seeds=seeds)
        got = api.direct_light_power(wd.scene, rays, hits, p, picks=2, pick_depth=3, seeds=seeds, mis=mis)
        assert (_bits(got.raw) == _bits(want.raw)).all(), f"{kind} with mis"
        # the uniform route is the route it was
        a = api.direct_light(wd.scene, rays, hits, p, seeds=seeds, picks=2, pick_depth=3)
        lr_u, sl_u = api.light_rays_picked(wd.scene, rays, hits, p, pick, seeds=seeds)
        occ_u = api.trace_rays(wd.scene, lr_u, any_hit=True).occluded
        assert (_bits(a.raw) == _bits(api.shade_hits_picked(wd.scene, rays, hits, p, pick, sl_u, occ_u, seeds=seeds).raw)).all()


def test_direct_light_power_has_the_full_loops_mean(gpu_ctx, scene_cache):
    """The image sum of the shadowed radiance of the camera hits over 64 frame seeds, the full loops against one power pick: the two
    averages agree within 5 sqrt(se1^2 + se2^2), the standard errors from the frame-to-frame scatter of each.  The uniform pick's
    scatter is printed beside the power pick's, not asserted."""
    s = _box(scene_cache, UNEQUAL)
    scene = api.Scene(gpu_ctx, s.desc)
    rays = api.camera_rays(gpu_ctx, s.camera, 64, 64, 1)
    hits = api.trace_rays(scene, rays).hits
    sums = {"full": [], "power": [], "uniform": []}
    for f in range(64):
        lp = api.make_light_params(3, NS, f, 64, 1)
        sums["full"].append(float(api.direct_light(scene, rays, hits, lp).shadowed.double().sum()))
        sums["power"].append(float(api.direct_light_power(scene, rays, hits, lp, picks=1).shadowed.double().sum()))
        sums["uniform"].append(float(api.direct_light(scene, rays, hits, lp, picks=1).shadowed.double().sum()))
    scene.close()
    full, power, uniform = (np.array(sums[k]) for k in ("full", "power", "uniform"))
    assert np.isfinite(full).all() and np.isfinite(power).all() and full.mean() > 0
    se1, se2 = full.std(ddof=1) / np.sqrt(64), power.std(ddof=1) / np.sqrt(64)
    dev = (power.mean() - full.mean()) / np.sqrt(se1 ** 2 + se2 ** 2)
    print(f"image sum of the camera hits: full loops {full.mean():.4f} +- {se1:.4f}, one power pick {power.mean():.4f} +- {se2:.4f}: {dev:+.2f} standard errors "
          f"apart; one uniform pick {uniform.mean():.4f} +- {uniform.std(ddof=1) / np.sqrt(64):.4f}; variance of the sum power / uniform "
          f"{power.var(ddof=1) / uniform.var(ddof=1):.3f}")
    assert abs(dev) <= 5.0


def test_path_trace_power_with_equal_lights_has_path_trace_mis_mean_and_its_live_paths(gpu_ctx, scene_cache):
    """three lights of one mesh, one scale, one intensity and colours of one maximum: every triangle has the same power, so the picks'
    distribution is the uniform one.  bounces=1, pick_from=0, one pick, 32 x 32, frames 0 ... 63: the image sum of radiance has
    path_trace_mis's mean within 5 standard errors of their combined frame-to-frame scatter.  Then the live counts under compaction
    with roulette: the picks do not change which paths live."""
    tri = os.path.join(scene_cache, "power_light_triangle.obj")
    with open(tri, "w") as f:
        f.write("v -0.5 -0.5 0\nv 0.5 -0.5 0\nv 0 0.5 0\nf 1 2 3\n")
    hs = host.HostScene()
    for k, x in enumerate((150.0, 278.0, 410.0)):
        hs.addAreaLight(15.0, (1.0, 0.85 - 0.2 * k, 0.6 + 0.1 * k), k == 1, True, tri).move((x, 540.0, 279.5)).scale((130.0, 105.0, 1.0)).rotate((90.0, 0.0, 0.0))
    hs.addObjMtlPair(*scenes.write_cornell(None))
    hs.setSky((0.5, 0.7, 1.0))
    hs.build()
    pos = (278.0, 273.0, -800.0)
    s = scenes.SceneSetup("cornell_equal", hs, host.Camera(40.0, pos, (278.0, 273.0, 0.0), (0.0, 1.0, 0.0), 32, 32), pos, 32, 32)
    scene = api.Scene(gpu_ctx, s.desc)
    try:
        w, _ = scene.export_light_power()
        assert (w >= A.POWER_SCALE - 2).all(), f"the lights are not of equal power to the last place of their areas: {w}"
        rays = api.camera_rays(gpu_ctx, s.camera, 32, 32, 1)
        sums = {"mis": [], "power": []}
        for f in range(64):
            lp = api.make_light_params(3, NS, f, 32, 1)
            sums["mis"].append(float(api.path_trace_mis(scene, rays, lp, 1, light_picks=1, pick_from=0).radiance.double().sum()))
            sums["power"].append(float(api.path_trace_power(scene, rays, lp, 1, sky_samples=0, light_picks=1, pick_from=0).radiance.double().sum()))
        mis, power = np.array(sums["mis"]), np.array(sums["power"])
        assert np.isfinite(mis).all() and np.isfinite(power).all() and mis.mean() > 0
        se1, se2 = mis.std(ddof=1) / np.sqrt(64), power.std(ddof=1) / np.sqrt(64)
        dev = (power.mean() - mis.mean()) / np.sqrt(se1 ** 2 + se2 ** 2)
        print(f"image sum of radiance: path_trace_mis {mis.mean():.4f} +- {se1:.4f}, path_trace_power {power.mean():.4f} +- {se2:.4f}: {dev:+.2f} standard errors apart")
        assert abs(dev) <= 5.0
        lp = api.make_light_params(3, NS, 4, 32, 1)
        a = api.path_trace_mis(scene, rays, lp, 3, light_picks=2, compact=True, roulette_from=1)
        b = api.path_trace_power(scene, rays, lp, 3, sky_samples=0, light_picks=2, compact=True, roulette_from=1)
        assert a.live == b.live and a.live[0] == rays.shape[0] and 0 < a.live[3] < a.live[1]
        assert _same(a.per_depth[0], b.per_depth[0]) and torch.isfinite(b.radiance).all() and (b.per_depth[2] != 0).any()
        # the defaults (one sky sample per vertex) run, and compaction without roulette changes nothing
        c = api.path_trace_power(scene, rays, lp, 2)
        d = api.path_trace_power(scene, rays, lp, 2, compact=True)
        assert torch.isfinite(c.radiance).all() and torch.equal(c.radiance, d.radiance)
    finally:
        scene.close()
