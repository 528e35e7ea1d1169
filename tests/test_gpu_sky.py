"""Sky importance sampling on the device (rtr_scene_prepare_sky, rtr_sky_rays, rtr_shade_sky, rtr_sky_hits) in the textured room, whose
HDRI has a bright patch, in the same room under a 5 x 3 R8 HDRI, under a 2 x 4100 R8 HDRI (more rows than k_sky_rays stages in LDS: the
search in global memory), and under the constant sky:
  * the device's sky table is the host's, word for word, and no update, refit or rebuild touches it;
  * rtr_sky_rays and rtr_sky_hits give rtr_host_sky_rays' and rtr_host_sky_hits' bits at the wave's and the workgroup's edges, every
    slot written; rtr_shade_sky is the sum in sample order;
  * the sample rays are answered by both occlusion queries alike, and a dead sample is not occluded;
  * api.path_trace_sky without sky samples is path_trace_mis, tensor for tensor;
  * the enqueued forms on a prepared scene give the joined forms' bytes, and every refusal leaves its outputs alone."""
import ctypes as C

import numpy as np
import pytest
import torch

from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api, scenes

import bounce_witness as BW
import sky_witness as SW

pytestmark = pytest.mark.gpu

W, H = 64, 40
SIZES = [1, 63, 64, 65, 255, 256, 257]
MISS = 0xffffffff


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _bits(x):
    return np.ascontiguousarray(_np(x)).view(np.uint32)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


class World:
    """a scene, its sky on the host, its camera hits and their surfaces: computed once, never changed"""
    def __init__(self, ctx, kind):
        self.s = scenes.textured_room(W, H, hdri=kind != "constant")
        desc = self.s.desc
        self.hdri, self.color = SW.hdri_of(desc), None
        if kind in ("r8", "tall"):
            self.hdri = np.random.default_rng(8).integers(0, 256, (3, 5) if kind == "r8" else (4100, 2), dtype=np.uint8)
            self.hdri[1, -1] = 0
            self._tex = A.rtr_texture(self.hdri.ctypes.data_as(C.POINTER(C.c_uint8)), self.hdri.shape[1], self.hdri.shape[0], 1, 0)
            desc = A.rtr_scene_desc.from_buffer_copy(desc)
            desc.hdri = C.pointer(self._tex)
        if kind == "constant":
            self.color = tuple(desc.skyColor)
        self.desc = desc
        self.scene = api.Scene(ctx, desc)
        self.table = api.host_sky_table(self.hdri, self.color)
        self.rays = api.camera_rays(ctx, self.s.camera, W, H, 1)
        self.hits = api.trace_rays(self.scene, self.rays).hits
        self.surf = api.hit_surfaces(self.scene, self.rays, self.hits)

    def host_rays(self, rays, surf, p, seeds):
        return api.host_sky_rays(self.table, _np(rays), _np(surf), p, seeds=seeds, hdri=self.hdri, sky_color=self.color)

    def host_hits(self, rays, hits, surf, bounces, p):
        return api.host_sky_hits(self.table, _np(rays), _np(hits), _np(surf), _np(bounces), p, hdri=self.hdri, sky_color=self.color)


@pytest.fixture(scope="module", params=["room", "r8", "tall", "constant"])
def any_world(request, gpu_ctx, scene_cache):
    wd = World(gpu_ctx, request.param)
    yield wd
    wd.scene.close()


@pytest.fixture(scope="module")
def world(gpu_ctx, scene_cache):
    wd = World(gpu_ctx, "room")
    yield wd
    wd.scene.close()


@pytest.fixture(scope="module")
def synthetic():
    rays, sf, seeds = BW.make_surfaces(2000, seed=21, views="sphere")
    return rays, sf, seeds


def _same_table(a, b):
    return (a.width, a.height) == (b.width, b.height) and np.array_equal(a.rows, b.rows) and np.array_equal(a.marginal, b.marginal)


def test_device_table_is_the_hosts_and_stays(any_world, gpu_ctx):
    wd = any_world
    assert _same_table(wd.scene.export_sky_table(), wd.table)
    assert (wd.table.width, wd.table.height) == ((32, 16) if wd.hdri is None else wd.hdri.shape[1::-1])
    fresh = api.Scene(gpu_ctx, wd.desc)
    fresh.prepare_sky()
    fresh.prepare_sky()                                       # once per scene: the second call does nothing
    assert _same_table(fresh.export_sky_table(), wd.table)
    v = fresh.export_vertices(raw=True)
    fresh.update_vertices([(0, np.ascontiguousarray(v[:, 0:3] * np.float32(1.01)))])
    assert _same_table(fresh.export_sky_table(), wd.table)
    fresh.update_instances(list(fresh.export_instances()))
    assert _same_table(fresh.export_sky_table(), wd.table)
    fresh.rebuild("device")
    assert _same_table(fresh.export_sky_table(), wd.table)
    fresh.close()


def _check_rays(wd, rays, surf, seeds, S, mis, n):
    p = api.make_sky_params(samples=S, depth=2, frame=9, width=W, spp=1, mis=mis)
    r, s = rays[:n].contiguous(), surf[:n].contiguous()
    sd = None if seeds is None else seeds[:n].contiguous()
    ctx = wd.scene.ctx
    out_r = torch.full((n * S + 1, 8), -1, dtype=torch.int32, device="cuda")          # 0xff bytes, and a guard record behind
    out_s = torch.full((n * S + 1, 8), -1, dtype=torch.int32, device="cuda")
    rc = ctx.lib.rtr_sky_rays(ctx.h, wd.scene.h, A.VP(r.data_ptr()), A.VP(s.data_ptr()), n, C.byref(p), A.VP(sd.data_ptr()) if sd is not None else None,
                              A.VP(out_r.data_ptr()), A.VP(out_s.data_ptr()))
    assert rc == 0, ctx.lib.rtr_last_error()
    host = wd.host_rays(r, s, p, None if sd is None else _np(sd).view(np.uint32))
    assert np.array_equal(_bits(out_r[:-1]).reshape(n, S, 8), host.rays.view(np.uint32)), (n, S, mis)
    assert np.array_equal(_bits(out_s[:-1]).reshape(n, S, 8), host.raw.view(np.uint32)), (n, S, mis)
    assert (_np(out_r[-1]) == -1).all() and (_np(out_s[-1]) == -1).all()
    return host


@pytest.mark.parametrize("S", [1, 2, 8])
def test_sky_rays_equal_the_host_bits(any_world, synthetic, S):
    wd = any_world
    sr, ss, sseeds = (_dev(x) for x in (synthetic[0], synthetic[1], synthetic[2].view(np.int32)))
    live = 0
    for mis in (False, True):
        host = _check_rays(wd, wd.rays, wd.surf.raw, None, S, mis, W * H)                 # the pixel rule
        live += int((host.rays[:, :, 7] != 0).sum())
        _check_rays(wd, sr, ss, sseeds, S, mis, 2000)
        for n in SIZES:
            _check_rays(wd, wd.rays[1000:], wd.surf.raw[1000:], torch.arange(n, dtype=torch.int32, device="cuda") * 7919 + 5, S, mis, n)
            _check_rays(wd, sr, ss, None if n % 2 else sseeds, S, mis, n)
    kinds = _bits(wd.surf.raw)[:, 3]
    assert {A.SURFACE_OBJECT, A.SURFACE_LIGHT, A.SURFACE_MISS} <= set(kinds.tolist()) and live > W * H // 4


def test_sky_rays_api_and_shade_sky(world, synthetic):
    wd = world
    rng = np.random.default_rng(6)
    for S in (1, 2, 8):
        p = api.make_sky_params(samples=S, width=W, spp=1)
        k = api.sky_rays(wd.scene, wd.rays, wd.surf, p)
        host = wd.host_rays(wd.rays, wd.surf.raw, p, None)
        assert np.array_equal(_bits(k.rays), host.rays.view(np.uint32)) and np.array_equal(_bits(k.raw), host.raw.view(np.uint32))
        assert tuple(k.contrib.shape) == (W * H, S, 3) and tuple(k.cell.shape) == (W * H, S)
        for n in SIZES + [W * H]:
            occ = (rng.uniform(size=(n, S)) < 0.4).astype(np.uint8) * rng.integers(1, 256, (n, S)).astype(np.uint8)
            got = _np(api.shade_sky(wd.scene.ctx, k.raw[:n].contiguous(), _dev(occ)))
            acc = np.zeros((n, 3), np.float32)
            for j in range(S):
                c = host.contrib[:n, j]
                acc = np.where((occ[:, j] == 0)[:, None], acc + c, acc)
            assert np.array_equal(got.view(np.uint32), acc.view(np.uint32)), (S, n)
    kn = api.sky_rays(wd.scene, _np(wd.rays), _np(wd.surf.raw), p)                        # numpy in, numpy out
    assert isinstance(kn.raw, np.ndarray) and np.array_equal(kn.raw.view(np.uint32), host.raw.view(np.uint32))


@pytest.mark.parametrize("S", [0, 1, 8])
def test_sky_hits_equal_the_host_bits(any_world, synthetic, S):
    wd = any_world
    ctx = wd.scene.ctx
    b = api.bounce_rays(ctx, wd.rays, wd.surf, api.make_bounce_params(frame=3, width=W, spp=1))
    q = api.trace_rays(wd.scene, b.rays).hits
    custom = _bits(q)[:, 3]
    assert (custom == MISS).any() and (custom != MISS).any()
    for mis in (False, True):
        p = api.make_sky_params(samples=S, width=W, spp=1, mis=mis)
        for n in SIZES + [W * H]:
            e = api.sky_hits(wd.scene, b.rays[:n].contiguous(), q[:n].contiguous(), wd.surf.raw[:n].contiguous(), b.raw[:n].contiguous(), p)
            host = wd.host_hits(b.rays[:n], q[:n], wd.surf.raw[:n], b.raw[:n], p)
            assert np.array_equal(_bits(e.raw), host.raw.view(np.uint32)), (S, mis, n)
        miss = custom == MISS
        assert not _bits(e.raw)[~miss].any()                                              # objects, lights: 32 zero bytes
        if not mis or S == 0:
            color = _bits(api.hit_surfaces(wd.scene, b.rays, q).raw)[:, 12:15]
            assert np.array_equal(_bits(e.radiance)[miss], color[miss]) and (_np(e.w_bounce)[miss] == 1).all()
        else:
            wb = _np(e.w_bounce)[miss]
            assert (wb >= 0).all() and (wb <= 1).all() and (wb < 1).any()
    # an id that is neither a light nor an object is no miss
    bad = q.clone()
    bad[:, 3] = 0x7fffffff
    e = api.sky_hits(wd.scene, b.rays, bad, wd.surf.raw, b.raw, api.make_sky_params(samples=1, width=W, spp=1))
    assert not _bits(e.raw).any()


def test_sample_rays_are_answered_by_both_queries(world):
    wd = world
    p = api.make_sky_params(samples=2, width=W, spp=1)
    k = api.sky_rays(wd.scene, wd.rays, wd.surf, p)
    rays = k.rays.reshape(-1, 8)
    dense = _np(api.trace_rays(wd.scene, rays, any_hit=True).occluded)
    queued = _np(api.trace_occlusion(wd.scene, rays).occluded)
    assert np.array_equal(dense != 0, queued != 0)
    dead = _np(rays)[:, 7] == 0
    assert dead.any() and (~dead).any() and not dense[dead].any()
    assert (dense[~dead] != 0).any() and (dense[~dead] == 0).any()
    out = _np(api.shade_sky(wd.scene.ctx, k, _dev(dense).reshape(-1, 2)))
    assert np.isfinite(out).all() and not out[dead.reshape(-1, 2).all(axis=1)].any()


@pytest.mark.parametrize("compact", [False, True])
def test_path_trace_sky_without_samples_is_path_trace_mis(world, compact):
    wd = world
    lp = api.make_light_params(wd.s.num_lights, 3, 4, W, 1, A.LIGHT_SHADOWED)
    ref = api.path_trace_mis(wd.scene, wd.rays, lp, 2, compact=compact)
    got = api.path_trace_sky(wd.scene, wd.rays, lp, 2, sky_samples=0, compact=compact)
    assert torch.equal(ref.radiance, got.radiance) and len(ref.per_depth) == len(got.per_depth) == 3
    assert all(torch.equal(a, b) for a, b in zip(ref.per_depth, got.per_depth))
    miss = torch.from_numpy(_bits(wd.hits)[:, 3] == MISS).cuda()
    for mis in (True, False):
        sky = api.path_trace_sky(wd.scene, wd.rays, lp, 2, sky_samples=1, sky_mis=mis, compact=compact)
        assert all(bool(torch.isfinite(t).all()) for t in sky.per_depth) and bool(torch.isfinite(sky.radiance).all())
        assert torch.equal(sky.per_depth[0][miss], ref.per_depth[0][miss]) and bool(miss.any())
        assert not torch.equal(sky.per_depth[0], ref.per_depth[0])                        # the camera hits took sky samples


def test_enqueued_chain_on_a_prepared_scene(world):
    wd = world
    p = api.make_sky_params(samples=2, width=W, spp=1)
    n, S = W * H, 2
    k = api.sky_rays(wd.scene, wd.rays, wd.surf, p)
    occ = api.trace_rays(wd.scene, k.rays.reshape(-1, 8), any_hit=True).occluded
    ref = api.shade_sky(wd.scene.ctx, k, occ)
    ctx = api.Context(0)
    scene = api.Scene(ctx, wd.desc)
    scene.prepare_sky()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx.set_stream(stream.cuda_stream)
        r, s = wd.rays * 1.0, wd.surf.raw * 1.0
        for _ in range(2):
            out_r = torch.full((n * S, 8), -1, dtype=torch.int32, device="cuda")
            out_s = torch.full((n * S, 8), -1, dtype=torch.int32, device="cuda")
            out = torch.full((n, 4), -1, dtype=torch.int32, device="cuda")
            assert ctx.lib.rtr_sky_rays_async(ctx.h, scene.h, A.VP(r.data_ptr()), A.VP(s.data_ptr()), n, C.byref(p), None, A.VP(out_r.data_ptr()), A.VP(out_s.data_ptr())) == 0
            o = api.trace_rays(scene, out_r.view(torch.float32), any_hit=True, ctx=ctx, asynchronous=True).occluded
            assert ctx.lib.rtr_shade_sky_async(ctx.h, A.VP(out_s.data_ptr()), A.VP(o.data_ptr()), n, S, A.VP(out.data_ptr())) == 0
            stream.synchronize()
            assert np.array_equal(_bits(out_r).reshape(n, S, 8), _bits(k.rays)) and np.array_equal(_bits(out_s).reshape(n, S, 8), _bits(k.raw))
            assert np.array_equal(_bits(out)[:, 0:3], _bits(ref)) and not _bits(out)[:, 3].any()
        ctx.set_stream(None)
    scene.close()
    ctx.close()


def test_refusals_leave_the_outputs_alone(world):
    wd = world
    ctx, lib = wd.scene.ctx, wd.scene.ctx.lib
    n, S = 64, 2
    r, s = wd.rays[:n].contiguous(), wd.surf.raw[:n].contiguous()
    b = api.bounce_rays(ctx, r, s, api.make_bounce_params(width=W, spp=1))
    q = api.trace_rays(wd.scene, b.rays).hits
    out_r = torch.full((n * S, 8), -1, dtype=torch.int32, device="cuda")
    out_s = torch.full((n * S, 8), -1, dtype=torch.int32, device="cuda")
    out = torch.full((n, 8), -1, dtype=torch.int32, device="cuda")
    occ = torch.zeros(n * S, dtype=torch.uint8, device="cuda")
    good = api.make_sky_params(samples=S, width=W, spp=1)

    def params(**kw):
        p = api.make_sky_params(samples=S, width=W, spp=1)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def ptr(t, off=0):
        return None if t is None else A.VP(t.data_ptr() + off)

    def rays_call(p=good, rays=r, surf=s, seeds=None, o_r=out_r, o_s=out_s, count=n, scene=wd.scene, off=0):
        return lib.rtr_sky_rays(ctx.h, scene.h if scene else None, ptr(rays), ptr(surf), count, C.byref(p) if p else None, ptr(seeds), ptr(o_r, off), ptr(o_s))

    def hits_call(p=good, rays=b.rays, hits=q, surf=s, bounce=b.raw, o=out, off=0):
        return lib.rtr_sky_hits(ctx.h, wd.scene.h, ptr(rays), ptr(hits), ptr(surf), ptr(bounce), n, C.byref(p) if p else None, ptr(o, off))

    def shade_call(samples=out_s, o=out, num=S, occluded=occ, off=0):
        return lib.rtr_shade_sky(ctx.h, ptr(samples), ptr(occluded), n, num, ptr(o, off))

    cases = [
        (lambda: rays_call(p=None), "rtr_sky_rays", "params is null"),
        (lambda: rays_call(p=params(numSamples=0)), "rtr_sky_rays", "numSamples 0"),
        (lambda: rays_call(p=params(numSamples=9)), "rtr_sky_rays", "numSamples 9"),
        (lambda: rays_call(p=params(lobes=0)), "rtr_sky_rays", "lobes 0x0"),
        (lambda: rays_call(p=params(lobes=8)), "rtr_sky_rays", "lobes 0x8"),
        (lambda: rays_call(p=params(flags=4)), "rtr_sky_rays", "unknown flags bits 0x4"),
        (lambda: rays_call(p=params(_reserved=3)), "rtr_sky_rays", "_reserved"),
        (lambda: rays_call(p=params(width=0)), "rtr_sky_rays", "width 0"),
        (lambda: rays_call(p=params(spp=0)), "rtr_sky_rays", "spp 0"),
        (lambda: rays_call(rays=None), "rtr_sky_rays", "rays is null"),
        (lambda: rays_call(surf=None), "rtr_sky_rays", "surfaces is null"),
        (lambda: rays_call(o_s=None), "rtr_sky_rays", "outSamples is null"),
        (lambda: rays_call(off=4), "rtr_sky_rays", "outRays is not 16-B aligned"),
        (lambda: rays_call(o_r=r), "rtr_sky_rays", "outRays overlaps rays"),
        (lambda: rays_call(o_s=out_r, off=0), "rtr_sky_rays", "outRays overlaps outSamples"),
        (lambda: rays_call(count=0x80000000), "rtr_sky_rays", "do not fit 32 bits"),
        (lambda: rays_call(scene=None), "rtr_sky_rays", "null context or scene"),
        (lambda: hits_call(p=params(numSamples=9)), "rtr_sky_hits", "numSamples 9 (0 ... 8)"),
        (lambda: hits_call(p=params(flags=2)), "rtr_sky_hits", "unknown flags bits 0x2"),
        (lambda: hits_call(hits=None), "rtr_sky_hits", "hits is null"),
        (lambda: hits_call(bounce=None), "rtr_sky_hits", "bounces is null"),
        (lambda: hits_call(off=8), "rtr_sky_hits", "out is not 16-B aligned"),
        (lambda: hits_call(o=b.raw), "rtr_sky_hits", "out overlaps bounces"),
        (lambda: shade_call(num=0), "rtr_shade_sky", "numSamples 0"),
        (lambda: shade_call(num=9), "rtr_shade_sky", "numSamples 9"),
        (lambda: shade_call(occluded=None), "rtr_shade_sky", "occluded is null"),
        (lambda: shade_call(off=4), "rtr_shade_sky", "out is not 16-B aligned"),
        (lambda: shade_call(o=out_s), "rtr_shade_sky", "out overlaps samples"),
    ]
    keep = [t.view(torch.int32).clone() for t in (r, s, b.raw, b.rays)]                 # bits: a record may hold a NaN
    for call, who, needle in cases:
        assert call() == -1, needle
        msg = lib.rtr_last_error().decode()
        assert msg.startswith(who + ": ") and needle in msg, (needle, msg)
    torch.cuda.synchronize()
    assert (out_r == -1).all() and (out_s == -1).all() and (out == -1).all()
    assert all(torch.equal(a, b_.view(torch.int32)) for a, b_ in zip(keep, (r, s, b.raw, b.rays)))
    with pytest.raises(ValueError):
        api.path_trace_sky(wd.scene, wd.rays, api.make_light_params(wd.s.num_lights, 3, 0, W, 1), 1, sky_samples=9)
