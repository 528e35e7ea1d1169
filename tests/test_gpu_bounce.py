"""rtr_bounce_rays on the device: the kernel's records equal rtr_host_bounce_rays' bit for bit (the same header, two compilers), nothing is
written past the last record, the asynchronous form is stream-ordered and allocates nothing, and api.path_trace is the loop its
docstring states, written out here from the public calls."""
import ctypes as C

import numpy as np
import pytest
import torch

import bounce_witness as W
from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api, scenes
from test_gpu_surfaces import random_rays

pytestmark = pytest.mark.gpu

BOTH = A.BOUNCE_DIFFUSE | A.BOUNCE_SPECULAR
LOBES = [A.BOUNCE_DIFFUSE, A.BOUNCE_SPECULAR, BOTH]


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _synthetic():
    """bounce_witness.make_surfaces' 20 000 records with the dead cases and the seeds whose random numbers are exactly 1.0 written over
    the first of them"""
    rays, sf, seeds = W.make_surfaces(20000)
    k = 0
    for _, ray, s, _ in W.dead_cases():
        rays[k], sf[k] = ray, s
        k += 1
    for offset in (0, 100, 200):                     # u1, u2, uLobe == 1.0 at frame 0, depth 0
        seeds[k:k + 40] = (W.SEED_U1_IS_ONE - 7919 - offset) & 0xffffffff
        k += 40
    return rays, sf, seeds


def _assert_device_is_host(ctx, rays, sf, seeds, params, what):
    host = api.host_bounce_rays(rays, sf, params, seeds)
    dev = api.bounce_rays(ctx, torch.from_numpy(rays).cuda(), torch.from_numpy(sf).cuda(), params,
                          seeds=None if seeds is None else torch.from_numpy(seeds.view(np.int32)).cuda())
    dr, db = _np(dev.rays).view(np.uint32), _np(dev.raw).view(np.uint32)
    d = int((dr != host.rays.view(np.uint32)).sum() + (db != host.raw.view(np.uint32)).sum())
    assert d == 0, f"{what}: {d} words differ between the device and the host"
    assert np.isfinite(_np(dev.rays)).all() and np.isfinite(_np(dev.raw)[:, [0, 1, 2, 3, 5]]).all(), f"{what}: a NaN or an infinity"
    return host


@pytest.mark.parametrize("lobes", LOBES)
def test_device_equals_host_on_synthetic_surfaces(gpu_ctx, lobes):
    rays, sf, seeds = _synthetic()
    for n in (1, 63, 64, 65, 257, 20000):            # one lane, the wave boundary, a partial last workgroup
        p = api.make_bounce_params(lobes=lobes)
        host = _assert_device_is_host(gpu_ctx, rays[:n].copy(), sf[:n].copy(), seeds[:n].copy(), p, f"lobes {lobes}, {n} hits")
    always_dead = [k for k, c in enumerate(W.dead_cases()) if c[3] == BOTH or c[3] == lobes]      # the others are dead for their lobe mask only
    assert len(always_dead) > 15 and not host.lobe[always_dead].any() and (host.lobe != 0).sum() > 5000
    # the same through the pixel seeds, another frame and depth, and other ray numbers
    p = api.make_bounce_params(frame=9, depth=2, width=171, spp=2, lobes=lobes, normal_offset=0.002, tmin=0.01, tmax=50.0)
    _assert_device_is_host(gpu_ctx, rays, sf, None, p, f"lobes {lobes}, pixel seeds")


@pytest.mark.parametrize("lobes", LOBES)
def test_device_equals_host_on_synthetic_surfaces_over_the_sphere_of_views(gpu_ctx, lobes):
    """the 20 000 records of make_surfaces(views="sphere"): 47 % seen from behind the shading normal, a grazing band, dot(N, V) exactly
    0.  Rays, RtrBounce words and the dead records' zero bytes are the host's, and the density rtr_host_bounce_pdf gives for the
    direction drawn is RtrBounce::pdf bit for bit."""
    rays, sf, seeds = W.make_surfaces(20000, views="sphere")
    for n in (65, 20000):
        p = api.make_bounce_params(lobes=lobes)
        host = _assert_device_is_host(gpu_ctx, rays[:n].copy(), sf[:n].copy(), seeds[:n].copy(), p, f"sphere of views, lobes {lobes}, {n} hits")
    live = host.lobe != 0
    nov = np.sum(sf[:, 4:7].astype(np.float64) * (rays[:, 0:3].astype(np.float64) - sf[:, 0:3]), axis=1)
    assert (live & (nov < 0)).sum() > 500 and (~live & (nov < 0)).sum() > 1000
    assert not host.rays[~live].any() and not host.raw.view(np.uint32)[~live].any()
    pdf = api.host_bounce_pdf(rays[live], sf[live], host.rays[live, 4:7], lobes)
    assert (pdf.view(np.uint32) == host.pdf[live].view(np.uint32)).all()
    p = api.make_bounce_params(frame=9, depth=2, width=171, spp=2, lobes=lobes, normal_offset=0.002, tmin=0.01, tmax=50.0)
    _assert_device_is_host(gpu_ctx, rays, sf, None, p, f"sphere of views, lobes {lobes}, pixel seeds")


@pytest.mark.parametrize("case", ["cornell_box", "textured_room", "random_rays"])
def test_device_equals_host_on_real_surfaces(gpu_ctx, scene_cache, case):
    if case == "textured_room":
        s, w, h = scenes.textured_room(160, 100), 160, 100
    else:
        s, w, h = scenes.cornell_box(128, 128), 128, 128
    scene = api.Scene(gpu_ctx, s.desc)
    if case == "random_rays":
        st = scene.stats()
        rays = torch.from_numpy(random_rays(st.boundsMin[:], st.boundsMax[:], 20000, seed=51)).cuda()
        seeds = np.random.default_rng(3).integers(0, 2 ** 32, size=20000, dtype=np.uint64).astype(np.uint32)
    else:
        rays, seeds = api.camera_rays(gpu_ctx, s.camera, w, h, 1), None
    surf = api.hit_surfaces(scene, rays, api.trace_rays(scene, rays))
    kinds = set(_np(surf.kind).tolist())
    assert A.SURFACE_OBJECT in kinds and len(kinds) >= 2
    for lobes in LOBES:
        p = api.make_bounce_params(frame=2, depth=0, width=w, spp=1, lobes=lobes)
        host = _assert_device_is_host(gpu_ctx, _np(rays), _np(surf.raw), seeds, p, f"{case}, lobes {lobes}")
        live = host.lobe != 0
        assert live.sum() > 1000 and not live[_np(surf.kind) != A.SURFACE_OBJECT].any()
        # a continuation starts on its surface, offset along the normal, and leaves into the normal's hemisphere
        nrm, pos = _np(surf.normal)[live], _np(surf.position)[live]
        assert (np.sum(host.rays[live, 4:7] * nrm, axis=1) > 0).all()
        assert np.abs(host.rays[live, 0:3] - (pos + np.float32(0.01) * nrm)).max() <= 1e-5 * max(1.0, float(np.abs(pos).max()))
    scene.close()


def test_nothing_is_written_past_the_last_record(gpu_ctx):
    rays, sf, seeds = _synthetic()
    lib = gpu_ctx.lib
    for n in (1, 63, 65, 257, 1000):
        guard = 64
        r, s = torch.from_numpy(rays[:n].copy()).cuda(), torch.from_numpy(sf[:n].copy()).cuda()
        sd = torch.from_numpy(seeds[:n].view(np.int32).copy()).cuda()
        out_r = torch.full((n + guard, 8), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        out_b = torch.full((n + guard, 8), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        p = api.make_bounce_params()
        rc = lib.rtr_bounce_rays(gpu_ctx.h, A.VP(r.data_ptr()), A.VP(s.data_ptr()), n, C.byref(p), A.VP(sd.data_ptr()), A.VP(out_r.data_ptr()), A.VP(out_b.data_ptr()))
        assert rc == 0, lib.rtr_last_error()
        assert (out_r[n:] == 0x5A5A5A5A).all() and (out_b[n:] == 0x5A5A5A5A).all(), f"{n} hits: the guard words behind the records changed"
        host = api.host_bounce_rays(rays[:n], sf[:n], p, seeds[:n])
        assert (_np(out_r[:n]).view(np.uint32) == host.rays.view(np.uint32)).all() and (_np(out_b[:n]).view(np.uint32) == host.raw.view(np.uint32)).all()
    # a refused call writes nothing, and numHits == 0 does nothing
    bad = api.make_bounce_params(lobes=0)
    assert lib.rtr_bounce_rays(gpu_ctx.h, A.VP(r.data_ptr()), A.VP(s.data_ptr()), n, C.byref(bad), None, A.VP(out_r.data_ptr() + 32 * n), A.VP(out_b.data_ptr() + 32 * n)) == -1
    assert b"rtr_bounce_rays: lobes" in lib.rtr_last_error()
    assert lib.rtr_bounce_rays(gpu_ctx.h, None, None, 0, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert (out_r[n:] == 0x5A5A5A5A).all() and (out_b[n:] == 0x5A5A5A5A).all()
    empty = api.bounce_rays(gpu_ctx, torch.zeros((0, 8), device="cuda"), torch.zeros((0, 20), device="cuda"), api.make_bounce_params(width=4))
    assert tuple(empty.rays.shape) == (0, 8) and tuple(empty.weight.shape) == (0, 3)


def test_asynchronous_bounce_on_torchs_stream_allocates_nothing():
    rays, sf, seeds = _synthetic()
    p = api.make_bounce_params()
    host = api.host_bounce_rays(rays, sf, p, seeds)
    ctx = api.Context(0)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx.set_stream(stream.cuda_stream)
        r, s = torch.from_numpy(rays).cuda() * 1.0, torch.from_numpy(sf).cuda()          # torch work on the stream before the call
        sd = torch.from_numpy(seeds.view(np.int32)).cuda()
        res = api.bounce_rays(ctx, r, s, p, seeds=sd, asynchronous=True)
        got_r, got_b = res.rays.view(torch.int32) + 0, res.raw.view(torch.int32) + 0     # consumed on the same stream, no host join in between
        stream.synchronize()
        assert (_np(got_r).view(np.uint32) == host.rays.view(np.uint32)).all() and (_np(got_b).view(np.uint32) == host.raw.view(np.uint32)).all()
        # the call itself, on buffers that exist: torch's allocator statistics do not move across a second call
        out_r, out_b = torch.empty_like(r), torch.empty_like(r)
        args = (ctx.h, A.VP(r.data_ptr()), A.VP(s.data_ptr()), len(rays), C.byref(p), A.VP(sd.data_ptr()), A.VP(out_r.data_ptr()), A.VP(out_b.data_ptr()))
        assert ctx.lib.rtr_bounce_rays_async(*args) == 0
        stream.synchronize()
        stats0 = dict(torch.cuda.memory_stats())
        assert ctx.lib.rtr_bounce_rays_async(*args) == 0
        stream.synchronize()
        assert dict(torch.cuda.memory_stats()) == stats0
        assert torch.equal(out_r.view(torch.int32), got_r)
        ctx.set_stream(None)
    with pytest.raises(ValueError):
        api.bounce_rays(ctx, r, s, p, seeds=sd, asynchronous=True)                       # the context is no longer on torch's current stream
    ctx.close()


# ---- path_trace ---------------------------------------------------------------------------------------------------------------------
def _loop(scene, ctx, rays, lp, bounces, seeds=None, cull=None, flags=0, max_ray_bytes=256 << 20):
    """the definition in api.path_trace's docstring, from the public calls"""
    n = rays.shape[0]
    if seeds is None:
        k = torch.arange(n, device=rays.device, dtype=torch.int64) // int(lp.spp)
        base = (k % int(lp.width)) * 733 + (k // int(lp.width)) * 1933
    else:
        base = seeds.to(torch.int64)
    T, L, r, per_depth, kinds = torch.ones((n, 3), device=rays.device), torch.zeros((n, 3), device=rays.device), rays, [], []
    for d in range(bounces + 1):
        q = api.trace_rays(scene, r) if d == 0 else api.trace_rays(scene, r, cull_mask=cull, ray_flags=flags)
        sd = seeds
        if d:
            x = (base + d * 0x9E3779B1) & 0xffffffff
            sd = torch.where(x >= 2 ** 31, x - 2 ** 32, x).to(torch.int32)
        lit = api.direct_light(scene, r, q, lp, seeds=sd, max_ray_bytes=max_ray_bytes)
        rad = lit.shadowed.clone()
        if d >= 1:
            rad[lit.kind == A.SURFACE_LIGHT] = 0.0
        kinds.append(lit.kind)
        L = L + T * rad
        per_depth.append(T * rad)
        if d == bounces:
            break
        b = api.bounce_rays(ctx, r, api.hit_surfaces(scene, r, q), api.make_bounce_params(frame=lp.frame, depth=d, width=lp.width, spp=lp.spp), seeds=seeds)
        T, r = T * b.weight, b.rays
    return L, per_depth, kinds


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def cornell(gpu_ctx, scene_cache):
    s = scenes.cornell_box(128, 128)
    scene = api.Scene(gpu_ctx, s.desc)
    rays = api.camera_rays(gpu_ctx, s.camera, 128, 128, 1)
    lp = api.make_light_params(s.num_lights, 3, 4, 128, 1)
    yield s, scene, rays, lp
    scene.close()


def test_path_trace_without_bounces_is_direct_light(gpu_ctx, cornell):
    s, scene, rays, lp = cornell
    res = api.path_trace(scene, rays, lp, 0)
    ref = api.direct_light(scene, rays, None, lp).shadowed
    assert len(res.per_depth) == 1 and _same(res.radiance, ref) and _same(res.per_depth[0], ref)


def test_path_trace_is_the_loop_of_its_definition(gpu_ctx, cornell):
    s, scene, rays, lp = cornell
    L, per_depth, kinds = _loop(scene, gpu_ctx, rays, lp, 2)
    res = api.path_trace(scene, rays, lp, 2)
    assert len(res.per_depth) == 3
    assert _same(res.radiance, L) and all(_same(a, b) for a, b in zip(res.per_depth, per_depth))
    # chunks do not change the result: 4096 hits x Q light rays x 32 B at a time
    Q = api.light_slots(scene, lp)
    small = api.path_trace(scene, rays, lp, 2, max_ray_bytes=4096 * Q * 32)
    assert _same(small.radiance, L) and all(_same(a, b) for a, b in zip(small.per_depth, per_depth))
    # explicit seeds, and the queued occlusion route
    seeds = torch.from_numpy(np.random.default_rng(8).integers(-2 ** 31, 2 ** 31, size=rays.shape[0]).astype(np.int32)).cuda()
    L2, pd2, _ = _loop(scene, gpu_ctx, rays, lp, 2, seeds=seeds)
    res2 = api.path_trace(scene, rays, lp, 2, seeds=seeds, occlusion="queued")
    assert _same(res2.radiance, L2) and all(_same(a, b) for a, b in zip(res2.per_depth, pd2))
    assert not _same(L2, L)
    for term in res.per_depth:
        assert torch.isfinite(term).all() and (term >= 0).all()
    # indirect light arrives where direct light cannot: object pixels beside the one-sided light (the ceiling) with no direct term
    obj = kinds[0] == A.SURFACE_OBJECT
    lit_only_indirectly = obj & (res.per_depth[0] == 0).all(1) & (res.per_depth[1] > 0).any(1)
    assert int(lit_only_indirectly.sum()) > 50
    zero = api.path_trace(scene, rays, lp, 0)
    assert (res.radiance >= zero.radiance).all(), "a pixel lost radiance to its bounces"
    assert (res.radiance > zero.radiance).any(1).float().mean() > 0.3


def test_bounce_cull_mask_keeps_bounce_rays_off_the_lights(gpu_ctx, scene_cache):
    s = scenes.cornell_box(128, 128)
    scene = api.Scene(gpu_ctx, s.desc)
    rays = api.camera_rays(gpu_ctx, s.camera, 128, 128, 1)
    lp = api.make_light_params(s.num_lights, 3, 0, 128, 1)
    _, _, kinds = _loop(scene, gpu_ctx, rays, lp, 2)
    assert any((k == A.SURFACE_LIGHT).any() for k in kinds[1:]), "no bounce ray of the unmasked scene reaches the light: the test shows nothing"
    masks = np.array([0x80 if s.desc.instances[i].customIndex < s.desc.numLights else 0xff for i in range(s.desc.numInstances)], np.uint8)
    scene.set_instance_masks(masks)
    L, per_depth, kinds = _loop(scene, gpu_ctx, rays, lp, 2, cull=0x7f)
    assert (kinds[0] == A.SURFACE_LIGHT).any(), "camera rays are not masked"
    assert not any((k == A.SURFACE_LIGHT).any() for k in kinds[1:])
    res = api.path_trace(scene, rays, lp, 2, bounce_cull_mask=0x7f)
    assert _same(res.radiance, L) and all(_same(a, b) for a, b in zip(res.per_depth, per_depth))
    scene.close()


def test_a_path_trace_moves_nothing_else(gpu_ctx, cornell):
    s, scene, rays, lp = cornell
    images = A.IMAGES_FRAMEBUFFER | A.IMG_BIT(A.IMAGE_HDR)
    frame = api.Frame(gpu_ctx, 128, 128, images)
    params = api.make_params(128, 128, spp=1, images=images)
    api.render(scene, s.camera, s.scene_info(3), params, frame)
    before = [frame.download(k).copy() for k in (A.IMAGE_SHADOWED, A.IMAGE_HDR)]
    api.path_trace(scene, rays, lp, 2)
    api.render(scene, s.camera, s.scene_info(3), params, frame)
    after = [frame.download(k) for k in (A.IMAGE_SHADOWED, A.IMAGE_HDR)]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    frame.close()
