"""rtr_compact_paths on the device: every output word of the three kernels, the tail and the count included, equals
rtr_host_compact_paths' (the same header, two compilers); nothing is written behind the arrays or the scratch, whose contents do not
matter; the asynchronous form is stream-ordered and allocates nothing; chained calls compose the ids; and api.path_trace(compact=True)
is the plain loop's result over the live paths only, with roulette the loop its docstring states, written out here."""
import ctypes as C

import numpy as np
import pytest
import torch

import bounce_witness as BW
import compact_witness as W
from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api, scenes
from test_gpu_surfaces import random_rays

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _i32(x):
    return None if x is None else torch.from_numpy(x.view(np.int32)).cuda()


def _assert_device_is_host(ctx, rays, thr, seeds, ids, params, what, view3=False):
    """every word of every output, and the count"""
    host = api.host_compact_paths(rays, thr, seeds, ids, params)
    t = torch.from_numpy(thr).cuda()
    dev = api.compact_paths(ctx, torch.from_numpy(rays).cuda(), t[:, 0:3] if view3 else t, seeds=_i32(seeds), path_ids=_i32(ids), params=params)
    assert dev.count == host.count, f"{what}: the device counts {dev.count} survivors, the host {host.count}"
    assert int(_np(dev.count_tensor).view(np.uint32)[0]) == host.count
    for name in ("rays", "throughput", "seeds", "path_ids"):
        h, d = getattr(host, name), getattr(dev, name)
        assert (h is None) == (d is None), f"{what}: {name}"
        if h is not None:
            bad = int((_np(d).view(np.uint32) != h.view(np.uint32)).sum())
            assert bad == 0, f"{what}: {bad} words of {name} differ between the device and the host"
    return host


@pytest.mark.parametrize("pattern", W.PATTERNS)
def test_device_equals_host(gpu_ctx, pattern):
    for n in W.SIZES:                                # one lane, the wave boundary, the workgroup boundary, a partial last workgroup
        for stride_words, with_ids, with_seeds in ((3, True, True), (8, False, True), (8, True, False)):
            rays, thr, seeds, ids, mask = W.make_paths(n, pattern, stride_words=stride_words)
            host = _assert_device_is_host(gpu_ctx, rays, thr, seeds if with_seeds else None, ids if with_ids else None, api.make_compact_params(frame=3, depth=1),
                                          f"{pattern}, {n} paths, stride {4 * stride_words}", view3=stride_words == 8 and with_ids)
            assert host.count == int(mask.sum())
        rays, thr, seeds, ids, mask = W.make_paths(n, pattern, t_hi=2.0)
        host = _assert_device_is_host(gpu_ctx, rays, thr, seeds, ids, api.make_compact_params(frame=5, depth=2, roulette=True, survival_floor=0.1),
                                      f"{pattern}, {n} paths, roulette")
        if n == 20000 and pattern in ("all_live", "alternating", "dead_block", "random_half"):
            assert 0 < host.count < int(mask.sum()) <= n
    if pattern in ("alternating", "random_half", "random_sparse", "dead_block"):
        assert 0 < int(mask.sum()) < 20000


def test_device_equals_host_on_the_edge_cases(gpu_ctx):
    cases = W.dead_causes() + W.live_oddities()
    rays, thr = np.stack([c[1] for c in cases] * 5), np.stack([c[2] for c in cases] * 5)
    seeds = np.arange(len(rays), dtype=np.uint32) * np.uint32(2654435761)
    seeds[::3] = (BW.SEED_U1_IS_ONE - 2 - 7919 * 2 - 300) & 0xffffffff          # the roulette's number is exactly 1.0 at frame 2, depth 1
    assert W.uniform(W.roulette_seed(seeds[:1], 2, 1))[0] == 1.0
    for roulette in (False, True):
        host = _assert_device_is_host(gpu_ctx, rays, thr, seeds, None, api.make_compact_params(frame=2, depth=1, roulette=roulette, survival_floor=0.05), f"edge cases, roulette {roulette}")
        assert 0 < host.count <= 5 * len(W.live_oddities())
    # p = max3(T) from just below 1 down to denormals, and the floor's lift: the divisions are the host's
    n = 4096
    rng = np.random.default_rng(5)
    thr = (rng.uniform(0, 1, (n, 3)) * 10.0 ** rng.uniform(-44, 0.3, (n, 1))).astype(np.float32)
    rays = np.repeat(np.array([[1, 2, 3, 0.001, 0, 0.6, 0.8, 10000]], np.float32), n, 0)
    seeds = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    for floor in (1e-6, 0.05, 1.0):
        host = _assert_device_is_host(gpu_ctx, rays, thr, seeds, None, api.make_compact_params(roulette=True, survival_floor=floor), f"small throughputs, floor {floor}")
    assert host.count == int(((thr > 0).any(1)).sum())                  # floor 1: nobody draws


@pytest.mark.parametrize("roulette", [False, True])
def test_device_equals_host_on_a_million_paths(gpu_ctx, roulette):
    """1 000 003 paths, half of them live at random: 3907 workgroups, so the scan takes four turns of its loop with a carry and the last
    workgroup is partial"""
    n = 1000003
    rays, thr, seeds, ids, mask = W.make_paths(n, "random_half", t_hi=2.0 if roulette else 1.0, stride_words=8)
    host = _assert_device_is_host(gpu_ctx, rays, thr, seeds, ids, api.make_compact_params(frame=1, depth=3, roulette=roulette, survival_floor=0.05), f"{n} paths")
    assert 0 < host.count < n and (host.count == int(mask.sum())) != roulette


def _raw_call(ctx, n, rays, thr, seeds, ids, params, scratch, scratch_bytes, outs, count, asynchronous=False):
    fn = ctx.lib.rtr_compact_paths_async if asynchronous else ctx.lib.rtr_compact_paths
    args = (ctx.h, A.VP(rays.data_ptr()), A.VP(thr.data_ptr()), A.VP(seeds.data_ptr()), A.VP(ids.data_ptr()), n, C.byref(params), A.VP(scratch.data_ptr()), scratch_bytes,
            A.VP(outs[0].data_ptr()), A.VP(outs[1].data_ptr()), A.VP(outs[2].data_ptr()), A.VP(outs[3].data_ptr()), A.VP(count.data_ptr()))
    return fn(*args) if asynchronous else fn(*args, None)


def test_nothing_is_written_behind_the_arrays_or_the_scratch(gpu_ctx):
    lib = gpu_ctx.lib
    for n in (1, 63, 65, 257, 1000):
        rays, thr, seeds, ids, _ = W.make_paths(n, "random_half", t_hi=2.0)
        p = api.make_compact_params(frame=1, roulette=True, survival_floor=0.2)
        host = api.host_compact_paths(rays, thr, seeds, ids, p)
        r, t, sd, i = torch.from_numpy(rays).cuda(), torch.from_numpy(thr).cuda(), _i32(seeds), _i32(ids)
        nbytes = api.compact_scratch_bytes(lib, n)
        for fill in (0x5A, 0xFF, 0x00):              # what the scratch holds before the call does not matter
            outs = [torch.full((n * w + 64,), GUARD, dtype=torch.int32, device="cuda") for w in (8, 3, 1, 1)]
            count = torch.full((16,), GUARD, dtype=torch.int32, device="cuda")
            scratch = torch.full((nbytes + 256,), fill, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            host_count = A.u32(GUARD)
            fn_args = (gpu_ctx.h, A.VP(r.data_ptr()), A.VP(t.data_ptr()), A.VP(sd.data_ptr()), A.VP(i.data_ptr()), n, C.byref(p), A.VP(scratch.data_ptr()), nbytes,
                       A.VP(outs[0].data_ptr()), A.VP(outs[1].data_ptr()), A.VP(outs[2].data_ptr()), A.VP(outs[3].data_ptr()), A.VP(count.data_ptr()))
            assert lib.rtr_compact_paths(*fn_args, C.byref(host_count)) == 0, lib.rtr_last_error()
            assert host_count.value == host.count and int(count[0]) == host.count
            for o, w in zip(outs, (8, 3, 1, 1)):
                assert (o[n * w:] == GUARD).all(), f"{n} paths: the guard words behind an output changed"
            assert (count[1:] == GUARD).all() and (scratch[nbytes:] == fill).all(), f"{n} paths: the words behind the count or the scratch changed"
            for o, w, want in zip(outs, (8, 3, 1, 1), (host.rays, host.throughput, host.seeds, host.path_ids)):
                assert (_np(o[:n * w]).view(np.uint32) == want.view(np.uint32).ravel()).all(), f"{n} paths, scratch filled with {fill:#x}"
    # a refused call writes nothing; numPaths == 0 writes the count and nothing else
    bad = api.make_compact_params(throughput_stride=8)
    before = [o.clone() for o in outs]
    assert _raw_call(gpu_ctx, n, r, t, sd, i, bad, scratch, nbytes, outs, count) == -1 and b"rtr_compact_paths: throughputStrideBytes" in lib.rtr_last_error()
    assert _raw_call(gpu_ctx, n, r, t, sd, i, p, scratch, nbytes - 16, outs, count) == -1 and b"scratchBytes" in lib.rtr_last_error()
    count[0] = 77
    torch.cuda.synchronize()
    assert _raw_call(gpu_ctx, 0, r, t, sd, i, p, scratch, nbytes, outs, count) == 0
    torch.cuda.synchronize()
    assert int(count[0]) == 0 and (count[1:] == GUARD).all() and all(torch.equal(a, b) for a, b in zip(before, outs))
    empty = api.compact_paths(gpu_ctx, torch.zeros((0, 8), device="cuda"), torch.zeros((0, 3), device="cuda"))
    assert empty.count == 0 and tuple(empty.rays.shape) == (0, 8) and tuple(empty.throughput.shape) == (0, 3) and empty.seeds is None


def test_asynchronous_compaction_on_torchs_stream_allocates_nothing():
    n = 20000
    rays, thr, seeds, ids, _ = W.make_paths(n, "random_half", t_hi=2.0)
    p0, p1 = api.make_compact_params(frame=2, depth=0), api.make_compact_params(frame=2, depth=1, roulette=True, survival_floor=0.1)
    first = api.host_compact_paths(rays, thr, seeds, ids, p0)
    second = api.host_compact_paths(first.rays, first.throughput, first.seeds, first.path_ids, p1)
    assert 0 < second.count < first.count < n
    ctx = api.Context(0)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx.set_stream(stream.cuda_stream)
        r, t = torch.from_numpy(rays).cuda() * 1.0, torch.from_numpy(thr).cuda() * 1.0       # torch work on the stream before the call
        sd, i = _i32(seeds), _i32(ids)
        a = api.compact_paths(ctx, r, t, seeds=sd, path_ids=i, params=p0, asynchronous=True)
        b = api.compact_paths(ctx, a.rays, a.throughput, seeds=a.seeds, path_ids=a.path_ids, params=p1, asynchronous=True)     # no host join in between
        got = [x.view(torch.int32) + 0 for x in (b.rays, b.throughput, b.seeds, b.path_ids)]
        assert b.count == second.count and a.count == first.count                          # the only joins
        for g, want in zip(got, (second.rays, second.throughput, second.seeds, second.path_ids)):
            assert (_np(g).view(np.uint32) == want.view(np.uint32)).all()
        # and two synchronous calls give the same
        sa = api.compact_paths(ctx, r, t, seeds=sd, path_ids=i, params=p0)
        sb = api.compact_paths(ctx, sa.rays, sa.throughput, seeds=sa.seeds, path_ids=sa.path_ids, params=p1)
        assert sb.count == b.count and all(torch.equal(x.view(torch.int32), g) for x, g in zip((sb.rays, sb.throughput, sb.seeds, sb.path_ids), got))
        # the call itself, on buffers that exist: torch's allocator statistics do not move across a second call
        nbytes = api.compact_scratch_bytes(ctx.lib, n)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        outs = [torch.empty(n * w, dtype=torch.int32, device="cuda") for w in (8, 3, 1, 1)]
        count = torch.empty(1, dtype=torch.int32, device="cuda")
        assert _raw_call(ctx, n, r, t, sd, i, p0, scratch, nbytes, outs, count, asynchronous=True) == 0, ctx.lib.rtr_last_error()
        stream.synchronize()
        stats0 = dict(torch.cuda.memory_stats())
        assert _raw_call(ctx, n, r, t, sd, i, p0, scratch, nbytes, outs, count, asynchronous=True) == 0
        stream.synchronize()
        assert dict(torch.cuda.memory_stats()) == stats0
        assert int(count[0]) == first.count and (_np(outs[0]).view(np.uint32) == first.rays.view(np.uint32).ravel()).all()
        ctx.set_stream(None)
    with pytest.raises(ValueError):
        api.compact_paths(ctx, r, t, seeds=sd, path_ids=i, params=p0, asynchronous=True)      # the context is no longer on torch's current stream
    ctx.close()


def test_chained_compactions_index_the_original_slots(gpu_ctx):
    n = 5000
    rays, thr, seeds, _, mask = W.make_paths(n, "random_half", t_hi=2.0, edge_cases=False)
    r, t, sd = torch.from_numpy(rays).cuda(), torch.from_numpy(thr).cuda(), _i32(seeds)
    a = api.compact_paths(gpu_ctx, r, t, seeds=sd)                                            # ids: 0 ... n - 1
    assert (_np(a.path_ids)[:a.count] == np.flatnonzero(mask)).all() and a.count == int(mask.sum())
    # the whole N-wide output goes in again, as a caller that never joins would pass it: the tail is dead and stays behind
    b = api.compact_paths(gpu_ctx, a.rays, a.throughput, seeds=a.seeds, path_ids=a.path_ids, params=api.make_compact_params(depth=1, roulette=True, survival_floor=0.1))
    assert 0 < b.count < a.count
    ids = _np(b.path_ids).view(np.uint32)
    assert (ids[b.count:] == A.PATH_NONE).all() and (np.diff(ids[:b.count].astype(np.int64)) > 0).all() and mask[ids[:b.count]].all()
    assert (_np(b.rays)[:b.count].view(np.uint32) == rays[ids[:b.count]].view(np.uint32)).all()
    assert (_np(b.seeds)[:b.count].view(np.uint32) == seeds[ids[:b.count]]).all()
    # shrunk to the count, the same survivors
    c = api.compact_paths(gpu_ctx, a.rays[:a.count], a.throughput[:a.count], seeds=a.seeds[:a.count], path_ids=a.path_ids[:a.count],
                          params=api.make_compact_params(depth=1, roulette=True, survival_floor=0.1))
    assert c.count == b.count and torch.equal(c.path_ids[:c.count], b.path_ids[:b.count]) and torch.equal(c.throughput[:c.count].view(torch.int32), b.throughput[:b.count].view(torch.int32))


# ---- path_trace(compact=True) --------------------------------------------------------------------------------------------------------
def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def cornell(gpu_ctx, scene_cache):
    s = scenes.cornell_box(128, 128)
    scene = api.Scene(gpu_ctx, s.desc)
    cam = api.camera_rays(gpu_ctx, s.camera, 128, 128, 1)
    lp = api.make_light_params(s.num_lights, 3, 4, 128, 1)
    st = scene.stats()
    rnd = torch.from_numpy(random_rays(st.boundsMin[:], st.boundsMax[:], 20000, seed=51)).cuda()
    rnd_seeds = torch.from_numpy(np.random.default_rng(3).integers(-2 ** 31, 2 ** 31, size=20000).astype(np.int32)).cuda()
    plain = {"camera": api.path_trace(scene, cam, lp, 2), "random": api.path_trace(scene, rnd, lp, 2, seeds=rnd_seeds)}      # computed once, never changed
    yield s, scene, lp, {"camera": (cam, None), "random": (rnd, rnd_seeds)}, plain
    scene.close()


def _assert_compact_is_plain(res, plain, n, what):
    assert res.live[0] == n and all(a >= b for a, b in zip(res.live, res.live[1:])), f"{what}: live = {res.live}"
    assert 0 < res.live[1] < n, f"{what}: live = {res.live}: every path or none goes on, the test shows nothing"
    assert len(res.per_depth) == len(plain.per_depth) == 3
    assert torch.equal(res.radiance, plain.radiance), f"{what}: radiance"
    for d, (a, b) in enumerate(zip(res.per_depth, plain.per_depth)):
        assert torch.equal(a, b), f"{what}: per_depth[{d}]"
        on = (b != 0).any(1)
        assert _same(a[on], b[on]), f"{what}: per_depth[{d}], the bits of the paths that contribute"
    assert (plain.per_depth[1] != 0).any() and (plain.per_depth[2] != 0).any()


@pytest.mark.parametrize("case", ["camera", "random"])
def test_compact_path_trace_is_the_plain_loop(gpu_ctx, cornell, case):
    s, scene, lp, inputs, plain = cornell
    rays, seeds = inputs[case]
    n = rays.shape[0]
    assert plain[case].live is None
    res = api.path_trace(scene, rays, lp, 2, seeds=seeds, compact=True)
    _assert_compact_is_plain(res, plain[case], n, case)
    # the queued occlusion route in small chunks: the same bytes, the same live counts
    Q = api.light_slots(scene, lp)
    queued = api.path_trace(scene, rays, lp, 2, seeds=seeds, occlusion="queued", max_ray_bytes=4096 * Q * 32, compact=True)
    _assert_compact_is_plain(queued, plain[case], n, case + ", queued")
    assert queued.live == res.live


@pytest.mark.parametrize("case", ["camera", "random"])
def test_roulette_path_trace_is_the_loop_of_its_definition(gpu_ctx, cornell, case):
    s, scene, lp, inputs, plain = cornell
    rays, seeds = inputs[case]
    n, dev = rays.shape[0], rays.device
    res = api.path_trace(scene, rays, lp, 3, seeds=seeds, compact=True, roulette_from=1, survival_floor=0.05)
    # the docstring's loop, from the public calls
    if seeds is None:
        k = torch.arange(n, device=dev, dtype=torch.int64) // int(lp.spp)
        base = (k % int(lp.width)) * 733 + (k // int(lp.width)) * 1933
    else:
        base = seeds.to(torch.int64)

    def wrap(x):
        x = x & 0xffffffff
        return torch.where(x >= 2 ** 31, x - 2 ** 32, x).to(torch.int32)
    base = wrap(base)
    T, r, ids, live, per_depth = torch.ones((n, 3), device=dev), rays, torch.arange(n, device=dev, dtype=torch.int32), [n], []
    for d in range(4):
        q = api.trace_rays(scene, r)
        lit = api.direct_light(scene, r, q, lp, seeds=seeds if d == 0 else wrap(base.to(torch.int64) + d * 0x9E3779B1))
        rad = lit.shadowed.clone()
        if d >= 1:
            rad[lit.kind == A.SURFACE_LIGHT] = 0.0
        term = torch.zeros((n, 3), device=dev)
        term[ids.to(torch.int64)] = T * rad
        per_depth.append(term)
        if d == 3:
            break
        b = api.bounce_rays(gpu_ctx, r, api.hit_surfaces(scene, r, q), api.make_bounce_params(frame=lp.frame, depth=d, width=lp.width, spp=lp.spp), seeds=base)
        c = api.compact_paths(gpu_ctx, b.rays, T * b.weight, seeds=base, path_ids=ids, params=api.make_compact_params(frame=lp.frame, depth=d, roulette=d >= 1, survival_floor=0.05))
        m = c.count
        live.append(m)
        r, T, base, ids = c.rays[:m], c.throughput[:m], c.seeds[:m], c.path_ids[:m]
    assert res.live == live and len(res.per_depth) == 4
    assert all(_same(a, b) for a, b in zip(res.per_depth, per_depth))
    assert _same(res.radiance, per_depth[0] + per_depth[1] + per_depth[2] + per_depth[3])
    # the roulette kills paths that the run without it keeps, and never makes a term negative or not finite
    no_roulette = api.path_trace(scene, rays, lp, 3, seeds=seeds, compact=True)
    assert no_roulette.live[1] == res.live[1] and res.live[2] < no_roulette.live[2], f"live {res.live} with roulette, {no_roulette.live} without: the test shows nothing"
    assert all(_same(a, b) for a, b in zip(res.per_depth[:2], no_roulette.per_depth[:2]))
    for term in res.per_depth:
        assert torch.isfinite(term).all() and (term >= 0).all()
    assert (res.per_depth[2] > 0).any() and (res.per_depth[3] > 0).any()
    with pytest.raises(ValueError):
        api.path_trace(scene, rays, lp, 2, seeds=seeds, roulette_from=1)


def test_a_compacting_path_trace_moves_nothing_else(gpu_ctx, cornell):
    s, scene, lp, inputs, plain = cornell
    images = A.IMAGES_FRAMEBUFFER | A.IMG_BIT(A.IMAGE_HDR)
    frame = api.Frame(gpu_ctx, 128, 128, images)
    params = api.make_params(128, 128, spp=1, images=images)
    api.render(scene, s.camera, s.scene_info(3), params, frame)
    before = [frame.download(k).copy() for k in (A.IMAGE_SHADOWED, A.IMAGE_HDR)]
    api.path_trace(scene, inputs["camera"][0], lp, 2, compact=True, roulette_from=0)
    api.render(scene, s.camera, s.scene_info(3), params, frame)
    after = [frame.download(k) for k in (A.IMAGE_SHADOWED, A.IMAGE_HDR)]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    frame.close()
