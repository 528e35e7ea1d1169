"""rtr_accumulate_paths and rtr_gather_records on the device: every word of accum, outTerm and outThroughput equals
rtr_host_accumulate_paths' (the same header, two compilers), guard words included; the gather equals the host's on both of its paths;
the asynchronous form is stream-ordered and allocates nothing; and api.path_trace_library gives the radiance, every per_depth[d] and
live of the loop it names, torch.equal.

Why equality and no tolerance: the operations and their order are the torch loops' (include/rtr_accum.h) and contraction is off; a row
a compaction dropped adds +0.0 in torch and nothing in the kernel, and a running sum that starts at +0.0 is never -0.0."""
import ctypes as C

import numpy as np
import pytest
import torch

import accum_witness as W
from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api, scenes
from test_gpu_power import UNEQUAL, _box
from test_gpu_surfaces import random_rays

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]
BOTH = W.LIGHTS_FROM_EMITTERS | W.MISSES_FROM_ESCAPES


def _run(fn, handle, case, bufs_addr):
    return W.call_accumulate(fn, handle, case, A, bufs_addr)


def _host_result(case):
    lib = A.hip_lib()
    bufs = case.host_buffers()
    rc = _run(lib.rtr_host_accumulate_paths, None, case, lambda name: bufs[name][1].ctypes.data if bufs[name] is not None else None)
    assert rc == 0, lib.rtr_last_error()
    return bufs


def _device_result(ctx, case, name="rtr_accumulate_paths"):
    """the same guarded buffers on the device, guard words and all -> name -> the whole buffer's words after the call"""
    host = case.host_buffers()
    dev = {k: (torch.from_numpy(v[0].view(np.int32).copy()).cuda() if v is not None else None) for k, v in host.items()}
    torch.cuda.synchronize()
    rc = _run(getattr(ctx.lib, name), ctx.h, case, lambda k: dev[k].data_ptr() + 4 * W.GUARD_WORDS if dev[k] is not None else None)
    assert rc == 0, ctx.lib.rtr_last_error()
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy().view(np.uint32) if v is not None else None) for k, v in dev.items()}


def _assert_device_is_host(ctx, case, what):
    host, dev = _host_result(case), _device_result(ctx, case)
    for name, h in host.items():
        assert (h is None) == (dev[name] is None)
        if h is not None:
            bad = int((h[0] != dev[name]).sum())
            assert bad == 0, f"{what}: {bad} words of {name} (guards included) differ between the device and the host"
    return host


@pytest.mark.parametrize("n", SIZES)
def test_device_equals_host(gpu_ctx, n):
    for ids in ("identity", "mixed"):
        case = W.AccumCase(n, flags=BOTH, emitters=True, escapes=True, sky=True, bounces=True, term=True, ids=ids, seed=21)
        _assert_device_is_host(gpu_ctx, case, f"{n} paths, {ids} ids")
    _assert_device_is_host(gpu_ctx, W.AccumCase(n, seed=22), f"{n} paths, no optional array")


@pytest.mark.parametrize("slots", ["more", "equal", "fewer"])
def test_device_equals_host_past_65536_paths(gpu_ctx, slots):
    n = 65537
    S = {"more": n + 300, "equal": n, "fewer": n - 300}[slots]
    for ids in ("identity", "mixed"):
        case = W.AccumCase(n, num_slots=S, flags=BOTH, emitters=True, escapes=True, sky=True, bounces=True, term=True, ids=ids, seed=23)
        host = _assert_device_is_host(gpu_ctx, case, f"{n} paths, {S} slots, {ids} ids")
        assert not (host["accum"][1].reshape(S, 3) == case.accum0.view(np.uint32)).all()
        skipped = int((case.slots() >= S).sum())
        assert skipped > 0 or (slots != "fewer" and ids == "identity")


def test_device_equals_host_on_the_optional_array_combinations(gpu_ctx):
    cases = W.optional_cases(257)
    assert any(c.inplace for c in cases) and {c.t_words for c in cases} == {3, 4, 8} and {c.image_words for c in cases} == {3, 4}
    for k, case in enumerate(cases):
        host = _assert_device_is_host(gpu_ctx, case, f"combination {k}")
        want_acc, want_term, want_t = case.expected()                  # and both are the witness
        assert (host["accum"][1] == want_acc.view(np.uint32).ravel()).all()
        assert want_term is None or (host["term"][1] == want_term.view(np.uint32).ravel()).all()
        if want_t is not None:
            got = host["T"][1] if case.inplace else host["out_t"][1]
            assert (got == want_t.view(np.uint32).ravel()).all()


def test_the_async_form_and_zero_paths(gpu_ctx):
    case = W.AccumCase(257, flags=BOTH, emitters=True, escapes=True, sky=True, bounces=True, term=True, ids="mixed", seed=25)
    host, dev = _host_result(case), _device_result(gpu_ctx, case, "rtr_accumulate_paths_async")
    assert all((host[k][0] == dev[k]).all() for k in host if host[k] is not None)
    lib = gpu_ctx.lib
    acc = torch.full((64,), 3.0, device="cuda")
    for fn in (lib.rtr_accumulate_paths, lib.rtr_accumulate_paths_async):
        assert fn(gpu_ctx.h, None, None, None, None, None, None, None, 0, None, A.VP(acc.data_ptr()), None, None) == 0
    for fn in (lib.rtr_gather_records, lib.rtr_gather_records_async):
        assert fn(gpu_ctx.h, None, 12, 0, None, 0, A.VP(acc.data_ptr())) == 0
    torch.cuda.synchronize()
    assert (acc == 3.0).all()
    # a refused call writes nothing
    p = api.make_accum_params(8, image_stride=8)
    T = torch.ones((8, 3), device="cuda")
    rad = torch.zeros((8, 12), device="cuda")
    assert lib.rtr_accumulate_paths(gpu_ctx.h, A.VP(rad.data_ptr()), A.VP(T.data_ptr()), None, None, None, None, None, 8, C.byref(p), A.VP(acc.data_ptr()), None, None) == -1
    assert b"rtr_accumulate_paths: imageStrideBytes 8" in lib.rtr_last_error()
    torch.cuda.synchronize()
    assert (acc == 3.0).all()


def test_the_python_wrappers(gpu_ctx):
    case = W.AccumCase(300, flags=BOTH, emitters=True, escapes=True, sky=True, bounces=True, term=True, ids="mixed", t_words=8, image_words=4, seed=26)
    want_acc, want_term, want_t = case.expected()

    def dev(x, dtype=torch.float32):
        return torch.from_numpy(x.view(np.int32).copy()).cuda().view(dtype)
    acc, term = dev(case.accum0), dev(case.term0)
    T = dev(case.T)
    out_t = api.accumulate_paths(gpu_ctx, dev(case.radiance), T[:, 0:3], acc, api.make_accum_params(case.num_slots, True, True), path_ids=dev(case.ids, torch.int32),
                                 emitters=dev(case.emitters), escapes=dev(case.escapes), sky_sums=dev(case.sky)[:, 0:3], bounces=dev(case.bounces), out_term=term)
    for got, want in ((acc, want_acc), (term, want_term), (out_t, want_t)):
        assert (got.cpu().numpy().view(np.uint32) == want.view(np.uint32)).all()
    assert api.accumulate_paths(gpu_ctx, dev(case.radiance), T, acc, api.make_accum_params(case.num_slots)) is None
    with pytest.raises(ValueError):
        api.accumulate_paths(gpu_ctx, dev(case.radiance), T, acc[:100], api.make_accum_params(case.num_slots))
    with pytest.raises(ValueError):
        api.accumulate_paths(gpu_ctx, dev(case.radiance)[:10], T, acc, api.make_accum_params(case.num_slots))
    src = dev(case.radiance)
    rows = dev(case.slots(), torch.int32)
    got = api.gather_records(gpu_ctx, src, rows)
    assert (got.cpu().numpy().view(np.uint32) == W.witness_gather(case.radiance, case.slots())).all()
    ids = api.gather_records(gpu_ctx, rows, torch.arange(299, -1, -1, dtype=torch.int32, device="cuda"))
    assert ids.dtype == torch.int32 and torch.equal(ids, rows.flip(0))


@pytest.mark.parametrize("record_bytes", [4, 32, 80])
def test_device_gather_equals_host(gpu_ctx, record_bytes):
    lib = gpu_ctx.lib
    w = record_bytes // 4
    for n in SIZES + [65537]:
        rng = np.random.default_rng(record_bytes + n)
        num_src = max(1, n - 3)
        src = rng.integers(1, 2 ** 32, (num_src, w), dtype=np.uint32)
        rows = rng.integers(0, num_src, n).astype(np.uint32)
        rows[::7] = np.resize(np.array([W.PATH_NONE, num_src, num_src + 5], np.uint32), rows[::7].size)
        want = W.witness_gather(src, rows).ravel()
        assert (api.host_gather_records(src, rows).ravel() == want).all()
        d_rows = torch.from_numpy(rows.view(np.int32)).cuda()
        for shift in (0, 1):             # shift 1: both record arrays 4 B past a multiple of 16, the one-lane-per-word path
            d_src = torch.from_numpy(np.concatenate([np.zeros(shift, np.uint32), src.ravel()]).view(np.int32)).cuda()
            out = torch.full((W.GUARD_WORDS + shift + n * w + W.GUARD_WORDS,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            at = W.GUARD_WORDS + shift
            assert (d_src.data_ptr() + 4 * shift) % 16 == 4 * shift and (out.data_ptr() + 4 * at) % 16 == 4 * shift
            rc = lib.rtr_gather_records(gpu_ctx.h, A.VP(d_src.data_ptr() + 4 * shift), record_bytes, num_src, A.VP(d_rows.data_ptr()), n, A.VP(out.data_ptr() + 4 * at))
            assert rc == 0, lib.rtr_last_error()
            got = out.cpu().numpy().view(np.uint32)
            assert (got[at:at + n * w] == want).all(), f"{n} rows of {record_bytes} B, shift {shift}"
            assert (got[:at] == 0x5A5A5A5A).all() and (got[at + n * w:] == 0x5A5A5A5A).all(), f"{n} rows of {record_bytes} B: words around the output changed"


def test_asynchronous_accumulation_on_torchs_stream_allocates_nothing():
    n = 20000
    case = W.AccumCase(n, flags=BOTH, emitters=True, escapes=True, sky=True, bounces=True, term=True, ids="permutation", seed=27)
    want_acc, want_term, want_t = case.expected()
    ctx = api.Context(0)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx.set_stream(stream.cuda_stream)

        def dev(x, dtype=torch.float32):
            return (torch.from_numpy(x.view(np.int32).copy()).cuda() + 0).view(dtype)          # torch work on the stream before the call
        rad, T, ids, em, es, sky, bo = (dev(case.radiance), dev(case.T), dev(case.ids, torch.int32), dev(case.emitters), dev(case.escapes), dev(case.sky),
                                       dev(case.bounces))
        acc, term = dev(case.accum0), dev(case.term0)
        p = api.make_accum_params(n, True, True)
        out_t = api.accumulate_paths(ctx, rad, T, acc, p, path_ids=ids, emitters=em, escapes=es, sky_sums=sky, bounces=bo, out_term=term, asynchronous=True)
        rows = api.gather_records(ctx, out_t, ids, asynchronous=True)                        # no host join in between
        got = [x.view(torch.int32) + 0 for x in (acc, term, out_t, rows)]
        stream.synchronize()
        for g, want in zip(got, (want_acc, want_term, want_t, W.witness_gather(want_t, case.ids))):
            assert (g.cpu().numpy().view(np.uint32) == want.view(np.uint32)).all()
        # the calls themselves, on buffers that exist: torch's allocator statistics do not move across a second call
        pp = case.params(A)
        out = torch.empty((n, 3), device="cuda")
        gathered = torch.empty((n, 3), device="cuda")

        def calls():
            a = (ctx.h, A.VP(rad.data_ptr()), A.VP(T.data_ptr()), A.VP(ids.data_ptr()), A.VP(em.data_ptr()), A.VP(es.data_ptr()), A.VP(sky.data_ptr()),
                 A.VP(bo.data_ptr()), n, C.byref(pp), A.VP(acc.data_ptr()), A.VP(term.data_ptr()), A.VP(out.data_ptr()))
            assert ctx.lib.rtr_accumulate_paths_async(*a) == 0, ctx.lib.rtr_last_error()
            assert ctx.lib.rtr_gather_records_async(ctx.h, A.VP(out.data_ptr()), 12, n, A.VP(ids.data_ptr()), n, A.VP(gathered.data_ptr())) == 0, ctx.lib.rtr_last_error()
        calls()
        stream.synchronize()
        stats0 = dict(torch.cuda.memory_stats())
        calls()
        stream.synchronize()
        assert dict(torch.cuda.memory_stats()) == stats0
        assert (out.cpu().numpy().view(np.uint32) == want_t.view(np.uint32)).all()
        ctx.set_stream(None)
    with pytest.raises(ValueError):
        api.accumulate_paths(ctx, rad, T, acc, p, asynchronous=True)          # the context is no longer on torch's current stream
    ctx.close()


# ---- path_trace_library ------------------------------------------------------------------------------------------------------------------
LOOPS = {"plain": api.path_trace, "picked": api.path_trace_picked, "mis": api.path_trace_mis, "sky": api.path_trace_sky, "power": api.path_trace_power}
SETTINGS = [{}, {"compact": True}, {"compact": True, "roulette_from": 1}]


def _inputs(ctx, s, scene, n_random, seed):
    cam = api.camera_rays(ctx, s.camera, 128, 128, 1)
    st = scene.stats()
    rnd = torch.from_numpy(random_rays(st.boundsMin[:], st.boundsMax[:], n_random, seed=seed)).cuda()
    rnd_seeds = torch.from_numpy(np.random.default_rng(3).integers(-2 ** 31, 2 ** 31, size=n_random).astype(np.int32)).cuda()
    return {"camera": (cam, None), "random": (rnd, rnd_seeds)}


@pytest.fixture(scope="module")
def cornell(gpu_ctx, scene_cache):
    s = scenes.cornell_box(128, 128)
    scene = api.Scene(gpu_ctx, s.desc)
    yield scene, api.make_light_params(s.num_lights, 3, 4, 128, 1), _inputs(gpu_ctx, s, scene, 20000, 51)
    scene.close()


@pytest.fixture(scope="module")
def open_box(gpu_ctx, scene_cache):
    """the Cornell box under a sky with two lights of unequal power: bounce rays leave through its open front, and meet the lights"""
    s = _box(scene_cache, UNEQUAL[:2])
    scene = api.Scene(gpu_ctx, s.desc)
    yield scene, api.make_light_params(s.num_lights, 3, 4, 128, 1), _inputs(gpu_ctx, s, scene, 20000, 52)
    scene.close()


def _assert_library_is_the_loop(scene, lp, inputs, loop, case, want_kinds=False):
    rays, seeds = inputs[case]
    n = int(rays.shape[0])
    for kw in SETTINGS:
        want = LOOPS[loop](scene, rays, lp, 2, seeds=seeds, **kw)
        got = api.path_trace_library(scene, rays, lp, 2, loop=loop, seeds=seeds, **kw)
        what = f"{loop}, {case}, {kw}"
        assert len(got.per_depth) == len(want.per_depth) == 3
        assert torch.equal(got.radiance, want.radiance), f"{what}: radiance"
        for d in range(3):
            assert tuple(got.per_depth[d].shape) == (n, 3) and torch.equal(got.per_depth[d], want.per_depth[d]), f"{what}: per_depth[{d}]"
        assert got.live == want.live, f"{what}: live {got.live}, the loop's {want.live}"
        assert (want.per_depth[1] != 0).any() and (want.per_depth[2] != 0).any(), f"{what}: the later vertices add nothing, the test shows nothing"
        if kw:
            assert 0 < want.live[2] <= want.live[1] < n, f"{what}: live = {want.live}: every path or none goes on, the test shows nothing"
    if want_kinds:                       # the masks are exercised: some bounce rays miss and some end on a light
        q = api.trace_rays(scene, rays)
        surf = api.hit_surfaces(scene, rays, q)
        b = api.bounce_rays(scene.ctx, rays, surf, api.make_bounce_params(frame=lp.frame, depth=0, width=lp.width, spp=lp.spp), seeds=seeds)
        kinds = api.hit_surfaces(scene, b.rays, api.trace_rays(scene, b.rays)).kind[b.lobe != 0]
        assert (kinds == A.SURFACE_MISS).any() and (kinds == A.SURFACE_LIGHT).any() and (kinds == A.SURFACE_OBJECT).any()


@pytest.mark.parametrize("case", ["camera", "random"])
@pytest.mark.parametrize("loop", ["plain", "picked", "mis"])
def test_library_route_is_the_torch_loop_in_the_cornell_box(cornell, loop, case):
    scene, lp, inputs = cornell
    _assert_library_is_the_loop(scene, lp, inputs, loop, case)


@pytest.mark.parametrize("case", ["camera", "random"])
@pytest.mark.parametrize("loop", ["sky", "power"])
def test_library_route_is_the_torch_loop_under_an_open_sky(open_box, loop, case):
    scene, lp, inputs = open_box
    _assert_library_is_the_loop(scene, lp, inputs, loop, case, want_kinds=True)


def test_library_route_with_picks_at_every_vertex_and_no_sky_mis(open_box):
    """the other branches of the flags: a MIS vertex at the camera, sky samples without MIS (a miss then adds nothing), and the sky loop
    without sky samples"""
    scene, lp, inputs = open_box
    rays, seeds = inputs["random"]
    for loop, kw in (("sky", {"sky_mis": False, "pick_from": 0}), ("power", {"sky_from": 1, "light_picks": 2, "compact": True}), ("sky", {"sky_samples": 0, "compact": True}),
                     ("picked", {"light_picks": 2, "pick_from": 0, "compact": True})):
        want = LOOPS[loop](scene, rays, lp, 2, seeds=seeds, **kw)
        got = api.path_trace_library(scene, rays, lp, 2, loop=loop, seeds=seeds, **kw)
        assert torch.equal(got.radiance, want.radiance) and got.live == want.live, f"{loop}, {kw}"
        assert all(torch.equal(a, b) for a, b in zip(got.per_depth, want.per_depth)), f"{loop}, {kw}"
