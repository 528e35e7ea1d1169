"""The queued occlusion query (rtr_trace_occlusion and its hinted, masked and filtered forms) at the shapes that decide how its launch
is cut up — tests/shape_cases.py's EDGES and octant layouts, held to the source's constants by tests/test_shape_constants.py:
  * ray counts on both sides of the wave, the batch, the queue build's block and chunk, and nine chunks plus one ray;
  * octant layouts: one octant for a whole launch (the longest lists the list stride must hold), runs that end on, before and behind a
    wave, exact batch ends inside a chunk, nine batches of one octant per chunk, one live ray per octant among dead ones;
  * nothing to walk at all, and one live ray at a chunk's first and last place;
  * guard bytes around the scratch and the answers of raw calls;
  * the 512-ray batch of launches of 100 << 20 rays and more.
Every comparison is at tolerance 0, against multihit_witness.all_hits32's bytes; witness.ray_hits (float64) must agree wherever it is sure."""
import time

import numpy as np
import pytest
import torch

from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api

import shape_cases as SC
from shape_cases import assert_same_bytes

pytestmark = pytest.mark.gpu

PATTERN = 0xA5


@pytest.fixture(scope="module")
def world(gpu_ctx):
    return SC.world(gpu_ctx)


def both_forms(what, n_well_formed, exp, **kw):
    """the timed and the counting form of one query: the expected bytes, and the well-formed rays counted"""
    for collect in (False, True):
        r = api.trace_occlusion(collect_stats=collect, **kw)
        assert_same_bytes(r.occluded, exp, f"{what}, {'counting' if collect else 'timed'} form")
        if collect:
            assert r.stats.numRays == n_well_formed, f"{what}: numRays {r.stats.numRays} != {n_well_formed} well-formed rays"


# ---- 1. counts ------------------------------------------------------------------------------------------------------------------------
FORMS = ("plain", "hinted_zeros", "hinted_garbage", "masked_0xff", "cull_no_opaque")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", SC.EDGES)
def test_counts(world, n, form):
    what = f"{n} rays, {form} [{world.ref.check(n)}]"
    rays = world.rays_t[:n]
    exp = world.ref.occluded[:n]
    kw = dict(scene=world.scene, rays=rays)
    if form == "hinted_zeros":
        kw["start_leaves"] = torch.zeros(n, dtype=torch.int32, device="cuda")
    elif form == "hinted_garbage":          # any value is safe and none changes a byte
        g = torch.Generator(device="cuda").manual_seed(n)
        kw["start_leaves"] = torch.randint(-(1 << 31), (1 << 31) - 1, (n,), dtype=torch.int64, device="cuda", generator=g).to(torch.int32)
    elif form == "masked_0xff":
        kw["cull_mask"], kw["ray_masks"] = 0xff, torch.full((n,), 0xff, dtype=torch.uint8, device="cuda")
    elif form == "cull_no_opaque":          # the filtered forms; nothing in this scene is alpha-tested
        kw["ray_flags"] = A.QUERY_CULL_NO_OPAQUE
    both_forms(what, n, exp, **kw)
    assert_same_bytes(api.trace_rays(world.scene, rays, any_hit=True).occluded, exp, f"{what}: the dense query")


# ---- 2. octant layouts ----------------------------------------------------------------------------------------------------------------
def _one_per_octant(n):
    """per chunk one ray of each octant, 512 apart (one in every wave's share), the 4088 others dead"""
    want = np.full(n, -1, np.int64)
    at = np.arange(0, n, SC.GEN_BLOCK)
    want[at] = at // SC.GEN_BLOCK % 8
    return want


LAYOUTS = {f"octant_{o}": (lambda n, o=o: np.full(n, o, np.int64)) for o in range(8)}
LAYOUTS.update({
    "runs_of_64": lambda n: SC.runs(n, 64), "runs_of_63": lambda n: SC.runs(n, 63), "runs_of_65": lambda n: SC.runs(n, 65),
    "i_mod_8": lambda n: np.arange(n) % 8,
    "255_of_octant_5_per_chunk": lambda n: SC.chunk_counts(n, 5, SC.BATCH - 1, 2),
    "256_of_octant_5_per_chunk": lambda n: SC.chunk_counts(n, 5, SC.BATCH, 2),
    "257_of_octant_5_per_chunk": lambda n: SC.chunk_counts(n, 5, SC.BATCH + 1, 2),
    "nine_batches_of_octant_3_per_chunk": lambda n: SC.chunk_counts(n, 3, SC.REGIONS * SC.BATCH + 1, 6),
    "one_ray_per_octant_among_dead": _one_per_octant,
})


@pytest.mark.parametrize("n", [SC.MASTER, SC.GEN_RAYS + 1])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_octant_layouts(world, name, n):
    want = LAYOUTS[name](n)
    idx = SC.layout(world.octants, want)
    rays = world.rays[idx].copy()
    exp = world.ref.occluded[idx].copy()
    dead = want < 0
    SC.kill(rays, dead, "mixed")
    exp[dead] = 0
    live = ~dead
    assert (SC.octant_of(rays)[live] == want[live]).all()
    what = f"{name}, {n} rays [{world.ref.describe()}]"
    if live.sum() >= SC.WAVE - 1:
        assert SC.OCCLUDED_SHARE[0] <= exp[live].mean() <= SC.OCCLUDED_SHARE[1], f"{what}: occluded share of the layout {exp[live].mean():.3f}"
    assert world.ref.ambiguous[idx][live].mean() <= SC.AMBIGUOUS_CAP, what
    both_forms(what, int(SC.well_formed(rays).sum()), exp, scene=world.scene, rays=torch.from_numpy(rays).cuda())


# ---- 3. nothing to walk ---------------------------------------------------------------------------------------------------------------
NOTHING = 2 * SC.GEN_RAYS
ONE_LIVE = (None, 0, SC.GEN_RAYS - 1, SC.GEN_RAYS, NOTHING - 1)


@pytest.mark.parametrize("live_at", ONE_LIVE, ids=lambda x: "none_live" if x is None else f"live_at_{x}")
@pytest.mark.parametrize("kind", SC.DEAD_KINDS + ("mixed", "cull_mask_0", "ray_masks_0"))
def test_nothing_to_walk(world, kind, live_at):
    """with no batch in any list every wave of the walk falls through all 64 lists and leaves; with one batch of one ray, one wave takes
    it and the others leave"""
    rays = world.rays[:NOTHING].copy()
    exp = np.zeros(NOTHING, np.uint8)
    occluded_ray = world.rays[int(np.nonzero(world.ref.occluded)[0][0])]
    kw = {}
    if kind == "cull_mask_0" and live_at is None:
        kw["cull_mask"] = 0
    elif kind in ("cull_mask_0", "ray_masks_0"):
        masks = np.zeros(NOTHING, np.uint8)
        if live_at is not None:
            masks[live_at] = 0x10
        kw["cull_mask"], kw["ray_masks"] = (0x10 if kind == "cull_mask_0" else 0xff), torch.from_numpy(masks).cuda()
    else:
        SC.kill(rays, slice(None), kind)
    if live_at is not None:
        rays[live_at] = occluded_ray
        exp[live_at] = 1
    what = f"{NOTHING} rays, {kind}, live ray at {live_at}"
    rt = torch.from_numpy(rays).cuda()
    both_forms(what, int(SC.well_formed(rays).sum()), exp, scene=world.scene, rays=rt, **kw)
    assert_same_bytes(api.trace_rays(world.scene, rt, any_hit=True, **kw).occluded, exp, f"{what}: the dense query")


# ---- 4. guards ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["rtr_trace_occlusion", "rtr_trace_occlusion_hinted", "rtr_trace_occlusion_masked"])
@pytest.mark.parametrize("n", [1, 65, 257, 4097])
def test_raw_calls_stay_inside_their_scratch_and_answers(gpu_ctx, world, n, entry):
    """scratch of exactly rtr_occlusion_scratch_bytes(n) and n answer bytes, each carved out of a larger tensor of a pattern"""
    lib = gpu_ctx.lib
    need = api.occlusion_scratch_bytes(lib, n)
    s_off, o_off = 4096, 48
    scratch = torch.full((s_off + need + 4096,), PATTERN, dtype=torch.uint8, device="cuda")
    occ = torch.full((o_off + n + 256,), PATTERN, dtype=torch.uint8, device="cuda")
    assert (scratch.data_ptr() + s_off) % 16 == 0 and (occ.data_ptr() + o_off) % 16 == 0
    rays = world.rays_t[:n].contiguous()
    hints = torch.full((n,), 0x7fffffff, dtype=torch.int32, device="cuda")
    masks = torch.full((n,), 0xff, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    tail = (A.VP(scratch.data_ptr() + s_off), need, A.VP(occ.data_ptr() + o_off), None)
    rp = A.VP(rays.data_ptr())
    if entry == "rtr_trace_occlusion":
        args = (rp, n, 0) + tail
    elif entry == "rtr_trace_occlusion_hinted":
        args = (rp, A.VP(hints.data_ptr()), n, 0) + tail
    else:
        args = (rp, A.VP(hints.data_ptr()), A.VP(masks.data_ptr()), n, 0, 0xff) + tail
    assert getattr(lib, entry)(gpu_ctx.h, world.scene.h, *args) == 0, lib.rtr_last_error()
    what = f"{entry}, {n} rays"
    assert_same_bytes(occ[o_off:o_off + n], world.ref.occluded[:n], what)
    for name, buf, lo, hi in (("scratch", scratch, s_off, s_off + need), ("occluded", occ, o_off, o_off + n)):
        assert bool((buf[:lo] == PATTERN).all()), f"{what}: bytes before {name} were written"
        assert bool((buf[hi:] == PATTERN).all()), f"{what}: bytes behind {name} were written"


# ---- 5. the 512-ray batch -------------------------------------------------------------------------------------------------------------
TILE = 2 * SC.GEN_RAYS


@pytest.mark.parametrize("n", [SC.BIG_BATCH_FROM - 1, SC.BIG_BATCH_FROM], ids=["below_the_512_batch", "the_512_batch"])
def test_the_long_batch(world, n):
    """100 << 20 rays is the smallest launch whose batches are 512 rays, and one less the largest whose batches are 256: the first 8192
    master rays tiled on the device (3.4 GB of rays, 0.5 GB of scratch on a context of its own, freed at once)"""
    assert SC.BIG_BATCH_FROM % TILE == 0
    ctx = api.Context(0)
    try:
        rays = world.rays_t[:TILE].repeat(SC.BIG_BATCH_FROM // TILE, 1)[:n]
        exp = torch.from_numpy(world.ref.occluded[:TILE]).cuda().repeat(SC.BIG_BATCH_FROM // TILE)[:n]
        assert rays.is_contiguous() and rays.shape == (n, 8)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = api.trace_occlusion(world.scene, rays, ctx=ctx)
        torch.cuda.synchronize()
        secs = time.perf_counter() - t0
        print(f"\ntrace_occlusion of {n} rays: {secs * 1e3:.1f} ms")
        same = torch.equal(r.occluded, exp)
        wrong = 0 if same else int((r.occluded != exp).sum())
        values = torch.unique(r.occluded).tolist()
        del r, rays, exp
        assert same, f"{n} rays: {wrong} bytes differ"
        assert set(values) <= {0, 1}
    finally:
        ctx._occlusion_scratch = None
        ctx.close()
        torch.cuda.empty_cache()
