"""The multi-hit query (rtr_trace_rays_multi; k_multihit, k_multihit_tail) where its per-lane state is stressed and the well-behaved
scenes of tests/test_gpu_multihit.py do not reach: ties in t deeper than any K, chains that start and end inside a tie, resume keys no
call produced, windows whose tmin / tmax sit on a surface, every one of the nine compiled walks with a full list, trees of 1, 2, 8 and 9
triangles, the tail kernel at K = 8 and K = 1, and scenes that were refitted, rebuilt or moved before the query.  Every comparison is
assert_slots — all 8 words of every slot of every ray, and the counts — against multihit_witness.first_k over all_hits32; no
tolerance anywhere.  tests/test_multihit_edges_abi.py holds the constructions to their design without a device."""
import numpy as np
import pytest
import torch

import multihit_witness as M
import ray_flags_witness as W
import test_gpu_vertex_update as vu
from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api
from test_gpu_bvh import _with_flags
from test_gpu_cull_masks import by_custom, counters, seeded_masks
from test_gpu_multihit import BUILDS, assert_slots
from test_gpu_occlusion import mixed_rays
from deep_scene import _deep_scene
from test_gpu_rebuild_async import device_scene, prepared, status
from test_gpu_rebuild_if import policy_scene
from test_gpu_update_async import _filler, async_twin, on_device
from test_gpu_vertex_update import changed_ranges, made, query_rays

pytestmark = pytest.mark.gpu

F32 = np.float32
SAH, LBVH = A.BUILD_HOST_SAH, A.BUILD_DEVICE_LBVH
BACK = A.QUERY_CULL_BACK_FACING
INF = float("inf")
MAX_LINKS = 64

_stack = {}


@pytest.fixture(scope="module", autouse=True)
def _cleanup():
    yield
    for m in vu._made.values():
        m["scene"].close(); m["fresh"].close()
    vu._made.clear(); vu._setups.clear()
    for k, v in _stack.items():
        if isinstance(k, int):
            v["scene"].close()
    _stack.clear()


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def sorted_records(bvh):
    raw = np.frombuffer(bvh[1], dtype=np.uint32).reshape(-1, 12)
    return raw[np.lexsort((raw[:, 7], raw[:, 3]))].tobytes()


def stack_of(ctx, build):
    """the tie-stack scene by one builder, its rays, and the witness: all_hits32 once, shared by both builders (first_k sorts, so the
    list depends on the records only, and the two builders' records are compared as sets)"""
    if build not in _stack:
        desc, keep = M.tie_stack_scene()
        scene = api.Scene(ctx, _with_flags(desc, build))
        bvh = scene.export_bvh()
        if "wit" not in _stack:
            rays, kinds = M.tie_stack_rays()
            cands = M.all_hits32(bvh, rays)
            classes = M.trivial_classes(cands)
            _stack["wit"] = {"rays": rays, "kinds": kinds, "cands": cands, "classes": classes, "lists": M.accepted(cands, classes, rays, 0),
                             "records": sorted_records(bvh), "rt": torch.from_numpy(rays).cuda()}
        assert sorted_records(bvh) == _stack["wit"]["records"], "both builders flatten the same records"
        st = scene.stats()
        assert st.numTriangles == 88
        print(f"tie stack, build flags {build}: depth {st.maxDepth}, {st.numNodes} nodes, stack class {st.stackEntries}")
        _stack[build] = {"scene": scene, "desc": desc, "keep": keep, "bvh": bvh, "depth": st.maxDepth}
    return {**_stack["wit"], **_stack[build]}


def expect(s, K, sel=None, after=None):
    """first_k over the shared lists, for the rays sel (an index array or None for all)"""
    rays, lists = s["rays"], s["lists"]
    if sel is not None:
        rays, lists = rays[sel], [lists[k] for k in sel]
    return M.first_k(None, None, rays, K, 0, after=after, lists=lists)


def both_forms(scene, rt, K, exp, what, **kw):
    """the timed form and the counting form — different instantiations — against one expectation"""
    res = api.trace_rays_multi(scene, rt, K, **kw)
    assert_slots(res, exp, what)
    cnt = api.trace_rays_multi(scene, rt, K, collect_stats=True, **kw)
    assert_slots(cnt, exp, f"{what}, counting form")
    return res, cnt


def key_of(h, k, j):
    return (h[k, j, 0:1].view(F32)[0], int(h[k, j, 3]), int(h[k, j, 4]))


def customs_by_z(desc):
    out = {}
    for i in range(desc.numInstances):
        out.setdefault(float(desc.instances[i].transform[11]), []).append(int(desc.instances[i].customIndex))
    return {z: sorted(c) for z, c in out.items()}


# ---- 3.1 ties deeper than K ---------------------------------------------------------------------------------------------------------
@BUILDS
def test_ties_deeper_than_k(gpu_ctx, build):
    """20 (through the shared diagonal: 40) records on one t, more than any K: once the list is full its limit IS the tie's t, and a
    record met later with a smaller id must push the last one out.  All ray groups of tie_stack_rays, K = 1 .. 8, both forms.
    The tree's depth: 6 by the host SAH builder (19 nodes), 7 by the device LBVH builder (87 nodes: identical centroids are split by
    index, one record per leaf) — inside the 16-entry stack, so no ray of this scene takes the tail kernel (asserted: tailRays == 0)."""
    s = stack_of(gpu_ctx, build)
    scene, rays, kinds, rt = s["scene"], s["rays"], s["kinds"], s["rt"]
    per_t = np.array([max(np.unique([e[0][0] for e in lst], return_counts=True)[1]) if lst else 0 for lst in s["lists"]])
    for kind in (M.KIND_UP, M.KIND_DOWN):
        assert ((per_t > 8) & (kinds == kind)).sum() >= 100, "at least 100 rays per direction have more than 8 accepted records on a single t"
    raw = np.frombuffer(s["bvh"][1], dtype=np.uint32).reshape(-1, 12)
    for z in M.TIE_Z:                                       # in THIS builder's storage order a smaller customIndex sits behind a larger one
        order = raw[raw.view(F32)[:, 2] == F32(z), 3].tolist()
        assert any(a > b for a, b in zip(order, order[1:]))
    tails = 0
    for K in range(1, 9):
        _, cnt = both_forms(scene, rt, K, expect(s, K), f"tie stack K = {K}")
        assert cnt.stats.numRays == len(rays)
        tails += cnt.stats.tailRays
    print(f"tie stack, build flags {build}: tailRays over K = 1 .. 8: {tails}")
    assert s["depth"] <= 16 and tails == 0, "the docstring says that no ray of this scene takes the tail kernel"
    # whatever the permutation: behind the two single layers a through ray reports the smallest ids of the first tie, and a window
    # that opens ON the single layer in front of the tie reports the tie's three smallest at K = 3
    by_z = customs_by_z(s["desc"])
    thru = M.grid_inside(rays) & (rays[:, 0] != rays[:, 1])
    k5 = _np(api.trace_rays_multi(scene, rt, 5).custom_index)
    win = M.WINDOWS.index((0.25, 1.25))
    k3 = _np(api.trace_rays_multi(scene, rt, 3).custom_index)
    first_window = np.nonzero(kinds == M.KIND_WINDOW)[0][0]
    for kind, z, singles in ((M.KIND_UP, 0.5, 2), (M.KIND_DOWN, 1.0, 1)):      # single layers in front of the first tie: z = 0 and 0.25; z = 1.25
        rows = np.nonzero(thru & (kinds == kind))[0]
        assert len(rows) >= 100 and (k5[rows, singles:singles + 3] == by_z[z][:3]).all(), "K = 5: behind the single layers, the three smallest customIndices of the first tie"
        rows = first_window + 64 * win + 32 * (kind == M.KIND_DOWN) + np.arange(32)
        rows = rows[thru[rows]]
        assert len(rows) >= 20 and (k3[rows] == by_z[z][:3]).all(), "K = 3 behind the single layer: the three smallest customIndices of the tie"


# ---- 3.2 chains through ties --------------------------------------------------------------------------------------------------------
@BUILDS
def test_chains_through_ties(gpu_ctx, build):
    """K = 1, 3 and 8 chained to exhaustion: the concatenation is accepted(...) exactly — every record once, none twice, in order — and
    at K = 3 EVERY link is first_k(after = the previous link's last slot): 20 and 40 are no multiples of 3, so links start and end inside
    the ties.  At most 64 links; a ray through the shared diagonal has 88 records, which K = 1 cannot enumerate in 64 links, so the K = 1
    chain runs over the rays with fewer than 64 records (every ray off the diagonal: 44, and the shorter windows), the others over all
    rays."""
    s = stack_of(gpu_ctx, build)
    scene, lists = s["scene"], s["lists"]
    sizes = np.array([len(x) for x in lists])
    for K in (1, 3, 8):
        sel = np.nonzero(sizes < MAX_LINKS)[0] if K == 1 else np.arange(len(lists))
        assert len(sel) >= 1500 and (44 <= sizes[sel].max() < MAX_LINKS if K == 1 else sizes[sel].max() == 88)
        rt = s["rt"][torch.from_numpy(sel).cuda()].contiguous()
        seen = [[] for _ in sel]
        res, after, after_t, links, inside_tie = api.trace_rays_multi(scene, rt, K), None, None, 0, 0
        for _ in range(MAX_LINKS):
            c = _np(res.counts)
            if K == 3:                                       # every link, the one that finds nothing included
                assert_slots(res, expect(s, K, sel, after), f"K = 3 link {links}")
                assert torch.equal(api.trace_rays_multi(scene, rt, K, after=after_t, collect_stats=True).hits, res.hits), f"K = 3 link {links}, counting form"
            if not c.any():
                break
            links += 1
            h = _np(res.hits).view(np.uint32)
            for k in np.nonzero(c)[0]:
                for j in range(int(c[k])):
                    seen[k].append((key_of(h, k, j), h[k, j, 1], h[k, j, 2]))
            if K == 3:                                       # does a link end inside a tie? its last key's t is also the next record's
                inside_tie += sum(1 for k in np.nonzero(c == K)[0] if len(seen[k]) < sizes[sel[k]] and lists[sel[k]][len(seen[k])][0][0] == seen[k][-1][0][0])
            after, after_t = _np(res.last), res.last
            res = api.trace_rays_multi(scene, rt, K, after=res)
        else:
            raise AssertionError(f"K = {K}: the chain did not end in {MAX_LINKS} links")
        assert not _np(res.counts).any() and (_np(res.custom_index) == -1).all()
        assert links == -(-int(sizes[sel].max()) // K)
        for k, got in zip(sel, seen):
            exp = lists[k]
            assert [g[0] for g in got] == [e[0] for e in exp], f"K = {K} ray {k}: {[g[0] for g in got][:6]} ... against {[e[0] for e in exp][:6]} ..."
            assert [(g[1], g[2]) for g in got] == [(np.array([e[1]], F32).view(np.uint32)[0], np.array([e[2]], F32).view(np.uint32)[0]) for e in exp]
        if K == 3:
            assert inside_tie > 1000, "links end (and the next ones start) inside a tie"


# ---- 3.3 foreign resume keys --------------------------------------------------------------------------------------------------------
@BUILDS
def test_foreign_resume_keys(gpu_ctx, build):
    """`after` records no call produced, for every ray of the two through grids: the interface defines the result for any key"""
    s = stack_of(gpu_ctx, build)
    scene, kinds = s["scene"], s["kinds"]
    sel = np.nonzero(kinds <= M.KIND_DOWN)[0]
    rays = s["rays"][sel]
    rt = s["rt"][torch.from_numpy(sel).cuda()].contiguous()
    up = kinds[sel] == M.KIND_UP
    by_z = customs_by_z(s["desc"])
    lone = by_z[0.75][0]                                     # a customIndex of the scene that no record of a tie carries
    want = [c for c in by_z[0.5] if c > lone][:8]
    assert lone not in by_z[0.5] + by_z[1.0] and 0 < len(want) and min(by_z[0.5]) < lone, "the foreign key falls INSIDE the tie's id range"

    def t_at(z):
        return np.where(up, F32(z - M.UP_Z), F32(M.DOWN_Z - z)).astype(F32)

    def keys(t, custom, prim):
        rec = np.zeros((len(rays), 8), np.uint32)
        rec[:, 0], rec[:, 3], rec[:, 4] = np.broadcast_to(np.asarray(t, F32), (len(rays),)).view(np.uint32), custom, prim
        return rec.view(np.int32)

    cases = {"a t strictly between two layers": keys(t_at(0.625), 0, 0),
             "the tie's t, a customIndex of another layer": keys(t_at(0.5), lone, 0),
             "the tie's t, a customIndex the scene does not have": keys(t_at(1.0), len(M.TIE_STACK_Z), 0),
             "the tie's t, ids 0xfffffffe": keys(t_at(0.5), 0xfffffffe, 0xfffffffe),
             "the second tie's t, ids 0xfffffffe": keys(t_at(1.0), 0xfffffffe, 0xfffffffe),
             "the tie's t, customIndex 0, primitiveId 0": keys(t_at(0.5), 0, 0),
             "the second tie's t, customIndex 0, primitiveId 0": keys(t_at(1.0), 0, 0),
             "t = -inf": keys(-np.inf, 0, 0), "t = +inf": keys(np.inf, 0, 0)}
    plain = expect(s, 8, sel)
    for what, rec in cases.items():
        for K in (3, 8):
            exp = expect(s, K, sel, after=rec)
            both_forms(scene, rt, K, exp, f"after = {what}, K = {K}", after=torch.from_numpy(rec).cuda())
            if what == "t = -inf" and K == 8:
                assert (exp[0] == plain[0]).all(), "(-inf, 0, 0) is the key of a call without `after`"
            if what == "t = +inf":
                assert not exp[1].any(), "nothing lies behind +inf"
            elif K == 8:
                assert exp[1].any()
    cut = expect(s, 8, sel, after=cases["the tie's t, a customIndex of another layer"])[0]
    inside = M.grid_inside(rays) & (rays[:, 0] != rays[:, 1])
    assert (inside & up).sum() >= 100 and (cut[inside & up][:, :len(want), 3] == want).all(), "the key cuts the tie by its customIndex"


# ---- 3.4 windows --------------------------------------------------------------------------------------------------------------------
@BUILDS
def test_windows_that_open_and_close_on_a_surface(gpu_ctx, build):
    """tmin, tmax or both exactly on a layer's t (both ties, single layers, and tmin == tmax): both bounds are exclusive"""
    s = stack_of(gpu_ctx, build)
    scene = s["scene"]
    sel = np.nonzero(s["kinds"] == M.KIND_WINDOW)[0]
    assert len(sel) == 64 * len(M.WINDOWS)
    rt = s["rt"][torch.from_numpy(sel).cuda()].contiguous()
    for K in (1, 2, 8):
        exp = expect(s, K, sel)
        res, _ = both_forms(scene, rt, K, exp, f"windows K = {K}")
        if K == 1:
            closest = api.trace_rays(scene, rt, cull_mask=0xff)
            assert torch.equal(res.hits.view(-1, 8), closest.hits), "K = 1 is the closest-hit query in a window too"
            assert 0 < int(exp[1].sum()) < len(sel)
    empty = 64 * M.WINDOWS.index((0.5, 0.5))
    assert not expect(s, 8, sel)[1][empty:empty + 64].any(), "tmin == tmax: an empty interval"


# ---- 3.5 ray counts across the wave -------------------------------------------------------------------------------------------------
@BUILDS
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_ray_counts_across_the_wave(gpu_ctx, build, n):
    """the first n rays of the sign-pattern group alone: a partial wave, a full one, one lane of a second, a third"""
    s = stack_of(gpu_ctx, build)
    scene = s["scene"]
    group = s["rt"][M.SIGNS_FIRST:M.SIGNS_FIRST + 9 * 64].contiguous()
    sel = np.arange(M.SIGNS_FIRST, M.SIGNS_FIRST + 9 * 64)
    for K in (3, 8):
        full = api.trace_rays_multi(scene, group, K)
        assert_slots(full, expect(s, K, sel), f"the nine runs, K = {K}")
        assert int(full.counts.min()) == K, "every ray of the nine runs fills its list"
        for stats in (False, True):
            part = api.trace_rays_multi(scene, group[:n].contiguous(), K, collect_stats=stats)
            assert part.hits.shape == (n, K, 8)
            assert torch.equal(part.hits, full.hits[:n]) and torch.equal(part.counts, full.counts[:n]), f"n = {n}, K = {K}, counting form {stats}"


# ---- 3.6 tiny trees -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntri", [1, 2, 8, 9])
def test_tiny_trees(gpu_ctx, ntri):
    """1, 2, 8 and 9 triangles (fewer than 16: the host builder whatever the flag), all but one tied in t: the duplicate guard of the
    walk must drop the record a one-leaf tree names twice and nothing else"""
    desc, keep = M.tiny_scenes()[ntri]
    scene = api.Scene(gpu_ctx, desc)
    rays = M.tiny_rays()
    rt = torch.from_numpy(rays).cuda()
    bvh = scene.export_bvh()
    assert scene.stats().numTriangles == ntri
    cands = M.all_hits32(bvh, rays)
    lists = M.accepted(cands, M.trivial_classes(cands), rays, 0)
    sizes = np.array([len(x) for x in lists])
    assert set(sizes.tolist()) == {0, ntri} and (sizes == ntri).sum() >= 10 and (sizes == 0).sum() >= 40
    for K in (1, 2, 8):
        both_forms(scene, rt, K, M.first_k(None, None, rays, K, 0, lists=lists), f"{ntri} triangles, K = {K}")
    res, after, seen = api.trace_rays_multi(scene, rt, 3), None, np.zeros(len(rays), np.int64)
    for link in range(MAX_LINKS):
        both_forms(scene, rt, 3, M.first_k(None, None, rays, 3, 0, after=after, lists=lists), f"{ntri} triangles, K = 3 link {link}", after=None if after is None else torch.from_numpy(after).cuda())
        c = _np(res.counts)
        if not c.any():
            break
        seen += c
        after = _np(res.last)
        res = api.trace_rays_multi(scene, rt, 3, after=res)
    else:
        raise AssertionError("the chain did not end")
    assert (seen == sizes).all() and link == -(-ntri // 3)
    if ntri == 1:
        ch = np.frombuffer(bvh[0], dtype=np.int32).reshape(-1, 8)[0, 6:8]
        assert ch[0] == ch[1] < 0, "the root's two children name the same leaf: the case the dup branch exists for"
        thru = np.nonzero(sizes == 1)[0]
        for K in range(1, 9):
            for stats in (False, True):
                r = api.trace_rays_multi(scene, rt, K, collect_stats=stats)
                assert (_np(r.counts)[thru] == 1).all(), f"K = {K}: the one triangle is reported exactly once"
                assert (_np(r.custom_index)[thru, 1:] == -1).all()
    scene.close()


# ---- 3.7 the tail kernel at the ends of K -------------------------------------------------------------------------------------------
def test_the_tail_kernel_at_the_ends_of_k(gpu_ctx):
    """k_multihit_tail with the largest list (K = 8: its own dynamic LDS of 64 * 5 * 8 words), with K = 1, each also resumed, and with
    ray masks and a facing flag.  No ray of this scene has 8 accepted records, so behind a K = 8 call every ray is exhausted and walks
    nothing: both resumed runs start behind the CLOSEST hit (after = the K = 1 result), where the tail rays have a walk left to do.
    The compared subset — the only one in this file — is at most 64 rays that took the tail kernel at K = 8, found as
    tests/test_gpu_multihit.py finds them.  A launch of this scene walks for a good tenth of a second, so each run is two launches: all
    rays in the timed form, and the compared rays alone in the counting form, whose tailRays shows that the tail kernel is what
    answered them in THAT run; K = 1, which is held to the closest-hit query's counters, also counts all rays."""
    d, keep, scene, cam = _deep_scene(gpu_ctx)
    rays = api.camera_rays(gpu_ctx, cam, 16, 8, 2)
    n = rays.shape[0]
    rn = _np(rays)

    def tail_count(idx):
        return api.trace_rays_multi(scene, rays[torch.from_numpy(idx).to(rays.device)].contiguous(), 8, collect_stats=True).stats.tailRays

    tail = M.tail_rays(tail_count, n)
    assert tail, "some rays must take the tail kernel"
    ti = torch.tensor(tail, device=rays.device)
    sub, sub_t = rn[tail], rays[ti].contiguous()
    bvh = scene.export_bvh()
    cands = M.all_hits32(bvh, sub)
    assert any(len(c[0]) for c in cands), "some tail ray must hit"
    raw = np.frombuffer(bvh[1], dtype=np.uint32).reshape(-1, 12)          # classify looks records up by their ids: hand it the candidates' only
    ids = np.unique(np.array([(c << 32) | p for cand in cands for c, p in zip(cand[3], cand[4])], np.uint64))
    mine = raw[np.isin((raw[:, 3].astype(np.uint64) << np.uint64(32)) | raw[:, 7], ids)]
    classes = W.classify(cands, sub, (None, mine.tobytes()), W.mirrored_by_custom(d), W.AlphaWitness(d))

    def run(K, what, after=None, flags=0, wkw={}, all_counted=False, **kw):
        """all rays in the timed form and its tail subset against first_k; then the subset alone in the counting form: a counted run
        that must go through k_multihit_tail and give the same records.  all_counted: all rays in the counting form too."""
        timed = api.trace_rays_multi(scene, rays, K, after=after, ray_flags=flags, **kw)
        exp = M.first_k(cands, classes, sub, K, flags, after=None if after is None else _np(after)[tail], **wkw)
        got = api.MultiHitResult()
        got.hits, got.counts = timed.hits[ti], timed.counts[ti]
        assert_slots(got, exp, f"{len(tail)} tail rays, {what}")
        skw = {k: (v[ti].contiguous() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
        alone = api.trace_rays_multi(scene, sub_t, K, after=None if after is None else after[ti].contiguous(), collect_stats=True, ray_flags=flags, **skw)
        assert alone.stats.tailRays > 0 and alone.stats.numRays == len(tail), f"{what}: none of the compared rays took the tail kernel in this run"
        assert_slots(alone, exp, f"{len(tail)} tail rays alone, counting form, {what}")
        timed.stats = alone.stats
        if all_counted:
            cnt = api.trace_rays_multi(scene, rays, K, after=after, collect_stats=True, ray_flags=flags, **kw)
            assert cnt.stats.tailRays > 0 and cnt.stats.numRays == n, f"{what}: the rays must go through k_multihit_tail"
            assert torch.equal(timed.hits, cnt.hits) and torch.equal(timed.counts, cnt.counts), f"{what}: the counting form"
            timed.stats = cnt.stats
        return timed, exp

    closest = api.trace_rays(scene, rays, collect_stats=True, cull_mask=0xff)
    r8, e8 = run(8, "K = 8")
    assert (e8[1] > 0).any(), "some tail ray must hit"
    assert torch.equal(r8.hits[:, 0, :], closest.hits), "slot 0 of K = 8 is the closest hit, for all rays"
    assert int(r8.counts.max()) < 8, "premise of the docstring: behind a K = 8 call every ray is exhausted"
    r1, _ = run(1, "K = 1", all_counted=True)
    assert torch.equal(r1.hits.view(-1, 8), closest.hits) and counters(r1.stats) == counters(closest.stats), "K = 1 is the closest-hit query, for all rays"
    n8, _ = run(8, "K = 8 resumed behind the closest hit", after=r1.last)
    assert torch.equal(n8.hits[:, :7, :], r8.hits[:, 1:, :]), "K = 8 resumed behind the closest hit is slots 1 .. 7 of K = 8, for all rays"
    n1, _ = run(1, "K = 1 resumed behind the closest hit", after=r1.last)
    assert torch.equal(n1.hits[:, 0, :], r8.hits[:, 1, :]), "K = 1 resumed behind the closest hit is slot 1 of K = 8, for all rays"
    print(f"deep scene: {len(tail)} compared tail rays; tailRays among them K = 8: {r8.stats.tailRays}, resumed {n8.stats.tailRays}; K = 1 resumed {n1.stats.tailRays}; "
          f"among all {n} rays at K = 1: {r1.stats.tailRays}")
    # ray masks and a facing flag
    im = np.array([0x11, 0xfe], np.uint8)
    scene.set_instance_masks(im)
    rm = seeded_masks(n, 7)
    rm[np.array(tail)[::2]] |= 0x10                                    # half of the compared rays see both instances for sure
    rmt = torch.from_numpy(rm).cuda()
    mk, _ = run(8, "K = 8, ray masks, back faces culled", flags=BACK, wkw=dict(custom_masks=by_custom(d, im), ray_masks=rm[tail].astype(np.int64)), ray_masks=rmt)
    masked = api.trace_rays(scene, rays, ray_masks=rmt, ray_flags=BACK)
    assert torch.equal(mk.hits[:, 0, :], masked.hits), "slot 0 under masks and the flag is the closest-hit query's, for all rays"
    assert not torch.equal(mk.hits, r8.hits)
    scene.close()


# ---- 3.8 tree independence after every kind of change -------------------------------------------------------------------------------
def two_links(scene, rt, K, flags=0, **kw):
    """a call and a second link behind it, in both forms"""
    out = []
    after = None
    for _ in range(2):
        res = api.trace_rays_multi(scene, rt, K, after=after, ray_flags=flags, **kw)
        cnt = api.trace_rays_multi(scene, rt, K, after=after, ray_flags=flags, collect_stats=True, **kw)
        assert torch.equal(res.hits, cnt.hits) and torch.equal(res.counts, cnt.counts), "the counting form"
        out.append(res)
        after = res.last
    return out


def assert_routes_agree(routes, rays, bvh, desc, masks, rm, before):
    """every route gives first_k's bytes — computed once, from the fresh SAH scene's export — at K = 4 with a second link behind it,
    with ray_flags = 0 and with back faces culled under seeded ray masks and cullMask 0xb7; `before`: a scene that did NOT take the
    change, whose answers must differ.  Few rays of these scenes have more than 4 accepted records, so the pair is also run at K = 2,
    where the second link has records to report."""
    rt, rmt = torch.from_numpy(rays).cuda(), torch.from_numpy(rm).cuda()
    cands = M.all_hits32(bvh, rays)
    classes = W.classify(cands, rays, bvh, W.mirrored_by_custom(desc), W.AlphaWitness(desc))
    cm = by_custom(desc, masks)
    runs = [("no flags", 0, {}, dict(custom_masks=cm)),
            ("back faces culled, ray masks", BACK, dict(cull_mask=0xb7, ray_masks=rmt), dict(custom_masks=cm, ray_masks=rm.astype(np.int64) & 0xb7))]
    for what, flags, kw, wkw in runs:
        lists = M.accepted(cands, classes, rays, flags, **wkw)
        for K in (4, 2):
            first = M.first_k(None, None, rays, K, flags, lists=lists)
            second = M.first_k(None, None, rays, K, flags, after=first[0][:, K - 1, :], lists=lists)
            assert (first[1] > 0).sum() >= 20, f"{what}: some rays must hit"
            assert K == 4 or flags or second[1].any(), f"{what}: the second link of K = 2 must have something to report"
            for name, scene in routes.items():
                a, b = two_links(scene, rt, K, flags, **kw)
                assert_slots(a, first, f"{name}, {what}, K = {K}: the first link")
                assert_slots(b, second, f"{name}, {what}, K = {K}: the second link")
            old = two_links(before, rt, K, flags, **kw)
            assert (_np(old[0].hits).view(np.uint32) != first[0]).any(), f"{what}: the change must change the answer of some ray"


@pytest.mark.parametrize("name,deform", [("cornell", "far"), ("bunny", "smooth")])
def test_every_route_to_the_changed_vertices_gives_the_same_bytes(gpu_ctx, scene_cache, name, deform):
    """The answer is defined by the accepted set, not by the tree: scenes freshly built by either builder, refitted (update_vertices,
    update_vertices_async), refitted and rebuilt (rebuild by either builder, rebuild_async) and under the device's own policy
    (update_vertices_or_rebuild_async, once rebuilding and once skipping) give identical bytes."""
    ms = {f: made(gpu_ctx, name, f, deform) for f in (SAH, LBVH)}
    m = ms[SAH]
    s, ranges = m["s"], changed_ranges(m["old"], m["new"])
    routes, mine = {}, []
    for f, tag in ((SAH, "host SAH"), (LBVH, "device LBVH")):
        routes[f"fresh, {tag}"] = ms[f]["fresh"]
        routes[f"update_vertices, {tag}"] = ms[f]["scene"]
        routes[f"update_vertices_async, {tag}"] = async_twin(gpu_ctx, _with_flags(s.desc, f), ranges)
        x = api.Scene(gpu_ctx, _with_flags(s.desc, f))
        x.update_vertices(ranges)
        x.rebuild("host" if f == SAH else "device")
        routes[f"update_vertices and rebuild, {tag}"] = x
        mine += [routes[f"update_vertices_async, {tag}"], x]
    x = prepared(gpu_ctx, s.desc)
    x.update_vertices_async(on_device(ranges))
    x.rebuild_async()
    assert status(x) == (2, 0, None, None), "the enqueued rebuild was committed"
    routes["update_vertices_async and rebuild_async"] = x
    mine.append(x)
    for above, decision in ((0.0, True), (INF, False)):
        x = policy_scene(gpu_ctx, s.desc)
        assert x.update_vertices_or_rebuild_async(on_device(ranges), above) is None
        st = x.rebuild_if_status()
        assert (st.evaluated, st.rebuilt, st.last_decision) == (1, int(decision), decision), f"rebuild_above {above}: {st}"
        assert status(x)[1] == 0
        routes[f"update_vertices_or_rebuild_async, {'rebuilt' if decision else 'skipped'}"] = x
        mine.append(x)
    assert len(routes) == 11
    before = api.Scene(gpu_ctx, s.desc)
    masks = seeded_masks(s.desc.numInstances, 101)
    for scene in list(routes.values()) + [before]:
        scene.set_instance_masks(masks)
    rays = query_rays(gpu_ctx, m, name)[1][:500]
    assert_routes_agree(routes, rays, m["fresh"].export_bvh(), m["desc"], masks, seeded_masks(len(rays), 7), before)
    for x in mine + [before]:
        x.close()


@BUILDS
def test_every_route_to_the_moved_instances_gives_the_same_bytes(gpu_ctx, build):
    """the layered scene with every instance translated (exactly, in float32; copies keep their layer's transform, so the ties stay):
    update_instances and update_instances_async, then set_instance_masks, against a fresh scene with those transforms and masks"""
    desc, keep = M.layered_scene()
    desc.buildFlags = build
    moved, mkeep = M.layered_scene()
    moved.buildFlags = build
    n = desc.numInstances
    for i in range(n):
        layer = i if i < M.LAYERS else M.FIRST_COPIED + (i - M.LAYERS)
        tr = mkeep[3][i].transform
        tr[3], tr[7], tr[11] = 0.125 * (layer % 3), -0.0625 * (layer % 4), 0.375 * layer
    inst = [A.RtrInstance.from_buffer_copy(bytes(mkeep[3][i])) for i in range(n)]
    fresh = api.Scene(gpu_ctx, moved)
    a = api.Scene(gpu_ctx, desc)
    a.update_instances(inst)
    b = api.Scene(gpu_ctx, desc)
    b.prepare_async_updates()
    b.update_instances_async(torch.tensor([list(i.transform) for i in inst], dtype=torch.float32, device="cuda"))
    assert status(b) == (1, 0, None, None)
    before = api.Scene(gpu_ctx, desc)
    masks = seeded_masks(n, 5)
    masks[[3, 12]] = [0x01, 0x20]                            # one member of a tie pair is hidden from the rays the other one is not
    for scene in (fresh, a, b, before):
        scene.set_instance_masks(masks)
    rays, kinds = M.layered_rays(fresh.stats(), mixed_rays)
    routes = {"fresh": fresh, "update_instances": a, "update_instances_async": b}
    if build == SAH:                                         # and the other builder's fresh tree
        other = M.layered_scene()
        for i in range(n):
            other[1][3][i].transform[:] = inst[i].transform[:]
        other[0].buildFlags = LBVH
        routes["fresh, device LBVH"] = api.Scene(gpu_ctx, other[0])
        routes["fresh, device LBVH"].set_instance_masks(masks)
    assert_routes_agree(routes, rays, fresh.export_bvh(), moved, masks, seeded_masks(len(rays), 7), before)
    for scene in list(routes.values()) + [before]:
        scene.close()


# ---- 3.9 stream order with a changing scene -----------------------------------------------------------------------------------------
def test_a_chain_behind_an_enqueued_update_and_rebuild(scene_cache):
    """update_vertices_async, rebuild_async, trace_rays_multi and its resumed link enqueued on a side stream behind a filler, no host
    join in between: the query must see the vertices and the tree the stream produced"""
    ctx = api.Context(0)
    s = vu._setup("bunny")
    old = vu.verts_of(s.desc)
    new = vu.smooth(s.desc, old)
    twin = device_scene(ctx, s.desc)
    twin.update_vertices(changed_ranges(old, new))
    twin.rebuild("device")
    rays0 = torch.from_numpy(query_rays(ctx, {"s": s, "scene": twin}, "bunny")[1][:500]).cuda()
    a = api.trace_rays_multi(twin, rays0, 3)
    b = api.trace_rays_multi(twin, rays0, 3, after=a)
    assert int(b.counts.sum()) > 0
    scene = prepared(ctx, s.desc)
    stale = api.trace_rays_multi(scene, rays0, 3)
    dev_new = torch.from_numpy(new).cuda()
    x = torch.rand(2048, 2048, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx.set_stream(stream.cuda_stream)
        _filler(x, 20)
        pos, nrm = dev_new[:, 0:3] * 1.0, dev_new[:, 4:7].clone()         # made on the stream, behind the filler (x * 1 is exact)
        rays = rays0 * 1.0
        scene.update_vertices_async([(0, pos, nrm)])
        scene.rebuild_async()
        p = api.trace_rays_multi(scene, rays, 3, asynchronous=True)
        q = api.trace_rays_multi(scene, rays, 3, after=p, asynchronous=True)
        stream.synchronize()
        assert torch.equal(p.hits, a.hits) and torch.equal(p.counts, a.counts), "the first link saw the updated, rebuilt scene"
        assert torch.equal(q.hits, b.hits) and torch.equal(q.counts, b.counts), "the resumed link"
        ctx.set_stream(None)
    assert status(scene) == (2, 0, None, None)
    assert stale.hits.shape == a.hits.shape and not torch.equal(stale.hits, a.hits), "the update changes the answer: a stale scene would not pass"
    scene.close(); twin.close(); ctx.close()
