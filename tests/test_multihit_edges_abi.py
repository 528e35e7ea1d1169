"""The constructions of tests/test_gpu_multihit_edges.py held to their design, without a device: the tie stack (tests/multihit_witness.py:
tie_stack_scene, tie_stack_rays) and the tiny scenes (tiny_scenes, tiny_rays) through api.host_build_bvh and all_hits32 — the hit counts
of every ray group, the multiplicities per t, that record storage order disagrees with id order inside each tie, that each run of 64
sign-pattern rays is uniform and the mixed run is not, and that the window rays' tmin and tmax sit on a candidate's t bit for bit.  The
GPU tests rely on these conditions, so they cannot pass vacuously."""
import numpy as np
import pytest

from realtimeraytracer_amd import api

import multihit_witness as M

F32 = np.float32
INF = F32(np.inf)


def bits(x):
    return np.asarray(x, F32).view(np.uint32)


@pytest.fixture(scope="module")
def stack():
    desc, keep = M.tie_stack_scene()
    st, nodes, tris = api.host_build_bvh(desc)
    rays, kinds = M.tie_stack_rays()
    cands = M.all_hits32((nodes, tris), rays)
    return {"desc": desc, "keep": keep, "st": st, "nodes": nodes, "tris": tris, "rays": rays, "kinds": kinds, "cands": cands,
            "n": np.array([len(c[0]) for c in cands])}


def multiplicities(cand):
    """{t: how many records} of one ray"""
    ts, counts = np.unique(np.array(cand[0], F32), return_counts=True)
    return dict(zip(ts.tolist(), counts.tolist()))


def layer_t(kind_or_down, z):
    return (M.DOWN_Z - z) if kind_or_down else (z - M.UP_Z)


def test_the_tie_stack_scene_is_the_one_described(stack):
    raw = np.frombuffer(stack["tris"], dtype=np.uint32).reshape(-1, 12)
    n = len(M.TIE_STACK_Z)
    assert n == 44 and len(raw) == 88 and stack["st"].numTriangles == 88
    assert sorted(raw[:, 3].tolist()) == sorted(list(range(n)) * 2), "every customIndex is distinct: two triangles apiece"
    assert not (raw[:, 11] & 1).any()
    inst = stack["desc"].instances
    z_of = {int(inst[i].customIndex): float(inst[i].transform[11]) for i in range(n)}
    assert sorted(z_of.values()) == sorted(M.TIE_STACK_Z)
    assert [sum(1 for z in M.TIE_STACK_Z if z == t) for t in M.TIE_Z] == [M.TIE_DEPTH] * 2 and all(M.TIE_STACK_Z.count(z) == 1 for z in M.SINGLE_Z)
    for z in M.TIE_Z:                                # the copies carry ONE transform, bit for bit
        rows = {bytes(inst[i].transform) for i in range(n) if float(inst[i].transform[11]) == z}
        assert len(rows) == 1
    flt = raw.view(F32)
    assert all(float(flt[j, 2]) == z_of[int(raw[j, 3])] for j in range(len(raw))), "the records' v0.z is the instance's layer"
    customs = [int(inst[i].customIndex) for i in range(n)]
    assert customs != sorted(customs), "the customIndex is a permutation of the instance order, not the order itself"
    # record storage order against id order: inside each tie a smaller customIndex sits BEHIND a larger one
    for z in M.TIE_Z:
        order = [int(c) for c, zz in zip(raw[:, 3], flt[:, 2]) if float(zz) == z]
        assert len(order) == 2 * M.TIE_DEPTH
        assert any(a > b for a, b in zip(order, order[1:])), f"z = {z}: storage order is id order"
    print(f"tie stack, host SAH builder: depth {stack['st'].maxDepth}, {stack['st'].numNodes} nodes")


def test_the_tie_stack_rays_have_the_hit_counts_they_were_built_for(stack):
    rays, kinds, cands, n = stack["rays"], stack["kinds"], stack["cands"], stack["n"]
    assert [int((kinds == k).sum()) for k in range(5)] == [256, 256, 64, 576, 2 * 32 * len(M.WINDOWS)]
    assert np.nonzero(kinds == M.KIND_SIGNS)[0][0] == M.SIGNS_FIRST and M.SIGNS_FIRST % 64 == 0
    assert len(rays) < 1800
    # (a) the through grids
    for kind in (M.KIND_UP, M.KIND_DOWN):
        sel = np.nonzero(kinds == kind)[0]
        inside = M.grid_inside(rays[sel])
        off = inside & (rays[sel][:, 0] != rays[sel][:, 1])
        assert inside.sum() == M.INSIDE and off.sum() == M.INSIDE - 12 >= 100
        assert (n[sel][off] == 44).all() and (n[sel][inside & ~off] == 88).all() and (n[sel][~inside] == 0).all()
        deep = 0
        for k in sel[off]:
            m = multiplicities(cands[k])
            assert m == {**{layer_t(kind, z): 1 for z in M.SINGLE_Z}, **{layer_t(kind, z): M.TIE_DEPTH for z in M.TIE_Z}}, (k, m)
            deep += max(m.values()) > 8
        assert deep >= 100, "at least 100 rays per direction have more than 8 accepted records on a single t"
    # (b) through the shared diagonal: both triangles of every instance
    for k in np.nonzero(kinds == M.KIND_DIAG)[0]:
        assert n[k] == 88
        assert multiplicities(cands[k]) == {**{layer_t(0, z): 2 for z in M.SINGLE_Z}, **{layer_t(0, z): 2 * M.TIE_DEPTH for z in M.TIE_Z}}
        ts, cs, ps = np.array(cands[k][0], F32), np.array(cands[k][3]), np.array(cands[k][4])
        for z in M.TIE_Z:
            tie = ts == F32(layer_t(0, z))
            assert sorted(zip(cs[tie].tolist(), ps[tie].tolist())) == sorted((c, p) for c in set(cs[tie].tolist()) for p in (0, 1))
            assert len(set(cs[tie].tolist())) == M.TIE_DEPTH, "two primitiveIds per customIndex"
    # (c) the oblique runs: 44 records, two ties of 20 (the copies are bit copies, so their t is one value whatever the direction)
    for k in np.nonzero(kinds == M.KIND_SIGNS)[0]:
        assert n[k] == 44
        assert sorted(multiplicities(cands[k]).values()) == [1, 1, 1, 1, M.TIE_DEPTH, M.TIE_DEPTH], k


def test_each_sign_run_is_uniform_and_the_mixed_run_is_not(stack):
    rays, kinds = stack["rays"], stack["kinds"]
    c = rays[kinds == M.KIND_SIGNS]
    assert len(c) == 9 * 64 and (c[:, 4:7] != 0).all(), "no zero component: the sign is the octant"
    pat = M.sign_pattern(c)
    for p in range(8):
        assert (pat[64 * p: 64 * (p + 1)] == p).all(), f"run {p}"
    assert sorted(set(pat[512:].tolist())) == list(range(8)), "the ninth run mixes all eight patterns: the generic walk"
    # the other waves of the full launch are uniform too (+z: pattern 0, -z: pattern 4); the runs start on wave boundaries
    assert (M.sign_pattern(rays[kinds == M.KIND_UP]) == 0).all() and (M.sign_pattern(rays[kinds == M.KIND_DOWN]) == 4).all()


def test_the_window_bounds_sit_on_a_candidates_t_bit_for_bit(stack):
    rays, kinds, n = stack["rays"], stack["kinds"], stack["n"]
    w = rays[kinds == M.KIND_WINDOW]
    open_rays = w.copy()
    open_rays[:, 3], open_rays[:, 7] = 0.0, np.inf
    every = M.all_hits32((stack["nodes"], stack["tris"]), open_rays)
    got = n[kinds == M.KIND_WINDOW]
    inside = M.grid_inside(w)
    for v, (zmin, zmax) in enumerate(M.WINDOWS):
        for down in (0, 1):
            rows = np.arange(32) + 64 * v + 32 * down
            assert inside[rows].sum() == 24 and (got[rows][~inside[rows]] == 0).all()
            lo, hi = (zmin, zmax) if not down else (zmax, zmin)
            for k in rows[inside[rows]]:
                ts = set(bits(every[k][0]).tolist())
                assert len(every[k][0]) in (44, 88)
                if lo is None:
                    assert w[k, 3] == 0.0
                else:
                    assert int(bits(w[k, 3])) in ts and w[k, 3] == F32(layer_t(down, lo)), (v, down, k)
                if hi is None:
                    assert w[k, 7] == 100.0
                else:
                    assert int(bits(w[k, 7])) in ts and w[k, 7] == F32(layer_t(down, hi)), (v, down, k)
                # both bounds are exclusive: the records strictly between the two layers
                tlo, thi = w[k, 3], w[k, 7]
                per = 2 if w[k, 0] == w[k, 1] else 1
                between = sum(per for z in M.TIE_STACK_Z if tlo < F32(layer_t(down, z)) < thi)
                assert got[k] == between, (v, down, k, got[k], between)
    both_ties = [v for v, win in enumerate(M.WINDOWS) if set(win) - {None} <= set(M.TIE_Z)]
    assert len(both_ties) >= 5 and (0.5, 0.5) in M.WINDOWS, "both tie layers as tmin and as tmax, and tmin == tmax on a layer"
    assert (w[64 * M.WINDOWS.index((0.5, 0.5)):][:64, 3] == w[64 * M.WINDOWS.index((0.5, 0.5)):][:64, 7]).all()


def test_the_tiny_scenes(stack):
    scenes = M.tiny_scenes()
    rays = M.tiny_rays()
    assert sorted(scenes) == [1, 2, 8, 9] and len(rays) < 200
    for ntri, (desc, keep) in scenes.items():
        st, nodes, tris = api.host_build_bvh(desc)
        raw = np.frombuffer(tris, dtype=np.uint32).reshape(-1, 12)
        assert len(raw) == ntri == st.numTriangles and len(set(raw[:, 3].tolist())) == ntri
        flt = raw.view(F32)
        tied = raw[flt[:, 2] == F32(M.TINY_Z)]
        assert len(tied) == min(ntri, 8) and len({r[[0, 1, 2, 4, 5, 6, 8, 9, 10]].tobytes() for r in tied}) == 1, "bit copies of one triangle"
        if ntri == 9:
            behind = raw[flt[:, 2] == F32(M.TINY_BEHIND_Z)]
            assert len(behind) == 1 and int(behind[0, 3]) == 0 == int(raw[:, 3].min()), "the triangle behind the tie has the smallest customIndex"
        if ntri > 1:
            order = tied[:, 3].tolist()
            assert order != sorted(order) or ntri == 2, "storage order is not id order"
        cands = M.all_hits32((nodes, tris), rays)
        n = np.array([len(c[0]) for c in cands])
        centre = np.nonzero((rays[:, 0] == 0) & (rays[:, 1] == 0) & (np.abs(rays[:, 6]) == 1) & (rays[:, 2] != 5.0))[0]
        assert len(centre) >= 2 and (n[centre[:2]] == ntri).all(), "a ray through the middle meets every triangle"
        assert (n == ntri).sum() >= 10 and (n == 0).sum() >= 40 and set(n.tolist()) <= {0, ntri}
        assert (n[-8:] == 0).all(), "the rays along an edge inside the plane and the rays far outside hit nothing"
        if ntri == 1:
            ch = np.frombuffer(nodes, dtype=np.int32).reshape(-1, 8)[0, 6:8]
            assert ch[0] == ch[1] < 0, "a one-leaf tree names its leaf in both children of the root"


def test_tail_rays_finds_the_groups_that_hold_only_tail_rays():
    truth = np.zeros(200, bool)
    truth[[3, 40, 41, 42, 43, 64, 65, 190, 199]] = True
    launches = []

    def count(idx):
        launches.append(len(idx))
        return int(truth[idx].sum())

    assert M.tail_rays(count, 200) == np.nonzero(truth)[0].tolist()
    assert M.tail_rays(count, 200, cap=4) == [3, 40, 41, 42]
    assert M.tail_rays(lambda idx: 0, 200) == []
