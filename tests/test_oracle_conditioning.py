"""The host builder and the oracle on badly conditioned geometry (tests/conditioned_scenes.py), without a GPU: every case's tree keeps
the BVH invariants, the oracle's walks over it (camera rays over the BVH2, shadow rays over the 4-wide view) find what its brute-force
loop finds, bit for bit, and that brute-force loop agrees with an independent float64 ray / triangle test (tests/witness.py) on the
rays of the generator, away from triangle edges."""
import numpy as np
import pytest

import conditioned_scenes as cs
from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api
from test_gpu_query import MISS, brute_force
from test_oracle_bvh import _check_bvh
from witness import ray_hits

W, H, SPP = 96, 54, 2


@pytest.mark.parametrize("name", cs.ALL)
def test_host_tree_and_oracle_walks_equal_brute_force(oracle, scene_cache, tmp_path, name):
    c = cs.case(name, tmp_path)
    st, nodes, tris = api.host_build_bvh(c.desc)
    _check_bvh(c.desc, st, nodes, tris)
    cs.check_padding(nodes, tris, st.grid, st)
    assert st.maxDepth <= 64 and st.stackEntries >= st.maxDepth
    p = api.make_params(W, H, spp=SPP, collect_stats=1)
    a = oracle.primary_hits(c.desc, c.camera, p, bvh=(nodes, tris, st.grid), threads=8)
    b = oracle.primary_hits(c.desc, c.camera, p, bvh=None, threads=8)
    for x, y, n in zip(a, b, ("t", "u", "v", "customIndex", "primitiveId")):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), f"{name}: {n} differs between BVH walk and brute force"
    assert (a[3] != MISS).sum() >= 100, f"{name}: the camera must see the geometry"
    wide = api.host_build_bvh_wide(c.desc)
    assert bytes(wide[0]) == bytes(nodes) and bytes(wide[1]) == bytes(tris)
    for collect in (0, 1):
        p = api.make_params(W, H, spp=SPP, collect_stats=collect)
        fa = oracle.render(c.desc, c.camera, c.scene_info(1), p, bvh=wide, threads=8)
        fb = oracle.render(c.desc, c.camera, c.scene_info(1), p, bvh=None, threads=8)
        assert np.array_equal(fa.images[A.IMAGE_SHADOWED], fb.images[A.IMAGE_SHADOWED]), f"{name}, collect_stats={collect}"
        if collect:
            for f in ("numRays", "numPrimaryRays", "numShadowRays", "numHits"):
                assert getattr(fa.stats, f) == getattr(fb.stats, f), f


def _sample(c, seed):
    """the generator's rays, as many as a ctypes brute force over the case's triangles affords, plus tight-tmax rays"""
    n = int(np.clip(600_000 // c.num_triangles, 80, 600))
    return cs.rays(c, n, seed)


@pytest.mark.parametrize("name", cs.ALL)
def test_oracle_brute_force_against_float64_witness(oracle, scene_cache, tmp_path, name):
    c = cs.case(name, tmp_path)
    st, nodes, tris = api.host_build_bvh(c.desc)
    r = _sample(c, seed=3)
    t, u, v, cu, pr = brute_force(oracle, (nodes, tris, st.grid), r)
    tr, src = cs.tight(r, t, cu != MISS, 40, seed=4)
    if len(tr):
        t2, u2, v2, cu2, pr2 = brute_force(oracle, (nodes, tris, st.grid), tr)
        k = len(tr) // 2
        assert (cu2[:k] == MISS).all(), "tmax == closest t: t < tmax must reject the hit"
        assert np.array_equal(cu2[k:], cu[src[k:]]) and np.array_equal(t2[k:].view(np.uint32), t[src[k:]].view(np.uint32))
        r = np.concatenate([r, tr])
        t, u, v, cu, pr = (np.concatenate([x, y]) for x, y in zip((t, u, v, cu, pr), (t2, u2, v2, cu2, pr2)))
    # the oracle's hits in the witness's numbering (the records are in tree order; ids map them back)
    ids = np.frombuffer(tris, dtype=np.uint32).reshape(-1, 12)[:st.numTriangles][:, [3, 7]].astype(np.int64)
    row_of = {(int(a), int(b)): j for j, (a, b) in enumerate(ids)}
    best, bt, bu, bv, btol, amb, ties = ray_hits(c.v0, c.v1, c.v2, r)
    got = np.array([row_of[(int(a), int(b))] if a != MISS else -1 for a, b in zip(cu, pr)])
    clean = ~amb
    # edge, surface and tight rays are near an edge by design, and the margin grows with the origin's distance; the rest must stay
    # clean often enough that the comparison below cannot become empty
    assert clean.sum() >= 15 and clean.mean() >= 0.1, f"{name}: only {int(clean.sum())} of {len(r)} rays are away from edges"
    hit_o, hit_w = got >= 0, best >= 0
    bad = clean & (hit_o != hit_w)
    assert not bad.any(), f"{name}: {int(bad.sum())} clean rays hit in one and miss in the other; first {np.nonzero(bad)[0][:5].tolist()}"
    both = clean & hit_o
    # on the two lines, 1e-2 triangles seen from >= 1e4 units away, every hit lies within the fp32 error bound of an edge: there the
    # clean rays are misses, and they must be misses in both
    assert both.sum() >= (0 if name in ("line", "graded") else 5), f"{name}: too few clean hits to say anything"
    print(f"{name}: {int(clean.sum())} of {len(r)} rays clean, {int(both.sum())} clean hits")
    same = got[both] == best[both]
    tied = ties[both] > 1
    assert (same | tied).all(), f"{name}: {int((~(same | tied)).sum())} clean rays hit another triangle"
    dt = np.abs(t[both].astype(np.float64) - bt[both])
    assert (dt <= btol[both]).all(), f"{name}: t off by {float((dt / btol[both]).max()):.2f} margins"
