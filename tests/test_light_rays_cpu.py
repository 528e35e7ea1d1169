"""What tests/test_gpu_direct_light.py leaves out of its light-ray comparison, confirmed without a GPU: with the witness and the oracle's
primary hits alone, the hits of the chosen scenes and frames whose culling decisions (one-sided light, directional light in front) sit
inside their fp32 error margin are at most 0.5 % — the share tests/test_witness.py allows for discrete decisions.  Also pins the slot
layout and the null slots of the float64 restatement itself."""
import numpy as np
import pytest

from realtimeraytracer_amd import api, scenes
from light_witness import KIND_OBJECT, LightWitness, expected_light_rays, light_triangles
from test_gpu_surfaces import Expect
from witness import F, normalize, pcg


def _camera_rays(s, w, h):
    """raygen.rgen:83-92 for 1 spp in float64, pixel position rounded to fp32 once (tests/witness.py: render_all)"""
    cam = np.array(s.camera.position[:3], F)
    TL, dH, dV = (np.array(a[:3], F) for a in (s.camera.topLeftViewportCorner, s.camera.horizontalViewportDelta, s.camera.verticalViewportDelta))
    k = np.arange(w * h)
    xs, ys = k % w, k // w
    jx = jy = pcg(xs.astype(np.uint32))
    pw = (TL + dH * (xs + jx - 0.5)[:, None] + dV * (ys + jy - 0.5)[:, None]).astype(np.float32).astype(F)
    r = np.zeros((w * h, 8), np.float32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = cam, 0.001, normalize(pw - cam), 10000.0
    return r, xs, ys


@pytest.mark.parametrize("case", ["cornell_box", "textured_room"])
def test_few_hits_sit_on_a_decision_boundary(oracle, scene_cache, case):
    s, w, h = (scenes.cornell_box(128, 128), 128, 128) if case == "cornell_box" else (scenes.textured_room(160, 100), 160, 100)
    t, u, v, cu, pr = oracle.primary_hits(s.desc, s.camera, api.make_params(w, h, spp=1), bvh=None, threads=8)
    rays, xs, ys = _camera_rays(s, w, h)
    hits = np.zeros((w * h, 8), np.int32)
    hits[:, 0], hits[:, 1], hits[:, 2] = t.view(np.int32), u.view(np.int32), v.view(np.int32)
    hits[:, 3], hits[:, 4] = cu.view(np.int32), pr.view(np.int32)
    wit = LightWitness(s.desc)
    surf = Expect(wit, rays, hits)
    with np.errstate(over="ignore"):
        base = xs.astype(np.uint32) * np.uint32(733) + ys.astype(np.uint32) * np.uint32(1933)
    tris = light_triangles(wit, s.num_lights)
    Q = 3 * len(tris) + 1
    for f in (0, 5):
        exp = expected_light_rays(wit, surf, base, f, s.num_lights, 3)
        assert exp.rays.shape == (w * h, Q, 8)
        print(f"{case} frame {f}: {int(exp.boundary.sum())} of {w * h} hits on a decision boundary")
        assert exp.boundary.mean() <= 0.005
        obj = surf.kind == KIND_OBJECT
        assert obj.mean() > 0.2 and exp.null[~obj].all() and not exp.rays[exp.null].any()
        live = ~exp.null
        assert live[obj].any(1).mean() > 0.5
        # a live area ray aims at a point of its light triangle's plane, 0.5 short of it as measured from the hit point, and is normalised
        P = surf.val["position"]
        for ti, (L, Pl, ln) in enumerate(tris):
            for j in range(3 * ti, 3 * ti + 3):
                r, p0 = exp.rays[live[:, j], j], P[live[:, j]]
                if len(r):
                    end = p0 + r[:, 4:7] * (r[:, 7] + 0.5)[:, None]
                    assert np.abs((end - Pl[0]) @ ln).max() < 1e-6 and np.abs(np.linalg.norm(r[:, 4:7], axis=1) - 1).max() < 1e-12
        if case == "cornell_box":
            assert not s.desc.lights[0].isTwoSided and exp.null[obj][:, :Q - 1].all(1).any()     # the one-sided light's back: null slots occur
