"""What tests/test_gpu_ris.py runs on: the Cornell box with area lights below the ceiling (the small builder of tests/test_gpu_power.py,
with a height per light), random rays, and one World per box — scene, 64 x 64 camera hits (pixel seeds), 6 000 random-ray hits
(explicit seeds) and the host's light-power table, made once.  No test in here."""
import os

import numpy as np
import torch

from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api, host, scenes

NS = 3
W = H = 64


def random_rays(lo, hi, n, seed):
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    o = lo + (hi - lo) * rng.uniform(-0.2, 1.2, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, 0.001, d, 10000.0
    return r


def box(directory, lights, width=W, height=H):
    """the Cornell box with the given lights facing down: (mesh, intensity, two-sided, x, (scale x, scale y)[, y]) each; mesh: 1 (a
    triangle) or 2 (the quad); y: the light's height, 540 (just below the ceiling) when left out"""
    tri = os.path.join(directory, "ris_light_triangle.obj")
    if not os.path.exists(tri):
        with open(tri, "w") as f:
            f.write("v -0.5 -0.5 0\nv 0.5 -0.5 0\nv 0 0.5 0\nf 1 2 3\n")
    obj, mtldir = scenes.write_cornell(None)
    hs = host.HostScene()
    for k, (mesh, intensity, two_sided, x, scale, *rest) in enumerate(lights):
        light = hs.addAreaLight(intensity, (1.0, 0.85 - 0.2 * k, 0.6 + 0.1 * k), two_sided, True, tri if mesh == 1 else None)
        light.move((x, rest[0] if rest else 540.0, 279.5)).scale((scale[0], scale[1], 1.0)).rotate((90.0, 0.0, 0.0))
    hs.addObjMtlPair(obj, mtldir)
    hs.setSky((0.5, 0.7, 1.0))
    hs.build()
    pos = (278.0, 273.0, -800.0)
    cam = host.Camera(40.0, pos, (278.0, 273.0, 0.0), (0.0, 1.0, 0.0), width, height)
    return scenes.SceneSetup("cornell_ris", hs, cam, pos, width, height)


ONE = [(1, 20.0, False, 278.0, (130.0, 105.0))]
UNEQUAL = [(2, 40.0, False, 150.0, (150.0, 120.0)), (1, 0.5, True, 278.0, (60.0, 45.0)), (2, 6.0, False, 410.0, (100.0, 130.0))]
# two quads of one power (max colour 1, intensity x area = 2 x 300 x 300 = 50 x 60 x 60): a large one at the ceiling, a small one
# low over the floor, beside the tall block and above the short one
NEAR_AND_FAR = [(2, 2.0, False, 278.0, (300.0, 300.0)), (2, 50.0, False, 100.0, (60.0, 60.0), 200.0)]


def i32(x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).cuda()


class World:
    """one scene with its camera hits (seeds: the pixels'), random-ray hits (explicit seeds) and light table: computed once"""
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
        self.tris = sum(int(l.numTriangles) for l in self.lights)

    def params(self, kind, outputs=A.LIGHT_SHADOWED):
        return api.make_light_params(self.s.num_lights, NS, self.frame, W if kind == "camera" else 0, 1, outputs)

    def seeds(self, kind, n=None):
        sd = self.inputs[kind][2]
        return None if sd is None else i32(sd[:n])

    def host_seeds(self, kind, n=None):
        sd = self.inputs[kind][2]
        return None if sd is None else sd[:n]
