"""Float64 witnesses of the direct-lighting stage for ray-query hits — TEST INFRASTRUCTURE, on tests/witness.py's loader and helpers.

  expected_light_rays   the shadow rays raygen.rgen:165-231 and :289-303 send for a surface point, restated in numpy float64 from the
                        shader text: which slots carry a ray, origin, direction, tmax, each with the bound an fp32 evaluation must keep
                        and the hits whose culling decisions sit too close to 0 for fp32 and float64 to have to agree;
  LightWitness.shade    Witness._shade — the witness's brdf, texture sampler and LTC path — for hits the caller supplies (any ray origin,
                        explicit seeds), with the shadow queries answered from a table of visibility bytes instead of the witness's own
                        brute-force occlusion test, so that what is compared is the shading and not the shadow edges.
"""
from types import SimpleNamespace

import numpy as np

from witness import F, Witness, normalize, pcg

MISS = 0xffffffff
KIND_MISS, KIND_OBJECT, KIND_LIGHT, KIND_INVALID = 0, 1, 2, 3          # RTR_SURFACE_* (include/rtr_types.h)
RTOL, ATOL = 1e-5, 1e-6                                                # tests/test_gpu_surfaces.py: 1e-5 of the operands' magnitude + 1e-6
INV733 = pow(733, -1, 2 ** 32)                                         # 733 is odd: px = seed * INV733, py = 0 gives px * 733 + py * 1933 = seed (mod 2^32)


def light_triangles(w, num_area_lights):
    """[(light, world-space corners (3, 3), unit normal)] in slot order: the lights in order, their triangles in order (raygen.rgen:174-196)"""
    out = []
    for li in range(num_area_lights):
        L = w.lights[li]
        T = np.array(L.transform[:], F).reshape(4, 4).T                # column-major mat4
        for ti in range(L.numTriangles):
            j = w.idx[L.indexOffset + 3 * ti: L.indexOffset + 3 * ti + 3].astype(np.int64) + L.vertexOffset
            Pl = w.verts[j, 0:3] @ T[:3, :3].T + T[:3, 3]
            ln = np.cross(Pl[2] - Pl[1], Pl[0] - Pl[1])
            out.append((L, Pl, ln / np.sqrt(ln @ ln)))
    return out


def expected_light_rays(w, surf, base, frame, num_area_lights, num_shadow_rays):
    """surf: the witness's surfaces of the hits with their fp32 bounds (test_gpu_surfaces.Expect: val / bound / kind); base: uint32 (n,)
    seed bases.  Returns rays (n, Q, 8) float64 (zeros where no ray is sent), null (n, Q), boundary (n,) and per-ray bounds.

    Bounds (bp, bn: the surface's position and normal bounds; |.|: magnitudes of the operands):
      origin     hitPoint + 0.01 * normal                       bp + 0.01 * bn + ATOL
      sample     P0 + (P1 - P0) r1 + (P2 - P0) r2, r <= 1       b_l = 3 * RTOL * max|P_i| + ATOL   (r1, r2 are exact: fp32 values on both sides)
      tmax       |sample - hitPoint| - 0.5                      b_l + bp (both end points) + RTOL * distance + ATOL
      direction  (sample - hitPoint) / distance                 (b_l + bp) / distance + RTOL + ATOL
    Decisions: the one-sided test dot(n_l, hitPoint - P0) < 0 carries bp, P0's own error and the rounding of a dot product of that
    length, bp + RTOL * max|P_i| + 2 * RTOL * |hitPoint - P0| + ATOL; dot(normal, directional) <= 0 carries bn + ATOL.  A hit with a
    dot product inside its margin is `boundary`."""
    n = surf.n
    tris = light_triangles(w, num_area_lights)
    Q = len(tris) * num_shadow_rays + 1
    P, N = surf.val["position"], surf.val["normal"]
    bp, bn = surf.bound["position"], surf.bound["normal"]
    obj = surf.kind == KIND_OBJECT
    rays = np.zeros((n, Q, 8), F)
    null = np.ones((n, Q), bool)
    boundary = np.zeros(n, bool)
    bound_o = np.repeat((bp + 0.01 * bn + ATOL)[:, None], Q, 1)
    bound_d, bound_t = np.zeros((n, Q)), np.zeros((n, Q))
    so = P + 0.01 * N
    base = np.asarray(base, np.uint32)
    for t, (L, Pl, ln) in enumerate(tris):
        pmax = np.abs(Pl).max()
        b_l = 3 * RTOL * pmax + ATOL
        culled = np.zeros(n, bool)
        if not L.isTwoSided:
            rel = P - Pl[0]
            dotv = rel @ ln
            culled = dotv < 0.0                                                           # raygen.rgen:194-196
            boundary |= obj & (np.abs(dotv) <= bp + RTOL * pmax + 2 * RTOL * np.sqrt(np.sum(rel * rel, 1)) + ATOL)
        for s in range(num_shadow_rays):
            with np.errstate(over="ignore"):
                seed = np.uint32(s) + base + np.uint32(frame & 0xffffffff)
                r1, r2 = pcg(seed), pcg(seed + np.uint32(100))
            fold = (r1.astype(np.float32) + r2.astype(np.float32)) > np.float32(1.0)      # decided on the fp32 sum, as the shader does
            r1, r2 = np.where(fold, 1 - r1, r1), np.where(fold, 1 - r2, r2)
            lp = Pl[0] + (Pl[1] - Pl[0]) * r1[:, None] + (Pl[2] - Pl[0]) * r2[:, None]
            lv = lp - P
            dist = np.sqrt(np.sum(lv * lv, 1))
            slot = t * num_shadow_rays + s
            with np.errstate(invalid="ignore", divide="ignore"):
                rays[:, slot, 0:3], rays[:, slot, 3], rays[:, slot, 4:7], rays[:, slot, 7] = so, 0.001, lv / dist[:, None], dist - 0.5
                bound_d[:, slot] = (b_l + bp) / dist + RTOL + ATOL
            bound_t[:, slot] = b_l + bp + RTOL * dist + ATOL
            null[:, slot] = ~obj | culled
    dl = np.array([-1.0, 1.0, -0.5], F)
    dl /= np.sqrt(dl @ dl)                                                                # raygen.rgen:289
    dotn = N @ dl
    boundary |= obj & (np.abs(dotn) <= bn + ATOL)
    rays[:, Q - 1, 0:3], rays[:, Q - 1, 3], rays[:, Q - 1, 4:7], rays[:, Q - 1, 7] = so, 0.001, dl, 10000.0
    bound_d[:, Q - 1], bound_t[:, Q - 1] = RTOL + ATOL, ATOL
    null[:, Q - 1] = ~obj | ~(dotn > 0.0)                                                 # :291: sent only with the light in front
    rays[null] = 0.0
    return SimpleNamespace(rays=rays, null=null, boundary=boundary, bound_o=bound_o, bound_d=bound_d, bound_t=bound_t)


class LightWitness(Witness):
    def __init__(self, desc):
        super().__init__(desc)
        self.soup_first, at = {}, 0                                    # customIndex -> its first triangle in the witness's soup
        for inst in self.instances:
            self.soup_first[inst.customIndex] = at
            at += self.meshes[inst.meshIndex].indexCount // 3
        self._vis = None

    def occluded(self, o, d, tmax):
        """the shadow queries of Witness._shade, answered from the table: calls come in slot order, the directional light's last"""
        if self._vis is None:
            return np.zeros(len(o), bool)
        vis, rows, dir_rows = self._vis
        j, self._call = self._call, self._call + 1
        if j < vis.shape[1] - 1:
            return vis[rows, j] != 0
        return vis[dir_rows, vis.shape[1] - 1] != 0

    def shade(self, rays, hits, seeds, frame, num_area_lights, num_shadow_rays, occluded):
        """{shadowed, unshadowed, analytic (n, 3) float64, kind (n,)} for RtrRay / RtrHit rows; seeds: uint32 (n,) seed bases;
        occluded: (n, Q) visibility bytes"""
        n = len(rays)
        o, d = rays[:, 0:3].astype(F), rays[:, 4:7].astype(F)
        cu = hits[:, 3].astype(np.int64) & 0xffffffff
        pr = hits[:, 4].astype(np.int64) & 0xffffffff
        u, v = hits[:, 1].view(np.float32).astype(F), hits[:, 2].view(np.float32).astype(F)
        counts = np.array([self.lights[c].numTriangles if c < self.numLights else self.meshes[self.instances[c].meshIndex].indexCount // 3
                           for c in range(len(self.instances))], np.int64)
        valid = (cu < len(counts)) & (pr < counts[np.minimum(cu, len(counts) - 1)])
        kind = np.full(n, KIND_INVALID, np.int64)
        kind[cu == MISS] = KIND_MISS
        kind[valid & (cu < self.numLights)] = KIND_LIGHT
        kind[valid & (cu >= self.numLights)] = KIND_OBJECT
        out = {k: np.zeros((n, 3), F) for k in ("shadowed", "unshadowed", "analytic")}
        m = kind == KIND_MISS
        if m.any():                                                                       # miss.rmiss:15-27
            sky = np.broadcast_to(self.sky, (int(m.sum()), 3))
            if self.hdri is not None:
                dd = normalize(d[m])
                hu = np.arctan2(dd[:, 2], dd[:, 0]) / (2 * 3.14159265) + 0.5
                hv = 1.0 - np.arccos(np.clip(dd[:, 1], -1, 1)) / 3.14159265
                sky = np.power(self.sample(self.hdri, hu, hv)[:, :3], 2.2)
            for k in out:
                out[k][m] = sky
        for li in np.unique(cu[kind == KIND_LIGHT]):                                      # raygen.rgen:116-121
            for k in out:
                out[k][(kind == KIND_LIGHT) & (cu == li)] = np.array(self.lights[li].color[:3], F)
        rows = np.nonzero(kind == KIND_OBJECT)[0]
        if len(rows):
            soup = np.zeros(n, np.int64)
            soup[rows] = np.array([self.soup_first[c] for c in cu[rows]], np.int64) + pr[rows]
            xs = (np.asarray(seeds, np.uint64) * np.uint64(INV733)) & np.uint64(0xffffffff)
            ys = np.zeros(n, np.int64)
            info = SimpleNamespace(numAreaLights=num_area_lights, frame=frame)
            params = SimpleNamespace(numShadowRays=num_shadow_rays)
            args = (rows, xs.astype(np.int64), ys, o[rows], d, soup, u, v, info, params, True)
            self._vis = None
            N = self._shade(*args)[3]                                                     # a dry pass for the normals: who sends the directional ray
            dl = np.array([-1.0, 1.0, -0.5], F)
            dl /= np.sqrt(dl @ dl)
            self._vis, self._call = (np.asarray(occluded), rows, rows[N @ dl > 0]), 0
            sh, un, an, _, _ = self._shade(*args)
            self._vis = None
            out["shadowed"][rows], out["unshadowed"][rows], out["analytic"][rows] = sh, un, an
        out["kind"] = kind
        return out
