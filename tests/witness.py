"""An independent witness of the shading arithmetic — TEST INFRASTRUCTURE.

The CPU oracle (oracle/) and the HIP kernels share include/rtr_math.h: the same Moeller-Trumbore, the same pow / ACES / UNORM8
forms, the same expression order.  That is what makes bit-exact parity testable, and it is also why a wrong constant in that
header would be invisible to every parity test.  This module restates the path a SECOND time with nothing in common:
numpy, float64, libm (np.power, np.arctan2, ...), its own ray-triangle test, brute force over all triangles (no BVH), its own
texture sampler and tone map, written from the shader text (reference src/shaders/raygen.rgen, closesthit.rchit, miss.rmiss,
opacity.rahit, cook-torrance.glsl, raycommon.glsl, LTC.glsl) and the C-ABI scene description alone.

Covered: all five ray-gen images (Witness.render_all) — shadowed; unshadowed (the same sum, visibility 1); normal and position
(normalize(avg), avg * POSITION_SCALE, packed without a tone map); analytic (bilinear look-up of the two 64 x 64 x 4 LTC tables with
the sampler's repeat addressing, tangent frame, inverse transform from t1, the edge integrals with the shader's rational fit, the
clipped-sphere look-up in ltc2.w, one- / two-sided lights, the Fresnel mix from t2, x 5).  The passes behind the ray-gen dispatch
(a-trous, combine) have a witness of their own, tests/post_witness.py.

It cannot be bit-exact against fp32 code; tests/test_witness.py holds the oracle to it by measured bounds (median relative error of
the HDR radiance 1e-7, all but a handful of 20000 pixels byte-equal in every image), and allows the handful of pixels where a discrete
decision (hit / miss at a silhouette, occluded / visible at a shadow edge, r1 + r2 > 1 fold) flips between fp32 and fp64.  Values the
shader holds in fp32 and then amplifies are taken at fp32: the PCG floats, the fold's sum, and the pixel's world position (render_all).
"""
import ctypes as C

import numpy as np

F = np.float64
A_ANALYTIC, A_SHADOWED, A_UNSHADOWED, A_NORMAL, A_POSITION = 0, 1, 2, 6, 7      # rtr_image numbers (include/rtr.h)
POSITION_SCALE = 1.0                                                             # raygen.rgen:10


def _arr(ptr, n, dtype, width):
    if n == 0:
        return np.zeros((0, width), dtype)
    buf = C.cast(ptr, C.POINTER(C.c_uint8 * (n * width * np.dtype(dtype).itemsize))).contents
    return np.frombuffer(buf, dtype=dtype).reshape(n, width).copy()


def pcg(seed):
    """raycommon.glsl:22-27 on uint32 arrays (numpy wraps modulo 2^32)."""
    with np.errstate(over="ignore"):
        seed = np.asarray(seed, dtype=np.uint32)
        state = seed * np.uint32(747796405) + np.uint32(2891336453)
        word = ((state >> ((state >> np.uint32(28)) + np.uint32(4))) ^ state) * np.uint32(277803737)
        h = (word >> np.uint32(22)) ^ word
    # float(h) / 2^32 as the shader computes it: the uint -> float conversion rounds to 24 bits
    return h.astype(np.float32).astype(F) / 4294967296.0


def normalize(v):
    return v / np.sqrt(np.sum(v * v, axis=-1, keepdims=True))


class Witness:
    def __init__(self, desc):
        d = desc
        self.verts = _arr(d.vertices, d.numVertices, np.float32, 12).astype(F)        # pos(3) pad normal(3) pad uv(2) pad(2)
        self.idx = _arr(d.indices, d.numIndices, np.uint32, 1).reshape(-1)
        self.numLights = d.numLights
        self.meshes = [d.meshes[i] for i in range(d.numMeshes)]
        self.instances = sorted([d.instances[i] for i in range(d.numInstances)], key=lambda i: i.customIndex)
        self.objects = [d.objects[i] for i in range(d.numObjects)]
        self.lights = [d.lights[i] for i in range(d.numLights)]
        self.textures = []
        for t in range(d.numTextures):
            tx = d.textures[t]
            if not tx.pixels:
                self.textures.append(None)
                continue
            px = np.frombuffer(C.cast(tx.pixels, C.POINTER(C.c_uint8 * (tx.width * tx.height * tx.channels))).contents, dtype=np.uint8)
            self.textures.append(px.reshape(tx.height, tx.width, tx.channels).astype(F) / 255.0)
        self.hdri = None
        if d.hdri:
            tx = d.hdri.contents
            px = np.frombuffer(C.cast(tx.pixels, C.POINTER(C.c_uint8 * (tx.width * tx.height * tx.channels))).contents, dtype=np.uint8)
            self.hdri = px.reshape(tx.height, tx.width, tx.channels).astype(F) / 255.0
        tab = lambda p: np.ctypeslib.as_array(p, (64, 64, 4)).astype(F) if p else None     # noqa: E731  texSamplers[0], [1]: [v][u][rgba]
        self.ltc1, self.ltc2 = tab(d.ltc1), tab(d.ltc2)
        self.sky = np.power(np.array([d.skyColor[0], d.skyColor[1], d.skyColor[2]], F), 2.2)
        # world-space triangle soup in (instance, primitive) order + what the hit shader needs per triangle
        V0, V1, V2, cust, prim, alpha = [], [], [], [], [], []
        self.xform, self.nmat = {}, {}
        for inst in self.instances:
            me = self.meshes[inst.meshIndex]
            M = np.array(inst.transform[:], F).reshape(3, 4)
            self.xform[inst.customIndex] = M
            self.nmat[inst.customIndex] = np.linalg.inv(M[:, :3]).T                     # transpose(inverse(mat3(O2W))), closesthit.rchit:74
            tri = self.idx[me.indexOffset:me.indexOffset + me.indexCount].reshape(-1, 3).astype(np.int64) + me.vertexOffset
            P = self.verts[:, 0:3]
            w = [P[tri[:, k]] @ M[:, :3].T + M[:, 3] for k in range(3)]
            V0.append(w[0]); V1.append(w[1]); V2.append(w[2])
            cust.append(np.full(len(tri), inst.customIndex, np.int64)); prim.append(np.arange(len(tri), dtype=np.int64))
            tested = inst.customIndex >= self.numLights and self.objects[inst.customIndex - self.numLights].usesOpacityMap != 0 and me.isOpaque == 0
            alpha.append(np.full(len(tri), tested))
        cat = lambda xs, shape: np.concatenate(xs) if xs else np.zeros(shape)       # noqa: E731
        self.V0, self.V1, self.V2 = cat(V0, (0, 3)), cat(V1, (0, 3)), cat(V2, (0, 3))
        self.cust, self.prim, self.alpha = cat(cust, (0,)).astype(np.int64), cat(prim, (0,)).astype(np.int64), cat(alpha, (0,)).astype(bool)

    # ---- texture(): linear filter, repeat addressing, one mip (image_sampler.cppm:26-42) ------------------------------------
    @staticmethod
    def sample(img, u, v):
        H, W = img.shape[:2]
        x, y = (u - np.floor(u)) * W - 0.5, (v - np.floor(v)) * H - 0.5
        x0, y0 = np.floor(x), np.floor(y)
        fx, fy = (x - x0)[:, None], (y - y0)[:, None]
        x0, y0 = x0.astype(np.int64) % W, y0.astype(np.int64) % H
        x1, y1 = (x0 + 1) % W, (y0 + 1) % H
        a = img[y0, x0] * (1 - fx) + img[y0, x1] * fx
        b = img[y1, x0] * (1 - fx) + img[y1, x1] * fx
        out = a * (1 - fy) + b * fy
        if out.shape[1] == 1:                                                           # R8: (r, 0, 0, 1)
            out = np.concatenate([out, np.zeros_like(out), np.zeros_like(out), np.ones_like(out)], axis=1)
        return out

    # ---- ray / triangle, all rays against all triangles -------------------------------------------------------------------
    def _candidates(self, o, d, tmin, tmax):
        """(R, T) arrays t, u, v with t = inf where the ray misses the triangle (edge rule of intersect.rint:18-41)."""
        e1, e2 = self.V1 - self.V0, self.V2 - self.V0                                    # (T, 3)
        h = np.cross(d[:, None, :], e2[None, :, :])                                     # (R, T, 3)
        a = np.einsum("tk,rtk->rt", e1, h)
        with np.errstate(divide="ignore", invalid="ignore"):
            f = 1.0 / a
            s = o[:, None, :] - self.V0[None, :, :]
            u = f * np.einsum("rtk,rtk->rt", s, h)
            q = np.cross(s, e1[None, :, :])
            v = f * np.einsum("rk,rtk->rt", d, q)
            t = f * np.einsum("tk,rtk->rt", e2, q)
        ok = (np.abs(a) >= 1e-5) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t > tmin) & (t < tmax[:, None])
        return np.where(ok, t, np.inf), u, v

    def _alpha_reject(self, t, u, v):
        """opacity.rahit:31-64 for candidates on alpha-tested triangles: candidates whose opacity texel .r < 0.9 are ignored."""
        if not self.alpha.any():
            return t
        t = t.copy()
        for ti in np.nonzero(self.alpha)[0]:
            rows = np.nonzero(np.isfinite(t[:, ti]))[0]
            if len(rows) == 0:
                continue
            oi = self.objects[self.cust[ti] - self.numLights]
            tri = self.idx[oi.indexOffset + 3 * self.prim[ti]: oi.indexOffset + 3 * self.prim[ti] + 3].astype(np.int64) + oi.vertexOffset
            uv = self.verts[tri, 8:10]
            bu, bv = u[rows, ti], v[rows, ti]
            uu = uv[0, 0] * (1 - bu - bv) + uv[1, 0] * bu + uv[2, 0] * bv
            vv = uv[0, 1] * (1 - bu - bv) + uv[1, 1] * bu + uv[2, 1] * bv
            texel = self.sample(self.textures[oi.opacityIndex], uu, vv)
            t[rows[texel[:, 0] < 0.9], ti] = np.inf
        return t

    def closest(self, o, d, tmax):
        t, u, v = self._candidates(o, d, 0.001, np.full(len(o), tmax))
        t = self._alpha_reject(t, u, v)
        k = np.argmin(t, axis=1)                     # ties: the first in (instance, primitive) order = min (customIndex, primitiveID)
        r = np.arange(len(o))
        return np.isfinite(t[r, k]), k, t[r, k], u[r, k], v[r, k]

    def occluded(self, o, d, tmax):
        live = tmax > 0.001
        t, u, v = self._candidates(o, d, 0.001, tmax)
        t = self._alpha_reject(t, u, v)
        return live & np.isfinite(t).any(axis=1)

    # ---- cook-torrance.glsl ------------------------------------------------------------------------------------------------
    @staticmethod
    def ggx_d(n, h, alpha):
        noh = np.sum(n * h, -1)
        a2, noh2 = alpha * alpha, noh * noh
        den = np.maximum(noh2 * a2 + (1 - noh2), 0.001)
        return (noh > 0) * a2 / (np.pi * den * den)

    @staticmethod
    def ggx_g1(v, n, h, alpha):
        voh = np.clip(np.sum(v * h, -1), 0.001, 1.0)
        chi = (voh / np.clip(np.sum(v * n, -1), 0.001, 1.0)) > 0
        voh2 = voh * voh
        tan2 = (1 - voh2) / voh2
        return chi * 2 / (1 + np.sqrt(1 + alpha * alpha * tan2))

    def brdf(self, N, V, Ldir, color, metallic, roughness, mspec, ndotv_floor, ndotl_floor):
        H = normalize(V + Ldir)
        cosT = np.clip(np.sum(V * H, -1), 0, 1)
        D = self.ggx_d(N, H, roughness)
        G = self.ggx_g1(V, N, H, roughness) * self.ggx_g1(Ldir, N, H, roughness)
        Fr = mspec + (1 - mspec) * np.power(1 - cosT, 5.0)[:, None]
        ndv = np.maximum(np.sum(N * V, -1), ndotv_floor)
        ndl = np.maximum(np.sum(N * Ldir, -1), ndotl_floor)
        spec = (D * G)[:, None] * Fr / (4 * ndv * ndl)[:, None]
        diff = (1 - metallic)[:, None] * color / np.pi
        return spec + diff, ndl

    # ---- raygen.rgen for a set of pixels -------------------------------------------------------------------------------------
    def render(self, camera, info, params, xs, ys):
        """Returns (hdr (n,3) float64: pre-tonemap shadowed radiance, rgba8 (n,) uint32 packed B,G,R,255) for pixels (xs, ys)."""
        r = self.render_all(camera, info, params, xs, ys, analytic=False)
        return r["hdr"][A_SHADOWED], r["rgba8"][A_SHADOWED]

    def render_all(self, camera, info, params, xs, ys, analytic=True):
        """The five ray-gen images for pixels (xs, ys), keyed by rtr_image number (0 analytic, 1 shadowed, 2 unshadowed, 6 normal,
        7 position): {"hdr": float64 (n, 3) values before the pack — radiance before the tone map for 0 / 1 / 2, normalize(avg) and
        avg * POSITION_SCALE for 6 / 7 — and "rgba8": (n,) uint32 packed B,G,R,255}.  analytic needs the scene's LTC tables."""
        xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
        n = len(xs)
        cam = np.array(camera.position[:3], F)
        TL, dH, dV = (np.array(a[:3], F) for a in (camera.topLeftViewportCorner, camera.horizontalViewportDelta, camera.verticalViewportDelta))
        acc = {w: np.zeros((n, 3), F) for w in (A_ANALYTIC, A_SHADOWED, A_UNSHADOWED, A_NORMAL, A_POSITION)}
        ux, uy = xs.astype(np.uint32), ys.astype(np.uint32)
        for i in range(params.spp):
            with np.errstate(over="ignore"):
                jx, jy = pcg(ux + np.uint32(i)), pcg(ux + np.uint32(i) * np.uint32(322))     # raygen.rgen:83: both seeds use x only
            pw = TL + dH * (xs + jx - 0.5)[:, None] + dV * (ys + jy - 0.5)[:, None]
            # raygen.rgen:86-89 holds pixelWorldPos in an fp32 variable, one unit in front of a camera that stands hundreds of units from the
            # origin, and :92 subtracts the camera from it: the variable's representation error (half an ulp of 278, 1.5e-5) becomes a
            # relative error of 1.5e-5 in the direction, 0.02 units on a wall 1370 units away.  The ray the shader traces is defined by that
            # fp32 value, so the witness rounds the exact position to fp32 ONCE (nearest: no expression order is copied) and goes on in
            # float64.  Without it every fp32 evaluation of the shader traces rays this witness does not, and the position image — raw
            # coordinates as UNORM8, 1 LSB = 0.004 units — differed from the oracle's on 0.87 % of the Cornell box's pixels, by up to 4 LSB;
            # with it, on none of 3000 (tests/test_witness.py::test_five_images_normal_and_position).
            pw = pw.astype(np.float32).astype(F)
            rd = normalize(pw - cam)
            hit, k, t, bu, bv = self.closest(np.broadcast_to(cam, (n, 3)), rd, 10000.0)
            # miss.rmiss:15-27; raygen.rgen:110-121: a miss or a light adds its colour to all three and skips the G-buffer sums
            miss = ~hit
            if miss.any():
                sky = np.broadcast_to(self.sky, (miss.sum(), 3))
                if self.hdri is not None:
                    dd = rd[miss]
                    hu = np.arctan2(dd[:, 2], dd[:, 0]) / (2 * 3.14159265) + 0.5
                    hv = 1.0 - np.arccos(np.clip(dd[:, 1], -1, 1)) / 3.14159265
                    sky = np.power(self.sample(self.hdri, hu, hv)[:, :3], 2.2)
                for w in (A_ANALYTIC, A_SHADOWED, A_UNSHADOWED):
                    acc[w][miss] += sky
            cu = self.cust[k]
            islight = hit & (cu < self.numLights)
            for li in np.unique(cu[islight]):
                for w in (A_ANALYTIC, A_SHADOWED, A_UNSHADOWED):
                    acc[w][islight & (cu == li)] += np.array(self.lights[li].color[:3], F)
            surf = np.nonzero(hit & (cu >= self.numLights))[0]
            if len(surf) == 0:
                continue
            sh, un, an, N, P = self._shade(surf, xs, ys, cam, rd, k, bu, bv, info, params, analytic)
            acc[A_SHADOWED][surf] += sh; acc[A_UNSHADOWED][surf] += un; acc[A_ANALYTIC][surf] += an
            acc[A_NORMAL][surf] += N; acc[A_POSITION][surf] += P                      # raygen.rgen:132-133
        for w in acc:
            acc[w] /= params.spp
        with np.errstate(invalid="ignore", divide="ignore"):
            acc[A_NORMAL] = normalize(acc[A_NORMAL])                                    # raygen.rgen:359; 0 / 0 where no sample hit a surface
        acc[A_POSITION] = acc[A_POSITION] * POSITION_SCALE
        rgba = {w: self.pack(acc[w]) for w in (A_ANALYTIC, A_SHADOWED, A_UNSHADOWED)}
        rgba.update({w: self.pack_unorm(acc[w]) for w in (A_NORMAL, A_POSITION)})
        if not analytic:
            del acc[A_ANALYTIC], rgba[A_ANALYTIC]
        return {"hdr": acc, "rgba8": rgba}

    def _shade(self, rows, xs, ys, cam, rd, k, bu, bv, info, params, analytic):
        m = len(rows)
        out = np.zeros((m, 3), F); out_un = np.zeros((m, 3), F); out_an = np.zeros((m, 3), F)
        kk, u, v = k[rows], bu[rows], bv[rows]
        b0 = 1 - u - v
        P = np.zeros((m, 3), F); N = np.zeros((m, 3), F)
        color = np.zeros((m, 3), F); metallic = np.zeros(m, F); rough = np.zeros(m, F)
        for ci in np.unique(self.cust[kk]):                                             # closesthit.rchit:53-106, object by object
            sel = np.nonzero(self.cust[kk] == ci)[0]
            oi = self.objects[ci - self.numLights]
            tri = self.idx[(oi.indexOffset + 3 * self.prim[kk[sel]])[:, None] + np.arange(3)].astype(np.int64) + oi.vertexOffset
            vv = self.verts[tri]                                                        # (s, 3, 12)
            w = np.stack([b0[sel], u[sel], v[sel]], 1)[:, :, None]
            lp = np.sum(vv[:, :, 0:3] * w, 1)
            M = self.xform[ci]
            P[sel] = lp @ M[:, :3].T + M[:, 3]
            ns = np.sum(vv[:, :, 4:7] * w, 1)
            zero = np.sum(ns * ns, 1) <= 0
            g = np.cross(vv[:, 1, 0:3] - vv[:, 0, 0:3], vv[:, 2, 0:3] - vv[:, 0, 0:3])     # D1: geometric normal, facing the ray
            ns = np.where(zero[:, None], g, ns)
            nn = normalize(normalize(ns) @ self.nmat[ci].T)
            flip = zero & (np.sum(nn * rd[rows][sel], 1) > 0)
            N[sel] = np.where(flip[:, None], -nn, nn)
            uvw = np.sum(vv[:, :, 8:10] * w, 1)
            col = np.broadcast_to(np.array(oi.color[:3], F), (len(sel), 3)).copy()
            r_, me_ = np.full(len(sel), oi.specular, F), np.full(len(sel), oi.metallic, F)
            if oi.usesColorMap:
                col = self.sample(self.textures[oi.colorIndex], uvw[:, 0], uvw[:, 1])[:, :3]
            if oi.usesSpecularMap:
                r_ = self.sample(self.textures[oi.specularIndex], uvw[:, 0], uvw[:, 1])[:, 0]
            if oi.usesMetallicMap:
                me_ = self.sample(self.textures[oi.metallicIndex], uvw[:, 0], uvw[:, 1])[:, 0]
            color[sel] = np.power(col, 2.2); metallic[sel] = me_; rough[sel] = 1.0 - r_
        V = normalize(cam - P)
        mspec = 0.04 * (1 - metallic)[:, None] + color * metallic[:, None]              # mix(vec3(0.04), color, metallic)
        so = P + N * 0.01
        px, py = xs[rows].astype(np.uint32), ys[rows].astype(np.uint32)
        ns_ = params.numShadowRays
        if analytic:                                                                    # raygen.rgen:140-157
            mdiff = (1 - metallic)[:, None] * color
            dotnv = np.clip(np.sum(N * V, 1), 0.0, 1.0)
            lu, lv = rough * self.LUT_SCALE + self.LUT_BIAS, np.sqrt(1.0 - dotnv) * self.LUT_SCALE + self.LUT_BIAS
            t1, t2 = self.sample(self.ltc1, lu, lv), self.sample(self.ltc2, lu, lv)
            fresnel = mspec * t2[:, 0:1] + (1 - mspec) * t2[:, 1:2]                     # :280
        for li in range(info.numAreaLights):                                            # raygen.rgen:165-285
            L = self.lights[li]
            T = np.array(L.transform[:], F).reshape(4, 4).T                             # column-major mat4
            lcol = np.array(L.color[:3], F)
            for ti in range(L.numTriangles):
                j = self.idx[L.indexOffset + 3 * ti: L.indexOffset + 3 * ti + 3].astype(np.int64) + L.vertexOffset
                Pl = self.verts[j, 0:3] @ T[:3, :3].T + T[:3, 3]
                ln = np.cross(Pl[2] - Pl[1], Pl[0] - Pl[1])
                area = np.sqrt(ln @ ln) * 0.5
                pdf = 1.0 / (area * 0.7)
                ln = ln / np.sqrt(ln @ ln)
                front = np.ones(m, bool) if L.isTwoSided else ((P - Pl[0]) @ ln >= 0)
                acc = np.zeros((m, 3), F); acc_un = np.zeros((m, 3), F)
                for s in range(ns_):
                    with np.errstate(over="ignore"):
                        seed = np.uint32(s) + px * np.uint32(733) + py * np.uint32(1933) + np.uint32(info.frame)
                        r1, r2 = pcg(seed), pcg(seed + np.uint32(100))
                    # the fold is decided on the fp32 sum as the shader does it (r1, r2 are fp32 values)
                    fold = (r1.astype(np.float32) + r2.astype(np.float32)) > np.float32(1.0)
                    r1, r2 = np.where(fold, 1 - r1, r1), np.where(fold, 1 - r2, r2)
                    lp = Pl[0] + (Pl[1] - Pl[0]) * r1[:, None] + (Pl[2] - Pl[0]) * r2[:, None]
                    lv = lp - P
                    dist = np.sqrt(np.sum(lv * lv, 1))
                    ld = lv / dist[:, None]
                    vis = ~self.occluded(so, ld, dist - 0.5)
                    B, ndl = self.brdf(N, V, ld, color, metallic, rough, mspec, 0.1, 0.1)
                    Lr = lcol[None, :] * (L.intensity * ndl / (dist * dist) * 10.0)[:, None]
                    acc += vis[:, None] * B * Lr / pdf
                    acc_un += B * Lr / pdf                                              # :270: the same sum, visibility 1
                out += np.where(front[:, None], acc / ns_, 0.0)
                out_un += np.where(front[:, None], acc_un / ns_, 0.0)
                if analytic:                                                            # :277-283; `continue` at :196 skips it with the samples
                    two = bool(L.isTwoSided)
                    with np.errstate(invalid="ignore", divide="ignore"):
                        diffuse = self.ltc_evaluate(N, V, P, None, Pl, ln, two)
                        spec = self.ltc_evaluate(N, V, P, t1, Pl, ln, two)
                    a = lcol[None, :] * L.intensity * (spec[:, None] * fresnel + mdiff * diffuse[:, None]) * 5.0
                    out_an += np.where(front[:, None], a, 0.0)
        dl = np.array([-1.0, 1.0, -0.5], F); dl /= np.sqrt(dl @ dl)                    # raygen.rgen:289-338
        lit = N @ dl > 0
        if lit.any():
            r = np.nonzero(lit)[0]
            dd = np.broadcast_to(dl, (len(r), 3))
            vis = ~self.occluded(so[r], dd, np.full(len(r), 10000.0))
            B, ndl = self.brdf(N[r], V[r], dd, color[r], metallic[r], rough[r], mspec[r], 5.0, 0.0001)
            d = B * (np.array([1.0, 1.0, 0.5], F) * 0.2)[None, :] * (ndl * 20.0)[:, None]
            out[r] += vis[:, None] * d
            out_un[r] += d; out_an[r] += d                                              # :337-338
        return out, out_un, out_an, N, P

    # ---- LTC.glsl, raygen.rgen:65-67 -----------------------------------------------------------------------------------------
    LUT_SIZE = 64.0
    LUT_SCALE = (LUT_SIZE - 1.0) / LUT_SIZE
    LUT_BIAS = 0.5 / LUT_SIZE
    EDGE_A0 = 0.8543985                                                                 # class attributes so that a test can mutate its copy
    SWAP_T1_ZW = False
    FLIP_BEHIND = True

    def integrate_edge(self, v1, v2):
        """LTC.glsl:2-15.  The rational fit of theta / sin(theta) is the operation, not an approximation of it."""
        x = np.sum(v1 * v2, 1)
        y = np.abs(x)
        a = self.EDGE_A0 + (0.4965155 + 0.0145206 * y) * y
        b = 3.4175940 + (4.1616724 + y) * y
        v = a / b
        ts = np.where(x > 0.0, v, 0.5 / np.sqrt(np.maximum(1.0 - x * x, 1e-7)) - v)
        return np.cross(v1, v2) * ts[:, None]

    def ltc_evaluate(self, N, V, P, t1, points, light_normal, two_sided):
        """LTC.glsl:17-72; t1 = None is mat3(1).  Returns the scalar every component of Lo_i holds."""
        T1 = normalize(V - N * np.sum(V * N, 1)[:, None])
        T2 = np.cross(N, T1)
        Ls = []
        for k in range(3):
            w = points[k][None, :] - P
            q = np.stack([np.sum(T1 * w, 1), np.sum(T2 * w, 1), np.sum(N * w, 1)], 1)   # transpose(mat3(T1, T2, N)) * w
            if t1 is not None:                                                          # mat3(vec3(t1.x, 0, t1.y), vec3(0, 1, 0), vec3(t1.z, 0, t1.w)): columns
                c2x, c2z = (t1[:, 3], t1[:, 2]) if self.SWAP_T1_ZW else (t1[:, 2], t1[:, 3])
                q = np.stack([t1[:, 0] * q[:, 0] + c2x * q[:, 2], q[:, 1], t1[:, 1] * q[:, 0] + c2z * q[:, 2]], 1)
            Ls.append(normalize(q))
        behind = (points[0][None, :] - P) @ light_normal < 0.0
        vsum = self.integrate_edge(Ls[0], Ls[1]) + self.integrate_edge(Ls[1], Ls[2]) + self.integrate_edge(Ls[2], Ls[0])
        ln = np.sqrt(np.sum(vsum * vsum, 1))
        z = vsum[:, 2] / ln
        if self.FLIP_BEHIND:
            z = np.where(behind, -z, z)
        scale = self.sample(self.ltc2, (z * 0.5 + 0.5) * self.LUT_SCALE + self.LUT_BIAS, ln * self.LUT_SCALE + self.LUT_BIAS)[:, 3]
        out = ln * scale
        if not two_sided:
            out = np.where(behind, out, 0.0)
        return out

    @staticmethod
    def pack_unorm(c):
        """imageStore(vec4(v.b, v.g, v.r, 1)) into rgba8 without a tone map (raygen.rgen:363-364): clamp, round to nearest; NaN stores 0"""
        q = np.rint(np.clip(np.nan_to_num(np.asarray(c, F), nan=0.0), 0, 1) * 255.0).astype(np.uint32)
        return q[:, 2] | (q[:, 1] << 8) | (q[:, 0] << 16) | np.uint32(0xff000000)

    @staticmethod
    def pack(c):
        """ACESFilm, pow(1/2.2), imageStore(vec4(b, g, r, 1)) into rgba8 (raygen.rgen:45-59,345-357)."""
        x = np.asarray(c, F)
        with np.errstate(invalid="ignore", divide="ignore"):
            a = np.clip((x * (2.51 * x + 0.03)) / (x * (2.43 * x + 0.59) + 0.14), 0, 1)
        a = np.nan_to_num(a, nan=0.0)
        q = np.rint(np.power(a, 1 / 2.2) * 255.0).astype(np.uint32)
        return q[:, 2] | (q[:, 1] << 8) | (q[:, 0] << 16) | np.uint32(0xff000000)


# ---- ray / triangle for caller-supplied rays (the BVH conditioning tests) ----------------------------------------------------------
EPS_T = 2.0 ** -24          # fp32 unit roundoff


def ray_hits(v0, v1, v2, rays, chunk=1 << 21):
    """Closest hit of every RtrRay row (origin, tmin, direction, tmax) over the triangles (v0, v1, v2: (T, 3) float64 corners), by the
    intersect.rint rules (|det| >= 1e-5, 0 <= u <= 1, v >= 0, u + v <= 1, tmin < t < tmax; ties to the lower index) in float64.

    An fp32 evaluation of the same test can decide differently only near one of its boundaries.  For each ray and triangle the margin
    is 1e-6 in barycentrics plus the error bound of an fp32 evaluation, 8 eps |o - v0| max(|e1|, |e2|) / |det| (the cancellation in
    s = o - v0 grows with the distance of the origin and shrinks with the angle of incidence); a triangle whose barycentrics, det, or t
    against tmin / tmax lie within their margins is 'near'.  Returns (index or -1, t, u, v, t margin, ambiguous, ties) per ray: ambiguous
    rays are those with a near triangle (or non-finite input); ties counts the hits within the t margin of the closest one."""
    e1, e2 = v1 - v0, v2 - v0
    le = np.maximum(np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1))
    n = len(rays)
    best = np.full(n, -1, np.int64)
    bt, bu, bv, btol = np.full(n, np.inf), np.zeros(n), np.zeros(n), np.zeros(n)
    amb = np.zeros(n, bool)
    ties = np.zeros(n, np.int64)
    r64 = rays.astype(F)
    step = max(1, chunk // max(len(v0), 1))
    for lo in range(0, n, step):
        r = r64[lo:lo + step]
        o, d, tmin, tmax = r[:, 0:3], r[:, 4:7], r[:, 3], r[:, 7]
        h = np.cross(d[:, None, :], e2[None, :, :])
        a = np.einsum("tk,rtk->rt", e1, h)
        s = o[:, None, :] - v0[None, :, :]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            f = 1.0 / a
            u = f * np.einsum("rtk,rtk->rt", s, h)
            q = np.cross(s, e1[None, :, :])
            v = f * np.einsum("rk,rtk->rt", d, q)
            t = f * np.einsum("tk,rtk->rt", e2, q)
            ls = np.linalg.norm(s, axis=2)
            m = 1e-6 + 8 * EPS_T * ls * le[None, :] / np.abs(a)                      # barycentric margin
            tt = np.abs(t) * 1e-5 + 8 * EPS_T * ls * le[None, :] ** 2 / np.abs(a)    # t margin
            ma = 8 * EPS_T * np.linalg.norm(e1, axis=1)[None, :] * np.linalg.norm(h, axis=2)
            strict = ((np.abs(a) >= 1e-5 + ma) & (u >= m) & (u <= 1 - m) & (v >= m) & (u + v <= 1 - m) & (t > tmin[:, None] + tt)
                      & (t < tmax[:, None] - tt))
            loose = ((np.abs(a) >= 1e-5 - ma) & (u >= -m) & (u <= 1 + m) & (v >= -m) & (u + v <= 1 + m) & (t > tmin[:, None] - tt)
                     & (t < tmax[:, None] + tt))
        live = np.isfinite(r[:, :7]).all(1) & (d != 0).any(1)
        near = (loose & ~strict).any(1)
        ts = np.where(strict, t, np.inf)
        k = np.argmin(ts, axis=1)
        rows = np.arange(len(r))
        tk = ts[rows, k]
        hit = np.isfinite(tk)
        with np.errstate(invalid="ignore"):
            close = (strict & (np.abs(t - tk[:, None]) <= tt[rows, k][:, None] + tt)).sum(1)
        best[lo:lo + step] = np.where(hit, k, -1)
        bt[lo:lo + step], bu[lo:lo + step], bv[lo:lo + step] = tk, u[rows, k], v[rows, k]
        btol[lo:lo + step] = np.where(hit, tt[rows, k], 0.0)
        amb[lo:lo + step] = near | ~live
        ties[lo:lo + step] = close
    return best, bt, bu, bv, btol, amb, ties
