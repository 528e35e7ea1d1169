"""The test-side restatement the ray-flag tests (test_ray_flags_abi.py, test_gpu_ray_flags.py) rely on, in numpy float32, following
include/rtr_math.h operation for operation: the library is built with -ffp-contract=off, so an fma happens exactly where rtr_fma is
written and nowhere else, and a float32 restatement with an exact fma is bit-exact.

  fma32                 a correctly rounded float32 fma: the product of two float32 is exact in float64, the sum is rounded to odd in
                        float64 (two-sum gives the error's sign) and then once, to nearest even, to float32 — 53 bits are more than the
                        24 + 2 that makes the double rounding innocuous
  dot32, cross32        rtr_dot, rtr_cross
  mt32                  rtr_mt_intersect, which also returns the determinant a = rtr_dot(e1, rtr_cross(d, e2)) whose sign is the facing
  mirrored_by_custom    the mirrored bit of every instance, from the descriptor's transform, in float64
  AlphaWitness          alpha_pass / sample_tex of kernels/rtr_device.h (opacity.rahit): the opacity-map verdict of a candidate
  classify, filtered    the brute force over test_gpu_cull_masks.all_hits' candidates, filtered by mask, facing, opacity and alpha test"""
import ctypes as C

import numpy as np

from realtimeraytracer_amd import _abi as A

F32 = np.float32
MISS = 0xFFFFFFFF
EPS = F32(0.00001)
ANY, OPAQUE = A.QUERY_ANY, A.QUERY_OPAQUE
BACK, FRONT, CULL_OPAQUE, CULL_NO_OPAQUE = 0x10, 0x20, 0x40, 0x80


def fma32(a, b, c):
    a, b, c = (np.asarray(x, F32).astype(np.float64) for x in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b                                   # exact
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)             # p + c = s + err exactly
    s = np.atleast_1d(s).copy()
    err = np.broadcast_to(np.atleast_1d(err), s.shape)
    bits = s.view(np.uint64)
    fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((bits & np.uint64(1)) == 0)
    grow = fix & ((err > 0) == (s > 0))
    bits[grow] += np.uint64(1)
    bits[fix & ~grow] -= np.uint64(1)
    with np.errstate(over="ignore", under="ignore"):
        return s.astype(F32)


def dot32(a, b):
    return fma32(a[..., 2], b[..., 2], fma32(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))


def cross32(a, b):
    return np.stack([fma32(a[..., 1], b[..., 2], -(a[..., 2] * b[..., 1])),
                     fma32(a[..., 2], b[..., 0], -(a[..., 0] * b[..., 2])),
                     fma32(a[..., 0], b[..., 1], -(a[..., 1] * b[..., 0]))], axis=-1)


def det32(d, e1, e2):
    """a of rtr_mt_intersect: (N,) float32 for (N, 3) operands (d may be one direction)"""
    e1, e2 = np.atleast_2d(np.asarray(e1, F32)), np.atleast_2d(np.asarray(e2, F32))
    d = np.broadcast_to(np.asarray(d, F32), e2.shape)
    return dot32(e1, cross32(d, e2))


def mt32(o, d, v0, e1, e2, tmin):
    """rtr_mt_intersect for one ray against (N, 3) records: ok, t, u, v, a"""
    v0, e1, e2 = (np.atleast_2d(np.asarray(x, F32)) for x in (v0, e1, e2))
    o = np.broadcast_to(np.asarray(o, F32), v0.shape)
    d = np.broadcast_to(np.asarray(d, F32), v0.shape)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        h = cross32(d, e2)
        a = dot32(e1, h)
        ok = ~(np.abs(a) < EPS)
        f = F32(1.0) / a
        s = o - v0
        u = f * dot32(s, h)
        ok &= ~((u < 0) | (u > 1))
        q = cross32(s, e1)
        v = f * dot32(d, q)
        ok &= ~((v < 0) | (u + v > F32(1.0)))
        t = f * dot32(e2, q)
        ok &= t > F32(tmin)
    return ok, t, u, v, a


def mirrored_by_custom(desc, instances=None):
    """per customIndex: is the determinant of the instance's 3x3 transform negative?  float64."""
    out = np.zeros(desc.numInstances, bool)
    for i in range(desc.numInstances):
        inst = instances[i] if instances is not None else desc.instances[i]
        m = np.array(inst.transform[:], np.float64).reshape(3, 4)[:, :3]
        out[inst.customIndex] = np.linalg.det(m) < 0.0
    return out


def _arr(ptr, n, dtype, width):
    if n == 0:
        return np.zeros((0, width), dtype)
    buf = C.cast(ptr, C.POINTER(C.c_uint8 * (n * width * np.dtype(dtype).itemsize))).contents
    return np.frombuffer(buf, dtype=dtype).reshape(n, width).copy()


class AlphaWitness:
    """alpha_pass(custom, prim, u, v) of kernels/rtr_device.h in float32; texel() also returns the filtered value"""

    def __init__(self, desc):
        d = desc
        self.uv = _arr(d.vertices, d.numVertices, F32, 12)[:, 8:10]
        self.idx = _arr(d.indices, d.numIndices, np.uint32, 1).reshape(-1).astype(np.int64)
        self.numLights = d.numLights
        self.objects = [A.RtrObjectInfo.from_buffer_copy(d.objects[i]) for i in range(d.numObjects)]
        self.tex = []
        for t in range(d.numTextures):
            tx = d.textures[t]
            if not tx.pixels:
                self.tex.append(None)
                continue
            px = np.frombuffer(C.cast(tx.pixels, C.POINTER(C.c_uint8 * (tx.width * tx.height * tx.channels))).contents, dtype=np.uint8).copy()
            self.tex.append((px, int(tx.width), int(tx.height), int(tx.channels)))

    @staticmethod
    def _unorm8(b):
        x = F32(b)
        return fma32(x, F32(0.0039215688593685627), x * F32(-2.3191758e-10))[0]

    def _sample_r(self, tex, u, v):
        px, W, H, ch = tex
        u, v = F32(u), F32(v)
        if not (u > F32(-1.0e9) and u < F32(1.0e9)):
            u = F32(0.0)
        if not (v > F32(-1.0e9) and v < F32(1.0e9)):
            v = F32(0.0)
        uf, vf = F32(u - np.floor(u)), F32(v - np.floor(v))
        x, y = fma32(uf, F32(W), F32(-0.5))[0], fma32(vf, F32(H), F32(-0.5))[0]
        x0f, y0f = np.floor(x), np.floor(y)
        fx, fy = F32(x - x0f), F32(y - y0f)
        x0, y0 = int(x0f), int(y0f)
        if x0 < 0:
            x0 += W
        if x0 >= W:
            x0 -= W
        if y0 < 0:
            y0 += H
        if y0 >= H:
            y0 -= H
        x1, y1 = x0 + 1, y0 + 1
        if x1 >= W:
            x1 -= W
        if y1 >= H:
            y1 -= H
        at = (lambda yy, xx: px[(yy * W + xx) * 4]) if ch == 4 else (lambda yy, xx: px[yy * W + xx])
        t00, t10, t01, t11 = (self._unorm8(at(y0, x0)), self._unorm8(at(y0, x1)), self._unorm8(at(y1, x0)), self._unorm8(at(y1, x1)))
        a = fma32(F32(t10 - t00), fx, t00)[0]
        b = fma32(F32(t11 - t01), fx, t01)[0]
        return fma32(F32(b - a), fy, a)[0]

    def texel(self, custom, prim, bu, bv):
        """the opacity texel alpha_pass compares with 0.9, or None where the object has no opacity map (the candidate passes)"""
        oi = self.objects[custom - self.numLights]
        if oi.usesOpacityMap == 0:
            return None
        i = self.idx[oi.indexOffset + 3 * prim: oi.indexOffset + 3 * prim + 3] + oi.vertexOffset
        uv0, uv1, uv2 = self.uv[i[0]], self.uv[i[1]], self.uv[i[2]]
        bu, bv = F32(bu), F32(bv)
        b0 = F32(F32(F32(1.0) - bu) - bv)
        uu = fma32(uv2[0], bv, fma32(uv1[0], bu, uv0[0] * b0))[0]
        vv = fma32(uv2[1], bv, fma32(uv1[1], bu, uv0[1] * b0))[0]
        return self._sample_r(self.tex[oi.opacityIndex], uu, vv)

    def passes(self, custom, prim, bu, bv):
        t = self.texel(custom, prim, bu, bv)
        return True if t is None else not (t < F32(0.9))


def classify(cands, rays, bvh, mirrored, alpha):
    """per ray, per candidate of all_hits (t, u, v, customIndex, primitiveId): (front, bit 0 of the record's flags, passes the opacity
    map).  front = (a > 0) XOR mirrored[customIndex], a restated in float32 from the exported record."""
    raw = np.frombuffer(bvh[1], dtype=np.uint32).reshape(-1, 12)
    flt = raw.view(F32)
    where = {(int(c), int(p)): j for j, (c, p) in enumerate(zip(raw[:, 3], raw[:, 7]))}
    out = []
    for r, (ts, us, vs, cs, ps) in zip(rays, cands):
        if not ts:
            out.append(([], [], []))
            continue
        js = np.array([where[(c, p)] for c, p in zip(cs, ps)])
        a = det32(r[4:7], flt[js, 4:7], flt[js, 8:11])
        assert (np.abs(a) >= EPS).all(), "an accepted candidate's determinant is never within RTR_MT_EPSILON of 0"
        front = [bool((x > 0) != mirrored[c]) for x, c in zip(a, cs)]
        bit0 = [bool(raw[j, 11] & 1) for j in js]
        ok = [alpha.passes(c, p, u, v) if b else True for c, p, u, v, b in zip(cs, ps, us, vs, bit0)]
        out.append((front, bit0, ok))
    return out


def filtered(cands, classes, rays, flags, custom_masks=None, ray_masks=0xff):
    """the expected closest hit and occlusion byte of every ray under flags (RTR_QUERY_OPAQUE and the four culling flags), the instance
    masks (by customIndex; None: 0xff) and the rays' masks"""
    n = len(rays)
    t = rays[:, 7].copy(); u = np.zeros(n, F32); v = np.zeros(n, F32)
    cu = np.full(n, MISS, np.int64); pr = np.full(n, MISS, np.int64)
    occ = np.zeros(n, np.uint8)
    ray_masks = np.broadcast_to(np.asarray(ray_masks, np.int64), (n,))
    for k, ((ts, us, vs, cs, ps), (front, bit0, ok)) in enumerate(zip(cands, classes)):
        best = None
        for tt, uu, vv, c, p, fr, b0, al in zip(ts, us, vs, cs, ps, front, bit0, ok):
            if custom_masks is not None and not (custom_masks[c] & ray_masks[k]):
                continue
            if custom_masks is None and not ray_masks[k]:
                continue
            nonopaque = b0 and not (flags & OPAQUE)
            if (flags & CULL_OPAQUE and not nonopaque) or (flags & CULL_NO_OPAQUE and nonopaque):
                continue
            if (flags & FRONT and fr) or (flags & BACK and not fr):
                continue
            if nonopaque and not al:
                continue
            if best is None or (tt, c, p) < best[0]:
                best = ((tt, c, p), uu, vv)
        if best is not None:
            (t[k], cu[k], pr[k]), u[k], v[k] = best[0], best[1], best[2]
            occ[k] = 1
    return (t, u, v, cu, pr), occ
