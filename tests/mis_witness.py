"""A float64 numpy restatement of the estimator of include/rtr_mis.h, written from its formulas and not from the header: the balance
heuristic's weights, the radiance of a bounce ray that ends on a light, the light loops' sample point and contribution, a
Moeller-Trumbore for one triangle and the quadrature the estimates are held to.  No test in here; test_mis_host.py and test_gpu_mis.py
import it.

Notation: at a vertex x with normal N a light triangle t (corners P0 P1 P2, area, unit normal n_t, pdfrec = 1 / (0.7 area)) is seen in
direction L at distance d, cosL = dot(n_t, -L).  One pick has the solid-angle density q = d^2 / (Ttot area |cosL|); with s = d^2 / (Ttot
area) the balance heuristic over P picks and one bounce of density pb is wPick = P s / (P s + pb |cosL|), wBounce = pb |cosL| / (same)."""
import numpy as np

import bounce_witness as W


def weights(pb, dist, cos_light, area, tris, picks):
    """-> (lightPdf, wPick, wBounce) in float64 from the float32 inputs; 0 / 0 is 0 and lightPdf is 0 where it is not finite"""
    pb, dist, cos_light, area = (np.asarray(x, np.float64) for x in (pb, dist, cos_light, area))
    with np.errstate(all="ignore"):
        s = dist * dist / (tris * area) if tris else np.zeros_like(dist)
        a = picks * s if (tris and picks) else np.zeros_like(dist)
        b = np.where(pb > 0.0, pb * np.abs(cos_light), 0.0)
        den = a + b
        ok = den > 0.0
        w_pick = np.where(ok, a / np.where(ok, den, 1.0), 0.0)
        w_bounce = np.where(ok, b / np.where(ok, den, 1.0), 0.0)
        q = s / np.abs(cos_light)
        q = np.where(np.isfinite(q) & ok & (tris != 0), q, 0.0)
    return q, w_pick, w_bounce


def intermediates(pb, dist, cos_light, area, tris, picks):
    """the float64 values of every intermediate of the final form that is rounded in float32: d^2, Ttot area, s, P s, pb |cosL|, the sum"""
    pb, dist, cos_light, area = (np.asarray(x, np.float64) for x in (pb, dist, cos_light, area))
    with np.errstate(all="ignore"):
        d2, ta = dist * dist, tris * area
        s = d2 / ta
        a = picks * s
        b = pb * np.abs(cos_light)
        out = [b, a + b] if (tris and picks) else [b]
        if tris and picks:
            out += [d2, ta, s, a]
    return out


def tri_record(p0, p1, p2):
    """the float32 (16,) record the scene keeps for a light triangle: {P0, area} {P1, pdfrec} {P2, 0} {unit normal, 0}, the normal
    cross(P2 - P1, P0 - P1) as the light loops form it"""
    p0, p1, p2 = (np.asarray(p, np.float32) for p in (p0, p1, p2))
    n = np.cross((p2 - p1).astype(np.float64), (p0 - p1).astype(np.float64))
    area = np.float32(0.5 * np.linalg.norm(n))
    rec = np.zeros(16, np.float32)
    rec[0:3], rec[3] = p0, area
    rec[4:7], rec[7] = p1, np.float32(1.0) / (area * np.float32(0.7))
    rec[8:11] = p2
    rec[12:15] = n / np.linalg.norm(n)
    return rec


def light_points(rec, seeds, sample=0, frame=0):
    """the point of light triangle rec that sample `sample` of the hits with seed bases `seeds` aims at (raygen.rgen:206-215): r1, r2 =
    rtr_random(sample + seed + frame), rtr_random(the same + 100), folded into the triangle -> float64 (N, 3)"""
    sd = (np.asarray(seeds).astype(np.uint64) + sample + frame) & 0xffffffff
    r1, r2 = W.rtr_random(sd), W.rtr_random((sd + 100) & 0xffffffff)
    fold = (r1 + r2) > np.float32(1.0)
    r1 = np.where(fold, np.float32(1.0) - r1, r1).astype(np.float64)
    r2 = np.where(fold, np.float32(1.0) - r2, r2).astype(np.float64)
    p0, p1, p2 = (rec[i:i + 3].astype(np.float64) for i in (0, 4, 8))
    return p0 + (p1 - p0) * r1[:, None] + (p2 - p0) * r2[:, None]


def contribution(points, x, N, V, roughness, F0, om, color, light_color, intensity, pdfrec):
    """c = f(L) (col I max(NL, 0.1) 10 / d^2) / pdfrec for the light points seen from x -> (c (M, 3), L (M, 3), d (M,))"""
    v = points - x
    d = np.sqrt(np.sum(v * v, axis=-1))
    L = v / d[..., None]
    f = W.brdf(N, V, L, roughness, F0, om, color)
    nl = np.maximum(np.sum(N * L, axis=-1), 0.1)
    return f * (np.asarray(light_color, np.float64) * intensity * 10.0) * (nl / (d * d) / pdfrec)[..., None], L, d


def quadrature(rec, n, x, N, V, roughness, F0, om, color, light_color, intensity):
    """(1 / (area pdfrec)) * the integral over the triangle of f col I max(NL, 0.1) 10 / d^2 dA on the n-per-edge barycentric midpoint
    grid (the centroids of the n^2 congruent sub-triangles, each of area / n^2), which is the mean of contribution() over the grid"""
    p0, p1, p2 = (rec[i:i + 3].astype(np.float64) for i in (0, 4, 8))
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    up = (i + j) < n                      # the upright sub-triangles (i, j), centroid (i + 1/3, j + 1/3) / n
    down = (i + j) < n - 1                # the inverted ones between them, centroid (i + 2/3, j + 2/3) / n
    u = np.concatenate([(i[up] + 1.0 / 3.0), (i[down] + 2.0 / 3.0)]) / n
    v = np.concatenate([(j[up] + 1.0 / 3.0), (j[down] + 2.0 / 3.0)]) / n
    assert u.size == n * n
    pts = p0 + (p1 - p0) * u[:, None] + (p2 - p0) * v[:, None]
    c, _, _ = contribution(pts, x, N, V, roughness, F0, om, color, light_color, intensity, float(rec[7]))
    return c.mean(axis=0)


def moller_trumbore(o, d, rec):
    """rays (o, d) (N, 3) float64 against the triangle of rec -> (hit (N,) bool, t, u, v): either face, t > 0"""
    p0, p1, p2 = (rec[i:i + 3].astype(np.float64) for i in (0, 4, 8))
    e1, e2 = p1 - p0, p2 - p0
    with np.errstate(all="ignore"):
        pv = np.cross(d, e2)
        det = pv @ e1
        inv = 1.0 / det
        tv = o - p0
        u = np.sum(tv * pv, axis=1) * inv
        qv = np.cross(tv, e1)
        v = np.sum(d * qv, axis=1) * inv
        t = (qv @ e2) * inv
        hit = (np.abs(det) > 1e-12) & (u >= 0.0) & (v >= 0.0) & (u + v <= 1.0) & (t > 0.0)
    return hit, t, u, v


def emitter_radiance(nl, light_color, intensity, pdfrec, area, pb, dist, cos_light, tris, picks):
    """(max(NL, 0.1) / NL) (10 col I / (pdfrec area)) pb / (P s + pb |cosL|) per channel"""
    s = dist * dist / (tris * area) if tris else 0.0
    den = picks * s + pb * np.abs(cos_light)
    return (np.maximum(nl, 0.1) / nl * pb / den)[..., None] * (10.0 * np.asarray(light_color, np.float64) * intensity / (pdfrec * area))
