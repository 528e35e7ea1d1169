"""The host forms of include/rtr_mis.h without a device: rtr_host_bounce_pdf against rtr_host_bounce_rays' own density bit for bit, the
balance heuristic's weights on a grid with its edge cases against the float64 restatement of tests/mis_witness.py, and the estimator
itself — NEE-only picks and the MIS of picks and bounce, both against a quadrature over the light triangle."""
import itertools

import numpy as np
import pytest

import bounce_witness as W
import mis_witness as M
from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api

BOTH = A.BOUNCE_DIFFUSE | A.BOUNCE_SPECULAR
ULP1 = float(np.spacing(np.float32(1.0)))          # 2^-23


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---- 1. the bounce density for a direction handed in ---------------------------------------------------------------------------------
@pytest.mark.parametrize("lobes", [BOTH, A.BOUNCE_DIFFUSE, A.BOUNCE_SPECULAR])
def test_bounce_pdf_is_the_samples_own_density_bit_for_bit(lobes):
    rays, sf, seeds = W.make_surfaces(20000)
    h = api.host_bounce_rays(rays, sf, api.make_bounce_params(lobes=lobes), seeds)
    live = h.lobe != 0
    assert live.sum() > 5000
    pdf = api.host_bounce_pdf(rays[live], sf[live], h.rays[live, 4:7], lobes)
    assert (_bits(pdf) == _bits(h.pdf[live])).all(), f"{(_bits(pdf) != _bits(h.pdf[live])).sum()} of {live.sum()} densities differ from RtrBounce::pdf"
    # below the horizon: the drawn direction mirrored through the surface, and straight down
    N = sf[live, 4:7]
    L = h.rays[live, 4:7]
    below = (L - 2.0 * np.sum(N * L, axis=1, dtype=np.float32)[:, None] * N).astype(np.float32)
    assert np.sum(below * N, axis=1).max() < 0.0
    assert not api.host_bounce_pdf(rays[live], sf[live], below, lobes).any()
    assert not api.host_bounce_pdf(rays[live], sf[live], -N, lobes).any()


@pytest.mark.parametrize("lobes", [BOTH, A.BOUNCE_DIFFUSE, A.BOUNCE_SPECULAR])
def test_bounce_pdf_is_the_samples_own_density_over_the_sphere_of_views(lobes):
    """the same on the records whose views are not mirrored into the upper hemisphere: views from behind the shading normal, the
    grazing band, dot(N, V) exactly 0"""
    rays, sf, seeds = W.make_surfaces(20000, views="sphere")
    h = api.host_bounce_rays(rays, sf, api.make_bounce_params(lobes=lobes), seeds)
    live = h.lobe != 0
    assert live.sum() > 5000
    pdf = api.host_bounce_pdf(rays[live], sf[live], h.rays[live, 4:7], lobes)
    assert (_bits(pdf) == _bits(h.pdf[live])).all(), f"{(_bits(pdf) != _bits(h.pdf[live])).sum()} of {live.sum()} densities differ from RtrBounce::pdf"
    assert not api.host_bounce_pdf(rays[live], sf[live], -sf[live, 4:7], lobes).any()


def test_bounce_pdf_is_zero_for_dead_surfaces_and_nan_input():
    rays, sf, seeds = W.make_surfaces(64, seed=5)
    h = api.host_bounce_rays(rays, sf, api.make_bounce_params(), seeds)
    live = np.flatnonzero(h.lobe != 0)[:8]
    assert live.size == 8
    for name, ray, s, lobes in W.dead_cases():
        d = api.host_bounce_rays(ray[None], s[None], api.make_bounce_params(lobes=lobes), np.zeros(1, np.uint32))
        assert d.lobe[0] == 0, name
        for k in live:                    # whatever direction is asked about
            assert api.host_bounce_pdf(ray[None], s[None], h.rays[k:k + 1, 4:7], lobes)[0] == 0.0, name
    r, s, L = rays[live], sf[live], h.rays[live, 4:7].copy()
    assert api.host_bounce_pdf(r, s, L).all()
    for bad in (np.nan, np.inf, -np.inf):
        for col in range(3):
            Lb = L.copy()
            Lb[:, col] = bad
            out = api.host_bounce_pdf(r, s, Lb)
            assert not out.any() and np.isfinite(out).all()
        sb = s.copy()
        sb[:, 15] = bad
        assert not api.host_bounce_pdf(r, sb, L).any()
    lib = A.hip_lib()
    assert lib.rtr_host_bounce_pdf(None, None, None, 0, 0, None) == -1 and lib.rtr_last_error().decode().startswith("rtr_host_bounce_pdf: lobes 0x0")


# ---- 2. the weights ------------------------------------------------------------------------------------------------------------------
DENORMAL = float(np.float32(1e-40))
GRID_PB = [0.0, DENORMAL, 1e-3, 0.31830987, 7.5, 4.0e4]
GRID_DIST = [0.0, DENORMAL, 1e-3, 0.7, 2.0, 55.0, 1.0e4]
GRID_COS = [0.0, DENORMAL, -1e-3, 0.05, -0.6, 1.0]
GRID_AREA = [DENORMAL, 1e-4, 0.35, 2.0, 1.0e3]
GRID_TRIS_PICKS = [(0, 1), (1, 0), (0, 0), (1, 1), (2, 1), (5, 2), (12, 30), (1000, 4)]
# The final forms round: d * d, Ttot * area, their quotient, its product by P (4 roundings in a = P s); pb * |cosL| (1 in b); the sum (1); the
# quotient (1).  To first order wPick = a / (a + b) is off by at most 4 (from a) + 4 (the sum carries a's and b's, at most a's 4) + 1 (sum) +
# 1 (quotient) = 10 relative roundings of 2^-24 each, and wBounce by no more: the bound is (10 + 2) * 2^-24, the 2 for the second order.
ROUNDINGS = 10
WEIGHT_BOUND = (ROUNDINGS + 2) * 2.0 ** -24
FLT_MIN, FLT_MAX = 1.17549435e-38, 3.4028235e38


def test_mis_weights_on_a_grid():
    pb, dist, cosl, area = (np.array(x, np.float32) for x in zip(*itertools.product(GRID_PB, GRID_DIST, GRID_COS, GRID_AREA)))
    worst = 0.0
    compared = 0
    for tris, picks in GRID_TRIS_PICKS:
        s, wb = api.host_mis_weights(pb, dist, cosl, area, tris, picks)
        q, wp = s[:, 0], s[:, 2]
        assert np.isfinite(s[:, :6]).all() and np.isfinite(wb).all() and not s.view(np.uint32)[:, 6:8].any()
        assert (_bits(s[:, 1]) == _bits(pb)).all() and (_bits(s[:, 3]) == _bits(cosl)).all() and (_bits(s[:, 4]) == _bits(dist)).all() and (_bits(s[:, 5]) == _bits(area)).all()
        assert (wp >= 0).all() and (wp <= 1).all() and (wb >= 0).all() and (wb <= 1).all() and (q >= 0).all()
        nobody = tris == 0 or picks == 0
        b_zero = (pb == 0) | (cosl == 0)
        # the edge cases, exactly
        if nobody:
            assert (wp == 0).all() and (wb[~b_zero & (pb * np.abs(cosl) > 0)] == 1).all() and (wb[b_zero] == 0).all()
        else:
            sel = (pb == 0) & (dist.astype(np.float64) ** 2 >= FLT_MIN)
            assert (wp[sel] == 1).all() and (wb[sel] == 0).all(), "pb == 0: the pick takes it all"
        if tris == 0:
            assert (q == 0).all()
        some = (wp != 0) | (wb != 0)
        total = wp.astype(np.float64) + wb.astype(np.float64)
        assert np.abs(total[some] - 1.0).max() <= 2 * ULP1, "the weights do not add up to 1 within 2 ulp"
        # the float64 restatement, wherever no intermediate of the final form leaves float32's normal range (a bound counted in
        # roundings says nothing about an underflow or an overflow)
        q64, wp64, wb64 = M.weights(pb, dist, cosl, area, tris, picks)
        normal = np.ones(pb.size, bool)
        for x in M.intermediates(pb, dist, cosl, area, tris, picks):
            normal &= (x == 0.0) | ((np.abs(x) >= FLT_MIN) & (np.abs(x) <= FLT_MAX))
        normal &= area >= FLT_MIN
        assert normal.sum() > 0.3 * pb.size
        e = max(np.abs(wp[normal] - wp64[normal]).max(), np.abs(wb[normal] - wb64[normal]).max())
        worst = max(worst, e)
        compared += int(normal.sum())
        assert e <= WEIGHT_BOUND, (tris, picks, e)
        qn = normal & (q64 >= FLT_MIN) & (q64 <= FLT_MAX) & (np.abs(cosl) >= FLT_MIN)
        assert (np.abs(q[qn] - q64[qn]) <= 4 * 2.0 ** -24 * q64[qn]).all(), "lightPdf: three roundings behind the inputs"
    print(f"weights against float64: worst |error| {worst:.3e} over {compared} points (bound {WEIGHT_BOUND:.3e}, {ROUNDINGS} roundings)")


def test_mis_weights_refuse_and_survive_bad_input():
    lib = A.hip_lib()
    one = np.ones(1, np.float32)
    out = np.zeros((1, 8), np.float32)
    p = lambda x: x.ctypes.data_as(A.VP)
    assert lib.rtr_host_mis_weights(1, p(one), p(one), p(one), p(one), 1, 31, p(out), None) == -1
    assert lib.rtr_last_error().decode().startswith("rtr_host_mis_weights: P 31")
    assert lib.rtr_host_mis_weights(1, None, p(one), p(one), p(one), 1, 1, p(out), None) == -1 and "pb is null" in lib.rtr_last_error().decode()
    assert lib.rtr_host_mis_weights(1, p(one), p(one), p(one), p(one), 1, 1, None, None) == -1 and "outSamples is null" in lib.rtr_last_error().decode()
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(4):
            args = [np.float32(0.5)] * 4
            args[k] = np.float32(bad)
            s, wb = api.host_mis_weights(*[[a] for a in args], 3, 2)
            assert s[0, 0] == 0 and s[0, 2] == 0 and wb[0] == 0, (bad, k)
    # a triangle so small that P s overflows: the pick takes it all
    s, wb = api.host_mis_weights([1.0], [1.0e4], [0.5], [DENORMAL], 1, 1)
    assert s[0, 2] == 1.0 and wb[0] == 0.0 and np.isfinite(s).all()


# ---- 3. the estimator ----------------------------------------------------------------------------------------------------------------
TRIANGLES = {
    "overhead": ((-1, -1, 2), (1, -1, 2), (0, 1, 2)),
    "grazing": ((1, -1, 0.05), (6, 0, 0.3), (1, 1, 1.5)),
    "straddling": ((1, -1, -0.5), (3, 0, 1), (1, 1, 0.2)),
}
MATERIALS = [(r, m) for r in (0.1, 0.4, 1.0) for m in (0.0, 1.0)]
SEEDS = 200000
COLOR = np.array([0.8, 0.6, 0.4], np.float32)
LIGHT_COLOR, INTENSITY = np.array([1.0, 0.8, 0.6], np.float32), np.float32(5.0)
# dot(N, V) = 0.9 and the mirror direction (-Vx, -Vy, Vz) meets the plane z = 2 at (0.546, -0.8), inside the overhead triangle
_m = np.array([0.546, -0.8, 2.0])
_m[:2] *= np.sqrt(4.0 * (1.0 / 0.81 - 1.0)) / np.linalg.norm(_m[:2])
VIEW = np.array([-_m[0], -_m[1], _m[2]]) / np.linalg.norm(_m)


@pytest.fixture(scope="module")
def view():
    assert abs(VIEW[2] - 0.9) < 1e-12
    ray = np.zeros((1, 8), np.float32)
    ray[0, 0:3], ray[0, 3], ray[0, 7] = VIEW * 5.0, 0.001, 10000.0
    ray[0, 4:7] = -VIEW
    rec = M.tri_record(*TRIANGLES["overhead"])
    hit, t, u, v = M.moller_trumbore(np.zeros((1, 3)), np.array([[-VIEW[0], -VIEW[1], VIEW[2]]]), rec)
    assert hit[0] and min(u[0], v[0], 1 - u[0] - v[0]) > 0.05, "the mirror direction does not meet the overhead triangle"
    return ray


def _view_ray(nov):
    """a ray that sees the origin from the azimuth of VIEW at dot(N, V) = nov"""
    v = np.array([VIEW[0], VIEW[1], 0.0]) / np.hypot(VIEW[0], VIEW[1]) * np.sqrt(1.0 - nov * nov) + np.array([0.0, 0.0, nov])
    ray = np.zeros((1, 8), np.float32)
    ray[0, 0:3], ray[0, 3], ray[0, 7] = v * 5.0, 0.001, 10000.0
    ray[0, 4:7] = -v
    return ray


def _nee_and_mis(view, tri, roughness, metallic, n_seeds, normal_offset, first_seed=0, finest_grid=512):
    """-> {"NEE": (N, 3), "MIS": (N, 3), "bounce": (N, 3)} estimates per seed, the quadrature c512 and the share of bounce rays on the light"""
    rec = M.tri_record(*TRIANGLES[tri])
    area, pdfrec, nt = float(rec[3]), float(rec[7]), rec[12:15].astype(np.float64)
    sf = np.zeros((1, 20), np.float32)
    sf[0, 4:7] = sf[0, 8:11] = (0, 0, 1)
    sf.view(np.uint32)[0, 3] = A.SURFACE_OBJECT
    sf[0, 12:15], sf[0, 11], sf[0, 15] = COLOR, metallic, roughness
    x, N = np.zeros(3), np.array([0.0, 0.0, 1.0])
    V = view[0, 0:3].astype(np.float64) / np.linalg.norm(view[0, 0:3].astype(np.float64))
    r32, m32 = float(np.float32(roughness)), float(np.float32(metallic))
    om = 1.0 - m32
    F0 = COLOR.astype(np.float64) * m32 + 0.04 * om
    mat = (x, N, V, r32, F0, om, COLOR.astype(np.float64), LIGHT_COLOR, float(INTENSITY))
    # (c) and its condition
    # (from behind, the edge of the specular term, dot(N, Hm) = 0, can cross the triangle, and the grid has to be finer for the same 1e-4:
    # finest_grid, which only the views from behind raise)
    n_grid, c256 = 512, M.quadrature(rec, 256, *mat)
    c512 = M.quadrature(rec, n_grid, *mat)
    while not (np.abs(c512 - c256) <= 1e-4 * np.abs(c512)).all() and n_grid < finest_grid:
        n_grid, c256 = 2 * n_grid, c512
        c512 = M.quadrature(rec, n_grid, *mat)
    assert (np.abs(c512 - c256) <= 1e-4 * np.abs(c512)).all(), f"the quadrature has not converged: {c512} at {n_grid}, {c256} at {n_grid // 2}"
    # (a) the NEE-only estimate: Ttot = 1, P = 1, the default weight 1
    seeds = np.arange(first_seed, first_seed + n_seeds, dtype=np.uint32)
    pts = M.light_points(rec, seeds)
    c, L, d = M.contribution(pts, *mat[:7], LIGHT_COLOR, float(INTENSITY), pdfrec)
    nee = c
    # (b) the picks under MIS ...
    rays, sfs = np.repeat(view, n_seeds, axis=0), np.repeat(sf, n_seeds, axis=0)
    L32, d32 = L.astype(np.float32), d.astype(np.float32)
    cosl = np.sum(nt * -L, axis=1).astype(np.float32)
    pb = api.host_bounce_pdf(rays, sfs, L32)
    smp, _ = api.host_mis_weights(pb, d32, cosl, np.full(n_seeds, rec[3]), 1, 1)
    pick_term = c * smp[:, 2].astype(np.float64)[:, None]
    # ... and the bounce: host_bounce_rays' ray, met with the triangle here, host_emitter_hits' radiance times the bounce weight
    b = api.host_bounce_rays(rays, sfs, api.make_bounce_params(normal_offset=normal_offset), seeds)
    hit, t, u, v = M.moller_trumbore(b.rays[:, 0:3].astype(np.float64), b.rays[:, 4:7].astype(np.float64), rec)
    hit &= (b.lobe != 0) & (t >= 0.001)
    hits = np.zeros((n_seeds, 8), np.float32)
    hw = hits.view(np.uint32)
    hits[:, 0] = 10000.0
    hw[:, 3] = hw[:, 4] = 0xffffffff
    hits[hit, 0], hits[hit, 1], hits[hit, 2] = t[hit], u[hit], v[hit]
    hw[hit, 3] = hw[hit, 4] = 0
    light = A.RtrAreaLightInfo()
    light.color[:] = [float(cc) for cc in LIGHT_COLOR]
    light.intensity, light.numTriangles, light.isTwoSided = float(INTENSITY), 1, 1
    em = api.host_emitter_hits(b.rays, hits, sfs, b.raw, rec[None], np.zeros(1, np.uint32), [light], api.make_mis_params(1, 1, 1))
    assert np.isfinite(em.raw[:, :6]).all()
    assert not em.raw.view(np.uint32)[~hit].any(), "a ray that misses the light has a record"
    bounce_term = em.radiance.astype(np.float64) * b.weight.astype(np.float64)
    return {"NEE": nee, "MIS": pick_term + bounce_term, "bounce": bounce_term}, c512, hit.mean()


def _assert_the_quadratures_mean(est, c512, on_light, what):
    n = len(est["NEE"])
    for name in ("NEE", "MIS"):
        mean, se = est[name].mean(axis=0), est[name].std(axis=0, ddof=1) / np.sqrt(n)
        with np.errstate(all="ignore"):          # a metal seen from behind sees nothing of a low light: every term is 0, and so is the quadrature
            z = np.where(se > 0.0, (mean - c512) / se, np.where(mean == c512, 0.0, np.inf))
        print(f"{what} {name}: mean {mean}, quadrature {c512}, z {z}, variance {est[name].var(axis=0, ddof=1)}; bounce rays on the light: {on_light:.3f}")
        assert (np.abs(z) <= 5.0).all(), f"{name}: {mean} is {z} standard errors from the quadrature {c512}"


@pytest.mark.parametrize("tri", list(TRIANGLES))
@pytest.mark.parametrize("roughness,metallic", MATERIALS)
def test_nee_and_mis_have_the_quadratures_mean(view, tri, roughness, metallic):
    """One surface point at the origin, N = +z, one two-sided light triangle, 200 000 consecutive seeds, no occlusion: (a) the picks with
    the default weight and (b) picks * wPick + the bounce's emitter hit * the bounce weight each lie within 5 of their own standard
    errors of (c), the float64 quadrature on the 512-per-edge grid, per channel.  The variances are printed, not asserted."""
    est, c512, on_light = _nee_and_mis(view, tri, roughness, metallic, SEEDS, 0.01)
    _assert_the_quadratures_mean(est, c512, on_light, f"{tri} roughness {roughness} metallic {metallic}")


SEEDS_BEHIND = 600000          # at 200 000 the excess of a wrong density from behind sits near 5 standard errors
# the six materials, and the one in which both lobes carry weight (pSpec = 0.51): where a specular sample the evaluated density does not
# know of costs the most
MATERIALS_BEHIND = MATERIALS + [(1.0, 0.5)]


@pytest.mark.parametrize("nov", [0.02, -0.5, -0.9])
@pytest.mark.parametrize("tri", list(TRIANGLES))
@pytest.mark.parametrize("roughness,metallic", MATERIALS_BEHIND)
def test_nee_and_mis_have_the_quadratures_mean_from_a_grazing_view_and_from_behind(tri, roughness, metallic, nov):
    """The same statement for a view that grazes the surface and for two from behind the shading normal (dot(N, V) < 0, a face seen
    from behind its vertex normals), 600 000 seeds.  MIS divides by the bounce's density at the picks' directions and weighs the
    bounce by its own: a density that is not the sampler's reads high (1.3 % and 9 standard errors at roughness 1, metallic 0.5,
    NoV -0.9 on the grazing triangle before rtr_bounce_sample dropped half vectors on the far side of the view).  normalOffset is 0
    here, so that the bounce ray starts where the picks are evaluated and the offset's own excess (divergence D8 of DESIGN.md section
    4) cannot colour the result."""
    est, c512, on_light = _nee_and_mis(_view_ray(nov), tri, roughness, metallic, SEEDS_BEHIND, 0.0, finest_grid=2048)
    _assert_the_quadratures_mean(est, c512, on_light, f"NoV {nov} {tri} roughness {roughness} metallic {metallic}")


def _solid_angle(rec, x, n=512):
    """the solid angle of the triangle of rec seen from x: |cos| / d^2 on M.quadrature's barycentric midpoint grid, float64"""
    p0, p1, p2 = (rec[i:i + 3].astype(np.float64) for i in (0, 4, 8))
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    up, down = (i + j) < n, (i + j) < n - 1
    u = np.concatenate([(i[up] + 1.0 / 3.0), (i[down] + 2.0 / 3.0)]) / n
    v = np.concatenate([(j[up] + 1.0 / 3.0), (j[down] + 2.0 / 3.0)]) / n
    w = p0 + (p1 - p0) * u[:, None] + (p2 - p0) * v[:, None] - x
    nrm = np.cross(p1 - p0, p2 - p0)
    area = 0.5 * np.linalg.norm(nrm)
    d2 = np.sum(w * w, axis=1)
    return area * np.mean(np.abs(w @ (nrm / (2.0 * area))) / (d2 * np.sqrt(d2)))


def test_the_normal_offset_raises_mis_by_the_triangles_growth_in_solid_angle(view):
    """Divergence D8 of DESIGN.md section 4, stated instead of ignored.  The bounce ray starts normalOffset above the point its weight
    and the picks are evaluated at; a light overhead subtends a larger solid angle from there, the bounce meets it that much more often,
    and MIS reads high by, to first order, (the mean of the bounce term) * (Omega(x + normalOffset N) / Omega(x) - 1).  The overhead
    triangle, roughness 1, metallic 0, the default offset 0.01, 3 000 000 seeds in chunks: the excess of the MIS mean over the quadrature
    lies within 5 of its standard errors of that prediction, per channel.  Both are printed.  With the offset at 0 the same estimate is
    held to the quadrature itself (test_nee_and_mis_have_the_quadratures_mean_from_a_grazing_view_and_from_behind)."""
    rec = M.tri_record(*TRIANGLES["overhead"])
    x, N = np.zeros(3), np.array([0.0, 0.0, 1.0])
    o0, o1, oc = _solid_angle(rec, x), _solid_angle(rec, x + 0.01 * N), _solid_angle(rec, x, 256)
    assert abs(o0 - oc) <= 1e-5 * o0, "the solid angle has not converged"          # a thousandth of the growth it is differenced for
    growth = o1 / o0 - 1.0
    n, chunk = 3000000, 500000
    total, total2, bounce = np.zeros(3), np.zeros(3), np.zeros(3)
    for start in range(0, n, chunk):
        est, c512, _ = _nee_and_mis(view, "overhead", 1.0, 0.0, chunk, 0.01, first_seed=start)
        total += est["MIS"].sum(axis=0)
        total2 += (est["MIS"] ** 2).sum(axis=0)
        bounce += est["bounce"].sum(axis=0)
    mean, bounce = total / n, bounce / n
    se = np.sqrt((total2 / n - mean * mean) * (n / (n - 1.0)) / n)
    excess, predicted = mean - c512, bounce * growth
    print(f"solid angle {o0:.6f} -> {o1:.6f} (+{100.0 * growth:.3f} %), bounce term {bounce}; MIS excess {excess} ({100.0 * excess / c512} %), "
          f"predicted {predicted} ({100.0 * predicted / c512} %), standard error {se}, z {(excess - predicted) / se}")
    assert (np.abs(excess - predicted) <= 5.0 * se).all()
