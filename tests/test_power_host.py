"""The host forms of include/rtr_power.h without a device: the light-power table against the exact-rational integers of
tests/power_witness.py, the draws against the table's shares, the balance heuristic with the table's probabilities, and the estimators —
power picks alone and power picks with the bounce under MIS — against a float64 quadrature over two lights of very different power."""
import numpy as np
import pytest

import bounce_witness as BW
import mis_witness as M
import power_witness as PW
import ray_flags_witness as RW
from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api

ULP1 = float(np.spacing(np.float32(1.0)))


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _records(areas):
    """light-triangle records of the given areas: right triangles in the plane z = 2, legs sqrt(2 area) (the table reads the area word
    alone; the areas are written as they are, so that a record may carry a zero, a negative or a NaN)"""
    rec = np.zeros((len(areas), 16), np.float32)
    for t, a in enumerate(areas):
        e = np.sqrt(2.0 * a) if np.isfinite(a) and a > 0 else 1.0
        rec[t, 0:3], rec[t, 4:7], rec[t, 8:11] = (t, 0, 2), (t + e, 0, 2), (t, e, 2)
        rec[t, 3], rec[t, 7], rec[t, 14] = a, 1.0 / (0.7 * a) if a else 0.0, -1.0
    return rec


WHITE = (1.0, 1.0, 1.0)
# name -> ([(colour, intensity, triangles, two_sided)], areas)
TABLES = {
    "equal lights": ([(WHITE, 5.0, 2, 1), (WHITE, 5.0, 1, 0), (WHITE, 5.0, 2, 1)], [2.0] * 5),
    "1 : 1000": ([(WHITE, 0.05, 1, 1), (WHITE, 50.0, 1, 1)], [1.0, 1.0]),
    "a zero-intensity light": ([(WHITE, 3.0, 2, 1), (WHITE, 0.0, 2, 1), ((0.2, 0.9, 0.4), 7.0, 1, 1)], [0.7, 1.9, 1.0, 1.0, 0.35]),
    "all zero": ([(WHITE, 0.0, 2, 1), ((0.0, 0.0, 0.0), 9.0, 1, 1)], [1.0, 2.0, 3.0]),
    "negative and NaN intensities": ([(WHITE, -4.0, 1, 1), (WHITE, np.nan, 2, 1), (WHITE, 2.5, 2, 1), (WHITE, np.inf, 1, 1)], [1.0, 1.0, 2.0, 0.3, 1.7, 1.0]),
    "a triangle without area": ([((0.9, 0.3, 0.1), 11.0, 3, 1), (WHITE, 1.0, 1, 1)], [0.5, 0.0, 1.5, 4.0]),
    "a negative colour": ([((-1.0, -0.5, -2.0), 5.0, 1, 1), ((-1.0, 0.25, -2.0), 5.0, 1, 1)], [1.0, 1.0]),
    "a weight that rounds down to 1": ([(WHITE, 1.0e-7, 1, 1), (WHITE, 1.0, 1, 1)], [1.0, 1.0]),
    "odd quotients": ([((0.3, 0.7, 0.1), 13.7, 7, 1), ((0.9, 0.2, 0.2), 0.37, 6, 0)], [0.1 * (k + 1) ** 1.5 for k in range(13)]),
    "an empty light between two": ([(WHITE, 2.0, 2, 1), (WHITE, 9.0, 0, 1), (WHITE, 1.0, 1, 1)], [1.0, 3.0, 2.0]),
}


def _host_table(name):
    specs, areas = TABLES[name]
    lights, first = PW.lights_of(specs)
    rec = _records(np.array(areas, np.float32))
    w, cdf = api.host_light_power(rec, first, lights)
    return lights, first, rec, w, cdf


# ---- 1. the table ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TABLES))
def test_the_table_is_the_witnesses_integers(name):
    lights, first, rec, w, cdf = _host_table(name)
    ww, wc = PW.table(rec[:, 3], first, lights)
    assert [int(x) for x in w] == ww, f"{name}: weights {w} but the witness has {ww}"
    assert [int(x) for x in cdf] == wc
    assert w.dtype == np.uint32 and cdf.dtype == np.uint64
    if any(ww):
        assert max(ww) == A.POWER_SCALE, "the strongest triangle has the full weight"


def test_the_tables_edge_cases_by_hand():
    _, _, _, w, cdf = _host_table("equal lights")
    assert (w == A.POWER_SCALE).all() and (cdf == A.POWER_SCALE * np.arange(1, 6, dtype=np.uint64)).all()
    _, _, _, w, _ = _host_table("1 : 1000")
    assert list(w) == [int(np.float32(np.float32(0.05) / np.float32(50.0)) * np.float32(A.POWER_SCALE)), A.POWER_SCALE]
    _, _, _, w, cdf = _host_table("a zero-intensity light")
    assert w[2] == 0 and w[3] == 0 and cdf[3] == cdf[1] and w[0] and w[1] and w[4]
    _, _, _, w, cdf = _host_table("all zero")
    assert not w.any() and not cdf.any()
    _, _, _, w, _ = _host_table("negative and NaN intensities")
    assert list(w != 0) == [False, False, False, True, True, False], "only the light of intensity 2.5 emits"
    _, _, _, w, _ = _host_table("a triangle without area")
    assert w[1] == 0 and w[0] and w[2]
    _, _, _, w, _ = _host_table("a negative colour")
    assert w[0] == 0 and w[1] == A.POWER_SCALE, "max3 of the colour, held to 0"
    _, _, _, w, _ = _host_table("a weight that rounds down to 1")
    assert list(w) == [1, A.POWER_SCALE], "no triangle that emits is left out"


def test_the_table_refuses_before_it_writes():
    lib = A.hip_lib()
    lights, first = PW.lights_of([(WHITE, 1.0, 2, 1)])
    li = (A.RtrAreaLightInfo * 1)(*lights)
    rec = _records(np.array([1.0, 2.0], np.float32))
    w, cdf = np.full(2, 7, np.uint32), np.full(2, 7, np.uint64)
    p = lambda x: x.ctypes.data_as(A.VP)
    for args, needle in (((None, p(first), li, 1, p(w), p(cdf)), "lightTris is null"), ((p(rec), None, li, 1, p(w), p(cdf)), "lightTriFirst is null"),
                         ((p(rec), p(first), None, 1, p(w), p(cdf)), "lights is null"), ((p(rec), p(first), li, 1, None, p(cdf)), "outWeights is null"),
                         ((p(rec), p(first), li, 1, p(w), None), "outCdf is null")):
        assert lib.rtr_host_light_power(*args) == -1
        msg = lib.rtr_last_error().decode()
        assert msg.startswith("rtr_host_light_power: ") and needle in msg, msg
    assert (w == 7).all() and (cdf == 7).all()
    assert lib.rtr_host_light_power(None, None, None, 0, None, None) == 0


# ---- 2. the draws ----------------------------------------------------------------------------------------------------------------------
DRAWS = 200000


@pytest.mark.parametrize("name", ["1 : 1000", "a zero-intensity light", "odd quotients", "equal lights", "an empty light between two"])
@pytest.mark.parametrize("area_lights", ["all", "first"])
def test_the_draws_follow_the_table(name, area_lights):
    """among 200 000 seeds the share of picks per triangle is weight / total within 5 standard errors, the sample within the triangle
    is uniform over ns, and the weight is total / (P weight) of the triangle drawn"""
    lights, first, rec, w, cdf = _host_table(name)
    n_lights = len(lights) if area_lights == "all" else 1
    tris = sum(int(l.numTriangles) for l in lights[:n_lights])
    ns, P = 3, 2
    params, pick = api.make_light_params(n_lights, shadow_rays=ns, frame=11), api.make_pick_params(P, depth=2)
    seeds = np.arange(1000, 1000 + DRAWS, dtype=np.uint32)
    slots, weights = api.host_pick_slots_power(cdf, tris, seeds, seeds.size, params, pick)
    total = int(cdf[tris - 1])
    assert total > 0 and (slots < tris * ns).all()
    t, s = slots // ns, slots % ns
    n = slots.size
    share = w[:tris].astype(np.float64) / total
    counts = np.bincount(t.reshape(-1), minlength=tris)
    se = np.sqrt(share * (1.0 - share) / n)
    z = np.where(se > 0, (counts / n - share) / np.where(se > 0, se, 1.0), 0.0)
    print(f"{name} ({tris} triangles): shares {counts / n} against {share}, z {z}")
    assert (counts[share == 0] == 0).all(), "a triangle of weight 0 was drawn"
    assert (np.abs(z) <= 5.0).all()
    cs = np.bincount(s.reshape(-1), minlength=ns)
    zs = (cs / n - 1.0 / ns) / np.sqrt((1.0 / ns) * (1.0 - 1.0 / ns) / n)
    assert (np.abs(zs) <= 5.0).all(), f"the sample within the triangle is not uniform: {cs}"
    expect = (np.float32(total) / (np.float32(P) * w[t].astype(np.float32))).astype(np.float32)
    assert (_bits(weights) == _bits(expect)).all()
    # the mean of the weight over the draws of a triangle times its share: each triangle is counted once per pick
    assert abs(float(np.mean(weights.astype(np.float64))) * P - np.count_nonzero(share)) <= 5.0 * float(np.std(weights.astype(np.float64)) * P / np.sqrt(n))


@pytest.mark.parametrize("name", ["odd quotients", "1 : 1000", "a zero-intensity light"])
@pytest.mark.parametrize("explicit", [True, False])
def test_the_draws_are_the_witnesses_on_integers(name, explicit):
    lights, first, rec, w, cdf = _host_table(name)
    tris = rec.shape[0]
    ns, P, n, frame, depth, width, spp = 4, 3, 300, 5, 1, 13, 2
    params, pick = api.make_light_params(len(lights), shadow_rays=ns, frame=frame, width=width, spp=spp), api.make_pick_params(P, depth=depth)
    seeds = (np.arange(n, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32) if explicit else None
    slots, _ = api.host_pick_slots_power(cdf, tris, seeds, n, params, pick)
    ints = [int(c) for c in cdf]
    for k in range(n):
        base = int(seeds[k]) if explicit else PW.pixel_base(k, width, spp)
        for p in range(P):
            assert int(slots[k, p]) == PW.pick(ints, tris, ns, (base + frame) & 0xffffffff, depth, p), (k, p)


def test_a_number_of_exactly_one_stays_in_range_and_an_empty_table_gives_no_slot():
    lights, first, rec, w, cdf = _host_table("odd quotients")
    tris, ns = rec.shape[0], 5
    params, pick = api.make_light_params(len(lights), shadow_rays=ns), api.make_pick_params(1)
    assert BW.rtr_random(np.array([BW.SEED_U1_IS_ONE]))[0] == 1.0
    for offset in (0, 50):                # the triangle's number is 1.0, then the sample's
        base = np.array([(BW.SEED_U1_IS_ONE - 7919 - 400 - offset) & 0xffffffff], np.uint32)
        slots, weights = api.host_pick_slots_power(cdf, tris, base, 1, params, pick)
        assert slots[0, 0] < tris * ns and np.isfinite(weights).all() and weights[0, 0] > 0
        if offset == 0:
            assert slots[0, 0] // ns == tris - 1, "u = 1.0 is the last triangle"
        else:
            assert slots[0, 0] % ns == ns - 1, "u = 1.0 is the last sample"
    # total == 0: all lights dark, or numAreaLights leaves only dark ones, or no lights at all
    _, _, _, _, dark = _host_table("all zero")
    for c, tr in ((dark, 3), (dark, 2), (cdf, 0), (None, 0)):
        slots, weights = api.host_pick_slots_power(c if c is not None else np.zeros(0, np.uint64), tr, None, 40, api.make_light_params(1, width=8), api.make_pick_params(3))
        assert (slots == A.PICK_NONE).all() and not _bits(weights).any()


# ---- 3. the densities and the heuristic ---------------------------------------------------------------------------------------------------
def test_equal_powers_give_one_over_the_triangle_count_exactly():
    for tris in (1, 3, 5, 12, 1000):
        lights, first = PW.lights_of([(WHITE, 5.0, tris, 1)])
        rec = _records(np.full(tris, 0.75, np.float32))
        _, cdf = api.host_light_power(rec, first, lights)
        n = 64
        rng = np.random.default_rng(tris)
        pb, dist, cosl = rng.uniform(0.05, 3, n).astype(np.float32), rng.uniform(0.5, 9, n).astype(np.float32), rng.uniform(-1, 1, n).astype(np.float32)
        area = np.full(n, 0.75, np.float32)
        lt = rng.integers(0, tris, n).astype(np.uint32)
        s, wb, wt = api.host_mis_weights_power(pb, dist, cosl, area, lt, cdf, tris, 2)
        ptri = np.float32(1.0) / np.float32(tris)
        q = ((ptri * (dist * dist)) / area) / np.abs(cosl)
        assert (_bits(s[:, 0]) == _bits(q)).all(), "lightPdf is not the one of pTri = 1 / Ttot"
        assert (_bits(wt) == _bits((np.float32(tris) / np.float32(2)) * s[:, 2])).all(), "wPow is not Ttot / P"


def test_the_heuristic_against_float64_and_its_edges():
    lights, first, rec, w, cdf = _host_table("odd quotients")
    tris = rec.shape[0]
    rng = np.random.default_rng(9)
    n = 20000
    pb, dist = rng.uniform(0.0, 4.0, n).astype(np.float32), rng.uniform(0.3, 30.0, n).astype(np.float32)
    cosl, lt = rng.uniform(-1.0, 1.0, n).astype(np.float32), rng.integers(0, tris + 3, n).astype(np.uint32)
    pb[::17] = 0.0
    area = rec[np.minimum(lt, tris - 1), 3]
    for area_tris, picks in ((tris, 1), (tris, 30), (7, 2), (tris, 0), (0, 1)):
        s, wb, wt = api.host_mis_weights_power(pb, dist, cosl, area, lt, cdf, area_tris, picks)
        total = int(cdf[area_tris - 1]) if area_tris else 0
        ptri = np.where(lt < area_tris, w[np.minimum(lt, tris - 1)] / max(total, 1), 0.0)
        q64, wp64, wb64 = PW.mis_weights(pb, dist, cosl, area, ptri, picks)
        assert np.isfinite(s[:, :6]).all() and np.isfinite(wb).all() and np.isfinite(wt).all()
        assert (s.view(np.uint32)[:, 6] == lt).all() and not s.view(np.uint32)[:, 7].any()
        # 12 roundings: test_mis_host.py's count and one more for pTri's own quotient, which enters a once
        assert np.abs(s[:, 2] - wp64).max() <= 13 * 2.0 ** -24 and np.abs(wb - wb64).max() <= 13 * 2.0 ** -24
        ok = q64 > 0
        assert (np.abs(s[ok, 0] - q64[ok]) <= 6 * 2.0 ** -24 * q64[ok]).all()
        both = (s[:, 2] != 0) & (wb != 0)
        assert both.any() or picks == 0 or area_tris == 0
        assert (np.abs((s[both, 2].astype(np.float64) + wb[both].astype(np.float64)) - 1.0) <= ULP1).all(), "wPick + wBounce is not 1 within one ulp"
        nobody = ptri == 0
        assert not s[nobody, 0].any() and not s[nobody, 2].any() and not wt[nobody].any(), "a triangle nobody picks has a pick weight"
        assert (wb[nobody & (pb > 0) & (cosl != 0)] == 1.0).all(), "a triangle nobody picks is the bounce's alone"
        if picks and area_tris:
            wpow = (np.float32(total) / (np.float32(picks) * w[np.minimum(lt, tris - 1)].astype(np.float32))).astype(np.float32)
            assert (_bits(wt[~nobody]) == _bits(wpow[~nobody] * s[~nobody, 2])).all()
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(4):
            args = [np.float32(0.5)] * 4
            args[k] = np.float32(bad)
            s, wb, wt = api.host_mis_weights_power(*[[a] for a in args], [0], cdf, tris, 2)
            assert s[0, 0] == 0 and s[0, 2] == 0 and wb[0] == 0 and wt[0] == 0, (bad, k)


# ---- 4. the estimators -----------------------------------------------------------------------------------------------------------------
# two lights of very different power: the overhead triangle is dim, the low one to the side 400 times as intense
TRIANGLES = [((-1, -1, 2), (1, -1, 2), (0, 1, 2)), ((1, -1, 0.05), (6, 0, 0.3), (1, 1, 1.5))]
LIGHTS = [((1.0, 0.8, 0.6), 0.125, 1, 1), ((0.7, 0.9, 1.0), 50.0, 1, 1)]
COLOR = np.array([0.8, 0.6, 0.4], np.float32)
VIEW = np.array([-0.35, 0.26, 0.9]) / np.linalg.norm([-0.35, 0.26, 0.9])
SEEDS = 200000


@pytest.fixture(scope="module")
def two_lights():
    rec = np.stack([M.tri_record(*t) for t in TRIANGLES])
    lights, first = PW.lights_of(LIGHTS)
    w, cdf = api.host_light_power(rec, first, lights)
    assert w.max() == A.POWER_SCALE and 0 < w.min() < A.POWER_SCALE // 100, f"the powers are not far apart: {w}"
    return rec, lights, first, w, cdf


@pytest.mark.parametrize("roughness,metallic", [(0.15, 1.0), (1.0, 0.0)], ids=["smooth", "rough"])
@pytest.mark.parametrize("picks", [1, 2])
def test_power_picks_and_power_mis_have_the_quadratures_mean(two_lights, roughness, metallic, picks):
    """One surface point at the origin, N = +z, two two-sided light triangles of very different power, 200 000 consecutive seeds, no
    occlusion: (a) the power picks with wPow and (b) the picks with wPow * wPick plus the bounce's emitter hit (host_emitter_hits_power)
    times the bounce weight each lie within 5 of their own standard errors of (c), the float64 quadrature over both triangles, per
    channel.  The pick side's lightPdf and the emitter side's for the same direction and triangle are compared bit for bit on the way."""
    rec, lights, first, w, cdf = two_lights
    view = np.zeros((1, 8), np.float32)
    view[0, 0:3], view[0, 3], view[0, 7], view[0, 4:7] = VIEW * 5.0, 0.001, 10000.0, -VIEW
    sf = np.zeros((1, 20), np.float32)
    sf[0, 4:7] = sf[0, 8:11] = (0, 0, 1)
    sf.view(np.uint32)[0, 3] = A.SURFACE_OBJECT
    sf[0, 12:15], sf[0, 11], sf[0, 15] = COLOR, metallic, roughness
    x, N = np.zeros(3), np.array([0.0, 0.0, 1.0])
    V = view[0, 0:3].astype(np.float64) / np.linalg.norm(view[0, 0:3].astype(np.float64))
    r32, m32 = float(np.float32(roughness)), float(np.float32(metallic))
    om = 1.0 - m32
    surf = (x, N, V, r32, COLOR.astype(np.float64) * m32 + 0.04 * om, om, COLOR.astype(np.float64))
    # (c): the sum of the two triangles' quadratures, converged
    c_fine = np.zeros(3)
    for t in range(2):
        col, inten = np.array(LIGHTS[t][0], np.float32), float(np.float32(LIGHTS[t][1]))
        c256, c512 = M.quadrature(rec[t], 256, *surf, col, inten), M.quadrature(rec[t], 512, *surf, col, inten)
        assert (np.abs(c512 - c256) <= 1e-4 * np.abs(c512)).all(), f"the quadrature of light {t} has not converged: {c512}, {c256}"
        c_fine += c512
    # (a): P picks per seed, ns = 1, the light sample of the hit (sample 0 of the triangle drawn)
    n = SEEDS
    seeds = np.arange(n, dtype=np.uint32)
    params, pick = api.make_light_params(2, shadow_rays=1), api.make_pick_params(picks)
    slots, wpow = api.host_pick_slots_power(cdf, 2, seeds, n, params, pick)
    rays, sfs = np.repeat(view, n, axis=0), np.repeat(sf, n, axis=0)
    nee, pick_term = np.zeros((n, 3)), np.zeros((n, 3))
    pick_pdf = {}
    for p in range(picks):
        for t in range(2):
            sel = slots[:, p] == t
            col, inten = np.array(LIGHTS[t][0], np.float32), float(np.float32(LIGHTS[t][1]))
            pts = M.light_points(rec[t], seeds[sel])
            c, L, d = M.contribution(pts, *surf, col, inten, float(rec[t, 7]))
            nee[sel] += c * wpow[sel, p].astype(np.float64)[:, None]
            L32, d32 = L.astype(np.float32), d.astype(np.float32)
            cosl = np.sum(rec[t, 12:15].astype(np.float64) * -L, axis=1).astype(np.float32)
            pb = api.host_bounce_pdf(rays[sel], sfs[sel], L32)
            smp, _, wt = api.host_mis_weights_power(pb, d32, cosl, np.full(int(sel.sum()), rec[t, 3]), np.full(int(sel.sum()), t, np.uint32), cdf, 2, picks)
            pick_term[sel] += c * wt.astype(np.float64)[:, None]
            pick_pdf[(p, t)] = (pb, d32, cosl, smp[:, 0])
    # (b)'s bounce: host_bounce_rays' ray met with both triangles here, the nearer hit kept
    b = api.host_bounce_rays(rays, sfs, api.make_bounce_params(normal_offset=0.0), seeds)
    hits = np.zeros((n, 8), np.float32)
    hw = hits.view(np.uint32)
    hits[:, 0] = 10000.0
    hw[:, 3] = hw[:, 4] = 0xffffffff
    for t in range(2):
        hit, tt, u, v = M.moller_trumbore(b.rays[:, 0:3].astype(np.float64), b.rays[:, 4:7].astype(np.float64), rec[t])
        hit &= (b.lobe != 0) & (tt >= 0.001) & (tt < hits[:, 0])
        hits[hit, 0], hits[hit, 1], hits[hit, 2] = tt[hit], u[hit], v[hit]
        hw[hit, 3], hw[hit, 4] = t, 0
    mis = api.make_mis_params(picks, 2, 1)
    em = api.host_emitter_hits_power(b.rays, hits, sfs, b.raw, rec, first, lights, cdf, mis)
    on_light = hw[:, 3] != 0xffffffff
    assert np.isfinite(em.raw[:, :6]).all() and not em.raw.view(np.uint32)[~on_light].any()
    bounce_term = em.radiance.astype(np.float64) * b.weight.astype(np.float64)
    # ONE density on both sides: the emitter side's lightPdf equals the pick side's function of the same numbers, bit for bit
    live = em.kind == A.SURFACE_LIGHT
    assert live.sum() > 100
    nt, dirs = rec[em.light_tri[live], 12:15], np.ascontiguousarray(b.rays[live, 4:7])
    L32 = dirs * (np.float32(1.0) / np.sqrt(RW.dot32(dirs, dirs)))[:, None]          # rtr_normalize, operation for operation
    cos_b = RW.dot32(nt, -L32)
    same, wb_pick, _ = api.host_mis_weights_power(b.pdf[live], em.dist[live], cos_b, rec[em.light_tri[live], 3], em.light_tri[live].astype(np.uint32), cdf, 2, picks)
    assert (_bits(same[:, 0]) == _bits(em.light_pdf[live])).all(), "the emitter side's lightPdf is not the pick side's, bit for bit"
    assert (_bits(wb_pick) == _bits(em.w_bounce[live])).all()
    est = {"NEE": nee, "MIS": pick_term + bounce_term}
    for name in ("NEE", "MIS"):
        mean, se = est[name].mean(axis=0), est[name].std(axis=0, ddof=1) / np.sqrt(n)
        z = (mean - c_fine) / se
        print(f"roughness {roughness} metallic {metallic} P {picks} {name}: mean {mean}, quadrature {c_fine}, z {z}, variance {est[name].var(axis=0, ddof=1)}; "
              f"bounce rays on a light: {on_light.mean():.3f}")
        assert (np.abs(z) <= 5.0).all(), f"{name}: {mean} is {z} standard errors from the quadrature {c_fine}"
