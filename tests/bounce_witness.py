"""A float64 numpy restatement of include/rtr_bounce.h (rtr_bounce_sample): the witness the host function is held to, the synthetic
surfaces both run on, and the quadrature of the renderer's BRDF the estimator's mean is held to.  No test in here; test_bounce_host.py and
test_gpu_bounce.py import it.

The random numbers are the contract's own (the PCG hash is integer arithmetic and the scaling to [0, 1] is exact in float32), everything
after them is float64 with numpy's sin / cos / power, from the float32 inputs."""
import numpy as np

PI_F = float(np.float32(3.14159265359))          # RTR_PI_F as the float the kernels hold
SURFACE_MISS, SURFACE_OBJECT, SURFACE_LIGHT, SURFACE_INVALID = 0, 1, 2, 3
DIFFUSE, SPECULAR = 1, 2


def pcg_hash(seed):
    seed = np.asarray(seed).astype(np.uint64) & 0xffffffff
    state = (seed * 747796405 + 2891336453) & 0xffffffff
    word = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & 0xffffffff
    return ((word >> 22) ^ word).astype(np.uint32)


def rtr_random(seed):
    """float32: float(hash) * 2^-32, one round-to-nearest-even convert and an exact scaling"""
    return pcg_hash(seed).astype(np.float32) * np.float32(2.3283064365386963e-10)


# rtr_random(s0) == 1.0 needs hash >= 0xFFFFFF80: 128 of 2^32 seeds.  Found with a chunked search over seeds upwards from 0
# (np.flatnonzero(pcg_hash(np.arange(a, a + 2**24)) >= 0xFFFFFF80)); test_bounce_host.py asserts that it is one.
SEED_U1_IS_ONE = 60418823                         # hash 0xffffff90; the first such seed from 0 upwards


def pixel_seeds(n, width, spp):
    k = np.arange(n, dtype=np.uint64) // spp
    return (((k % width) * 733 + (k // width) * 1933) & 0xffffffff).astype(np.uint32)


def _dot(a, b):
    return np.sum(a * b, axis=-1)


def _normalize(a):
    with np.errstate(all="ignore"):
        return a / np.sqrt(_dot(a, a))[..., None]


def _basis(n):
    sign = np.where(n[:, 2] >= 0.0, 1.0, -1.0)
    a = -1.0 / (sign + n[:, 2])
    c = n[:, 0] * n[:, 1] * a
    t = np.stack([1.0 + sign * n[:, 0] * n[:, 0] * a, sign * c, -sign * n[:, 0]], axis=1)
    b = np.stack([c, sign + n[:, 1] * n[:, 1] * a, -n[:, 1]], axis=1)
    return t, b


def brdf(N, V, L, roughness, F0, om, color):
    """currSpecular + currDiffuse as the renderer forms them (kernels/rtr_device.h: GGX_Distribution, GGX_PartialGeometryTerm,
    Fresnel_Schlick, area_sample_contrib), in float64.  Arrays (M, 3) / (M,) or anything that broadcasts."""
    with np.errstate(all="ignore"):
        H = _normalize(V + L)
        cosT = np.clip(_dot(V, H), 0.0, 1.0)
        NoH = _dot(N, H)
        a2 = roughness * roughness
        den = np.maximum(NoH * NoH * a2 + (1.0 - NoH * NoH), 0.001)
        D = np.where(NoH > 0.0, 1.0, 0.0) * a2 / (PI_F * den * den)

        def g1(v):
            voh = np.clip(_dot(v, H), 0.001, 1.0)
            chi = np.where(voh / np.clip(_dot(v, N), 0.001, 1.0) > 0.0, 1.0, 0.0)
            voh2 = voh * voh
            return chi * 2.0 / (1.0 + np.sqrt(1.0 + a2 * (1.0 - voh2) / voh2))

        G = g1(V) * g1(L)
        x = 1.0 - cosT
        p = np.where(x >= 1.17549435e-38, x, 0.0) ** 5.0          # rtr_pow: 0 below FLT_MIN
        F = F0 + (1.0 - F0) * np.asarray(p)[..., None]
        NdotV = np.maximum(_dot(N, V), 0.1)
        NdotL = np.maximum(_dot(N, L), 0.1)
        spec = np.asarray(D * G / (4.0 * NdotV * NdotL))[..., None] * F
        diff = np.asarray(om)[..., None] * color / PI_F
        return spec + diff


def sample(rays, surfaces, seed_base, frame=0, depth=0, lobes=DIFFUSE | SPECULAR, normal_offset=0.01, tmin=0.001, tmax=10000.0):
    """rtr_bounce_sample in float64 on (N, 8) float32 rays and (N, 20) float32 RtrSurface records -> dict of float64 arrays:
    rays (N, 8), weight (N, 3), pdf, p_spec, lobe (0 = dead), and the two margins a discrete decision hangs on: lobe_margin =
    |uLobe - pSpec| where both lobes are on (inf otherwise), nol = dot(N, L) of the sampled direction (nan where none was sampled)."""
    rays = np.asarray(rays, np.float32)
    sf = np.asarray(surfaces).view(np.float32)
    n = len(rays)
    kind = sf.view(np.uint32)[:, 3]
    O = rays[:, 0:3].astype(np.float64)
    P, N, color = (sf[:, a:a + 3].astype(np.float64) for a in (0, 4, 12))
    metallic, roughness = sf[:, 11].astype(np.float64), sf[:, 15].astype(np.float64)
    finite = np.isfinite(O).all(1) & np.isfinite(P).all(1) & np.isfinite(N).all(1) & np.isfinite(color).all(1) & np.isfinite(metallic) & np.isfinite(roughness)
    live = (kind == SURFACE_OBJECT) & finite
    with np.errstate(all="ignore"):
        V = _normalize(O - P)
        live &= np.isfinite(V).all(1)                      # a ray that starts at its hit has no view vector
        om = 1.0 - metallic
        mDiffuse = color * om[:, None]
        F0 = color * metallic[:, None] + 0.04 * om[:, None]
        # roughness * roughness == 0 is decided in float32, as the contract does (a float32 product can underflow where float64's does not)
        a2_is_zero = (sf[:, 15] * sf[:, 15]) == 0.0
        a2 = roughness * roughness
        s0 = (np.asarray(seed_base).astype(np.uint64) + (frame & 0xffffffff) + 7919 * ((depth + 1) & 0xffffffff)) & 0xffffffff
        u1 = rtr_random(s0).astype(np.float64)
        u2 = rtr_random(s0 + 100).astype(np.float64)
        uL = rtr_random(s0 + 200).astype(np.float64)
        s, d = F0.max(1), mDiffuse.max(1)
        spec_on = ~a2_is_zero & bool(lobes & SPECULAR)
        diff_on = ((sf[:, 12:15] * (np.float32(1.0) - sf[:, 11])[:, None]).max(1) != 0.0) & bool(lobes & DIFFUSE)
        live &= spec_on | diff_on
        p_spec = np.where(spec_on & diff_on, s / (s + d), np.where(spec_on, 1.0, 0.0))
        take_spec = spec_on & (~diff_on | (uL < p_spec))
        lobe_margin = np.where(spec_on & diff_on, np.abs(uL - p_spec), np.inf)
        T, B = _basis(N)
        sn, cs = np.sin(2.0 * np.pi * u2), np.cos(2.0 * np.pi * u2)
        # specular
        den = a2 * u1 + (1.0 - u1)
        cosT, sinT = np.sqrt((1.0 - u1) / den), np.sqrt(a2 * u1 / den)
        H = _normalize((sinT * cs)[:, None] * T + (sinT * sn)[:, None] * B + cosT[:, None] * N)
        Ls = _normalize(2.0 * _dot(V, H)[:, None] * H - V)
        # diffuse
        r = np.sqrt(u1)
        Ld = _normalize((r * cs)[:, None] * T + (r * sn)[:, None] * B + np.sqrt(np.maximum(1.0 - u1, 0.0))[:, None] * N)
        L = np.where(take_spec[:, None], Ls, Ld)
        NoL = _dot(N, L)
        live &= NoL > 0.0
        Hm = _normalize(V + L)
        NoH, VoH = _dot(N, Hm), _dot(V, Hm)
        pdfD = NoL / PI_F
        # the density of the angle between N and H as such: a float32 normal is a unit vector to 6e-8 only, and 1 - NoH^2 of such a
        # normal is off by 1e-7, a tenth of alpha^2 at roughness 0.001
        Nn = _normalize(N)
        NxH = np.cross(Nn, Hm)
        dn = _dot(Nn, Hm) ** 2 * a2 + _dot(NxH, NxH)
        pdfS =np.where(spec_on & (NoH > 0.0) & (VoH > 0.0), a2 / (PI_F * dn * dn) * NoH / (4.0 * VoH), 0.0)
        pdf = p_spec * pdfS + (1.0 - p_spec) * pdfD
        live &= (pdf > 0.0) & np.isfinite(pdf)
        w = brdf(N, V, L, roughness, F0, om, color) * NoL[:, None] / pdf[:, None]
        live &= np.isfinite(w).all(1) & (w >= 0.0).all(1)
        origin = P + normal_offset * N
    out = np.zeros((n, 8))
    out[:, 0:3], out[:, 3], out[:, 4:7], out[:, 7] = origin, tmin, L, tmax
    out[~live] = 0.0
    z = lambda x: np.where(live if np.ndim(x) == 1 else live[:, None], x, 0.0)      # noqa: E731
    return {"rays": out, "weight": z(w), "pdf": z(pdf), "p_spec": z(p_spec), "lobe": z(np.where(take_spec, SPECULAR, DIFFUSE)).astype(np.int64),
            "lobe_margin": lobe_margin, "nol": NoL}


def make_surfaces(n, seed=1234):
    """About n synthetic hits: (rays (N, 8) float32, surfaces (N, 20) float32, seeds (N,) uint32).  Random unit normals, view directions in
    the normal's upper hemisphere at distances 0.5 ... 20, roughness of {0, 1e-3, 0.05, 0.3, 1}, metallic of {0, 0.5, 1}, colours random
    or black or white, random seeds.  Every record is an object with finite floats."""
    rng = np.random.default_rng(seed)
    N = rng.normal(size=(n, 3))
    N /= np.linalg.norm(N, axis=1)[:, None]
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    nv = np.sum(v * N, axis=1)
    v = np.where((nv < 0)[:, None], v - 2.0 * nv[:, None] * N, v)          # mirrored into the upper hemisphere
    P = rng.uniform(-10.0, 10.0, size=(n, 3))
    O = P + v * rng.uniform(0.5, 20.0, size=(n, 1))
    color = rng.uniform(0.0, 1.0, size=(n, 3))
    pick = rng.integers(0, 8, size=n)
    color[pick == 0] = 0.0
    color[pick == 1] = 1.0
    sf = np.zeros((n, 20), np.float32)
    sf[:, 0:3], sf[:, 4:7], sf[:, 8:11], sf[:, 12:15] = P, N, N, color
    sf.view(np.uint32)[:, 3] = SURFACE_OBJECT
    sf.view(np.uint32)[:, 7] = rng.integers(0, 100, size=n)
    sf[:, 11] = rng.choice(np.array([0.0, 0.5, 1.0], np.float32), size=n)
    sf[:, 15] = rng.choice(np.array([0.0, 1e-3, 0.05, 0.3, 1.0], np.float32), size=n)
    sf[:, 16:18] = rng.uniform(0, 1, size=(n, 2))
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 7] = O, 0.001, 10000.0
    rays[:, 4:7] = -v
    return rays, sf, rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)


def dead_cases():
    """(name, ray (8,), surface (20,), lobes) of records that have no continuation"""
    rays, sf, _ = make_surfaces(1, seed=7)
    ray, base = rays[0], sf[0]
    base[11], base[15], base[12:15] = 0.5, 0.3, (0.8, 0.6, 0.4)
    out = []

    def case(name, lobes=DIFFUSE | SPECULAR, ray_edit=None, **edits):
        s, r = base.copy(), ray.copy()
        for k, v in edits.items():
            if k == "kind":
                s.view(np.uint32)[3] = v
            else:
                a, b = {"position": (0, 3), "normal": (4, 7), "color": (12, 15), "metallic": (11, 12), "roughness": (15, 16)}[k]
                s[a:b] = v
        if ray_edit is not None:
            r[0:3] = ray_edit
        out.append((name, r, s, lobes))

    for name, kind in (("miss", SURFACE_MISS), ("light", SURFACE_LIGHT), ("invalid", SURFACE_INVALID)):
        case(name, kind=kind)
    for bad_name, bad in (("nan", np.nan), ("inf", np.inf), ("-inf", -np.inf)):
        for field in ("normal", "position", "color"):
            case(f"{bad_name} in {field}", **{field: (base[{"normal": 4, "position": 0, "color": 12}[field]], bad, 0.25)})
        case(f"{bad_name} roughness", roughness=bad)
        case(f"{bad_name} in the ray origin", ray_edit=(1.0, bad, 2.0))
    case("black metal without roughness: both lobes off", metallic=1.0, color=(0.0, 0.0, 0.0), roughness=0.0)
    case("roughness 0, specular only", lobes=SPECULAR, roughness=0.0)
    case("metal, diffuse only", lobes=DIFFUSE, metallic=1.0)
    case("a ray that starts at its hit", ray_edit=base[0:3].copy())
    return out


def albedo_quadrature(roughness, metallic, color, nov, n_theta=1200, n_phi=2400):
    """integral of BRDF * cos over the hemisphere for N = +z and V at dot(N, V) = nov: midpoint rule in (cos theta, phi) -> (3,)"""
    N = np.array([0.0, 0.0, 1.0])
    V = np.array([np.sqrt(1.0 - nov * nov), 0.0, nov])
    color = np.asarray(color, np.float64)
    om = 1.0 - metallic
    F0 = color * metallic + 0.04 * om
    phi = (np.arange(n_phi) + 0.5) * (2.0 * np.pi / n_phi)
    total = np.zeros(3)
    for block in np.array_split(np.arange(n_theta), 24):
        mu = (block + 0.5) / n_theta                                             # cos theta, uniform: d omega = d mu d phi
        st = np.sqrt(1.0 - mu * mu)
        L = np.stack([st[:, None] * np.cos(phi)[None, :], st[:, None] * np.sin(phi)[None, :], np.broadcast_to(mu[:, None], (len(mu), n_phi))], axis=-1)
        f = brdf(N, V, L.reshape(-1, 3), roughness, F0, om, color) * L.reshape(-1, 3)[:, 2:3]
        total += f.sum(0)
    return total * (1.0 / n_theta) * (2.0 * np.pi / n_phi)
