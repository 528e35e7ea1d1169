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
    rays (N, 8), weight (N, 3), pdf, p_spec, lobe (0 = dead), and the three margins a discrete decision hangs on: lobe_margin =
    |uLobe - pSpec| where both lobes are on (inf otherwise), nol = dot(N, L) of the sampled direction (nan where none was sampled),
    voh = dot(V, H) of the half vector the specular lobe drew (inf where the diffuse lobe was taken).

    The rule for a view from behind the shading normal (dot(N, V) < 0), as DESIGN.md section 3 states it: the specular lobe draws H
    around N and reflects V about it; a draw with dot(V, H) <= 0 is DEAD.  For the draws that remain, normalize(V + L) is H itself, so
    the density evaluated from L, D(N.H) N.H / (4 V.H) where N.H > 0, is the density L was drawn with; the directions the dropped draws
    would have reached are left to the cosine lobe."""
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
        VoHs = _dot(V, H)
        voh = np.where(take_spec, VoHs, np.inf)
        live &= ~take_spec | (VoHs > 0.0)                   # a half vector on the far side of the view: no specular sample
        Ls = _normalize(2.0 * VoHs[:, None] * H - V)
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
        pdfS = np.where(spec_on & (NoH > 0.0) & (VoH > 0.0), a2 / (PI_F * dn * dn) * NoH / (4.0 * VoH), 0.0)
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
            "lobe_margin": lobe_margin, "nol": NoL, "voh": voh}


GRAZING_BAND = 1e-3          # |dot(N, V)| of the grazing band of make_surfaces(views="sphere")


def make_surfaces(n, seed=1234, views="upper"):
    """About n synthetic hits: (rays (N, 8) float32, surfaces (N, 20) float32, seeds (N,) uint32).  Random unit normals, view directions
    at distances 0.5 ... 20, roughness of {0, 1e-3, 0.05, 0.3, 1}, metallic of {0, 0.5, 1}, colours random or black or white, random
    seeds.  Every record is an object with finite floats.

    views="upper": every view vector mirrored into the normal's upper hemisphere.
    views="sphere": the view vectors as drawn, half of them behind the shading normal, and two bands of grazing views from a random
    stream of their own: 6 % of the records with dot(N, V) uniform in [-1e-3, 1e-3], and 6 % with dot(N, V) exactly 0 in float32 (the
    normal is a signed coordinate axis, and the ray's origin and the hit share that coordinate bit for bit)."""
    if views not in ("upper", "sphere"):
        raise ValueError(f"views {views!r}: 'upper' or 'sphere'")
    rng = np.random.default_rng(seed)
    N = rng.normal(size=(n, 3))
    N /= np.linalg.norm(N, axis=1)[:, None]
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    nv = np.sum(v * N, axis=1)
    if views == "upper":
        v = np.where((nv < 0)[:, None], v - 2.0 * nv[:, None] * N, v)      # mirrored into the upper hemisphere
    else:
        rb = np.random.default_rng([seed, 1])
        band = rb.uniform(size=n)
        near, zero = band < 0.06, (band >= 0.06) & (band < 0.12)
        axis, sign = rb.integers(0, 3, size=n), rb.choice([-1.0, 1.0], size=n)
        N[zero] = 0.0
        N[zero, axis[zero]] = sign[zero]
        graze = near | zero
        t = v - np.sum(v * N, axis=1)[:, None] * N                         # the tangential part of the drawn view, exactly 0 along an axis normal
        t[zero, axis[zero]] = 0.0
        t /= np.linalg.norm(t, axis=1)[:, None]
        eps = np.where(near, rb.uniform(-GRAZING_BAND, GRAZING_BAND, size=n), 0.0)
        v = np.where(graze[:, None], t * np.sqrt(1.0 - eps * eps)[:, None] + eps[:, None] * N, v)
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
    """integral of BRDF * cos over the hemisphere of N = +z for V at dot(N, V) = nov: midpoint rule in (cos theta, phi) -> (3,).  nov may
    be 0 or negative, a view from behind the shading normal: the integral is still over the directions with dot(N, L) > 0, of the BRDF
    as the renderer evaluates it there (dot(N, V) clamped at 0.1 in the denominator, chi(dot(N, H)) of the evaluated half vector)."""
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


def _midpoint_rect(density, mu0, mu1, phi0, phi1, sub):
    mu = mu0 + (np.arange(sub) + 0.5) * ((mu1 - mu0) / sub)
    phi = phi0 + (np.arange(sub) + 0.5) * ((phi1 - phi0) / sub)
    st = np.sqrt(1.0 - mu * mu)
    L = np.stack([st[:, None] * np.cos(phi)[None, :], st[:, None] * np.sin(phi)[None, :], np.broadcast_to(mu[:, None], (sub, sub))], axis=-1)
    return float(np.asarray(density(L.reshape(-1, 3)), np.float64).sum()) * ((mu1 - mu0) / sub) * ((phi1 - phi0) / sub)


def _graded_rect(density, mu0, mu1, phi0, phi1, sub, point, levels):
    """the midpoint rule on a rectangle that is halved in both directions, level after level, around the point it contains or touches"""
    tol = 1e-12
    if levels == 0 or not (mu0 - tol <= point[0] <= mu1 + tol and phi0 - tol <= point[1] <= phi1 + tol):
        return _midpoint_rect(density, mu0, mu1, phi0, phi1, sub)
    mm, pm = 0.5 * (mu0 + mu1), 0.5 * (phi0 + phi1)
    return sum(_graded_rect(density, a, b, c, d, sub, point, levels - 1)
               for a, b in ((mu0, mm), (mm, mu1)) for c, d in ((phi0, pm), (pm, phi1)))


def density_cells(density, n_mu=8, n_phi=16, sub=64, refine_at=None, levels=0):
    """The integral of density(L) over each cell of a grid of n_mu (cos theta = L.z, 0 ... 1) x n_phi (phi = atan2(L.y, L.x), 0 ... 2 pi)
    cells of the hemisphere around +z: the midpoint rule on sub x sub points per cell, in float64 -> (n_mu, n_phi).  density takes
    (M, 3) float64 unit vectors and returns (M,) values per unit solid angle; d omega = d mu d phi.

    refine_at = (mu, phi), 0 < phi < 2 pi: the cells that contain or touch that point are integrated on a graded grid instead, halved
    `levels` times around it with sub x sub midpoints in every piece.  The density of a reflection about a sampled half vector,
    D N.H / (4 V.H), has an integrable 1 / r singularity at L = -V (V.H = 0), which lies inside the hemisphere for a view from behind
    the normal and just below its horizon for a grazing one; there the plain midpoint rule converges with the first power of the
    spacing only, the graded one loses nothing to it."""
    mu = (np.arange(n_mu * sub) + 0.5) / (n_mu * sub)
    phi = (np.arange(n_phi * sub) + 0.5) * (2.0 * np.pi / (n_phi * sub))
    st = np.sqrt(1.0 - mu * mu)
    out = np.zeros((n_mu, n_phi))
    for i in range(n_mu):
        rows = slice(i * sub, (i + 1) * sub)
        L = np.stack([st[rows, None] * np.cos(phi)[None, :], st[rows, None] * np.sin(phi)[None, :],
                      np.broadcast_to(mu[rows, None], (sub, len(phi)))], axis=-1)
        f = np.asarray(density(L.reshape(-1, 3)), np.float64).reshape(sub, n_phi, sub)
        out[i] = f.sum(axis=(0, 2))
    out *= (1.0 / (n_mu * sub)) * (2.0 * np.pi / (n_phi * sub))
    if refine_at is not None and levels > 0:
        dm, dp, tol = 1.0 / n_mu, 2.0 * np.pi / n_phi, 1e-12
        for i in range(n_mu):
            for j in range(n_phi):
                if i * dm - tol <= refine_at[0] <= (i + 1) * dm + tol and j * dp - tol <= refine_at[1] <= (j + 1) * dp + tol:
                    out[i, j] = _graded_rect(density, i * dm, (i + 1) * dm, j * dp, (j + 1) * dp, sub, refine_at, levels)
    return out


def albedo_quadrature_half_vector(roughness, metallic, color, nov, n_theta=900, n_psi=1800):
    """The integral of albedo_quadrature over the half vector instead of the direction: L = 2 (V.H) H - V, d omega_L = 4 (V.H) d omega_H,
    H over the half of the sphere with V.H > 0 (which L covers the sphere from once), on a midpoint grid of (theta_h, psi) around N = +z,
    d omega_H = sin theta_h d theta_h d psi -> (3,).  For a grazing view of a narrow lobe the directions of the lobe lie in a sliver
    2 alpha wide and 2 alpha (V.H) thick that no uniform grid of directions resolves, while the half vectors fill a round cap of
    radius alpha.  The integrand is continuous: BRDF * dot(N, L) goes to 0 at the horizon and the Jacobian at V.H = 0."""
    N = np.array([0.0, 0.0, 1.0])
    V = np.array([np.sqrt(1.0 - nov * nov), 0.0, nov])
    color = np.asarray(color, np.float64)
    om = 1.0 - metallic
    F0 = color * metallic + 0.04 * om
    psi = (np.arange(n_psi) + 0.5) * (2.0 * np.pi / n_psi)
    total = np.zeros(3)
    for block in np.array_split(np.arange(n_theta), 24):
        th = (block + 0.5) * (np.pi / n_theta)
        st, ct = np.sin(th), np.cos(th)
        H = np.stack([st[:, None] * np.cos(psi)[None, :], st[:, None] * np.sin(psi)[None, :], np.broadcast_to(ct[:, None], (len(th), n_psi))], axis=-1).reshape(-1, 3)
        voh = H @ V
        L = 2.0 * voh[:, None] * H - V
        jac = np.where((voh > 0.0) & (L[:, 2] > 0.0), 4.0 * voh * L[:, 2], 0.0) * np.repeat(st, n_psi)
        total += (brdf(N, V, L, roughness, F0, om, color) * jac[:, None]).sum(0)
    return total * (np.pi / n_theta) * (2.0 * np.pi / n_psi)
