"""The device compile of the numerical contract (include/rtr_math.h, and the device-only slab forms of kernels/rtr_device.h) held to
the host compile, bit for bit, over whole domains.  Both sides are the op table of tests/math_probe/math_ops.h: libmath_probe.so is
built by the product's Makefile with the product's compiler, target and flags, libmath_probe_host.so by the oracle's Makefile with
the oracle's.  tests/test_math_contract.py holds the host side to float64 references.

The comparison rule
  * Results are compared as bit patterns; the sign of a zero counts.
  * NaN: any NaN equals any NaN (x86 and gfx950 produce default NaNs of different sign; the contract promises none).
  * rtr_hwmin / rtr_hwmax: operands are NaN-free and zeros compare by value — the precondition written above them in rtr_math.h
    ("only for NaN-free operands whose zero sign is never observed").  The same holds for rtr_slab, rtr_slab_q and the device
    forms built on them: inputs that would form a NaN plane distance are outside the domain.  rtr_safe_rcp_dir keeps every
    reciprocal direction finite and non-zero, box planes are finite (non-finite vertices and transforms are rejected when a scene
    is made or updated: bvh_build.cpp, rtr_api.cpp), so fma(finite, finite non-zero, anything but NaN) is never NaN; the lattices
    below are built the same way.
  * rtr_div_by: zeros compare by value ("a zero keeps its value, not always its sign", rtr_math.h).
  * Float-to-int conversions, undefined for NaN and out of range, x86 and gfx950 differing there:
      rtr_unorm8  converts a value the select-form clamp has put into [0, 255], NaN included (-> 0): never out of range.
      rtr_exp2    converts floor(z + 0.5) with z in [-126, 127] — or NaN for z = NaN.  Its callers (rtr_pow: x >= FLT_MIN and a
                  constant exponent; exp_f of the denoise kernels: differences of UNORM8 values over positive constants) pass no
                  NaN, and where one is passed the converted value only scales a polynomial that is NaN already.  NaN stays in
                  the swept domain and compares as NaN.
      rtr_quant_lo / rtr_quant_hi  clamp in double before converting, but the clamp let a NaN quotient through.  A device build
                  can form one (finite vertices times a finite transform overflowing to inf), so this was FIXED in rtr_math.h:
                  the clamp now sends NaN to 0.  Non-finite v, origin and scale are in the lattice.

Sweeps: measured time of a full 2^32 host sweep per op (8 cores; math_probe_sweep uses at most 16 threads) and what is run:
    sqrt 5.2 s, pcg_hash 1.7, random 2.6, log2 4.0, exp2 4.4, pow_2_2 4.0, pow_5 3.2, unorm8_to_float 1.8 (its domain is 0..255),
    safe_rcp_dir 2.2, aces 3.8, to_linear 3.8, unorm8 1.8                                        -> all 2^32 patterns
    pow_inv_2_2 5.7, to_srgb 5.5 (srgb_unorm8 the same), acos 8.4, atan_small 11.6, atan2_y1 21.4, atan2_1x 21.5
                                                                                                 -> stride 31 + neighbourhoods
A strided sweep visits every 31st pattern (every exponent, both signs) and all 2^20 patterns on either side of +-0, +-FLT_MIN,
+-1, +-inf, +-0.41421356237 (the atan split), +-126 and +-127 (exp2's ends)."""
import numpy as np
import pytest

import probe_lib as P

F32 = np.float32
U32 = np.uint32
CHUNK = P.CHUNK


def bits(x):
    return int(np.asarray(x, F32).view(U32))


def f32(words):
    return np.ascontiguousarray(words, U32).view(F32)


def _pm(*xs):
    return [s * x for x in xs for s in (1.0, -1.0)]


def _near(x):
    x = F32(x)
    return [float(np.nextafter(x, F32(0))), float(x), float(np.nextafter(x, F32(np.inf)))]


# the value set of the lattices: finite part, then inf and NaN
FINITE = f32(np.array([bits(v) for v in _pm(0.0, 1e-45, 1.1754942e-38, 1.17549435e-38, 1e-20, *_near(1e-5), *_near(1.0), 65535.0, 1e20,
                                             3.4028235e38)], U32))
NANFREE = np.concatenate([FINITE, np.array([np.inf, -np.inf], F32)])
VALUES = np.concatenate([NANFREE, np.array([np.nan], F32)])

MUTANTS = {"mut_atan_small", "mut_hwmin"}
RAN = set()                          # ops that went through a device-equals-host assertion


def product(vals, k):
    g = np.meshgrid(*([vals] * k), indexing="ij")
    return np.stack([a.ravel() for a in g], 1).astype(F32)


def draw(rng, vals, n, k):
    return vals[rng.integers(vals.size, size=(n, k))].astype(F32)


def rbits(rng, n, k, finite=False, nanfree=False):
    w = rng.integers(0, 1 << 32, size=(n, k), dtype=np.uint64).astype(U32)
    f = w.view(F32)
    if finite:
        w[~np.isfinite(f)] = bits(1.5)
    elif nanfree:
        w[np.isnan(f)] = bits(-2.5)
    return w.view(F32)


# ---- the two assertions ---------------------------------------------------------------------------------------------------------------
def assert_sweep_equal(host, dev, op, segments, device_op=None):
    """digests of every segment (first, count, stride) equal chunk by chunk; a differing chunk is re-evaluated element by element"""
    dop = device_op or op
    for first, count, stride in segments:
        h, d = host.sweep(op, first, count, stride), dev.sweep(dop, first, count, stride)
        bad = np.flatnonzero(h != d)
        if bad.size:
            c = int(bad[0])
            n = min(CHUNK, count - c * CHUNK)
            pat = ((first + (c * CHUNK + np.arange(n, dtype=np.uint64)) * stride) & 0xFFFFFFFF).astype(U32).reshape(-1, 1)
            rh, rd = P.canon(op, host, host.eval(op, pat)), P.canon(op, host, dev.eval(dop, pat))
            rows = np.flatnonzero((rh != rd).any(1))
            assert rows.size, f"{op}: digests of chunk {c} differ ({int(h[c]):#x} / {int(d[c]):#x}) but no element does"
            i = int(rows[0])
            raise AssertionError(f"{op}: first difference at pattern 0x{int(pat[i, 0]):08x} ({f32(pat[i])[0]!r}): "
                                 f"host {' '.join(f'0x{int(w):08x}' for w in rh[i])}, device {' '.join(f'0x{int(w):08x}' for w in rd[i])}"
                                 f" ({rows.size} of {n} patterns of the chunk differ)")
    RAN.add(op)


def assert_lattice_equal(host, dev, op, tuples, zeros=False, device_op=None, host_op=None):
    t = np.ascontiguousarray(tuples, F32).view(U32).reshape(-1, host.nin[op]) if np.asarray(tuples).dtype != U32 else tuples
    assert 0 < t.shape[0] <= 1 << 22
    rh, rd = P.canon(op, host, host.eval(host_op or op, t)), P.canon(op, host, dev.eval(device_op or op, t))
    if zeros:
        rh, rd = P.zeros_by_value(op, host, rh), P.zeros_by_value(op, host, rd)
    rows = np.flatnonzero((rh != rd).any(1))
    if rows.size:
        i = int(rows[0])
        raise AssertionError(f"{op}: {rows.size} of {t.shape[0]} tuples differ; first: in {' '.join(f'0x{int(w):08x}' for w in t[i])} "
                             f"({f32(t[i]).tolist()}): host {' '.join(f'0x{int(w):08x}' for w in rh[i])}, "
                             f"device {' '.join(f'0x{int(w):08x}' for w in rd[i])}")
    RAN.add(op)


# ---- sweeps ---------------------------------------------------------------------------------------------------------------------------
FULL = [(0, 1 << 32, 1)]
_CENTRES = [bits(v) for v in _pm(0.0, 1.17549435e-38, 1.0, np.inf, 0.41421356237, 126.0, 127.0)]
STRIDED = [(0, (1 << 32) // 31 + 1, 31)] + [((c - CHUNK) & 0xFFFFFFFF, 2 * CHUNK, 1) for c in _CENTRES]
SWEEPS = {
    "sqrt": FULL, "pcg_hash": FULL, "random": FULL, "log2": FULL, "exp2": FULL, "pow_2_2": FULL, "pow_5": FULL,
    "safe_rcp_dir": FULL, "aces": FULL, "to_linear": FULL, "unorm8": FULL,
    "pow_inv_2_2": STRIDED, "to_srgb": STRIDED, "srgb_unorm8": STRIDED, "acos": STRIDED, "atan_small": STRIDED,
    "atan2_y1": STRIDED, "atan2_1x": STRIDED,
    "unorm8_to_float": [(0, 256, 1)],
}


@pytest.fixture(scope="module")
def probes(gpu_ctx):
    return P.host(), P.device()


@pytest.mark.gpu
@pytest.mark.parametrize("op", sorted(SWEEPS))
def test_sweep_device_equals_host(probes, op):
    assert_sweep_equal(*probes, op, SWEEPS[op])


# ---- lattices: scalar helpers ---------------------------------------------------------------------------------------------------------
def lat_pairs(rng):
    return np.concatenate([product(VALUES, 2), rbits(rng, 1 << 16, 2)])


def lat_triples(rng):
    return np.concatenate([product(VALUES, 3), rbits(rng, 1 << 16, 3)])


def lat_hw(rng):
    return np.concatenate([product(NANFREE, 2), rbits(rng, 1 << 16, 2, nanfree=True)])


DIVISORS = np.array([0.001, 0.37] + [float((i + 1) ** 2) for i in range(64)], F32)      # test_math.py: what rtr_denoise_combine can issue


def lat_div_by(rng):
    """the value set squared with r = fl(1 / b); and the real domain: |a| <= 16 of either sign, every divisor in use"""
    with np.errstate(all="ignore"):
        ab = product(VALUES, 2)
        a = rbits(rng, 4096, 1)[:, 0].view(U32)
        a = f32((a & U32(0x80000000)) | (U32(bits(2.0 ** -40)) + a % U32(bits(16.0) - bits(2.0 ** -40) + 1)))
        a = np.concatenate([a, np.array([0.0, -0.0, 16.0, -16.0], F32)])
        real = np.stack([np.repeat(a, DIVISORS.size), np.tile(DIVISORS, a.size)], 1)
        ab = np.concatenate([ab, real])
        return np.concatenate([ab, (F32(1.0) / ab[:, 1:2]).astype(F32)], 1)


def lat_pow(rng):
    x = rbits(rng, 1 << 15, 1)
    ys = np.array([2.2, 0.45454545454545453, 5.0], F32)
    return np.concatenate([product(VALUES, 2), rbits(rng, 1 << 14, 2)] + [np.concatenate([x, np.full_like(x, y)], 1) for y in ys])


def lat_atan2(rng):
    return np.concatenate([product(VALUES, 2), rbits(rng, 1 << 16, 2), rng.normal(0, 1, (1 << 16, 2)).astype(F32)])


# ---- lattices: vectors and transforms -------------------------------------------------------------------------------------------------
def lat_vec(k):
    def make(rng):
        parts = [draw(rng, VALUES, 1 << 17, k), rbits(rng, 1 << 15, k), rng.normal(0, 1, (1 << 15, k)).astype(F32), np.zeros((1, k), F32)]
        if k == 3:
            parts.append(product(VALUES, 3))             # the zero vector, squared lengths that overflow (1e20) or are denormal (1e-20)
        else:
            pair = product(VALUES, 2)
            rest = draw(rng, FINITE, pair.shape[0], k - 2)
            parts.append(np.concatenate([pair[:, :1], rest[:, :2], pair[:, 1:], rest[:, 2:]], 1))
        return np.concatenate(parts)
    return make


def _matrices(rng, n):
    """3x3 blocks: identity, mirrored, singular (a repeated row, a zero row, rank one), rotations, scaled; then random and value-set ones"""
    eye = np.eye(3, dtype=F32)
    fixed = [eye, np.diag([-1, 1, 1]).astype(F32), np.diag([1, -1, -1]).astype(F32), -eye,
             np.array([[1, 2, 3], [1, 2, 3], [0, 1, 0]], F32), np.array([[1, 0, 0], [0, 0, 0], [0, 0, 1]], F32),
             np.outer([1, 2, 3], [4, 5, 6]).astype(F32), np.zeros((3, 3), F32), eye * F32(1e-20), eye * F32(1e20), eye * F32(3e5)]
    q, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    rot = (q * rng.choice([1e-3, 1.0, 3e5], size=(n, 1, 1))).astype(F32)
    return np.concatenate([np.stack(fixed), rot, draw(rng, VALUES, n, 9).reshape(n, 3, 3), rbits(rng, n // 4, 9).reshape(-1, 3, 3)])


def lat_xform(kind):
    def make(rng):
        m3 = _matrices(rng, 1 << 12)
        pts = np.concatenate([product(VALUES, 3)[:: 7], rng.normal(0, 1, (4096, 3)).astype(F32) * F32(3e5), rbits(rng, 1024, 3)])
        mi, pi = rng.integers(m3.shape[0], size=1 << 17), rng.integers(pts.shape[0], size=1 << 17)
        mi[: 11 * 64], pi[: 11 * 64] = np.repeat(np.arange(11), 64), np.tile(np.arange(64), 11)
        m, p = m3[mi], pts[pi]
        tr = draw(rng, np.concatenate([VALUES, np.array([3e5, -3e5, 1e-3], F32)]), m.shape[0], 3)
        if kind == "mul33":
            return np.concatenate([m.reshape(-1, 9), p], 1)
        if kind == "34":
            return np.concatenate([np.concatenate([m, tr[:, :, None]], 2).reshape(-1, 12), p], 1)
        if kind == "normal":
            return np.concatenate([m, tr[:, :, None]], 2).reshape(-1, 12)
        m4 = np.zeros((m.shape[0], 4, 4), F32)            # column-major: m4[c, r]
        m4[:, :3, :3] = m.transpose(0, 2, 1)
        m4[:, 3, :3] = tr
        m4[:, :, 3] = draw(rng, VALUES, m.shape[0], 4)    # the bottom row, which the function does not read
        return np.concatenate([m4.reshape(-1, 16), p], 1)
    return make


# ---- lattices: the triangle -----------------------------------------------------------------------------------------------------------
def lat_mt(rng):
    """rays through edges and vertices, parallel to the plane, determinants around +-1e-5, t around tmin, (u, v, u + v) around 0
    and 1, slivers and zero-area records; triangles of size 1e-3, 1 and 3e5, at the origin and 3e5 away (conditioned_scenes.py)"""
    host = P.host()
    out = []
    edge = np.array([0.0, 1.0, 0.5, 1e-7, 1 - 1e-7, -1e-7, 1 + 1e-7, 0.25, 1e-3], np.float64)
    uv = np.array([(u, v) for u in edge for v in edge] + [(u, 1 - u + e) for u in edge for e in (0, 1e-7, -1e-7)])
    for size in (1e-3, 1.0, 3e5):
        for centre in (0.0, 3e5):
            n = 96
            v0 = (rng.normal(0, size, (n, 3)) + centre)
            e1, e2 = rng.normal(0, size, (n, 3)), rng.normal(0, size, (n, 3))
            e2[:8] = e1[:8] * rng.uniform(-2, 2, (8, 1))                       # zero area: collinear edges
            e1[8:12] = 0                                                       # a zero edge
            e2[12:16] = e1[12:16] + rng.normal(0, size * 1e-6, (4, 3))         # slivers
            e2[16:20] = e1[16:20]
            ti = np.repeat(np.arange(n), uv.shape[0])
            uu, vv = np.tile(uv[:, 0], n), np.tile(uv[:, 1], n)
            target = v0[ti] + uu[:, None] * e1[ti] + vv[:, None] * e2[ti]
            nrm = np.cross(e1[ti], e2[ti])
            nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
            o = target + nrm * rng.choice([size, 10 * size, 1e-3 * size], size=(ti.size, 1)) * rng.choice([-1, 1], size=(ti.size, 1)) \
                + rng.normal(0, size, (ti.size, 3)) * rng.choice([0, 1], size=(ti.size, 1))
            d = target - o
            d[::3] /= np.maximum(np.linalg.norm(d[::3], axis=1, keepdims=True), 1e-300)
            inplane = e1[ti] * rng.normal(size=(ti.size, 1)) + e2[ti] * rng.normal(size=(ti.size, 1))
            d[1::7] = inplane[1::7]                                            # parallel to the plane
            # determinants a few ULP around +-1e-5: scale d so that a = e1 . (d x e2) lands there
            a = np.einsum("ij,ij->i", e1[ti], np.cross(d, e2[ti]))
            k = np.arange(ti.size) % 5 == 2
            with np.errstate(all="ignore"):
                s = np.where(np.abs(a) > 0, 1e-5 / np.abs(a), 1.0) * (1 + rng.integers(-4, 5, ti.size) * 2.0 ** -24)
            d[k] *= s[k, None]
            tmin = rng.choice([0.0, 1e-3, 1e-4], size=(ti.size, 1))
            t = np.concatenate([o, d, v0[ti], e1[ti], e2[ti], tmin], 1).astype(F32)
            # t a few ULP around tmin: take the host's t, put tmin beside it
            r = host.eval("mt_intersect", t.view(U32))
            hit = np.flatnonzero(r[:, 0] == 1)[:2048]
            near = t[hit].copy()
            near[:, 15] = f32((r[hit, 1].astype(np.int64) + rng.integers(-3, 4, hit.size)).astype(U32))
            out += [t, near]
    out += [draw(rng, VALUES, 1 << 16, 16), rbits(rng, 1 << 14, 16)]
    return np.concatenate(out)


# ---- lattices: ray setup and boxes ----------------------------------------------------------------------------------------------------
def _scenes(rng, n):
    """scene bounds: sizes 1e-3, 1, 3e5, at the origin and 3e5 away, some flat (extent 0) on an axis"""
    size = rng.choice([1e-3, 1.0, 3e5], size=(n, 1))
    lo = (rng.normal(0, 1, (n, 3)) * size + rng.choice([0.0, 3e5], size=(n, 1))).astype(F32)
    hi = (lo + np.abs(rng.normal(0, 1, (n, 3)) * size).astype(F32)).astype(F32)
    flat = rng.integers(0, 4, size=n)
    for k in range(3):
        hi[flat == k, k] = lo[flat == k, k]
    return lo, hi


def _dirs(rng, n):
    d = rng.normal(0, 1, (n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d.astype(F32)
    kill = rng.integers(0, 8, size=(n, 3)) == 0            # axis-parallel rays: zero components (idir = +-1e20)
    d[kill] = rng.choice(np.array([0.0, -0.0, 1e-30, -1e-25], F32), size=int(kill.sum()))
    return d


def chain(rng, n):
    """the path's own chain, evaluated by the host library: bounds -> grid; direction -> idir; (o, idir, grid) -> ga, gb, gbc"""
    host = P.host()
    lo, hi = _scenes(rng, n)
    g = f32(host.eval("grid_from_bounds", np.concatenate([lo, hi], 1).view(U32)))
    origin, scale = g[:, :3].copy(), g[:, 3:].copy()
    d = _dirs(rng, n)
    idir = f32(host.eval("safe_rcp_dir", d.reshape(-1, 1).view(U32))).reshape(n, 3)
    o = (lo + (hi - lo) * rng.uniform(-8, 9, (n, 3)).astype(F32)).astype(F32)
    rg = f32(host.eval("ray_grid", np.concatenate([o, idir, origin, scale], 1).view(U32)))
    cw = rng.integers(0, 1 << 32, size=(n, 2), dtype=np.uint64).astype(U32)
    cw[::5] = U32(0x80008000)
    centre = f32(host.eval("wide_centre_world", np.concatenate([origin.view(U32), scale.view(U32), cw], 1)))
    ra = f32(host.eval("ray_grid_about", np.concatenate([o, idir, scale, centre], 1).view(U32)))
    tmin = rng.choice(np.array([0.0, 1e-3, 1e-4], F32), size=(n, 1))
    tmax = rng.choice(np.array([np.inf, 1e30, 1.0, 1e3, 5e5], F32), size=(n, 1))
    return dict(lo=lo, hi=hi, origin=origin, scale=scale, o=o, d=d, idir=idir, ga=rg[:, :3].copy(), gb=rg[:, 3:].copy(),
                cw=cw, centre=centre, gbc=ra[:, 3:].copy(), tmin=tmin, tmax=tmax)


def _slab_ok(a, b):
    """inside the precondition of rtr_hwmin / rtr_hwmax: slope finite, offset not NaN -> no NaN plane distance for finite planes"""
    return np.isfinite(a).all(1) & ~np.isnan(b).any(1)


def quant_lattice(rng, n):
    """(v, origin, scale) per axis: v on a grid plane (origin + k scale, as fp32 gives it) and one ULP off, at both ends of the
    grid, inside, outside; flat scenes"""
    c = chain(rng, n)
    k = rng.integers(0, 65536, size=(n, 3)).astype(F32)
    on = (c["origin"] + k * c["scale"]).astype(F32)
    vs = [on, np.nextafter(on, F32(np.inf)), np.nextafter(on, F32(-np.inf)), c["lo"], c["hi"],
          (c["lo"] + (c["hi"] - c["lo"]) * rng.uniform(-0.1, 1.1, (n, 3)).astype(F32)).astype(F32)]
    return np.concatenate([np.stack([v.ravel(), c["origin"].ravel(), c["scale"].ravel()], 1) for v in vs]).astype(F32).view(U32)


def lat_quant(rng):
    t = f32(quant_lattice(rng, 1 << 13)).reshape(-1, 3)
    return np.concatenate([t, product(VALUES, 3), rbits(rng, 1 << 14, 3)])           # non-finite v, origin and scale included


def lat_grid_from_bounds(rng):
    lo, hi = _scenes(rng, 1 << 15)
    return np.concatenate([np.concatenate([lo, hi], 1), draw(rng, VALUES, 1 << 15, 6), rbits(rng, 1 << 13, 6)])


def lat_ray_grid(rng):
    c = chain(rng, 1 << 15)
    return np.concatenate([np.concatenate([c["o"], c["idir"], c["origin"], c["scale"]], 1), draw(rng, VALUES, 1 << 15, 12), rbits(rng, 1 << 13, 12)])


def lat_ray_grid_about(rng):
    c = chain(rng, 1 << 15)
    return np.concatenate([np.concatenate([c["o"], c["idir"], c["scale"], c["centre"]], 1), draw(rng, VALUES, 1 << 15, 12), rbits(rng, 1 << 13, 12)])


def lat_wide_centre(rng):
    c = chain(rng, 1 << 15)
    n = 1 << 14
    w = rng.integers(0, 1 << 32, size=(n, 2), dtype=np.uint64).astype(U32)
    return np.concatenate([np.concatenate([c["origin"].view(U32), c["scale"].view(U32), c["cw"]], 1),
                           np.concatenate([draw(rng, VALUES, n, 6).view(U32), w], 1)])


def lat_slab(rng):
    n = 1 << 16
    c = chain(rng, n)
    with np.errstate(all="ignore"):
        ood = (-c["o"] * c["idir"]).astype(F32)               # overflows to +-inf for axis-parallel rays far from the origin
    bl, bh = _scenes(rng, n)
    bl[::2] = (c["lo"] + (c["hi"] - c["lo"]) * rng.uniform(0, 0.6, (n, 3)).astype(F32))[::2]
    bh[::2] = (bl + (c["hi"] - c["lo"]) * rng.uniform(0, 0.4, (n, 3)).astype(F32))[::2]
    t = np.concatenate([bl, bh, c["idir"], ood, c["tmin"], c["tmax"]], 1).astype(F32)
    extra = np.concatenate([draw(rng, FINITE, n, 6), c["idir"], draw(rng, NANFREE, n, 3), draw(rng, NANFREE, n, 2)], 1)
    return np.concatenate([t[_slab_ok(c["idir"], ood)], extra])


def _boxes(rng, n):
    a, b = rng.integers(0, 65536, size=(n, 3)), rng.integers(0, 65536, size=(n, 3))
    a[::7], b[::7] = 0, 65535
    b[1::7] = a[1::7]                                          # flat boxes
    return np.minimum(a, b).astype(U32), np.maximum(a, b).astype(U32)


def _rays(rng, n, about=False):
    """(ga, gb, tmin, tmax) of the chain, with the non-finite slopes and NaN offsets the precondition excludes replaced"""
    c = chain(rng, n)
    ga, gb = c["ga"], c["gbc" if about else "gb"]
    bad = ~_slab_ok(ga, gb)
    ga[bad], gb[bad] = F32(0.25), F32(-3.0)
    third = n // 3
    ga[:third] = draw(rng, FINITE, third, 3)                   # +-0, denormal and huge slopes; offsets of the value set, +-inf too
    gb[:third] = draw(rng, NANFREE, third, 3)
    return ga, gb, c["tmin"], c["tmax"]


def lat_slab_q(rng):
    n = 1 << 17
    qlo, qhi = _boxes(rng, n)
    ga, gb, tmin, tmax = _rays(rng, n)
    return np.concatenate([qlo, qhi, ga.view(U32), gb.view(U32), tmin.view(U32), tmax.view(U32)], 1)


def _words(qlo, qhi):
    return np.stack([qlo[:, 0] | (qlo[:, 1] << 16), qhi[:, 0] | (qhi[:, 1] << 16), qlo[:, 2] | (qhi[:, 2] << 16)], 1).astype(U32)


def _octant(ga, k):
    """the slopes with the signs of octant k (bit a set: ga.a < 0; a zero of either sign counts as >= 0)"""
    g = np.abs(ga)
    for a in range(3):
        if (k >> a) & 1:
            g[:, a] = -np.where(g[:, a] == 0, F32(1e-30), g[:, a])
        else:
            g[::11, a] = np.where(g[::11, a] == 0, F32(-0.0), g[::11, a])
    return g.astype(F32)


def lat_slab_pair(rng):
    n = 1 << 17
    w = rng.integers(0, 1 << 32, size=(n, 3), dtype=np.uint64).astype(U32)      # any (wmin, wmax, wz): inside-out boxes too
    w[: n // 2] = _words(*_boxes(rng, n // 2))
    ga, gb, tmin, tmax = _rays(rng, n)
    return np.concatenate([w, ga.view(U32), gb.view(U32), tmin.view(U32), tmax.view(U32)], 1)


def lat_slab_oct(k):
    def make(rng):
        n = 1 << 16
        ga, gb, tmin, tmax = _rays(rng, n)
        return np.concatenate([_words(*_boxes(rng, n)), _octant(ga, k).view(U32), gb.view(U32), tmin.view(U32), tmax.view(U32)], 1)
    return make


HALVES = np.concatenate([np.arange(0x0000, 0x7C00), np.arange(0x8000, 0xFC00)]).astype(np.uint16)      # every finite half: 63 488


def lat_slab_wide(k):
    """planes: every finite half value on one axis (each axis in turn), random ones on the other two, ordered pmin <= pmax per axis
    for k < 8; tmax finite (vmin_raw's precondition), also exactly the far z distance and one ULP either side of it"""
    def make(rng):
        host = P.host()
        out = []
        for axis in range(3):
            n = HALVES.size
            p0, p1 = HALVES[rng.integers(n, size=(n, 3))], HALVES[rng.integers(n, size=(n, 3))]
            p0[:, axis] = HALVES
            if k < 8:
                f0, f1 = p0.view(np.float16).astype(F32), p1.view(np.float16).astype(F32)      # exact
                swap = f0 > f1
                p0, p1 = np.where(swap, p1, p0), np.where(swap, p0, p1)
            p0, p1 = p0.astype(U32), p1.astype(U32)
            w = _words(p0, p1)
            ga, gb, tmin, tmax = _rays(rng, n, about=True)
            if k < 8:
                ga = _octant(ga, k)
            tmax = np.where(np.isfinite(tmax), tmax, F32(1e30)).astype(F32)
            far = np.where(ga[:, 2] < 0, p0[:, 2], p1[:, 2]).astype(np.uint16).view(np.float16).astype(F32)
            fz = f32(host.eval("fma", np.stack([far, ga[:, 2], gb[:, 2]], 1).view(U32)))[:, 0]
            pick = np.isfinite(fz) & (np.arange(n) % 2 == 0)
            near = f32((fz.view(U32).astype(np.int64) + rng.integers(-1, 2, n)).astype(U32))
            pick &= np.isfinite(near)
            tmax[pick, 0] = near[pick]
            out.append(np.concatenate([w, ga.view(U32), gb.view(U32), tmin.view(U32), tmax.view(U32)], 1))
        return np.concatenate(out)
    return make


# op -> (lattice builder, zeros compare by value)
LATTICES = {
    "fma": (lat_triples, False), "min": (lat_pairs, False), "max": (lat_pairs, False), "clamp": (lat_triples, False),
    "hwmin": (lat_hw, True), "hwmax": (lat_hw, True), "div_by": (lat_div_by, True),
    "pow": (lat_pow, False), "atan2": (lat_atan2, False), "pack_bgra8": (lat_triples, False),
    "dot": (lat_vec(6), False), "cross": (lat_vec(6), False), "normalize": (lat_vec(3), False), "length": (lat_vec(3), False),
    "xform_point34": (lat_xform("34"), False), "xform_point44cm": (lat_xform("44"), False), "mul33": (lat_xform("mul33"), False),
    "normal_matrix": (lat_xform("normal"), False),
    "mt_intersect": (lat_mt, False),
    "slab": (lat_slab, True), "grid_from_bounds": (lat_grid_from_bounds, False), "quant_lo": (lat_quant, False), "quant_hi": (lat_quant, False),
    "ray_grid": (lat_ray_grid, False), "wide_centre_world": (lat_wide_centre, False), "ray_grid_about": (lat_ray_grid_about, False),
    "slab_q": (lat_slab_q, True), "slab_pair": (lat_slab_pair, True),
}
LATTICES.update({f"slab_oct{k}": (lat_slab_oct(k), True) for k in range(8)})
LATTICES.update({f"slab_wide{k}": (lat_slab_wide(k), True) for k in range(9)})
LATTICES.update({f"slab_wide_exit{k}": (lat_slab_wide(k), True) for k in range(9)})


@pytest.mark.gpu
@pytest.mark.parametrize("op", sorted(LATTICES))
def test_lattice_device_equals_host(probes, op):
    make, zeros = LATTICES[op]
    assert_lattice_equal(*probes, op, make(np.random.default_rng(len(op) * 1000 + sum(map(ord, op)))), zeros=zeros)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(8))
def test_slab_oct_gives_slab_pairs_answer(probes, k):
    """slab_oct<k> against slab_pair, both on the device, on boxes with qmin <= qmax and rays of octant k: decision and t_entry"""
    host, dev = probes
    t = lat_slab_oct(k)(np.random.default_rng(40 + k))
    a, b = (P.zeros_by_value("slab_pair", host, P.canon("slab_pair", host, dev.eval(op, t))) for op in (f"slab_oct{k}", "slab_pair"))
    rows = np.flatnonzero((a != b).any(1))
    assert rows.size == 0, (k, rows.size, t[rows[0]].tolist(), a[rows[0]].tolist(), b[rows[0]].tolist())


def test_every_op_has_a_domain():
    """every op of the table appears in a sweep or a lattice above (the mutants excepted, which must differ)"""
    assert set(SWEEPS) | set(LATTICES) == set(P.host().names) - MUTANTS
    assert all(P.host().nin[op] == 1 for op in SWEEPS)


@pytest.mark.gpu
def test_every_op_was_compared(probes):
    """runs last: the ops that went through a device-equals-host assertion in this session are the whole table"""
    assert RAN == set(probes[0].names) - MUTANTS, sorted(set(probes[0].names) - MUTANTS - RAN)
