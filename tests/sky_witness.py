"""An independent restatement of include/rtr_sky.h for the tests: numpy, float64 and Python integers, sharing no code with the header.

The sky table is a table of INTEGERS and is held to this witness exactly, so the one place where float32 rounding decides an integer —
weight = (uint32_t)(M * s_y * 65536.0f), with M a float32 power and s_y a float32 sine — is restated here in exact rational
arithmetic (fractions.Fraction over Python integers) rounded to binary32 once per operation, which is what IEEE-754 asks of + - * /
and fma.  Everything else (the prefix sums, the 3 x 3 neighbourhood, the density, the radiance, the quadratures) is float64 or integer."""
import ctypes as C
from fractions import Fraction

import numpy as np

import bounce_witness as BW

F32 = np.float32
PI_MISS = 3.14159265          # the miss rule's pi
CONST_W, CONST_H = 32, 16


# ---- binary32, one correctly rounded operation at a time -------------------------------------------------------------------------
def _round32(q):
    """the binary32 nearest to the rational q, ties to even (no overflow in the uses here)"""
    if q == 0:
        return F32(0.0)
    s, q = (-1, -q) if q < 0 else (1, q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    e = max(e, -126)
    scale = Fraction(2) ** (23 - e)
    n = q * scale
    r = n.numerator // n.denominator
    rem = n - r
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (r & 1)):
        r += 1
    return F32(s * float(Fraction(r) / scale))


def _q(x):
    return Fraction(float(x))


def _k(text):
    """a C float literal"""
    return _round32(Fraction(text))


def _fma(a, b, c):
    return _round32(_q(a) * _q(b) + _q(c))


def _mul(a, b):
    return _round32(_q(a) * _q(b))


def _add(a, b):
    return _round32(_q(a) + _q(b))


def _div(a, b):
    return _round32(_q(a) / _q(b))


def _bits(x):
    return int(np.array(x, F32).view(np.uint32))


def _from_bits(u):
    return np.array(u & 0xffffffff, np.uint32).view(F32)[()]


def _log2(x):
    t = (_bits(x) + (0x3f800000 - 0x3f3504f3)) & 0xffffffff
    e = (t >> 23) - 127
    m = _from_bits((t & 0x007fffff) + 0x3f3504f3)
    s = _div(_add(m, F32(-1.0)), _add(m, F32(1.0)))
    z = _mul(s, s)
    p = _k("0.09090909090909091")
    for c in ("0.1111111111111111", "0.14285714285714285", "0.2", "0.3333333333333333", "1.0"):
        p = _fma(p, z, _k(c))
    return _fma(_mul(_add(s, s), p), _k("1.4426950408889634"), F32(e))


def _exp2(z):
    if z < F32(-126.0):
        return F32(0.0)
    if z > F32(127.0):
        z = F32(127.0)
    nf = F32(np.floor(_add(z, F32(0.5))))
    r = _mul(_add(z, -nf), _k("0.6931471805599453"))
    p = _k("2.48015873015873e-05")
    for c in ("1.984126984126984e-04", "1.388888888888889e-03", "8.333333333333333e-03", "4.1666666666666664e-02", "0.16666666666666666", "0.5", "1.0", "1.0"):
        p = _fma(p, r, _k(c))
    return _mul(p, _from_bits((int(nf) + 127) << 23))


def _to_linear(x):
    if not x >= F32(1.17549435e-38):
        return F32(0.0)
    return _exp2(_mul(_k("2.2"), _log2(x)))


def _unorm8(b):
    x = F32(b)
    return _fma(x, _k("0.0039215688593685627"), _mul(x, _k("-2.3191758e-10")))


def _sin_turn(u):
    """sin(2 pi u), u in [0, 1]: the octant reduction and the degree-7 / degree-8 forms the sampling contract uses"""
    m = _mul(u, F32(8.0))
    q = int(_fma(u, F32(4.0), F32(0.5)))
    r = _add(m, -_mul(F32(2.0), F32(q)))
    x = _mul(r, _k("0.78539816339744831"))
    z = _mul(x, x)
    ps = _fma(_fma(_k("-1.9515295891e-4"), z, _k("8.3321608736e-3")), z, _k("-1.6666654611e-1"))
    s = _fma(_mul(ps, z), x, x)
    pc = _fma(_fma(_k("2.443315711809948e-5"), z, _k("-1.388731625493765e-3")), z, _k("4.166664568298827e-2"))
    c = _fma(_mul(pc, z), z, _fma(F32(-0.5), z, F32(1.0)))
    k = q & 3
    ss = c if k & 1 else s
    return -ss if k & 2 else ss


_LINEAR = None


def linear_of_byte():
    """rtr_to_linear(b / 255) for the 256 bytes, binary32"""
    global _LINEAR
    if _LINEAR is None:
        _LINEAR = np.array([_to_linear(_unorm8(b)) for b in range(256)], F32)
    return _LINEAR


# ---- the table -------------------------------------------------------------------------------------------------------------------
def as_texels(hdri):
    """uint8 (H, W, C) of an (H, W), (H, W, 1) or (H, W, 4) array"""
    px = np.asarray(hdri, np.uint8)
    return px[:, :, None] if px.ndim == 2 else px


def hdri_of(desc):
    """the HDRI of an rtr_scene_desc as uint8 (H, W, C), or None"""
    if not desc.hdri:
        return None
    tx = desc.hdri.contents
    px = np.frombuffer(C.cast(tx.pixels, C.POINTER(C.c_uint8 * (tx.width * tx.height * tx.channels))).contents, dtype=np.uint8)
    return px.reshape(tx.height, tx.width, tx.channels).copy()


def table(hdri=None, sky_color=None):
    """-> (weights, rows, marginal): Python-integer arrays (object dtype is avoided: uint64 holds them) of shape (H, W), (H, W), (H,)"""
    if hdri is None:
        lin = [_to_linear(F32(c)) for c in sky_color]
        m = max(lin)
        M = np.full((CONST_H, CONST_W), min(m, F32(1.0)) if m > 0 else F32(0.0), F32)
    else:
        px = as_texels(hdri)
        lin = linear_of_byte()
        m = lin[px[:, :, :3] if px.shape[2] == 4 else px[:, :, :1]].max(axis=2)
        M = np.max([np.roll(np.roll(m, dy, axis=0), dx, axis=1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)
    H, W = M.shape
    w = np.zeros((H, W), np.uint64)
    for y in range(H):
        s = _sin_turn(_div(_add(F32(y), F32(0.5)), _mul(F32(2.0), F32(H))))
        for v in np.unique(M[y]):
            if v > 0:
                p = _mul(_mul(v, s), F32(65536.0))
                w[y, M[y] == v] = int(p) if p >= 1 else 1
    rows = np.cumsum(w, axis=1, dtype=np.uint64)
    marginal = np.cumsum(rows[:, -1], dtype=np.uint64)
    return w, rows, marginal


# ---- float64: the look-up, the density ---------------------------------------------------------------------------------------------
def uv_of(dirs):
    d = np.asarray(dirs, np.float64)
    d = d / np.linalg.norm(d, axis=1)[:, None]
    hu = np.arctan2(d[:, 2], d[:, 0]) / (2 * PI_MISS) + 0.5
    hv = 1.0 - np.arccos(np.clip(d[:, 1], -1, 1)) / PI_MISS
    return hu, hv, d[:, 1]


def radiance(dirs, hdri=None, sky_color=None):
    """the miss rule in float64 -> (N, 3)"""
    if hdri is None:
        return np.broadcast_to(np.power(np.asarray(sky_color, np.float64), 2.2), (len(dirs), 3)).copy()
    img = as_texels(hdri).astype(np.float64) / 255.0
    H, W = img.shape[:2]
    hu, hv, _ = uv_of(dirs)
    x, y = (hu - np.floor(hu)) * W - 0.5, (hv - np.floor(hv)) * H - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    x0, y0 = x0.astype(np.int64) % W, y0.astype(np.int64) % H
    x1, y1 = (x0 + 1) % W, (y0 + 1) % H
    a = img[y0, x0] * (1 - fx) + img[y0, x1] * fx
    b = img[y1, x0] * (1 - fx) + img[y1, x1] * fx
    out = a * (1 - fy) + b * fy
    if out.shape[1] == 1:
        out = np.concatenate([out, np.zeros((len(out), 2))], axis=1)
    return np.power(out[:, :3], 2.2)


def cells_of(dirs, W, H):
    hu, hv, y = uv_of(dirs)
    cx = np.clip(np.floor(hu * W), 0, W - 1).astype(np.int64)
    cy = np.clip(np.floor(hv * H), 0, H - 1).astype(np.int64)
    return cx, cy, y


def pdf(weights, dirs):
    """the solid-angle density of the table for dirs, float64"""
    H, W = weights.shape
    total = int(weights.sum())
    cx, cy, y = cells_of(dirs, W, H)
    with np.errstate(all="ignore"):
        p = weights[cy, cx].astype(np.float64) / total * W * H / (2 * np.pi ** 2 * np.sqrt(1 - y * y)) if total else np.zeros(len(cx))
    return np.where(np.isfinite(p) & (p > 0), p, 0.0)


def sphere_grid(n_theta, n_phi):
    """midpoints of an equal (theta, phi) grid -> (dirs (n_theta * n_phi, 3), solid angle of each cell)"""
    th = (np.arange(n_theta) + 0.5) * np.pi / n_theta
    ph = (np.arange(n_phi) + 0.5) * 2 * np.pi / n_phi - np.pi
    T, Pp = np.meshgrid(th, ph, indexing="ij")
    dirs = np.stack([np.sin(T) * np.cos(Pp), np.cos(T), np.sin(T) * np.sin(Pp)], -1).reshape(-1, 3)
    dw = (np.cos(th - 0.5 * np.pi / n_theta) - np.cos(th + 0.5 * np.pi / n_theta))[:, None] * np.full((1, n_phi), 2 * np.pi / n_phi)
    return dirs, dw.reshape(-1)


def reflected(ray, surface, hdri=None, sky_color=None, n_theta=1536, n_phi=3072):
    """integral of f cos sky over the directions with dot(N, L) > 0, by the midpoint rule on a (theta, phi) grid about the world's y
    axis (the grid of the HDRI's texel rows and columns: n_theta, n_phi multiples of its extent keep every cell inside one texel cell)"""
    P, N, color = surface[0:3].astype(np.float64), surface[4:7].astype(np.float64), surface[12:15].astype(np.float64)
    metallic, roughness = float(surface[11]), float(surface[15])
    V = ray[0:3].astype(np.float64) - P
    V /= np.linalg.norm(V)
    om = 1.0 - metallic
    F0 = color * metallic + 0.04 * om
    out = np.zeros(3)
    dirs, dw = sphere_grid(n_theta, n_phi)
    for a in range(0, len(dirs), 1 << 20):
        L, w = dirs[a:a + (1 << 20)], dw[a:a + (1 << 20)]
        nol = L @ N
        keep = nol > 0
        L, w, nol = L[keep], w[keep], nol[keep]
        f = BW.brdf(N[None, :], V[None, :], L, roughness, F0[None, :], om, color[None, :])
        out += ((f * radiance(L, hdri, sky_color)) * (nol * w)[:, None]).sum(axis=0)
    return out
