"""The numerical contract (include/rtr_math.h), host compile, held to float64 references; and the contract probe
(tests/math_probe/, tests/probe_lib.py) held to itself.  No GPU.  tests/test_gpu_math_contract.py holds the device compile to this
host compile bit for bit, so the accuracies pinned here are the device's as well.

Every function is evaluated by libmath_probe_host.so: the op table of tests/math_probe/math_ops.h under the oracle's compile line."""
from fractions import Fraction

import numpy as np
import pytest

import probe_lib as P

F32 = np.float32
U32 = np.uint32


def bits(x):
    return int(np.asarray(x, F32).view(U32))


def f32(words):
    return np.ascontiguousarray(words, U32).view(F32)


def strided(lo, hi, stride, ends=1 << 20):
    """bit patterns lo..hi (inclusive): every stride-th, plus all of the first and last `ends`"""
    body = np.arange(lo, hi + 1, stride, dtype=np.uint64)
    return np.unique(np.concatenate([body, np.arange(lo, min(hi, lo + ends) + 1, dtype=np.uint64),
                                     np.arange(max(lo, hi - ends), hi + 1, dtype=np.uint64)])).astype(U32)


@pytest.fixture(scope="module")
def host():
    return P.host()


def run1(host, op, words):
    return f32(host.eval(op, words.reshape(-1, host.nin[op]))[:, 0])


# ---- accuracy ------------------------------------------------------------------------------------------------------------------------
TAN_PI_8 = 0x3ED413CD                # 0.41421356237f, the split point of rtr_atan2


def test_atan_small_is_within_the_headers_bound(host):
    """rtr_atan_small on [0, tan(pi/8)] against np.arctan in float64: every 127th float of the interval and all of the first and
    last 2^20.  Bound: the 2e-7 of the function's comment in rtr_math.h.  Measured: 2.6e-8."""
    w = strided(0, TAN_PI_8, 127)
    err = np.abs(run1(host, "atan_small", w).astype(np.float64) - np.arctan(f32(w).astype(np.float64)))
    print(f"rtr_atan_small: max |err| = {err.max():.3e} rad at x = {f32(w)[err.argmax()]!r} over {w.size} inputs")
    assert err.max() <= 2e-7


ATAN2_BOUND = 6e-7                   # rad; measured 2.8e-7, times two, one significant digit up


def test_atan2_accuracy(host):
    """rtr_atan2 against np.arctan2 in float64, absolute error in radians, over the 4096 x 4096 lattice of directions
    (x_i, y_j), x_i and y_j the 4096 equally spaced floats of [-1, 1], plus the axes and the diagonals at every power of two and
    at the value set's magnitudes.  Measured worst error: 2.8e-7 rad (4.4e-8 of a turn); asserted: twice that, rounded up to one
    digit, 6e-7 rad.  The error is taken as an angle on the circle: on the cut the function returns +pi by its contract (range
    (-pi, pi]) where np.arctan2 follows the sign of a zero y to -pi.  tests/test_gpu_surfaces.py::_tex_slack leans on this bound."""
    def err(t):
        e = np.abs(run1(host, "atan2", t.view(U32)).astype(np.float64) - np.arctan2(t[:, 0].astype(np.float64), t[:, 1].astype(np.float64)))
        return np.minimum(e, 2 * np.pi - e)
    g = np.linspace(-1.0, 1.0, 4096).astype(F32)
    worst, at = 0.0, None
    for lo in range(0, 4096, 1024):
        y, x = np.meshgrid(g[lo:lo + 1024], g, indexing="ij")
        t = np.stack([y.ravel(), x.ravel()], 1)
        e = err(t)
        if e.max() > worst:
            worst, at = float(e.max()), tuple(t[e.argmax()])
    mags = np.concatenate([np.ldexp(F32(1), np.arange(-149, 128)).astype(F32),
                           np.array([1e-20, 1e-5, 65535.0, 1e20, 3.4028235e38], F32)])
    z = np.zeros_like(mags)
    rows = [(a * sy, b * sx) for a, b in ((mags, z), (z, mags), (mags, mags)) for sy in (1, -1) for sx in (1, -1)]
    t = np.concatenate([np.stack(r, 1) for r in rows]).astype(F32)
    e = err(t)
    if e.max() > worst:
        worst, at = float(e.max()), tuple(t[e.argmax()])
    print(f"rtr_atan2: max |err| = {worst:.3e} rad = {worst / (2 * np.pi):.3e} turn at (y, x) = {at}")
    assert worst <= ATAN2_BOUND
    assert ATAN2_BOUND <= 2 * np.pi * 1e-6          # what the HDRI lookup's slack in tests/test_gpu_surfaces.py assumes


ACOS_BOUND = 7e-7                    # rad; measured 3.5e-7, times two, one significant digit up


def test_acos_accuracy(host):
    """rtr_acos on [-1, 1] against np.arccos in float64: every 255th float of either sign, and all of the 2^20 floats next to 0,
    below 1 and above -1.  Measured worst error: 3.5e-7 rad; asserted 7e-7."""
    one = bits(1.0)
    w = np.concatenate([strided(0, one, 255), strided(0x80000000, 0x80000000 + one, 255)])
    x = f32(w)
    err = np.abs(run1(host, "acos", w).astype(np.float64) - np.arccos(x.astype(np.float64)))
    print(f"rtr_acos: max |err| = {err.max():.3e} rad at x = {x[err.argmax()]!r} over {w.size} inputs")
    assert err.max() <= ACOS_BOUND


ACES_BOUND = 5e-7                    # measured 2.4e-7, times two, one significant digit up


def aces64(x):
    x = x.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.clip((x * (2.51 * x + 0.03)) / (x * (2.43 * x + 0.59) + 0.14), 0.0, 1.0)


def test_aces_accuracy(host):
    """rtr_aces on [0, FLT_MAX] against the clamped rational function in float64 (x^2 stays below DBL_MAX there): every 511th
    float and the first and last 2^20.  Measured worst error: 2.4e-7 (at x = 7.2, where the curve reaches 1); asserted 5e-7.
    Found by this test: beyond x = 1.2e19 the squares overflowed in fp32, inf / inf gave NaN and the clamp turned it into 0 where
    the curve is 1 — an error of 1.0.  rtr_aces now clamps its argument at 1e18 (where the curve has long been 1)."""
    w = strided(0, bits(3.4028235e38), 511)
    err = np.abs(run1(host, "aces", w).astype(np.float64) - aces64(f32(w)))
    print(f"rtr_aces: max |err| = {err.max():.3e} at x = {f32(w)[err.argmax()]!r} over {w.size} inputs")
    assert err.max() <= ACES_BOUND
    assert run1(host, "aces", np.array([bits(np.inf)], U32))[0] == 1.0


def test_srgb_store_is_within_one_code_of_float64(host):
    """rtr_unorm8(rtr_to_srgb(x)) for ALL floats x of [0, 1] against round(255 x^(1/2.2)) in float64 (half to even, as the store
    rounds).  The float64 code is a step function of x; its 255 steps are located by bisection on the float64 formula itself, then
    every float is compared.  More than one code away fails.  Measured: largest distance 1; 447 of the 1 065 353 217 inputs
    land one code away (the fp32 pow is good to ~1e-5 relative, test_math.py: only floats beside a step can move)."""
    def ref(word):
        return int(np.rint(255.0 * np.float64(f32([word])[0]) ** (1.0 / 2.2)))
    one = bits(1.0)
    assert ref(0) == 0 and ref(one) == 255
    first = [0]                                      # first[k]: the first pattern whose float64 code is >= k
    for k in range(1, 256):
        lo, hi = first[-1], one                      # ref(lo) < k <= ref(hi)
        if ref(lo) >= k:
            first.append(lo)
            continue
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if ref(mid) >= k else (mid, hi)
        first.append(hi)
    first.append(one + 1)
    off_by_one, worst = 0, 0
    step = 1 << 24
    for base in range(0, one + 1, step):
        n = min(step, one + 1 - base)
        got = host.eval("srgb_unorm8", np.arange(base, base + n, dtype=np.uint64).astype(U32).reshape(-1, 1))[:, 0].astype(np.int16)
        want = np.empty(n, np.int16)
        for k in range(256):
            a, b = max(first[k], base) - base, min(first[k + 1], base + n) - base
            if a < b:
                want[a:b] = k
        d = np.abs(got - want)
        off_by_one += int((d == 1).sum())
        worst = max(worst, int(d.max()))
    print(f"srgb store: {off_by_one} of {one + 1} inputs one code from the float64 rounding; largest distance {worst}")
    assert worst <= 1


# ---- reference-agnostic properties -----------------------------------------------------------------------------------------------------
def test_quantisation_brackets_the_value_in_exact_arithmetic(host):
    """origin + qlo scale <= v <= origin + qhi scale in exact rationals (fractions.Fraction), wherever the exact quotient lies in
    the grid's range [0, 65535], on the grids and coordinates of the contract lattice (tests/test_gpu_math_contract.py: flat
    scenes, v on a grid plane and one ULP off, both ends).  The quantiser works in double and its comment in rtr_math.h allows a
    slip of 2e-11 grid steps beside a plane; that is the slack asserted.  Measured: no slip at all on this lattice."""
    from test_gpu_math_contract import quant_lattice
    t = quant_lattice(np.random.default_rng(11), 3000)
    lo = host.eval("quant_lo", t)[:, 0]
    hi = host.eval("quant_hi", t)[:, 0]
    slack, slips, checked = Fraction(2, 10 ** 11), 0, 0
    for (v, o, s), ql, qh in zip(f32(t).tolist(), lo.tolist(), hi.tolist()):
        x = (Fraction(v) - Fraction(o)) / Fraction(s)
        if not 0 <= x <= 65535:
            continue
        checked += 1
        assert ql <= x + slack and x - slack <= qh, (v, o, s, ql, qh, float(x))
        assert x - ql < 1 + slack and qh - x < 1 + slack, (v, o, s, ql, qh, float(x))     # and tightly: the nearest planes
        slips += (ql > x) + (qh < x)
    print(f"quantiser: {checked} tuples inside the grid, {slips} exact slips")
    assert checked > 1000


def test_half_planes_are_ordered_along_the_ray(host):
    """slab_oct / slab_wide<0..7> take the entry plane of an axis from the sign of ga alone.  That needs q -> fma(q, ga, gb) to be
    monotone after rounding: for half-float planes p0 <= p1, x0 <= x1 when ga >= 0 and x0 >= x1 when ga < 0.  Every finite half
    value against its successor and against random partners, for path-like and extreme ga, gb."""
    rng = np.random.default_rng(5)
    h = np.concatenate([np.arange(0x0000, 0x7C00), np.arange(0x8000, 0xFC00)]).astype(np.uint16)
    v = h.view(np.float16).astype(F32)
    order = np.argsort(v, kind="stable")
    v = v[order]
    p0 = np.concatenate([v[:-1], v[rng.integers(v.size, size=1 << 18)]])
    p1 = np.concatenate([v[1:], v[rng.integers(v.size, size=1 << 18)]])
    p0, p1 = np.minimum(p0, p1), np.maximum(p0, p1)
    n = p0.size
    ga = np.abs(f32(rng.integers(0, 0x7F800000, n).astype(U32)))
    ga[: n // 2] = rng.uniform(1e-6, 1e3, n // 2).astype(F32)
    gb = f32(rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U32))
    gb[~np.isfinite(gb)] = 0
    gb[: n // 2] = rng.normal(0, 100, n // 2).astype(F32)
    for sign in (1, -1):
        g = (ga * F32(sign)).astype(F32)
        x0 = run1(host, "fma", np.stack([p0, g, gb], 1).view(U32))
        x1 = run1(host, "fma", np.stack([p1, g, gb], 1).view(U32))
        ok = np.isfinite(x0) & np.isfinite(x1)
        assert ok.sum() > n // 2
        assert np.all((x0 <= x1)[ok]) if sign > 0 else np.all((x0 >= x1)[ok])


# ---- the probe can fail ----------------------------------------------------------------------------------------------------------------
def test_the_comparison_sees_one_ulp_and_the_sign_of_zero(host):
    """Two mutants of the table: rtr_atan_small with its last fma written as a multiplication and an addition, and rtr_hwmin as a
    select with its operands exchanged.  Their digests and lattice results must differ from the true ops': by one ULP for the
    first, by the sign of a zero for the second (which only the strict rule sees: rtr_hwmin's own rule takes zeros by value)."""
    first, count = bits(0.25), 1 << 21
    a, m = host.sweep("atan_small", first, count), host.sweep("mut_atan_small", first, count)
    assert a.shape == m.shape == (2,) and np.all(a != m)
    w = np.arange(first, first + count, dtype=U32).reshape(-1, 1)
    ra, rm = host.eval("atan_small", w)[:, 0], host.eval("mut_atan_small", w)[:, 0]
    d = np.abs(ra.astype(np.int64) - rm.astype(np.int64))
    assert d.max() == 1 and 0 < (d == 1).sum() < count          # a one-ULP difference on part of the domain is what the digests saw
    pz, nz = bits(0.0), bits(-0.0)
    t = np.array([[pz, nz], [nz, pz], [bits(1.0), bits(2.0)]], U32)
    rh, rmh = host.eval("hwmin", t), host.eval("mut_hwmin", t)
    assert np.any(P.canon("hwmin", host, rh) != P.canon("hwmin", host, rmh))                    # strict rule: differs
    assert np.all(P.zeros_by_value("hwmin", host, rh) == P.zeros_by_value("hwmin", host, rmh))  # zeros by value: the same


def test_a_mutant_in_the_devices_place_is_reported_with_its_pattern(host):
    """the assertion of the device tests, pointed at a mutant: it fails and names the first differing pattern and both results"""
    from test_gpu_math_contract import assert_sweep_equal
    first = bits(0.25)
    with pytest.raises(AssertionError, match=r"atan_small: first difference at pattern 0x3e8[0-9a-f]{5} .*host 0x[0-9a-f]{8}.*device 0x[0-9a-f]{8}"):
        assert_sweep_equal(host, host, "atan_small", [(first, 1 << 21, 1)], device_op="mut_atan_small")


def test_host_eval_and_sweep_agree(host):
    """the digest of a chunk is the sum of the mixes of what eval returns (the mix restated here); NaN results fold as one pattern"""
    def mix(p, r):
        M = (1 << 64) - 1
        h = ((p + 1) * 0x9E3779B97F4A7C15) & M
        h ^= r
        h = (h * 0xBF58476D1CE4E5B9) & M
        h ^= h >> 29
        h = (h * 0x94D049BB133111EB) & M
        return h ^ (h >> 32)
    for op, first, stride in (("sqrt", bits(-1.0) - 500, 1), ("pcg_hash", 0xFFFFFF00, 3), ("unorm8", bits(0.5), 77)):
        n = 1000
        pat = ((first + np.arange(n, dtype=np.uint64) * stride) & 0xFFFFFFFF).astype(U32)
        out = P.canon(op, host, host.eval(op, pat.reshape(-1, 1)))[:, 0]
        want = sum(mix(int(p), int(r)) for p, r in zip(pat, out)) & ((1 << 64) - 1)
        assert int(host.sweep(op, first, n, stride)[0]) == want, op
    d = host.sweep("log2", 5, (1 << 20) + 7, 9)          # two chunks: a full one and a short one
    assert d.size == 2 and int(d[1]) == int(host.sweep("log2", (5 + 9 * (1 << 20)) & 0xFFFFFFFF, 7, 9)[0])
    with pytest.raises(RuntimeError):
        host.sweep("dot", 0, 10)                         # not a one-word op


def test_both_libraries_hold_the_same_table(host):
    """libmath_probe.so loads without a GPU and lists the same ops, with the same word counts, as the host library"""
    dev = P.device()
    assert dev.names == host.names and len(set(host.names)) == len(host.names)
    assert dev.nin == host.nin and dev.nout == host.nout and dev.fmask == host.fmask
