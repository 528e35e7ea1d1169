"""The numerical contract (include/rtr_math.h), exercised through the oracle's exported helpers:
known-answer tests that are implementation independent + accuracy pins vs libm.
The rest of the contract's pins: tests/test_math_contract.py (every function of the header against float64 references, host compile)
and tests/test_gpu_math_contract.py (the device compile equals the host compile, bit for bit, over whole domains)."""
import ctypes as C

import numpy as np

from realtimeraytracer_amd import _abi as A

# PCG random(seed) (reference src/shaders/raycommon.glsl:22-27): hash, then fp32 value
PCG_KAT = [(0, 0x07BB2FE2, 0.030199997), (1, 0xA8BEEA3C, 0.6591631), (2, 0x7A7ECC88, 0.4784973), (100, 0x3729B868, 0.21548036),
           (322, 0x3AB991B4, 0.22939406), (733, 0xD552B6EF, 0.8332934), (1933, 0x84A81685, 0.51818985),
           (3492334, 0x7EBFE89D, 0.4951158), (0xFFFFFFFF, 0xE62A4902, 0.8990827)]


def test_pcg_known_answers(oracle):
    L = oracle.lib()
    for seed, h, f in PCG_KAT:
        assert L.oracle_pcg_hash(seed) == h
        assert np.float32(L.oracle_random(seed)) == np.float32(np.float32(h) / np.float32(4294967296.0))
        assert abs(L.oracle_random(seed) - f) < 5e-8


def test_random_can_return_one(oracle):
    # quirk Q2: float(hash)/2^32 rounds to exactly 1.0 for hash >= 0xFFFFFF80 — find nothing special, just the formula
    assert np.float32(0xFFFFFF80) / np.float32(4294967296.0) == np.float32(1.0)


def _ulp_diff(a, b):
    ia = np.frombuffer(np.float32(a).tobytes(), np.int32)[0]
    ib = np.frombuffer(np.float32(b).tobytes(), np.int32)[0]
    return abs(int(ia) - int(ib))


def test_pow_log_exp_accuracy(oracle):
    """own pow/exp2/log2 vs float64 libm.  Stated tolerance: pow = exp2(y*log2(x)) carries the fp32 rounding of
    y*log2(x), so its relative error grows with |log2 x|: <= 1e-5 relative on x in [1e-6, 50] (the path uses
    x in [0,1] and feeds an 8-bit quantiser, 1/255 = 3.9e-3); log2 <= 2e-6 relative; exp2 <= 3 ULP."""
    L = oracle.lib()
    rng = np.random.default_rng(7)
    worst = 0.0
    for x in np.concatenate([rng.uniform(1e-6, 1.0, 4000), rng.uniform(1.0, 50.0, 500), [1.0, 0.5, 0.25, 1e-30, 3.0e38]]).astype(np.float32):
        for y in (np.float32(2.2), np.float32(0.45454545454545453), np.float32(5.0)):
            ref = np.float32(np.float64(x) ** np.float64(y)) if np.float64(x) ** np.float64(y) < 3.4e38 else None
            if ref is None or ref < 1.2e-38:
                continue
            worst = max(worst, abs(L.oracle_pow(float(x), float(y)) - float(ref)) / float(ref))
    assert worst <= 1e-5, f"pow relative error {worst}"
    for x in rng.uniform(1e-30, 1e30, 2000).astype(np.float32):
        ref = np.float32(np.log2(np.float64(x)))
        assert abs(L.oracle_log2(float(x)) - ref) <= 2e-6 * max(1.0, abs(ref))
    for z in rng.uniform(-120, 120, 2000).astype(np.float32):
        assert _ulp_diff(L.oracle_exp2(float(z)), np.float32(2.0 ** np.float64(z))) <= 3


def test_pow_edge_cases(oracle):
    L = oracle.lib()
    assert L.oracle_pow(0.0, 2.2) == 0.0
    assert L.oracle_pow(-1.0, 2.2) == 0.0          # documented divergence: GLSL pow(x<0) is undefined
    assert L.oracle_pow(float("nan"), 2.2) == 0.0
    assert L.oracle_pow(1.0, 2.2) == 1.0 and L.oracle_pow(1.0, 0.45454545454545453) == 1.0
    assert L.oracle_exp2(-200.0) == 0.0


def test_unorm8_pack(oracle):
    L = oracle.lib()
    assert L.oracle_pack_bgra8(1.0, 0.0, 0.0) == 0xFFFF0000          # bytes B,G,R,A = 00,00,FF,FF
    assert L.oracle_pack_bgra8(0.0, 0.0, 1.0) == 0xFF0000FF
    assert L.oracle_pack_bgra8(2.0, -1.0, float("nan")) == 0xFFFF0000  # clamp; NaN -> 0
    assert L.oracle_pack_bgra8(0.5, 0.5, 0.5) == 0xFF808080          # 127.5 rounds to even = 128


def test_unorm8_unpack_without_division_is_exact(oracle):
    """The denoise kernels unpack UNORM8 as fma(b, head, b * tail) with fl(1/255) split in two (rtr_unorm8_to_float); the oracle
    divides.  Both must agree for every byte."""
    import numpy as np
    L = oracle.lib()
    for b in range(256):
        assert np.float32(L.oracle_unorm8_to_float_fast(b)) == np.float32(b) / np.float32(255.0), b


def test_division_by_a_known_divisor_is_the_ieee_quotient(oracle):
    """rtr_div_by (a * fl(1/b) corrected twice by its exact remainder: what the denoise kernel issues instead of the division
    sequence) against a / b for EVERY float a of either sign with 2^-40 <= |a| <= 16 — the squared distances of UNORM8 vectors and
    their quotients lie inside — for the divisors the pass uses: the phis and EVERY step^2 the API can issue, (i + 1)^2 for i < 64
    (rtr_denoise_combine accepts iterations <= 64), and a few others; and at zero."""
    import numpy as np
    from concurrent.futures import ThreadPoolExecutor
    L = oracle.lib()

    def bits(x):
        return int(np.float32(x).view(np.uint32))
    # the smallest non-zero squared UNORM8 distance over the largest divisor stays above the range's lower end, the largest below its top
    assert np.float32(1.0 / 255.0) ** 2 / np.float32(64 ** 2) > np.float32(2.0 ** -40)
    assert 4 * np.float32(1.0) ** 2 <= 16.0                 # four channels, each at most 1 apart
    divisors = [0.001, 0.37] + [float((i + 1) ** 2) for i in range(64)]

    def bad(b):
        return L.oracle_div_by_mismatches(b, bits(2.0 ** -40), bits(16.0)) + L.oracle_div_by_mismatches(b, 0, 0)
    with ThreadPoolExecutor(8) as pool:                     # ctypes releases the GIL: 66 sweeps of 2 x 3.7e8 floats
        for b, n in zip(divisors, pool.map(bad, divisors)):
            assert n == 0, (b, n)


def test_moeller_trumbore_edge_cases(oracle):
    """intersect.rint:18-41 semantics: EPSILON rejection, u/v/u+v rejections, t > tmin, no back-face culling."""
    L = oracle.lib()
    F3 = A.f32 * 3
    v0, e1, e2 = F3(0, 0, 0), F3(1, 0, 0), F3(0, 1, 0)
    tuv = F3()

    def mt(o, d, tmin=0.001):
        return L.oracle_mt(F3(*o), F3(*d), v0, e1, e2, tmin, tuv), tuple(tuv)
    hit, (t, u, v) = mt((0.25, 0.25, 1.0), (0, 0, -1))
    assert hit and t == 1.0 and u == 0.25 and v == 0.25
    assert mt((0.25, 0.25, -1.0), (0, 0, 1))[0] == 1              # back face still hits (cull disabled, tlas.cppm:67)
    assert mt((0.25, 0.25, 1.0), (1, 0, 0))[0] == 0               # parallel: |a| < EPSILON
    assert mt((0.25, 0.25, -1.0), (0, 0, -1))[0] == 0             # behind the origin: t <= tmin
    assert mt((0.25, 0.25, 0.0005), (0, 0, -1))[0] == 0           # t = 0.0005 <= 0.001
    assert mt((0.0, 0.5, 1.0), (0, 0, -1))[0] == 1                # on the u = 0 edge
    assert mt((0.5, 0.5, 1.0), (0, 0, -1))[0] == 1                # on the u+v = 1 edge
    assert mt((0.51, 0.5, 1.0), (0, 0, -1))[0] == 0               # just outside
    assert mt((-0.01, 0.5, 1.0), (0, 0, -1))[0] == 0
