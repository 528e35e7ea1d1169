"""GGX_PartialGeometryTerm (kernels/rtr_device.h) no longer forms chi = chiGGX(VoH2 / clamp(dot(v, n), 0.001, 1)): with
VoH2 = clamp(dot(v, h), 0.001, 1) and rtr_clamp in select form, the quotient is positive for every input, so chi is 1.0f and
chi * 2.0f is 2.0f.  This file walks the argument's corners in float32 (numpy), with the select-form clamp of include/rtr_math.h
restated: NaN and infinite dot products, the interval's ends and their neighbours, and the quotient's extremes."""
import numpy as np

F = np.float32
LO, HI = F(0.001), F(1.0)


def clamp(x):
    """rtr_clamp(x, 0.001f, 1.0f) = rtr_min(rtr_max(x, lo), hi) with rtr_max(a, b) = a > b ? a : b and rtr_min(a, b) = a < b ? a : b"""
    x = np.asarray(x, F)
    m = np.where(x > LO, x, LO).astype(F)
    return np.where(m < HI, m, HI).astype(F)


def chi(x):
    return np.where(np.asarray(x, F) > F(0.0), F(1.0), F(0.0)).astype(F)


def corners():
    tiny = np.array([1.0e-45, 1.17549435e-38, 1.0e-30, 1.0e-6], F)
    around = []
    for c in (LO, HI, F(0.5), F(0.0)):
        around += [c, np.nextafter(c, F(-np.inf)), np.nextafter(c, F(np.inf))]
    special = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 3.0e38, -3.0e38], F)
    return np.concatenate([tiny, -tiny, np.array(around, F), special, np.linspace(-2.0, 2.0, 4001, dtype=F)])


def test_select_form_clamp_sends_nan_to_the_lower_bound():
    got = clamp(np.array([np.nan, -np.nan, -np.inf, np.inf, 0.0, -0.0, 0.001, 1.0, 2.0, 0.5], F))
    assert got.tolist() == [LO, LO, LO, HI, LO, LO, LO, HI, HI, F(0.5)]
    c = clamp(corners())
    assert not np.isnan(c).any() and (c >= LO).all() and (c <= HI).all()


def test_the_quotients_extremes_are_positive_and_finite():
    assert F(LO / HI) == LO and F(LO / HI) > 0                       # 0.001f / 1.0f: the smallest quotient, far above the denormals
    big = F(HI / LO)
    assert np.isfinite(big) and abs(float(big) - 1000.0) < 1e-3      # 1.0f / 0.001f: the largest
    assert F(LO / LO) == F(1.0) and F(HI / HI) == F(1.0)


def test_chi_is_one_for_every_pair_of_dot_products():
    x = corners()
    num, den = np.meshgrid(clamp(x), clamp(x), indexing="ij")
    with np.errstate(all="raise"):                                   # no overflow, underflow, invalid or division by zero on the way
        q = (num / den).astype(F)
    assert np.isfinite(q).all() and (q >= LO).all() and (q <= F(1000.0) * (F(1.0) + F(2.0) ** -22)).all()
    c = chi(q)
    assert (c == F(1.0)).all()
    assert ((c * F(2.0)).view(np.uint32) == F(2.0).view(np.uint32)).all()      # what the kernel now writes in its place
