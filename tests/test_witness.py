"""The oracle against an independent restatement (tests/witness.py: numpy, float64, libm, brute force, nothing shared with
include/rtr_math.h).  The product is held bit-exact to the oracle elsewhere; this is what stands behind the arithmetic both
of them share (parity weak-1).

Tolerances.  fp32 against fp64 cannot be bit-exact.  The first three tests below keep the bounds they were given when the witness
still held the pixel's world position at float64 — the shader holds it in an fp32 variable one unit in front of a camera 800 units
from the origin, which moves a hit 1370 units away by up to 0.02 units and the distance and cosine to the light by 1-3e-4 (what an
earlier version of this text took for ill-conditioning of Moeller-Trumbore): the median pixel within 5e-5 relative, 99 % within the
stated bound, at most 0.5 % beyond ten times it — those are the pixels where a discrete decision (silhouette, shadow edge, alpha
edge, the r1 + r2 > 1 fold) falls on the
other side; RGBA8 bytes equal for >= 98.5 % of the pixels and within +-1 LSB for >= 99.5 %.  Since the witness rounds that position to
fp32 once (witness.render_all) the agreement is two orders closer, and the five-image tests further down hold it there: bounds
measured with that witness, figures beside them."""
import numpy as np
import pytest

from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api, scenes
from witness import Witness


def _compare(oracle, setup, W, H, spp, frame, n, p99_bound):
    images = A.IMAGES_FRAMEBUFFER | A.IMG_BIT(A.IMAGE_HDR)
    p = api.make_params(W, H, spp=spp, images=images)
    ref = oracle.render(setup.desc, setup.camera, setup.scene_info(frame), p, bvh=None, images=images, threads=8)
    idx = np.random.default_rng(7).choice(W * H, n, replace=False)
    ys, xs = idx // W, idx % W
    hdr, rgba = Witness(setup.desc).render(setup.camera, setup.scene_info(frame), p, xs, ys)
    rh = ref.hdr[ys, xs, :3].astype(np.float64)
    rel = (np.abs(hdr - rh) / np.maximum(np.abs(rh), 1e-3)).max(1)
    assert np.median(rel) <= 5e-5, np.median(rel)
    assert np.percentile(rel, 99) <= p99_bound, np.percentile(rel, 99)
    assert (rel > 10 * p99_bound).mean() <= 0.005, (rel > 10 * p99_bound).sum()
    rr = ref.images[A.IMAGE_SHADOWED][ys, xs]
    d = np.stack([np.abs(((rgba >> s) & 255).astype(int) - ((rr >> s) & 255).astype(int)) for s in (0, 8, 16)], 1).max(1)
    assert (d == 0).mean() >= 0.985, (d == 0).mean()
    assert (d <= 1).mean() >= 0.995, (d <= 1).mean()
    assert np.all((rgba >> 24) == 0xff) and np.all((rr >> 24) == 0xff)
    return rel, d


def test_cornell_oracle_vs_independent_float64_witness(oracle, scene_cache):
    s = scenes.cornell_box(256, 256)
    rel, d = _compare(oracle, s, 256, 256, spp=2, frame=3, n=3000, p99_bound=1e-3)
    assert (rel < 1e-5).mean() > 0.3                 # a third of the pixels are sky / light / well-conditioned hits: there fp32 = fp64 to 1e-5


def test_textured_room_oracle_vs_independent_float64_witness(oracle, scene_cache):
    """textures (colour / specular / metallic maps, bilinear + repeat), alpha-tested any-hit, equirect HDRI miss"""
    s = scenes.textured_room(320, 200)
    _compare(oracle, s, 320, 200, spp=2, frame=1, n=3000, p99_bound=1e-2)


def test_witness_catches_a_wrong_constant(oracle, scene_cache):
    """The witness is only worth something if a mistake in the shared arithmetic would show: tone-map the oracle's own HDR radiance
    with a slightly wrong ACES constant (2.51 -> 2.50) and the bytes fall outside the tolerance the tests above accept."""
    s = scenes.cornell_box(128, 128)
    images = A.IMAGES_FRAMEBUFFER | A.IMG_BIT(A.IMAGE_HDR)
    p = api.make_params(128, 128, spp=1, images=images)
    ref = oracle.render(s.desc, s.camera, s.scene_info(0), p, bvh=None, images=images, threads=8)
    x = ref.hdr[..., :3].reshape(-1, 3).astype(np.float64)
    good = Witness.pack(x)
    a = np.clip((x * (2.50 * x + 0.03)) / (x * (2.43 * x + 0.59) + 0.14), 0, 1)
    q = np.rint(np.power(a, 1 / 2.2) * 255.0).astype(np.uint32)
    wrong = q[:, 2] | (q[:, 1] << 8) | (q[:, 0] << 16) | np.uint32(0xff000000)
    rr = ref.images[A.IMAGE_SHADOWED].reshape(-1)
    same = lambda z: (z == rr).mean()       # noqa: E731
    assert same(good) >= 0.985 and same(wrong) < 0.9


# ---- the other four ray-gen images: analytic (LTC), unshadowed, normal, position ---------------------------------------------------
# Measured: CPU oracle against witness.render_all, N = 20000 sampled pixels, spp 2 — `pytest -s tests/test_witness.py -k five_images`
# prints every figure before it asserts.  Per (scene, image): pixels of N whose B,G,R bytes differ, pixels that differ by more than 1 LSB.
# Each share bound is the measurement minus a quarter of its deficit below 1, that is, at most 1.25 x the measured count; where no
# pixel differed the bound is equality.  (The figures are this small since the witness holds pixelWorldPos at fp32 as the shader does,
# see witness.render_all: before that, the Cornell box's analytic image had 0.73 % of its pixels unequal and its position image 0.87 %.)
# The oracle exports HDR radiance for the shadowed image only, so the relative-error quantiles are applied there — bounds 2 x measured:
#   Cornell box    median 9.2e-8 -> 2e-7,   p99 7.3e-7 -> 1.5e-6
#   textured room  median 1.5e-7 -> 3e-7,   p99 3.2e-5 -> 6.5e-5     (shadow and alpha edges)
# with at most 0.5 % of the pixels beyond 10 x the p99 bound; the analytic and unshadowed images are held by their bytes.
N5 = 20000
MEASURED = {
    ("cornell_synthetic", A.IMAGE_ANALYTIC): (1, 0), ("cornell_synthetic", A.IMAGE_SHADOWED): (0, 0),
    ("cornell_synthetic", A.IMAGE_UNSHADOWED): (0, 0),
    ("cornell_shipped", A.IMAGE_ANALYTIC): (0, 0), ("cornell_shipped", A.IMAGE_SHADOWED): (0, 0),
    ("cornell_shipped", A.IMAGE_UNSHADOWED): (0, 0),
    ("room_synthetic", A.IMAGE_ANALYTIC): (4, 0), ("room_synthetic", A.IMAGE_SHADOWED): (15, 9),
    ("room_synthetic", A.IMAGE_UNSHADOWED): (4, 0),
    ("room_shipped", A.IMAGE_ANALYTIC): (6, 0), ("room_shipped", A.IMAGE_SHADOWED): (15, 9),
    ("room_shipped", A.IMAGE_UNSHADOWED): (4, 0),
}
HDR_BOUNDS = {"cornell": (2e-7, 1.5e-6), "room": (3e-7, 6.5e-5)}            # (median, p99) of the shadowed image's relative error
FIVE = (A.IMAGE_ANALYTIC, A.IMAGE_SHADOWED, A.IMAGE_UNSHADOWED, A.IMAGE_NORMAL, A.IMAGE_POSITION)


def _setup(name):
    ltc = scenes.shipped_ltc() if name.endswith("shipped") else scenes.synthetic_ltc()
    if name.startswith("cornell"):
        return scenes.cornell_box(256, 256, ltc=ltc), 256, 256, 3
    return scenes.textured_room(320, 200, ltc=ltc), 320, 200, 1


def _lsb(a, b):
    return np.stack([np.abs(((a >> s) & 255).astype(int) - ((b >> s) & 255).astype(int)) for s in (0, 8, 16)], 1).max(1)


_cache = {}


def _five(oracle, name, witness_cls=Witness):
    """({image: per-pixel largest byte difference}, per-pixel relative error of the shadowed radiance), oracle against witness, over N5
    sampled pixels; no pixel is dropped"""
    s, W, H, frame = _setup(name)
    images = A.IMAGES_RAYGEN5 | A.IMG_BIT(A.IMAGE_HDR)
    p = api.make_params(W, H, spp=2, images=images)
    idx = np.random.default_rng(7).choice(W * H, N5, replace=False)
    ys, xs = idx // W, idx % W
    if name not in _cache:
        ref = oracle.render(s.desc, s.camera, s.scene_info(frame), p, bvh=None, images=images, threads=8)
        _cache[name] = {w: ref.images[w][ys, xs] for w in FIVE}, ref.hdr[ys, xs, :3].astype(np.float64)
    want, rh = _cache[name]
    r = witness_cls(s.desc).render_all(s.camera, s.scene_info(frame), p, xs, ys)
    got = r["rgba8"]
    for w in FIVE:
        assert np.all((got[w] >> 24) == 0xff) and np.all((want[w] >> 24) == 0xff)
    rel = (np.abs(r["hdr"][A.IMAGE_SHADOWED] - rh) / np.maximum(np.abs(rh), 1e-3)).max(1)
    return {w: _lsb(got[w], want[w]) for w in FIVE}, rel


SCENES5 = ("cornell_synthetic", "cornell_shipped", "room_synthetic", "room_shipped")


@pytest.mark.parametrize("name", SCENES5)
def test_five_images_analytic_shadowed_unshadowed(oracle, scene_cache, name):
    d, rel = _five(oracle, name)
    for w in (A.IMAGE_ANALYTIC, A.IMAGE_SHADOWED, A.IMAGE_UNSHADOWED):
        ne, b1 = int((d[w] != 0).sum()), int((d[w] > 1).sum())
        m_ne, m_b1 = MEASURED[(name, w)]
        print(f"{name} image {w}: of {N5} pixels {ne} differ (measured {m_ne}), {b1} by more than 1 LSB (measured {m_b1}), max {d[w].max()}")
        assert ne <= 1.25 * m_ne, (name, w, ne, m_ne)
        assert b1 <= 1.25 * m_b1, (name, w, b1, m_b1)
        assert b1 <= 0.005 * N5
    med, p99 = HDR_BOUNDS[name.split("_")[0]]
    print(f"{name} shadowed radiance: median {np.median(rel):.2e} (bound {med:.1e}), p99 {np.percentile(rel, 99):.2e} (bound {p99:.1e}), "
          f"{(rel > 10 * p99).sum()} pixels beyond 10 x")
    assert np.median(rel) <= med, np.median(rel)
    assert np.percentile(rel, 99) <= p99, np.percentile(rel, 99)
    assert (rel > 10 * p99).mean() <= 0.005, (rel > 10 * p99).sum()


@pytest.mark.parametrize("image", (A.IMAGE_NORMAL, A.IMAGE_POSITION), ids=("normal", "position"))
@pytest.mark.parametrize("name", ("cornell_synthetic", "room_synthetic"))
def test_five_images_normal_and_position(oracle, scene_cache, name, image):
    """An average and a pack: bytes equal, except +-1 LSB on at most 0.5 % of the pixels.  A condition, not a measurement.
    Measured, 20000 pixels: every normal byte equal in both scenes; every position byte equal in the Cornell box, 2 pixels 1 LSB off in
    the textured room.  (With pixelWorldPos held at float64 the position image missed this: Cornell 0.87 % of the pixels, up to 4 LSB —
    the image stores raw world coordinates as UNORM8, 1 LSB = 0.004 units, and the fp32 variable moves the hit by up to 0.02.)"""
    d = _five(oracle, name)[0][image]
    print(f"{name} image {image}: of {N5} pixels {(d != 0).sum()} differ, {(d > 1).sum()} by more than 1 LSB, max {d.max()}")
    assert d.max() <= 1, (name, image, int((d > 1).sum()), int(d.max()))
    assert (d != 0).mean() <= 0.005, (name, image, (d != 0).mean())


# Mutations of the witness's copy of each LTC sub-stage (test_witness_catches_a_wrong_constant's idea): the comparison must leave the
# accepted tolerance, or the witness could not see such a mistake in the shared restatement.
class _NoBias(Witness):
    LUT_BIAS = 0.0                      # table addressing without the half-texel bias


class _SwapT1(Witness):
    SWAP_T1_ZW = True                   # inverse transform with t1.z and t1.w exchanged


class _EdgeConstant(Witness):
    EDGE_A0 = 0.8443985                 # edge integral: 0.8543985 -> 0.8443985


class _NoBehindFlip(Witness):
    FLIP_BEHIND = False                 # sphere look-up without the `behind` sign flip


@pytest.mark.parametrize("mutant", (_NoBias, _SwapT1, _EdgeConstant, _NoBehindFlip), ids=lambda c: c.__name__.strip("_"))
@pytest.mark.parametrize("name", ("cornell_shipped",))
def test_witness_catches_a_mutated_ltc_stage(oracle, scene_cache, name, mutant):
    """Measured, analytic pixels of 20000 that differ on the Cornell box with the shipped tables: witness 0; NoBias 10051,
    SwapT1 9846, EdgeConstant 4703, NoBehindFlip 15043 (the light is one-sided and every lit point is `behind` it, so the sign
    flip is taken at every pixel) — against 0 accepted."""
    allowed = 1.25 * MEASURED[(name, A.IMAGE_ANALYTIC)][0]
    good = int((_five(oracle, name)[0][A.IMAGE_ANALYTIC] != 0).sum())
    bad = int((_five(oracle, name, mutant)[0][A.IMAGE_ANALYTIC] != 0).sum())
    print(f"{mutant.__name__}: analytic pixels of {N5} that differ: witness {good}, mutated {bad}, accepted <= {allowed}")
    assert good <= allowed < bad, f"analytic pixels of {N5} that differ: witness {good}, {mutant.__name__} {bad}, accepted <= {allowed}"
