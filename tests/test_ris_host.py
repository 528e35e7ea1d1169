"""The resampling rule of include/rtr_ris.h on the host, no GPU: rtr_host_ris_candidates and rtr_host_ris_select
  * draw candidate 0 of every pick where rtr_host_pick_slots_power draws its slot, word for word;
  * equal the independent numpy witness (tests/ris_witness.py) bit for bit for P = 1, 2, 30 and M = 1, 2, 5, 16, with seeds and with
    the pixel rule, with and without wPick;
  * are unbiased: over 200 000 seeds the mean of sum_p w_p F[slot_p] meets sum_t (1 / ns) sum_s F within 5 standard errors for three
    kinds of target, meets sum F wPick / ns with wPick given, and with target = F the variance at M = 16 is below that at M = 1;
  * give RTR_PICK_NONE and 0, never a word that is not finite, for degenerate targets, an empty table and a W that overflows;
  * with M = 1 are the power pick, the weight within 8 * 2^-24 relative: (phat * (total / w)) / phat / P against total / (P * w) is at
    most six binary32 roundings apart (phat in the normal range).
The same two functions run under ASan + UBSan in a stand-alone program, by hand like the other *_host_check programs:
`make -C realtimeraytracer_amd/csrc ris_host_check && realtimeraytracer_amd/csrc/build/ris_host_check`."""
import numpy as np
import pytest

import ris_witness as RW
from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api

NONE = A.PICK_NONE

# five triangles of unequal weight, one of weight 0; ns = 2
WEIGHTS = np.array([1048576, 0, 524288, 200000, 50000], np.uint64)
CDF = np.cumsum(WEIGHTS).astype(np.uint64)
TRIS, NS = 5, 2
# F per slot: positive, some zeros; 0 on the triangle of weight 0, which emits nothing and is in no sum
F = np.array([3.0, 0.5, 0.0, 0.0, 0.0, 7.25, 1.5, 0.125, 20.0, 0.0], np.float32)
NOISE = np.array([0.3, 2.0, 1.0, 1.0, 5.0, 0.7, 1.9, 0.2, 0.5, 3.0], np.float32)      # a fixed positive factor per slot
W_PICK = np.array([1.0, 0.25, 0.5, 0.5, 0.9, 0.05, 0.6, 1.0, 0.35, 0.75], np.float32)   # in (0, 1] per slot


def _params(frame=3, width=37, spp=2):
    return api.make_light_params(1, NS, frame, width, spp)


def _seeds(n, seed=11):
    return np.random.default_rng(seed).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("explicit", [False, True])
@pytest.mark.parametrize("P", [1, 2, 30])
def test_candidate_0_is_the_power_picks_slot(P, explicit):
    n, lp, pick = 3000, _params(), api.make_pick_params(P, 2)
    sd = _seeds(n) if explicit else None
    cand = api.host_ris_candidates(CDF, TRIS, sd, n, lp, pick, 5)
    slots, _ = api.host_pick_slots_power(CDF, TRIS, sd, n, lp, pick)
    assert cand.shape == (n, P, 5) and (cand[:, :, 0] == slots).all()
    assert (cand < TRIS * NS).all() and (WEIGHTS[cand // NS] != 0).all()      # a triangle of weight 0 is never drawn
    assert len(np.unique(cand[:, :, 1:])) == 8 and (cand[:, :, 1] != cand[:, :, 2]).any()


@pytest.mark.parametrize("explicit", [False, True])
@pytest.mark.parametrize("M", [1, 2, 5, 16])
@pytest.mark.parametrize("P", [1, 2, 30])
def test_both_host_forms_equal_the_witness_bit_for_bit(P, M, explicit):
    n, depth = 700, 3
    lp, pick = _params(), api.make_pick_params(P, depth)
    sd = _seeds(n, 5 + P) if explicit else None
    bf = RW.base_frame(sd, n, lp.frame, lp.width, lp.spp)
    cand = api.host_ris_candidates(CDF, TRIS, sd, n, lp, pick, M)
    assert (cand == RW.candidates(CDF, TRIS, bf, depth, NS, P, M)).all()
    rng = np.random.default_rng(P * 100 + M)
    targets = (F[cand] * rng.uniform(0.1, 4.0, cand.shape)).astype(np.float32)
    odd = rng.integers(0, 12, cand.shape)
    for k, v in enumerate((np.nan, np.inf, -1.0, 1e-42, 3e38)):               # what counts as 0, a denormal, and what overflows W
        targets[odd == k] = v
    cand[odd == 11] = NONE
    for mis in (False, True):
        wp = (W_PICK[np.minimum(cand, 9)] * rng.uniform(0.5, 1.0, cand.shape)).astype(np.float32) if mis else None
        ris = api.make_ris_params(M, mis, 3 if mis else 0)
        slots, weights = api.host_ris_select(CDF, TRIS, sd, n, lp, pick, ris, cand, targets, wp)
        ws, ww = RW.select(CDF, TRIS, bf, depth, NS, P, M, cand, targets, wp)
        assert (slots == ws).all()
        assert (weights.view(np.uint32) == ww.view(np.uint32)).all()
        assert np.isfinite(weights).all() and (weights[slots == NONE] == 0).all() and (slots != NONE).any() and (M > 2 or (slots == NONE).any())


N_SEEDS = 200_000


@pytest.fixture(scope="module")
def drawn():
    """the candidates of N_SEEDS hits for P = 1, 2 and M = 16 (the candidates of a smaller M are the first M of these), drawn once"""
    sd, lp = _seeds(N_SEEDS, 2024), _params(frame=9)
    return sd, lp, {P: api.host_ris_candidates(CDF, TRIS, sd, N_SEEDS, lp, api.make_pick_params(P, 1), 16) for P in (1, 2)}


def _estimate(drawn, P, M, targets_of_slot, w_pick_of_slot=None):
    sd, lp, cands = drawn
    cand = np.ascontiguousarray(cands[P][:, :, :M])
    mis = w_pick_of_slot is not None
    tg = targets_of_slot[cand] * (w_pick_of_slot[cand] if mis else np.float32(1))
    slots, weights = api.host_ris_select(CDF, TRIS, sd, N_SEEDS, lp, api.make_pick_params(P, 1), api.make_ris_params(M, mis, 3 if mis else 0), cand, tg,
                                         w_pick_of_slot[cand] if mis else None)
    f = np.where(slots == NONE, 0.0, F[np.minimum(slots, 9)].astype(np.float64))
    return (weights.astype(np.float64) * f).sum(axis=1)


@pytest.mark.parametrize("M", [1, 2, 4, 16])
@pytest.mark.parametrize("P", [1, 2])
def test_the_estimator_is_unbiased(drawn, P, M):
    want = float(F.astype(np.float64).sum()) / NS
    for name, tg in (("F", F), ("F x noise", F * NOISE), ("constant", np.ones(10, np.float32))):
        est = _estimate(drawn, P, M, tg)
        se = est.std(ddof=1) / np.sqrt(N_SEEDS)
        print(f"P {P} M {M} target {name}: mean {est.mean():.5f} +- {se:.5f}, want {want:.5f} ({(est.mean() - want) / max(se, 1e-300):+.2f} se)")
        assert abs(est.mean() - want) <= 5 * se, name
    want = float((F.astype(np.float64) * W_PICK).sum()) / NS
    est = _estimate(drawn, P, M, F, W_PICK)
    se = est.std(ddof=1) / np.sqrt(N_SEEDS)
    print(f"P {P} M {M} with wPick: mean {est.mean():.5f} +- {se:.5f}, want {want:.5f}")
    assert abs(est.mean() - want) <= 5 * se


@pytest.mark.parametrize("P", [1, 2])
def test_resampling_on_the_contribution_lowers_the_variance(drawn, P):
    v1, v16 = _estimate(drawn, P, 1, F).var(ddof=1), _estimate(drawn, P, 16, F).var(ddof=1)
    print(f"P {P}: variance at M = 1 {v1:.5f}, at M = 16 {v16:.5f}")
    assert v16 < v1


def test_degenerate_inputs_give_no_pick_and_never_a_word_that_is_not_finite():
    n, P, M = 500, 2, 5
    lp, pick, ris = _params(), api.make_pick_params(P), api.make_ris_params(M)
    cand = api.host_ris_candidates(CDF, TRIS, None, n, lp, pick, M)
    for v in (0.0, np.nan, np.inf, -np.inf, -2.0):
        slots, weights = api.host_ris_select(CDF, TRIS, None, n, lp, pick, ris, cand, np.full(cand.shape, v, np.float32))
        assert (slots == NONE).all() and (weights.view(np.uint32) == 0).all(), v
    # W overflows: every target near the largest float
    slots, weights = api.host_ris_select(CDF, TRIS, None, n, lp, pick, ris, cand, np.full(cand.shape, 3e38, np.float32))
    assert (slots == NONE).all() and (weights.view(np.uint32) == 0).all()
    # total == 0: an empty table, and a table none of whose triangles emits
    zero = np.zeros(TRIS, np.uint64)
    for cdf, tris in ((zero, TRIS), (zero, 0)):
        c0 = api.host_ris_candidates(cdf, tris, None, n, lp, pick, M)
        assert (c0 == NONE).all()
        slots, weights = api.host_ris_select(cdf, tris, None, n, lp, pick, ris, cand, np.ones(cand.shape, np.float32))
        assert (slots == NONE).all() and (weights.view(np.uint32) == 0).all()
    # a mixture: whatever is held, the words are finite
    rng = np.random.default_rng(3)
    tg = rng.choice(np.array([0.0, np.nan, np.inf, -1.0, 1e-45, 1e-30, 1.0, 1e30, 3e38], np.float32), cand.shape)
    for mis in (False, True):
        wp = rng.choice(np.array([np.nan, np.inf, 0.0, -0.5, 1e-45, 0.5, 1.0], np.float32), cand.shape) if mis else None
        slots, weights = api.host_ris_select(CDF, TRIS, None, n, lp, pick, api.make_ris_params(M, mis, 3 if mis else 0), cand, tg, wp)
        assert np.isfinite(weights).all() and (weights >= 0).all() and (weights[slots == NONE] == 0).all()
        assert ((slots == NONE) | (slots < TRIS * NS)).all() and (slots != NONE).any()


@pytest.mark.parametrize("P", [1, 2, 30])
def test_one_candidate_is_the_power_pick(P):
    n = 4000
    lp, pick = _params(), api.make_pick_params(P, 4)
    sd = _seeds(n, 77)
    cand = api.host_ris_candidates(CDF, TRIS, sd, n, lp, pick, 1)
    tg = (F[cand] * np.random.default_rng(1).uniform(0.01, 100.0, cand.shape)).astype(np.float32)
    slots, weights = api.host_ris_select(CDF, TRIS, sd, n, lp, pick, api.make_ris_params(1), cand, tg)
    ps, pw = api.host_pick_slots_power(CDF, TRIS, sd, n, lp, pick)
    pos = tg[:, :, 0] > 0
    assert pos.any() and (~pos).any()
    assert (slots[pos] == ps[pos]).all() and (slots[~pos] == NONE).all() and (weights[~pos] == 0).all()
    rel = np.abs(weights[pos].astype(np.float64) - pw[pos]) / pw[pos]
    print(f"P {P}: largest relative difference of the weights {rel.max():.3e} (bound {8 * 2.0 ** -24:.3e})")
    assert rel.max() <= 8 * 2.0 ** -24
