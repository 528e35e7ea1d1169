"""The CPU oracle's a-trous pass and combine against the float64 witness (tests/post_witness.py: numpy, np.exp, plain division, nothing
shared with include/rtr_math.h) over the made input families of tests/post_cases.py.  The kernels are held to the oracle at 0 differing
pixels and to the same witness in tests/test_gpu_post_edges.py; this module is what shows, without a GPU, that the rule those tests apply
(|byte - unrounded float64 value| <= 0.5 + DELTA, every byte, no share cap) is one the reference side itself keeps, that the witness's
ping-pong protocol is the oracle's, and that each quirk the witness restates is observable.

`python tests/test_post_witness.py` prints the oracle's largest excess per family (the measurement DELTA comes from)."""
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import post_cases
import post_witness as PW

SMALL, MID = (23, 45), (70, 131)                    # (H, W): neither a multiple of the 32 x 8 workgroup
MID_ITERATIONS = tuple(range(9)) + (16, 33, 64)
TINY = ((1, 1), (1, 64), (64, 1), (3, 70))


def _sweep(oracle, family, shape, iterations, seed=0):
    """(largest pass excess, largest combine excess, (iterations at the pass maximum)) of the oracle's chains"""
    H, W = shape
    worst_p, worst_c, at = -1.0, -1.0, None
    states = {}
    for k in iterations:
        stride = max(k, 1) if family in ("checker", "tile") else 1          # these depend on the step under test
        img = post_cases.make(family, H, W, seed, stride=stride)
        for j in (k - 1, k):
            if j >= 0 and (j, stride) not in states:
                states[(j, stride)] = post_cases.oracle_chain(oracle, img, j)
        ep, ec = PW.judge(states[(k, stride)], states.get((k - 1, stride)), img, k)
        if ep is not None and ep > worst_p:
            worst_p, at = ep, k
        worst_c = max(worst_c, ec)
        states = {key: v for key, v in states.items() if key == (k, stride)}
    return worst_p, worst_c, at


@pytest.mark.parametrize("family", post_cases.FAMILIES)
def test_oracle_obeys_the_rounding_rule_at_every_step(oracle, family):
    """every byte of the last pass and of the combine, steps 1...64 on a small image, 0...8, 16, 33, 64 on a larger one, tiny shapes"""
    runs = [(SMALL, range(65)), (MID, MID_ITERATIONS)] + [(s, range(6)) for s in TINY]
    for shape, its in runs:
        ep, ec, at = _sweep(oracle, family, shape, its)
        assert ep <= PW.DELTA, f"{family} {shape}: a-trous excess {ep:.3e} byte at step {at} > DELTA {PW.DELTA:.1e}"
        assert ec <= PW.DELTA, f"{family} {shape}: combine excess {ec:.3e} byte > DELTA {PW.DELTA:.1e}"


def test_protocol_is_the_oracles_buffer_use(oracle):
    """Which pair each pass writes and which pair the combine reads, iterations 0...8, seen from outside: the pair that changed between
    the chains of k - 1 and k passes, and the pair whose combine reproduces the final image (the other pair's does not)."""
    img = post_cases.make("flat_g", 17, 29, seed=3)     # constant G-buffers: the passes do blend (on noise G-buffers only the centre tap weighs)
    prev = None
    for k in range(9):
        st = post_cases.oracle_chain(oracle, img, k)
        passes, reads = PW.protocol(k)
        assert [p[0] for p in passes] == list(range(1, k + 1))
        if k:
            step, src, dst = passes[-1]
            assert src != dst
            for i in PW.PAIR[dst]:
                assert (st[i] != prev[i]).mean() > 0.5, (k, i)
            for i in PW.PAIR[src]:
                assert (st[i] == prev[i]).all(), (k, i)
            assert reads == src                                       # Q8: the combine reads what the last pass read, not what it wrote
        else:
            assert reads == PW.DENOISED
            for i in (1, 2, 3, 4):
                assert (st[i] == img[i]).all()
        other = PW.SAMPLED if reads == PW.DENOISED else PW.DENOISED
        fit = {pair: float(PW.excess(st[5], PW.combine(img[0], st[PW.PAIR[pair][0]], st[PW.PAIR[pair][1]])).max()) for pair in (reads, other)}
        assert fit[reads] <= PW.DELTA and fit[other] > 1.0, (k, fit)
        prev = st


def _good_and_mutated(oracle, family, shape, k, **mutation):
    H, W = shape
    img = post_cases.make(family, H, W, stride=max(k, 1))
    st, before = post_cases.oracle_chain(oracle, img, k), post_cases.oracle_chain(oracle, img, k - 1)
    return PW.judge(st, before, img, k), PW.judge(st, before, img, k, **mutation)


def test_witness_sees_q9(oracle):
    """Mutation: the 5 x 5 weight indexed by the tap's number instead of by the count of in-bounds taps (denoise.comp:72-73 skip :96).
    Measured (flat_g, 23 x 45, step 2): excess -5.5e-5 byte good, 35 byte mutated."""
    (gp, _), (mp, _) = _good_and_mutated(oracle, "flat_g", SMALL, 2, q9=False)
    assert gp <= PW.DELTA and mp > 1.0, f"a-trous excess: witness {gp:.3e}, witness without Q9 {mp:.3e}"


def test_witness_sees_the_normal_distance_divided_by_step_squared(oracle):
    """Mutation: denoise.comp:84 without `/ (step_width * step_width)`; G-buffers whose neighbours are 1 LSB apart, step 3 (an odd step
    lands on the other parity).  Measured: excess -1.4e-5 byte good, 0.165 byte mutated (900 x DELTA: the weights of half the
    taps move by 2.7 %); the assertion asks for 0.1."""
    (gp, _), (mp, _) = _good_and_mutated(oracle, "lsb1", SMALL, 3, normal_by_step2=False)
    assert gp <= PW.DELTA and mp > 0.1, f"a-trous excess: witness {gp:.3e}, witness without the division {mp:.3e}"


@pytest.mark.parametrize("k", [1, 2, 4])
def test_witness_sees_q8(oracle, k):
    """Mutation: the combine reads the pair the last pass wrote.  Measured (flat_g, 23 x 45): excess 2.8e-14 byte good; 250, 144, 26 byte mutated
    for 1, 2, 4 passes (less as the passes converge)."""
    (_, gc), (_, mc) = _good_and_mutated(oracle, "flat_g", SMALL, k, combine_reads_last_written=True)
    assert gc <= PW.DELTA and mc > 1.0, f"combine excess: witness {gc:.3e}, witness reading the written pair {mc:.3e}"


def test_made_inputs_reach_what_rendered_images_do_not():
    """the families are what they claim: alpha bytes other than 255, u = 0 under s > 0, 1-LSB and 255 neighbours, exact combine ties"""
    n = post_cases.make("noise", 9, 33)
    assert all(len(np.unique(n[k] >> 24)) > 100 for k in (0, 1, 2, 6, 7))
    u = post_cases.make("u_zero", 9, 33)
    assert (u[2] == 0).all() and (u[4] == 0).all() and (PW.image_bytes(u[1]) > 0).all() and (PW.image_bytes(u[3]) > 0).all()
    for fam, d in (("lsb1", 1), ("lsb255", 255)):
        g = PW.image_bytes(post_cases.make(fam, 9, 33)[6])[..., 0]
        assert (np.abs(np.diff(g, axis=1)) == d).all() and (np.abs(np.diff(g, axis=0)) == d).all()
    raw = PW.combine(n[0], n[3], n[4])
    assert (np.abs(raw - np.floor(raw) - 0.5) < 1e-9).any()


if __name__ == "__main__":
    from oracle import oracle_py
    oracle_py.lib()
    tp = tc = -1.0
    for fam in post_cases.FAMILIES:
        for shape, its in [(SMALL, range(65)), (MID, MID_ITERATIONS)] + [(s, range(6)) for s in TINY]:
            for seed in (0, 1):
                ep, ec, at = _sweep(oracle_py, fam, shape, its, seed)
                print(f"{fam:8s} {shape[0]:3d} x {shape[1]:3d} seed {seed}: a-trous excess {ep:10.3e} (step {at}), combine {ec:10.3e}", flush=True)
                tp, tc = max(tp, ep), max(tc, ec)
    print(f"largest excess: a-trous {tp:.3e} byte, combine {tc:.3e} byte; DELTA = {PW.DELTA:.1e}")
