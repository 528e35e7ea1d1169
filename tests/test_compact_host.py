"""rtr_host_compact_paths, the host compile of include/rtr_paths.h in a plain loop, against the numpy witness (tests/compact_witness.py):
every output word, the tail included; the roulette's edge cases; and that the roulette keeps the estimator's mean.  No GPU: what the
kernels are then held to (tests/test_gpu_compact.py) is this function."""
import numpy as np
import pytest

import bounce_witness as BW
import compact_witness as W
from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api

F32 = np.float32
OK_RAY = np.array([1, 2, 3, 0.001, 0, 0.6, 0.8, 10000], F32)


def assert_host_is_witness(rays, thr, seeds, ids, params, what):
    got = api.host_compact_paths(rays, thr, seeds, ids, params)
    r, t, s, i, count = W.compact(rays, thr, seeds, ids, params.frame, params.depth, params.flags, params.survivalFloor)
    assert got.count == count, f"{what}: {got.count} survivors, the witness has {count}"
    assert (got.rays.view(np.uint32) == r).all(), f"{what}: rays"
    assert (got.throughput.view(np.uint32) == t).all(), f"{what}: throughput"
    assert (got.path_ids.view(np.uint32) == i).all(), f"{what}: path ids"
    assert (got.seeds is None) == (s is None) and (s is None or (got.seeds.view(np.uint32) == s).all()), f"{what}: seeds"
    return got


@pytest.mark.parametrize("pattern", W.PATTERNS)
def test_host_equals_witness(pattern):
    for n in W.SIZES:
        for stride_words, with_ids, with_seeds in ((3, True, True), (8, False, True), (3, False, False), (8, True, False)):
            rays, thr, seeds, ids, mask = W.make_paths(n, pattern, stride_words=stride_words)
            got = assert_host_is_witness(rays, thr, seeds if with_seeds else None, ids if with_ids else None, api.make_compact_params(frame=3, depth=1),
                                         f"{pattern}, {n} paths, stride {4 * stride_words}")
            # the pattern is what was asked for, the order is stable and the tail is cleared
            assert got.count == int(mask.sum())
            want = ids[mask] if with_ids else np.flatnonzero(mask).astype(np.uint32)
            assert (got.path_ids.view(np.uint32)[:got.count] == want).all() and (got.path_ids.view(np.uint32)[got.count:] == A.PATH_NONE).all()
            assert not got.rays.view(np.uint32)[got.count:].any() and not got.throughput.view(np.uint32)[got.count:].any()
        # the roulette over the same paths, throughputs in (0, 2): some draw, some are above 1
        rays, thr, seeds, ids, mask = W.make_paths(n, pattern, t_hi=2.0)
        got = assert_host_is_witness(rays, thr, seeds, ids, api.make_compact_params(frame=5, depth=2, roulette=True, survival_floor=0.1), f"{pattern}, {n} paths, roulette")
        assert got.count <= int(mask.sum())
        if n == 20000 and pattern in ("all_live", "alternating", "random_half"):
            assert 0 < got.count < int(mask.sum())


def test_every_dead_cause_is_dead_and_the_oddities_live():
    causes, odd = W.dead_causes(), W.live_oddities()
    for k, (name, ray, T) in enumerate(causes + odd):
        rays = np.stack([OK_RAY, ray, OK_RAY])
        thr = np.stack([np.ones(3, F32), T, np.ones(3, F32)])
        got = assert_host_is_witness(rays, thr, None, None, api.make_compact_params(), name)
        assert got.count == (2 if k < len(causes) else 3), name
    got = api.host_compact_paths(OK_RAY[None], np.array([[-0.0, 0.0, 1.0]], F32))
    assert got.count == 1 and got.throughput.view(np.uint32).tolist() == [[0x80000000, 0, 0x3f800000]]


def test_roulette_edge_cases():
    frame, depth = 4, 2
    seed_one = np.array([(BW.SEED_U1_IS_ONE - frame - 7919 * (depth + 1) - 300) & 0xffffffff], np.uint32)
    assert W.uniform(W.roulette_seed(seed_one, frame, depth))[0] == 1.0
    p = api.make_compact_params(frame=frame, depth=depth, roulette=True, survival_floor=0.05)
    # p >= 1: no number is drawn and T comes back bit for bit, also for the seed whose number is exactly 1.0
    for T in ([1.0, 0.5, 0.25], [3.5, 0.0, -0.0], [np.nextafter(F32(1), F32(2)), 1e-30, 0.1]):
        thr = np.array([T], F32)
        got = assert_host_is_witness(OK_RAY[None], thr, seed_one, None, p, f"T = {T}")
        assert got.count == 1 and (got.throughput.view(np.uint32) == thr.view(np.uint32)).all()
    # the same seed with p < 1 dies, whatever p
    for m in (np.nextafter(F32(1), F32(0)), 0.5, 0.001):
        got = assert_host_is_witness(OK_RAY[None], np.array([[m, 0.0, 0.0]], F32), seed_one, None, p, f"u = 1, p = {m}")
        assert got.count == 0
    # and lives without the flag
    assert api.host_compact_paths(OK_RAY[None], np.array([[0.5, 0, 0]], F32), seed_one, None, api.make_compact_params(frame=frame, depth=depth)).count == 1
    # the floor lifts p: T = 0.01 with floor 0.1 survives for u < 0.1 with T / 0.1
    seeds = np.arange(4000, dtype=np.uint32)
    u = W.uniform(W.roulette_seed(seeds, 0, 0))
    thr = np.full((4000, 3), 0.01, F32)
    got = assert_host_is_witness(np.repeat(OK_RAY[None], 4000, 0), thr, seeds, None, api.make_compact_params(roulette=True, survival_floor=0.1), "floor")
    assert got.count == int((u < F32(0.1)).sum()) and 300 < got.count < 500
    assert (got.throughput[:got.count].view(np.uint32) == (F32(0.01) / F32(0.1)).view(np.uint32)).all()
    # a floor of 1 switches the roulette off
    got = api.host_compact_paths(np.repeat(OK_RAY[None], 4000, 0), thr, seeds, None, api.make_compact_params(roulette=True, survival_floor=1.0))
    assert got.count == 4000 and (got.throughput.view(np.uint32) == thr.view(np.uint32)).all()


@pytest.mark.parametrize("frame,depth", [(0, 0), (9, 2), (3, 5)])
def test_the_roulette_keeps_the_mean(frame, depth):
    """the surviving share is p within 5 standard errors sqrt(p (1 - p) / n), and every survivor carries T / p: E[outT] = T.  (These
    inputs against the generator on the CPU: the largest deviation was 1.8 standard errors.)"""
    n = 200000
    rays = np.repeat(OK_RAY[None], n, 0)
    seed_sets = {"consecutive": np.arange(n, dtype=np.uint32) + np.uint32(12345),
                 "random": np.random.default_rng(17).integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)}
    for name, seeds in seed_sets.items():
        for p in (0.05, 0.1, 0.25, 0.5, 0.8):
            T = (F32(p) * np.array([1.0, 0.5, 0.25], F32)).astype(F32)
            thr = np.repeat(T[None], n, 0)
            got = api.host_compact_paths(rays, thr, seeds, None, api.make_compact_params(frame=frame, depth=depth, roulette=True, survival_floor=0.01))
            se = np.sqrt(p * (1 - p) / n)
            dev = (got.count / n - p) / se
            print(f"frame {frame} depth {depth} {name} seeds p = {p}: {got.count} survive, {dev:+.2f} standard errors")
            assert abs(dev) <= 5.0, f"{name} seeds, p = {p}: the surviving share {got.count / n} is {dev:+.2f} standard errors from p"
            want = (T / T[0]).astype(F32)            # T / p with p = max3(T) = T[0], in float32
            assert (got.throughput[:got.count].view(np.uint32) == want.view(np.uint32)).all()
            assert not got.throughput[got.count:].any()
            # who survived: exactly the seeds whose number is below p
            u = W.uniform(W.roulette_seed(seeds, frame, depth))
            assert (got.path_ids.view(np.uint32)[:got.count] == np.flatnonzero(u < T[0]).astype(np.uint32)).all()
