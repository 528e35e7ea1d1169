"""rtr_host_pick_slots, the host compile of include/rtr_pick.h in a plain loop: every slot is below A, the clamp at u == 1.0, the words
against a numpy restatement of the rule, and that the drawn slots are uniform and two picks of one hit uncorrelated.  No GPU: what the
kernel's slots are then held to (tests/test_gpu_light_pick.py) is this function."""
import ctypes as C

import numpy as np
import pytest

import bounce_witness as BW
from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api

INVALID = -1
U32 = np.uint32


def restated_slots(base, frame, depth, picks, area):
    """the rule in numpy: u = rtr_random(b + frame + 7919 * (depth + 1) + 400 + 100 * p) in 32-bit words, j = (uint32)(u * (float)A)
    clamped to A - 1, RTR_PICK_NONE for A == 0 -> uint32 (n, picks)"""
    base = np.asarray(base).astype(np.uint64)
    out = np.empty((len(base), picks), U32)
    for p in range(picks):
        seed = (base + frame + 7919 * (depth + 1) + 400 + 100 * p) & 0xffffffff
        u = BW.pcg_hash(seed).astype(np.float32) * np.float32(2.3283064365386963e-10)
        if area == 0:
            out[:, p] = 0xffffffff
        else:
            j = (u * np.float32(area)).astype(np.uint64)          # a float32 product, truncated
            out[:, p] = np.minimum(j, area - 1).astype(U32)
    return out


def _seed_sets(n):
    return {"consecutive": np.arange(n, dtype=U32) + U32(12345),
            "random": np.random.default_rng(23).integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(U32)}


@pytest.mark.parametrize("area", [1, 2, 6, 13, 1000, 1 << 24])
def test_every_slot_is_below_the_area_and_equals_the_restatement(area):
    n = 20000
    for name, seeds in _seed_sets(n).items():
        for frame, depth, picks in ((0, 0, 1), (7, 2, 2), (0xfffffff0, 5, A.PICK_MAX)):
            p = api.make_light_params(1, 3, frame=frame, width=16)
            got = api.host_pick_slots(seeds, n, p, api.make_pick_params(picks, depth), area)
            assert got.shape == (n, picks) and got.dtype == U32
            assert (got < area).all(), f"{name} seeds, A = {area}: a slot is not below A"
            assert (got == restated_slots(seeds, frame, depth, picks, area)).all(), f"{name} seeds, A = {area}, frame {frame}, depth {depth}"
    if area == 1 << 24:                  # the far end is reached: with 20 000 x 30 numbers some land in the last 1/64 of the slots
        assert got.max() > area - area // 64


def test_pixel_seeds_are_light_rays_rule():
    w, spp, n = 37, 2, 5000
    p = api.make_light_params(1, 3, frame=3, width=w, spp=spp)
    got = api.host_pick_slots(None, n, p, api.make_pick_params(3, 1), 13)
    assert (got == restated_slots(BW.pixel_seeds(n, w, spp), 3, 1, 3, 13)).all()
    # and the same hits with those seeds handed in
    assert (got == api.host_pick_slots(BW.pixel_seeds(n, w, spp), n, p, api.make_pick_params(3, 1), 13)).all()


def test_no_area_gives_pick_none_and_too_much_area_is_refused():
    lib = A.hip_lib()
    p = api.make_light_params(0, 3, width=8)
    got = api.host_pick_slots(None, 100, p, api.make_pick_params(2), 0)
    assert (got == A.PICK_NONE).all() and A.PICK_NONE == 0xffffffff
    api.host_pick_slots(None, 4, p, api.make_pick_params(1), A.PICK_MAX_SLOTS)          # 2^24 itself is allowed
    out = np.full(8, 0xA5A5A5A5, U32)
    pick = api.make_pick_params(1)
    assert lib.rtr_host_pick_slots(None, 4, 0, 8, 1, C.byref(pick), A.PICK_MAX_SLOTS + 1, out.ctypes.data_as(A.VP)) == INVALID
    msg = lib.rtr_last_error().decode()
    assert msg.startswith("rtr_host_pick_slots: ") and "16777217 area slots" in msg and "2^24" in msg
    assert (out == 0xA5A5A5A5).all()     # nothing was written


def test_the_clamp_at_u_equal_one():
    """rtr_random returns exactly 1.0 for 128 of the 2^32 seeds (quirk Q2); bounce_witness knows one.  u * A == A there: the slot is
    clamped to A - 1, for every A"""
    frame, depth = 4, 2
    for p in (0, 1, 5):
        base = (BW.SEED_U1_IS_ONE - frame - 7919 * (depth + 1) - 400 - 100 * p) & 0xffffffff
        assert BW.rtr_random(np.array([BW.SEED_U1_IS_ONE], U32))[0] == 1.0
        for area in (1, 2, 6, 13, 1000, 1 << 24):
            got = api.host_pick_slots(np.array([base], U32), 1, api.make_light_params(1, 3, frame=frame), api.make_pick_params(p + 1, depth), area)
            assert got[0, p] == area - 1, f"A = {area}: u = 1.0 gave slot {got[0, p]}"
            assert (got == restated_slots([base], frame, depth, p + 1, area)).all()


@pytest.mark.parametrize("frame,depth", [(0, 0), (9, 2), (3, 5)])
def test_slots_are_uniform_and_two_picks_uncorrelated(frame, depth):
    """every slot's count within 5 standard errors sqrt(N (1/A)(1 - 1/A)) of N / A, and the count of hits whose picks 0 and 1 took the
    same slot within 5 standard errors of N / A, the count of independent uniform picks"""
    n = 200000
    p = api.make_light_params(1, 3, frame=frame)
    for name, seeds in _seed_sets(n).items():
        for area in (2, 6, 13, 100):
            got = api.host_pick_slots(seeds, n, p, api.make_pick_params(2, depth), area)
            se = np.sqrt(n * (1.0 / area) * (1.0 - 1.0 / area))
            for pick in (0, 1):
                counts = np.bincount(got[:, pick], minlength=area)
                assert counts.shape == (area,)
                dev = (counts - n / area) / se
                print(f"frame {frame} depth {depth} {name} seeds A = {area} pick {pick}: worst slot {np.abs(dev).max():.2f} standard errors")
                assert np.abs(dev).max() <= 5.0, f"{name} seeds, A = {area}, pick {pick}: slot {int(np.abs(dev).argmax())} is {dev[np.abs(dev).argmax()]:+.2f} standard errors from N / A"
            same = int((got[:, 0] == got[:, 1]).sum())
            dev = (same - n / area) / se
            print(f"frame {frame} depth {depth} {name} seeds A = {area}: {same} hits picked one slot twice, {dev:+.2f} standard errors")
            assert abs(dev) <= 5.0, f"{name} seeds, A = {area}: picks 0 and 1 agree for {same} hits, {dev:+.2f} standard errors from N / A"


def test_no_hits_do_nothing_and_bad_picks_are_refused():
    lib = A.hip_lib()
    pick = api.make_pick_params(2)
    assert lib.rtr_host_pick_slots(None, 0, 0, 0, 0, C.byref(pick), 6, None) == 0
    out = np.full(4, 0xA5A5A5A5, U32)
    for picks, needle in ((0, "numPicks 0 (1 ... 30)"), (A.PICK_MAX + 1, "numPicks 31 (1 ... 30)")):
        bad = api.make_pick_params(picks)
        assert lib.rtr_host_pick_slots(None, 1, 0, 8, 1, C.byref(bad), 6, out.ctypes.data_as(A.VP)) == INVALID
        assert lib.rtr_last_error().decode() == f"rtr_host_pick_slots: {needle}"
    bad = api.make_pick_params(1)
    bad._reserved[3] = 1
    assert lib.rtr_host_pick_slots(None, 1, 0, 8, 1, C.byref(bad), 6, out.ctypes.data_as(A.VP)) == INVALID
    assert "_reserved" in lib.rtr_last_error().decode()
    assert lib.rtr_host_pick_slots(None, 1, 0, 0, 1, C.byref(pick), 6, out.ctypes.data_as(A.VP)) == INVALID
    assert "width 0, spp 1" in lib.rtr_last_error().decode()
    assert lib.rtr_host_pick_slots(None, 1, 0, 8, 1, C.byref(pick), 6, None) == INVALID
    assert "outSlots is null" in lib.rtr_last_error().decode()
    assert (out == 0xA5A5A5A5).all()
