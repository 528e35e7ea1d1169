"""rtr_host_accumulate_paths and rtr_host_gather_records against the numpy witness of tests/accum_witness.py, bit for bit, with guard
words behind (and before) every array.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import accum_witness as W
from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api


def run_host(case):
    """the host form on guarded buffers -> (accum, out_term, out_throughput) payload words, after checking every guard"""
    lib = A.hip_lib()
    bufs = case.host_buffers()
    before = {k: v[0].copy() for k, v in bufs.items() if v is not None}
    rc = W.call_accumulate(lib.rtr_host_accumulate_paths, None, case, A, lambda name: bufs[name][1].ctypes.data if bufs[name] is not None else None)
    assert rc == 0, lib.rtr_last_error()
    for name, v in bufs.items():
        if v is None:
            continue
        assert W.guards_intact(v[0]), f"{name}: guard words changed"
        if name not in ("accum", "term", "out_t") and not (name == "T" and case.inplace):
            assert (v[0] == before[name]).all(), f"{name}: an input changed"
    S = case.num_slots
    acc = bufs["accum"][1].reshape(S, case.image_words)
    term = bufs["term"][1].reshape(S, case.image_words) if bufs["term"] is not None else None
    if case.inplace:
        out_t = bufs["T"][1].reshape(case.n, 3)
    else:
        out_t = bufs["out_t"][1].reshape(case.n, 3) if bufs["out_t"] is not None else None
    return acc, term, out_t


def assert_case(case):
    acc, term, out_t = run_host(case)
    want_acc, want_term, want_t = case.expected()
    assert (acc == want_acc.view(np.uint32)).all()
    assert (term is None) == (want_term is None) and (term is None or (term == want_term.view(np.uint32)).all())
    assert (out_t is None) == (want_t is None) and (out_t is None or (out_t == want_t.view(np.uint32)).all())
    # image rows that no id names keep their bytes
    named = np.zeros(case.num_slots, bool)
    slots = case.slots()
    named[slots[slots < case.num_slots]] = True
    assert (acc[~named] == case.accum0.view(np.uint32)[~named]).all()
    if term is not None:
        assert (term[~named] == case.term0.view(np.uint32)[~named]).all()


@pytest.mark.parametrize("n", [1, 5, 64, 257, 1000])
def test_host_form_equals_the_witness(n):
    for case in W.optional_cases(n):
        assert_case(case)


def test_every_branch_of_the_rule_is_taken_by_the_cases():
    """light rows with a non-zero emitter record, miss rows with a non-zero escape record, rows of all four kinds and skipped rows are
    in the input, and the flags change the result: else a pass shows nothing"""
    both = W.LIGHTS_FROM_EMITTERS | W.MISSES_FROM_ESCAPES
    case = W.AccumCase(257, flags=both, emitters=True, escapes=True, sky=True, bounces=True, term=True, ids="mixed", seed=11)
    kind = case.radiance[:, 3]
    assert set(kind.tolist()) == {0, 1, 2, 3}
    assert (case.emitters[kind == W.SURFACE_LIGHT, 0:3].view(np.float32) != 0).all() and (kind == W.SURFACE_LIGHT).sum() > 10
    assert (case.escapes[kind == W.SURFACE_MISS, 0:3].view(np.float32) != 0).all() and (kind == W.SURFACE_MISS).sum() > 10
    slots = case.slots()
    assert (slots == W.PATH_NONE).any() and (slots == case.num_slots).any() and (slots == case.num_slots + 5).any() and (slots < case.num_slots).sum() > 100
    acc = {}
    for flags in (0, W.LIGHTS_FROM_EMITTERS, W.MISSES_FROM_ESCAPES, both):
        case.flags = flags
        assert_case(case)
        acc[flags] = run_host(case)[0].copy()
    assert len({a.tobytes() for a in acc.values()}) == 4
    # the flags without their arrays: those rows add T * 0
    case.flags, case.emitters, case.escapes = both, None, None
    assert_case(case)
    assert run_host(case)[0].tobytes() not in {a.tobytes() for a in acc.values()}


def test_a_term_of_zero_is_still_added_and_written():
    case = W.AccumCase(64, term=True, seed=5)
    case.radiance[:, 0:3] = 0
    case.accum0[:, 0:3] = np.float32(-0.0)
    acc, term, _ = run_host(case)
    assert (acc.reshape(64, 3) == 0).all() and (term.reshape(64, 3) == 0).all()      # -0 + +0 = +0: the addition happened; the 9.0 is gone


def test_zero_paths_write_nothing():
    lib = A.hip_lib()
    assert lib.rtr_host_accumulate_paths(None, None, None, None, None, None, None, 0, None, None, None, None) == 0
    assert lib.rtr_host_gather_records(None, 0, 0, None, 0, None) == 0
    case = W.AccumCase(0, num_slots=4, term=True)
    bufs = case.host_buffers()
    before = bufs["accum"][0].copy()
    assert W.call_accumulate(lib.rtr_host_accumulate_paths, None, case, A, lambda name: bufs[name][1].ctypes.data if bufs[name] is not None else None) == 0
    assert (bufs["accum"][0] == before).all()


@pytest.mark.parametrize("record_bytes", [4, 12, 32, 80, 256])
@pytest.mark.parametrize("n", [1, 65, 1000])
def test_host_gather_equals_numpy_take(record_bytes, n):
    lib = A.hip_lib()
    rng = np.random.default_rng(record_bytes * 7 + n)
    w = record_bytes // 4
    num_src = max(1, n - 3)
    src = rng.integers(1, 2 ** 32, (num_src, w), dtype=np.uint32)
    rows = rng.integers(0, num_src, n).astype(np.uint32)
    rows[::7] = np.resize(np.array([W.PATH_NONE, num_src, num_src + 5], np.uint32), rows[::7].size)
    sb, rb, ob = W.guarded(src), W.guarded(rows), W.guarded(np.full((n, w), 0x5A5A5A5A, np.uint32))
    rc = lib.rtr_host_gather_records(C.c_void_p(sb[1].ctypes.data), record_bytes, num_src, C.c_void_p(rb[1].ctypes.data), n, C.c_void_p(ob[1].ctypes.data))
    assert rc == 0, lib.rtr_last_error()
    want = W.witness_gather(src, rows)
    assert (want[::7] == 0).all() and (ob[1].reshape(n, w) == want).all()
    assert W.guards_intact(ob[0]) and W.guards_intact(sb[0]) and W.guards_intact(rb[0])
    assert (api.host_gather_records(src, rows.view(np.int32)) == want).all()
    # the word path: records at an address that is 4 B past a multiple of 16
    shifted = W.guarded(np.concatenate([np.zeros(1, np.uint32), src.reshape(-1)]))
    ob2 = W.guarded(np.full(n * w + 1, 0x5A5A5A5A, np.uint32))
    rc = lib.rtr_host_gather_records(C.c_void_p(shifted[1].ctypes.data + 4), record_bytes, num_src, C.c_void_p(rb[1].ctypes.data), n, C.c_void_p(ob2[1].ctypes.data + 4))
    assert rc == 0 and (ob2[1][1:].reshape(n, w) == want).all() and ob2[1][0] == 0x5A5A5A5A and W.guards_intact(ob2[0])


def test_python_host_form():
    case = W.AccumCase(100, flags=3, emitters=True, escapes=True, sky=True, bounces=True, term=True, ids="mixed", t_words=8, image_words=4, seed=2)
    acc, term = case.accum0.copy(), case.term0.copy()
    out_t = api.host_accumulate_paths(case.radiance, case.T.view(np.float32), acc, api.make_accum_params(case.num_slots, True, True), path_ids=case.ids,
                                      emitters=case.emitters, escapes=case.escapes, sky_sums=case.sky, bounces=case.bounces, out_term=term)
    want_acc, want_term, want_t = case.expected()
    assert acc.tobytes() == want_acc.tobytes() and term.tobytes() == want_term.tobytes() and out_t.tobytes() == want_t.tobytes()
    assert api.host_accumulate_paths(case.radiance, case.T.view(np.float32), acc, api.make_accum_params(case.num_slots)) is None
