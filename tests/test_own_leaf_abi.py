"""Start hints for the queued occlusion query — the C-ABI surface of rtr_hit_leaves, rtr_light_rays_hinted and
rtr_trace_occlusion_hinted (each with its _async form) and what needs no device: the header declares them, the product and the test
library export them, _abi.py binds them, the ABI version stays 3, the argument errors that come before any device work name the call,
and api.direct_light knows the route that uses them."""
import ctypes as C
import os
import re
import subprocess

import pytest

from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rtr_hit_leaves_async", "rtr_hit_leaves", "rtr_light_rays_hinted_async", "rtr_light_rays_hinted", "rtr_trace_occlusion_hinted_async",
         "rtr_trace_occlusion_hinted")
INVALID = -1


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "rtr.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(rtr_[a-z0-9_]+)\s*\(", text))
    for path in (A.LIB_HIP_PATH, A.LIB_HIP_HOOKS_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        for n in NAMES:
            assert n in declared, f"{n} is not declared in include/rtr.h"
            assert n in exported, f"{os.path.basename(path)} does not export {n}"
            assert n in A.RTR_SYMBOLS, f"{n} is not bound in _abi.RTR_SYMBOLS"
    # an _async form takes its synchronous form's arguments (the hinted query: without the stats)
    for n in ("rtr_hit_leaves", "rtr_light_rays_hinted"):
        assert A.RTR_SYMBOLS[n] == A.RTR_SYMBOLS[n + "_async"]
    assert A.RTR_SYMBOLS["rtr_trace_occlusion_hinted"][1][:-1] == A.RTR_SYMBOLS["rtr_trace_occlusion_hinted_async"][1]
    # the hinted calls are their plain calls plus one pointer: outLeaves last, startLeaves after rays
    assert A.RTR_SYMBOLS["rtr_light_rays_hinted"][1] == A.RTR_SYMBOLS["rtr_light_rays"][1] + [A.VP]
    plain = A.RTR_SYMBOLS["rtr_trace_occlusion"][1]
    assert A.RTR_SYMBOLS["rtr_trace_occlusion_hinted"][1] == plain[:3] + [A.VP] + plain[3:]
    assert A.hip_lib().rtr_abi_version() == 3
    assert re.search(r"#define\s+RTR_ABI_VERSION\s+3\b", header)
    assert callable(api.hit_leaves)
    # the header says that the first use allocates
    assert re.search(r"FIRST CALL.*?ALLOCATES", header, flags=re.S)


def test_argument_errors_that_need_no_device():
    lib = A.hip_lib()
    err = lib.rtr_last_error
    fake = A.VP(0x1000)                     # aligned, never dereferenced: every call below fails before it touches a device
    p = api.make_light_params(1, 3, 0, 8, 1)
    # a null context or scene
    calls = (("rtr_hit_leaves", (fake, 64, fake)), ("rtr_hit_leaves_async", (fake, 64, fake)),
             ("rtr_light_rays_hinted", (fake, fake, 64, C.byref(p), None, fake, fake)),
             ("rtr_light_rays_hinted_async", (fake, fake, 64, C.byref(p), None, fake, fake)),
             ("rtr_trace_occlusion_hinted", (fake, fake, 64, 0, fake, 1 << 20, fake, None)),
             ("rtr_trace_occlusion_hinted_async", (fake, fake, 64, 0, fake, 1 << 20, fake)))
    for name, args in calls:
        assert getattr(lib, name)(None, None, *args) == INVALID, name
        assert b"null context" in err() and name.encode() + b":" in err(), err()
    # a null pointer of the call's own
    assert lib.rtr_hit_leaves(None, None, fake, 64, None) == INVALID
    assert b"rtr_hit_leaves: leaves is null" in err(), err()
    assert lib.rtr_hit_leaves_async(None, None, None, 64, fake) == INVALID
    assert b"rtr_hit_leaves_async: hits is null" in err(), err()
    assert lib.rtr_light_rays_hinted(None, None, fake, fake, 64, C.byref(p), None, fake, None) == INVALID
    assert b"rtr_light_rays_hinted: outLeaves is null" in err(), err()
    assert lib.rtr_light_rays_hinted_async(None, None, fake, fake, 64, C.byref(p), None, fake, None) == INVALID
    assert b"rtr_light_rays_hinted_async: outLeaves is null" in err(), err()
    # a misaligned one
    assert lib.rtr_hit_leaves(None, None, A.VP(0x1008), 64, fake) == INVALID
    assert b"rtr_hit_leaves: hits is not 16-B aligned" in err(), err()
    assert lib.rtr_hit_leaves(None, None, fake, 64, A.VP(0x1002)) == INVALID
    assert b"rtr_hit_leaves: leaves is not 4-B aligned" in err(), err()
    assert lib.rtr_light_rays_hinted(None, None, fake, fake, 64, C.byref(p), None, fake, A.VP(0x1001)) == INVALID
    assert b"rtr_light_rays_hinted: outLeaves is not 4-B aligned" in err(), err()
    assert lib.rtr_trace_occlusion_hinted(None, None, fake, A.VP(0x1002), 64, 0, fake, 1 << 20, fake, None) == INVALID
    assert b"rtr_trace_occlusion_hinted: startLeaves is not 4-B aligned" in err(), err()
    assert lib.rtr_trace_occlusion_hinted_async(None, None, fake, A.VP(0x1003), 64, 0, fake, 1 << 20, fake) == INVALID
    assert b"rtr_trace_occlusion_hinted_async: startLeaves is not 4-B aligned" in err(), err()
    # NULL hints are the unhinted call: its own refusal, under the hinted name
    assert lib.rtr_trace_occlusion_hinted(None, None, fake, None, 64, 0, fake, 1 << 20, fake, None) == INVALID
    assert b"rtr_trace_occlusion_hinted: null context or scene" in err(), err()


def test_which_refusal_wins_under_two_faults():
    """rtr_hit_leaves checks its arrays before the handles, every null before any misaligned pointer; the hinted calls check their own
    array first, then the handles, and only then the other arrays"""
    lib = A.hip_lib()
    err = lib.rtr_last_error
    fake, odd16, odd4 = A.VP(0x1000), A.VP(0x1008), A.VP(0x1002)
    p = api.make_light_params(1, 3, 0, 8, 1)
    for name in ("rtr_hit_leaves", "rtr_hit_leaves_async"):
        fn, who = getattr(lib, name), name.encode() + b": "
        assert fn(None, None, odd16, 64, None) == INVALID and err().startswith(who + b"leaves is null"), err()
        assert fn(None, None, None, 64, None) == INVALID and err().startswith(who + b"hits is null"), err()
        assert fn(None, None, odd16, 64, odd4) == INVALID and err().startswith(who + b"hits is not 16-B aligned"), err()
        assert fn(None, None, None, 0, None) == INVALID and err().startswith(who + b"null context or scene"), err()
    for name in ("rtr_light_rays_hinted", "rtr_light_rays_hinted_async"):
        fn, who = getattr(lib, name), name.encode() + b": "
        assert fn(None, None, None, odd16, 64, None, odd4, None, None) == INVALID and err().startswith(who + b"outLeaves is null"), err()
        assert fn(None, None, None, odd16, 64, None, odd4, None, odd4) == INVALID and err().startswith(who + b"outLeaves is not 4-B aligned"), err()
        assert fn(None, None, None, odd16, 64, C.byref(p), odd4, None, fake) == INVALID and err().startswith(who + b"null context, scene or params"), err()
        assert fn(None, None, None, None, 0, None, None, None, None) == INVALID and err().startswith(who + b"null context, scene or params"), err()
    for name, tail in (("rtr_trace_occlusion_hinted", (None,)), ("rtr_trace_occlusion_hinted_async", ())):
        fn, who = getattr(lib, name), name.encode() + b": "
        assert fn(None, None, None, odd4, 64, 0x100, None, 0, odd16, *tail) == INVALID and err().startswith(who + b"startLeaves is not 4-B aligned"), err()
        assert fn(None, None, None, fake, 64, 0x100, None, 0, odd16, *tail) == INVALID and err().startswith(who + b"null context or scene"), err()
        assert fn(None, None, None, odd4, 0, 0x100, None, 0, odd16, *tail) == INVALID and err().startswith(who + b"null context or scene"), err()


def test_direct_light_knows_the_own_leaf_route():
    with pytest.raises(ValueError, match="occlusion must be"):
        api.direct_light(None, None, occlusion="sparse")
    with pytest.raises(ValueError, match="occlusion must be"):
        api.direct_light(None, None, occlusion="queued_own_leaf ")
    # an accepted name goes on to the next check (params are missing), with no device touched
    for name in ("dense", "queued", "queued_own_leaf"):
        with pytest.raises(ValueError, match="params"):
            api.direct_light(None, None, occlusion=name)
