"""The picked light samples' C-ABI surface (include/rtr.h, rtr_types.h, rtr_pick.h): the layout of rtr_pick_params, the constants, the
five entry points in the product library and its test build, and every refusal that needs no device, by message.  No GPU needed: the
calls below are all refused before a handle is looked at, so host buffers stand in for the device arrays."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rtr_light_rays_picked_async", "rtr_light_rays_picked", "rtr_shade_hits_picked_async", "rtr_shade_hits_picked", "rtr_host_pick_slots")
INVALID, UNSUPPORTED = -1, -4
N = 4


def test_pick_params_layout():
    S = A.rtr_pick_params
    assert C.sizeof(S) == 32
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("numPicks", 0), ("depth", 4), ("_reserved", 8)]
    assert S._reserved.size == 24
    text = open(os.path.join(ROOT, "include", "rtr_types.h")).read()
    body = re.search(r"typedef struct rtr_pick_params \{(.*?)\} rtr_pick_params;", text, re.S).group(1)
    assert re.sub(r"\s+", " ", body).strip() == "uint32_t numPicks, depth; uint32_t _reserved[6];"
    assert 'static_assert(sizeof(rtr_pick_params) == 32' in text
    p = api.make_pick_params()
    assert (p.numPicks, p.depth, list(p._reserved)) == (1, 0, [0] * 6)
    p = api.make_pick_params(picks=3, depth=2)
    assert (p.numPicks, p.depth) == (3, 2)


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "rtr_types.h")).read()
    assert re.search(r"#define RTR_PICK_MAX\s+30u", text) and A.PICK_MAX == 30
    assert re.search(r"#define RTR_PICK_NONE\s+0xffffffffu", text) and A.PICK_NONE == 0xffffffff
    assert re.search(r"#define RTR_PICK_MAX_SLOTS\s+\(1u << 24\)", text) and A.PICK_MAX_SLOTS == 1 << 24
    rule = open(os.path.join(ROOT, "include", "rtr_pick.h")).read()
    assert "7919u * (depth + 1u) + 400u + 100u * p" in rule


def test_abi_version_unchanged():
    assert A.hip_lib().rtr_abi_version() == 3


def test_pick_symbols_are_exported():
    text = open(os.path.join(ROOT, "include", "rtr.h")).read()
    for lib in (C.CDLL(A.LIB_HIP_PATH), C.CDLL(A.LIB_HIP_HOOKS_PATH)):
        for n in NEW:
            assert hasattr(lib, n), n
            assert n in A.RTR_SYMBOLS
            assert re.search(r"\b%s\(" % n, text), n


class Call:
    """one call of each entry point over host buffers of N hits and P picks, any argument replaceable"""
    def __init__(self, picks=2):
        self.P = picks
        self.rays, self.hits = np.zeros((N, 8), np.float32), np.zeros((N, 8), np.int32)
        self.out_rays, self.out = np.zeros((N * (picks + 1), 8), np.float32), np.zeros((N, 12), np.float32)
        self.slots, self.out_slots = np.zeros(N * picks + 1, np.uint32), np.zeros(N * picks + 1, np.uint32)
        self.weights, self.occ = np.zeros(N * picks + 1, np.float32), np.zeros(N * (picks + 1) + 1, np.uint8)
        self.seeds = np.zeros(N + 1, np.uint32)
        self.light = api.make_light_params(1, 3, frame=0, width=2, spp=1)
        self.pick = api.make_pick_params(picks)

    @staticmethod
    def ptr(x, off=0):
        return None if x is None else C.c_void_p(x.ctypes.data + off)

    def rays_call(self, fn, n=N, **kw):
        a = dict(rays=self.ptr(self.rays), hits=self.ptr(self.hits), light=C.byref(self.light), pick=C.byref(self.pick), seeds=None, slots=None,
                 out_rays=self.ptr(self.out_rays), out_slots=self.ptr(self.out_slots))
        a.update(kw)
        return fn(None, None, a["rays"], a["hits"], n, a["light"], a["pick"], a["seeds"], a["slots"], a["out_rays"], a["out_slots"])

    def shade_call(self, fn, n=N, **kw):
        a = dict(rays=self.ptr(self.rays), hits=self.ptr(self.hits), light=C.byref(self.light), pick=C.byref(self.pick), seeds=None,
                 slots=self.ptr(self.slots), weights=None, occ=self.ptr(self.occ), out=self.ptr(self.out))
        a.update(kw)
        return fn(None, None, a["rays"], a["hits"], n, a["light"], a["pick"], a["seeds"], a["slots"], a["weights"], a["occ"], a["out"])


def _entry(lib, name):
    return (lambda c, **kw: c.rays_call(getattr(lib, name), **kw)) if "light_rays" in name else (lambda c, **kw: c.shade_call(getattr(lib, name), **kw))


@pytest.mark.parametrize("name", NEW[:4])
def test_refusals_by_message(name):
    lib = A.hip_lib()
    call = _entry(lib, name)
    shade = "shade" in name

    def refused(needle, status=INVALID, c=None, **kw):
        c = c or Call()
        assert call(c, **kw) == status, needle
        msg = lib.rtr_last_error().decode()
        assert msg.startswith(name + ": ") and needle in msg, f"expected '{name}: ... {needle}', got '{msg}'"

    # the params
    refused("params is null", light=None)
    refused("pick params is null", pick=None)
    for picks, needle in ((0, "numPicks 0 (1 ... 30)"), (31, "numPicks 31 (1 ... 30)")):
        c = Call()
        c.pick.numPicks = picks
        refused(needle, c=c)
    for word in range(6):
        c = Call()
        c.pick._reserved[word] = 1
        refused("_reserved words of pick params are not 0", c=c)
    # what rtr_light_slots refuses of the params alone
    for ns in (0, 1025):
        c = Call()
        c.light.numShadowRays = ns
        refused(f"numShadowRays {ns} (1 ... 1024)", c=c)
    c = Call()
    c.light.outputs = 8
    refused("unknown output bits 0x8", c=c)
    # numHits x R past 32 bits: R = 3 here, 31 at the most picks
    refused("hits x 3 slots do not fit 32 bits", n=0x60000000)
    refused("hits x 31 slots do not fit 32 bits", c=Call(30), n=0x09000000)
    # null and misaligned arrays
    c = Call()
    arrays = [("rays", c.rays, 16), ("hits", c.hits, 16)]
    arrays += [("slots", c.slots, 4), ("occ", c.occ, 0), ("out", c.out, 16)] if shade else [("out_rays", c.out_rays, 16), ("out_slots", c.out_slots, 4)]
    names = {"occ": "occluded", "out_rays": "outRays", "out_slots": "outSlots"}
    for key, arr, align in arrays:
        refused(f"{names.get(key, key)} is null", **{key: None})
        if align:
            refused(f"{names.get(key, key)} is not {align}-B aligned", **{key: Call.ptr(arr, 2)})
    refused("seeds is not 4-B aligned", seeds=Call.ptr(c.seeds, 2))
    if shade:
        refused("weights is not 4-B aligned", weights=Call.ptr(c.weights, 1))
    else:
        refused("slotsIn is not 4-B aligned", slots=Call.ptr(c.slots, 3))
    # without seeds the hits are pixel-samples of a frame
    for width, spp in ((0, 1), (2, 0)):
        c = Call()
        c.light.width, c.light.spp = width, spp
        refused(f"width {width}, spp {spp}", c=c)
        assert call(c, seeds=Call.ptr(c.seeds)) == INVALID and "null context or scene" in lib.rtr_last_error().decode()      # with seeds they pass
    # the analytic sum has no per-sample form
    c = Call()
    c.light.outputs = A.LIGHT_SHADOWED | A.LIGHT_ANALYTIC
    if shade:
        refused("RTR_LIGHT_ANALYTIC has no per-sample form", status=UNSUPPORTED, c=c)
        refused("RTR_LIGHT_ANALYTIC has no per-sample form", status=UNSUPPORTED, c=c, n=0)
    else:
        refused("null context or scene", c=c)
    # everything in order: the handles come next, also for no hits
    refused("null context or scene")
    refused("null context or scene", n=0, rays=None, hits=None)
    for buf in (c.out_rays, c.out, c.out_slots):
        assert not buf.any()             # nothing was written


@pytest.mark.parametrize("name", NEW[:4])
def test_which_refusal_wins_under_two_faults(name):
    """the light params, the pick params, the light params' values, numHits x R, every null before any misaligned pointer in the
    argument order, the pixel-seed rule, and only then the handles"""
    lib = A.hip_lib()
    call = _entry(lib, name)
    shade = "shade" in name
    last, last_name = ("out", "out") if shade else ("out_slots", "outSlots")

    def wins(needle, status=INVALID, c=None, **kw):
        c = c or Call()
        assert call(c, **kw) == status, needle
        msg = lib.rtr_last_error().decode()
        assert msg.startswith(f"{name}: {needle}"), f"expected '{name}: {needle}', got '{msg}'"

    c = Call()
    wins(f"{last_name} is null", rays=Call.ptr(c.rays, 2), **{last: None})
    wins("rays is null", rays=None, hits=None)
    wins("hits is not 16-B aligned", hits=Call.ptr(c.hits, 2), seeds=Call.ptr(c.seeds, 2))
    wins("seeds is not 4-B aligned", seeds=Call.ptr(c.seeds, 2), slots=Call.ptr(c.slots, 2))
    wins("params is null", light=None, pick=None)
    wins("pick params is null", pick=None, rays=None)
    c = Call()
    c.pick.numPicks, c.pick._reserved[0], c.light.numShadowRays = 0, 1, 0
    wins("numPicks 0 (1 ... 30)", c=c)
    c = Call()
    c.pick._reserved[3], c.light.numShadowRays, c.light.outputs = 1, 0, 8
    wins("_reserved words of pick params are not 0", c=c)
    c = Call()
    c.light.numShadowRays, c.light.outputs = 0, 8 | A.LIGHT_ANALYTIC
    wins("numShadowRays 0 (1 ... 1024)", c=c, rays=None)
    c = Call()
    c.light.outputs = 8 | A.LIGHT_ANALYTIC
    wins("unknown output bits 0xc", c=c, n=0x60000000)
    wins("1610612736 hits x 3 slots do not fit 32 bits", n=0x60000000, rays=None)
    c = Call()
    c.light.width = 0
    wins("rays is not 16-B aligned", c=c, rays=Call.ptr(c.rays, 2))
    c = Call()
    c.light.width = 0
    wins("width 0, spp 1", c=c)                  # before the handles, which are null throughout


def test_host_pick_slots_under_two_faults():
    lib = A.hip_lib()
    seeds, out = np.zeros(N + 1, np.uint32), np.zeros(2 * N + 1, np.uint32)
    pick = api.make_pick_params(2)
    p = Call.ptr

    def wins(needle, seeds_p=p(seeds), n=N, width=2, spp=1, pick_p=C.byref(pick), area=6, out_p=p(out)):
        assert lib.rtr_host_pick_slots(seeds_p, n, 0, width, spp, pick_p, area, out_p) == INVALID, needle
        msg = lib.rtr_last_error().decode()
        assert msg.startswith("rtr_host_pick_slots: " + needle), msg

    wins("pick params is null", pick_p=None, area=(1 << 24) + 1)
    wins("16777217 area slots", area=(1 << 24) + 1, n=0, out_p=None)
    wins("4294967295 hits x 2 picks do not fit 32 bits", n=0xffffffff, out_p=None)
    wins("outSlots is null", out_p=None, seeds_p=p(seeds, 2))
    wins("outSlots is not 4-B aligned", out_p=p(out, 2), seeds_p=p(seeds, 2))
    wins("seeds is not 4-B aligned", seeds_p=p(seeds, 2), width=0)
    wins("width 0, spp 0", seeds_p=None, width=0, spp=0)
    assert not out.any()


def test_the_python_signatures():
    sig = inspect.signature(api.make_pick_params).parameters
    assert [(k, sig[k].default) for k in sig] == [("picks", 1), ("depth", 0)]
    sig = inspect.signature(api.light_rays_picked).parameters
    assert list(sig) == ["scene", "rays", "hits", "params", "pick", "seeds", "slots", "ctx", "asynchronous"]
    assert [sig[k].default for k in list(sig)[5:]] == [None, None, None, False]
    sig = inspect.signature(api.shade_hits_picked).parameters
    assert list(sig) == ["scene", "rays", "hits", "params", "pick", "slots", "occluded", "weights", "seeds", "ctx", "asynchronous"]
    assert [sig[k].default for k in list(sig)[7:]] == [None, None, None, False]
    # the new arguments come last and default to the routes as they were
    sig = inspect.signature(api.direct_light).parameters
    assert list(sig)[-2:] == ["picks", "pick_depth"] and (sig["picks"].default, sig["pick_depth"].default) == (None, 0)
    # path_trace keeps its arguments; path_trace_picked takes them all, by the same names and defaults, and the two of the picks
    old, sig = inspect.signature(api.path_trace).parameters, inspect.signature(api.path_trace_picked).parameters
    assert "light_picks" not in old and "pick_from" not in old
    assert list(sig)[:6] == ["scene", "rays", "light_params", "bounces", "light_picks", "pick_from"] and list(sig)[6:] == list(old)[4:]
    assert (sig["light_picks"].default, sig["pick_from"].default) == (None, 1)
    assert all(sig[k].default == old[k].default for k in old)


def test_python_wrappers_refuse_before_the_device():
    with pytest.raises(ValueError, match="roulette_from needs compact"):
        api.path_trace_picked(None, None, api.make_light_params(1), 1, roulette_from=1, light_picks=1)
    with pytest.raises(ValueError, match="light_picks cannot give the analytic sum"):
        api.path_trace_picked(None, None, api.make_light_params(1, outputs=A.LIGHT_SHADOWED | A.LIGHT_ANALYTIC), 1, light_picks=1)
    with pytest.raises(ValueError, match="pick_from must be >= 0"):
        api.path_trace_picked(None, None, api.make_light_params(1), 1, light_picks=1, pick_from=-1)
