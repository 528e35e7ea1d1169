"""The MIS calls' C-ABI surface (include/rtr.h, rtr_types.h, rtr_mis.h): the layouts of rtr_mis_params, RtrMisSample and RtrEmitter, the
entry points in the product library and its test build, and every refusal that needs no device, by message.  No GPU needed: the calls
below are all refused before a handle is looked at, so host buffers stand in for the device arrays."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rtr_mis_pick_weights_async", "rtr_mis_pick_weights", "rtr_emitter_hits_async", "rtr_emitter_hits", "rtr_scene_export_light_tris",
       "rtr_host_bounce_pdf", "rtr_host_mis_weights", "rtr_host_emitter_hits")
INVALID, UNSUPPORTED = -1, -4
N = 4


def test_struct_layouts():
    text = open(os.path.join(ROOT, "include", "rtr_types.h")).read()
    for S, fields in ((A.rtr_mis_params, [("numPicks", 0), ("numAreaLights", 4), ("numShadowRays", 8), ("lobes", 12), ("_reserved", 16)]),
                      (A.RtrMisSample, [("lightPdf", 0), ("bouncePdf", 4), ("wPick", 8), ("cosLight", 12), ("dist", 16), ("area", 20), ("lightTri", 24), ("_r", 28)]),
                      (A.RtrEmitter, [("radiance", 0), ("wBounce", 12), ("lightPdf", 16), ("dist", 20), ("lightTri", 24), ("kind", 28)])):
        assert C.sizeof(S) == 32
        assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == fields
        assert f"static_assert(sizeof({S.__name__}) == 32" in text
    p = api.make_mis_params(2, 3, 4)
    assert (p.numPicks, p.numAreaLights, p.numShadowRays, p.lobes, list(p._reserved)) == (2, 3, 4, A.BOUNCE_DIFFUSE | A.BOUNCE_SPECULAR, [0] * 4)
    assert api.make_mis_params(1, 1, 1, lobes=A.BOUNCE_DIFFUSE).lobes == A.BOUNCE_DIFFUSE


def test_abi_version_and_kernel_revision_unchanged():
    lib = A.hip_lib()
    assert lib.rtr_abi_version() == 3
    text = open(os.path.join(ROOT, "include", "rtr_mis.h")).read()
    assert '#include "rtr_bounce.h"' in text and "rtr_device.h\"" not in text
    assert "rtr_mis.h" not in open(os.path.join(ROOT, "realtimeraytracer_amd", "csrc", "kernels", "rtr_device.h")).read()


def test_mis_symbols_are_exported():
    text = open(os.path.join(ROOT, "include", "rtr.h")).read()
    for lib in (C.CDLL(A.LIB_HIP_PATH), C.CDLL(A.LIB_HIP_HOOKS_PATH)):
        for n in NEW:
            assert hasattr(lib, n), n
            assert n in A.RTR_SYMBOLS
            assert re.search(r"\b%s\(" % n, text), n
    for n in ("rtr_mis_pick_weights", "rtr_emitter_hits"):
        assert A.RTR_SYMBOLS[n] == A.RTR_SYMBOLS[n + "_async"]


class Call:
    """one call of each device entry point over host buffers of N hits and P picks, any argument replaceable"""
    def __init__(self, picks=2):
        self.P = picks
        self.rays, self.hits = np.zeros((N, 8), np.float32), np.zeros((N, 8), np.int32)
        self.surf, self.bounce = np.zeros((N, 20), np.float32), np.zeros((N, 8), np.float32)
        self.slots, self.seeds = np.zeros(N * picks + 1, np.uint32), np.zeros(N + 1, np.uint32)
        self.weights, self.samples, self.out = np.zeros(N * picks + 1, np.float32), np.zeros((N * picks + 1, 8), np.float32), np.zeros((N + 1, 8), np.float32)
        self.light = api.make_light_params(1, 3, frame=0, width=2, spp=1)
        self.pick = api.make_pick_params(picks)
        self.mis = api.make_mis_params(picks, 1, 3)

    @staticmethod
    def ptr(x, off=0):
        return None if x is None else C.c_void_p(x.ctypes.data + off)

    def weights_call(self, fn, n=N, **kw):
        a = dict(rays=self.ptr(self.rays), hits=self.ptr(self.hits), light=C.byref(self.light), pick=C.byref(self.pick), mis=C.byref(self.mis), seeds=None,
                 slots=self.ptr(self.slots), out_weights=self.ptr(self.weights), out_samples=self.ptr(self.samples))
        a.update(kw)
        return fn(None, None, a["rays"], a["hits"], n, a["light"], a["pick"], a["mis"], a["seeds"], a["slots"], a["out_weights"], a["out_samples"])

    def emitter_call(self, fn, n=N, **kw):
        a = dict(rays=self.ptr(self.rays), hits=self.ptr(self.hits), surf=self.ptr(self.surf), bounce=self.ptr(self.bounce), mis=C.byref(self.mis), out=self.ptr(self.out))
        a.update(kw)
        return fn(None, None, a["rays"], a["hits"], a["surf"], a["bounce"], n, a["mis"], a["out"])


@pytest.mark.parametrize("name", NEW[:4])
def test_refusals_by_message(name):
    lib = A.hip_lib()
    weights = "pick_weights" in name
    call = (lambda c, **kw: c.weights_call(getattr(lib, name), **kw)) if weights else (lambda c, **kw: c.emitter_call(getattr(lib, name), **kw))

    def refused(needle, status=INVALID, c=None, **kw):
        c = c or Call()
        assert call(c, **kw) == status, needle
        msg = lib.rtr_last_error().decode()
        assert msg.startswith(name + ": ") and needle in msg, f"expected '{name}: ... {needle}', got '{msg}'"

    refused("mis params is null", mis=None)
    for picks, needle in ((0, "numPicks 0 (1 ... 30)"), (31, "numPicks 31 (1 ... 30)")):
        c = Call()
        c.mis.numPicks = picks
        refused(needle, c=c)
    for word in range(4):
        c = Call()
        c.mis._reserved[word] = 1
        refused("_reserved words of mis params are not 0", c=c)
    for lobes in (0, 4, 7):
        c = Call()
        c.mis.lobes = lobes
        refused(f"lobes 0x{lobes:x}", c=c)
    for ns in (0, 1025):
        c = Call()
        c.mis.numShadowRays = ns
        refused(f"numShadowRays {ns} (1 ... 1024)", c=c)
    c = Call()
    arrays = [("rays", c.rays, "rays"), ("hits", c.hits, "hits")]
    arrays += [("out_weights", c.weights, "outWeights")] if weights else [("surf", c.surf, "prevSurfaces"), ("bounce", c.bounce, "bounces"), ("out", c.out, "out")]
    for key, arr, cname in arrays:
        refused(f"{cname} is null", **{key: None})
        refused(f"{cname} is not {4 if key == 'out_weights' else 16}-B aligned", **{key: Call.ptr(arr, 2)})
    if weights:
        refused("pick params is null", pick=None)
        refused("params is null", light=None)
        c = Call()
        c.pick.numPicks = 31
        refused("numPicks", c=c)
        c = Call()
        c.pick._reserved[0] = 1
        refused("_reserved words of pick params are not 0", c=c)
        c = Call()
        c.pick.numPicks = 3
        refused("numPicks 2 of the mis params is not the pick params' 3", c=c)
        c = Call()
        c.mis.numAreaLights = 2
        refused("of the mis params are not the light params'", c=c)
        c = Call()
        c.light.numShadowRays = 2
        refused("of the mis params are not the light params'", c=c)
        refused("outSamples is not 16-B aligned", out_samples=Call.ptr(c.samples, 4))
        refused("slots is not 4-B aligned", slots=Call.ptr(c.slots, 2))
        refused("seeds is not 4-B aligned", seeds=Call.ptr(c.seeds, 2))
        refused("hits x 2 picks do not fit 32 bits", n=0x80000000)
        for width, spp in ((0, 1), (2, 0)):
            c = Call()
            c.light.width, c.light.spp = width, spp
            refused(f"width {width}, spp {spp}", c=c)
        c = Call()
        c.light.outputs = A.LIGHT_SHADOWED | A.LIGHT_ANALYTIC
        refused("RTR_LIGHT_ANALYTIC has no per-sample form", status=UNSUPPORTED, c=c)
        # the optional arrays may be left out
        refused("null context or scene", slots=None, out_samples=None)
    # everything in order: the handles come next, also for no rays
    refused("null context or scene")
    refused("null context or scene", n=0, rays=None, hits=None)
    c = Call()
    call(c)
    for buf in (c.weights, c.samples, c.out):
        assert not buf.any()                 # nothing was written


@pytest.mark.parametrize("name", NEW[:4])
def test_which_refusal_wins_under_two_faults(name):
    """the mis params and their values in order, (rtr_mis_pick_weights: the light and pick params, what the three must agree on, numHits x
    picks), every null before any misaligned pointer in the argument order, the pixel-seed rule, and only then the handles"""
    lib = A.hip_lib()
    weights = "pick_weights" in name
    call = (lambda c, **kw: c.weights_call(getattr(lib, name), **kw)) if weights else (lambda c, **kw: c.emitter_call(getattr(lib, name), **kw))

    def wins(needle, c=None, **kw):
        c = c or Call()
        assert call(c, **kw) == INVALID, needle
        msg = lib.rtr_last_error().decode()
        assert msg.startswith(f"{name}: {needle}"), f"expected '{name}: {needle}', got '{msg}'"

    c = Call()
    wins("mis params is null", mis=None, rays=None)
    c.mis.numPicks, c.mis.numShadowRays, c.mis.lobes, c.mis._reserved[0] = 0, 0, 0, 1
    wins("numPicks 0 (1 ... 30)", c=c)
    c.mis.numPicks = 2
    wins("numShadowRays 0 (1 ... 1024)", c=c)
    c.mis.numShadowRays = 3
    wins("lobes 0x0", c=c, rays=None)
    c.mis.lobes = 3
    wins("_reserved words of mis params are not 0", c=c, rays=None)
    c = Call()
    wins("rays is null", rays=None, hits=None)
    wins("hits is null", hits=None, rays=Call.ptr(c.rays, 2))
    if weights:
        wins("outWeights is null", out_weights=None, rays=Call.ptr(c.rays, 2))
        wins("hits is not 16-B aligned", hits=Call.ptr(c.hits, 2), out_samples=Call.ptr(c.samples, 4))
        wins("seeds is not 4-B aligned", seeds=Call.ptr(c.seeds, 2), slots=Call.ptr(c.slots, 2), out_weights=Call.ptr(c.weights, 2))
        wins("params is null", light=None, pick=None)
        wins("pick params is null", pick=None, rays=None)
        c = Call()
        c.mis.lobes, c.light.numShadowRays = 0, 0
        wins("lobes 0x0", c=c)
        c = Call()
        c.pick.numPicks, c.mis.numAreaLights = 3, 2
        wins("numPicks 2 of the mis params is not the pick params' 3", c=c, rays=None)
        c = Call()
        c.mis.numAreaLights = 2
        wins("numAreaLights 2, numShadowRays 3 of the mis params are not the light params' 1, 3", c=c, n=0x80000000)
        wins("2147483648 hits x 2 picks do not fit 32 bits", n=0x80000000, rays=None)
        c = Call()
        c.light.width = 0
        wins("rays is not 16-B aligned", c=c, rays=Call.ptr(c.rays, 2))
        wins("width 0, spp 1", c=c)
    else:
        wins("out is null", out=None, rays=Call.ptr(c.rays, 2))
        wins("prevSurfaces is not 16-B aligned", surf=Call.ptr(c.surf, 2), out=Call.ptr(c.out, 8))


def test_the_host_forms_under_two_faults():
    lib = A.hip_lib()
    c = Call()
    p = Call.ptr
    x, out = np.zeros(3 * N + 1, np.float32), np.zeros(N + 1, np.float32)

    def wins(fn, needle, *args):
        assert getattr(lib, fn)(*args) == INVALID, needle
        msg = lib.rtr_last_error().decode()
        assert msg.startswith(f"{fn}: {needle}"), msg

    wins("rtr_host_bounce_pdf", "lobes 0x0", None, p(c.surf), p(x), N, 0, p(out))
    wins("rtr_host_bounce_pdf", "outPdf is null", p(c.rays, 2), p(c.surf), p(x), N, 3, None)
    wins("rtr_host_bounce_pdf", "rays is null", None, None, p(x), N, 3, p(out))
    wins("rtr_host_bounce_pdf", "dirs is not 4-B aligned", p(c.rays), p(c.surf), p(x, 2), N, 3, p(out, 2))
    wins("rtr_host_mis_weights", "P 31 (0 ... 30)", N, None, p(x), p(x), p(x), (1 << 24) + 1, 31, p(c.samples), None)
    wins("rtr_host_mis_weights", "Ttot 16777217", N, None, p(x), p(x), p(x), (1 << 24) + 1, 1, p(c.samples), None)
    wins("rtr_host_mis_weights", "outSamples is null", N, p(x, 2), p(x), p(x), p(x), 1, 1, None, None)
    wins("rtr_host_mis_weights", "dist is null", N, p(x), None, p(x), None, 1, 1, p(c.samples), None)
    wins("rtr_host_mis_weights", "cosLight is not 4-B aligned", N, p(x), p(x), p(x, 2), p(x), 1, 1, p(c.samples), p(out, 2))
    rec, first = np.zeros((1, 16), np.float32), np.zeros(1, np.uint32)
    light = (A.RtrAreaLightInfo * 1)()
    light[0].numTriangles = 1
    mis = C.byref(c.mis)
    wins("rtr_host_emitter_hits", "mis params is null", None, p(c.hits), p(c.surf), p(c.bounce), N, None, p(first), light, 1, None, p(c.out))
    wins("rtr_host_emitter_hits", "numAreaLights 1 > lights 0", None, p(c.hits), p(c.surf), p(c.bounce), N, None, p(first), light, 0, mis, p(c.out))
    wins("rtr_host_emitter_hits", "lightTris is null", None, p(c.hits), p(c.surf), p(c.bounce), N, None, None, light, 1, mis, p(c.out))
    wins("rtr_host_emitter_hits", "lightTriFirst is null", None, p(c.hits), p(c.surf), p(c.bounce), N, p(rec), None, None, 1, mis, p(c.out))
    wins("rtr_host_emitter_hits", "out is null", p(c.rays, 2), p(c.hits), p(c.surf), p(c.bounce), N, p(rec), p(first), light, 1, mis, None)
    wins("rtr_host_emitter_hits", "hits is not 16-B aligned", p(c.rays), p(c.hits, 2), p(c.surf), p(c.bounce, 2), N, p(rec), p(first), light, 1, mis, p(c.out))
    assert not c.out.any() and not out.any() and not c.samples.any()


def test_export_light_tris_refusals():
    lib = A.hip_lib()
    count = C.c_uint32(7)
    assert lib.rtr_scene_export_light_tris(None, None, 0, None, C.byref(count)) == INVALID
    assert lib.rtr_last_error().decode().startswith("rtr_scene_export_light_tris: null scene")


def test_host_emitter_refusals():
    lib = A.hip_lib()
    c = Call()
    rec, first = np.zeros((1, 16), np.float32), np.zeros(1, np.uint32)
    light = (A.RtrAreaLightInfo * 1)()
    light[0].numTriangles = 1
    p = Call.ptr

    def host(n=N, **kw):
        a = dict(rays=p(c.rays), hits=p(c.hits), surf=p(c.surf), bounce=p(c.bounce), rec=p(rec), first=p(first), lights=light, nl=1, mis=C.byref(c.mis), out=p(c.out))
        a.update(kw)
        return lib.rtr_host_emitter_hits(a["rays"], a["hits"], a["surf"], a["bounce"], n, a["rec"], a["first"], a["lights"], a["nl"], a["mis"], a["out"])

    def refused(needle, **kw):
        assert host(**kw) == INVALID, needle
        msg = lib.rtr_last_error().decode()
        assert msg.startswith("rtr_host_emitter_hits: ") and needle in msg, msg

    refused("mis params is null", mis=None)
    refused("numAreaLights 1 > lights 0", nl=0)
    refused("lightTris is null", rec=None)
    refused("lightTriFirst is null", first=None)
    refused("lights is null", lights=None)
    for key, cname in (("rays", "rays"), ("hits", "hits"), ("surf", "prevSurfaces"), ("bounce", "bounces"), ("out", "out")):
        refused(f"{cname} is null", **{key: None})
    refused("out is not 16-B aligned", out=p(c.out, 8))
    assert host() == 0 and not c.out.any()       # hits of customIndex 0, primitive 0 on a light whose surfaces are not objects: zeros
    assert host(n=0, rays=None, hits=None, surf=None, bounce=None, out=None) == 0


def test_the_python_signatures():
    sig = inspect.signature(api.make_mis_params).parameters
    assert list(sig) == ["picks", "num_area_lights", "shadow_rays", "lobes"] and sig["lobes"].default == A.BOUNCE_DIFFUSE | A.BOUNCE_SPECULAR
    sig = inspect.signature(api.mis_pick_weights).parameters
    assert list(sig) == ["scene", "rays", "hits", "params", "pick", "mis", "slots", "seeds", "samples", "ctx", "asynchronous"]
    assert [sig[k].default for k in list(sig)[7:]] == [None, False, None, False]
    sig = inspect.signature(api.emitter_hits).parameters
    assert list(sig) == ["scene", "rays", "hits", "prev_surfaces", "bounces", "mis", "ctx", "asynchronous"]
    sig = inspect.signature(api.direct_light).parameters
    assert sig["pick_weights"].default is None
    old, sig = inspect.signature(api.path_trace_picked).parameters, inspect.signature(api.path_trace_mis).parameters
    assert list(sig) == list(old) and sig["light_picks"].default == 1 and sig["pick_from"].default == 1
    assert all(sig[k].default == old[k].default for k in old if k != "light_picks")
    assert hasattr(api.Scene, "export_light_tris") and all(hasattr(api, f) for f in ("host_bounce_pdf", "host_mis_weights", "host_emitter_hits"))
    res = api.EmitterResult()
    assert all(hasattr(res, f) for f in ("radiance", "w_bounce", "light_pdf", "kind", "raw"))


def test_python_wrappers_refuse_before_the_device():
    with pytest.raises(ValueError, match="roulette_from needs compact"):
        api.path_trace_mis(None, None, api.make_light_params(1), 1, roulette_from=1)
    with pytest.raises(ValueError, match="light_picks must be given"):
        api.path_trace_mis(None, None, api.make_light_params(1), 1, light_picks=None)
    with pytest.raises(ValueError, match="pick_weights are the weights of the picked route"):
        api.direct_light(None, None, params=api.make_light_params(1), pick_weights=np.zeros((1, 1), np.float32))
