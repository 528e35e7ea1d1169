"""The C-ABI surface of rtr_bounce_rays — what needs no device: the header declares the entry points and the two structs, the product and
the test library export them with C linkage, _abi.py binds them with the header's argument lists, both structs are 32 bytes on both
sides, every refusal comes with a message that names the function and the argument, and a refused call writes nothing."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import bounce_witness as W
from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
VP, u32 = A.VP, A.u32
PP = C.POINTER(A.rtr_bounce_params)
DEVICE_PARAMS = ("rtr_ctx* ctx, const RtrRay* rays, const RtrSurface* surfaces, uint32_t numHits, const rtr_bounce_params* params, "
                 "const uint32_t* seeds, RtrRay* outRays, RtrBounce* outBounce")
EXPECTED = {
    "rtr_bounce_rays_async": (DEVICE_PARAMS, [VP, VP, VP, u32, PP, VP, VP, VP]),
    "rtr_bounce_rays": (DEVICE_PARAMS, [VP, VP, VP, u32, PP, VP, VP, VP]),
    "rtr_host_bounce_rays": (DEVICE_PARAMS.split(", ", 1)[1], [VP, VP, u32, PP, VP, VP, VP]),
    "rtr_host_sincos_turn": ("const float* u, uint32_t n, float* outSin, float* outCos", [VP, u32, VP, VP]),
}


def _text(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def _norm(params):
    return [re.sub(r"\s+", " ", p).strip() for p in params.split(",")]


def test_the_entry_points_are_declared_exported_and_bound():
    text = _text("rtr.h")
    for path in (A.LIB_HIP_PATH, A.LIB_HIP_HOOKS_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        for n in EXPECTED:
            assert n in exported, f"{os.path.basename(path)} does not export {n} with C linkage"
    for n, (params, argtypes) in EXPECTED.items():
        m = re.search(r"\bint\s+" + n + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{n} is not declared in include/rtr.h"
        assert _norm(m.group(1)) == _norm(params), f"{n}: the header's parameters are {_norm(m.group(1))}"
        res, args = A.RTR_SYMBOLS[n]
        assert res is C.c_int and list(args) == argtypes, f"{n}: bound as {args}"
    assert A.hip_lib().rtr_abi_version() == 3 and re.search(r"#define\s+RTR_ABI_VERSION\s+3\b", open(os.path.join(ROOT, "include", "rtr.h")).read())


def test_the_structs():
    text = _text("rtr_types.h")
    assert re.search(r"#define\s+RTR_BOUNCE_DIFFUSE\s+1u", text) and re.search(r"#define\s+RTR_BOUNCE_SPECULAR\s+2u", text)
    assert (A.BOUNCE_DIFFUSE, A.BOUNCE_SPECULAR) == (1, 2)
    for name in ("RtrBounce", "rtr_bounce_params"):
        assert re.search(r"typedef\s+struct\s+" + name + r"\s*\{.*?\}\s*" + name + r"\s*;", text, flags=re.S), f"{name} is not declared"
        assert f"static_assert(sizeof({name}) == 32" in text
        assert C.sizeof(getattr(A, name)) == 32
    B, Pm = A.RtrBounce, A.rtr_bounce_params
    assert (B.weight.offset, B.pdf.offset, B.lobe.offset, B.pSpecular.offset, B._reserved.offset) == (0, 12, 16, 20, 24)
    assert [f[0] for f in Pm._fields_] == ["frame", "depth", "width", "spp", "lobes", "normalOffset", "tmin", "tmax"]
    assert [getattr(Pm, f[0]).offset for f in Pm._fields_] == list(range(0, 32, 4))


def test_make_bounce_params_and_the_python_signatures():
    p = api.make_bounce_params()
    assert (p.frame, p.depth, p.width, p.spp, p.lobes) == (0, 0, 0, 1, A.BOUNCE_DIFFUSE | A.BOUNCE_SPECULAR)
    assert (p.normalOffset, p.tmin, p.tmax) == (np.float32(0.01), np.float32(0.001), np.float32(10000.0))
    sig = inspect.signature(api.make_bounce_params).parameters
    assert list(sig) == ["frame", "depth", "width", "spp", "lobes", "normal_offset", "tmin", "tmax"]
    assert list(inspect.signature(api.bounce_rays).parameters) == ["ctx", "rays", "surfaces", "params", "seeds", "asynchronous"]
    assert list(inspect.signature(api.host_bounce_rays).parameters) == ["rays", "surfaces", "params", "seeds"]
    sig = inspect.signature(api.path_trace).parameters
    assert list(sig)[:9] == ["scene", "rays", "light_params", "bounces", "seeds", "occlusion", "bounce_cull_mask", "bounce_ray_flags", "max_ray_bytes"]
    assert sig["occlusion"].default == "dense" and sig["bounce_cull_mask"].default is None and sig["bounce_ray_flags"].default == 0
    assert sig["max_ray_bytes"].default == 256 << 20


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
N = 96
PATTERN = 0xA5


class Buffers:
    """16-B aligned host arrays of N records, the outputs pre-filled with a pattern; the outputs have room for 2 N records, so that an
    output moved to the last record of the other one still ends inside that array and reaches no third one"""

    def __init__(self):
        rays, sf, seeds = W.make_surfaces(N, seed=11)
        self.keep = [np.zeros(len(x.tobytes()) + 64, np.uint8) for x in (rays, sf, seeds)] + [np.full(64 * N + 64, PATTERN, np.uint8) for _ in range(2)]
        self.addr = []
        for k, buf in enumerate(self.keep):
            a = (buf.ctypes.data + 15) & ~15
            self.addr.append(a)
            if k < 3:
                C.memmove(a, (rays, sf, seeds)[k].ctypes.data, (rays, sf, seeds)[k].nbytes)
        self.rays, self.surfaces, self.seeds, self.out_rays, self.out_bounce = self.addr

    def args(self, **kw):
        a = {"rays": self.rays, "surfaces": self.surfaces, "n": N, "params": api.make_bounce_params(width=8, spp=1), "seeds": self.seeds,
             "outRays": self.out_rays, "outBounce": self.out_bounce}
        a.update(kw)
        p = a["params"]
        return (VP(a["rays"]), VP(a["surfaces"]), a["n"], C.byref(p) if p is not None else None, VP(a["seeds"]) if a["seeds"] else None,
                VP(a["outRays"]), VP(a["outBounce"]))

    def untouched(self):
        return all((self.keep[k] == PATTERN).all() for k in (3, 4))


def _refusals(b):
    mk = api.make_bounce_params
    nan, inf = float("nan"), float("inf")
    return [
        ({"rays": 0}, b"rays is null"), ({"surfaces": 0}, b"surfaces is null"), ({"outRays": 0}, b"outRays is null"),
        ({"outBounce": 0}, b"outBounce is null"), ({"params": None}, b"params is null"),
        ({"rays": b.rays + 4}, b"rays is not 16-B aligned"), ({"surfaces": b.surfaces + 8}, b"surfaces is not 16-B aligned"),
        ({"outRays": b.out_rays + 4}, b"outRays is not 16-B aligned"), ({"outBounce": b.out_bounce + 8}, b"outBounce is not 16-B aligned"),
        ({"seeds": b.seeds + 2}, b"seeds is not 4-B aligned"),
        ({"params": mk(lobes=0, width=8)}, b"lobes"), ({"params": mk(lobes=4, width=8)}, b"lobes"), ({"params": mk(lobes=7, width=8)}, b"lobes"),
        ({"params": mk(width=0, spp=1), "seeds": 0}, b"width"), ({"params": mk(width=8, spp=0), "seeds": 0}, b"spp"),
        ({"params": mk(normal_offset=nan)}, b"normalOffset"), ({"params": mk(normal_offset=inf)}, b"normalOffset"),
        ({"params": mk(tmin=nan)}, b"tmin"), ({"params": mk(tmin=-inf)}, b"tmin"),
        ({"params": mk(tmax=nan)}, b"tmax"), ({"params": mk(tmax=inf)}, b"tmax"),
        ({"params": mk(tmin=1.0, tmax=1.0)}, b"tmax"), ({"params": mk(tmin=2.0, tmax=1.0)}, b"tmax"),
        ({"outRays": b.rays}, b"outRays overlaps rays"), ({"outBounce": b.surfaces + 16 * (N // 2)}, b"outBounce overlaps surfaces"),
        ({"outBounce": b.out_rays + 32 * (N - 1)}, b"outRays overlaps outBounce"),
    ]


def test_the_host_call_refuses_and_writes_nothing():
    lib = A.hip_lib()
    b = Buffers()
    for kw, needle in _refusals(b):
        assert lib.rtr_host_bounce_rays(*b.args(**kw)) == INVALID, kw
        msg = lib.rtr_last_error()
        assert b"rtr_host_bounce_rays: " in msg and needle in msg, (kw, msg)
        if "outRays" not in kw or kw["outRays"] != b.rays:
            assert b.untouched(), f"a refused call wrote to its outputs: {kw}"
    assert b.untouched()
    # numHits == 0 does nothing, whatever else is passed
    assert lib.rtr_host_bounce_rays(None, None, 0, None, None, None, None) == 0
    # and the accepted call fills every record
    assert lib.rtr_host_bounce_rays(*b.args()) == 0, lib.rtr_last_error()
    assert not b.untouched()
    # width / spp == 0 are fine with explicit seeds
    assert lib.rtr_host_bounce_rays(*b.args(params=api.make_bounce_params(width=0, spp=0))) == 0, lib.rtr_last_error()


@pytest.mark.parametrize("name", ["rtr_bounce_rays", "rtr_bounce_rays_async"])
def test_the_device_calls_check_their_arguments_before_the_context(name):
    """the argument checks need no device: with a null context every refusal still names its own argument, and a call whose arguments
    are in order is refused for the context"""
    lib = A.hip_lib()
    fn = getattr(lib, name)
    b = Buffers()
    for kw, needle in _refusals(b):
        assert fn(None, *b.args(**kw)) == INVALID, kw
        msg = lib.rtr_last_error()
        assert name.encode() + b": " in msg and needle in msg, (kw, msg)
    assert fn(None, *b.args()) == INVALID and b"ctx is null" in lib.rtr_last_error()
    assert b.untouched()


def _two_faults(b):
    """calls with two faults, and the one whose message wins: every null before any misaligned pointer, each in the argument order
    (seeds' alignment after the 16-B ones), the arrays before the params' values, the params in their order, overlaps last"""
    mk = api.make_bounce_params
    return [
        ({"rays": b.rays + 4, "outBounce": 0}, b"outBounce is null"), ({"surfaces": 0, "outRays": 0}, b"surfaces is null"),
        ({"surfaces": b.surfaces + 8, "outRays": b.out_rays + 4}, b"surfaces is not 16-B aligned"),
        ({"outRays": b.out_rays + 4, "seeds": b.seeds + 2}, b"outRays is not 16-B aligned"),
        ({"params": None, "rays": 0}, b"params is null"), ({"params": mk(lobes=0, width=8), "rays": 0}, b"rays is null"),
        ({"params": mk(lobes=0, width=8), "seeds": b.seeds + 2}, b"seeds is not 4-B aligned"),
        ({"params": mk(lobes=0, width=0), "seeds": 0}, b"lobes 0x0"), ({"params": mk(width=0, tmin=float("nan")), "seeds": 0}, b"width 0, spp 1"),
        ({"params": mk(width=8, tmin=2.0, tmax=1.0), "outRays": b.rays}, b"tmax 1 is not above tmin 2"),
        ({"outRays": b.rays, "outBounce": b.out_rays}, b"outRays overlaps rays"),
        ({"outRays": b.surfaces, "outBounce": b.rays}, b"outRays overlaps surfaces"),
    ]


@pytest.mark.parametrize("name", ["rtr_host_bounce_rays", "rtr_bounce_rays", "rtr_bounce_rays_async"])
def test_which_refusal_wins_under_two_faults(name):
    lib = A.hip_lib()
    fn = getattr(lib, name) if "host" in name else (lambda *a: getattr(lib, name)(None, *a))      # a null context: the arrays' faults win
    b = Buffers()
    for kw, needle in _two_faults(b):
        assert fn(*b.args(**kw)) == INVALID, kw
        msg = lib.rtr_last_error()
        assert msg.startswith(name.encode() + b": " + needle), (kw, msg)


def test_host_sincos_turn_names_its_first_null_array():
    lib = A.hip_lib()
    u = np.zeros(4, np.float32)
    for args, needle in (((None, 4, None, None), b"u is null"), ((VP(u.ctypes.data), 4, None, None), b"outSin is null"),
                         ((VP(u.ctypes.data), 4, VP(u.ctypes.data), None), b"outCos is null")):
        assert lib.rtr_host_sincos_turn(*args) == INVALID and lib.rtr_last_error() == b"rtr_host_sincos_turn: " + needle
    assert lib.rtr_host_sincos_turn(None, 0, None, None) == 0


def test_host_bounce_rays_checks_its_arrays():
    rays, sf, seeds = W.make_surfaces(8, seed=2)
    p = api.make_bounce_params()
    for bad in ((rays[:, :7], sf, seeds), (rays.astype(np.float64), sf, seeds), (rays, sf[:, :19], seeds), (rays, sf[:4], seeds),
                (rays, sf, seeds[:4]), (rays, sf, seeds.astype(np.int64))):
        with pytest.raises(ValueError):
            api.host_bounce_rays(bad[0], bad[1], p, bad[2])
    with pytest.raises(api.RtrError):
        api.host_bounce_rays(rays, sf, api.make_bounce_params(lobes=0), seeds)
