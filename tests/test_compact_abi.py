"""The C-ABI surface of rtr_compact_paths — what needs no device: the header declares the four entry points and the struct, the product
and the test library export them with C linkage, _abi.py binds them with the header's argument lists, the struct is 32 bytes with the
stated offsets on both sides, rtr_compact_scratch_bytes is the arithmetic it is said to be, every refusal comes with a message that
names the function and the argument, and a refused call writes nothing."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import compact_witness as W
from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
VP, u32 = A.VP, A.u32
INPUTS = "const RtrRay* rays, const float* throughput, const uint32_t* seeds, const uint32_t* pathIds, uint32_t numPaths, const rtr_compact_params* params"
OUTPUTS = "RtrRay* outRays, float* outThroughput, uint32_t* outSeeds, uint32_t* outPathIds, uint32_t* outCount"
DEVICE_PARAMS = "rtr_ctx* ctx, " + INPUTS + ", void* scratch, size_t scratchBytes, " + OUTPUTS


def _expected():
    PP = C.POINTER(A.rtr_compact_params)
    dev = [VP, VP, VP, VP, VP, u32, PP, VP, C.c_size_t, VP, VP, VP, VP, VP]
    return {
        "rtr_compact_scratch_bytes": ("uint32_t numPaths, size_t* bytes", [u32, C.POINTER(C.c_size_t)]),
        "rtr_compact_paths_async": (DEVICE_PARAMS, dev),
        "rtr_compact_paths": (DEVICE_PARAMS + ", uint32_t* hostCount", dev + [C.POINTER(u32)]),
        "rtr_host_compact_paths": (INPUTS + ", " + OUTPUTS, [VP, VP, VP, VP, u32, PP, VP, VP, VP, VP, C.POINTER(u32)]),
    }


def _text(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def _norm(params):
    return [re.sub(r"\s+", " ", p).strip() for p in params.split(",")]


def test_the_entry_points_are_declared_exported_and_bound():
    text = _text("rtr.h")
    expected = _expected()
    for path in (A.LIB_HIP_PATH, A.LIB_HIP_HOOKS_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        for n in expected:
            assert n in exported, f"{os.path.basename(path)} does not export {n} with C linkage"
    for n, (params, argtypes) in expected.items():
        m = re.search(r"\bint\s+" + n + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{n} is not declared in include/rtr.h"
        assert _norm(m.group(1)) == _norm(params), f"{n}: the header's parameters are {_norm(m.group(1))}"
        res, args = A.RTR_SYMBOLS[n]
        assert res is C.c_int and list(args) == argtypes, f"{n}: bound as {args}"
    assert A.hip_lib().rtr_abi_version() == 3 and re.search(r"#define\s+RTR_ABI_VERSION\s+3\b", open(os.path.join(ROOT, "include", "rtr.h")).read())


def test_the_struct_and_the_constants():
    text = _text("rtr_types.h")
    assert re.search(r"#define\s+RTR_COMPACT_ROULETTE\s+1u", text) and re.search(r"#define\s+RTR_PATH_NONE\s+0xffffffffu", text)
    assert (A.COMPACT_ROULETTE, A.PATH_NONE) == (1, 0xffffffff)
    assert re.search(r"typedef\s+struct\s+rtr_compact_params\s*\{.*?\}\s*rtr_compact_params\s*;", text, flags=re.S)
    assert "static_assert(sizeof(rtr_compact_params) == 32" in text
    Pm = A.rtr_compact_params
    assert C.sizeof(Pm) == 32
    assert [f[0] for f in Pm._fields_] == ["frame", "depth", "flags", "survivalFloor", "throughputStrideBytes", "_reserved"]
    assert [getattr(Pm, f[0]).offset for f in Pm._fields_] == [0, 4, 8, 12, 16, 20]
    assert Pm.survivalFloor.size == 4 and Pm._reserved.size == 12
    # the contract's header stands alone: the two headers it names, and the render kernels do not take it
    paths = open(os.path.join(ROOT, "include", "rtr_paths.h")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', paths) == ["rtr_math.h", "rtr_types.h"]
    assert "rtr_paths.h" not in open(os.path.join(ROOT, "realtimeraytracer_amd", "csrc", "kernels", "rtr_device.h")).read()
    assert re.search(r"\bint\s+rtr_path_survive\s*\(\s*const RtrRay\*\s*\w+,\s*const float \w+\[3\],\s*uint32_t \w+,\s*const rtr_compact_params\*\s*\w+,\s*float \w+\[3\]\s*\)", paths)


def test_the_python_signatures():
    p = api.make_compact_params()
    assert (p.frame, p.depth, p.flags, p.throughputStrideBytes, list(p._reserved)) == (0, 0, 0, 12, [0, 0, 0]) and p.survivalFloor == np.float32(0.05)
    p = api.make_compact_params(frame=2 ** 32 + 5, depth=3, roulette=True, survival_floor=0.25, throughput_stride=32)
    assert (p.frame, p.depth, p.flags, p.survivalFloor, p.throughputStrideBytes) == (5, 3, A.COMPACT_ROULETTE, 0.25, 32)
    sig = inspect.signature(api.make_compact_params).parameters
    assert list(sig) == ["frame", "depth", "roulette", "survival_floor", "throughput_stride"]
    assert [sig[k].default for k in sig] == [0, 0, False, 0.05, 12]
    sig = inspect.signature(api.compact_paths).parameters
    assert list(sig) == ["ctx", "rays", "throughput", "seeds", "path_ids", "params", "asynchronous"]
    assert [sig[k].default for k in list(sig)[3:]] == [None, None, None, False]
    sig = inspect.signature(api.host_compact_paths).parameters
    assert list(sig) == ["rays", "throughput", "seeds", "path_ids", "params"]
    sig = inspect.signature(api.path_trace).parameters
    assert list(sig) == ["scene", "rays", "light_params", "bounces", "seeds", "occlusion", "bounce_cull_mask", "bounce_ray_flags", "max_ray_bytes", "ctx",
                         "compact", "roulette_from", "survival_floor"]
    assert sig["occlusion"].default == "dense" and sig["bounce_cull_mask"].default is None and sig["bounce_ray_flags"].default == 0
    assert sig["max_ray_bytes"].default == 256 << 20 and sig["seeds"].default is None and sig["ctx"].default is None
    assert (sig["compact"].default, sig["roulette_from"].default, sig["survival_floor"].default) == (False, None, 0.05)
    for f in ("rays", "throughput", "seeds", "path_ids", "count_tensor", "count"):
        assert hasattr(api.CompactResult, f)
    assert api.PathResult.live is None


def test_roulette_from_needs_compact():
    with pytest.raises(ValueError, match="compact"):
        api.path_trace(None, None, None, 1, roulette_from=1)


def test_scratch_bytes_is_arithmetic():
    lib = A.hip_lib()
    assert lib.rtr_compact_scratch_bytes(100, None) == INVALID and b"rtr_compact_scratch_bytes: bytes is null" in lib.rtr_last_error()
    last = 0
    sweep = list(range(0, 2100)) + [2 ** k + d for k in range(12, 32) for d in (-1, 0, 1)] + [2 ** 32 - 257, 2 ** 32 - 256, 2 ** 32 - 255, 2 ** 32 - 1]
    for n in sweep:
        b = C.c_size_t(12345)
        assert lib.rtr_compact_scratch_bytes(n, C.byref(b)) == 0
        assert b.value % 16 == 0 and b.value >= last, (n, b.value, last)
        # room for one bit per path and one 32-bit total per 256 paths
        assert b.value >= (n + 7) // 8 + 4 * ((n + 255) // 256)
        last = b.value
        assert api.compact_scratch_bytes(lib, n) == b.value
    assert last < 2 ** 32 - 1             # and no more than about a byte per path


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
N = 96
PATTERN = 0xA5


SLOT = 8192                # one array per slot of the arena: an output moved onto another array reaches no third one


class Buffers:
    """16-B aligned host arrays of N paths in one arena, SLOT bytes apart — rays, a stride-32 throughput, seeds, ids — then the outputs, the
    count and the scratch, pre-filled with a pattern.  The device entry points never get as far as touching them: their argument checks
    come before the context."""

    def __init__(self):
        ins = W.make_paths(N, "random_half", stride_words=8)[:4]
        self.scratch_bytes = api.compact_scratch_bytes(A.hip_lib(), N)
        self.arena = np.full(10 * SLOT + 64, PATTERN, np.uint8)
        base = (self.arena.ctypes.data + 15) & ~15
        self.addr = [base + k * SLOT for k in range(10)]
        for k, x in enumerate(ins):
            assert x.nbytes <= SLOT // 2
            C.memmove(self.addr[k], x.ctypes.data, x.nbytes)
        (self.rays, self.throughput, self.seeds, self.ids, self.out_rays, self.out_t, self.out_seeds, self.out_ids, self.out_count, self.scratch) = self.addr
        self.first_out = self.out_rays - self.arena.ctypes.data

    def region(self, addr, nbytes):
        o = addr - self.arena.ctypes.data
        return self.arena[o:o + nbytes]

    def args(self, device, **kw):
        a = {"rays": self.rays, "throughput": self.throughput, "seeds": self.seeds, "pathIds": self.ids, "n": N,
             "params": api.make_compact_params(throughput_stride=32), "scratch": self.scratch, "scratchBytes": self.scratch_bytes,
             "outRays": self.out_rays, "outThroughput": self.out_t, "outSeeds": self.out_seeds, "outPathIds": self.out_ids, "outCount": self.out_count}
        a.update(kw)
        p = a["params"]

        def vp(x):
            return VP(x) if x else None
        ins = (vp(a["rays"]), vp(a["throughput"]), vp(a["seeds"]), vp(a["pathIds"]), a["n"], C.byref(p) if p is not None else None)
        outs = (vp(a["outRays"]), vp(a["outThroughput"]), vp(a["outSeeds"]), vp(a["outPathIds"]), vp(a["outCount"]))
        if device:
            return ins + (vp(a["scratch"]), a["scratchBytes"]) + outs
        return ins + outs[:4] + (C.cast(outs[4], C.POINTER(u32)) if outs[4] else None,)

    def untouched(self):
        return bool((self.arena[self.first_out:] == PATTERN).all())


def _params(**kw):
    stride = kw.pop("stride", 32)
    reserved = kw.pop("reserved", None)
    flags = kw.pop("flags", None)
    p = api.make_compact_params(throughput_stride=stride, **kw)
    if reserved is not None:
        p._reserved[reserved] = 1
    if flags is not None:
        p.flags = flags
    return p


def _refusals(b, device):
    nan = float("nan")
    r = [
        ({"rays": 0}, b"rays is null"), ({"throughput": 0}, b"throughput is null"), ({"outRays": 0}, b"outRays is null"),
        ({"outThroughput": 0}, b"outThroughput is null"), ({"outSeeds": 0}, b"outSeeds is null"), ({"outPathIds": 0}, b"outPathIds is null"),
        ({"outCount": 0}, b"outCount is null"), ({"params": None}, b"params is null"),
        ({"seeds": 0}, b"outSeeds without seeds"),
        ({"rays": b.rays + 4}, b"rays is not 16-B aligned"), ({"outRays": b.out_rays + 8}, b"outRays is not 16-B aligned"),
        ({"throughput": b.throughput + 2}, b"throughput is not 4-B aligned"), ({"outThroughput": b.out_t + 1}, b"outThroughput is not 4-B aligned"),
        ({"seeds": b.seeds + 2}, b"seeds is not 4-B aligned"), ({"pathIds": b.ids + 3}, b"pathIds is not 4-B aligned"),
        ({"outSeeds": b.out_seeds + 2}, b"outSeeds is not 4-B aligned"), ({"outPathIds": b.out_ids + 2}, b"outPathIds is not 4-B aligned"),
        ({"outCount": b.out_count + 2}, b"outCount is not 4-B aligned"),
        ({"params": _params(stride=8)}, b"throughputStrideBytes"), ({"params": _params(stride=0)}, b"throughputStrideBytes"),
        ({"params": _params(stride=14)}, b"throughputStrideBytes"), ({"params": _params(stride=33)}, b"throughputStrideBytes"),
        ({"params": _params(flags=2)}, b"flags"), ({"params": _params(flags=3)}, b"flags"), ({"params": _params(flags=0x80000000)}, b"flags"),
        ({"params": _params(roulette=True), "seeds": 0, "outSeeds": 0}, b"RTR_COMPACT_ROULETTE needs seeds"),
        ({"params": _params(roulette=True, survival_floor=0.0)}, b"survivalFloor"), ({"params": _params(roulette=True, survival_floor=-0.5)}, b"survivalFloor"),
        ({"params": _params(roulette=True, survival_floor=1.0000001)}, b"survivalFloor"), ({"params": _params(roulette=True, survival_floor=nan)}, b"survivalFloor"),
        ({"params": _params(reserved=0)}, b"_reserved"), ({"params": _params(reserved=1)}, b"_reserved"), ({"params": _params(reserved=2)}, b"_reserved"),
        ({"outRays": b.rays}, b"outRays overlaps rays"), ({"outRays": b.rays + 32 * (N - 1)}, b"outRays overlaps rays"),
        ({"outThroughput": b.throughput + 32 * (N - 1) + 8}, b"outThroughput overlaps throughput"),
        ({"outSeeds": b.seeds + 4 * (N // 2)}, b"outSeeds overlaps seeds"), ({"outPathIds": b.ids}, b"outPathIds overlaps pathIds"),
        ({"outCount": b.seeds + 4 * (N - 1)}, b"outCount overlaps seeds"), ({"outPathIds": b.rays + 16}, b"outPathIds overlaps rays"),
        ({"outThroughput": b.out_rays + 32 * (N - 1) + 28}, b"outRays overlaps outThroughput"),
        ({"outSeeds": b.out_t + 12 * N - 4}, b"outThroughput overlaps outSeeds"), ({"outPathIds": b.out_seeds + 4 * (N - 1)}, b"outSeeds overlaps outPathIds"),
        ({"outCount": b.out_ids + 4 * (N - 1)}, b"outPathIds overlaps outCount"), ({"outCount": b.out_rays + 16}, b"outRays overlaps outCount"),
    ]
    if device:
        r += [({"scratch": 0}, b"scratch is null"), ({"scratch": b.scratch + 8}, b"scratch is not 16-B aligned"),
              ({"scratchBytes": b.scratch_bytes - 1}, b"scratchBytes"), ({"scratchBytes": 0}, b"scratchBytes"),
              ({"scratch": b.rays + 16 * 7}, b"scratch overlaps rays"), ({"scratch": b.out_ids + 4 * (N - 4)}, b"outPathIds overlaps scratch"),
              ({"outCount": b.scratch + b.scratch_bytes - 4}, b"outCount overlaps scratch")]
    return r


def test_the_host_call_refuses_and_writes_nothing():
    lib = A.hip_lib()
    b = Buffers()
    for kw, needle in _refusals(b, False):
        assert lib.rtr_host_compact_paths(*b.args(False, **kw)) == INVALID, kw
        msg = lib.rtr_last_error()
        assert b"rtr_host_compact_paths: " in msg and needle in msg, (kw, msg)
        assert b.untouched(), f"a refused call wrote to its outputs: {kw}"
    # survivalFloor is read only with the flag; seeds may be absent without it
    assert lib.rtr_host_compact_paths(*b.args(False, params=_params(survival_floor=float("nan")), seeds=0, outSeeds=0)) == 0, lib.rtr_last_error()
    assert (b.region(b.out_seeds, 4 * N) == PATTERN).all() and (b.region(b.scratch, b.scratch_bytes) == PATTERN).all()
    assert not (b.region(b.out_rays, 32 * N) == PATTERN).all() and not (b.region(b.out_count, 4) == PATTERN).all()
    assert (b.region(b.out_rays + 32 * N, SLOT - 32 * N) == PATTERN).all() and (b.region(b.out_t + 12 * N, SLOT - 12 * N) == PATTERN).all()
    assert lib.rtr_host_compact_paths(*b.args(False, params=_params(roulette=True, survival_floor=1.0))) == 0, lib.rtr_last_error()
    # numPaths == 0 writes the count and nothing else, whatever else is passed
    cnt = u32(77)
    assert lib.rtr_host_compact_paths(None, None, None, None, 0, None, None, None, None, None, C.byref(cnt)) == 0 and cnt.value == 0
    assert lib.rtr_host_compact_paths(None, None, None, None, 0, None, None, None, None, None, None) == 0


@pytest.mark.parametrize("name", ["rtr_compact_paths", "rtr_compact_paths_async"])
def test_the_device_calls_check_their_arguments_before_the_context(name):
    """the argument checks need no device: with a null context every refusal still names its own argument, and a call whose arguments
    are in order is refused for the context"""
    lib = A.hip_lib()
    fn = getattr(lib, name)
    extra = (None,) if name == "rtr_compact_paths" else ()
    b = Buffers()
    for kw, needle in _refusals(b, True):
        assert fn(None, *b.args(True, **kw), *extra) == INVALID, kw
        msg = lib.rtr_last_error()
        assert name.encode() + b": " in msg and needle in msg, (kw, msg)
    assert fn(None, *b.args(True), *extra) == INVALID and b"ctx is null" in lib.rtr_last_error()
    assert fn(None, *b.args(True, n=0), *extra) == INVALID and b"ctx is null" in lib.rtr_last_error()
    assert b.untouched()


def _two_faults(b, device):
    """calls with two faults, and the one whose message wins: every null before any misaligned pointer, each in the argument order
    (the scratch last), the arrays before the params' values, the params in their order, overlaps last and per output"""
    r = [
        ({"rays": b.rays + 4, "outCount": 0}, b"outCount is null"), ({"throughput": 0, "outRays": 0}, b"throughput is null"),
        ({"seeds": b.seeds + 2, "outRays": b.out_rays + 8}, b"seeds is not 4-B aligned"),
        ({"outThroughput": b.out_t + 1, "outCount": b.out_count + 2}, b"outThroughput is not 4-B aligned"),
        ({"params": None, "rays": 0}, b"params is null"), ({"params": _params(stride=8), "outRays": b.out_rays + 8}, b"outRays is not 16-B aligned"),
        ({"seeds": 0, "rays": b.rays + 4}, b"rays is not 16-B aligned"), ({"seeds": 0, "params": _params(stride=8)}, b"outSeeds without seeds"),
        ({"params": _params(stride=8, flags=2)}, b"throughputStrideBytes 8"), ({"params": _params(flags=2, reserved=0)}, b"flags 0x2"),
        ({"params": _params(roulette=True, survival_floor=0.0, reserved=1)}, b"survivalFloor 0"),
        ({"params": _params(reserved=0), "outRays": b.rays}, b"_reserved words of params are not 0"),
        ({"outRays": b.rays, "outPathIds": b.ids}, b"outRays overlaps rays"),
        ({"outPathIds": b.ids, "outCount": b.out_rays + 16}, b"outPathIds overlaps pathIds"),
        ({"outThroughput": b.out_rays + 32 * (N - 1) + 28, "outCount": b.seeds}, b"outRays overlaps outThroughput"),
    ]
    if device:
        r += [({"rays": b.rays + 4, "scratch": 0}, b"scratch is null"), ({"outCount": b.out_count + 2, "scratch": b.scratch + 8}, b"outCount is not 4-B aligned"),
              ({"scratchBytes": 0, "params": _params(stride=8)}, b"scratchBytes 0"), ({"scratchBytes": 0, "seeds": 0}, b"outSeeds without seeds"),
              ({"scratch": b.rays + 16 * 7, "outCount": b.seeds}, b"outCount overlaps seeds")]
    return r


@pytest.mark.parametrize("name", ["rtr_host_compact_paths", "rtr_compact_paths", "rtr_compact_paths_async"])
def test_which_refusal_wins_under_two_faults(name):
    lib = A.hip_lib()
    device = "host" not in name
    extra = (None,) if name == "rtr_compact_paths" else ()
    fn = (lambda *a: getattr(lib, name)(None, *a, *extra)) if device else getattr(lib, name)      # a null context: the arrays' faults win
    b = Buffers()
    for kw, needle in _two_faults(b, device):
        assert fn(*b.args(device, **kw)) == INVALID, kw
        msg = lib.rtr_last_error()
        assert msg.startswith(name.encode() + b": " + needle), (kw, msg)
    assert b.untouched()


def test_host_compact_paths_checks_its_arrays():
    rays, thr, seeds, ids, _ = W.make_paths(8, "random_half")
    for bad in ((rays[:, :7], thr, seeds, ids), (rays.astype(np.float64), thr, seeds, ids), (rays, thr[:, :2], seeds, ids), (rays, thr[:4], seeds, ids),
                (rays, thr, seeds[:4], ids), (rays, thr, seeds.astype(np.int64), ids), (rays, thr, seeds, ids[:3])):
        with pytest.raises(ValueError):
            api.host_compact_paths(bad[0], bad[1], bad[2], bad[3])
    with pytest.raises(api.RtrError):
        api.host_compact_paths(rays, thr, None, ids, api.make_compact_params(roulette=True))
    with pytest.raises(api.RtrError):
        api.host_compact_paths(rays, thr, seeds, ids, api.make_compact_params(roulette=True, survival_floor=2.0))
