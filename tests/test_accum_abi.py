"""The C-ABI surface of rtr_accumulate_paths and rtr_gather_records — what needs no device: the header declares the six entry points and
the struct, the product and the test library export them with C linkage, _abi.py binds them with the header's argument lists, the
struct is 32 bytes with the stated offsets on both sides, the Python signatures are the stated ones, every refusal comes before the
context is looked at with a message that names the function and the argument, and a refused call writes nothing."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
VP, u32 = A.VP, A.u32
ACCUM = ("const RtrRadiance* radiance, const float* throughput, const uint32_t* pathIds, const RtrEmitter* emitters, const RtrSkyEscape* escapes, "
         "const float* skySums, const RtrBounce* bounces, uint32_t numPaths, const rtr_accum_params* params, float* accum, float* outTerm, float* outThroughput")
GATHER = "const void* src, uint32_t recordBytes, uint32_t numSrc, const uint32_t* rows, uint32_t numRows, void* out"


def _expected():
    PP = C.POINTER(A.rtr_accum_params)
    accum = [VP, VP, VP, VP, VP, VP, VP, u32, PP, VP, VP, VP]
    gather = [VP, u32, u32, VP, u32, VP]
    return {
        "rtr_accumulate_paths_async": ("rtr_ctx* ctx, " + ACCUM, [VP] + accum),
        "rtr_accumulate_paths": ("rtr_ctx* ctx, " + ACCUM, [VP] + accum),
        "rtr_host_accumulate_paths": (ACCUM, accum),
        "rtr_gather_records_async": ("rtr_ctx* ctx, " + GATHER, [VP] + gather),
        "rtr_gather_records": ("rtr_ctx* ctx, " + GATHER, [VP] + gather),
        "rtr_host_gather_records": (GATHER, gather),
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
    assert re.search(r"#define\s+RTR_ACCUM_LIGHTS_FROM_EMITTERS\s+1u", text) and re.search(r"#define\s+RTR_ACCUM_MISSES_FROM_ESCAPES\s+2u", text)
    assert (A.ACCUM_LIGHTS_FROM_EMITTERS, A.ACCUM_MISSES_FROM_ESCAPES) == (1, 2)
    assert re.search(r"typedef\s+struct\s+rtr_accum_params\s*\{.*?\}\s*rtr_accum_params\s*;", text, flags=re.S)
    assert "static_assert(sizeof(rtr_accum_params) == 32" in text
    Pm = A.rtr_accum_params
    assert C.sizeof(Pm) == 32
    assert [f[0] for f in Pm._fields_] == ["flags", "numSlots", "throughputStrideBytes", "imageStrideBytes", "_reserved"]
    assert [getattr(Pm, f[0]).offset for f in Pm._fields_] == [0, 4, 8, 12, 16] and Pm._reserved.size == 16
    # the contract's header stands alone: the two headers it names, and the render kernels do not take it
    accum = open(os.path.join(ROOT, "include", "rtr_accum.h")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', accum) == ["rtr_math.h", "rtr_types.h"]
    assert "rtr_accum.h" not in open(os.path.join(ROOT, "realtimeraytracer_amd", "csrc", "kernels", "rtr_device.h")).read()


def test_the_python_signatures():
    p = api.make_accum_params(7)
    assert (p.flags, p.numSlots, p.throughputStrideBytes, p.imageStrideBytes, list(p._reserved)) == (0, 7, 12, 12, [0, 0, 0, 0])
    p = api.make_accum_params(9, lights_from_emitters=True, misses_from_escapes=True, throughput_stride=32, image_stride=16)
    assert (p.flags, p.numSlots, p.throughputStrideBytes, p.imageStrideBytes) == (3, 9, 32, 16)
    assert api.make_accum_params(1, misses_from_escapes=True).flags == A.ACCUM_MISSES_FROM_ESCAPES
    sig = inspect.signature(api.make_accum_params).parameters
    assert list(sig) == ["num_slots", "lights_from_emitters", "misses_from_escapes", "throughput_stride", "image_stride"]
    assert [sig[k].default for k in list(sig)[1:]] == [False, False, 12, 12]
    sig = inspect.signature(api.accumulate_paths).parameters
    assert list(sig) == ["ctx", "radiance", "throughput", "accum", "params", "path_ids", "emitters", "escapes", "sky_sums", "bounces", "out_term", "asynchronous"]
    assert [sig[k].default for k in list(sig)[5:]] == [None, None, None, None, None, None, False]
    sig = inspect.signature(api.gather_records).parameters
    assert list(sig) == ["ctx", "src", "rows", "asynchronous"] and sig["asynchronous"].default is False
    sig = inspect.signature(api.host_accumulate_paths).parameters
    assert list(sig) == ["radiance", "throughput", "accum", "params", "path_ids", "emitters", "escapes", "sky_sums", "bounces", "out_term"]
    assert list(inspect.signature(api.host_gather_records).parameters) == ["src", "rows"]
    sig = inspect.signature(api.path_trace_library).parameters
    power = inspect.signature(api.path_trace_power).parameters
    assert list(sig) == list(power)[:4] + ["loop"] + list(power)[4:]
    assert sig["loop"].default == "power"
    for k in ("sky_samples", "sky_from", "sky_mis", "light_picks", "pick_from"):
        assert sig[k].default is api.LOOP_DEFAULT
    for k in ("seeds", "occlusion", "bounce_cull_mask", "bounce_ray_flags", "max_ray_bytes", "ctx", "compact", "roulette_from", "survival_floor"):
        assert sig[k].default == power[k].default
    # the five loops keep their signatures
    assert list(inspect.signature(api.path_trace).parameters) == ["scene", "rays", "light_params", "bounces", "seeds", "occlusion", "bounce_cull_mask",
                                                                  "bounce_ray_flags", "max_ray_bytes", "ctx", "compact", "roulette_from", "survival_floor"]


def test_path_trace_library_checks_its_keywords():
    with pytest.raises(ValueError, match="loop must be"):
        api.path_trace_library(None, None, None, 1, loop="fast")
    for loop, kw in (("plain", {"light_picks": 1}), ("plain", {"pick_from": 1}), ("plain", {"sky_samples": 1}), ("picked", {"sky_from": 0}), ("mis", {"sky_mis": True}),
                     ("mis", {"sky_samples": 0})):
        with pytest.raises(ValueError, match=f"has no {list(kw)[0]}"):
            api.path_trace_library(None, None, None, 1, loop=loop, **kw)
    with pytest.raises(ValueError, match="needs light_picks"):
        api.path_trace_library(None, None, None, 1, loop="mis", light_picks=None)
    with pytest.raises(ValueError, match="sky_samples"):
        api.path_trace_library(None, None, None, 1, loop="sky", sky_samples=9)
    with pytest.raises(ValueError, match="sky_from"):
        api.path_trace_library(None, None, None, 1, loop="power", sky_from=-1)
    with pytest.raises(ValueError, match="compact"):
        api.path_trace_library(None, None, None, 1, loop="plain", roulette_from=1)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
N = 96
S = 128
PATTERN = 0xA5
SLOT = 8192                # one array per slot of the arena: an output moved onto another array reaches no third one
NAMES = ["radiance", "throughput", "pathIds", "emitters", "escapes", "skySums", "bounces", "accum", "outTerm", "outThroughput", "rows", "out"]


class Buffers:
    """16-B aligned host arrays in one arena, SLOT bytes apart, pre-filled with a pattern (as floats and ids the pattern is as good as
    any data).  The device entry points never get as far as touching them: their argument checks come before the context."""

    def __init__(self):
        self.arena = np.full(len(NAMES) * SLOT + 64, PATTERN, np.uint8)
        base = (self.arena.ctypes.data + 15) & ~15
        for k, name in enumerate(NAMES):
            setattr(self, name, base + k * SLOT)

    def params(self, **kw):
        p = A.rtr_accum_params(kw.pop("flags", 3), kw.pop("numSlots", S), kw.pop("tStride", 32), kw.pop("iStride", 16), (u32 * 4)(0, 0, 0, 0))
        if "reserved" in kw:
            p._reserved[kw.pop("reserved")] = 1
        assert not kw
        return p

    def args(self, **kw):
        a = {name: getattr(self, name) for name in NAMES[:10]}
        a.update({"n": N, "params": self.params()})
        a.update(kw)
        p = a["params"]

        def vp(x):
            return VP(x) if x else None
        return tuple(vp(a[k]) for k in NAMES[:7]) + (a["n"], C.byref(p) if p is not None else None) + tuple(vp(a[k]) for k in NAMES[7:10])

    def gather_args(self, **kw):
        a = {"src": self.radiance, "recordBytes": 48, "numSrc": N, "rows": self.rows, "numRows": N, "out": self.out}
        a.update(kw)
        return (VP(a["src"]) if a["src"] else None, a["recordBytes"], a["numSrc"], VP(a["rows"]) if a["rows"] else None, a["numRows"], VP(a["out"]) if a["out"] else None)

    def untouched(self):
        return bool((self.arena == PATTERN).all())


def _refusals(b):
    P = b.params
    return [
        ({"radiance": 0}, b"radiance is null"), ({"throughput": 0}, b"throughput is null"), ({"accum": 0}, b"accum is null"), ({"params": None}, b"params is null"),
        ({"outThroughput": 0}, b"bounces without outThroughput"), ({"bounces": 0}, b"outThroughput without bounces"),
        ({"radiance": b.radiance + 4}, b"radiance is not 16-B aligned"), ({"emitters": b.emitters + 8}, b"emitters is not 16-B aligned"),
        ({"escapes": b.escapes + 4}, b"escapes is not 16-B aligned"), ({"skySums": b.skySums + 12}, b"skySums is not 16-B aligned"),
        ({"bounces": b.bounces + 8}, b"bounces is not 16-B aligned"), ({"throughput": b.throughput + 2}, b"throughput is not 4-B aligned"),
        ({"pathIds": b.pathIds + 1}, b"pathIds is not 4-B aligned"), ({"accum": b.accum + 2}, b"accum is not 4-B aligned"),
        ({"outTerm": b.outTerm + 3}, b"outTerm is not 4-B aligned"), ({"outThroughput": b.outThroughput + 2}, b"outThroughput is not 4-B aligned"),
        ({"params": P(tStride=8)}, b"throughputStrideBytes 8"), ({"params": P(tStride=0)}, b"throughputStrideBytes 0"), ({"params": P(tStride=14)}, b"throughputStrideBytes 14"),
        ({"params": P(iStride=8)}, b"imageStrideBytes 8"), ({"params": P(iStride=13)}, b"imageStrideBytes 13"), ({"params": P(iStride=0)}, b"imageStrideBytes 0"),
        ({"params": P(flags=4)}, b"flags 0x4"), ({"params": P(flags=7)}, b"flags 0x7"), ({"params": P(flags=0x80000000)}, b"flags 0x80000000"),
        ({"params": P(reserved=0)}, b"_reserved"), ({"params": P(reserved=3)}, b"_reserved"),
        ({"params": P(numSlots=0)}, b"numSlots is 0"),
        ({"params": P(numSlots=0xffffffff, iStride=0xfffffffc)}, b"accum: numSlots 4294967295 x imageStrideBytes 4294967292 does not fit"),
        ({"params": P(tStride=0xfffffffc), "n": 0xffffffff}, b"throughput: 4294967295 rows of stride 4294967292 do not fit"),
        ({"accum": b.radiance + 16}, b"accum overlaps radiance"), ({"accum": b.throughput + 32 * (N - 1) + 8}, b"accum overlaps throughput"),
        ({"outTerm": b.pathIds + 4 * (N - 1)}, b"outTerm overlaps pathIds"), ({"accum": b.emitters}, b"accum overlaps emitters"),
        ({"outTerm": b.escapes + 32 * (N - 1) + 28}, b"outTerm overlaps escapes"), ({"accum": b.skySums + 16 * (N - 1)}, b"accum overlaps skySums"),
        ({"outThroughput": b.bounces + 32}, b"outThroughput overlaps bounces"), ({"outTerm": b.accum + 16 * (S - 1) + 8}, b"accum overlaps outTerm"),
        ({"outThroughput": b.accum}, b"accum overlaps outThroughput"), ({"outThroughput": b.outTerm + 16 * (S - 1) + 8}, b"outTerm overlaps outThroughput"),
        # the in-place throughput is the packed input itself: the same address at another stride, or any other overlap, is refused
        ({"outThroughput": b.throughput}, b"outThroughput overlaps throughput"),
        ({"outThroughput": b.throughput + 12, "params": P(tStride=12)}, b"outThroughput overlaps throughput"),
        ({"outThroughput": b.throughput - 12 * (N - 1) - 8, "params": P(tStride=12)}, b"outThroughput overlaps throughput"),
    ]


def _gather_refusals(b):
    return [
        ({"recordBytes": 0}, b"recordBytes 0"), ({"recordBytes": 6}, b"recordBytes 6"), ({"recordBytes": 260}, b"recordBytes 260"), ({"recordBytes": 0xfffffffc}, b"recordBytes"),
        ({"src": 0}, b"src is null"), ({"rows": 0}, b"rows is null"), ({"out": 0}, b"out is null"),
        ({"src": b.radiance + 2}, b"src is not 4-B aligned"), ({"rows": b.rows + 1}, b"rows is not 4-B aligned"), ({"out": b.out + 3}, b"out is not 4-B aligned"),
        ({"out": b.radiance + 48 * (N - 1) + 44}, b"out overlaps src"), ({"out": b.rows + 4 * (N - 1)}, b"out overlaps rows"), ({"out": b.rows - 48 * N + 4}, b"out overlaps rows"),
    ]


def test_the_host_calls_refuse_and_write_nothing():
    lib = A.hip_lib()
    b = Buffers()
    for kw, needle in _refusals(b):
        assert lib.rtr_host_accumulate_paths(*b.args(**kw)) == INVALID, kw
        msg = lib.rtr_last_error()
        assert msg.startswith(b"rtr_host_accumulate_paths: ") and needle in msg, (kw, msg)
        assert b.untouched(), f"a refused call wrote: {kw}"
    for kw, needle in _gather_refusals(b):
        assert lib.rtr_host_gather_records(*b.gather_args(**kw)) == INVALID, kw
        msg = lib.rtr_last_error()
        assert msg.startswith(b"rtr_host_gather_records: ") and needle in msg, (kw, msg)
        assert b.untouched(), f"a refused call wrote: {kw}"
    # what is allowed: the in-place throughput at stride 12, src NULL with numSrc 0, adjacent arrays
    assert lib.rtr_host_gather_records(*b.gather_args(src=0, numSrc=0)) == 0, lib.rtr_last_error()
    assert not (b.arena[b.out - b.arena.ctypes.data:][:48 * N] != 0).any()
    assert lib.rtr_host_gather_records(*b.gather_args(out=b.rows + 4 * N)) == 0, lib.rtr_last_error()
    b = Buffers()
    b.arena[:] = 0
    assert lib.rtr_host_accumulate_paths(*b.args(pathIds=0, outThroughput=b.throughput, params=b.params(tStride=12))) == 0, lib.rtr_last_error()
    assert lib.rtr_host_accumulate_paths(*b.args(pathIds=0, outThroughput=b.throughput + 12 * N, params=b.params(tStride=12))) == 0, lib.rtr_last_error()


@pytest.mark.parametrize("name", ["rtr_accumulate_paths", "rtr_accumulate_paths_async"])
def test_the_device_accumulation_checks_its_arguments_before_the_context(name):
    lib = A.hip_lib()
    fn = getattr(lib, name)
    b = Buffers()
    for kw, needle in _refusals(b):
        assert fn(None, *b.args(**kw)) == INVALID, kw
        msg = lib.rtr_last_error()
        assert msg.startswith(name.encode() + b": ") and needle in msg, (kw, msg)
    assert fn(None, *b.args()) == INVALID and b"ctx is null" in lib.rtr_last_error()
    assert fn(None, *b.args(n=0)) == INVALID and b"ctx is null" in lib.rtr_last_error()
    assert b.untouched()


@pytest.mark.parametrize("name", ["rtr_gather_records", "rtr_gather_records_async"])
def test_the_device_gather_checks_its_arguments_before_the_context(name):
    lib = A.hip_lib()
    fn = getattr(lib, name)
    b = Buffers()
    for kw, needle in _gather_refusals(b):
        assert fn(None, *b.gather_args(**kw)) == INVALID, kw
        msg = lib.rtr_last_error()
        assert msg.startswith(name.encode() + b": ") and needle in msg, (kw, msg)
    assert fn(None, *b.gather_args()) == INVALID and b"ctx is null" in lib.rtr_last_error()
    assert fn(None, *b.gather_args(numRows=0)) == INVALID and b"ctx is null" in lib.rtr_last_error()
    assert b.untouched()


def test_the_python_host_forms_check_their_arrays():
    rad, T, acc = np.zeros((8, 12), np.float32), np.ones((8, 3), np.float32), np.zeros((8, 3), np.float32)
    p = api.make_accum_params(8)
    for bad in ((rad[:, :11], T, acc), (rad, T[:, :2], acc), (rad, T[:4], acc), (rad, T.astype(np.float64), acc), (rad, T, acc[:4]), (rad, T, np.zeros((8, 5), np.float32))):
        with pytest.raises(ValueError):
            api.host_accumulate_paths(bad[0], bad[1], bad[2], p)
    with pytest.raises(ValueError):
        api.host_accumulate_paths(rad, T, acc, p, path_ids=np.zeros(4, np.int32))
    with pytest.raises(ValueError):
        api.host_accumulate_paths(rad, T, acc, p, bounces=np.zeros((4, 8), np.float32))
    with pytest.raises(ValueError):
        api.host_accumulate_paths(rad, T, acc, p, out_term=np.zeros((8, 4), np.float32))
    with pytest.raises(ValueError):
        api.host_gather_records(np.zeros((4, 65), np.float32), np.zeros(2, np.int32))
    with pytest.raises(ValueError):
        api.host_gather_records(np.zeros((4, 3), np.float32), np.zeros(2, np.int64))
