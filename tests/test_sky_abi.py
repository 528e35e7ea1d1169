"""The sky calls' C-ABI surface (include/rtr.h, rtr_types.h, rtr_sky.h): the layouts of rtr_sky_params, RtrSkySample and RtrSkyEscape,
the entry points in the product library and its test build, and every refusal that needs no device, by message.  No GPU needed: the
device calls below are all refused before a handle is looked at, so host buffers stand in for the device arrays."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = ("rtr_sky_rays_async", "rtr_sky_rays", "rtr_shade_sky_async", "rtr_shade_sky", "rtr_sky_hits_async", "rtr_sky_hits")
NEW = DEVICE + ("rtr_scene_prepare_sky", "rtr_scene_export_sky_table", "rtr_host_sky_table", "rtr_host_sky_rays", "rtr_host_sky_hits",
                "rtr_host_sky_pdf", "rtr_host_sky_radiance")
INVALID = -1
N, S = 4, 2
SKY = (0.2, 0.5, 0.9)


def test_struct_layouts():
    text = open(os.path.join(ROOT, "include", "rtr_types.h")).read()
    for T, fields in ((A.rtr_sky_params, [("numSamples", 0), ("depth", 4), ("frame", 8), ("width", 12), ("spp", 16), ("lobes", 20), ("flags", 24), ("_reserved", 28)]),
                      (A.RtrSkySample, [("contrib", 0), ("skyPdf", 12), ("bouncePdf", 16), ("wSky", 20), ("cell", 24), ("_r", 28)]),
                      (A.RtrSkyEscape, [("radiance", 0), ("wBounce", 12), ("skyPdf", 16), ("bouncePdf", 20), ("cell", 24), ("kind", 28)])):
        assert C.sizeof(T) == 32
        assert [(n, getattr(T, n).offset) for n, _ in T._fields_] == fields
        assert f"static_assert(sizeof({T.__name__}) == 32" in text
    assert "#define RTR_SKY_MAX_SAMPLES 8u" in text and "#define RTR_SKY_MIS         1u" in text
    assert (A.SKY_MAX_SAMPLES, A.SKY_MIS) == (8, 1)
    p = api.make_sky_params()
    assert (p.numSamples, p.depth, p.frame, p.width, p.spp, p.lobes, p.flags, p._reserved) == (1, 0, 0, 0, 1, A.BOUNCE_DIFFUSE | A.BOUNCE_SPECULAR, A.SKY_MIS, 0)
    p = api.make_sky_params(samples=3, depth=2, frame=7, width=9, spp=4, lobes=A.BOUNCE_DIFFUSE, mis=False)
    assert (p.numSamples, p.depth, p.frame, p.width, p.spp, p.lobes, p.flags, p._reserved) == (3, 2, 7, 9, 4, A.BOUNCE_DIFFUSE, 0, 0)


def test_abi_version_unchanged_and_header_stands_alone():
    assert A.hip_lib().rtr_abi_version() == 3
    text = open(os.path.join(ROOT, "include", "rtr_sky.h")).read()
    assert set(re.findall(r'#include "([^"]+)"', text)) == {"rtr_math.h", "rtr_types.h", "rtr_bounce.h", "rtr_mis.h"}
    kernels = os.path.join(ROOT, "realtimeraytracer_amd", "csrc", "kernels")
    for name in ("rtr_device.h", "rtr_kernels.hip", "rtr_query.hip", "rtr_occlusion.hip"):
        assert "rtr_sky" not in open(os.path.join(kernels, name)).read(), name


def test_sky_symbols_are_exported():
    text = open(os.path.join(ROOT, "include", "rtr.h")).read()
    for lib in (C.CDLL(A.LIB_HIP_PATH), C.CDLL(A.LIB_HIP_HOOKS_PATH)):
        for n in NEW:
            assert hasattr(lib, n), n
            assert n in A.RTR_SYMBOLS
            assert re.search(r"\b%s\(" % n, text), n
    for n in ("rtr_sky_rays", "rtr_shade_sky", "rtr_sky_hits"):
        assert A.RTR_SYMBOLS[n] == A.RTR_SYMBOLS[n + "_async"]
    for n in ("Scene.prepare_sky", "Scene.export_sky_table", "make_sky_params", "sky_rays", "shade_sky", "sky_hits", "host_sky_table", "host_sky_rays",
              "host_sky_hits", "host_sky_pdf", "host_sky_radiance", "path_trace_sky", "SkyResult", "SkyEscapeResult"):
        obj = api
        for part in n.split("."):
            obj = getattr(obj, part)


def aligned(shape, dtype, fill=0):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    buf = np.full(n + 16, fill, np.uint8)
    off = (-buf.ctypes.data) % 16
    return buf[off:off + n].view(dtype).reshape(shape)


def ptr(x, off=0):
    return None if x is None else C.c_void_p(x.ctypes.data + off)


class Call:
    """one call of each entry point over host buffers of N hits and S samples, any argument replaceable; the outputs are pre-filled"""
    def __init__(self):
        self.rays, self.surf = aligned((N, 8), np.float32), aligned((N, 20), np.float32)
        self.hits, self.bounce = aligned((N, 8), np.int32), aligned((N, 8), np.float32)
        self.seeds = np.zeros(N, np.uint32)
        self.out_rays, self.out_samples = aligned((N * S, 8), np.float32, 0xA5), aligned((N * S, 8), np.float32, 0xA5)
        self.occ = np.zeros(N * S, np.uint8)
        self.out, self.esc = aligned((N, 4), np.float32, 0xA5), aligned((N, 8), np.float32, 0xA5)
        self.params = api.make_sky_params(samples=S, width=2, spp=1)
        self.table = api.host_sky_table(None, SKY)
        self.sky = np.array(SKY, np.float32)

    def outputs(self):
        return b"".join(x.tobytes() for x in (self.out_rays, self.out_samples, self.out, self.esc))

    def head(self, name):
        if "host" not in name:
            return (None,) if "shade" in name else (None, None)          # ctx, scene
        self._t = self.table._c()
        return (None, ptr(self.sky), C.byref(self._t))

    def run(self, lib, name, n=N, **kw):
        a = dict(rays=ptr(self.rays), surf=ptr(self.surf), hits=ptr(self.hits), bounce=ptr(self.bounce), params=C.byref(self.params), seeds=None,
                 out_rays=ptr(self.out_rays), out_samples=ptr(self.out_samples), samples=ptr(self.out_samples), occ=ptr(self.occ), out=ptr(self.out),
                 esc=ptr(self.esc), num_samples=S)
        a.update(kw)
        fn = getattr(lib, name)
        if "sky_rays" in name:
            return fn(*self.head(name), a["rays"], a["surf"], n, a["params"], a["seeds"], a["out_rays"], a["out_samples"])
        if "shade" in name:
            return fn(*self.head(name), a["samples"], a["occ"], n, a["num_samples"], a["out"])
        return fn(*self.head(name), a["rays"], a["hits"], a["surf"], a["bounce"], n, a["params"], a["esc"])


@pytest.mark.parametrize("name", DEVICE + ("rtr_host_sky_rays", "rtr_host_sky_hits"))
def test_refusals_by_message(name):
    lib = A.hip_lib()
    rays_call, shade, hits_call = "sky_rays" in name, "shade" in name, "sky_hits" in name

    def refused(needle, c=None, **kw):
        c = c or Call()
        before = c.outputs()
        assert c.run(lib, name, **kw) == INVALID, needle
        msg = lib.rtr_last_error().decode()
        assert msg.startswith(name + ": ") and needle in msg, (needle, msg)
        assert c.outputs() == before, needle          # a refused call writes nothing

    def with_params(**fields):
        c = Call()
        for k, v in fields.items():
            setattr(c.params, k, v)
        return c

    if shade:
        refused("numSamples 0 (1 ... 8)", num_samples=0)
        refused("numSamples 9 (1 ... 8)", num_samples=9)
        refused("samples is null", samples=None)
        refused("occluded is null", occ=None)
        refused("out is null", out=None)
        c = Call()
        refused("samples is not 16-B aligned", c=c, samples=ptr(c.out_samples, 4))
        c = Call()
        refused("out is not 16-B aligned", c=c, out=ptr(c.out, 8))
        c = Call()
        refused("out overlaps samples", c=c, out=ptr(c.out_samples))
        refused("do not fit 32 bits", n=0x80000000)
        assert Call().run(lib, name, n=0, samples=None, occ=None, out=None) == INVALID         # n == 0 passes the checks: then the null context
        assert "null context" in lib.rtr_last_error().decode()
        return
    refused("params is null", params=None)
    refused("numSamples 9", c=with_params(numSamples=9))
    if rays_call:
        refused("numSamples 0 (1 ... 8)", c=with_params(numSamples=0))
    refused("lobes 0x0", c=with_params(lobes=0))
    refused("lobes 0x4", c=with_params(lobes=4))
    refused("unknown flags bits 0x2", c=with_params(flags=2))
    refused("_reserved", c=with_params(_reserved=1))
    refused("rays is null", rays=None)
    c = Call()
    refused("rays is not 16-B aligned", c=c, rays=ptr(c.rays, 4))
    if rays_call:
        refused("width 0, spp 1", c=with_params(width=0))
        refused("width 2, spp 0", c=with_params(spp=0))
        refused("surfaces is null", surf=None)
        refused("outRays is null", out_rays=None)
        refused("outSamples is null", out_samples=None)
        c = Call()
        refused("outSamples is not 16-B aligned", c=c, out_samples=ptr(c.out_samples, 8))
        c = Call()
        refused("seeds is not 4-B aligned", c=c, seeds=ptr(c.seeds, 2))
        c = Call()
        refused("outRays overlaps rays", c=c, out_rays=ptr(c.rays))
        c = Call()
        refused("outSamples overlaps surfaces", c=c, out_samples=ptr(c.surf))
        c = Call()
        refused("outRays overlaps outSamples", c=c, out_samples=ptr(c.out_rays, 32))
        refused("do not fit 32 bits", n=0x80000000)
        c = with_params(width=0)
        assert c.run(lib, name, seeds=ptr(c.seeds)) == (0 if "host" in name else INVALID)       # explicit seeds need no frame
    if hits_call:
        refused("hits is null", hits=None)
        refused("prevSurfaces is null", surf=None)
        refused("bounces is null", bounce=None)
        refused("out is null", esc=None)
        c = Call()
        refused("out is not 16-B aligned", c=c, esc=ptr(c.esc, 8))
        c = Call()
        refused("out overlaps bounces", c=c, esc=ptr(c.bounce))
        c = with_params(numSamples=0)                                                            # a vertex that drew no sky sample
        assert c.run(lib, name) == (0 if "host" in name else INVALID)
    if "host" not in name:
        c = Call()
        before = c.outputs()
        assert c.run(lib, name) == INVALID and "null context or scene" in lib.rtr_last_error().decode()
        assert c.outputs() == before


def test_host_only_refusals():
    lib = A.hip_lib()

    def expect(rc, who, needle):
        msg = lib.rtr_last_error().decode()
        assert rc == INVALID and msg.startswith(who + ": ") and needle in msg, (who, needle, rc, msg)

    sky = np.array(SKY, np.float32)
    px = np.zeros(16, np.uint8)
    w, h = C.c_uint32(0), C.c_uint32(0)
    rows, marg = np.full(32 * 16, 0xA5A5A5A5, np.uint32), np.full(16, 0xA5, np.uint64)
    before = rows.tobytes() + marg.tobytes()

    def table(tex, color=sky, cells=512, nrows=16, r=rows, m=marg):
        return lib.rtr_host_sky_table(C.byref(tex) if tex is not None else None, ptr(color), C.byref(w), C.byref(h), ptr(r), cells, ptr(m), nrows)

    def tex(width, height, channels, pixels=px):
        return A.rtr_texture(pixels.ctypes.data_as(C.POINTER(C.c_uint8)) if pixels is not None else None, width, height, channels, 0)

    expect(table(tex(65536, 1, 1)), "rtr_host_sky_table", "65536 texels wide")
    expect(table(tex(2, 2, 3)), "rtr_host_sky_table", "bad extent or channels")
    expect(table(tex(0, 2, 4)), "rtr_host_sky_table", "bad extent or channels")
    expect(table(tex(2, 2, 4, None)), "rtr_host_sky_table", "hdri has no pixels")
    expect(table(None, None), "rtr_host_sky_table", "skyColor is null")
    expect(table(None, cells=511), "rtr_host_sky_table", "capacity 511 cells, 16 rows; 512 and 16 are needed")
    assert (w.value, h.value) == (32, 16)
    expect(table(None, nrows=15), "rtr_host_sky_table", "15 rows")
    expect(table(None, r=None), "rtr_host_sky_table", "capacity 0 cells")
    assert rows.tobytes() + marg.tobytes() == before
    assert table(None) == 0 and (w.value, h.value) == (32, 16)

    t = api.host_sky_table(None, SKY)
    good = t._c()
    d = np.ones((2, 3), np.float32)
    out = np.zeros((2, 3), np.float32)
    expect(lib.rtr_host_sky_pdf(None, ptr(d), 2, ptr(out)), "rtr_host_sky_pdf", "table is null")
    expect(lib.rtr_host_sky_pdf(C.byref(good), None, 2, ptr(out)), "rtr_host_sky_pdf", "dirs is null")
    expect(lib.rtr_host_sky_pdf(C.byref(good), ptr(d), 2, None), "rtr_host_sky_pdf", "outPdf is null")
    expect(lib.rtr_host_sky_pdf(C.byref(good), ptr(d, 2), 1, ptr(out)), "rtr_host_sky_pdf", "dirs is not 4-B aligned")
    bad = A.rtr_sky_table(good.rows, good.marginal, 0, 16)
    expect(lib.rtr_host_sky_pdf(C.byref(bad), ptr(d), 2, ptr(out)), "rtr_host_sky_pdf", "table is 0 x 16")
    bad = A.rtr_sky_table(None, good.marginal, 32, 16)
    expect(lib.rtr_host_sky_pdf(C.byref(bad), ptr(d), 2, ptr(out)), "rtr_host_sky_pdf", "table has no sums")
    expect(lib.rtr_host_sky_radiance(None, ptr(sky), None, 2, ptr(out)), "rtr_host_sky_radiance", "dirs is null")
    expect(lib.rtr_host_sky_radiance(None, ptr(sky), ptr(d), 2, None), "rtr_host_sky_radiance", "out is null")
    expect(lib.rtr_host_sky_radiance(None, None, ptr(d), 2, ptr(out)), "rtr_host_sky_radiance", "skyColor is null")
    expect(lib.rtr_host_sky_radiance(C.byref(tex(2, 2, 2)), ptr(sky), ptr(d), 2, ptr(out)), "rtr_host_sky_radiance", "bad extent or channels")
    assert not out.any()
    # a table of another sky's extent
    c = Call()
    small = A.rtr_sky_table(good.rows, good.marginal, 16, 16)
    rc = lib.rtr_host_sky_rays(None, ptr(c.sky), C.byref(small), ptr(c.rays), ptr(c.surf), N, C.byref(c.params), None, ptr(c.out_rays), ptr(c.out_samples))
    expect(rc, "rtr_host_sky_rays", "table is 16 x 16, the sky's is 32 x 16")
    rc = lib.rtr_host_sky_hits(None, ptr(c.sky), None, ptr(c.rays), ptr(c.hits), ptr(c.surf), ptr(c.bounce), N, C.byref(c.params), ptr(c.esc))
    expect(rc, "rtr_host_sky_hits", "table is null")
    assert lib.rtr_scene_prepare_sky(None) == INVALID and "rtr_scene_prepare_sky: null scene" in lib.rtr_last_error().decode()
    assert lib.rtr_scene_export_sky_table(None, None, None, None, 0, None, 0) == INVALID and "rtr_scene_export_sky_table: null scene" in lib.rtr_last_error().decode()
    # no records, no pointers
    assert lib.rtr_host_sky_rays(None, ptr(c.sky), C.byref(good), None, None, 0, C.byref(c.params), None, None, None) == 0
    assert lib.rtr_host_sky_hits(None, ptr(c.sky), C.byref(good), None, None, None, None, 0, C.byref(c.params), None) == 0
    assert lib.rtr_host_sky_pdf(C.byref(good), None, 0, None) == 0 and lib.rtr_host_sky_radiance(None, ptr(c.sky), None, 0, None) == 0
