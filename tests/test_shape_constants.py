"""tests/shape_cases.py's numbers are the source's.  The launch-shape tests (test_gpu_occlusion_shapes.py, test_gpu_query_shapes.py,
test_gpu_light_shapes.py) sit on both sides of the constants that cut a launch up; a constant that changes fails here and points at the
table to extend.  No GPU."""
import os
import re

import numpy as np

import shape_cases as SC

KERNELS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "realtimeraytracer_amd", "csrc", "kernels")


def _source(name):
    with open(os.path.join(KERNELS, name)) as f:
        return f.read()


def _constant(text, name):
    m = re.search(r"constexpr\s+(?:uint32_t|int)\s+" + name + r"\s*=\s*([^;]+);", text)
    assert m, f"{name} is no longer a constexpr of this file: tests/shape_cases.py names its value"
    return m.group(1).strip()


def test_queue_build_constants_are_the_edge_tables():
    q, occ, k = _source("rtr_query.h"), _source("rtr_occlusion.hip"), _source("rtr_kernels.h")
    assert _constant(q, "kOcclusionGenRays") == str(SC.GEN_RAYS) == "4096"
    assert _constant(occ, "kOccGenBlock") == str(SC.GEN_BLOCK) == "512"
    assert _constant(k, "kQueueRegions") == str(SC.REGIONS) == "8"
    m = re.search(r"constexpr\s+uint32_t\s+occlusion_batch\(uint32_t n\)\s*\{\s*return\s+\(size_t\)n\s*>=\s*\(\(size_t\)(\d+)\s*<<\s*(\d+)\)\s*\?\s*(\d+)u\s*:\s*(\d+)u;",
                  q)
    assert m, "occlusion_batch() changed its form: tests/shape_cases.py names its two batches and its threshold"
    assert int(m.group(1)) << int(m.group(2)) == SC.BIG_BATCH_FROM == 100 << 20
    assert (int(m.group(3)), int(m.group(4))) == (SC.BIG_BATCH, SC.BATCH) == (512, 256)
    for c in (SC.WAVE, SC.BATCH, SC.GEN_BLOCK, SC.GEN_RAYS):
        assert {c - 1, c, c + 1} <= set(SC.EDGES), c
    assert SC.EDGES == (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 8191, 8193, 36865)
    assert SC.MASTER == (SC.REGIONS + 1) * SC.GEN_RAYS + 1, "nine queue-build workgroups: every blockIdx.x % kQueueRegions and one of them twice"


def test_light_stage_constants_are_the_slot_edges():
    src = _source("rtr_query.hip")
    assert _constant(src, "kLightRaysBlock") == str(SC.LIGHT_BLOCK) == "64"
    assert _constant(src, "kLightStagedSlots") == str(SC.LIGHT_STAGED_SLOTS) == "31"
    m = re.fullmatch(r"(\d+)u\s*<<\s*(\d+)", _constant(src, "kLightStagedLds"))
    assert m and int(m.group(1)) << int(m.group(2)) == SC.LIGHT_STAGED_LDS == 64 << 10
    # the hinted stage's size, as launch_light_rays writes it, and light_hint_pitch
    assert re.search(r"\(size_t\)kLightRaysBlock \* \(\(2u \* \(size_t\)la\.slots \+ 1u\) \* sizeof\(rtr_q4\) \+ light_hint_pitch\(la\.slots\) \* sizeof\(int32_t\)\)", src)
    assert re.search(r"light_hint_pitch\(uint32_t \w+\)\s*\{\s*return \w+ \| 1u;", src + _source("rtr_query.h"))
    # the crossovers test_gpu_light_shapes.py straddles: Q = shadow_rays + 1 with one light triangle and the directional light
    assert [SC.hinted_stage_fits(q) for q in (27, 28, 31, 32)] == [True, False, False, False]
    assert [q <= SC.LIGHT_STAGED_SLOTS for q in (27, 28, 31, 32, 33)] == [True, True, True, False, False]
    # the picked stage: P + 1 slots, refused beyond the stage
    assert re.search(r"pa\.picks \+ 1u > kLightStagedSlots", src)


def test_the_list_stride_holds_the_worst_case_of_one_list():
    src = _source("rtr_query.h")
    assert re.search(r"return \(uint32_t\)\(\(uint64_t\)n / 256u / kQueueRegions \+ \(\(uint64_t\)n \+ kOcclusionGenRays - 1\) / kOcclusionGenRays \+ 1u\);", src), \
        "occlusion_list_stride() changed: restate it in tests/shape_cases.py"
    for n in SC.EDGES + (SC.BIG_BATCH_FROM - 1, SC.BIG_BATCH_FROM):
        assert SC.occlusion_list_stride(n) >= SC.worst_list_length(n), n
    # the worst case, list by list, as k_occlusion_gen deals the batches: block b hands list x the batches b0, b0 + 8, ... of an octant's run
    for n in (4097, SC.MASTER):
        per_list = np.zeros(SC.REGIONS, np.int64)
        for b in range(-(-n // SC.GEN_RAYS)):
            nb = -(-min(SC.GEN_RAYS, n - b * SC.GEN_RAYS) // SC.BATCH)
            for x in range(SC.REGIONS):
                b0 = (x + SC.REGIONS - b % SC.REGIONS) % SC.REGIONS
                per_list[x] += (nb - b0 + SC.REGIONS - 1) // SC.REGIONS if b0 < nb else 0
        assert per_list.max() <= SC.worst_list_length(n) <= SC.occlusion_list_stride(n)
