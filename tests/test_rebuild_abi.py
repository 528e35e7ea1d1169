"""The rebuild's and the tree cost's C-ABI surface (rtr_scene_rebuild, rtr_scene_tree_cost, rtr_host_tree_cost, rtr_tree_cost) — what
needs no device: the header declares the entry points and the struct, the product and the test library export them, _abi.py binds them
with the header's argument lists, the struct is 96 bytes on both sides, the argument errors that come before any device work, and
rtr_host_tree_cost against a numpy restatement of the definition in include/rtr.h on host-built trees."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1

VP, u32 = A.VP, A.u32
EXPECTED = {
    "rtr_scene_rebuild": ("rtr_scene* scene, uint32_t buildFlags", [VP, u32]),
    "rtr_scene_tree_cost": ("const rtr_scene* scene, rtr_tree_cost* out", [VP, C.POINTER(A.rtr_tree_cost)]),
    "rtr_host_tree_cost": ("const RtrBvhNode* nodes, size_t nodeBytes, const RtrBvhGrid* grid, rtr_tree_cost* out",
                           [VP, C.c_size_t, C.POINTER(A.RtrBvhGrid), C.POINTER(A.rtr_tree_cost)]),
}


def _raw_header():
    return open(os.path.join(ROOT, "include", "rtr.h")).read()


def _header():
    return re.sub(r"/\*.*?\*/", "", _raw_header(), flags=re.S)


def _norm(params):
    return [re.sub(r"\s+", " ", p).strip() for p in params.split(",")]


# ---- the definition of include/rtr.h, restated in numpy (shared with tests/test_gpu_rebuild.py) -------------------------------------
def numpy_tree_cost(nodes, grid, in_tree=None):
    """(the eleven integers as Python ints: innerArea[3], leafArea[3], rootArea[3], numInner, numLeafRefs; sah).  nodes: RtrBvhNode array
    (ctypes or bytes); in_tree: a boolean mask of the slots that are part of the tree (None: the slots the root reaches)."""
    raw = np.frombuffer(bytes(nodes), dtype=np.uint16).reshape(-1, 16)
    q = raw[:, :12].astype(np.int64)
    child = np.frombuffer(bytes(nodes), dtype=np.int32).reshape(-1, 8)[:, 6:8].astype(np.int64)
    n = len(q)
    if in_tree is None:
        in_tree = np.zeros(n, bool)
        in_tree[0] = True
        todo = [0]
        while todo:
            i = todo.pop()
            for c in child[i].tolist():
                if c >= 0 and not in_tree[c]:
                    in_tree[c] = True
                    todo.append(c)

    def slot(side, is_max, axis):      # RTR_BVH_QSLOT
        return side * 4 + is_max * 2 + axis if axis < 2 else 8 + side * 2 + is_max

    def triple(lo, hi):
        d = [max(0, int(hi[a]) - int(lo[a])) for a in range(3)]
        return [d[0] * d[1], d[1] * d[2], d[2] * d[0]]

    inner, leaf, num_inner, num_leaf = [0, 0, 0], [0, 0, 0], 0, 0
    for i in np.flatnonzero(in_tree).tolist():
        for side in range(2):
            lo = [q[i, slot(side, 0, a)] for a in range(3)]
            hi = [q[i, slot(side, 1, a)] for a in range(3)]
            t = triple(lo, hi)
            code = int(child[i, side])
            if code >= 0:
                inner = [x + y for x, y in zip(inner, t)]
                num_inner += 1
            else:
                count = ((~code) & 7) + 1
                leaf = [x + count * y for x, y in zip(leaf, t)]
                num_leaf += 1
    lo = [min(q[0, slot(0, 0, a)], q[0, slot(1, 0, a)]) for a in range(3)]
    hi = [max(q[0, slot(0, 1, a)], q[0, slot(1, 1, a)]) for a in range(3)]
    root = triple(lo, hi)
    inner = [x + y for x, y in zip(inner, root)]
    num_inner += 1
    sx, sy, sz = (float(grid.scale[k]) for k in range(3))

    def W(a):
        return float(a[0]) * sx * sy + float(a[1]) * sy * sz + float(a[2]) * sz * sx

    r = W(root)
    sah = (W(inner) * 1.0 + W(leaf) * 1.0) / r if r > 0.0 else 0.0
    return tuple(inner + leaf + root + [num_inner, num_leaf]), sah


def assert_cost(got, nodes, grid, what, in_tree=None):
    ints, sah = numpy_tree_cost(nodes, grid, in_tree)
    assert got.integers() == ints, f"{what}: the integers {got.integers()} != the restatement's {ints}"
    assert max(ints[:9]) < 2 ** 61
    assert math.isfinite(got.sah) and abs(got.sah - sah) <= 1e-12 * abs(sah), f"{what}: sah {got.sah!r} != {sah!r}"


def one_triangle_desc():
    s = scenes.cornell_box(16, 16)
    d = A.rtr_scene_desc.from_buffer_copy(bytes(s.desc))
    # the first object instance and the first triangle of its mesh, nothing else
    k = next(i for i in range(s.desc.numInstances) if s.desc.instances[i].customIndex >= s.desc.numLights)
    inst = A.RtrInstance.from_buffer_copy(bytes(s.desc.instances[k]))
    mesh = A.RtrMesh.from_buffer_copy(bytes(s.desc.meshes[inst.meshIndex]))
    mesh.indexCount = 3
    obj = A.RtrObjectInfo.from_buffer_copy(bytes(s.desc.objects[inst.customIndex - s.desc.numLights]))
    inst.meshIndex, inst.customIndex = 0, 0
    d._keep = [s, (A.RtrInstance * 1)(inst), (A.RtrMesh * 1)(mesh), (A.RtrObjectInfo * 1)(obj)]
    d.instances, d.numInstances = C.cast(d._keep[1], C.POINTER(A.RtrInstance)), 1
    d.meshes, d.numMeshes = C.cast(d._keep[2], C.POINTER(A.RtrMesh)), 1
    d.objects, d.numObjects = C.cast(d._keep[3], C.POINTER(A.RtrObjectInfo)), 1
    d.lights, d.numLights = None, 0
    return d


def empty_desc():
    d = A.rtr_scene_desc()
    d.skyColor[0] = d.skyColor[1] = d.skyColor[2] = 0.5
    return d


# ---- the surface --------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_exported_and_bound():
    text = _header()
    for path in (A.LIB_HIP_PATH, A.LIB_HIP_HOOKS_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        for n in EXPECTED:
            assert n in exported, f"{os.path.basename(path)} does not export {n}"
    for n, (params, argtypes) in EXPECTED.items():
        m = re.search(r"\bint\s+" + n + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{n} is not declared in include/rtr.h"
        assert _norm(m.group(1)) == _norm(params), f"{n}: the header's parameters are {_norm(m.group(1))}"
        assert n in A.RTR_SYMBOLS, f"{n} is not bound in _abi.RTR_SYMBOLS"
        res, args = A.RTR_SYMBOLS[n]
        assert res is C.c_int and list(args) == argtypes, f"{n}: bound as {args}"
        assert len(args) == len(_norm(params))
    # new symbols only: no layout and no kernel changed
    assert A.hip_lib().rtr_abi_version() == 3
    assert re.search(r"#define\s+RTR_ABI_VERSION\s+3\b", _raw_header())


def test_the_struct():
    text = _header()
    m = re.search(r"typedef\s+struct\s+rtr_tree_cost\s*\{(.*?)\}\s*rtr_tree_cost\s*;", text, flags=re.S)
    assert m, "rtr_tree_cost is not declared in include/rtr.h"
    fields = [re.sub(r"\s+", " ", f).strip() for f in m.group(1).split(";") if f.strip()]
    assert fields == ["uint64_t innerArea[3], leafArea[3], rootArea[3]", "uint64_t numInner, numLeafRefs", "double sah"], fields
    assert "static_assert(sizeof(rtr_tree_cost) == 96" in text
    assert C.sizeof(A.rtr_tree_cost) == 96 and C.alignment(A.rtr_tree_cost) == 8
    assert [f[0] for f in A.rtr_tree_cost._fields_] == ["innerArea", "leafArea", "rootArea", "numInner", "numLeafRefs", "sah"]
    T = A.rtr_tree_cost
    assert (T.innerArea.offset, T.leafArea.offset, T.rootArea.offset, T.numInner.offset, T.numLeafRefs.offset, T.sah.offset) == (0, 24, 48, 72, 80, 88)


def test_argument_errors_that_need_no_device():
    lib = A.hip_lib()
    out = A.rtr_tree_cost()
    assert lib.rtr_scene_rebuild(None, A.BUILD_DEVICE_LBVH) == INVALID
    assert b"rtr_scene_rebuild" in lib.rtr_last_error() and b"null scene" in lib.rtr_last_error()
    assert lib.rtr_scene_tree_cost(None, C.byref(out)) == INVALID
    assert b"rtr_scene_tree_cost" in lib.rtr_last_error() and b"null" in lib.rtr_last_error()
    s = scenes.cornell_box(16, 16)
    st, nodes, _ = api.host_build_bvh(s.desc)
    grid = st.grid
    nbytes = C.sizeof(nodes)
    for args, needle in (((None, nbytes, C.byref(grid), C.byref(out)), b"null"), ((nodes, nbytes, None, C.byref(out)), b"null"),
                         ((nodes, nbytes, C.byref(grid), None), b"null"), ((nodes, 0, C.byref(grid), C.byref(out)), b"nodeBytes"),
                         ((nodes, 31, C.byref(grid), C.byref(out)), b"nodeBytes"), ((nodes, nbytes - 1, C.byref(grid), C.byref(out)), b"nodeBytes")):
        assert lib.rtr_host_tree_cost(*args) == INVALID, args
        assert b"rtr_host_tree_cost" in lib.rtr_last_error() and needle in lib.rtr_last_error(), lib.rtr_last_error()
    # a short array: the root names children past its end
    if st.numNodes > 1:
        assert lib.rtr_host_tree_cost(nodes, 32, C.byref(grid), C.byref(out)) == INVALID
        assert b"names child" in lib.rtr_last_error()


def test_python_layer_has_the_documented_methods():
    assert list(inspect.signature(api.Scene.tree_cost).parameters) == ["self"]
    p = inspect.signature(api.Scene.rebuild).parameters
    assert list(p) == ["self", "build"] and p["build"].default == "device"
    p = inspect.signature(api.Scene.update_vertices_or_rebuild).parameters
    assert list(p) == ["self", "ranges", "instances", "lights", "rebuild_above", "rebuild_build"]
    assert p["rebuild_above"].default is None and p["rebuild_build"].default == "device"
    assert list(inspect.signature(api.host_tree_cost).parameters) == ["nodes", "grid"]


# ---- rtr_host_tree_cost against the definition --------------------------------------------------------------------------------------
SCENES = {"cornell": lambda: scenes.cornell_box(32, 32), "bunny": lambda: scenes.bunny_class(32, 32, subdiv=3), "room": lambda: scenes.textured_room(32, 32)}


@pytest.mark.parametrize("name", list(SCENES))
def test_host_tree_cost_equals_the_definition(name):
    s = SCENES[name]()
    st, nodes, _ = api.host_build_bvh(s.desc)
    got = api.host_tree_cost(nodes, st.grid)
    assert_cost(got, nodes, st.grid, name)
    assert got.num_inner == st.numNodes and got.num_leaf_refs == st.numNodes + 1      # a binary tree whose every slot the root reaches
    assert got == api.host_tree_cost(np.frombuffer(bytes(nodes), np.uint8), st.grid), "a numpy array of the same bytes"
    # beside the builder's own fp32 number (no contract: the quantised boxes are rounded outward, so the cost on them is not below it)
    rel = (got.sah - st.sahCost) / st.sahCost
    print(f"{name}: sah on the quantised BVH2 {got.sah!r}, stats.sahCost {st.sahCost!r}, relative difference {rel:.3e}")
    assert math.isfinite(rel) and rel >= 0.0


def test_a_single_leaf_counts_twice():
    st, nodes, _ = api.host_build_bvh(one_triangle_desc())
    assert st.numNodes == 1 and st.numTriangles == 1 and nodes[0].child[0] == nodes[0].child[1] < 0
    got = api.host_tree_cost(nodes, st.grid)
    assert_cost(got, nodes, st.grid, "one triangle")
    assert (got.num_inner, got.num_leaf_refs) == (1, 2)
    assert got.inner_area == got.root_area and got.leaf_area == tuple(2 * x for x in got.root_area)


def test_the_empty_scene_and_a_root_without_area():
    """The empty scene holds one degenerate triangle, whose box is PADDED like every box (2^-18 of the largest coordinate, at least
    3.8e-12): on its grid that box has an area, and the scene prices as the single leaf it is — root + 2 leaf references = 3 — by the
    formula, on the host as on the device.  sah == 0 is what a root WITHOUT area gives; that rule is checked on a tree whose boxes are
    flat."""
    st, nodes, _ = api.host_build_bvh(empty_desc())
    assert st.numNodes == 1 and st.numTriangles == 0
    got = api.host_tree_cost(nodes, st.grid)
    assert_cost(got, nodes, st.grid, "empty scene")
    assert (got.num_inner, got.num_leaf_refs) == (1, 2)
    flat = (A.RtrBvhNode * 1)()
    for k in range(12):
        flat[0].q[k] = 7
    flat[0].q[1] = 9; flat[0].q[3] = 3         # an inside-out y extent on the left child counts as 0, not as a negative number
    flat[0].child[0] = flat[0].child[1] = ~0
    got = api.host_tree_cost(flat, st.grid)
    assert got.integers() == (0,) * 9 + (1, 2) and got.sah == 0.0
    assert numpy_tree_cost(flat, st.grid) == ((0,) * 9 + (1, 2), 0.0)
