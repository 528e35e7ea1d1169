"""Thin Python handles over the C ABI (include/rtr.h): Context / Scene / Frame / render.
Every non-zero status becomes RtrError carrying rtr_last_error() — the same convention as the C++
shim csrc/host/renderer.hpp (reference: exceptions caught once in main, src/main.cpp:12-15)."""
import ctypes as C
import dataclasses

import numpy as np

from . import _abi as A


class RtrError(RuntimeError):
    def __init__(self, status, what):
        lib = A.hip_lib()
        self.status = status
        self.status_name = lib.rtr_status_string(status).decode()
        super().__init__(f"{what}: {self.status_name}: {lib.rtr_last_error().decode()}")


def _check(status, what):
    if status != 0:
        raise RtrError(status, what)


class Context:
    def __init__(self, device=0, test_hooks=False):
        """test_hooks: everything made from this context goes through librtr_hip_test.so (the product's sources + the test switches)"""
        self.lib = A.hip_lib_with_hooks() if test_hooks else A.hip_lib()
        self.device = int(device)
        self.h = A.VP()
        _check(self.lib.rtr_ctx_create(device, C.byref(self.h)), "rtr_ctx_create")

    def set_tunable(self, name, value):
        _check(self.lib.rtr_ctx_set_tunable(self.h, name.encode(), int(value)), "rtr_ctx_set_tunable")

    def get_tunable(self, name):
        v = C.c_uint32(0)
        _check(self.lib.rtr_ctx_get_tunable(self.h, name.encode(), C.byref(v)), "rtr_ctx_get_tunable")
        return int(v.value)

    def set_stream(self, stream_ptr):
        _check(self.lib.rtr_ctx_set_stream(self.h, A.VP(stream_ptr) if stream_ptr else None), "rtr_ctx_set_stream")

    def get_stream(self):
        """the hipStream_t (as an int) this context's work is enqueued on"""
        p = A.VP()
        _check(self.lib.rtr_ctx_get_stream(self.h, C.byref(p)), "rtr_ctx_get_stream")
        return p.value or 0

    def device_name(self):
        buf = C.create_string_buffer(256)
        _check(self.lib.rtr_ctx_device_name(self.h, buf, 256), "rtr_ctx_device_name")
        return buf.value.decode()

    def close(self):
        if self.h:
            self.lib.rtr_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BvhExport(tuple):
    """(nodes, tris, grid) of rtr_scene_export_bvh, with the 4-wide view of rtr_scene_export_wide as .wide"""
    wide = None
    stats = None


class TreeCost:
    """What Scene.tree_cost and host_tree_cost give back: the integer area sums of the quantised BVH2 as Python ints — inner_area,
    leaf_area, root_area, each (x*y, y*z, z*x) in grid steps — the counts num_inner and num_leaf_refs, and sah, the cost made from the
    sums with the grid's scale (include/rtr.h, rtr_tree_cost)."""

    def __init__(self, c):
        self.inner_area = tuple(int(x) for x in c.innerArea)
        self.leaf_area = tuple(int(x) for x in c.leafArea)
        self.root_area = tuple(int(x) for x in c.rootArea)
        self.num_inner, self.num_leaf_refs = int(c.numInner), int(c.numLeafRefs)
        self.sah = float(c.sah)
        self.raw = bytes(c)

    def integers(self):
        return self.inner_area + self.leaf_area + self.root_area + (self.num_inner, self.num_leaf_refs)

    def __eq__(self, other):
        return isinstance(other, TreeCost) and self.raw == other.raw

    def __repr__(self):
        return f"TreeCost(sah={self.sah!r}, num_inner={self.num_inner}, num_leaf_refs={self.num_leaf_refs}, root_area={self.root_area})"


@dataclasses.dataclass(frozen=True)
class UpdateStatus:
    """Scene.update_status(): enqueued — update_vertices_async and update_instances_async calls accepted so far, whose serials count
    from 1 on one sequence; refused — how many of them the device refused for bad data; first_refused_update / first_bad_vertex — the
    serial of the first refused update since the last status call and the smallest scene vertex index it refused, None where there
    was none.  For a refused instance update first_bad_vertex is its smallest bad element: an instance index (instance order), or
    the number of instances plus a light index."""
    enqueued: int
    refused: int
    first_refused_update: "int | None"
    first_bad_vertex: "int | None"


@dataclasses.dataclass(frozen=True)
class RebuildIfStatus:
    """Scene.rebuild_if_status(): evaluated — rebuild_if_async calls whose decision has run; rebuilt — how many of them built and
    committed a new tree; built_sah — the baseline, the sah of the tree right after its last build; last_sah — the sah the last
    decision looked at (0.0 before the first); last_decision — True: it built, False: it skipped, None: none yet."""
    evaluated: int
    rebuilt: int
    built_sah: float
    last_sah: float
    last_decision: "bool | None"


class Scene:
    def __init__(self, ctx, desc, like=None):
        """like: a Scene made from the same description whose tree is uploaded instead of built again (rtr_scene_create_like)"""
        self.ctx, self.lib = ctx, ctx.lib
        self._async_keep = []         # tensors of enqueued updates: referenced until the next update_status (or the scene's end)
        self._num_lights = int(desc.numLights)
        self._built_sah = None        # tree_cost().sah right after the last build or rebuild: taken on first use (update_vertices' policy)
        self._policy_ever = False     # prepare_async_rebuild_if succeeded once: a device rebuild prepares the policy again by itself
        self._policy_ready = False    # ... and no host rebuild has dropped the readiness since: the baseline lives on the device
        self.h = A.VP()
        self._num_instances = int(desc.numInstances)
        self._num_vertices = int(desc.numVertices)
        if like is None:
            _check(self.lib.rtr_scene_create(ctx.h, C.byref(desc), C.byref(self.h)), "rtr_scene_create")
        else:
            _check(self.lib.rtr_scene_create_like(ctx.h, C.byref(desc), like.h, C.byref(self.h)), "rtr_scene_create_like")

    def stats(self):
        s = A.rtr_scene_stats()
        _check(self.lib.rtr_scene_get_stats(self.h, C.byref(s)), "rtr_scene_get_stats")
        return s

    def export_bvh(self):
        s = self.stats()
        nodes = (A.RtrBvhNode * s.numNodes)()
        # numTriangles==0 scenes carry one dummy record
        ntri = max(s.numTriangles, 1)
        tris = (A.RtrBvhTri * ntri)()
        _check(self.lib.rtr_scene_export_bvh(self.h, nodes, C.sizeof(nodes), tris, C.sizeof(tris)), "rtr_scene_export_bvh")
        out = BvhExport((nodes, tris, s.grid))      # the nodes' 16-bit planes live on s.grid
        if s.numWideNodes:
            wn = (A.RtrWideNode * s.numWideNodes)()
            _check(self.lib.rtr_scene_export_wide(self.h, wn, C.sizeof(wn)), "rtr_scene_export_wide")
            out.wide = wn
        return out

    def export_wide_resident(self):
        """rtr_scene_export_wide_resident: the 4-wide records in the order the device holds them (a best-first top towards the lights,
        then breadth-first) -> a ctypes RtrWideNode array, or None for a scene without a wide view"""
        s = self.stats()
        if not s.numWideNodes:
            return None
        wn = (A.RtrWideNode * s.numWideNodes)()
        _check(self.lib.rtr_scene_export_wide_resident(self.h, wn, C.sizeof(wn)), "rtr_scene_export_wide_resident")
        return wn

    def update_instances(self, instances, lights=None):
        """rtr_scene_update_instances: new transforms (+ optional light infos) -> device-side re-flatten + BVH refit."""
        arr = (A.RtrInstance * len(instances))(*instances)
        if lights is None:
            _check(self.lib.rtr_scene_update_instances(self.h, arr, len(instances), None, 0), "rtr_scene_update_instances")
        else:
            larr = (A.RtrAreaLightInfo * len(lights))(*lights)
            _check(self.lib.rtr_scene_update_instances(self.h, arr, len(instances), larr, len(lights)), "rtr_scene_update_instances")

    def tree_cost(self):
        """rtr_scene_tree_cost: the SAH cost of the tree the kernels walk now (a device kernel over the quantised BVH2) -> TreeCost"""
        c = A.rtr_tree_cost()
        _check(self.lib.rtr_scene_tree_cost(self.h, C.byref(c)), "rtr_scene_tree_cost")
        return TreeCost(c)

    def rebuild(self, build="device"):
        """rtr_scene_rebuild: build the tree again, in place, from the vertices and transforms the scene has now.  build: "device" (the
        LBVH build on the device) or "host" (the SAH builder; vertices are read back).  Everything else of the scene stays; the hints of
        hit_leaves made before are stale (and still safe)."""
        flags = {"device": A.BUILD_DEVICE_LBVH, "host": A.BUILD_HOST_SAH}.get(build)
        if flags is None:
            raise ValueError(f"rebuild: build must be 'device' or 'host', got {build!r}")
        _check(self.lib.rtr_scene_rebuild(self.h, flags), "rtr_scene_rebuild")
        self._built_sah = self.tree_cost().sah
        self._policy_ready = self._policy_ever and build == "device"

    def update_vertices_or_rebuild(self, ranges, instances=None, lights=None, rebuild_above=None, rebuild_build="device"):
        """update_vertices with a rebuild policy on top; the arguments before rebuild_above are update_vertices' own.
        rebuild_above: None (the default) — update_vertices and nothing else, no cost kernel runs — or a number: after the refit, if
        tree_cost().sah > rebuild_above * (the sah right after the last build or rebuild of this scene), rebuild(rebuild_build).  The
        build-time sah is taken on first use — before this call's refit — and refreshed by rebuild.  Returns whether it rebuilt.  No
        ratio is recommended: profiles/rebuild/ is where the relation between sah and frame time is written down."""
        who = "update_vertices_or_rebuild"
        if rebuild_above is None:
            self.update_vertices(ranges, instances, lights)
            return False
        rebuild_above = float(rebuild_above)
        if rebuild_build not in ("device", "host"):
            raise ValueError(f"{who}: rebuild_build must be 'device' or 'host', got {rebuild_build!r}")
        if self._policy_ready:        # the device keeps the baseline, through rebuild_async and rebuild_if_async too: the policies mix
            self._built_sah = self.rebuild_if_status().built_sah
        if self._built_sah is None:
            self._built_sah = self.tree_cost().sah
        self.update_vertices(ranges, instances, lights)
        if self.tree_cost().sah > rebuild_above * self._built_sah:
            self.rebuild(rebuild_build)
            return True
        return False

    def prepare_async_updates(self):
        """rtr_scene_prepare_async_updates: once, synchronously, everything update_vertices_async must not do later"""
        _check(self.lib.rtr_scene_prepare_async_updates(self.h), "rtr_scene_prepare_async_updates")

    def prepare_async_rebuild(self):
        """rtr_scene_prepare_async_rebuild: once, synchronously, everything rebuild_async must not do later — prepare_async_updates, the
        stage the device build writes and the build's scratch (some 300 B per triangle, kept).  The scene's tree must be a device
        tree of at least 16 triangles (rebuild("device") makes one)."""
        _check(self.lib.rtr_scene_prepare_async_rebuild(self.h), "rtr_scene_prepare_async_rebuild")

    def rebuild_async(self, build="device"):
        """rtr_scene_rebuild_async: rebuild("device") as stream-ordered work on the context's stream; returns at once, joins nothing.
        Only build="device" can be enqueued.  The device refuses a tree deeper than the stack class the scene renders with
        (stats().stackEntries): update_status() reports it, and the refused rebuild changes nothing.  _built_sah is not refreshed: the
        cost is not known without a join.  On a scene prepared with prepare_async_rebuild_if the DEVICE refreshes the baseline
        (rebuild_if_status().built_sah), which update_vertices_or_rebuild then uses."""
        if build != "device":
            raise ValueError(f"rebuild_async: only build='device' can be enqueued, got {build!r}")
        _check(self.lib.rtr_scene_rebuild_async(self.h, A.BUILD_DEVICE_LBVH), "rtr_scene_rebuild_async")

    def prepare_async_rebuild_if(self):
        """rtr_scene_prepare_async_rebuild_if: once, synchronously, everything rebuild_if_async must not do later —
        prepare_async_rebuild, the policy's words on the device, and the baseline: tree_cost().sah of the tree as it is now."""
        _check(self.lib.rtr_scene_prepare_async_rebuild_if(self.h), "rtr_scene_prepare_async_rebuild_if")
        self._policy_ever = self._policy_ready = True

    def rebuild_if_async(self, rebuild_above, build="device"):
        """rtr_scene_rebuild_if_async: the policy of update_vertices_or_rebuild decided ON THE DEVICE, as stream-ordered work; returns at
        once, joins nothing.  The stream evaluates the tree's sah, and rebuilds — rebuild_async's chain — when it is above
        rebuild_above * (the sah right after the last build); otherwise the chain's kernels return at once and no byte changes.
        rebuild_above: a number >= 0; inf never rebuilds, 0.0 rebuilds whenever the cost is positive.  rebuild_if_status() tells
        what was decided."""
        if build != "device":
            raise ValueError(f"rebuild_if_async: only build='device' can be enqueued, got {build!r}")
        _check(self.lib.rtr_scene_rebuild_if_async(self.h, A.BUILD_DEVICE_LBVH, float(rebuild_above)), "rtr_scene_rebuild_if_async")

    def rebuild_if_status(self):
        """rtr_scene_rebuild_if_status: joins the context's stream and reports the policy's record -> RebuildIfStatus"""
        st = A.rtr_rebuild_if_status()
        _check(self.lib.rtr_scene_rebuild_if_status(self.h, C.byref(st)), "rtr_scene_rebuild_if_status")
        return RebuildIfStatus(int(st.evaluated), int(st.rebuilt), float(st.builtSah), float(st.lastSah),
                               None if st.lastDecision == 0xffffffff else bool(st.lastDecision))

    def update_vertices_or_rebuild_async(self, ranges, rebuild_above):
        """update_vertices_async(ranges), then rebuild_if_async(rebuild_above): update_vertices_or_rebuild with build="device" as
        stream-ordered work.  Returns nothing: rebuild_if_status() tells what the device decided."""
        self.update_vertices_async(ranges)
        self.rebuild_if_async(rebuild_above)

    def update_status(self):
        """rtr_scene_update_status: joins the context's stream and reports the enqueued updates -> UpdateStatus.  The tensors of the
        updates enqueued so far are released.  For a refused rebuild_async, first_bad_vertex is the depth of the tree that was refused."""
        st = A.rtr_update_status()
        _check(self.lib.rtr_scene_update_status(self.h, C.byref(st)), "rtr_scene_update_status")
        self._async_keep = []
        none = 0xffffffff
        return UpdateStatus(int(st.enqueued), int(st.refused), None if st.firstRefusedUpdate == none else int(st.firstRefusedUpdate),
                            None if st.firstBadVertex == none else int(st.firstBadVertex))

    def update_vertices_async(self, ranges, instances=None, lights=None):
        """rtr_scene_update_vertices_async: update_vertices as stream-ordered work.  The update is ENQUEUED on the context's stream
        (Context.set_stream makes that torch's) and the call returns at once: nothing is joined, so the tensors must be produced on that
        stream (or ordered before it by the caller).  ranges as in update_vertices, torch tensors on the scene's device only, strided
        views as they are; numpy arrays, instances= and lights= raise ValueError (they stay with the synchronous call).  The scene needs
        prepare_async_updates() once.  Bad data cannot raise here: update_status() reports it, and a refused update changes nothing.
        The tensors stay referenced until the next update_status() or the scene's end."""
        self._update_vertices(ranges, instances, lights, True)

    def update_vertices(self, ranges, instances=None, lights=None):
        """rtr_scene_update_vertices: deform meshes — new positions (and normals) for ranges of the scene's vertex array, then ONE refit
        that also carries `instances` / `lights` when they are given (as update_instances takes them; None keeps the current ones).
        ranges: a list of (first_vertex, positions) or (first_vertex, positions, normals); first_vertex indexes the scene's concatenated
        vertex array (desc.vertices), a range may span meshes, ranges must not overlap.  The arrays are float32 (n, 3) or (n, 4) — the
        first three columns are used — and either ALL numpy arrays (the host route) or ALL torch tensors on the scene's device (the
        device route: the data never leaves the device); mixing the kinds is refused.  A strided view is taken as it is when its row
        stride is a multiple of 4 bytes and its columns are adjacent: a (n, 4)[:, :3] column view, rows of an (n, 12) RtrVertex array.
        One call passes one position stride and one normal stride, so arrays whose strides differ (or that do not qualify) are made
        contiguous first.  uv and the vertices outside the ranges keep their bytes.  A position that is not finite refuses the whole
        call (RtrError, RTR_ERR_INVALID_ARGUMENT) and leaves the scene as it was.  With tensors, torch's current stream is joined first
        when the context works on another one, as in the query calls.  update_vertices_async is the enqueued form."""
        self._update_vertices(ranges, instances, lights, False)

    def _update_vertices(self, ranges, instances, lights, asynchronous):
        who = "update_vertices_async" if asynchronous else "update_vertices"
        if asynchronous and (instances is not None or lights is not None):
            raise ValueError(f"{who}: takes no instances= and no lights=: they stay with the synchronous call")
        rows = []
        for k, r in enumerate(ranges):
            if not isinstance(r, (tuple, list)) or len(r) not in (2, 3):
                raise ValueError(f"{who}: range {k} must be (first_vertex, positions[, normals])")
            rows.append((int(r[0]), r[1], r[2] if len(r) == 3 else None))
        if not rows:
            raise ValueError(f"{who}: no ranges")
        arrays = [a for _, p, n in rows for a in (p, n) if a is not None]
        if any(p is None for _, p, _ in rows):
            raise ValueError(f"{who}: a range without positions")
        as_numpy = all(isinstance(a, np.ndarray) for a in arrays)
        if asynchronous and (as_numpy or any(isinstance(a, np.ndarray) for a in arrays)):
            raise ValueError(f"{who}: takes torch tensors on the scene's device, not numpy arrays")
        if not as_numpy:
            torch = _torch()
            if not all(isinstance(a, torch.Tensor) for a in arrays):
                raise ValueError(f"{who}: the arrays must be all numpy arrays or all torch tensors on the scene's device, not a mixture")
            dev = torch.device("cuda", self.ctx.device)
        for k, (first, p, n) in enumerate(rows):
            for name, a in (("positions", p), ("normals", n)):
                if a is None:
                    continue
                ok = (a.dtype == np.float32) if as_numpy else (a.dtype == torch.float32)
                if not ok or len(a.shape) != 2 or a.shape[1] not in (3, 4):
                    raise ValueError(f"{who}: range {k}: {name} must be float32 (n, 3) or (n, 4), got {a.dtype} {tuple(a.shape)}")
                if not as_numpy and a.device != dev:
                    raise ValueError(f"{who}: range {k}: {name} live on {a.device}, the scene on {dev}")
            if n is not None and n.shape[0] != p.shape[0]:
                raise ValueError(f"{who}: range {k}: {p.shape[0]} positions but {n.shape[0]} normals")
            if first < 0 or first + p.shape[0] > 0xffffffff:
                raise ValueError(f"{who}: range {k}: first_vertex {first} with {p.shape[0]} vertices does not fit 32 bits")

        def pack(a):
            return np.ascontiguousarray(a[:, :3]) if as_numpy else a[:, :3].contiguous()

        def unify(which):        # one stride per call: every array of this kind as it is, or all of them packed (stride 12)
            seen = set()
            for a in (r[which] for r in rows if r[which] is not None and r[which].shape[0]):
                sb, sc = (a.strides[0], a.strides[1]) if as_numpy else (4 * a.stride(0), 4 * a.stride(1))
                if sc != 4 or (a.shape[0] > 1 and (sb % 4 or sb < 12)):
                    return 12, pack
                if a.shape[0] > 1:
                    seen.add(sb)
            if len(seen) > 1:
                return 12, pack
            return (seen.pop() if seen else 12), (lambda a: a)

        pstride, pfix = unify(1)
        nstride, nfix = unify(2)
        keep, table = [], (A.rtr_vertex_range * len(rows))()
        for k, (first, p, n) in enumerate(rows):
            p = pfix(p)
            n = nfix(n) if n is not None else None
            keep += [p, n]
            ptr = (lambda a: a.ctypes.data) if as_numpy else (lambda a: a.data_ptr())
            cnt = int(p.shape[0])
            table[k] = A.rtr_vertex_range(first, cnt, ptr(p) if cnt else None, ptr(n) if n is not None and cnt else None)
        if asynchronous:
            _check(self.lib.rtr_scene_update_vertices_async(self.h, table, len(rows), pstride, nstride), "rtr_scene_update_vertices_async")
            self._async_keep += keep
            return
        if not as_numpy and self.ctx.get_stream() != torch.cuda.current_stream(dev).cuda_stream:
            torch.cuda.current_stream(dev).synchronize()        # the tensors are complete for the context's stream
        iarr = (A.RtrInstance * len(instances))(*instances) if instances is not None else None
        larr = (A.RtrAreaLightInfo * len(lights))(*lights) if lights is not None else None
        _check(self.lib.rtr_scene_update_vertices(self.h, table, len(rows), pstride, nstride, A.VERTICES_HOST if as_numpy else A.VERTICES_DEVICE,
                                                  iarr, len(instances) if instances is not None else 0,
                                                  larr, len(lights) if lights is not None else 0), "rtr_scene_update_vertices")
        del keep

    def update_instances_async(self, transforms, first_instance=0, lights=None):
        """rtr_scene_update_instances_async: update_instances as stream-ordered work — rigid bodies moved from transforms that live on
        the device.  The update is ENQUEUED on the context's stream and the call returns at once, as update_vertices_async.
        transforms: a float32 torch tensor on the scene's device of shape (n, 3, 4), (n, 12), (n, 4, 4) or (n, 16) — row-major
        matrices, the top three rows are used — for the instances first_instance .. first_instance + n - 1 in instance order (lights
        first, then objects); the others keep their transforms.  A strided row view is taken as it is when its rows qualify (stride a
        multiple of 4 bytes and at least 48, 12 adjacent floats), else it is made contiguous.  None: a lights-only update.
        lights: None keeps the light infos; a torch uint8 or float32 tensor of numLights * 96 bytes on the device; or a sequence of
        A.RtrAreaLightInfo, staged once into a device tensor on the context's stream (a non-blocking copy from pinned memory the Scene
        keeps referenced).  numpy arrays raise ValueError: host data stays with update_instances.  The scene needs
        prepare_async_updates() once.  Bad data cannot raise here: update_status() reports it (first_bad_vertex: the instance index, or
        the number of instances plus the light index), and a refused update changes nothing.  The tensors stay referenced until the
        next update_status() or the scene's end."""
        who = "update_instances_async"
        torch = _torch()
        dev = torch.device("cuda", self.ctx.device)
        if isinstance(transforms, np.ndarray) or isinstance(lights, np.ndarray):
            raise ValueError(f"{who}: takes torch tensors on the scene's device, not numpy arrays: host data stays with update_instances")
        if transforms is None and lights is None:
            raise ValueError(f"{who}: no transforms and no lights: nothing to update")
        keep, tptr, stride, count = [], None, 48, 0
        if transforms is not None:
            t = transforms
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
                raise ValueError(f"{who}: transforms must be a float32 torch tensor on the scene's device, got {type(t).__name__}")
            if t.device != dev:
                raise ValueError(f"{who}: transforms live on {t.device}, the scene on {dev}")
            shape = tuple(t.shape)
            if len(shape) == 3 and shape[1:] in ((3, 4), (4, 4)):
                inner_ok = t.stride(2) == 1 and t.stride(1) == 4
            elif len(shape) == 2 and shape[1] in (12, 16):
                inner_ok = t.stride(1) == 1
            else:
                raise ValueError(f"{who}: transforms must be (n, 3, 4), (n, 12), (n, 4, 4) or (n, 16), got {shape}")
            count = int(shape[0])
            if count == 0:
                raise ValueError(f"{who}: transforms without rows (pass None for a lights-only update)")
            row = 4 * t.stride(0)
            if not inner_ok or (count > 1 and (row % 4 or row < 48)):
                t = t.contiguous()
                row = 4 * t.stride(0)
            stride = row if count > 1 else 48
            if first_instance < 0 or first_instance + count > 0xffffffff:
                raise ValueError(f"{who}: first_instance {first_instance} with {count} instances does not fit 32 bits")
            keep.append(t)
            tptr = t.data_ptr()
        lptr, nl = None, 0
        if lights is not None:
            if isinstance(lights, torch.Tensor):
                lt = lights
                if lt.dtype not in (torch.uint8, torch.float32):
                    raise ValueError(f"{who}: a lights tensor must be uint8 or float32, got {lt.dtype}")
                if lt.device != dev:
                    raise ValueError(f"{who}: lights live on {lt.device}, the scene on {dev}")
                lt = lt.contiguous()
                nbytes = lt.numel() * lt.element_size()
                if nbytes % 96:
                    raise ValueError(f"{who}: a lights tensor holds whole RtrAreaLightInfo records of 96 bytes, got {nbytes} bytes")
                nl = nbytes // 96
                keep.append(lt)
            else:
                seq = list(lights)
                nl = len(seq)
                raw = bytes((A.RtrAreaLightInfo * nl)(*seq))
                pinned = torch.frombuffer(bytearray(raw), dtype=torch.uint8).pin_memory() if nl else torch.zeros(0, dtype=torch.uint8)
                with torch.cuda.stream(torch.cuda.ExternalStream(self.ctx.get_stream(), device=dev)):      # staged on the context's stream, once
                    lt = pinned.to(dev, non_blocking=True) if nl else torch.zeros(1, dtype=torch.uint8, device=dev)
                keep += [pinned, lt]
            lptr = lt.data_ptr()
        _check(self.lib.rtr_scene_update_instances_async(self.h, A.VP(tptr) if tptr else None, stride, int(first_instance) if tptr else 0, count,
                                                         C.cast(A.VP(lptr), C.POINTER(A.RtrAreaLightInfo)) if lptr else None, nl),
               "rtr_scene_update_instances_async")
        self._async_keep += keep

    def export_instances(self):
        """rtr_scene_export_instances: the instances as they are now, in instance order — a ctypes array of A.RtrInstance"""
        out = (A.RtrInstance * self._num_instances)()
        _check(self.lib.rtr_scene_export_instances(self.h, out if self._num_instances else None, C.sizeof(out)), "rtr_scene_export_instances")
        return out

    VERTEX_DTYPE = np.dtype([("position", np.float32, 3), ("pad0", np.float32), ("normal", np.float32, 3), ("pad1", np.float32),
                             ("uv", np.float32, 2), ("pad2", np.float32, 2)])

    def export_vertices(self, raw=False):
        """rtr_scene_export_vertices: the device vertex array as it is now — a numpy structured array of RtrVertex records (position,
        pad0, normal, pad1, uv, pad2), or with raw=True its (n, 12) float32 view"""
        out = np.zeros(self._num_vertices, self.VERTEX_DTYPE)
        _check(self.lib.rtr_scene_export_vertices(self.h, out.ctypes.data_as(A.VP) if out.size else None, out.nbytes), "rtr_scene_export_vertices")
        return out.view(np.float32).reshape(-1, 12) if raw else out

    def export_light_tris(self):
        """rtr_scene_export_light_tris: the light-triangle table as it is now -> (records, first): float32 (T, 16) — per triangle of all
        the lights {P0, area} {P1, pdfrec} {P2, -} {unit normal, -} in world space — and uint32 (numLights,), the first record of each light"""
        count = C.c_uint32(0)
        self.lib.rtr_scene_export_light_tris(self.h, None, 0, None, C.byref(count))      # refused unless there are none: reports the count
        n = int(count.value)
        rec = np.zeros((n, 16), np.float32)
        first = np.zeros(self._num_lights, np.uint32)
        _check(self.lib.rtr_scene_export_light_tris(self.h, rec.ctypes.data_as(A.VP) if n else None, n, first.ctypes.data_as(A.VP) if first.size else None,
                                                    C.byref(count)), "rtr_scene_export_light_tris")
        return rec, first

    def prepare_sky(self):
        """rtr_scene_prepare_sky: build the sky table on the device now (synchronous; once per scene), so that the enqueued sky calls
        neither allocate nor join.  The first sky call of a scene that was not prepared builds it the same way."""
        _check(self.lib.rtr_scene_prepare_sky(self.h), "rtr_scene_prepare_sky")

    def export_sky_table(self):
        """rtr_scene_export_sky_table: the device's sky table -> SkyTable (width, height, rows uint32 (H, W), marginal uint64 (H,)):
        the words host_sky_table gives for the scene's HDRI or constant sky"""
        w, h = C.c_uint32(0), C.c_uint32(0)
        self.lib.rtr_scene_export_sky_table(self.h, C.byref(w), C.byref(h), None, 0, None, 0)      # refused: reports the extent
        rows, marginal = np.zeros((h.value, w.value), np.uint32), np.zeros(h.value, np.uint64)
        _check(self.lib.rtr_scene_export_sky_table(self.h, C.byref(w), C.byref(h), rows.ctypes.data_as(A.VP), rows.size, marginal.ctypes.data_as(A.VP),
                                                   h.value), "rtr_scene_export_sky_table")
        return SkyTable(w.value, h.value, rows, marginal)

    def prepare_light_power(self):
        """rtr_scene_prepare_light_power: build the light-power table on the device now (synchronous; once per scene), so that the enqueued
        power calls neither allocate nor join.  The first power call of a scene that was not prepared builds it the same way; from then on
        every update of the lights or of their triangles remakes it on its own stream."""
        _check(self.lib.rtr_scene_prepare_light_power(self.h), "rtr_scene_prepare_light_power")

    def export_light_power(self):
        """rtr_scene_export_light_power: the device's light-power table as it is now -> (weights, cdf): uint32 (T,) and uint64 (T,), one
        integer weight and one inclusive sum per light triangle of all the lights, in export_light_tris' order: the words
        host_light_power gives for export_light_tris() and the scene's lights"""
        count = C.c_uint32(0)
        self.lib.rtr_scene_export_light_power(self.h, None, None, 0, C.byref(count))      # refused unless there are none: reports the count
        n = int(count.value)
        w, cdf = np.zeros(n, np.uint32), np.zeros(n, np.uint64)
        _check(self.lib.rtr_scene_export_light_power(self.h, w.ctypes.data_as(A.VP) if n else None, cdf.ctypes.data_as(A.VP) if n else None, n,
                                                     C.byref(count)), "rtr_scene_export_light_power")
        return w, cdf

    def set_instance_masks(self, masks):
        """rtr_scene_set_instance_masks: one 8-bit cull mask per instance, in instance order (array-like of uint8; default 0xff).  Only
        the masked queries (trace_rays / trace_occlusion with cull_mask or ray_masks) look at them; renders ignore them."""
        m = np.asarray(masks)
        if m.ndim != 1 or m.dtype.kind not in "ui" or (m.size and (int(m.min()) < 0 or int(m.max()) > 0xff)):
            raise ValueError(f"set_instance_masks: masks must be a 1-D array of values 0..255, got {m.dtype} {m.shape}")
        m = np.ascontiguousarray(m, dtype=np.uint8)
        _check(self.lib.rtr_scene_set_instance_masks(self.h, m.ctypes.data_as(A.VP) if m.size else None, int(m.size)), "rtr_scene_set_instance_masks")

    def instance_masks(self):
        """rtr_scene_get_instance_masks: the masks as a uint8 array, in instance order (0xff where never set)"""
        n = self._num_instances
        m = np.zeros(n, np.uint8)
        _check(self.lib.rtr_scene_get_instance_masks(self.h, m.ctypes.data_as(A.VP) if n else None, n), "rtr_scene_get_instance_masks")
        return m

    def update_lights(self, lights):
        arr = (A.RtrAreaLightInfo * len(lights))(*lights)
        _check(self.lib.rtr_scene_update_lights(self.h, arr, len(lights)), "rtr_scene_update_lights")

    def close(self):
        if self.h:
            self.lib.rtr_scene_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Frame:
    def __init__(self, ctx, width, rows, images=A.IMAGES_FRAMEBUFFER):
        self.ctx, self.lib = ctx, ctx.lib
        self.width, self.rows = width, rows
        self.h = A.VP()
        _check(self.lib.rtr_frame_create(ctx.h, width, rows, images, C.byref(self.h)), "rtr_frame_create")

    def download(self, which=A.IMAGE_SHADOWED):
        if which == A.IMAGE_HDR:
            out = np.empty((self.rows, self.width, 4), dtype=np.float32)
        else:
            out = np.empty((self.rows, self.width), dtype=np.uint32)
        _check(self.lib.rtr_frame_download(self.h, which, out.ctypes.data_as(A.VP), out.nbytes), "rtr_frame_download")
        return out

    def bind_external(self, which, device_ptr, nbytes):
        _check(self.lib.rtr_frame_bind_external(self.h, which, A.VP(device_ptr), nbytes), "rtr_frame_bind_external")

    def device_ptr(self, which=A.IMAGE_SHADOWED):
        p, n = A.VP(), C.c_size_t()
        _check(self.lib.rtr_frame_device_ptr(self.h, which, C.byref(p), C.byref(n)), "rtr_frame_device_ptr")
        return p.value, n.value

    def clear(self):
        _check(self.lib.rtr_frame_clear(self.h), "rtr_frame_clear")

    def denoise_combine(self, iterations=4):
        """reference frame loop tail (application.cppm:391-445): 4 x a-trous on both sampled images, then combine."""
        _check(self.lib.rtr_denoise_combine(self.h, iterations), "rtr_denoise_combine")

    def denoise_combine_async(self, iterations=4):
        """the same passes enqueued on the frame's context stream (behind a render or a batch launch that wrote the frame), not
        waited for: wait() joins, and the next frame's render on another context runs under them"""
        _check(self.lib.rtr_denoise_combine_async(self.h, iterations), "rtr_denoise_combine_async")

    def wait(self):
        _check(self.lib.rtr_frame_wait(self.h), "rtr_frame_wait")

    def stats(self):
        s = A.rtr_frame_stats()
        _check(self.lib.rtr_frame_get_stats(self.h, C.byref(s)), "rtr_frame_get_stats")
        return s

    def close(self):
        if self.h:
            self.lib.rtr_frame_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def make_params(width, height, spp=1, shadow_rays=3, images=A.IMAGES_FRAMEBUFFER, band_rows=8, shard_index=0,
                shard_count=1, accumulate=0, accumulated_frames=0, collect_stats=0, pipeline=0):
    return A.rtr_render_params(width, height, spp, shadow_rays, images, band_rows, shard_index, shard_count,
                               accumulate, accumulated_frames, collect_stats, pipeline)


def shard_rows(height, band_rows=8, shard_count=1):
    return A.hip_lib().rtr_shard_rows(height, band_rows, shard_count)


def render(scene, camera, scene_info, params, frame, asynchronous=False):
    fn = scene.lib.rtr_render_async if asynchronous else scene.lib.rtr_render
    _check(fn(scene.h, C.byref(camera), C.byref(scene_info), C.byref(params), frame.h), "rtr_render")


def render_split(scene, camera, scene_info, params, frame, parts, asynchronous=False):
    """rtr_render_split[_async]: ONE frame as `parts` band-shards on streams of their own, written in place (the latency form)"""
    fn = scene.lib.rtr_render_split_async if asynchronous else scene.lib.rtr_render_split
    _check(fn(scene.h, C.byref(camera), C.byref(scene_info), C.byref(params), frame.h, int(parts)), "rtr_render_split")


def marshal_batch(cameras, scene_infos, frames):
    """the argument arrays of rtr_render_batch_async, built once (a caller that knows its next launches prepares them ahead)"""
    n = len(frames)
    return ((A.RtrCameraData * n)(*cameras), (A.RtrSceneInfo * n)(*scene_infos), (A.VP * n)(*[f.h.value for f in frames]), n)


def render_batch(scene, cameras, scene_infos, params, frames, marshalled=None):
    """rtr_render_batch_async: len(frames) <= A.MAX_BATCH frames in one launch of every kernel; asynchronous, join with frames[k].wait()."""
    cams, infos, hs, n = marshalled if marshalled is not None else marshal_batch(cameras, scene_infos, frames)
    _check(scene.lib.rtr_render_batch_async(scene.h, cams, infos, C.byref(params), hs, n), "rtr_render_batch_async")


def render_batch_limit(scene, params, num_area_lights):
    """rtr_render_batch_limit: how many frames of these params one launch of the pipeline takes (<= A.MAX_BATCH)"""
    n = C.c_uint32(0)
    _check(scene.lib.rtr_render_batch_limit(scene.h, C.byref(params), num_area_lights, C.byref(n)), "rtr_render_batch_limit")
    return int(n.value)


def deinterleave_bands(ctx, gathered_ptr, dst_ptr, width, height, band_rows, shard_count):
    _check(ctx.lib.rtr_deinterleave_bands(ctx.h, A.VP(gathered_ptr), A.VP(dst_ptr), width, height, band_rows, shard_count),
           "rtr_deinterleave_bands")


def deinterleave_images(ctx, gathered_ptr, dst_ptrs, width, height, band_rows, shard_count):
    """rtr_deinterleave_images: [shard][image][local row][x] gather buffer -> len(dst_ptrs) whole images, one launch, on the ctx stream"""
    n = len(dst_ptrs)
    arr = (A.VP * max(n, 1))(*[A.VP(p) for p in dst_ptrs])
    _check(ctx.lib.rtr_deinterleave_images(ctx.h, A.VP(gathered_ptr), n, arr, width, height, band_rows, shard_count), "rtr_deinterleave_images")


def host_build_bvh(desc):
    """rtr_host_build_bvh: the product's BVH builder without a device -> (stats, nodes, tris)."""
    lib = A.hip_lib()
    st = A.rtr_scene_stats()
    _check(lib.rtr_host_build_bvh(C.byref(desc), C.byref(st), None, 0, None, 0), "rtr_host_build_bvh")
    nodes = (A.RtrBvhNode * st.numNodes)()
    tris = (A.RtrBvhTri * max(st.numTriangles, 1))()
    _check(lib.rtr_host_build_bvh(C.byref(desc), C.byref(st), nodes, C.sizeof(nodes), tris, C.sizeof(tris)), "rtr_host_build_bvh")
    return st, nodes, tris


def host_tree_cost(nodes, grid):
    """rtr_host_tree_cost: the host restatement of Scene.tree_cost, no device -> TreeCost.  nodes: a ctypes RtrBvhNode array (what
    host_build_bvh or export_bvh return) or a C-contiguous numpy array of its bytes; grid: the RtrBvhGrid its planes live on (stats.grid /
    the export's third element)."""
    lib = A.hip_lib()
    c = A.rtr_tree_cost()
    if isinstance(nodes, np.ndarray):
        nodes = np.ascontiguousarray(nodes)
        ptr, nbytes = nodes.ctypes.data_as(A.VP), nodes.nbytes
    else:
        ptr, nbytes = C.cast(nodes, A.VP), C.sizeof(nodes)
    _check(lib.rtr_host_tree_cost(ptr, nbytes, C.byref(grid), C.byref(c)), "rtr_host_tree_cost")
    return TreeCost(c)


def host_build_bvh_wide(desc):
    """rtr_host_build_bvh_wide: the build plus the 4-wide view the device would hold for it -> BvhExport (nodes, tris, grid) with
    .wide and .stats; what the oracle needs to walk a shadow ray the way k_shadow_trace4 does, on a CPU-only box."""
    lib = A.hip_lib()
    st = A.rtr_scene_stats()
    _check(lib.rtr_host_build_bvh_wide(C.byref(desc), C.byref(st), None, 0, None, 0, None, 0), "rtr_host_build_bvh_wide")
    nodes = (A.RtrBvhNode * st.numNodes)()
    tris = (A.RtrBvhTri * max(st.numTriangles, 1))()
    wide = (A.RtrWideNode * st.numWideNodes)()
    _check(lib.rtr_host_build_bvh_wide(C.byref(desc), C.byref(st), nodes, C.sizeof(nodes), tris, C.sizeof(tris), wide, C.sizeof(wide)), "rtr_host_build_bvh_wide")
    out = BvhExport((nodes, tris, st.grid))
    out.wide = wide
    out.stats = st
    return out


def trace_top_nodes():
    """rtr_trace_top_nodes: the 4-wide records the any-hit kernel of this build keeps in LDS"""
    return int(A.hip_lib().rtr_trace_top_nodes())


def host_wide_resident(wide, grid, lights, top=None):
    """rtr_host_wide_resident: the resident order of a breadth-first 4-wide view, no device -> a ctypes RtrWideNode array.  wide: what
    host_build_bvh_wide(...).wide or export_bvh().wide hold; grid: their grid (stats.grid / the export's third element); lights: the
    scene's A.RtrAreaLightInfo records (a sequence or a ctypes array, may be empty); top: the size of the best-first top
    (default: trace_top_nodes())."""
    lib = A.hip_lib()
    n = len(lights) if lights is not None else 0
    li = (A.RtrAreaLightInfo * n)(*lights) if n else None
    out = (A.RtrWideNode * len(wide))()
    _check(lib.rtr_host_wide_resident(wide, C.sizeof(wide), C.byref(grid), li, n, trace_top_nodes() if top is None else int(top), out), "rtr_host_wide_resident")
    return out


# ---- ray queries (rtr_trace_rays, rtr_camera_rays_async) ----------------------------------------------------------------------------
class QueryResult:
    """What trace_rays gives back.  Closest hit: t, u, v (float32), custom_index, primitive_id (int32, -1 for a miss; t = the ray's tmax
    then).  Any hit: occluded (uint8, 1 = occluded).  The other fields are None.  stats: rtr_query_stats of the counting form, or None.
    hits: the closest-hit records themselves, an (N, 8) int32 array of RtrHit (what hit_surfaces takes), or None."""
    t = u = v = custom_index = primitive_id = occluded = stats = hits = None


def _torch():
    import torch
    return torch


def _join_ctx_stream(ctx, torch, dev):
    """torch's current stream waits for what the context's stream holds (a no-op when they are one stream)"""
    cs = ctx.get_stream()
    cur = torch.cuda.current_stream(dev)
    if cs != cur.cuda_stream:
        torch.cuda.ExternalStream(cs, device=dev).synchronize()


def _check_async(ctx, torch, dev, who, asynchronous, collect_stats=False):
    """what an asynchronous call needs: the context on torch's current stream, so that its results are ordered for torch without a
    join, and no counting form, which reads back"""
    if asynchronous and collect_stats:
        raise ValueError(f"{who}: collect_stats needs the synchronous form")
    if asynchronous and ctx.get_stream() != torch.cuda.current_stream(dev).cuda_stream:
        raise ValueError(f"{who}: an asynchronous call needs the context on torch's current stream (ctx.set_stream)")


def _join_torchs_stream(ctx, torch, dev, asynchronous=False):
    """before a synchronous call: the inputs (and the outputs' memory) are ready for the context's stream"""
    if not asynchronous and ctx.get_stream() != torch.cuda.current_stream(dev).cuda_stream:
        torch.cuda.current_stream(dev).synchronize()


def _ptr(x, n=1):
    """tensor x's address for the library; null for None and for a call of n = 0 elements"""
    return A.VP(x.data_ptr()) if x is not None and n else None


def _call_query(ctx, name, asynchronous, collect_stats, *args):
    """lib.<name>_async(*args), or lib.<name>(*args, stats or null) -> the rtr_query_stats of the counting form, else None"""
    if asynchronous:
        _check(getattr(ctx.lib, name + "_async")(*args), name + "_async")
        return None
    st = A.rtr_query_stats() if collect_stats else None
    _check(getattr(ctx.lib, name)(*args, C.byref(st) if st is not None else None), name)
    return st


def _device_array(torch, x, dtype, np_dtype, name, dev, who):
    """an (N, 8) array of 32-bit words on dev: a device tensor as it is (checked), a numpy array copied there"""
    if isinstance(x, np.ndarray):
        if x.dtype != np_dtype or x.ndim != 2 or x.shape[1] != 8:
            raise ValueError(f"{who}: {name} must be {np.dtype(np_dtype)} (N, 8), got {x.dtype} {x.shape}")
        return torch.from_numpy(np.ascontiguousarray(x)).to(dev), True
    if isinstance(x, torch.Tensor):
        if x.dtype != dtype or x.dim() != 2 or x.shape[1] != 8:
            raise ValueError(f"{who}: {name} must be {dtype} (N, 8), got {x.dtype} {tuple(x.shape)}")
        if x.device != dev:
            raise ValueError(f"{who}: {name} live on {x.device}, the context on {dev}")
        if not x.is_contiguous():
            raise ValueError(f"{who}: {name} must be contiguous")
        return x, False
    raise ValueError(f"{who}: {name} must be a torch tensor or a numpy array, got {type(x).__name__}")


def _device_vector(torch, x, dtype, np_dtypes, n, name, dev, who, as_numpy=None):
    """an (n,) vector of 8- or 32-bit words on dev, or None for None: a device tensor of dtype as it is (checked), a numpy array of one
    of np_dtypes copied there as the first of them.  as_numpy: whether the rays came as numpy, which x must then do too (None: either)"""
    if x is None:
        return None
    if not isinstance(x, (np.ndarray, torch.Tensor)):
        raise ValueError(f"{who}: {name} must be a torch tensor or a numpy array, got {type(x).__name__}")
    is_numpy = isinstance(x, np.ndarray)
    ok = (x.dtype in np_dtypes) if is_numpy else (x.dtype == dtype and x.device == dev and x.is_contiguous())
    if not ok or tuple(x.shape) != (n,) or (as_numpy is not None and is_numpy != as_numpy):
        like = "" if as_numpy is None else ", numpy or tensor as the rays are"
        raise ValueError(f"{who}: {name} must be {dtype} ({n},), a numpy array or a contiguous tensor on {dev}{like}; got {x.dtype} {tuple(x.shape)}")
    return torch.from_numpy(np.ascontiguousarray(x).view(np_dtypes[0])).to(dev) if is_numpy else x


def _cull_mask_args(torch, who, cull_mask, ray_masks, n, dev):
    """(ray-mask tensor or None, cull mask) of a masked query; cull_mask None -> 0xff.  ray_masks: a contiguous uint8 (N,) tensor on
    dev, or a numpy array, which is uploaded."""
    return _device_vector(torch, ray_masks, torch.uint8, (np.uint8,), n, "ray_masks", dev, who), 0xff if cull_mask is None else int(cull_mask)


def _ray_flags(who, ray_flags, opaque):
    """the extra flag bits of a query (A.QUERY_CULL_*), checked for the combinations the interface refuses — both face flags; more than
    one of opaque, QUERY_CULL_OPAQUE and QUERY_CULL_NO_OPAQUE — before anything is launched.  Unknown bits are left to the library, which
    refuses them.  QUERY_ANY is not taken here: trace_rays has any_hit for it."""
    f = int(ray_flags)
    if f < 0 or f > 0xffffffff:
        raise ValueError(f"{who}: ray_flags must be a 32-bit mask, got {ray_flags!r}")
    if f & A.QUERY_ANY:
        raise ValueError(f"{who}: QUERY_ANY is not a ray flag here (trace_rays(any_hit=True) or trace_occlusion)")
    if (f & A.QUERY_CULL_BACK_FACING) and (f & A.QUERY_CULL_FRONT_FACING):
        raise ValueError(f"{who}: QUERY_CULL_BACK_FACING and QUERY_CULL_FRONT_FACING exclude each other")
    if (1 if opaque or f & A.QUERY_OPAQUE else 0) + (1 if f & A.QUERY_CULL_OPAQUE else 0) + (1 if f & A.QUERY_CULL_NO_OPAQUE else 0) > 1:
        raise ValueError(f"{who}: at most one of opaque (QUERY_OPAQUE), QUERY_CULL_OPAQUE and QUERY_CULL_NO_OPAQUE")
    return f


def trace_rays(scene, rays, any_hit=False, opaque=False, collect_stats=False, ctx=None, asynchronous=False, cull_mask=None, ray_masks=None, ray_flags=0):
    """rtr_trace_rays: rays is a contiguous float32 (N, 8) tensor on the context's device — rows are RtrRay (origin, tmin, direction,
    tmax) — whose results come back as device tensors without a copy, or a numpy array, which is copied to the device and whose results
    come back as numpy.  any_hit: occlusion only (RTR_QUERY_ANY); opaque: no opacity-map test (RTR_QUERY_OPAQUE).  ctx: the context whose
    stream carries the work (default: the scene's).  asynchronous: enqueue and return (rtr_trace_rays_async); the context must then be
    on torch's current stream (ctx.set_stream), so that the results are ordered for torch without a join.  collect_stats: the counting
    form, synchronous.  Wrong shape, dtype, device or layout raises ValueError before anything is launched.
    cull_mask (8 bits) and ray_masks (one uint8 per ray: a device tensor, or a numpy array that is uploaded): traceRayEXT's cullMask —
    ray k sees the instances whose mask (Scene.set_instance_masks) meets cull_mask & ray_masks[k]; with either given the call is
    rtr_trace_rays_masked, with both None it is rtr_trace_rays exactly as before.
    ray_flags: the culling flags of traceRayEXT's rayFlags, or-ed — A.QUERY_CULL_BACK_FACING or A.QUERY_CULL_FRONT_FACING (facing by the
    as-wound object-space normal, RtrSurface.geom_normal's side), A.QUERY_CULL_OPAQUE or A.QUERY_CULL_NO_OPAQUE (only the alpha-tested
    layer / only the rest) — for the whole launch; ValueError for the combinations Vulkan forbids.  0: the call as before."""
    ray_flags = _ray_flags("trace_rays", ray_flags, opaque)
    torch = _torch()
    ctx = ctx or scene.ctx
    dev = torch.device("cuda", ctx.device)
    r, as_numpy = _device_array(torch, rays, torch.float32, np.float32, "rays", dev, "trace_rays")
    _check_async(ctx, torch, dev, "trace_rays", asynchronous, collect_stats)
    n = int(r.shape[0])
    flags = (A.QUERY_ANY if any_hit else A.QUERY_CLOSEST) | (A.QUERY_OPAQUE if opaque else 0) | ray_flags
    hits = occ = None
    if any_hit:
        occ = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)[:n]
    else:
        hits = torch.empty((n, 8), dtype=torch.int32, device=dev)
    _join_torchs_stream(ctx, torch, dev, asynchronous)
    out = QueryResult()
    rm = None
    if cull_mask is not None or ray_masks is not None:
        rm, cm = _cull_mask_args(torch, "trace_rays", cull_mask, ray_masks, n, dev)
        name, args = "rtr_trace_rays_masked", (_ptr(r, n), _ptr(rm, n), n, flags, cm, _ptr(hits, n), _ptr(occ, n))
    else:
        name, args = "rtr_trace_rays", (_ptr(r, n), n, flags, _ptr(hits, n), _ptr(occ, n))
    out.stats = _call_query(ctx, name, asynchronous, collect_stats, ctx.h, scene.h, *args)
    if any_hit:
        out.occluded = occ
    else:
        f = hits.view(torch.float32)
        out.t, out.u, out.v = f[:, 0], f[:, 1], f[:, 2]
        out.custom_index, out.primitive_id = hits[:, 3], hits[:, 4]
        out.hits = hits
    if as_numpy:
        for k in ("t", "u", "v", "custom_index", "primitive_id", "occluded", "hits"):
            x = getattr(out, k)
            if x is not None:
                setattr(out, k, x.cpu().numpy())
    out._keep = (r, hits, occ, rm)       # an asynchronous query's buffers stay alive with its result
    return out


class MultiHitResult:
    """What trace_rays_multi gives back.  hits: the (N, K, 8) int32 array of RtrHit records, ray-major — slot j of ray k is its j-th hit by
    (t, customIndex, primitiveId), slots past counts[k] are the ray's miss record (t = its tmax, ids -1).  counts: (N,) int32.
    t, u, v (float32) and custom_index, primitive_id (int32) are (N, K) views of hits.  last: the (N, 8) last-slot records, a contiguous
    copy made on first use — what the next call of a chain takes as `after`.  stats: rtr_query_stats of the counting form, or None."""
    hits = counts = t = u = v = custom_index = primitive_id = stats = None
    _last = None

    @property
    def last(self):
        if self._last is None:
            x = self.hits[:, -1, :]
            self._last = np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x.contiguous()
        return self._last


def trace_rays_multi(scene, rays, max_hits, after=None, opaque=False, ray_flags=0, cull_mask=None, ray_masks=None, collect_stats=False, ctx=None,
                     asynchronous=False):
    """rtr_trace_rays_multi: the first max_hits (1 .. A.MULTIHIT_MAX) hits along every ray, in order — the members of the set the
    closest-hit trace_rays would consider under the same opaque, ray_flags, cull_mask and ray_masks, smallest first by
    (t, customIndex, primitiveId).  rays, opaque, ray_flags, cull_mask, ray_masks, collect_stats, ctx and asynchronous are trace_rays';
    numpy rays give numpy results.  With max_hits=1 and no `after` the records are trace_rays(..., cull_mask=0xff)'s, bit for bit.
    after: None, a MultiHitResult (its .last is taken) or (N, 8) int32 RtrHit records: ray k reports only hits whose key is strictly
    greater than after[k]'s, and nothing once after[k] is a miss record — so
        r = trace_rays_multi(scene, rays, 2)
        while int(r.counts.sum()):
            ...                                   # r.hits[:, :, :], r.counts
            r = trace_rays_multi(scene, rays, 2, after=r)
    enumerates every hit of every ray exactly once, ties in t included.  The scene must not change inside a chain.
    The hits compose with hit_surfaces as K rays apiece: hit_surfaces(scene, rays.repeat_interleave(K, 0), r.hits.view(-1, 8)) gives the
    surface of every slot (a miss record gives the sky), ray-major.
    ValueError before any device work for max_hits outside 1 .. 8, A.QUERY_ANY among ray_flags and the flag combinations Vulkan forbids."""
    k_hits = int(max_hits)
    if k_hits < 1 or k_hits > A.MULTIHIT_MAX:
        raise ValueError(f"trace_rays_multi: max_hits must be 1 .. {A.MULTIHIT_MAX}, got {max_hits!r}")
    ray_flags = _ray_flags("trace_rays_multi", ray_flags, opaque)
    torch = _torch()
    ctx = ctx or scene.ctx
    dev = torch.device("cuda", ctx.device)
    r, as_numpy = _device_array(torch, rays, torch.float32, np.float32, "rays", dev, "trace_rays_multi")
    n = int(r.shape[0])
    a = None
    if after is not None:
        if isinstance(after, MultiHitResult):
            after = after.last
        a, an = _device_array(torch, after, torch.int32, np.int32, "after", dev, "trace_rays_multi")
        if an != as_numpy:
            raise ValueError("trace_rays_multi: rays and after must both be numpy arrays or both be tensors")
        if a.shape[0] != n:
            raise ValueError(f"trace_rays_multi: {n} rays but {a.shape[0]} after records")
    _check_async(ctx, torch, dev, "trace_rays_multi", asynchronous, collect_stats)
    rm, cm = _cull_mask_args(torch, "trace_rays_multi", cull_mask, ray_masks, n, dev)
    flags = (A.QUERY_OPAQUE if opaque else 0) | ray_flags
    hits = torch.empty((n, k_hits, 8), dtype=torch.int32, device=dev)
    counts = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
    _join_torchs_stream(ctx, torch, dev, asynchronous)
    out = MultiHitResult()
    out.stats = _call_query(ctx, "rtr_trace_rays_multi", asynchronous, collect_stats, ctx.h, scene.h, _ptr(r, n), _ptr(rm, n), n, k_hits, flags, cm, _ptr(a, n),
                            _ptr(hits, n), _ptr(counts, n))
    out.hits, out.counts = (hits.cpu().numpy(), counts.cpu().numpy()) if as_numpy else (hits, counts)
    f = out.hits.view(np.float32) if as_numpy else out.hits.view(torch.float32)
    out.t, out.u, out.v = f[:, :, 0], f[:, :, 1], f[:, :, 2]
    out.custom_index, out.primitive_id = out.hits[:, :, 3], out.hits[:, :, 4]
    out._keep = (r, a, rm, hits, counts)     # an asynchronous query's buffers stay alive with its result
    return out


def occlusion_scratch_bytes(lib, n):
    """rtr_occlusion_scratch_bytes: device scratch a queued occlusion query of n rays needs"""
    b = C.c_size_t(0)
    _check(lib.rtr_occlusion_scratch_bytes(int(n), C.byref(b)), "rtr_occlusion_scratch_bytes")
    return int(b.value)


def trace_occlusion(scene, rays, opaque=False, collect_stats=False, ctx=None, asynchronous=False, start_leaves=None, cull_mask=None, ray_masks=None, ray_flags=0):
    """rtr_trace_occlusion: the queued occlusion query — the same bytes as trace_rays(any_hit=True), answered by the renderer's any-hit
    machinery (rays binned by direction octant, persistent waves over the 4-wide tree).  rays, opaque, ctx, asynchronous, collect_stats
    and the QueryResult (occluded, stats) as in trace_rays.  The query's scratch is a uint8 device tensor kept on the context and grown
    when a longer ray array comes; queries on one context are ordered on its stream, so they share it.
    start_leaves (rtr_trace_occlusion_hinted): one int32 start hint per ray — light_rays(hints=True)'s or hit_leaves' — as an (N,) int32
    device tensor or numpy array like the rays; any value is safe and none changes a byte, only the work.  None: the unhinted query.
    cull_mask, ray_masks: as in trace_rays; with either given the call is rtr_trace_occlusion_masked (hinted or not), with both None the
    entry points called before.  ray_flags: the culling flags, as in trace_rays; every route writes the same bytes, and a hinted leaf
    whose hits are all culled does not stop its ray."""
    ray_flags = _ray_flags("trace_occlusion", ray_flags, opaque)
    torch = _torch()
    ctx = ctx or scene.ctx
    dev = torch.device("cuda", ctx.device)
    r, as_numpy = _device_array(torch, rays, torch.float32, np.float32, "rays", dev, "trace_occlusion")
    _check_async(ctx, torch, dev, "trace_occlusion", asynchronous, collect_stats)
    n = int(r.shape[0])
    sl = _device_vector(torch, start_leaves, torch.int32, (np.int32,), n, "start_leaves", dev, "trace_occlusion", as_numpy)
    need = occlusion_scratch_bytes(ctx.lib, n)
    scratch = getattr(ctx, "_occlusion_scratch", None)
    if scratch is None or scratch.numel() < need:
        scratch = ctx._occlusion_scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    occ = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)[:n]
    _join_torchs_stream(ctx, torch, dev, asynchronous)
    flags = (A.QUERY_OPAQUE if opaque else 0) | ray_flags
    tail = (_ptr(scratch, n), scratch.numel() if n else 0, _ptr(occ, n))
    out = QueryResult()
    rm = None
    if cull_mask is not None or ray_masks is not None:
        rm, cm = _cull_mask_args(torch, "trace_occlusion", cull_mask, ray_masks, n, dev)
        name, args = "rtr_trace_occlusion_masked", (_ptr(r, n), _ptr(sl, n), _ptr(rm, n), n, flags, cm) + tail
    elif sl is not None:
        name, args = "rtr_trace_occlusion_hinted", (_ptr(r, n), _ptr(sl, n), n, flags) + tail
    else:
        name, args = "rtr_trace_occlusion", (_ptr(r, n), n, flags) + tail
    out.stats = _call_query(ctx, name, asynchronous, collect_stats, ctx.h, scene.h, *args)
    out.occluded = occ.cpu().numpy() if as_numpy else occ
    out._keep = (r, sl, occ, scratch, rm)    # an asynchronous query's buffers stay alive with its result
    return out


def camera_rays(ctx, camera, width, height, spp=1):
    """rtr_camera_rays_async: the (width * height * spp, 8) float32 device tensor of the camera rays the renderer traces for `camera`,
    row k = (py * width + px) * spp + i; ready for torch's current stream when it returns."""
    torch = _torch()
    dev = torch.device("cuda", ctx.device)
    n = int(width) * int(height) * int(spp)
    out = torch.empty((max(n, 1), 8), dtype=torch.float32, device=dev)[:n]
    _join_torchs_stream(ctx, torch, dev)                    # the tensor's memory is free for the context's stream
    _check(ctx.lib.rtr_camera_rays_async(ctx.h, C.byref(camera), int(width), int(height), int(spp), A.VP(out.data_ptr()) if n else None),
           "rtr_camera_rays_async")
    _join_ctx_stream(ctx, torch, dev)
    return out


class SurfaceResult:
    """What hit_surfaces gives back: views into one (N, 20) array of RtrSurface records (raw, float32).  position, normal, geom_normal,
    color (N, 3) and roughness, metallic (N,) and uv (N, 2) are float32; kind (A.SURFACE_*) and object_index (the ObjectInfo row of an
    object, the light index of a light, -1 otherwise) are int32."""
    raw = position = normal = geom_normal = color = roughness = metallic = uv = kind = object_index = None


def hit_surfaces(scene, rays, hits, ctx=None, asynchronous=False):
    """rtr_hit_surfaces: what the closest-hit shader computes for each hit.  rays: as trace_rays takes them (float32 (N, 8)); hits: the
    QueryResult of a closest-hit trace_rays or its (N, 8) int32 RtrHit records.  Device tensors give device results without a copy; numpy
    in gives numpy out (both must then be numpy).  ctx and asynchronous as in trace_rays: an asynchronous call needs the context on
    torch's current stream.  Wrong shape, dtype, device, layout or a length mismatch raises ValueError before anything is launched."""
    torch = _torch()
    ctx = ctx or scene.ctx
    dev = torch.device("cuda", ctx.device)
    if isinstance(hits, QueryResult):
        if hits.hits is None:
            raise ValueError("hit_surfaces: the QueryResult holds no hit records (an any-hit query)")
        hits = hits.hits
    r, rn = _device_array(torch, rays, torch.float32, np.float32, "rays", dev, "hit_surfaces")
    h, hn = _device_array(torch, hits, torch.int32, np.int32, "hits", dev, "hit_surfaces")
    if rn != hn:
        raise ValueError("hit_surfaces: rays and hits must both be numpy arrays or both be tensors")
    if r.shape[0] != h.shape[0]:
        raise ValueError(f"hit_surfaces: {r.shape[0]} rays but {h.shape[0]} hits")
    _check_async(ctx, torch, dev, "hit_surfaces", asynchronous)
    n = int(r.shape[0])
    out = torch.empty((n, 20), dtype=torch.float32, device=dev)
    _join_torchs_stream(ctx, torch, dev, asynchronous)
    args = (A.VP(r.data_ptr()), A.VP(h.data_ptr()), n, A.VP(out.data_ptr())) if n else (None, None, 0, None)
    if asynchronous:
        _check(ctx.lib.rtr_hit_surfaces_async(ctx.h, scene.h, *args), "rtr_hit_surfaces_async")
    else:
        _check(ctx.lib.rtr_hit_surfaces(ctx.h, scene.h, *args), "rtr_hit_surfaces")
    raw = out.cpu().numpy() if rn else out
    words = raw.view(np.int32) if rn else raw.view(torch.int32)
    res = SurfaceResult()
    res.raw = raw
    res.position, res.normal, res.geom_normal, res.color = raw[:, 0:3], raw[:, 4:7], raw[:, 8:11], raw[:, 12:15]
    res.metallic, res.roughness, res.uv = raw[:, 11], raw[:, 15], raw[:, 16:18]
    res.kind, res.object_index = words[:, 3], words[:, 7]
    res._keep = (r, h)                   # an asynchronous call's inputs stay alive with its result
    return res


def hit_leaves(scene, hits, ctx=None, asynchronous=False):
    """rtr_hit_leaves: the start hint of each hit — the code of the BVH leaf its triangle sits in, 0 for a miss or ids out of range — as
    int32 (N,), for rays the caller makes from a hit and hands to trace_occlusion(start_leaves=...).  hits: a closest-hit QueryResult or
    its (N, 8) int32 RtrHit records; a device tensor gives a device tensor, numpy gives numpy.  The scene's first call builds its
    triangle -> leaf table.  ctx and asynchronous as in trace_rays."""
    torch = _torch()
    ctx = ctx or scene.ctx
    dev = torch.device("cuda", ctx.device)
    if isinstance(hits, QueryResult):
        if hits.hits is None:
            raise ValueError("hit_leaves: the QueryResult holds no hit records (an any-hit query)")
        hits = hits.hits
    h, as_numpy = _device_array(torch, hits, torch.int32, np.int32, "hits", dev, "hit_leaves")
    _check_async(ctx, torch, dev, "hit_leaves", asynchronous)
    n = int(h.shape[0])
    out = torch.empty(n, dtype=torch.int32, device=dev)
    _join_torchs_stream(ctx, torch, dev, asynchronous)
    fn = ctx.lib.rtr_hit_leaves_async if asynchronous else ctx.lib.rtr_hit_leaves
    _check(fn(ctx.h, scene.h, A.VP(h.data_ptr()) if n else None, n, A.VP(out.data_ptr()) if n else None), "rtr_hit_leaves")
    if as_numpy:
        return out.cpu().numpy()
    out._keep = h                        # an asynchronous call's input stays alive with its result
    return out


# ---- direct lighting for ray-query hits (rtr_light_rays, rtr_shade_hits, rtr_tonemap_pack) ----------------------------------------
class RadianceResult:
    """What shade_hits and direct_light give back: views into one (N, 12) array of RtrRadiance records (raw, float32).  shadowed,
    unshadowed, analytic (N, 3) float32 — a sum that was not asked for is zeros — and kind (A.SURFACE_*) int32."""
    raw = shadowed = unshadowed = analytic = kind = None


def make_light_params(num_area_lights, shadow_rays=3, frame=0, width=0, spp=1, outputs=A.LIGHT_SHADOWED):
    """rtr_light_params.  width / spp say which pixel a hit belongs to (camera_rays' order) and matter only without explicit seeds"""
    return A.rtr_light_params(int(num_area_lights), int(shadow_rays), int(frame) & 0xffffffff, int(width), int(spp), int(outputs))


def light_slots(scene, params):
    """rtr_light_slots: Q, the slots (light rays, visibility bytes) every hit owns for these params"""
    q = C.c_uint32(0)
    _check(scene.lib.rtr_light_slots(scene.h, C.byref(params), C.byref(q)), "rtr_light_slots")
    return int(q.value)


def _light_inputs(torch, scene, rays, hits, seeds, ctx, who, asynchronous):
    """the checked device arrays of light_rays / shade_hits: (rays, hits, seeds or None, numpy in?)"""
    dev = torch.device("cuda", ctx.device)
    if isinstance(hits, QueryResult):
        if hits.hits is None:
            raise ValueError(f"{who}: the QueryResult holds no hit records (an any-hit query)")
        hits = hits.hits
    r, rn = _device_array(torch, rays, torch.float32, np.float32, "rays", dev, who)
    h, hn = _device_array(torch, hits, torch.int32, np.int32, "hits", dev, who)
    if rn != hn:
        raise ValueError(f"{who}: rays and hits must both be numpy arrays or both be tensors")
    if r.shape[0] != h.shape[0]:
        raise ValueError(f"{who}: {r.shape[0]} rays but {h.shape[0]} hits")
    sd = _device_vector(torch, seeds, torch.int32, (np.int32, np.uint32), int(r.shape[0]), "seeds", dev, who)
    _check_async(ctx, torch, dev, who, asynchronous)
    return r, h, sd, rn


def light_rays(scene, rays, hits, params, seeds=None, ctx=None, asynchronous=False, hints=False):
    """rtr_light_rays: the shadow rays the ray-gen shader sends for each hit, as an (N * Q, 8) float32 array of RtrRay (Q =
    light_slots(scene, params)); hit k's rays are rows k * Q ... k * Q + Q, a slot without a ray holds eight zeros.  rays, hits as
    hit_surfaces takes them; seeds: int32 (N,) bases of the sample seeds, default the pixel's (params.width, params.spp).  Device
    tensors in give a device tensor out, numpy in gives numpy out; ctx and asynchronous as in trace_rays.
    hints=True (rtr_light_rays_hinted): returns (rays, leaves) — the same rays and the int32 (N * Q,) start hints of the queued occlusion
    query (trace_occlusion(start_leaves=...)): the hit's leaf where the renderer marks the ray as leaving into its surface, else 0."""
    torch = _torch()
    ctx = ctx or scene.ctx
    dev = torch.device("cuda", ctx.device)
    r, h, sd, as_numpy = _light_inputs(torch, scene, rays, hits, seeds, ctx, "light_rays", asynchronous)
    n, q = int(r.shape[0]), light_slots(scene, params)
    if n * q > 0xffffffff:
        raise ValueError(f"light_rays: {n} hits x {q} slots do not fit 32 bits")
    out = torch.empty((n * q, 8), dtype=torch.float32, device=dev)
    leaves = torch.empty(n * q, dtype=torch.int32, device=dev) if hints else None
    _join_torchs_stream(ctx, torch, dev, asynchronous)
    if hints:
        fn, who = (ctx.lib.rtr_light_rays_hinted_async if asynchronous else ctx.lib.rtr_light_rays_hinted), "rtr_light_rays_hinted"
        extra = (A.VP(leaves.data_ptr()) if n else None,)
    else:
        fn, who, extra = (ctx.lib.rtr_light_rays_async if asynchronous else ctx.lib.rtr_light_rays), "rtr_light_rays", ()
    if n:
        _check(fn(ctx.h, scene.h, A.VP(r.data_ptr()), A.VP(h.data_ptr()), n, C.byref(params), A.VP(sd.data_ptr()) if sd is not None else None,
                  A.VP(out.data_ptr()), *extra), who)
    else:
        _check(fn(ctx.h, scene.h, None, None, 0, C.byref(params), None, None, *extra), who)
    if as_numpy:
        return (out.cpu().numpy(), leaves.cpu().numpy()) if hints else out.cpu().numpy()
    out._keep = (r, h, sd)               # an asynchronous call's inputs stay alive with its result
    return (out, leaves) if hints else out


def shade_hits(scene, rays, hits, params, occluded, seeds=None, ctx=None, asynchronous=False):
    """rtr_shade_hits: one primary sample's contribution for each hit -> RadianceResult.  occluded: the (N * Q,) uint8 answers of
    trace_rays(any_hit=True) for light_rays' rays (or the QueryResult itself), with the same rays, hits, params and seeds."""
    torch = _torch()
    ctx = ctx or scene.ctx
    dev = torch.device("cuda", ctx.device)
    r, h, sd, as_numpy = _light_inputs(torch, scene, rays, hits, seeds, ctx, "shade_hits", asynchronous)
    if isinstance(occluded, QueryResult):
        if occluded.occluded is None:
            raise ValueError("shade_hits: the QueryResult holds no visibility bytes (a closest-hit query)")
        occluded = occluded.occluded
    n, q = int(r.shape[0]), light_slots(scene, params)
    if occluded is None:
        raise ValueError("shade_hits: occluded must be a torch tensor or a numpy array, got NoneType")
    oc = _device_vector(torch, occluded, torch.uint8, (np.uint8,), n * q, "occluded", dev, "shade_hits", as_numpy)
    out = torch.empty((n, 12), dtype=torch.float32, device=dev)
    _join_torchs_stream(ctx, torch, dev, asynchronous)
    fn = ctx.lib.rtr_shade_hits_async if asynchronous else ctx.lib.rtr_shade_hits
    if n:
        _check(fn(ctx.h, scene.h, A.VP(r.data_ptr()), A.VP(h.data_ptr()), n, C.byref(params), A.VP(sd.data_ptr()) if sd is not None else None,
                  A.VP(oc.data_ptr()), A.VP(out.data_ptr())), "rtr_shade_hits")
    else:
        _check(fn(ctx.h, scene.h, None, None, 0, C.byref(params), None, None, None), "rtr_shade_hits")
    res = _radiance_result(out.cpu().numpy() if as_numpy else out, as_numpy, torch)
    res._keep = (r, h, sd, oc)
    return res


def _radiance_result(raw, as_numpy, torch):
    res = RadianceResult()
    words = raw.view(np.int32) if as_numpy else raw.view(torch.int32)
    res.raw = raw
    res.shadowed, res.unshadowed, res.analytic, res.kind = raw[:, 0:3], raw[:, 4:7], raw[:, 8:11], words[:, 3]
    return res


# ---- picked light samples (rtr_light_rays_picked, rtr_shade_hits_picked): P area-light samples per hit instead of all ----------------
def make_pick_params(picks=1, depth=0):
    """rtr_pick_params: picks (P, 1 ... A.PICK_MAX) area-light samples per hit; depth enters their seeds as it enters bounce_rays'"""
    return A.rtr_pick_params(int(picks), int(depth) & 0xffffffff)


def host_pick_slots(seeds, n, params, pick, area_slots):
    """rtr_host_pick_slots: the slots light_rays_picked draws for n hits, on the host -> uint32 (n, P).  seeds: int32 / uint32 (n,) or
    None (then the pixels' of params.width / spp); params: the rtr_light_params (frame, width, spp); area_slots: A = light_slots - 1"""
    lib = A.hip_lib()
    n = int(n)
    sd = None
    if seeds is not None:
        sd = np.ascontiguousarray(seeds)
        if sd.dtype not in (np.int32, np.uint32) or sd.shape != (n,):
            raise ValueError(f"host_pick_slots: seeds must be int32 or uint32 ({n},), got {sd.dtype} {sd.shape}")
    out = np.zeros((n, int(pick.numPicks)), np.uint32)
    _check(lib.rtr_host_pick_slots(sd.ctypes.data_as(A.VP) if sd is not None and n else None, n, int(params.frame), int(params.width), int(params.spp),
                                   C.byref(pick), int(area_slots), out.ctypes.data_as(A.VP) if out.size else None), "rtr_host_pick_slots")
    return out


def _pick_vector(torch, x, dtype, np_dtypes, n, p, name, dev, who, as_numpy):
    """_device_vector for an (n, p) or (n * p,) array of per-pick words, flattened"""
    if x is not None and isinstance(x, (np.ndarray, torch.Tensor)) and tuple(x.shape) == (n, p):
        x = x.reshape(-1)
    return _device_vector(torch, x, dtype, np_dtypes, n * p, name, dev, who, as_numpy)


def light_rays_picked(scene, rays, hits, params, pick, seeds=None, slots=None, ctx=None, asynchronous=False):
    """rtr_light_rays_picked: per hit the shadow rays of pick.numPicks (P) of its area-light slots and of the directional light ->
    (rays, slots): an (N * R, 8) float32 array of RtrRay, R = P + 1, hit k's at rows k * R ... k * R + R — pick p at row k * R + p, the
    directional light last — each the ray light_rays writes for that slot (eight zeros where that is null); and the (N, P) area slots
    used (int32 words on the device, uint32 for numpy; A.PICK_NONE: no slot).  slots: None (drawn by include/rtr_pick.h's rule, what
    host_pick_slots restates) or the caller's (N, P) choice, e.g. stratified or power-proportional.  The other arguments as light_rays."""
    torch = _torch()
    ctx = ctx or scene.ctx
    dev = torch.device("cuda", ctx.device)
    r, h, sd, as_numpy = _light_inputs(torch, scene, rays, hits, seeds, ctx, "light_rays_picked", asynchronous)
    n, p = int(r.shape[0]), int(pick.numPicks)
    sl = _pick_vector(torch, slots, torch.int32, (np.int32, np.uint32), n, p, "slots", dev, "light_rays_picked", as_numpy)
    out = torch.empty((n * (p + 1), 8), dtype=torch.float32, device=dev)
    out_slots = torch.empty((n, p), dtype=torch.int32, device=dev)
    _join_torchs_stream(ctx, torch, dev, asynchronous)
    fn = ctx.lib.rtr_light_rays_picked_async if asynchronous else ctx.lib.rtr_light_rays_picked
    _check(fn(ctx.h, scene.h, _ptr(r, n), _ptr(h, n), n, C.byref(params), C.byref(pick), _ptr(sd, n), _ptr(sl, n), _ptr(out, n), _ptr(out_slots, n)),
           "rtr_light_rays_picked")
    if as_numpy:
        return out.cpu().numpy(), out_slots.cpu().numpy().view(np.uint32)
    out._keep = (r, h, sd, sl)           # an asynchronous call's inputs stay alive with its result
    return out, out_slots


def shade_hits_picked(scene, rays, hits, params, pick, slots, occluded, weights=None, seeds=None, ctx=None, asynchronous=False):
    """rtr_shade_hits_picked: shade_hits' RadianceResult from the picks.  slots: light_rays_picked's (N, P); occluded: the (N * R,) uint8
    answers of trace_rays(any_hit=True) for its rays (or the QueryResult); weights: None — each pick counts (light triangles) / P, which
    makes the picks' sum an unbiased estimate of the light loops' area sum for uniformly drawn slots — or float32 (N, P),
    1 / (P * pdf * shadow_rays) for slots drawn with probability pdf each.  The analytic sum cannot be asked for."""
    torch = _torch()
    ctx = ctx or scene.ctx
    dev = torch.device("cuda", ctx.device)
    r, h, sd, as_numpy = _light_inputs(torch, scene, rays, hits, seeds, ctx, "shade_hits_picked", asynchronous)
    if isinstance(occluded, QueryResult):
        if occluded.occluded is None:
            raise ValueError("shade_hits_picked: the QueryResult holds no visibility bytes (a closest-hit query)")
        occluded = occluded.occluded
    n, p = int(r.shape[0]), int(pick.numPicks)
    if occluded is None or slots is None:
        raise ValueError("shade_hits_picked: slots and occluded must be torch tensors or numpy arrays")
    sl = _pick_vector(torch, slots, torch.int32, (np.int32, np.uint32), n, p, "slots", dev, "shade_hits_picked", as_numpy)
    wt = _pick_vector(torch, weights, torch.float32, (np.float32,), n, p, "weights", dev, "shade_hits_picked", as_numpy)
    oc = _device_vector(torch, occluded, torch.uint8, (np.uint8,), n * (p + 1), "occluded", dev, "shade_hits_picked", as_numpy)
    out = torch.empty((n, 12), dtype=torch.float32, device=dev)
    _join_torchs_stream(ctx, torch, dev, asynchronous)
    fn = ctx.lib.rtr_shade_hits_picked_async if asynchronous else ctx.lib.rtr_shade_hits_picked
    _check(fn(ctx.h, scene.h, _ptr(r, n), _ptr(h, n), n, C.byref(params), C.byref(pick), _ptr(sd, n), _ptr(sl, n), _ptr(wt, n), _ptr(oc, n), _ptr(out, n)),
           "rtr_shade_hits_picked")
    res = _radiance_result(out.cpu().numpy() if as_numpy else out, as_numpy, torch)
    res._keep = (r, h, sd, sl, wt, oc)
    return res


def tonemap_pack(ctx, radiance, asynchronous=False):
    """rtr_tonemap_pack: the tone-mapped BGRA8 pixel (ACES, sRGB; uint32 as Frame.download gives them, here int32 (N,) on the device) of
    each row of radiance, a float32 (N, >= 3) array whose first three columns are used and whose rows may be a view into wider records
    (RadianceResult.shadowed, an HDR image reshaped to (N, 4)).  numpy in gives numpy (uint32) out."""
    torch = _torch()
    dev = torch.device("cuda", ctx.device)
    as_numpy = isinstance(radiance, np.ndarray)
    x = torch.from_numpy(np.ascontiguousarray(radiance, dtype=np.float32)).to(dev) if as_numpy else radiance
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] < 3 or x.device != dev:
        raise ValueError(f"tonemap_pack: radiance must be float32 (N, >= 3) on {dev}")
    n = int(x.shape[0])
    if n and (x.stride(1) != 1 or x.stride(0) < 3):
        raise ValueError("tonemap_pack: the three floats of a row must be adjacent")
    _check_async(ctx, torch, dev, "tonemap_pack", asynchronous)
    out = torch.empty(n, dtype=torch.int32, device=dev)
    _join_torchs_stream(ctx, torch, dev, asynchronous)
    fn = ctx.lib.rtr_tonemap_pack_async if asynchronous else ctx.lib.rtr_tonemap_pack
    if n:
        _check(fn(ctx.h, A.VP(x.data_ptr()), 4 * int(x.stride(0)), n, A.VP(out.data_ptr())), "rtr_tonemap_pack")
    if as_numpy:
        return out.cpu().numpy().view(np.uint32)
    out._keep = x
    return out


def direct_light(scene, rays, hits=None, params=None, seeds=None, ctx=None, max_ray_bytes=256 << 20, occlusion="dense", shadow_cull_mask=None, shadow_ray_flags=0,
                 pick_weights=None, picks=None, pick_depth=0):
    """The composed stage: closest hit (when hits is None) -> light_rays -> trace_rays(any_hit=True) -> shade_hits, in chunks of hits
    so that a chunk's light rays (n * Q * 32 bytes) stay within max_ray_bytes — a 1080p frame at Q = 7 would be 464 MB of rays at once.
    Chunks do not change the result.  occlusion: "dense" (trace_rays, the default), "queued" (trace_occlusion) or "queued_own_leaf"
    (light_rays(hints=True) and trace_occlusion(start_leaves=...): the renderer's own walk, own-leaf rule included): the same bytes.  rays: a float32 (N, 8) device tensor; hits: a QueryResult, (N, 8) int32 records, or None;
    params: make_light_params(...).  shadow_cull_mask: the cull mask of the shadow rays (instances whose mask does not meet it cast no
    shadow), passed to whichever occlusion route is selected; None: the unmasked calls, as before.  shadow_ray_flags: the culling flags
    (A.QUERY_CULL_*, as trace_rays' ray_flags) of the shadow rays, passed to that route likewise; 0: as before.  Returns a RadianceResult
    on the device.
    picks=P: the picked route — light_rays_picked(make_pick_params(P, pick_depth)) -> the same occlusion query -> shade_hits_picked with
    the default weights: P + 1 rays per hit instead of Q, an unbiased estimate of the same shadowed (and unshadowed) sum; the analytic sum
    is refused.  "queued_own_leaf" raises ValueError with picks: the picked rays have no start hints.  None: the full loops, as before.
    pick_weights: with picks, a float32 (N, P) device tensor handed to shade_hits_picked as its weights (mis_pick_weights' for the slots
    this call draws); None: the default weights, as before.  Without picks it raises ValueError."""
    if pick_weights is not None and picks is None:
        raise ValueError("direct_light: pick_weights are the weights of the picked route (picks must be given)")
    shadow_ray_flags = _ray_flags("direct_light", shadow_ray_flags, False)
    if occlusion not in ("dense", "queued", "queued_own_leaf"):
        raise ValueError(f"direct_light: occlusion must be 'dense', 'queued' or 'queued_own_leaf', got {occlusion!r}")
    return _direct_light("direct_light", scene, rays, hits, params, seeds, ctx, max_ray_bytes, occlusion, shadow_cull_mask, shadow_ray_flags, picks, pick_depth,
                         pick_weights=pick_weights)


def _pixel_seeds(torch, params, a, b, device):
    """the seed words px * 733 + py * 1933 of the pixels of hits a ... b - 1 in camera_rays' order (the pixel of hit k is (k // spp) %
    width, (k // spp) // width): what the kernels give a hit without explicit seeds, as int32 (b - a,).  For every frame this project
    allows the sum stays far inside 32 bits, so _wrap32 and the plain conversion to int32 give the same words; the conversion it is,
    one launch where _wrap32 is five: a chunked direct_light builds these for every later chunk, and a frame's time showed the four."""
    k = torch.arange(a, b, device=device, dtype=torch.int64) // int(params.spp)
    return ((k % int(params.width)) * 733 + (k // int(params.width)) * 1933).to(torch.int32)


def _occluded(scene, rays, occlusion, ctx, cull_mask=None, ray_flags=0):
    """the visibility bytes of rays by the occlusion= route: trace_occlusion ("queued"), else the dense any-hit query"""
    if occlusion == "queued":
        return trace_occlusion(scene, rays, ctx=ctx, cull_mask=cull_mask, ray_flags=ray_flags).occluded
    return trace_rays(scene, rays, any_hit=True, ctx=ctx, cull_mask=cull_mask, ray_flags=ray_flags).occluded


def _direct_light(who, scene, rays, hits, params, seeds, ctx, max_ray_bytes, occlusion, shadow_cull_mask, shadow_ray_flags, picks, pick_depth, pick_weights=None,
                  power=False, mis=None, ris=None):
    """the chunked stage of direct_light, direct_light_power and direct_light_ris (who: the one that was called, which has checked
    occlusion and the flags).  A chunk's light rays and its shading come from one of four routes: the full light loops (picks is None;
    "queued_own_leaf" with their start hints), uniform picks (pick_weights: the caller's weights or None), power-proportional picks
    (power; mis: the MIS params of the vertex's bounce or None) or resampled picks (power and ris: the rtr_ris_params, which carry the
    MIS flag themselves).  A later chunk without seeds carries its pixels' own."""
    if params is None:
        raise ValueError(f"{who}: params (make_light_params) are needed")
    torch = _torch()
    ctx = ctx or scene.ctx
    if not isinstance(rays, torch.Tensor):
        raise ValueError(f"{who}: rays must be a device tensor")
    if hits is None:
        hits = trace_rays(scene, rays, ctx=ctx)
    if isinstance(hits, QueryResult):
        hits = hits.hits
    n, pick = int(rays.shape[0]), None
    q = None if power else light_slots(scene, params)      # direct_light asks for Q on its picked route too: the first check of the params
    if picks is not None:
        if occlusion == "queued_own_leaf":
            raise ValueError(f"{who}: occlusion='queued_own_leaf' needs start hints, which the picked rays do not have (picks must be None)")
        pick = make_pick_params(picks, pick_depth)
        q = int(pick.numPicks) + 1
    chunk = max(1, int(max_ray_bytes) // (32 * q))
    out = torch.empty((n, 12), dtype=torch.float32, device=rays.device)
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        sd = seeds[a:b] if seeds is not None else _pixel_seeds(torch, params, a, b, rays.device) if a else None
        r, h = rays[a:b], hits[a:b]
        if pick is None:                 # the full light loops
            if occlusion == "queued_own_leaf":
                lr, leaves = light_rays(scene, r, h, params, seeds=sd, ctx=ctx, hints=True)
                occ = trace_occlusion(scene, lr, ctx=ctx, start_leaves=leaves, cull_mask=shadow_cull_mask, ray_flags=shadow_ray_flags).occluded
            else:
                occ = _occluded(scene, light_rays(scene, r, h, params, seeds=sd, ctx=ctx), occlusion, ctx, shadow_cull_mask, shadow_ray_flags)
            out[a:b] = shade_hits(scene, r, h, params, occ, seeds=sd, ctx=ctx).raw
            continue
        if power:                        # power-proportional picks: the slots and their weights come first
            if ris is not None:          # resampled among candidates of the table: one call gives both, MIS or not
                got = pick_slots_ris(scene, r, h, params, pick, ris, seeds=sd, ctx=ctx)
                sl, w = got.slots, got.weights
            else:
                sl, w = pick_slots_power(scene, b - a, params, pick, seeds=sd, ctx=ctx)
                if mis is not None:
                    w = mis_pick_weights_power(scene, r, h, params, pick, mis, sl, seeds=sd, ctx=ctx)
            lr, sl = light_rays_picked(scene, r, h, params, pick, seeds=sd, slots=sl, ctx=ctx)
        else:                            # uniform picks: light_rays_picked draws the slots
            lr, sl = light_rays_picked(scene, r, h, params, pick, seeds=sd, ctx=ctx)
            w = None if pick_weights is None else pick_weights[a:b]
        occ = _occluded(scene, lr, occlusion, ctx, shadow_cull_mask, shadow_ray_flags)
        out[a:b] = shade_hits_picked(scene, r, h, params, pick, sl, occ, weights=w, seeds=sd, ctx=ctx).raw
    return _radiance_result(out, False, torch)


# ---- continuation rays for ray-query hits (rtr_bounce_rays) and the path they make (path_trace) ------------------------------------
class BounceResult:
    """What bounce_rays and host_bounce_rays give back.  rays: the (N, 8) float32 RtrRay of the continuation (eight zeros: no
    continuation).  raw: the (N, 8) float32 array of RtrBounce records, of which weight (N, 3) and pdf, p_specular (N,) are float32
    views and lobe (A.BOUNCE_*, 0 = dead) an int32 view."""
    rays = raw = weight = pdf = lobe = p_specular = None


def _bounce_result(rays, raw, as_numpy, torch):
    res = BounceResult()
    words = raw.view(np.int32) if as_numpy else raw.view(torch.int32)
    res.rays, res.raw = rays, raw
    res.weight, res.pdf, res.lobe, res.p_specular = raw[:, 0:3], raw[:, 3], words[:, 4], raw[:, 5]
    return res


def make_bounce_params(frame=0, depth=0, width=0, spp=1, lobes=A.BOUNCE_DIFFUSE | A.BOUNCE_SPECULAR, normal_offset=0.01, tmin=0.001, tmax=10000.0):
    """rtr_bounce_params.  frame and depth enter every seed; width / spp say which pixel a hit belongs to (camera_rays' order) and matter
    only without explicit seeds; normal_offset, tmin, tmax: the continuation ray (the defaults are the shader's shadow-ray numbers)"""
    return A.rtr_bounce_params(int(frame) & 0xffffffff, int(depth) & 0xffffffff, int(width), int(spp), int(lobes), float(normal_offset), float(tmin), float(tmax))


def bounce_rays(ctx, rays, surfaces, params, seeds=None, asynchronous=False):
    """rtr_bounce_rays: one BRDF-sampled continuation ray per hit and its throughput weight -> BounceResult.  rays: the float32 (N, 8)
    rays that found the hits; surfaces: hit_surfaces' SurfaceResult or its (N, 20) float32 raw records (edited or not: no scene is read);
    seeds: int32 (N,) seed bases, default the pixel's (params.width, params.spp).  Device tensors in give device tensors out, numpy in
    gives numpy out; asynchronous as in trace_rays: the context must then be on torch's current stream."""
    torch = _torch()
    dev = torch.device("cuda", ctx.device)
    if isinstance(surfaces, SurfaceResult):
        surfaces = surfaces.raw
    r, rn = _device_array(torch, rays, torch.float32, np.float32, "rays", dev, "bounce_rays")
    sn = isinstance(surfaces, np.ndarray)
    if sn != rn:
        raise ValueError("bounce_rays: rays and surfaces must both be numpy arrays or both be tensors")
    if sn:
        if surfaces.dtype != np.float32 or surfaces.ndim != 2 or surfaces.shape[1] != 20:
            raise ValueError(f"bounce_rays: surfaces must be float32 (N, 20), got {surfaces.dtype} {surfaces.shape}")
        s = torch.from_numpy(np.ascontiguousarray(surfaces)).to(dev)
    else:
        s = surfaces
        if not isinstance(s, torch.Tensor) or s.dtype != torch.float32 or s.dim() != 2 or s.shape[1] != 20 or s.device != dev or not s.is_contiguous():
            raise ValueError(f"bounce_rays: surfaces must be a contiguous float32 (N, 20) tensor on {dev}")
    if r.shape[0] != s.shape[0]:
        raise ValueError(f"bounce_rays: {r.shape[0]} rays but {s.shape[0]} surfaces")
    n = int(r.shape[0])
    sd = _device_vector(torch, seeds, torch.int32, (np.int32, np.uint32), n, "seeds", dev, "bounce_rays")
    _check_async(ctx, torch, dev, "bounce_rays", asynchronous)
    out_rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
    out_b = torch.empty((n, 8), dtype=torch.float32, device=dev)
    _join_torchs_stream(ctx, torch, dev, asynchronous)
    fn, who = (ctx.lib.rtr_bounce_rays_async, "rtr_bounce_rays_async") if asynchronous else (ctx.lib.rtr_bounce_rays, "rtr_bounce_rays")
    if n:
        _check(fn(ctx.h, A.VP(r.data_ptr()), A.VP(s.data_ptr()), n, C.byref(params), A.VP(sd.data_ptr()) if sd is not None else None,
                  A.VP(out_rays.data_ptr()), A.VP(out_b.data_ptr())), who)
    else:
        _check(fn(ctx.h, None, None, 0, C.byref(params), None, None, None), who)
    res = _bounce_result(out_rays.cpu().numpy(), out_b.cpu().numpy(), True, torch) if rn else _bounce_result(out_rays, out_b, False, torch)
    res._keep = (r, s, sd)               # an asynchronous call's inputs stay alive with its result
    return res


def host_bounce_rays(rays, surfaces, params, seeds=None):
    """rtr_host_bounce_rays: the host restatement of bounce_rays on numpy arrays, no device -> BounceResult of numpy arrays.  rays float32
    (N, 8), surfaces float32 (N, 20) (or 32-bit words of that shape), seeds int32 / uint32 (N,) or None."""
    lib = A.hip_lib()
    r = np.ascontiguousarray(rays)
    s = np.ascontiguousarray(surfaces)
    if r.dtype != np.float32 or r.ndim != 2 or r.shape[1] != 8:
        raise ValueError(f"host_bounce_rays: rays must be float32 (N, 8), got {r.dtype} {r.shape}")
    if s.dtype.itemsize != 4 or s.ndim != 2 or s.shape[1] != 20 or s.shape[0] != r.shape[0]:
        raise ValueError(f"host_bounce_rays: surfaces must be 32-bit words ({r.shape[0]}, 20), got {s.dtype} {s.shape}")
    n = int(r.shape[0])
    sd = None
    if seeds is not None:
        sd = np.ascontiguousarray(seeds)
        if sd.dtype not in (np.int32, np.uint32) or sd.shape != (n,):
            raise ValueError(f"host_bounce_rays: seeds must be int32 or uint32 ({n},), got {sd.dtype} {sd.shape}")
    out_rays = np.zeros((n, 8), np.float32)
    out_b = np.zeros((n, 8), np.float32)
    if n:
        _check(lib.rtr_host_bounce_rays(r.ctypes.data_as(A.VP), s.ctypes.data_as(A.VP), n, C.byref(params), sd.ctypes.data_as(A.VP) if sd is not None else None,
                                        out_rays.ctypes.data_as(A.VP), out_b.ctypes.data_as(A.VP)), "rtr_host_bounce_rays")
    return _bounce_result(out_rays, out_b, True, None)


# ---- compaction of live paths, with Russian roulette (rtr_compact_paths) -------------------------------------------------------------
class CompactResult:
    """What compact_paths and host_compact_paths give back, every array N long: rays (N, 8) float32, throughput (N, 3) float32, seeds
    (N,) int32 or None (no seeds went in), path_ids (N,) int32 (-1 = A.PATH_NONE behind the survivors).  The first count rows are the
    survivors in input order; the rest are the null ray, zero throughput, seed 0.  count_tensor: the 1-element int32 device tensor the
    count was written to; count: that number as an int, read on first use — the only join (numpy results carry it already)."""
    rays = throughput = seeds = path_ids = count_tensor = None
    _count = None

    @property
    def count(self):
        if self._count is None:
            self._count = int(self.count_tensor.item()) & 0xffffffff
        return self._count


def make_compact_params(frame=0, depth=0, roulette=False, survival_floor=0.05, throughput_stride=12):
    """rtr_compact_params.  frame and depth enter the roulette's seed and are those of the bounce before (make_bounce_params); roulette:
    RTR_COMPACT_ROULETTE; survival_floor: the least survival probability, in (0, 1]; throughput_stride: bytes between two paths'
    throughputs in the input (compact_paths sets it from the array it is given)"""
    return A.rtr_compact_params(int(frame) & 0xffffffff, int(depth) & 0xffffffff, A.COMPACT_ROULETTE if roulette else 0, float(survival_floor),
                                int(throughput_stride), (A.u32 * 3)(0, 0, 0))


def _with_stride(params, stride):
    return A.rtr_compact_params(params.frame, params.depth, params.flags, params.survivalFloor, int(stride), params._reserved)


def compact_scratch_bytes(lib, n):
    """rtr_compact_scratch_bytes(n)"""
    b = C.c_size_t(0)
    _check(lib.rtr_compact_scratch_bytes(int(n), C.byref(b)), "rtr_compact_scratch_bytes")
    return int(b.value)


def compact_paths(ctx, rays, throughput, seeds=None, path_ids=None, params=None, asynchronous=False):
    """rtr_compact_paths: the live paths gathered to the front in their order, the rest cleared -> CompactResult (the rule: include/rtr.h,
    include/rtr_paths.h).  rays: float32 (N, 8); throughput: float32 (N, 3) — contiguous, or a view of the first three columns of wider
    rows, as BounceResult.weight is — or the (N, 8) raw RtrBounce records themselves (stride 32 either way); seeds, path_ids: int32 (N,)
    or None (no roulette without seeds; None ids: path k is k); params: make_compact_params(...), default no roulette — its
    throughput_stride is replaced by the array's.  Device tensors in give device tensors out and NO join: the count stays on the device
    until CompactResult.count is read; numpy in gives numpy out.  The scratch is a tensor of this call's own, kept alive with the
    result.  asynchronous as in trace_rays: the context must then be on torch's current stream."""
    torch = _torch()
    dev = torch.device("cuda", ctx.device)
    who = "compact_paths"
    params = params if params is not None else make_compact_params()
    r, rn = _device_array(torch, rays, torch.float32, np.float32, "rays", dev, who)
    n = int(r.shape[0])
    t = throughput
    if isinstance(t, np.ndarray) != rn:
        raise ValueError(f"{who}: rays and throughput must both be numpy arrays or both be tensors")
    if rn:
        if t.dtype != np.float32 or t.ndim != 2 or t.shape[0] != n or t.shape[1] not in (3, 8):
            raise ValueError(f"{who}: throughput must be float32 ({n}, 3) or ({n}, 8), got {t.dtype} {t.shape}")
        t = torch.from_numpy(np.ascontiguousarray(t)).to(dev)
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != n or t.shape[1] not in (3, 8) or t.device != dev:
        raise ValueError(f"{who}: throughput must be a float32 ({n}, 3) or ({n}, 8) tensor on {dev}")
    if n and (t.stride(1) != 1 or (n > 1 and t.stride(0) < 3)):
        raise ValueError(f"{who}: the three floats of a throughput row must be adjacent and the rows apart")
    stride = 4 * int(t.stride(0)) if n > 1 else 4 * int(t.shape[1])
    sd = _device_vector(torch, seeds, torch.int32, (np.int32, np.uint32), n, "seeds", dev, who, as_numpy=rn)
    ids = _device_vector(torch, path_ids, torch.int32, (np.int32, np.uint32), n, "path_ids", dev, who, as_numpy=rn)
    _check_async(ctx, torch, dev, who, asynchronous)
    out_rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
    out_t = torch.empty((n, 3), dtype=torch.float32, device=dev)
    out_seeds = torch.empty(n, dtype=torch.int32, device=dev) if sd is not None else None
    out_ids = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    nbytes = compact_scratch_bytes(ctx.lib, n)
    scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    _join_torchs_stream(ctx, torch, dev, asynchronous)
    p = _with_stride(params, stride)
    args = (ctx.h, _ptr(r, n), _ptr(t, n), _ptr(sd, n), _ptr(ids, n), n, C.byref(p), A.VP(scratch.data_ptr()), nbytes,
            _ptr(out_rays, n), _ptr(out_t, n), _ptr(out_seeds, n), _ptr(out_ids, n), A.VP(count.data_ptr()))
    if asynchronous:
        _check(ctx.lib.rtr_compact_paths_async(*args), "rtr_compact_paths_async")
    else:
        _check(ctx.lib.rtr_compact_paths(*args, None), "rtr_compact_paths")
    res = CompactResult()
    if rn:
        res.rays, res.throughput, res.path_ids = out_rays.cpu().numpy(), out_t.cpu().numpy(), out_ids.cpu().numpy()
        res.seeds = out_seeds.cpu().numpy() if out_seeds is not None else None
        res.count_tensor = count
        res._count = int(count.item()) & 0xffffffff
    else:
        res.rays, res.throughput, res.seeds, res.path_ids, res.count_tensor = out_rays, out_t, out_seeds, out_ids, count
    res._keep = (r, t, sd, ids, scratch)      # an asynchronous call's inputs and its scratch stay alive with its result
    return res


def host_compact_paths(rays, throughput, seeds=None, path_ids=None, params=None):
    """rtr_host_compact_paths: the host restatement of compact_paths on numpy arrays, no device -> CompactResult of numpy arrays (count
    is set; count_tensor is None).  rays float32 (N, 8) (or 32-bit words of that shape); throughput float32 (N, 3), or (N, 8) RtrBounce
    records (stride 32); seeds, path_ids int32 / uint32 (N,) or None."""
    lib = A.hip_lib()
    params = params if params is not None else make_compact_params()
    r = np.ascontiguousarray(rays)
    if r.dtype.itemsize != 4 or r.ndim != 2 or r.shape[1] != 8:
        raise ValueError(f"host_compact_paths: rays must be 32-bit words (N, 8), got {r.dtype} {r.shape}")
    n = int(r.shape[0])
    t = np.ascontiguousarray(throughput)
    if t.dtype.itemsize != 4 or t.ndim != 2 or t.shape[0] != n or t.shape[1] not in (3, 8):
        raise ValueError(f"host_compact_paths: throughput must be 32-bit words ({n}, 3) or ({n}, 8), got {t.dtype} {t.shape}")
    vec = []
    for name, x in (("seeds", seeds), ("path_ids", path_ids)):
        if x is not None:
            x = np.ascontiguousarray(x)
            if x.dtype not in (np.int32, np.uint32) or x.shape != (n,):
                raise ValueError(f"host_compact_paths: {name} must be int32 or uint32 ({n},), got {x.dtype} {x.shape}")
        vec.append(x)
    sd, ids = vec
    out_rays = np.zeros((n, 8), np.float32)
    out_t = np.zeros((n, 3), np.float32)
    out_seeds = np.zeros(n, np.int32) if sd is not None else None
    out_ids = np.zeros(n, np.int32)
    count = A.u32(0)
    p = _with_stride(params, 4 * t.shape[1])

    def ptr(x):
        return x.ctypes.data_as(A.VP) if x is not None and n else None
    _check(lib.rtr_host_compact_paths(ptr(r), ptr(t), ptr(sd), ptr(ids), n, C.byref(p), ptr(out_rays), ptr(out_t), ptr(out_seeds), ptr(out_ids),
                                      C.byref(count)), "rtr_host_compact_paths")
    res = CompactResult()
    res.rays, res.throughput, res.seeds, res.path_ids, res._count = out_rays, out_t, out_seeds, out_ids, int(count.value)
    return res


# ---- accumulation of a vertex and the record gather (rtr_accumulate_paths, rtr_gather_records; include/rtr_accum.h) -------------------
def make_accum_params(num_slots, lights_from_emitters=False, misses_from_escapes=False, throughput_stride=12, image_stride=12):
    """rtr_accum_params.  num_slots: the rows of the image (a path whose id is not below it touches nothing); lights_from_emitters,
    misses_from_escapes: RTR_ACCUM_LIGHTS_FROM_EMITTERS, RTR_ACCUM_MISSES_FROM_ESCAPES; throughput_stride, image_stride: bytes between
    two rows of the input throughput and of the images (accumulate_paths sets both from the arrays it is given)"""
    flags = (A.ACCUM_LIGHTS_FROM_EMITTERS if lights_from_emitters else 0) | (A.ACCUM_MISSES_FROM_ESCAPES if misses_from_escapes else 0)
    return A.rtr_accum_params(flags, int(num_slots), int(throughput_stride), int(image_stride), (A.u32 * 4)(0, 0, 0, 0))


def _accum_with_strides(params, throughput_stride, image_stride):
    return A.rtr_accum_params(params.flags, params.numSlots, int(throughput_stride), int(image_stride), params._reserved)


def _row_stride_bytes(x):
    """bytes between two rows of a 2-D tensor or numpy array whose rows hold adjacent floats"""
    if isinstance(x, np.ndarray):
        return int(x.strides[0]) if x.shape[0] > 1 else 4 * int(x.shape[1])
    return 4 * int(x.stride(0)) if x.shape[0] > 1 else 4 * int(x.shape[1])


def _accum_rows(torch, x, widths, n, name, dev, who):
    """a float32 tensor on dev of n rows (None: any number) whose leading three floats are adjacent: contiguous (rows, w) for a w of
    widths, or a view of the first three columns of such rows"""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2 or x.device != dev or (n is not None and int(x.shape[0]) != n):
        raise ValueError(f"{who}: {name} must be a float32 ({'rows' if n is None else n}, 3) tensor on {dev}")
    rows, w = int(x.shape[0]), int(x.shape[1])
    view_of_wider = w == 3 and (rows < 2 or int(x.stride(0)) in widths)
    if rows and ((w not in widths and not view_of_wider) or x.stride(1) != 1 or (rows > 1 and x.stride(0) < 3)):
        raise ValueError(f"{who}: {name} must have {' or '.join(map(str, widths))} columns (or be the first three of such rows), the floats of a row adjacent")
    return x


def accumulate_paths(ctx, radiance, throughput, accum, params, path_ids=None, emitters=None, escapes=None, sky_sums=None, bounces=None, out_term=None,
                     asynchronous=False):
    """rtr_accumulate_paths: one vertex of the paths added to the image, accum[id] += T * rad (+ T * sky_sums), in place, and the
    throughput after the vertex's bounce -> the new float32 (N, 3) throughput tensor, or None without bounces (the rule: include/rtr.h,
    include/rtr_accum.h).  radiance: a RadianceResult or its raw (N, 12) tensor; throughput: float32 (N, 3), contiguous or a view of the
    first three columns of wider rows, or (N, 8) RtrBounce records; accum: float32 (S, 3) or (S, 4), S >= params.numSlots; params:
    make_accum_params(...) — its two strides are replaced by the arrays'; path_ids: int32 (N,) or None (path k is k); emitters, escapes:
    an EmitterResult / SkyEscapeResult or their raw (N, 8) tensors; sky_sums: what shade_sky gave, (N, 3) over 16-B rows, or (N, 4);
    bounces: a BounceResult or its raw (N, 8) tensor; out_term: None, or a tensor laid out as accum that takes the terms at their ids
    (the caller clears it).  Device tensors only.  asynchronous as in trace_rays: the context must then be on torch's current stream."""
    torch = _torch()
    dev = torch.device("cuda", ctx.device)
    who = "accumulate_paths"
    unwrap = ((RadianceResult, radiance), (EmitterResult, emitters), (SkyEscapeResult, escapes), (BounceResult, bounces))
    radiance, emitters, escapes, bounces = (x.raw if isinstance(x, cls) else x for cls, x in unwrap)
    rad = _records(torch, radiance, 12, "radiance", dev, who, False)
    n = int(rad.shape[0])
    t = _accum_rows(torch, throughput, (3, 8), n, "throughput", dev, who)
    acc = _accum_rows(torch, accum, (3, 4), None, "accum", dev, who)
    if int(acc.shape[0]) < int(params.numSlots):
        raise ValueError(f"{who}: accum has {acc.shape[0]} rows, params.numSlots is {params.numSlots}")
    term = out_term
    if term is not None:
        _accum_rows(torch, term, (3, 4), int(acc.shape[0]), "out_term", dev, who)
        if _row_stride_bytes(term) != _row_stride_bytes(acc):
            raise ValueError(f"{who}: out_term must be laid out as accum")
    ids = _device_vector(torch, path_ids, torch.int32, (np.int32, np.uint32), n, "path_ids", dev, who, as_numpy=False)
    em = _records(torch, emitters, 8, "emitters", dev, who, False) if emitters is not None else None
    es = _records(torch, escapes, 8, "escapes", dev, who, False) if escapes is not None else None
    bo = _records(torch, bounces, 8, "bounces", dev, who, False) if bounces is not None else None
    sk = _accum_rows(torch, sky_sums, (4,), n, "sky_sums", dev, who) if sky_sums is not None else None
    if sk is not None and n > 1 and int(sk.stride(0)) != 4:
        raise ValueError(f"{who}: sky_sums must lie in 16-B rows, as shade_sky gives them")
    for name, x in (("emitters", em), ("escapes", es), ("bounces", bo)):
        if x is not None and int(x.shape[0]) != n:
            raise ValueError(f"{who}: {n} paths but {x.shape[0]} {name}")
    _check_async(ctx, torch, dev, who, asynchronous)
    out_t = torch.empty((n, 3), dtype=torch.float32, device=dev) if bo is not None else None
    _join_torchs_stream(ctx, torch, dev, asynchronous)
    p = _accum_with_strides(params, _row_stride_bytes(t) if n else 12, _row_stride_bytes(acc) if acc.shape[0] else 12)
    fn = ctx.lib.rtr_accumulate_paths_async if asynchronous else ctx.lib.rtr_accumulate_paths
    _check(fn(ctx.h, _ptr(rad, n), _ptr(t, n), _ptr(ids, n), _ptr(em, n), _ptr(es, n), _ptr(sk, n), _ptr(bo, n), n, C.byref(p), _ptr(acc, n), _ptr(term, n),
              _ptr(out_t, n)), "rtr_accumulate_paths")
    if out_t is not None:
        out_t._keep = (rad, t, ids, em, es, sk, bo, acc, term)      # an asynchronous call's arrays stay alive with its result
    return out_t


def gather_records(ctx, src, rows, asynchronous=False):
    """rtr_gather_records: out[j] = src[rows[j]], a zero record where rows[j] is not a row of src (A.PATH_NONE) -> a tensor of
    src's dtype, (len(rows),) + src.shape[1:].  src: a contiguous device tensor of 32-bit elements whose rows are at most 256 B;
    rows: int32 (M,) on the device (the words are read as unsigned)."""
    torch = _torch()
    dev = torch.device("cuda", ctx.device)
    who = "gather_records"
    if not isinstance(src, torch.Tensor) or src.device != dev or not src.is_contiguous() or src.element_size() != 4 or src.dim() < 1:
        raise ValueError(f"{who}: src must be a contiguous tensor of 32-bit elements on {dev}")
    num_src = int(src.shape[0])
    record = 4 * int(np.prod(src.shape[1:], dtype=np.int64))
    if not 4 <= record <= 256:
        raise ValueError(f"{who}: a row of src is {record} B (4 ... 256)")
    if not isinstance(rows, torch.Tensor) or rows.dim() != 1:
        raise ValueError(f"{who}: rows must be an int32 (M,) tensor on {dev}")
    m = int(rows.shape[0])
    rw = _device_vector(torch, rows, torch.int32, (np.int32, np.uint32), m, "rows", dev, who, as_numpy=False)
    _check_async(ctx, torch, dev, who, asynchronous)
    out = torch.empty((m,) + tuple(src.shape[1:]), dtype=src.dtype, device=dev)
    _join_torchs_stream(ctx, torch, dev, asynchronous)
    fn = ctx.lib.rtr_gather_records_async if asynchronous else ctx.lib.rtr_gather_records
    _check(fn(ctx.h, _ptr(src, num_src), record, num_src, _ptr(rw, m), m, _ptr(out, m)), "rtr_gather_records")
    out._keep = (src, rw)
    return out


def host_accumulate_paths(radiance, throughput, accum, params, path_ids=None, emitters=None, escapes=None, sky_sums=None, bounces=None, out_term=None):
    """rtr_host_accumulate_paths: the host restatement of accumulate_paths on numpy arrays, no device -> the new float32 (N, 3)
    throughput, or None without bounces.  radiance: 32-bit words (N, 12); throughput: float32 (N, 3) or (N, 8); accum and out_term:
    C-contiguous float32 (S, 3) or (S, 4), updated in place; path_ids: int32 / uint32 (N,); emitters, escapes, bounces: 32-bit words
    (N, 8); sky_sums: float32 (N, 4).  params' strides are replaced by the arrays'."""
    lib = A.hip_lib()
    who = "host_accumulate_paths"
    rad = _aligned_copy(_host_words(radiance, (12,), "radiance", who))
    n = int(rad.shape[0])
    t = np.ascontiguousarray(throughput)
    if t.dtype != np.float32 or t.ndim != 2 or t.shape[0] != n or t.shape[1] not in (3, 8):
        raise ValueError(f"{who}: throughput must be float32 ({n}, 3) or ({n}, 8), got {t.dtype} {t.shape}")
    for name, x in (("accum", accum), ("out_term", out_term)):
        if x is not None and (not isinstance(x, np.ndarray) or x.dtype != np.float32 or x.ndim != 2 or x.shape[1] not in (3, 4) or not x.flags.c_contiguous
                              or not x.flags.writeable or x.shape != accum.shape or x.shape[0] < int(params.numSlots)):
            raise ValueError(f"{who}: {name} must be a writable C-contiguous float32 (S, 3) or (S, 4) array, S >= numSlots")
    ids = None
    if path_ids is not None:
        ids = np.ascontiguousarray(path_ids)
        if ids.dtype not in (np.int32, np.uint32) or ids.shape != (n,):
            raise ValueError(f"{who}: path_ids must be int32 or uint32 ({n},), got {ids.dtype} {ids.shape}")
    rec = []
    for name, x, w in (("emitters", emitters, 8), ("escapes", escapes, 8), ("sky_sums", sky_sums, 4), ("bounces", bounces, 8)):
        if x is not None:
            x = _aligned_copy(_host_words(x, (w,), name, who))
            if x.shape[0] != n:
                raise ValueError(f"{who}: {n} paths but {x.shape[0]} {name}")
        rec.append(x)
    em, es, sk, bo = rec
    out_t = np.zeros((n, 3), np.float32) if bo is not None else None
    p = _accum_with_strides(params, 4 * t.shape[1], 4 * accum.shape[1])

    def ptr(x):
        return x.ctypes.data_as(A.VP) if x is not None and n else None
    _check(lib.rtr_host_accumulate_paths(ptr(rad), ptr(t), ptr(ids), ptr(em), ptr(es), ptr(sk), ptr(bo), n, C.byref(p), ptr(accum), ptr(out_term), ptr(out_t)),
           "rtr_host_accumulate_paths")
    return out_t


def host_gather_records(src, rows):
    """rtr_host_gather_records on numpy arrays -> out[j] = src[rows[j]], zeros where rows[j] is not a row of src.  src: 32-bit elements,
    rows of at most 256 B; rows: int32 / uint32 (M,)."""
    lib = A.hip_lib()
    s = np.ascontiguousarray(src)
    if s.dtype.itemsize != 4 or s.ndim < 1:
        raise ValueError(f"host_gather_records: src must hold 32-bit elements, got {s.dtype} {s.shape}")
    record = 4 * int(np.prod(s.shape[1:], dtype=np.int64))
    if not 4 <= record <= 256:
        raise ValueError(f"host_gather_records: a row of src is {record} B (4 ... 256)")
    rw = np.ascontiguousarray(rows)
    if rw.dtype not in (np.int32, np.uint32) or rw.ndim != 1:
        raise ValueError(f"host_gather_records: rows must be int32 or uint32 (M,), got {rw.dtype} {rw.shape}")
    out = np.zeros((rw.shape[0],) + s.shape[1:], s.dtype)
    _check(lib.rtr_host_gather_records(s.ctypes.data_as(A.VP) if s.shape[0] else None, record, int(s.shape[0]), rw.ctypes.data_as(A.VP) if rw.shape[0] else None,
                                       int(rw.shape[0]), out.ctypes.data_as(A.VP) if rw.shape[0] else None), "rtr_host_gather_records")
    return out


# ---- MIS at a path vertex (rtr_mis_pick_weights, rtr_emitter_hits; include/rtr_mis.h) -------------------------------------------------
class EmitterResult:
    """What emitter_hits and host_emitter_hits give back.  raw: the (N, 8) float32 array of RtrEmitter records, of which radiance (N, 3)
    (to be multiplied by the throughput after the bounce), w_bounce, light_pdf and dist (N,) are float32 views and light_tri, kind
    (A.SURFACE_LIGHT where the record counts, 0 beside 32 zero bytes) int32 views."""
    raw = radiance = w_bounce = light_pdf = dist = light_tri = kind = None


def _emitter_result(raw, as_numpy, torch):
    res = EmitterResult()
    words = raw.view(np.int32) if as_numpy else raw.view(torch.int32)
    res.raw = raw
    res.radiance, res.w_bounce, res.light_pdf, res.dist, res.light_tri, res.kind = raw[:, 0:3], raw[:, 3], raw[:, 4], raw[:, 5], words[:, 6], words[:, 7]
    return res


def make_mis_params(picks, num_area_lights, shadow_rays, lobes=A.BOUNCE_DIFFUSE | A.BOUNCE_SPECULAR):
    """rtr_mis_params: the picks per vertex (P), the light params' numAreaLights and numShadowRays, and the lobes the vertex's bounce samples"""
    return A.rtr_mis_params(int(picks), int(num_area_lights), int(shadow_rays), int(lobes))


def mis_pick_weights(scene, rays, hits, params, pick, mis, slots, seeds=None, samples=False, ctx=None, asynchronous=False):
    """rtr_mis_pick_weights: the weights shade_hits_picked (weights=) is to give the picks of each hit when the vertex's bounce ray counts
    the lights it meets (emitter_hits) -> float32 (N, P): (light triangles / P) * wPick of the balance heuristic, 0 for a pick without a
    ray.  slots: light_rays_picked's (N, P), or None — the slots it draws by itself for the same params, pick and seeds.  samples=True:
    -> (weights, samples), samples the float32 (N, P, 8) RtrMisSample records (lightPdf, bouncePdf, wPick, cosLight, dist, area and the
    words lightTri, 0).  The other arguments as shade_hits_picked; numpy in gives numpy out."""
    return _mis_pick_weights("mis_pick_weights", scene, rays, hits, params, pick, mis, slots, seeds, samples, ctx, asynchronous, need_slots=False)


def _mis_pick_weights(name, scene, rays, hits, params, pick, mis, slots, seeds, samples, ctx, asynchronous, need_slots):
    """mis_pick_weights and mis_pick_weights_power: the same arrays; name: the entry point without its rtr_; need_slots: None is refused"""
    torch = _torch()
    ctx = ctx or scene.ctx
    dev = torch.device("cuda", ctx.device)
    r, h, sd, as_numpy = _light_inputs(torch, scene, rays, hits, seeds, ctx, name, asynchronous)
    n, p = int(r.shape[0]), int(pick.numPicks)
    if need_slots and slots is None:
        raise ValueError(f"{name}: slots must be given (pick_slots_power's, or the caller's)")
    sl = _pick_vector(torch, slots, torch.int32, (np.int32, np.uint32), n, p, "slots", dev, name, as_numpy)
    out = torch.empty((n, p), dtype=torch.float32, device=dev)
    rec = torch.empty((n, p, 8), dtype=torch.float32, device=dev) if samples else None
    _join_torchs_stream(ctx, torch, dev, asynchronous)
    fn = getattr(ctx.lib, f"rtr_{name}_async" if asynchronous else f"rtr_{name}")
    _check(fn(ctx.h, scene.h, _ptr(r, n), _ptr(h, n), n, C.byref(params), C.byref(pick), C.byref(mis), _ptr(sd, n), _ptr(sl, n), _ptr(out, n),
              _ptr(rec, n) if samples else None), f"rtr_{name}")
    if as_numpy:
        return (out.cpu().numpy(), rec.cpu().numpy()) if samples else out.cpu().numpy()
    out._keep = (r, h, sd, sl)           # an asynchronous call's inputs stay alive with its result
    return (out, rec) if samples else out


def _records(torch, x, width, name, dev, who, as_numpy):
    """a float32 (N, width) record array on the device: a tensor as it is, numpy uploaded"""
    if as_numpy:
        x = np.ascontiguousarray(x)
        if x.dtype.itemsize != 4 or x.ndim != 2 or x.shape[1] != width:
            raise ValueError(f"{who}: {name} must be 32-bit words (N, {width}), got {x.dtype} {x.shape}")
        return torch.from_numpy(x.view(np.float32)).to(dev)
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != width or x.device != dev or not x.is_contiguous():
        raise ValueError(f"{who}: {name} must be a contiguous float32 (N, {width}) tensor on {dev}")
    return x


def emitter_hits(scene, rays, hits, prev_surfaces, bounces, mis, ctx=None, asynchronous=False):
    """rtr_emitter_hits: what each bounce ray adds where its closest hit is a light -> EmitterResult.  rays: the bounce rays (N, 8);
    hits: their closest hits (a QueryResult or (N, 8) int32 records); prev_surfaces: the SurfaceResult (or (N, 20) float32 records) of the
    vertices the rays left; bounces: bounce_rays' BounceResult (or its (N, 8) raw records) at those vertices; mis: make_mis_params(...).
    Device tensors in give device tensors out, numpy in gives numpy out."""
    return _emitter_hits("rtr_emitter_hits", scene, rays, hits, prev_surfaces, bounces, mis, ctx, asynchronous)


def _emitter_hits(name, scene, rays, hits, prev_surfaces, bounces, mis, ctx, asynchronous):
    """emitter_hits and emitter_hits_power: the same arrays; name: the entry point"""
    torch = _torch()
    ctx = ctx or scene.ctx
    dev = torch.device("cuda", ctx.device)
    if isinstance(prev_surfaces, SurfaceResult):
        prev_surfaces = prev_surfaces.raw
    if isinstance(bounces, BounceResult):
        bounces = bounces.raw
    r, h, _, as_numpy = _light_inputs(torch, scene, rays, hits, None, ctx, "emitter_hits", asynchronous)
    n = int(r.shape[0])
    if isinstance(prev_surfaces, np.ndarray) != as_numpy or isinstance(bounces, np.ndarray) != as_numpy:
        raise ValueError("emitter_hits: rays, hits, prev_surfaces and bounces must all be numpy arrays or all be tensors")
    s = _records(torch, prev_surfaces, 20, "prev_surfaces", dev, "emitter_hits", as_numpy)
    b = _records(torch, bounces, 8, "bounces", dev, "emitter_hits", as_numpy)
    if int(s.shape[0]) != n or int(b.shape[0]) != n:
        raise ValueError(f"emitter_hits: {n} rays but {s.shape[0]} surfaces and {b.shape[0]} bounce records")
    out = torch.empty((n, 8), dtype=torch.float32, device=dev)
    _join_torchs_stream(ctx, torch, dev, asynchronous)
    fn = getattr(ctx.lib, name + "_async" if asynchronous else name)
    _check(fn(ctx.h, scene.h, _ptr(r, n), _ptr(h, n), _ptr(s, n), _ptr(b, n), n, C.byref(mis), _ptr(out, n)), name)
    res = _emitter_result(out.cpu().numpy() if as_numpy else out, as_numpy, torch)
    res._keep = (r, h, s, b)
    return res


def _host_words(x, shape_tail, name, who):
    x = np.ascontiguousarray(x)
    if x.dtype.itemsize != 4 or x.ndim != 1 + len(shape_tail) or tuple(x.shape[1:]) != tuple(shape_tail):
        raise ValueError(f"{who}: {name} must be 32-bit words (N, {', '.join(map(str, shape_tail))}), got {x.dtype} {x.shape}")
    return x


def host_bounce_pdf(rays, surfaces, dirs, lobes=A.BOUNCE_DIFFUSE | A.BOUNCE_SPECULAR):
    """rtr_host_bounce_pdf: the density bounce_rays divides by, for the unit directions dirs (N, 3) at surfaces (N, 20) found by rays
    (N, 8) -> float32 (N,).  For the direction host_bounce_rays drew it is BounceResult.pdf bit for bit; 0 below the horizon, for a
    surface that is not an object and for input that is not finite."""
    lib = A.hip_lib()
    r, s, d = _host_words(rays, (8,), "rays", "host_bounce_pdf"), _host_words(surfaces, (20,), "surfaces", "host_bounce_pdf"), _host_words(dirs, (3,), "dirs", "host_bounce_pdf")
    n = int(r.shape[0])
    if s.shape[0] != n or d.shape[0] != n:
        raise ValueError(f"host_bounce_pdf: {n} rays but {s.shape[0]} surfaces and {d.shape[0]} directions")
    out = np.zeros(n, np.float32)
    _check(lib.rtr_host_bounce_pdf(r.ctypes.data_as(A.VP) if n else None, s.ctypes.data_as(A.VP) if n else None, d.ctypes.data_as(A.VP) if n else None, n,
                                   int(lobes), out.ctypes.data_as(A.VP) if n else None), "rtr_host_bounce_pdf")
    return out


def host_mis_weights(pb, dist, cos_light, area, tris, picks):
    """rtr_host_mis_weights: the balance heuristic of include/rtr_mis.h for N directions -> (samples, w_bounce): the float32 (N, 8)
    RtrMisSample records (lightPdf, pb, wPick, cosLight, dist, area, 0, 0) and wBounce (N,).  tris: Ttot; picks: P (0: nobody picks)."""
    lib = A.hip_lib()
    arrs = [np.ascontiguousarray(x, dtype=np.float32).reshape(-1) for x in (pb, dist, cos_light, area)]
    n = int(arrs[0].size)
    if any(a.size != n for a in arrs):
        raise ValueError("host_mis_weights: pb, dist, cos_light and area must have one length")
    out = np.zeros((n, 8), np.float32)
    wb = np.zeros(n, np.float32)
    ptrs = [a.ctypes.data_as(A.VP) if n else None for a in arrs]
    _check(lib.rtr_host_mis_weights(n, ptrs[0], ptrs[1], ptrs[2], ptrs[3], int(tris), int(picks), out.ctypes.data_as(A.VP) if n else None,
                                    wb.ctypes.data_as(A.VP) if n else None), "rtr_host_mis_weights")
    return out, wb


def _aligned_copy(x, align=16):
    """a C-contiguous copy of x whose data starts at a multiple of align bytes"""
    buf = np.zeros(x.nbytes + align, np.uint8)
    off = (-buf.ctypes.data) % align
    out = buf[off:off + x.nbytes].view(x.dtype).reshape(x.shape)
    out[...] = x
    return out


def host_emitter_hits(rays, hits, prev_surfaces, bounces, light_tris, light_first, lights, mis):
    """rtr_host_emitter_hits: emitter_hits on the host, no device -> EmitterResult of numpy arrays.  light_tris, light_first:
    Scene.export_light_tris(); lights: the scene's A.RtrAreaLightInfo records (a sequence or a ctypes array)."""
    return _host_emitter_hits(rays, hits, prev_surfaces, bounces, light_tris, light_first, lights, mis, None)


def _host_emitter_hits(rays, hits, prev_surfaces, bounces, light_tris, light_first, lights, mis, _cdf):
    """host_emitter_hits (_cdf is None) and host_emitter_hits_power: the same arrays"""
    lib = A.hip_lib()
    who = "host_emitter_hits"
    r, h = _aligned_copy(_host_words(rays, (8,), "rays", who)), _aligned_copy(_host_words(hits, (8,), "hits", who))
    s, b = _aligned_copy(_host_words(prev_surfaces, (20,), "prev_surfaces", who)), _aligned_copy(_host_words(bounces, (8,), "bounces", who))
    n = int(r.shape[0])
    if h.shape[0] != n or s.shape[0] != n or b.shape[0] != n:
        raise ValueError(f"{who}: {n} rays but {h.shape[0]} hits, {s.shape[0]} surfaces and {b.shape[0]} bounce records")
    lt = np.ascontiguousarray(light_tris, dtype=np.float32).reshape(-1, 16)
    lf = np.ascontiguousarray(light_first, dtype=np.uint32).reshape(-1)
    li = (A.RtrAreaLightInfo * len(lights))(*lights)
    if lf.size != len(lights):
        raise ValueError(f"{who}: {lf.size} first records but {len(lights)} lights")
    if any(int(lf[l]) + int(li[l].numTriangles) > lt.shape[0] for l in range(len(lights))):
        raise ValueError(f"{who}: the lights' triangles reach past the {lt.shape[0]} records of light_tris")
    out = _aligned_copy(np.zeros((n, 8), np.float32))
    if _cdf is not None:                 # host_emitter_hits_power: the same arrays and the table's sums
        c = np.ascontiguousarray(_cdf, dtype=np.uint64).reshape(-1)
        _check(lib.rtr_host_emitter_hits_power(r.ctypes.data_as(A.VP) if n else None, h.ctypes.data_as(A.VP) if n else None, s.ctypes.data_as(A.VP) if n else None,
                                               b.ctypes.data_as(A.VP) if n else None, n, lt.ctypes.data_as(A.VP) if lt.size else None,
                                               lf.ctypes.data_as(A.VP) if lf.size else None, li if len(lights) else None, len(lights),
                                               c.ctypes.data_as(A.VP) if c.size else None, C.byref(mis), out.ctypes.data_as(A.VP) if n else None),
               "host_emitter_hits_power")
        return _emitter_result(out, True, None)
    _check(lib.rtr_host_emitter_hits(r.ctypes.data_as(A.VP) if n else None, h.ctypes.data_as(A.VP) if n else None, s.ctypes.data_as(A.VP) if n else None,
                                     b.ctypes.data_as(A.VP) if n else None, n, lt.ctypes.data_as(A.VP) if lt.size else None,
                                     lf.ctypes.data_as(A.VP) if lf.size else None, li if len(lights) else None, len(lights), C.byref(mis),
                                     out.ctypes.data_as(A.VP) if n else None), who)
    return _emitter_result(out, True, None)


# ---- power-proportional light picks (rtr_pick_slots_power and the power forms of the MIS calls; include/rtr_power.h) --------------------
def pick_slots_power(scene, n, params, pick, seeds=None, ctx=None, asynchronous=False):
    """rtr_pick_slots_power: for n hits the area slots of pick.numPicks (P) picks each, drawn in proportion to the power of the light
    triangles (the scene's light-power table), and the weights shade_hits_picked is to give them -> (slots, weights): int32 (n, P)
    (uint32 for numpy; A.PICK_NONE: no triangle emits) and float32 (n, P), total / (P * weight of the slot's triangle).  seeds: int32
    (n,) on the device (numpy in gives numpy out) or None, then the pixels' of params.width / spp; params: make_light_params(...) —
    numAreaLights, numShadowRays, frame; pick.depth enters the seeds as in light_rays_picked.  slots go to light_rays_picked(slots=)."""
    torch = _torch()
    ctx = ctx or scene.ctx
    dev = torch.device("cuda", ctx.device)
    n, p = int(n), int(pick.numPicks)
    as_numpy = isinstance(seeds, np.ndarray)
    sd = _device_vector(torch, seeds, torch.int32, (np.int32, np.uint32), n, "seeds", dev, "pick_slots_power")
    _check_async(ctx, torch, dev, "pick_slots_power", asynchronous)
    slots = torch.empty((n, p), dtype=torch.int32, device=dev)
    weights = torch.empty((n, p), dtype=torch.float32, device=dev)
    _join_torchs_stream(ctx, torch, dev, asynchronous)
    fn = ctx.lib.rtr_pick_slots_power_async if asynchronous else ctx.lib.rtr_pick_slots_power
    _check(fn(ctx.h, scene.h, n, C.byref(params), C.byref(pick), _ptr(sd, n), _ptr(slots, n), _ptr(weights, n)), "rtr_pick_slots_power")
    if as_numpy:
        return slots.cpu().numpy().view(np.uint32), weights.cpu().numpy()
    slots._keep = sd                     # an asynchronous call's inputs stay alive with its result
    return slots, weights


def mis_pick_weights_power(scene, rays, hits, params, pick, mis, slots, seeds=None, samples=False, ctx=None, asynchronous=False):
    """rtr_mis_pick_weights_power: mis_pick_weights for power-proportional picks -> float32 (N, P): wPow * wPick, with the probability
    of each slot's triangle read from the scene's light-power table; 0 for a pick without a ray and for a triangle of weight 0.
    slots is needed: pick_slots_power's (N, P), or the caller's.  The other arguments and samples=True as mis_pick_weights."""
    return _mis_pick_weights("mis_pick_weights_power", scene, rays, hits, params, pick, mis, slots, seeds, samples, ctx, asynchronous, need_slots=True)


def emitter_hits_power(scene, rays, hits, prev_surfaces, bounces, mis, ctx=None, asynchronous=False):
    """rtr_emitter_hits_power: emitter_hits for a vertex whose picks were power-proportional -> EmitterResult; the pick density of the
    hit triangle comes from the scene's light-power table.  The arguments as emitter_hits."""
    return _emitter_hits("rtr_emitter_hits_power", scene, rays, hits, prev_surfaces, bounces, mis, ctx, asynchronous)


def host_light_power(light_tris, light_first, lights):
    """rtr_host_light_power: the light-power table on the host, no device -> (weights, cdf): uint32 (T,), uint64 (T,).  light_tris,
    light_first: Scene.export_light_tris(); lights: the scene's A.RtrAreaLightInfo records (a sequence or a ctypes array)."""
    lib = A.hip_lib()
    who = "host_light_power"
    lt = np.ascontiguousarray(light_tris, dtype=np.float32).reshape(-1, 16)
    lf = np.ascontiguousarray(light_first, dtype=np.uint32).reshape(-1)
    li = (A.RtrAreaLightInfo * len(lights))(*lights)
    if lf.size != len(lights):
        raise ValueError(f"{who}: {lf.size} first records but {len(lights)} lights")
    total = sum(int(l.numTriangles) for l in li)
    if total != lt.shape[0]:
        raise ValueError(f"{who}: the lights have {total} triangles but light_tris {lt.shape[0]} records")
    w, cdf = np.zeros(total, np.uint32), np.zeros(total, np.uint64)
    _check(lib.rtr_host_light_power(lt.ctypes.data_as(A.VP) if lt.size else None, lf.ctypes.data_as(A.VP) if lf.size else None, li if len(lights) else None,
                                    len(lights), w.ctypes.data_as(A.VP) if total else None, cdf.ctypes.data_as(A.VP) if total else None), who)
    return w, cdf


def _host_cdf(cdf, tris, who):
    c = np.ascontiguousarray(cdf, dtype=np.uint64).reshape(-1)
    if int(tris) > c.size:
        raise ValueError(f"{who}: tris {tris} but the table has {c.size} sums")
    return c


def host_pick_slots_power(cdf, tris, seeds, n, params, pick):
    """rtr_host_pick_slots_power: the slots and weights pick_slots_power gives n hits, on the host -> (uint32 (n, P), float32 (n, P)).
    cdf: the table's sums (host_light_power's or an exported table's); tris: Ttot, the triangles of the first params.numAreaLights
    lights; seeds: int32 / uint32 (n,) or None (the pixels' of params.width / spp)."""
    lib = A.hip_lib()
    who = "host_pick_slots_power"
    n = int(n)
    c = _host_cdf(cdf, tris, who)
    sd = None
    if seeds is not None:
        sd = np.ascontiguousarray(seeds)
        if sd.dtype not in (np.int32, np.uint32) or sd.shape != (n,):
            raise ValueError(f"{who}: seeds must be int32 or uint32 ({n},), got {sd.dtype} {sd.shape}")
    p = int(pick.numPicks)
    slots, weights = np.zeros((n, p), np.uint32), np.zeros((n, p), np.float32)
    _check(lib.rtr_host_pick_slots_power(c.ctypes.data_as(A.VP) if c.size else None, int(tris), sd.ctypes.data_as(A.VP) if sd is not None and n else None, n,
                                         C.byref(params), C.byref(pick), slots.ctypes.data_as(A.VP) if slots.size else None,
                                         weights.ctypes.data_as(A.VP) if weights.size else None), who)
    return slots, weights


def host_mis_weights_power(pb, dist, cos_light, area, light_tri, cdf, tris, picks):
    """rtr_host_mis_weights_power: the balance heuristic of include/rtr_power.h for N directions -> (samples, w_bounce, weights): the
    float32 (N, 8) RtrMisSample records (lightPdf, pb, wPick, cosLight, dist, area and the words lightTri, 0), wBounce (N,) and the
    weight mis_pick_weights_power gives a pick on that triangle (N,).  light_tri: the triangle of each direction; cdf, tris: the table
    and Ttot; picks: P (0: nobody picks)."""
    lib = A.hip_lib()
    who = "host_mis_weights_power"
    arrs = [np.ascontiguousarray(x, dtype=np.float32).reshape(-1) for x in (pb, dist, cos_light, area)]
    lt = np.ascontiguousarray(light_tri).reshape(-1)
    if lt.dtype not in (np.int32, np.uint32):
        lt = lt.astype(np.uint32)
    n = int(arrs[0].size)
    if any(a.size != n for a in arrs) or lt.size != n:
        raise ValueError(f"{who}: pb, dist, cos_light, area and light_tri must have one length")
    c = _host_cdf(cdf, tris, who)
    out = np.zeros((n, 8), np.float32)
    wb, wt = np.zeros(n, np.float32), np.zeros(n, np.float32)
    ptrs = [a.ctypes.data_as(A.VP) if n else None for a in arrs]
    _check(lib.rtr_host_mis_weights_power(n, ptrs[0], ptrs[1], ptrs[2], ptrs[3], lt.ctypes.data_as(A.VP) if n else None,
                                          c.ctypes.data_as(A.VP) if c.size else None, int(tris), int(picks), out.ctypes.data_as(A.VP) if n else None,
                                          wb.ctypes.data_as(A.VP) if n else None, wt.ctypes.data_as(A.VP) if n else None), who)
    return out, wb, wt


def host_emitter_hits_power(rays, hits, prev_surfaces, bounces, light_tris, light_first, lights, cdf, mis):
    """rtr_host_emitter_hits_power: emitter_hits_power on the host, no device -> EmitterResult of numpy arrays.  cdf: the table's sums;
    the other arguments as host_emitter_hits."""
    return _host_emitter_hits(rays, hits, prev_surfaces, bounces, light_tris, light_first, lights, mis, cdf)


def direct_light_power(scene, rays, hits=None, params=None, picks=1, pick_depth=0, seeds=None, mis=None, ctx=None, max_ray_bytes=256 << 20, occlusion="dense",
                       shadow_cull_mask=None, shadow_ray_flags=0):
    """direct_light's picked route with power-proportional picks: closest hit (when hits is None) -> pick_slots_power ->
    light_rays_picked(slots=) -> trace_rays(any_hit=True) ("dense") or trace_occlusion ("queued") -> shade_hits_picked(weights=), in
    direct_light's chunks: picks + 1 rays per hit, an unbiased estimate of the light loops' shadowed (and unshadowed) sum whose variance
    does not grow with the spread of the lights' powers.  mis: None — the weights are pick_slots_power's — or make_mis_params(...) of
    the vertex's bounce: then they are mis_pick_weights_power's for the same slots, and the bounce ray is to count the lights it meets
    (emitter_hits_power).  The analytic sum is refused.  The other arguments as direct_light.  -> RadianceResult on the device."""
    shadow_ray_flags = _ray_flags("direct_light_power", shadow_ray_flags, False)
    if occlusion not in ("dense", "queued"):
        raise ValueError(f"direct_light_power: occlusion must be 'dense' or 'queued' (the picked rays have no start hints), got {occlusion!r}")
    return _direct_light("direct_light_power", scene, rays, hits, params, seeds, ctx, max_ray_bytes, occlusion, shadow_cull_mask, shadow_ray_flags, picks, pick_depth,
                         power=True, mis=mis)


# ---- resampled light picks (rtr_pick_slots_ris; include/rtr_ris.h) -----------------------------------------------------------------------
class RisResult:
    """What pick_slots_ris gives back: slots int32 (N, P) (uint32 for numpy; A.PICK_NONE: no pick) and weights float32 (N, P) for
    light_rays_picked(slots=) and shade_hits_picked(weights=); with samples=True candidates (N, P, M), the slots the picks were chosen
    among, and targets float32 (N, P, M), each candidate's target as used; None without."""
    slots = weights = candidates = targets = None


def make_ris_params(candidates, mis=False, lobes=0):
    """rtr_ris_params: candidates (M, 1 ... A.RIS_MAX_CANDIDATES) draws from the light-power table per pick; mis: A.RIS_MIS — the picks are
    weighted against the vertex's bounce, whose lobes (make_bounce_params') are then needed; without it lobes stays 0"""
    return A.rtr_ris_params(int(candidates), A.RIS_MIS if mis else 0, int(lobes))


def pick_slots_ris(scene, rays, hits, params, pick, ris, seeds=None, samples=False, ctx=None, asynchronous=False):
    """rtr_pick_slots_ris: pick_slots_power with eyes — each of the pick.numPicks (P) picks of a hit is chosen among ris.numCandidates
    (M) slots drawn from the scene's light-power table, in proportion to the unshadowed contribution shade_hits_picked would evaluate
    at each (the BRDF, both cosines, the distance, the light's colour and its one-sidedness) -> RisResult, on the device (numpy in gives
    numpy out).  With ris.flags = A.RIS_MIS the weights carry the wPick of mis_pick_weights_power, whose place the call takes too.
    rays, hits, params, seeds as shade_hits_picked takes them; samples=True: the candidates and their targets as well."""
    torch = _torch()
    ctx = ctx or scene.ctx
    dev = torch.device("cuda", ctx.device)
    r, h, sd, as_numpy = _light_inputs(torch, scene, rays, hits, seeds, ctx, "pick_slots_ris", asynchronous)
    n, p, m = int(r.shape[0]), int(pick.numPicks), int(ris.numCandidates)
    res = RisResult()
    res.slots = torch.empty((n, p), dtype=torch.int32, device=dev)
    res.weights = torch.empty((n, p), dtype=torch.float32, device=dev)
    if samples:
        res.candidates = torch.empty((n, p, m), dtype=torch.int32, device=dev)
        res.targets = torch.empty((n, p, m), dtype=torch.float32, device=dev)
    _join_torchs_stream(ctx, torch, dev, asynchronous)
    fn = ctx.lib.rtr_pick_slots_ris_async if asynchronous else ctx.lib.rtr_pick_slots_ris
    _check(fn(ctx.h, scene.h, _ptr(r, n), _ptr(h, n), n, C.byref(params), C.byref(pick), C.byref(ris), _ptr(sd, n), _ptr(res.slots, n), _ptr(res.weights, n),
              _ptr(res.candidates, n) if samples else None, _ptr(res.targets, n) if samples else None), "rtr_pick_slots_ris")
    if as_numpy:
        res.slots, res.weights = res.slots.cpu().numpy().view(np.uint32), res.weights.cpu().numpy()
        if samples:
            res.candidates, res.targets = res.candidates.cpu().numpy().view(np.uint32), res.targets.cpu().numpy()
    res._keep = (r, h, sd)               # an asynchronous call's inputs stay alive with its result
    return res


def _host_seeds(seeds, n, who):
    if seeds is None:
        return None
    sd = np.ascontiguousarray(seeds)
    if sd.dtype not in (np.int32, np.uint32) or sd.shape != (n,):
        raise ValueError(f"{who}: seeds must be int32 or uint32 ({n},), got {sd.dtype} {sd.shape}")
    return sd


def host_ris_candidates(cdf, tris, seeds, n, params, pick, candidates):
    """rtr_host_ris_candidates: the candidates pick_slots_ris draws for n hits, on the host -> uint32 (n, P, M).  cdf, tris, seeds, params,
    pick as host_pick_slots_power takes them; candidates: M."""
    lib = A.hip_lib()
    who = "host_ris_candidates"
    n, m = int(n), int(candidates)
    c = _host_cdf(cdf, tris, who)
    sd = _host_seeds(seeds, n, who)
    out = np.zeros((n, int(pick.numPicks), max(m, 0)), np.uint32)
    _check(lib.rtr_host_ris_candidates(c.ctypes.data_as(A.VP) if c.size else None, int(tris), sd.ctypes.data_as(A.VP) if sd is not None and n else None, n,
                                       C.byref(params), C.byref(pick), m, out.ctypes.data_as(A.VP) if out.size else None), who)
    return out


def host_ris_select(cdf, tris, seeds, n, params, pick, ris, candidates, targets, w_pick=None):
    """rtr_host_ris_select: the reservoir of include/rtr_ris.h over candidates uint32 (n, P, M) and targets float32 (n, P, M) handed in, on
    the host -> (slots uint32 (n, P), weights float32 (n, P)).  w_pick: float32 (n, P, M), the candidates' wPick, with ris.flags =
    A.RIS_MIS (the targets already contain it); None without.  The other arguments as host_ris_candidates."""
    lib = A.hip_lib()
    who = "host_ris_select"
    n, p, m = int(n), int(pick.numPicks), int(ris.numCandidates)
    c = _host_cdf(cdf, tris, who)
    sd = _host_seeds(seeds, n, who)
    cand = np.ascontiguousarray(candidates)
    if cand.dtype not in (np.int32, np.uint32) or cand.size != n * p * m:
        raise ValueError(f"{who}: candidates must be int32 or uint32 ({n}, {p}, {m}), got {cand.dtype} {cand.shape}")
    tg = np.ascontiguousarray(targets, dtype=np.float32)
    wp = None if w_pick is None else np.ascontiguousarray(w_pick, dtype=np.float32)
    if tg.size != n * p * m or (wp is not None and wp.size != n * p * m):
        raise ValueError(f"{who}: targets and w_pick must be float32 ({n}, {p}, {m})")
    slots, weights = np.zeros((n, p), np.uint32), np.zeros((n, p), np.float32)
    ptr = lambda x: x.ctypes.data_as(A.VP) if x is not None and x.size else None
    _check(lib.rtr_host_ris_select(ptr(c), int(tris), ptr(sd) if n else None, n, C.byref(params), C.byref(pick), C.byref(ris), ptr(cand), ptr(tg), ptr(wp),
                                   ptr(slots), ptr(weights)), who)
    return slots, weights


def direct_light_ris(scene, rays, hits=None, params=None, picks=1, candidates=4, pick_depth=0, seeds=None, mis=None, ctx=None, max_ray_bytes=256 << 20,
                     occlusion="dense", shadow_cull_mask=None, shadow_ray_flags=0):
    """direct_light_power with resampled picks: closest hit (when hits is None) -> pick_slots_ris(make_ris_params(candidates, ...)) ->
    light_rays_picked(slots=) -> the occlusion query -> shade_hits_picked(weights=), in direct_light's chunks: still picks + 1 rays per
    hit, each pick chosen among `candidates` draws of the power table by what it would contribute at the hit.  mis: None, or
    make_mis_params(...) of the vertex's bounce — then the call passes A.RIS_MIS with mis.lobes, and the bounce ray is to count the lights
    it meets (emitter_hits_power), as with direct_light_power.  The other arguments as direct_light_power.  -> RadianceResult."""
    shadow_ray_flags = _ray_flags("direct_light_ris", shadow_ray_flags, False)
    if occlusion not in ("dense", "queued"):
        raise ValueError(f"direct_light_ris: occlusion must be 'dense' or 'queued' (the picked rays have no start hints), got {occlusion!r}")
    ris = make_ris_params(candidates, mis is not None, mis.lobes if mis is not None else 0)
    return _direct_light("direct_light_ris", scene, rays, hits, params, seeds, ctx, max_ray_bytes, occlusion, shadow_cull_mask, shadow_ray_flags, picks, pick_depth,
                         power=True, mis=mis, ris=ris)


# ---- sky importance sampling at a path vertex (rtr_sky_rays, rtr_shade_sky, rtr_sky_hits; include/rtr_sky.h) ---------------------------
class SkyTable:
    """A sky table on the host: width, height, rows — uint32 (height, width), each row's inclusive prefix sums of its cell weights — and
    marginal — uint64 (height,), the inclusive prefix sums of the row totals.  total: the sum of all weights (0: a black sky)."""
    def __init__(self, width, height, rows, marginal):
        self.width, self.height, self.rows, self.marginal = int(width), int(height), rows, marginal

    @property
    def total(self):
        return int(self.marginal[-1])

    def weights(self):
        """the cell weights, uint32 (height, width)"""
        return np.diff(self.rows.astype(np.int64), axis=1, prepend=0).astype(np.uint32)

    def _c(self):
        return A.rtr_sky_table(self.rows.ctypes.data_as(C.POINTER(C.c_uint32)), self.marginal.ctypes.data_as(C.POINTER(C.c_uint64)), self.width, self.height)


class SkyResult:
    """What sky_rays and host_sky_rays give back.  rays: the (N, S, 8) float32 RtrRay of the samples (eight zeros: a dead sample).  raw:
    the (N, S, 8) float32 array of RtrSkySample records, of which contrib (N, S, 3), sky_pdf, bounce_pdf and w_sky (N, S) are float32
    views and cell (y * W + x of the table) an int32 view."""
    rays = raw = contrib = sky_pdf = bounce_pdf = w_sky = cell = None


def _sky_result(rays, raw, as_numpy, torch):
    res = SkyResult()
    words = raw.view(np.int32) if as_numpy else raw.view(torch.int32)
    res.rays, res.raw = rays, raw
    res.contrib, res.sky_pdf, res.bounce_pdf, res.w_sky, res.cell = raw[..., 0:3], raw[..., 3], raw[..., 4], raw[..., 5], words[..., 6]
    return res


class SkyEscapeResult:
    """What sky_hits and host_sky_hits give back.  raw: the (N, 8) float32 array of RtrSkyEscape records, of which radiance (N, 3) (to be
    multiplied by the throughput after the bounce), w_bounce, sky_pdf and bounce_pdf (N,) are float32 views and cell, kind int32 views."""
    raw = radiance = w_bounce = sky_pdf = bounce_pdf = cell = kind = None


def _sky_escape_result(raw, as_numpy, torch):
    res = SkyEscapeResult()
    words = raw.view(np.int32) if as_numpy else raw.view(torch.int32)
    res.raw = raw
    res.radiance, res.w_bounce, res.sky_pdf, res.bounce_pdf, res.cell, res.kind = raw[:, 0:3], raw[:, 3], raw[:, 4], raw[:, 5], words[:, 6], words[:, 7]
    return res


def make_sky_params(samples=1, depth=0, frame=0, width=0, spp=1, lobes=A.BOUNCE_DIFFUSE | A.BOUNCE_SPECULAR, mis=True):
    """rtr_sky_params: the sky samples per vertex (S), depth and frame of the seeds, width / spp of the pixel rule (used without explicit
    seeds), the lobes the vertex's bounce samples, and whether the balance heuristic against that bounce applies"""
    return A.rtr_sky_params(int(samples), int(depth) & 0xffffffff, int(frame) & 0xffffffff, int(width), int(spp), int(lobes), A.SKY_MIS if mis else 0, 0)


def sky_rays(scene, rays, surfaces, params, seeds=None, ctx=None, asynchronous=False):
    """rtr_sky_rays: S directions per hit drawn in proportion to the scene's sky, each with its shadow ray and its contribution ->
    SkyResult.  rays: the float32 (N, 8) rays that found the hits; surfaces: hit_surfaces' SurfaceResult or its (N, 20) raw records;
    seeds: int32 (N,) seed bases, default the pixel's (params.width, params.spp).  Device tensors in give device tensors out, numpy in
    gives numpy out; asynchronous as in trace_rays."""
    torch = _torch()
    ctx = ctx or scene.ctx
    dev = torch.device("cuda", ctx.device)
    who = "sky_rays"
    if isinstance(surfaces, SurfaceResult):
        surfaces = surfaces.raw
    r, as_numpy = _device_array(torch, rays, torch.float32, np.float32, "rays", dev, who)
    if isinstance(surfaces, np.ndarray) != as_numpy:
        raise ValueError(f"{who}: rays and surfaces must both be numpy arrays or both be tensors")
    s = _records(torch, surfaces, 20, "surfaces", dev, who, as_numpy)
    n, S = int(r.shape[0]), int(params.numSamples)
    if int(s.shape[0]) != n:
        raise ValueError(f"{who}: {n} rays but {s.shape[0]} surfaces")
    sd = _device_vector(torch, seeds, torch.int32, (np.int32, np.uint32), n, "seeds", dev, who)
    _check_async(ctx, torch, dev, who, asynchronous)
    out_rays = torch.empty((n, S, 8), dtype=torch.float32, device=dev)
    out_s = torch.empty((n, S, 8), dtype=torch.float32, device=dev)
    _join_torchs_stream(ctx, torch, dev, asynchronous)
    fn = ctx.lib.rtr_sky_rays_async if asynchronous else ctx.lib.rtr_sky_rays
    _check(fn(ctx.h, scene.h, _ptr(r, n), _ptr(s, n), n, C.byref(params), _ptr(sd, n), _ptr(out_rays, n * S), _ptr(out_s, n * S)), "rtr_sky_rays")
    res = _sky_result(out_rays.cpu().numpy(), out_s.cpu().numpy(), True, torch) if as_numpy else _sky_result(out_rays, out_s, False, torch)
    res._keep = (r, s, sd)               # an asynchronous call's inputs stay alive with its result
    return res


def shade_sky(ctx, samples, occluded, asynchronous=False):
    """rtr_shade_sky: per hit the sum, over its samples in order, of contrib where the sample's ray is not occluded -> float32 (N, 3).
    samples: sky_rays' SkyResult or its (N, S, 8) raw records; occluded: uint8 (N, S) or (N * S,), what an any-hit query of the sample
    rays reported.  Device tensors in give a device tensor out, numpy in gives numpy out."""
    torch = _torch()
    dev = torch.device("cuda", ctx.device)
    who = "shade_sky"
    if isinstance(samples, SkyResult):
        samples = samples.raw
    as_numpy = isinstance(samples, np.ndarray)
    if samples.ndim != 3 or samples.shape[2] != 8:
        raise ValueError(f"{who}: samples must be float32 (N, S, 8), got {tuple(samples.shape)}")
    n, S = int(samples.shape[0]), int(samples.shape[1])
    rec = _records(torch, samples.reshape(n * S, 8), 8, "samples", dev, who, as_numpy)
    if isinstance(occluded, np.ndarray) != as_numpy:
        raise ValueError(f"{who}: samples and occluded must both be numpy arrays or both be tensors")
    occ = torch.from_numpy(np.ascontiguousarray(occluded)).to(dev) if as_numpy else occluded
    if occ.dtype != torch.uint8 or occ.numel() != n * S or occ.device != dev or not occ.is_contiguous():
        raise ValueError(f"{who}: occluded must be contiguous uint8 with {n * S} elements on {dev}")
    _check_async(ctx, torch, dev, who, asynchronous)
    out = torch.empty((n, 4), dtype=torch.float32, device=dev)
    _join_torchs_stream(ctx, torch, dev, asynchronous)
    fn = ctx.lib.rtr_shade_sky_async if asynchronous else ctx.lib.rtr_shade_sky
    _check(fn(ctx.h, _ptr(rec, n), _ptr(occ, n), n, S, _ptr(out, n)), "rtr_shade_sky")
    res = out[:, 0:3]
    if as_numpy:
        return res.cpu().numpy()
    res._keep = (rec, occ)
    return res


def sky_hits(scene, rays, hits, prev_surfaces, bounces, params, ctx=None, asynchronous=False):
    """rtr_sky_hits: what each bounce ray adds where it misses the scene -> SkyEscapeResult.  rays: the bounce rays (N, 8); hits: their
    closest hits (a QueryResult or (N, 8) int32 records); prev_surfaces: the SurfaceResult (or (N, 20) float32 records) of the vertices the
    rays left; bounces: bounce_rays' BounceResult (or its (N, 8) raw records) at those vertices; params: make_sky_params(...), whose
    samples may be 0 here.  Device tensors in give device tensors out, numpy in gives numpy out."""
    torch = _torch()
    ctx = ctx or scene.ctx
    dev = torch.device("cuda", ctx.device)
    who = "sky_hits"
    if isinstance(prev_surfaces, SurfaceResult):
        prev_surfaces = prev_surfaces.raw
    if isinstance(bounces, BounceResult):
        bounces = bounces.raw
    r, h, _, as_numpy = _light_inputs(torch, scene, rays, hits, None, ctx, who, asynchronous)
    n = int(r.shape[0])
    if isinstance(prev_surfaces, np.ndarray) != as_numpy or isinstance(bounces, np.ndarray) != as_numpy:
        raise ValueError(f"{who}: rays, hits, prev_surfaces and bounces must all be numpy arrays or all be tensors")
    s = _records(torch, prev_surfaces, 20, "prev_surfaces", dev, who, as_numpy)
    b = _records(torch, bounces, 8, "bounces", dev, who, as_numpy)
    if int(s.shape[0]) != n or int(b.shape[0]) != n:
        raise ValueError(f"{who}: {n} rays but {s.shape[0]} surfaces and {b.shape[0]} bounce records")
    out = torch.empty((n, 8), dtype=torch.float32, device=dev)
    _join_torchs_stream(ctx, torch, dev, asynchronous)
    fn = ctx.lib.rtr_sky_hits_async if asynchronous else ctx.lib.rtr_sky_hits
    _check(fn(ctx.h, scene.h, _ptr(r, n), _ptr(h, n), _ptr(s, n), _ptr(b, n), n, C.byref(params), _ptr(out, n)), "rtr_sky_hits")
    res = _sky_escape_result(out.cpu().numpy() if as_numpy else out, as_numpy, torch)
    res._keep = (r, h, s, b)
    return res


def _host_sky(hdri, sky_color, who):
    """(texture pointer or None, its keep-alive, the sky colour's pointer) of a host sky: hdri a uint8 (H, W, 4) / (H, W, 1) / (H, W) array or None"""
    col = np.ascontiguousarray(sky_color if sky_color is not None else (0.0, 0.0, 0.0), dtype=np.float32).reshape(3)
    if hdri is None:
        return None, (col,), col.ctypes.data_as(A.VP)
    px = np.ascontiguousarray(hdri)
    if px.dtype != np.uint8 or px.ndim not in (2, 3) or (px.ndim == 3 and px.shape[2] not in (1, 4)):
        raise ValueError(f"{who}: hdri must be uint8 (H, W, 4), (H, W, 1) or (H, W), got {px.dtype} {px.shape}")
    tex = A.rtr_texture(px.ctypes.data_as(C.POINTER(C.c_uint8)), px.shape[1], px.shape[0], px.shape[2] if px.ndim == 3 else 1, 0)
    return C.byref(tex), (px, tex, col), col.ctypes.data_as(A.VP)


def host_sky_table(hdri=None, sky_color=None):
    """rtr_host_sky_table: the sky table of an HDRI (uint8 (H, W, 4) RGBA8 or (H, W) / (H, W, 1) R8) or, with hdri None, of the constant
    sky of sky_color (three sRGB-encoded floats), built on the host -> SkyTable.  Scene.export_sky_table() gives the same words."""
    lib = A.hip_lib()
    tex, keep, col = _host_sky(hdri, sky_color, "host_sky_table")
    w, h = C.c_uint32(0), C.c_uint32(0)
    lib.rtr_host_sky_table(tex, col, C.byref(w), C.byref(h), None, 0, None, 0)      # refused: reports the extent
    if w.value == 0:
        _check(lib.rtr_host_sky_table(tex, col, C.byref(w), C.byref(h), None, 0, None, 0), "rtr_host_sky_table")
    rows, marginal = np.zeros((h.value, w.value), np.uint32), np.zeros(h.value, np.uint64)
    _check(lib.rtr_host_sky_table(tex, col, C.byref(w), C.byref(h), rows.ctypes.data_as(A.VP), rows.size, marginal.ctypes.data_as(A.VP), h.value), "rtr_host_sky_table")
    return SkyTable(w.value, h.value, rows, marginal)


def host_sky_rays(table, rays, surfaces, params, seeds=None, hdri=None, sky_color=None):
    """rtr_host_sky_rays: sky_rays on the host, no device -> SkyResult of numpy arrays.  table: the SkyTable of the sky (hdri, sky_color
    as host_sky_table takes them)."""
    lib = A.hip_lib()
    who = "host_sky_rays"
    tex, keep, col = _host_sky(hdri, sky_color, who)
    r, s = _aligned_copy(_host_words(rays, (8,), "rays", who)), _aligned_copy(_host_words(surfaces, (20,), "surfaces", who))
    n, S = int(r.shape[0]), int(params.numSamples)
    if s.shape[0] != n:
        raise ValueError(f"{who}: {n} rays but {s.shape[0]} surfaces")
    sd = None
    if seeds is not None:
        sd = np.ascontiguousarray(seeds)
        if sd.dtype not in (np.int32, np.uint32) or sd.shape != (n,):
            raise ValueError(f"{who}: seeds must be int32 or uint32 ({n},), got {sd.dtype} {sd.shape}")
    out_rays, out_s = _aligned_copy(np.zeros((n, max(S, 1), 8), np.float32)), _aligned_copy(np.zeros((n, max(S, 1), 8), np.float32))
    t = table._c()
    _check(lib.rtr_host_sky_rays(tex, col, C.byref(t), r.ctypes.data_as(A.VP) if n else None, s.ctypes.data_as(A.VP) if n else None, n, C.byref(params),
                                 sd.ctypes.data_as(A.VP) if sd is not None and n else None, out_rays.ctypes.data_as(A.VP) if n else None,
                                 out_s.ctypes.data_as(A.VP) if n else None), "rtr_host_sky_rays")
    return _sky_result(out_rays, out_s, True, None)


def host_sky_hits(table, rays, hits, prev_surfaces, bounces, params, hdri=None, sky_color=None):
    """rtr_host_sky_hits: sky_hits on the host, no device -> SkyEscapeResult of numpy arrays"""
    lib = A.hip_lib()
    who = "host_sky_hits"
    tex, keep, col = _host_sky(hdri, sky_color, who)
    r, h = _aligned_copy(_host_words(rays, (8,), "rays", who)), _aligned_copy(_host_words(hits, (8,), "hits", who))
    s, b = _aligned_copy(_host_words(prev_surfaces, (20,), "prev_surfaces", who)), _aligned_copy(_host_words(bounces, (8,), "bounces", who))
    n = int(r.shape[0])
    if h.shape[0] != n or s.shape[0] != n or b.shape[0] != n:
        raise ValueError(f"{who}: {n} rays but {h.shape[0]} hits, {s.shape[0]} surfaces and {b.shape[0]} bounce records")
    out = _aligned_copy(np.zeros((n, 8), np.float32))
    t = table._c()
    _check(lib.rtr_host_sky_hits(tex, col, C.byref(t), r.ctypes.data_as(A.VP) if n else None, h.ctypes.data_as(A.VP) if n else None,
                                 s.ctypes.data_as(A.VP) if n else None, b.ctypes.data_as(A.VP) if n else None, n, C.byref(params),
                                 out.ctypes.data_as(A.VP) if n else None), "rtr_host_sky_hits")
    return _sky_escape_result(out, True, None)


def host_sky_pdf(table, dirs):
    """rtr_host_sky_pdf: the solid-angle density of the table for the directions dirs (N, 3) -> float32 (N,)"""
    lib = A.hip_lib()
    d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
    n = int(d.shape[0])
    out = np.zeros(n, np.float32)
    t = table._c()
    _check(lib.rtr_host_sky_pdf(C.byref(t), d.ctypes.data_as(A.VP) if n else None, n, out.ctypes.data_as(A.VP) if n else None), "rtr_host_sky_pdf")
    return out


def host_sky_radiance(dirs, hdri=None, sky_color=None):
    """rtr_host_sky_radiance: the miss rule's radiance for the directions dirs (N, 3) -> float32 (N, 3): RtrSurface::color of a miss"""
    lib = A.hip_lib()
    tex, keep, col = _host_sky(hdri, sky_color, "host_sky_radiance")
    d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
    n = int(d.shape[0])
    out = np.zeros((n, 3), np.float32)
    _check(lib.rtr_host_sky_radiance(tex, col, d.ctypes.data_as(A.VP) if n else None, n, out.ctypes.data_as(A.VP) if n else None), "rtr_host_sky_radiance")
    return out


class PathResult:
    """What path_trace gives back: radiance (N, 3) float32, the sum of per_depth, a list of bounces + 1 (N, 3) tensors — entry d is what
    the path's vertex d contributes, already multiplied by the throughput up to it.  live: with compact=True the number of paths that
    reached vertex d, a list of bounces + 1 ints (live[0] = N); None without."""
    radiance = per_depth = live = None


PATH_SEED_STEP = 0x9E3779B1      # the direct-light seeds of vertex d are the bases + d * this (32-bit words)


def _wrap32(x):
    """an int64 tensor's low 32 bits as int32 (the two's-complement word), without leaning on an out-of-range conversion"""
    x = x & 0xffffffff
    return (x - ((x >> 31) << 32)).to(_torch().int32)


def path_trace(scene, rays, light_params, bounces, seeds=None, occlusion="dense", bounce_cull_mask=None, bounce_ray_flags=0, max_ray_bytes=256 << 20, ctx=None,
               compact=False, roulette_from=None, survival_floor=0.05):
    """N-bounce global illumination from the public parts, all on the device:

        T = 1, L = 0, r = rays
        for d in 0 ... bounces:
            q    = trace_rays(scene, r)                      (from d = 1 on with cull_mask=bounce_cull_mask, ray_flags=bounce_ray_flags)
            rad  = direct_light(scene, r, q, light_params, seeds = seeds if d == 0 else base + d * PATH_SEED_STEP).shadowed
            rad  = 0 where d >= 1 and the hit is a light     (next-event estimation counted that light at the vertex before)
            L   += T * rad;  per_depth.append(T * rad)
            if d == bounces: break
            b    = bounce_rays(ctx, r, hit_surfaces(scene, r, q), make_bounce_params(light_params.frame, d, width, spp), seeds)
            T   *= b.weight;  r = b.rays                      (a dead path carries the null ray and T = 0 from here on)

    base: the explicit seeds, or, with seeds=None, the pixels' px * 733 + py * 1933 from light_params.width / spp, built once.  rays: a
    float32 (N, 8) device tensor; light_params: make_light_params(...); occlusion, max_ray_bytes as direct_light takes them.
    bounce_cull_mask: e.g. the complement of the emitters' mask bit keeps bounce rays off the lights.  By default no Russian roulette
    and no compaction of dead paths: their null rays cost no walk, but they keep their lanes.

    compact=True: the same sum over the LIVE paths only.  r, T, base and ids (ids = 0 ... N - 1 at the start) are arrays of live[d] rows,
    and after the last line of the loop above

            c    = compact_paths(ctx, r, T, base, ids, make_compact_params(light_params.frame, d, roulette, survival_floor))
            n    = c.count                                   (the one join of the vertex);  live.append(n)
            r, T, base, ids = the first n rows of c.rays, c.throughput, c.seeds, c.path_ids        (n = 0 ends the loop: every later term is zeros)

    with roulette = roulette_from is not None and d >= roulette_from.  From the first compaction on every seed is explicit: direct_light
    takes base + d * PATH_SEED_STEP and bounce_rays takes base, the gathered words, which are what the plain loop gives those paths.
    per_depth[d] is zeros (N, 3) with the live terms written at their ids (ids are unique: no atomics).  Without roulette the result
    is the plain loop's: a path compact_paths drops has T = 0 or the null ray, so all its later terms are 0 there too (one difference,
    outside what bounce_rays produces: a throughput that is negative or not finite is dead here).  With roulette a live path of
    p = max(max3(T), survival_floor) < 1 goes on with probability p and T / p (include/rtr_paths.h): the same mean, fewer paths, more
    variance.  roulette_from without compact raises ValueError.  Every vertex takes the full light loops; path_trace_picked is this
    loop with picked light samples at the later vertices.  -> PathResult."""
    return _path_trace("path_trace", "plain", False, scene, rays, light_params, bounces, seeds, occlusion, bounce_cull_mask, bounce_ray_flags, max_ray_bytes, ctx,
                       compact, roulette_from, survival_floor)


def path_trace_picked(scene, rays, light_params, bounces, light_picks=None, pick_from=1, seeds=None, occlusion="dense", bounce_cull_mask=None, bounce_ray_flags=0,
                      max_ray_bytes=256 << 20, ctx=None, compact=False, roulette_from=None, survival_floor=0.05):
    """path_trace with one-sample direct lighting at the path vertices: the same loop, the same arguments, and
    light_picks=P: the vertices d >= pick_from take direct_light(..., picks=P, pick_depth=d) with the seeds path_trace gives them: P picked
    area-light samples and the directional light instead of all Q shadow rays, the same mean (include/rtr_pick.h).  The camera hits keep
    the renderer's full loops by default (pick_from=1).  The picks read other random numbers than the bounce and the roulette, so which
    paths live does not depend on them.  light_picks with light_params.outputs asking for the analytic sum raises ValueError; None: every
    vertex takes the full loops, path_trace's calls and bytes.  -> PathResult."""
    return _path_trace("path_trace_picked", "picked", False, scene, rays, light_params, bounces, seeds, occlusion, bounce_cull_mask, bounce_ray_flags, max_ray_bytes, ctx,
                       compact, roulette_from, survival_floor, light_picks=light_picks, pick_from=pick_from)


def path_trace_mis(scene, rays, light_params, bounces, light_picks=1, pick_from=1, seeds=None, occlusion="dense", bounce_cull_mask=None, bounce_ray_flags=0,
                   max_ray_bytes=256 << 20, ctx=None, compact=False, roulette_from=None, survival_floor=0.05):
    """path_trace_picked with multiple importance sampling between the picks of a vertex and its bounce ray (include/rtr_mis.h): the
    same loop, the same arguments (light_picks=P is needed), and with mis = make_mis_params(P, numAreaLights, numShadowRays)

        a vertex d >= pick_from with d < bounces is a MIS VERTEX: its direct_light(..., picks=P, pick_depth=d) takes
            pick_weights = mis_pick_weights(scene, r, q, light_params, make_pick_params(P, d), mis, None, seeds = that call's seeds)
        at a vertex d >= 1 whose hit is a light, rad = emitter_hits(scene, r, q, S, B, mis).radiance when vertex d - 1 was a MIS vertex
            (S, B: the hit_surfaces and the bounce_rays records of vertex d - 1; T already holds that bounce's weight), else 0 as before.

    The last vertex has no bounce after it: its picks keep the default weights.  A vertex that takes the full light loops (d < pick_from)
    is no MIS vertex, and the bounce ray that leaves it counts no light.  With bounces=0 these are path_trace_picked's calls and bytes.
    compact=True: S and B follow the survivors — compact_paths is called with path_ids=None, so that its ids are the row indices of that
    call; S, B and the pixel ids are gathered with them in torch (ids = ids[rows]), which gives the ids compact_paths would have
    gathered.  Without roulette the result is the plain loop's.  -> PathResult."""
    return _path_trace("path_trace_mis", "mis", False, scene, rays, light_params, bounces, seeds, occlusion, bounce_cull_mask, bounce_ray_flags, max_ray_bytes, ctx,
                       compact, roulette_from, survival_floor, light_picks=light_picks, pick_from=pick_from)


def path_trace_sky(scene, rays, light_params, bounces, sky_samples=1, sky_from=0, sky_mis=True, light_picks=1, pick_from=1, seeds=None, occlusion="dense",
                   bounce_cull_mask=None, bounce_ray_flags=0, max_ray_bytes=256 << 20, ctx=None, compact=False, roulette_from=None, survival_floor=0.05):
    """path_trace_mis with sky importance sampling at the path vertices (include/rtr_sky.h): the same loop, the same arguments, and with
    sky = make_sky_params(S = sky_samples, d, light_params.frame, width, spp, mis=sky_mis)

        a vertex d >= sky_from with d < bounces is a SKY VERTEX: it adds T * shade_sky(k, occluded) of its S samples
            k = sky_rays(scene, r, hit_surfaces(scene, r, q), sky, seeds = the bounce's seeds), traced with RTR_QUERY_ANY by the occlusion=
            route of the light rays ("queued": trace_occlusion, else the dense query)
        at a vertex d >= 1 whose hit is a miss, rad = sky_hits(scene, r, q, S', B', sky).radiance when vertex d - 1 was a sky vertex
            (S', B': the hit_surfaces and bounce_rays records of vertex d - 1), and 0 there with sky_mis=False: that vertex sampled the
            sky itself, as a picked vertex's light hit counts for nothing.  Every other miss adds T * sky as before, and so does the miss
            of a camera ray.

    compact=True: the escape records' inputs follow the survivors as the emitter records' do.  sky_samples=0 is path_trace_mis, tensor
    for tensor.  The samples cover the whole sphere of directions (about half fall below the surface and are dead), and are drawn
    without regard to the BRDF.  -> PathResult."""
    return _path_trace("path_trace_sky", "sky", False, scene, rays, light_params, bounces, seeds, occlusion, bounce_cull_mask, bounce_ray_flags, max_ray_bytes, ctx,
                       compact, roulette_from, survival_floor, sky_samples=sky_samples, sky_from=sky_from, sky_mis=sky_mis, light_picks=light_picks, pick_from=pick_from)


def path_trace_power(scene, rays, light_params, bounces, sky_samples=1, sky_from=0, sky_mis=True, light_picks=1, pick_from=1, seeds=None, occlusion="dense",
                     bounce_cull_mask=None, bounce_ray_flags=0, max_ray_bytes=256 << 20, ctx=None, compact=False, roulette_from=None, survival_floor=0.05):
    """path_trace_sky with power-proportional light picks (include/rtr_power.h): the same loop, the same arguments and defaults, and

        a vertex d >= pick_from takes direct_light_power(..., picks=P, pick_depth=d, mis = the MIS params at a MIS vertex, else None)
            in place of direct_light(..., picks=P): its slots are pick_slots_power's and its weights that call's or
            mis_pick_weights_power's
        at a vertex d >= 1 whose hit is a light, rad = emitter_hits_power(...).radiance when vertex d - 1 was a MIS vertex.

    The picks read the uniform picks' random numbers and one more each, none of them the bounce's or the roulette's, so which paths live
    does not depend on them.  In a scene whose light triangles all have one power the picks' distribution is the uniform one.
    occlusion="queued_own_leaf" raises ValueError at the first picked vertex, as with path_trace_picked.  -> PathResult."""
    return _path_trace("path_trace_power", "power", False, scene, rays, light_params, bounces, seeds, occlusion, bounce_cull_mask, bounce_ray_flags, max_ray_bytes, ctx,
                       compact, roulette_from, survival_floor, sky_samples=sky_samples, sky_from=sky_from, sky_mis=sky_mis, light_picks=light_picks, pick_from=pick_from)


def path_trace_ris(scene, rays, light_params, bounces, sky_samples=1, sky_from=0, sky_mis=True, light_picks=1, pick_from=1, ris_candidates=4, seeds=None,
                   occlusion="dense", bounce_cull_mask=None, bounce_ray_flags=0, max_ray_bytes=256 << 20, ctx=None, compact=False, roulette_from=None,
                   survival_floor=0.05):
    """path_trace_power with resampled light picks (include/rtr_ris.h): the same loop, the same arguments and defaults, and

        a vertex d >= pick_from takes direct_light_ris(..., picks=P, candidates=ris_candidates, pick_depth=d, mis = the MIS params at a
            MIS vertex, else None) in place of direct_light_power: each pick is chosen among ris_candidates draws of the power table by
            what it would contribute at the vertex; a MIS vertex passes RTR_RIS_MIS
        at a vertex d >= 1 whose hit is a light, rad = emitter_hits_power(...).radiance when vertex d - 1 was a MIS vertex, as there.

    The candidates read numbers of their own, none of them the bounce's or the roulette's, so which paths live does not depend on them.
    ris_candidates=1 is path_trace_power's picks.  -> PathResult."""
    return _path_trace("path_trace_ris", "ris", False, scene, rays, light_params, bounces, seeds, occlusion, bounce_cull_mask, bounce_ray_flags, max_ray_bytes, ctx,
                       compact, roulette_from, survival_floor, sky_samples=sky_samples, sky_from=sky_from, sky_mis=sky_mis, light_picks=light_picks, pick_from=pick_from,
                       ris_candidates=ris_candidates)


class _LoopDefault:
    """the default of a path_trace_library keyword: whatever the named loop's own default is"""
    def __repr__(self):
        return "LOOP_DEFAULT"


LOOP_DEFAULT = _LoopDefault()

# the keywords each loop has beyond path_trace's, with their defaults there
_LOOPS = {
    "plain": {},
    "picked": {"light_picks": None, "pick_from": 1},
    "mis": {"light_picks": 1, "pick_from": 1},
    "sky": {"sky_samples": 1, "sky_from": 0, "sky_mis": True, "light_picks": 1, "pick_from": 1},
    "power": {"sky_samples": 1, "sky_from": 0, "sky_mis": True, "light_picks": 1, "pick_from": 1},
    "ris": {"sky_samples": 1, "sky_from": 0, "sky_mis": True, "light_picks": 1, "pick_from": 1, "ris_candidates": 4},
}
# the loops with MIS vertices, and why each of them cannot do without light_picks
_PICKS_NEEDED = {
    "mis": "the MIS is between the picks and the bounce",
    "sky": "the loop is path_trace_mis's",
    "power": "the power table is what the picks are drawn from",
    "ris": "the picks are what is resampled",
}


def _loop_keywords(who, loop, library, given):
    """the keywords of a loop resolved through _LOOPS and checked -> (light_picks, pick_from, sky, ris), sky: (samples, from, mis) or None,
    ris: the candidates per pick or None.
    who: the function that was called; given: its keywords (LOOP_DEFAULT or absent: the loop's own default).  Nothing but the keywords
    is looked at."""
    if loop not in _LOOPS:
        raise ValueError(f"{who}: loop must be one of {', '.join(map(repr, _LOOPS))}, got {loop!r}")
    own, kw = _LOOPS[loop], {}
    for name in _LOOPS["ris"]:
        value = given.get(name, LOOP_DEFAULT)
        if name not in own and value is not LOOP_DEFAULT:
            raise ValueError(f"{who}: loop={loop!r} has no {name}")
        kw[name] = own.get(name) if value is LOOP_DEFAULT else value
    if loop in _PICKS_NEEDED and kw["light_picks"] is None:
        raise ValueError(f"{who}: loop={loop!r} needs light_picks (the MIS is between the picks and the bounce)" if library
                         else f"{who}: light_picks must be given ({_PICKS_NEEDED[loop]})")
    sky = None
    if "sky_samples" in own:
        s = int(kw["sky_samples"])
        if not 0 <= s <= A.SKY_MAX_SAMPLES:
            raise ValueError(f"{who}: sky_samples must be 0 ... {A.SKY_MAX_SAMPLES}, got {s}")
        if int(kw["sky_from"]) < 0:
            raise ValueError(f"{who}: sky_from must be >= 0, got {kw['sky_from']}")
        sky = (s, int(kw["sky_from"]), bool(kw["sky_mis"])) if s else None
    if library and kw["pick_from"] is None:      # path_trace_library reads None as 1; a loop without picks never reads it
        kw["pick_from"] = 1
    ris = None
    if "ris_candidates" in own:
        ris = int(kw["ris_candidates"])
        if not 1 <= ris <= A.RIS_MAX_CANDIDATES:
            raise ValueError(f"{who}: ris_candidates must be 1 ... {A.RIS_MAX_CANDIDATES}, got {ris}")
    return kw["light_picks"], kw["pick_from"], sky, ris


def _path_trace(who, loop, library, scene, rays, light_params, bounces, seeds, occlusion, bounce_cull_mask, bounce_ray_flags, max_ray_bytes, ctx, compact, roulette_from,
                survival_floor, **given):
    """the loop of path_trace, path_trace_picked, path_trace_mis, path_trace_sky, path_trace_power, path_trace_ris and path_trace_library.
    loop: its name in _LOOPS ("mis", "sky", "power", "ris": with MIS vertices; "power", "ris": the pick vertices take direct_light_power
    or direct_light_ris and the light hits emitter_hits_power); who, given: as _loop_keywords takes them.  library chooses between the two forms of what differs: step, the
    arithmetic of a vertex (include/rtr_accum.h) in torch or by accumulate_paths, and take, the records of a compaction's survivors by
    torch indexing or by gather_records.  Everything else, and its order, is written once, here."""
    light_picks, pick_from, sky, ris = _loop_keywords(who, loop, library, given)
    mis, power = loop in _PICKS_NEEDED, loop in ("power", "ris")
    if roulette_from is not None and not compact:
        raise ValueError("path_trace: roulette_from needs compact=True (a path the roulette kills saves nothing while it keeps its lane)")
    if roulette_from is not None and int(roulette_from) < 0:
        raise ValueError(f"path_trace: roulette_from must be >= 0, got {roulette_from}")
    if light_picks is not None and int(light_params.outputs) & A.LIGHT_ANALYTIC:
        raise ValueError("path_trace_picked: light_picks cannot give the analytic sum (light_params.outputs has LIGHT_ANALYTIC): the LTC term has no per-sample form")
    if light_picks is not None and int(pick_from) < 0:
        raise ValueError(f"path_trace_picked: pick_from must be >= 0, got {pick_from}")
    torch = _torch()
    ctx = ctx or scene.ctx
    bounces = int(bounces)
    if bounces < 0:
        raise ValueError(f"path_trace: bounces must be >= 0, got {bounces}")
    if not isinstance(rays, torch.Tensor):
        raise ValueError("path_trace: rays must be a device tensor")
    n = int(rays.shape[0])
    base = seeds
    if base is None and bounces > 0:
        base = _pixel_seeds(torch, light_params, 0, n, rays.device)
    res = PathResult()
    res.per_depth = []
    res.radiance = torch.zeros((n, 3), dtype=torch.float32, device=rays.device)      # the library's step adds to it in place
    T = torch.ones((n, 3), dtype=torch.float32, device=rays.device)
    r = rays
    ids = None                           # compact: the original slot of each row, from the first compaction on
    bounce_seeds = seeds
    if compact:
        res.live = [n]
    mis_params = make_mis_params(light_picks, light_params.numAreaLights, light_params.numShadowRays) if mis else None
    prev = None                          # mis: (surfaces, bounce records) of the vertex before when it was a MIS vertex
    prev_sky = None                      # sky: the same records of the vertex before when it was a sky vertex

    # step: the vertex's term, (n, 3) with the live paths' at their ids, added to res.radiance -> (term, the throughput after bounce b or
    # None).  met, esc: the emitter and the escape records or None; lights_from, misses_from: a light hit / a miss takes their radiance,
    # 0 without them (RTR_ACCUM_LIGHTS_FROM_EMITTERS, RTR_ACCUM_MISSES_FROM_ESCAPES); sums: shade_sky's or None
    def step_torch(lit, T, ids, met, esc, lights_from, misses_from, sums, b):
        rad = lit.shadowed
        if lights_from:
            rad = torch.where((lit.kind == A.SURFACE_LIGHT).unsqueeze(1), met.radiance if met is not None else torch.zeros_like(rad), rad)
        if misses_from:
            rad = torch.where((lit.kind == A.SURFACE_MISS).unsqueeze(1), esc.radiance if esc is not None else torch.zeros_like(rad), rad)
        term = T * rad
        if sums is not None:
            term = term + T * sums
        if ids is not None:
            full = torch.zeros((n, 3), dtype=torch.float32, device=rays.device)
            full[ids.to(torch.int64)] = term
            term = full
        res.radiance = res.radiance + term
        return term, T * b.weight if b is not None else None

    def step_library(lit, T, ids, met, esc, lights_from, misses_from, sums, b):
        term = torch.zeros((n, 3), dtype=torch.float32, device=rays.device)
        ap = make_accum_params(n, lights_from_emitters=lights_from, misses_from_escapes=misses_from)
        return term, accumulate_paths(ctx, lit, T, res.radiance, ap, path_ids=ids, emitters=met, escapes=esc, sky_sums=sums, bounces=b, out_term=term)

    def take(records, rows):             # the records of the survivors; rows: compact_paths' ids, for torch as int64
        return gather_records(ctx, records, rows) if library else records[rows].contiguous()

    step = step_library if library else step_torch
    for d in range(bounces + 1):
        q = trace_rays(scene, r, ctx=ctx) if d == 0 else trace_rays(scene, r, ctx=ctx, cull_mask=bounce_cull_mask, ray_flags=bounce_ray_flags)
        sd = seeds if d == 0 else _wrap32(base.to(torch.int64) + d * PATH_SEED_STEP)
        mis_vertex = mis and int(pick_from) <= d < bounces
        if ris is not None and d >= int(pick_from):
            lit = direct_light_ris(scene, r, q, light_params, picks=light_picks, candidates=ris, pick_depth=d, seeds=sd, mis=mis_params if mis_vertex else None, ctx=ctx,
                                   max_ray_bytes=max_ray_bytes, occlusion=occlusion)
        elif power and d >= int(pick_from):
            lit = direct_light_power(scene, r, q, light_params, picks=light_picks, pick_depth=d, seeds=sd, mis=mis_params if mis_vertex else None, ctx=ctx,
                                     max_ray_bytes=max_ray_bytes, occlusion=occlusion)
        elif mis_vertex:
            w = mis_pick_weights(scene, r, q, light_params, make_pick_params(light_picks, d), mis_params, None, seeds=sd, ctx=ctx)
            lit = direct_light(scene, r, q, light_params, seeds=sd, ctx=ctx, max_ray_bytes=max_ray_bytes, occlusion=occlusion, picks=light_picks, pick_depth=d,
                               pick_weights=w)
        elif light_picks is not None and d >= int(pick_from):
            lit = direct_light(scene, r, q, light_params, seeds=sd, ctx=ctx, max_ray_bytes=max_ray_bytes, occlusion=occlusion, picks=light_picks, pick_depth=d)
        else:
            lit = direct_light(scene, r, q, light_params, seeds=sd, ctx=ctx, max_ray_bytes=max_ray_bytes, occlusion=occlusion)
        met = esc = None                 # a light hit (a miss) at d >= 1 takes these records' radiance, 0 without them
        if d >= 1 and prev is not None:
            met = (emitter_hits_power if power else emitter_hits)(scene, r, q, prev[0], prev[1], mis_params, ctx=ctx)
        if d >= 1 and prev_sky is not None and sky[2]:
            esc = sky_hits(scene, r, q, prev_sky[0], prev_sky[1], make_sky_params(sky[0], d - 1, light_params.frame, light_params.width, light_params.spp, mis=True),
                           ctx=ctx)
        misses_from = d >= 1 and prev_sky is not None
        sky_vertex = sky is not None and sky[1] <= d < bounces
        surf = hit_surfaces(scene, r, q, ctx=ctx) if d < bounces else None
        sums = b = None
        if sky_vertex:
            k = sky_rays(scene, r, surf, make_sky_params(sky[0], d, light_params.frame, light_params.width, light_params.spp, mis=sky[2]), seeds=bounce_seeds, ctx=ctx)
            sums = shade_sky(ctx, k, _occluded(scene, k.rays.reshape(-1, 8), occlusion, ctx))
        if d < bounces:
            b = bounce_rays(ctx, r, surf, make_bounce_params(frame=light_params.frame, depth=d, width=light_params.width, spp=light_params.spp), seeds=bounce_seeds)
        term, T = step(lit, T, ids, met, esc, d >= 1, misses_from, sums, b)
        res.per_depth.append(term)
        if d == bounces:
            break
        r = b.rays
        prev = (surf.raw, b.raw) if mis_vertex else None
        prev_sky = (surf.raw, b.raw) if sky_vertex else None
        if compact:
            c = compact_paths(ctx, r, T, seeds=base, path_ids=None if mis else ids,
                              params=make_compact_params(frame=light_params.frame, depth=d, roulette=roulette_from is not None and d >= int(roulette_from),
                                                         survival_floor=survival_floor))
            m = c.count
            res.live.append(m)
            if m == 0:                   # nothing goes on: every later term is zero
                for _ in range(d + 1, bounces + 1):
                    res.per_depth.append(torch.zeros((n, 3), dtype=torch.float32, device=rays.device))
                res.live += [0] * (bounces - d - 1)
                break
            r, T, base, rows = c.rays[:m], c.throughput[:m], c.seeds[:m], c.path_ids[:m]
            if mis:                      # the ids are this call's row indices: the records of the vertex and the pixel ids follow the survivors
                at = rows if library else rows.to(torch.int64)
                if prev is not None:
                    prev = (take(prev[0], at), take(prev[1], at))
                if prev_sky is not None:
                    prev_sky = prev if mis_vertex and sky_vertex else (take(prev_sky[0], at), take(prev_sky[1], at))
                if ids is not None:
                    rows = take(ids, at)
            ids = rows
            bounce_seeds = base
    return res


# ---- the same loops with the per-vertex arithmetic in the library (rtr_accumulate_paths, rtr_gather_records) ---------------------------
def path_trace_library(scene, rays, light_params, bounces, loop="power", sky_samples=LOOP_DEFAULT, sky_from=LOOP_DEFAULT, sky_mis=LOOP_DEFAULT,
                       light_picks=LOOP_DEFAULT, pick_from=LOOP_DEFAULT, seeds=None, occlusion="dense", bounce_cull_mask=None, bounce_ray_flags=0,
                       max_ray_bytes=256 << 20, ctx=None, compact=False, roulette_from=None, survival_floor=0.05):
    """path_trace ("plain"), path_trace_picked ("picked"), path_trace_mis ("mis"), path_trace_sky ("sky"), path_trace_power ("power") or
    path_trace_ris ("ris", with its default ris_candidates) with the arithmetic of a vertex done by the library: the same calls in the same order, but where those loops mask light hits and
    misses, form T * rad and T * sky, scatter the terms to their ids, add them to the sum and multiply T by the bounce's weight in
    torch, this one calls accumulate_paths once per vertex, after bounce_rays, so that it makes the next T too — with
    RTR_ACCUM_LIGHTS_FROM_EMITTERS at every vertex d >= 1 (the emitter records where the vertex before was a MIS vertex, none
    otherwise) and RTR_ACCUM_MISSES_FROM_ESCAPES where the vertex before was a sky vertex (none with sky_mis=False) — and after a
    compaction gather_records moves the records of the vertex and the pixel ids to the survivors' rows.  The operations and their
    order are those loops' (include/rtr_accum.h), so radiance, every per_depth[d] and live equal theirs bit for bit.
    The keywords after loop are path_trace_power's; LOOP_DEFAULT stands for the named loop's own default, and a keyword that loop does
    not have raises ValueError when it is given.  -> PathResult."""
    return _path_trace("path_trace_library", loop, True, scene, rays, light_params, bounces, seeds, occlusion, bounce_cull_mask, bounce_ray_flags, max_ray_bytes, ctx,
                       compact, roulette_from, survival_floor, sky_samples=sky_samples, sky_from=sky_from, sky_mis=sky_mis, light_picks=light_picks, pick_from=pick_from)
