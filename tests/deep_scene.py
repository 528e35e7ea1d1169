"""The deep scene of the ray-query tests: a tree deep enough that camera rays overflow the walk's short stack and take the tail kernel."""
import ctypes as C

import numpy as np

from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api, host


def _deep_scene(ctx):
    """the squeezed row of tests/test_gpu_parity.py (2^19 triangles 0.01 apart) whose camera rays, looking down its length from its
    head, keep one pending far child per level of the ~20-level tree"""
    N = 1 << 19
    x = np.arange(N, dtype=np.float32) * np.float32(0.01)
    tri = np.stack([np.stack([x, np.full(N, -1.0, np.float32), np.full(N, -0.3, np.float32)], 1),
                    np.stack([x + np.float32(0.006), np.full(N, -1.0, np.float32), np.zeros(N, np.float32)], 1),
                    np.stack([x, np.full(N, -1.0, np.float32), np.full(N, 0.3, np.float32)], 1)], 1).reshape(-1, 3)
    wall = np.array([[N * 0.01 + 1.0, -4.0, -4.0], [N * 0.01 + 1.0, 4.0, -4.0], [N * 0.01 + 1.0, 0.0, 4.0]], np.float32)
    verts = np.concatenate([wall, tri])
    V = np.zeros((len(verts), 12), np.float32)
    V[:, :3] = verts
    idx = np.concatenate([np.array([0, 1, 2], np.uint32), np.arange(3 * N, dtype=np.uint32)])
    meshes = (A.RtrMesh * 2)()
    for m, (vo, io, vc, ic) in zip(meshes, [(0, 0, 3, 3), (3, 3, 3 * N, 3 * N)]):
        m.vertexOffset, m.indexOffset, m.vertexCount, m.indexCount, m.isOpaque = vo, io, vc, ic, 1
    inst = (A.RtrInstance * 2)()
    for i, (mi, ci) in zip(inst, [(0, 0), (1, 1)]):
        i.meshIndex, i.customIndex = mi, ci
        for k, val in enumerate((1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)):
            i.transform[k] = float(val)
    objs = (A.RtrObjectInfo * 2)()
    for o, (vo, io) in zip(objs, [(0, 0), (3, 3)]):
        o.vertexOffset, o.indexOffset = vo, io
        o.color[0] = o.color[1] = o.color[2] = 0.8
    d = A.rtr_scene_desc()
    d.vertices = V.ctypes.data_as(C.POINTER(A.RtrVertex)); d.numVertices = len(V)
    d.indices = idx.ctypes.data_as(C.POINTER(A.u32)); d.numIndices = len(idx)
    d.meshes, d.numMeshes = meshes, 2
    d.instances, d.numInstances = inst, 2
    d.objects, d.numObjects = objs, 2
    d.skyColor[0] = d.skyColor[1] = d.skyColor[2] = 0.5
    keep = (V, idx, meshes, inst, objs)
    scene = api.Scene(ctx, d)
    assert scene.stats().maxDepth > 16
    end = float(N) * 0.01
    cam = host.Camera(0.004, (-30.0, -0.995, 0.0), (0.8 * end, -1.0, 0.0), (0.0, 1.0, 0.0), 16, 8).getGPUData()
    return d, keep, scene, cam
