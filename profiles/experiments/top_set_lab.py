#!/usr/bin/env python3
"""CPU-only pricing of WHICH 4-wide records k_shadow_trace4 keeps in LDS (its first kTopNodes records).

The oracle walks the reduced bench frame's shadow rays over the tree of api.host_build_bvh_wide with a walk profile
(oracle_py.render(..., walk_profile=...): entries per (record, slot)); the visits of an inner record are the entries of the slot that
leads to it, the root's are the rest of the frame's record visits.  For views 0 / 48 / 95 of the bench's camera path the script prints
the share of all record visits that fall on three resident sets of rtr_trace_top_nodes() records:

    breadth-first   the first records of the exported order (what the device held before the best-first top)
    most visited    the records with the most visits in that view: the ceiling for any set of this size
    library         the first records of the library's resident order (api.host_wide_resident: kernels/rtr_hot_top.h)

and, for reference, the most visited set of view 0 used on the other views.

    python profiles/experiments/top_set_lab.py [W H]            # default 480 270; output committed as profiles/hot_top/top_set_lab.log
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from realtimeraytracer_amd import _abi as A, api, scenes  # noqa: E402
from oracle import oracle_py as O  # noqa: E402

VIEWS = (0, 48, 95)
PATH_PERIOD = 192      # bench.py's


def child_codes(wide):
    return np.frombuffer(bytes(wide), dtype=np.int32).reshape(-1, 16)[:, 12:16]


def resident_positions(bfs, res):
    """pos[i]: where record i of the breadth-first view sits in the resident one (the two are one tree: walked together from the root)"""
    a, b = child_codes(bfs), child_codes(res)
    pos = np.full(len(a), -1, np.int64)
    pos[0] = 0
    for i in range(len(a)):                      # breadth-first order: a record's position is known before its children are looked at
        for k in range(4):
            if a[i, k] >= 0:
                pos[a[i, k]] = b[pos[i], k]
    assert sorted(pos.tolist()) == list(range(len(a)))
    return pos


def record_visits(s, bvh, p, cam, info):
    prof = np.zeros((len(bvh.wide), 4, 3), dtype=np.uint64)
    r = O.render(s.desc, cam, info, p, bvh=bvh, threads=16, walk_profile=prof)
    codes = child_codes(bvh.wide)
    visits = np.zeros(len(codes), np.float64)
    inner = codes >= 0
    visits[codes[inner]] = prof[:, :, 0][inner].astype(np.float64)
    total = float(r.stats.numShadowNodeVisits)
    visits[0] = total - visits.sum()             # the walks that start at the root (and the few BVH2 visits of the tail rays)
    return visits, total, r.stats.numShadowRays


def main():
    W = int(sys.argv[1]) if len(sys.argv) > 1 else 480
    H = int(sys.argv[2]) if len(sys.argv) > 2 else 270
    top = api.trace_top_nodes()
    print(f"resident set: {top} records (rtr_trace_top_nodes), kernel revision {A.hip_lib().rtr_kernel_revision().decode()}, {W}x{H}, 1 spp, 3 shadow rays")
    worst = None
    for name in ("sponza_class", "sponza_mixed", "bunny_class"):
        s = getattr(scenes, name)(W, H)
        p = api.make_params(W, H, spp=1, shadow_rays=3, collect_stats=1)
        bvh = api.host_build_bvh_wide(s.desc)
        lights = [s.desc.lights[i] for i in range(s.desc.numLights)]
        res = api.host_wide_resident(bvh.wide, bvh[2], lights, top)
        pos = resident_positions(bvh.wide, res)
        lib = pos < top
        bfs = np.arange(len(pos)) < top
        path = s.camera_path(PATH_PERIOD) if (s.cam_args and s.walk_scale > 0) else None
        print(f"\n{name}: {len(pos)} wide records, {s.desc.numLights} area lights, {'camera path' if path else 'static camera (every view the same)'}")
        print(f"{'view':>5s} {'visits/ray':>10s} | {'breadth-first':>13s} {'most visited':>12s} {'library':>8s} {'most visited of view 0':>22s} | library - breadth-first")
        first = None
        for v in VIEWS:
            cam, info = (path[v][0], s.scene_info(v, cam_pos=path[v][1])) if path else (s.camera, s.scene_info(v))
            visits, total, rays = record_visits(s, bvh, p, cam, info)
            hot = np.zeros(len(pos), bool)
            hot[np.argsort(-visits, kind="stable")[:top]] = True
            if first is None:
                first = hot
            share = lambda m: 100.0 * visits[m].sum() / total
            d = share(lib) - share(bfs)
            worst = d if worst is None else min(worst, d)
            print(f"{v:5d} {total / max(rays, 1):10.3f} | {share(bfs):12.1f}% {share(hot):11.1f}% {share(lib):7.1f}% {share(first):21.1f}% | {d:+.1f} points", flush=True)
    print(f"\nsmallest (library - breadth-first) over all scenes and views: {worst:+.1f} points")


if __name__ == "__main__":
    main()
