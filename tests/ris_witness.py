"""A numpy restatement of include/rtr_ris.h: the witness rtr_host_ris_candidates and rtr_host_ris_select are held to bit for bit.  No
test in here; test_ris_host.py imports it.

Independent of the header's code: the table search is numpy's searchsorted, the loops over hits are array operations.  The random
numbers are the contract's own (bounce_witness.rtr_random: an integer hash and an exact scaling); everything after them is float32 in
the header's order — one operation per numpy call, so nothing is contracted or reassociated — except the table target, which the
header forms in binary64 too."""
import numpy as np

import bounce_witness as BW

NONE = 0xffffffff
F32 = np.float32


def _u32(x):
    return (np.asarray(x).astype(np.uint64) & 0xffffffff).astype(np.uint64)


def base_frame(seeds, n, frame, width, spp):
    """seed base + frame of every hit, as 32-bit words held in uint64"""
    b = BW.pixel_seeds(n, width, spp) if seeds is None else np.asarray(seeds).view(np.uint32)
    return _u32(b.astype(np.uint64) + frame)


def _s0(bf, depth):
    return bf + 7919 * (depth + 1)


def _ris_seed(bf, depth, p, j):
    return _s0(bf, depth) + 5000 + 48 * p + 3 * j


def candidates(cdf, tris, bf, depth, ns, P, M):
    """-> uint32 (n, P, M)"""
    n = len(bf)
    out = np.full((n, P, M), NONE, np.uint32)
    cdf = np.asarray(cdf, np.uint64)[:tris]
    total = int(cdf[-1]) if tris else 0
    if total == 0 or ns == 0:
        return out
    for p in range(P):
        for j in range(M):
            seed_t = _s0(bf, depth) + 400 + 100 * p if j == 0 else _ris_seed(bf, depth, p, j)
            seed_s = seed_t + (50 if j == 0 else 1)
            u = BW.rtr_random(_u32(seed_t))
            target = np.minimum(np.floor(u.astype(np.float64) * np.float64(total)).astype(np.uint64), np.uint64(total - 1))
            t = np.searchsorted(cdf, target, side="right").astype(np.uint64)      # the first t with cdf[t] > target
            s = np.minimum((BW.rtr_random(_u32(seed_s)) * F32(ns)).astype(np.uint32), np.uint32(ns - 1)).astype(np.uint64)
            out[:, p, j] = (t * ns + s).astype(np.uint32)
    return out


def select(cdf, tris, bf, depth, ns, P, M, cand, targets, w_pick=None):
    """-> (slots uint32 (n, P), weights float32 (n, P))"""
    n = len(bf)
    cdf = np.asarray(cdf, np.uint64)[:tris]
    weight = np.diff(np.concatenate([[np.uint64(0)], cdf])).astype(np.uint32) if tris else np.zeros(0, np.uint32)
    total = int(cdf[-1]) if tris else 0
    cand = np.asarray(cand).view(np.uint32).reshape(n, P, M)
    targets = np.asarray(targets, F32).reshape(n, P, M)
    slots, weights = np.full((n, P), NONE, np.uint32), np.zeros((n, P), F32)
    if total == 0:
        return slots, weights
    total_f = F32(np.uint64(total))
    with np.errstate(all="ignore"):
        for p in range(P):
            W = np.zeros(n, F32)
            held = np.full(n, NONE, np.uint32)
            held_phat, held_wp = np.zeros(n, F32), np.zeros(n, F32)
            for j in range(M):
                c = cand[:, p, j]
                ok = c.astype(np.uint64) < np.uint64(tris * ns)
                wt = weight[np.where(ok, c // np.uint32(ns), 0)]
                tg = targets[:, p, j]
                tg = np.where((tg > 0) & np.isfinite(tg), tg, F32(0))
                wp = np.zeros(n, F32)
                if w_pick is not None:
                    wp = np.asarray(w_pick, F32).reshape(n, P, M)[:, p, j]
                    ok &= (wp > 0) & np.isfinite(wp)
                ok &= (wt != 0) & (tg > 0)
                rj = tg * (total_f / (F32(1) * np.where(ok, wt, 1).astype(F32)))
                ok &= (rj > 0) & np.isfinite(rj)
                W = np.where(ok, W + rj, W).astype(F32)
                u = BW.rtr_random(_u32(_ris_seed(bf, depth, p, j) + 2))
                take = ok & ((held == NONE) | (u * W < rj))
                held, held_phat, held_wp = np.where(take, c, held), np.where(take, tg, held_phat).astype(F32), np.where(take, wp, held_wp).astype(F32)
            w = (W / held_phat) / F32(M * P)
            if w_pick is not None:
                w = w * held_wp
            good = (held != NONE) & np.isfinite(w)
            slots[:, p] = np.where(good, held, NONE)
            weights[:, p] = np.where(good, w, F32(0))
    return slots, weights
