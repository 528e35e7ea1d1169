"""An independent numpy statement of rtr_compact_paths (include/rtr.h): which paths of a wavefront go on, with what throughput, and where
they land.  Written from the interface's words, not from include/rtr_paths.h: whole-array float32 arithmetic and a uint32 PCG of its
own; the host function is held to it word for word (tests/test_compact_host.py) and the kernels to the host function."""
import numpy as np

ROULETTE = 1
PATH_NONE = 0xffffffff
F32 = np.float32
PATTERNS = ("all_live", "all_dead", "first_only", "last_only", "alternating", "dead_block", "random_half", "random_sparse")
SIZES = (1, 63, 64, 65, 255, 256, 257, 20000)


def _pcg(seed):
    with np.errstate(over="ignore"):
        state = seed.astype(np.uint32) * np.uint32(747796405) + np.uint32(2891336453)
        word = ((state >> ((state >> np.uint32(28)) + np.uint32(4))) ^ state) * np.uint32(277803737)
    return (word >> np.uint32(22)) ^ word


def uniform(seed):
    """float(hash) / 2^32 in float32: one rounding in the conversion, then an exact scaling.  May be exactly 1.0."""
    return _pcg(seed).astype(F32) * F32(2.0 ** -32)


def roulette_seed(seed, frame, depth):
    """the 32-bit word the roulette's number is drawn from"""
    return ((seed.astype(np.uint64) + np.uint64(frame) + np.uint64(7919) * np.uint64(depth + 1) + np.uint64(300)) & np.uint64(0xffffffff)).astype(np.uint32)


def live(rays, T):
    """the ray would cost a walk, and the throughput is finite, nowhere negative and somewhere positive"""
    r = rays.view(F32)
    o, tmin, d, tmax = r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7]
    with np.errstate(invalid="ignore"):
        walks = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0).any(1) & (tmax > tmin)
        carries = np.isfinite(T).all(1) & (T >= 0).all(1) & (T.max(axis=1) > 0)
    return walks & carries


def compact(rays, throughput, seeds=None, path_ids=None, frame=0, depth=0, flags=0, survival_floor=0.05):
    """-> (out_rays (N, 8) uint32, out_T (N, 3) uint32, out_seeds (N,) uint32 or None, out_ids (N,) uint32, count).  throughput: (N, 3)
    float32, or (N, 8) records whose first three columns are used."""
    n = rays.shape[0]
    T = np.ascontiguousarray(throughput.view(F32)[:, 0:3])
    keep = live(rays, T)
    out_T = T.copy()
    if flags & ROULETTE:
        with np.errstate(invalid="ignore"):
            p = np.maximum(np.where(keep, T.max(axis=1), F32(1)), F32(survival_floor)).astype(F32)
        draws = keep & (p < 1)
        u = uniform(roulette_seed(seeds.view(np.uint32), frame, depth))
        keep = keep & (~draws | (u < p))
        with np.errstate(invalid="ignore", divide="ignore"):
            out_T = np.where(draws[:, None], (T / p[:, None]).astype(F32), T)
    order = np.flatnonzero(keep)                                   # ascending: the stable order
    count = len(order)
    o_rays = np.zeros((n, 8), np.uint32)
    o_T = np.zeros((n, 3), np.uint32)
    o_ids = np.full(n, PATH_NONE, np.uint32)
    o_rays[:count] = rays.view(np.uint32)[order]
    o_T[:count] = out_T.view(np.uint32)[order]
    o_ids[:count] = order.astype(np.uint32) if path_ids is None else path_ids.view(np.uint32)[order]
    o_seeds = None
    if seeds is not None:
        o_seeds = np.zeros(n, np.uint32)
        o_seeds[:count] = seeds.view(np.uint32)[order]
    return o_rays, o_T, o_seeds, o_ids, count


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def live_mask(pattern, n, seed=7):
    rng = np.random.default_rng(seed + n)
    m = {"all_live": np.ones(n, bool), "all_dead": np.zeros(n, bool), "first_only": np.arange(n) == 0, "last_only": np.arange(n) == n - 1,
         "alternating": np.arange(n) % 2 == 0, "dead_block": (np.arange(n) // 256) != 1,
         "random_half": rng.random(n) < 0.5, "random_sparse": rng.random(n) < 0.05}[pattern]
    return m


def dead_causes():
    """(name, ray (8,) float32, T (3,) float32): one dead path per cause"""
    nan, inf = F32(np.nan), F32(np.inf)
    ok_ray = np.array([1, 2, 3, 0.001, 0, 0.6, 0.8, 10000], F32)
    ok_T = np.array([0.5, 0.25, 0.125], F32)

    def ray(**kw):
        r = ok_ray.copy()
        for k, v in kw.items():
            r[int(k[1:])] = v
        return r
    return [("null ray", np.zeros(8, F32), ok_T), ("tmax == tmin", ray(_3=5.0, _7=5.0), ok_T), ("tmax < tmin", ray(_3=6.0, _7=5.0), ok_T),
            ("NaN origin", ray(_1=nan), ok_T), ("infinite origin", ray(_0=-inf), ok_T), ("infinite direction", ray(_5=inf), ok_T),
            ("NaN direction", ray(_6=nan), ok_T), ("zero direction", ray(_4=0.0, _5=0.0, _6=-0.0), ok_T), ("NaN tmax", ray(_7=nan), ok_T),
            ("NaN tmin", ray(_3=nan), ok_T),
            ("T with a NaN", ok_ray, np.array([0.5, nan, 0.1], F32)), ("T with an infinity", ok_ray, np.array([inf, 0.5, 0.1], F32)),
            ("T with a negative channel", ok_ray, np.array([0.5, 0.5, -1e-30], F32)), ("T all zero", ok_ray, np.zeros(3, F32)),
            ("T all minus zero", ok_ray, np.array([-0.0, -0.0, -0.0], F32))]


def live_oddities():
    """(name, ray, T): live paths that look like dead ones"""
    ok_ray = np.array([1, 2, 3, 0.001, 0, 0.6, 0.8, 10000], F32)
    return [("T = (-0, 0, 1)", ok_ray, np.array([-0.0, 0.0, 1.0], F32)), ("a denormal T", ok_ray, np.array([0, 1e-42, 0], F32)),
            ("one direction word", np.array([0, 0, 0, 0, 0, 0, 1e-30, 1e-30], F32), np.array([2.0, 0.0, 3.0], F32)),
            ("infinite tmax", np.array([0, 0, 0, 0, 1, 0, 0, np.inf], F32), np.array([1.0, 1.0, 1.0], F32)),
            ("negative tmin", np.array([0, 0, 0, -1, 1, 0, 0, 0], F32), np.array([0.3, 0.0, 0.0], F32))]


def make_paths(n, pattern, seed=7, t_hi=1.0, stride_words=3, edge_cases=True):
    """n paths whose liveness follows the pattern: (rays (n, 8) float32, throughput (n, stride_words) float32, seeds (n,) uint32, ids (n,)
    uint32, expected live mask).  Dead paths cycle through dead_causes(); with edge_cases some live ones are live_oddities().  The words of
    a wide throughput row beyond the third are garbage the call must not read as throughput.  t_hi: live throughputs are in (0, t_hi)."""
    rng = np.random.default_rng(seed * 1000003 + n)
    mask = live_mask(pattern, n, seed)
    rays = np.empty((n, 8), F32)
    rays[:, 0:3] = rng.uniform(-10, 10, (n, 3))
    rays[:, 3] = 0.001
    d = rng.normal(size=(n, 3))
    rays[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 7] = 10000.0
    thr = rng.uniform(-5, 5, (n, stride_words)).astype(F32)
    thr[:, 0:3] = (rng.uniform(0.001, 1.0, (n, 3)) * t_hi).astype(F32)
    causes, odd = dead_causes(), live_oddities()
    dead = np.flatnonzero(~mask)
    which = np.arange(len(dead)) % len(causes)
    rays[dead] = np.stack([c[1] for c in causes])[which]
    thr[dead, 0:3] = np.stack([c[2] for c in causes])[which]
    if edge_cases:
        alive = np.flatnonzero(mask)[::7][:len(odd) * 3]
        which = np.arange(len(alive)) % len(odd)
        rays[alive] = np.stack([c[1] for c in odd])[which]
        thr[alive, 0:3] = np.stack([c[2] for c in odd])[which]
    seeds = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    ids = rng.permutation(n).astype(np.uint32) + np.uint32(1000)
    return rays, thr, seeds, ids, mask
