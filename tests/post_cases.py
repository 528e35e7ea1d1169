"""Input families for the a-trous pass and the combine — TEST INFRASTRUCTURE shared by tests/test_post_witness.py (CPU: oracle against
the float64 witness) and tests/test_gpu_post_edges.py (GPU: kernels against the oracle and against the witness).

Rendered images never enter most of the passes' decision space (smooth G-buffers, correlated colours, alpha 255, u > 0), so these are
made, not rendered: eight (H, W) uint32 images keyed by rtr_image number.  0, 1, 2, 6, 7 are the chain's inputs; 3 and 4 (the denoised
pair) are pre-filled with noise so that iterations = 0 — the combine reads a pair no pass wrote — is defined; 5 is a pattern the
combine must overwrite."""
import ctypes as C
import zlib

import numpy as np

FAMILIES = ("noise", "flat_g", "edge", "zeros", "ones", "u_zero", "lsb1", "lsb255", "checker", "tile")

U = np.uint32


def _rgba(r, g, b, a):
    return (np.asarray(r, U) | (np.asarray(g, U) << U(8)) | (np.asarray(b, U) << U(16)) | (np.asarray(a, U) << U(24))).astype(U)


def make(family, H, W, seed=0, stride=1):
    """stride: the step width of the pass under test — the cell size of 'checker' (taps alternate between the two colours) and the
    period of 'tile'."""
    rng = np.random.default_rng([seed, zlib.crc32(family.encode()), H, W])
    noise = lambda: rng.integers(0, 2 ** 32, (H, W), dtype=np.uint64).astype(U)          # noqa: E731
    ys, xs = np.mgrid[0:H, 0:W]
    img = {3: noise(), 4: noise(), 5: np.full((H, W), 0xdeadbeef, U)}
    flat = np.full((H, W), 0xff808080, U)
    if family == "noise":                       # every byte of every input random, alpha included
        img.update({k: noise() for k in (0, 1, 2, 6, 7)})
    elif family == "flat_g":                    # constant G-buffers: every weight is a colour weight and all 25 taps count
        img.update({0: noise(), 1: noise(), 2: noise(), 6: flat, 7: flat.copy()})
    elif family == "edge":                      # smooth G-buffers with one hard edge, close colours
        ramp = _rgba(xs * 255 // max(W - 1, 1), ys * 255 // max(H - 1, 1), np.where(xs > W // 2, 200, 30), 255)
        base = U(0x60) + rng.integers(0, 64, (H, W)).astype(U)
        col = lambda: _rgba(*(base + rng.integers(0, 8, (H, W)).astype(U) for _ in range(3)), 255)      # noqa: E731
        img.update({0: col(), 1: col(), 2: col(), 6: ramp, 7: ramp[::-1, ::-1].copy()})
    elif family == "zeros":
        img.update({k: np.zeros((H, W), U) for k in range(8)})
    elif family == "ones":
        img.update({k: np.full((H, W), 0xffffffff, U) for k in range(8)})
    elif family == "u_zero":                    # unshadowed = 0 under shadowed > 0: the combine's max(u, 0.001) and the store's clamp
        z = np.zeros((H, W), U)
        img.update({0: noise(), 1: noise() | U(0x01010101), 2: z, 4: z.copy(), 3: noise() | U(0x01010101), 6: flat, 7: flat.copy()})
    elif family == "lsb1":                      # neighbours 1 LSB apart in the G-buffers: weights just under 1
        g = U(128) + ((xs + ys) & 1).astype(U)
        img.update({0: noise(), 1: noise(), 2: noise(), 6: _rgba(g, 128, g, 255), 7: _rgba(128, g, 128, 255)})
    elif family == "lsb255":                    # neighbours 255 apart: exp(-4 / 0.001) underflows, only taps of the own colour count
        g = U(255) * ((xs + ys) & 1).astype(U)
        img.update({0: noise(), 1: noise(), 2: noise(), 6: _rgba(g, g, g, g), 7: _rgba(g, g, g, g)})
    elif family == "checker":                   # colours alternate 0 / 255 at the tap stride over constant G-buffers
        c = U(255) * (((xs // stride) + (ys // stride)) & 1).astype(U)
        img.update({0: noise(), 1: _rgba(c, c, c, c), 2: _rgba(255 - c, c, 255 - c, 255), 6: flat, 7: flat.copy()})
    elif family == "tile":
        # noise G-buffers of period `stride` under noise colours: only taps a whole period away share the centre's G-buffer values, so
        # the passes with step = stride / 2 (3 x 3 taps) and step = stride (all 25) are the first to blend, and a chain still has
        # structure when it gets there (63 passes over anything that blends at every step leave it flat)
        t = lambda: np.tile(rng.integers(0, 2 ** 32, (stride, stride), dtype=np.uint64).astype(U),      # noqa: E731
                            (H // stride + 1, W // stride + 1))[:H, :W]
        img.update({0: noise(), 1: noise(), 2: noise(), 6: t(), 7: t()})
    else:
        raise ValueError(family)
    return {k: np.ascontiguousarray(v, dtype=U) for k, v in img.items()}


def oracle_chain(oracle, img, iterations):
    """oracle_denoise_combine on copies of the eight images, the denoised pair as given (oracle_py.denoise_combine zero-fills it).
    Returns {1, 2, 3, 4, 5: image} after the chain."""
    H, W = img[0].shape
    st = {k: img[k].copy() for k in range(8)}
    p = lambda k: C.c_void_p(st[k].ctypes.data)         # noqa: E731
    rc = oracle.lib().oracle_denoise_combine(W, H, p(0), p(1), p(2), p(6), p(7), p(3), p(4), p(5), int(iterations))
    if rc != 0:
        raise RuntimeError(f"oracle_denoise_combine failed: {rc}")
    return {k: st[k] for k in (1, 2, 3, 4, 5)}
