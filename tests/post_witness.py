"""An independent witness of the passes behind the ray-gen dispatch — TEST INFRASTRUCTURE.

The a-trous pass and the combine are held bit-exact between the HIP kernels (csrc/kernels/rtr_post.hip) and the CPU oracle, and those
two share one header, one author and one expression order.  This module restates both passes a second time with nothing in common:
numpy, float64, np.exp, a plain `/`, written from the shader text alone (reference src/shaders/denoise.comp:36-116,
src/shaders/combine.comp:20-37) and, for protocol(), from the host loop that dispatches them (src/app/application.cppm:391-445).

Values are returned UNROUNDED, in byte units: clip(v, 0, 1) * 255 with no rint, because what an rgba8 imageStore leaves is the
nearest byte and fp32 against fp64 cannot agree on which one that is when the value sits next to k + 1/2 (the combine puts 0.3 % of its
bytes on exact ties: a * s / u = 255 * 1 / 2).  The rule a byte b is judged by has no share cap:

    accepted  iff  |b - raw| <= 0.5 + DELTA

So that one rounding flip does not travel into the next pass, each pass is judged on the bytes the implementation under test itself
left for the previous one (judge()).

DELTA.  The bound is measured against the reference side, never against the kernels: the largest excess |b - raw| - 0.5 of the CPU
oracle over every input family of tests/post_cases.py, two seeds each, shapes 1 x 1 to 70 x 131, every step 1...64, was

    4.34e-5 byte in an a-trous pass    (family 'edge', 70 x 131, step 3; every other family between 0.7e-5 and 3.0e-5, 'tile' 1.7e-5)
    8.5e-14 byte in the combine

measured by `python tests/test_post_witness.py` (it prints one line per family and the maxima).  DELTA is 4 x the larger figure:
fp32-against-fp64 noise of a 25-term weighted mean; the margin covers families, seeds and shapes that were not sampled.

Constants are the fp32 values the shader is handed: n_phi = p_phi = 0.001f and c_phi = 1.0f are push constants written as C++ float
literals (application.cppm:406), max(cum_weight, 1e-5) and max(u, vec3(0.001)) are GLSL float literals.  Everything computed from them
is float64.
"""
import numpy as np

F = np.float64

DELTA = 1.8e-4                      # 4 x 4.34e-5 rounded up, see above

C_PHI = F(np.float32(1.0))          # DenoisingInfo(step, 1.0f, 0.001f, 0.001f, flag, 0), application.cppm:406
N_PHI = F(np.float32(0.001))
P_PHI = F(np.float32(0.001))
CUM_FLOOR = F(np.float32(1e-5))     # denoise.comp:100
U_FLOOR = F(np.float32(0.001))      # combine.comp:31

# denoise.comp:28-34
KERNEL = np.array([1, 4, 7, 4, 1,
                   4, 16, 26, 16, 4,
                   7, 26, 41, 26, 7,
                   4, 16, 26, 16, 4,
                   1, 4, 7, 4, 1], F)

SAMPLED, DENOISED = "sampled", "denoised"       # the ping-pong pairs: images (1, 2) and images (3, 4)


def image_bytes(img):
    """(H, W) uint32 -> (H, W, 4) float64 byte values, channel order as imageLoad returns them (x = bits 0-7)."""
    img = np.asarray(img).view(np.uint32)
    return np.stack([(img >> np.uint32(s)) & np.uint32(255) for s in (0, 8, 16, 24)], -1).astype(F)


def load(img):
    """imageLoad on rgba8: UNORM8 -> [0, 1]"""
    return image_bytes(img) / 255.0


def store_raw(v):
    """imageStore on rgba8 up to, and without, the rounding: byte units"""
    return np.clip(v, 0.0, 1.0) * 255.0


def denoise_pass(inp, normal, position, step, q9=True, normal_by_step2=True):
    """denoise.comp:55-100 for one image at one step width.  inp, normal, position: (H, W) uint32.  Returns (H, W, 4) unrounded.
    q9 / normal_by_step2 = False are MUTATIONS for the tests that show each quirk observable: the weight indexed by the tap's number
    instead of by the count of in-bounds taps so far (:72-73 `continue` skips :96 `++k`), and the normal distance left undivided (:84)."""
    H, W = inp.shape
    c, n, p = load(inp), load(normal), load(position)
    ys, xs = np.mgrid[0:H, 0:W]
    k = np.zeros((H, W), np.int64)
    cum = np.zeros((H, W), F)
    acc = np.zeros((H, W, 4), F)
    tap = 0
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            ox, oy = xs + dx * step, ys + dy * step
            inside = (ox >= 0) & (oy >= 0) & (ox < W) & (oy < H)
            if inside.any():
                oxc, oyc = np.clip(ox, 0, W - 1), np.clip(oy, 0, H - 1)     # out-of-bounds taps get weight 0 below
                ct, nt, pt = c[oyc, oxc], n[oyc, oxc], p[oyc, oxc]
                d = ((c - ct) ** 2).sum(-1)
                cw = np.minimum(np.exp(-d / C_PHI), 1.0)
                d = ((n - nt) ** 2).sum(-1)
                if normal_by_step2:
                    d = np.maximum(d / (step * step), 0.0)
                nw = np.minimum(np.exp(-d / N_PHI), 1.0)
                d = ((p - pt) ** 2).sum(-1)                                     # POSITION_SCALE = 1 (:6, :88)
                pw = np.minimum(np.exp(-d / P_PHI), 1.0)
                kw = KERNEL[k] if q9 else KERNEL[tap]
                w = np.where(inside, cw * nw * pw * kw, 0.0)
                cum += w
                acc += ct * w[..., None]
                k += inside
            tap += 1
    return store_raw(acc / np.maximum(cum, CUM_FLOOR)[..., None])


def combine(analytic, sh, un):
    """combine.comp:24-37.  Returns (H, W, 4) unrounded; alpha is the stored constant 1."""
    a, s, u = load(analytic), load(sh), load(un)
    f = a * (s / np.maximum(u, U_FLOOR))
    f[..., 3] = 1.0
    return store_raw(f)


def protocol(iterations, combine_reads_last_written=False):
    """The host loop of application.cppm:391-445: ([(step, pair read, pair written) per pass], pair the combine reads).
    The flag starts at 1 (:392); a pass with flag 1 reads the sampled pair and writes the denoised one, with flag 0 the reverse
    (denoise.comp:36-50, 102-115); the flag flips after every pass (:433) and is then handed to the combine (:444), which reads
    the sampled pair for 0 and the denoised pair for 1 (combine.comp:24-29) — the pair the last pass did NOT write (Q8).
    combine_reads_last_written = True is a MUTATION."""
    flag = 1
    passes = []
    for i in range(iterations):
        passes.append((i + 1, SAMPLED, DENOISED) if flag == 1 else (i + 1, DENOISED, SAMPLED))       # step = (i + 1) * DENOISING_STRENGTH
        flag = 1 - flag
    reads = SAMPLED if flag == 0 else DENOISED
    if combine_reads_last_written and passes:
        reads = passes[-1][2]
    return passes, reads


def excess(img, raw):
    """|b - raw| - 0.5 per byte: <= DELTA for an accepted byte"""
    return np.abs(image_bytes(img) - raw) - 0.5


PAIR = {SAMPLED: (1, 2), DENOISED: (3, 4)}      # rtr_image numbers: (shadowed, unshadowed), (denoised shadowed, denoised unshadowed)


def judge(state, before, images, iterations, **mutation):
    """Largest excess of the last a-trous pass and of the combine of a chain of `iterations` passes.
    state: {1, 2, 3, 4, 5: (H, W) uint32} left by the implementation under test after `iterations` passes and the combine;
    before: the same after iterations - 1 passes from the same inputs (None for iterations = 0);
    images: {0, 6, 7: ...} analytic, normal, position.
    The last pass is restated from the pair `before` holds as that pass's input; the combine from the pair `state` holds.
    Returns (pass excess or None, combine excess)."""
    pw = {k: mutation.pop(k) for k in ("q9", "normal_by_step2") if k in mutation}
    passes, reads = protocol(iterations, **mutation)
    worst_pass = None
    if passes:
        step, src, dst = passes[-1]
        worst_pass = max(float(excess(state[o], denoise_pass(before[i], images[6], images[7], step, **pw)).max())
                         for i, o in zip(PAIR[src], PAIR[dst]))
    sh, un = PAIR[reads]
    return worst_pass, float(excess(state[5], combine(images[0], state[sh], state[un])).max())
