"""The a-trous and combine kernels (csrc/kernels/rtr_post.hip) on inputs no render produces.  Rendered G-buffers are smooth and rendered
colours correlated, and every other test runs the passes with iterations = 4, so most of the kernels' decision space is entered here
only: the non-INTERIOR form everywhere (images smaller than the tap reach, than one 32 x 8 workgroup), INTERIOR workgroups at step 64,
weight_exp's underflow select, rtr_div_by with divisors 25...4096, iterations 0 and odd (which pair the combine reads — Q8 — depends
on parity), alpha bytes other than 255, u = 0 in the combine.  The inputs are the made families of tests/post_cases.py in torch tensors
bound with rtr_frame_bind_external to all eight images.

Every case asserts BOTH 0 differing pixels against the CPU oracle on the five images the chain touches AND the float64 rule of
tests/post_witness.py (|byte - unrounded value| <= 0.5 + DELTA, every byte; DELTA measured on the oracle, see there) on the last pass
and on the combine, through rtr_denoise_combine and through rtr_denoise_combine_async + rtr_frame_wait.

CPHI_ONE = false of k_denoise_pair is unreachable through the C ABI (c_phi is the constant 1 at the only call site) and is not run."""
import numpy as np
import pytest

from realtimeraytracer_amd import api

import post_cases
import post_witness as PW

pytestmark = pytest.mark.gpu

CHAIN = (1, 2, 3, 4, 5)
# (W, H): below the tap reach, below / at / just over one 32 x 8 workgroup, and a few workgroups with ragged edges
SMALL_SHAPES = ((1, 1), (1, 64), (64, 1), (3, 70), (31, 7), (32, 8), (33, 9), (97, 40))
# neither extent a multiple of 32 / 8, both above 2 * 128 + 32: workgroups at x0 = 128, 160 and y0 = 128 ... 160 are INTERIOR at step 64
LARGE = (331, 301)


class _Bound:
    """a frame whose eight images are torch tensors"""

    def __init__(self, ctx, W, H):
        import torch
        self.torch = torch
        self.frame = api.Frame(ctx, W, H, 0xff)
        self.t = [torch.zeros((H, W), dtype=torch.int32, device="cuda") for _ in range(8)]
        for k in range(8):
            self.frame.bind_external(k, self.t[k].data_ptr(), self.t[k].numel() * 4)

    def run(self, img, iterations, asynchronous):
        for k in range(8):
            self.t[k].copy_(self.torch.from_numpy(img[k].view(np.int32)))
        self.torch.cuda.synchronize()               # the passes run on the context's stream, the copies ran on torch's
        if asynchronous:
            self.frame.denoise_combine_async(iterations)
            self.frame.wait()
        else:
            self.frame.denoise_combine(iterations)
        out = {k: self.t[k].cpu().numpy().view(np.uint32) for k in range(8)}
        for k in (0, 6, 7):
            assert (out[k] == img[k]).all(), f"image {k} is an input and was written"
        return {k: out[k] for k in CHAIN}

    def close(self):
        self.frame.close()


def _check(bound, oracle, family, W, H, iterations, seed=0):
    for k in iterations:
        what = f"{family} {W}x{H} iterations {k}"
        img = post_cases.make(family, H, W, seed, stride=max(k, 1))
        got = bound.run(img, k, asynchronous=False)
        again = bound.run(img, k, asynchronous=True)
        want = post_cases.oracle_chain(oracle, img, k)
        for w in CHAIN:
            diff = int((got[w] != want[w]).sum())
            assert diff == 0, f"{what}: image {w}: {diff} of {got[w].size} pixels differ from the oracle"
            assert (again[w] == got[w]).all(), f"{what}: image {w}: rtr_denoise_combine_async differs from rtr_denoise_combine"
        # the last pass is judged on the bytes the kernels themselves left after k - 1 passes from the same inputs
        before = bound.run(img, k - 1, asynchronous=False) if k else None
        ep, ec = PW.judge(got, before, img, k)
        print(f"{what}: a-trous excess {ep if ep is None else format(ep, '.3e')}, combine excess {ec:.3e}")
        assert ep is None or ep <= PW.DELTA, f"{what}: a-trous excess {ep:.3e} byte over the float64 witness > DELTA {PW.DELTA:.1e}"
        assert ec <= PW.DELTA, f"{what}: combine excess {ec:.3e} byte over the float64 witness > DELTA {PW.DELTA:.1e}"


@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("family", post_cases.FAMILIES)
def test_small_shapes_every_family(gpu_ctx, oracle, family, shape):
    W, H = shape
    b = _Bound(gpu_ctx, W, H)
    _check(b, oracle, family, W, H, (0, 1, 2, 3, 4, 5, 8))
    b.close()


@pytest.mark.parametrize("family", ("noise", "flat_g", "lsb1", "tile"))
def test_sixty_four_iterations_on_a_shape_below_the_reach(gpu_ctx, oracle, family):
    """33 x 9 under a reach of up to 128: from step 17 on whole passes run with only the centre tap in bounds, k stays 0 and the centre
    takes kernel[0] = 1 (Q9); divisors up to 4096 in rtr_div_by"""
    b = _Bound(gpu_ctx, 33, 9)
    _check(b, oracle, family, 33, 9, (16, 17, 33, 63, 64))
    b.close()


@pytest.mark.parametrize("family", ("noise", "edge", "lsb1", "lsb255", "checker", "tile"))
def test_interior_workgroups_up_to_step_eight(gpu_ctx, oracle, family):
    W, H = LARGE
    b = _Bound(gpu_ctx, W, H)
    _check(b, oracle, family, W, H, (1, 4, 5, 8))
    b.close()


def test_interior_workgroups_at_step_sixty_four(gpu_ctx, oracle):
    """'tile' with period 64: steps 1...31 and 33...63 find no tap with the centre's G-buffer values, step 32 blends 3 x 3 and step 64 all
    25 taps of noise colours — the 64th pass has something to get wrong (63 passes over any blendable input leave it flat)"""
    W, H = LARGE
    b = _Bound(gpu_ctx, W, H)
    _check(b, oracle, "tile", W, H, (64,))
    b.close()


def test_full_hd_noise(gpu_ctx, oracle):
    b = _Bound(gpu_ctx, 1920, 1080)
    _check(b, oracle, "noise", 1920, 1080, (3,))
    b.close()
