"""The presented frame (five ray-gen images, a-trous rounds, combine: reference application.cppm:391-445) asynchronously and from the
multi-GPU path: rtr_denoise_combine_async against rtr_denoise_combine and the oracle, rtr_deinterleave_images against the numpy
restatement and against rtr_deinterleave_bands, and librtr_mgpu.so's present mode (RTR_MGPU_PRESENT) through real RCCL and through
the same-device RCCL double with 2, 3 and 8 ranks.  Every image comparison is 0 pixels differing."""
import os
import textwrap

import numpy as np
import pytest

from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api, mgpu, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL8 = 0xff

pytestmark = [pytest.mark.gpu]


def _assert_same(got, want, what):
    diff = int((got != want).sum())
    if diff:
        ys, xs = np.nonzero(got != want)
        first = [(int(y), int(x), hex(int(got[y, x])), hex(int(want[y, x]))) for y, x in list(zip(ys, xs))[:5]]
        raise AssertionError(f"{what}: {diff} of {got.size} pixels differ; first (y,x,got,want): {first}")


def _all8(frame):
    return {w: frame.download(w) for w in range(8)}


def _presented(scene, setup, p, frame, frame_no, iterations=4):
    """the reference's frame loop, synchronously: render, then rtr_denoise_combine; all 8 images"""
    api.render(scene, setup.camera, setup.scene_info(frame_no), p, frame)
    frame.denoise_combine(iterations)
    return _all8(frame)


@pytest.mark.parametrize("size", [(1920, 1080), (333, 187)])
def test_denoise_combine_async_equals_the_synchronous_passes_and_the_oracle(gpu_ctx, oracle, scene_cache, size):
    W, H = size
    s = scenes.cornell_box(W, H, ltc=scenes.synthetic_ltc())
    scene = api.Scene(gpu_ctx, s.desc)
    p = api.make_params(W, H, spp=2, images=A.IMAGES_RAYGEN5)
    sync = api.Frame(gpu_ctx, W, H, ALL8)
    api.render(scene, s.camera, s.scene_info(3), p, sync)
    src = {k: sync.download(k) for k in (0, 1, 2, 6, 7)}
    sync.denoise_combine(4)
    want = _all8(sync)
    ref = oracle.denoise_combine(src[0], src[1], src[2], src[6], src[7], iterations=4)
    for w in (1, 2, 3, 4, 5):
        _assert_same(want[w], ref[w], f"rtr_denoise_combine vs oracle, image {w}")
    # render_async -> denoise_combine_async -> wait, no host join in between, on a context of its own
    ctx = api.Context(0)
    f = api.Frame(ctx, W, H, ALL8)
    api.render(scene, s.camera, s.scene_info(3), p, f, asynchronous=True)
    f.denoise_combine_async(4)
    f.wait()
    got = _all8(f)
    for w in range(8):
        _assert_same(got[w], want[w], f"async vs sync, image {w} at {W}x{H}")
    with pytest.raises(api.RtrError):
        api.Frame(ctx, W, H, A.IMAGES_RAYGEN5).denoise_combine_async(4)         # lacks images 3-5
    with pytest.raises(api.RtrError):
        f.denoise_combine_async(65)
    for o in (f, sync, scene, ctx):
        o.close()


def test_two_frames_in_flight_on_two_contexts(gpu_ctx, scene_cache):
    """Two contexts alternate render_async + denoise_combine_async against one scene, joined only one frame behind: every presented
    frame equals the synchronous one."""
    W, H = 480, 270
    s = scenes.sponza_class(W, H, ltc=scenes.shipped_ltc())
    scene = api.Scene(gpu_ctx, s.desc)
    p = api.make_params(W, H, spp=1, images=A.IMAGES_RAYGEN5, pipeline=2)
    one = api.Frame(gpu_ctx, W, H, ALL8)
    want = {f: _presented(scene, s, p, one, f) for f in range(6)}
    ctxs = [api.Context(0), api.Context(0)]
    frames = [api.Frame(c, W, H, ALL8) for c in ctxs]
    got = {}
    for f in range(6):
        fr = frames[f % 2]
        api.render(scene, s.camera, s.scene_info(f), p, fr, asynchronous=True)
        fr.denoise_combine_async(4)
        if f >= 1:                                  # join the frame one behind, while this one is in flight
            prev = frames[(f - 1) % 2]
            prev.wait()
            got[f - 1] = _all8(prev)
    frames[1].wait()
    got[5] = _all8(frames[1])
    for f in range(6):
        for w in range(8):
            _assert_same(got[f][w], want[f][w], f"frame {f}, image {w}")
    for o in frames + ctxs + [one, scene]:
        o.close()


def test_denoise_combine_async_after_a_batch_on_a_following_frame(gpu_ctx, scene_cache):
    """rtr_denoise_combine_async on frames that FOLLOWED in an rtr_render_batch_async launch (it ran on the leader's stream) comes behind
    that launch, and the next launch comes behind it — no host join in between."""
    W, H = 480, 270
    s = scenes.sponza_class(W, H, ltc=scenes.shipped_ltc())
    scene = api.Scene(gpu_ctx, s.desc)
    p = api.make_params(W, H, spp=1, images=A.IMAGES_RAYGEN5, pipeline=2)
    one = api.Frame(gpu_ctx, W, H, ALL8)
    want = {f: _presented(scene, s, p, one, f)[A.IMAGE_FINAL] for f in range(40, 46)}
    ctxs = [api.Context(0) for _ in range(3)]
    frames = [api.Frame(c, W, H, ALL8) for c in ctxs]
    api.render_batch(scene, [s.camera] * 3, [s.scene_info(40 + b) for b in range(3)], p, frames)
    frames[2].denoise_combine_async(4)
    frames[1].denoise_combine_async(4)
    # the second launch overwrites the sampled images of frames 1 and 2: it must wait for their post passes
    api.render_batch(scene, [s.camera] * 3, [s.scene_info(43 + b) for b in range(3)], p, frames)
    frames[2].denoise_combine_async(4)
    frames[1].denoise_combine_async(4)
    frames[0].denoise_combine_async(4)
    for b in range(3):
        frames[b].wait()
        _assert_same(frames[b].download(A.IMAGE_FINAL), want[43 + b], f"frame {b} of the second launch")
    for o in frames + ctxs + [one, scene]:
        o.close()


def _gathered(n, planes, W, H, band, rng):
    """a random [shard][plane][local row][x] gather buffer (padding rows random too: they must never be read)"""
    rows = api.shard_rows(H, band, n)
    return rng.integers(0, 2 ** 32, size=(n, planes, rows, W), dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("n", [1, 2, 3, 8, 16])
@pytest.mark.parametrize("W,H,band", [(128, 64, 8), (97, 52, 8), (333, 187, 16)])
@pytest.mark.parametrize("planes", [1, 5, 8])
def test_deinterleave_images_matches_numpy_and_the_one_image_kernel(gpu_ctx, n, W, H, band, planes):
    import torch
    rng = np.random.default_rng(n * 1000 + W + planes)
    g = _gathered(n, planes, W, H, band, rng)
    dev = torch.from_numpy(g.view(np.int32)).cuda()
    outs = [torch.zeros((H, W), dtype=torch.int32, device="cuda") for _ in range(planes)]
    torch.cuda.synchronize()                      # the library's kernels run on the context's stream, not torch's
    api.deinterleave_images(gpu_ctx, dev.data_ptr(), [o.data_ptr() for o in outs], W, H, band, n)
    torch.cuda.synchronize()
    one = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    for k in range(planes):
        want = mgpu.assemble_numpy(np.ascontiguousarray(g[:, k]), H, band)
        got = outs[k].cpu().numpy().view(np.uint32)
        _assert_same(got, want, f"plane {k} of {planes}, N = {n}, {W}x{H}")
        plane = dev[:, k].contiguous()
        torch.cuda.synchronize()
        api.deinterleave_bands(gpu_ctx, plane.data_ptr(), one.data_ptr(), W, H, band, n)
        torch.cuda.synchronize()
        _assert_same(one.cpu().numpy().view(np.uint32), got, f"rtr_deinterleave_bands vs rtr_deinterleave_images, plane {k}")


def test_deinterleave_images_unaligned_destination_and_bad_arguments(gpu_ctx):
    import torch
    W, H, band, n = 128, 52, 8, 3
    g = _gathered(n, 2, W, H, band, np.random.default_rng(7))
    dev = torch.from_numpy(g.view(np.int32)).cuda()
    big = torch.zeros(2 * H * W + 2, dtype=torch.int32, device="cuda")
    dst = [big[1:].data_ptr(), big[1 + H * W:].data_ptr()]        # 4-byte aligned, not 16: the 4-byte form
    torch.cuda.synchronize()
    api.deinterleave_images(gpu_ctx, dev.data_ptr(), dst, W, H, band, n)
    torch.cuda.synchronize()
    flat = big.cpu().numpy().view(np.uint32)
    assert flat[0] == 0 and flat[-1] == 0, "wrote outside the destinations"
    for k in range(2):
        _assert_same(flat[1 + k * H * W:1 + (k + 1) * H * W].reshape(H, W), mgpu.assemble_numpy(np.ascontiguousarray(g[:, k]), H, band), f"unaligned plane {k}")
    lib = gpu_ctx.lib
    ok = dev.data_ptr()
    arr9 = (A.VP * 9)(*([A.VP(big.data_ptr())] * 9))
    withnull = (A.VP * 2)(A.VP(big.data_ptr()), A.VP(0))
    assert lib.rtr_deinterleave_images(gpu_ctx.h, A.VP(ok), 0, arr9, W, H, band, n) == -1
    assert lib.rtr_deinterleave_images(gpu_ctx.h, A.VP(ok), 9, arr9, W, H, band, n) == -1
    assert lib.rtr_deinterleave_images(gpu_ctx.h, A.VP(0), 2, arr9, W, H, band, n) == -1
    assert lib.rtr_deinterleave_images(gpu_ctx.h, A.VP(ok), 2, None, W, H, band, n) == -1
    assert lib.rtr_deinterleave_images(gpu_ctx.h, A.VP(ok), 2, withnull, W, H, band, n) == -1
    assert lib.rtr_deinterleave_images(gpu_ctx.h, A.VP(ok), 2, arr9, W, H, 12, n) == -1
    assert lib.rtr_deinterleave_images(None, A.VP(ok), 2, arr9, W, H, band, n) == -1
    assert lib.rtr_deinterleave_images(gpu_ctx.h, A.VP(ok), 2, arr9, 0, H, band, n) == -1


def _run_staged_child(code, env, timeout):
    import subprocess, sys
    try:
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        stages = [ln for ln in out.splitlines() if ln.startswith("STAGE")]
        raise AssertionError(f"child timed out after {timeout} s; last stage announced: {stages[-1] if stages else 'none'}\n" + out[-1500:])
    return r


# what both mgpu tests run in their child process: present slots in flight, slot reuse, a present batch, the framebuffer mode through
# the same slot, other iteration counts; every image of every present slot == single-GPU render + rtr_denoise_combine
_PRESENT_CHILD = """
import os, sys
sys.path.insert(0, os.getcwd())
def stage(s): print("STAGE", s, flush=True)
stage("imports")
import numpy as np
from realtimeraytracer_amd import _abi as A, api, mgpu, scenes
DEVICES, W, H, ORACLE = {devices}, {W}, {H}, {oracle}
s = scenes.cornell_box(W, H, ltc=scenes.synthetic_ltc())
stage("rtr_mgpu_create")
m = mgpu.MultiGpu(devices=DEVICES, frames_in_flight=2)
n = m.info.nranks
stage("rtr_mgpu_scene_create")
m.scene_create(s.desc)
p = api.make_params(W, H, spp=2, images=A.IMAGES_RAYGEN5)
got = {{}}
def collect(slot, key):
    got[key] = ({{w: m.download(slot, w) for w in range(8)}}, m.download(slot))
stage("refusals")
for kw, params in ((dict(exchange=False, present=True), p), (dict(present=True), api.make_params(W, H, spp=2)),
                   (dict(present=True), api.make_params(W, H, spp=2, images=A.IMAGES_RAYGEN5 | A.IMG_BIT(A.IMAGE_HDR)))):
    try:
        m.render_async(0, s.camera, s.scene_info(0), params, **kw)
        raise SystemExit(f"present launch accepted: {{kw}}")
    except RuntimeError:
        pass
stage("two present slots in flight")
m.render_async(0, s.camera, s.scene_info(0), p, present=True)
m.render_async(1, s.camera, s.scene_info(1), p, present=True)
m.wait(0); m.wait(1)
collect(0, (0, 4)); collect(1, (1, 4))
stage("slot reuse")
m.render_async(0, s.camera, s.scene_info(2), p, present=True)
m.wait(0)
collect(0, (2, 4))
stage("a present batch of two slots")
m.render_batch_async([0, 1], [s.camera, s.camera], [s.scene_info(5), s.scene_info(6)], p, present=True)
m.wait(1); m.wait(0)
collect(0, (5, 4)); collect(1, (6, 4))
stage("the framebuffer mode through the same slot")
pf = api.make_params(W, H, spp=2)
m.render_async(0, s.camera, s.scene_info(7), pf)
m.wait(0)
fb = m.download(0)
try:
    m.download(0, A.IMAGE_FINAL)
    raise SystemExit("rtr_mgpu_image_download answered for a framebuffer slot")
except RuntimeError:
    pass
stage("other iteration counts")
for it, f in ((0, 8), (3, 9)):
    m.set_denoise_iterations(it)
    m.render_async(1, s.camera, s.scene_info(f), p, present=True)
    m.wait(1)
    collect(1, (f, it))
try:
    m.set_denoise_iterations(65)
    raise SystemExit("65 iterations accepted")
except RuntimeError:
    pass
stage("reference renders")
ctx = api.Context(0)
scene = api.Scene(ctx, s.desc)
frame = api.Frame(ctx, W, H, 0xff)
for (f, it), (imgs, final) in sorted(got.items()):
    api.render(scene, s.camera, s.scene_info(f), p, frame)
    if ORACLE and f == 0:
        from oracle import oracle_py as O
        src = {{k: frame.download(k) for k in (0, 1, 2, 6, 7)}}
        ref = O.render(s.desc, s.camera, s.scene_info(f), p, bvh=scene.export_bvh(), images=A.IMAGES_RAYGEN5, threads=8)
        for k in (0, 1, 2, 6, 7):
            assert int((src[k] != ref.images[k]).sum()) == 0, ("ray-gen image vs oracle", k)
        post = O.denoise_combine(src[0], src[1], src[2], src[6], src[7], iterations=it)
        for k, v in post.items():
            assert int((imgs[k] != v).sum()) == 0, ("present image vs oracle", k)
    frame.denoise_combine(it)
    for w in range(8):
        bad = int((imgs[w] != frame.download(w)).sum())
        assert bad == 0, ("frame", f, "iterations", it, "image", w, "pixels differing", bad)
    assert int((final != frame.download(A.IMAGE_FINAL)).sum()) == 0, ("frame_download of a present slot is FINAL", f)
f1 = api.Frame(ctx, W, H)
api.render(scene, s.camera, s.scene_info(7), pf, f1)
assert int((fb != f1.download()).sum()) == 0, "framebuffer mode after present mode in the same slot"
stage("rtr_mgpu_destroy")
m.close()
print("PRESENT_OK", n, len(got))
"""


def test_mgpu_present_single_process_through_rccl(scene_cache):
    """RTR_MGPU_PRESENT with one rank through a real RCCL communicator (RTR_MGPU_SELF_EXCHANGE=1: the five-plane shard travels through
    grouped ncclSend / ncclRecv all the same); the rank-0 de-interleave of five images and the post passes on the communication stream."""
    code = textwrap.dedent(_PRESENT_CHILD.format(devices="[0]", W=330, H=186, oracle=True))
    env = dict(os.environ, RTR_MGPU_SELF_EXCHANGE="1", HSA_ENABLE_IPC_MODE_LEGACY="0", RTR_MGPU_TIMEOUT_MS="60000")
    env.pop("RTR_MGPU_TEST_SHARED_DEVICE", None)
    r = _run_staged_child(code, env, 300)
    assert r.returncode == 0 and "PRESENT_OK 1 7" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("nranks", [2, 3, 8])
def test_mgpu_present_several_ranks_on_one_gpu(nranks, scene_cache):
    """The same with 2, 3 and 8 ranks sharing the one GPU (RTR_MGPU_TEST_SHARED_DEVICE=1) through tests/fake_rccl/, preloaded in
    front of whatever the environment already preloads: rank 0 receives N - 1 five-plane shards at peer x 5 x shardBytes."""
    fake = os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so")
    if not os.path.exists(fake):
        pytest.fail("tests/fake_rccl/libfake_rccl.so is missing: run __graft_entry__.build()")
    code = textwrap.dedent(_PRESENT_CHILD.format(devices=f"[0] * {nranks}", W=320, H=186, oracle=False))
    pre = os.environ.get("LD_PRELOAD", "")
    env = dict(os.environ, LD_PRELOAD=fake + (":" + pre if pre else ""), RTR_MGPU_TEST_SHARED_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0", RTR_MGPU_TIMEOUT_MS="60000")
    env.pop("RTR_MGPU_SELF_EXCHANGE", None)
    r = _run_staged_child(code, env, 300)
    assert r.returncode == 0 and f"PRESENT_OK {nranks} 7" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
