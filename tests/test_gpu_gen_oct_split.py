"""The binned queue build has two instantiations, chosen by the launcher from the launch's samples per pixel: k_shadow_gen_oct<true>
(spp == 1: the emit pass reads hit point and normal back from LDS and nothing else; eight waves per SIMD) and k_shadow_gen_oct<false>
(spp > 1: the surface is fetched again per sample plane; seven).  Neither may change a byte: framebuffer, HDR bits and the counting
form's shadow counters against the CPU oracle, with 3 and 5 shadow rays per light triangle (5 is past kParkedPairs, so the pairs are
drawn where they are used), at an extent of whole tiles and one with a partial tile row and column, with the queue forced binned
(small frames would never launch the kernel otherwise) and once plain, and three frames in one launch."""
import numpy as np
import pytest

from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api, scenes
from test_gpu_sample_pairs import IMGS, World, _same

pytestmark = pytest.mark.gpu

SHADOW_RAYS = (3, 5)
SPPS = (1, 2)


@pytest.fixture(scope="module")
def worlds(gpu_ctx, oracle, scene_cache):
    made = {}

    def get(name, W, H):
        if (name, W, H) not in made:
            made[name, W, H] = World(gpu_ctx, oracle, scenes.cornell_box(W, H) if name == "cornell" else scenes.textured_room(W, H))
        return made[name, W, H]
    yield get
    for w in made.values():
        w.scene.close()


@pytest.mark.parametrize("size", [(64, 64), (70, 50)], ids=["64x64", "70x50"])
@pytest.mark.parametrize("name", ["cornell", "room"])
def test_both_instantiations_of_the_binned_queue_build(worlds, name, size):
    worlds(name, *size).check("binned", shadow_rays=SHADOW_RAYS, spps=SPPS)


def test_the_plain_queue_once(worlds):
    worlds("cornell", 70, 50).check("plain", shadow_rays=SHADOW_RAYS, spps=SPPS)


def test_three_frames_in_one_launch(worlds, oracle):
    """a launch of several frames: a wave's frame is looked up per wave, and with one sample per pixel every frame is one sample plane"""
    W, H, N = 70, 50, 3
    w = worlds("cornell", W, H)
    c = api.Context(0)
    try:
        c.set_tunable("trace_binned", 1)
        frames = [api.Frame(c, W, H, IMGS) for _ in range(N)]
        for f in frames:
            f.clear()
        p = w.params(3, 1, 2, 0)
        infos = [w.s.scene_info(7 + b) for b in range(N)]
        api.render_batch(w.scene, [w.s.camera] * N, infos, p, frames)
        for b, f in enumerate(frames):
            f.wait()
            hdr = np.zeros((H, W, 4), np.float32)
            ref = oracle.render(w.s.desc, w.s.camera, infos[b], p, bvh=w.bvh, images=IMGS, hdr=hdr, threads=8)
            _same(f.download(), ref.images[A.IMAGE_SHADOWED], f"frame {b} of a launch of {N}")
            assert np.array_equal(f.download(A.IMAGE_HDR).view(np.uint32), hdr.view(np.uint32)), f"frame {b} of a launch of {N}: HDR bits"
        for f in frames:
            f.close()
    finally:
        c.close()
