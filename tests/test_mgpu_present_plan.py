"""librtr_mgpu.so's present mode (RTR_MGPU_PRESENT) on a CPU-only box: the plans rtr_mgpu_plan / rtr_mgpu_plan_batch return with the
flag (what enqueue() carries out on the GPU) checked for every communicator size and launch size, and carried out — in one process
and over gloo with 2 and 3 ranks — with the oracle standing in for the renderer and the post passes: the five-plane shards must
assemble into the frame whose denoise + combine equals the unsharded oracle frame's, on all 8 images, 0 pixels differing."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest

from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import mgpu

import plan_exec as PE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = A.MGPU_PRESENT_PLANES
NPL = len(PLANES)


def check_present_plans(plans, width, height, nslots, band_rows=8, group_per_slot=False, self_exchange=0):
    """plans[r] = rank r's present plan of one launch of nslots frames.  Raises AssertionError naming the broken invariant."""
    n = len(plans)
    shard = mgpu.shard_rows(height, band_rows, n) * width * 4
    unit = NPL * shard                                   # a rank's five planes travel together
    frame = width * height * 4
    self_ex = bool(self_exchange) and n == 1
    sends, recvs = {}, {}
    for r, ops in enumerate(plans):
        kinds = [o["kind"] for o in ops]
        # the same plan as without the flag, but for the PRESENT operations and five planes instead of one
        plain = PE.plan_batch(r, n, width, height, nslots, band_rows, flags=A.MGPU_GROUP_PER_SLOT if group_per_slot else 0, self_exchange=self_exchange)
        strip = [o for o in ops if o["kind"] != A.MGPU_OP_PRESENT]
        assert [{k: v for k, v in o.items() if k != "bytes" and k != "offset"} for o in strip] == \
               [{k: v for k, v in o.items() if k != "bytes" and k != "offset"} for o in plain], (r, "present plan = plain plan + PRESENT operations")
        for a, b in zip(strip, plain):
            if a["kind"] in (A.MGPU_OP_RENDER, A.MGPU_OP_SEND, A.MGPU_OP_RECV, A.MGPU_OP_DEINTERLEAVE):
                assert a["bytes"] == NPL * b["bytes"] and a["offset"] == NPL * b["offset"], (r, "five planes", a, b)
            else:
                assert a["bytes"] == b["bytes"] and a["offset"] == b["offset"], (r, a, b)
        i_ren = kinds.index(A.MGPU_OP_RENDER)
        ren = ops[i_ren]
        assert kinds.count(A.MGPU_OP_RENDER) == 1 and ren["slot"] == 0 and ren["peer"] == r and ren["bytes"] == unit and ren["offset"] == 0, (r, "one render of five planes")
        want_buf = (A.MGPU_BUF_SELF_SRC if self_ex else A.MGPU_BUF_GATHER) if r == 0 else A.MGPU_BUF_LOCAL
        assert ren["buffer"] == want_buf, (r, "render target")
        assert sorted(o["slot"] for o in ops[:i_ren]) == list(range(nslots)) and all(o["kind"] == A.MGPU_OP_WAIT and o["event"] == A.MGPU_EV_COMM_DONE for o in ops[:i_ren]), (r, "slot guards")
        for o in ops:
            if o["kind"] in (A.MGPU_OP_SEND, A.MGPU_OP_RECV):
                assert o["stream"] == A.MGPU_STREAM_COMM and o["bytes"] == unit, (r, "transfer of five planes")
                if o["kind"] == A.MGPU_OP_SEND:
                    assert o["peer"] == 0 and o["offset"] == 0 and o["buffer"] == (A.MGPU_BUF_SELF_SRC if self_ex else A.MGPU_BUF_LOCAL), (r, "send")
                    sends.setdefault(r, []).append(o["slot"])
                else:
                    assert r == 0 and o["buffer"] == A.MGPU_BUF_GATHER and o["offset"] == unit * o["peer"], (r, "recv at peer x 5 x shardBytes")
                    recvs.setdefault(o["peer"], []).append(o["slot"])
        de = [i for i, k in enumerate(kinds) if k == A.MGPU_OP_DEINTERLEAVE]
        pr = [i for i, k in enumerate(kinds) if k == A.MGPU_OP_PRESENT]
        done = {ops[i]["slot"]: i for i, k in enumerate(kinds) if k == A.MGPU_OP_RECORD and ops[i]["event"] == A.MGPU_EV_COMM_DONE}
        assert sorted(done) == list(range(nslots)), (r, "an exchange-done record per slot")
        if r == 0:
            assert sorted(ops[i]["slot"] for i in pr) == list(range(nslots)), (r, "exactly one PRESENT per slot")
            assert all(ops[i]["bytes"] == NPL * frame and ops[i]["buffer"] == A.MGPU_BUF_FULL for i in de), (r, "de-interleave of five images")
            last_xfer = max([i for i, k in enumerate(kinds) if k in (A.MGPU_OP_SEND, A.MGPU_OP_RECV, A.MGPU_OP_GROUP_END)] or [0])
            for j in range(nslots):
                i_de = next(i for i in de if ops[i]["slot"] == j)
                i_pr = next(i for i in pr if ops[i]["slot"] == j)
                o = ops[i_pr]
                assert o["stream"] == A.MGPU_STREAM_COMM and o["buffer"] == A.MGPU_BUF_FULL and o["bytes"] == frame and o["peer"] == -1 and o["event"] == A.MGPU_EV_NONE, (j, "PRESENT operation")
                assert last_xfer < i_de < i_pr < done[j], (j, "PRESENT after the slot's DEINTERLEAVE, before its COMM_DONE record")
        else:
            assert not pr and not de, (r, "PRESENT and DEINTERLEAVE on rank 0 only")
    # the transfers pair up slot by slot, and the five-plane shards tile every slot's gather buffer exactly once
    assert sends == recvs or self_ex, ("sends and receives do not pair up", sends, recvs)
    if n > 1:
        assert sorted(sends) == list(range(1, n)) and all(v == list(range(nslots)) for v in sends.values())
    for j in range(nslots):
        pieces = [(0, unit)] if not self_ex else []
        pieces += [(o["offset"], o["bytes"]) for o in plans[0] if o["kind"] == A.MGPU_OP_RECV and o["slot"] == j]
        pieces.sort()
        assert pieces[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(pieces, pieces[1:])) and pieces[-1][0] + pieces[-1][1] == n * unit, (j, "tiling", pieces)


@pytest.mark.parametrize("n", list(range(1, 17)))
@pytest.mark.parametrize("group_per_slot", [False, True])
def test_present_plans_for_every_size(n, group_per_slot):
    W, H, band = 96, 52, 8
    flags = A.MGPU_PRESENT | (A.MGPU_GROUP_PER_SLOT if group_per_slot else 0)
    for nslots in range(1, 33):
        plans = [PE.plan_batch(r, n, W, H, nslots, band, flags=flags) for r in range(n)]
        check_present_plans(plans, W, H, nslots, band, group_per_slot)
        assert max(len(p) for p in plans) <= A.MGPU_BATCH_PLAN_MAX_OPS
        # rank 0 gains exactly one operation per slot
        assert len(plans[0]) == len(PE.plan_batch(0, n, W, H, nslots, band, flags=flags & ~A.MGPU_PRESENT)) + nslots
    one = [PE.plan(r, n, W, H, band, flags=flags) for r in range(n)]           # fits RTR_MGPU_PLAN_MAX_OPS (PE.plan's array)
    assert one == [PE.plan_batch(r, n, W, H, 1, band, flags=flags) for r in range(n)]


@pytest.mark.parametrize("extent", [(1920, 1080, 8), (7, 7, 8), (3840, 2160, 16), (640, 360, 24)])
def test_present_plans_other_extents_and_self_exchange(extent):
    W, H, band = extent
    for n in (1, 3, 8):
        check_present_plans([PE.plan_batch(r, n, W, H, 2, band, flags=A.MGPU_PRESENT) for r in range(n)], W, H, 2, band)
    check_present_plans([PE.plan_batch(0, 1, W, H, 3, band, flags=A.MGPU_PRESENT, self_exchange=1)], W, H, 3, band, self_exchange=1)


def test_checker_catches_broken_present_plans():
    W, H, band, n, nslots = 96, 52, 8, 3, 2
    good = [PE.plan_batch(r, n, W, H, nslots, band, flags=A.MGPU_PRESENT) for r in range(n)]
    check_present_plans(good, W, H, nslots, band)

    def mutated(fn):
        plans = [[dict(o) for o in p] for p in good]
        fn(plans)
        return plans
    k0 = [o["kind"] for o in good[0]]
    i_pr = k0.index(A.MGPU_OP_PRESENT)
    i_rec = next(i for i, o in enumerate(good[0]) if o["kind"] == A.MGPU_OP_RECV)

    def present_after_record(p): p[0].append(p[0].pop(i_pr))
    def present_before_deinterleave(p): p[0].insert(i_pr - 1, p[0].pop(i_pr))
    def present_missing(p): del p[0][i_pr]
    def present_on_rank1(p): p[1].insert(len(p[1]) - 1, dict(good[0][i_pr]))
    def one_plane_recv(p): p[0][i_rec]["bytes"] //= NPL
    def overlapping_recv(p): p[0][i_rec]["offset"] -= 4
    for fn in (present_after_record, present_before_deinterleave, present_missing, present_on_rank1, one_plane_recv, overlapping_recv):
        with pytest.raises((AssertionError, StopIteration, ValueError)):
            check_present_plans(mutated(fn), W, H, nslots, band)


def test_present_is_refused_with_no_exchange():
    lib = A.mgpu_lib()
    ops = (A.rtr_mgpu_op * A.MGPU_BATCH_PLAN_MAX_OPS)()
    cnt = C.c_int(0)
    for nranks in (1, 2, 8):
        assert lib.rtr_mgpu_plan(0, nranks, 64, 64, 8, A.MGPU_PRESENT | A.MGPU_NO_EXCHANGE, 0, ops, A.MGPU_PLAN_MAX_OPS, C.byref(cnt)) == -1
        assert lib.rtr_mgpu_plan_batch(0, nranks, 64, 64, 8, A.MGPU_PRESENT | A.MGPU_NO_EXCHANGE, 0, 2, ops, A.MGPU_BATCH_PLAN_MAX_OPS, C.byref(cnt)) == -1
        assert lib.rtr_mgpu_plan(0, nranks, 64, 64, 8, A.MGPU_PRESENT, 0, ops, A.MGPU_PLAN_MAX_OPS, C.byref(cnt)) == 0
    with pytest.raises(ValueError):
        PE.plan(0, 2, 64, 64, 8, flags=A.MGPU_PRESENT | A.MGPU_NO_EXCHANGE)


class PresentRunner(PE.PlanRunner):
    """One rank's PRESENT plan carried out on CPU.  render_shard(shard_index, shard_count, slot) -> {image: rows x width uint32} for the
    five ray-gen images; RENDER writes them as five planes; DEINTERLEAVE is a numpy restatement of the planes layout
    ([shard][plane][local row][x] -> five whole images); PRESENT is `post(five images) -> {image: height x width}` (the oracle's
    denoise_combine), whose result is kept per slot in .frames."""

    def __init__(self, rank, nranks, width, height, band_rows, render_shard, post, dist=None, nslots=1, self_exchange=False):
        super().__init__(rank, nranks, width, height, band_rows, render_shard, dist, nslots)
        self.rows = mgpu.shard_rows(height, band_rows, nranks)
        self.shard_bytes = NPL * self.rows * width * 4
        self.post = post
        self.frames = [None] * nslots
        self.bufs = []
        for _ in range(nslots):
            buf = {A.MGPU_BUF_LOCAL: np.zeros(self.shard_bytes, np.uint8)}
            if rank == 0:
                buf[A.MGPU_BUF_GATHER] = np.zeros(self.shard_bytes * nranks, np.uint8)
                buf[A.MGPU_BUF_FULL] = np.zeros(NPL * width * height * 4, np.uint8)
                buf[A.MGPU_BUF_LOCAL] = buf[A.MGPU_BUF_GATHER][:self.shard_bytes]
                if self_exchange:
                    buf[A.MGPU_BUF_SELF_SRC] = np.zeros(self.shard_bytes, np.uint8)
            self.bufs.append(buf)
        self.buf = self.bufs[0]

    def run(self, ops):
        import torch
        group, in_group = [], False
        for o in ops:
            k, sl = o["kind"], o["slot"]
            if k == A.MGPU_OP_WAIT:
                if o["event"] == A.MGPU_EV_COMM_DONE and self.uses == 0:
                    continue
                assert (o["event"], sl) in self.recorded, ("waits for an event nobody recorded", o)
            elif k == A.MGPU_OP_RECORD:
                self.recorded.add((o["event"], sl))
            elif k == A.MGPU_OP_RENDER:
                for j in range(self.nslots):
                    imgs = self.render_shard(o["peer"], self.n, j)
                    planes = np.concatenate([np.ascontiguousarray(imgs[w], np.uint32).reshape(-1) for w in PLANES]).view(np.uint8)
                    assert planes.size == o["bytes"], ("five planes", planes.size, o["bytes"])
                    self.bufs[j][o["buffer"]][o["offset"]:o["offset"] + o["bytes"]] = planes
            elif k == A.MGPU_OP_GROUP_START:
                assert not in_group
                in_group = True
            elif k in (A.MGPU_OP_SEND, A.MGPU_OP_RECV):
                assert in_group, "a transfer outside a group"
                group.append((k, torch.from_numpy(self.bufs[sl][o["buffer"]][o["offset"]:o["offset"] + o["bytes"]]), o["peer"]))
            elif k == A.MGPU_OP_GROUP_END:
                in_group = False
                sends = [(kk, v, p) for kk, v, p in group if kk == A.MGPU_OP_SEND]
                recvs = [(kk, v, p) for kk, v, p in group if kk == A.MGPU_OP_RECV]
                works = [self.dist.isend(v, dst=p) for _, v, p in sends] + [self.dist.irecv(v, src=p) for _, v, p in recvs]
                for w in works:
                    w.wait()
                group = []
            elif k == A.MGPU_OP_DEINTERLEAVE:
                assert o["bytes"] == NPL * self.W * self.H * 4
                g = self.bufs[sl][A.MGPU_BUF_GATHER].view(np.uint32).reshape(self.n, NPL, self.rows, self.W)
                full = self.bufs[sl][A.MGPU_BUF_FULL].view(np.uint32).reshape(NPL, self.H, self.W)
                for p in range(NPL):
                    full[p] = mgpu.assemble_numpy(np.ascontiguousarray(g[:, p]), self.H, self.band)
            elif k == A.MGPU_OP_PRESENT:
                full = self.bufs[sl][A.MGPU_BUF_FULL].view(np.uint32).reshape(NPL, self.H, self.W)
                self.frames[sl] = self.post({w: full[p].copy() for p, w in enumerate(PLANES)})
            else:
                raise AssertionError(("unknown operation", o))
        self.uses += 1


def _post(O, iterations=4):
    """PRESENT by the oracle: the whole frame's 8 images after denoise + combine"""
    def post(five):
        out = dict(five)
        out.update(O.denoise_combine(five[A.IMAGE_ANALYTIC], five[A.IMAGE_SHADOWED], five[A.IMAGE_UNSHADOWED], five[A.IMAGE_NORMAL], five[A.IMAGE_POSITION], iterations=iterations))
        return out
    return post


@pytest.mark.parametrize("n,self_exchange", [(1, False), (1, True), (2, False), (3, False), (5, False), (16, False)])
def test_present_plans_executed_in_one_process(n, self_exchange, oracle):
    """Every rank's present plans against an in-memory mailbox that matches transfers in posting order: synthetic images whose pixels
    encode (image, slot, y, x) — and the post passes of the oracle on them — come back exactly as the unsharded frames give them, for a
    one-frame plan run twice through the same slot and a two-slot launch."""
    W, H, band = 37, 52, 8                             # ragged width, 6.5 bands
    truth = {(w, j): (((np.arange(H, dtype=np.uint32)[:, None] * 7 + np.arange(W, dtype=np.uint32)[None, :] * 13 + w * 31 + j * 57) * 2654435761) & 0xffffffff).astype(np.uint32)
             for w in PLANES for j in range(3)}

    def shard_of(idx, cnt, slot):
        ys = mgpu.global_rows_of_shard(H, band, cnt, idx)
        out = {}
        for w in PLANES:
            a = np.zeros((len(ys), W), np.uint32)
            a[ys >= 0] = truth[(w, slot)][ys[ys >= 0]]
            out[w] = a
        return out

    class _W:
        def __init__(self, fn): self.fn = fn
        def wait(self): self.fn()
    mail = {}

    class Dist:
        def __init__(self, me): self.me = me
        def isend(self, v, dst):
            mail.setdefault((self.me, dst), []).append(v.clone())
            return _W(lambda: None)
        def irecv(self, v, src):
            me = self.me
            return _W(lambda: v.copy_(mail[(src, me)].pop(0)))
    post = _post(oracle)
    want = [post({w: truth[(w, j)] for w in PLANES}) for j in range(2)]
    for nslots, rounds in ((1, 2), (2, 2)):
        runners = [PresentRunner(r, n, W, H, band, shard_of, post, Dist(r), nslots=nslots, self_exchange=self_exchange) for r in range(n)]
        for _ in range(rounds):
            for r in range(n - 1, -1, -1):              # senders first: the mailbox has no blocking
                ops = PE.plan_batch(r, n, W, H, nslots, band, flags=A.MGPU_PRESENT, self_exchange=1 if self_exchange else 0)
                runners[r].run(ops)
            for j in range(nslots):
                got = runners[0].frames[j]
                assert sorted(got) == list(range(8))
                for w in range(8):
                    assert int((got[w] != want[j][w]).sum()) == 0, (n, nslots, j, w)
            assert not any(mail.values())


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, cache, out_path):
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RTR_SCENE_CACHE": cache})
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    from realtimeraytracer_amd import _abi as A
    from realtimeraytracer_amd import api, scenes
    from oracle import oracle_py as O
    import plan_exec as PE
    import test_mgpu_present_plan as T
    dist.init_process_group("gloo", rank=rank, world_size=world)
    W, H = 96, 52                                   # ragged: 6.5 bands -> padding rows on some ranks
    s = scenes.cornell_box(W, H, ltc=scenes.synthetic_ltc())
    st, nodes, tris = api.host_build_bvh(s.desc)
    bvh = (nodes, tris, st.grid)
    frame_no = [1]

    def render_slot(index, count, slot):            # RTR_MGPU_OP_RENDER: the oracle's sharded five-image render
        p = api.make_params(W, H, spp=2, images=A.IMAGES_RAYGEN5, shard_index=index, shard_count=count)
        return O.render(s.desc, s.camera, s.scene_info(frame_no[0] + slot), p, bvh=bvh, images=A.IMAGES_RAYGEN5, threads=2).images

    def reference(f):                               # the unsharded frame after the reference's post passes
        r = O.render(s.desc, s.camera, s.scene_info(f), api.make_params(W, H, spp=2, images=A.IMAGES_RAYGEN5), bvh=bvh, images=A.IMAGES_RAYGEN5, threads=2).images
        return T._post(O)({w: r[w][:H] for w in T.PLANES})
    diffs = []
    for nslots, firsts in ((1, (1, 2)), (2, (5, 9))):      # two frames through the same slot; a launch of two slots, twice
        runner = T.PresentRunner(rank, world, W, H, 8, render_slot, T._post(O), dist, nslots=nslots)
        ops = PE.plan_batch(rank, world, W, H, nslots, 8, flags=A.MGPU_PRESENT)
        for f in firsts:
            frame_no[0] = f
            runner.run(ops)
            if rank == 0:
                for j in range(nslots):
                    ref = reference(f + j)
                    diffs.extend(int((runner.frames[j][w] != ref[w]).sum()) for w in range(8))
            dist.barrier()
    if rank == 0:
        np.save(out_path, np.array(diffs + [H, W]))
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_present_frame_over_gloo_equals_the_unsharded_oracle_frame(world, tmp_path, scene_cache):
    import torch.multiprocessing as mp
    out = str(tmp_path / "result.npy")
    mp.spawn(_worker, args=(world, _free_port(), scene_cache, out), nprocs=world, join=True)
    *d, h, w = np.load(out)
    assert (h, w) == (52, 96) and len(d) == 8 * (2 + 4)
    assert not any(d), f"pixels differing per image between the present frames carried out over gloo and the unsharded oracle frames: {d}"
