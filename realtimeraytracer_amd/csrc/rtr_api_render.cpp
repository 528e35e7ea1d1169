/* rtr_api_render.cpp — the frame object and the render dispatch of the C ABI in include/rtr.h: rtr_frame_*, rtr_render_*, the
 * denoiser and the deinterleave calls (rtr_api_internal.h has what the ABI's files share).  rtr_frame is this file's alone. */
#include "../../include/rtr.h"
#include "kernels/rtr_kernels.h"
#include "kernels/rtr_post.h"
#include "rtr_api_internal.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace rtrapi;

struct rtr_frame {
    rtr_ctx* ctx = nullptr;
    uint32_t width = 0, rows = 0, images = 0;
    DevBuf<uint32_t> img[8];
    uint32_t* ext[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    DevBuf<float4> hdr;
    /* wavefront scratch */
    DevBuf<float4> hitTuvp, rayDT, rayOrigin;      /* hit records; per ray (direction, tmax); per pixel-sample the shadow rays' origin */
    DevBuf<uint32_t> raySlot;                      /* per ray: index of its visibility byte */
    uint32_t slotStride = 0;                       /* distance of the visibility planes: a power of two >= the pixel-sample slots */
    uint32_t visFill = 1;                          /* pre-fill of the visibility array for the next launch: the commoner outcome of the last one (1 = occluded) */
    DevBuf<uint32_t> hitCustom, queueCount;
    DevBuf<uint8_t> vis;
    DevBuf<int32_t> spill;
    DevBuf<uint32_t> overflow;
    uint32_t overflowCap = 0;
    DevBuf<uint2> batchLists;
    DevBuf<unsigned long long> clk;
    uint32_t listStride = 0;
    DevBuf<Counters> counters;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   /* [5]: between the any-hit kernel and k_shadow_tail */
    hipEvent_t evMega[2] = {nullptr, nullptr};
    rtr_frame_stats stats{};
    bool pendingStats = false, pendingWave = false, pendingCounters = false;
    uint32_t pendingImagesK = 0; bool pendingHdr = false, pendingAccum = false;
    hipEvent_t evDone = nullptr;         /* a frame rendered as a later frame of a batch: recorded on the leading frame's stream behind the launch */
    bool viaBatch = false;
    /* ordering between a batch launch (on the leading frame's stream) and the other frames' own streams, paid only when it is needed:
     * batchStream = the stream of the launch that last wrote this frame as a later frame of a batch and has not been joined (evDone
     * marks its end); ownPending = the frame's own stream may still hold work for it (a launch it led); evOwn orders a later batch
     * behind that work */
    hipStream_t batchStream = nullptr;
    bool ownPending = false;
    hipEvent_t evOwn = nullptr;
    /* rtr_render_split_async: the frame as band-shards ("parts") on streams of their own.  A part is an internal frame object — its
     * own scratch, events, counters and context (= stream) — that owns no image: it is bound to THIS frame's images and writes its
     * rows where they belong (RenderArgs::directRows) */
    std::vector<rtr_ctx*> partCtx;
    std::vector<rtr_frame*> parts;
    std::vector<hipEvent_t> evPart;      /* part k's launches are done (recorded on its stream, waited for by this frame's) */
    hipEvent_t evSplit[2] = {nullptr, nullptr};     /* on this frame's stream: the fork, and behind the join — the split render's duration */
    uint32_t pendingSplit = 0;           /* parts of the split render in flight (0: the last render was not split) */
    float4* extHdr = nullptr;            /* a part: the HDR image of the frame it belongs to */
    uint32_t* image_ptr(int which) const { return ext[which] ? ext[which] : img[which].p; }
    float4* hdr_ptr() const { return extHdr ? extHdr : hdr.p; }
};

extern "C" {

/* ---- frame -------------------------------------------------------------------------------- */
/* ownImages == false: a part of a split render (no images of its own, see rtr_frame::parts) */
static int frame_new(rtr_ctx* ctx, uint32_t width, uint32_t rows, uint32_t images, bool ownImages, rtr_frame** out) {
    if (!ctx || !out) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_frame_create: null ctx/out");
    if (ctx->destroyed) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_frame_create: the context has been destroyed");
    *out = nullptr;
    if (width == 0 || rows == 0 || width > 65536 || rows > 65536) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_frame_create: bad extent %ux%u", width, rows);
    if (images == 0) images = RTR_IMAGES_FRAMEBUFFER;
    const uint32_t known = 0xffu | RTR_IMG_BIT(RTR_IMAGE_HDR);
    if (images & ~known) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_frame_create: unknown image bits 0x%x", images & ~known);
    HIP_TRY(hipSetDevice(ctx->device));
    rtr_frame* f = new rtr_frame();
    f->ctx = ctx; ++ctx->children; f->width = width; f->rows = rows; f->images = images;
    const size_t px = (size_t)width * rows;
    hipError_t e = hipSuccess;
    for (int i = 0; i < 8 && e == hipSuccess && ownImages; ++i)
        if (images & RTR_IMG_BIT(i)) { e = f->img[i].alloc(px); if (e == hipSuccess) e = hipMemsetAsync(f->img[i].p, 0, px * 4, ctx->stream); }
    if (e == hipSuccess && ownImages && (images & RTR_IMG_BIT(RTR_IMAGE_HDR))) { e = f->hdr.alloc(px); if (e == hipSuccess) e = hipMemsetAsync(f->hdr.p, 0, px * 16, ctx->stream); }
    if (e == hipSuccess) e = f->counters.alloc(1);
    for (int i = 0; i < 6 && e == hipSuccess; ++i) e = hipEventCreate(&f->ev[i]);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipEventCreate(&f->evMega[i]);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { rtr_frame_destroy(f); return fail(e == hipErrorOutOfMemory ? RTR_ERR_OUT_OF_MEMORY : RTR_ERR_HIP, "rtr_frame_create: %s", hipGetErrorString(e)); }
    *out = f;
    return RTR_OK;
}

int rtr_frame_create(rtr_ctx* ctx, uint32_t width, uint32_t rows, uint32_t images, rtr_frame** out) {
    return frame_new(ctx, width, rows, images, true, out);
}

void rtr_frame_destroy(rtr_frame* f) {
    if (!f) return;
    (void)hipSetDevice(f->ctx->device);
    (void)hipStreamSynchronize(f->ctx->stream);
    for (auto& e : f->ev) if (e) (void)hipEventDestroy(e);
    for (auto& e : f->evMega) if (e) (void)hipEventDestroy(e);
    if (f->evDone) { (void)hipEventSynchronize(f->evDone); (void)hipEventDestroy(f->evDone); }
    if (f->evOwn) (void)hipEventDestroy(f->evOwn);
    for (rtr_frame* part : f->parts) rtr_frame_destroy(part);
    for (rtr_ctx* pc : f->partCtx) rtr_ctx_destroy(pc);
    for (auto& e : f->evPart) if (e) (void)hipEventDestroy(e);
    for (auto& e : f->evSplit) if (e) (void)hipEventDestroy(e);
    rtr_ctx* c = f->ctx;
    delete f;
    ctx_release_child(c);
}

int rtr_frame_bind_external(rtr_frame* f, int which, void* dptr, size_t bytes) {
    if (!f || which < 0 || which > 7) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_frame_bind_external: bad argument");
    if (dptr && bytes != (size_t)f->width * f->rows * 4) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_frame_bind_external: %zu bytes given, image is %zu", bytes, (size_t)f->width * f->rows * 4);
    if (dptr && ((uintptr_t)dptr & 3u)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_frame_bind_external: pointer not 4-byte aligned");
    f->ext[which] = (uint32_t*)dptr;
    if (dptr) f->images |= RTR_IMG_BIT(which);
    return RTR_OK;
}

int rtr_frame_device_ptr(const rtr_frame* f, int which, void** dptr, size_t* bytes) {
    if (!f || !dptr) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_frame_device_ptr: null argument");
    if (which == RTR_IMAGE_HDR) {
        if (!f->hdr.p) return fail(RTR_ERR_INVALID_ARGUMENT, "frame has no HDR image");
        *dptr = f->hdr.p; if (bytes) *bytes = (size_t)f->width * f->rows * 16; return RTR_OK;
    }
    if (which < 0 || which > 7 || !f->image_ptr(which)) return fail(RTR_ERR_INVALID_ARGUMENT, "frame has no image %d", which);
    *dptr = f->image_ptr(which); if (bytes) *bytes = (size_t)f->width * f->rows * 4;
    return RTR_OK;
}

int rtr_frame_download(const rtr_frame* f, int which, void* dst, size_t bytes) {
    if (!f || !dst) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_frame_download: null argument");
    void* src = nullptr; size_t need = 0;
    int rc = rtr_frame_device_ptr(f, which, &src, &need);
    if (rc != RTR_OK) return rc;
    if (bytes != need) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_frame_download: %zu bytes given, image %d is %zu", bytes, which, need);
    HIP_TRY(hipSetDevice(f->ctx->device));
    if (f->viaBatch) HIP_TRY(hipEventSynchronize(f->evDone));          /* its pixels came from another frame's stream */
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, f->ctx->stream));
    HIP_TRY(hipStreamSynchronize(f->ctx->stream));
    return RTR_OK;
}

/* Work about to be enqueued for `f` on its own stream comes behind a batch launch on another stream that wrote it last (the launch
 * runs on its leading frame's stream), and a later batch must come behind this work (ownPending): the ordering contract of
 * rtr_render_batch_async for everything that is not itself a render */
static int order_on_own_stream(rtr_frame* f) {
    hipStream_t st = f->ctx->stream;
    if (f->batchStream && f->batchStream != st) HIP_TRY(hipStreamWaitEvent(st, f->evDone, 0));
    f->batchStream = nullptr;
    f->ownPending = true;
    return RTR_OK;
}

int rtr_frame_clear(rtr_frame* f) {
    if (!f) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_frame_clear: null frame");
    HIP_TRY(hipSetDevice(f->ctx->device));
    { const int rc = order_on_own_stream(f); if (rc != RTR_OK) return rc; }
    const size_t px = (size_t)f->width * f->rows;
    for (int i = 0; i < 8; ++i) if (f->image_ptr(i)) HIP_TRY(hipMemsetAsync(f->image_ptr(i), 0, px * 4, f->ctx->stream));
    if (f->hdr.p) HIP_TRY(hipMemsetAsync(f->hdr.p, 0, px * 16, f->ctx->stream));
    HIP_TRY(hipStreamSynchronize(f->ctx->stream));
    return RTR_OK;
}

/* ---- dispatch ------------------------------------------------------------------------------ */
/* Enqueues one launch of the pipeline over n frames (n = 1: rtr_render / rtr_render_async).  frames[0] leads: its context's stream
 * carries the work, its scratch holds the batch, its statistics describe the launch. */
static_assert(RTR_MAX_BATCH == rtrdev::kMaxBatch, "include/rtr.h and kernels/rtr_device.h disagree on the frames per launch");
static int enqueue_render(rtr_scene* s, const RtrCameraData* cams, const RtrSceneInfo* infos, const rtr_render_params* pin, rtr_frame* const* frames, uint32_t n, bool direct = false) {
    if (!s || !cams || !infos || !pin || !frames || n < 1 || !frames[0]) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render: null argument");
    if (n > rtrdev::kMaxBatch) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_batch_async: %u frames, at most %u per launch", n, rtrdev::kMaxBatch);
    rtr_frame* f = frames[0];
    /* work is enqueued on the (leading) FRAME's context stream; the (read-only) scene may belong to another context of the same
     * device, so two frames on two streams can be in flight against one scene */
    if (s->ctx->device != f->ctx->device) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render: scene and frame live on different devices");
    rtr_render_params p = *pin;
    if (p.bandRows == 0) p.bandRows = 8;
    if (p.shardCount == 0) p.shardCount = 1;
    if (p.images == 0) p.images = RTR_IMAGES_FRAMEBUFFER;
    if (p.width == 0 || p.height == 0 || p.spp == 0 || p.spp > 1024 || p.numShadowRays > 1024)
        return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render: bad width/height/spp/numShadowRays (%u,%u,%u,%u)", p.width, p.height, p.spp, p.numShadowRays);
    if (p.bandRows % 8u) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render: bandRows %u must be a multiple of 8 (one wave = one 8x8 tile)", p.bandRows);
    if (p.shardIndex >= p.shardCount) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render: shardIndex %u >= shardCount %u", p.shardIndex, p.shardCount);
    const uint32_t rows = rtr_shard_rows(p.height, p.bandRows, p.shardCount);
    const uint32_t frameRows = direct ? p.height : rows;     /* direct: the images are the whole frame, this shard writes its own rows of them */
    if (p.images & RTR_IMAGES_DENOISE) return fail(RTR_ERR_UNSUPPORTED, "rtr_render: denoise/combine images are produced by rtr_denoise_combine, not by the ray-gen dispatch");
    if ((p.images & RTR_IMG_BIT(RTR_IMAGE_ANALYTIC)) && !s->hasLtc) return fail(RTR_ERR_UNSUPPORTED, "rtr_render: RTR_IMAGE_ANALYTIC needs the LTC tables (rtr_scene_desc.ltc1/ltc2)");
    const bool wantHdr = (p.images & RTR_IMG_BIT(RTR_IMAGE_HDR)) != 0 || p.accumulate;
    if (n > 1 && p.pipeline == 1) return fail(RTR_ERR_UNSUPPORTED, "rtr_render_batch_async: the megakernel renders one frame per launch");

    rtrdev::FrameBatch fb{};
    fb.n = n;
    uint32_t k = 0;
    uint64_t maxRays = 1;
    for (uint32_t b = 0; b < n; ++b) {
        rtr_frame* fr = frames[b];
        if (!fr) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_batch_async: frame %u is null", b);
        for (uint32_t c = 0; c < b; ++c) if (frames[c] == fr) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_batch_async: frame %u given twice", b);
        if (fr->ctx->device != f->ctx->device) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_batch_async: frame %u lives on another device", b);
        if (infos[b].numAreaLights > s->numLights) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render: SceneInfo.numAreaLights %u > scene lights %u", infos[b].numAreaLights, s->numLights);
        if (infos[b].numAreaLights != infos[0].numAreaLights) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_batch_async: the frames of a launch must use the same number of area lights");
        if (fr->width != p.width || fr->rows != frameRows) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render: frame is %ux%u, this shard needs %ux%u", fr->width, fr->rows, p.width, frameRows);
        if (wantHdr && !fr->hdr_ptr()) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render: HDR accumulation requested but the frame has no RTR_IMAGE_HDR");
        FrameOut& fo = fb.fo[b];
        k = 0;
        for (int i = 0; i < 8; ++i) {
            fo.img[i] = nullptr;
            if (p.images & RTR_IMG_BIT(i)) {
                if (!fr->image_ptr(i)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render: image %d requested but not in the frame", i);
                fo.img[i] = fr->image_ptr(i); ++k;
            }
        }
        fo.hdr = wantHdr ? fr->hdr_ptr() : nullptr;
        RenderArgs& ra = fb.ra[b];
        ra.cam = cams[b]; ra.info = infos[b];
        ra.width = p.width; ra.height = p.height; ra.spp = p.spp; ra.numShadowRays = p.numShadowRays;
        ra.bandRows = p.bandRows; ra.shardIndex = p.shardIndex; ra.shardCount = p.shardCount;
        ra.localRows = rows; ra.tilesPerRow = (p.width + 7u) / 8u;
        ra.images = p.images; ra.accumulate = p.accumulate; ra.accumulatedFrames = p.accumulatedFrames; ra.directRows = direct ? 1u : 0u;
        if (b == 0) for (uint32_t l = 0; l < infos[0].numAreaLights; ++l) maxRays += (uint64_t)s->hostLights[l].numTriangles * p.numShadowRays;
        ra.maxRaysPerSample = (uint32_t)maxRays;
    }
    const RenderArgs& ra = fb.ra[0];
    const FrameOut& fo = fb.fo[0];

    HIP_TRY(hipSetDevice(f->ctx->device));
    hipStream_t st = f->ctx->stream;
    Counters* dstats = nullptr;
    if (p.collectStats) { HIP_TRY(hipMemsetAsync(f->counters.p, 0, sizeof(Counters), st)); dstats = f->counters.p; }

    const uint64_t paddedPixels = (uint64_t)((rows + 7u) / 8u) * ra.tilesPerRow * 64u;
    const uint64_t blocks = (paddedPixels + 255u) / 256u;
    const uint64_t nPS = blocks * 256u * p.spp * n;          /* pixel-sample slots of the launch */
    const uint64_t nRays = nPS * maxRays;                    /* queue capacity: every pixel-sample issuing every query */
    uint64_t slotStride = 256;                                /* the visibility planes are a power of two apart, so a slot names its pixel-sample with a mask */
    while (slotStride < nPS) slotStride <<= 1;
    const uint64_t nSlots = slotStride * maxRays;
    bool wave = p.pipeline != 1;
    if (wave && (nSlots >= (1ull << 31) || maxRays > 4096)) {
        if (p.pipeline == 2 || n > 1) return fail(RTR_ERR_UNSUPPORTED, "rtr_render: wavefront scratch would need %llu visibility slots", (unsigned long long)nSlots);
        wave = false;
    }
    if (blocks * n >= (1ull << 31)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render: frame too large");

    /* the counting form IS the timed kernel template; the 2-wide comparison kernel has none, and counting another kernel's work
     * under its name would be a wrong number */
    if (wave && p.collectStats && f->ctx->tun.trace_bvh4 == 0u)
        return fail(RTR_ERR_UNSUPPORTED, "rtr_render: collectStats with the tunable trace_bvh4 = 0: the 2-wide comparison kernel has no counting form (set it back to 1, or render with pipeline 1)");
    f->pendingWave = wave; f->pendingCounters = p.collectStats != 0;
    f->pendingImagesK = k; f->pendingHdr = wantHdr; f->pendingAccum = p.accumulate != 0;
    memset(&f->stats, 0, sizeof f->stats);
    f->stats.localRows = rows; f->stats.localPixels = rows * p.width * n;
    f->viaBatch = false; f->pendingSplit = 0;
    /* The launch runs on THIS frame's stream.  What another stream still holds for one of its frames comes first: a launch the frame
     * led on its own stream (ownPending), or a batch on a third stream that wrote it (batchStream).  In steady state — the same
     * frames batched behind the same leader, or frames joined between uses — neither is set and nothing is enqueued here (cross-stream
     * waits on every launch cost 3 % of the frame rate at N = 1 and 25 % on a 1/8 shard: profiles/r03/ab_batch_stream_order.log). */
    if (f->batchStream && f->batchStream != st) HIP_TRY(hipStreamWaitEvent(st, f->evDone, 0));
    f->batchStream = nullptr;
    for (uint32_t b = 1; b < n; ++b) {
        rtr_frame* fr = frames[b];
        if (fr->ownPending && fr->ctx->stream != st) {
            if (!fr->evOwn) HIP_TRY(hipEventCreateWithFlags(&fr->evOwn, hipEventDisableTiming));
            HIP_TRY(hipEventRecord(fr->evOwn, fr->ctx->stream));
            HIP_TRY(hipStreamWaitEvent(st, fr->evOwn, 0));
        }
        if (fr->batchStream && fr->batchStream != st) HIP_TRY(hipStreamWaitEvent(st, fr->evDone, 0));
    }
    hipError_t e;
    if (wave) {
        /* the list of rays left to the redo kernels: the camera rays' needs one entry per pixel-sample at most; the any-hit kernel's
         * gets 1/16 of the queue (at least 2^20 entries) and k_shadow_tail redoes the whole queue should that ever overflow */
        uint64_t ovCap = std::max<uint64_t>(std::max<uint64_t>(nPS, nRays / 16), 1ull << 20);
        if (ovCap > nRays) ovCap = std::max<uint64_t>(nRays, nPS);
        if (f->hitTuvp.n < nPS) { HIP_TRY(f->hitTuvp.alloc(nPS)); HIP_TRY(f->hitCustom.alloc(nPS)); HIP_TRY(f->rayOrigin.alloc(nPS)); }
        if (f->vis.n < nSlots) HIP_TRY(f->vis.alloc(nSlots));
        if (f->rayDT.n < nRays) { HIP_TRY(f->rayDT.alloc(nRays)); HIP_TRY(f->raySlot.alloc(nRays)); }
        /* every array is (re)sized by its OWN need: the redo list is also k_primary's (one entry per pixel-sample at most), and a
         * launch with fewer queries per sample but more samples than an earlier one needs a longer list with a shorter queue */
        if (f->overflow.n < ovCap + 1) HIP_TRY(f->overflow.alloc(ovCap + 1));
        f->overflowCap = (uint32_t)std::min<uint64_t>(ovCap, f->overflow.n - 1);      /* what the any-hit kernel may use of it */
#ifdef RTR_TEST_HOOKS
        if (const char* e = getenv("RTR_TRACE_OVERFLOW_CAP")) { const uint64_t v = strtoull(e, nullptr, 10); if (v >= 1 && v < f->overflowCap) f->overflowCap = (uint32_t)v; }   /* a list short enough to overflow */
#endif
        {   /* batch lists of the binned queue (octant x consumer XCD): a run's batches are dealt round-robin to the eight lists of
             * its octant, so a list holds at most 1/8 of one batch per 64 rays (the smallest batch) + one per k_shadow_gen_oct workgroup */
            const uint64_t ls = nRays / 64 / rtrdev::kQueueRegions + nPS / 256 + 16;
            if ((uint64_t)f->listStride < ls) { HIP_TRY(f->batchLists.alloc((size_t)ls * rtrdev::kQueueLists)); f->listStride = (uint32_t)ls; }
        }
        f->slotStride = (uint32_t)slotStride;
        if (!f->queueCount.p) HIP_TRY(f->queueCount.alloc(rtrdev::kQueueCtrlWords));
        if (!f->clk.p) { HIP_TRY(f->clk.alloc(2 * rtrdev::kQueueRegions)); HIP_TRY(hipMemsetAsync(f->clk.p, 0, 2 * rtrdev::kQueueRegions * sizeof(unsigned long long), st)); }
        if (!f->spill.p) HIP_TRY(f->spill.alloc(rtrdev::kSpillInts));      /* 64 entries x the redo kernels' grid */
        Workspace ws;
        ws.hitTuvp = f->hitTuvp.p; ws.hitCustom = f->hitCustom.p; ws.vis = f->vis.p; ws.visFill = f->visFill;
        ws.visPlaneBytes = (size_t)nPS; ws.visPlanes = (uint32_t)maxRays;      /* what a launch fills: the first nPS bytes of each of the maxRays planes, not the power-of-two pitch between them */
#ifdef RTR_TEST_HOOKS
        if (const char* e = getenv("RTR_TRACE_VIS_FILL")) if ((e[0] == '0' || e[0] == '1') && !e[1]) ws.visFill = (uint32_t)(e[0] - '0');      /* force the pre-fill */
#endif
        ws.rayQueue.dt = f->rayDT.p; ws.rayQueue.slot = f->raySlot.p; ws.rayQueue.origin = f->rayOrigin.p; ws.rayQueue.slotStride = f->slotStride; ws.rayQueue.slotMask = f->slotStride - 1u;
        ws.queueCount = f->queueCount.p; ws.capPixelSamples = nPS; ws.capRays = nRays; ws.spill = f->spill.p; ws.overflow = f->overflow.p; ws.overflowCap = f->overflowCap; ws.batchLists = f->batchLists.p; ws.listStride = f->listStride; ws.clk = f->clk.p;
        e = rtrdev::launch_wavefront(s->dev, fb, ws, f->ctx->tun, (int)s->tree.stats.stackEntries, dstats, st, f->ev, (uint32_t)f->ctx->prop.multiProcessorCount);
    } else {
        (void)hipEventRecord(f->evMega[0], st);
        e = rtrdev::launch_megakernel(s->dev, ra, fo, (int)s->tree.stats.stackEntries, dstats, st);
        (void)hipEventRecord(f->evMega[1], st);
    }
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
    f->pendingStats = true;
    f->ownPending = true;
    /* ... and each of the other frames gets an event behind the launch: rtr_frame_wait / rtr_frame_download wait on it, and so does
     * the stream of whatever launch writes the frame next (above) */
    for (uint32_t b = 1; b < n; ++b) {
        rtr_frame* fr = frames[b];
        if (!fr->evDone) HIP_TRY(hipEventCreateWithFlags(&fr->evDone, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(fr->evDone, st));
        fr->batchStream = st;
        fr->viaBatch = true; fr->pendingStats = false;
        memset(&fr->stats, 0, sizeof fr->stats);
    }
    return RTR_OK;
}

int rtr_render_batch_limit(const rtr_scene* s, const rtr_render_params* pin, uint32_t numAreaLights, uint32_t* maxFrames) {
    if (!s || !pin || !maxFrames) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_batch_limit: null argument");
    if (numAreaLights > s->numLights) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_batch_limit: %u area lights, the scene has %u", numAreaLights, s->numLights);
    rtr_render_params p = *pin;
    if (p.bandRows == 0) p.bandRows = 8;
    if (p.shardCount == 0) p.shardCount = 1;
    if (p.width == 0 || p.height == 0 || p.spp == 0 || p.bandRows % 8u) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_batch_limit: bad width/height/spp/bandRows");
    *maxFrames = 1;
    if (p.pipeline == 1) return RTR_OK;
    /* the arithmetic of enqueue_render() */
    uint64_t maxRays = 1;
    for (uint32_t l = 0; l < numAreaLights; ++l) maxRays += (uint64_t)s->hostLights[l].numTriangles * p.numShadowRays;
    const uint32_t rows = rtr_shard_rows(p.height, p.bandRows, p.shardCount);
    const uint64_t blocks = ((uint64_t)((rows + 7u) / 8u) * ((p.width + 7u) / 8u) * 64u + 255u) / 256u;
    for (uint32_t n = rtrdev::kMaxBatch; n > 1; --n) {
        const uint64_t nPS = blocks * 256u * p.spp * n;
        uint64_t slotStride = 256;
        while (slotStride < nPS) slotStride <<= 1;
        if (slotStride * maxRays < (1ull << 31) && maxRays <= 4096 && blocks * n < (1ull << 31)) { *maxFrames = n; break; }
    }
    return RTR_OK;
}

/* One frame as `parts` band-shards, each on a stream of its own, all writing their rows of the SAME images: the kernels of one frame
 * are a dependency chain and each ends in a tail, so part k+1's camera rays and queue build run under part k's traversal and its
 * traversal fills the tail of part k's — frames in flight, inside one frame. */
int rtr_render_split_async(rtr_scene* s, const RtrCameraData* cam, const RtrSceneInfo* info, const rtr_render_params* pin, rtr_frame* f, uint32_t parts) {
    if (!s || !cam || !info || !pin || !f) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_split_async: null argument");
    if (parts < 1 || parts > RTR_MAX_SPLIT) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_split_async: %u parts, 1 to %d", parts, RTR_MAX_SPLIT);
    if (pin->shardCount > 1) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_split_async: the frame must be whole (shardCount %u); a shard of a multi-GPU frame is not split again", pin->shardCount);
    if (f->extHdr) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_split_async: not a frame of the caller's");
    rtr_render_params p = *pin;
    if (p.bandRows == 0) p.bandRows = 8;
    if (p.bandRows % 8u) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_split_async: bandRows %u must be a multiple of 8", p.bandRows);
    if (p.height == 0 || p.width == 0) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_split_async: empty frame");
    const uint32_t bands = (p.height + p.bandRows - 1) / p.bandRows;
    if (parts > bands) parts = bands;                 /* never a part without a band */
    if (parts <= 1) { p.shardIndex = 0; p.shardCount = 1; return enqueue_render(s, cam, info, &p, &f, 1); }
    if (f->width != p.width || f->rows != p.height) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_split_async: frame is %ux%u, the whole frame is %ux%u", f->width, f->rows, p.width, p.height);
    HIP_TRY(hipSetDevice(f->ctx->device));
    hipStream_t st = f->ctx->stream;
    /* the parts: internal frame objects (scratch, events, counters; no images) on contexts (streams) of their own */
    while (f->parts.size() < parts) {
        rtr_ctx* pc = nullptr; rtr_frame* pf = nullptr;
        int rc = ctx_create_prio(f->ctx->device, f->ctx->tun.split_priorities ? (int)f->parts.size() : -1, &pc);
        if (rc != RTR_OK) return rc;
        rc = frame_new(pc, f->width, f->rows, f->images, false, &pf);
        if (rc != RTR_OK) { rtr_ctx_destroy(pc); return rc; }
        hipEvent_t ev = nullptr;
        hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e != hipSuccess) { rtr_frame_destroy(pf); rtr_ctx_destroy(pc); return fail(RTR_ERR_HIP, "hipEventCreate: %s", hipGetErrorString(e)); }
        f->partCtx.push_back(pc); f->parts.push_back(pf); f->evPart.push_back(ev);
    }
    for (auto& e : f->evSplit) if (!e) HIP_TRY(hipEventCreate(&e));
    /* what another stream still holds for this frame comes first (enqueue_render's rule) */
    if (f->batchStream && f->batchStream != st) HIP_TRY(hipStreamWaitEvent(st, f->evDone, 0));
    f->batchStream = nullptr;
    HIP_TRY(hipEventRecord(f->evSplit[0], st));          /* the fork */
    /* A failure inside the loop must not leave the frame's stream un-joined from parts that were already enqueued (a download, clear
     * or denoise that follows would race them, and rtr_frame_wait would never collect them): the error is kept, every part that WAS
     * enqueued is joined, the frame is marked pending for exactly those, and then the error is returned. */
    int rc = RTR_OK;
    uint32_t started = 0;
    auto hip_keep = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && rc == RTR_OK) rc = fail(RTR_ERR_HIP, "rtr_render_split_async: %s: %s", what, hipGetErrorString(e));
        return e == hipSuccess;
    };
    for (uint32_t k = 0; k < parts && rc == RTR_OK; ++k) {
        rtr_frame* pf = f->parts[k];
        pf->ctx->tun = f->ctx->tun;
        pf->images = f->images;
        for (int i = 0; i < 8; ++i) pf->ext[i] = f->image_ptr(i);
        pf->extHdr = f->hdr.p;
        hipStream_t ps = pf->ctx->stream;
        if (!hip_keep(hipStreamWaitEvent(ps, f->evSplit[0], 0), "hipStreamWaitEvent (fork)")) break;
        p.shardIndex = k; p.shardCount = parts;
        const int prc = enqueue_render(s, cam, info, &p, &pf, 1, true);
        if (prc != RTR_OK) { rc = prc; break; }
        ++started;                                              /* from here on part k has work on its stream: it must be joined */
        if (hip_keep(hipEventRecord(f->evPart[k], ps), "hipEventRecord (part)")) hip_keep(hipStreamWaitEvent(st, f->evPart[k], 0), "hipStreamWaitEvent (join)");
        else hip_keep(hipStreamSynchronize(ps), "hipStreamSynchronize (join of last resort)");      /* no event to order behind: drain the part here */
    }
    hip_keep(hipEventRecord(f->evSplit[1], st), "hipEventRecord (join)");
    f->ownPending = true; f->viaBatch = false;
    f->pendingSplit = started; f->pendingStats = started != 0;
    return rc;
}

int rtr_render_split(rtr_scene* s, const RtrCameraData* cam, const RtrSceneInfo* info, const rtr_render_params* p, rtr_frame* f, uint32_t parts) {
    int rc = rtr_render_split_async(s, cam, info, p, f, parts);
    if (rc != RTR_OK) return rc;
    return rtr_frame_wait(f);
}

/* joins a split render and makes the frame's statistics out of its parts': counters and per-kernel times are SUMS over the parts (the
 * parts' kernels overlap: the sum of their durations exceeds the frame's), totalMs is the frame's own duration, fork to join */
static int wait_split(rtr_frame* f) {
    const uint32_t parts = f->pendingSplit;
    f->pendingSplit = 0; f->pendingStats = false;
    rtr_frame_stats t; memset(&t, 0, sizeof t);
    double clk = 0; uint32_t nclk = 0;
    for (uint32_t k = 0; k < parts; ++k) {
        int rc = rtr_frame_wait(f->parts[k]);
        if (rc != RTR_OK) return rc;
        const rtr_frame_stats& a = f->parts[k]->stats;
        t.numRays += a.numRays; t.numPrimaryRays += a.numPrimaryRays; t.numShadowRays += a.numShadowRays; t.numNodeVisits += a.numNodeVisits;
        t.numTriTests += a.numTriTests; t.numHits += a.numHits; t.numLightFetches += a.numLightFetches; t.numLightTriFetches += a.numLightTriFetches;
        t.numTexFetches += a.numTexFetches; t.numAlphaTests += a.numAlphaTests; t.algorithmicBytes += a.algorithmicBytes;
        t.numShadowNodeVisits += a.numShadowNodeVisits; t.numShadowTriTests += a.numShadowTriTests; t.shadowTraceBytes += a.shadowTraceBytes;
        t.primaryMs += a.primaryMs; t.shadowGenMs += a.shadowGenMs; t.shadowTraceMs += a.shadowTraceMs; t.resolveMs += a.resolveMs; t.shadowTailMs += a.shadowTailMs;
        t.localRows += a.localRows; t.localPixels += a.localPixels; t.pipelineUsed = a.pipelineUsed;
        t.shadowInnerIterations += a.shadowInnerIterations; t.shadowInnerActiveLanes += a.shadowInnerActiveLanes;
        t.shadowTriIterations += a.shadowTriIterations; t.shadowTriActiveLanes += a.shadowTriActiveLanes; t.shadowRefills += a.shadowRefills;
        t.primaryTailRays += a.primaryTailRays; t.shadowTailRays += a.shadowTailRays;
        if (a.shadowTraceClockMHz > 0.f) {
            clk += a.shadowTraceClockMHz; ++nclk;
            t.shadowTraceClockMinMHz = (t.shadowTraceClockMinMHz == 0.f || a.shadowTraceClockMinMHz < t.shadowTraceClockMinMHz) ? a.shadowTraceClockMinMHz : t.shadowTraceClockMinMHz;
            t.shadowTraceClockMaxMHz = a.shadowTraceClockMaxMHz > t.shadowTraceClockMaxMHz ? a.shadowTraceClockMaxMHz : t.shadowTraceClockMaxMHz;
        }
    }
    if (nclk) t.shadowTraceClockMHz = (float)(clk / nclk);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, f->evSplit[0], f->evSplit[1]);
    t.totalMs = ms;
    f->stats = t;
    return RTR_OK;
}

int rtr_frame_wait(rtr_frame* f) {
    if (!f) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_frame_wait: null frame");
    HIP_TRY(hipSetDevice(f->ctx->device));
    HIP_TRY(hipStreamSynchronize(f->ctx->stream));
    f->ownPending = false;
    if (f->pendingSplit) return wait_split(f);
    if (f->viaBatch) { HIP_TRY(hipEventSynchronize(f->evDone)); f->batchStream = nullptr; return RTR_OK; }      /* rendered in another frame's launch: that launch's times and counters are the leading frame's */
    if (!f->pendingStats) return RTR_OK;
    f->pendingStats = false;
    rtr_frame_stats& s = f->stats;
    if (f->pendingWave) {
        float a = 0, b = 0, c = 0, d = 0;
        (void)hipEventElapsedTime(&a, f->ev[0], f->ev[1]);
        (void)hipEventElapsedTime(&b, f->ev[1], f->ev[2]);
        (void)hipEventElapsedTime(&c, f->ev[2], f->ev[5]);
        float tail = 0;
        (void)hipEventElapsedTime(&tail, f->ev[5], f->ev[3]);
        s.shadowTailMs = tail;
        (void)hipEventElapsedTime(&d, f->ev[3], f->ev[4]);
        s.primaryMs = a; s.shadowGenMs = b; s.shadowTraceMs = c; s.resolveMs = d; s.totalMs = a + b + c + tail + d;
        s.pipelineUsed = 2;
        if (f->clk.p) {      /* shader clock held during the any-hit launch: s_memtime ticks over 100-MHz ticks of one wave per XCD; the MEAN over the XCDs — they clock
                              * independently (2.25 ... 2.40 GHz within one launch on a warm part) and the launch's vector-issue capacity is the sum of theirs */
            unsigned long long h[2 * rtrdev::kQueueRegions];
            HIP_TRY(hipMemcpy(h, f->clk.p, sizeof h, hipMemcpyDeviceToHost));
            float mhz[rtrdev::kQueueRegions]; int nv = 0;
            for (uint32_t r = 0; r < rtrdev::kQueueRegions; ++r) if (h[2 * r + 1]) mhz[nv++] = (float)((double)h[2 * r] / (double)h[2 * r + 1] * 100.0);
            for (int i = 1; i < nv; ++i) for (int j = i; j > 0 && mhz[j] < mhz[j - 1]; --j) { const float t = mhz[j]; mhz[j] = mhz[j - 1]; mhz[j - 1] = t; }
            double sum = 0; for (int i = 0; i < nv; ++i) sum += mhz[i];
            s.shadowTraceClockMHz = nv ? (float)(sum / nv) : 0.f;
            s.shadowTraceClockMinMHz = nv ? mhz[0] : 0.f; s.shadowTraceClockMaxMHz = nv ? mhz[nv - 1] : 0.f;
        }
        if (f->queueCount.p) {      /* the next launch pre-fills the visibility array with this one's commoner outcome */
            uint32_t q[4] = {0, 0, 0, 0};
            HIP_TRY(hipMemcpy(q, f->queueCount.p, sizeof q, hipMemcpyDeviceToHost));
            if (q[0]) f->visFill = (2ull * q[3] >= q[0]) ? 1u : 0u;
        }
    } else {
        float a = 0;
        (void)hipEventElapsedTime(&a, f->evMega[0], f->evMega[1]);
        s.primaryMs = a; s.totalMs = a;
        s.pipelineUsed = 1;
    }
    if (f->pendingCounters) {
        Counters h;
        HIP_TRY(hipMemcpy(&h, f->counters.p, sizeof h, hipMemcpyDeviceToHost));
        s.numRays = h.rays; s.numPrimaryRays = h.primary; s.numShadowRays = h.shadow;
        s.numNodeVisits = h.nodes; s.numTriTests = h.tris; s.numHits = h.hits;
        s.numLightFetches = h.lightFetch; s.numLightTriFetches = h.lightTriFetch;
        s.numShadowNodeVisits = h.shadowNodes; s.numShadowTriTests = h.shadowTris;
        s.numTexFetches = h.texFetch; s.numAlphaTests = h.alphaTests;
        const uint64_t shadowNodeBytes = f->pendingWave ? RTR_WIDE_NODE_BYTES : RTR_BVH_NODE_BYTES;     /* the megakernel walks the BVH2 for its shadow rays too */
        s.shadowTraceBytes = shadowNodeBytes * h.shadowNodes + 48ull * h.shadowTris + 37ull * h.shadow;      /* per ray: 20 B of queue record + the 16-B origin of its pixel-sample + its visibility byte */
        s.shadowInnerIterations = h.innerIters; s.shadowInnerActiveLanes = h.innerLanes;
        s.shadowTriIterations = h.triIters; s.shadowTriActiveLanes = h.triLanes; s.shadowRefills = h.refills;
        if (f->overflow.p) { uint32_t ov = 0; HIP_TRY(hipMemcpy(&ov, f->overflow.p, sizeof ov, hipMemcpyDeviceToHost)); s.shadowTailRays = ov; }
        if (f->pendingWave && f->queueCount.p) { uint32_t rd = 0; HIP_TRY(hipMemcpy(&rd, f->queueCount.p + 2, sizeof rd, hipMemcpyDeviceToHost)); s.primaryTailRays = rd; }
        s.algorithmicBytes = (uint64_t)RTR_BVH_NODE_BYTES * (h.nodes - h.shadowNodes) + shadowNodeBytes * h.shadowNodes + 48ull * h.tris + 236ull * (h.hits + h.alphaTests) + 96ull * h.lightFetch + 156ull * h.lightTriFetch +
                             16ull * h.texFetch +
                             4ull * f->pendingImagesK * s.localPixels + (f->pendingHdr ? (f->pendingAccum ? 32ull : 16ull) * s.localPixels : 0ull);
    }
    return RTR_OK;
}

int rtr_render_async(rtr_scene* s, const RtrCameraData* cam, const RtrSceneInfo* info, const rtr_render_params* p, rtr_frame* f) {
    return enqueue_render(s, cam, info, p, &f, 1);
}

int rtr_render_batch_async(rtr_scene* s, const RtrCameraData* cams, const RtrSceneInfo* infos, const rtr_render_params* p, rtr_frame* const* frames, uint32_t n) {
    return enqueue_render(s, cams, infos, p, frames, n);
}

int rtr_render(rtr_scene* s, const RtrCameraData* cam, const RtrSceneInfo* info, const rtr_render_params* p, rtr_frame* f) {
    int rc = enqueue_render(s, cam, info, p, &f, 1);
    if (rc != RTR_OK) return rc;
    return rtr_frame_wait(f);
}

int rtr_frame_get_stats(const rtr_frame* f, rtr_frame_stats* out) {
    if (!f || !out) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_frame_get_stats: null argument");
    *out = f->stats;
    return RTR_OK;
}

/* the checks, launches and ping-pong of rtr_denoise_combine, enqueued on the frame's context stream (behind a batch launch that wrote
 * the frame on another stream, and ahead of a later one: order_on_own_stream) */
static int enqueue_denoise_combine(rtr_frame* f, int iterations, const char* who) {
    if (!f) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null frame", who);
    if (iterations < 0 || iterations > 64) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: iterations %d", who, iterations);
    for (int i = 0; i < 8; ++i)
        if (!f->image_ptr(i)) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: the frame lacks image %d (create it with all of images 0-7)", who, i);
    HIP_TRY(hipSetDevice(f->ctx->device));
    { const int rc = order_on_own_stream(f); if (rc != RTR_OK) return rc; }
    hipStream_t st = f->ctx->stream;
    uint32_t* sh = f->image_ptr(RTR_IMAGE_SHADOWED); uint32_t* un = f->image_ptr(RTR_IMAGE_UNSHADOWED);
    uint32_t* dsh = f->image_ptr(RTR_IMAGE_DENOISED_SHADOWED); uint32_t* dun = f->image_ptr(RTR_IMAGE_DENOISED_UNSHADOWED);
    const uint32_t* nrm = f->image_ptr(RTR_IMAGE_NORMAL); const uint32_t* pos = f->image_ptr(RTR_IMAGE_POSITION);
    int denoisingOutput = 1;                                            /* application.cppm:392 */
    for (int i = 0; i < iterations; ++i) {
        const int step = (i + 1) * 1;                                   /* (i + 1) * DENOISING_STRENGTH */
        hipError_t e;
        if (denoisingOutput == 1) {
            e = rtrdev::launch_denoise_pair(un, dun, sh, dsh, nrm, pos, f->width, f->rows, step, 1.0f, 0.001f, 0.001f, st);
        } else {
            e = rtrdev::launch_denoise_pair(dun, un, dsh, sh, nrm, pos, f->width, f->rows, step, 1.0f, 0.001f, 0.001f, st);
        }
        if (e != hipSuccess) return fail(RTR_ERR_HIP, "denoise launch: %s", hipGetErrorString(e));
        denoisingOutput = 1 - denoisingOutput;
    }
    hipError_t e = rtrdev::launch_combine(f->image_ptr(RTR_IMAGE_ANALYTIC), denoisingOutput == 0 ? sh : dsh, denoisingOutput == 0 ? un : dun,
                                          f->image_ptr(RTR_IMAGE_FINAL), f->width, f->rows, st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "combine launch: %s", hipGetErrorString(e));
    return RTR_OK;
}

int rtr_denoise_combine(rtr_frame* f, int iterations) {
    const int rc = enqueue_denoise_combine(f, iterations, "rtr_denoise_combine");
    if (rc != RTR_OK) return rc;
    HIP_TRY(hipStreamSynchronize(f->ctx->stream));
    return RTR_OK;
}

int rtr_denoise_combine_async(rtr_frame* f, int iterations) {
    return enqueue_denoise_combine(f, iterations, "rtr_denoise_combine_async");     /* rtr_frame_wait joins */
}

int rtr_deinterleave_bands(rtr_ctx* ctx, const void* gathered, void* dst, uint32_t width, uint32_t height, uint32_t bandRows, uint32_t shardCount) {
    if (!ctx || !gathered || !dst || width == 0 || height == 0) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_deinterleave_bands: bad argument");
    if (bandRows == 0) bandRows = 8;
    if (shardCount == 0) shardCount = 1;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint32_t localRows = rtr_shard_rows(height, bandRows, shardCount);
    hipError_t e = rtrdev::launch_deinterleave((const uint32_t*)gathered, (uint32_t*)dst, width, height, bandRows, shardCount, localRows, ctx->stream);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "deinterleave launch: %s", hipGetErrorString(e));
    return RTR_OK;   /* enqueued on the ctx stream; the caller synchronises (stream order is enough for a following copy) */
}

int rtr_deinterleave_images(rtr_ctx* ctx, const void* gathered, uint32_t numImages, void* const* dst, uint32_t width, uint32_t height,
                            uint32_t bandRows, uint32_t shardCount) {
    if (!ctx || !gathered || !dst || width == 0 || height == 0) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_deinterleave_images: bad argument");
    if (numImages == 0 || numImages > rtrdev::kMaxDeinterleaveImages) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_deinterleave_images: %u images, 1 to %u", numImages, rtrdev::kMaxDeinterleaveImages);
    for (uint32_t i = 0; i < numImages; ++i) if (!dst[i]) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_deinterleave_images: destination %u is null", i);
    if (bandRows == 0) bandRows = 8;
    if (bandRows % 8u) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_deinterleave_images: bandRows %u is not a multiple of 8", bandRows);
    if (shardCount == 0) shardCount = 1;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint32_t localRows = rtr_shard_rows(height, bandRows, shardCount);
    uint32_t* d[rtrdev::kMaxDeinterleaveImages];
    for (uint32_t i = 0; i < numImages; ++i) d[i] = static_cast<uint32_t*>(dst[i]);
    hipError_t e = rtrdev::launch_deinterleave_images(static_cast<const uint32_t*>(gathered), d, numImages, width, height, bandRows, shardCount, localRows, ctx->stream);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "deinterleave launch: %s", hipGetErrorString(e));
    return RTR_OK;   /* enqueued on the ctx stream, like rtr_deinterleave_bands */
}

#ifdef RTR_TEST_HOOKS
/* librtr_hip_test.so only: what the loaded code object says of the binned queue build, k_shadow_gen_oct<single> (spp == 1) or <false> —
 * out[0] VGPRs, out[1] private-segment bytes per lane, out[2] static LDS bytes, out[3] the launch bound.  Register and scratch figures
 * only: the spp == 1 form is meant to have no private segment at its eight waves per SIMD (tests/test_gpu_gen_oct_scratch.py). */
int rtr_test_gen_oct_attributes(int single, uint32_t out[4]) {
    if (!out) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_test_gen_oct_attributes: null output");
    hipFuncAttributes a{};
    HIP_TRY(rtrdev::gen_oct_attributes(single != 0, &a));
    out[0] = (uint32_t)a.numRegs; out[1] = (uint32_t)a.localSizeBytes; out[2] = (uint32_t)a.sharedSizeBytes; out[3] = (uint32_t)a.maxThreadsPerBlock;
    return RTR_OK;
}
#endif

}  // extern "C"
