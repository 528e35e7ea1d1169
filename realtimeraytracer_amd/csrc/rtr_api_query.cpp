/* rtr_api_query.cpp — the ray queries of the C ABI in include/rtr.h: rtr_trace_rays and its masked, multi-hit and queued-occlusion
 * forms, rtr_hit_surfaces, the triangle -> leaf table and rtr_hit_leaves, rtr_camera_rays_async (rtr_api_internal.h has what the ABI's
 * files share).  They read the scene and never write its tree. */
#include "../../include/rtr.h"
#include "kernels/rtr_kernels.h"
#include "kernels/rtr_query.h"
#include "rtr_api_internal.h"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

using namespace rtrapi;

/* ---- ray queries ---------------------------------------------------------------------------- */
bool rtrapi::aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
bool rtrapi::aligned4(const void* p) { return ((uintptr_t)p & 3u) == 0; }

/* the handles every call of this section takes, and the device they must share */
int rtrapi::check_handles(const rtr_ctx* c, const rtr_scene* s, const char* who) {
    if (!c || !s) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null context or scene", who);
    return RTR_OK;
}
int rtrapi::check_same_device(const rtr_ctx* c, const rtr_scene* s, const char* who) {
    if (s->ctx->device != c->device) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: the scene lives on device %d, the context on device %d", who, s->ctx->device, c->device);
    return RTR_OK;
}
/* a synchronous call joins the context's stream when its asynchronous form (rc) enqueued something */
int rtrapi::join_if_enqueued(rtr_ctx* c, int rc, uint32_t n) {
    if (rc != RTR_OK || n == 0) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RTR_OK;
}

extern "C" {

/* the context's query scratch, allocated by its first query (the current device is the context's) */
static int query_scratch(rtr_ctx* c) {
    if (c->qCtrl.p) return RTR_OK;
    HIP_TRY(c->qRedo.alloc(rtrdev::kQueryRedoCap));
    HIP_TRY(c->qSpill.alloc(rtrdev::kSpillInts));
    HIP_TRY(c->qCounters.alloc(1));
    for (hipEvent_t& e : c->qEv) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(c->qCtrl.alloc(rtrdev::kQueryCtrlWords));
    return RTR_OK;
}

/* Every query that walks rays (rtr_trace_rays, rtr_trace_rays_multi, rtr_trace_occlusion and their forms) goes through that scratch the
 * same way: scratch_open, its own memsets, qEv[0], its launches, scratch_close; the counting form reads back in query_join. */

/* entries of a redo list of cap entries the query may use: all of them, or in the test build a list short enough to overflow */
static uint32_t redo_cap(uint32_t cap) {
#ifdef RTR_TEST_HOOKS
    if (const char* e = getenv("RTR_QUERY_REDO_CAP")) { const uint64_t v = strtoull(e, nullptr, 10); if (v >= 1 && v < cap) cap = (uint32_t)v; }
#endif
    return cap;
}

/* The scratch is the context's — redo list, deep stacks, counters, events — so a query enqueued on another stream than the last one
 * (rtr_ctx_set_stream) comes behind it.  count: the counting form, whose counters start at zero. */
static int scratch_open(rtr_ctx* c, bool count) {
    HIP_TRY(hipSetDevice(c->device));
    if (const int rc = query_scratch(c)) return rc;
    hipStream_t st = c->stream;
    if (c->qLastStream && c->qLastStream != st) HIP_TRY(hipStreamWaitEvent(st, c->qEv[1], 0));
    if (count) HIP_TRY(hipMemsetAsync(c->qCounters.p, 0, sizeof(Counters), st));
    return RTR_OK;
}

/* launch: what the query's launcher returned */
static int scratch_close(rtr_ctx* c, hipError_t launch, const char* who) {
    if (const int rc = launched(launch, who)) return rc;
    hipStream_t st = c->stream;
    HIP_TRY(hipEventRecord(c->qEv[1], st));
    c->qLastStream = st;
    return RTR_OK;
}

/* the cull mask of the masked calls: NoMask for the unmasked ones, which launch the kernels' unmasked forms */
struct CullMask { bool masked; const uint8_t* rayMasks; uint32_t cullMask; };
static const CullMask NoMask{false, nullptr, 0xffu};

/* the flags argument of every query entry point: the known bits, and the combinations Vulkan forbids (VUID-RayFlags: one face flag at
 * most; one of Opaque, CullOpaque, CullNoOpaque at most) */
static const uint32_t kQueryCullFlags = RTR_QUERY_CULL_BACK_FACING | RTR_QUERY_CULL_FRONT_FACING | RTR_QUERY_CULL_OPAQUE | RTR_QUERY_CULL_NO_OPAQUE;
static int check_query_flags(uint32_t flags, const char* who) {
    const uint32_t known = RTR_QUERY_ANY | RTR_QUERY_OPAQUE | kQueryCullFlags;
    if (flags & ~known) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: unknown flag bits 0x%x", who, flags & ~known);
    if ((flags & RTR_QUERY_CULL_BACK_FACING) && (flags & RTR_QUERY_CULL_FRONT_FACING))
        return fail(RTR_ERR_INVALID_ARGUMENT, "%s: flags RTR_QUERY_CULL_BACK_FACING and RTR_QUERY_CULL_FRONT_FACING exclude each other", who);
    const uint32_t op = flags & (RTR_QUERY_OPAQUE | RTR_QUERY_CULL_OPAQUE | RTR_QUERY_CULL_NO_OPAQUE);
    if (op & (op - 1u))
        return fail(RTR_ERR_INVALID_ARGUMENT, "%s: flags%s%s%s exclude each other (at most one of RTR_QUERY_OPAQUE, RTR_QUERY_CULL_OPAQUE, RTR_QUERY_CULL_NO_OPAQUE)", who,
                    (op & RTR_QUERY_OPAQUE) ? " RTR_QUERY_OPAQUE" : "", (op & RTR_QUERY_CULL_OPAQUE) ? " RTR_QUERY_CULL_OPAQUE" : "",
                    (op & RTR_QUERY_CULL_NO_OPAQUE) ? " RTR_QUERY_CULL_NO_OPAQUE" : "");
    return RTR_OK;
}
/* what the kernels get: a call with culling flags launches the MASKED forms — with the mask 0xff and no per-ray bytes when it brought no
 * cull mask — and hands them the flags beside the selecting bit; a call without launches what it always did */
static rtrdev::RayMaskArgs ray_mask_args(const CullMask& cm, uint32_t flags) {
    rtrdev::RayMaskArgs rm;
    const uint32_t cull = flags & kQueryCullFlags;
    rm.rayMasks = cm.masked ? cm.rayMasks : nullptr; rm.cullMask = cm.masked ? cm.cullMask : 0xffu;
    rm.masked = (cm.masked || cull) ? (1u | cull) : 0u;
    return rm;
}

/* what the three kinds of query check first, in this order: the handles, the cull mask's range, the flags */
static int check_query(const rtr_ctx* c, const rtr_scene* s, const CullMask& cm, uint32_t flags, const char* who) {
    if (const int rc = check_handles(c, s, who)) return rc;
    if (cm.masked && (cm.cullMask & ~0xffu)) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: cullMask 0x%x has bits above the low 8 (an instance mask is 8 bits)", who, cm.cullMask);
    return check_query_flags(flags, who);
}

/* the checks and launches of rtr_trace_rays[_async], enqueued on the context's stream; count: the counting form */
static int enqueue_query(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, uint32_t n, uint32_t flags, RtrHit* hits, uint8_t* occluded,
                         bool count, const char* who, const CullMask& cm = NoMask) {
    if (const int rc = check_query(c, s, cm, flags, who)) return rc;
    if (const int rc = check_same_device(c, s, who)) return rc;
    if (n == 0) return RTR_OK;
    const bool any = (flags & RTR_QUERY_ANY) != 0u;
    if (!rays) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: rays is null", who);
    if (!aligned16(rays)) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: rays is not 16-B aligned", who);
    if (!any && !hits) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: a closest-hit query needs hits", who);
    if (!any && !aligned16(hits)) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: hits is not 16-B aligned", who);
    if (any && !occluded) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: an any-hit query (RTR_QUERY_ANY) needs occluded", who);
    if (any && !aligned16(occluded)) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: occluded is not 16-B aligned", who);
    if (const int rc = scratch_open(c, count)) return rc;
    hipStream_t st = c->stream;
    HIP_TRY(hipMemsetAsync(c->qCtrl.p, 0, rtrdev::kQueryCtrlWords * sizeof(uint32_t), st));
    HIP_TRY(hipEventRecord(c->qEv[0], st));
    rtrdev::QueryArgs qa{};
    qa.rays = reinterpret_cast<const float4*>(rays); qa.hits = reinterpret_cast<float4*>(hits); qa.occluded = occluded; qa.n = n;
    qa.redoCap = redo_cap(rtrdev::kQueryRedoCap); qa.ctrl = c->qCtrl.p; qa.redoList = c->qRedo.p; qa.spill = c->qSpill.p;
    const rtrdev::RayMaskArgs rm = ray_mask_args(cm, flags);
    return scratch_close(c, rtrdev::launch_query(s->dev, qa, flags & (RTR_QUERY_ANY | RTR_QUERY_OPAQUE), count ? c->qCounters.p : nullptr, st, rm), who);
}

/* ---- queued occlusion queries (kernels/rtr_occlusion.hip): the layout of the caller's scratch ---- */
namespace {
/* the caller's scratch: control block (zeroed with the count of abandoned rays behind it) | abandoned rays' list | index queue | batch lists */
struct OcclusionLayout { size_t ctrl, overflow, queue, lists, bytes; uint32_t overflowCap, listStride; };
size_t up16(size_t x) { return (x + 15u) & ~(size_t)15u; }
OcclusionLayout occlusion_layout(uint32_t n) {
    OcclusionLayout l{};
    l.overflowCap = n < rtrdev::kQueryRedoCap ? n : rtrdev::kQueryRedoCap;
    l.listStride = rtrdev::occlusion_list_stride(n);
    l.ctrl = 0;
    l.overflow = up16(rtrdev::kQueueCtrlWords * sizeof(uint32_t));
    l.queue = l.overflow + up16(((size_t)l.overflowCap + 1u) * sizeof(uint32_t));
    l.lists = l.queue + up16((size_t)n * sizeof(uint32_t));
    l.bytes = l.lists + up16((size_t)rtrdev::kQueueLists * l.listStride * sizeof(uint2));
    return l;
}
}  // namespace

/* What a synchronous query does behind its asynchronous form (rc: what that returned): it joins the context's stream, and the counting
 * form reads back the counters, the count of abandoned rays and the time between the two events — copies on the context's stream, so the
 * call joins that stream only.  occlusionScratch: the caller's scratch of a queued occlusion query, which keeps that count behind its
 * control block; null: the count is the context's control word. */
static int query_join(rtr_ctx* c, int rc, uint32_t n, rtr_query_stats* stats, const void* occlusionScratch = nullptr) {
    if (rc != RTR_OK) return rc;
    if (stats) memset(stats, 0, sizeof *stats);
    if (n == 0) return RTR_OK;
    hipStream_t st = c->stream;
    if (stats) {
        Counters h;
        uint32_t tail = 0;
        const void* tailWord = c->qCtrl.p + rtrdev::kQueryRedoWord;
        if (occlusionScratch) tailWord = static_cast<const char*>(occlusionScratch) + occlusion_layout(n).overflow;
        HIP_TRY(hipMemcpyAsync(&h, c->qCounters.p, sizeof h, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&tail, tailWord, sizeof tail, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        stats->numRays = h.rays; stats->numNodeVisits = h.nodes; stats->numTriTests = h.tris; stats->numAlphaTests = h.alphaTests;
        stats->tailRays = tail;
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c->qEv[0], c->qEv[1]));
        stats->ms = ms;
    } else HIP_TRY(hipStreamSynchronize(st));
    return RTR_OK;
}

int rtr_trace_rays_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, uint32_t n, uint32_t flags, RtrHit* hits, uint8_t* occluded) {
    return enqueue_query(c, s, rays, n, flags, hits, occluded, false, "rtr_trace_rays_async");
}

int rtr_trace_rays(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, uint32_t n, uint32_t flags, RtrHit* hits, uint8_t* occluded, rtr_query_stats* stats) {
    return query_join(c, enqueue_query(c, s, rays, n, flags, hits, occluded, stats != nullptr, "rtr_trace_rays"), n, stats);
}

int rtr_trace_rays_masked_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const uint8_t* rayMasks, uint32_t n, uint32_t flags, uint32_t cullMask,
                                RtrHit* hits, uint8_t* occluded) {
    return enqueue_query(c, s, rays, n, flags, hits, occluded, false, "rtr_trace_rays_masked_async", CullMask{true, rayMasks, cullMask});
}

int rtr_trace_rays_masked(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const uint8_t* rayMasks, uint32_t n, uint32_t flags, uint32_t cullMask,
                          RtrHit* hits, uint8_t* occluded, rtr_query_stats* stats) {
    return query_join(c, enqueue_query(c, s, rays, n, flags, hits, occluded, stats != nullptr, "rtr_trace_rays_masked", CullMask{true, rayMasks, cullMask}), n, stats);
}

/* ---- multi-hit queries (kernels/rtr_multihit.hip) ---- */
/* the checks and launches of rtr_trace_rays_multi[_async], enqueued on the context's stream; count: the counting form.  The flag and mask
 * validation is the masked query's; the kernels have the filtered form only, so the call always brings a cull mask. */
static int enqueue_multihit(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const uint8_t* rayMasks, uint32_t n, uint32_t maxHits, uint32_t flags,
                            uint32_t cullMask, const RtrHit* after, RtrHit* hits, uint32_t* counts, bool count, const char* who) {
    const CullMask cm{true, rayMasks, cullMask};
    if (const int rc = check_query(c, s, cm, flags, who)) return rc;
    if (flags & RTR_QUERY_ANY) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: RTR_QUERY_ANY is refused: an any-hit walk has no order to report hits in", who);
    if (maxHits == 0u || maxHits > RTR_MULTIHIT_MAX) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: maxHits %u, 1 to %u", who, maxHits, RTR_MULTIHIT_MAX);
    if (const int rc = check_same_device(c, s, who)) return rc;
    if (n == 0) return RTR_OK;
    const Arg args[4] = {{rays, "rays", 16, true}, {hits, "hits", 16, true}, {after, "after", 16, false}, {counts, "counts", 4, false}};
    if (const int rc = check_ptrs(who, args)) return rc;
    if (const int rc = scratch_open(c, count)) return rc;
    hipStream_t st = c->stream;
    HIP_TRY(hipMemsetAsync(c->qCtrl.p, 0, rtrdev::kQueryCtrlWords * sizeof(uint32_t), st));
    HIP_TRY(hipEventRecord(c->qEv[0], st));
    rtrdev::MultiHitArgs ma{};
    ma.rays = reinterpret_cast<const float4*>(rays); ma.after = reinterpret_cast<const float4*>(after); ma.hits = reinterpret_cast<float4*>(hits);
    ma.counts = counts; ma.n = n; ma.maxHits = maxHits;
    ma.redoCap = redo_cap(rtrdev::kQueryRedoCap); ma.ctrl = c->qCtrl.p; ma.redoList = c->qRedo.p; ma.spill = c->qSpill.p;
    const rtrdev::RayMaskArgs rm = ray_mask_args(cm, flags);
    return scratch_close(c, rtrdev::launch_multihit(s->dev, ma, (flags & RTR_QUERY_OPAQUE) == 0u, count ? c->qCounters.p : nullptr, st, rm), who);
}

int rtr_trace_rays_multi_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const uint8_t* rayMasks, uint32_t n, uint32_t maxHits, uint32_t flags,
                               uint32_t cullMask, const RtrHit* after, RtrHit* hits, uint32_t* counts) {
    return enqueue_multihit(c, s, rays, rayMasks, n, maxHits, flags, cullMask, after, hits, counts, false, "rtr_trace_rays_multi_async");
}

int rtr_trace_rays_multi(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const uint8_t* rayMasks, uint32_t n, uint32_t maxHits, uint32_t flags,
                         uint32_t cullMask, const RtrHit* after, RtrHit* hits, uint32_t* counts, rtr_query_stats* stats) {
    return query_join(c, enqueue_multihit(c, s, rays, rayMasks, n, maxHits, flags, cullMask, after, hits, counts, stats != nullptr, "rtr_trace_rays_multi"), n, stats);
}

/* ---- queued occlusion queries (kernels/rtr_occlusion.hip) ---- */
int rtr_occlusion_scratch_bytes(uint32_t numRays, size_t* bytes) {
    if (!bytes) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_occlusion_scratch_bytes: bytes is null");
    *bytes = occlusion_layout(numRays).bytes;
    return RTR_OK;
}

/* startLeaves: the hints of rtr_trace_occlusion_hinted (null: none; the unhinted calls pass null) */
static int enqueue_occlusion(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const int32_t* startLeaves, uint32_t n, uint32_t flags, void* scratch,
                             size_t scratchBytes, uint8_t* occluded, bool count, const char* who, const CullMask& cm = NoMask) {
    if (n && !aligned4(startLeaves)) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: startLeaves is not 4-B aligned", who);
    if (const int rc = check_query(c, s, cm, flags, who)) return rc;
    if (const int rc = check_same_device(c, s, who)) return rc;
    if (n == 0) return RTR_OK;
    const Arg args[3] = {{rays, "rays", 16, true}, {occluded, "occluded", 16, true}, {scratch, "scratch", 16, true}};
    if (const int rc = check_ptrs(who, args)) return rc;
    const OcclusionLayout l = occlusion_layout(n);
    if (scratchBytes < l.bytes) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: %zu bytes of scratch, %u rays need %zu (rtr_occlusion_scratch_bytes)", who, scratchBytes, n, l.bytes);
    if (const int rc = scratch_open(c, count)) return rc;      /* the deep stacks and the counters are the context's */
    hipStream_t st = c->stream;
    char* const base = static_cast<char*>(scratch);
    HIP_TRY(hipMemsetAsync(base + l.ctrl, 0, l.overflow + 16u, st));       /* the control block and the count of abandoned rays */
    HIP_TRY(hipMemsetAsync(occluded, 0, n, st));                           /* the walk stores the occluded rays' bytes only */
    HIP_TRY(hipEventRecord(c->qEv[0], st));
    rtrdev::OcclusionArgs oa{};
    oa.rays = reinterpret_cast<const float4*>(rays); oa.occluded = occluded; oa.n = n; oa.batch = rtrdev::occlusion_batch(n);
    oa.ctrl = reinterpret_cast<uint32_t*>(base + l.ctrl); oa.overflow = reinterpret_cast<uint32_t*>(base + l.overflow); oa.overflowCap = redo_cap(l.overflowCap);
    oa.queue = reinterpret_cast<uint32_t*>(base + l.queue); oa.lists = reinterpret_cast<uint2*>(base + l.lists); oa.listStride = l.listStride;
    oa.startLeaves = startLeaves; oa.numTris = (uint32_t)(s->tree.tris.n / 3);          /* a hint is checked against the records the scene holds */
    const rtrdev::RayMaskArgs rm = ray_mask_args(cm, flags);
    return scratch_close(c, rtrdev::launch_occlusion(s->dev, oa, c->tun, (flags & RTR_QUERY_OPAQUE) == 0u, c->qSpill.p, count ? c->qCounters.p : nullptr, st,
                                                     (uint32_t)c->prop.multiProcessorCount, rm), who);
}

int rtr_trace_occlusion_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, uint32_t n, uint32_t flags, void* scratch, size_t scratchBytes, uint8_t* occluded) {
    return enqueue_occlusion(c, s, rays, nullptr, n, flags, scratch, scratchBytes, occluded, false, "rtr_trace_occlusion_async");
}

int rtr_trace_occlusion_hinted_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const int32_t* startLeaves, uint32_t n, uint32_t flags, void* scratch,
                                     size_t scratchBytes, uint8_t* occluded) {
    return enqueue_occlusion(c, s, rays, startLeaves, n, flags, scratch, scratchBytes, occluded, false, "rtr_trace_occlusion_hinted_async");
}

int rtr_trace_occlusion_masked_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const int32_t* startLeaves, const uint8_t* rayMasks, uint32_t n,
                                     uint32_t flags, uint32_t cullMask, void* scratch, size_t scratchBytes, uint8_t* occluded) {
    return enqueue_occlusion(c, s, rays, startLeaves, n, flags, scratch, scratchBytes, occluded, false, "rtr_trace_occlusion_masked_async", CullMask{true, rayMasks, cullMask});
}

int rtr_trace_occlusion_masked(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const int32_t* startLeaves, const uint8_t* rayMasks, uint32_t n,
                               uint32_t flags, uint32_t cullMask, void* scratch, size_t scratchBytes, uint8_t* occluded, rtr_query_stats* stats) {
    return query_join(c, enqueue_occlusion(c, s, rays, startLeaves, n, flags, scratch, scratchBytes, occluded, stats != nullptr, "rtr_trace_occlusion_masked",
                                           CullMask{true, rayMasks, cullMask}), n, stats, scratch);
}

int rtr_trace_occlusion(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, uint32_t n, uint32_t flags, void* scratch, size_t scratchBytes, uint8_t* occluded,
                        rtr_query_stats* stats) {
    return query_join(c, enqueue_occlusion(c, s, rays, nullptr, n, flags, scratch, scratchBytes, occluded, stats != nullptr, "rtr_trace_occlusion"), n, stats, scratch);
}

int rtr_trace_occlusion_hinted(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const int32_t* startLeaves, uint32_t n, uint32_t flags, void* scratch,
                               size_t scratchBytes, uint8_t* occluded, rtr_query_stats* stats) {
    return query_join(c, enqueue_occlusion(c, s, rays, startLeaves, n, flags, scratch, scratchBytes, occluded, stats != nullptr, "rtr_trace_occlusion_hinted"), n, stats, scratch);
}

/* the checks and the launch of rtr_hit_surfaces[_async], enqueued on the context's stream */
static int enqueue_surfaces(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, RtrSurface* out, const char* who) {
    if (const int rc = check_handles(c, s, who)) return rc;
    if (const int rc = check_same_device(c, s, who)) return rc;
    if (n == 0) return RTR_OK;
    const Arg args[3] = {{rays, "rays", 16, true}, {hits, "hits", 16, true}, {out, "out", 16, true}};
    if (const int rc = check_ptrs(who, args)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    rtrdev::SurfaceArgs sa{};
    sa.rays = reinterpret_cast<const float4*>(rays); sa.hits = reinterpret_cast<const float4*>(hits); sa.out = reinterpret_cast<float4*>(out);
    sa.triCount = s->triCount.p; sa.numInstances = s->numInstances; sa.n = n;
    return launched(rtrdev::launch_hit_surfaces(s->dev, sa, c->stream), who);
}

int rtr_hit_surfaces_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, RtrSurface* out) {
    return enqueue_surfaces(c, s, rays, hits, n, out, "rtr_hit_surfaces_async");
}

int rtr_hit_surfaces(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, RtrSurface* out) {
    return join_if_enqueued(c, enqueue_surfaces(c, s, rays, hits, n, out, "rtr_hit_surfaces"), n);
}

/* ---- start hints: the triangle -> leaf table (kernels/rtr_query.hip: k_leaf_table) ---- */
/* Made by the first call that needs it, on the calling context's stream (the current device is the scene's), and JOINED before the call
 * goes on: whichever context of the device asks next finds it complete, without an event to wait for.  rtr_scene_update_instances
 * keeps it (a refit moves boxes and records, not the leaves they sit in). */
extern "C++" int rtrapi::ensure_leaf_table(rtr_ctx* c, const rtr_scene* s, const char* who) {
    const SceneTree& t = s->tree;
    if (t.leafReady) return RTR_OK;
    { const int rcm = refresh_mirrors(s); if (rcm != RTR_OK) return rcm; }      /* joins an enqueued refit: this kernel may run on another stream */
    std::vector<uint32_t> base(s->hostTriCount.size() + 1, 0u);
    uint64_t total = 0;
    for (size_t i = 0; i < s->hostTriCount.size(); ++i) { base[i] = (uint32_t)total; total += s->hostTriCount[i]; }
    if (total > 0xffffffffull) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: %llu (customIndex, primitiveId) pairs do not fit the leaf table's 32-bit index", who, (unsigned long long)total);
    hipStream_t st = c->stream;
    HIP_TRY(s->leafBase.upload(base.data(), base.size(), st));
    HIP_TRY(t.leafTable.alloc((size_t)total));
    HIP_TRY(hipMemsetAsync(t.leafTable.p, 0, t.leafTable.n * sizeof(int32_t), st));
    const hipError_t e = rtrdev::launch_leaf_table(t.nodes.p, (uint32_t)(t.nodes.n / 2), t.tris.p, (uint32_t)(t.tris.n / 3), s->triCount.p, s->leafBase.p,
                                                   s->numInstances, t.leafTable.p, st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: leaf table: %s", who, hipGetErrorString(e));
    HIP_TRY(hipStreamSynchronize(st));
    t.leafReady = true;
    return RTR_OK;
}

/* the checks and the launch of rtr_hit_leaves[_async].  The pointers are checked first: that needs nothing of the handles */
static int enqueue_hit_leaves(rtr_ctx* c, const rtr_scene* s, const RtrHit* hits, uint32_t n, int32_t* leaves, const char* who) {
    const Arg args[2] = {{hits, "hits", 16, true}, {leaves, "leaves", 4, true}};
    if (const int rc = n ? check_ptrs(who, args) : RTR_OK) return rc;
    if (const int hrc = check_handles(c, s, who)) return hrc;
    if (const int drc = check_same_device(c, s, who)) return drc;
    if (n == 0) return RTR_OK;
    HIP_TRY(hipSetDevice(c->device));
    const int rc = ensure_leaf_table(c, s, who);
    if (rc != RTR_OK) return rc;
    rtrdev::LeafArgs a{};
    a.hits = reinterpret_cast<const float4*>(hits); a.leaves = leaves; a.triCount = s->triCount.p; a.base = s->leafBase.p; a.table = s->tree.leafTable.p;
    a.numInstances = s->numInstances; a.n = n;
    return launched(rtrdev::launch_hit_leaves(a, c->stream), who);
}

int rtr_hit_leaves_async(rtr_ctx* c, const rtr_scene* s, const RtrHit* hits, uint32_t n, int32_t* leaves) {
    return enqueue_hit_leaves(c, s, hits, n, leaves, "rtr_hit_leaves_async");
}

int rtr_hit_leaves(rtr_ctx* c, const rtr_scene* s, const RtrHit* hits, uint32_t n, int32_t* leaves) {
    return join_if_enqueued(c, enqueue_hit_leaves(c, s, hits, n, leaves, "rtr_hit_leaves"), n);
}

int rtr_camera_rays_async(rtr_ctx* c, const RtrCameraData* cam, uint32_t width, uint32_t height, uint32_t spp, RtrRay* out) {
    if (!c || !cam || !out) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_camera_rays_async: null argument");
    if (!aligned16(out)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_camera_rays_async: out is not 16-B aligned");
    if (width == 0 || height == 0 || spp == 0) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_camera_rays_async: extent %ux%u x %u spp", width, height, spp);
    if ((uint64_t)width * height * spp > 0xffffffffull) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_camera_rays_async: %ux%u x %u spp is more than 2^32 - 1 rays", width, height, spp);
    HIP_TRY(hipSetDevice(c->device));
    return launched(rtrdev::launch_camera_rays(*cam, width, height, spp, reinterpret_cast<float4*>(out), c->stream), "rtr_camera_rays_async");
}

}  // extern "C"
