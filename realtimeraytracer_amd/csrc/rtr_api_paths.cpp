/* rtr_api_paths.cpp — the path-vertex calls of the C ABI in include/rtr.h: direct lighting and the tone map, continuation rays,
 * compaction, accumulation and the record gather, picked light samples, MIS and the sky, and rtr_scene_export_light_tris (rtr_api_internal.h has what the ABI's files
 * share).  They read the scene and never write its tree. */
#include "../../include/rtr.h"
#include "kernels/rtr_kernels.h"
#include "kernels/rtr_query.h"
#include "kernels/rtr_bounce_launch.h"
#include "rtr_bounce_host.h"
#include "kernels/rtr_paths_launch.h"
#include "rtr_paths_host.h"
#include "kernels/rtr_accum_launch.h"
#include "rtr_accum_host.h"
#include "rtr_pick_host.h"
#include "kernels/rtr_mis_launch.h"
#include "rtr_mis_host.h"
#include "kernels/rtr_sky_launch.h"
#include "rtr_sky_host.h"
#include "rtr_api_internal.h"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

using namespace rtrapi;

extern "C" {

/* ---- direct lighting for ray-query hits -------------------------------------------------------------------------------------- */

/* Q of rtr_light_slots, from the host copy of the light table (as enqueue_render counts maxRaysPerSample) */
static int light_slots(const rtr_scene* s, const rtr_light_params* p, uint32_t* q, const char* who) {
    if (!s || !p) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null scene or params", who);
    if (p->numAreaLights > s->numLights) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: numAreaLights %u > scene lights %u", who, p->numAreaLights, s->numLights);
    if (const int rc = rtrdev::check_shadow_rays(who, p->numShadowRays)) return rc;
    if (const int rc = rtrdev::check_light_outputs(who, p->outputs)) return rc;
    uint64_t slots = 1;
    for (uint32_t l = 0; l < p->numAreaLights; ++l) slots += (uint64_t)s->hostLights[l].numTriangles * p->numShadowRays;
    if (slots > 0xffffffffull) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: %llu slots per hit do not fit 32 bits", who, (unsigned long long)slots);
    *q = (uint32_t)slots;
    return RTR_OK;
}

int rtr_light_slots(const rtr_scene* s, const rtr_light_params* p, uint32_t* slotsPerHit) {
    if (!slotsPerHit) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_light_slots: slotsPerHit is null");
    return light_slots(s, p, slotsPerHit, "rtr_light_slots");
}

/* what every lighting launch takes of the call alike; slots, the output arrays, the hint fields and the test hook are the caller's */
static void fill_light_args(rtrdev::LightArgs& la, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                            const uint32_t* seeds) {
    la.rays = reinterpret_cast<const float4*>(rays); la.hits = reinterpret_cast<const float4*>(hits); la.seeds = seeds;
    la.triCount = s->triCount.p; la.numInstances = s->numInstances; la.n = n;
    la.numAreaLights = p->numAreaLights; la.numShadowRays = p->numShadowRays; la.frame = p->frame; la.width = p->width; la.spp = p->spp;
    la.outputs = p->outputs;
}

/* the checks and the launch of rtr_light_rays[_async] (shade == false) and rtr_shade_hits[_async], enqueued on the context's stream */
static int enqueue_light(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                         const uint32_t* seeds, RtrRay* outRays, const uint8_t* occluded, RtrRadiance* out, bool shade, const char* who,
                         int32_t* outLeaves = nullptr, bool hinted = false) {
    const Arg own[1] = {{outLeaves, "outLeaves", 4, true}};       /* rtr_light_rays_hinted: its own array is checked first, which needs nothing of the handles */
    if (const int rc = hinted && n ? check_ptrs(who, own) : RTR_OK) return rc;
    if (!c || !s || !p) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null context, scene or params", who);
    if (const int rc = check_same_device(c, s, who)) return rc;
    uint32_t slots = 0;
    if (const int rc = light_slots(s, p, &slots, who)) return rc;
    if (shade && (p->outputs & RTR_LIGHT_ANALYTIC) && !s->hasLtc) return fail(RTR_ERR_UNSUPPORTED, "%s: RTR_LIGHT_ANALYTIC needs the LTC tables (rtr_scene_desc.ltc1/ltc2)", who);
    if (n == 0) return RTR_OK;
    if (const int rc = rtrdev::check_fits_32(who, n, "hits", slots, "slots")) return rc;
    const Arg args[5] = {{rays, "rays", 16, true}, {hits, "hits", 16, true}, shade ? Arg{out, "out", 16, true} : Arg{outRays, "outRays", 16, true},
                         {occluded, "occluded", 1, shade}, {seeds, "seeds", 4, false}};
    if (const int rc = check_ptrs(who, args)) return rc;
    if (const int rc = rtrdev::check_pixel_seeds(who, seeds, p->width, p->spp)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (const int rc = hinted ? ensure_leaf_table(c, s, who) : RTR_OK) return rc;
    rtrdev::LightArgs la{};
    if (hinted) { la.outLeaves = outLeaves; la.leafTable = s->tree.leafTable.p; la.leafBase = s->leafBase.p; }
    fill_light_args(la, s, rays, hits, n, p, seeds);
    la.slots = slots;
    la.outRays = reinterpret_cast<float4*>(outRays); la.occluded = occluded; la.out = reinterpret_cast<float4*>(out);
#ifdef RTR_TEST_HOOKS
    if (const char* e = getenv("RTR_LIGHT_RAYS_DIRECT")) la.direct = atoi(e) != 0 ? 1u : 0u;   /* the kernel's unstaged form for a light table that would be staged */
#endif
    return launched(shade ? rtrdev::launch_shade_hits(s->dev, la, c->stream) : rtrdev::launch_light_rays(s->dev, la, c->stream), who);
}

int rtr_light_rays_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                         const uint32_t* seeds, RtrRay* outRays) {
    return enqueue_light(c, s, rays, hits, n, p, seeds, outRays, nullptr, nullptr, false, "rtr_light_rays_async");
}

int rtr_light_rays(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                   const uint32_t* seeds, RtrRay* outRays) {
    return join_if_enqueued(c, enqueue_light(c, s, rays, hits, n, p, seeds, outRays, nullptr, nullptr, false, "rtr_light_rays"), n);
}

int rtr_light_rays_hinted_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                                const uint32_t* seeds, RtrRay* outRays, int32_t* outLeaves) {
    return enqueue_light(c, s, rays, hits, n, p, seeds, outRays, nullptr, nullptr, false, "rtr_light_rays_hinted_async", outLeaves, true);
}

int rtr_light_rays_hinted(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                          const uint32_t* seeds, RtrRay* outRays, int32_t* outLeaves) {
    return join_if_enqueued(c, enqueue_light(c, s, rays, hits, n, p, seeds, outRays, nullptr, nullptr, false, "rtr_light_rays_hinted", outLeaves, true), n);
}

int rtr_shade_hits_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                         const uint32_t* seeds, const uint8_t* occluded, RtrRadiance* out) {
    return enqueue_light(c, s, rays, hits, n, p, seeds, nullptr, occluded, out, true, "rtr_shade_hits_async");
}

int rtr_shade_hits(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                   const uint32_t* seeds, const uint8_t* occluded, RtrRadiance* out) {
    return join_if_enqueued(c, enqueue_light(c, s, rays, hits, n, p, seeds, nullptr, occluded, out, true, "rtr_shade_hits"), n);
}

int rtr_tonemap_pack_async(rtr_ctx* c, const float* radiance, uint32_t strideBytes, uint32_t n, uint32_t* out) {
    if (!c) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_tonemap_pack: null context");
    if (strideBytes < 12 || (strideBytes & 3u)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_tonemap_pack: strideBytes %u (a multiple of 4, at least 12)", strideBytes);
    if (n == 0) return RTR_OK;
    const Arg args[2] = {{radiance, "radiance", 4, true}, {out, "outBGRA8", 4, true}};
    if (const int rc = check_ptrs("rtr_tonemap_pack", args)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return launched(rtrdev::launch_tonemap_pack(radiance, strideBytes / 4u, n, out, c->stream), "rtr_tonemap_pack");
}

int rtr_tonemap_pack(rtr_ctx* c, const float* radiance, uint32_t strideBytes, uint32_t n, uint32_t* out) {
    return join_if_enqueued(c, rtr_tonemap_pack_async(c, radiance, strideBytes, n, out), n);
}

/* ---- continuation rays for ray-query hits (kernels/rtr_bounce.hip; the host form is rtr_bounce_host.cpp) -------------------------- */
static int enqueue_bounce(rtr_ctx* c, const RtrRay* rays, const RtrSurface* surfaces, uint32_t n, const rtr_bounce_params* p, const uint32_t* seeds,
                          RtrRay* outRays, RtrBounce* outBounce, const char* who) {
    /* the arrays and the params are checked first, which needs nothing of the handle */
    if (const int rc = n ? rtrdev::bounce_check_args(who, rays, surfaces, n, p, seeds, outRays, outBounce) : RTR_OK) return rc;
    if (!c) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: ctx is null", who);
    if (n == 0) return RTR_OK;
    HIP_TRY(hipSetDevice(c->device));
    rtrdev::BounceArgs a{};
    a.rays = reinterpret_cast<const float4*>(rays); a.surfaces = reinterpret_cast<const float4*>(surfaces); a.seeds = seeds;
    a.outRays = reinterpret_cast<float4*>(outRays); a.outBounce = reinterpret_cast<float4*>(outBounce); a.params = *p; a.n = n;
    return launched(rtrdev::launch_bounce_rays(a, c->stream), who);
}

int rtr_bounce_rays_async(rtr_ctx* c, const RtrRay* rays, const RtrSurface* surfaces, uint32_t n, const rtr_bounce_params* p, const uint32_t* seeds,
                          RtrRay* outRays, RtrBounce* outBounce) {
    return enqueue_bounce(c, rays, surfaces, n, p, seeds, outRays, outBounce, "rtr_bounce_rays_async");
}

int rtr_bounce_rays(rtr_ctx* c, const RtrRay* rays, const RtrSurface* surfaces, uint32_t n, const rtr_bounce_params* p, const uint32_t* seeds,
                    RtrRay* outRays, RtrBounce* outBounce) {
    return join_if_enqueued(c, enqueue_bounce(c, rays, surfaces, n, p, seeds, outRays, outBounce, "rtr_bounce_rays"), n);
}

/* ---- compaction of live paths (kernels/rtr_paths.hip; the host form and the argument checks are rtr_paths_host.cpp) ----------------- */
static int enqueue_compact(rtr_ctx* c, const RtrRay* rays, const float* throughput, const uint32_t* seeds, const uint32_t* pathIds, uint32_t n,
                           const rtr_compact_params* p, void* scratch, size_t scratchBytes, RtrRay* outRays, float* outThroughput,
                           uint32_t* outSeeds, uint32_t* outPathIds, uint32_t* outCount, const char* who) {
    /* the arrays and the params are checked first, which needs nothing of the handle */
    const rtrdev::CompactCall call{rays, throughput, seeds, pathIds, n, p, scratch, scratchBytes, rtrdev::compact_scratch_bytes(n), true,
                                   outRays, outThroughput, outSeeds, outPathIds, outCount};
    if (const int rc = n ? rtrdev::compact_check_args(who, call) : RTR_OK) return rc;
    if (!c) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: ctx is null", who);
    if (n == 0 && !outCount) return RTR_OK;
    if (n == 0 && !aligned4(outCount)) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: outCount is not 4-B aligned", who);
    HIP_TRY(hipSetDevice(c->device));
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(outCount, 0, sizeof(uint32_t), c->stream));
        return RTR_OK;
    }
    const size_t groups = ((size_t)n + 255u) / 256u;
    rtrdev::CompactArgs a{};
    a.rays = reinterpret_cast<const float4*>(rays); a.throughput = reinterpret_cast<const char*>(throughput); a.seeds = seeds; a.pathIds = pathIds;
    a.ballots = static_cast<unsigned long long*>(scratch);
    a.groupTotals = reinterpret_cast<uint32_t*>(static_cast<char*>(scratch) + groups * 32u);
    a.outRays = reinterpret_cast<float4*>(outRays); a.outThroughput = outThroughput; a.outSeeds = outSeeds; a.outPathIds = outPathIds;
    a.outCount = outCount; a.params = *p; a.n = n;
    return launched(rtrdev::launch_compact_paths(a, c->stream), who);
}

int rtr_compact_paths_async(rtr_ctx* c, const RtrRay* rays, const float* throughput, const uint32_t* seeds, const uint32_t* pathIds, uint32_t n,
                            const rtr_compact_params* p, void* scratch, size_t scratchBytes, RtrRay* outRays, float* outThroughput,
                            uint32_t* outSeeds, uint32_t* outPathIds, uint32_t* outCount) {
    return enqueue_compact(c, rays, throughput, seeds, pathIds, n, p, scratch, scratchBytes, outRays, outThroughput, outSeeds, outPathIds, outCount,
                           "rtr_compact_paths_async");
}

int rtr_compact_paths(rtr_ctx* c, const RtrRay* rays, const float* throughput, const uint32_t* seeds, const uint32_t* pathIds, uint32_t n,
                      const rtr_compact_params* p, void* scratch, size_t scratchBytes, RtrRay* outRays, float* outThroughput,
                      uint32_t* outSeeds, uint32_t* outPathIds, uint32_t* outCount, uint32_t* hostCount) {
    const int rc = enqueue_compact(c, rays, throughput, seeds, pathIds, n, p, scratch, scratchBytes, outRays, outThroughput, outSeeds, outPathIds,
                                   outCount, "rtr_compact_paths");
    if (rc != RTR_OK) return rc;
    if (n == 0) {                        /* nothing was launched; the count's memset, when there is one, is joined like a launch */
        if (hostCount) *hostCount = 0u;
        if (outCount) HIP_TRY(hipStreamSynchronize(c->stream));
        return RTR_OK;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (hostCount) {                     /* on the context's stream, so that no other stream is joined */
        HIP_TRY(hipMemcpyAsync(hostCount, outCount, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return RTR_OK;
}

/* ---- accumulation of a vertex and the record gather (kernels/rtr_accum.hip; the rule is include/rtr_accum.h, the host forms and the argument checks rtr_accum_host.cpp) -- */
static int enqueue_accumulate(rtr_ctx* c, const RtrRadiance* radiance, const float* throughput, const uint32_t* pathIds, const RtrEmitter* emitters,
                              const RtrSkyEscape* escapes, const float* skySums, const RtrBounce* bounces, uint32_t n, const rtr_accum_params* p,
                              float* accum, float* outTerm, float* outThroughput, const char* who) {
    /* the arrays and the params are checked first, which needs nothing of the handle */
    const rtrdev::AccumCall call{radiance, throughput, pathIds, emitters, escapes, skySums, bounces, n, p, accum, outTerm, outThroughput};
    if (const int rc = n ? rtrdev::accum_check_args(who, call) : RTR_OK) return rc;
    if (!c) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: ctx is null", who);
    if (n == 0) return RTR_OK;
    HIP_TRY(hipSetDevice(c->device));
    rtrdev::AccumArgs a{};
    a.radiance = reinterpret_cast<const float4*>(radiance); a.throughput = reinterpret_cast<const char*>(throughput); a.pathIds = pathIds;
    a.emitters = reinterpret_cast<const float4*>(emitters); a.escapes = reinterpret_cast<const float4*>(escapes);
    a.skySums = reinterpret_cast<const float4*>(skySums); a.bounces = reinterpret_cast<const float4*>(bounces);
    a.accum = reinterpret_cast<char*>(accum); a.outTerm = reinterpret_cast<char*>(outTerm); a.outThroughput = outThroughput;
    a.params = *p; a.n = n;
    return launched(rtrdev::launch_accumulate_paths(a, c->stream), who);
}

int rtr_accumulate_paths_async(rtr_ctx* c, const RtrRadiance* radiance, const float* throughput, const uint32_t* pathIds, const RtrEmitter* emitters,
                               const RtrSkyEscape* escapes, const float* skySums, const RtrBounce* bounces, uint32_t n, const rtr_accum_params* p,
                               float* accum, float* outTerm, float* outThroughput) {
    return enqueue_accumulate(c, radiance, throughput, pathIds, emitters, escapes, skySums, bounces, n, p, accum, outTerm, outThroughput,
                              "rtr_accumulate_paths_async");
}

int rtr_accumulate_paths(rtr_ctx* c, const RtrRadiance* radiance, const float* throughput, const uint32_t* pathIds, const RtrEmitter* emitters,
                         const RtrSkyEscape* escapes, const float* skySums, const RtrBounce* bounces, uint32_t n, const rtr_accum_params* p,
                         float* accum, float* outTerm, float* outThroughput) {
    return join_if_enqueued(c, enqueue_accumulate(c, radiance, throughput, pathIds, emitters, escapes, skySums, bounces, n, p, accum, outTerm,
                                                  outThroughput, "rtr_accumulate_paths"), n);
}

static int enqueue_gather(rtr_ctx* c, const void* src, uint32_t recordBytes, uint32_t numSrc, const uint32_t* rows, uint32_t numRows, void* out, const char* who) {
    if (const int rc = numRows ? rtrdev::gather_check_args(who, src, recordBytes, numSrc, rows, numRows, out) : RTR_OK) return rc;
    if (!c) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: ctx is null", who);
    if (numRows == 0) return RTR_OK;
    HIP_TRY(hipSetDevice(c->device));
    rtrdev::GatherArgs a{};
    a.src = static_cast<const char*>(src); a.rows = rows; a.out = static_cast<char*>(out);
    a.recordBytes = recordBytes; a.numSrc = numSrc; a.numRows = numRows;
    return launched(rtrdev::launch_gather_records(a, c->stream), who);
}

int rtr_gather_records_async(rtr_ctx* c, const void* src, uint32_t recordBytes, uint32_t numSrc, const uint32_t* rows, uint32_t numRows, void* out) {
    return enqueue_gather(c, src, recordBytes, numSrc, rows, numRows, out, "rtr_gather_records_async");
}

int rtr_gather_records(rtr_ctx* c, const void* src, uint32_t recordBytes, uint32_t numSrc, const uint32_t* rows, uint32_t numRows, void* out) {
    return join_if_enqueued(c, enqueue_gather(c, src, recordBytes, numSrc, rows, numRows, out, "rtr_gather_records"), numRows);
}

/* ---- picked light samples (kernels/rtr_query.hip; the rule is include/rtr_pick.h, the host form and the argument checks rtr_pick_host.cpp) -- */
/* What the picked calls and rtr_mis_pick_weights do between their own argument checks and the launch: the handles, their device, the
 * scene's lights against the params.  areaSlots: A of include/rtr_pick.h; tris: the light triangles behind it.  (rtr_api_power.cpp calls it too.) */
extern "C++" int rtrapi::picked_scene_checks(const rtr_ctx* c, const rtr_scene* s, const rtr_light_params* p, const char* who, uint32_t* areaSlots, uint32_t* tris) {
    if (const int rc = check_handles(c, s, who)) return rc;
    if (const int rc = check_same_device(c, s, who)) return rc;
    uint32_t q = 0;
    if (const int rc = light_slots(s, p, &q, who)) return rc;
    *areaSlots = q - 1u; *tris = *areaSlots / p->numShadowRays;
    return rtrdev::pick_check_area(who, *areaSlots);
}

/* and what their launches take alike; the output arrays and the weights are the caller's.  (rtr_api_ris.cpp calls it too.) */
extern "C++" void rtrapi::fill_pick_args(rtrdev::PickArgs& pa, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                           const rtr_pick_params* pick, const uint32_t* seeds, const uint32_t* slots, uint32_t areaSlots, uint32_t tris) {
    fill_light_args(pa.la, s, rays, hits, n, p, seeds);
    pa.la.slots = pick->numPicks + 1u;
    pa.picks = pick->numPicks; pa.depth = pick->depth; pa.areaSlots = areaSlots;
    pa.defaultWeight = (float)tris / (float)pick->numPicks;
    pa.slotsIn = slots;
}

static int enqueue_light_picked(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                                const rtr_pick_params* pick, const uint32_t* seeds, const uint32_t* slots, RtrRay* outRays, uint32_t* outSlots,
                                const float* weights, const uint8_t* occluded, RtrRadiance* out, bool shade, const char* who) {
    /* the params and the arrays are checked first, which needs nothing of the handles */
    if (const int rc = rtrdev::pick_check_params(who, p, pick, shade)) return rc;
    const rtrdev::PickCall call{rays, hits, n, p, pick, seeds, shade, slots, outRays, outSlots, weights, occluded, out};
    if (const int rc = n ? rtrdev::pick_check_arrays(who, call) : RTR_OK) return rc;
    uint32_t areaSlots = 0, tris = 0;
    if (const int rc = picked_scene_checks(c, s, p, who, &areaSlots, &tris)) return rc;
    if (n == 0) return RTR_OK;
    HIP_TRY(hipSetDevice(c->device));
    rtrdev::PickArgs pa{};
    fill_pick_args(pa, s, rays, hits, n, p, pick, seeds, slots, areaSlots, tris);
    pa.la.outRays = reinterpret_cast<float4*>(outRays); pa.la.occluded = occluded; pa.la.out = reinterpret_cast<float4*>(out);
    pa.outSlots = outSlots; pa.weights = weights;
    return launched(shade ? rtrdev::launch_shade_hits_picked(s->dev, pa, c->stream) : rtrdev::launch_light_rays_picked(s->dev, pa, c->stream), who);
}

int rtr_light_rays_picked_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                                const rtr_pick_params* pick, const uint32_t* seeds, const uint32_t* slotsIn, RtrRay* outRays, uint32_t* outSlots) {
    return enqueue_light_picked(c, s, rays, hits, n, p, pick, seeds, slotsIn, outRays, outSlots, nullptr, nullptr, nullptr, false, "rtr_light_rays_picked_async");
}

int rtr_light_rays_picked(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                          const rtr_pick_params* pick, const uint32_t* seeds, const uint32_t* slotsIn, RtrRay* outRays, uint32_t* outSlots) {
    return join_if_enqueued(c, enqueue_light_picked(c, s, rays, hits, n, p, pick, seeds, slotsIn, outRays, outSlots, nullptr, nullptr, nullptr, false,
                                                    "rtr_light_rays_picked"), n);
}

int rtr_shade_hits_picked_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                                const rtr_pick_params* pick, const uint32_t* seeds, const uint32_t* slots, const float* weights,
                                const uint8_t* occluded, RtrRadiance* out) {
    return enqueue_light_picked(c, s, rays, hits, n, p, pick, seeds, slots, nullptr, nullptr, weights, occluded, out, true, "rtr_shade_hits_picked_async");
}

int rtr_shade_hits_picked(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                          const rtr_pick_params* pick, const uint32_t* seeds, const uint32_t* slots, const float* weights,
                          const uint8_t* occluded, RtrRadiance* out) {
    return join_if_enqueued(c, enqueue_light_picked(c, s, rays, hits, n, p, pick, seeds, slots, nullptr, nullptr, weights, occluded, out, true,
                                                    "rtr_shade_hits_picked"), n);
}

/* ---- MIS at a path vertex (kernels/rtr_query.hip, kernels/rtr_mis.hip; the rule is include/rtr_mis.h, the host forms and the argument checks rtr_mis_host.cpp) -- */
static int enqueue_mis_pick_weights(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                                    const rtr_pick_params* pick, const rtr_mis_params* mis, const uint32_t* seeds, const uint32_t* slots,
                                    float* outWeights, RtrMisSample* outSamples, const char* who, bool power = false) {
    /* the params and the arrays are checked first, which needs nothing of the handles */
    if (const int rc = rtrdev::mis_check_params(who, mis)) return rc;
    if (const int rc = rtrdev::pick_check_params(who, p, pick, true)) return rc;
    if (const int rc = rtrdev::mis_check_pick_call(who, p, pick, mis, rays, hits, n, seeds, slots, outWeights, outSamples)) return rc;
    if (power && n && !slots) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: slots is null", who);      /* the power form draws none itself */
    uint32_t areaSlots = 0, tris = 0;
    if (const int rc = picked_scene_checks(c, s, p, who, &areaSlots, &tris)) return rc;
    if (n == 0) return RTR_OK;
    HIP_TRY(hipSetDevice(c->device));
    rtrdev::MisPickArgs ma{};
    fill_pick_args(ma.pa, s, rays, hits, n, p, pick, seeds, slots, areaSlots, tris);
    ma.outWeights = outWeights; ma.outSamples = reinterpret_cast<float4*>(outSamples); ma.lobes = mis->lobes; ma.tris = tris;
    if (power) {
        if (const int rc = ensure_light_power(s, c->stream, who)) return rc;
        ma.cdf = s->powerCdf.p;
    }
    return launched(rtrdev::launch_mis_pick_weights(s->dev, ma, c->stream), who);
}

int rtr_mis_pick_weights_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                               const rtr_pick_params* pick, const rtr_mis_params* mis, const uint32_t* seeds, const uint32_t* slots, float* outWeights,
                               RtrMisSample* outSamples) {
    return enqueue_mis_pick_weights(c, s, rays, hits, n, p, pick, mis, seeds, slots, outWeights, outSamples, "rtr_mis_pick_weights_async");
}

int rtr_mis_pick_weights(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                         const rtr_pick_params* pick, const rtr_mis_params* mis, const uint32_t* seeds, const uint32_t* slots, float* outWeights,
                         RtrMisSample* outSamples) {
    return join_if_enqueued(c, enqueue_mis_pick_weights(c, s, rays, hits, n, p, pick, mis, seeds, slots, outWeights, outSamples, "rtr_mis_pick_weights"), n);
}

/* the power forms (include/rtr_power.h): the same checks and the same kernel's other instantiation, with the scene's power table */
int rtr_mis_pick_weights_power_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                                     const rtr_pick_params* pick, const rtr_mis_params* mis, const uint32_t* seeds, const uint32_t* slots,
                                     float* outWeights, RtrMisSample* outSamples) {
    return enqueue_mis_pick_weights(c, s, rays, hits, n, p, pick, mis, seeds, slots, outWeights, outSamples, "rtr_mis_pick_weights_power_async", true);
}

int rtr_mis_pick_weights_power(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                               const rtr_pick_params* pick, const rtr_mis_params* mis, const uint32_t* seeds, const uint32_t* slots, float* outWeights,
                               RtrMisSample* outSamples) {
    return join_if_enqueued(c, enqueue_mis_pick_weights(c, s, rays, hits, n, p, pick, mis, seeds, slots, outWeights, outSamples,
                                                        "rtr_mis_pick_weights_power", true), n);
}

static int enqueue_emitter_hits(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces,
                                const RtrBounce* bounces, uint32_t n, const rtr_mis_params* mis, RtrEmitter* out, const char* who, bool power = false) {
    /* the params and the arrays are checked first, which needs nothing of the handles */
    if (const int rc = rtrdev::mis_check_params(who, mis)) return rc;
    if (const int rc = n ? rtrdev::mis_check_emitter_arrays(who, rays, hits, prevSurfaces, bounces, out) : RTR_OK) return rc;
    if (const int rc = check_handles(c, s, who)) return rc;
    if (const int rc = check_same_device(c, s, who)) return rc;
    if (mis->numAreaLights > s->numLights) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: numAreaLights %u > scene lights %u", who, mis->numAreaLights, s->numLights);
    uint64_t tris = 0;
    for (uint32_t l = 0; l < mis->numAreaLights; ++l) tris += s->hostLights[l].numTriangles;
    if (tris > RTR_PICK_MAX_SLOTS) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: %llu light triangles are more than 2^24", who, (unsigned long long)tris);
    if (n == 0) return RTR_OK;
    HIP_TRY(hipSetDevice(c->device));
    rtrdev::EmitterArgs a{};
    a.rays = reinterpret_cast<const float4*>(rays); a.hits = reinterpret_cast<const float4*>(hits);
    a.prevSurfaces = reinterpret_cast<const float4*>(prevSurfaces); a.bounces = reinterpret_cast<const float4*>(bounces);
    a.out = reinterpret_cast<float4*>(out);
    a.lightTris = s->dev.lightTris; a.lightTriFirst = s->dev.lightTriFirst; a.lights = s->dev.lights; a.numLights = s->numLights;
    a.numAreaLights = mis->numAreaLights; a.tris = (uint32_t)tris; a.picks = mis->numPicks; a.n = n;
    if (power) {
        if (const int rc = ensure_light_power(s, c->stream, who)) return rc;
        a.cdf = s->powerCdf.p;
    }
    return launched(rtrdev::launch_emitter_hits(a, c->stream), who);
}

int rtr_emitter_hits_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces, const RtrBounce* bounces,
                           uint32_t n, const rtr_mis_params* mis, RtrEmitter* out) {
    return enqueue_emitter_hits(c, s, rays, hits, prevSurfaces, bounces, n, mis, out, "rtr_emitter_hits_async");
}

int rtr_emitter_hits(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces, const RtrBounce* bounces,
                     uint32_t n, const rtr_mis_params* mis, RtrEmitter* out) {
    return join_if_enqueued(c, enqueue_emitter_hits(c, s, rays, hits, prevSurfaces, bounces, n, mis, out, "rtr_emitter_hits"), n);
}

int rtr_emitter_hits_power_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces,
                                 const RtrBounce* bounces, uint32_t n, const rtr_mis_params* mis, RtrEmitter* out) {
    return enqueue_emitter_hits(c, s, rays, hits, prevSurfaces, bounces, n, mis, out, "rtr_emitter_hits_power_async", true);
}

int rtr_emitter_hits_power(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces, const RtrBounce* bounces,
                           uint32_t n, const rtr_mis_params* mis, RtrEmitter* out) {
    return join_if_enqueued(c, enqueue_emitter_hits(c, s, rays, hits, prevSurfaces, bounces, n, mis, out, "rtr_emitter_hits_power", true), n);
}

/* ---- sky importance sampling (kernels/rtr_sky.hip; the rule is include/rtr_sky.h, the host forms and the argument checks rtr_sky_host.cpp) -- */
static rtr_sky_source scene_sky_source(const rtr_scene* s) {
    rtr_sky_source src{};
    src.pixels = s->dev.hdri.pixels; src.width = s->dev.hdri.width; src.height = s->dev.hdri.height; src.channels = s->dev.hdri.channels;
    for (int k = 0; k < 3; ++k) src.skyLinear[k] = s->dev.skyLinear[k];
    return src;
}

/* Made by the first call that needs it, on `st` (the current device is the scene's), and JOINED before the call goes on, as the leaf
 * table is: whichever context of the device asks next finds it complete.  It reads the HDRI's texels and the sky colour alone, which
 * no update, refit or rebuild writes. */
static int ensure_sky_table(const rtr_scene* s, hipStream_t st, const char* who) {
    if (s->skyReady) return RTR_OK;
    const rtr_sky_source src = scene_sky_source(s);
    const uint32_t W = rtr_sky_table_width(&src), H = rtr_sky_table_height(&src);
    if (W > RTR_SKY_MAX_WIDTH) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: the scene's hdri is %u texels wide: a row's sum fits 32 bits up to %u", who, W, RTR_SKY_MAX_WIDTH);
    HIP_TRY(s->skyRows.alloc((size_t)W * H));
    HIP_TRY(s->skyMarginal.alloc(H));
    const hipError_t e = rtrdev::launch_sky_table(src, s->skyRows.p, s->skyMarginal.p, st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: sky table: %s", who, hipGetErrorString(e));
    HIP_TRY(hipStreamSynchronize(st));
    s->skyReady = true;
    return RTR_OK;
}

static rtrdev::SkyDevice scene_sky_device(const rtr_scene* s) {
    rtrdev::SkyDevice sd{};
    sd.sky = scene_sky_source(s);
    sd.table.rows = s->skyRows.p; sd.table.marginal = s->skyMarginal.p;
    sd.table.width = rtr_sky_table_width(&sd.sky); sd.table.height = rtr_sky_table_height(&sd.sky);
    return sd;
}

int rtr_scene_prepare_sky(rtr_scene* s) {
    static const char* who = "rtr_scene_prepare_sky";
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null scene", who);
    HIP_TRY(hipSetDevice(s->ctx->device));
    return ensure_sky_table(s, s->ctx->stream, who);
}

int rtr_scene_export_sky_table(const rtr_scene* s, uint32_t* outWidth, uint32_t* outHeight, uint32_t* outRows, size_t capacityCells, uint64_t* outMarginal,
                               uint32_t capacityRows) {
    static const char* who = "rtr_scene_export_sky_table";
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null scene", who);
    const rtr_sky_source src = scene_sky_source(s);
    const uint32_t W = rtr_sky_table_width(&src), H = rtr_sky_table_height(&src);
    if (outWidth) *outWidth = W;
    if (outHeight) *outHeight = H;
    if (!outRows || !outMarginal || capacityCells < (size_t)W * H || capacityRows < H)
        return fail(RTR_ERR_INVALID_ARGUMENT, "%s: capacity %zu cells, %u rows; %zu and %u are needed", who, outRows ? capacityCells : (size_t)0,
                    outMarginal ? capacityRows : 0u, (size_t)W * H, H);
    HIP_TRY(hipSetDevice(s->ctx->device));
    if (const int rc = ensure_sky_table(s, s->ctx->stream, who)) return rc;
    HIP_TRY(hipMemcpy(outRows, s->skyRows.p, (size_t)W * H * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(outMarginal, s->skyMarginal.p, (size_t)H * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return RTR_OK;
}

static int enqueue_sky_rays(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrSurface* surfaces, uint32_t n, const rtr_sky_params* p,
                            const uint32_t* seeds, RtrRay* outRays, RtrSkySample* outSamples, const char* who) {
    /* the params and the arrays are checked first, which needs nothing of the handles */
    if (const int rc = rtrdev::sky_check_params(who, p, false)) return rc;
    if (const int rc = rtrdev::sky_check_rays_call(who, p, rays, surfaces, n, seeds, outRays, outSamples)) return rc;
    if (const int rc = check_handles(c, s, who)) return rc;
    if (const int rc = check_same_device(c, s, who)) return rc;
    if (n == 0) return RTR_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (const int rc = ensure_sky_table(s, c->stream, who)) return rc;
    rtrdev::SkyRaysArgs a{};
    a.sd = scene_sky_device(s);
    a.rays = reinterpret_cast<const float4*>(rays); a.surfaces = reinterpret_cast<const float4*>(surfaces); a.seeds = seeds;
    a.outRays = reinterpret_cast<float4*>(outRays); a.outSamples = reinterpret_cast<float4*>(outSamples);
    a.params = *p; a.n = n;
    return launched(rtrdev::launch_sky_rays(a, a.sd.table.height <= rtrdev::kSkyLdsRows, c->stream), who);
}

int rtr_sky_rays_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrSurface* surfaces, uint32_t n, const rtr_sky_params* p,
                       const uint32_t* seeds, RtrRay* outRays, RtrSkySample* outSamples) {
    return enqueue_sky_rays(c, s, rays, surfaces, n, p, seeds, outRays, outSamples, "rtr_sky_rays_async");
}

int rtr_sky_rays(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrSurface* surfaces, uint32_t n, const rtr_sky_params* p,
                 const uint32_t* seeds, RtrRay* outRays, RtrSkySample* outSamples) {
    return join_if_enqueued(c, enqueue_sky_rays(c, s, rays, surfaces, n, p, seeds, outRays, outSamples, "rtr_sky_rays"), n);
}

static int enqueue_shade_sky(rtr_ctx* c, const RtrSkySample* samples, const uint8_t* occluded, uint32_t n, uint32_t numSamples, float* out, const char* who) {
    if (const int rc = rtrdev::sky_check_shade_call(who, samples, occluded, n, numSamples, out)) return rc;
    if (!c) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null context", who);
    if (n == 0) return RTR_OK;
    HIP_TRY(hipSetDevice(c->device));
    rtrdev::SkyShadeArgs a{};
    a.samples = reinterpret_cast<const float4*>(samples); a.occluded = occluded; a.out = reinterpret_cast<float4*>(out);
    a.numSamples = numSamples; a.n = n;
    return launched(rtrdev::launch_shade_sky(a, c->stream), who);
}

int rtr_shade_sky_async(rtr_ctx* c, const RtrSkySample* samples, const uint8_t* occluded, uint32_t n, uint32_t numSamples, float* out) {
    return enqueue_shade_sky(c, samples, occluded, n, numSamples, out, "rtr_shade_sky_async");
}

int rtr_shade_sky(rtr_ctx* c, const RtrSkySample* samples, const uint8_t* occluded, uint32_t n, uint32_t numSamples, float* out) {
    const int rc = enqueue_shade_sky(c, samples, occluded, n, numSamples, out, "rtr_shade_sky");
    return rc == RTR_OK ? join_if_enqueued(c, rc, n) : rc;
}

static int enqueue_sky_hits(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces, const RtrBounce* bounces,
                            uint32_t n, const rtr_sky_params* p, RtrSkyEscape* out, const char* who) {
    if (const int rc = rtrdev::sky_check_params(who, p, true)) return rc;
    if (const int rc = n ? rtrdev::sky_check_hits_arrays(who, rays, hits, prevSurfaces, bounces, n, out) : RTR_OK) return rc;
    if (const int rc = check_handles(c, s, who)) return rc;
    if (const int rc = check_same_device(c, s, who)) return rc;
    if (n == 0) return RTR_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (const int rc = ensure_sky_table(s, c->stream, who)) return rc;
    rtrdev::SkyHitsArgs a{};
    a.sd = scene_sky_device(s);
    a.rays = reinterpret_cast<const float4*>(rays); a.hits = reinterpret_cast<const float4*>(hits);
    a.prevSurfaces = reinterpret_cast<const float4*>(prevSurfaces); a.bounces = reinterpret_cast<const float4*>(bounces);
    a.out = reinterpret_cast<float4*>(out); a.numSamples = p->numSamples; a.flags = p->flags; a.n = n;
    return launched(rtrdev::launch_sky_hits(a, c->stream), who);
}

int rtr_sky_hits_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces, const RtrBounce* bounces,
                       uint32_t n, const rtr_sky_params* p, RtrSkyEscape* out) {
    return enqueue_sky_hits(c, s, rays, hits, prevSurfaces, bounces, n, p, out, "rtr_sky_hits_async");
}

int rtr_sky_hits(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces, const RtrBounce* bounces,
                 uint32_t n, const rtr_sky_params* p, RtrSkyEscape* out) {
    return join_if_enqueued(c, enqueue_sky_hits(c, s, rays, hits, prevSurfaces, bounces, n, p, out, "rtr_sky_hits"), n);
}

int rtr_scene_export_light_tris(const rtr_scene* s, float* outRecords, uint32_t capacityTris, uint32_t* outFirst, uint32_t* outCount) {
    static const char* who = "rtr_scene_export_light_tris";
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null scene", who);
    uint32_t total = 0;
    std::vector<uint32_t> first(s->numLights);
    for (uint32_t l = 0; l < s->numLights; ++l) { first[l] = total; total += s->hostLights[l].numTriangles; }
    if (outCount) *outCount = total;
    if (capacityTris < total || (total && !outRecords))
        return fail(RTR_ERR_INVALID_ARGUMENT, "%s: capacity %u light triangles, %u are needed", who, outRecords ? capacityTris : 0u, total);
    HIP_TRY(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    if (total) HIP_TRY(hipMemcpyAsync(outRecords, s->lightTris.p, (size_t)total * rtrdev::kLightTriRecord * sizeof(float4), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (outFirst) for (uint32_t l = 0; l < s->numLights; ++l) outFirst[l] = first[l];
    return RTR_OK;
}

}  // extern "C"
