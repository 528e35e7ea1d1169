/* rtr_api_power.cpp — the light-power table of a scene and the picks drawn from it (include/rtr.h; the rule is include/rtr_power.h, the
 * kernels kernels/rtr_power.hip, the host forms and the argument checks rtr_power_host.cpp).  The power forms of rtr_mis_pick_weights and
 * rtr_emitter_hits stand beside their uniform forms in rtr_api_paths.cpp and take the table from here. */
#include "../../include/rtr.h"
#include "kernels/rtr_power_launch.h"
#include "rtr_pick_host.h"
#include "rtr_power_host.h"
#include "rtr_api_internal.h"

#include <hip/hip_runtime.h>

using namespace rtrapi;

static rtrdev::PowerTable scene_power_table(const rtr_scene* s) {
    rtrdev::PowerTable t{};
    t.weights = s->powerWeights.p; t.cdf = s->powerCdf.p; t.maxBits = s->powerMax.p; t.numTris = s->powerTris;
    return t;
}

static hipError_t launch_scene_power(const rtr_scene* s, hipStream_t st) {
    return rtrdev::launch_light_power(s->lightTris.p, s->lightTriFirst.p, s->lights.p, s->numLights, scene_power_table(s), st);
}

int rtrapi::ensure_light_power(const rtr_scene* s, hipStream_t st, const char* who) {
    if (s->powerReady) return RTR_OK;
    uint64_t tris = 0;
    for (uint32_t l = 0; l < s->numLights; ++l) tris += s->hostLights[l].numTriangles;
    if (tris > 0xffffffffull) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: %llu light triangles do not fit 32 bits", who, (unsigned long long)tris);
    HIP_TRY(s->powerWeights.alloc((size_t)tris));
    HIP_TRY(s->powerCdf.alloc((size_t)tris));
    HIP_TRY(s->powerMax.alloc(1));
    s->powerTris = (uint32_t)tris;
    HIP_TRY(hipMemsetAsync(s->powerMax.p, 0, sizeof(uint32_t), st));      /* every build leaves the word 0 behind it: this is the only memset */
    const hipError_t e = launch_scene_power(s, st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: light-power table: %s", who, hipGetErrorString(e));
    HIP_TRY(hipStreamSynchronize(st));
    s->powerReady = true;
    return RTR_OK;
}

int rtrapi::enqueue_light_power(const rtr_scene* s, hipStream_t st, const char* who) {
    if (!s->powerReady) return RTR_OK;
    const hipError_t e = launch_scene_power(s, st);
    return e == hipSuccess ? RTR_OK : fail(RTR_ERR_HIP, "%s: light-power table: %s", who, hipGetErrorString(e));
}

extern "C" {

int rtr_scene_prepare_light_power(rtr_scene* s) {
    static const char* who = "rtr_scene_prepare_light_power";
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null scene", who);
    HIP_TRY(hipSetDevice(s->ctx->device));
    return ensure_light_power(s, s->ctx->stream, who);
}

int rtr_scene_export_light_power(const rtr_scene* s, uint32_t* outWeights, uint64_t* outCdf, uint32_t capacityTris, uint32_t* outCount) {
    static const char* who = "rtr_scene_export_light_power";
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null scene", who);
    uint32_t total = 0;
    for (uint32_t l = 0; l < s->numLights; ++l) total += s->hostLights[l].numTriangles;
    if (outCount) *outCount = total;
    if (capacityTris < total || (total && (!outWeights || !outCdf)))
        return fail(RTR_ERR_INVALID_ARGUMENT, "%s: capacity %u light triangles, %u are needed", who, outWeights && outCdf ? capacityTris : 0u, total);
    HIP_TRY(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    if (const int rc = ensure_light_power(s, st, who)) return rc;
    /* on the scene's stream, behind the builds its updates enqueued there */
    if (total) {
        HIP_TRY(hipMemcpyAsync(outWeights, s->powerWeights.p, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(outCdf, s->powerCdf.p, (size_t)total * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return RTR_OK;
}

static int enqueue_pick_slots_power(rtr_ctx* c, const rtr_scene* s, uint32_t n, const rtr_light_params* p, const rtr_pick_params* pick,
                                    const uint32_t* seeds, uint32_t* outSlots, float* outWeights, const char* who) {
    /* the params and the arrays are checked first, which needs nothing of the handles */
    if (const int rc = rtrdev::pick_check_params(who, p, pick, false)) return rc;
    if (const int rc = rtrdev::power_check_pick_call(who, p, pick, n, seeds, outSlots, outWeights)) return rc;
    uint32_t areaSlots = 0, tris = 0;
    if (const int rc = picked_scene_checks(c, s, p, who, &areaSlots, &tris)) return rc;
    if (n == 0) return RTR_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (const int rc = ensure_light_power(s, c->stream, who)) return rc;
    rtrdev::PowerPickArgs a{};
    a.cdf = s->powerCdf.p; a.seeds = seeds; a.outSlots = outSlots; a.outWeights = outWeights;
    a.tris = tris; a.numShadowRays = p->numShadowRays; a.frame = p->frame; a.width = p->width; a.spp = p->spp;
    a.picks = pick->numPicks; a.depth = pick->depth; a.n = n;
    return launched(rtrdev::launch_pick_slots_power(a, c->stream), who);
}

int rtr_pick_slots_power_async(rtr_ctx* c, const rtr_scene* s, uint32_t n, const rtr_light_params* p, const rtr_pick_params* pick, const uint32_t* seeds,
                               uint32_t* outSlots, float* outWeights) {
    return enqueue_pick_slots_power(c, s, n, p, pick, seeds, outSlots, outWeights, "rtr_pick_slots_power_async");
}

int rtr_pick_slots_power(rtr_ctx* c, const rtr_scene* s, uint32_t n, const rtr_light_params* p, const rtr_pick_params* pick, const uint32_t* seeds,
                         uint32_t* outSlots, float* outWeights) {
    return join_if_enqueued(c, enqueue_pick_slots_power(c, s, n, p, pick, seeds, outSlots, outWeights, "rtr_pick_slots_power"), n);
}

}  // extern "C"
