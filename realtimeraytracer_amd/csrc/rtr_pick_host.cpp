/* rtr_pick_host.cpp — rtr_host_pick_slots and the argument checks rtr_light_rays_picked / rtr_shade_hits_picked share with it.
 * Pure host C++ with no HIP in it: include/rtr_pick.h compiled for the host cores with the kernels' flags (-ffp-contract=off, no
 * fast-math), so that the device's slots can be held to these words; a translation unit of its own so that a stand-alone program
 * (tools/pick_host_check.cpp) can run it under the host sanitizers. */
#include "rtr_pick_host.h"
#include "../../include/rtr_pick.h"

#include <cstdint>
#include <cstdio>

namespace rtrdev {

static bool pick_params_ok(const char* who, const rtr_pick_params* pick, char* msg, size_t msgBytes) {
    if (!pick) { snprintf(msg, msgBytes, "%s: pick params is null", who); return false; }
    if (pick->numPicks == 0u || pick->numPicks > RTR_PICK_MAX) {
        snprintf(msg, msgBytes, "%s: numPicks %u (1 ... %u)", who, pick->numPicks, RTR_PICK_MAX);
        return false;
    }
    uint32_t r = 0;
    for (int i = 0; i < 6; ++i) r |= pick->_reserved[i];
    if (r) { snprintf(msg, msgBytes, "%s: _reserved words of pick params are not 0", who); return false; }
    return true;
}

bool pick_check_params(const char* who, const rtr_light_params* p, const rtr_pick_params* pick, bool shade, char* msg, size_t msgBytes, int* rc) {
    *rc = RTR_ERR_INVALID_ARGUMENT;
    if (!p) { snprintf(msg, msgBytes, "%s: params is null", who); return false; }
    if (!pick_params_ok(who, pick, msg, msgBytes)) return false;
    /* what rtr_light_slots refuses of the params alone; numAreaLights is held to the scene's lights once there is a scene */
    if (p->numShadowRays == 0 || p->numShadowRays > 1024) { snprintf(msg, msgBytes, "%s: numShadowRays %u (1 ... 1024)", who, p->numShadowRays); return false; }
    if (p->outputs & ~(RTR_LIGHT_SHADOWED | RTR_LIGHT_UNSHADOWED | RTR_LIGHT_ANALYTIC)) {
        snprintf(msg, msgBytes, "%s: unknown output bits 0x%x", who, p->outputs);
        return false;
    }
    if (shade && (p->outputs & RTR_LIGHT_ANALYTIC)) {
        *rc = RTR_ERR_UNSUPPORTED;
        snprintf(msg, msgBytes, "%s: RTR_LIGHT_ANALYTIC has no per-sample form (the LTC term integrates whole lights): use rtr_shade_hits", who);
        return false;
    }
    return true;
}

bool pick_check_arrays(const char* who, const PickCall& c, char* msg, size_t msgBytes) {
    const uint32_t P = c.pick->numPicks, R = P + 1u;
    if ((uint64_t)c.n * R > 0xffffffffull) { snprintf(msg, msgBytes, "%s: %u hits x %u slots do not fit 32 bits", who, c.n, R); return false; }
    struct Arg { const void* ptr; const char* name; unsigned align; bool needed; };
    const Arg light[6] = {{c.rays, "rays", 16, true}, {c.hits, "hits", 16, true}, {c.seeds, "seeds", 4, false}, {c.slots, "slotsIn", 4, false},
                          {c.outRays, "outRays", 16, true}, {c.outSlots, "outSlots", 4, true}};
    const Arg shade[7] = {{c.rays, "rays", 16, true}, {c.hits, "hits", 16, true}, {c.seeds, "seeds", 4, false}, {c.slots, "slots", 4, true},
                          {c.weights, "weights", 4, false}, {c.occluded, "occluded", 1, true}, {c.out, "out", 16, true}};
    const Arg* args = c.shade ? shade : light;
    const int count = c.shade ? 7 : 6;
    for (int i = 0; i < count; ++i)
        if (args[i].needed && !args[i].ptr) { snprintf(msg, msgBytes, "%s: %s is null", who, args[i].name); return false; }
    for (int i = 0; i < count; ++i)
        if (args[i].ptr && ((uintptr_t)args[i].ptr & (args[i].align - 1u))) {
            snprintf(msg, msgBytes, "%s: %s is not %u-B aligned", who, args[i].name, args[i].align);
            return false;
        }
    if (!c.seeds && (c.light->width == 0 || c.light->spp == 0)) {
        snprintf(msg, msgBytes, "%s: width %u, spp %u: without seeds the hits are pixel-samples of a frame", who, c.light->width, c.light->spp);
        return false;
    }
    return true;
}

bool pick_check_area(const char* who, uint64_t areaSlots, char* msg, size_t msgBytes) {
    if (areaSlots > RTR_PICK_MAX_SLOTS) {
        snprintf(msg, msgBytes, "%s: %llu area slots per hit are more than RTR_PICK_MAX_SLOTS = 2^24", who, (unsigned long long)areaSlots);
        return false;
    }
    return true;
}

}  // namespace rtrdev

extern "C" int rtr_host_pick_slots(const uint32_t* seeds, uint32_t n, uint32_t frame, uint32_t width, uint32_t spp, const rtr_pick_params* pick,
                                   uint32_t areaSlots, uint32_t* outSlots) {
    const char* who = "rtr_host_pick_slots";
    char msg[256];
    if (!rtrdev::pick_params_ok(who, pick, msg, sizeof msg) || !rtrdev::pick_check_area(who, areaSlots, msg, sizeof msg)) {
        rtrdev::set_last_error(msg);
        return RTR_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return RTR_OK;
    const uint32_t P = pick->numPicks;
    if ((uint64_t)n * P > 0xffffffffull) snprintf(msg, sizeof msg, "%s: %u hits x %u picks do not fit 32 bits", who, n, P);
    else if (!outSlots) snprintf(msg, sizeof msg, "%s: outSlots is null", who);
    else if (((uintptr_t)outSlots | (uintptr_t)seeds) & 3u) snprintf(msg, sizeof msg, "%s: %s is not 4-B aligned", who, ((uintptr_t)outSlots & 3u) ? "outSlots" : "seeds");
    else if (!seeds && (width == 0 || spp == 0)) snprintf(msg, sizeof msg, "%s: width %u, spp %u: without seeds the hits are pixel-samples of a frame", who, width, spp);
    else {
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t baseFrame = rtr_pick_base(seeds, k, width, spp) + frame;
            for (uint32_t p = 0; p < P; ++p) outSlots[(size_t)k * P + p] = rtr_pick_slot(baseFrame, pick->depth, p, areaSlots);
        }
        return RTR_OK;
    }
    rtrdev::set_last_error(msg);
    return RTR_ERR_INVALID_ARGUMENT;
}
