/* rtr_arg_check.h — the argument checks the ray-query, lighting and path-vertex calls share, device and host forms alike (internal to
 * librtr_hip.so).  Host-only and header-only, no HIP in it.  Every check returns RTR_OK when the call may go on; else it leaves the
 * refusal's message (it names `who` and the argument) as the thread's last error and returns the refusal's status. */
#pragma once
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/rtr.h"

namespace rtrdev {

/* rtr_last_error's text for this thread; defined by rtr_api.cpp (a stand-alone program around a rtr_*_host.cpp brings its own) */
void set_last_error(const char* msg);

inline int refuse(const char* msg) {
    set_last_error(msg);
    return RTR_ERR_INVALID_ARGUMENT;
}

__attribute__((format(printf, 1, 2))) inline int refusef(const char* fmt, ...) {
    char msg[256];
    va_list ap; va_start(ap, fmt); vsnprintf(msg, sizeof msg, fmt, ap); va_end(ap);
    return refuse(msg);
}

/* one pointer argument of a call; bytes: its extent, read by check_overlaps only */
struct Arg { const void* ptr; const char* name; unsigned align; bool needed; size_t bytes; };

/* the first needed entry that is null, in table order; if there is none, the first entry that is not null and misaligned */
inline int check_ptrs(const char* who, const Arg* args, size_t count) {
    for (size_t i = 0; i < count; ++i)
        if (args[i].needed && !args[i].ptr) return refusef("%s: %s is null", who, args[i].name);
    for (size_t i = 0; i < count; ++i)
        if ((uintptr_t)args[i].ptr & (args[i].align - 1u)) return refusef("%s: %s is not %u-B aligned", who, args[i].name, args[i].align);
    return RTR_OK;
}
template <size_t N>
int check_ptrs(const char* who, const Arg (&args)[N]) { return check_ptrs(who, args, N); }

inline bool overlaps(const Arg& a, const Arg& b) {
    const uintptr_t a0 = (uintptr_t)a.ptr, b0 = (uintptr_t)b.ptr;
    return a.ptr && b.ptr && a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

/* each output in turn against every input, then against the outputs before it (the earlier one is named first); null entries are skipped */
inline int check_overlaps(const char* who, const Arg* in, size_t numIn, const Arg* out, size_t numOut) {
    for (size_t o = 0; o < numOut; ++o) {
        for (size_t i = 0; i < numIn; ++i)
            if (overlaps(out[o], in[i])) return refusef("%s: %s overlaps %s", who, out[o].name, in[i].name);
        for (size_t q = 0; q < o; ++q)
            if (overlaps(out[o], out[q])) return refusef("%s: %s overlaps %s", who, out[q].name, out[o].name);
    }
    return RTR_OK;
}

/* ---- the rules several params structs share ---- */
inline int check_num_picks(const char* who, uint32_t numPicks) {
    return numPicks == 0u || numPicks > RTR_PICK_MAX ? refusef("%s: numPicks %u (1 ... %u)", who, numPicks, RTR_PICK_MAX) : RTR_OK;
}

inline int check_shadow_rays(const char* who, uint32_t numShadowRays) {
    return numShadowRays == 0u || numShadowRays > 1024u ? refusef("%s: numShadowRays %u (1 ... 1024)", who, numShadowRays) : RTR_OK;
}

inline int check_light_outputs(const char* who, uint32_t outputs) {
    return outputs & ~(RTR_LIGHT_SHADOWED | RTR_LIGHT_UNSHADOWED | RTR_LIGHT_ANALYTIC) ? refusef("%s: unknown output bits 0x%x", who, outputs) : RTR_OK;
}

inline int check_lobes(const char* who, uint32_t lobes) {
    if (lobes == 0u || (lobes & ~(RTR_BOUNCE_DIFFUSE | RTR_BOUNCE_SPECULAR)))
        return refusef("%s: lobes 0x%x (RTR_BOUNCE_DIFFUSE | RTR_BOUNCE_SPECULAR, at least one)", who, lobes);
    return RTR_OK;
}

/* without seeds the hits are numbered as the pixel-samples of a frame, which has a width and a sample count */
inline int check_pixel_seeds(const char* who, const uint32_t* seeds, uint32_t width, uint32_t spp) {
    if (!seeds && (width == 0u || spp == 0u))
        return refusef("%s: width %u, spp %u: without seeds the hits are pixel-samples of a frame", who, width, spp);
    return RTR_OK;
}

/* noun: whose words they are ("params", "pick params", "mis params") */
inline int check_reserved(const char* who, const uint32_t* words, size_t count, const char* noun) {
    uint32_t r = 0;
    for (size_t i = 0; i < count; ++i) r |= words[i];
    return r ? refusef("%s: _reserved words of %s are not 0", who, noun) : RTR_OK;
}

/* a x b is an element count the kernels index with 32 bits */
inline int check_fits_32(const char* who, uint32_t a, const char* nounA, uint32_t b, const char* nounB) {
    return (uint64_t)a * b > 0xffffffffull ? refusef("%s: %u %s x %u %s do not fit 32 bits", who, a, nounA, b, nounB) : RTR_OK;
}

}  // namespace rtrdev
