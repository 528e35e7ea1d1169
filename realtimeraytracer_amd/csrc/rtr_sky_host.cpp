/* rtr_sky_host.cpp — rtr_host_sky_table, rtr_host_sky_rays, rtr_host_sky_hits, rtr_host_sky_pdf, rtr_host_sky_radiance and the argument
 * checks rtr_sky_rays / rtr_shade_sky / rtr_sky_hits share with them.  Pure host C++ with no HIP in it: include/rtr_sky.h compiled for
 * the host cores with the kernels' flags (-ffp-contract=off, no fast-math), so that the device's records can be held to these bits; a
 * translation unit of its own so that a stand-alone program (tools/sky_host_check.cpp) can run it under the host sanitizers. */
#include "rtr_sky_host.h"
#include "../../include/rtr_sky.h"

#include <cstdint>

namespace rtrdev {

int sky_check_params(const char* who, const rtr_sky_params* p, bool zeroSamples) {
    if (!p) return refusef("%s: params is null", who);
    if ((p->numSamples == 0u && !zeroSamples) || p->numSamples > RTR_SKY_MAX_SAMPLES)
        return refusef("%s: numSamples %u (%u ... %u)", who, p->numSamples, zeroSamples ? 0u : 1u, RTR_SKY_MAX_SAMPLES);
    if (const int rc = check_lobes(who, p->lobes)) return rc;
    if (p->flags & ~RTR_SKY_MIS) return refusef("%s: unknown flags bits 0x%x", who, p->flags);
    return check_reserved(who, &p->_reserved, 1, "params");
}

int sky_check_rays_call(const char* who, const rtr_sky_params* p, const RtrRay* rays, const RtrSurface* surfaces, uint32_t n, const uint32_t* seeds,
                        const RtrRay* outRays, const RtrSkySample* outSamples) {
    if (const int rc = check_pixel_seeds(who, seeds, p->width, p->spp)) return rc;
    if (n == 0u) return RTR_OK;
    if (const int rc = check_fits_32(who, n, "hits", p->numSamples, "samples")) return rc;
    const size_t slots = (size_t)n * p->numSamples;
    const Arg in[3] = {{rays, "rays", 16, true, (size_t)n * sizeof(RtrRay)}, {surfaces, "surfaces", 16, true, (size_t)n * sizeof(RtrSurface)},
                       {seeds, "seeds", 4, false, (size_t)n * 4}};
    const Arg out[2] = {{outRays, "outRays", 16, true, slots * sizeof(RtrRay)}, {outSamples, "outSamples", 16, true, slots * sizeof(RtrSkySample)}};
    if (const int rc = check_ptrs(who, in)) return rc;
    if (const int rc = check_ptrs(who, out)) return rc;
    return check_overlaps(who, in, 3, out, 2);
}

int sky_check_shade_call(const char* who, const RtrSkySample* samples, const uint8_t* occluded, uint32_t n, uint32_t numSamples, const float* out) {
    if (numSamples == 0u || numSamples > RTR_SKY_MAX_SAMPLES) return refusef("%s: numSamples %u (1 ... %u)", who, numSamples, RTR_SKY_MAX_SAMPLES);
    if (n == 0u) return RTR_OK;
    if (const int rc = check_fits_32(who, n, "hits", numSamples, "samples")) return rc;
    const size_t slots = (size_t)n * numSamples;
    const Arg in[2] = {{samples, "samples", 16, true, slots * sizeof(RtrSkySample)}, {occluded, "occluded", 1, true, slots}};
    const Arg o[1] = {{out, "out", 16, true, (size_t)n * 16}};
    if (const int rc = check_ptrs(who, in)) return rc;
    if (const int rc = check_ptrs(who, o)) return rc;
    return check_overlaps(who, in, 2, o, 1);
}

int sky_check_hits_arrays(const char* who, const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces, const RtrBounce* bounces, uint32_t n,
                          const RtrSkyEscape* out) {
    const Arg in[4] = {{rays, "rays", 16, true, (size_t)n * sizeof(RtrRay)}, {hits, "hits", 16, true, (size_t)n * sizeof(RtrHit)},
                       {prevSurfaces, "prevSurfaces", 16, true, (size_t)n * sizeof(RtrSurface)}, {bounces, "bounces", 16, true, (size_t)n * sizeof(RtrBounce)}};
    const Arg o[1] = {{out, "out", 16, true, (size_t)n * sizeof(RtrSkyEscape)}};
    if (const int rc = check_ptrs(who, in)) return rc;
    if (const int rc = check_ptrs(who, o)) return rc;
    return check_overlaps(who, in, 4, o, 1);
}

int sky_check_texture(const char* who, const rtr_texture* hdri) {
    if (!hdri) return RTR_OK;
    if (!hdri->pixels) return refusef("%s: hdri has no pixels", who);
    if (hdri->width == 0u || hdri->height == 0u || (hdri->channels != 4u && hdri->channels != 1u))
        return refusef("%s: hdri: bad extent or channels", who);
    if (hdri->width > RTR_SKY_MAX_WIDTH) return refusef("%s: hdri is %u texels wide: a row's sum fits 32 bits up to %u", who, hdri->width, RTR_SKY_MAX_WIDTH);
    return RTR_OK;
}

namespace {

int sky_source(const char* who, const rtr_texture* hdri, const float* skyColor, rtr_sky_source* src) {
    if (const int rc = sky_check_texture(who, hdri)) return rc;
    if (!hdri && !skyColor) return refusef("%s: skyColor is null", who);
    src->pixels = hdri ? hdri->pixels : nullptr;
    src->width = hdri ? hdri->width : 0u; src->height = hdri ? hdri->height : 0u; src->channels = hdri ? hdri->channels : 0u;
    for (int k = 0; k < 3; ++k) src->skyLinear[k] = skyColor ? rtr_to_linear(skyColor[k]) : 0.0f;
    return RTR_OK;
}

int sky_check_table(const char* who, const rtr_sky_source* src, const rtr_sky_table* t) {
    if (!t) return refusef("%s: table is null", who);
    if (!t->rows || !t->marginal) return refusef("%s: table has no sums", who);
    if (t->width == 0u || t->height == 0u || t->width > RTR_SKY_MAX_WIDTH) return refusef("%s: table is %u x %u", who, t->width, t->height);
    if (src && (t->width != rtr_sky_table_width(src) || t->height != rtr_sky_table_height(src)))
        return refusef("%s: table is %u x %u, the sky's is %u x %u", who, t->width, t->height, rtr_sky_table_width(src), rtr_sky_table_height(src));
    return RTR_OK;
}

}  // namespace
}  // namespace rtrdev

extern "C" int rtr_host_sky_table(const rtr_texture* hdri, const float* skyColor, uint32_t* outWidth, uint32_t* outHeight, uint32_t* outRows,
                                  size_t capacityCells, uint64_t* outMarginal, uint32_t capacityRows) {
    const char* who = "rtr_host_sky_table";
    rtr_sky_source src;
    if (const int rc = rtrdev::sky_source(who, hdri, skyColor, &src)) return rc;
    const uint32_t W = rtr_sky_table_width(&src), H = rtr_sky_table_height(&src);
    if (outWidth) *outWidth = W;
    if (outHeight) *outHeight = H;
    if (!outRows || !outMarginal || capacityCells < (size_t)W * H || capacityRows < H)
        return rtrdev::refusef("%s: capacity %zu cells, %u rows; %zu and %u are needed", who, outRows ? capacityCells : (size_t)0,
                               outMarginal ? capacityRows : 0u, (size_t)W * H, H);
    uint64_t sum = 0;
    for (uint32_t y = 0; y < H; ++y) {
        uint32_t row = 0;
        for (uint32_t x = 0; x < W; ++x) { row += rtr_sky_weight(&src, x, y); outRows[(size_t)y * W + x] = row; }
        sum += row;
        outMarginal[y] = sum;
    }
    return RTR_OK;
}

extern "C" int rtr_host_sky_rays(const rtr_texture* hdri, const float* skyColor, const rtr_sky_table* table, const RtrRay* rays,
                                 const RtrSurface* surfaces, uint32_t n, const rtr_sky_params* p, const uint32_t* seeds, RtrRay* outRays,
                                 RtrSkySample* outSamples) {
    const char* who = "rtr_host_sky_rays";
    if (const int rc = rtrdev::sky_check_params(who, p, false)) return rc;
    if (const int rc = rtrdev::sky_check_rays_call(who, p, rays, surfaces, n, seeds, outRays, outSamples)) return rc;
    rtr_sky_source src;
    if (const int rc = rtrdev::sky_source(who, hdri, skyColor, &src)) return rc;
    if (const int rc = rtrdev::sky_check_table(who, &src, table)) return rc;
    const uint32_t S = p->numSamples;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t base = seeds ? seeds[k] : rtr_bounce_pixel_seed(k, p->width, p->spp);
        const uint32_t s0 = rtr_sky_seed(base, p->frame, p->depth);
        for (uint32_t j = 0; j < S; ++j) {
            float u1, u2;
            rtr_sky_randoms(s0, j, &u1, &u2);
            rtr_sky_vertex(&rays[k], &surfaces[k], &src, table, u1, u2, S, p->flags, p->lobes, &outRays[(size_t)k * S + j], &outSamples[(size_t)k * S + j]);
        }
    }
    return RTR_OK;
}

extern "C" int rtr_host_sky_hits(const rtr_texture* hdri, const float* skyColor, const rtr_sky_table* table, const RtrRay* rays, const RtrHit* hits,
                                 const RtrSurface* prevSurfaces, const RtrBounce* bounces, uint32_t n, const rtr_sky_params* p, RtrSkyEscape* out) {
    const char* who = "rtr_host_sky_hits";
    if (const int rc = rtrdev::sky_check_params(who, p, true)) return rc;
    if (n == 0) return RTR_OK;
    if (const int rc = rtrdev::sky_check_hits_arrays(who, rays, hits, prevSurfaces, bounces, n, out)) return rc;
    rtr_sky_source src;
    if (const int rc = rtrdev::sky_source(who, hdri, skyColor, &src)) return rc;
    if (const int rc = rtrdev::sky_check_table(who, &src, table)) return rc;
    for (uint32_t k = 0; k < n; ++k) {
        rtr_sky_escape_zero(&out[k]);
        if (hits[k].customIndex != 0xffffffffu) continue;
        rtr_sky_escape(&rays[k], prevSurfaces[k].kind, bounces[k].pdf, &src, table, p->numSamples, p->flags, &out[k]);
    }
    return RTR_OK;
}

extern "C" int rtr_host_sky_pdf(const rtr_sky_table* table, const float* dirs, uint32_t n, float* outPdf) {
    const char* who = "rtr_host_sky_pdf";
    if (const int rc = rtrdev::sky_check_table(who, nullptr, table)) return rc;
    if (n == 0) return RTR_OK;
    const rtrdev::Arg args[2] = {{dirs, "dirs", 4, true}, {outPdf, "outPdf", 4, true}};
    if (const int rc = rtrdev::check_ptrs(who, args)) return rc;
    for (uint32_t k = 0; k < n; ++k) outPdf[k] = rtr_sky_pdf(table, rtr_ld3(dirs + 3 * (size_t)k));
    return RTR_OK;
}

extern "C" int rtr_host_sky_radiance(const rtr_texture* hdri, const float* skyColor, const float* dirs, uint32_t n, float* out) {
    const char* who = "rtr_host_sky_radiance";
    rtr_sky_source src;
    if (const int rc = rtrdev::sky_source(who, hdri, skyColor, &src)) return rc;
    if (n == 0) return RTR_OK;
    const rtrdev::Arg args[2] = {{dirs, "dirs", 4, true}, {out, "out", 4, true}};
    if (const int rc = rtrdev::check_ptrs(who, args)) return rc;
    for (uint32_t k = 0; k < n; ++k) {
        const rtr_v3 r = rtr_sky_radiance(&src, rtr_ld3(dirs + 3 * (size_t)k));
        out[3 * (size_t)k] = r.x; out[3 * (size_t)k + 1] = r.y; out[3 * (size_t)k + 2] = r.z;
    }
    return RTR_OK;
}
