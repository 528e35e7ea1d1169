/* rtr_mis.h — the multiple-importance-sampling contract of rtr_mis_pick_weights and rtr_emitter_hits: the balance heuristic over the
 * P picked light samples of a path vertex (include/rtr_pick.h) and its one BRDF-sampled bounce (include/rtr_bounce.h).
 *
 * One definition for the host (rtr_host_bounce_pdf, rtr_host_mis_weights, rtr_host_emitter_hits) and the device (k_mis_pick_weights,
 * k_emitter_hits), in the terms of rtr_math.h: IEEE-754 binary32 + - * / rtr_sqrt and explicit rtr_fma, compiled with -ffp-contract=off
 * on both sides, so that the kernels' records can be held to the host's bits (tests/test_gpu_mis.py).  Uses rtr_math.h, rtr_types.h and
 * rtr_bounce.h only; the render kernels do not include this header.
 *
 * THE ESTIMATOR.  At a vertex x with shading normal N, light triangle t (area area_t, unit normal n_t, pdfrec_t =
 * 1 / (0.7 area_t)) seen in direction L at distance d, cosL = dot(n_t, -L): one pick has the solid-angle density
 * q = d^2 / (Ttot area_t |cosL|), the bounce has pb(L) (rtr_mis_bounce_pdf).  With s = d^2 / (Ttot area_t) the balance heuristic over P
 * picks and one bounce is, in the forms that do not divide by |cosL|,
 *     wPick = P s / (P s + pb |cosL|)        wBounce = pb |cosL| / (P s + pb |cosL|)
 * PICK SIDE: a pick's weight for rtr_shade_hits_picked is ((float)Ttot / (float)P) * wPick.
 * BOUNCE SIDE: a bounce ray that ends on light triangle t adds, per channel,
 *     radiance = (max(NL, 0.1) / NL) * (10 col I / (pdfrec_t area_t)) * pb / (P s + pb |cosL|)
 * times the throughput after the bounce (which holds f NL / pb): g / (P q + pb) with g = f max(NL, 0.1) 10 col I / (pdfrec_t area_t
 * |cosL|), the expression the pick side evaluates.  A light nobody picks from (its index >= numAreaLights, or Ttot == 0) has P s = 0.
 *
 * Used by: kernels/rtr_query.hip and kernels/rtr_mis.hip (device), rtr_mis_host.cpp (host).
 */
#ifndef RTR_MIS_H
#define RTR_MIS_H

#include "rtr_math.h"
#include "rtr_types.h"
#include "rtr_bounce.h"

/* The density rtr_bounce_sample divides by, for an arbitrary UNIT direction L: its expressions in its order, so that for the direction it
 * drew this is RtrBounce::pdf bit for bit (a record rtr_bounce_sample declared dead for its weight or origin has pdf 0 there and not
 * here).  The specular term is that of the evaluated half vector Hm = normalize(V + L) where dot(N, Hm) > 0 and nothing elsewhere:
 * rtr_bounce_sample drops a drawn half vector with dot(V, H) <= 0, so that Hm is the H every live specular sample was drawn with, also
 * for a view from behind the shading normal.  0 for a surface that is not an object, a float that is not finite,
 * no lobe to sample, dot(N, L) <= 0, or a density that is not positive and finite. */
RTR_HD float rtr_mis_bounce_pdf(const RtrRay* ray, const RtrSurface* sf, rtr_v3 L, uint32_t lobes) {
    if (sf->kind != RTR_SURFACE_OBJECT) return 0.0f;
    const rtr_v3 P = rtr_ld3(sf->position), N = rtr_ld3(sf->normal), color = rtr_ld3(sf->color), O = rtr_ld3(ray->origin);
    const float roughness = sf->roughness, metallic = sf->metallic;
    if (!(rtr_bounce_finite3(P) & rtr_bounce_finite3(N) & rtr_bounce_finite3(color) & rtr_bounce_finite3(O) & rtr_bounce_finite3(L) &
          rtr_bounce_finite(roughness) & rtr_bounce_finite(metallic))) return 0.0f;
    const rtr_v3 V = rtr_normalize(rtr_sub(O, P));
    if (!rtr_bounce_finite3(V)) return 0.0f;
    const float om = 1.0f - metallic;
    const rtr_v3 mDiffuse = rtr_scale(color, om);
    const rtr_v3 F0 = rtr_mk(rtr_fma(color.x, metallic, 0.04f * om), rtr_fma(color.y, metallic, 0.04f * om), rtr_fma(color.z, metallic, 0.04f * om));
    const float alpha2 = roughness * roughness;
    const float s = rtr_bounce_max3(F0), d = rtr_bounce_max3(mDiffuse);
    const int specOn = (alpha2 != 0.0f) & ((lobes & RTR_BOUNCE_SPECULAR) != 0u);
    const int diffOn = (d != 0.0f) & ((lobes & RTR_BOUNCE_DIFFUSE) != 0u);
    if (!(specOn | diffOn)) return 0.0f;
    const float pSpec = (specOn & diffOn) ? s / (s + d) : (specOn ? 1.0f : 0.0f);
    const float NoL = rtr_dot(N, L);
    if (!(NoL > 0.0f)) return 0.0f;
    const rtr_v3 Hm = rtr_normalize(rtr_add(V, L));
    const float NoH = rtr_dot(N, Hm);
    float VoH = rtr_dot(V, Hm);
    if (!(rtr_dot(N, V) > 0.0f) | !(VoH > 0.0f)) VoH = 0.5f * rtr_length(rtr_add(V, L));      /* V + L cancels near L = -V: as rtr_bounce_sample */
    const float pdfD = NoL / RTR_BOUNCE_PI_F;
    float pdfS = 0.0f;
    if (specOn & (NoH > 0.0f) & (VoH > 0.0f)) {
        const rtr_v3 NxH = rtr_cross(N, Hm);
        const float NoH2 = NoH * NoH;
        const float den = rtr_fma(NoH2, alpha2, rtr_dot(NxH, NxH));
        const float Dtrue = alpha2 / (RTR_BOUNCE_PI_F * den * den);
        pdfS = (Dtrue * NoH) / (4.0f * VoH);
    }
    const float pdf = rtr_fma(pSpec, pdfS, (1.0f - pSpec) * pdfD);
    if (!(pdf > 0.0f) || !rtr_bounce_finite(pdf)) return 0.0f;
    return pdf;
}

/* The two terms of the heuristic's denominator: a = P s (0 when nobody picks: Ttot == 0 or P == 0), b = pb |cosL| (0 for pb <= 0).
 * Roundings: d * d, (float)Ttot * area, their quotient and the product by (float)P make a (4); b has 1.  Ttot <= 2^24 and P <= 30 convert
 * exactly. */
RTR_HD void rtr_mis_terms(float pb, float dist, float cosLight, float area, uint32_t Ttot, uint32_t P, float* a, float* b) {
    *a = (Ttot != 0u && P != 0u) ? (float)P * ((dist * dist) / ((float)Ttot * area)) : 0.0f;
    *b = pb > 0.0f ? pb * rtr_abs(cosLight) : 0.0f;
}

/* lightPdf = q, wPick, wBounce of one direction.  pb == 0 gives wPick = 1 and wBounce = 0 exactly (a / (a + 0)); Ttot == 0 or P == 0 gives
 * 0 and 1; a + b == 0 (both, or d == 0 with pb == 0, or cosLight == 0 with nobody picking) gives 0 and 0.  An input that is not finite,
 * or a negative distance or area, gives three zeros; a sum that overflows with finite inputs (a tiny area) is all the pick's: 1 and 0.
 * lightPdf is 0 where s / |cosL| is not finite (cosLight == 0).  No output is ever a NaN or an infinity. */
RTR_HD void rtr_mis_weights(float pb, float dist, float cosLight, float area, uint32_t Ttot, uint32_t P, float* lightPdf, float* wPick, float* wBounce) {
    *lightPdf = 0.0f; *wPick = 0.0f; *wBounce = 0.0f;
    if (!(rtr_bounce_finite(pb) & rtr_bounce_finite(dist) & rtr_bounce_finite(cosLight) & rtr_bounce_finite(area))) return;
    if (dist < 0.0f || area < 0.0f) return;
    float a, b;
    rtr_mis_terms(pb, dist, cosLight, area, Ttot, P, &a, &b);
    const float sum = a + b;
    if (!(sum > 0.0f)) return;                            /* 0, or a NaN from 0 / 0 (d == 0 on a triangle without area) */
    if (Ttot != 0u) {
        const float q = ((dist * dist) / ((float)Ttot * area)) / rtr_abs(cosLight);
        if (rtr_bounce_finite(q)) *lightPdf = q;
    }
    if (!rtr_bounce_finite(sum)) {                        /* b is finite (pb and cosLight are): a overflowed */
        if (rtr_bounce_finite(b)) *wPick = 1.0f;
        return;
    }
    *wPick = a / sum;
    *wBounce = b / sum;
}

RTR_HD void rtr_mis_emitter_zero(RtrEmitter* e) {
    e->radiance[0] = e->radiance[1] = e->radiance[2] = 0.0f; e->wBounce = 0.0f;
    e->lightPdf = 0.0f; e->dist = 0.0f; e->lightTri = 0u; e->kind = 0u;
}

/* What the bounce side measures of one ray before any pick density enters: pb (the vertex's bounce density), NL = dot(N, L), d (the
 * distance from x), cosL = dot(n_t, -L), and the area and pdfrec words of the record.  Shared by rtr_mis_emitter and
 * rtr_power_mis_emitter (include/rtr_power.h), which differ in the pick term alone. */
typedef struct rtr_mis_emitter_geom { float pb, NL, d, cosL, area, pdfrec; } rtr_mis_emitter_geom;

/* 0 where the record stays zeros: a previous surface that is not an object, pb <= 0, NL <= 0, d == 0, a one-sided light met from behind
 * (dot(n_t, x - P0) < 0, the light loops' test), or anything not finite on the way.  d is measured from x, not from the ray's origin
 * normalOffset above it, and the ray does not stop 0.5 short as a shadow ray does. */
RTR_HD int rtr_mis_emitter_measure(const RtrRay* ray, float t, const RtrSurface* prev, const RtrBounce* bounce, const float* rec, uint32_t twoSided,
                                   rtr_mis_emitter_geom* g) {
    if (prev->kind != RTR_SURFACE_OBJECT) return 0;
    const float pb = bounce->pdf;
    if (!(pb > 0.0f) || !rtr_bounce_finite(pb)) return 0;
    const rtr_v3 o = rtr_ld3(ray->origin), dir = rtr_ld3(ray->direction), x = rtr_ld3(prev->position), N = rtr_ld3(prev->normal);
    if (!(rtr_bounce_finite3(o) & rtr_bounce_finite3(dir) & rtr_bounce_finite3(x) & rtr_bounce_finite3(N) & rtr_bounce_finite(t))) return 0;
    const rtr_v3 L = rtr_normalize(dir);
    if (!rtr_bounce_finite3(L)) return 0;
    const float NL = rtr_dot(N, L);
    if (!(NL > 0.0f)) return 0;
    const rtr_v3 y = rtr_madd(o, dir, t);
    const float d = rtr_length(rtr_sub(y, x));
    if (!(d > 0.0f) || !rtr_bounce_finite(d)) return 0;
    const rtr_v3 P0 = rtr_ld3(rec), nt = rtr_ld3(rec + 12);
    if (twoSided == 0u) {
        if (rtr_dot(nt, rtr_sub(x, P0)) < 0.0f) return 0;
    }
    g->pb = pb; g->NL = NL; g->d = d; g->cosL = rtr_dot(nt, rtr_neg(L)); g->area = rec[3]; g->pdfrec = rec[7];
    return 1;
}

/* The record of a measured ray once the heuristic's terms are known: a, b of the denominator, lightPdf and wBounce of the weights. */
RTR_HD void rtr_mis_emitter_record(const rtr_mis_emitter_geom* m, float a, float b, float lightPdf, float wBounce, uint32_t lightTri,
                                   const float* lightColor, float intensity, RtrEmitter* e) {
    const float sum = a + b;
    const float g = m->pb / sum;
    const float k = rtr_max(m->NL, 0.1f) / m->NL;
    const float den = m->pdfrec * m->area;
    const rtr_v3 E = rtr_mk(((10.0f * lightColor[0]) * intensity) / den, ((10.0f * lightColor[1]) * intensity) / den, ((10.0f * lightColor[2]) * intensity) / den);
    const rtr_v3 rad = rtr_mk((k * E.x) * g, (k * E.y) * g, (k * E.z) * g);
    if (!rtr_bounce_finite3(rad)) return;
    e->radiance[0] = rad.x; e->radiance[1] = rad.y; e->radiance[2] = rad.z; e->wBounce = wBounce;
    e->lightPdf = lightPdf; e->dist = m->d; e->lightTri = lightTri; e->kind = RTR_SURFACE_LIGHT;
}

/* The whole per-ray function of the bounce side.  ray: the bounce ray (its direction need not be normalised; t is in its units); t: its
 * closest hit's parameter; prev: the RtrSurface of the vertex it left (x, N); bounce: that vertex's RtrBounce (pb = pdf); rec: the 16
 * floats of the light triangle's record {P0, area} {P1, pdfrec} {P2, -} {n_t, -}; lightTri: that record's index; lightColor, intensity,
 * twoSided: its light's words; sampled: the light is one of the first numAreaLights (the picks can reach it).  The caller has made sure
 * that the hit is a triangle of a light.  Zeros (rtr_mis_emitter_zero) where rtr_mis_emitter_measure gives 0. */
RTR_HD void rtr_mis_emitter(const RtrRay* ray, float t, const RtrSurface* prev, const RtrBounce* bounce, const float* rec, uint32_t lightTri,
                            const float* lightColor, float intensity, uint32_t twoSided, int sampled, uint32_t Ttot, uint32_t P, RtrEmitter* e) {
    rtr_mis_emitter_zero(e);
    rtr_mis_emitter_geom m;
    if (!rtr_mis_emitter_measure(ray, t, prev, bounce, rec, twoSided, &m)) return;
    const uint32_t tt = sampled ? Ttot : 0u;
    float a, b;
    rtr_mis_terms(m.pb, m.d, m.cosL, m.area, tt, P, &a, &b);
    float lightPdf, wPick, wBounce;
    rtr_mis_weights(m.pb, m.d, m.cosL, m.area, tt, P, &lightPdf, &wPick, &wBounce);
    rtr_mis_emitter_record(&m, a, b, lightPdf, wBounce, lightTri, lightColor, intensity, e);
}

#endif /* RTR_MIS_H */
