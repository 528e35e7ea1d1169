/* rtr_bounce.h — the sampling contract of rtr_bounce_rays: the continuation ray of a hit and its throughput weight.
 *
 * One definition for the host (rtr_host_bounce_rays) and the device (k_bounce_rays), in the terms of rtr_math.h: IEEE-754 binary32
 * + - * / rtr_sqrt and explicit rtr_fma, no libm, no ocml, compiled with -ffp-contract=off on both sides, so that the kernel's records
 * can be held to the host's bits (tests/test_gpu_bounce.py).  The BRDF is the renderer's: GGX_Distribution, GGX_PartialGeometryTerm,
 * Fresnel_Schlick and the sum area_sample_contrib forms are restated here operation for operation from kernels/rtr_device.h under
 * rtr_bounce_* names (the render kernels do not include this header: their code cannot move with it).
 *
 * The estimator: one direction from the mixture of a cosine lobe and the GGX half-vector lobe with alpha =
 * roughness, chosen by the larger channels of F0 and of the diffuse colour, weighted by the one-sample balance heuristic:
 * weight = BRDF * cos / (pSpec * pdfS + (1 - pSpec) * pdfD).
 *
 * Used by: kernels/rtr_bounce.hip (device), rtr_bounce_host.cpp (host).
 */
#ifndef RTR_BOUNCE_H
#define RTR_BOUNCE_H

#include "rtr_math.h"
#include "rtr_types.h"

#define RTR_BOUNCE_PI_F 3.14159265359f      /* RTR_PI_F of kernels/rtr_device.h */

RTR_HD int rtr_bounce_finite(float x) { return (rtr_f2u(x) & 0x7f800000u) != 0x7f800000u; }
RTR_HD int rtr_bounce_finite3(rtr_v3 a) { return rtr_bounce_finite(a.x) & rtr_bounce_finite(a.y) & rtr_bounce_finite(a.z); }
RTR_HD float rtr_bounce_max3(rtr_v3 a) { return rtr_max(rtr_max(a.x, a.y), a.z); }

/* sin(2 pi u) and cos(2 pi u) for u in [0, 1] (1.0 included: rtr_random returns it, quirk Q2).  m = 8u counts octants and is exact;
 * q = the nearest quarter turn, r = m - 2q in [-1, 1] octants is exact as well (both are multiples of ulp(m), and the difference is
 * the smaller), so the only rounding of the reduction is x = r * pi/4, |x| <= pi/4.  There the degree-7 / degree-8 minimax forms of
 * the Cephes single-precision sine and cosine, then the quarter turns as swaps and signs: u = 0, 1/4, 1/2, 3/4, 1 give 0 and +-1
 * exactly.  Measured against float64 over 2^20 + 1 evenly spaced u, both ends and the octant boundaries +- 1 ULP: |err| <= 1.01e-7 for
 * either output and |s^2 + c^2 - 1| <= 1.49e-7; tests/test_bounce_host.py asserts 2.2e-7 for all three. */
RTR_HD void rtr_sincos_turn(float u, float* s_out, float* c_out) {
    const float m = u * 8.0f;
    const uint32_t q = (uint32_t)(int32_t)rtr_fma(u, 4.0f, 0.5f);      /* 0 ... 4; truncation is the floor of a value >= 0.5 */
    const float r = m - 2.0f * (float)q;
    const float x = r * 0.78539816339744831f;
    const float z = x * x;
    float ps = -1.9515295891e-4f;
    ps = rtr_fma(ps, z, 8.3321608736e-3f);
    ps = rtr_fma(ps, z, -1.6666654611e-1f);
    const float s = rtr_fma(ps * z, x, x);
    float pc = 2.443315711809948e-5f;
    pc = rtr_fma(pc, z, -1.388731625493765e-3f);
    pc = rtr_fma(pc, z, 4.166664568298827e-2f);
    const float c = rtr_fma(pc * z, z, rtr_fma(-0.5f, z, 1.0f));
    const uint32_t k = q & 3u;
    const float ss = (k & 1u) ? c : s, cc = (k & 1u) ? s : c;
    *s_out = (k & 2u) ? -ss : ss;
    *c_out = (k == 1u || k == 2u) ? -cc : cc;
}

/* An orthonormal basis (t, b, n) from a unit normal without a branch on the data: Duff et al., "Building an Orthonormal Basis,
 * Revisited" (JCGT 2017).  GGX is isotropic here, so any tangent frame serves; the reference's normalize(V - N dot(N, V)) is NaN for
 * V parallel to N and is not used. */
RTR_HD void rtr_bounce_basis(rtr_v3 n, rtr_v3* t, rtr_v3* b) {
    const float sign = n.z >= 0.0f ? 1.0f : -1.0f;
    const float a = -1.0f / (sign + n.z);
    const float c = (n.x * n.y) * a;
    *t = rtr_mk(rtr_fma((sign * n.x) * n.x, a, 1.0f), sign * c, -(sign * n.x));
    *b = rtr_mk(c, rtr_fma(n.y * n.y, a, sign), -n.y);
}

/* ---- cook-torrance.glsl as kernels/rtr_device.h:370-390 states it ---------------------------------------------------------------- */
RTR_HD float rtr_bounce_chi(float v) { return v > 0.0f ? 1.0f : 0.0f; }
RTR_HD float rtr_bounce_ggx_d(rtr_v3 n, rtr_v3 h, float alpha) {
    const float NoH = rtr_dot(n, h);
    const float alpha2 = alpha * alpha;
    const float NoH2 = NoH * NoH;
    const float den = rtr_max(rtr_fma(NoH2, alpha2, 1.0f - NoH2), 0.001f);
    return (rtr_bounce_chi(NoH) * alpha2) / (RTR_BOUNCE_PI_F * den * den);
}
RTR_HD float rtr_bounce_ggx_g1(rtr_v3 v, rtr_v3 n, rtr_v3 h, float alpha) {
    float VoH2 = rtr_clamp(rtr_dot(v, h), 0.001f, 1.0f);
    const float chi = rtr_bounce_chi(VoH2 / rtr_clamp(rtr_dot(v, n), 0.001f, 1.0f));
    VoH2 = VoH2 * VoH2;
    const float tan2 = (1.0f - VoH2) / VoH2;
    return (chi * 2.0f) / (1.0f + rtr_sqrt(rtr_fma(alpha * alpha, tan2, 1.0f)));
}
RTR_HD rtr_v3 rtr_bounce_fresnel(float cosT, rtr_v3 F0) {
    const float p = rtr_pow(1.0f - cosT, 5.0f);
    return rtr_mk(rtr_fma(1.0f - F0.x, p, F0.x), rtr_fma(1.0f - F0.y, p, F0.y), rtr_fma(1.0f - F0.z, p, F0.z));
}
/* currSpecular + currDiffuse of one sample, as area_sample_contrib forms them (kernels/rtr_device.h:609-627): NdotV and NdotL clamped
 * at 0.1 in the denominator, the products in GLSL's left-to-right order; currDiffuse = (om * color) / pi per channel. */
RTR_HD rtr_v3 rtr_bounce_brdf(rtr_v3 hitNormal, rtr_v3 viewDir, rtr_v3 lightDir, float roughness, rtr_v3 mSpecular, float om, rtr_v3 color) {
    const rtr_v3 halfVector = rtr_normalize(rtr_add(viewDir, lightDir));
    const float cosTheta = rtr_clamp(rtr_dot(viewDir, halfVector), 0.0f, 1.0f);
    const float Dg = rtr_bounce_ggx_d(hitNormal, halfVector, roughness);
    const float G = rtr_bounce_ggx_g1(viewDir, hitNormal, halfVector, roughness) * rtr_bounce_ggx_g1(lightDir, hitNormal, halfVector, roughness);
    const rtr_v3 F = rtr_bounce_fresnel(cosTheta, mSpecular);
    const float NdotV = rtr_max(rtr_dot(hitNormal, viewDir), 0.1f);
    const float NdotL = rtr_max(rtr_dot(hitNormal, lightDir), 0.1f);
    const float den = 4.0f * NdotV * NdotL;
    const rtr_v3 currSpecular = rtr_mk(((Dg * F.x) * G) / den, ((Dg * F.y) * G) / den, ((Dg * F.z) * G) / den);
    const rtr_v3 currDiffuse = rtr_mk((om * color.x) / RTR_BOUNCE_PI_F, (om * color.y) / RTR_BOUNCE_PI_F, (om * color.z) / RTR_BOUNCE_PI_F);
    return rtr_add(currSpecular, currDiffuse);
}

/* The dead record: the null ray (eight zero floats, which every query answers without a walk) and an all-zero RtrBounce. */
RTR_HD void rtr_bounce_dead(RtrRay* next, RtrBounce* b) {
    next->origin[0] = next->origin[1] = next->origin[2] = 0.0f; next->tmin = 0.0f;
    next->direction[0] = next->direction[1] = next->direction[2] = 0.0f; next->tmax = 0.0f;
    b->weight[0] = b->weight[1] = b->weight[2] = 0.0f; b->pdf = 0.0f;
    b->lobe = 0u; b->pSpecular = 0.0f; b->_reserved[0] = b->_reserved[1] = 0u;
}

/* The whole per-hit function.  ray: the ray that found the hit (its origin gives the view vector, as in rtr_light_rays); sf: the hit's
 * RtrSurface; seedBase: seeds[k] or the pixel's px * 733 + py * 1933.  A record is DEAD (rtr_bounce_dead) when the surface is not an
 * object, a float it uses is not finite, no lobe that was asked for can be sampled, the specular lobe drew a half vector on the far side
 * of the view (dot(V, H) <= 0: DESIGN.md section 3, views from behind the shading normal), the direction leaves below the surface
 * (dot(N, L) <= 0), the mixture pdf is <= 0 or not finite, or a weight channel is negative or not finite.  No output word is ever a
 * NaN or an infinity. */
RTR_HD void rtr_bounce_sample(const RtrRay* ray, const RtrSurface* sf, uint32_t seedBase, const rtr_bounce_params* p, RtrRay* next, RtrBounce* b) {
    rtr_bounce_dead(next, b);
    if (sf->kind != RTR_SURFACE_OBJECT) return;
    const rtr_v3 P = rtr_ld3(sf->position), N = rtr_ld3(sf->normal), color = rtr_ld3(sf->color), O = rtr_ld3(ray->origin);
    const float roughness = sf->roughness, metallic = sf->metallic;
    if (!(rtr_bounce_finite3(P) & rtr_bounce_finite3(N) & rtr_bounce_finite3(color) & rtr_bounce_finite3(O) &
          rtr_bounce_finite(roughness) & rtr_bounce_finite(metallic))) return;
    const rtr_v3 V = rtr_normalize(rtr_sub(O, P));
    if (!rtr_bounce_finite3(V)) return;                 /* a ray that starts at its hit has no view vector (the clamps below would swallow the NaN) */
    const float om = 1.0f - metallic;
    const rtr_v3 mDiffuse = rtr_scale(color, om);
    const rtr_v3 F0 = rtr_mk(rtr_fma(color.x, metallic, 0.04f * om), rtr_fma(color.y, metallic, 0.04f * om), rtr_fma(color.z, metallic, 0.04f * om));
    const float alpha2 = roughness * roughness;

    const uint32_t s0 = seedBase + p->frame + 7919u * (p->depth + 1u);
    const float u1 = rtr_random(s0), u2 = rtr_random(s0 + 100u), uLobe = rtr_random(s0 + 200u);

    const float s = rtr_bounce_max3(F0), d = rtr_bounce_max3(mDiffuse);
    const int specOn = (alpha2 != 0.0f) & ((p->lobes & RTR_BOUNCE_SPECULAR) != 0u);      /* the renderer's D is 0 at alpha2 == 0 */
    const int diffOn = (d != 0.0f) & ((p->lobes & RTR_BOUNCE_DIFFUSE) != 0u);
    if (!(specOn | diffOn)) return;
    const float pSpec = (specOn & diffOn) ? s / (s + d) : (specOn ? 1.0f : 0.0f);
    const int takeSpec = specOn & (!diffOn | (uLobe < pSpec));

    rtr_v3 T, B;
    rtr_bounce_basis(N, &T, &B);
    float sn, cs;
    rtr_sincos_turn(u2, &sn, &cs);
    rtr_v3 L;
    if (takeSpec) {
        /* cos^2 = (1 - u1) / (1 + (alpha2 - 1) u1) and sin^2 = 1 - cos^2 in the forms that do not cancel: alpha2 - 1 rounds a small
         * alpha2 away (3 % of it at roughness 0.001), 1 - cos^2 the small angle */
        const float den = rtr_fma(alpha2, u1, 1.0f - u1);
        const float cosT = rtr_sqrt((1.0f - u1) / den), sinT = rtr_sqrt((alpha2 * u1) / den);
        const rtr_v3 H = rtr_normalize(rtr_madd(rtr_madd(rtr_scale(T, sinT * cs), B, sinT * sn), N, cosT));
        /* A half vector on the far side of the view has no specular sample.  Seen from above (dot(N, V) > 0) its reflection leaves below
         * the surface and was dead already; seen from behind the shading normal it can leave above it, dot(N, L) = 2 VoH NoH - NoV > 0,
         * in a direction whose evaluated half vector is -H, where the density below has no specular term (its NoH > 0 guard, and the
         * renderer's chi(NoH)): the record would be live with a density it was not drawn from.  With VoH > 0, normalize(V + L) is H. */
        const float VoHs = rtr_dot(V, H);
        if (!(VoHs > 0.0f)) return;
        L = rtr_normalize(rtr_sub(rtr_scale(H, 2.0f * VoHs), V));
    } else {
        const float r = rtr_sqrt(u1);
        L = rtr_normalize(rtr_madd(rtr_madd(rtr_scale(T, r * cs), B, r * sn), N, rtr_sqrt(rtr_max(1.0f - u1, 0.0f))));
    }
    const float NoL = rtr_dot(N, L);
    if (!(NoL > 0.0f)) return;                                                            /* below the surface, or a NaN on the way */

    /* the balance heuristic over the lobes that are on; the density of the specular lobe is the UNCLAMPED GGX the directions are drawn
     * from (the max(den, 0.001) of GGX_Distribution belongs to the BRDF) */
    const rtr_v3 Hm = rtr_normalize(rtr_add(V, L));
    const float NoH = rtr_dot(N, Hm);
    float VoH = rtr_dot(V, Hm);
    /* V + L cancels for L near -V, where the specular density has its 1 / VoH singularity: the sum is 2 VoH long and its float32 components
     * are good to 6e-8 absolute, so that Hm is good to 3e-8 / VoH and dot(V, Hm), nearly at right angles to V, to no more than that
     * ABSOLUTE: 30 % of a VoH of 3e-4, and no sign left below 2e-4, which used to strike the specular term from a density that is at its
     * largest there.  |V + L| / 2 is the same number and keeps its digits (3e-8 / VoH RELATIVE).  A view from above keeps the bits of the
     * dot product: alive, it is never near -V (dot(N, L) = 2 VoH NoH - NoV).  A view from behind or along the surface (dot(N, V) <= 0),
     * which is, takes the length, and so does any record whose dot product has lost its sign. */
    if (!(rtr_dot(N, V) > 0.0f) | !(VoH > 0.0f)) VoH = 0.5f * rtr_length(rtr_add(V, L));
    const float pdfD = NoL / RTR_BOUNCE_PI_F;
    float pdfS = 0.0f;
    if (specOn & (NoH > 0.0f) & (VoH > 0.0f)) {
        /* 1 - NoH^2 as |N x H|^2: near the peak of a narrow lobe the subtraction would keep no digit of a den that is about alpha2 */
        const rtr_v3 NxH = rtr_cross(N, Hm);
        const float NoH2 = NoH * NoH;
        const float den = rtr_fma(NoH2, alpha2, rtr_dot(NxH, NxH));
        const float Dtrue = alpha2 / (RTR_BOUNCE_PI_F * den * den);
        pdfS = (Dtrue * NoH) / (4.0f * VoH);
    }
    const float pdf = rtr_fma(pSpec, pdfS, (1.0f - pSpec) * pdfD);
    if (!(pdf > 0.0f) || !rtr_bounce_finite(pdf)) return;

    const rtr_v3 brdf = rtr_bounce_brdf(N, V, L, roughness, F0, om, color);
    const rtr_v3 w = rtr_mk((brdf.x * NoL) / pdf, (brdf.y * NoL) / pdf, (brdf.z * NoL) / pdf);
    if (!(rtr_bounce_finite3(w) & (w.x >= 0.0f) & (w.y >= 0.0f) & (w.z >= 0.0f))) return;
    const rtr_v3 origin = rtr_madd(P, N, p->normalOffset);
    if (!(rtr_bounce_finite3(origin) & rtr_bounce_finite3(L))) return;

    next->origin[0] = origin.x; next->origin[1] = origin.y; next->origin[2] = origin.z; next->tmin = p->tmin;
    next->direction[0] = L.x; next->direction[1] = L.y; next->direction[2] = L.z; next->tmax = p->tmax;
    b->weight[0] = w.x; b->weight[1] = w.y; b->weight[2] = w.z; b->pdf = pdf;
    b->lobe = takeSpec ? RTR_BOUNCE_SPECULAR : RTR_BOUNCE_DIFFUSE; b->pSpecular = pSpec;
}

/* seedBase of hit k without explicit seeds: the pixel rtr_camera_rays' order gives it (rtr_light_rays' rule) */
RTR_HD uint32_t rtr_bounce_pixel_seed(uint32_t k, uint32_t width, uint32_t spp) {
    const uint32_t pix = k / spp;
    return (pix % width) * 733u + (pix / width) * 1933u;
}

#endif /* RTR_BOUNCE_H */
