/* math_ops.h — the op table of the numerical-contract probe (TEST INFRASTRUCTURE).
 *
 * Every function of include/rtr_math.h that computes something, as a pure op  (const uint32_t* in, uint32_t* out)  with fixed counts
 * of input and output words.  The table is compiled twice: by hipcc for gfx950 with the product's own flags (math_probe.hip ->
 * libmath_probe.so) and by the oracle's compiler with the oracle's flags (math_probe_host.cpp -> libmath_probe_host.so).
 * tests/test_gpu_math_contract.py holds the two compiles to the same bits; tests/test_math_contract.py holds the host compile to
 * float64 references.
 *
 * The device-only restatements of rtr_slab_q in kernels/rtr_device.h (slab_pair, slab_oct<k>, slab_wide<k, EXIT>) are ops of the
 * same table: the device compile runs the device form, the host compile runs what the form claims to equal, in rtr_math.h terms.
 * math_probe.hip defines PROBE_DEVICE_FORMS after including rtr_device.h to select them.
 */
#ifndef RTR_MATH_OPS_H
#define RTR_MATH_OPS_H

#include "../../include/rtr_math.h"

#if defined(PROBE_DEVICE_FORMS) && RTR_DEVICE_CODE
#define PROBE_DEV 1
#else
#define PROBE_DEV 0
#endif

#define PROBE_CHUNK_LOG2 20          /* a sweep folds 2^20 consecutive patterns into one digest */

#define PF(k) rtr_u2f(in[k])
#define PV(k) rtr_mk(rtr_u2f(in[k]), rtr_u2f(in[(k) + 1]), rtr_u2f(in[(k) + 2]))
#define PU(f) rtr_f2u(f)

/* 64-bit mix of (pattern, result words); a sweep's digest is the sum modulo 2^64 of these, so it does not depend on the order of
 * evaluation.  fmask bit k: result word k is a float, and any NaN in it folds as 0x7fc00000 (the contract promises no NaN sign or
 * payload). */
RTR_HD uint64_t probe_mix(uint32_t pattern, const uint32_t* r, int nout, uint32_t fmask) {
    uint64_t h = ((uint64_t)pattern + 1u) * 0x9E3779B97F4A7C15ull;
    for (int k = 0; k < nout; ++k) {
        uint32_t w = r[k];
        if (((fmask >> k) & 1u) && (w & 0x7fffffffu) > 0x7f800000u) w = 0x7fc00000u;
        h ^= w;
        h *= 0xBF58476D1CE4E5B9ull;
        h ^= h >> 29;
    }
    h *= 0x94D049BB133111EBull;
    h ^= h >> 32;
    return h;
}

/* binary16 -> binary32, exact (what v_fma_mix / (float)_Float16 do), in integer terms so that both compiles mean the same */
RTR_HD float probe_half(uint32_t h) {
    const uint32_t s = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    if (e == 0) return rtr_u2f(rtr_f2u((float)m * 5.9604644775390625e-08f) | s);      /* m * 2^-24, exact */
    if (e == 31) return rtr_u2f(s | 0x7f800000u | (m << 13));
    return rtr_u2f(s | ((e + 112u) << 23) | (m << 13));
}

/* ---- scalar helpers ---- */
RTR_HD void op_fma(const uint32_t* in, uint32_t* out) { out[0] = PU(rtr_fma(PF(0), PF(1), PF(2))); }
RTR_HD void op_sqrt(const uint32_t* in, uint32_t* out) { out[0] = PU(rtr_sqrt(PF(0))); }
RTR_HD void op_min(const uint32_t* in, uint32_t* out) { out[0] = PU(rtr_min(PF(0), PF(1))); }
RTR_HD void op_max(const uint32_t* in, uint32_t* out) { out[0] = PU(rtr_max(PF(0), PF(1))); }
RTR_HD void op_clamp(const uint32_t* in, uint32_t* out) { out[0] = PU(rtr_clamp(PF(0), PF(1), PF(2))); }
RTR_HD void op_hwmin(const uint32_t* in, uint32_t* out) { out[0] = PU(rtr_hwmin(PF(0), PF(1))); }
RTR_HD void op_hwmax(const uint32_t* in, uint32_t* out) { out[0] = PU(rtr_hwmax(PF(0), PF(1))); }
/* ---- random ---- */
RTR_HD void op_pcg_hash(const uint32_t* in, uint32_t* out) { out[0] = rtr_pcg_hash(in[0]); }
RTR_HD void op_random(const uint32_t* in, uint32_t* out) { out[0] = PU(rtr_random(in[0])); }
/* ---- vector ---- */
RTR_HD void op_dot(const uint32_t* in, uint32_t* out) { out[0] = PU(rtr_dot(PV(0), PV(3))); }
RTR_HD void op_cross(const uint32_t* in, uint32_t* out) {
    const rtr_v3 r = rtr_cross(PV(0), PV(3));
    out[0] = PU(r.x); out[1] = PU(r.y); out[2] = PU(r.z);
}
RTR_HD void op_normalize(const uint32_t* in, uint32_t* out) {
    const rtr_v3 r = rtr_normalize(PV(0));
    out[0] = PU(r.x); out[1] = PU(r.y); out[2] = PU(r.z);
}
RTR_HD void op_length(const uint32_t* in, uint32_t* out) { out[0] = PU(rtr_length(PV(0))); }
/* ---- transforms: the matrix first, then the point ---- */
RTR_HD void op_xform_point34(const uint32_t* in, uint32_t* out) {
    float m[12];
    for (int k = 0; k < 12; ++k) m[k] = PF(k);
    const rtr_v3 r = rtr_xform_point34(m, PV(12));
    out[0] = PU(r.x); out[1] = PU(r.y); out[2] = PU(r.z);
}
RTR_HD void op_xform_point44cm(const uint32_t* in, uint32_t* out) {
    float m[16];
    for (int k = 0; k < 16; ++k) m[k] = PF(k);
    const rtr_v3 r = rtr_xform_point44cm(m, PV(16));
    out[0] = PU(r.x); out[1] = PU(r.y); out[2] = PU(r.z);
}
RTR_HD void op_mul33(const uint32_t* in, uint32_t* out) {
    float m[9];
    for (int k = 0; k < 9; ++k) m[k] = PF(k);
    const rtr_v3 r = rtr_mul33(m, PV(9));
    out[0] = PU(r.x); out[1] = PU(r.y); out[2] = PU(r.z);
}
RTR_HD void op_normal_matrix(const uint32_t* in, uint32_t* out) {
    float m[12], o[9];
    for (int k = 0; k < 12; ++k) m[k] = PF(k);
    rtr_normal_matrix(m, o);
    for (int k = 0; k < 9; ++k) out[k] = PU(o[k]);
}
/* ---- transcendentals ---- */
RTR_HD void op_log2(const uint32_t* in, uint32_t* out) { out[0] = PU(rtr_log2(PF(0))); }
RTR_HD void op_exp2(const uint32_t* in, uint32_t* out) { out[0] = PU(rtr_exp2(PF(0))); }
RTR_HD void op_pow(const uint32_t* in, uint32_t* out) { out[0] = PU(rtr_pow(PF(0), PF(1))); }
RTR_HD void op_pow_2_2(const uint32_t* in, uint32_t* out) { out[0] = PU(rtr_pow(PF(0), 2.2f)); }
RTR_HD void op_pow_inv_2_2(const uint32_t* in, uint32_t* out) { out[0] = PU(rtr_pow(PF(0), 0.45454545454545453f)); }
RTR_HD void op_pow_5(const uint32_t* in, uint32_t* out) { out[0] = PU(rtr_pow(PF(0), 5.0f)); }
RTR_HD void op_atan_small(const uint32_t* in, uint32_t* out) { out[0] = PU(rtr_atan_small(PF(0))); }
RTR_HD void op_atan2(const uint32_t* in, uint32_t* out) { out[0] = PU(rtr_atan2(PF(0), PF(1))); }
RTR_HD void op_atan2_y1(const uint32_t* in, uint32_t* out) { out[0] = PU(rtr_atan2(PF(0), 1.0f)); }      /* atan2(., 1) */
RTR_HD void op_atan2_1x(const uint32_t* in, uint32_t* out) { out[0] = PU(rtr_atan2(1.0f, PF(0))); }      /* atan2(1, .) */
RTR_HD void op_acos(const uint32_t* in, uint32_t* out) { out[0] = PU(rtr_acos(PF(0))); }
/* ---- UNORM8 and division ---- */
RTR_HD void op_unorm8_to_float(const uint32_t* in, uint32_t* out) { out[0] = PU(rtr_unorm8_to_float(in[0])); }
RTR_HD void op_div_by(const uint32_t* in, uint32_t* out) { out[0] = PU(rtr_div_by(PF(0), PF(1), PF(2))); }
/* ---- ray setup and boxes ---- */
RTR_HD void op_safe_rcp_dir(const uint32_t* in, uint32_t* out) { out[0] = PU(rtr_safe_rcp_dir(PF(0))); }
/* bmin[3], bmax[3], idir, ood, tmin, tmax -> decision, t_entry */
RTR_HD void op_slab(const uint32_t* in, uint32_t* out) {
    float bmin[3] = {PF(0), PF(1), PF(2)}, bmax[3] = {PF(3), PF(4), PF(5)}, te;
    out[0] = (uint32_t)rtr_slab(bmin, bmax, PV(6), PV(9), PF(12), PF(13), &te);
    out[1] = PU(te);
}
RTR_HD void op_grid_from_bounds(const uint32_t* in, uint32_t* out) {
    float bmin[3] = {PF(0), PF(1), PF(2)}, bmax[3] = {PF(3), PF(4), PF(5)}, origin[3], scale[3];
    rtr_grid_from_bounds(bmin, bmax, origin, scale);
    for (int k = 0; k < 3; ++k) { out[k] = PU(origin[k]); out[3 + k] = PU(scale[k]); }
}
RTR_HD void op_quant_lo(const uint32_t* in, uint32_t* out) { out[0] = rtr_quant_lo(PF(0), PF(1), PF(2)); }
RTR_HD void op_quant_hi(const uint32_t* in, uint32_t* out) { out[0] = rtr_quant_hi(PF(0), PF(1), PF(2)); }
/* o, idir, origin[3], scale[3] -> ga, gb */
RTR_HD void op_ray_grid(const uint32_t* in, uint32_t* out) {
    float origin[3] = {PF(6), PF(7), PF(8)}, scale[3] = {PF(9), PF(10), PF(11)};
    rtr_v3 ga, gb;
    rtr_ray_grid(PV(0), PV(3), origin, scale, &ga, &gb);
    out[0] = PU(ga.x); out[1] = PU(ga.y); out[2] = PU(ga.z); out[3] = PU(gb.x); out[4] = PU(gb.y); out[5] = PU(gb.z);
}
/* origin[3], scale[3], centreXY, centreZ -> centre */
RTR_HD void op_wide_centre_world(const uint32_t* in, uint32_t* out) {
    float origin[3] = {PF(0), PF(1), PF(2)}, scale[3] = {PF(3), PF(4), PF(5)};
    const rtr_v3 r = rtr_wide_centre_world(origin, scale, in[6], in[7]);
    out[0] = PU(r.x); out[1] = PU(r.y); out[2] = PU(r.z);
}
/* o, idir, scale, centreWorld -> ga, gbc */
RTR_HD void op_ray_grid_about(const uint32_t* in, uint32_t* out) {
    rtr_v3 ga, gb;
    rtr_ray_grid_about(PV(0), PV(3), PV(6), PV(9), &ga, &gb);
    out[0] = PU(ga.x); out[1] = PU(ga.y); out[2] = PU(ga.z); out[3] = PU(gb.x); out[4] = PU(gb.y); out[5] = PU(gb.z);
}
/* qmin[3], qmax[3] (words), ga, gb, tmin, tmax -> decision, t_entry */
RTR_HD void op_slab_q(const uint32_t* in, uint32_t* out) {
    float te;
    out[0] = (uint32_t)rtr_slab_q(in[0], in[1], in[2], in[3], in[4], in[5], PV(6), PV(9), PF(12), PF(13), &te);
    out[1] = PU(te);
}
/* ---- triangle: o, d, v0, e1, e2, tmin -> hit, t, u, v (0 where the function leaves them unset) ---- */
RTR_HD void op_mt_intersect(const uint32_t* in, uint32_t* out) {
    float t = 0.0f, u = 0.0f, v = 0.0f;
    out[0] = (uint32_t)rtr_mt_intersect(PV(0), PV(3), PV(6), PV(9), PV(12), PF(15), &t, &u, &v);
    out[1] = PU(t); out[2] = PU(u); out[3] = PU(v);
}
/* ---- tone map ---- */
RTR_HD void op_aces(const uint32_t* in, uint32_t* out) { out[0] = PU(rtr_aces(PF(0))); }
RTR_HD void op_to_srgb(const uint32_t* in, uint32_t* out) { out[0] = PU(rtr_to_srgb(PF(0))); }
RTR_HD void op_to_linear(const uint32_t* in, uint32_t* out) { out[0] = PU(rtr_to_linear(PF(0))); }
RTR_HD void op_unorm8(const uint32_t* in, uint32_t* out) { out[0] = rtr_unorm8(PF(0)); }
RTR_HD void op_srgb_unorm8(const uint32_t* in, uint32_t* out) { out[0] = rtr_unorm8(rtr_to_srgb(PF(0))); }      /* one channel of the tone map's store */
RTR_HD void op_pack_bgra8(const uint32_t* in, uint32_t* out) { out[0] = rtr_pack_bgra8(PF(0), PF(1), PF(2)); }

/* ---- the device-only forms of kernels/rtr_device.h: wmin, wmax, wz, ga, gb, tmin, tmax -> decision, distance ---- */
RTR_HD void probe_slab_q_words(const uint32_t* in, uint32_t* out) {                 /* what slab_pair and slab_oct<k> restate */
    float te;
    out[0] = (uint32_t)rtr_slab_q(in[0] & 0xffffu, in[0] >> 16, in[2] & 0xffffu, in[1] & 0xffffu, in[1] >> 16, in[2] >> 16,
                                  PV(3), PV(6), PF(9), PF(10), &te);
    out[1] = PU(te);
}
/* what slab_wide<k, EXIT> restates: the planes are half floats, converted exactly; then rtr_slab_q's fma and min/max tree */
template <bool EXIT>
RTR_HD void probe_slab_wide_host(const uint32_t* in, uint32_t* out) {
    const rtr_v3 ga = PV(3), gb = PV(6);
    const float tmin = PF(9), tmax = PF(10);
    float tx0 = rtr_fma(probe_half(in[0] & 0xffffu), ga.x, gb.x), tx1 = rtr_fma(probe_half(in[1] & 0xffffu), ga.x, gb.x);
    float ty0 = rtr_fma(probe_half(in[0] >> 16), ga.y, gb.y), ty1 = rtr_fma(probe_half(in[1] >> 16), ga.y, gb.y);
    float tz0 = rtr_fma(probe_half(in[2] & 0xffffu), ga.z, gb.z), tz1 = rtr_fma(probe_half(in[2] >> 16), ga.z, gb.z);
    float lo = rtr_hwmax(rtr_hwmax(rtr_hwmin(tx0, tx1), rtr_hwmin(ty0, ty1)), rtr_hwmax(rtr_hwmin(tz0, tz1), tmin));
    float hi = rtr_hwmin(rtr_hwmin(rtr_hwmax(tx0, tx1), rtr_hwmax(ty0, ty1)), rtr_hwmin(rtr_hwmax(tz0, tz1), tmax));
    out[0] = (uint32_t)(lo <= hi * RTR_BOX_WIDEN);
    out[1] = PU(EXIT ? hi : lo);
}
RTR_HD void op_slab_pair(const uint32_t* in, uint32_t* out) {
#if PROBE_DEV
    float te;
    out[0] = (uint32_t)slab_pair(in[0], in[1], in[2], PV(3), PV(6), PF(9), PF(10), te);
    out[1] = PU(te);
#else
    probe_slab_q_words(in, out);
#endif
}
template <int OCT>
RTR_HD void probe_slab_oct(const uint32_t* in, uint32_t* out) {
#if PROBE_DEV
    float te;
    out[0] = (uint32_t)slab_oct<OCT>(in[0], in[1], in[2], PV(3), PV(6), PF(9), PF(10), te);
    out[1] = PU(te);
#else
    probe_slab_q_words(in, out);
#endif
}
template <int OCT, bool EXIT>
RTR_HD void probe_slab_wide(const uint32_t* in, uint32_t* out) {
#if PROBE_DEV
    float te;
    out[0] = (uint32_t)slab_wide<OCT, EXIT>(in[0], in[1], in[2], PV(3), PV(6), PF(9), PF(10), te);
    out[1] = PU(te);
#else
    probe_slab_wide_host<EXIT>(in, out);
#endif
}
#define PROBE_OCT(k) RTR_HD void op_slab_oct##k(const uint32_t* in, uint32_t* out) { probe_slab_oct<k>(in, out); }
#define PROBE_WIDE(k) \
    RTR_HD void op_slab_wide##k(const uint32_t* in, uint32_t* out) { probe_slab_wide<k, false>(in, out); } \
    RTR_HD void op_slab_wide_exit##k(const uint32_t* in, uint32_t* out) { probe_slab_wide<k, true>(in, out); }
PROBE_OCT(0) PROBE_OCT(1) PROBE_OCT(2) PROBE_OCT(3) PROBE_OCT(4) PROBE_OCT(5) PROBE_OCT(6) PROBE_OCT(7)
PROBE_WIDE(0) PROBE_WIDE(1) PROBE_WIDE(2) PROBE_WIDE(3) PROBE_WIDE(4) PROBE_WIDE(5) PROBE_WIDE(6) PROBE_WIDE(7) PROBE_WIDE(8)

/* ---- mutants, used only to show that the comparison can fail ---- */
/* rtr_atan_small with its last fma written as a multiplication and an addition: off by one ULP on part of the domain */
RTR_HD void op_mut_atan_small(const uint32_t* in, uint32_t* out) {
    const float x = PF(0), z = x * x;
    float p = 8.05374449538e-2f;
    p = rtr_fma(p, z, -1.38776856032e-1f);
    p = rtr_fma(p, z, 1.99777106478e-1f);
    p = rtr_fma(p, z, -3.33329491539e-1f);
    const float prod = (p * z) * x;              /* -ffp-contract=off keeps these two roundings apart */
    out[0] = PU(prod + x);
}
/* a select with the operands the other way round where rtr_hwmin is: the other zero of (+0, -0), the other operand on a NaN */
RTR_HD void op_mut_hwmin(const uint32_t* in, uint32_t* out) {
    const float a = PF(0), b = PF(1);
    out[0] = PU(b < a ? b : a);
}

/* X(name, input words, output words, mask of the outputs that are floats) */
#define PROBE_OPS(X) \
    X(fma, 3, 1, 1) X(sqrt, 1, 1, 1) X(min, 2, 1, 1) X(max, 2, 1, 1) X(clamp, 3, 1, 1) X(hwmin, 2, 1, 1) X(hwmax, 2, 1, 1) \
    X(pcg_hash, 1, 1, 0) X(random, 1, 1, 1) \
    X(dot, 6, 1, 1) X(cross, 6, 3, 7) X(normalize, 3, 3, 7) X(length, 3, 1, 1) \
    X(xform_point34, 15, 3, 7) X(xform_point44cm, 19, 3, 7) X(mul33, 12, 3, 7) X(normal_matrix, 12, 9, 0x1ff) \
    X(log2, 1, 1, 1) X(exp2, 1, 1, 1) X(pow, 2, 1, 1) X(pow_2_2, 1, 1, 1) X(pow_inv_2_2, 1, 1, 1) X(pow_5, 1, 1, 1) \
    X(atan_small, 1, 1, 1) X(atan2, 2, 1, 1) X(atan2_y1, 1, 1, 1) X(atan2_1x, 1, 1, 1) X(acos, 1, 1, 1) \
    X(unorm8_to_float, 1, 1, 1) X(div_by, 3, 1, 1) \
    X(safe_rcp_dir, 1, 1, 1) X(slab, 14, 2, 2) X(grid_from_bounds, 6, 6, 0x3f) X(quant_lo, 3, 1, 0) X(quant_hi, 3, 1, 0) \
    X(ray_grid, 12, 6, 0x3f) X(wide_centre_world, 8, 3, 7) X(ray_grid_about, 12, 6, 0x3f) X(slab_q, 14, 2, 2) \
    X(mt_intersect, 16, 4, 0xe) \
    X(aces, 1, 1, 1) X(to_srgb, 1, 1, 1) X(to_linear, 1, 1, 1) X(unorm8, 1, 1, 0) X(srgb_unorm8, 1, 1, 0) X(pack_bgra8, 3, 1, 0) \
    X(slab_pair, 11, 2, 2) \
    X(slab_oct0, 11, 2, 2) X(slab_oct1, 11, 2, 2) X(slab_oct2, 11, 2, 2) X(slab_oct3, 11, 2, 2) \
    X(slab_oct4, 11, 2, 2) X(slab_oct5, 11, 2, 2) X(slab_oct6, 11, 2, 2) X(slab_oct7, 11, 2, 2) \
    X(slab_wide0, 11, 2, 2) X(slab_wide1, 11, 2, 2) X(slab_wide2, 11, 2, 2) X(slab_wide3, 11, 2, 2) X(slab_wide4, 11, 2, 2) \
    X(slab_wide5, 11, 2, 2) X(slab_wide6, 11, 2, 2) X(slab_wide7, 11, 2, 2) X(slab_wide8, 11, 2, 2) \
    X(slab_wide_exit0, 11, 2, 2) X(slab_wide_exit1, 11, 2, 2) X(slab_wide_exit2, 11, 2, 2) X(slab_wide_exit3, 11, 2, 2) \
    X(slab_wide_exit4, 11, 2, 2) X(slab_wide_exit5, 11, 2, 2) X(slab_wide_exit6, 11, 2, 2) X(slab_wide_exit7, 11, 2, 2) \
    X(slab_wide_exit8, 11, 2, 2) \
    X(mut_atan_small, 1, 1, 1) X(mut_hwmin, 2, 1, 1)

enum {
#define X(name, nin, nout, fmask) PROBE_OP_##name,
    PROBE_OPS(X)
#undef X
    PROBE_OP_COUNT
};

#define PROBE_MAX_IN 19
#define PROBE_MAX_OUT 9

struct probe_op_info { const char* name; int nin, nout; uint32_t fmask; };
static const probe_op_info PROBE_INFO[PROBE_OP_COUNT] = {
#define X(name, nin, nout, fmask) {#name, nin, nout, fmask},
    PROBE_OPS(X)
#undef X
};

#endif /* RTR_MATH_OPS_H */
