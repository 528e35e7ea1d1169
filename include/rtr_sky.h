/* rtr_sky.h — the sky-sampling contract of rtr_sky_rays and rtr_sky_hits: directions drawn in proportion to the sky (the HDRI or the
 * constant sky), their solid-angle density, and the balance heuristic between S such draws of a path vertex and its one BRDF-sampled
 * bounce (include/rtr_bounce.h, include/rtr_mis.h).
 *
 * One definition for the host (rtr_host_sky_table, rtr_host_sky_rays, rtr_host_sky_hits, rtr_host_sky_pdf, rtr_host_sky_radiance) and
 * the device (k_sky_weights, k_sky_rays, k_sky_hits), in the terms of rtr_math.h: IEEE-754 binary32 + - * / rtr_sqrt and explicit
 * rtr_fma, compiled with -ffp-contract=off on both sides, so that the kernels' records can be held to the host's bits
 * (tests/test_gpu_sky.py).  Uses rtr_math.h, rtr_types.h, rtr_bounce.h and rtr_mis.h only; the render kernels do not include this
 * header.  The miss rule of fetch_surface and its bilinear 8-bit sampler (kernels/rtr_device.h) are restated here operation for
 * operation under rtr_sky_* names, so that rtr_sky_radiance gives the bits rtr_hit_surfaces writes into RtrSurface::color at a miss.
 *
 * THE TABLE.  A piecewise-constant importance function over the HDRI's W x H texel cells, held as INTEGERS so
 * that its sums do not depend on the order they are formed in.  m(x, y) = the largest channel of the texel after rtr_to_linear;
 * M(x, y) = the largest m over the texel's 3 x 3 neighbourhood with repeat addressing (every texel the bilinear filter can blend
 * anywhere inside cell (x, y), so M > 0 wherever the radiance is positive in the cell); s_y = sin(pi (y + 0.5) / H);
 * weight = 0 when M == 0, else max(1, (uint32_t)(M * s_y * 65536.0f)).  rows[y * W + x]: the inclusive prefix sums of row y's weights
 * (uint32_t; W <= RTR_SKY_MAX_WIDTH keeps a row total below 2^32); marginal[y]: the inclusive prefix sums of the row totals
 * (uint64_t).  A scene without an HDRI has the table of a RTR_SKY_CONST_W x RTR_SKY_CONST_H sky whose every m is the largest channel
 * of the linear sky colour, held to [0, 1] (the shape of the table is all that counts).  A table whose total is 0 is valid: every
 * sample of it is dead.
 *
 * RESOLUTION.  rtr_random gives 24-bit numbers k / 2^24 (and 1.0).  A number u picks the integer target floor(u * total) in double
 * precision, exactly, and what the product leaves behind the target places the point inside the cell.  A table whose total is above
 * 2^24 — any HDRI of more than 256 cells of full weight — therefore has targets no draw can reach: the 2^24 numbers fall total / 2^24
 * weight units apart, so that a cell of weight w is met by about w 2^24 / total of them and a cell lighter than total / 2^24 by one or
 * none.  The expectation stays right (the numbers are evenly spaced, and the density is evaluated for the direction that came out),
 * but within a cell of a very large table the points sit on a lattice of that spacing instead of filling it.
 *
 * Used by: kernels/rtr_sky.hip (device), rtr_sky_host.cpp (host).
 */
#ifndef RTR_SKY_H
#define RTR_SKY_H

#include "rtr_math.h"
#include "rtr_types.h"
#include "rtr_bounce.h"
#include "rtr_mis.h"

#define RTR_SKY_CONST_W   32u
#define RTR_SKY_CONST_H   16u
#define RTR_SKY_MAX_WIDTH 65535u            /* 65535 cells of at most 65536 + 1 weight units stay below 2^32 */
#define RTR_SKY_TWO_PI_SQ 19.739208802f     /* 2 pi^2 */

/* the sky as the miss rule sees it: pixels == NULL is the constant sky, whose LINEAR colour is skyLinear */
typedef struct rtr_sky_source {
    const uint8_t* pixels;
    uint32_t width, height, channels;       /* 4 = RGBA8, 1 = R8 */
    float skyLinear[3];
} rtr_sky_source;

/* ---- sample_tex of kernels/rtr_device.h: 8-bit texels, linear filter, repeat addressing ------------------------------------------ */
RTR_HD void rtr_sky_sample_tex(const rtr_sky_source* tx, float u, float v, float* o) {
    if (!(u > -1.0e9f && u < 1.0e9f)) u = 0.0f;
    if (!(v > -1.0e9f && v < 1.0e9f)) v = 0.0f;
    const int W = (int)tx->width, H = (int)tx->height, ch = (int)tx->channels;
    const float uf = u - __builtin_floorf(u), vf = v - __builtin_floorf(v);
    const float x = rtr_fma(uf, (float)W, -0.5f), y = rtr_fma(vf, (float)H, -0.5f);
    const float x0f = __builtin_floorf(x), y0f = __builtin_floorf(y);
    const float fx = x - x0f, fy = y - y0f;
    int x0 = (int)x0f, y0 = (int)y0f;
    if (x0 < 0) x0 += W;
    if (x0 >= W) x0 -= W;
    if (y0 < 0) y0 += H;
    if (y0 >= H) y0 -= H;
    int x1 = x0 + 1, y1 = y0 + 1;
    if (x1 >= W) x1 -= W;
    if (y1 >= H) y1 -= H;
    const uint8_t* p = tx->pixels;
    if (ch == 4) {
        const uint8_t* q00 = p + ((size_t)y0 * W + x0) * 4;
        const uint8_t* q10 = p + ((size_t)y0 * W + x1) * 4;
        const uint8_t* q01 = p + ((size_t)y1 * W + x0) * 4;
        const uint8_t* q11 = p + ((size_t)y1 * W + x1) * 4;
        for (int k = 0; k < 4; ++k) {
            const float t00 = rtr_unorm8_to_float(q00[k]), t10 = rtr_unorm8_to_float(q10[k]);
            const float t01 = rtr_unorm8_to_float(q01[k]), t11 = rtr_unorm8_to_float(q11[k]);
            const float a = rtr_fma(t10 - t00, fx, t00), b = rtr_fma(t11 - t01, fx, t01);
            o[k] = rtr_fma(b - a, fy, a);
        }
    } else {
        const float t00 = rtr_unorm8_to_float(p[(size_t)y0 * W + x0]), t10 = rtr_unorm8_to_float(p[(size_t)y0 * W + x1]);
        const float t01 = rtr_unorm8_to_float(p[(size_t)y1 * W + x0]), t11 = rtr_unorm8_to_float(p[(size_t)y1 * W + x1]);
        const float a = rtr_fma(t10 - t00, fx, t00), b = rtr_fma(t11 - t01, fx, t01);
        o[0] = rtr_fma(b - a, fy, a); o[1] = 0.0f; o[2] = 0.0f; o[3] = 1.0f;
    }
}

/* ---- the miss rule of fetch_surface -------------------------------------------------------------------------------------------- */
/* the equirect coordinates of a direction (it need not be normalised) */
RTR_HD void rtr_sky_uv(rtr_v3 rayDir, float* hu, float* hv, float* dirY) {
    const rtr_v3 dir = rtr_normalize(rayDir);
    *hu = rtr_atan2(dir.z, dir.x) / (2.0f * 3.14159265f) + 0.5f;
    const float v = rtr_acos(rtr_clamp(dir.y, -1.0f, 1.0f)) / 3.14159265f;
    *hv = 1.0f - v;
    *dirY = dir.y;
}

RTR_HD rtr_v3 rtr_sky_radiance_uv(const rtr_sky_source* sky, float hu, float hv) {
    if (!sky->pixels) return rtr_ld3(sky->skyLinear);
    float tx[4];
    rtr_sky_sample_tex(sky, hu, hv, tx);
    return rtr_mk(rtr_to_linear(tx[0]), rtr_to_linear(tx[1]), rtr_to_linear(tx[2]));
}

RTR_HD rtr_v3 rtr_sky_radiance(const rtr_sky_source* sky, rtr_v3 rayDir) {
    if (!sky->pixels) return rtr_ld3(sky->skyLinear);
    float hu, hv, y;
    rtr_sky_uv(rayDir, &hu, &hv, &y);
    return rtr_sky_radiance_uv(sky, hu, hv);
}

/* ---- the table ------------------------------------------------------------------------------------------------------------------ */
RTR_HD uint32_t rtr_sky_table_width(const rtr_sky_source* sky) { return sky->pixels ? sky->width : RTR_SKY_CONST_W; }
RTR_HD uint32_t rtr_sky_table_height(const rtr_sky_source* sky) { return sky->pixels ? sky->height : RTR_SKY_CONST_H; }

/* m of one texel: what sample_tex gives an R8 texel's other channels is (0, 0), and rtr_to_linear(0) is 0 */
RTR_HD float rtr_sky_texel_max(const rtr_sky_source* sky, uint32_t x, uint32_t y) {
    const uint8_t* p = sky->pixels;
    const size_t at = (size_t)y * sky->width + x;
    if (sky->channels == 4u) {
        const float r = rtr_to_linear(rtr_unorm8_to_float(p[4 * at])), g = rtr_to_linear(rtr_unorm8_to_float(p[4 * at + 1]));
        const float b = rtr_to_linear(rtr_unorm8_to_float(p[4 * at + 2]));
        return rtr_max(rtr_max(r, g), b);
    }
    return rtr_max(rtr_max(rtr_to_linear(rtr_unorm8_to_float(p[at])), rtr_to_linear(0.0f)), rtr_to_linear(0.0f));
}

/* the weight of cell (x, y), x < W, y < H */
RTR_HD uint32_t rtr_sky_weight(const rtr_sky_source* sky, uint32_t x, uint32_t y) {
    const uint32_t W = rtr_sky_table_width(sky), H = rtr_sky_table_height(sky);
    float M = 0.0f;
    if (sky->pixels) {
        const uint32_t xs[3] = {x == 0u ? W - 1u : x - 1u, x, x + 1u == W ? 0u : x + 1u};
        const uint32_t ys[3] = {y == 0u ? H - 1u : y - 1u, y, y + 1u == H ? 0u : y + 1u};
        for (int j = 0; j < 3; ++j)
            for (int i = 0; i < 3; ++i) M = rtr_max(M, rtr_sky_texel_max(sky, xs[i], ys[j]));
    } else {
        const float m = rtr_bounce_max3(rtr_ld3(sky->skyLinear));
        M = m > 0.0f ? rtr_min(m, 1.0f) : 0.0f;          /* a NaN is no sky */
    }
    if (!(M > 0.0f)) return 0u;
    float sy, cy;
    rtr_sincos_turn(((float)y + 0.5f) / (2.0f * (float)H), &sy, &cy);
    const float p = (M * sy) * 65536.0f;
    const uint32_t w = p >= 1.0f ? (uint32_t)p : 1u;
    return w;
}

RTR_HD uint64_t rtr_sky_total(const rtr_sky_table* t) { return t->marginal[t->height - 1u]; }

RTR_HD uint32_t rtr_sky_cell_weight(const rtr_sky_table* t, uint32_t x, uint32_t y) {
    const uint32_t* row = t->rows + (size_t)y * t->width;
    return row[x] - (x ? row[x - 1u] : 0u);
}

/* the cell a pair of equirect coordinates falls into, clamped into range (a NaN goes to 0) */
RTR_HD uint32_t rtr_sky_cell_axis(float h, uint32_t n) {
    const float a = h * (float)n;
    if (!(a >= 0.0f)) return 0u;
    if (a >= (float)n) return n - 1u;
    const uint32_t c = (uint32_t)a;
    return c < n ? c : n - 1u;
}

RTR_HD void rtr_sky_cell_of(const rtr_sky_table* t, rtr_v3 dir, uint32_t* cx, uint32_t* cy, float* dirY) {
    float hu, hv;
    rtr_sky_uv(dir, &hu, &hv, dirY);
    *cx = rtr_sky_cell_axis(hu, t->width);
    *cy = rtr_sky_cell_axis(hv, t->height);
}

/* The solid-angle density of rtr_sky_sample for direction dir: weight(cell) / total * W H / (2 pi^2 sin theta), sin theta =
 * rtr_sqrt(1 - y^2) of the normalised direction; 0 where that is not finite or not positive.  The ONE density of both sides of the
 * heuristic: the sample side evaluates it for the direction it drew, not for the cell it drew. */
RTR_HD float rtr_sky_pdf_cell(const rtr_sky_table* t, rtr_v3 dir, uint32_t* cell) {
    uint32_t cx, cy;
    float y;
    rtr_sky_cell_of(t, dir, &cx, &cy, &y);
    *cell = cy * t->width + cx;
    const uint64_t total = rtr_sky_total(t);
    if (total == 0u) return 0.0f;
    const uint32_t w = rtr_sky_cell_weight(t, cx, cy);
    const float sinT = rtr_sqrt(1.0f - y * y);
    const float pdf = (((float)w / (float)total) * ((float)t->width * (float)t->height)) / (RTR_SKY_TWO_PI_SQ * sinT);
    if (!(pdf > 0.0f) || !rtr_bounce_finite(pdf)) return 0.0f;
    return pdf;
}
RTR_HD float rtr_sky_pdf(const rtr_sky_table* t, rtr_v3 dir) { uint32_t cell; return rtr_sky_pdf_cell(t, dir, &cell); }

/* u in [0, 1] -> the integer target floor(u * total), at most total - 1, and what is left of the product behind it.  A double holds
 * the 24-bit u and any total below 2^53 exactly; their product is one IEEE rounding on either compiler. */
RTR_HD uint64_t rtr_sky_target(float u, uint64_t total, double* scaled) {
    double s = (double)u * (double)total;
    if (!(s >= 0.0)) s = 0.0;
    uint64_t k = (uint64_t)s;
    if (k >= total) { k = total - 1u; s = (double)total; }
    *scaled = s;
    return k;
}

/* the first row whose inclusive sum is above target (target < total): marginal may live in any address space */
#define RTR_SKY_SEARCH(sums, count, target, found) do { \
        uint32_t lo_ = 0u, hi_ = (count) - 1u; \
        while (lo_ < hi_) { const uint32_t mid_ = (lo_ + hi_) >> 1; if ((sums)[mid_] > (target)) hi_ = mid_; else lo_ = mid_ + 1u; } \
        (found) = lo_; \
    } while (0)

/* the rest of rtr_sky_sample once the row y is found: prevRows = marginal[y - 1] (0 for y == 0), rowTotal = marginal[y] - prevRows > 0,
 * sRow: rtr_sky_target's scaled product */
RTR_HD rtr_v3 rtr_sky_sample_in_row(const rtr_sky_table* t, uint32_t y, uint64_t prevRows, uint64_t rowTotal, double sRow, float u2) {
    const uint32_t W = t->width, H = t->height;
    const float fv = (float)(sRow - (double)prevRows) / (float)rowTotal;
    const float hv = ((float)y + fv) / (float)H;
    double sCol;
    const uint32_t target = (uint32_t)rtr_sky_target(u2, rowTotal, &sCol);
    const uint32_t* row = t->rows + (size_t)y * W;
    uint32_t x;
    RTR_SKY_SEARCH(row, W, target, x);
    const uint32_t prev = x ? row[x - 1u] : 0u;
    const float fu = (float)(sCol - (double)prev) / (float)(row[x] - prev);
    const float hu = ((float)x + fu) / (float)W;
    /* the inverse of the miss look-up: phi = 2 pi (hu - 0.5), so that sin and cos of phi are those of the turn hu, negated;
     * theta = pi (1 - hv), the turn (1 - hv) / 2 */
    float sp, cp, st, ct;
    rtr_sincos_turn(rtr_clamp(hu, 0.0f, 1.0f), &sp, &cp);
    rtr_sincos_turn(0.5f * (1.0f - rtr_clamp(hv, 0.0f, 1.0f)), &st, &ct);
    return rtr_normalize(rtr_mk(st * -cp, ct, st * -sp));
}

/* u1 finds the row in the 64-bit marginal sums, u2 the column in the row's 32-bit sums; uniform in (hu, hv) inside the cell.
 * The table's total must not be 0. */
RTR_HD rtr_v3 rtr_sky_sample(const rtr_sky_table* t, float u1, float u2) {
    double sRow;
    const uint64_t target = rtr_sky_target(u1, rtr_sky_total(t), &sRow);
    uint32_t y;
    RTR_SKY_SEARCH(t->marginal, t->height, target, y);
    const uint64_t prevRows = y ? t->marginal[y - 1u] : 0u;
    return rtr_sky_sample_in_row(t, y, prevRows, t->marginal[y] - prevRows, sRow, u2);
}

/* ---- one sky sample of one path vertex ------------------------------------------------------------------------------------------- */
RTR_HD void rtr_sky_dead(RtrRay* out, RtrSkySample* s) {
    out->origin[0] = out->origin[1] = out->origin[2] = 0.0f; out->tmin = 0.0f;
    out->direction[0] = out->direction[1] = out->direction[2] = 0.0f; out->tmax = 0.0f;
    s->contrib[0] = s->contrib[1] = s->contrib[2] = 0.0f; s->skyPdf = 0.0f;
    s->bouncePdf = 0.0f; s->wSky = 0.0f; s->cell = 0u; s->_r = 0u;
}

/* ray: the ray that found the vertex (its origin gives the view vector); sf: the vertex's RtrSurface; L: the direction rtr_sky_sample
 * drew for it; S: the vertex's sky samples.  The contribution is f cos sky / (S ps + pb) with RTR_SKY_MIS — the balance heuristic over
 * S sky samples and the one bounce, wSky = S ps / (S ps + pb), already divided by S ps — and f cos sky / (S ps) without.  The ray is
 * the directional light's shadow ray of rtr_light_rays with direction L: origin position + 0.01 normal, [0.001, 10000].  DEAD (the null
 * ray and 32 zero bytes): a surface that is not an object, a value that is not finite, cos <= 0, ps == 0, a contribution that is not
 * finite or has a negative channel (a negative colour, as rtr_bounce_sample treats a negative weight).  No output word is ever a NaN
 * or an infinity. */
RTR_HD void rtr_sky_vertex_dir(const RtrRay* ray, const RtrSurface* sf, const rtr_sky_source* sky, const rtr_sky_table* t, rtr_v3 L, uint32_t S,
                               uint32_t flags, uint32_t lobes, RtrRay* out, RtrSkySample* s) {
    rtr_sky_dead(out, s);
    if (sf->kind != RTR_SURFACE_OBJECT) return;
    const rtr_v3 P = rtr_ld3(sf->position), N = rtr_ld3(sf->normal), color = rtr_ld3(sf->color), O = rtr_ld3(ray->origin);
    const float roughness = sf->roughness, metallic = sf->metallic;
    if (!(rtr_bounce_finite3(P) & rtr_bounce_finite3(N) & rtr_bounce_finite3(color) & rtr_bounce_finite3(O) & rtr_bounce_finite3(L) &
          rtr_bounce_finite(roughness) & rtr_bounce_finite(metallic))) return;
    const rtr_v3 V = rtr_normalize(rtr_sub(O, P));
    if (!rtr_bounce_finite3(V)) return;
    uint32_t cell;
    const float ps = rtr_sky_pdf_cell(t, L, &cell);
    if (!(ps > 0.0f)) return;
    const float NoL = rtr_dot(N, L);
    if (!(NoL > 0.0f)) return;
    const float om = 1.0f - metallic;
    const rtr_v3 F0 = rtr_mk(rtr_fma(color.x, metallic, 0.04f * om), rtr_fma(color.y, metallic, 0.04f * om), rtr_fma(color.z, metallic, 0.04f * om));
    const rtr_v3 f = rtr_bounce_brdf(N, V, L, roughness, F0, om, color);
    const float pb = rtr_mis_bounce_pdf(ray, sf, L, lobes);
    const rtr_v3 rad = rtr_sky_radiance(sky, L);
    const float a = (float)S * ps;
    const int mis = (flags & RTR_SKY_MIS) != 0u;
    const float den = mis ? a + pb : a;
    const float wSky = mis ? a / den : 1.0f;
    const rtr_v3 c = rtr_mk(((f.x * NoL) * rad.x) / den, ((f.y * NoL) * rad.y) / den, ((f.z * NoL) * rad.z) / den);
    if (!(rtr_bounce_finite3(c) & rtr_bounce_finite(wSky) & rtr_bounce_finite(pb) & (c.x >= 0.0f) & (c.y >= 0.0f) & (c.z >= 0.0f))) return;
    const rtr_v3 origin = rtr_madd(P, N, 0.01f);
    if (!rtr_bounce_finite3(origin)) return;
    out->origin[0] = origin.x; out->origin[1] = origin.y; out->origin[2] = origin.z; out->tmin = 0.001f;
    out->direction[0] = L.x; out->direction[1] = L.y; out->direction[2] = L.z; out->tmax = 10000.0f;
    s->contrib[0] = c.x; s->contrib[1] = c.y; s->contrib[2] = c.z; s->skyPdf = ps;
    s->bouncePdf = pb; s->wSky = wSky; s->cell = cell;
}

/* the seed of a vertex: s0 = base + frame + 7919 (depth + 1), base = seeds[k] or the pixel's; sample j takes rtr_random(s0 + 3400 +
 * 200 j) and rtr_random(s0 + 3500 + 200 j), the next free offsets behind the bounce (0, 100, 200), the roulette (300) and the picks
 * (400 ... 3300); S <= RTR_SKY_MAX_SAMPLES keeps the largest, 4900, below 7919. */
RTR_HD uint32_t rtr_sky_seed(uint32_t base, uint32_t frame, uint32_t depth) { return base + frame + 7919u * (depth + 1u); }
RTR_HD void rtr_sky_randoms(uint32_t s0, uint32_t j, float* u1, float* u2) {
    *u1 = rtr_random(s0 + 3400u + 200u * j);
    *u2 = rtr_random(s0 + 3500u + 200u * j);
}

RTR_HD void rtr_sky_vertex(const RtrRay* ray, const RtrSurface* sf, const rtr_sky_source* sky, const rtr_sky_table* t, float u1, float u2, uint32_t S,
                           uint32_t flags, uint32_t lobes, RtrRay* out, RtrSkySample* s) {
    rtr_sky_dead(out, s);
    if (sf->kind != RTR_SURFACE_OBJECT || rtr_sky_total(t) == 0u) return;
    rtr_sky_vertex_dir(ray, sf, sky, t, rtr_sky_sample(t, u1, u2), S, flags, lobes, out, s);
}

/* ---- the bounce side --------------------------------------------------------------------------------------------------------------- */
RTR_HD void rtr_sky_escape_zero(RtrSkyEscape* e) {
    e->radiance[0] = e->radiance[1] = e->radiance[2] = 0.0f; e->wBounce = 0.0f;
    e->skyPdf = 0.0f; e->bouncePdf = 0.0f; e->cell = 0u; e->kind = 0u;
}

/* For a bounce ray that MISSED, having left the vertex whose bounce density is pb (RtrBounce::pdf) and whose surface kind is prevKind:
 * radiance = rtr_sky_radiance(direction) * wBounce, wBounce = pb / (S ps + pb) with ps = rtr_sky_pdf(direction); wBounce = 1 (and the
 * radiance the bits of the miss rule) when the flag is off or S == 0.  With the heuristic on, zeros for a vertex that is not an object, a
 * pb that is not positive and finite, or a weight or radiance that is not finite. */
RTR_HD void rtr_sky_escape(const RtrRay* ray, uint32_t prevKind, float pb, const rtr_sky_source* sky, const rtr_sky_table* t, uint32_t S,
                           uint32_t flags, RtrSkyEscape* e) {
    rtr_sky_escape_zero(e);
    const rtr_v3 dir = rtr_ld3(ray->direction);
    const rtr_v3 rad = rtr_sky_radiance(sky, dir);
    uint32_t cell;
    const float ps = rtr_sky_pdf_cell(t, dir, &cell);
    const float pbOut = (pb > 0.0f) & rtr_bounce_finite(pb) ? pb : 0.0f;
    float w = 1.0f;
    if ((flags & RTR_SKY_MIS) != 0u && S != 0u) {
        if (prevKind != RTR_SURFACE_OBJECT) return;
        if (!(pb > 0.0f) || !rtr_bounce_finite(pb)) return;
        const float sum = (float)S * ps + pb;
        w = pb / sum;
        if (!rtr_bounce_finite(w)) return;
    }
    const rtr_v3 r = rtr_mk(rad.x * w, rad.y * w, rad.z * w);
    if (!rtr_bounce_finite3(r)) return;
    e->radiance[0] = r.x; e->radiance[1] = r.y; e->radiance[2] = r.z; e->wBounce = w;
    e->skyPdf = ps; e->bouncePdf = pbOut; e->cell = cell; e->kind = RTR_SURFACE_MISS;
}

#endif /* RTR_SKY_H */
