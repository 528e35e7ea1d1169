/* rtr_accum_host.cpp — rtr_host_accumulate_paths, rtr_host_gather_records and the argument checks rtr_accumulate_paths and
 * rtr_gather_records share with them.  Pure host C++ with no HIP in it: include/rtr_accum.h compiled for the host cores with the
 * kernels' flags (-ffp-contract=off, no fast-math), so that the device's words can be held to these bits; a translation unit of its
 * own so that a stand-alone program (tools/accum_host_check.cpp) can run it under the host sanitizers. */
#include "rtr_accum_host.h"
#include "../../include/rtr_accum.h"

#include <cstdint>
#include <cstring>

namespace rtrdev {

/* bytes = (count - 1) * stride + tail, the extent of an array of count > 0 rows; false when it, or the end of the array at p, does not
 * fit the address space */
static bool extent_fits(const void* p, size_t count, size_t stride, size_t tail, size_t* bytes) {
    size_t b = 0;
    if (__builtin_mul_overflow(count - 1u, stride, &b) || __builtin_add_overflow(b, tail, &b)) return false;
    uintptr_t end = 0;
    if (p && __builtin_add_overflow((uintptr_t)p, (uintptr_t)b, &end)) return false;
    *bytes = b;
    return true;
}

int accum_check_args(const char* who, const AccumCall& c) {
    const rtr_accum_params* p = c.params;
    if (!p) return refusef("%s: params is null", who);
    Arg in[7] = {{c.radiance, "radiance", 16, true, 0}, {c.throughput, "throughput", 4, true, 0}, {c.pathIds, "pathIds", 4, false, 0},
                 {c.emitters, "emitters", 16, false, 0}, {c.escapes, "escapes", 16, false, 0}, {c.skySums, "skySums", 16, false, 0},
                 {c.bounces, "bounces", 16, false, 0}};
    Arg out[3] = {{c.accum, "accum", 4, true, 0}, {c.outTerm, "outTerm", 4, false, 0}, {c.outThroughput, "outThroughput", 4, false, 0}};
    if (const int rc = check_ptrs(who, in)) return rc;
    if (const int rc = check_ptrs(who, out)) return rc;
    if (c.bounces && !c.outThroughput) return refusef("%s: bounces without outThroughput (outThroughput is null)", who);
    if (!c.bounces && c.outThroughput) return refusef("%s: outThroughput without bounces (bounces is null)", who);
    const size_t tStride = p->throughputStrideBytes, iStride = p->imageStrideBytes;
    if (tStride < 12u || (tStride & 3u)) return refusef("%s: throughputStrideBytes %u (a multiple of 4, at least 12)", who, p->throughputStrideBytes);
    if (iStride < 12u || (iStride & 3u)) return refusef("%s: imageStrideBytes %u (a multiple of 4, at least 12)", who, p->imageStrideBytes);
    if (p->flags & ~(RTR_ACCUM_LIGHTS_FROM_EMITTERS | RTR_ACCUM_MISSES_FROM_ESCAPES))
        return refusef("%s: flags 0x%x (RTR_ACCUM_LIGHTS_FROM_EMITTERS | RTR_ACCUM_MISSES_FROM_ESCAPES or 0)", who, p->flags);
    if (const int rc = check_reserved(who, p->_reserved, 4, "params")) return rc;
    if (p->numSlots == 0u) return refusef("%s: numSlots is 0", who);
    const size_t n = c.n;
    const size_t inStride[7] = {sizeof(RtrRadiance), tStride, 4u, sizeof(RtrEmitter), sizeof(RtrSkyEscape), 16u, sizeof(RtrBounce)};
    const size_t inTail[7] = {sizeof(RtrRadiance), 12u, 4u, sizeof(RtrEmitter), sizeof(RtrSkyEscape), 16u, sizeof(RtrBounce)};
    for (int i = 0; i < 7; ++i)
        if (!extent_fits(in[i].ptr, n, inStride[i], inTail[i], &in[i].bytes))
            return refusef("%s: %s: %u rows of stride %zu do not fit the address space", who, in[i].name, c.n, inStride[i]);
    for (int o = 0; o < 2; ++o)
        if (!extent_fits(out[o].ptr, p->numSlots, iStride, 12u, &out[o].bytes))
            return refusef("%s: %s: numSlots %u x imageStrideBytes %u does not fit the address space", who, out[o].name, p->numSlots, p->imageStrideBytes);
    if (!extent_fits(out[2].ptr, n, 12u, 12u, &out[2].bytes)) return refusef("%s: outThroughput: %u rows do not fit the address space", who, c.n);
    if (const int rc = check_overlaps(who, in, 7, out, 2)) return rc;
    /* in place: the packed input throughput itself may take the new one; every other overlap of outThroughput is refused */
    if (c.outThroughput && c.outThroughput == c.throughput && tStride == 12u) in[1].ptr = nullptr;
    return check_overlaps(who, in, 7, out, 3);
}

int gather_check_args(const char* who, const void* src, uint32_t recordBytes, uint32_t numSrc, const uint32_t* rows, uint32_t numRows, const void* out) {
    if (recordBytes == 0u || (recordBytes & 3u) || recordBytes > 256u) return refusef("%s: recordBytes %u (a multiple of 4, 4 ... 256)", who, recordBytes);
    Arg in[2] = {{src, "src", 4, numSrc != 0u, 0}, {rows, "rows", 4, true, 0}};
    Arg o[1] = {{out, "out", 4, true, 0}};
    if (const int rc = check_ptrs(who, in)) return rc;
    if (const int rc = check_ptrs(who, o)) return rc;
    if (numSrc && !extent_fits(src, numSrc, recordBytes, recordBytes, &in[0].bytes)) return refusef("%s: src: %u records of %u B do not fit the address space", who, numSrc, recordBytes);
    if (!extent_fits(rows, numRows, 4u, 4u, &in[1].bytes)) return refusef("%s: rows: %u rows do not fit the address space", who, numRows);
    if (!extent_fits(out, numRows, recordBytes, recordBytes, &o[0].bytes)) return refusef("%s: out: %u records of %u B do not fit the address space", who, numRows, recordBytes);
    return check_overlaps(who, in, 2, o, 1);
}

}  // namespace rtrdev

extern "C" int rtr_host_accumulate_paths(const RtrRadiance* radiance, const float* throughput, const uint32_t* pathIds, const RtrEmitter* emitters,
                                         const RtrSkyEscape* escapes, const float* skySums, const RtrBounce* bounces, uint32_t n,
                                         const rtr_accum_params* p, float* accum, float* outTerm, float* outThroughput) {
    if (n == 0) return RTR_OK;
    const rtrdev::AccumCall c{radiance, throughput, pathIds, emitters, escapes, skySums, bounces, n, p, accum, outTerm, outThroughput};
    if (const int rc = rtrdev::accum_check_args("rtr_host_accumulate_paths", c)) return rc;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t kind = radiance[k].kind;
        float rad[3] = {radiance[k].shadowed[0], radiance[k].shadowed[1], radiance[k].shadowed[2]};
        if (rtr_accum_from_emitters(kind, p->flags))
            for (int a = 0; a < 3; ++a) rad[a] = emitters ? emitters[k].radiance[a] : 0.0f;
        if (rtr_accum_from_escapes(kind, p->flags))
            for (int a = 0; a < 3; ++a) rad[a] = escapes ? escapes[k].radiance[a] : 0.0f;
        float T[3], term[3];
        memcpy(T, reinterpret_cast<const char*>(throughput) + (size_t)k * p->throughputStrideBytes, 12);
        rtr_accum_term(T, rad, skySums != nullptr, skySums ? skySums + 4 * (size_t)k : T, term);
        const uint32_t id = pathIds ? pathIds[k] : k;
        if (rtr_accum_slot_ok(id, p->numSlots)) {
            const size_t at = (size_t)id * p->imageStrideBytes;
            float acc[3];
            memcpy(acc, reinterpret_cast<char*>(accum) + at, 12);
            for (int a = 0; a < 3; ++a) acc[a] = acc[a] + term[a];
            memcpy(reinterpret_cast<char*>(accum) + at, acc, 12);
            if (outTerm) memcpy(reinterpret_cast<char*>(outTerm) + at, term, 12);
        }
        if (bounces) {
            float outT[3];
            rtr_accum_next_throughput(T, bounces[k].weight, outT);
            memcpy(outThroughput + 3 * (size_t)k, outT, 12);
        }
    }
    return RTR_OK;
}

extern "C" int rtr_host_gather_records(const void* src, uint32_t recordBytes, uint32_t numSrc, const uint32_t* rows, uint32_t numRows, void* out) {
    if (numRows == 0) return RTR_OK;
    if (const int rc = rtrdev::gather_check_args("rtr_host_gather_records", src, recordBytes, numSrc, rows, numRows, out)) return rc;
    for (uint32_t j = 0; j < numRows; ++j) {
        char* o = static_cast<char*>(out) + (size_t)j * recordBytes;
        if (rtr_gather_row_ok(rows[j], numSrc)) memcpy(o, static_cast<const char*>(src) + (size_t)rows[j] * recordBytes, recordBytes);
        else memset(o, 0, recordBytes);
    }
    return RTR_OK;
}
