/* rtr_api.cpp — implementation of the C ABI in include/rtr.h (host side of librtr_hip.so): errors, version and status strings, the
 * context and the scene.  Frames and dispatch are rtr_api_render.cpp, the ray queries rtr_api_query.cpp, lighting and the path-vertex
 * calls rtr_api_paths.cpp; rtr_api_internal.h has what they share.
 * HIP runtime for device memory / streams / events; kernels in kernels/rtr_kernels.hip.
 * There is NO CPU rendering fallback in this library: without a HIP device every entry point
 * that needs one fails with RTR_ERR_NO_DEVICE / RTR_ERR_HIP. */
#include "../../include/rtr.h"
#include "../../include/rtr_math.h"
#include "bvh_build.h"
#include "kernels/rtr_kernels.h"
#include "kernels/rtr_bvh.h"
#include "kernels/rtr_mirrored.h"
#include "kernels/rtr_tree_sah.h"
#include "kernels/rtr_query.h"
#include "rtr_api_internal.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace rtrapi;

namespace {

thread_local std::string g_err;

}  // namespace

int rtrapi::fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    g_err = buf;
    return code;
}

/* the status of a call whose kernel launcher returned e */
int rtrapi::launched(hipError_t e, const char* who) {
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: kernel launch: %s", who, hipGetErrorString(e));
    return RTR_OK;
}

constexpr size_t kPolicyRecordAt = 12, kPolicyWords = kPolicyRecordAt + sizeof(rtrdev::RebuildIfRecord) / sizeof(unsigned long long);
static rtrdev::RebuildIfRecord* policy_record(const rtr_scene* s) { return reinterpret_cast<rtrdev::RebuildIfRecord*>(s->policy.p + kPolicyRecordAt); }

/* no geometry: the host builder's tree of such a scene is one node over one placeholder record */
static bool scene_is_empty(const rtr_scene* s) { return s->tree.hostTris.empty() || s->tree.hostTris[0].customIndex == 0xffffffffu; }

static void ctx_free(rtr_ctx* c) {
    (void)hipSetDevice(c->device);
    if (c->qLastStream) (void)hipEventSynchronize(c->qEv[1]);      /* the scratch below is freed with the context */
    for (hipEvent_t e : c->qEv) if (e) (void)hipEventDestroy(e);
    if (c->ownStream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}
void rtrapi::ctx_release_child(rtr_ctx* c) {
    if (--c->children == 0 && c->destroyed) ctx_free(c);
}

/* rtr_bounce_host.cpp's way to this thread's error text */
void rtrdev::set_last_error(const char* msg) { g_err = msg; }

extern "C" {

const char* rtr_last_error(void) { return g_err.c_str(); }

const char* rtr_status_string(int s) {
    switch (s) {
        case RTR_OK: return "RTR_OK";
        case RTR_ERR_INVALID_ARGUMENT: return "RTR_ERR_INVALID_ARGUMENT";
        case RTR_ERR_HIP: return "RTR_ERR_HIP";
        case RTR_ERR_NO_DEVICE: return "RTR_ERR_NO_DEVICE";
        case RTR_ERR_UNSUPPORTED: return "RTR_ERR_UNSUPPORTED";
        case RTR_ERR_OUT_OF_MEMORY: return "RTR_ERR_OUT_OF_MEMORY";
        case RTR_ERR_BVH_TOO_DEEP: return "RTR_ERR_BVH_TOO_DEEP";
        case RTR_ERR_IO: return "RTR_ERR_IO";
        default: return "RTR_ERR_UNKNOWN";
    }
}

int rtr_abi_version(void) { return RTR_ABI_VERSION; }

const char* rtr_kernel_revision(void) { return RTR_ANYHIT_KERNEL_REVISION; }

uint32_t rtr_shard_rows(uint32_t height, uint32_t bandRows, uint32_t shardCount) {
    if (bandRows == 0) bandRows = 8;
    if (shardCount <= 1) return height;               /* unsharded: no padding rows */
    uint32_t bands = (height + bandRows - 1) / bandRows;
    uint32_t per = (bands + shardCount - 1) / shardCount;
    return per * bandRows;
}

/* ---- context ------------------------------------------------------------------------------ */
/* priorityRank < 0: a stream of default priority.  >= 0: rank 0 gets the device's highest stream priority, rank 1 the next ... (the
 * parts of a split render: the dispatcher then prefers the workgroups of an earlier part wherever two parts compete for a slot) */
extern "C++" int rtrapi::ctx_create_prio(int ordinal, int priorityRank, rtr_ctx** out) {
    if (!out) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_ctx_create: out is null");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(RTR_ERR_NO_DEVICE, "rtr_ctx_create: no HIP device (%s); this library has no CPU fallback",
                    e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    if (ordinal < 0 || ordinal >= count) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_ctx_create: ordinal %d not in [0,%d)", ordinal, count);
    HIP_TRY(hipSetDevice(ordinal));
    rtr_ctx* c = new rtr_ctx();
    c->device = ordinal;
    e = hipGetDeviceProperties(&c->prop, ordinal);
    if (e != hipSuccess) { delete c; return fail(RTR_ERR_HIP, "hipGetDeviceProperties: %s", hipGetErrorString(e)); }
    if (hipDeviceGetAttribute(&c->numXccs, hipDeviceAttributeNumberOfXccs, ordinal) != hipSuccess) c->numXccs = 0;
    if (priorityRank >= 0) {
        int least = 0, greatest = 0;                     /* numerically: greatest priority = the smaller number */
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { least = greatest = 0; }
        int prio = greatest + priorityRank;
        if (prio > least) prio = least;
        e = hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, prio);
    } else e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; return fail(RTR_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
    c->ownStream = true;
    c->tun = rtrdev::tunables_from_env();
    *out = c;
    return RTR_OK;
}

int rtr_ctx_create(int ordinal, rtr_ctx** out) { return ctx_create_prio(ordinal, -1, out); }

int rtr_ctx_set_tunable(rtr_ctx* c, const char* name, uint32_t value) {
    if (!c || !name) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_ctx_set_tunable: null argument");
    if (!rtrdev::tunable_set(c->tun, name, value)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_ctx_set_tunable: no tunable '%s', or %u is outside its range", name, value);
    return RTR_OK;
}

int rtr_ctx_get_tunable(const rtr_ctx* c, const char* name, uint32_t* value) {
    if (!c || !name || !value) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_ctx_get_tunable: null argument");
    if (!rtrdev::tunable_get(c->tun, name, value)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_ctx_get_tunable: no tunable '%s'", name);
    return RTR_OK;
}

void rtr_ctx_destroy(rtr_ctx* c) {
    if (!c || c->destroyed) return;
    if (c->children > 0) { (void)hipSetDevice(c->device); (void)hipStreamSynchronize(c->stream); c->destroyed = true; return; }
    ctx_free(c);
}

int rtr_ctx_set_stream(rtr_ctx* c, void* s) {
    if (!c) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_ctx_set_stream: ctx is null");
    HIP_TRY(hipSetDevice(c->device));
    if (c->ownStream && c->stream) { HIP_TRY(hipStreamSynchronize(c->stream)); (void)hipStreamDestroy(c->stream); }
    if (s) { c->stream = (hipStream_t)s; c->ownStream = false; }
    else { HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->ownStream = true; }
    return RTR_OK;
}

int rtr_ctx_get_stream(rtr_ctx* c, void** out) {
    if (!c || !out) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_ctx_get_stream: null argument");
    *out = (void*)c->stream;
    return RTR_OK;
}

int rtr_ctx_device_name(rtr_ctx* c, char* buf, size_t bytes) {
    if (!c || !buf || bytes == 0) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_ctx_device_name: bad argument");
    if (c->numXccs > 0) snprintf(buf, bytes, "%s (%s, %d CUs in %d XCDs)", c->prop.name, c->prop.gcnArchName, c->prop.multiProcessorCount, c->numXccs);
    else snprintf(buf, bytes, "%s (%s)", c->prop.name, c->prop.gcnArchName);
    return RTR_OK;
}

/* ---- scene -------------------------------------------------------------------------------- */
static int validate_desc(const rtr_scene_desc* d) {
    if (!d) return fail(RTR_ERR_INVALID_ARGUMENT, "scene desc is null");
    if ((d->numVertices && !d->vertices) || (d->numIndices && !d->indices) || (d->numMeshes && !d->meshes) ||
        (d->numInstances && !d->instances) || (d->numObjects && !d->objects) || (d->numLights && !d->lights))
        return fail(RTR_ERR_INVALID_ARGUMENT, "scene desc: null array with non-zero count");
    if ((d->ltc1 == nullptr) != (d->ltc2 == nullptr)) return fail(RTR_ERR_INVALID_ARGUMENT, "scene desc: ltc1 and ltc2 must both be given or both null");
    for (uint32_t m = 0; m < d->numMeshes; ++m) {
        const RtrMesh& me = d->meshes[m];
        if (me.indexCount % 3u) return fail(RTR_ERR_INVALID_ARGUMENT, "mesh %u: indexCount %u not a multiple of 3", m, me.indexCount);
        if ((uint64_t)me.indexOffset + me.indexCount > d->numIndices) return fail(RTR_ERR_INVALID_ARGUMENT, "mesh %u: index range exceeds the index array", m);
        if ((uint64_t)me.vertexOffset + me.vertexCount > d->numVertices) return fail(RTR_ERR_INVALID_ARGUMENT, "mesh %u: vertex range exceeds the vertex array", m);
        for (uint32_t i = 0; i < me.indexCount; ++i)
            if (d->indices[me.indexOffset + i] >= me.vertexCount)
                return fail(RTR_ERR_INVALID_ARGUMENT, "mesh %u: index %u (= %u) outside its %u vertices", m, i, d->indices[me.indexOffset + i], me.vertexCount);
    }
    std::vector<uint8_t> seen(d->numInstances, 0);
    for (uint32_t i = 0; i < d->numInstances; ++i) {
        const RtrInstance& in = d->instances[i];
        if (in.meshIndex >= d->numMeshes) return fail(RTR_ERR_INVALID_ARGUMENT, "instance %u: meshIndex %u >= %u", i, in.meshIndex, d->numMeshes);
        if (in.customIndex >= d->numInstances || seen[in.customIndex]) return fail(RTR_ERR_INVALID_ARGUMENT, "instance %u: customIndex %u out of range or duplicated", i, in.customIndex);
        seen[in.customIndex] = 1;
        if (in.customIndex >= d->numLights && in.customIndex - d->numLights >= d->numObjects)
            return fail(RTR_ERR_INVALID_ARGUMENT, "instance %u: customIndex %u has no ObjectInfo (numLights %u, numObjects %u)", i, in.customIndex, d->numLights, d->numObjects);
        if (in.customIndex >= d->numLights) {
            /* the hit shader reads indices / vertices through the ObjectInfo's offsets (closesthit.rchit:59-65), which the
             * reference sets to the mesh's own when it builds the TLAS (tlas.cppm:58-71): anything else would fetch another
             * mesh's data, or none */
            const RtrObjectInfo& oi = d->objects[in.customIndex - d->numLights];
            const RtrMesh& me = d->meshes[in.meshIndex];
            if (oi.vertexOffset != me.vertexOffset || oi.indexOffset != me.indexOffset)
                return fail(RTR_ERR_INVALID_ARGUMENT, "instance %u: ObjectInfo offsets (%u, %u) differ from its mesh's (%u, %u)", i, oi.vertexOffset, oi.indexOffset,
                            me.vertexOffset, me.indexOffset);
        }
        for (int k = 0; k < 12; ++k)
            if (!(in.transform[k] == in.transform[k]) || in.transform[k] > 3.0e38f || in.transform[k] < -3.0e38f)
                return fail(RTR_ERR_INVALID_ARGUMENT, "instance %u: non-finite transform", i);
    }
    if (d->numLights > d->numInstances) return fail(RTR_ERR_INVALID_ARGUMENT, "numLights %u > numInstances %u (lights are the first instances)", d->numLights, d->numInstances);
    if (d->numTextures && !d->textures) return fail(RTR_ERR_INVALID_ARGUMENT, "scene desc: null texture array with non-zero count");
    auto tex_ok = [&](const rtr_texture& t) { return t.pixels && t.width > 0 && t.height > 0 && t.width <= 65536 && t.height <= 65536 && (t.channels == 1 || t.channels == 4); };
    for (uint32_t t = 0; t < d->numTextures; ++t)
        if (d->textures[t].pixels && !tex_ok(d->textures[t])) return fail(RTR_ERR_INVALID_ARGUMENT, "texture %u: bad extent %ux%u or channels %u (1 or 4)", t, d->textures[t].width, d->textures[t].height, d->textures[t].channels);
    if (d->hdri && !tex_ok(*d->hdri)) return fail(RTR_ERR_INVALID_ARGUMENT, "hdri: bad extent or channels");
    for (uint32_t o = 0; o < d->numObjects; ++o) {
        const RtrObjectInfo& oi = d->objects[o];
        const struct { uint32_t uses, index; const char* what; } maps[4] = {{oi.usesColorMap, oi.colorIndex, "color"}, {oi.usesSpecularMap, oi.specularIndex, "specular"},
                                                                            {oi.usesMetallicMap, oi.metallicIndex, "metallic"}, {oi.usesOpacityMap, oi.opacityIndex, "opacity"}};
        for (const auto& m : maps)
            if (m.uses && (m.index >= d->numTextures || !d->textures[m.index].pixels))
                return fail(RTR_ERR_INVALID_ARGUMENT, "object %u uses a %s map but texture index %u is not in the texture array (%u entries); "
                            "the library never substitutes a constant for a missing texture", o, m.what, m.index, d->numTextures);
    }
    for (uint32_t l = 0; l < d->numLights; ++l) {
        const RtrAreaLightInfo& li = d->lights[l];
        if ((uint64_t)li.indexOffset + 3ull * li.numTriangles > d->numIndices) return fail(RTR_ERR_INVALID_ARGUMENT, "light %u: triangle range exceeds the index array", l);
        for (uint32_t i = 0; i < 3u * li.numTriangles; ++i)
            if ((uint64_t)li.vertexOffset + d->indices[li.indexOffset + i] >= d->numVertices)
                return fail(RTR_ERR_INVALID_ARGUMENT, "light %u: vertex reference outside the vertex array", l);
    }
    return RTR_OK;
}

/* The mirrored bit of an instance (the ray queries' face culling, RTR_QUERY_CULL_BACK/FRONT_FACING): 1 iff the determinant of its 3x3
 * transform, evaluated in double, is negative — the instance turns the winding of its triangles over, and Vulkan decides facing in object
 * space.  It lives in word kMirroredWord of the instance's 12-float slot of the normal-matrix table, which the matrix does not use: a
 * per-customIndex table that is uploaded with the transforms by create, create_like and update_instances, and that no triangle record
 * and no kernel argument had to change for.  The determinant is rtr_mirrored_bit (kernels/rtr_mirrored.h), which the enqueued instance update's kernel evaluates too. */
static void set_mirrored_word(const float* m, float* nmatSlot) {
    const uint32_t bit = rtr_mirrored_bit(m);
    memcpy(&nmatSlot[rtrdev::kMirroredWord], &bit, sizeof bit);
}

/* the per-customIndex transform tables: the 3x4 transforms, and the normal matrices with the mirrored word */
static void instance_tables(uint32_t numInstances, const RtrInstance* instances, std::vector<float>& xforms, std::vector<float>& nmats) {
    xforms.assign(12 * (size_t)numInstances, 0.f);
    nmats.assign(12 * (size_t)numInstances, 0.f);
    for (uint32_t i = 0; i < numInstances; ++i) {
        memcpy(&xforms[12 * (size_t)instances[i].customIndex], instances[i].transform, 12 * sizeof(float));
        rtr_normal_matrix(instances[i].transform, &nmats[12 * (size_t)instances[i].customIndex]);
        set_mirrored_word(instances[i].transform, &nmats[12 * (size_t)instances[i].customIndex]);
    }
}

/* flatten TLAS instances to one world-space triangle soup (instance order, then primitive order),
 * fill the per-customIndex transform tables, build the BVH */
static int flatten_and_build(const rtr_scene_desc* d, rtr::BvhResult& bvh, std::vector<float>& xforms, std::vector<float>& nmats,
                             uint32_t* stackEntries, size_t* numTris) {
    std::vector<rtr::WorldTriangle> soup;
    size_t total = 0;
    for (uint32_t i = 0; i < d->numInstances; ++i) total += d->meshes[d->instances[i].meshIndex].indexCount / 3u;
    soup.reserve(total);
    instance_tables(d->numInstances, d->instances, xforms, nmats);
    for (uint32_t i = 0; i < d->numInstances; ++i) {
        const RtrInstance& in = d->instances[i];
        const RtrMesh& me = d->meshes[in.meshIndex];
        for (uint32_t t = 0; t < me.indexCount / 3u; ++t) {
            rtr::WorldTriangle w;
            for (int k = 0; k < 3; ++k) {
                const uint32_t idx = d->indices[me.indexOffset + 3u * t + k] + me.vertexOffset;
                const rtr_v3 p = rtr_xform_point34(in.transform, rtr_ld3(d->vertices[idx].position));
                w.v[k][0] = p.x; w.v[k][1] = p.y; w.v[k][2] = p.z;
            }
            w.customIndex = in.customIndex; w.primitiveId = t;
            /* any-hit (opacity.rahit) runs only on non-opaque geometry (blas.cppm:98-100) of objects with an opacity map */
            w.flags = (in.customIndex >= d->numLights && d->objects[in.customIndex - d->numLights].usesOpacityMap != 0 && me.isOpaque == 0) ? 1u : 0u;
            soup.push_back(w);
        }
    }
    std::string err;
    if (!rtr::build_bvh(soup, bvh, &err)) return fail(RTR_ERR_INVALID_ARGUMENT, "BVH build: %s", err.c_str());
    if (bvh.maxDepth > 64)
        return fail(RTR_ERR_BVH_TOO_DEEP, "BVH depth %u exceeds the 64-entry LDS traversal stack", bvh.maxDepth);
    *stackEntries = bvh.maxDepth <= 16 ? 16 : (bvh.maxDepth <= 32 ? 32 : 64);
    *numTris = soup.size();
    return RTR_OK;
}

static void fill_stats(rtr_scene_stats& st, const rtr::BvhResult& bvh, uint32_t stackEntries, size_t numTris) {
    memset(&st, 0, sizeof st);
    st.numTriangles = (uint32_t)numTris;
    st.numNodes = (uint32_t)bvh.nodes.size();
    st.maxDepth = bvh.maxDepth;
    st.maxLeafSize = bvh.maxLeafSize;
    st.bvhLayoutVersion = RTR_BVH_LAYOUT_VERSION;
    st.stackEntries = stackEntries;
    st.buildMs = bvh.buildMs;
    st.sahCost = bvh.sahCost;
    st.grid = bvh.grid;
    for (int k = 0; k < 3; ++k) { st.boundsMin[k] = bvh.boundsMin[k]; st.boundsMax[k] = bvh.boundsMax[k]; }
    st.boxPad = bvh.boxPad;
}

int rtr_host_build_bvh(const rtr_scene_desc* d, rtr_scene_stats* stats, RtrBvhNode* nodes, size_t nodeBytes, RtrBvhTri* tris, size_t triBytes) {
    return rtr_host_build_bvh_wide(d, stats, nodes, nodeBytes, tris, triBytes, nullptr, 0);
}

int rtr_host_build_bvh_wide(const rtr_scene_desc* d, rtr_scene_stats* stats, RtrBvhNode* nodes, size_t nodeBytes, RtrBvhTri* tris, size_t triBytes,
                            RtrWideNode* wide, size_t wideBytes) {
    int rc = validate_desc(d);
    if (rc != RTR_OK) return rc;
    rtr::BvhResult bvh; std::vector<float> xf, nm; uint32_t stackEntries = 0; size_t numTris = 0;
    rc = flatten_and_build(d, bvh, xf, nm, &stackEntries, &numTris);
    if (rc != RTR_OK) return rc;
    if (stats) fill_stats(*stats, bvh, stackEntries, numTris);
    if (wide || (stats && !nodes && !tris)) {
        std::vector<RtrWideNode> w;
        rtr::make_wide_host(bvh.nodes.data(), bvh.nodes.size(), bvh.wideShape.size() == bvh.nodes.size() ? bvh.wideShape.data() : nullptr, bvh.grid, w);
        if (stats) { stats->grid = bvh.grid; stats->numWideNodes = (uint32_t)w.size(); stats->wideLayoutVersion = RTR_WIDE_LAYOUT_VERSION; }
        if (wide) {
            if (wideBytes != w.size() * sizeof(RtrWideNode)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_host_build_bvh_wide: wideBytes %zu != %zu", wideBytes, w.size() * sizeof(RtrWideNode));
            memcpy(wide, w.data(), wideBytes);
        }
    }
    if (nodes) {
        if (nodeBytes != bvh.nodes.size() * sizeof(RtrBvhNode)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_host_build_bvh: nodeBytes %zu != %zu", nodeBytes, bvh.nodes.size() * sizeof(RtrBvhNode));
        memcpy(nodes, bvh.nodes.data(), nodeBytes);
    }
    if (tris) {
        if (triBytes != bvh.tris.size() * sizeof(RtrBvhTri)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_host_build_bvh: triBytes %zu != %zu", triBytes, bvh.tris.size() * sizeof(RtrBvhTri));
        memcpy(tris, bvh.tris.data(), triBytes);
    }
    return RTR_OK;
}

/* canonical (instance-major) primitive table + per-customIndex instance table for the device flatten kernel */
static void make_prim_tables(const rtr_scene_desc* d, const RtrInstance* instances, std::vector<rtrdev::PrimRef>& prims,
                             std::vector<rtrdev::InstanceRef>& refs) {
    prims.clear();
    refs.assign(d->numInstances, rtrdev::InstanceRef{});
    for (uint32_t i = 0; i < d->numInstances; ++i) {
        const RtrInstance& in = instances[i];
        const RtrMesh& me = d->meshes[in.meshIndex];
        rtrdev::InstanceRef& r = refs[in.customIndex];
        memcpy(r.transform, in.transform, sizeof r.transform);
        r.vertexOffset = me.vertexOffset; r.indexOffset = me.indexOffset;
        const uint32_t flags = (in.customIndex >= d->numLights && d->objects[in.customIndex - d->numLights].usesOpacityMap != 0 && me.isOpaque == 0) ? 1u : 0u;
        for (uint32_t t = 0; t < me.indexCount / 3u; ++t) prims.push_back(rtrdev::PrimRef{in.customIndex, t, flags, 0u});
    }
}

/* The host mirrors of a tree the device has (re)written, behind a join of the stream that did it: nodes, records, grid, and the
 * reduction words (`red`, handed back: [6] the largest |coordinate|, which gives boxPad, [7] the tree's depth). */
static int read_back_tree(SceneTree& t, uint32_t (&red)[8]) {
    HIP_TRY(hipMemcpy(t.hostNodes.data(), t.nodes.p, t.hostNodes.size() * sizeof(RtrBvhNode), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(t.hostTris.data(), t.tris.p, t.hostTris.size() * sizeof(RtrBvhTri), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&t.stats.grid, t.grid.p, sizeof(RtrBvhGrid), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(red, t.red.p, sizeof red, hipMemcpyDeviceToHost));
    float mabs; memcpy(&mabs, &red[6], 4);
    t.stats.boxPad = (mabs > 1e-6f ? mabs : 1e-6f) * 3.814697265625e-06f;
    return RTR_OK;
}

/* The host mirrors after enqueued updates (rtr_scene_update_vertices_async and rtr_scene_update_instances_async leave them stale):
 * joins the scene's stream and reads back what the synchronous refit reads back — nodes, records, grid, boxPad — and the count of
 * reached 4-wide entries k_wide_order left on the device; after an enqueued INSTANCE update also the transforms of hostInstances (from
 * the InstanceRef table, through customIndex) and hostLights.  Every call that looks at a mirror comes through here first; it costs
 * nothing while no update has been enqueued. */
extern "C++" int rtrapi::refresh_mirrors(const rtr_scene* cs) {
    if (!cs->mirrorsStale) return RTR_OK;
    rtr_scene* s = const_cast<rtr_scene*>(cs);
    HIP_TRY(hipSetDevice(s->ctx->device));
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    uint32_t red[8], reached = 0;
    { const int rc = read_back_tree(s->tree, red); if (rc != RTR_OK) return rc; }
    HIP_TRY(hipMemcpy(&reached, s->asyncWords.p + 1, sizeof reached, hipMemcpyDeviceToHost));
    s->tree.wideReached = reached; s->tree.stats.numWideNodes = reached;
    /* after an enqueued rebuild the depth is the new tree's (or, refused, still the old one's: a refit keeps it); stackEntries stays — an
     * enqueued rebuild never lowers the class, and the device refused one that would raise it */
    if (s->depthStale) { s->tree.stats.maxDepth = red[7]; s->depthStale = false; }
    if (s->instancesStale) {
        static_assert(sizeof(rtrdev::InstanceRef) == 64 && sizeof(RtrInstance) == 64, "layout");
        std::vector<rtrdev::InstanceRef> refs(s->hostInstances.size());
        if (!refs.empty()) HIP_TRY(hipMemcpy(refs.data(), s->tree.instRefs.p, refs.size() * sizeof(rtrdev::InstanceRef), hipMemcpyDeviceToHost));
        for (RtrInstance& in : s->hostInstances) memcpy(in.transform, refs[in.customIndex].transform, sizeof in.transform);
        if (s->numLights) HIP_TRY(hipMemcpy(s->hostLights.data(), s->lights.p, s->numLights * sizeof(RtrAreaLightInfo), hipMemcpyDeviceToHost));
        s->instancesStale = false;
    }
    s->mirrorsStale = false;
    return RTR_OK;
}

/* (re)computes the per-light-triangle records light_loops reads; the light transforms live in s->lights on the device */
static int make_light_tris(rtr_scene* s) {
    if (s->numLights == 0) return RTR_OK;
    hipError_t e = rtrdev::launch_light_tris(s->lights.p, s->vertices.p, s->indices.p, s->lightTriFirst.p, s->numLights, s->lightTris.p, s->ctx->stream);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "light-triangle records: %s", hipGetErrorString(e));
    if (const int rc = enqueue_light_power(s, s->ctx->stream, "light-triangle records")) return rc;      /* a power table follows its records */
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));     /* frames of other contexts may render this scene next */
    return RTR_OK;
}

/* computes the per-object material terms fetch_surface reads, on the device, from s->objects */
static int make_object_terms(rtr_scene* s) {
    if (s->numObjects == 0) return RTR_OK;
    HIP_TRY(s->objectTerms.alloc((size_t)s->numObjects * rtrdev::kObjectTermsRecord));
    hipError_t e = rtrdev::launch_object_terms(s->objects.p, s->numObjects, s->objectTerms.p, s->ctx->stream);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "object terms: %s", hipGetErrorString(e));
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));     /* frames of other contexts may render this scene next */
    return RTR_OK;
}

/* (re)builds the 4-wide view of the tree the any-hit kernel walks, on the device, from the quantised BVH2 nodes */
static int make_wide_nodes(SceneTree& t, const RtrAreaLightInfo* lights, uint32_t numLights, hipStream_t st) {
    const uint32_t n = (uint32_t)t.hostNodes.size();
    /* wideRemap: the permutation, then bvh_hot_top's scratch */
    if (!t.nodes4.p) { HIP_TRY(t.nodes4.alloc((size_t)n * 4)); HIP_TRY(t.nodes4tmp.alloc((size_t)n * 4)); HIP_TRY(t.wideRemap.alloc(n + rtrdev::bvh_hot_top_words())); HIP_TRY(t.wideSums.alloc(rtrdev::bvh_wide_scratch_words())); }
    if (!t.hostWideShape.empty() && !t.wideShape.p) HIP_TRY(t.wideShape.upload(t.hostWideShape.data(), t.hostWideShape.size(), st));
    hipError_t e = rtrdev::bvh_make_wide(t.nodes.p, n, t.refitReady ? t.parent.p : nullptr, t.grid.p, t.hostWideShape.size() == n ? t.wideShape.p : nullptr, t.nodes4tmp.p, t.wideSums.p, st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "4-wide node build: %s", hipGetErrorString(e));
    /* breadth-first order of the 4-wide tree (child codes = the 4th 16 bytes of every entry); entries the 4-wide tree does not reach
     * keep the ids after them.  bvh_hot_top then moves the best-first top towards the lights to the front (kernels/rtr_hot_top.h):
     * k_shadow_trace4 keeps the first entries in LDS. */
    std::vector<uint32_t> codes((size_t)n * 4), remap(n, 0xffffffffu), order;
    HIP_TRY(hipMemcpy2DAsync(codes.data(), 16, reinterpret_cast<const char*>(t.nodes4tmp.p) + 48, 64, 16, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    order.reserve(n);
    order.push_back(0); remap[0] = 0;
    for (size_t head = 0; head < order.size(); ++head)
        for (int k = 0; k < 4; ++k) {
            const int32_t c = (int32_t)codes[(size_t)order[head] * 4 + k];
            if (c >= 0 && (uint32_t)c < n && remap[c] == 0xffffffffu) { remap[c] = (uint32_t)order.size(); order.push_back((uint32_t)c); }
        }
    uint32_t next = (uint32_t)order.size();
    for (uint32_t i = 0; i < n; ++i) if (remap[i] == 0xffffffffu) remap[i] = next++;
    HIP_TRY(hipMemcpyAsync(t.wideRemap.p, remap.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    e = rtrdev::bvh_hot_top(t.nodes4tmp.p, n, t.wideRemap.p, t.wideRemap.p + n, t.grid.p, lights, numLights, rtrdev::trace_top_capacity(), st);
    if (e == hipSuccess) e = rtrdev::bvh_permute_wide(t.nodes4tmp.p, n, t.wideRemap.p, t.nodes4.p, st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "4-wide node order: %s", hipGetErrorString(e));
    HIP_TRY(hipStreamSynchronize(st));
    t.wideReached = (uint32_t)order.size();
    HIP_TRY(hipMemcpy(&t.stats.grid, t.grid.p, sizeof(RtrBvhGrid), hipMemcpyDeviceToHost));     /* the wide centre was set on the device */
    t.stats.numWideNodes = t.wideReached; t.stats.wideLayoutVersion = RTR_WIDE_LAYOUT_VERSION;
    return RTR_OK;
}

static rtrdev::BvhDeviceArrays device_arrays(SceneTree& t) {
    rtrdev::BvhDeviceArrays a{};
    a.nodes = t.nodes.p; a.nodesF = t.nodesF.p; a.grid = t.grid.p; a.tris = t.tris.p; a.boxMin = t.boxMin.p; a.boxMax = t.boxMax.p; a.parent = t.parent.p;
    a.counters = t.counters.p; a.depth = t.depth.p; a.slotOfPrim = t.slotOfPrim.p; a.red = t.red.p;
    return a;
}

/* the build scratch for n triangles, allocated on first use and kept */
static int ensure_build_scratch(BuildScratch& bs, uint32_t n) {
    const uint32_t numNodes = n - 1;
    HIP_TRY(bs.trisCanon.ensure((size_t)n * 3)); HIP_TRY(bs.minCanon.ensure(n)); HIP_TRY(bs.maxCanon.ensure(n));
    HIP_TRY(bs.keysIn.ensure(n)); HIP_TRY(bs.keysOut.ensure(n)); HIP_TRY(bs.range.ensure(numNodes)); HIP_TRY(bs.rawChild.ensure(numNodes));
    bs.sortTempBytes = rtrdev::bvh_sort_temp_bytes(n);
    HIP_TRY(bs.sortTemp.ensure(bs.sortTempBytes));
    return RTR_OK;
}
static rtrdev::BvhScratch scratch_view(const BuildScratch& bs) {
    rtrdev::BvhScratch sc{};
    sc.trisCanon = bs.trisCanon.p; sc.minCanon = bs.minCanon.p; sc.maxCanon = bs.maxCanon.p; sc.keysIn = bs.keysIn.p; sc.keysOut = bs.keysOut.p;
    sc.range = bs.range.p; sc.rawChild = bs.rawChild.p; sc.sortTemp = bs.sortTemp.p; sc.sortTempBytes = bs.sortTempBytes;
    return sc;
}

/* Device LBVH build into t.nodes / t.tris (+ refit arrays) from the primitive tables and the DEVICE vertex / index arrays given;
 * fills hostNodes/hostTris and the stats.  The core rtr_scene_create (build_on_device) and rtr_scene_rebuild share: `t` is the fresh
 * tree that is built, `bs` the scratch (the caller's to keep or free). */
static int build_on_device_core(SceneTree& t, hipStream_t st, const std::vector<rtrdev::PrimRef>& prims, const std::vector<rtrdev::InstanceRef>& refs,
                                const RtrVertex* vertices, const uint32_t* indices, BuildScratch& bs, size_t numPrims) {
    const uint32_t n = (uint32_t)numPrims, numNodes = n - 1;
    auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(t.prims.upload(prims.data(), prims.size(), st));
    HIP_TRY(t.instRefs.upload(refs.data(), refs.size(), st));
    HIP_TRY(t.nodes.alloc((size_t)numNodes * 2)); HIP_TRY(t.nodesF.alloc((size_t)numNodes * 4)); HIP_TRY(t.grid.alloc(1));
    HIP_TRY(t.tris.alloc((size_t)n * 3));
    HIP_TRY(t.boxMin.alloc(n)); HIP_TRY(t.boxMax.alloc(n)); HIP_TRY(t.parent.alloc(numNodes));
    HIP_TRY(t.counters.alloc(numNodes)); HIP_TRY(t.depth.alloc(numNodes)); HIP_TRY(t.slotOfPrim.alloc(n)); HIP_TRY(t.red.alloc(8));
    { const int rcs = ensure_build_scratch(bs, n); if (rcs != RTR_OK) return rcs; }
    const rtrdev::BvhScratch sc = scratch_view(bs);
    HIP_TRY(hipMemsetAsync(t.nodesF.p, 0, (size_t)numNodes * 64, st));
    rtrdev::BvhInputs in{t.prims.p, t.instRefs.p, vertices, indices};
    hipError_t e = rtrdev::bvh_build_lbvh(in, n, device_arrays(t), sc, st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "device BVH build: %s", hipGetErrorString(e));
    HIP_TRY(hipStreamSynchronize(st));
    t.hostNodes.resize(numNodes); t.hostTris.resize(n);
    memset(&t.stats, 0, sizeof t.stats);
    uint32_t red[8];
    { const int rc = read_back_tree(t, red); if (rc != RTR_OK) return rc; }
    const float buildMs = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (red[7] > 64) return fail(RTR_ERR_BVH_TOO_DEEP, "device-built BVH depth %u exceeds the 64-entry LDS traversal stack", red[7]);
    t.stats.numTriangles = n; t.stats.numNodes = numNodes; t.stats.maxDepth = red[7]; t.stats.maxLeafSize = 4;
    t.stats.bvhLayoutVersion = RTR_BVH_LAYOUT_VERSION;
    t.stats.stackEntries = red[7] <= 16 ? 16 : (red[7] <= 32 ? 32 : 64);
    t.stats.buildMs = buildMs;
    t.numPrims = n; t.numNodeSlots = numNodes; t.refitReady = true;
    return RTR_OK;
}

/* rtr_scene_create's device build: the tables from the description, the vertices it uploaded; the scratch goes with the call */
static int build_on_device(rtr_scene* s, const rtr_scene_desc* d, size_t numPrims) {
    std::vector<rtrdev::PrimRef> prims; std::vector<rtrdev::InstanceRef> refs;
    make_prim_tables(d, d->instances, prims, refs);
    for (uint32_t v = 0; v < d->numVertices; ++v)
        for (int k = 0; k < 3; ++k)
            if (!(d->vertices[v].position[k] > -3.0e38f && d->vertices[v].position[k] < 3.0e38f))
                return fail(RTR_ERR_INVALID_ARGUMENT, "BVH build: non-finite vertex position in vertex %u", v);
    BuildScratch scratch;
    return build_on_device_core(s->tree, s->ctx->stream, prims, refs, s->vertices.p, s->indices.p, scratch, numPrims);
}

/* DeviceScene's view of the tree: what the kernels walk */
static void point_at_tree(DeviceScene& dv, const SceneTree& t) {
    dv.nodes = t.nodes.p; dv.nodes4 = t.nodes4.p; dv.numNodes4 = (uint32_t)t.hostNodes.size(); dv.grid = t.grid.p; dv.tris = t.tris.p;
}

static int scene_create_impl(rtr_ctx* ctx, const rtr_scene_desc* d, const rtr_scene* like, rtr_scene** out) {
    if (!ctx || !out) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_create: null ctx/out");
    if (ctx->destroyed) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_create: the context has been destroyed");
    *out = nullptr;
    int rc = validate_desc(d);
    if (rc != RTR_OK) return rc;
    if (d->buildFlags > RTR_BUILD_DEVICE_LBVH) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_create: unknown buildFlags %u", d->buildFlags);
    HIP_TRY(hipSetDevice(ctx->device));
    size_t totalPrims = 0;
    for (uint32_t i = 0; i < d->numInstances; ++i) totalPrims += d->meshes[d->instances[i].meshIndex].indexCount / 3u;
    /* every triangle may end up in a leaf of its own: numTriangles - 1 inner nodes, hence as many 4-wide records at most */
    rc = rtr_check_scene_limits(totalPrims, totalPrims ? totalPrims - 1 : 0);
    if (rc != RTR_OK) return rc;
    /* tiny scenes always take the host builder (the radix tree needs a root with more than one leaf's worth of primitives) */
    const bool deviceBuild = !like && d->buildFlags == RTR_BUILD_DEVICE_LBVH && totalPrims >= 16;
    rtr::BvhResult bvh; std::vector<float> xforms, nmats; uint32_t stackEntries = 0; size_t numTris = 0;
    if (like) {
        rc = refresh_mirrors(like);
        if (rc != RTR_OK) return rc;
        /* the tree of `like`, as its host copy holds it (nodes and records are kept in step with the device by every update) */
        const SceneTree& lt = like->tree;
        if (lt.stats.numTriangles != totalPrims || lt.hostNodes.empty() || lt.hostTris.empty())
            return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_create_like: the built scene has %u triangles, this description %zu", lt.stats.numTriangles, totalPrims);
        bvh.nodes = lt.hostNodes; bvh.tris = lt.hostTris; bvh.grid = lt.stats.grid; bvh.wideShape = lt.hostWideShape;
        if (!like->hostMasks.empty()) for (RtrBvhTri& t : bvh.tris) t.flags &= ~RTR_TRI_MASK_BITS;      /* a new scene's instance masks are 0xff, whatever `like` has set */
        bvh.maxDepth = lt.stats.maxDepth; bvh.maxLeafSize = lt.stats.maxLeafSize; bvh.sahCost = lt.stats.sahCost; bvh.boxPad = lt.stats.boxPad;
        for (int k = 0; k < 3; ++k) { bvh.boundsMin[k] = lt.stats.boundsMin[k]; bvh.boundsMax[k] = lt.stats.boundsMax[k]; }
        bvh.buildMs = 0.f;                                   /* nothing was built here */
        stackEntries = lt.stats.stackEntries; numTris = lt.stats.numTriangles;
        instance_tables(d->numInstances, d->instances, xforms, nmats);
    } else if (!deviceBuild) {
        rc = flatten_and_build(d, bvh, xforms, nmats, &stackEntries, &numTris);
        if (rc != RTR_OK) return rc;
    } else {
        instance_tables(d->numInstances, d->instances, xforms, nmats);
    }

    rtr_scene* s = new rtr_scene();
    s->ctx = ctx; ++ctx->children;
    SceneTree& tree = s->tree;
    hipStream_t st = ctx->stream;
    hipError_t e = hipSuccess;
    auto chk = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    static_assert(sizeof(RtrBvhNode) == 2 * sizeof(uint4) && sizeof(RtrBvhTri) == 3 * sizeof(float4), "layout");
    if (!deviceBuild) {
        chk(tree.nodes.upload(reinterpret_cast<const uint4*>(bvh.nodes.data()), bvh.nodes.size() * 2, st));
        chk(tree.grid.upload(&bvh.grid, 1, st));
        chk(tree.tris.upload(reinterpret_cast<const float4*>(bvh.tris.data()), bvh.tris.size() * 3, st));
    }
    chk(s->vertices.upload(d->vertices, d->numVertices, st));
    chk(s->indices.upload(d->indices, d->numIndices, st));
    chk(s->objects.upload(d->objects, d->numObjects, st));
    chk(s->lights.upload(d->lights, d->numLights, st));
    {
        std::vector<uint32_t> first(d->numLights);
        uint32_t total = 0;
        for (uint32_t l = 0; l < d->numLights; ++l) { first[l] = total; total += d->lights[l].numTriangles; }
        chk(s->lightTriFirst.upload(first.data(), first.size(), st));
        chk(s->lightTris.alloc((size_t)total * rtrdev::kLightTriRecord));
        /* what a hit's primitiveId may be, per customIndex: a light's records or its instance's mesh triangles */
        std::vector<uint32_t> count(d->numInstances);
        for (uint32_t i = 0; i < d->numInstances; ++i) {
            const RtrInstance& in = d->instances[i];
            count[in.customIndex] = in.customIndex < d->numLights ? d->lights[in.customIndex].numTriangles : d->meshes[in.meshIndex].indexCount / 3u;
        }
        chk(s->triCount.upload(count.data(), count.size(), st));
        s->hostTriCount.swap(count);
    }
    chk(s->xforms.upload(xforms.data(), xforms.size(), st));
    chk(s->nmats.upload(nmats.data(), nmats.size(), st));
    if (d->ltc1) {
        chk(s->ltc1.upload(d->ltc1, 64 * 64 * 4, st));
        chk(s->ltc2.upload(d->ltc2, 64 * 64 * 4, st));
        s->hasLtc = true;
    }
    std::vector<rtrdev::DeviceTexture> table(d->numTextures);
    s->texPixels.resize(d->numTextures);
    for (uint32_t t = 0; t < d->numTextures; ++t) {
        const rtr_texture& tx = d->textures[t];
        table[t] = rtrdev::DeviceTexture{nullptr, 0, 0, 0, 0};
        if (!tx.pixels) continue;
        chk(s->texPixels[t].upload(tx.pixels, (size_t)tx.width * tx.height * tx.channels, st));
        table[t] = rtrdev::DeviceTexture{s->texPixels[t].p, tx.width, tx.height, tx.channels, 0};
    }
    chk(s->texTable.upload(table.data(), table.size(), st));
    rtrdev::DeviceTexture hdri{nullptr, 0, 0, 0, 0};
    if (d->hdri) {
        chk(s->hdriPixels.upload(d->hdri->pixels, (size_t)d->hdri->width * d->hdri->height * d->hdri->channels, st));
        hdri = rtrdev::DeviceTexture{s->hdriPixels.p, d->hdri->width, d->hdri->height, d->hdri->channels, 0};
    }
    if (e != hipSuccess) {
        delete s; ctx_release_child(ctx);
        return fail(e == hipErrorOutOfMemory ? RTR_ERR_OUT_OF_MEMORY : RTR_ERR_HIP, "scene upload: %s", hipGetErrorString(e));
    }
    s->numLights = d->numLights; s->numObjects = d->numObjects; s->numInstances = d->numInstances; s->numVertices = d->numVertices; s->numIndices = d->numIndices;
    if (d->numLights) s->hostLights.assign(d->lights, d->lights + d->numLights);
    if (d->numInstances) s->hostInstances.assign(d->instances, d->instances + d->numInstances);
    if (d->numMeshes) s->hostMeshes.assign(d->meshes, d->meshes + d->numMeshes);
    if (d->numObjects) s->hostObjects.assign(d->objects, d->objects + d->numObjects);
    if (deviceBuild) {
        rc = build_on_device(s, d, totalPrims);
        if (rc != RTR_OK) { delete s; ctx_release_child(ctx); return rc; }
    } else {
        fill_stats(tree.stats, bvh, stackEntries, numTris);
        tree.hostNodes.swap(bvh.nodes);
        tree.hostTris.swap(bvh.tris);
        tree.hostWideShape.swap(bvh.wideShape);
        tree.numPrims = (uint32_t)tree.hostTris.size(); tree.numNodeSlots = (uint32_t)tree.hostNodes.size();
    }

    rc = make_wide_nodes(tree, s->lights.p, s->numLights, st);
    if (rc == RTR_OK) rc = make_light_tris(s);
    if (rc == RTR_OK) rc = make_object_terms(s);
    if (rc != RTR_OK) { delete s; ctx_release_child(ctx); return rc; }
    DeviceScene& dv = s->dev;
    point_at_tree(dv, tree);
    dv.vertices = s->vertices.p; dv.indices = s->indices.p;
    dv.objects = s->objects.p; dv.objectTerms = s->objectTerms.p; dv.lights = s->lights.p;
    dv.lightTris = s->lightTris.p; dv.lightTriFirst = s->lightTriFirst.p;
    dv.xforms = s->xforms.p; dv.nmats = s->nmats.p;
    dv.ltc1 = s->hasLtc ? s->ltc1.p : nullptr; dv.ltc2 = s->hasLtc ? s->ltc2.p : nullptr;
    for (int k = 0; k < 3; ++k) dv.skyLinear[k] = rtr_to_linear(d->skyColor[k]);
    dv.numLights = d->numLights;
    dv.numLightTris = 0;
    for (uint32_t l = 0; l < d->numLights; ++l) dv.numLightTris += d->lights[l].numTriangles;
    dv.textures = s->texTable.p;
    dv.hdri = hdri;
    *out = s;
    return RTR_OK;
}

int rtr_scene_create(rtr_ctx* ctx, const rtr_scene_desc* d, rtr_scene** out) { return scene_create_impl(ctx, d, nullptr, out); }

int rtr_scene_create_like(rtr_ctx* ctx, const rtr_scene_desc* d, const rtr_scene* built, rtr_scene** out) {
    if (!built) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_create_like: null scene to copy the tree from");
    return scene_create_impl(ctx, d, built, out);
}

/* parent links of a node array, as the refit keeps them: (parentIndex << 1) | slot, -1 for the root, -2 for a slot the root does not
 * reach; returns how many slots it reaches */
static size_t host_parent_array(const std::vector<RtrBvhNode>& nodes, std::vector<int32_t>& parent) {
    parent.assign(nodes.size(), -2);
    if (nodes.empty()) return 0;
    parent[0] = -1;
    size_t reached = 1;
    std::vector<uint32_t> stack{0};
    while (!stack.empty()) {
        const uint32_t i = stack.back(); stack.pop_back();
        for (int sl = 0; sl < 2; ++sl) {
            const int32_t c = nodes[i].child[sl];
            if (c >= 0 && parent[(size_t)c] == -2) { parent[(size_t)c] = (int32_t)((i << 1) | (uint32_t)sl); stack.push_back((uint32_t)c); ++reached; }
        }
    }
    return reached;
}

/* A host-built tree gets its refit arrays on the first update: parent links from the node array, the
 * canonical-primitive -> leaf-slot map from the ids stored in the triangle records. */
static int ensure_refit_ready(rtr_scene* s) {
    SceneTree& t = s->tree;
    if (t.refitReady) return RTR_OK;
    if (s->hostInstances.empty()) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_update_instances: the scene has no instances");
    hipStream_t st = s->ctx->stream;
    const uint32_t numNodes = (uint32_t)t.hostNodes.size(), n = (uint32_t)t.hostTris.size();
    std::vector<int32_t> parent;
    host_parent_array(t.hostNodes, parent);
    /* canonical order = instances in creation order, primitives in mesh order */
    std::vector<uint32_t> base(s->hostInstances.size(), 0);       /* by customIndex */
    uint32_t acc = 0;
    for (const RtrInstance& in : s->hostInstances) { base[in.customIndex] = acc; acc += s->hostMeshes[in.meshIndex].indexCount / 3u; }
    if (acc != n) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_update_instances: scene has no geometry to refit");
    std::vector<uint32_t> slotOfPrim(n, 0);
    for (uint32_t slot = 0; slot < n; ++slot) slotOfPrim[base[t.hostTris[slot].customIndex] + t.hostTris[slot].primitiveId] = slot;
    /* the fit works on fp32 planes: child codes from the host tree, boxes recomputed by the refit */
    std::vector<rtr::BvhNodeF> nf(numNodes);
    for (uint32_t i = 0; i < numNodes; ++i) {
        memset(&nf[i], 0, sizeof nf[i]);
        nf[i].child[0] = t.hostNodes[i].child[0]; nf[i].child[1] = t.hostNodes[i].child[1];
    }
    HIP_TRY(t.nodesF.upload(reinterpret_cast<const float4*>(nf.data()), (size_t)numNodes * 4, st));
    HIP_TRY(t.parent.upload(parent.data(), parent.size(), st));
    HIP_TRY(t.slotOfPrim.upload(slotOfPrim.data(), slotOfPrim.size(), st));
    HIP_TRY(t.boxMin.alloc(n)); HIP_TRY(t.boxMax.alloc(n));
    HIP_TRY(t.counters.alloc(numNodes)); HIP_TRY(t.depth.alloc(numNodes)); HIP_TRY(t.red.alloc(8));
    t.numPrims = n; t.numNodeSlots = numNodes; t.refitReady = true;
    return RTR_OK;
}

/* per customIndex: the complement of the instance's mask where the records keep it (RtrBvhTri::flags, RTR_TRI_MASK_SHIFT) */
static std::vector<uint32_t> instance_mask_bits(const rtr_scene* s, const uint8_t* masks) {
    std::vector<uint32_t> bits(s->hostInstances.size(), 0u);
    for (size_t i = 0; i < s->hostInstances.size(); ++i) bits[s->hostInstances[i].customIndex] = ((uint32_t)(uint8_t)~masks[i]) << RTR_TRI_MASK_SHIFT;
    return bits;
}

/* the description a scene's host mirrors make (no vertices, no indices: the device holds those) */
static rtr_scene_desc host_view(const rtr_scene* s) {
    rtr_scene_desc view{};
    view.meshes = s->hostMeshes.data(); view.numMeshes = (uint32_t)s->hostMeshes.size();
    view.instances = s->hostInstances.data(); view.numInstances = (uint32_t)s->hostInstances.size();
    view.objects = s->hostObjects.data(); view.numObjects = (uint32_t)s->hostObjects.size();
    view.lights = s->hostLights.data(); view.numLights = s->numLights;
    return view;
}

/* the tables a refit or a device build flattens from (PrimRef / InstanceRef) for the transforms given, with the instance masks in the
 * flags: both write the records from this table */
static void scene_prim_tables(const rtr_scene* s, const RtrInstance* inst, std::vector<rtrdev::PrimRef>& prims, std::vector<rtrdev::InstanceRef>& refs) {
    const rtr_scene_desc view = host_view(s);
    make_prim_tables(&view, inst, prims, refs);
    if (s->hostMasks.empty()) return;
    const std::vector<uint32_t> bits = instance_mask_bits(s, s->hostMasks.data());
    for (rtrdev::PrimRef& pr : prims) pr.flags |= bits[pr.customIndex];
}

/* those tables on the device, for the scene's tree */
static int upload_prim_tables(rtr_scene* s, const RtrInstance* inst) {
    std::vector<rtrdev::PrimRef> prims; std::vector<rtrdev::InstanceRef> refs;
    scene_prim_tables(s, inst, prims, refs);
    HIP_TRY(s->tree.prims.upload(prims.data(), prims.size(), s->ctx->stream));
    HIP_TRY(s->tree.instRefs.upload(refs.data(), refs.size(), s->ctx->stream));
    return RTR_OK;
}

int rtr_scene_set_instance_masks(rtr_scene* s, const uint8_t* masks, uint32_t numInstances) {
    if (!s || (!masks && numInstances)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_set_instance_masks: null argument");
    if (numInstances != s->hostInstances.size()) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_set_instance_masks: %u masks given, scene has %zu instances", numInstances, s->hostInstances.size());
    if (numInstances == 0) return RTR_OK;
    const std::vector<uint32_t> bits = instance_mask_bits(s, masks);
    HIP_TRY(hipSetDevice(s->ctx->device));
    { const int rcm = refresh_mirrors(s); if (rcm != RTR_OK) return rcm; }
    /* queries of OTHER contexts (other streams) may be walking these records: everything enqueued on the device so far is joined before
     * they are rewritten (contract in rtr.h, as rtr_scene_update_instances) */
    HIP_TRY(hipDeviceSynchronize());
    hipStream_t st = s->ctx->stream;
    const uint32_t numTris = (uint32_t)(s->tree.tris.n / 3);
    HIP_TRY(s->maskBits.upload(bits.data(), bits.size(), st));
    const hipError_t e = rtrdev::launch_set_instance_masks(s->tree.tris.p, numTris, s->maskBits.p, numInstances, st);
    if (const int rc = launched(e, "rtr_scene_set_instance_masks")) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    /* the host mirror (rtr_scene_export_bvh, rtr_scene_create_like) in step: the same rule as the kernel's */
    for (RtrBvhTri& t : s->tree.hostTris)
        if (t.customIndex < numInstances) t.flags = (t.flags & ~RTR_TRI_MASK_BITS) | bits[t.customIndex];
    s->hostMasks.assign(masks, masks + numInstances);
    /* an enqueued refit writes its records from the device tables: they carry the new masks from here on */
    if (s->tree.asyncReady) return upload_prim_tables(s, s->hostInstances.data());
    return RTR_OK;
}

int rtr_scene_get_instance_masks(const rtr_scene* s, uint8_t* masks, uint32_t numInstances) {
    if (!s || (!masks && numInstances)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_get_instance_masks: null argument");
    if (numInstances != s->hostInstances.size()) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_get_instance_masks: room for %u masks, scene has %zu instances", numInstances, s->hostInstances.size());
    for (uint32_t i = 0; i < numInstances; ++i) masks[i] = s->hostMasks.empty() ? 0xffu : s->hostMasks[i];
    return RTR_OK;
}

/* The argument checks the two refitting calls share (rtr_scene_update_instances, rtr_scene_update_vertices); `who` names the caller in
 * the message.  instances == NULL (rtr_scene_update_vertices only): the current transforms are kept and nothing is checked for them. */
static int check_refit_args(const rtr_scene* s, const RtrInstance* instances, uint32_t numInstances, const RtrAreaLightInfo* lights, uint32_t numLights,
                            const char* who) {
    if (instances) {
        if (numInstances != s->hostInstances.size()) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: %u instances given, scene has %zu", who, numInstances, s->hostInstances.size());
        for (uint32_t i = 0; i < numInstances; ++i) {
            if (instances[i].meshIndex != s->hostInstances[i].meshIndex || instances[i].customIndex != s->hostInstances[i].customIndex)
                return fail(RTR_ERR_INVALID_ARGUMENT, "%s: instance %u changed mesh or customIndex; only transforms may change (a refit keeps the topology)", who, i);
            for (int k = 0; k < 12; ++k)
                if (!(instances[i].transform[k] > -3.0e38f && instances[i].transform[k] < 3.0e38f))
                    return fail(RTR_ERR_INVALID_ARGUMENT, "%s: instance %u has a non-finite transform", who, i);
        }
    }
    if (lights) {
        if (numLights != s->numLights) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: %u lights given, scene has %u", who, numLights, s->numLights);
        for (uint32_t l = 0; l < numLights; ++l)
            if (lights[l].vertexOffset != s->hostLights[l].vertexOffset || lights[l].indexOffset != s->hostLights[l].indexOffset ||
                lights[l].numTriangles != s->hostLights[l].numTriangles)
                return fail(RTR_ERR_INVALID_ARGUMENT, "%s: light %u changed its mesh", who, l);
    }
    return RTR_OK;
}

/* The refit both calls end in, on a scene that is refit-ready and a device that has been joined: world-space records from the device
 * vertex array, boxes, grid, 4-wide view, host mirrors, boxPad.  instances == NULL keeps the current transforms (and with them the
 * transform, normal-matrix and mirrored tables); lights == NULL keeps the light infos.  lightTris: remake the light-triangle table even
 * when no lights are given (the vertices of a light's mesh may have changed). */
static int refit_scene(rtr_scene* s, const RtrInstance* instances, const RtrAreaLightInfo* lights, bool lightTris) {
    hipStream_t st = s->ctx->stream;
    const uint32_t numInstances = (uint32_t)s->hostInstances.size(), numLights = s->numLights;
    { const int rct = upload_prim_tables(s, instances ? instances : s->hostInstances.data()); if (rct != RTR_OK) return rct; }
    std::vector<float> xforms, nmats;      /* outlive the asynchronous copies: the stream is joined below */
    if (instances) {
        instance_tables(numInstances, instances, xforms, nmats);
        HIP_TRY(hipMemcpyAsync(s->xforms.p, xforms.data(), xforms.size() * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(s->nmats.p, nmats.data(), nmats.size() * sizeof(float), hipMemcpyHostToDevice, st));
    }
    if (lights && numLights) HIP_TRY(hipMemcpyAsync(s->lights.p, lights, numLights * sizeof(RtrAreaLightInfo), hipMemcpyHostToDevice, st));
    SceneTree& t = s->tree;
    rtrdev::BvhInputs in{t.prims.p, t.instRefs.p, s->vertices.p, s->indices.p};
    hipError_t e = rtrdev::bvh_refit(in, t.numPrims, t.numNodeSlots, device_arrays(t), st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "device BVH refit: %s", hipGetErrorString(e));
    HIP_TRY(hipStreamSynchronize(st));
    /* keep the host mirror (rtr_scene_export_bvh) and the stats in step */
    uint32_t red[8];
    { const int rcb = read_back_tree(t, red); if (rcb != RTR_OK) return rcb; }
    { const int rc4 = make_wide_nodes(t, s->lights.p, s->numLights, st); if (rc4 != RTR_OK) return rc4; }
    if (lightTris || (lights && numLights)) { const int rcl = make_light_tris(s); if (rcl != RTR_OK) return rcl; }
    if (instances) s->hostInstances.assign(instances, instances + numInstances);
    if (lights && numLights) s->hostLights.assign(lights, lights + numLights);
    return RTR_OK;
}

int rtr_scene_update_instances(rtr_scene* s, const RtrInstance* instances, uint32_t numInstances, const RtrAreaLightInfo* lights, uint32_t numLights) {
    if (!s || (!instances && numInstances)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_update_instances: null argument");
    if (numInstances != s->hostInstances.size()) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_update_instances: %u instances given, scene has %zu", numInstances, s->hostInstances.size());
    int rc = check_refit_args(s, instances, numInstances, lights, numLights, "rtr_scene_update_instances");
    if (rc != RTR_OK) return rc;
    rc = refresh_mirrors(s);
    if (rc != RTR_OK) return rc;
    if (scene_is_empty(s)) return RTR_OK;     /* nothing to refit */
    HIP_TRY(hipSetDevice(s->ctx->device));
    rc = ensure_refit_ready(s);
    if (rc != RTR_OK) return rc;
    /* frames of OTHER contexts (other streams) may be rendering this scene: everything enqueued on the device so far is joined
     * before the nodes, records and light tables are rewritten (contract in rtr.h) */
    HIP_TRY(hipDeviceSynchronize());
    return refit_scene(s, instances, lights, false);
}

/* The checks of the ranges that the synchronous and the enqueued vertex update share, with the same messages (`who` names the caller):
 * strides, ranges inside the vertex array, null positions, device-pointer alignment, overlaps. */
static int check_vertex_ranges(const rtr_scene* s, const rtr_vertex_range* ranges, uint32_t numRanges, uint32_t positionStride, uint32_t normalStride,
                               bool device, const char* who) {
    if ((positionStride & 3u) || positionStride < 12u) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: positionStride %u must be a multiple of 4 and at least 12", who, positionStride);
    bool anyNormals = false;
    for (uint32_t r = 0; r < numRanges; ++r) {
        const rtr_vertex_range& vr = ranges[r];
        if ((uint64_t)vr.firstVertex + vr.numVertices > s->numVertices)
            return fail(RTR_ERR_INVALID_ARGUMENT, "%s: range %u (vertices %u .. %llu) leaves the scene's %u vertices", who, r, vr.firstVertex,
                        (unsigned long long)vr.firstVertex + vr.numVertices, s->numVertices);
        if (vr.numVertices && !vr.positions) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: range %u has %u vertices and null positions", who, r, vr.numVertices);
        if (device && ((((uintptr_t)vr.positions) | ((uintptr_t)vr.normals)) & 3u))
            return fail(RTR_ERR_INVALID_ARGUMENT, "%s: range %u: device pointers must be 4-byte aligned", who, r);
        anyNormals = anyNormals || (vr.normals && vr.numVertices);
    }
    if (anyNormals && ((normalStride & 3u) || normalStride < 12u)) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: normalStride %u must be a multiple of 4 and at least 12", who, normalStride);
    {   /* no two ranges may name a vertex twice: the result would depend on the order the lanes run in */
        std::vector<uint32_t> order;
        for (uint32_t r = 0; r < numRanges; ++r) if (ranges[r].numVertices) order.push_back(r);
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return ranges[a].firstVertex < ranges[b].firstVertex; });
        for (size_t k = 1; k < order.size(); ++k) {
            const rtr_vertex_range& a = ranges[order[k - 1]]; const rtr_vertex_range& b = ranges[order[k]];
            if ((uint64_t)a.firstVertex + a.numVertices > b.firstVertex)
                return fail(RTR_ERR_INVALID_ARGUMENT, "%s: ranges %u and %u overlap (vertex %u)", who, order[k - 1], order[k], b.firstVertex);
        }
    }
    return RTR_OK;
}

int rtr_scene_update_vertices(rtr_scene* s, const rtr_vertex_range* ranges, uint32_t numRanges, uint32_t positionStride, uint32_t normalStride, uint32_t flags,
                              const RtrInstance* instances, uint32_t numInstances, const RtrAreaLightInfo* lights, uint32_t numLights) {
    static const char* who = "rtr_scene_update_vertices";
    static_assert(sizeof(rtr_vertex_range) == 24, "layout");
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null scene", who);
    if (!ranges || numRanges == 0) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null ranges (or numRanges == 0): nothing to update", who);
    if (flags > RTR_VERTICES_DEVICE) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: unknown flag bits 0x%x", who, flags & ~RTR_VERTICES_DEVICE);
    const bool device = flags == RTR_VERTICES_DEVICE;
    int rc = check_vertex_ranges(s, ranges, numRanges, positionStride, normalStride, device, who);
    if (rc != RTR_OK) return rc;
    rc = check_refit_args(s, instances, numInstances, lights, numLights, who);
    if (rc != RTR_OK) return rc;
    rc = refresh_mirrors(s);
    if (rc != RTR_OK) return rc;
    if (scene_is_empty(s)) return RTR_OK;     /* nothing to refit */

    /* the device tables of the launches: the ranges in chunks of kVertexRangesPerLaunch, each with its own prefix counts */
    const uint32_t kChunk = rtrdev::kVertexRangesPerLaunch;
    const uint32_t numChunks = (numRanges + kChunk - 1) / kChunk;
    std::vector<rtrdev::VertexRange> table(numRanges);
    std::vector<uint32_t> prefix((size_t)numRanges + numChunks), chunkBase(numChunks + 1, 0u);
    for (uint32_t c = 0; c < numChunks; ++c) {
        uint32_t acc = 0;
        const uint32_t r0 = c * kChunk, r1 = std::min(numRanges, r0 + kChunk);
        for (uint32_t r = r0; r < r1; ++r) { prefix[(size_t)r + c] = acc; acc += ranges[r].numVertices; }      /* non-overlapping ranges inside a 32-bit array: no wrap */
        prefix[(size_t)r1 + c] = acc;
        chunkBase[c + 1] = chunkBase[c] + acc;
    }
    auto name_bad = [&](uint64_t concat, uint32_t* range, uint32_t* vertex) {      /* concatenated index -> (range, vertex in it) */
        uint32_t r = 0; uint64_t before = 0;
        while (before + ranges[r].numVertices <= concat) before += ranges[r++].numVertices;
        *range = r; *vertex = (uint32_t)(concat - before);
    };

    HIP_TRY(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    const uint32_t posWords = device ? positionStride / 4u : 3u, nrmWords = device ? normalStride / 4u : 3u;
    if (!device) {
        /* host data: checked here, then packed (three words per vertex: all positions, then the normals of the ranges that bring them)
         * and staged in a device buffer of the scene, from where it takes the path of device data */
        size_t words = 0;
        for (uint32_t r = 0; r < numRanges; ++r) words += (size_t)ranges[r].numVertices * (ranges[r].normals ? 6u : 3u);
        s->vtxHost.resize(words);
        size_t at = 0;
        for (uint32_t r = 0; r < numRanges; ++r) {
            const char* src = static_cast<const char*>(ranges[r].positions);
            for (uint32_t v = 0; v < ranges[r].numVertices; ++v, at += 3) {
                float p[3];
                memcpy(p, src + (size_t)v * positionStride, sizeof p);
                for (int k = 0; k < 3; ++k)
                    if (!(p[k] > -3.0e38f && p[k] < 3.0e38f))
                        return fail(RTR_ERR_INVALID_ARGUMENT, "%s: range %u, vertex %u (scene vertex %u): non-finite position", who, r, v, ranges[r].firstVertex + v);
                memcpy(&s->vtxHost[at], p, sizeof p);
            }
        }
        HIP_TRY(s->vtxStage.grow(words));
        size_t pos = 0;
        for (uint32_t r = 0; r < numRanges; ++r) {
            table[r] = rtrdev::VertexRange{s->vtxStage.p + pos, nullptr, ranges[r].firstVertex, 0u};
            pos += (size_t)ranges[r].numVertices * 3u;
        }
        for (uint32_t r = 0; r < numRanges; ++r) {
            if (!ranges[r].normals || !ranges[r].numVertices) continue;
            const char* src = static_cast<const char*>(ranges[r].normals);
            table[r].normals = s->vtxStage.p + at;
            for (uint32_t v = 0; v < ranges[r].numVertices; ++v, at += 3) memcpy(&s->vtxHost[at], src + (size_t)v * normalStride, 12);
        }
    } else {
        for (uint32_t r = 0; r < numRanges; ++r)
            table[r] = rtrdev::VertexRange{static_cast<const uint32_t*>(ranges[r].positions), ranges[r].numVertices ? static_cast<const uint32_t*>(ranges[r].normals) : nullptr,
                                           ranges[r].firstVertex, 0u};
    }
    /* renders and queries of other streams read the vertices, and with RTR_VERTICES_DEVICE the caller's data may still be in the
     * making on one of them: everything enqueued on the device so far is joined (contract in rtr.h) */
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(s->vtxRanges.grow(table.size()));
    HIP_TRY(s->vtxPrefix.grow(prefix.size() + 1));        /* the last word: first bad vertex */
    uint32_t* firstBad = s->vtxPrefix.p + prefix.size();
    const uint32_t none = 0xffffffffu;
    HIP_TRY(hipMemcpyAsync(s->vtxRanges.p, table.data(), table.size() * sizeof(rtrdev::VertexRange), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s->vtxPrefix.p, prefix.data(), prefix.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(firstBad, &none, sizeof none, hipMemcpyHostToDevice, st));
    if (!device && !s->vtxHost.empty()) HIP_TRY(hipMemcpyAsync(s->vtxStage.p, s->vtxHost.data(), s->vtxHost.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    for (uint32_t c = 0; c < numChunks; ++c) {
        const uint32_t r0 = c * kChunk, n = std::min(numRanges, r0 + kChunk) - r0;
        const hipError_t e = rtrdev::launch_check_vertices(s->vtxRanges.p + r0, s->vtxPrefix.p + r0 + c, n, chunkBase[c + 1] - chunkBase[c], posWords, chunkBase[c], firstBad, st);
        if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: checking kernel: %s", who, hipGetErrorString(e));
    }
    uint32_t bad = none;
    HIP_TRY(hipMemcpyAsync(&bad, firstBad, sizeof bad, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (bad != none) {
        uint32_t r = 0, v = 0;
        name_bad(bad, &r, &v);
        return fail(RTR_ERR_INVALID_ARGUMENT, "%s: range %u, vertex %u (scene vertex %u): non-finite position", who, r, v, ranges[r].firstVertex + v);
    }
    /* nothing of the scene has been touched up to here */
    rc = ensure_refit_ready(s);
    if (rc != RTR_OK) return rc;
    for (uint32_t c = 0; c < numChunks; ++c) {
        const uint32_t r0 = c * kChunk, n = std::min(numRanges, r0 + kChunk) - r0;
        const hipError_t e = rtrdev::launch_write_vertices(s->vtxRanges.p + r0, s->vtxPrefix.p + r0 + c, n, chunkBase[c + 1] - chunkBase[c], posWords, nrmWords, s->vertices.p, st);
        if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: writing kernel: %s", who, hipGetErrorString(e));
    }
    return refit_scene(s, instances, lights, true);
}

int rtr_scene_export_vertices(const rtr_scene* s, RtrVertex* out, size_t bytes) {
    if (!s || (!out && bytes)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_export_vertices: null argument");
    if (bytes != (size_t)s->numVertices * sizeof(RtrVertex)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_export_vertices: bytes %zu != %zu", bytes, (size_t)s->numVertices * sizeof(RtrVertex));
    if (!bytes) return RTR_OK;
    HIP_TRY(hipSetDevice(s->ctx->device));
    HIP_TRY(hipMemcpy(out, s->vertices.p, bytes, hipMemcpyDeviceToHost));
    return RTR_OK;
}

/* ---- the enqueued vertex update (contract in rtr.h) ---- */
int rtr_scene_prepare_async_updates(rtr_scene* s) {
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_prepare_async_updates: null scene");
    HIP_TRY(hipSetDevice(s->ctx->device));
    int rc = refresh_mirrors(s);
    if (rc != RTR_OK) return rc;
    if (s->tree.asyncReady) return RTR_OK;
    if (!scene_is_empty(s)) {
        rc = ensure_refit_ready(s);
        if (rc != RTR_OK) return rc;
        rc = upload_prim_tables(s, s->hostInstances.data());
        if (rc != RTR_OK) return rc;
        HIP_TRY(s->tree.orderScratch.ensure(2 * s->tree.hostNodes.size()));
        if (!s->instCustom.p) {      /* kept through a rebuild: the instances are the scene's, not the tree's */
            std::vector<uint32_t> custom(s->hostInstances.size());
            for (size_t i = 0; i < custom.size(); ++i) custom[i] = s->hostInstances[i].customIndex;
            HIP_TRY(s->instCustom.upload(custom.data(), custom.size(), s->ctx->stream));
        }
    }
    if (!s->asyncWords.p) {      /* kept through a rebuild: the status is the scene's, not the tree's */
        const uint32_t none = 0xffffffffu, init[8] = {none, 0u, 0u, 0u, 0u, none, none, 0u};
        HIP_TRY(s->asyncWords.upload(init, 8, s->ctx->stream));
    }
    s->tree.asyncReady = true;
    return RTR_OK;
}

/* What both enqueued updates end in, on the tables and vertices as they are when the stream gets there: the refit, the 4-wide view, its
 * breadth-first order made on the device, the permutation, the light triangles (always remade), and the fold of the update's word
 * (asyncWords[0]) into the sticky status under this call's serial.  Counts the update as enqueued. */
static int enqueue_refit_tail(rtr_scene* s, uint32_t serial, const char* who) {
    hipStream_t st = s->ctx->stream;
    uint32_t* firstBad = s->asyncWords.p;
    SceneTree& t = s->tree;
    const uint32_t n = (uint32_t)t.hostNodes.size();
    rtrdev::BvhInputs in{t.prims.p, t.instRefs.p, s->vertices.p, s->indices.p};
    hipError_t e = rtrdev::bvh_refit_enqueued(in, t.numPrims, t.numNodeSlots, device_arrays(t), st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: device BVH refit: %s", who, hipGetErrorString(e));
    s->mirrorsStale = true;
    e = rtrdev::bvh_make_wide(t.nodes.p, n, t.parent.p, t.grid.p, t.hostWideShape.size() == n ? t.wideShape.p : nullptr, t.nodes4tmp.p, t.wideSums.p, st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: 4-wide node build: %s", who, hipGetErrorString(e));
    e = rtrdev::bvh_wide_order(t.nodes4tmp.p, n, t.wideRemap.p, t.orderScratch.p, s->asyncWords.p + 1, st);
    if (e == hipSuccess) e = rtrdev::bvh_hot_top(t.nodes4tmp.p, n, t.wideRemap.p, t.wideRemap.p + n, t.grid.p, s->lights.p, s->numLights, rtrdev::trace_top_capacity(), st);
    if (e == hipSuccess) e = rtrdev::bvh_permute_wide(t.nodes4tmp.p, n, t.wideRemap.p, t.nodes4.p, st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: 4-wide node order: %s", who, hipGetErrorString(e));
    if (s->numLights) {
        e = rtrdev::launch_light_tris(s->lights.p, s->vertices.p, s->indices.p, s->lightTriFirst.p, s->numLights, s->lightTris.p, st);
        if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: light-triangle records: %s", who, hipGetErrorString(e));
        /* a power table follows its records; a refused update rebuilds the same table from unchanged data */
        if (const int rc = enqueue_light_power(s, st, who)) return rc;
    }
    e = rtrdev::launch_fold_update_status(firstBad, s->asyncWords.p + 4, serial, st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: status kernel: %s", who, hipGetErrorString(e));
    ++s->asyncEnqueued;
    return RTR_OK;
}

int rtr_scene_update_vertices_async(rtr_scene* s, const rtr_vertex_range* ranges, uint32_t numRanges, uint32_t positionStride, uint32_t normalStride) {
    static const char* who = "rtr_scene_update_vertices_async";
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null scene", who);
    if (!ranges || numRanges == 0) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null ranges (or numRanges == 0): nothing to update", who);
    int rc = check_vertex_ranges(s, ranges, numRanges, positionStride, normalStride, true, who);
    if (rc != RTR_OK) return rc;
    if (!s->tree.asyncReady) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: the scene has not been prepared: call rtr_scene_prepare_async_updates once first", who);
    const uint32_t serial = (uint32_t)(s->asyncEnqueued + 1);
    if (scene_is_empty(s)) { ++s->asyncEnqueued; return RTR_OK; }      /* nothing to refit, as the synchronous call */
    HIP_TRY(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    uint32_t* firstBad = s->asyncWords.p;
    HIP_TRY(hipMemsetAsync(firstBad, 0xff, sizeof(uint32_t), st));
    const uint32_t posWords = positionStride / 4u, nrmWords = normalStride / 4u;
    const uint32_t kChunk = rtrdev::kVertexRangesPerArgs;
    /* the ranges reach the kernels as kernel arguments, a chunk per launch: first every check, then every (predicated) write */
    for (int pass = 0; pass < 2; ++pass)
        for (uint32_t r0 = 0; r0 < numRanges; r0 += kChunk) {
            rtrdev::VertexRangeArgs t;
            t.numRanges = std::min(numRanges - r0, kChunk);
            uint32_t acc = 0;
            for (uint32_t k = 0; k < t.numRanges; ++k) {
                const rtr_vertex_range& vr = ranges[r0 + k];
                t.ranges[k] = rtrdev::VertexRange{static_cast<const uint32_t*>(vr.positions), vr.numVertices ? static_cast<const uint32_t*>(vr.normals) : nullptr, vr.firstVertex, 0u};
                t.prefix[k] = acc; acc += vr.numVertices;
            }
            t.prefix[t.numRanges] = acc;
            const hipError_t e = pass == 0 ? rtrdev::launch_check_vertices_args(t, posWords, firstBad, st)
                                           : rtrdev::launch_write_vertices_args(t, posWords, nrmWords, s->vertices.p, firstBad, st);
            if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: %s kernel: %s", who, pass == 0 ? "checking" : "writing", hipGetErrorString(e));
        }
    return enqueue_refit_tail(s, serial, who);
}

int rtr_scene_update_instances_async(rtr_scene* s, const void* transforms, uint32_t transformStride, uint32_t firstInstance, uint32_t numInstances,
                                     const RtrAreaLightInfo* lights, uint32_t numLights) {
    static const char* who = "rtr_scene_update_instances_async";
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null scene", who);
    if (!transforms && !lights) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null transforms and null lights: nothing to update", who);
    if (!transforms && numInstances) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null transforms with numInstances %u", who, numInstances);
    if (transforms && !numInstances) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: transforms given with numInstances 0", who);
    if (transforms && ((transformStride & 3u) || transformStride < 48u))
        return fail(RTR_ERR_INVALID_ARGUMENT, "%s: transformStride %u must be a multiple of 4 and at least 48", who, transformStride);
    if ((((uintptr_t)transforms) | ((uintptr_t)lights)) & 3u) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: device pointers must be 4-byte aligned", who);
    /* nothing of the scene has been read up to here */
    if ((uint64_t)firstInstance + numInstances > s->hostInstances.size())
        return fail(RTR_ERR_INVALID_ARGUMENT, "%s: instances %u .. %llu leave the scene's %zu instances", who, firstInstance,
                    (unsigned long long)firstInstance + numInstances, s->hostInstances.size());
    if (lights && numLights != s->numLights) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: %u lights given, scene has %u", who, numLights, s->numLights);
    if (!s->tree.asyncReady) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: the scene has not been prepared: call rtr_scene_prepare_async_updates once first", who);
    const uint32_t serial = (uint32_t)(s->asyncEnqueued + 1);
    if (scene_is_empty(s)) { ++s->asyncEnqueued; return RTR_OK; }      /* nothing to refit, as the synchronous call */
    HIP_TRY(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    uint32_t* firstBad = s->asyncWords.p;
    HIP_TRY(hipMemsetAsync(firstBad, 0xff, sizeof(uint32_t), st));
    const uint32_t strideWords = transforms ? transformStride / 4u : 12u, sceneInstances = (uint32_t)s->hostInstances.size();
    hipError_t e = rtrdev::launch_check_instances(transforms, strideWords, firstInstance, numInstances, lights, numLights, sceneInstances, s->lights.p, firstBad, st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: checking kernel: %s", who, hipGetErrorString(e));
    e = rtrdev::launch_write_instances(transforms, strideWords, firstInstance, numInstances, lights, numLights, s->instCustom.p, rtrdev::kMirroredWord,
                                       s->xforms.p, s->nmats.p, s->tree.instRefs.p, s->lights.p, firstBad, st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: writing kernel: %s", who, hipGetErrorString(e));
    s->instancesStale = true;      /* with mirrorsStale, which the tail sets: refresh_mirrors reads the transforms and lights back */
    s->mirrorsStale = true;
    return enqueue_refit_tail(s, serial, who);
}

int rtr_scene_export_instances(const rtr_scene* s, RtrInstance* out, size_t bytes) {
    if (!s || (!out && bytes)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_export_instances: null argument");
    if (bytes != s->hostInstances.size() * sizeof(RtrInstance))
        return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_export_instances: bytes %zu != %zu", bytes, s->hostInstances.size() * sizeof(RtrInstance));
    { const int rcm = refresh_mirrors(s); if (rcm != RTR_OK) return rcm; }
    if (bytes) memcpy(out, s->hostInstances.data(), bytes);
    return RTR_OK;
}

int rtr_scene_update_status(rtr_scene* s, rtr_update_status* out) {
    static_assert(sizeof(rtr_update_status) == 32, "layout");
    if (!s || !out) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_update_status: null argument");
    memset(out, 0, sizeof *out);
    out->enqueued = s->asyncEnqueued;
    out->firstRefusedUpdate = out->firstBadVertex = 0xffffffffu;
    if (!s->asyncWords.p) return RTR_OK;      /* never prepared: nothing was enqueued */
    HIP_TRY(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    uint32_t w[3];
    HIP_TRY(hipMemcpyAsync(w, s->asyncWords.p + 4, sizeof w, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    out->refused = w[0]; out->firstRefusedUpdate = w[1]; out->firstBadVertex = w[2];
    if (w[1] != 0xffffffffu) HIP_TRY(hipMemsetAsync(s->asyncWords.p + 5, 0xff, 2 * sizeof(uint32_t), st));      /* "first since the last status call" starts again */
    return RTR_OK;
}

/* ---- the enqueued rebuild (contract in rtr.h) ---- */
int rtr_scene_prepare_async_rebuild(rtr_scene* s) {
    static const char* who = "rtr_scene_prepare_async_rebuild";
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null scene", who);
    HIP_TRY(hipSetDevice(s->ctx->device));
    int rc = refresh_mirrors(s);
    if (rc != RTR_OK) return rc;
    SceneTree& t = s->tree;
    if (t.rebuildReady) return RTR_OK;
    if (scene_is_empty(s)) {
        rc = rtr_scene_prepare_async_updates(s);
        if (rc == RTR_OK) t.rebuildReady = true;
        return rc;
    }
    /* the commit copies a device build over the live arrays IN PLACE: they must have a device build's sizes already */
    const size_t n = t.hostTris.size();
    if (n < 16 || t.hostNodes.size() != n - 1 || !t.hostWideShape.empty())
        return fail(RTR_ERR_INVALID_ARGUMENT, "%s: the scene's tree (%zu triangles, %zu node slots%s) was not made by the device builder, whose arrays an enqueued "
                    "rebuild commits into: call rtr_scene_rebuild(scene, RTR_BUILD_DEVICE_LBVH) first%s", who, n, t.hostNodes.size(),
                    t.hostWideShape.empty() ? "" : ", a cost-driven 4-wide shape", n < 16 ? " (a scene of fewer than 16 triangles always takes the host builder: it has no enqueued rebuild)" : "");
    rc = rtr_scene_prepare_async_updates(s);
    if (rc != RTR_OK) return rc;
    const size_t numNodes = n - 1;
    if (!t.refitReady || t.numPrims != n || t.numNodeSlots != numNodes || t.nodes.n < numNodes * 2 || t.nodesF.n < numNodes * 4 || t.tris.n < n * 3 || t.boxMin.n < n ||
        t.boxMax.n < n || t.parent.n < numNodes || t.counters.n < numNodes || t.depth.n < numNodes || t.slotOfPrim.n < n || t.red.n < 8)
        return fail(RTR_ERR_INVALID_ARGUMENT, "%s: the live arrays do not have a device build's sizes: call rtr_scene_rebuild(scene, RTR_BUILD_DEVICE_LBVH) first", who);
    TreeStage& g = s->stage;
    HIP_TRY(g.nodes.ensure(numNodes * 2)); HIP_TRY(g.nodesF.ensure(numNodes * 4)); HIP_TRY(g.grid.ensure(1)); HIP_TRY(g.tris.ensure(n * 3));
    HIP_TRY(g.boxMin.ensure(n)); HIP_TRY(g.boxMax.ensure(n)); HIP_TRY(g.parent.ensure(numNodes)); HIP_TRY(g.slotOfPrim.ensure(n)); HIP_TRY(g.red.ensure(8));
    rc = ensure_build_scratch(s->buildScratch, (uint32_t)n);
    if (rc != RTR_OK) return rc;
    t.rebuildReady = true;
    return RTR_OK;
}

/* The chain of an enqueued rebuild, counted as enqueued under `serial`.  go: null — rtr_scene_rebuild_async, every launch as it always
 * was — or the policy's decision word (rtr_scene_rebuild_if_async): the build's kernels, the commit and the tail do nothing when it is 0.
 * On a scene prepared for the policy the chain closes with the baseline: the cost of the live tree again, predicated on this chain's own
 * commit, and the one lane that takes it as builtSah. */
static int enqueue_rebuild_chain(rtr_scene* s, uint32_t serial, const char* who, const uint32_t* go) {
    hipStream_t st = s->ctx->stream;
    SceneTree& t = s->tree;
    TreeStage& g = s->stage;
    uint32_t* word = s->asyncWords.p;
    rtrdev::RebuildIfRecord* rec = t.rebuildIfReady ? policy_record(s) : nullptr;
    uint32_t* committed = rec ? &rec->committed : nullptr;
    HIP_TRY(hipMemsetAsync(word, 0xff, sizeof(uint32_t), st));
    /* the build, into the stage, from the LIVE tables (current after enqueued instance updates and mask changes) and the scene's vertices */
    const uint32_t n = t.numPrims, numNodes = t.numNodeSlots;
    rtrdev::BvhDeviceArrays a{};
    a.nodes = g.nodes.p; a.nodesF = g.nodesF.p; a.grid = g.grid.p; a.tris = g.tris.p; a.boxMin = g.boxMin.p; a.boxMax = g.boxMax.p; a.parent = g.parent.p;
    a.counters = t.counters.p; a.depth = t.depth.p; a.slotOfPrim = g.slotOfPrim.p; a.red = g.red.p;
    rtrdev::BvhInputs in{t.prims.p, t.instRefs.p, s->vertices.p, s->indices.p};
    hipError_t e = rtrdev::bvh_build_lbvh_enqueued(in, n, a, scratch_view(s->buildScratch), st, go);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: device BVH build: %s", who, hipGetErrorString(e));
    /* the commit: all staged arrays over their live twins, unless the stack class would have to rise */
    rtrdev::CommitTable ct{};
    auto add = [&](const void* src, void* dst, size_t bytes) { ct.a[ct.count].src = src; ct.a[ct.count].dst = dst; ct.a[ct.count].bytes = bytes; ++ct.count; };
    add(g.nodesF.p, t.nodesF.p, (size_t)numNodes * 64); add(g.tris.p, t.tris.p, (size_t)n * 48); add(g.nodes.p, t.nodes.p, (size_t)numNodes * 32);
    add(g.boxMin.p, t.boxMin.p, (size_t)n * 16); add(g.boxMax.p, t.boxMax.p, (size_t)n * 16); add(g.parent.p, t.parent.p, (size_t)numNodes * 4);
    add(g.slotOfPrim.p, t.slotOfPrim.p, (size_t)n * 4); add(g.grid.p, t.grid.p, sizeof(RtrBvhGrid)); add(g.red.p, t.red.p, 8 * sizeof(uint32_t));
    e = rtrdev::bvh_commit_tree(ct, g.red.p, t.stats.stackEntries, word, st, go, committed);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: commit kernel: %s", who, hipGetErrorString(e));
    s->mirrorsStale = true; s->depthStale = true;
    /* the 4-wide view of whatever tree is live now (after a refused commit: the unchanged one, whose bytes these launches reproduce) */
    e = rtrdev::bvh_make_wide(t.nodes.p, numNodes, t.parent.p, t.grid.p, nullptr, t.nodes4tmp.p, t.wideSums.p, st, go);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: 4-wide node build: %s", who, hipGetErrorString(e));
    e = rtrdev::bvh_wide_order(t.nodes4tmp.p, numNodes, t.wideRemap.p, t.orderScratch.p, s->asyncWords.p + 1, st, go);
    if (e == hipSuccess) e = rtrdev::bvh_hot_top(t.nodes4tmp.p, numNodes, t.wideRemap.p, t.wideRemap.p + numNodes, t.grid.p, s->lights.p, s->numLights, rtrdev::trace_top_capacity(), st, go);
    if (e == hipSuccess) e = rtrdev::bvh_permute_wide(t.nodes4tmp.p, numNodes, t.wideRemap.p, t.nodes4.p, st, go);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: 4-wide node order: %s", who, hipGetErrorString(e));
    if (t.leafReady) {      /* the leaf order changed: the table is made again where it is (4 B per triangle, nothing to allocate) */
        /* gated, the clearing is a kernel: a skip must not clear the table without the launch that fills it again */
        if (go) e = rtrdev::bvh_clear_words(reinterpret_cast<uint32_t*>(t.leafTable.p), t.leafTable.n, st, go);
        else HIP_TRY(hipMemsetAsync(t.leafTable.p, 0, t.leafTable.n * sizeof(int32_t), st));
        if (e == hipSuccess)
            e = rtrdev::launch_leaf_table(t.nodes.p, (uint32_t)(t.nodes.n / 2), t.tris.p, (uint32_t)(t.tris.n / 3), s->triCount.p, s->leafBase.p, s->numInstances, t.leafTable.p, st, go);
        if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: leaf table: %s", who, hipGetErrorString(e));
    }
    if (rec) {      /* the baseline follows the build: sums of the new live tree and builtSah from them, when this chain's commit copied */
        e = rtrdev::bvh_tree_cost(t.nodes.p, numNodes, t.parent.p, s->policy.p, st, committed);
        if (e == hipSuccess) e = rtrdev::bvh_rebuild_if_close(s->policy.p, t.grid.p, rec, go ? 1u : 0u, st);
        if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: baseline kernels: %s", who, hipGetErrorString(e));
    }
    e = rtrdev::launch_fold_update_status(word, s->asyncWords.p + 4, serial, st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: status kernel: %s", who, hipGetErrorString(e));
    ++s->asyncEnqueued;
    return RTR_OK;
}

int rtr_scene_rebuild_async(rtr_scene* s, uint32_t buildFlags) {
    static const char* who = "rtr_scene_rebuild_async";
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null scene", who);
    if (buildFlags == RTR_BUILD_HOST_SAH) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: buildFlags RTR_BUILD_HOST_SAH: the host builder is host code and cannot be enqueued; only RTR_BUILD_DEVICE_LBVH can", who);
    if (buildFlags != RTR_BUILD_DEVICE_LBVH) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: unknown buildFlags %u", who, buildFlags);
    /* nothing of the scene has been read up to here */
    if (!s->tree.rebuildReady)
        return fail(RTR_ERR_INVALID_ARGUMENT, "%s: the scene is not prepared for an enqueued rebuild: call rtr_scene_prepare_async_rebuild first (once per scene, and again after a host rebuild)", who);
    const uint32_t serial = (uint32_t)(s->asyncEnqueued + 1);
    if (scene_is_empty(s)) { ++s->asyncEnqueued; return RTR_OK; }      /* nothing to build, as the synchronous call */
    HIP_TRY(hipSetDevice(s->ctx->device));
    return enqueue_rebuild_chain(s, serial, who, nullptr);
}

/* ---- the rebuild policy on the device (contract in rtr.h) ---- */
/* sets the baseline to the cost of the tree as it is now; the counts of a scene that was prepared before go on */
static int prepare_rebuild_if(rtr_scene* s, const char* who) {
    int rc = rtr_scene_prepare_async_rebuild(s);
    if (rc != RTR_OK) return rc;
    SceneTree& t = s->tree;
    if (t.rebuildIfReady) return RTR_OK;
    if (scene_is_empty(s)) { t.rebuildIfReady = true; return RTR_OK; }
    if (rtrdev::bvh_tree_cost_words() + 1 != kPolicyRecordAt) return fail(RTR_ERR_HIP, "%s: the cost kernel has %zu words, the policy expects 11", who, rtrdev::bvh_tree_cost_words());
    rtr_tree_cost c{};
    rc = rtr_scene_tree_cost(s, &c);      /* joins the scene's stream */
    if (rc != RTR_OK) return rc;
    hipStream_t st = s->ctx->stream;
    if (!s->policy.p) {
        HIP_TRY(s->policy.alloc(kPolicyWords));
        HIP_TRY(hipMemsetAsync(s->policy.p, 0, kPolicyWords * sizeof(unsigned long long), st));
        rtrdev::RebuildIfRecord r{};
        r.builtSah = c.sah; r.lastDecision = 0xffffffffu;
        HIP_TRY(hipMemcpyAsync(policy_record(s), &r, sizeof r, hipMemcpyHostToDevice, st));
    } else
        HIP_TRY(hipMemcpyAsync(&policy_record(s)->builtSah, &c.sah, sizeof c.sah, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));      /* the copies read this frame's variables */
    t.rebuildIfReady = true;
    return RTR_OK;
}

int rtr_scene_prepare_async_rebuild_if(rtr_scene* s) {
    static const char* who = "rtr_scene_prepare_async_rebuild_if";
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null scene", who);
    return prepare_rebuild_if(s, who);
}

int rtr_scene_rebuild_if_async(rtr_scene* s, uint32_t buildFlags, double rebuildAbove) {
    static const char* who = "rtr_scene_rebuild_if_async";
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null scene", who);
    if (buildFlags == RTR_BUILD_HOST_SAH) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: buildFlags RTR_BUILD_HOST_SAH: the host builder is host code and cannot be enqueued; only RTR_BUILD_DEVICE_LBVH can", who);
    if (buildFlags != RTR_BUILD_DEVICE_LBVH) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: unknown buildFlags %u", who, buildFlags);
    if (!(rebuildAbove >= 0.0)) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: rebuildAbove %g must be a number >= 0 (+inf: never rebuild)", who, rebuildAbove);
    /* nothing of the scene has been read up to here */
    if (!s->tree.rebuildIfReady)
        return fail(RTR_ERR_INVALID_ARGUMENT, "%s: the scene is not prepared for the rebuild policy: call rtr_scene_prepare_async_rebuild_if first (once per scene, and again after a host rebuild)", who);
    const uint32_t serial = (uint32_t)(s->asyncEnqueued + 1);
    if (scene_is_empty(s)) { ++s->asyncEnqueued; return RTR_OK; }      /* nothing to look at */
    HIP_TRY(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    SceneTree& t = s->tree;
    rtrdev::RebuildIfRecord* rec = policy_record(s);
    /* the cost of the live tree and the decision, both on the device */
    hipError_t e = rtrdev::bvh_tree_cost(t.nodes.p, t.numNodeSlots, t.parent.p, s->policy.p, st);
    if (e == hipSuccess) e = rtrdev::bvh_rebuild_if_decide(s->policy.p, t.grid.p, rec, rebuildAbove, st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: cost and decision kernels: %s", who, hipGetErrorString(e));
    return enqueue_rebuild_chain(s, serial, who, &rec->go);
}

int rtr_scene_rebuild_if_status(rtr_scene* s, rtr_rebuild_if_status* out) {
    static const char* who = "rtr_scene_rebuild_if_status";
    static_assert(sizeof(rtr_rebuild_if_status) == sizeof(rtrdev::RebuildIfRecord), "layout");
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null scene", who);
    if (!out) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null out", who);
    memset(out, 0, sizeof *out);
    out->lastDecision = 0xffffffffu;
    if (!s->policy.p) return RTR_OK;      /* never prepared (or empty): nothing was evaluated */
    HIP_TRY(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    rtrdev::RebuildIfRecord r{};
    HIP_TRY(hipMemcpyAsync(&r, policy_record(s), sizeof r, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    out->evaluated = r.evaluated; out->rebuilt = r.rebuilt; out->builtSah = r.builtSah; out->lastSah = r.lastSah; out->lastDecision = r.lastDecision;
    return RTR_OK;
}

/* ---- the cost of the tree, and the rebuild (contracts in rtr.h) ---- */
/* the integer sums are complete: sah from them in double, in the order rtr.h states (-ffp-contract=off: no fused step) */
static void finish_tree_cost(rtr_tree_cost* c, const RtrBvhGrid& grid) {
    uint64_t w[11];
    for (int k = 0; k < 3; ++k) { w[k] = c->innerArea[k]; w[3 + k] = c->leafArea[k]; w[6 + k] = c->rootArea[k]; }
    w[9] = c->numInner; w[10] = c->numLeafRefs;
    c->sah = rtr_tree_sah(w, grid.scale[0], grid.scale[1], grid.scale[2]);      /* the device's function too (kernels/rtr_tree_sah.h) */
}

int rtr_host_tree_cost(const RtrBvhNode* nodes, size_t nodeBytes, const RtrBvhGrid* grid, rtr_tree_cost* out) {
    if (!nodes || !grid || !out) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_host_tree_cost: null argument");
    if (nodeBytes == 0 || nodeBytes % sizeof(RtrBvhNode)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_host_tree_cost: nodeBytes %zu is not a positive multiple of %zu", nodeBytes, sizeof(RtrBvhNode));
    const size_t n = nodeBytes / sizeof(RtrBvhNode);
    rtr_tree_cost c{};
    auto triple = [](const uint32_t lo[3], const uint32_t hi[3], uint64_t t[3]) {
        uint64_t d[3];
        for (int k = 0; k < 3; ++k) d[k] = hi[k] > lo[k] ? (uint64_t)(hi[k] - lo[k]) : 0u;
        t[0] = d[0] * d[1]; t[1] = d[1] * d[2]; t[2] = d[2] * d[0];
    };
    /* the walk from the root: every node it reaches is counted once, whichever slots name it */
    std::vector<uint8_t> seen(n, 0);
    std::vector<uint32_t> stack{0};
    seen[0] = 1;
    while (!stack.empty()) {
        const uint32_t i = stack.back(); stack.pop_back();
        const RtrBvhNode& nd = nodes[i];
        uint32_t lo[2][3], hi[2][3];
        uint64_t t[3];
        for (int sd = 0; sd < 2; ++sd) {
            for (int a = 0; a < 3; ++a) { lo[sd][a] = nd.q[RTR_BVH_QSLOT(sd, 0, a)]; hi[sd][a] = nd.q[RTR_BVH_QSLOT(sd, 1, a)]; }
            triple(lo[sd], hi[sd], t);
            const int32_t code = nd.child[sd];
            if (code >= 0) {
                if ((size_t)code >= n) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_host_tree_cost: node %u names child %d, the array has %zu nodes", i, code, n);
                for (int k = 0; k < 3; ++k) c.innerArea[k] += t[k];
                ++c.numInner;
                if (!seen[(size_t)code]) { seen[(size_t)code] = 1; stack.push_back((uint32_t)code); }
            } else {
                const uint64_t cnt = ((uint32_t)~code & 7u) + 1u;
                for (int k = 0; k < 3; ++k) c.leafArea[k] += cnt * t[k];
                ++c.numLeafRefs;
            }
        }
        if (i == 0) {
            uint32_t rlo[3], rhi[3];
            for (int a = 0; a < 3; ++a) { rlo[a] = std::min(lo[0][a], lo[1][a]); rhi[a] = std::max(hi[0][a], hi[1][a]); }
            triple(rlo, rhi, t);
            for (int k = 0; k < 3; ++k) { c.innerArea[k] += t[k]; c.rootArea[k] = t[k]; }
            ++c.numInner;
        }
    }
    finish_tree_cost(&c, *grid);
    *out = c;
    return RTR_OK;
}

int rtr_scene_tree_cost(const rtr_scene* s, rtr_tree_cost* out) {
    if (!s || !out) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_tree_cost: null argument");
    HIP_TRY(hipSetDevice(s->ctx->device));
    { const int rcm = refresh_mirrors(s); if (rcm != RTR_OK) return rcm; }      /* the grid the sums are scaled with */
    hipStream_t st = s->ctx->stream;
    const SceneTree& t = s->tree;
    const uint32_t numNodes = (uint32_t)t.hostNodes.size();
    /* which slots are part of the tree: the refit's parent array where the scene has one (a device build leaves slots unused); a host
     * tree without one is looked at once, and gets a parent array of its own only if the root does not reach every slot */
    const int32_t* parent = t.refitReady ? t.parent.p : nullptr;
    if (!t.refitReady && t.costParentState == 0) {
        std::vector<int32_t> par;
        if (host_parent_array(t.hostNodes, par) == t.hostNodes.size()) t.costParentState = 1;
        else { HIP_TRY(t.costParent.upload(par.data(), par.size(), st)); t.costParentState = 2; }
    }
    if (!t.refitReady && t.costParentState == 2) parent = t.costParent.p;
    const size_t words = rtrdev::bvh_tree_cost_words();
    HIP_TRY(s->costWords.ensure(words));
    const hipError_t e = rtrdev::bvh_tree_cost(t.nodes.p, numNodes, parent, s->costWords.p, st);
    if (const int rc = launched(e, "rtr_scene_tree_cost")) return rc;
    uint64_t w[11];
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "layout");
    if (words != 11) return fail(RTR_ERR_HIP, "rtr_scene_tree_cost: the kernel has %zu words, the host expects 11", words);
    HIP_TRY(hipMemcpyAsync(w, s->costWords.p, sizeof w, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    rtr_tree_cost c{};
    for (int k = 0; k < 3; ++k) { c.innerArea[k] = w[k]; c.leafArea[k] = w[3 + k]; c.rootArea[k] = w[6 + k]; }
    c.numInner = w[9]; c.numLeafRefs = w[10];
    finish_tree_cost(&c, t.stats.grid);
    *out = c;
    return RTR_OK;
}

int rtr_scene_rebuild(rtr_scene* s, uint32_t buildFlags) {
    static const char* who = "rtr_scene_rebuild";
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null scene", who);
    if (buildFlags > RTR_BUILD_DEVICE_LBVH) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: unknown buildFlags %u", who, buildFlags);
    { const int rcm = refresh_mirrors(s); if (rcm != RTR_OK) return rcm; }
    if (scene_is_empty(s)) return RTR_OK;     /* nothing to build */
    HIP_TRY(hipSetDevice(s->ctx->device));
    /* frames and queries of OTHER contexts (other streams) may be walking this tree: everything enqueued on the device so far is joined
     * before it is replaced (contract in rtr.h, as the update calls) */
    HIP_TRY(hipDeviceSynchronize());
    hipStream_t st = s->ctx->stream;
    const size_t totalPrims = s->tree.hostTris.size();
    const bool deviceBuild = buildFlags == RTR_BUILD_DEVICE_LBVH && totalPrims >= 16;     /* tiny scenes: the host builder, as at creation */
    /* the new tree is built apart from the scene, from its vertices and host mirrors: whatever fails, `s` is as it was */
    SceneTree fresh;
    int rc = RTR_OK;
    if (deviceBuild) {
        std::vector<rtrdev::PrimRef> prims; std::vector<rtrdev::InstanceRef> refs;
        scene_prim_tables(s, s->hostInstances.data(), prims, refs);
        rc = build_on_device_core(fresh, st, prims, refs, s->vertices.p, s->indices.p, s->buildScratch, totalPrims);
        if (rc != RTR_OK) return rc;
    } else {
        std::vector<RtrVertex> vertices(s->numVertices); std::vector<uint32_t> indices(s->numIndices);
        if (s->numVertices) HIP_TRY(hipMemcpy(vertices.data(), s->vertices.p, vertices.size() * sizeof(RtrVertex), hipMemcpyDeviceToHost));
        if (s->numIndices) HIP_TRY(hipMemcpy(indices.data(), s->indices.p, indices.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        rtr_scene_desc view = host_view(s);
        view.vertices = vertices.data(); view.numVertices = s->numVertices; view.indices = indices.data(); view.numIndices = s->numIndices;
        rtr::BvhResult bvh; std::vector<float> xforms, nmats; uint32_t stackEntries = 0; size_t numTris = 0;
        rc = flatten_and_build(&view, bvh, xforms, nmats, &stackEntries, &numTris);      /* the transform tables it fills are the scene's own already */
        if (rc != RTR_OK) return rc;
        if (!s->hostMasks.empty()) {      /* the new records carry the instance masks, as a refit's do */
            const std::vector<uint32_t> maskBits = instance_mask_bits(s, s->hostMasks.data());
            for (RtrBvhTri& tr : bvh.tris) if (tr.customIndex < maskBits.size()) tr.flags |= maskBits[tr.customIndex];
        }
        HIP_TRY(fresh.nodes.upload(reinterpret_cast<const uint4*>(bvh.nodes.data()), bvh.nodes.size() * 2, st));
        HIP_TRY(fresh.grid.upload(&bvh.grid, 1, st));
        HIP_TRY(fresh.tris.upload(reinterpret_cast<const float4*>(bvh.tris.data()), bvh.tris.size() * 3, st));
        fill_stats(fresh.stats, bvh, stackEntries, numTris);
        fresh.hostNodes.swap(bvh.nodes); fresh.hostTris.swap(bvh.tris); fresh.hostWideShape.swap(bvh.wideShape);
        fresh.numPrims = (uint32_t)fresh.hostTris.size(); fresh.numNodeSlots = (uint32_t)fresh.hostNodes.size();
    }
    rc = make_wide_nodes(fresh, s->lights.p, s->numLights, st);
    if (rc != RTR_OK) return rc;
    /* the stage outlives a host rebuild, which drops the readiness: a scene that was EVER prepared for the enqueued rebuild is prepared
     * again by the next rebuild that gives it a device tree */
    const bool prepared = s->tree.asyncReady, preparedRebuild = s->tree.rebuildReady || s->stage.red.p != nullptr;
    const bool preparedPolicy = s->tree.rebuildIfReady || s->policy.p != nullptr;      /* likewise; its baseline becomes the new tree's cost */
    std::swap(s->tree, fresh);      /* `fresh` takes the old tree away: freed on return — the device was joined, and nothing has been enqueued against it since */
    point_at_tree(s->dev, s->tree);
    /* the enqueued update's tables and scratch belong to a tree: made again for the new one (its node count, its leaf slots) */
    if (prepared) { rc = rtr_scene_prepare_async_updates(s); if (rc != RTR_OK) return rc; }
    /* and the enqueued rebuild's readiness, where the new tree can take a commit: a host tree has other sizes, and stays unprepared */
    if (preparedRebuild && deviceBuild) { rc = rtr_scene_prepare_async_rebuild(s); if (rc != RTR_OK) return rc; }
    return preparedPolicy && deviceBuild ? prepare_rebuild_if(s, who) : RTR_OK;
}

void rtr_scene_destroy(rtr_scene* s) {
    if (!s) return;
    rtr_ctx* c = s->ctx;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    delete s;
    ctx_release_child(c);
}

int rtr_scene_get_stats(const rtr_scene* s, rtr_scene_stats* out) {
    if (!s || !out) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_get_stats: null argument");
    { const int rcm = refresh_mirrors(s); if (rcm != RTR_OK) return rcm; }
    *out = s->tree.stats;
    return RTR_OK;
}

int rtr_scene_export_bvh(const rtr_scene* s, RtrBvhNode* nodes, size_t nodeBytes, RtrBvhTri* tris, size_t triBytes) {
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_export_bvh: null scene");
    { const int rcm = refresh_mirrors(s); if (rcm != RTR_OK) return rcm; }
    if (nodes) {
        if (nodeBytes != s->tree.hostNodes.size() * sizeof(RtrBvhNode)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_export_bvh: nodeBytes %zu != %zu", nodeBytes, s->tree.hostNodes.size() * sizeof(RtrBvhNode));
        memcpy(nodes, s->tree.hostNodes.data(), nodeBytes);
    }
    if (tris) {
        if (triBytes != s->tree.hostTris.size() * sizeof(RtrBvhTri)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_export_bvh: triBytes %zu != %zu", triBytes, s->tree.hostTris.size() * sizeof(RtrBvhTri));
        memcpy(tris, s->tree.hostTris.data(), triBytes);
    }
    return RTR_OK;
}

int rtr_scene_export_wide(const rtr_scene* s, RtrWideNode* nodes, size_t nodeBytes) {
    if (!s || !nodes) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_export_wide: null argument");
    { const int rcm = refresh_mirrors(s); if (rcm != RTR_OK) return rcm; }
    if (nodeBytes != (size_t)s->tree.wideReached * sizeof(RtrWideNode)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_export_wide: nodeBytes %zu != %zu", nodeBytes, (size_t)s->tree.wideReached * sizeof(RtrWideNode));
    HIP_TRY(hipSetDevice(s->ctx->device));
    /* the device holds the RESIDENT order (best-first top, kernels/rtr_hot_top.h); the export is the same tree numbered breadth-first,
     * as it always was: a record's walk does not depend on where it is stored */
    std::vector<RtrWideNode> resident(s->tree.wideReached), bfs;
    HIP_TRY(hipMemcpy(resident.data(), s->tree.nodes4.p, nodeBytes, hipMemcpyDeviceToHost));      /* the records the tree reaches come first */
    rtr::wide_breadth_first(resident.data(), resident.size(), bfs);
    if (bfs.size() != resident.size()) return fail(RTR_ERR_HIP, "rtr_scene_export_wide: the resident records reach %zu of %zu", bfs.size(), resident.size());
    memcpy(nodes, bfs.data(), nodeBytes);
    return RTR_OK;
}

int rtr_scene_export_wide_resident(const rtr_scene* s, RtrWideNode* nodes, size_t nodeBytes) {
    if (!s || !nodes) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_export_wide_resident: null argument");
    { const int rcm = refresh_mirrors(s); if (rcm != RTR_OK) return rcm; }
    if (nodeBytes != (size_t)s->tree.wideReached * sizeof(RtrWideNode)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_export_wide_resident: nodeBytes %zu != %zu", nodeBytes, (size_t)s->tree.wideReached * sizeof(RtrWideNode));
    HIP_TRY(hipSetDevice(s->ctx->device));
    HIP_TRY(hipMemcpy(nodes, s->tree.nodes4.p, nodeBytes, hipMemcpyDeviceToHost));
    return RTR_OK;
}

uint32_t rtr_trace_top_nodes(void) { return rtrdev::trace_top_capacity(); }

int rtr_host_wide_resident(const RtrWideNode* wide, size_t wideBytes, const RtrBvhGrid* grid, const RtrAreaLightInfo* lights, uint32_t numLights, uint32_t topNodes,
                           RtrWideNode* out) {
    if (!wide || !grid || !out || (!lights && numLights)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_host_wide_resident: null argument");
    if (wideBytes == 0 || wideBytes % sizeof(RtrWideNode)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_host_wide_resident: wideBytes %zu is not a positive multiple of %zu", wideBytes, sizeof(RtrWideNode));
    const size_t count = wideBytes / sizeof(RtrWideNode);
    std::vector<uint32_t> pos;
    rtr::hot_top_positions(wide, count, *grid, lights, numLights, topNodes, pos);
    rtr::permute_wide_host(wide, count, pos, out);
    return RTR_OK;
}

int rtr_scene_update_lights(rtr_scene* s, const RtrAreaLightInfo* lights, uint32_t n) {
    if (!s || (!lights && n)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_update_lights: null argument");
    if (n != s->numLights) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_update_lights: %u lights given, scene has %u (light geometry is part of the BVH)", n, s->numLights);
    { const int rcm = refresh_mirrors(s); if (rcm != RTR_OK) return rcm; }      /* the transforms compared below: an enqueued instance update may have moved the lights */
    for (uint32_t l = 0; l < n; ++l) {
        if (lights[l].vertexOffset != s->hostLights[l].vertexOffset || lights[l].indexOffset != s->hostLights[l].indexOffset ||
            lights[l].numTriangles != s->hostLights[l].numTriangles || memcmp(lights[l].transform, s->hostLights[l].transform, sizeof lights[l].transform))
            return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_update_lights: light %u geometry/transform changed; only colour, intensity and sidedness may be updated without a rebuild", l);
    }
    HIP_TRY(hipSetDevice(s->ctx->device));
    if (n) {
        HIP_TRY(hipDeviceSynchronize());       /* frames in flight on other streams read s->lights: joined before the rewrite (contract in rtr.h) */
        HIP_TRY(hipMemcpyAsync(s->lights.p, lights, n * sizeof(RtrAreaLightInfo), hipMemcpyHostToDevice, s->ctx->stream));
        if (const int rc = enqueue_light_power(s, s->ctx->stream, "rtr_scene_update_lights")) return rc;      /* the powers follow colour and intensity */
        HIP_TRY(hipStreamSynchronize(s->ctx->stream));
        s->hostLights.assign(lights, lights + n);
    }
    return RTR_OK;
}

/* The traversal kernels address triangle records, BVH2 nodes and 4-wide records through 32-bit byte offsets from one buffer base
 * each ((first + i) * 48, node << 5, record << 6 in signed 32-bit lane arithmetic: kernels/rtr_device.h trace(), kernels/rtr_kernels.hip
 * inner_nodes4 / tri_any): a scene whose arrays reach 2 GiB would silently intersect the wrong records, so it is refused here. */
int rtr_check_scene_limits(uint64_t numTriangles, uint64_t numNodes) {
    const uint64_t kMaxBytes = 1ull << 31;
    if (numTriangles >= (1ull << 28)) return fail(RTR_ERR_INVALID_ARGUMENT, "%llu triangles: too many for the leaf encoding (2^28)", (unsigned long long)numTriangles);
    if (numTriangles * sizeof(RtrBvhTri) >= kMaxBytes)
        return fail(RTR_ERR_INVALID_ARGUMENT, "%llu triangles: the %zu-byte triangle records would reach 2 GiB, past the kernels' 32-bit record offsets (at most %llu triangles)",
                    (unsigned long long)numTriangles, sizeof(RtrBvhTri), (unsigned long long)((kMaxBytes - 1) / sizeof(RtrBvhTri)));
    if (numNodes * RTR_WIDE_NODE_BYTES >= kMaxBytes)
        return fail(RTR_ERR_INVALID_ARGUMENT, "%llu BVH nodes: the %d-byte 4-wide records would reach 2 GiB, past the kernels' 32-bit record offsets (at most %llu nodes)",
                    (unsigned long long)numNodes, RTR_WIDE_NODE_BYTES, (unsigned long long)((kMaxBytes - 1) / RTR_WIDE_NODE_BYTES));
    return RTR_OK;
}

}  // extern "C"
