/* rtr.h — C ABI of librtr_hip.so, the MI355X-native replacement for the reference's
 * Vulkan dispatch + GLSL ray-tracing pipeline.
 *
 * The reference has no plugin / FFI interface: Application::run() talks to its Vulkan
 * wrappers directly (reference src/app/application.cppm:99-484).  The boundary cut here is
 * "everything run() hands to the GPU and everything it reads back" (SURVEY.md §8b).  Each
 * entry point cites the reference code it replaces.  Plain pointers and sizes only; no
 * C++/torch types; no exceptions cross this boundary (every call returns an rtr_status and
 * rtr_last_error() gives the thread-local message — the C++ shim in
 * realtimeraytracer_amd/csrc/host rethrows std::runtime_error to keep the reference's
 * caller-visible convention, src/main.cpp:12-15).
 *
 * Threading: handles are not thread-safe; one rtr_ctx per device; calls are synchronous
 * unless stated (reference is single-threaded with waitIdle between passes,
 * src/app/application.cppm:353,396,437).
 */
#ifndef RTR_H
#define RTR_H

#include <stddef.h>
#include <stdint.h>
#include "rtr_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RTR_ABI_VERSION 3

typedef enum rtr_status {
    RTR_OK = 0,
    RTR_ERR_INVALID_ARGUMENT = -1,
    RTR_ERR_HIP = -2,            /* a HIP runtime call failed (message has hipGetErrorString) */
    RTR_ERR_NO_DEVICE = -3,
    RTR_ERR_UNSUPPORTED = -4,    /* a feature that is not built (e.g. an image format the host loader cannot decode) */
    RTR_ERR_OUT_OF_MEMORY = -5,
    RTR_ERR_BVH_TOO_DEEP = -6,   /* traversal stack bound exceeded; fail loudly, never clamp */
    RTR_ERR_IO = -7
} rtr_status;

typedef struct rtr_ctx   rtr_ctx;    /* one per device: replaces Instance/Device/CommandPool (src/vulkan/context/) */
typedef struct rtr_scene rtr_scene;  /* replaces vertex/index/info buffers + BLAS[] + TLAS (src/app/application.cppm:230-271) */
typedef struct rtr_frame rtr_frame;  /* replaces the storage images of descriptor set 0 (src/app/application.cppm:108-138) */

/* Which image of the reference's descriptor set 0 (src/shaders/raygen.rgen:12-16;
 * binding numbers kept).  All are R8G8B8A8_UNORM with bytes B,G,R,255 as raygen stores them. */
typedef enum rtr_image {
    RTR_IMAGE_ANALYTIC = 0,           /* binding 0: LTC analytic, needs LTC tables */
    RTR_IMAGE_SHADOWED = 1,           /* binding 1: THE framebuffer of the north-star path */
    RTR_IMAGE_UNSHADOWED = 2,         /* binding 2 */
    RTR_IMAGE_DENOISED_SHADOWED = 3,  /* binding 3 (denoise.comp output) */
    RTR_IMAGE_DENOISED_UNSHADOWED = 4,/* binding 4 */
    RTR_IMAGE_FINAL = 5,              /* binding 5 (combine.comp output) */
    RTR_IMAGE_NORMAL = 6,             /* binding 6 */
    RTR_IMAGE_POSITION = 7,           /* binding 7 */
    RTR_IMAGE_HDR = 16                /* float4 pre-tonemap accumulation of SHADOWED (build-side extension) */
} rtr_image;

/* Bit mask of images a frame owns / a render call writes. */
#define RTR_IMG_BIT(which) (1u << (which))
#define RTR_IMAGES_FRAMEBUFFER (RTR_IMG_BIT(RTR_IMAGE_SHADOWED))
#define RTR_IMAGES_RAYGEN5 (RTR_IMG_BIT(RTR_IMAGE_ANALYTIC) | RTR_IMG_BIT(RTR_IMAGE_SHADOWED) | \
                            RTR_IMG_BIT(RTR_IMAGE_UNSHADOWED) | RTR_IMG_BIT(RTR_IMAGE_NORMAL) | \
                            RTR_IMG_BIT(RTR_IMAGE_POSITION))
#define RTR_IMAGES_DENOISE (RTR_IMG_BIT(RTR_IMAGE_DENOISED_SHADOWED) | RTR_IMG_BIT(RTR_IMAGE_DENOISED_UNSHADOWED) | \
                            RTR_IMG_BIT(RTR_IMAGE_FINAL))

/* One entry of the reference's texSamplers[] array (src/app/setup/create_scene.cppm:71-141): 8-bit texels as
 * core::file::createTextureImage produces them (src/core/file.cppm:272-311: stb_image, vertical flip,
 * R8G8B8A8_UNORM or R8_UNORM), sampled with the reference's sampler — linear filter, repeat addressing, one mip
 * (src/vulkan/memory/image_sampler.cppm:26-42).  Row 0 of `pixels` is v = 0. */
typedef struct rtr_texture {
    const uint8_t* pixels;     /* width*height*channels bytes; NULL for an unused slot (indices 0,1 = LTC tables) */
    uint32_t       width, height;
    uint32_t       channels;   /* 4 = RGBA8, 1 = R8 */
    uint32_t       _pad;
} rtr_texture;

/* What Application::run() uploads once (src/app/application.cppm:226-271,
 * src/app/setup/geometry_builder.cppm:50-212, src/vulkan/raytracing/tlas.cppm:44-149).
 * The library copies everything; the caller keeps ownership of its arrays. */
typedef struct rtr_scene_desc {
    const RtrVertex*        vertices;      uint32_t numVertices;   /* Vertex SSBO, application.cppm:242-248 */
    const uint32_t*         indices;       uint32_t numIndices;    /* mesh-local indices, geometry_builder.cppm:162-169 */
    const RtrMesh*          meshes;        uint32_t numMeshes;     /* one per BLAS */
    const RtrInstance*      instances;     uint32_t numInstances;  /* TLAS instances: lights first, then objects */
    const RtrObjectInfo*    objects;       uint32_t numObjects;    /* ObjectInfo SSBO, application.cppm:254-261 */
    const RtrAreaLightInfo* lights;        uint32_t numLights;     /* LightInfo SSBO, application.cppm:264-271 */
    /* texSamplers[0], [1]: 64x64 RGBA32F LTC tables (src/app/setup/create_scene.cppm:65-69,162-214).
     * NULL -> RTR_IMAGE_ANALYTIC cannot be rendered (RTR_ERR_UNSUPPORTED if asked for). */
    const float*            ltc1;          /* 64*64*4 floats or NULL */
    const float*            ltc2;          /* 64*64*4 floats or NULL */
    /* miss.rmiss:21-26 samples an equirect HDRI (binding 7); when `hdri` is NULL the sky is this constant
     * (sRGB-encoded; ToLinear applied as the miss shader does). */
    float                   skyColor[3];
    float                   _pad;
    /* texSamplers[] (set 1 binding 4): ObjectInfo.colorIndex / specularIndex / metallicIndex / opacityIndex index
     * this array; the reference keeps the LTC tables at 0 and 1 so material textures start at 2. */
    const rtr_texture*      textures;      uint32_t numTextures;
    const rtr_texture*      hdri;          /* equirect sky (RGBA8, as stbi_load of the .hdr gives, file.cppm:279-291) or NULL */
    /* Acceleration-structure build preference (reference: vk::BuildAccelerationStructureFlagBitsKHR, blas.cppm:115
     * ePreferFastTrace; tlas.cppm eAllowUpdate): RTR_BUILD_HOST_SAH (default, best trace speed) or
     * RTR_BUILD_DEVICE_LBVH (Morton/radix-tree build on the GPU, fastest build).  Rendered images are identical. */
    uint32_t                buildFlags;
    uint32_t                _pad2;
} rtr_scene_desc;

#define RTR_BUILD_HOST_SAH    0u
#define RTR_BUILD_DEVICE_LBVH 1u

typedef struct rtr_scene_stats {
    uint32_t numTriangles;
    uint32_t numNodes;
    uint32_t maxDepth;        /* deepest leaf, root = 1 */
    uint32_t maxLeafSize;
    uint32_t bvhLayoutVersion;
    uint32_t stackEntries;    /* LDS stack entries per lane the kernels were specialised for */
    float    buildMs;
    float    sahCost;
    float    boundsMin[3];
    float    boundsMax[3];
    float    boxPad;
    float    _pad;
    RtrBvhGrid grid;          /* the 16-bit planes of the exported nodes live on this grid (rewritten by a refit) */
    uint32_t numWideNodes;    /* RtrWideNode records of the wide view (rtr_scene_export_wide, rtr_host_build_bvh_wide); 0 from rtr_host_build_bvh */
    uint32_t wideLayoutVersion;
    uint32_t _pad2[2];
} rtr_scene_stats;

/* Per-dispatch arguments: what the reference passes as the traceRaysKHR extent + the two
 * shader constants (src/vulkan/ray_tracing_pipeline.cppm:212-214, src/shaders/raygen.rgen:8-9),
 * plus the band sharding and accumulation that are new in this build. */
typedef struct rtr_render_params {
    uint32_t width;            /* full frame width  (dispatch extent x) */
    uint32_t height;           /* full frame height (dispatch extent y) */
    uint32_t spp;              /* NUM_PRIMARY_RAYS (reference: 4) */
    uint32_t numShadowRays;    /* NUM_SHADOW_RAYS  (reference: 3) */
    uint32_t images;           /* mask of RTR_IMG_BIT(...) to produce; 0 -> RTR_IMAGES_FRAMEBUFFER */
    uint32_t bandRows;         /* rows per band; 0 -> 8 */
    uint32_t shardIndex;       /* this device renders bands b with b % shardCount == shardIndex */
    uint32_t shardCount;       /* 0 or 1 -> whole frame */
    uint32_t accumulate;       /* 0: HDR = this frame; 1: HDR += this frame (needs RTR_IMAGE_HDR in the frame) */
    uint32_t accumulatedFrames;/* frames already summed in HDR (tonemap divides by accumulatedFrames+1) */
    uint32_t collectStats;     /* 1: run the counting variants of the kernels and fill rtr_frame_stats counters */
    uint32_t pipeline;         /* 0: default; 1: megakernel; 2: wavefront (staged) */
} rtr_render_params;

typedef struct rtr_frame_stats {
    /* exact work counters of the last render with collectStats=1 */
    uint64_t numRays;          /* every traceRay-equivalent issued: primary + shadow */
    uint64_t numPrimaryRays;
    uint64_t numShadowRays;
    uint64_t numNodeVisits;    /* N_node: node record fetches */
    uint64_t numTriTests;      /* N_tri : 48-B triangle record fetches */
    uint64_t numHits;          /* N_hit : closest-hit shading fetches (236 B each) */
    uint64_t numLightFetches;  /* N_lightfetch: LightInfo reads (96 B each) */
    uint64_t numLightTriFetches;/* light triangle vertex fetches (3 idx + 3 x 48 B = 156 B each) */
    uint64_t numTexFetches;    /* bilinear texture / HDRI lookups (4 texels, 16 B each) */
    uint64_t numAlphaTests;    /* opacity.rahit invocations that sampled an opacity map (236 B fetch + 1 lookup each) */
    uint64_t algorithmicBytes; /* B = 32 N_node_primary (RTR_BVH_NODE_BYTES) + 64 N_node_shadow (RTR_WIDE_NODE_BYTES; 32 in the megakernel) + 48 N_tri + 236 (N_hit + N_alpha) + 96 N_lf + 156 N_ltf + 16 N_tex + 4 k P (+16/32 P HDR) */
    /* the any-hit share of the above (work of the k_shadow_trace launch, the dominant kernel) */
    uint64_t numShadowNodeVisits;
    uint64_t numShadowTriTests;
    uint64_t shadowTraceBytes; /* 64 N_node_shadow (RTR_WIDE_NODE_BYTES: 4-wide records visited; 32 in the megakernel, which walks the BVH2) + 48 N_tri_shadow + 37 N_shadow_rays (20-B queue record + the 16-B origin its pixel-sample's rays share + the visibility byte) */
    /* timings of the last render (HIP events on the render stream), milliseconds */
    float    totalMs;
    float    primaryMs;        /* k_primary (wavefront) or the whole megakernel */
    float    shadowGenMs;      /* k_shadow_gen */
    float    shadowTraceMs;    /* the any-hit kernel (k_shadow_trace4) alone: the dominant kernel */
    float    resolveMs;        /* k_resolve */
    uint32_t localRows;        /* rows this shard rendered */
    uint32_t localPixels;
    uint32_t pipelineUsed;     /* 1 megakernel, 2 wavefront */
    float    shadowTraceClockMHz; /* shader clock the any-hit launch ran at: s_memtime ticks / s_memrealtime (100 MHz) ticks of one wave per XCD, MEAN over the XCDs (they clock independently; slowest / fastest below) */
    /* scheduling of the any-hit kernel, from its counting form (collectStats = 1): loop trips of its node and triangle phases,
     * summed over waves, and the lanes that had work in those trips (lane utilisation = lanes / (64 trips)) */
    uint64_t shadowInnerIterations, shadowInnerActiveLanes;
    uint64_t shadowTriIterations, shadowTriActiveLanes;
    uint64_t shadowRefills;
    float    shadowTailMs;     /* k_shadow_tail (the rays that outgrew the LDS stack, redone over the BVH2); part of totalMs */
    uint32_t _padTail;
    uint64_t primaryTailRays;  /* camera rays that outgrew the 16-entry LDS stack of k_primary_persist and were redone by k_primary_tail over the BVH2 */
    uint64_t shadowTailRays;   /* rays that outgrew the 16-entry LDS stack and were finished by k_shadow_tail over the BVH2 (both parts of their work are in the counters) */
    float    shadowTraceClockMinMHz, shadowTraceClockMaxMHz;   /* the slowest and the fastest XCD of that launch */
} rtr_frame_stats;

/* ---- context -------------------------------------------------------------------------- */
/* replaces Instance+Device creation (src/app/application.cppm:65-69): picks HIP device `ordinal`. */
int  rtr_ctx_create(int deviceOrdinal, rtr_ctx** out);
/* Scenes and frames created on a context may be destroyed after it (garbage-collected bindings do that): the context's
 * resources are released when its last child is gone.  Creating new objects on a destroyed context is an error. */
void rtr_ctx_destroy(rtr_ctx* ctx);
/* Use an existing HIP stream (e.g. torch's current stream) for all work of this ctx; NULL -> own stream. */
int  rtr_ctx_set_stream(rtr_ctx* ctx, void* hipStream);
/* The HIP stream (hipStream_t) this context's work is enqueued on, for callers that order their own work against it with events. */
int  rtr_ctx_get_stream(rtr_ctx* ctx, void** hipStream);
int  rtr_ctx_device_name(rtr_ctx* ctx, char* buf, size_t bytes);
/* Run-time tunables of the staged pipeline (scheduling knobs of its kernels: queue binning, batch lengths, persistent workgroups per
 * CU ...; the names are the fields of rtrdev::Tunables, kernels/rtr_kernels.h).  A context reads them from the environment ONCE, when
 * it is created (RTR_<NAME IN CAPITALS>); a render uses those of the context of its (leading) frame.  No setting changes a pixel
 * (tested); the defaults are the measured optima.  RTR_ERR_INVALID_ARGUMENT for an unknown name or a value outside its range.
 * The reference has no counterpart: its traversal is the driver's (src/vulkan/ray_tracing_pipeline.cppm:212-214). */
int  rtr_ctx_set_tunable(rtr_ctx* ctx, const char* name, uint32_t value);
int  rtr_ctx_get_tunable(const rtr_ctx* ctx, const char* name, uint32_t* value);

/* ---- scene ---------------------------------------------------------------------------- */
/* replaces createSceneFromObjectsAndLights' GPU half (src/app/setup/create_scene.cppm:48-160):
 * validates, flattens instances to world space, builds the BVH on the host, uploads. */
int  rtr_scene_create(rtr_ctx* ctx, const rtr_scene_desc* desc, rtr_scene** out);
/* The same scene once more — on another context, usually another device — WITHOUT building its tree again: `built` is a scene
 * made from the same `desc` (same arrays, same buildFlags) whose host-side copy of the tree is uploaded as it is.  What
 * librtr_mgpu.so replicates the scene with: one build per node instead of one per GPU.  The reference builds its acceleration
 * structure once, on its one device (src/vulkan/raytracing/blas.cppm:75-167); this is that build shared by N devices.
 * RTR_ERR_INVALID_ARGUMENT if `built` does not match `desc` (triangle count).  After rtr_scene_update_vertices on `built`, `desc` must
 * carry the vertices `built` currently has (rtr_scene_export_vertices): its tree was fitted to those, and nothing here can check it. */
int  rtr_scene_create_like(rtr_ctx* ctx, const rtr_scene_desc* desc, const rtr_scene* built, rtr_scene** out);
void rtr_scene_destroy(rtr_scene* scene);
int  rtr_scene_get_stats(const rtr_scene* scene, rtr_scene_stats* out);
/* Copy out the device BVH arrays (test / oracle hook; sizes and the plane grid from rtr_scene_get_stats). */
int  rtr_scene_export_bvh(const rtr_scene* scene, RtrBvhNode* nodes, size_t nodeBytes,
                          RtrBvhTri* tris, size_t triBytes);
/* Copy out the 4-wide view the any-hit kernel walks (RtrWideNode, layout RTR_WIDE_LAYOUT_VERSION): numWideNodes records; their
 * leaf codes index the triangle array of rtr_scene_export_bvh.  Test / oracle hook: the oracle restates the kernel's walk over
 * it to check the kernel's work counters. */
int  rtr_scene_export_wide(const rtr_scene* scene, RtrWideNode* nodes, size_t nodeBytes);
/* The same records in the RESIDENT order, byte for byte what the device holds: a best-first top towards the area lights — what the
 * any-hit kernel keeps in LDS, rtr_trace_top_nodes() records at the most — then every other record in breadth-first order.  The
 * top grows from the root: the inner child with the highest priority of any record already in it comes next, ties to the lower
 * breadth-first index; a record's priority is the sum over the area lights of min(1, box area / (4 pi d^2)), d the distance from the
 * light's centre (its transform's translation) to the record's box.  Record 0 is the root and a record precedes its children, so
 * every walk is the one over rtr_scene_export_wide; a scene without area lights is resident in breadth-first order.  Every build,
 * refit and rebuild, synchronous or enqueued, orders the records it writes this way, from the boxes and lights it finds. */
int  rtr_scene_export_wide_resident(const rtr_scene* scene, RtrWideNode* nodes, size_t nodeBytes);
/* The 4-wide records the any-hit kernel of this build keeps in LDS (its kTopNodes): the size of the resident order's top. */
uint32_t rtr_trace_top_nodes(void);
/* Host restatement of the resident order, no device: `wide` (wideBytes = a positive multiple of 64) is a breadth-first view
 * (rtr_host_build_bvh_wide or rtr_scene_export_wide), `grid` its grid with the wide centre, `lights` the scene's area lights;
 * `out` takes the same records in the order rtr_scene_export_wide_resident shows for them with a top of topNodes records. */
int  rtr_host_wide_resident(const RtrWideNode* wide, size_t wideBytes, const RtrBvhGrid* grid, const RtrAreaLightInfo* lights, uint32_t numLights,
                            uint32_t topNodes, RtrWideNode* out);
/* Host-only BVH build (no device needed): validates `desc`, flattens and builds exactly as
 * rtr_scene_create does and copies the result out.  Call with nodes == tris == NULL to get the counts
 * in `stats`.  Used by the CPU-side tests (BVH invariants, oracle BVH-vs-brute-force). */
int  rtr_host_build_bvh(const rtr_scene_desc* desc, rtr_scene_stats* stats, RtrBvhNode* nodes, size_t nodeBytes,
                        RtrBvhTri* tris, size_t triBytes);
/* The same build, plus the 4-wide view rtr_scene_create would put on the device for it: the host restatement of the kernels that
 * make it (the wide centre, the records the builder's cost-driven collapse chose, breadth-first order) — byte-identical to
 * rtr_scene_export_wide of a scene made from `desc` (checked in the GPU tests).  stats->numWideNodes / wideLayoutVersion and the
 * wide centre in stats->grid are filled; call with all arrays NULL for the counts.  No device needed: CPU-only tests walk the wide
 * view with the oracle, and tree experiments price a builder change by the oracle's visit counters before any GPU time is spent. */
int  rtr_host_build_bvh_wide(const rtr_scene_desc* desc, rtr_scene_stats* stats, RtrBvhNode* nodes, size_t nodeBytes,
                             RtrBvhTri* tris, size_t triBytes, RtrWideNode* wide, size_t wideBytes);
/* Limits of the 32-bit record offsets the traversal kernels use: RTR_OK if a scene of numTriangles triangles and numNodes BVH nodes
 * can be addressed (triangle records and 4-wide records each below 2 GiB: at most 44 739 242 triangles, 33 554 431 nodes; and the
 * 2^28 of the leaf encoding), else RTR_ERR_INVALID_ARGUMENT with the reason in rtr_last_error().  rtr_scene_create applies it
 * to the worst case for its triangle count (numTriangles - 1 nodes) before anything is built or allocated. */
int  rtr_check_scene_limits(uint64_t numTriangles, uint64_t numNodes);
/* Dynamic scenes: new instance transforms (same instances, meshes and customIndex as at creation) and, optionally,
 * new light infos (NULL keeps them).  World-space triangle records are recomputed and every BVH box is re-fitted ON
 * THE DEVICE; the topology is kept.  Replaces TLAS::updateTransform + TLAS::refit
 * (src/vulkan/raytracing/tlas.cppm:151-207; present in the reference, never called by its app). */
/* Both update calls rewrite device arrays that renders read (nodes, 4-wide records, triangle records, light tables).  A scene may be
 * rendered by frames of several contexts / streams at once, so the calls first JOIN THE WHOLE DEVICE (hipDeviceSynchronize: every
 * frame in flight on any stream of this process finishes with the old scene), rewrite, and return when the new state is complete.
 * They are therefore safe to call at any time from the thread that enqueues the renders; a caller that renders the scene from
 * other threads or processes must itself keep those from enqueueing new frames of this scene until the call has returned. */
int  rtr_scene_update_instances(rtr_scene* scene, const RtrInstance* instances, uint32_t numInstances,
                                const RtrAreaLightInfo* lights, uint32_t numLights);
/* Deforming meshes: new vertex positions (and, optionally, normals) for parts of the scene's vertex array, then ONE refit — what Vulkan
 * does with a BLAS built with ALLOW_UPDATE and rebuilt in MODE_UPDATE (the reference sets eAllowUpdate on its TLAS and leaves the rest
 * as a TODO, src/vulkan/raytracing/tlas.cppm:20,106,176-178).  Skinned characters, cloth, morph targets, a simulation that lives in a
 * torch tensor: the topology (indices, meshes, instances) stays, the vertices move.
 * ranges[r] names numVertices vertices from firstVertex of the scene's CONCATENATED vertex array (rtr_scene_desc::vertices; a range may
 * span meshes) and where their new data is: three floats per vertex, positionStride / normalStride bytes apart — 12 is packed float3,
 * 16 a float4 column, 48 an RtrVertex array with normals = base + 16.  A stride is a multiple of 4 and at least 12 (normalStride is only
 * looked at when a range brings normals).  flags: RTR_VERTICES_HOST — the pointers are host pointers — or RTR_VERTICES_DEVICE — they
 * are DEVICE pointers on the scene's device (torch tensors, hipMalloc), 4-B aligned; one call is one kind.
 * Written: position[0..2] of the named vertices, and normal[0..2] where the range's normals is not NULL.  uv and the pad words keep their
 * bytes; vertices outside the ranges are untouched.  Then comes exactly one refit, rtr_scene_update_instances' own, with `instances`
 * and `lights`, or with the current ones where they are NULL (numInstances / numLights are then ignored): world-space records, boxes,
 * grid, 4-wide view, host mirrors, boxPad; the light-triangle table is ALWAYS remade (a light's mesh may be among the vertices).
 * Instance masks and the triangle -> leaf table survive; the mirrored bits are recomputed only when instances are given.
 * Everything is validated BEFORE anything is written, and a refused call leaves the scene byte for byte as it was:
 * RTR_ERR_INVALID_ARGUMENT (with a message) for a null scene or ranges, numRanges == 0, a null positions in a range with vertices,
 * a bad stride, a range that leaves the vertex array or overlaps another (checked on the host), unknown flag bits, a device pointer
 * that is not 4-B aligned, everything rtr_scene_update_instances refuses in instances / lights, and a position that rtr_scene_create
 * would refuse — not finite, or beyond +-3.0e38 — anywhere in any range: the message names the range and the vertex (the first in range
 * order).  Host data is checked by a host loop; device data by a kernel that reduces the first bad (range, vertex) into a word the host
 * reads before the writing kernel is launched.  Normals are NOT validated: they are shading data.  An empty scene returns RTR_OK and
 * does nothing, as rtr_scene_update_instances.
 * Synchronisation: as the other update calls (above): the call joins the whole device, rewrites, and returns when the new state is
 * complete.  With RTR_VERTICES_DEVICE the caller's data must be complete before the call: the device join guarantees that for work
 * ALREADY ENQUEUED on any stream of this process when the call is made; work of other processes, or work enqueued from another thread
 * during the call, is the caller's to order.  The data is read during the call only; the library keeps no pointer to it.
 * rtr_scene_create_like afterwards: `desc` must carry the vertices the `built` scene has NOW (rtr_scene_export_vertices gives them),
 * since the tree that is copied was fitted to those. */
#define RTR_VERTICES_HOST   0u   /* positions / normals of the ranges are host pointers */
#define RTR_VERTICES_DEVICE 1u   /* ... are DEVICE pointers on the scene's device (torch tensors, hipMalloc), 4-B aligned */
typedef struct rtr_vertex_range {
    uint32_t    firstVertex, numVertices;  /* into the scene's concatenated vertex array (rtr_scene_desc::vertices) */
    const void* positions;                 /* numVertices x 3 floats, positionStride bytes apart */
    const void* normals;                   /* the same with normalStride, or NULL: normals are kept */
} rtr_vertex_range;                        /* 24 bytes */
int  rtr_scene_update_vertices(rtr_scene* scene, const rtr_vertex_range* ranges, uint32_t numRanges,
                               uint32_t positionStride, uint32_t normalStride, uint32_t flags,
                               const RtrInstance* instances, uint32_t numInstances,
                               const RtrAreaLightInfo* lights, uint32_t numLights);
/* Copy out the device vertex array as it is now (test / oracle hook like rtr_scene_export_bvh, and what rtr_scene_create_like needs
 * after a deformation): numVertices records; RTR_ERR_INVALID_ARGUMENT for a null pointer or a `bytes` that is not numVertices * 48. */
int  rtr_scene_export_vertices(const rtr_scene* scene, RtrVertex* out, size_t bytes);
/* The ENQUEUED vertex update: rtr_scene_update_vertices as stream-ordered work.  The synchronous call joins the device, remakes tables on
 * the host, reads the tree back and renumbers the 4-wide view in a host loop; this form touches the host for argument checks and kernel
 * launches only: check kernel -> predicated write kernel -> refit -> 4-wide view -> its breadth-first order ON THE DEVICE (kernels/
 * rtr_bvh.hip, k_wide_order) -> permutation -> light triangles, all enqueued on the stream of the scene's context (rtr_ctx_set_stream
 * makes that a caller's stream, torch's for one).  The result is the synchronous call's, byte for byte (tested).
 * rtr_scene_prepare_async_updates: ONCE per scene, synchronous — everything the enqueued form must not do later.  It may join and
 * allocate: the refit arrays of a host-built tree, the order kernel's scratch, the status words, and the device tables a refit flattens
 * from (primitives and instances, the current instance masks in the flags).  Afterwards rtr_scene_set_instance_masks,
 * rtr_scene_update_instances, rtr_scene_update_vertices and rtr_scene_rebuild keep those tables current (a rebuild prepares the new tree
 * again by itself), so an enqueued update after any of them writes records with the right masks and leaf slots.  Idempotent; an empty
 * scene returns RTR_OK.
 * rtr_scene_update_vertices_async: ranges, strides and rules of RTR_VERTICES_DEVICE (device pointers, 4-B aligned; stride a multiple of
 * 4, at least 12; normals optional).  No instances and no lights: they have an enqueued call of their own,
 * rtr_scene_update_instances_async below.  The call returns without joining the device, the stream or the host to anything; inside it there is no allocation,
 * no synchronisation, no device -> host copy and no copy from host memory that could be reused before the copy runs — the table of
 * ranges travels as kernel arguments, 64 ranges per launch, and the caller's `ranges` array is free when the call returns (the DEVICE
 * memory it points at is read when the stream gets there).  Refused BEFORE anything is enqueued, with the synchronous call's messages:
 * a null scene or ranges, numRanges == 0, a bad stride, a range that leaves the vertex array or overlaps another, null positions in a
 * range with vertices, a misaligned pointer; and a scene that has not been prepared (RTR_ERR_INVALID_ARGUMENT; the message names
 * rtr_scene_prepare_async_updates).
 * ORDERING.  Work enqueued on that stream before the call sees the old scene; work enqueued after it sees the new one; the caller's
 * kernels that produce the positions on that stream come before it without any event.  Work on OTHER streams or contexts that reads the
 * scene — renders of frames of other contexts, queries — is the caller's to order with events (rtr_ctx_get_stream), as a Vulkan
 * application barriers an acceleration-structure update.  The refit scratch is the scene's and shared: two updates of one scene are
 * ordered by being on one stream, so the context's stream must not be changed while updates of its scenes are pending.
 * BAD DATA.  An enqueued call cannot refuse.  The checking kernel (the rule of rtr_scene_create: inside +-3.0e38) reduces the smallest
 * offending SCENE vertex index into a device word; the writing kernel writes NOTHING for that update when the word is set — all ranges
 * land or none does — and the refit runs on the vertices as they are: after a refused update the vertex array keeps its bytes and every
 * query and render answers as before it (tested).  A one-lane kernel folds the word into the sticky status below.
 * rtr_scene_update_status: joins the scene's context stream (only that stream) and reports: `enqueued` — calls that returned RTR_OK, the
 * serial numbers of the updates counting from 1; `refused` — how many of them the device refused, since preparation; firstRefusedUpdate
 * / firstBadVertex — the serial (its low 32 bits) of the first refused update SINCE THE LAST STATUS CALL and the smallest scene vertex
 * index it refused, 0xffffffff each when there was none.  A scene never prepared reports zeros.
 * HOST MIRRORS.  After an enqueued update the library's host copies (nodes, records, grid, boxPad, the count of reached 4-wide
 * records) are stale and marked so; rtr_scene_export_bvh / _export_wide, rtr_scene_get_stats, rtr_scene_create_like,
 * rtr_scene_tree_cost, rtr_scene_set_instance_masks, the synchronous update calls, rtr_scene_rebuild and the first rtr_hit_leaves /
 * rtr_light_rays_hinted (the leaf-table build) first join the scene's stream and read them back, once.  Renders and queries need none
 * of them.  The triangle -> leaf table and the instance masks survive, as in the synchronous call; the light-triangle table is always
 * remade.  Scenes replicated by librtr_mgpu have no enqueued update, as they have no update path. */
/* Both enqueued updates — rtr_scene_update_vertices_async and rtr_scene_update_instances_async (below) — count on ONE serial sequence:
 * `enqueued`, `refused` and firstRefusedUpdate speak of updates of either kind.  For a refused INSTANCE update firstBadVertex carries the
 * smallest offending ELEMENT INDEX of that update instead of a vertex: i < numInstances(scene) is instance i (instance order),
 * numInstances(scene) + l is light l.  An enqueued REBUILD (rtr_scene_rebuild_async, below) counts on the same sequence; for a refused
 * rebuild firstBadVertex carries the DEPTH of the tree that was refused.  The caller knows which call had which serial. */
typedef struct rtr_update_status {
    uint64_t enqueued, refused;
    uint32_t firstRefusedUpdate, firstBadVertex;
    uint32_t _pad[2];
} rtr_update_status;                       /* 32 bytes */
#ifdef __cplusplus
static_assert(sizeof(rtr_update_status) == 32, "rtr_update_status is 32 B");
#endif
int  rtr_scene_prepare_async_updates(rtr_scene* scene);
int  rtr_scene_update_vertices_async(rtr_scene* scene, const rtr_vertex_range* ranges, uint32_t numRanges,
                                     uint32_t positionStride, uint32_t normalStride);
int  rtr_scene_update_status(rtr_scene* scene, rtr_update_status* out);
/* The ENQUEUED instance update: rtr_scene_update_instances as stream-ordered work — rigid bodies moved every frame from transforms that
 * live on the device (a torch tensor, a physics kernel's output), the TLAS update of the reference (TLAS::updateTransform + TLAS::refit,
 * src/vulkan/raytracing/tlas.cppm:151-207).  The synchronous call joins the whole device and makes the transform, normal-matrix,
 * mirrored-bit and InstanceRef tables in host loops; this form makes them ON THE DEVICE and ends in the chain of
 * rtr_scene_update_vertices_async.  The result is the synchronous call's, byte for byte (tested).
 * transforms: a DEVICE pointer on the scene's device, 4-B aligned, or NULL (below): 12 floats per instance, a row-major 3x4 as
 * RtrInstance::transform, transformStride bytes apart.  The stride is a multiple of 4 and at least 48: 48 is a packed (n,3,4) array, 64
 * the top three rows of an (n,4,4) row-major matrix array, or an RtrInstance array entered at +16.  The records are for the instances
 * firstInstance .. firstInstance + numInstances - 1 in INSTANCE ORDER (rtr_scene_desc::instances: lights first, then objects); the other
 * instances keep their transforms.  Meshes and customIndex cannot change: there is nothing to pass them with.
 * lights: a DEVICE array of numLights RtrAreaLightInfo (96 B each, 4-B aligned), or NULL to keep the light infos; numLights must be the
 * scene's.  transforms == NULL with numInstances == 0 and a non-NULL lights is a lights-only update.  A light instance's transform and
 * its RtrAreaLightInfo::transform must agree: as in the synchronous call, that is the caller's business.
 * The scene must have been prepared (rtr_scene_prepare_async_updates, which also makes the instance-order -> customIndex device table
 * this call needs; rtr_scene_rebuild prepares again by itself).  The call itself does no allocation, no synchronisation, no device ->
 * host copy and no copy from reusable host memory: argument checks and launches only, everything enqueued on the scene's context
 * stream — ORDERING as documented for rtr_scene_update_vertices_async.  The chain:
 *   check kernel   one lane per element; reduces the smallest offending ELEMENT INDEX of this update into a device word.  Element
 *                  i < numInstances(scene) is instance i: bad when one of its 12 floats is not inside +-3.0e38 (the synchronous call's
 *                  rule).  Element numInstances(scene) + l is light l: bad when its vertexOffset, indexOffset or numTriangles differ
 *                  from the scene's current device light table.  No other light field is validated, as in the synchronous call.
 *   write kernel   nothing at all when the word is set: all of the update lands or none of it.  Otherwise, for each named instance at
 *                  its customIndex slot: the transform table (12 floats), words 0..8 of the normal-matrix slot (rtr_normal_matrix),
 *                  the mirrored word (1 iff the 3x3 determinant, in double, is negative — the host's expression and operation order;
 *                  the other words of the slot keep their bytes) and the transform of the refit's instance table; and the light infos.
 *   the refit chain of rtr_scene_update_vertices_async: refit -> 4-wide view -> its breadth-first order -> permutation -> light
 *                  triangles (always remade) -> the status fold with this call's serial.  After a refused update the chain runs on
 *                  unchanged tables: every byte and every answer stays.
 * Refused BEFORE anything is enqueued (RTR_ERR_INVALID_ARGUMENT, the message names the function): a null scene; transforms and lights
 * both NULL; transforms == NULL with numInstances != 0, or the reverse; a stride that is not a multiple of 4 or below 48; a misaligned
 * pointer; firstInstance + numInstances (in 64 bits) past the scene's instances; a numLights that is not the scene's when lights is
 * given; a scene that has not been prepared (the message names rtr_scene_prepare_async_updates).  An empty scene returns RTR_OK, counts
 * as enqueued and does nothing.
 * STATUS: rtr_scene_update_status, one serial sequence with the vertex updates (see rtr_update_status above).
 * HOST MIRRORS.  After this call the library's host copies of the instance transforms and the light infos are stale too, and marked so:
 * every call that reads them — rtr_scene_update_vertices with instances == NULL, rtr_scene_set_instance_masks, rtr_scene_rebuild,
 * rtr_scene_update_lights, rtr_scene_update_instances, rtr_scene_create_like, rtr_scene_export_instances — first joins the scene's
 * stream and reads them back from the device (transforms from the refit's instance table, lights from the light table), once. */
int  rtr_scene_update_instances_async(rtr_scene* scene, const void* transforms, uint32_t transformStride,
                                      uint32_t firstInstance, uint32_t numInstances,
                                      const RtrAreaLightInfo* lights, uint32_t numLights);
/* Copy out the instances as they are now, in instance order (test hook like rtr_scene_export_vertices, and what rtr_scene_create_like
 * needs after a device-side animation): numInstances records; RTR_ERR_INVALID_ARGUMENT for a null pointer or a `bytes` that is not
 * numInstances * 64.  Joins only the scene's stream, and only when an enqueued update has left the host copies stale. */
int  rtr_scene_export_instances(const rtr_scene* scene, RtrInstance* out, size_t bytes);
/* The SAH cost of the tree the kernels walk NOW: what a refit did to the tree's quality, and what a rebuild would win back.  A refit
 * keeps the split decisions made for the old shape, and rtr_scene_stats::sahCost is the host builder's number at creation (0 for a device
 * build), which no update ever touches; this is the measure a caller decides with (rtr_scene_rebuild below).
 * Defined on the quantised BVH2 (RtrBvhNode on RtrBvhGrid, what rtr_scene_export_bvh shows), in integers: for a child box,
 * d[a] = max(0, qmax[a] - qmin[a]) in grid steps and its area triple is (d.x d.y, d.y d.z, d.z d.x).  Over the nodes that are part of the
 * tree (a device build leaves slots of its node array unused; they are skipped):
 *   innerArea   every child slot that holds an inner node adds its triple; the root's own box — the union of its two child boxes in grid
 *               coordinates — adds its triple too
 *   leafArea    every child slot that holds a leaf adds count * triple, count = (code & 7) + 1
 *   rootArea    the root box's triple
 *   numInner    the inner nodes of the tree (the root included)      numLeafRefs    the child slots that hold a leaf
 * d <= 65535, count <= 8 and at most 2^25 nodes keep every sum below 2^61: the sums are exact and identical from run to run.  Then, in
 * double, in exactly this order, with (sx, sy, sz) = grid.scale and W(a) = a[0]*sx*sy + a[1]*sy*sz + a[2]*sz*sx:
 *   sah = (W(innerArea) * 1.0 + W(leafArea) * 1.0) / W(rootArea)        (0 where W(rootArea) is 0)
 * — the unit costs are the host builder's defaults, costTraverse = costIntersect = 1.  A scene of a single leaf stores it as both
 * children of the root, and it counts twice, as the formula says (the empty scene's one degenerate triangle is such a leaf: its box is
 * padded like every box, has an area on its own grid, and prices as 3).  The number prices the BVH2; the any-hit kernel walks the 4-wide view
 * made from it, and how well one predicts the other's frame time is a measurement (profiles/rebuild/rebuild_rate.json), not a promise.
 * rtr_scene_tree_cost: a device kernel (kernels/rtr_bvh.hip, k_tree_cost) over the scene's node array, enqueued on the scene's
 * context stream and joined before the words are read; it writes nothing a render reads, so it does not join the whole device, and it is
 * ordered behind the update calls, which return complete.  rtr_host_tree_cost: the host restatement, a walk from the root over `nodes`
 * (nodeBytes = a multiple of 32, at least one node; rtr_host_build_bvh or rtr_scene_export_bvh output) — the same integers, no device:
 * tree experiments price a refit on the CPU.  RTR_ERR_INVALID_ARGUMENT (with a message) for a null pointer, a nodeBytes that is 0 or
 * not a multiple of sizeof(RtrBvhNode), or a child index outside the array. */
typedef struct rtr_tree_cost {
    uint64_t innerArea[3], leafArea[3], rootArea[3];
    uint64_t numInner, numLeafRefs;
    double   sah;
} rtr_tree_cost;                           /* 96 bytes */
#ifdef __cplusplus
static_assert(sizeof(rtr_tree_cost) == 96 && alignof(rtr_tree_cost) == 8, "rtr_tree_cost is 96 B, 8-byte aligned");
#endif
int  rtr_scene_tree_cost(const rtr_scene* scene, rtr_tree_cost* out);
int  rtr_host_tree_cost(const RtrBvhNode* nodes, size_t nodeBytes, const RtrBvhGrid* grid, rtr_tree_cost* out);
/* Build the tree AGAIN, in place, from the vertices and transforms the scene has now — Vulkan's MODE_BUILD on a live acceleration
 * structure, where the update calls above are MODE_UPDATE.  buildFlags: RTR_BUILD_DEVICE_LBVH — the device build of rtr_scene_create,
 * fed from the scene's own device vertex and index arrays and its current instances (nothing goes through the host but the mirrors and
 * stats creation also reads back; its scratch is kept by the scene after the first such call and reused) — or RTR_BUILD_HOST_SAH —
 * vertices and indices are read back, the host builder runs as at creation and the result is uploaded: "the pose changed once, now trace
 * fast".  A scene of fewer than 16 triangles takes the host builder whatever the flag, as in rtr_scene_create.  The result is the tree
 * (nodes, records, 4-wide view, grid, stats) rtr_scene_create would make from rtr_scene_export_vertices' array with that flag, byte for
 * byte (tested); stats.sahCost is the host builder's number, or 0 after a device build, as at creation.
 * Everything else stays: textures, HDRI, LTC tables, vertices, indices, objects, light tables, the transform, normal-matrix and
 * mirrored tables, the instance masks (the new records carry them; the getter returns what was set), and every pointer a caller holds.
 * Frames created before the call render the new tree afterwards with no further step.  The triangle -> leaf table is DROPPED (the leaf
 * order changed) and remade by the next rtr_hit_leaves / rtr_light_rays_hinted under the first-use rule above; start hints a caller
 * made BEFORE the rebuild are stale, and, by the contract of the hinted calls, still safe: they change no byte of any answer, only the
 * work saved.  After a host rebuild the next update call prepares its refit arrays for the new tree, as after a host creation.
 * Synchronisation: as the other update calls (above): the call joins the whole device, rewrites, and returns when the new state is
 * complete.  The new tree is built into arrays of its own and swapped in only on success: a refused or failed build —
 * RTR_ERR_INVALID_ARGUMENT (with a message) for a null scene or a buildFlags above RTR_BUILD_DEVICE_LBVH, RTR_ERR_BVH_TOO_DEEP from a
 * build's depth check — leaves the scene as it was (HIP runtime errors excepted).  An empty scene returns RTR_OK and does nothing.
 * Scenes replicated by librtr_mgpu have no rebuild path, as they have no update path. */
int  rtr_scene_rebuild(rtr_scene* scene, uint32_t buildFlags);
/* The ENQUEUED rebuild: rtr_scene_rebuild with RTR_BUILD_DEVICE_LBVH as stream-ordered work, so that a frame loop that animates on the
 * device gets a good tree back every few frames without stopping.  The synchronous call joins the whole device, makes the primitive
 * tables in host loops, allocates a new tree, orders the 4-wide view in a host loop and reads the tree back; this form builds into a
 * STAGE — a second set of the build's arrays that nothing else reads — and lets the device decide the commit.
 * rtr_scene_prepare_async_rebuild: ONCE per scene, synchronous; may join and allocate.  It implies (and calls)
 * rtr_scene_prepare_async_updates, and allocates the stage (nodes, fp32 nodes, grid, records, leaf boxes, parent links, the primitive ->
 * slot map, the reduction words: 184 B per triangle) and the device build's scratch (112 B per triangle and the sort's temporary
 * storage; the scratch the first synchronous device rebuild allocates, and shared with it) — some 300 B per triangle, kept for the
 * scene's life.  The commit copies into the live arrays IN PLACE, so they must have a device build's sizes: the scene's current tree must
 * have been made by RTR_BUILD_DEVICE_LBVH (at creation or by rtr_scene_rebuild) from at least 16 triangles; otherwise
 * RTR_ERR_INVALID_ARGUMENT, and the message names rtr_scene_rebuild(scene, RTR_BUILD_DEVICE_LBVH) as the way to get there.  Idempotent; an
 * empty scene returns RTR_OK.  A synchronous rtr_scene_rebuild of a prepared scene prepares the new tree by itself when that is a device
 * tree; after a HOST rebuild the readiness is gone and the enqueued call is refused until a synchronous device rebuild gives the scene a
 * device tree again (which prepares it, without a call).
 * rtr_scene_rebuild_async: buildFlags must be RTR_BUILD_DEVICE_LBVH (RTR_BUILD_HOST_SAH — the host builder is host code — and anything
 * above are refused).  Argument checks and launches only: no allocation, no synchronisation, no device -> host copy, no copy from
 * reusable host memory, everything on the scene's context stream — ORDERING as documented for rtr_scene_update_vertices_async.  Refused
 * BEFORE anything is enqueued (RTR_ERR_INVALID_ARGUMENT, the message names the function): a null scene, bad flags (checked before the
 * scene is looked at), a scene not prepared for it.  An empty scene returns RTR_OK, counts as enqueued and does nothing.  The chain:
 *   the device build  rtr_scene_create's kernels in their order, into the stage, from the LIVE device tables (primitives, instances with
 *                     their current transforms, the instance masks in the flags: current after enqueued instance updates and after
 *                     rtr_scene_set_instance_masks) and the scene's vertex and index arrays.  It writes nothing a render or query reads.
 *   the commit        one kernel (k_commit_tree) reads the staged tree's depth.  THE ONE REFUSAL RULE: the scene's render kernels are
 *                     specialised on the host for a traversal-stack class — 16, 32 or 64 entries, stats.stackEntries — and the host
 *                     cannot learn a new depth without a join; so a tree DEEPER than stats.stackEntries at the time of the call is
 *                     refused: the depth goes into the update word and nothing is copied.  Otherwise every staged array is copied over
 *                     its live twin, all of it or none.  A tree that fits a SMALLER class is committed and stats.stackEntries keeps its
 *                     value: a larger stack is always correct and changes no byte of any answer; an enqueued rebuild never lowers it
 *                     (the next synchronous rtr_scene_rebuild does).  A device tree is never deeper than 64.
 *   the 4-wide view   of the live arrays, its breadth-first order on the device, the permutation; the triangle -> leaf table, if the
 *                     scene has one, is made again in place (it stays ready and current; a scene that never asked for it gets it on
 *                     first use, as always); the status fold with this call's serial.  After a refused commit these run on the
 *                     unchanged tree and reproduce its bytes, as after a refused update.
 * The result is the synchronous call's, byte for byte (tested) — tree, records, grid, 4-wide view, tree cost, stats.maxDepth at the next
 * read-back — except stats.stackEntries as said, and stats.buildMs, which keeps its old value: nobody timed the build.  The contract of
 * rtr_scene_rebuild otherwise holds: textures, tables, vertices, masks, frames made before the call; every pointer a caller holds stays
 * literally the same, because nothing is swapped.  Start hints made before the call are stale and, by the hinted calls' contract, change
 * no byte.  STATUS and HOST MIRRORS: as the enqueued updates (rtr_update_status above; for a refused rebuild firstBadVertex is the
 * refused tree's depth).  Scenes replicated by librtr_mgpu have no enqueued rebuild, as they have no update path. */
int  rtr_scene_prepare_async_rebuild(rtr_scene* scene);
int  rtr_scene_rebuild_async(rtr_scene* scene, uint32_t buildFlags);
/* The REBUILD POLICY on the device: rtr_scene_rebuild_async behind a decision the device makes, so that a frame loop on a stream neither
 * rebuilds blindly every N frames nor stops once a frame to look at rtr_scene_tree_cost.  The device evaluates the cost of the live tree,
 * compares it with the cost right after the last build, and builds only when the comparison says so.
 * rtr_scene_prepare_async_rebuild_if: ONCE per scene, synchronous; may join and allocate.  It implies (and calls)
 * rtr_scene_prepare_async_rebuild — the same refusals, the same messages — and allocates the policy's device memory: the eleven words of
 * the cost kernel and one record of the fields below with the decision word.  builtSah, the BASELINE, is set to the cost of the tree as
 * it is at this call: exactly rtr_scene_tree_cost's sah.  Idempotent: a second call does not move the baseline.  An empty scene returns
 * RTR_OK.
 * rtr_scene_rebuild_if_async: argument checks and launches only — no allocation, no synchronisation, no device -> host copy, no copy from
 * reusable host memory, everything on the scene's context stream; ORDERING as documented for rtr_scene_update_vertices_async.  Refused
 * BEFORE anything is enqueued (RTR_ERR_INVALID_ARGUMENT, the message names the function), in this order: a null scene; buildFlags, as
 * rtr_scene_rebuild_async checks it (before the scene is looked at); a rebuildAbove that is NaN or negative (likewise; +inf is allowed and
 * means "never", 0.0 means "whenever the cost is positive"); a scene not prepared (the message names
 * rtr_scene_prepare_async_rebuild_if).  An empty scene returns RTR_OK, counts as enqueued and does nothing.  The call takes the next serial
 * of the one sequence of rtr_update_status: a skipped rebuild is an enqueued update that was not refused.  The chain:
 *   cost      the sums of rtr_scene_tree_cost over the live tree, into the policy's words.
 *   decide    one lane: sah from the words and the live grid's scale, by the very function the host uses (bit for bit rtr_scene_tree_cost's
 *             sah at that point of the stream); lastSah = sah, evaluated += 1, lastDecision = go = sah > rebuildAbove * builtSah, in double.
 *   the build, the commit, the 4-wide view and the leaf table of rtr_scene_rebuild_async, every kernel of them GATED by the decision
 *             word: with go == 0 each returns at once, and no byte a render, a query or a hint reads is written (the build's sort,
 *             which runs regardless, touches scratch only).  With go == 1 they are rtr_scene_rebuild_async's, with its
 *             one refusal rule: a staged tree deeper than stats.stackEntries puts its depth into the update word, copies nothing and counts
 *             as a refused update; the tail then runs on the unchanged tree.
 *   close     when the commit copied: the cost of the new live tree, builtSah = its sah, rebuilt += 1.  Then the status fold.
 * THE BASELINE FOLLOWS EVERY BUILD of a prepared scene: rtr_scene_rebuild_async gets the close (without counting in `rebuilt`), predicated on
 * its own commit; a synchronous rtr_scene_rebuild that gives the scene a device tree prepares the policy again by itself, builtSah being
 * the new tree's cost, while evaluated and rebuilt keep counting.  After a HOST rebuild the readiness is gone, as for
 * rtr_scene_rebuild_async, and comes back with the next synchronous device rebuild.  HOST MIRRORS: stale after the call, exactly as after
 * rtr_scene_rebuild_async — the host cannot know whether the tree changed.
 * rtr_scene_rebuild_if_status: joins the scene's context stream (only that) and copies the record out.  A scene never prepared reports
 * zeros and lastDecision = 0xffffffff.  It does not touch rtr_update_status's "first since the last status call" words.
 * Scenes replicated by librtr_mgpu have no such call, as they have no update path. */
typedef struct rtr_rebuild_if_status {
    uint64_t evaluated;     /* rtr_scene_rebuild_if_async calls whose decision kernel has run, since preparation */
    uint64_t rebuilt;       /* of those, how many built AND committed a new tree */
    double   builtSah;      /* the baseline: sah of the tree right after its last build */
    double   lastSah;       /* the sah the last decision looked at (the refitted tree's); 0 before the first */
    uint32_t lastDecision;  /* 1: the last call built, 0: it skipped, 0xffffffff: none yet */
    uint32_t _pad[3];
} rtr_rebuild_if_status;                   /* 48 bytes */
#ifdef __cplusplus
static_assert(sizeof(rtr_rebuild_if_status) == 48, "rtr_rebuild_if_status is 48 B");
#endif
int  rtr_scene_prepare_async_rebuild_if(rtr_scene* scene);
int  rtr_scene_rebuild_if_async(rtr_scene* scene, uint32_t buildFlags, double rebuildAbove);
int  rtr_scene_rebuild_if_status(rtr_scene* scene, rtr_rebuild_if_status* out);
/* Instance cull masks: VkAccelerationStructureInstanceKHR::mask (reference src/vulkan/raytracing/tlas.cppm:63, instance.setMask(0xFF): the
 * only value the reference uses).  masks: a HOST array, one byte per instance, in instance order (rtr_scene_desc::instances); every new
 * scene — one made by rtr_scene_create_like too — starts with 0xff everywhere.  Only the MASKED ray queries (rtr_trace_rays_masked,
 * rtr_trace_occlusion_masked) look at the masks: rtr_render and every other entry point IGNORE them and give the bytes they gave before
 * the call (tested).  The masks live in the triangle records (RtrBvhTri::flags bits 8..15, complemented: rtr_types.h), which a kernel
 * rewrites; rtr_scene_export_bvh shows them, and a scene that never called the setter exports the records it always did.  They survive
 * rtr_scene_update_instances.  The setter rewrites a device array that queries read, so it synchronises as the update calls do: it first
 * JOINS THE WHOLE DEVICE (hipDeviceSynchronize: every query and frame in flight on any stream of this process finishes with the old
 * masks), rewrites, and returns when the new state is complete; safe to call at any time from the thread that enqueues the work, and a
 * caller that uses the scene from other threads or processes must itself keep those from enqueueing until the call has returned.
 * RTR_ERR_INVALID_ARGUMENT for a null pointer or a numInstances that is not the scene's.  The getter returns what was set (0xff if never). */
int  rtr_scene_set_instance_masks(rtr_scene* scene, const uint8_t* masks, uint32_t numInstances);
int  rtr_scene_get_instance_masks(const rtr_scene* scene, uint8_t* masks, uint32_t numInstances);
/* replaces the host-visible LightInfo buffer rewrite (src/app/application.cppm:264-271). */
int  rtr_scene_update_lights(rtr_scene* scene, const RtrAreaLightInfo* lights, uint32_t numLights);

/* ---- frame ---------------------------------------------------------------------------- */
/* replaces the 8 storage images (src/app/application.cppm:108-138).  `rows` is the number of
 * LOCAL rows (== height when unsharded; see rtr_shard_rows).  `images` is a RTR_IMG_BIT mask. */
int  rtr_frame_create(rtr_ctx* ctx, uint32_t width, uint32_t rows, uint32_t images, rtr_frame** out);
void rtr_frame_destroy(rtr_frame* frame);
/* Let an RGBA8 image of this frame live in caller-owned device memory (e.g. a torch tensor that
 * RCCL will gather).  bytes must be width*rows*4. */
int  rtr_frame_bind_external(rtr_frame* frame, int which, void* devicePtr, size_t bytes);
int  rtr_frame_device_ptr(const rtr_frame* frame, int which, void** devicePtr, size_t* bytes);
/* replaces the image->swapchain copy / readback (src/app/application.cppm:450-457). */
int  rtr_frame_download(const rtr_frame* frame, int which, void* dst, size_t bytes);
int  rtr_frame_clear(rtr_frame* frame);
int  rtr_frame_get_stats(const rtr_frame* frame, rtr_frame_stats* out);

/* Number of local rows a shard owns: `height` when unsharded, otherwise ceil(bands / shardCount) * bandRows so
 * every shard has the same count (equal-size shards for the gather; padding rows stay zero). */
uint32_t rtr_shard_rows(uint32_t height, uint32_t bandRows, uint32_t shardCount);

/* ---- dispatch ------------------------------------------------------------------------- */
/* replaces bind pipeline + push constants + vkCmdTraceRaysKHR + waitIdle
 * (src/app/application.cppm:362-389, src/vulkan/ray_tracing_pipeline.cppm:212-214). Synchronous. */
int  rtr_render(rtr_scene* scene, const RtrCameraData* camera, const RtrSceneInfo* sceneInfo,
                const rtr_render_params* params, rtr_frame* frame);
/* Asynchronous variant: enqueues on the stream of the FRAME's context and returns; rtr_frame_wait() joins.  The scene
 * may belong to another context of the same device (it is read-only during rendering), so frames created on
 * different contexts render concurrently on their own streams against one scene. */
int  rtr_render_async(rtr_scene* scene, const RtrCameraData* camera, const RtrSceneInfo* sceneInfo,
                      const rtr_render_params* params, rtr_frame* frame);
/* Several frames in ONE launch of every kernel of the pipeline: cameras[b] / sceneInfos[b] -> frames[b], b < n <= RTR_MAX_BATCH, all
 * with the same params (extent, spp, sharding, images; accumulate applies to each frame's own HDR image).  A frame at 1 spp — and
 * a 1/N shard of one even more so — is too little work per launch for the latency-bound kernels (the camera-ray kernel takes
 * 0.34 ms for one 1080p frame's rays and 0.41 ms for four times as many): batching trades latency of the individual frame for
 * throughput, like frames in flight do, and composes with them.  Same pixels as n calls of rtr_render_async (tested).  The
 * launch runs on frames[0]'s context stream and its times / counters (rtr_frame_get_stats) are frames[0]'s, for the whole launch;
 * rtr_frame_wait on any of the frames joins it.  The other frames may live on other contexts (streams) of the device: the launch waits
 * for what their streams hold when it is enqueued and their streams wait for the launch, so work enqueued for a frame before and
 * after a batch is ordered around it without a host join (tested).  Staged pipeline only; the frames must live on one device and be distinct.
 * The reference records one vkCmdTraceRaysKHR per frame (src/app/application.cppm:362-389); this is n of them in one. */
#define RTR_MAX_BATCH 32
int  rtr_render_batch_async(rtr_scene* scene, const RtrCameraData* cameras, const RtrSceneInfo* sceneInfos, const rtr_render_params* params,
                            rtr_frame* const* frames, uint32_t n);
/* The LATENCY form: ONE frame as `parts` (<= RTR_MAX_SPLIT) band-shards — bands of params->bandRows rows, band b to part b mod parts,
 * the sharding of the multi-GPU path — each on a stream of its own inside the library, all writing their rows of `frame`'s images in
 * place (no gather: `frame` is the whole frame, rows == height).  The kernels of a frame are a dependency chain and each ends in a
 * tail; split, part k+1's camera rays and queue build run under part k's traversal.  Same pixels as rtr_render (tested), stream-ordered
 * on the frame's context stream like rtr_render_async (fork and join are events); rtr_frame_wait joins, and rtr_frame_get_stats then
 * gives totalMs = the frame's duration, fork to join, and the counters and per-kernel times SUMMED over the parts (they overlap).
 * params->shardCount must be 0 or 1.  parts == 1 is rtr_render_async.  What the reference's loop needs — one frame per iteration, then
 * waitIdle (src/app/application.cppm:352-389,437) — where rtr_render_batch_async trades that latency for throughput. */
#define RTR_MAX_SPLIT 16
int  rtr_render_split_async(rtr_scene* scene, const RtrCameraData* camera, const RtrSceneInfo* sceneInfo, const rtr_render_params* params,
                            rtr_frame* frame, uint32_t parts);
int  rtr_render_split(rtr_scene* scene, const RtrCameraData* camera, const RtrSceneInfo* sceneInfo, const rtr_render_params* params,
                      rtr_frame* frame, uint32_t parts);
/* How many frames of these params one launch takes: min(RTR_MAX_BATCH, what the staged pipeline's scratch can address — its
 * visibility slots are 31-bit indices: pixel-sample slots of the launch, rounded up to a power of two, x queries per pixel-sample).
 * 1 when only a single frame fits (or the megakernel is asked for); a caller that batches asks this first.  Pure arithmetic. */
int  rtr_render_batch_limit(const rtr_scene* scene, const rtr_render_params* params, uint32_t numAreaLights, uint32_t* maxFrames);
int  rtr_frame_wait(rtr_frame* frame);

/* The passes that follow the ray-gen dispatch in the reference's frame loop (src/app/application.cppm:391-445):
 * `iterations` (reference: NUM_DENOISING_ITERATIONS = 4) rounds of {a-trous pass on the unshadowed image, then on the
 * shadowed image} ping-ponging between the sampled (1,2) and denoised (3,4) images with step (i+1), c_phi 1,
 * n_phi = p_phi = 1e-3 (src/shaders/denoise.comp), then combine.comp: FINAL = ANALYTIC * shadowed / max(unshadowed, .001)
 * reading the pair the ping-pong flag points at.  The frame must own images 0-7 and hold a full (unsharded) frame
 * rendered with RTR_IMAGES_RAYGEN5.  Synchronous. */
int  rtr_denoise_combine(rtr_frame* frame, int iterations);
/* The same checks, launches and ping-pong, ENQUEUED on the stream of the frame's context and not waited for: it comes behind a
 * render of the frame on that stream and behind an rtr_render_batch_async launch that rendered it on another frame's stream, and a
 * later batch comes behind it — all without a host join.  rtr_frame_wait joins.  With two frames on two contexts, the post passes of
 * frame n run while frame n+1 is rendered (the frame the reference presents, two in flight). */
int  rtr_denoise_combine_async(rtr_frame* frame, int iterations);

/* Rank-0 step after the RCCL gather: `gathered` holds shardCount blocks of (localRows x width)
 * RGBA8 pixels in rank order; writes the de-interleaved (height x width) image to `dst`.
 * Both are device pointers; ENQUEUED on the ctx stream (asynchronous; synchronise the stream to read). */
int  rtr_deinterleave_bands(rtr_ctx* ctx, const void* gathered, void* dst, uint32_t width, uint32_t height,
                            uint32_t bandRows, uint32_t shardCount);
/* The same for several images in ONE launch (librtr_mgpu.so's present mode): `gathered` holds shardCount blocks, each of numImages
 * planes of (localRows x width) RGBA8 pixels — [shard][image][localRow][x], localRows = rtr_shard_rows(height, bandRows, shardCount) —
 * and image i is de-interleaved into dst[i] (height x width).  Same band -> shard map as rtr_deinterleave_bands.  ENQUEUED on the ctx
 * stream.  RTR_ERR_INVALID_ARGUMENT for 0 or more than 8 images, a null pointer, or a bandRows that is not a multiple of 8 (0 -> 8). */
int  rtr_deinterleave_images(rtr_ctx* ctx, const void* gathered, uint32_t numImages, void* const* dst, uint32_t width,
                             uint32_t height, uint32_t bandRows, uint32_t shardCount);

/* ---- ray queries ---------------------------------------------------------------------- */
/* The traversal of the renderer for rays the CALLER makes: what traceRayEXT does for raygen.rgen, without the fixed shaders.
 * Flags (bit mask):
 *   RTR_QUERY_CLOSEST  the closest hit: the (t, customIndex, primitiveId)-minimal one with tmin < t < tmax — gl_RayFlagsNoneEXT
 *                      (reference src/shaders/raygen.rgen:99-107, the camera rays: tmin 0.001, tmax 10000).  Writes hits[].
 *   RTR_QUERY_ANY      terminate on the first accepted hit and report only whether there is one (occluded[] = 1, else 0) —
 *                      gl_RayFlagsTerminateOnFirstHitEXT | gl_RayFlagsSkipClosestHitShaderEXT (raygen.rgen:226-231, :299-303, the
 *                      shadow rays).  Which triangle the walk meets first depends on the walk, so no hit record is defined.
 *   RTR_QUERY_OPAQUE   skip the opacity-map test (opacity.rahit:31-64) as gl_RayFlagsOpaqueEXT does; without it alpha-tested
 *                      geometry is treated exactly as the renderer treats it.
 * Culling flags, with Vulkan's own bit values (bit values 4, 8 and everything above 0x80 are refused).  They are per launch and are
 * taken by every query entry point that has `flags`: rtr_trace_rays[_masked][_async], rtr_trace_occlusion[_hinted|_masked][_async].
 *   RTR_QUERY_CULL_BACK_FACING / RTR_QUERY_CULL_FRONT_FACING   gl_RayFlagsCullBackFacingTrianglesEXT / ...CullFrontFacing...: a triangle
 *                      is FRONT-facing for a ray iff the ray arrives on the side its as-wound geometric normal points to — the normal
 *                      rtr_hit_surfaces reports as RtrSurface::geomNormal = normalize(nmat * cross(p1 - p0, p2 - p0)).  Facing is decided
 *                      in object space, as in Vulkan, so a mirrored instance (negative determinant of its 3x3 transform) does not change
 *                      it.  In the kernels' arithmetic: with a = rtr_dot(e1, rtr_cross(d, e2)), the fp32 determinant rtr_mt_intersect
 *                      computes on the world-space record, front = (a > 0) XOR mirrored(instance).  An accepted hit has
 *                      |a| >= RTR_MT_EPSILON, so the sign is never ambiguous and every walk gives the same answer.  mirrored() is
 *                      evaluated on the host, in double, by rtr_scene_create, rtr_scene_create_like and rtr_scene_update_instances (it
 *                      follows a refit) and kept in a per-customIndex device table beside the transforms, NOT in the triangle records:
 *                      their bytes are what they were.  Light instances follow the same rule (so a one-sided emitter,
 *                      RtrAreaLightInfo::isTwoSided == 0, can be passed through from behind).
 *   RTR_QUERY_CULL_OPAQUE / RTR_QUERY_CULL_NO_OPAQUE   gl_RayFlagsCullOpaqueEXT / gl_RayFlagsCullNoOpaqueEXT: a record is NON-OPAQUE iff
 *                      its flags bit 0 (alpha-tested) is set and RTR_QUERY_OPAQUE is not given, otherwise opaque; CULL_OPAQUE drops the
 *                      opaque records, CULL_NO_OPAQUE the non-opaque ones: a caller traces only the alpha-tested layer, or only the rest.
 * Refused (RTR_ERR_INVALID_ARGUMENT, the message names the flags), as Vulkan forbids them: both face flags together; more than one of
 * RTR_QUERY_OPAQUE, RTR_QUERY_CULL_OPAQUE and RTR_QUERY_CULL_NO_OPAQUE.
 * Order, as in Vulkan: culling comes before the any-hit shader — a culled record runs no opacity-map test and adds nothing to
 * numAlphaTests; it was fetched, so it counts in numTriTests (as a record the cull mask drops does).  The closest hit is the
 * (t, customIndex, primitiveId)-minimal hit among the records that survive the cull mask, the facing cull, the opacity cull and the
 * opacity-map test; an occlusion byte is 1 iff such a record exists, the same byte on every route (dense any-hit, queued, queued with
 * hints: a hinted leaf whose hits are all culled does not stop the ray), and the rays finished over the BVH2 honour the flags too.
 * Without these bits every entry point launches the kernels it launched before, with the same results and counters; a call that has
 * them launches the filtered (cull-mask) forms of the kernels, with mask 0xff where the call brings none.  rtr_render ignores all of it. */
#define RTR_QUERY_CLOSEST 0u
#define RTR_QUERY_ANY     1u
#define RTR_QUERY_OPAQUE  2u
#define RTR_QUERY_CULL_BACK_FACING  0x10u   /* gl_RayFlagsCullBackFacingTrianglesEXT  */
#define RTR_QUERY_CULL_FRONT_FACING 0x20u   /* gl_RayFlagsCullFrontFacingTrianglesEXT */
#define RTR_QUERY_CULL_OPAQUE       0x40u   /* gl_RayFlagsCullOpaqueEXT               */
#define RTR_QUERY_CULL_NO_OPAQUE    0x80u   /* gl_RayFlagsCullNoOpaqueEXT             */

typedef struct rtr_query_stats {
    /* exact work counters of the query (the counting form of the kernels), counted as rtr_frame_stats counts the renderer's camera
     * rays: a ray that outgrew the 16-entry LDS stack and was walked again over the BVH2 counts once, its two walks both */
    uint64_t numRays;
    uint64_t numNodeVisits;
    uint64_t numTriTests;
    uint64_t numAlphaTests;
    uint64_t tailRays;         /* rays walked again by the tail kernel */
    float    ms;               /* the query's kernels, HIP events on the context stream */
    uint32_t _pad;
} rtr_query_stats;

/* numRays rays[] against `scene`, results in hits[] (RTR_QUERY_CLOSEST) or occluded[] (RTR_QUERY_ANY).  rays, hits and occluded are
 * DEVICE pointers (torch tensors, hipMalloc), 16-B aligned; the pointer the mode does not use may be NULL and is not touched.  The work
 * is ENQUEUED on ctx's stream (rtr_ctx_set_stream) and not waited for; the scene may belong to another context of the same device, as
 * in rtr_render_async.  A ray with !(tmax > tmin), or whose origin or direction is not finite or whose direction is zero, is a miss.
 * numRays == 0 does nothing.  RTR_ERR_INVALID_ARGUMENT (with a message) for a null pointer the mode needs, a pointer that is not
 * 16-B aligned, unknown flag bits or a scene on another device.  The context keeps a small scratch area for the rays that need a deeper
 * stack (bounded, whatever numRays is); calls on one context are ordered on its stream. */
int  rtr_trace_rays_async(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, uint32_t numRays, uint32_t flags,
                          RtrHit* hits, uint8_t* occluded);
/* The same, then joins ctx's stream (only that stream).  stats (may be NULL): run the counting form of the kernels and fill it. */
int  rtr_trace_rays(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, uint32_t numRays, uint32_t flags,
                    RtrHit* hits, uint8_t* occluded, rtr_query_stats* stats);
/* ---- cull masks: traceRayEXT's cullMask argument (reference src/shaders/raygen.rgen:102,234,306, always 0xFF there) ----
 * Vulkan's rule: an instance's triangles exist for a ray iff (instanceMask & rayMask) != 0, with the instance masks of
 * rtr_scene_set_instance_masks (default 0xff) and the ray's EFFECTIVE mask cullMask & (rayMasks ? rayMasks[k] : 0xff).  cullMask: 8 bits;
 * higher bits are refused (RTR_ERR_INVALID_ARGUMENT, with a message).  rayMasks: a DEVICE pointer, one byte per ray, no alignment asked,
 * or NULL: one launch can carry rays of different kinds (bounce rays that skip the emitters beside probe rays that see one layer), as one
 * Vulkan dispatch does.  A ray whose effective mask is 0 is a miss (t = its tmax) / not occluded and costs no walk.  Everything else is
 * the unmasked call's: the closest hit is the (t, customIndex, primitiveId)-minimal ACCEPTED hit, RTR_QUERY_ANY / RTR_QUERY_OPAQUE, the
 * opacity-map test (not run on a masked-out record), tmin / tmax, degenerate rays, pointers, alignment, stream order, numRays == 0, a
 * scene on another context of the same device.  stats: as rtr_trace_rays; numTriTests counts FETCHED records, so a masked-out record
 * counts (a box whose triangles are all masked out is still entered: the mask is a filter in the leaves, not a culled subtree).  With
 * default instance masks, cullMask 0xff and rayMasks NULL, results and every counter equal the unmasked call's.  The unmasked entry
 * points launch the unmasked forms of the kernels, whose instructions are what they were. */
int  rtr_trace_rays_masked_async(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const uint8_t* rayMasks, uint32_t numRays,
                                 uint32_t flags, uint32_t cullMask, RtrHit* hits, uint8_t* occluded);
int  rtr_trace_rays_masked(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const uint8_t* rayMasks, uint32_t numRays,
                           uint32_t flags, uint32_t cullMask, RtrHit* hits, uint8_t* occluded, rtr_query_stats* stats);
/* ---- multi-hit queries: the first K hits along a ray, in order, resumable ----
 * What a Vulkan caller builds from an any-hit shader that records a hit and ignores it: MORE than the nearest surface along a ray —
 * transmission through layers, thickness and exit-face probes, X-ray and CSG picking, inside/outside by crossing parity, a robust way past
 * a coincident surface.  One dense route: one ray per lane over the BVH2, the sibling of rtr_trace_rays_masked(RTR_QUERY_CLOSEST).
 * ACCEPTED SET.  The set of ray k is exactly the records rtr_trace_rays_masked(RTR_QUERY_CLOSEST, the same flags, cullMask and rayMasks)
 * would consider: those that pass the cull mask, the opacity cull, rtr_mt_intersect with the ray's tmin, t < tmax, the facing cull and the
 * opacity-map test (unless RTR_QUERY_OPAQUE) — in that order, counted the same way.  A degenerate ray (as in rtr_trace_rays) and a ray
 * whose effective mask is 0 have an empty set and walk nothing.
 * RESULT.  hits has numRays * maxHits records, ray-major: ray k's j-th hit is hits[k * maxHits + j].  The count = min(maxHits, |set|)
 * smallest members by (t, customIndex, primitiveId) — t as float, the ids unsigned: the total order of the closest-hit rule — go,
 * ascending, into slots 0 .. count-1.  Every slot j >= count is the miss record rtr_trace_rays writes for that ray: t = the ray's own tmax
 * bits, u = v = 0, both ids 0xffffffff, pad words 0.  counts[k] = count where counts is given.  EVERY slot of every ray is written.
 * K = 1.  With maxHits == 1 and after == NULL the bytes of hits are those of rtr_trace_rays_masked(..., RTR_QUERY_CLOSEST, ...), and so
 * are the work counters (numRays, numNodeVisits, numTriTests, numAlphaTests, tailRays): the walk is the closest-hit walk whose far limit
 * stays tmax until maxHits hits are held and is then the t of the LAST of them, which at 1 is the closest-hit walk itself.
 * RESUME.  after (may be NULL): one RtrHit per ray.  If after[k].customIndex is 0xffffffff ray k is EXHAUSTED: count 0, all slots miss
 * records, no walk.  Otherwise only members whose key is STRICTLY greater than after[k]'s (t, customIndex, primitiveId) are reported; tmin
 * applies unchanged.  A caller passes the previous call's LAST slot of every ray, hits[k * maxHits + maxHits - 1] (gathered into an array of
 * its own: after must not overlap hits): a miss record there says the ray has no more, a hit says where to go on.  Chained calls then
 * enumerate a ray's hits exactly once each — exact ties in t included, which re-tracing from t + epsilon skips or repeats — for any
 * maxHits.  The scene must not change between the calls of a chain (no update, refit, rebuild or mask change): the keys are compared
 * bit for bit.
 * FLAGS.  RTR_QUERY_OPAQUE and the four RTR_QUERY_CULL_* bits, with the refusals of every query (both face flags; more than one of
 * OPAQUE / CULL_OPAQUE / CULL_NO_OPAQUE; bit values 4, 8 and above 0x80).  RTR_QUERY_ANY is refused: an any-hit walk has no order.
 * cullMask above 8 bits is refused; maxHits == 0 and maxHits > RTR_MULTIHIT_MAX are refused.
 * POINTERS.  rays, rayMasks, after, hits and counts are DEVICE pointers; rays, after and hits 16-B aligned, counts 4-B aligned; rayMasks,
 * after and counts may be NULL.  Null, misaligned or other-device arguments are refused as in rtr_trace_rays (RTR_ERR_INVALID_ARGUMENT,
 * with a message); numRays == 0 does nothing.  A refused call writes nothing.
 * STREAM ORDER.  Enqueued on ctx's stream; uses the context's fixed query scratch (redo list, control words, spill stacks: a ray that
 * outgrows the 16-entry stack is walked again from scratch by a tail kernel, and counts in tailRays).  Apart from that scratch's first
 * use there is no allocation, no join and no copy back, so a chain can be enqueued whole.  rtr_render and every other query are
 * untouched: they launch the kernels they launched. */
#define RTR_MULTIHIT_MAX 8u
int  rtr_trace_rays_multi_async(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const uint8_t* rayMasks, uint32_t numRays,
                                uint32_t maxHits, uint32_t flags, uint32_t cullMask, const RtrHit* after, RtrHit* hits, uint32_t* counts);
/* The same, then joins ctx's stream (only that stream).  stats (may be NULL): run the counting form of the kernels and fill it. */
int  rtr_trace_rays_multi(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const uint8_t* rayMasks, uint32_t numRays,
                          uint32_t maxHits, uint32_t flags, uint32_t cullMask, const RtrHit* after, RtrHit* hits, uint32_t* counts,
                          rtr_query_stats* stats);
/* ---- queued occlusion queries ----
 * A second way to answer occlusion rays, with the renderer's own any-hit machinery: the rays are binned by direction octant into a
 * queue of ray indices, persistent waves walk the 4-wide tree and refill their finished lanes from it, and the few rays that need a
 * deeper stack are finished over the BVH2.  occluded[k] is BYTE FOR BYTE what rtr_trace_rays(..., RTR_QUERY_ANY | the same
 * RTR_QUERY_OPAQUE bit) writes for the same rays — every k < numRays is written, 0 or 1; a null ray, a ray with !(tmax > tmin) or
 * with a non-finite origin or direction or a zero direction is 0 and costs no walk; every ray's own tmin is honoured — only the work is
 * scheduled differently: worth it for long arrays of incoherent rays (the light rays of a frame), not for a handful.
 * flags: 0 or RTR_QUERY_OPAQUE; RTR_QUERY_ANY is accepted and ignored (the query is any-hit by nature); other bits are refused.
 * The queue lives in SCRATCH THE CALLER OWNS: rtr_occlusion_scratch_bytes(numRays) bytes of device memory (a multiple of 16, monotone
 * in numRays; pure arithmetic, no device is touched), 16-B aligned, free for reuse once the query has run; it need not be initialised
 * and nothing is kept in it between calls.  Beside it the call uses the context's small fixed-size query scratch (the deep stacks and
 * the counters rtr_trace_rays uses, allocated by the context's first query of either kind); apart from that first use it allocates
 * nothing and never joins the host.  rays, occluded: DEVICE pointers, 16-B aligned.  ENQUEUED on ctx's stream; calls on one context
 * are ordered on its stream; the scene may belong to another context of the same device.  numRays == 0 does nothing.
 * RTR_ERR_INVALID_ARGUMENT (with a message) for a null or misaligned pointer the call needs, a scratch smaller than
 * rtr_occlusion_scratch_bytes(numRays), unknown flag bits or a scene on another device. */
int  rtr_occlusion_scratch_bytes(uint32_t numRays, size_t* bytes);
int  rtr_trace_occlusion_async(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, uint32_t numRays, uint32_t flags,
                               void* scratch, size_t scratchBytes, uint8_t* occluded);
/* The same, then joins ctx's stream (only that stream).  stats (may be NULL): run the counting form of the kernels and fill it:
 * numRays = the well-formed rays (finite origin and direction, direction not zero), whether their interval is empty or not — what
 * rtr_frame_stats counts as shadow rays when the rays are rtr_light_rays'; null rays are not counted.  numNodeVisits = 4-wide
 * record visits + the BVH2 visits of the tailRays rays that were walked again; numTriTests, numAlphaTests: both walks.  For the light
 * rays of a frame's camera hits these are the renderer's any-hit counters with the tunable trace_own_leaf = 0.  ms: queue build, walk
 * and tail together. */
int  rtr_trace_occlusion(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, uint32_t numRays, uint32_t flags,
                         void* scratch, size_t scratchBytes, uint8_t* occluded, rtr_query_stats* stats);
/* ---- start hints: the renderer's own-leaf rule for the queued query ----
 * The renderer's any-hit walk starts a shadow ray that leaves its surface point INTO the surface (dot(hitNormal, lightVec) < 0) at the
 * leaf of the triangle it starts on, the root waiting on the stack: 0.01 above that triangle it nearly always re-enters it, and the leaf
 * answers without a record visit (the tunable trace_own_leaf).  An RtrRay carries no leaf, so the caller passes it beside the ray.
 * A HINT is an int32_t.  Negative: a leaf child code as in RtrBvhNode / RtrWideNode — code = ~hint, first = code >> 3, count =
 * (code & 7) + 1, indexing the leaf-ordered triangle array — and the walk tests that leaf first, then walks from the root.  0: no hint,
 * the walk starts at the root.  ANYTHING ELSE COUNTS AS 0: a positive value, 0x80000000, a code whose first + count exceeds the scene's
 * triangle records; no value makes the walk read outside the triangle array.  Any-hit is a pure function of the ray and the triangles, so
 * a hint — right, wrong or another triangle's — changes the work and never a byte: occluded[] is rtr_trace_rays(RTR_QUERY_ANY)'s.
 * Hints come from the scene's triangle -> leaf table: for every (customIndex, primitiveId) of the scene the child code of the leaf that
 * holds that world-space record.  The table is NOT part of rtr_scene_create: THE FIRST CALL of rtr_hit_leaves or rtr_light_rays_hinted
 * (either form) on a scene ALLOCATES it (4 B per triangle + 4 B per instance) and fills it on ctx's stream, which that one call joins;
 * every later call, from any context of the device, finds it complete.  It survives rtr_scene_update_instances (a refit keeps topology
 * and leaf order); a scene made by rtr_scene_create_like makes its own.
 *
 * leaves[k] = the table's entry for hits[k] (customIndex, primitiveId): light instances are in the tree, so light hits get theirs; a miss
 * or ids out of range give 0 and read nothing.  For callers who make their own rays from a hit (transmission, a probe below a surface).
 * hits (16-B aligned) and leaves (4-B aligned) are DEVICE pointers; ENQUEUED on ctx's stream (apart from the first use, above); the
 * scene may belong to another context of the same device.  numHits == 0 does nothing.  RTR_ERR_INVALID_ARGUMENT (with a message) for a
 * null or misaligned pointer or a scene on another device. */
int  rtr_hit_leaves_async(rtr_ctx* ctx, const rtr_scene* scene, const RtrHit* hits, uint32_t numHits, int32_t* leaves);
/* The same, then joins ctx's stream (only that stream). */
int  rtr_hit_leaves(rtr_ctx* ctx, const rtr_scene* scene, const RtrHit* hits, uint32_t numHits, int32_t* leaves);
/* rtr_trace_occlusion with a start hint per ray: startLeaves is a DEVICE pointer, 4-B aligned, numRays entries, read at the refill beside
 * the ray it belongs to (the queue build does not look at it); NULL behaves exactly as the unhinted call.  Everything else — flags,
 * the scratch and its size, occluded[], the rays that need a deeper stack (finished over the BVH2 from the root) — as there.  stats: as
 * documented for rtr_trace_occlusion; for rtr_light_rays_hinted's rays and hints of a frame's camera hits the counters are the renderer's
 * any-hit counters with the default trace_own_leaf = 1. */
int  rtr_trace_occlusion_hinted_async(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const int32_t* startLeaves, uint32_t numRays,
                                      uint32_t flags, void* scratch, size_t scratchBytes, uint8_t* occluded);
int  rtr_trace_occlusion_hinted(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const int32_t* startLeaves, uint32_t numRays,
                                uint32_t flags, void* scratch, size_t scratchBytes, uint8_t* occluded, rtr_query_stats* stats);
/* The queued query with a cull mask (see "cull masks" above): rtr_trace_occlusion_hinted — startLeaves == NULL is the unhinted query —
 * plus rayMasks (DEVICE pointer, one byte per ray, gathered at the refill beside the ray and its hint; or NULL) and cullMask (8 bits,
 * higher bits refused).  occluded[] is byte for byte rtr_trace_rays_masked(RTR_QUERY_ANY)'s.  A ray whose effective mask is 0 is not
 * queued: its byte is 0 and stats count it as a ray with an empty interval is counted.  A hinted leaf whose triangles are all masked out
 * does not stop the ray.  Scratch, flags, pointers, alignment and stream order as rtr_trace_occlusion. */
int  rtr_trace_occlusion_masked_async(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const int32_t* startLeaves, const uint8_t* rayMasks,
                                      uint32_t numRays, uint32_t flags, uint32_t cullMask, void* scratch, size_t scratchBytes, uint8_t* occluded);
int  rtr_trace_occlusion_masked(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const int32_t* startLeaves, const uint8_t* rayMasks,
                                uint32_t numRays, uint32_t flags, uint32_t cullMask, void* scratch, size_t scratchBytes, uint8_t* occluded,
                                rtr_query_stats* stats);
/* Writes to the device array out[] the width * height * spp camera rays the renderer traces for `camera` (raygen.rgen:83-107:
 * jittered direction through the viewport, tmin 0.001, tmax 10000): ray k = (py * width + px) * spp + i.  ENQUEUED on ctx's stream.
 * Callers generate, edit and trace camera rays this way; traced with RTR_QUERY_CLOSEST they give the renderer's primary hits.
 * RTR_ERR_INVALID_ARGUMENT for a null or unaligned pointer, a zero extent or more than 2^32 - 1 rays. */
int  rtr_camera_rays_async(rtr_ctx* ctx, const RtrCameraData* camera, uint32_t width, uint32_t height, uint32_t spp, RtrRay* out);

/* What the closest-hit shader computes for numRays hits[] of rays[] (a closest-hit query's results, or hits of the caller's own): out[k]
 * is the RtrSurface of hits[k], by the renderer's own surface fetch (closesthit.rchit:53-106, raygen.rgen:110-121, miss.rmiss:15-27),
 * with the scene's current instance transforms.  rays[k] gives the direction the normal is turned against and the miss looks up.
 * rays, hits and out are DEVICE pointers, 16-B aligned.  The work is ENQUEUED on ctx's stream; the scene may belong to another context
 * of the same device.  numRays == 0 does nothing.  A hit whose ids are out of range gives RTR_SURFACE_INVALID and reads nothing there.
 * RTR_ERR_INVALID_ARGUMENT (with a message) for a null or unaligned pointer or a scene on another device. */
int  rtr_hit_surfaces_async(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const RtrHit* hits, uint32_t numRays,
                            RtrSurface* out);
/* The same, then joins ctx's stream (only that stream). */
int  rtr_hit_surfaces(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const RtrHit* hits, uint32_t numRays, RtrSurface* out);

/* ---- direct lighting for ray-query hits ----------------------------------------------------------------------------------
 * What the ray-gen shader does AFTER the closest hit (raygen.rgen:165-338, :345-357), in the stages the renderer itself runs it in:
 *   rtr_light_rays   the shadow rays of each hit        (the area-light samples of :206-231, the directional light of :299-303)
 *   rtr_trace_rays   RTR_QUERY_ANY answers them         (the caller's launch: any of the stages can be replaced; rtr_trace_occlusion
 *                                                        gives the same bytes, and so does rtr_trace_occlusion_hinted with
 *                                                        rtr_light_rays_hinted's hints: the renderer's own walk, rule for rule)
 *   rtr_shade_hits   the Cook-Torrance sums, the LTC term, sky and light hits
 *   rtr_tonemap_pack ACES + sRGB + B,G,R,255
 * camera rays -> closest hit -> these four reproduce rtr_render's images from public parts: at 1 sample per pixel bit for bit (with
 * more, the renderer adds all samples of a pixel into ONE running sum before it divides, which per-hit outputs cannot restate; and
 * divergence D6 of DESIGN.md section 4 holds here as there).
 * Every hit owns Q = numShadowRays * (triangles of the first numAreaLights lights) + 1 SLOTS, whether or not a ray is sent for them:
 * sample s of triangle ti of light l is slot (T_l + ti) * numShadowRays + s, T_l = the triangles of the lights before l; the
 * directional light is slot Q - 1. */
#define RTR_LIGHT_SHADOWED   1u   /* always produced */
#define RTR_LIGHT_UNSHADOWED 2u
#define RTR_LIGHT_ANALYTIC   4u   /* needs the scene's LTC tables */

typedef struct rtr_light_params {
    uint32_t numAreaLights;   /* SceneInfo.numAreaLights: the first lights of the scene that are sampled */
    uint32_t numShadowRays;   /* NUM_SHADOW_RAYS (reference: 3) */
    uint32_t frame;           /* SceneInfo.frame: enters every sample seed */
    uint32_t width, spp;      /* hit k belongs to pixel ((k / spp) % width, (k / spp) / width): rtr_camera_rays_async's order.  Used when seeds == NULL */
    uint32_t outputs;         /* RTR_LIGHT_SHADOWED (always produced) | RTR_LIGHT_UNSHADOWED | RTR_LIGHT_ANALYTIC */
    uint32_t _pad[2];
} rtr_light_params;           /* 32 bytes */

/* Q for these params: pure arithmetic on the scene's light table, no device is touched.  RTR_ERR_INVALID_ARGUMENT for a null pointer,
 * numAreaLights above the scene's lights, numShadowRays == 0 (or above 1024, rtr_render's limit), or a Q past 32 bits. */
int  rtr_light_slots(const rtr_scene* scene, const rtr_light_params* params, uint32_t* slotsPerHit);
/* For hit k of numHits, writes Q RtrRay at outRays[k * Q ... k * Q + Q): exactly the shadow rays the shader sends for that surface point —
 * origin hitPoint + 0.01 * hitNormal, normalised direction, tmin 0.001, tmax = distance - 0.5 (10000 for the directional light).  A slot
 * whose ray the shader does not send — a one-sided light triangle facing away, the directional light behind the surface, a hit that is a
 * miss, a light or has ids out of range — gets the NULL RAY, eight zero floats, which rtr_trace_rays answers "not occluded" without a walk.
 * seeds: device array of numHits uint32, or NULL.  The seed of sample s is s + base_k + frame (32-bit words), base_k = seeds[k], or
 * px * 733 + py * 1933 of the pixel params->width / spp give: camera-ray callers pass NULL and get the renderer's seeds.  The view
 * vector is normalize(rays[k].origin - hitPoint), for a camera ray the shader's cameraPosition - hitPoint.
 * rays, hits, outRays: DEVICE pointers, 16-B aligned; seeds 4-B aligned.  ENQUEUED on ctx's stream; the scene may belong to another
 * context of the same device.  numHits == 0 does nothing.  RTR_ERR_INVALID_ARGUMENT (with a message) for a null or misaligned pointer,
 * a scene on another device, params rtr_light_slots refuses, width or spp == 0 with seeds == NULL, or numHits * Q past 32 bits. */
int  rtr_light_rays_async(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const RtrHit* hits, uint32_t numHits,
                          const rtr_light_params* params, const uint32_t* seeds, RtrRay* outRays);
/* rtr_light_rays and the start hints of its rays (rtr_trace_occlusion_hinted): outRays is byte for byte what rtr_light_rays writes, and
 * outLeaves (DEVICE pointer, 4-B aligned, numHits * Q entries) gets at k * Q + slot the leaf code of hit k's own triangle exactly where
 * the renderer marks the ray — the slot's ray is sent and dot(hitNormal, lightVec) < 0 with the un-normalised vector to the light sample —
 * and 0 at every other slot: null slots, the directional light's slot Q - 1, every slot of a hit that is a miss, a light or invalid.
 * The leaf is looked up in the scene's triangle -> leaf table, whose first use allocates (see rtr_hit_leaves).  Otherwise as
 * rtr_light_rays_async; RTR_ERR_INVALID_ARGUMENT also for a null or misaligned outLeaves. */
int  rtr_light_rays_hinted_async(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const RtrHit* hits, uint32_t numHits,
                                 const rtr_light_params* params, const uint32_t* seeds, RtrRay* outRays, int32_t* outLeaves);
/* out[k] = the RtrRadiance of hit k: one primary sample's contribution — the sky at a miss and the light's colour at a light hit in every
 * sum asked for, the light loops at an object, zeros and RTR_SURFACE_INVALID for ids out of range.  occluded: the numHits * Q bytes an
 * RTR_QUERY_ANY query of rtr_light_rays' rays returned (no alignment asked); bytes of null slots are not read.  Sums not in
 * params->outputs are written as zeros and their work is skipped under the renderer's rule: an occluded sample's BRDF is evaluated only
 * when the unshadowed sum is wanted.  RTR_LIGHT_ANALYTIC on a scene without LTC tables: RTR_ERR_UNSUPPORTED.  out: 16-B aligned.
 * Otherwise as rtr_light_rays_async, with the same rays, hits, params and seeds. */
int  rtr_shade_hits_async(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const RtrHit* hits, uint32_t numHits,
                          const rtr_light_params* params, const uint32_t* seeds, const uint8_t* occluded, RtrRadiance* out);
/* outBGRA8[k] = the tone-mapped, packed pixel (raygen.rgen:345-357) of the three floats at (char*)radiance + k * strideBytes: a column of
 * RtrRadiance (stride 48), an RGBA float image (16), packed float3 (12).  strideBytes: a multiple of 4, >= 12; both pointers 4-B
 * aligned DEVICE pointers.  ENQUEUED on ctx's stream. */
int  rtr_tonemap_pack_async(rtr_ctx* ctx, const float* radiance, uint32_t strideBytes, uint32_t numValues, uint32_t* outBGRA8);
/* The same four, then join ctx's stream (only that stream). */
int  rtr_light_rays(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const RtrHit* hits, uint32_t numHits,
                    const rtr_light_params* params, const uint32_t* seeds, RtrRay* outRays);
int  rtr_light_rays_hinted(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const RtrHit* hits, uint32_t numHits,
                           const rtr_light_params* params, const uint32_t* seeds, RtrRay* outRays, int32_t* outLeaves);
int  rtr_shade_hits(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const RtrHit* hits, uint32_t numHits,
                    const rtr_light_params* params, const uint32_t* seeds, const uint8_t* occluded, RtrRadiance* out);
int  rtr_tonemap_pack(rtr_ctx* ctx, const float* radiance, uint32_t strideBytes, uint32_t numValues, uint32_t* outBGRA8);

/* ---- continuation rays for ray-query hits ----------------------------------------------------------------------------------
 * The second path vertex: for hit k, outRays[k] is ONE direction drawn from the renderer's material at surfaces[k] and outBounce[k] its
 * throughput weight BRDF * cos / pdf (RtrBounce, include/rtr_types.h), by rtr_bounce_sample of include/rtr_bounce.h — a cosine lobe and
 * the GGX lobe of alpha = roughness mixed by the one-sample balance heuristic, the BRDF the light loops evaluate.
 * surfaces are RtrSurface records, rtr_hit_surfaces' output or the caller's edit of it: the call reads NO scene memory and takes no
 * scene.  rays[k] is the ray that found the hit: its origin gives the view vector normalize(origin - position), rtr_light_rays'
 * convention.  The random numbers of hit k are rtr_random(s0), (s0 + 100), (s0 + 200), s0 = base_k + frame + 7919 * (depth + 1) in
 * 32-bit words, base_k = seeds[k], or px * 733 + py * 1933 of the pixel params->width / spp give: rtr_light_rays' rule.
 * A hit without a continuation (RtrBounce's comment) gets the NULL RAY, which every query answers without a walk, and 32 zero bytes;
 * every slot of every hit is written, and no output word is a NaN or an infinity.
 * rays, surfaces, outRays, outBounce: DEVICE pointers, 16-B aligned; seeds 4-B aligned; the outputs must not overlap the inputs.
 * ENQUEUED on ctx's stream: no allocation, no join, no copy back.  numHits == 0 does nothing.  RTR_ERR_INVALID_ARGUMENT (with a message
 * that names the function and the argument, and nothing written) for a null or misaligned pointer, lobes == 0 or unknown lobe bits,
 * width or spp == 0 with seeds == NULL, a normalOffset, tmin or tmax that is not finite, or !(tmax > tmin). */
int  rtr_bounce_rays_async(rtr_ctx* ctx, const RtrRay* rays, const RtrSurface* surfaces, uint32_t numHits, const rtr_bounce_params* params,
                           const uint32_t* seeds, RtrRay* outRays, RtrBounce* outBounce);
/* The same, then joins ctx's stream (only that stream). */
int  rtr_bounce_rays(rtr_ctx* ctx, const RtrRay* rays, const RtrSurface* surfaces, uint32_t numHits, const rtr_bounce_params* params,
                     const uint32_t* seeds, RtrRay* outRays, RtrBounce* outBounce);
/* The host restatement: the same function of the same bytes on HOST pointers, no device (as rtr_host_tree_cost).  The same header
 * compiled for the host cores; the device's records equal these bit for bit. */
int  rtr_host_bounce_rays(const RtrRay* rays, const RtrSurface* surfaces, uint32_t numHits, const rtr_bounce_params* params,
                          const uint32_t* seeds, RtrRay* outRays, RtrBounce* outBounce);
/* outSin[k], outCos[k] = rtr_sincos_turn(u[k]) of include/rtr_bounce.h, u in [0, 1]: the one function of the sampling contract that is
 * a polynomial of this library's own, on HOST pointers, so that it can be held to float64 by itself (tests/test_bounce_host.py).
 * RTR_ERR_INVALID_ARGUMENT for a null pointer with n > 0. */
int  rtr_host_sincos_turn(const float* u, uint32_t n, float* outSin, float* outCos);

/* ---- compaction of live paths, with Russian roulette -------------------------------------------------------------------------
 * Between two vertices of a path tracer's wavefront: the paths that go on are gathered to the front of every array IN THEIR ORDER
 * (a stable compaction), the rest of every array is cleared.  Which paths go on is rtr_path_survive of include/rtr_paths.h: a path is
 * LIVE when its ray would cost a walk (origin and direction finite, direction not zero, tmax > tmin), every channel of its throughput
 * is finite and >= 0 and one is > 0; with RTR_COMPACT_ROULETTE a live path of p = max(max3(T), survivalFloor) < 1 goes on with
 * probability p — iff rtr_random(seeds[k] + frame + 7919 * (depth + 1) + 300) < p, the fourth random number of the vertex whose
 * rtr_bounce_rays took the first three — and with throughput T / p.
 * Inputs, DEVICE pointers: rays (16-B aligned); throughput: path k's three floats are at (char*)throughput + k * throughputStrideBytes
 * (a multiple of 4, at least 12; 4-B aligned — an RtrBounce array is passed as it is with stride 32); seeds (4-B aligned) or NULL:
 * then outSeeds must be NULL too and the roulette is refused; pathIds or NULL: path k has id k.
 * Outputs: ALL numPaths slots of each are written.  With count survivors, slot j < count holds the j-th survivor in input order: its
 * ray's 32 bytes, its throughput as PACKED floats (stride 12), its seed and its id; slot j >= count holds the null ray, zero
 * throughput, seed 0 and id RTR_PATH_NONE; *outCount = count, a DEVICE word.  A caller that never joins keeps launching numPaths wide,
 * its dead lanes gathered into whole dead waves at the end; one that reads the count shrinks every later launch.  Chained calls
 * compose the ids: the second call's ids index the first call's input.
 * scratch: rtr_compact_scratch_bytes(numPaths) bytes of device memory the CALLER owns (a multiple of 16, monotone in numPaths; pure
 * arithmetic), 16-B aligned; it need not be initialised and nothing is kept in it between calls.
 * ENQUEUED on ctx's stream, three launches: no allocation, no join, no copy back.  numPaths == 0 writes *outCount = 0 when outCount
 * is not NULL, and nothing else.  RTR_ERR_INVALID_ARGUMENT (with a message that names the function and the argument, and nothing
 * written) for a null or misaligned pointer the call needs (outSeeds exactly when seeds; outCount), a scratch that is too small, a
 * stride that is not a multiple of 4 or below 12, unknown flag bits, the roulette without seeds, a survivalFloor outside (0, 1] with
 * the roulette, non-zero _reserved words, or an output range (the scratch and the count included) that overlaps an input range or
 * another output. */
int  rtr_compact_scratch_bytes(uint32_t numPaths, size_t* bytes);
int  rtr_compact_paths_async(rtr_ctx* ctx, const RtrRay* rays, const float* throughput, const uint32_t* seeds, const uint32_t* pathIds,
                             uint32_t numPaths, const rtr_compact_params* params, void* scratch, size_t scratchBytes,
                             RtrRay* outRays, float* outThroughput, uint32_t* outSeeds, uint32_t* outPathIds, uint32_t* outCount);
/* The same, then joins ctx's stream (only that stream).  hostCount: NULL, or where one 4-byte copy after the join puts the count. */
int  rtr_compact_paths(rtr_ctx* ctx, const RtrRay* rays, const float* throughput, const uint32_t* seeds, const uint32_t* pathIds,
                       uint32_t numPaths, const rtr_compact_params* params, void* scratch, size_t scratchBytes,
                       RtrRay* outRays, float* outThroughput, uint32_t* outSeeds, uint32_t* outPathIds, uint32_t* outCount, uint32_t* hostCount);
/* The host restatement: the same function of the same bytes on HOST pointers, no device, no scratch; outCount is a host word.  The same
 * header in a plain loop; the device's words equal these bit for bit. */
int  rtr_host_compact_paths(const RtrRay* rays, const float* throughput, const uint32_t* seeds, const uint32_t* pathIds,
                            uint32_t numPaths, const rtr_compact_params* params,
                            RtrRay* outRays, float* outThroughput, uint32_t* outSeeds, uint32_t* outPathIds, uint32_t* outCount);

/* ---- accumulation: a vertex's radiance added to the image, and the throughput after its bounce --------------------------------
 * What a path tracer does with the records of one vertex, so that a frame is library launches on one stream and nothing else.  The
 * rule is include/rtr_accum.h, every step one IEEE binary32 operation per channel: for path k < numPaths
 *     rad  = radiance[k].shadowed; for a light hit with RTR_ACCUM_LIGHTS_FROM_EMITTERS emitters[k].radiance, for a miss with
 *            RTR_ACCUM_MISSES_FROM_ESCAPES escapes[k].radiance (0 where that array is NULL)
 *     term = T[k] * rad, then + T[k] * skySums[4k .. 4k + 2] when skySums (rtr_shade_sky's output) is given
 *     id   = pathIds ? pathIds[k] : k;  with id < params->numSlots: accum[id] += term, and outTerm[id] = term when outTerm is given
 *     outThroughput[3k ..] = T[k] * bounces[k].weight when bounces and outThroughput are given (both or neither), for every k.
 * Without the flags a light hit or a miss adds `shadowed`, the camera vertex's rule.  A term of zero is still added.  A path whose id
 * is not below numSlots — RTR_PATH_NONE, what rtr_compact_paths writes behind the survivors — touches neither image, so a caller
 * that never joins launches numPaths wide.  The ids below numSlots must be DISTINCT: there are no atomics, and an image row named
 * twice ends up holding one of the two results.  Rows of outTerm that no path names keep their bytes; the caller clears them.
 * DEVICE pointers: radiance, emitters, escapes, bounces and skySums 16-B aligned; throughput (path k's three floats at (char*)throughput
 * + k * throughputStrideBytes), pathIds, accum, outTerm (slot id's three floats at id * imageStrideBytes) and outThroughput (packed,
 * stride 12) 4-B aligned.  outThroughput == throughput with throughputStrideBytes 12 is allowed (in place); every other overlap of
 * an output with an input or with another output is refused.
 * ENQUEUED on ctx's stream, one launch: no allocation, no join, no copy back.  numPaths == 0 is RTR_OK and launches nothing.
 * RTR_ERR_INVALID_ARGUMENT (with a message that names the function and the argument, and nothing written; the arrays and the params
 * are checked before the handle) for a null radiance, throughput, accum or params, bounces without outThroughput or the reverse, a
 * misaligned pointer, a stride that is not a multiple of 4 or below 12, unknown flag bits, non-zero _reserved words, numSlots 0, an
 * array whose extent does not fit the address space, or such an overlap. */
int  rtr_accumulate_paths_async(rtr_ctx* ctx, const RtrRadiance* radiance, const float* throughput, const uint32_t* pathIds,
                                const RtrEmitter* emitters, const RtrSkyEscape* escapes, const float* skySums, const RtrBounce* bounces,
                                uint32_t numPaths, const rtr_accum_params* params, float* accum, float* outTerm, float* outThroughput);
/* The same, then joins ctx's stream (only that stream). */
int  rtr_accumulate_paths(rtr_ctx* ctx, const RtrRadiance* radiance, const float* throughput, const uint32_t* pathIds,
                          const RtrEmitter* emitters, const RtrSkyEscape* escapes, const float* skySums, const RtrBounce* bounces,
                          uint32_t numPaths, const rtr_accum_params* params, float* accum, float* outTerm, float* outThroughput);
/* The host restatement: the same function of the same bytes on HOST pointers, no device.  The same header in a plain loop; the
 * device's words equal these bit for bit. */
int  rtr_host_accumulate_paths(const RtrRadiance* radiance, const float* throughput, const uint32_t* pathIds,
                               const RtrEmitter* emitters, const RtrSkyEscape* escapes, const float* skySums, const RtrBounce* bounces,
                               uint32_t numPaths, const rtr_accum_params* params, float* accum, float* outTerm, float* outThroughput);
/* The gather that goes with it: out[j] = src[rows[j]] for j < numRows, records of recordBytes bytes (a multiple of 4, at most 256);
 * a row that is not below numSrc (RTR_PATH_NONE) gives a record of zero bytes.  With the ids of a rtr_compact_paths call that took
 * pathIds == NULL as rows, the records of a vertex (RtrSurface, RtrBounce) and the pixel ids follow the survivors.  src, rows and out
 * 4-B aligned DEVICE pointers (src may be NULL with numSrc == 0); 16-B accesses are used when recordBytes and both record arrays
 * allow it.  One launch on ctx's stream; numRows == 0 is RTR_OK and launches nothing.  RTR_ERR_INVALID_ARGUMENT for a recordBytes
 * that is 0, not a multiple of 4 or above 256, a null or misaligned pointer, or out overlapping src or rows. */
int  rtr_gather_records_async(rtr_ctx* ctx, const void* src, uint32_t recordBytes, uint32_t numSrc, const uint32_t* rows, uint32_t numRows, void* out);
int  rtr_gather_records(rtr_ctx* ctx, const void* src, uint32_t recordBytes, uint32_t numSrc, const uint32_t* rows, uint32_t numRows, void* out);
int  rtr_host_gather_records(const void* src, uint32_t recordBytes, uint32_t numSrc, const uint32_t* rows, uint32_t numRows, void* out);

/* ---- picked light samples: one-sample direct lighting for path vertices ------------------------------------------------------
 * rtr_light_rays sends all Q shadow rays of a hit; these send P picked area-light samples and the directional light.  With Ttot the
 * triangles of the first numAreaLights lights and ns = numShadowRays a hit has A = Ttot * ns = Q - 1 AREA SLOTS, rtr_light_slots' first
 * Q - 1 under the same numbers, and owns R = P + 1 slots here: pick p at slot p, the directional light at slot R - 1.  Which area slot a
 * pick takes is the rule of include/rtr_pick.h (rtr_pick_params, include/rtr_types.h), or the caller's choice (slotsIn).  Each pick
 * weighted Ttot / P, the picks' sum is an unbiased estimate of the light loops' area sum.
 *
 * rtr_light_rays_picked: outSlots[k * P + p] = the area slot of pick p of hit k — slotsIn[k * P + p] as it is, or drawn — written for
 * every hit; outRays[k * R + p] = byte for byte the ray rtr_light_rays writes at outRays[k * Q + that slot] for the same hit, params and
 * seeds, the null ray where that is null and for a slot >= A (RTR_PICK_NONE included); outRays[k * R + R - 1] = rtr_light_rays' slot
 * Q - 1.  A hit that is a miss, a light or invalid gets R null rays.  slotsIn: NULL or numHits * P words, 4-B aligned; outSlots
 * likewise, required; the others as rtr_light_rays_async.
 * rtr_shade_hits_picked: out[k] as rtr_shade_hits' — kind, the sky at a miss and the colour at a light hit unchanged — with, at an
 * object, shadowed = sum over the picks in order of contrib_p * (occluded[k * R + p] ? 0 : w_p), then the directional term as the light
 * loops add it; unshadowed the same with every sample visible, when asked for; analytic zeros.  contrib_p: the light loops' BRDF * L / pdf
 * of slots[k * P + p] (a null slot contributes nothing).  slots: rtr_light_rays_picked's outSlots; occluded: the numHits * R bytes of an
 * RTR_QUERY_ANY query of its rays; weights: NULL (w_p = (float)Ttot / (float)P) or numHits * P floats — 1 / (P * pdf_slot * ns) for slots
 * drawn with probability pdf_slot each.  RTR_LIGHT_ANALYTIC: RTR_ERR_UNSUPPORTED, the LTC term integrates whole lights.
 * Both are ENQUEUED on ctx's stream.  Refused before anything is written (RTR_ERR_INVALID_ARGUMENT, the message names the function and
 * the argument): a null or misaligned pointer, numPicks 0 or above RTR_PICK_MAX, non-zero _reserved words, numHits * R past 32 bits,
 * A above RTR_PICK_MAX_SLOTS, width or spp == 0 with seeds == NULL, params rtr_light_slots refuses, a scene on another device. */
int  rtr_light_rays_picked_async(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const RtrHit* hits, uint32_t numHits,
                                 const rtr_light_params* params, const rtr_pick_params* pick, const uint32_t* seeds, const uint32_t* slotsIn,
                                 RtrRay* outRays, uint32_t* outSlots);
int  rtr_shade_hits_picked_async(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const RtrHit* hits, uint32_t numHits,
                                 const rtr_light_params* params, const rtr_pick_params* pick, const uint32_t* seeds, const uint32_t* slots,
                                 const float* weights, const uint8_t* occluded, RtrRadiance* out);
/* The same two, then join ctx's stream (only that stream). */
int  rtr_light_rays_picked(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const RtrHit* hits, uint32_t numHits,
                           const rtr_light_params* params, const rtr_pick_params* pick, const uint32_t* seeds, const uint32_t* slotsIn,
                           RtrRay* outRays, uint32_t* outSlots);
int  rtr_shade_hits_picked(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const RtrHit* hits, uint32_t numHits,
                           const rtr_light_params* params, const rtr_pick_params* pick, const uint32_t* seeds, const uint32_t* slots,
                           const float* weights, const uint8_t* occluded, RtrRadiance* out);
/* The drawn slots on the host: outSlots[k * P + p] for numHits hits by the rule of include/rtr_pick.h in a plain loop, HOST pointers, no
 * device.  frame, width, spp: rtr_light_params' (width, spp used when seeds == NULL); areaSlots: A.  The device's words equal these. */
int  rtr_host_pick_slots(const uint32_t* seeds, uint32_t numHits, uint32_t frame, uint32_t width, uint32_t spp, const rtr_pick_params* pick,
                         uint32_t areaSlots, uint32_t* outSlots);

/* ---- multiple importance sampling at a path vertex: the picks and the bounce under the balance heuristic ------------------------
 * With the picked samples alone a light reaches a path vertex only through its shadow rays, and a bounce ray that lands on a light counts
 * for nothing.  These two calls let both count: rtr_mis_pick_weights gives the P picks of a vertex the weights rtr_shade_hits_picked is
 * to apply, and rtr_emitter_hits gives what the vertex's bounce ray adds when its closest hit is a light.  The rule is include/rtr_mis.h
 * (rtr_mis_params, RtrMisSample, RtrEmitter: include/rtr_types.h); DESIGN.md section 3 has the estimator.
 *
 * rtr_mis_pick_weights: outWeights[k * P + p] = ((float)Ttot / (float)P) * wPick of pick p of hit k, 0 for a pick that sends no ray
 * (RTR_PICK_NONE, a slot >= A, a one-sided triangle facing away), for a hit that is not an object and where a value is not finite;
 * outSamples (NULL, or numHits * P records, 16-B aligned): what each weight was made from, zeros beside a zero weight.  rays, hits,
 * params, pick, seeds as rtr_shade_hits_picked takes them; slots: the numHits * P words rtr_light_rays_picked wrote, or NULL — then the
 * slots it draws with slotsIn == NULL for the same params, pick and seeds.  mis: numPicks, numAreaLights and numShadowRays repeat pick's
 * and params' (a difference is refused); lobes: the lobes the vertex's rtr_bounce_rays call samples.
 * rtr_emitter_hits: out[k] for bounce ray rays[k] with closest hit hits[k], having left the vertex whose RtrSurface is prevSurfaces[k]
 * and whose RtrBounce is bounces[k]: where the hit is a triangle of a light, radiance (to be multiplied by the throughput after the
 * bounce), wBounce, the pick density lightPdf, the distance and the light-triangle record, kind = RTR_SURFACE_LIGHT; 32 zero bytes for a
 * miss, an object, ids out of range, a dead bounce (pdf <= 0), a one-sided light met from behind, and where a value is not finite.  A
 * light with index >= mis->numAreaLights is sampled by the bounce alone: wBounce = 1.  All arrays numRays records, 16-B aligned.
 * Both are ENQUEUED on ctx's stream: no allocation, no join, no copy back.  Refused before anything is written
 * (RTR_ERR_INVALID_ARGUMENT, the message names the function and the argument): a null or misaligned pointer, numPicks 0 or above
 * RTR_PICK_MAX, lobes 0 or unknown, non-zero _reserved words, what rtr_shade_hits_picked refuses of params and pick, numAreaLights above
 * the scene's lights, a scene on another device. */
int  rtr_mis_pick_weights_async(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const RtrHit* hits, uint32_t numHits,
                                const rtr_light_params* params, const rtr_pick_params* pick, const rtr_mis_params* mis, const uint32_t* seeds,
                                const uint32_t* slots, float* outWeights, RtrMisSample* outSamples);
int  rtr_emitter_hits_async(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces,
                            const RtrBounce* bounces, uint32_t numRays, const rtr_mis_params* mis, RtrEmitter* out);
/* The same two, then join ctx's stream (only that stream). */
int  rtr_mis_pick_weights(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const RtrHit* hits, uint32_t numHits,
                          const rtr_light_params* params, const rtr_pick_params* pick, const rtr_mis_params* mis, const uint32_t* seeds,
                          const uint32_t* slots, float* outWeights, RtrMisSample* outSamples);
int  rtr_emitter_hits(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces,
                      const RtrBounce* bounces, uint32_t numRays, const rtr_mis_params* mis, RtrEmitter* out);
/* A read-back of the scene's light-triangle table, current after updates: outRecords gets 16 floats per light triangle of ALL the
 * scene's lights — {P0, area} {P1, pdfrec} {P2, -} {unit normal, -} in world space — and outFirst (NULL, or one word per light) the first
 * record of each light; *outCount the number of triangles.  capacityTris < that count (or outRecords == NULL) copies nothing, reports the
 * count and is refused with RTR_ERR_INVALID_ARGUMENT.  Joins the scene's stream and copies: HOST pointers. */
int  rtr_scene_export_light_tris(const rtr_scene* scene, float* outRecords, uint32_t capacityTris, uint32_t* outFirst, uint32_t* outCount);
/* The host forms of include/rtr_mis.h in plain loops, HOST pointers, no device; the device's words equal these.
 * rtr_host_bounce_pdf: outPdf[k] = the density rtr_bounce_rays divides by at surfaces[k] (found by rays[k]) for the UNIT direction
 * dirs[3k ... 3k + 2] and the lobes given: RtrBounce::pdf bit for bit for the direction it drew.
 * rtr_host_mis_weights: outSamples[k] = {lightPdf, pb[k], wPick, cosLight[k], dist[k], area[k], 0, 0} and, with outWBounce != NULL,
 * outWBounce[k] = wBounce.  P may be 0 here (nobody picks).
 * rtr_host_emitter_hits: rtr_emitter_hits for a light table handed in (lightTris, lightTriFirst: rtr_scene_export_light_tris';
 * lights: the scene's light infos). */
int  rtr_host_bounce_pdf(const RtrRay* rays, const RtrSurface* surfaces, const float* dirs, uint32_t n, uint32_t lobes, float* outPdf);
int  rtr_host_mis_weights(uint32_t n, const float* pb, const float* dist, const float* cosLight, const float* area, uint32_t Ttot, uint32_t P,
                          RtrMisSample* outSamples, float* outWBounce);
int  rtr_host_emitter_hits(const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces, const RtrBounce* bounces, uint32_t n,
                           const float* lightTris, const uint32_t* lightTriFirst, const RtrAreaLightInfo* lights, uint32_t numLights,
                           const rtr_mis_params* mis, RtrEmitter* out);

/* ---- sky importance sampling at a path vertex: directions drawn in proportion to the sky, under the balance heuristic ------------------
 * Without these calls the sky reaches a path vertex only when its bounce ray happens to miss the scene.  rtr_sky_rays draws S directions
 * per vertex in proportion to the scene's SKY TABLE — a piecewise-constant importance function over the HDRI's texel cells (or over a
 * 32 x 16 grid for the constant sky), held as integer prefix sums — and gives each its shadow ray and its contribution; rtr_shade_sky
 * sums the contributions the occlusion query let through; rtr_sky_hits gives what the vertex's bounce ray adds when it misses.  The rule
 * is include/rtr_sky.h (rtr_sky_params, RtrSkySample, RtrSkyEscape, rtr_sky_table: include/rtr_types.h); DESIGN.md section 3 has the
 * estimator and the table.
 *
 * rtr_scene_prepare_sky: builds the table on the device from the HDRI the scene holds, 4 B per texel and 8 B per row.  SYNCHRONOUS: it
 * allocates and joins, once per scene (a second call does nothing).  The first rtr_sky_rays / rtr_sky_hits / export of a scene builds
 * the table the same way, so only a caller that wants a chain without allocation or join has to call this first.  The HDRI and the sky
 * colour cannot change after rtr_scene_create, so no refit, rebuild, vertex or instance update touches the table.  Refused: an HDRI wider
 * than 65535 texels (a row's sum would not fit 32 bits).
 * rtr_scene_export_sky_table: *outWidth, *outHeight of the table; with capacities of at least width * height and height, the row sums and
 * the marginal sums to HOST pointers; smaller capacities (or NULL arrays) copy nothing, report the extent and are refused with
 * RTR_ERR_INVALID_ARGUMENT.  Joins and copies.
 * rtr_host_sky_table: the same table built on the host from a texture (NULL: the constant sky of skyColor, sRGB-encoded as
 * rtr_scene_desc's), with the same capacity rule.  The device's words equal the host's, all of them.
 *
 * rtr_sky_rays: for hit k (found by rays[k], surface surfaces[k]: rtr_hit_surfaces') and sample j < S, outRays[k * S + j] and
 * outSamples[k * S + j]; every slot of every hit is written, a dead sample as the null ray and 32 zero bytes.  seeds: one word per hit,
 * or NULL for the pixel rule (params->width, params->spp).
 * rtr_shade_sky: out[4k ... 4k + 2] = the sum over j, in order, of samples[k * S + j].contrib where occluded[k * S + j] == 0 (the bytes
 * an RTR_QUERY_ANY query of outRays wrote), out[4k + 3] = 0.  16 B per hit.
 * rtr_sky_hits: out[k] for bounce ray rays[k] with closest hit hits[k], having left the vertex whose RtrSurface is prevSurfaces[k] and
 * whose RtrBounce is bounces[k] — read only where the hit is a miss; 32 zero bytes for every hit that is not a miss.  params->numSamples
 * may be 0 here (the vertex drew no sky sample: wBounce = 1).
 * The _async forms are ENQUEUED on ctx's stream: on a prepared scene no allocation, no join, no copy back.  The plain forms then join
 * that stream (only that stream).  Refused before anything is written (RTR_ERR_INVALID_ARGUMENT, the message names the function and the
 * argument): a null or misaligned pointer, numSamples 0 (rtr_sky_rays, rtr_shade_sky) or above RTR_SKY_MAX_SAMPLES, lobes 0 or unknown,
 * unknown flag bits, a non-zero _reserved word, width or spp 0 with seeds == NULL, numHits * S past 32 bits, an output that overlaps an
 * input or another output, a scene on another device. */
int  rtr_scene_prepare_sky(rtr_scene* scene);
int  rtr_scene_export_sky_table(const rtr_scene* scene, uint32_t* outWidth, uint32_t* outHeight, uint32_t* outRows, size_t capacityCells,
                                uint64_t* outMarginal, uint32_t capacityRows);
int  rtr_sky_rays_async(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const RtrSurface* surfaces, uint32_t numHits,
                        const rtr_sky_params* params, const uint32_t* seeds, RtrRay* outRays, RtrSkySample* outSamples);
int  rtr_shade_sky_async(rtr_ctx* ctx, const RtrSkySample* samples, const uint8_t* occluded, uint32_t numHits, uint32_t numSamples, float* out);
int  rtr_sky_hits_async(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces,
                        const RtrBounce* bounces, uint32_t numRays, const rtr_sky_params* params, RtrSkyEscape* out);
int  rtr_sky_rays(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const RtrSurface* surfaces, uint32_t numHits,
                  const rtr_sky_params* params, const uint32_t* seeds, RtrRay* outRays, RtrSkySample* outSamples);
int  rtr_shade_sky(rtr_ctx* ctx, const RtrSkySample* samples, const uint8_t* occluded, uint32_t numHits, uint32_t numSamples, float* out);
int  rtr_sky_hits(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces,
                  const RtrBounce* bounces, uint32_t numRays, const rtr_sky_params* params, RtrSkyEscape* out);
/* The host forms of include/rtr_sky.h in plain loops, HOST pointers, no device; the device's words equal these.  hdri: the sky's texture
 * or NULL for the constant sky of skyColor (three floats, sRGB-encoded); table: rtr_host_sky_table's (or an exported one) of that sky.
 * rtr_host_sky_pdf: outPdf[k] = the solid-angle density of the table for direction dirs[3k ... 3k + 2] (it need not be normalised).
 * rtr_host_sky_radiance: out[3k ... 3k + 2] = the miss rule's radiance for that direction: RtrSurface::color of a miss, bit for bit. */
int  rtr_host_sky_table(const rtr_texture* hdri, const float* skyColor, uint32_t* outWidth, uint32_t* outHeight, uint32_t* outRows,
                        size_t capacityCells, uint64_t* outMarginal, uint32_t capacityRows);
int  rtr_host_sky_rays(const rtr_texture* hdri, const float* skyColor, const rtr_sky_table* table, const RtrRay* rays, const RtrSurface* surfaces,
                       uint32_t numHits, const rtr_sky_params* params, const uint32_t* seeds, RtrRay* outRays, RtrSkySample* outSamples);
int  rtr_host_sky_hits(const rtr_texture* hdri, const float* skyColor, const rtr_sky_table* table, const RtrRay* rays, const RtrHit* hits,
                       const RtrSurface* prevSurfaces, const RtrBounce* bounces, uint32_t numRays, const rtr_sky_params* params, RtrSkyEscape* out);
int  rtr_host_sky_pdf(const rtr_sky_table* table, const float* dirs, uint32_t n, float* outPdf);
int  rtr_host_sky_radiance(const rtr_texture* hdri, const float* skyColor, const float* dirs, uint32_t n, float* out);

/* ---- power-proportional light picks: a light-power table, its picks and their MIS -------------------------------------------------
 * rtr_light_rays_picked draws a vertex's picks uniformly over the light triangles.  These calls draw them in proportion to the emitted
 * power of each triangle — max(colour) * intensity * area — from the scene's LIGHT-POWER TABLE: one integer weight and one 64-bit
 * inclusive sum per light triangle of ALL lights, in rtr_scene_export_light_tris' order.  The rule is include/rtr_power.h; DESIGN.md
 * section 3 has the table, the estimator and the unbiasedness argument.  The chain is rtr_pick_slots_power ->
 * rtr_light_rays_picked(slotsIn) -> an occlusion query -> rtr_shade_hits_picked(weights), with rtr_mis_pick_weights_power between
 * the first two and rtr_emitter_hits_power on the bounce ray when the bounce is to count the lights it meets.
 *
 * rtr_scene_prepare_light_power: builds the table on the device, 12 B per light triangle.  SYNCHRONOUS: it allocates and joins, once per
 * scene (a second call does nothing).  The first power call or export of a scene builds it the same way, so only a caller that wants a
 * chain without allocation or join has to call this first.  Once a scene has a table, every call that rewrites its light triangles or
 * its light infos — rtr_scene_update_lights, rtr_scene_update_instances, rtr_scene_update_vertices, rtr_scene_rebuild's refit and the
 * _async updates — enqueues the two launches of the build right behind its own, on the same stream: no allocation, no join, the _async
 * updates keep their contract.  A scene without a table launches what it launched before.
 * rtr_scene_export_light_power: *outCount = the light triangles of all lights; with capacityTris of at least that, the weights and the
 * sums to HOST pointers; a smaller capacity (or a NULL array) copies nothing, reports the count and is refused with
 * RTR_ERR_INVALID_ARGUMENT.  Joins the scene's stream and copies.
 * rtr_pick_slots_power: for hit k and pick p < P, outSlots[k * P + p] = the area slot drawn (RTR_PICK_NONE when no triangle of the first
 * numAreaLights lights emits) and outWeights[k * P + p] = total / (P * weight) of its triangle, the weight rtr_shade_hits_picked is to
 * apply (0 beside RTR_PICK_NONE).  It needs the seeds alone: seeds (one word per hit) or NULL for the pixel rule (params->width,
 * params->spp); params->frame and pick->depth enter as in rtr_light_rays_picked.
 * rtr_mis_pick_weights_power: rtr_mis_pick_weights' arguments; slots is REQUIRED (rtr_pick_slots_power's, or the caller's);
 * outWeights[k * P + p] = wPow * wPick with the table's probability of the slot's triangle; 0 for a triangle of weight 0.
 * rtr_emitter_hits_power: rtr_emitter_hits' arguments and records with the table's probability of the hit triangle; a triangle of weight
 * 0, or of a light with index >= mis->numAreaLights, is the bounce's alone (wBounce = 1).
 * The _async forms are ENQUEUED on ctx's stream: on a prepared scene no allocation, no join, no copy back.  The plain forms then join
 * that stream (only that stream).  Refused before anything is written (RTR_ERR_INVALID_ARGUMENT, the message names the function and the
 * argument): a null or misaligned pointer, numPicks 0 or above RTR_PICK_MAX, non-zero _reserved words, A above RTR_PICK_MAX_SLOTS,
 * numAreaLights above the scene's lights, width or spp 0 with seeds == NULL, a scene on another device. */
int  rtr_scene_prepare_light_power(rtr_scene* scene);
int  rtr_scene_export_light_power(const rtr_scene* scene, uint32_t* outWeights, uint64_t* outCdf, uint32_t capacityTris, uint32_t* outCount);
int  rtr_pick_slots_power_async(rtr_ctx* ctx, const rtr_scene* scene, uint32_t numHits, const rtr_light_params* params, const rtr_pick_params* pick,
                                const uint32_t* seeds, uint32_t* outSlots, float* outWeights);
int  rtr_pick_slots_power(rtr_ctx* ctx, const rtr_scene* scene, uint32_t numHits, const rtr_light_params* params, const rtr_pick_params* pick,
                          const uint32_t* seeds, uint32_t* outSlots, float* outWeights);
int  rtr_mis_pick_weights_power_async(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const RtrHit* hits, uint32_t numHits,
                                      const rtr_light_params* params, const rtr_pick_params* pick, const rtr_mis_params* mis, const uint32_t* seeds,
                                      const uint32_t* slots, float* outWeights, RtrMisSample* outSamples);
int  rtr_mis_pick_weights_power(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const RtrHit* hits, uint32_t numHits,
                                const rtr_light_params* params, const rtr_pick_params* pick, const rtr_mis_params* mis, const uint32_t* seeds,
                                const uint32_t* slots, float* outWeights, RtrMisSample* outSamples);
int  rtr_emitter_hits_power_async(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces,
                                  const RtrBounce* bounces, uint32_t numRays, const rtr_mis_params* mis, RtrEmitter* out);
int  rtr_emitter_hits_power(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces,
                            const RtrBounce* bounces, uint32_t numRays, const rtr_mis_params* mis, RtrEmitter* out);
/* The host forms of include/rtr_power.h in plain loops, HOST pointers, no device; the device's words equal these.
 * rtr_host_light_power: the table of a light table handed in (lightTris, lightTriFirst: rtr_scene_export_light_tris'; lights: the scene's
 * light infos): one weight and one sum per light triangle of all numLights lights.
 * rtr_host_pick_slots_power: rtr_pick_slots_power for a table handed in; tris: Ttot, the triangles of the first numAreaLights lights.
 * rtr_host_mis_weights_power: rtr_host_mis_weights with the probability of triangle lightTri[k] in place of 1 / Ttot; outSamples[k] =
 * {lightPdf, pb[k], wPick, cosLight[k], dist[k], area[k], lightTri[k], 0}; outWBounce (or NULL): wBounce; outWeights (or NULL): the
 * weight rtr_mis_pick_weights_power gives a pick on that triangle.  P may be 0 here (nobody picks).
 * rtr_host_emitter_hits_power: rtr_host_emitter_hits with the table. */
int  rtr_host_light_power(const float* lightTris, const uint32_t* lightTriFirst, const RtrAreaLightInfo* lights, uint32_t numLights,
                          uint32_t* outWeights, uint64_t* outCdf);
int  rtr_host_pick_slots_power(const uint64_t* cdf, uint32_t tris, const uint32_t* seeds, uint32_t numHits, const rtr_light_params* params,
                               const rtr_pick_params* pick, uint32_t* outSlots, float* outWeights);
int  rtr_host_mis_weights_power(uint32_t n, const float* pb, const float* dist, const float* cosLight, const float* area, const uint32_t* lightTri,
                                const uint64_t* cdf, uint32_t tris, uint32_t P, RtrMisSample* outSamples, float* outWBounce, float* outWeights);
int  rtr_host_emitter_hits_power(const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces, const RtrBounce* bounces, uint32_t n,
                                 const float* lightTris, const uint32_t* lightTriFirst, const RtrAreaLightInfo* lights, uint32_t numLights,
                                 const uint64_t* cdf, const rtr_mis_params* mis, RtrEmitter* out);

/* ---- resampled light picks: candidates from the power table, chosen by what they would contribute at the vertex --------------------
 * rtr_pick_slots_power looks at the lights and never at the vertex.  rtr_pick_slots_ris takes its place in the chain (-> rtr_light_rays_picked
 * (slotsIn) -> an occlusion query -> rtr_shade_hits_picked(weights)): for hit k and pick p < P it draws ris->numCandidates (M) slots from the
 * scene's light-power table, gives each the largest channel of the unshadowed contribution rtr_shade_hits_picked would evaluate there
 * (the BRDF, both cosines, the distance, the light's colour and its one-sidedness) as its target, keeps one in proportion to target /
 * table probability, and writes outSlots[k * P + p] and outWeights[k * P + p] = (sum_j target_j / q_j) / (target_y M P): ONE shadow ray
 * per pick, M BRDFs.  The rule is include/rtr_ris.h (rtr_ris_params: include/rtr_types.h); DESIGN.md section 3 has the estimator and the
 * unbiasedness argument.  M = 1 is the power pick.  A hit that is not an object, a pick whose candidates all have target 0 (one-sided
 * triangles facing away, no positive channel) and a table without power give RTR_PICK_NONE and 0.  No output word is ever a NaN or an
 * infinity.  With RTR_RIS_MIS the target is multiplied by, and the weight carries, the wPick rtr_mis_pick_weights_power computes for
 * ris->lobes: the outputs replace that call's too, and the bounce ray takes rtr_emitter_hits_power as before.
 * outCandidates, outTargets (both or neither): [(k * P + p) * M + j] = the slot of candidate j (RTR_PICK_NONE without a table) and its
 * target as used (0 where it counted as 0, and at a hit that is not an object).
 * The _async form is ENQUEUED on ctx's stream: on a scene that has its power table (rtr_scene_prepare_light_power) no allocation, no
 * join, no copy back; the first call of an unprepared scene builds the table as the power calls do.  The plain form then joins that
 * stream (only that stream).  Refused before anything is written (RTR_ERR_INVALID_ARGUMENT, the message names the function and the
 * argument): a null or misaligned pointer, numCandidates 0 or above RTR_RIS_MAX_CANDIDATES, unknown flag bits, lobes 0 or unknown with
 * RTR_RIS_MIS or non-zero without it, non-zero _reserved words, outCandidates without outTargets or the reverse, what
 * rtr_pick_slots_power and rtr_shade_hits_picked refuse of params and pick, numHits * P * M past 32 bits, an output that overlaps an
 * input or another output, a scene on another device. */
int  rtr_pick_slots_ris_async(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const RtrHit* hits, uint32_t numHits,
                              const rtr_light_params* params, const rtr_pick_params* pick, const rtr_ris_params* ris, const uint32_t* seeds,
                              uint32_t* outSlots, float* outWeights, uint32_t* outCandidates, float* outTargets);
int  rtr_pick_slots_ris(rtr_ctx* ctx, const rtr_scene* scene, const RtrRay* rays, const RtrHit* hits, uint32_t numHits,
                        const rtr_light_params* params, const rtr_pick_params* pick, const rtr_ris_params* ris, const uint32_t* seeds,
                        uint32_t* outSlots, float* outWeights, uint32_t* outCandidates, float* outTargets);
/* The host forms of include/rtr_ris.h in plain loops, HOST pointers, no device; the device's words equal these.
 * rtr_host_ris_candidates: outCandidates[(k * P + p) * M + j], the slots rtr_pick_slots_ris draws for a table handed in (cdf, tris: as
 * rtr_host_pick_slots_power takes them).
 * rtr_host_ris_select: the reservoir over candidates and targets handed in ([(k * P + p) * M + j]; a candidate that is RTR_PICK_NONE, is
 * not a slot of the table, lies on a triangle of weight 0 or, with RTR_RIS_MIS, has a wPick that is not finite or not > 0 is passed over) -> outSlots, outWeights [k * P + p].  wPick: with
 * RTR_RIS_MIS the wPick of every candidate (the targets already contain it; the weight carries the held one), NULL without. */
int  rtr_host_ris_candidates(const uint64_t* cdf, uint32_t tris, const uint32_t* seeds, uint32_t numHits, const rtr_light_params* params,
                             const rtr_pick_params* pick, uint32_t numCandidates, uint32_t* outCandidates);
int  rtr_host_ris_select(const uint64_t* cdf, uint32_t tris, const uint32_t* seeds, uint32_t numHits, const rtr_light_params* params,
                         const rtr_pick_params* pick, const rtr_ris_params* ris, const uint32_t* candidates, const float* targets,
                         const float* wPick, uint32_t* outSlots, float* outWeights);

/* ---- errors --------------------------------------------------------------------------- */
const char* rtr_last_error(void);
const char* rtr_status_string(int status);
int         rtr_abi_version(void);
/* Revision tag of the any-hit kernel + the tree layout it walks (bumped when either changes); measurement files carry it. */
const char* rtr_kernel_revision(void);

#ifdef __cplusplus
}
#endif
#endif /* RTR_H */
