/* rtr_types.h — plain-old-data layouts shared by the host scene layer, the C ABI,
 * the HIP kernels and the CPU oracle.  All little-endian fp32 / u32.
 *
 * Every struct here is byte-for-byte the layout the reference hands to its GPU
 * (SURVEY.md Appendix A); the reference file:line each one mirrors is cited.
 * No glm, no Vulkan types: a 3x4 row-major float matrix replaces
 * vk::TransformMatrixKHR, float[3]+pad replaces glm::vec3+pad.
 */
#ifndef RTR_TYPES_H
#define RTR_TYPES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* reference: src/scene/geometry/vertex.cppm:11-15, src/shaders/raycommon.glsl:4-8 (48 B) */
typedef struct RtrVertex {
    float position[3]; float pad0;
    float normal[3];   float pad1;
    float uv[2];       float pad2[2];
} RtrVertex;

/* reference: src/scene/camera.cppm:21-26, src/shaders/raycommon.glsl:10-15 (64 B) */
typedef struct RtrCameraData {
    float position[3];                float _pad0;
    float topLeftViewportCorner[3];   float _pad1;
    float horizontalViewportDelta[3]; float _pad2;
    float verticalViewportDelta[3];   float _pad3;
} RtrCameraData;

/* reference: src/scene/scene_info.cppm:10-20, src/shaders/raygen.rgen:35-43 (32 B push constant) */
typedef struct RtrSceneInfo {
    uint32_t frame;
    uint32_t numAreaLights;
    uint32_t _pad0;
    uint32_t _pad1;
    float    camPosition[3];
    float    pad2_;
} RtrSceneInfo;

/* reference: src/scene/object.cppm:21-44, src/shaders/raycommon.glsl:29-51 (80 B) */
typedef struct RtrObjectInfo {
    uint32_t vertexOffset;
    uint32_t indexOffset;
    float    pad0_[2];
    uint32_t usesColorMap;
    uint32_t usesSpecularMap;
    uint32_t usesMetallicMap;
    uint32_t usesOpacityMap;
    uint32_t colorIndex;
    uint32_t specularIndex;
    uint32_t metallicIndex;
    uint32_t opacityIndex;
    float    color[3];
    float    pad1_;
    float    specular;
    float    metallic;
    float    pad3_[2];
} RtrObjectInfo;

/* reference: src/scene/area_light.cppm:23-33, src/shaders/raycommon.glsl:53-63 (96 B).
 * transform is a column-major mat4 (element [c*4+r]), packed as in src/core/utils.cppm:11-39. */
typedef struct RtrAreaLightInfo {
    float    color[3];
    float    intensity;
    uint32_t vertexOffset;
    uint32_t indexOffset;
    uint32_t numTriangles;
    uint32_t isTwoSided;
    float    transform[16];
} RtrAreaLightInfo;

/* reference: src/app/structs.cppm:14-21, src/shaders/denoise.comp:9-16 (24 B) */
typedef struct RtrDenoisingInfo {
    int32_t step_width;
    float   c_phi;
    float   n_phi;
    float   p_phi;
    int32_t denoisedImagesAreOutput;
    int32_t isShadowedImage;
} RtrDenoisingInfo;

/* One mesh = one BLAS in the reference (src/vulkan/raytracing/blas.cppm:75-167;
 * BLASCreateInfo filled at src/app/setup/geometry_builder.cppm:98-112, src/core/file.cppm:254-267).
 * Offsets are element indices into the concatenated vertex / index arrays; indices are mesh-local. */
typedef struct RtrMesh {
    uint32_t vertexOffset;   /* vertexIndexOffset */
    uint32_t indexOffset;    /* indexIndexOffset  */
    uint32_t vertexCount;
    uint32_t indexCount;     /* 3 * triangles */
    uint32_t isOpaque;       /* BLAS geometry OPAQUE flag (blas.cppm:98-100) */
    uint32_t _pad[3];
} RtrMesh;

/* One TLAS instance (src/vulkan/raytracing/tlas.cppm:52-82): lights first, then objects;
 * customIndex = position in that list; transform = 3x4 row-major object->world. */
typedef struct RtrInstance {
    uint32_t meshIndex;
    uint32_t customIndex;
    uint32_t _pad[2];
    float    transform[12];  /* row-major 3x4: m[r*4+c] */
} RtrInstance;

/* ---- device BVH layout, version 3 ("BVH2 / children-in-parent / 32 B, 16-bit planes on a scene grid") ----------
 * One node holds the boxes of BOTH children, each plane quantised OUTWARD to a 16-bit coordinate of the scene-wide
 * grid `RtrBvhGrid` (plane = origin + q * scale per axis), so a visit is one 32-B fetch (2 x dwordx4): the traversal
 * kernels are bound by the bytes they pull through the vector-memory path, and version 2 (fp32 planes, 64 B) cost
 * 21 % more time in the dominant kernel.  Boxes only have to be conservative — the hit a ray reports is decided by the
 * triangle tests alone — so rendered results do not depend on the quantisation.
 *   q[side*4 + isMax*2 + axis]   axis = 0 (x), 1 (y);  side 0 = left child, 1 = right child
 *   q[8 + side*2 + isMax]        axis = 2 (z)
 *   i.e. as 32-bit words: (lminx|lminy<<16) (lmaxx|lmaxy<<16) (rminx|rminy<<16) (rmaxx|rmaxy<<16) (lminz|lmaxz<<16)
 *   (rminz|rmaxz<<16) — the pairing lets one packed FMA decode-and-slab two planes.
 *   child[0], child[1]: >= 0 -> index of an inner node;
 *                       <  0 -> leaf: code = ~child; first = code >> 3; count = (code & 7) + 1
 *   The root is always an inner node: a scene with a single leaf stores that leaf as BOTH children (testing a
 *   triangle twice cannot change the (t, id)-minimal hit); an empty scene holds one degenerate triangle.
 */
#define RTR_BVH_LAYOUT_VERSION 3
#define RTR_BVH_MAX_LEAF 8
#define RTR_BVH_NODE_BYTES 32   /* bytes a node visit fetches (the N_node coefficient of the algorithmic-byte formulas) */
typedef struct RtrBvhNode {
    uint16_t q[12];
    int32_t  child[2];
} RtrBvhNode;
#define RTR_BVH_QSLOT(side, isMax, axis) ((axis) < 2 ? (side) * 4 + (isMax) * 2 + (axis) : 8 + (side) * 2 + (isMax))

/* The grid the planes of every node live on (one per scene; rewritten by a refit). */
typedef struct RtrBvhGrid {
    float origin[3]; uint32_t wideCentreXY;    /* x | y << 16: grid coordinate the planes of the 4-wide records are offsets from (below) */
    float scale[3];  uint32_t wideCentreZ;     /* z */
} RtrBvhGrid;

/* ---- 4-wide view of the same tree (layout W4.0): what the any-hit kernel walks (k_shadow_trace4) ---------------------------
 * One 64-B record = a collapsed subtree of the BVH2 (greedy: open the inner child with the largest box while a slot is free):
 * up to four child boxes and their four child codes, so a ray makes about half as many DEPENDENT visits.  A plane is stored as
 * a HALF FLOAT: its offset in grid steps from the scene's WIDE CENTRE c (q - c; RtrBvhGrid::wideCentreXY / Z: per axis the mean midpoint of
 * the tree's leaf boxes, so the half floats are finest where the geometry is), rounded outward to 11 significant bits
 * (exact within 2048 steps of c, 2^-11 of the distance from it beyond; a magnitude above 65504 becomes infinite), so that its parameter on a ray is ONE
 * instruction, t = fma(f16 plane, ga, gbc) with v_fma_mix_f32, no conversion (ga, gbc: rtr_ray_grid_centre).  Exported records are in breadth-first order; record 0 is
 * the root.  On the device they are in the resident order (rtr_scene_export_wide_resident: a best-first top towards the lights, which
 * the kernel keeps in LDS, then breadth-first).  Built on the device after every build / refit (kernels/rtr_bvh.hip: k_wide_nodes, k_permute_wide).
 *   plane[k] : slot k: (xmin | ymin << 16) (xmax | ymax << 16) (zmin | zmax << 16), IEEE binary16 each
 *   child[k] : >= 0 index of a record of this array; < 0 leaf code as in RtrBvhNode (triangles in the same leaf-ordered array);
 *              0x80000000 = empty slot (slots 0 and 1 are never empty); its planes are min = +inf, max = -inf: an inside-out box
 *              no ray enters when the entry / exit planes are picked by the ray's direction signs (the kernel's octant forms)
 */
#define RTR_WIDE_LAYOUT_VERSION 45
#define RTR_WIDE_NODE_BYTES 64
/* entries of the per-ray stack the any-hit kernel keeps in LDS while it walks the wide view; a ray that holds more after a visit is
 * redone over the BVH2 (k_shadow_tail).  Part of the definition of a ray's walk (the counting form and the oracle follow it). */
#ifndef RTR_WIDE_STACK
#define RTR_WIDE_STACK 16
#endif
#define RTR_WIDE_EMPTY ((int32_t)0x80000000)
typedef struct RtrWideNode {
    uint32_t plane[4][3];
    int32_t  child[4];
} RtrWideNode;

/* 48-B world-space Moeller-Trumbore record, in BVH leaf order.
 * v0 / e1 = v1-v0 / e2 = v2-v0 in world space; the three w slots carry the ids the
 * reference's hit shaders read (gl_InstanceCustomIndexEXT, gl_PrimitiveID) and flags. */
typedef struct RtrBvhTri {
    float    v0[3]; uint32_t customIndex;
    float    e1[3]; uint32_t primitiveId;
    float    e2[3]; uint32_t flags;      /* bit0: alpha-tested (any-hit needed); bits 8..15: ~instance cull mask (below); others 0 */
} RtrBvhTri;
/* Bits 8..15 of RtrBvhTri::flags hold the COMPLEMENT of the 8-bit cull mask of the record's instance (rtr_scene_set_instance_masks;
 * VkAccelerationStructureInstanceKHR::mask, reference src/vulkan/raytracing/tlas.cppm:63): the default mask 0xff is stored as 0, so the
 * records of a scene whose masks were never set are what every builder has always written.  The record exists for a ray with the 8-bit
 * mask m iff ((m << RTR_TRI_MASK_SHIFT) & ~flags) != 0.  Only the masked ray queries read the bits; the renderer reads bit 0 alone. */
#define RTR_TRI_MASK_SHIFT 8u
#define RTR_TRI_MASK_BITS  (0xffu << RTR_TRI_MASK_SHIFT)

/* ---- ray queries (rtr_trace_rays): one caller-supplied ray and its closest hit ---------------------------------------------
 * What traceRayEXT takes (origin, tMin, direction, tMax: reference src/shaders/raygen.rgen:99-107) and what its hit shader reads
 * (gl_HitTEXT, the barycentrics of hitAttributeEXT, gl_InstanceCustomIndexEXT, gl_PrimitiveID: closesthit.rchit:45-56), 32 B each
 * so that a lane moves its record as two 16-B accesses.  The direction need not be normalised; t is in its units. */
typedef struct RtrRay {
    float origin[3];    float tmin;
    float direction[3]; float tmax;
} RtrRay;

/* A miss: customIndex = primitiveId = 0xffffffff, t = the ray's tmax, u = v = 0.  _reserved is written as 0. */
typedef struct RtrHit {
    float    t, u, v;
    uint32_t customIndex;
    uint32_t primitiveId;
    uint32_t _reserved[3];
} RtrHit;

/* ---- hit surfaces (rtr_hit_surfaces): what the closest-hit shader computes for one RtrHit ----------------------------------
 * closesthit.rchit:53-106 for an object, and the light-hit and miss rules of raygen.rgen:110-121 / miss.rmiss:15-27.  80 B, so a lane
 * writes its record as five 16-B stores.  Per kind:
 *   RTR_SURFACE_OBJECT   position, normal, color (linear), roughness, metallic: the renderer's hit point, shading normal (with its
 *                        geometric fallback, turned against the ray), colour and material; uv: the interpolated texture coordinate;
 *                        geomNormal: normalize(nmat * normalize(cross(p1 - p0, p2 - p0))), as wound, never turned.
 *                        objectIndex = customIndex - numLights (the ObjectInfo row).
 *   RTR_SURFACE_LIGHT    color: the light's colour; position: (u, v) over the light triangle's world-space corners; normal = geomNormal:
 *                        that triangle's unit normal; the other floats 0.  objectIndex = the light index.
 *   RTR_SURFACE_MISS     color: the sky radiance in the ray's direction (HDRI or the constant sky); every other float 0.
 *   RTR_SURFACE_INVALID  a customIndex that is neither, or a primitiveId past the instance's (light's) triangles: every float 0.
 * objectIndex is 0xffffffff for MISS and INVALID; _reserved is written as 0. */
#define RTR_SURFACE_MISS    0u
#define RTR_SURFACE_OBJECT  1u
#define RTR_SURFACE_LIGHT   2u
#define RTR_SURFACE_INVALID 3u

typedef struct RtrSurface {
    float    position[3];   uint32_t kind;
    float    normal[3];     uint32_t objectIndex;
    float    geomNormal[3]; float    metallic;
    float    color[3];      float    roughness;
    float    uv[2];         uint32_t _reserved[2];
} RtrSurface;

/* ---- direct lighting (rtr_shade_hits): one primary sample's contribution, as the ray-gen shader forms it -------------------
 * The three sums of raygen.rgen:165-338 for one RtrHit — shadowed (what the framebuffer shows), unshadowed (every sample counted as
 * visible) and analytic (the LTC term) — before the division by the samples per pixel and the tone map.  48 B, three 16-B stores.
 * kind: the RTR_SURFACE_* of the hit.  A sum that was not asked for (rtr_light_params.outputs) is written as zeros; _r0, _r1 as 0. */
typedef struct RtrRadiance {
    float    shadowed[3];   uint32_t kind;
    float    unshadowed[3]; uint32_t _r0;
    float    analytic[3];   uint32_t _r1;
} RtrRadiance;

/* ---- continuation rays (rtr_bounce_rays): one BRDF-sampled direction per hit and its throughput weight ------------------------
 * What a path tracer multiplies its throughput by when it follows RtrRay next from the hit: weight = BRDF * cos / pdf per channel, the
 * renderer's Cook-Torrance BRDF (include/rtr_bounce.h), pdf = the mixture density the direction was drawn from.  32 B, two 16-B stores.
 * A DEAD record — no continuation: not an object, a direction below the surface, a non-finite input — is 32 zero bytes beside the null
 * ray.  lobe: the RTR_BOUNCE_* lobe the direction was drawn from, 0 when dead; pSpecular: the probability the specular lobe had. */
#define RTR_BOUNCE_DIFFUSE  1u
#define RTR_BOUNCE_SPECULAR 2u
typedef struct RtrBounce {
    float    weight[3]; float pdf;
    uint32_t lobe;      float pSpecular; uint32_t _reserved[2];
} RtrBounce;

typedef struct rtr_bounce_params {
    uint32_t frame, depth;    /* enter every seed: s0 = seedBase + frame + 7919 * (depth + 1) */
    uint32_t width, spp;      /* hit k belongs to pixel ((k / spp) % width, (k / spp) / width), as in rtr_light_params.  Used when seeds == NULL */
    uint32_t lobes;           /* RTR_BOUNCE_DIFFUSE | RTR_BOUNCE_SPECULAR: the lobes that may be sampled */
    float    normalOffset, tmin, tmax;   /* the next ray: origin position + normalOffset * normal, [tmin, tmax].  The shader's shadow rays: 0.01, 0.001, 10000 */
} rtr_bounce_params;          /* 32 bytes */

/* ---- path compaction (rtr_compact_paths): the live paths of a wavefront, gathered to the front in their order ------------------
 * frame and depth enter the roulette's seed: u = rtr_random(seed + frame + 7919 * (depth + 1) + 300), the fourth random number of the
 * vertex whose rtr_bounce_rays took + 0, + 100 and + 200.  flags: RTR_COMPACT_ROULETTE or 0.  survivalFloor: the least survival
 * probability of the roulette, in (0, 1] (read only with the flag).  throughputStrideBytes: the distance between two paths' throughputs
 * in the INPUT, a multiple of 4 and at least 12 (32: the weight column of RtrBounce records as they are).  _reserved must be 0.
 * RTR_PATH_NONE is the path id of an output slot behind the survivors.  The rule itself is include/rtr_paths.h. */
#define RTR_COMPACT_ROULETTE 1u
#define RTR_PATH_NONE 0xffffffffu
typedef struct rtr_compact_params {
    uint32_t frame, depth, flags;
    float    survivalFloor;
    uint32_t throughputStrideBytes;
    uint32_t _reserved[3];
} rtr_compact_params;         /* 32 bytes */

/* ---- path accumulation (rtr_accumulate_paths): one vertex's radiance added to the image, and the throughput after its bounce --------
 * flags: with RTR_ACCUM_LIGHTS_FROM_EMITTERS a path whose hit is a light takes its radiance from the RtrEmitter records (0 without
 * them) instead of RtrRadiance::shadowed; with RTR_ACCUM_MISSES_FROM_ESCAPES a path that missed takes it from the RtrSkyEscape records
 * in the same way.  The rule itself is include/rtr_accum.h. */
#define RTR_ACCUM_LIGHTS_FROM_EMITTERS 1u
#define RTR_ACCUM_MISSES_FROM_ESCAPES  2u
typedef struct rtr_accum_params {
    uint32_t flags;
    uint32_t numSlots;               /* rows of accum / outTerm; a path whose id is >= numSlots touches neither image */
    uint32_t throughputStrideBytes;  /* input T: a multiple of 4, at least 12, as in rtr_compact_params */
    uint32_t imageStrideBytes;       /* accum and outTerm: a multiple of 4, at least 12 (12: an (N,3) tensor; 16: float4) */
    uint32_t _reserved[4];           /* must be 0 */
} rtr_accum_params;                  /* 32 bytes */

/* ---- picked light samples (rtr_light_rays_picked, rtr_shade_hits_picked): numPicks of a hit's area-light slots instead of all ---
 * A hit's AREA SLOTS are the first A = Q - 1 slots of rtr_light_slots, numbered the same way: slot j is sample j % numShadowRays of
 * light triangle j / numShadowRays.  numPicks (P, 1 ... RTR_PICK_MAX) of them are drawn per hit — pick p by
 * u = rtr_random(seedBase + frame + 7919 * (depth + 1) + 400 + 100 * p), slot (uint32_t)(u * A) clamped to A - 1 — or handed in by the
 * caller; the directional light is never picked, it keeps a ray of its own.  depth enters the seed as in rtr_bounce_params; _reserved
 * must be 0.  RTR_PICK_NONE: no slot (what is drawn when A == 0; a caller's way to leave a pick out).  A may be at most
 * RTR_PICK_MAX_SLOTS, so that every slot can be drawn from a float.  The rule itself is include/rtr_pick.h. */
#define RTR_PICK_MAX       30u
#define RTR_PICK_NONE      0xffffffffu
#define RTR_PICK_MAX_SLOTS (1u << 24)
typedef struct rtr_pick_params {
    uint32_t numPicks, depth;
    uint32_t _reserved[6];
} rtr_pick_params;            /* 32 bytes */

/* ---- multiple importance sampling at a path vertex (rtr_mis_pick_weights, rtr_emitter_hits; the rule is include/rtr_mis.h) -----------
 * The balance heuristic over the numPicks (P) picked light samples of a vertex and its one bounce sample.  numAreaLights, numShadowRays:
 * rtr_light_params' of the picks (Ttot = the triangles of the first numAreaLights lights; slot j belongs to light triangle
 * j / numShadowRays); lobes: rtr_bounce_params::lobes of the bounce.  _reserved must be 0.
 * RtrMisSample: what the pick side used for one pick — the solid-angle density of the pick (lightPdf, 0 where it is not finite) and of
 * the bounce (bouncePdf) for the pick's direction, the MIS weight wPick, cosLight = dot(n_t, -dir), the distance, the light triangle's
 * area and its record (lightTri); 32 zero bytes for a pick without a ray.
 * RtrEmitter: what a bounce ray that ends on a light adds, to be multiplied by the throughput after the bounce; kind = RTR_SURFACE_LIGHT
 * on a record that counts, 32 zero bytes otherwise. */
typedef struct rtr_mis_params {
    uint32_t numPicks, numAreaLights, numShadowRays, lobes;
    uint32_t _reserved[4];
} rtr_mis_params;             /* 32 bytes */

typedef struct RtrMisSample {
    float    lightPdf, bouncePdf, wPick, cosLight;
    float    dist, area; uint32_t lightTri, _r;
} RtrMisSample;

typedef struct RtrEmitter {
    float    radiance[3]; float wBounce;
    float    lightPdf, dist; uint32_t lightTri, kind;
} RtrEmitter;

/* ---- resampled light picks at a path vertex (rtr_pick_slots_ris; the rule is include/rtr_ris.h) --------------------------------------
 * Each of a vertex's picks is chosen among numCandidates (M, 1 ... RTR_RIS_MAX_CANDIDATES) draws from the light-power table in proportion
 * to the unshadowed contribution each would make at the vertex.  flags: RTR_RIS_MIS (the picks are weighted against the vertex's bounce,
 * whose ray then counts the lights it meets: rtr_emitter_hits_power) or 0.  lobes: rtr_bounce_params::lobes of that bounce, required with
 * the flag and 0 without it.  _reserved must be 0. */
#define RTR_RIS_MAX_CANDIDATES 16u
#define RTR_RIS_MIS            1u
typedef struct rtr_ris_params {
    uint32_t numCandidates, flags, lobes;
    uint32_t _reserved[5];
} rtr_ris_params;             /* 32 bytes */

/* ---- sky importance sampling at a path vertex (rtr_sky_rays, rtr_shade_sky, rtr_sky_hits; the rule is include/rtr_sky.h) --------------
 * numSamples (S, 1 ... RTR_SKY_MAX_SAMPLES) directions per vertex drawn in proportion to the scene's sky table.  depth and frame enter
 * the seed as in rtr_bounce_params (sample j takes the offsets 3400 + 200 j and 3500 + 200 j); width, spp: the pixel rule, used when
 * seeds == NULL; lobes: rtr_bounce_params::lobes of the vertex's bounce; flags: RTR_SKY_MIS (the balance heuristic against that bounce)
 * or 0.  _reserved must be 0.  rtr_sky_hits takes numSamples 0 as well: a vertex that drew no sky sample.
 * RtrSkySample: contrib = f cos sky / (S skyPdf + bouncePdf) (without the flag: / (S skyPdf)), to be multiplied by the throughput and
 * added where the sample's ray is not occluded; skyPdf, bouncePdf: the solid-angle densities of the sky table and of the bounce for the
 * sample's direction; wSky = S skyPdf / (S skyPdf + bouncePdf) (1 without the flag); cell = y * W + x of the table.  A DEAD sample is 32
 * zero bytes beside the null ray.
 * RtrSkyEscape: what a bounce ray that MISSED adds, to be multiplied by the throughput after the bounce: radiance = sky * wBounce,
 * wBounce = bouncePdf / (S skyPdf + bouncePdf) (1 without the flag or with S == 0).  kind = RTR_SURFACE_MISS on a record that counts, 32
 * zero bytes otherwise. */
#define RTR_SKY_MAX_SAMPLES 8u
#define RTR_SKY_MIS         1u
typedef struct rtr_sky_params {
    uint32_t numSamples, depth, frame, width;
    uint32_t spp, lobes, flags, _reserved;
} rtr_sky_params;             /* 32 bytes */

/* a sky table as the calls that take one read it (rtr_host_sky_table and rtr_scene_export_sky_table fill the two arrays): rows[y *
 * width + x], the inclusive prefix sums of row y's cell weights; marginal[y], the inclusive prefix sums of the row totals */
typedef struct rtr_sky_table {
    const uint32_t* rows;
    const uint64_t* marginal;
    uint32_t width, height;
} rtr_sky_table;

typedef struct RtrSkySample {
    float    contrib[3]; float skyPdf;
    float    bouncePdf, wSky; uint32_t cell, _r;
} RtrSkySample;

typedef struct RtrSkyEscape {
    float    radiance[3]; float wBounce;
    float    skyPdf, bouncePdf; uint32_t cell, kind;
} RtrSkyEscape;

#ifdef __cplusplus
}
#endif

#ifdef __cplusplus
static_assert(sizeof(RtrVertex) == 48, "Vertex must be 48 B");
static_assert(sizeof(RtrCameraData) == 64, "GPUCameraData must be 64 B");
static_assert(sizeof(RtrSceneInfo) == 32, "SceneInfo must be 32 B");
static_assert(sizeof(RtrObjectInfo) == 80, "GPUObjectInfo must be 80 B");
static_assert(sizeof(RtrAreaLightInfo) == 96, "GPUAreaLightInfo must be 96 B");
static_assert(sizeof(RtrDenoisingInfo) == 24, "DenoisingInfo must be 24 B");
static_assert(sizeof(RtrBvhNode) == 32, "BVH node must be 32 B");
static_assert(sizeof(RtrBvhGrid) == 32, "BVH grid record must be 32 B");
static_assert(sizeof(RtrBvhTri) == 48, "BVH triangle must be 48 B");
static_assert(sizeof(RtrWideNode) == 64, "wide node must be 64 B");
static_assert(sizeof(RtrRay) == 32, "ray must be 32 B");
static_assert(sizeof(RtrHit) == 32, "hit must be 32 B");
static_assert(sizeof(RtrSurface) == 80, "surface must be 80 B");
static_assert(sizeof(RtrRadiance) == 48, "radiance must be 48 B");
static_assert(sizeof(RtrBounce) == 32, "bounce record must be 32 B");
static_assert(sizeof(rtr_bounce_params) == 32, "bounce params must be 32 B");
static_assert(sizeof(rtr_compact_params) == 32, "compact params must be 32 B");
static_assert(sizeof(rtr_accum_params) == 32, "accum params must be 32 B");
static_assert(sizeof(rtr_pick_params) == 32, "pick params must be 32 B");
static_assert(sizeof(rtr_mis_params) == 32, "mis params must be 32 B");
static_assert(sizeof(RtrMisSample) == 32, "mis sample must be 32 B");
static_assert(sizeof(RtrEmitter) == 32, "emitter record must be 32 B");
static_assert(sizeof(rtr_ris_params) == 32, "ris params must be 32 B");
static_assert(sizeof(rtr_sky_params) == 32, "sky params must be 32 B");
static_assert(sizeof(RtrSkySample) == 32, "sky sample must be 32 B");
static_assert(sizeof(RtrSkyEscape) == 32, "sky escape record must be 32 B");
#endif

#endif /* RTR_TYPES_H */
