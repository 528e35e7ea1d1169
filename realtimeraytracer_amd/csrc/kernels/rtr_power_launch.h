/* rtr_power_launch.h — host-callable launchers of the light-power kernels (kernels/rtr_power.hip; internal to librtr_hip.so). */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../../include/rtr_types.h"

namespace rtrdev {

/* light triangles one pass of the scan's single workgroup covers (its size); a longer table goes on with the carry of the passes before */
constexpr uint32_t kPowerScanChunk = 256;

/* the scene's power table on the device: weights[t], cdf[t] for all numTris light triangles of all lights; maxBits: one word, the
 * largest pw of the build in flight as the bits of a non-negative float, 0 between builds (the scan puts it back) */
struct PowerTable {
    uint32_t* weights;
    uint64_t* cdf;
    uint32_t* maxBits;
    uint32_t numTris;
};

struct PowerPickArgs {
    const uint64_t* cdf;
    const uint32_t* seeds;           /* or null: the pixel rule */
    uint32_t* outSlots;              /* n x P */
    float* outWeights;               /* n x P */
    uint32_t tris;                   /* Ttot: the triangles of the first numAreaLights lights */
    uint32_t numShadowRays, frame, width, spp;
    uint32_t picks, depth;
    uint32_t n;
};

/* The two launches of the table build, from the light-triangle records and the light infos as they are when the stream gets there:
 * pw_t and their maximum, then the weights and their 64-bit inclusive sums.  No allocation, no join. */
hipError_t launch_light_power(const float4* lightTris, const uint32_t* lightTriFirst, const RtrAreaLightInfo* lights, uint32_t numLights,
                              const PowerTable& t, hipStream_t stream);
/* per hit and pick: the slot drawn from the table and its plain weight (include/rtr_power.h) */
hipError_t launch_pick_slots_power(const PowerPickArgs& a, hipStream_t stream);

}  // namespace rtrdev
