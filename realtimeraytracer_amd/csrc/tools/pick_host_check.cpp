/* pick_host_check — rtr_host_pick_slots under the host sanitizers: a stand-alone program around rtr_pick_host.cpp, built with
 * -fsanitize=address,undefined by `make pick_host_check` (never part of a library, never loaded into Python).  It draws the slots of
 * 1 ... 20000 hits for every number of picks, with explicit seeds and with the pixels', for area-slot counts from 0 to 2^24, on exactly
 * sized heap arrays so that a read or write past an array is caught; checks that every slot is below A (RTR_PICK_NONE at A == 0) and
 * equals the header's function of its seed; the argument checks the device entry points share; and every kind of refusal.  Exit
 * status 0 and "ok" when nothing was reported. */
#include "../rtr_pick_host.h"
#include "host_check.h"
#include "../../../include/rtr_pick.h"

#include <cstring>

int main() {
    const uint32_t sizes[7] = {1, 63, 64, 65, 257, 4099, 20000};
    const uint32_t areas[8] = {0, 1, 2, 6, 13, 1000, (1u << 24) - 1u, 1u << 24};
    const uint32_t picks[4] = {1, 2, 7, RTR_PICK_MAX};
    int bad = 0;
    size_t runs = 0, slots = 0;
    for (uint32_t n : sizes)
        for (uint32_t A : areas)
            for (uint32_t P : picks)
                for (int withSeeds = 0; withSeeds < 2; ++withSeeds) {
                    uint32_t* seeds = static_cast<uint32_t*>(malloc((size_t)n * 4));
                    uint32_t* out = static_cast<uint32_t*>(malloc((size_t)n * P * 4));
                    uint32_t s = 7u + n + A + P;
                    for (uint32_t k = 0; k < n; ++k) seeds[k] = (k & 1u) ? lcg(s) : 0xfffffff0u + k;      /* sums that wrap among them */
                    memset(out, 0xA5, (size_t)n * P * 4);
                    rtr_pick_params pp{};
                    pp.numPicks = P; pp.depth = n % 5u;
                    const uint32_t frame = 0xffffff00u + P, width = 37u, spp = 2u;
                    const int rc = rtr_host_pick_slots(withSeeds ? seeds : nullptr, n, frame, width, spp, &pp, A, out);
                    ++runs;
                    if (rc != RTR_OK) { fprintf(stderr, "rtr_host_pick_slots: %d %s\n", rc, g_err.c_str()); return 1; }
                    for (uint32_t k = 0; k < n && !bad; ++k)
                        for (uint32_t p = 0; p < P; ++p) {
                            const uint32_t j = out[(size_t)k * P + p];
                            const uint32_t pix = k / spp, base = withSeeds ? seeds[k] : (pix % width) * 733u + (pix / width) * 1933u;
                            const uint32_t want = rtr_pick_slot_of(rtr_random(base + frame + 7919u * (pp.depth + 1u) + 400u + 100u * p), A);
                            if (j != want || (A ? j >= A : j != RTR_PICK_NONE)) {
                                fprintf(stderr, "n %u A %u P %u hit %u pick %u: slot %u, expected %u\n", n, A, P, k, p, j, want);
                                ++bad;
                                break;
                            }
                            ++slots;
                        }
                    free(seeds); free(out);
                }
    /* the clamp: u == 1.0 and the largest u below it */
    if (rtr_pick_slot_of(1.0f, 6u) != 5u || rtr_pick_slot_of(0.99999994f, 6u) != 5u || rtr_pick_slot_of(0.0f, 6u) != 0u ||
        rtr_pick_slot_of(1.0f, 1u << 24) != (1u << 24) - 1u || rtr_pick_slot_of(0.5f, 0u) != RTR_PICK_NONE) { fprintf(stderr, "rtr_pick_slot_of: the clamp\n"); ++bad; }

    uint32_t out[64], seeds[32];
    memset(seeds, 0, sizeof seeds);
    rtr_pick_params p{};
    p.numPicks = 2;
    rtr_pick_params q = p;
    int refusals = 0;
    const char* who = "rtr_host_pick_slots";
    REFUSED(rtr_host_pick_slots(seeds, 32, 0, 0, 0, nullptr, 6, out), who, "pick params is null");
    q = p; q.numPicks = 0; REFUSED(rtr_host_pick_slots(seeds, 32, 0, 0, 0, &q, 6, out), who, "numPicks 0");
    q = p; q.numPicks = RTR_PICK_MAX + 1u; REFUSED(rtr_host_pick_slots(seeds, 32, 0, 0, 0, &q, 6, out), who, "numPicks 31");
    q = p; q._reserved[5] = 1; REFUSED(rtr_host_pick_slots(seeds, 32, 0, 0, 0, &q, 6, out), who, "_reserved");
    REFUSED(rtr_host_pick_slots(seeds, 32, 0, 0, 0, &p, (1u << 24) + 1u, out), who, "area slots");
    REFUSED(rtr_host_pick_slots(seeds, 32, 0, 0, 0, &p, 6, nullptr), who, "outSlots is null");
    REFUSED(rtr_host_pick_slots(seeds, 32, 0, 0, 0, &p, 6, reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(out) + 2)), who, "outSlots is not 4-B aligned");
    REFUSED(rtr_host_pick_slots(reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(seeds) + 1), 31, 0, 0, 0, &p, 6, out), who, "seeds is not 4-B aligned");
    REFUSED(rtr_host_pick_slots(nullptr, 32, 0, 0, 1, &p, 6, out), who, "width 0");
    REFUSED(rtr_host_pick_slots(nullptr, 32, 0, 8, 0, &p, 6, out), who, "spp 0");
    REFUSED(rtr_host_pick_slots(seeds, 0xffffffffu, 0, 0, 0, &p, 6, out), who, "do not fit 32 bits");
    if (rtr_host_pick_slots(nullptr, 0, 0, 0, 0, &p, 6, nullptr) != RTR_OK) ++bad;

    /* the checks the device entry points share */
    rtr_light_params lp{};
    lp.numShadowRays = 3; lp.width = 8; lp.spp = 1; lp.outputs = RTR_LIGHT_SHADOWED;
    if (rtrdev::pick_check_params("f", &lp, &p, true) != RTR_OK) ++bad;
    rtr_light_params lq = lp;
    lq.outputs |= RTR_LIGHT_ANALYTIC;
    if (rtrdev::pick_check_params("f", &lq, &p, true) != RTR_ERR_UNSUPPORTED) ++bad;
    if (rtrdev::pick_check_params("f", &lq, &p, false) != RTR_OK) ++bad;
    lq = lp; lq.numShadowRays = 1025;
    if (rtrdev::pick_check_params("f", &lq, &p, false) != RTR_ERR_INVALID_ARGUMENT) ++bad;
    alignas(16) static RtrRay rays[2];
    alignas(16) static RtrHit hits[2];
    alignas(16) static RtrRadiance rad[2];
    uint8_t occ[6];
    float w[4];
    rtrdev::PickCall c{rays, hits, 2, &lp, &p, nullptr, false, nullptr, rays, out, nullptr, nullptr, nullptr};
    if (rtrdev::pick_check_arrays("f", c) != RTR_OK) ++bad;
    c.outSlots = nullptr;
    bad += expect_refused(rtrdev::pick_check_arrays("f", c), "f", "outSlots is null");
    rtrdev::PickCall d{rays, hits, 2, &lp, &p, seeds, true, out, nullptr, nullptr, w, occ, rad};
    if (rtrdev::pick_check_arrays("f", d) != RTR_OK) ++bad;
    d.slots = nullptr;
    bad += expect_refused(rtrdev::pick_check_arrays("f", d), "f", "slots is null");
    d.slots = out; d.n = 0x10000000u;
    if (rtrdev::pick_check_arrays("f", d) != RTR_OK) ++bad;                /* 2^28 x 3 fits */
    d.n = 0x60000000u;
    bad += expect_refused(rtrdev::pick_check_arrays("f", d), "f", "do not fit 32 bits");

    if (bad) { fprintf(stderr, "%d problems\n", bad); return 1; }
    printf("ok: %zu runs, %zu slots, %d refusals\n", runs, slots, refusals);
    return 0;
}
