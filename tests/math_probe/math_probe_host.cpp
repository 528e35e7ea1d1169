/* math_probe_host.cpp — the op table of math_ops.h compiled for the host with the oracle's own compile line (TEST INFRASTRUCTURE;
 * built by oracle/Makefile into tests/math_probe/libmath_probe_host.so).  Exports the same calls as math_probe.hip; `device` is
 * ignored.  Threaded, with at most 16 threads. */
#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "math_ops.h"

typedef void (*probe_fn)(const uint32_t*, uint32_t*);
static const probe_fn PROBE_FN[PROBE_OP_COUNT] = {
#define X(name, nin, nout, fmask) op_##name,
    PROBE_OPS(X)
#undef X
};

template <probe_fn F, int NOUT, uint32_t FMASK>
static uint64_t sweep_chunk(uint32_t first, uint64_t b, uint64_t e, uint32_t stride) {        /* F inlines: the sweeps are the cost */
    uint64_t acc = 0;
    uint32_t r[NOUT];
    for (uint64_t i = b; i < e; ++i) {
        const uint32_t p = first + (uint32_t)i * stride;
        F(&p, r);
        acc += probe_mix(p, r, NOUT, FMASK);
    }
    return acc;
}
typedef uint64_t (*chunk_fn)(uint32_t, uint64_t, uint64_t, uint32_t);
static const chunk_fn PROBE_CHUNK_FN[PROBE_OP_COUNT] = {
#define X(name, nin, nout, fmask) nin == 1 ? sweep_chunk<op_##name, nout, fmask> : nullptr,
    PROBE_OPS(X)
#undef X
};

static unsigned thread_count(uint64_t items) {
    unsigned hw = std::thread::hardware_concurrency();
    unsigned t = std::min(16u, hw ? hw : 1u);
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(t, items));
}

extern "C" {

int math_probe_op_count(void) { return PROBE_OP_COUNT; }
const char* math_probe_op_name(int op) { return op >= 0 && op < PROBE_OP_COUNT ? PROBE_INFO[op].name : nullptr; }
int math_probe_op_nin(int op) { return op >= 0 && op < PROBE_OP_COUNT ? PROBE_INFO[op].nin : -1; }
int math_probe_op_nout(int op) { return op >= 0 && op < PROBE_OP_COUNT ? PROBE_INFO[op].nout : -1; }
uint32_t math_probe_op_fmask(int op) { return op >= 0 && op < PROBE_OP_COUNT ? PROBE_INFO[op].fmask : 0; }

int math_probe_eval(int, int op, const uint32_t* in, uint32_t n, uint32_t* out) {
    if (op < 0 || op >= PROBE_OP_COUNT || !in || !out) return -1;
    const probe_fn f = PROBE_FN[op];
    const int nin = PROBE_INFO[op].nin, nout = PROBE_INFO[op].nout;
    const unsigned T = thread_count((n + 4095u) / 4096u);
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < T; ++t)
        pool.emplace_back([=] {
            const uint64_t b = (uint64_t)n * t / T, e = (uint64_t)n * (t + 1) / T;
            for (uint64_t i = b; i < e; ++i) f(in + i * nin, out + i * nout);
        });
    for (auto& th : pool) th.join();
    return 0;
}

int math_probe_sweep(int, int op, uint32_t first, uint64_t count, uint32_t stride, uint64_t* digests) {
    if (op < 0 || op >= PROBE_OP_COUNT || !digests || count > (1ull << 32)) return -1;
    if (PROBE_INFO[op].nin != 1) return -2;
    const chunk_fn f = PROBE_CHUNK_FN[op];
    const uint64_t nd = (count + (1ull << PROBE_CHUNK_LOG2) - 1) >> PROBE_CHUNK_LOG2;
    std::atomic<uint64_t> next(0);
    std::vector<std::thread> pool;
    for (unsigned t = 0, T = thread_count(nd); t < T; ++t)
        pool.emplace_back([&] {
            for (uint64_t c; (c = next.fetch_add(1)) < nd;) {
                const uint64_t b = c << PROBE_CHUNK_LOG2, e = std::min<uint64_t>(count, b + (1ull << PROBE_CHUNK_LOG2));
                digests[c] = f(first, b, e, stride);
            }
        });
    for (auto& th : pool) th.join();
    return 0;
}

}  /* extern "C" */
