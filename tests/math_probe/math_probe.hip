/* math_probe.hip — the op table of math_ops.h compiled for the device with the product's own compile line (TEST INFRASTRUCTURE; built
 * by realtimeraytracer_amd/csrc/Makefile into tests/math_probe/libmath_probe.so, links nothing of the product).
 *   math_probe_eval : n input tuples -> n results, one lane per tuple
 *   math_probe_sweep: for one-word ops, the patterns first + i * stride, folded into one digest per 2^20 consecutive i
 * Each call is one launch on stream 0, joined before it returns. */
#include "../../realtimeraytracer_amd/csrc/kernels/rtr_device.h"
using namespace rtrdev;
#define PROBE_DEVICE_FORMS 1
#include "math_ops.h"

typedef void (*probe_fn)(const uint32_t*, uint32_t*);

template <probe_fn F, int NIN, int NOUT>
__global__ void __launch_bounds__(256) eval_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint32_t a[NIN], r[NOUT];
    for (int k = 0; k < NIN; ++k) a[k] = in[(size_t)i * NIN + k];
    F(a, r);
    for (int k = 0; k < NOUT; ++k) out[(size_t)i * NOUT + k] = r[k];
}

/* one block folds 4096 consecutive i (all of one chunk: 4096 divides 2^20); a wave adds its lanes' mixes, then issues one atomic */
#define SWEEP_SPAN 4096u
template <probe_fn F, int NOUT, uint32_t FMASK>
__global__ void __launch_bounds__(256) sweep_kernel(uint32_t first, unsigned long long count, uint32_t stride, unsigned long long* __restrict__ digests) {
    const unsigned long long base = (unsigned long long)blockIdx.x * SWEEP_SPAN;
    unsigned long long acc = 0;
    for (uint32_t it = 0; it < SWEEP_SPAN / 256u; ++it) {
        const unsigned long long i = base + it * 256u + threadIdx.x;
        if (i < count) {
            const uint32_t p = first + (uint32_t)i * stride;
            uint32_t r[NOUT];
            F(&p, r);
            acc += probe_mix(p, r, NOUT, FMASK);
        }
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63u) == 0) atomicAdd(&digests[base >> PROBE_CHUNK_LOG2], acc);     /* base < count: inside the digest array */
}

template <probe_fn F, int NIN, int NOUT, uint32_t FMASK>
static void launch_sweep(uint32_t blocks, uint32_t first, unsigned long long count, uint32_t stride, unsigned long long* d) {
    if constexpr (NIN == 1) sweep_kernel<F, NOUT, FMASK><<<blocks, 256, 0, 0>>>(first, count, stride, d);
}

#define CHECK(e) do { hipError_t err_ = (e); if (err_ != hipSuccess) { rc = (int)err_; goto done; } } while (0)

extern "C" {

int math_probe_op_count(void) { return PROBE_OP_COUNT; }
const char* math_probe_op_name(int op) { return op >= 0 && op < PROBE_OP_COUNT ? PROBE_INFO[op].name : nullptr; }
int math_probe_op_nin(int op) { return op >= 0 && op < PROBE_OP_COUNT ? PROBE_INFO[op].nin : -1; }
int math_probe_op_nout(int op) { return op >= 0 && op < PROBE_OP_COUNT ? PROBE_INFO[op].nout : -1; }
uint32_t math_probe_op_fmask(int op) { return op >= 0 && op < PROBE_OP_COUNT ? PROBE_INFO[op].fmask : 0; }

/* in: n * nin words, out: n * nout words, both host arrays.  0 on success, -1 on a bad argument, else the hipError_t. */
int math_probe_eval(int device, int op, const uint32_t* in, uint32_t n, uint32_t* out) {
    if (op < 0 || op >= PROBE_OP_COUNT || !in || !out) return -1;
    if (n == 0) return 0;
    const size_t inBytes = (size_t)n * PROBE_INFO[op].nin * 4, outBytes = (size_t)n * PROBE_INFO[op].nout * 4;
    uint32_t *din = nullptr, *dout = nullptr;
    int rc = 0;
    const uint32_t blocks = (n + 255u) / 256u;
    CHECK(hipSetDevice(device));
    CHECK(hipMalloc(&din, inBytes));
    CHECK(hipMalloc(&dout, outBytes));
    CHECK(hipMemcpy(din, in, inBytes, hipMemcpyHostToDevice));
    switch (op) {
#define X(name, nin, nout, fmask) case PROBE_OP_##name: eval_kernel<op_##name, nin, nout><<<blocks, 256, 0, 0>>>(din, dout, n); break;
        PROBE_OPS(X)
#undef X
    }
    CHECK(hipGetLastError());
    CHECK(hipStreamSynchronize(0));
    CHECK(hipMemcpy(out, dout, outBytes, hipMemcpyDeviceToHost));
done:
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    return rc;
}

/* digests: ceil(count / 2^20) words of 64 bits, a host array.  count <= 2^32.  -2: the op does not take one input word. */
int math_probe_sweep(int device, int op, uint32_t first, uint64_t count, uint32_t stride, uint64_t* digests) {
    if (op < 0 || op >= PROBE_OP_COUNT || !digests || count > (1ull << 32)) return -1;
    if (PROBE_INFO[op].nin != 1) return -2;
    if (count == 0) return 0;
    const size_t nd = (size_t)((count + (1ull << PROBE_CHUNK_LOG2) - 1) >> PROBE_CHUNK_LOG2);
    const uint32_t blocks = (uint32_t)((count + SWEEP_SPAN - 1) / SWEEP_SPAN);
    unsigned long long* d = nullptr;
    int rc = 0;
    CHECK(hipSetDevice(device));
    CHECK(hipMalloc(&d, nd * 8));
    CHECK(hipMemset(d, 0, nd * 8));
    switch (op) {
#define X(name, nin, nout, fmask) case PROBE_OP_##name: launch_sweep<op_##name, nin, nout, fmask>(blocks, first, count, stride, d); break;
        PROBE_OPS(X)
#undef X
    }
    CHECK(hipGetLastError());
    CHECK(hipStreamSynchronize(0));
    CHECK(hipMemcpy(digests, d, nd * 8, hipMemcpyDeviceToHost));
done:
    if (d) (void)hipFree(d);
    return rc;
}

}  /* extern "C" */
