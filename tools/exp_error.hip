// exp_error.hip -- the error in ulp of the candidates for the edge softmax's exponential, over EVERY fp32 argument in [-104, 0], against
// float64 exp on the same argument (tools/probe_attention.py builds and calls this; the softmax kernels use expf).
// The arguments are walked by their bit patterns: -0.0f = 0x80000000 up to -104.0f = 0xC2D00000, 1 120 927 745 values.  Results below
// 2^-126 are measured in units of 2^-149 (the spacing of subnormals), so a flushed subnormal counts as what it loses.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

namespace {
constexpr uint32_t kFirst = 0x80000000u, kLast = 0xC2D00000u;

template <int F>
__device__ float candidate(float x) {
    if (F == 0) return expf(x);
    if (F == 1) return __expf(x);
    return exp2f(x * 1.44269504088896340736f);
}

__device__ double ulp_error(float got, double want) {
    int e;
    frexp(want, &e);  // want = f x 2^e, f in [0.5, 1): the ulp of an fp32 value there is 2^(e - 24)
    const double ulp = e - 24 < -149 ? 0x1p-149 : ldexp(1.0, e - 24);
    return fabs(static_cast<double>(got) - want) / ulp;
}

template <int F>
__global__ __launch_bounds__(256) void exp_error(double *worst_per_block) {
    __shared__ double red[256];
    double worst = 0.0;
    const uint64_t n = static_cast<uint64_t>(kLast - kFirst) + 1, stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += stride) {
        const float x = __uint_as_float(kFirst + static_cast<uint32_t>(i));
        worst = fmax(worst, ulp_error(candidate<F>(x), exp(static_cast<double>(x))));
    }
    red[threadIdx.x] = worst;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (static_cast<int>(threadIdx.x) < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) worst_per_block[blockIdx.x] = red[0];
}
}  // namespace

// worst[f] = the largest error in ulp of candidate f (0 expf, 1 __expf, 2 exp2f of the prescaled argument); 0 on success
extern "C" int exp_error_ulp(double worst[3]) {
    constexpr int kBlocks = 4096;
    double *d = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&d), 3 * kBlocks * sizeof(double)) != hipSuccess) return 1;
    hipLaunchKernelGGL(exp_error<0>, dim3(kBlocks), dim3(256), 0, nullptr, d);
    hipLaunchKernelGGL(exp_error<1>, dim3(kBlocks), dim3(256), 0, nullptr, d + kBlocks);
    hipLaunchKernelGGL(exp_error<2>, dim3(kBlocks), dim3(256), 0, nullptr, d + 2 * kBlocks);
    static double h[3 * kBlocks];
    const bool ok = hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipFree(d);
    if (!ok) return 2;
    for (int f = 0; f < 3; ++f) {
        worst[f] = 0.0;
        for (int b = 0; b < kBlocks; ++b) worst[f] = fmax(worst[f], h[f * kBlocks + b]);
    }
    return 0;
}
