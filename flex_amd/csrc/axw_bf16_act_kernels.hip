// axw_bf16_act_kernels.hip -- ReLU and dropout fused into the bf16 root layer (libflex_axw.so; flex_axw_run_root_act_bf16,
// flex_axw_backward_root_act_bf16):
//   forward   Out[n x cp] = keep ? rn_bf16(cs relu(z)) : +0,  z = L1 W1 + L2 W2 + Cin + bias as axw_bf16_root_kernels.hip sums it
//   backward  dZ[n x cp]  = Out > 0 ? rn_bf16(fp32(dOut) cs) : +0
// The forward is the kRootAct form of axw_gemm_bf16_stream_kernel (axw_bf16_device.h): the root form -- same pack, same grid, same LDS,
// same chain -- with the activation applied to a tile's 16 accumulators just before that tile's store.  Where the dense kernel is the
// layer's last stage (it is, in both association orders) z exists nowhere cheaper: fp32, in registers, a lane holding runs of four
// columns of one row.  keep(seed, row c + column) is the library's dropout hash (internal.h: dropout_bits, DropMask -- what
// flex_dropout_mask evaluates on the host), recomputed, never stored; c is the true width, so the mask does not depend on the padding.
// drop_p == 0 runs instantiations without the hash, whose Out is max(Out of the root kernel, +0) bit for bit: rounding is monotone and
// keeps the sign.
// The backward needs neither mask nor seed: a unit was active and kept exactly where the stored Out > 0 (a float compare: NaN, +0 and -0
// give +0).  axw_bf16_act_grad_kernel is one streaming pass -- two 16-byte loads, eight elements and one 16-byte store a thread, a grid
// sized to the array -- that writes dZ, padding columns +0, for the root backward's kernels to read in place of dOut.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "axw_bf16_device.h"

namespace flex_axw_bf16 {

__global__ __launch_bounds__(256) void axw_bf16_act_grad_kernel(const u32x4 *__restrict__ Out, const u32x4 *__restrict__ dOut,
                                                                u32x4 *__restrict__ dZ, uint64_t chunks, int c, int cp, float cs) {
    const uint64_t f = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;  // eight elements of one row: cp % 8 == 0
    if (f >= chunks) return;
    const int col = static_cast<int>(f % static_cast<uint32_t>(cp >> 3)) * 8;
    const u32x4 o = Out[f], g = dOut[f];
    u32x4 z;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        auto one = [&](uint32_t ob, uint32_t gb, int k) {  // both in the upper 16 bits: the fp32 numbers they are
            return __uint_as_float(ob) > 0.f && k < c ? bf16_bits(__uint_as_float(gb) * cs) : 0u;
        };
        z[i] = one(o[i] << 16, g[i] << 16, col + 2 * i) | (one(o[i] & 0xFFFF0000u, g[i] & 0xFFFF0000u, col + 2 * i + 1) << 16);
    }
    dZ[f] = z;
}

}  // namespace flex_axw_bf16

// flex_axw_gemm_bf16_root_launch (axw_bf16_root_kernels.hip: its operands, its checks, its pack launch, its grid) with ReLU and dropout
// between the chain and the store: Out = keep(seed, row c + col) ? rn_bf16(relu(z) / (1 - drop_p)) : +0.  drop_p must be finite,
// 0 <= drop_p < 1 (hipErrorInvalidValue before a launch, like every other refusal); drop_p == 0 evaluates no hash.
extern "C" hipError_t flex_axw_gemm_bf16_root_act_launch(const flex_bf16 *L1, const flex_bf16 *W1, int d1, const flex_bf16 *L2, const flex_bf16 *W2,
                                                         int d2, const flex_bf16 *Cin, const float *bias, flex_bf16 *Wf, flex_bf16 *Out, int n, int c,
                                                         int cp, int n_cus, float drop_p, uint64_t seed, hipStream_t s) {
    using namespace flex_axw_bf16;
    auto width = [](int d, int least) { return d >= least && d <= 4096 && d % 16 == 0; };
    if (!L1 || !W1 || !Wf || !Out || n < kRows || !width(d1, 16) || !width(d2, 0) || (d2 > 0) != (L2 != nullptr) || (d2 > 0) != (W2 != nullptr) ||
        cp <= 0 || cp % 64 != 0 || cp > 256 || c <= 0 || c > cp || n_cus <= 0 || misaligned(L1) || misaligned(L2) || misaligned(Cin) ||
        misaligned(Wf) || misaligned(Out) || !flex::drop_p_ok(drop_p))
        return hipErrorInvalidValue;
    const uintptr_t bytes = static_cast<uintptr_t>(n) * cp * sizeof(flex_bf16), ci = reinterpret_cast<uintptr_t>(Cin),
                    oi = reinterpret_cast<uintptr_t>(Out);
    if (Cin && ci < oi + bytes && oi < ci + bytes) return hipErrorInvalidValue;
    u32x4 *wf = reinterpret_cast<u32x4 *>(Wf);
    const hipError_t e = pack_launch(W1, W2, wf, d1, d2, c, cp / 32, s);
    if (e != hipSuccess) return e;
    const flex::DropMask dm = flex::drop_mask(drop_p, seed);
    return dispatch_tiles<2, 4, 6, 8>(cp / 32, [&](auto tiles) {
        constexpr int NT = decltype(tiles)::value, P = stream_panels(NT);
        const dim3 grid(panel_groups(n, kWaves * P, n_cus));
        const size_t lds = stream_lds(NT) + cp * sizeof(float);
        const flex_bf16 *l2 = d2 ? L2 : L1;
        if (drop_p == 0.f)
            return launch(axw_gemm_bf16_stream_kernel<NT, P, Stream::kRootAct>, grid, 64 * kWaves, lds, s, L1, d1, l2, d2, wf, Cin, bias, Out, n, c);
        return launch(axw_gemm_bf16_stream_kernel<NT, P, Stream::kRootAct, flex::DropMask>, grid, 64 * kWaves, lds, s, L1, d1, l2, d2, wf, Cin, bias,
                      Out, n, c, dm);
    });
}

// dZ[n x cp] = Out > 0 ? rn_bf16(fp32(dOut) cs) : +0 on flex_bf16, columns c .. cp-1 of dZ written as +0 bits whatever Out and dOut hold
// there.  Takes n > 0, cp % 64 == 0, 0 < c <= cp <= 256, a finite cs and 16-byte aligned pointers, dZ distinct from Out and dOut; anything
// else returns hipErrorInvalidValue before a launch.
extern "C" hipError_t flex_axw_act_grad_bf16_launch(const flex_bf16 *Out, const flex_bf16 *dOut, flex_bf16 *dZ, int n, int c, int cp, float cs,
                                                    hipStream_t s) {
    using namespace flex_axw_bf16;
    if (!Out || !dOut || !dZ || dZ == Out || dZ == dOut || n <= 0 || cp <= 0 || cp % 64 != 0 || cp > 256 || c <= 0 || c > cp || !(cs - cs == 0.f) ||
        misaligned(Out) || misaligned(dOut) || misaligned(dZ))
        return hipErrorInvalidValue;
    const uint64_t chunks = static_cast<uint64_t>(n) * (cp / 8);
    return launch(axw_bf16_act_grad_kernel, dim3(static_cast<unsigned>((chunks + 255) / 256)), 256, 0, s, reinterpret_cast<const u32x4 *>(Out),
                  reinterpret_cast<const u32x4 *>(dOut), reinterpret_cast<u32x4 *>(dZ), chunks, c, cp, cs);
}
