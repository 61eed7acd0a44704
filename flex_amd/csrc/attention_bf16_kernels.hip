// attention_bf16_kernels.hip -- the multi-head fused attention on bf16 row operands (include/flex_spmm.h: flex_attention_bf16,
// flex_attention_bf16_backward): Q, K, V, Out, g, gQ, gK and gV are flex_bf16, the edge arrays dP and dWork stay fp32, and everything
// between a row's load and a row's store is the fp32 code of flex_attention_heads and flex_attention_heads_backward.
// tests/test_gpu_attention_bf16.py covers it; its (k, H) table is tests/attention_forms.py's, and tests/test_attention_routes.py holds
// every instantiation to a case that launches it.
//
// The sweeps are attention_heads_device.h's with the element type flex_bf16: the same walk, head split, slot placement, merges and LDS
// meeting places (fp32) as attention_heads_kernels.hip, one forward launch and two backward launches on the same plans.  A row load is
// one 8-byte load of four bf16 widened by shifts (exact), a row store narrows four fp32 to bf16 (round to nearest even, the one rounding
// of an output element) and is one 8-byte store (attention_device.h: load_cols, store_cols).  With the same source expressions under
// -ffp-contract=on, the fp32 value that is rounded at the store -- and every element of dP and dWork -- has the bits that
// flex_attention_heads and flex_attention_heads_backward give on the widened operands.  heads = 1 runs here as well (there is no
// generic form to forward to), so d = k is then a power of two.  Only the 8-byte form is built (the host refuses the rest).
#include <cmath>
#include <cstdint>
#include <initializer_list>

#include "attention_heads_device.h"

namespace flex {
namespace attention {

template <int W, int NS>
__global__ __launch_bounds__(256) void attention_bf16_rows(View v, HeadSplit hs, const flex_bf16 *__restrict__ Q, const flex_bf16 *__restrict__ K,
                                                            const flex_bf16 *__restrict__ V, float scale, flex_bf16 *__restrict__ Out,
                                                            float *__restrict__ P) {
    __shared__ HeadsShared<W, NS> sh;
    walk_rows_heads<W, NS>(v, hs, Q, K, V, scale, Out, P, sh);
}

template <int W, int NS>
__global__ __launch_bounds__(256) void attention_bf16_rows_backward(View v, HeadSplit hs, const flex_bf16 *__restrict__ K, const flex_bf16 *__restrict__ V,
                                                                     const float *__restrict__ P, const flex_bf16 *__restrict__ G, float scale,
                                                                     flex_bf16 *__restrict__ GQ, float *__restrict__ Work) {
    __shared__ HeadsRowShared<W, NS> sh;
    walk_rows_heads_backward<W, NS>(v, hs, K, V, P, G, scale, GQ, Work, sh);
}

template <int W, int NS>
__global__ __launch_bounds__(256) void attention_bf16_columns_backward(ColumnView v, HeadSplit hs, const flex_bf16 *__restrict__ Q,
                                                                        const flex_bf16 *__restrict__ G, const float *__restrict__ P,
                                                                        const float *__restrict__ DS, flex_bf16 *__restrict__ GK,
                                                                        flex_bf16 *__restrict__ GV) {
    __shared__ HeadsColumnShared<W, NS> sh;
    walk_columns_heads_backward<W, NS>(v, hs, Q, G, P, DS, GK, GV, sh);
}

// ---- launches

// W and NS of the plan's k, and whether the 8-byte form serves: k and both strides multiples of four elements, every row operand 8-byte
// aligned (a NULL output is aligned)
inline AttentionPick pick_bf16(const flex_plan *p, std::initializer_list<const void *> rows) {
    AttentionPick pick = attention_pick(p->k, p->ldb, p->ldc, nullptr, nullptr, nullptr, nullptr);
    for (const void *r : rows) pick.vec4 = pick.vec4 && reinterpret_cast<uintptr_t>(r) % 8 == 0;
    return pick;
}

struct Bf16Operands {
    const flex_bf16 *Q, *K, *V;
    const float *P;
    const flex_bf16 *G;
    float scale;
    flex_bf16 *GQ, *GK, *GV;
    float *Work;
};

void launch_columns_backward(const flex_plan *p, const AttentionPick &pick, const HeadSplit &hs, const flex_bf16 *Q, const flex_bf16 *G, const float *P,
                             const float *DS, flex_bf16 *GK, flex_bf16 *GV, hipStream_t s) {
    const ColumnView cv = column_view(p);
    const dim3 cgrid = launch_grid(cv), block(64 * kWavesPerBlock);
    dispatch(pick, [&](auto W, auto NS) {
        hipLaunchKernelGGL((attention_bf16_columns_backward<W(), NS()>), cgrid, block, 0, s, cv, hs, Q, G, P, DS, GK, GV);
    });
}

}  // namespace attention
}  // namespace flex

using namespace flex;

extern "C" {

int flex_attention_bf16(const flex_plan *p, int heads, const flex_bf16 *dQ, const flex_bf16 *dK, const flex_bf16 *dV, float scale, flex_bf16 *dOut,
                        float *dP, flex_stream_t stream) {
    if (!p || !p->at_ok || heads < 1) return FLEX_ERR_INVALID;
    if (!std::isfinite(scale) || !(scale > 0.f)) return FLEX_ERR_INVALID;
    attention::HeadSplit hs;
    if (const int rc = attention::split_of(p->k, heads, &hs)) return rc;
    if (p->at_entries == 0) return FLEX_OK;
    if (!dQ || !dK || !dV || !dOut) return FLEX_ERR_INVALID;
    const AttentionPick pick = attention::pick_bf16(p, {dQ, dK, dV, dOut});
    if (!pick.vec4) return FLEX_ERR_UNSUPPORTED;
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    const attention::View v = attention::row_view(p);
    const dim3 grid = attention::launch_grid(v), block(64 * kWavesPerBlock);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    attention::dispatch(pick, [&](auto W, auto NS) {
        hipLaunchKernelGGL((attention::attention_bf16_rows<W(), NS()>), grid, block, 0, s, v, hs, dQ, dK, dV, scale, dOut, dP);
    });
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

int flex_attention_bf16_backward(const flex_plan *p, int heads, const flex_bf16 *dQ, const flex_bf16 *dK, const flex_bf16 *dV, const float *dP,
                                 const flex_bf16 *dGradOut, float scale, flex_bf16 *dGradQ, flex_bf16 *dGradK, flex_bf16 *dGradV, float *dWork,
                                 flex_stream_t stream) {
    if (!p || !p->ab_ok || heads < 1) return FLEX_ERR_INVALID;
    if (!std::isfinite(scale) || !(scale > 0.f)) return FLEX_ERR_INVALID;
    attention::HeadSplit hs;
    if (const int rc = attention::split_of(p->k, heads, &hs)) return rc;
    if (p->at_entries == 0) return FLEX_OK;
    if (!dQ || !dK || !dV || !dP || !dGradOut || !dWork || dWork == dP) return FLEX_ERR_INVALID;
    const AttentionPick pick = attention::pick_bf16(p, {dQ, dK, dV, dGradOut, dGradQ, dGradK, dGradV});
    if (!pick.vec4) return FLEX_ERR_UNSUPPORTED;
    if (!dGradQ && !dGradK && !dGradV) return FLEX_OK;
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    const attention::View rv = attention::row_view(p);
    const attention::ColumnView cv = attention::column_view(p);
    const dim3 rgrid = attention::launch_grid(rv), cgrid = attention::launch_grid(cv), block(64 * kWavesPerBlock);
    const attention::Bf16Operands o{dQ, dK, dV, dP, dGradOut, scale, dGradQ, dGradK, dGradV, dWork};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    attention::dispatch(pick, [&](auto W, auto NS) {
        using namespace attention;
        if (o.GQ || o.GK) hipLaunchKernelGGL((attention_bf16_rows_backward<W(), NS()>), rgrid, block, 0, s, rv, hs, o.K, o.V, o.P, o.G, o.scale, o.GQ, o.Work);
        if (o.GK || o.GV) hipLaunchKernelGGL((attention_bf16_columns_backward<W(), NS()>), cgrid, block, 0, s, cv, hs, o.Q, o.G, o.P, o.Work, o.GK, o.GV);
    });
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

}  // extern "C"
