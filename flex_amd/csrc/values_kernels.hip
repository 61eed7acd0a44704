// values_kernels.hip -- learnable edge values on FLEX_PLAN_MUTABLE_VALUES plans (include/flex_spmm.h): the value refresh
// (flex_plan_set_values) and the SDDMM of the plan's pattern (flex_sddmm).  What they read besides the plan is built by the planner
// (plan_build.cpp, upload_value_image); flex_plan_self_check verifies it (plan_check.cpp).
//
// These are not SpMM kernels: they live in a namespace of their own, outside the route table of the SpMM kernels
// (tests/f64ref.py, ROUTES); tests/test_gpu_values.py covers them, and tests/test_gpu_values_address_limits.py declares a case for
// every instantiation (tests/test_kernel_routes.py checks the declarations against sddmm_pick / refresh_passes of internal.h).
#include <cstdint>

#include "plan.h"

namespace flex {
namespace values {

// ---- value refresh.  Two passes over the plan, in stream order:
//   1. every record: the real ones take dVals[entry] into their value half and into the plan's copy (20 bytes a record: the map, the
//      gathered value, the copy, the record's value half -- a 4-byte store into every 8-byte record, i.e. its whole line);
//   2. every padded run: pad_values again on the fresh values (runs are disjoint; a run is at most one task's records, so the pass
//      reads what pass 1 wrote, mostly from the L2).
__global__ __launch_bounds__(256) void refresh_records(uint2 *__restrict__ rec, float *__restrict__ vrec, const uint32_t *__restrict__ src,
                                                        const float *__restrict__ vals, uint64_t n) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t e = src[i];
    if (e == kNoEntry) return;
    const float v = vals[e];
    vrec[i] = v;
    rec[i].y = __float_as_uint(v);
}

__global__ __launch_bounds__(256) void refresh_padding(uint2 *__restrict__ rec, const uint4 *__restrict__ seg, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint4 s = seg[i];
    pad_values(rec + s.x, s.y, s.z, s.w);
}

// ---- SDDMM.  A wave walks one group of items (plan_build.cpp: runs of <= 64 real records of one C row, in task order, so the waves
// gather the B rows in the order the plan's SpMM does).  The wave is S = 64 / W slots of W lanes; lane l of a slot holds columns
// 4l + 4Wq .. +3 (q < ns = ceil(k / 4W) <= 4) of the item's G row in registers.  Per pass, slot s takes records s, s + S, s + 2S,
// s + 3S of the item: 4 B-row gathers per slab in flight, each lane folds its four columns of a record into one fma chain, and the
// slot sums its W lanes per record in a fixed order.  Four records at a time make that a TRANSPOSED reduction: two exchange steps
// (offsets W/2, W/4) each trade half of the lanes' values, leaving lane l with the half-sums of ONE record (2 b(W/2) + b(W/4)), then a
// butterfly over the offsets below W/4 -- 3 + log2(W/4) shuffles per 4 records instead of 4 log2(W).  A lane with no columns (k not a
// multiple of 4W) adds +0: it multiplies nothing, so no 0 x inf ever reaches a sum.  Rounding depth of a term: 4 ns fma + log2 W adds
// <= k for every k (the header's gamma(k)).
struct SddmmView {
    const uint2 *rec;
    const uint32_t *src;
    const uint4 *item;
    const uint32_t *grp;
    uint32_t n_groups;
    uint32_t xcd_remap;  // the plan's choice: each XCD walks one contiguous slice of the groups (as its SpMM does)
    int32_t k, ldb, ldc, ns;
};

template <bool VEC>
__device__ __forceinline__ float4 load_cols(const float *row, int c, int k) {
    if constexpr (VEC) {
        if (c < k) return *reinterpret_cast<const float4 *>(row + c);
        return make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < k) r.x = row[c];
        if (c + 1 < k) r.y = row[c + 1];
        if (c + 2 < k) r.z = row[c + 2];
        if (c + 3 < k) r.w = row[c + 3];
        return r;
    }
}

// sum over the lane's columns of g * b; columns at or past k add nothing (not even 0 x b)
template <bool VEC>
__device__ __forceinline__ float dot_cols(float acc, const float4 &g, const float4 &b, int c, int k) {
    if (VEC) {
        if (c < k) {
            acc = __builtin_fmaf(g.x, b.x, acc);
            acc = __builtin_fmaf(g.y, b.y, acc);
            acc = __builtin_fmaf(g.z, b.z, acc);
            acc = __builtin_fmaf(g.w, b.w, acc);
        }
    } else {
        if (c < k) acc = __builtin_fmaf(g.x, b.x, acc);
        if (c + 1 < k) acc = __builtin_fmaf(g.y, b.y, acc);
        if (c + 2 < k) acc = __builtin_fmaf(g.z, b.z, acc);
        if (c + 3 < k) acc = __builtin_fmaf(g.w, b.w, acc);
    }
    return acc;
}

constexpr int kMaxSlabs = 4;

template <int W, bool OFF32, bool VEC>
__global__ __launch_bounds__(256) void sddmm_slots(SddmmView v, const float *__restrict__ G, const float *__restrict__ B, float *__restrict__ out) {
    constexpr uint32_t S = 64 / W;
    static_assert(W >= 4 && W <= 64, "four records per pass need two exchange steps inside the slot");
    uint32_t wg = blockIdx.x;
    if (v.xcd_remap) {  // the hardware deals workgroup i to XCD i % 8; give XCD x the x-th eighth of the groups instead
        const uint32_t per = gridDim.x / kXcds;
        wg = (blockIdx.x % kXcds) * per + blockIdx.x / kXcds;
    }
    const uint32_t g = wg * kWavesPerBlock + (threadIdx.x >> 6);
    if (g >= v.n_groups) return;
    const uint32_t lane = threadIdx.x & 63u, slot = lane / W, li = lane % W;
    const bool hi2 = (li & (W / 2)) != 0, hi4 = (li & (W / 4)) != 0;
    const bool writer = (li & (W / 4 - 1)) == 0;
    const uint32_t it1 = v.grp[g + 1];
    for (uint32_t it = v.grp[g]; it < it1; ++it) {
        const uint4 item = v.item[it];  // {first record, records, stride, C row}: the same for every lane
        const float *grow = G + static_cast<size_t>(item.w) * v.ldc;
        float4 gv[kMaxSlabs];
#pragma unroll
        for (int q = 0; q < kMaxSlabs; ++q)
            gv[q] = q < v.ns ? load_cols<VEC>(grow, 4 * static_cast<int>(li) + 4 * W * q, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
        for (uint32_t j0 = 0; j0 < item.y; j0 += 4 * S) {
            uint32_t ent[4];
            const float *brow[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t j = j0 + u * S + slot;
                const bool valid = j < item.y;
                const uint32_t r = item.x + (valid ? j : 0u) * item.z;  // past the item: its first record again, result dropped
                const uint2 rr = v.rec[r];
                ent[u] = valid ? v.src[r] : kNoEntry;
                brow[u] = OFF32 ? reinterpret_cast<const float *>(reinterpret_cast<const char *>(B) + rr.x) : B + static_cast<size_t>(rr.x) * v.ldb;
            }
            float pr[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float acc = 0.f;
#pragma unroll
                for (int q = 0; q < kMaxSlabs; ++q) {
                    if (q < v.ns) {
                        const int c = 4 * static_cast<int>(li) + 4 * W * q;
                        acc = dot_cols<VEC>(acc, gv[q], load_cols<VEC>(brow[u], c, v.k), c, v.k);
                    }
                }
                pr[u] = acc;
            }
            // transposed reduction: after the offset-W/2 step the lane holds records {2 hi2, 2 hi2 + 1}, after W/4 record 2 hi2 + hi4
            const float a0 = (hi2 ? pr[2] : pr[0]) + __shfl_xor(hi2 ? pr[0] : pr[2], W / 2);
            const float a1 = (hi2 ? pr[3] : pr[1]) + __shfl_xor(hi2 ? pr[1] : pr[3], W / 2);
            float t = (hi4 ? a1 : a0) + __shfl_xor(hi4 ? a0 : a1, W / 4);
#pragma unroll
            for (int o = W / 8; o >= 1; o >>= 1) t += __shfl_xor(t, o);
            const uint32_t e = hi2 ? (hi4 ? ent[3] : ent[2]) : (hi4 ? ent[1] : ent[0]);
            if (writer && e != kNoEntry) out[e] = t;
        }
    }
}

template <int W>
int launch_sddmm_w(const SddmmView &v, bool off32, bool vec4, const float *G, const float *B, float *out, hipStream_t s) {
    uint32_t blocks = (v.n_groups + kWavesPerBlock - 1) / kWavesPerBlock;
    if (v.xcd_remap) blocks = (blocks + kXcds - 1) / kXcds * kXcds;
    if (off32 && vec4) hipLaunchKernelGGL((sddmm_slots<W, true, true>), dim3(blocks), dim3(256), 0, s, v, G, B, out);
    else if (off32) hipLaunchKernelGGL((sddmm_slots<W, true, false>), dim3(blocks), dim3(256), 0, s, v, G, B, out);
    else if (vec4) hipLaunchKernelGGL((sddmm_slots<W, false, true>), dim3(blocks), dim3(256), 0, s, v, G, B, out);
    else hipLaunchKernelGGL((sddmm_slots<W, false, false>), dim3(blocks), dim3(256), 0, s, v, G, B, out);
    return FLEX_OK;
}

}  // namespace values
}  // namespace flex

using namespace flex;

extern "C" {

int flex_plan_set_values(flex_plan *p, const float *dVals, flex_stream_t stream) {
    if (!p || !p->mutable_vals) return FLEX_ERR_INVALID;
    const uint64_t n = p->d_rec.size();
    const int passes = refresh_passes(n, p->d_seg.size());
    if (passes == 0) return FLEX_OK;
    if (!dVals && p->nnz > 0) return FLEX_ERR_INVALID;
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(values::refresh_records, dim3(static_cast<uint32_t>((n + 255) / 256)), dim3(256), 0, s, p->d_rec.get(), p->d_vrec.get(), p->d_src.get(), dVals, n);
    FLEX_HIP_TRY(hipGetLastError());
    if (passes == 2) {
        const uint32_t n_segs = static_cast<uint32_t>(p->d_seg.size());
        hipLaunchKernelGGL(values::refresh_padding, dim3((n_segs + 255) / 256), dim3(256), 0, s, p->d_rec.get(), p->d_seg.get(), n_segs);
        FLEX_HIP_TRY(hipGetLastError());
    }
    return FLEX_OK;
}

int flex_sddmm(const flex_plan *p, const float *dG, const float *dB, float *dOut, flex_stream_t stream) {
    if (!p || !p->mutable_vals) return FLEX_ERR_INVALID;
    if (p->n_sd_groups == 0) return FLEX_OK;
    if (!dG || !dB || !dOut) return FLEX_ERR_INVALID;
    const SddmmPick pick = sddmm_pick(p->k, p->ldb, p->ldc, p->off32, dG, dB);
    const int W = pick.W;
    const int ns = (p->k + 4 * W - 1) / (4 * W);
    if (ns > values::kMaxSlabs) return FLEX_ERR_UNSUPPORTED;
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    const values::SddmmView v{p->d_rec.get(), p->d_src.get(), p->d_sd_item.get(), p->d_sd_grp.get(), p->n_sd_groups, p->xcd_remap ? 1u : 0u, p->k, p->ldb, p->ldc, ns};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (W) {
        case 4: values::launch_sddmm_w<4>(v, pick.off32, pick.vec4, dG, dB, dOut, s); break;
        case 8: values::launch_sddmm_w<8>(v, pick.off32, pick.vec4, dG, dB, dOut, s); break;
        case 16: values::launch_sddmm_w<16>(v, pick.off32, pick.vec4, dG, dB, dOut, s); break;
        case 32: values::launch_sddmm_w<32>(v, pick.off32, pick.vec4, dG, dB, dOut, s); break;
        default: values::launch_sddmm_w<64>(v, pick.off32, pick.vec4, dG, dB, dOut, s); break;
    }
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

}  // extern "C"
