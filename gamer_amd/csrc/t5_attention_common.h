// Device helpers and the host argument check shared by the T5 attention families: the resident kernels of t5_attention.hip (K / V of a
// head in LDS, Sq, Sk <= 128) and the key-streaming kernels of t5_attention_long.hip (Sq, Sk <= 512).  The semantics are written at the
// top of t5_attention.hip.
#pragma once
#include "common.h"
#include <cmath>

namespace gamer {

constexpr int T5_THREADS = 256, T5_WAVES = T5_THREADS / WAVE;
constexpr int T5_MAX_H = 16;
constexpr int T5_BIAS_MAX_S = 512;       // gamer_t5_bias_expand / _fold: offsets R < 2 T5_BIAS_MAX_S (the longest family's bound)

struct T5Args {
    const float *q, *k, *v;        // q [B*Sq, ldq], k / v [B*Sk, ld*]: head h at column h*D
    int ldq, ldk, ldv;
    const float* rel;              // [H][Sq + Sk - 1] or nullptr
    const uint8_t* keep;           // [B][Sk] or nullptr
    const int32_t* kv_rows;        // forward only: row b reads k / v / keep of row kv_rows[b] (beams of one user), nullptr: b
    int B, Sq, Sk, H, causal;
    float p_drop;
    uint64_t seed;
};

// rows [0, rows) of a head's [rows, D] block -> LDS [rows16][D + 4], zero rows behind
template <int D>
__device__ __forceinline__ void t5_stage(float* __restrict__ dst, const float* __restrict__ g, int ld, int rows, int rows16) {
    constexpr int LD = D + 4, V4 = D / 4;
    for (int e = threadIdx.x; e < rows16 * V4; e += T5_THREADS) {
        const int r = e / V4, c = (e % V4) * 4;
        const float4 x = r < rows ? *reinterpret_cast<const float4*>(g + (int64_t)r * ld + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(dst + r * LD + c) = x;
    }
}
// a row's D values as the B operand of the transposed tile product: element s = x[4 s + (lane >> 4)]  (zeros for row = nullptr)
template <int D>
__device__ __forceinline__ void t5_row_operand(float (&r)[D / 4], const float* __restrict__ row, int lane) {
#pragma unroll
    for (int s = 0; s < D / 4; ++s) r[s] = row ? row[4 * s + (lane >> 4)] : 0.f;
}
// T[key 4 (lane >> 4) + reg][query lane & 15] = sum_n X[key][n] r_query[n] for the 16 LDS rows at `tile` (two accumulators: the
// 16x16x4 MFMA's dependent latency is longer than its issue interval)
template <int D>
__device__ __forceinline__ f32x4v t5_tile(const float* __restrict__ tile, const float (&r)[D / 4], int lane) {
    constexpr int LD = D + 4;
    const float* a = tile + (lane & 15) * LD + (lane >> 4);
    f32x4v acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < D / 4; s += 2) {
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * s], r[s], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * s + 4], r[s + 1], acc1, 0, 0, 0);
    }
    return acc0 + acc1;
}
// acc[n] += A X_tile: A[query lane & 15][key 4 (lane >> 4) + reg] = a[reg], X the 16 LDS rows at `tile`, column block n
template <int D>
__device__ __forceinline__ void t5_tile_out(f32x4v (&acc)[D / 16], const f32x4v a, const float* __restrict__ tile, int lane) {
    constexpr int LD = D + 4;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const float* x = tile + (4 * (lane >> 4) + reg) * LD + (lane & 15);
#pragma unroll
        for (int n = 0; n < D / 16; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[reg], x[16 * n], acc[n], 0, 0, 0);
    }
}
// rows i0 .. i0 + 15 of a [., D] head block from the accumulator layout (row 4 (lane >> 4) + reg, column 16 n + (lane & 15))
template <int D>
__device__ __forceinline__ void t5_store_rows(float* __restrict__ g, int ld, int i0, int rows, const f32x4v (&acc)[D / 16], int lane) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int i = i0 + 4 * (lane >> 4) + reg;
        if (i < rows) {
#pragma unroll
            for (int n = 0; n < D / 16; ++n) g[(int64_t)i * ld + 16 * n + (lane & 15)] = acc[n][reg];
        }
    }
}
__device__ __forceinline__ float t5_xor_max(float v) { return fmaxf(fmaxf(v, __shfl_xor(v, 16, 64)), fmaxf(__shfl_xor(v, 32, 64), __shfl_xor(v, 48, 64))); }
// (fixed order: the same bits in every lane of the four that share a query)
__device__ __forceinline__ float t5_xor_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

// ---- host: the argument check of both families' entry points (max_s: the family's bound on Sq and Sk)
static inline int t5_args(const char* name, T5Args& a, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* rel,
                   const uint8_t* keep, int B, int Sq, int Sk, int H, int dh, int causal, float p_drop, uint64_t seed, int max_s) {
    GAMER_CHECK_ARG(q && k && v, "%s: null pointer", name);
    GAMER_CHECK_ARG(B > 0 && Sq > 0 && Sq <= max_s && Sk > 0 && Sk <= max_s && H > 0 && H <= T5_MAX_H && (dh == 32 || dh == 64) &&
                        (int64_t)B * H < (1LL << 31),
                    "%s: bad shape B=%d Sq=%d Sk=%d H=%d head_dim=%d (Sq, Sk <= %d, H <= %d, head_dim 32 or 64)", name, B, Sq, Sk, H, dh,
                    max_s, T5_MAX_H);
    GAMER_CHECK_ARG(ldq >= H * dh && ldk >= H * dh && ldv >= H * dh && ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && aligned16(q) &&
                        aligned16(k) && aligned16(v),
                    "%s: bad leading dims (>= H head_dim, multiples of 4, 16-byte aligned bases)", name);
    GAMER_CHECK_ARG(p_drop >= 0.f && p_drop < 1.f, "%s: p_drop=%f", name, p_drop);
    a.q = q; a.k = k; a.v = v; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.rel = rel; a.keep = keep; a.kv_rows = nullptr;
    a.B = B; a.Sq = Sq; a.Sk = Sk; a.H = H; a.causal = causal != 0; a.p_drop = p_drop; a.seed = seed;
    return 0;
}

}  // namespace gamer
