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
    int B, Sq, Sk, H, causal;      // packed: Sq / Sk are max_sq / max_sk, the shape of the dense run (bias offsets, dropout counters)
    float p_drop;
    uint64_t seed;
    const int32_t *q_start, *k_start;      // packed entry points only: the rows' first query / key row, B + 1 (kv_batch + 1) entries
    int Tq;                                // packed: q_start[B]; lse is [H][Tq]
};

// One batch row as its workgroup sees it: its own lengths, the first row of its queries and of its keys in q / k / v, and the index
// of its query 0 in lse (and the long backward's row terms).  Dense: the fixed pitch.  Packed: the offset arrays.  The bias offset
// j - i + a.Sq - 1 and the dropout counter ((b H + head) a.Sq + i) a.Sk + j keep the dense geometry in both forms.
struct T5Row {
    int Sq, Sk;
    int64_t q0, k0, l0;
};
template <bool PK>
__device__ __forceinline__ T5Row t5_row(const T5Args& a, int b, int bk, int hh) {
    if (PK) {
        const int q0 = a.q_start[b], k0 = a.k_start[bk];
        return T5Row{a.q_start[b + 1] - q0, a.k_start[bk + 1] - k0, q0, k0, (int64_t)hh * a.Tq + q0};
    }
    return T5Row{a.Sq, a.Sk, (int64_t)b * a.Sq, (int64_t)bk * a.Sk, ((int64_t)b * a.H + hh) * a.Sq};
}

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
    a.q_start = a.k_start = nullptr; a.Tq = 0;
    return 0;
}

// one offset array of a packed call, read from its host copy: starts at 0, never decreases, no row longer than max_len
static inline int t5_offsets(const char* name, const char* what, const int32_t* host, int n, int max_len) {
    GAMER_CHECK_ARG(host[0] == 0, "%s: %s[0] = %d (offsets start at 0)", name, what, host[0]);
    for (int b = 0; b < n; ++b) {
        GAMER_CHECK_ARG(host[b + 1] >= host[b], "%s: %s decreases at row %d (%d -> %d)", name, what, b, host[b], host[b + 1]);
        GAMER_CHECK_ARG(host[b + 1] - host[b] <= max_len, "%s: row %d of %s holds %d tokens, more than max %d", name, b, what,
                        host[b + 1] - host[b], max_len);
    }
    GAMER_CHECK_ARG(host[n] > 0, "%s: %s holds no token", name, what);
    return 0;
}
// the packed entry points: the dense check on the geometry (max_sq, max_sk), then the offsets.  q_start / k_start are device arrays of
// B + 1 / kv_rows_n + 1 entries and *_host their host copies, which is what this check reads (no device-to-host copy in a call).
static inline int t5_packed_args(const char* name, T5Args& a, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                                 const float* rel, const int32_t* q_start, const int32_t* k_start, const int32_t* q_start_host,
                                 const int32_t* k_start_host, int B, int kv_batch, int max_sq, int max_sk, int H, int dh, int causal,
                                 float p_drop, uint64_t seed, int max_s) {
    GAMER_TRY(t5_args(name, a, q, ldq, k, ldk, v, ldv, rel, nullptr, B, max_sq, max_sk, H, dh, causal, p_drop, seed, max_s));
    GAMER_CHECK_ARG(q_start && k_start && q_start_host && k_start_host && kv_batch > 0, "%s: null offsets", name);
    GAMER_TRY(t5_offsets(name, "q_start", q_start_host, B, max_sq));
    GAMER_TRY(t5_offsets(name, "k_start", k_start_host, kv_batch, max_sk));
    GAMER_CHECK_ARG((int64_t)H * q_start_host[B] < (1LL << 31), "%s: H Tq >= 2^31", name);
    a.q_start = q_start; a.k_start = k_start; a.Tq = q_start_host[B];
    return 0;
}

}  // namespace gamer
