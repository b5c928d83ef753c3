// q/k per-head RMSNorm + RoPE (+ behaviour bias), head_dim = 64, forward and backward: gamer_qknorm_rope_fwd / _bwd (+ _bf16).
// The arithmetic of a (token, head) row is stated ONCE, in fwd_row and bwd_row; the four kernel templates only walk and index.
#include "common.h"

// The floating-point form of this file is fixed by its source: no contraction by the compiler, every fused multiply-add is a
// __builtin_fmaf.  (Left to the compiler, the earlier per-kernel copies of these formulas were fused differently from copy to
// copy - even from element to element of one bf16 row - and their outputs differed in the last bit.)
#pragma clang fp contract(off)

namespace gamer {

// ---------------------------------------------------------------------------------------------
// lane layout of a row
// ---------------------------------------------------------------------------------------------
// A (token, head) row of 64 values lies across LANES adjacent lanes, E values (16 bytes of the activation type) per lane, ROWS rows
// per wave: the 64-wide reductions are xor-shuffles inside the group of lanes, the RoPE partner (d +- 32) is lane ^ (LANES / 2).
//            lanes per row   values per lane   partner    load / store
//   fp32          16               4            xor 8      ld4 / st4
//   bf16           8               8            xor 4      ld8 / st8
__device__ __forceinline__ void ld8(const bf16_t* p, float (&f)[8]) {
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = (float)v[e];
}
__device__ __forceinline__ void st8(bf16_t* p, const float (&f)[8]) {
    f32x8v v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = f[e];
    *reinterpret_cast<bf16x8*>(p) = __builtin_convertvector(v, bf16x8);
}
template <typename TA> struct RowLanes;
template <> struct RowLanes<float> {
    static constexpr int LANES = 16, E = 4;
    static __device__ __forceinline__ void ld(const float* p, float (&f)[4]) {
        const float4 v = ld4(p);
        f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
    }
    static __device__ __forceinline__ void st(float* p, const float (&f)[4]) { st4(p, make_float4(f[0], f[1], f[2], f[3])); }
};
template <> struct RowLanes<bf16_t> {
    static constexpr int LANES = 8, E = 8;
    static __device__ __forceinline__ void ld(const bf16_t* p, float (&f)[8]) { ld8(p, f); }
    static __device__ __forceinline__ void st(bf16_t* p, const float (&f)[8]) { st8(p, f); }
};
// E consecutive floats of a weight / cos / sin / bias row or of the partial sums (p aligned to 16 bytes)
template <int E> __device__ __forceinline__ void ld_f32(const float* p, float (&f)[E]) {
#pragma unroll
    for (int i = 0; i < E / 4; ++i) {
        const float4 v = reinterpret_cast<const float4*>(p)[i];
        f[4 * i] = v.x; f[4 * i + 1] = v.y; f[4 * i + 2] = v.z; f[4 * i + 3] = v.w;
    }
}
template <int E> __device__ __forceinline__ void st_f32(float* p, const float (&f)[E]) {
#pragma unroll
    for (int i = 0; i < E / 4; ++i) reinterpret_cast<float4*>(p)[i] = make_float4(f[4 * i], f[4 * i + 1], f[4 * i + 2], f[4 * i + 3]);
}
// sum over the lanes of a row (every lane of the group ends with it); sum over the groups of a wave
template <typename L> __device__ __forceinline__ float row_sum(float v) {
#pragma unroll
    for (int o = 1; o < L::LANES; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <typename L> __device__ __forceinline__ float rows_sum(float v) {
#pragma unroll
    for (int o = L::LANES; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <int E> __device__ __forceinline__ float amax_row(float m, const float (&v)[E]) {
#pragma unroll
    for (int e = 0; e < E; ++e) m = fmaxf(m, fabsf(v[e]));
    return m;
}

// ---------------------------------------------------------------------------------------------
// the arithmetic of one row
// ---------------------------------------------------------------------------------------------
// TA = activation type of qkv / q_rot / k_rot.  With bf16 activations the arithmetic mirrors what the reference does under autocast
// (ref:SeqRec/tasks/train_SMB_decoder.py:114-118): the projection output is bf16; for the self attention Qwen3MoeRMSNorm sees a bf16
// input and rounds the normalised value to bf16 before the fp32 weight multiply; for the cross attention the fp32 behaviour bias is
// added first, so the norm runs in fp32; RoPE is fp32; SDPA's inputs (q_rot, k_rot, v) are rounded to bf16.

// x: the pre-norm row, behaviour bias included.  o = rope(w * x / rms(x)); sgn = -1 in the lower half of the row, +1 in the upper.
template <typename TA>
__device__ __forceinline__ void fwd_row(const float (&x)[RowLanes<TA>::E], const float (&w)[RowLanes<TA>::E], const float (&cs)[RowLanes<TA>::E],
                                        const float (&sn)[RowLanes<TA>::E], float eps, float sgn, bool cross, float (&o)[RowLanes<TA>::E]) {
    using L = RowLanes<TA>;
    float ss = x[0] * x[0];
#pragma unroll
    for (int e = 1; e < L::E; ++e) ss += x[e] * x[e];
    const float rstd = rsqrtf(__builtin_fmaf(row_sum<L>(ss), 1.f / 64.f, eps));
#pragma unroll
    for (int e = 0; e < L::E; ++e) {
        float xn = x[e] * rstd;
        if (sizeof(TA) == 2 && !cross) xn = round_as<TA>(xn);      // Qwen3MoeRMSNorm on a bf16 tensor: .to(input_dtype) before * weight
        const float y = w[e] * xn;
        const float pr = __shfl_xor(y, L::LANES / 2, 64);
        o[e] = __builtin_fmaf(sn[e], sgn * pr, y * cs[e]);
    }
}

// x: the pre-norm row (bias included), d: the gradient of the rotated row; sgn = +1 in the lower half, -1 in the upper (the transpose
// of the rotation).  dx = the gradient of x; dw += lv * dy * x^ with one rounding (lv = 1, or 0 for a row that only fills the wave),
// x^ as the weight saw it in the forward: rounded to bf16 for the bf16 self attention (the cast's gradient is the identity).
template <typename TA>
__device__ __forceinline__ void bwd_row(const float (&x)[RowLanes<TA>::E], const float (&d)[RowLanes<TA>::E], const float (&w)[RowLanes<TA>::E],
                                        const float (&cs)[RowLanes<TA>::E], const float (&sn)[RowLanes<TA>::E], float eps, float sgn, bool cross,
                                        float lv, float (&dx)[RowLanes<TA>::E], float (&dw)[RowLanes<TA>::E]) {
    using L = RowLanes<TA>;
    float ss = x[0] * x[0];
#pragma unroll
    for (int e = 1; e < L::E; ++e) ss += x[e] * x[e];
    const float rstd = rsqrtf(__builtin_fmaf(row_sum<L>(ss), 1.f / 64.f, eps));
    float xh[L::E], gg[L::E], dot = 0.f;
#pragma unroll
    for (int e = 0; e < L::E; ++e) {
        const float dp = __shfl_xor(d[e], L::LANES / 2, 64);
        const float dy = __builtin_fmaf(cs[e], d[e], sn[e] * (sgn * dp));   // dy_j = dout_j cos_j + (j < 32 ? +1 : -1) dout_partner sin_j
        xh[e] = x[e] * rstd;
        dw[e] = __builtin_fmaf(lv * dy, (sizeof(TA) == 2 && !cross) ? round_as<TA>(xh[e]) : xh[e], dw[e]);
        gg[e] = dy * w[e];
        dot = e ? dot + gg[e] * xh[e] : gg[e] * xh[e];
    }
    dot = row_sum<L>(dot) * (1.f / 64.f);
#pragma unroll
    for (int e = 0; e < L::E; ++e) dx[e] = rstd * __builtin_fmaf(-xh[e], dot, gg[e]);
}

// ---------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------
// The biased pre-norm values are NOT written back in bf16 (the backward adds the bias again, exactly); the fp32 kernels write them
// back.  amax_*: gamer_amax_sink(3), fp32 only: max |q_rot|, max |k_rot|, max |v + bias_v|.
template <typename TA>
__device__ __forceinline__ void fwd_amax_commit(float amq, float amk, float amv, uint32_t* amax_q, uint32_t* amax_k, uint32_t* amax_v) {
    if constexpr (sizeof(TA) == 4) {
        __shared__ uint32_t amax_lds[3][4];
        amax_block_commit(__float_as_uint(amq), amax_q, amax_lds[0]);
        amax_block_commit(__float_as_uint(amk), amax_k, amax_lds[1]);
        amax_block_commit(__float_as_uint(amv), amax_v, amax_lds[2]);
    }
}

// row-major walk (GAMER_QKNORM_ROW_MAJOR): one group of lanes per (token, head) row, the v + bias_v rows of a cross call among them
template <typename TA>
__global__ void __launch_bounds__(EW_THREADS)
qknorm_rope_fwd_row_kernel(TA* __restrict__ qkv, int T, int S, int nq, int nkv,
                           const float* __restrict__ wq, const float* __restrict__ wk, float eps,
                           const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                           const float* __restrict__ bias_q, const float* __restrict__ bias_k,
                           const float* __restrict__ bias_v, const int32_t* __restrict__ act_idx,
                           TA* __restrict__ q_rot, TA* __restrict__ k_rot, const int32_t* __restrict__ pos_ids,
                           uint32_t* __restrict__ amax_q, uint32_t* __restrict__ amax_k, uint32_t* __restrict__ amax_v) {
    using L = RowLanes<TA>;
    constexpr int E = L::E, ROWS = 64 / L::LANES;
    constexpr bool F32 = sizeof(TA) == 4;
    float amq = 0.f, amk = 0.f, amv = 0.f;
    const int lane = threadIdx.x & 63;
    const int g = lane % L::LANES, sub = lane / L::LANES;
    const int64_t wave = ((int64_t)blockIdx.x * EW_THREADS + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * EW_THREADS) >> 6;
    const bool cross = bias_q != nullptr;
    const int NH = nq + nkv + (cross ? nkv : 0);
    const int ldqkv = (nq + 2 * nkv) * 64;
    float wqv[E], wkv[E];
    ld_f32(wq + E * g, wqv);
    ld_f32(wk + E * g, wkv);
    const float sgn = g < L::LANES / 2 ? -1.f : 1.f;
    const int64_t total = (int64_t)T * NH;
    for (int64_t i0 = wave * ROWS; i0 < total; i0 += nwaves * ROWS) {
        const int64_t i = i0 + sub;
        const bool live = i < total;
        const int64_t ic = live ? i : total - 1;
        const int t = (int)(ic / NH);
        const int hd = (int)(ic % NH);
        const int a = cross ? act_idx[t] : 0;
        TA* row = qkv + (int64_t)t * ldqkv + E * g;
        float x[E], b[E];
        if (hd < nq + nkv) {
            const bool isq = hd < nq;
            L::ld(row + hd * 64, x);                  // q heads then k heads are contiguous
            if (cross) {
                ld_f32(isq ? bias_q + (int64_t)a * nq * 64 + hd * 64 + E * g : bias_k + (int64_t)a * nkv * 64 + (hd - nq) * 64 + E * g, b);
#pragma unroll
                for (int e = 0; e < E; ++e) x[e] += b[e];
                if (F32 && live) L::st(row + hd * 64, x);         // fp32: keep the pre-norm (biased) value for the backward
            }
            const int pos = pos_ids ? pos_ids[t] : t % S;        // per-token RoPE position (session model) or the index
            float cs[E], sn[E], o[E];
            ld_f32(cos_t + pos * 64 + E * g, cs);
            ld_f32(sin_t + pos * 64 + E * g, sn);
            fwd_row<TA>(x, isq ? wqv : wkv, cs, sn, eps, sgn, cross, o);
            if (live) {
                if (isq) { L::st(q_rot + (int64_t)t * nq * 64 + hd * 64 + E * g, o); if (F32) amq = amax_row(amq, o); }
                else { L::st(k_rot + (int64_t)t * nkv * 64 + (hd - nq) * 64 + E * g, o); if (F32) amk = amax_row(amk, o); }
            }
        } else {
            // (only reached when cross) v += bias_v; the shuffles of fwd_row are skipped by the whole group of lanes
            const int hv = hd - nq - nkv;
            L::ld(row + (nq + nkv + hv) * 64, x);
            ld_f32(bias_v + (int64_t)a * nkv * 64 + hv * 64 + E * g, b);
#pragma unroll
            for (int e = 0; e < E; ++e) x[e] += b[e];
            if (live) { L::st(row + (nq + nkv + hv) * 64, x); if (F32) amv = amax_row(amv, x); }
        }
    }
    fwd_amax_commit<TA>(amq, amk, amv, amax_q, amax_k, amax_v);
}

// token-major walk (the default): one group of lanes per TOKEN, walking its q and k heads three at a time (three 16-byte loads in
// flight per lane, the token's cos / sin rows and behaviour index loaded once instead of once per head, no 64-bit division per row).
// The row-major walk reached 3.5 TB/s of 5.6 achievable: one dependent load -> reduce -> store chain per lane and per iteration,
// behind ~100 integer instructions.
template <typename TA>
__global__ void __launch_bounds__(EW_THREADS)
qknorm_rope_fwd_tok_kernel(TA* __restrict__ qkv, int T, int S, int nq, int nkv,
                           const float* __restrict__ wq, const float* __restrict__ wk, float eps,
                           const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                           const float* __restrict__ bias_q, const float* __restrict__ bias_k,
                           const float* __restrict__ bias_v, const int32_t* __restrict__ act_idx,
                           TA* __restrict__ q_rot, TA* __restrict__ k_rot, const int32_t* __restrict__ pos_ids,
                           uint32_t* __restrict__ amax_q, uint32_t* __restrict__ amax_k, uint32_t* __restrict__ amax_v) {
    using L = RowLanes<TA>;
    constexpr int E = L::E, ROWS = 64 / L::LANES;
    constexpr bool F32 = sizeof(TA) == 4;
    // the bias rows of a group of heads are loaded together with the heads (bf16) or head by head (fp32, where the twelve registers
    // more would cost a wave of occupancy)
    constexpr bool BIAS_EARLY = !F32;
    float amq = 0.f, amk = 0.f, amv = 0.f;
    const int lane = threadIdx.x & 63;
    const int g = lane % L::LANES, sub = lane / L::LANES;
    const int64_t wave = ((int64_t)blockIdx.x * EW_THREADS + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * EW_THREADS) >> 6;
    const bool cross = bias_q != nullptr;
    const int nqk = nq + nkv;
    const int ldqkv = (nq + 2 * nkv) * 64;
    float wqv[E], wkv[E];
    ld_f32(wq + E * g, wqv);
    ld_f32(wk + E * g, wkv);
    const float sgn = g < L::LANES / 2 ? -1.f : 1.f;
    for (int64_t t0 = wave * ROWS; t0 < T; t0 += nwaves * ROWS) {
        const int64_t tt = t0 + sub;
        const bool live = tt < T;
        const int t = (int)(live ? tt : T - 1);
        const int a = cross ? act_idx[t] : 0;
        const int pos = pos_ids ? pos_ids[t] : t % S;
        float cs[E], sn[E], b[E];
        ld_f32(cos_t + pos * 64 + E * g, cs);
        ld_f32(sin_t + pos * 64 + E * g, sn);
        TA* row = qkv + (int64_t)t * ldqkv + E * g;
        const float* bq = cross ? bias_q + (int64_t)a * nq * 64 + E * g : nullptr;
        const float* bk = cross ? bias_k + (int64_t)a * nkv * 64 + E * g : nullptr;
        for (int h0 = 0; h0 < nqk; h0 += 3) {
            float x[3][E], bx[3][E];
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const int hd = min(h0 + u, nqk - 1);
                L::ld(row + hd * 64, x[u]);
                if (BIAS_EARLY && cross) ld_f32(hd < nq ? bq + hd * 64 : bk + (hd - nq) * 64, bx[u]);
            }
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const int hd = h0 + u;
                if (hd >= nqk) break;                       // (uniform over the wave)
                const bool isq = hd < nq;
                if (cross) {
                    if (!BIAS_EARLY) ld_f32(isq ? bq + hd * 64 : bk + (hd - nq) * 64, bx[u]);
#pragma unroll
                    for (int e = 0; e < E; ++e) x[u][e] += bx[u][e];
                    if (F32 && live) L::st(row + hd * 64, x[u]);  // fp32: keep the pre-norm (biased) value for the backward
                }
                float o[E];
                fwd_row<TA>(x[u], isq ? wqv : wkv, cs, sn, eps, sgn, cross, o);
                if (live) {
                    if (isq) { L::st(q_rot + (int64_t)t * nq * 64 + hd * 64 + E * g, o); if (F32) amq = amax_row(amq, o); }
                    else { L::st(k_rot + (int64_t)t * nkv * 64 + (hd - nq) * 64 + E * g, o); if (F32) amk = amax_row(amk, o); }
                }
            }
        }
        if (cross) {                                        // v += bias_v
            for (int hv = 0; hv < nkv; ++hv) {
                TA* dst = row + (nqk + hv) * 64;
                float xv[E];
                L::ld(dst, xv);
                ld_f32(bias_v + (int64_t)a * nkv * 64 + hv * 64 + E * g, b);
#pragma unroll
                for (int e = 0; e < E; ++e) xv[e] += b[e];
                if (live) { L::st(dst, xv); if (F32) amv = amax_row(amv, xv); }
            }
        }
    }
    fwd_amax_commit<TA>(amq, amk, amv, amax_q, amax_k, amax_v);
}

// ---------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------
// amax_out: gamer_amax_sink, fp32 only: max |dq|, |dk| (one atomic per wave)
__device__ __forceinline__ void bwd_amax_commit(float am, uint32_t* __restrict__ amax_out, int lane, uint32_t wave) {
    if (!amax_out) return;
    uint32_t m = __float_as_uint(am);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
    if (lane == 0 && m) amax_publish(m, amax_out, wave);
}

// head-major walk (the cross calls; self calls under GAMER_QKNORM_ROW_MAJOR): each wave keeps one head for its whole life so that
// the norm-weight and bias gradients accumulate in registers (one token per group of lanes and iteration).  At the end every wave
// writes its sums as one row of `partial` [waves_per_head][NH][1 + nb1][64] (slot 0: norm weight, slots 1..: bias rows) and
// qknorm_partial_reduce_kernel folds the rows in a fixed order.  (Round 1 finished with same-address float atomics from ~8000 waves
// into 64 + nb1*64 addresses per head: a 0.4 ms floor per call at every batch size.)
// NBR = compile-time bound of the bias-table rows (bf16: 4 for the shipped three behaviours, 8 otherwise)
template <typename TA, int NBR>
__global__ void __launch_bounds__(EW_THREADS)
qknorm_rope_bwd_head_kernel(const TA* __restrict__ qkv, const TA* __restrict__ dq_rot,
                            const TA* __restrict__ dk_rot, int T, int S, int nq, int nkv,
                            const float* __restrict__ wq, const float* __restrict__ wk, float eps,
                            const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                            int cross, const float* __restrict__ bias_q, const float* __restrict__ bias_k,
                            const int32_t* __restrict__ act_idx, int nb1,
                            TA* __restrict__ dqkv, float* __restrict__ partial,
                            int waves_per_head, const int32_t* __restrict__ pos_ids, uint32_t* __restrict__ amax_out) {
    using L = RowLanes<TA>;
    constexpr int E = L::E, ROWS = 64 / L::LANES;
    constexpr bool F32 = sizeof(TA) == 4;
    const int lane = threadIdx.x & 63;
    const int g = lane % L::LANES, sub = lane / L::LANES;
    const int64_t wave = ((int64_t)blockIdx.x * EW_THREADS + threadIdx.x) >> 6;
    const int NH = nq + nkv + (cross ? nkv : 0);
    if (wave >= (int64_t)NH * waves_per_head) return;
    float am = 0.f;
    const int hd = (int)(wave % NH);
    const int w0 = (int)(wave / NH);
    const int ldqkv = (nq + 2 * nkv) * 64;
    float dwacc[E], dbacc[NBR][E];
#pragma unroll
    for (int e = 0; e < E; ++e) dwacc[e] = 0.f;
#pragma unroll
    for (int a = 0; a < NBR; ++a)
#pragma unroll
        for (int e = 0; e < E; ++e) dbacc[a][e] = 0.f;
    const float sgn = g < L::LANES / 2 ? 1.f : -1.f;
    if (hd < nq + nkv) {
        const bool isq = hd < nq;
        float w[E];
        ld_f32((isq ? wq : wk) + E * g, w);
        for (int tb = w0 * ROWS; tb < T; tb += waves_per_head * ROWS) {
            const int t = tb + sub;
            const bool live = t < T;
            const int tc = live ? t : T - 1;
            float x[E], d[E], cs[E], sn[E], dx[E];
            L::ld(qkv + (int64_t)tc * ldqkv + hd * 64 + E * g, x);       // pre-norm (fp32: bias included)
            const int a_t = cross ? act_idx[tc] : 0;
            if (!F32 && cross) {
                float b[E];
                ld_f32(isq ? bias_q + (int64_t)a_t * nq * 64 + hd * 64 + E * g : bias_k + (int64_t)a_t * nkv * 64 + (hd - nq) * 64 + E * g, b);
#pragma unroll
                for (int e = 0; e < E; ++e) x[e] += b[e];
            }
            L::ld(isq ? dq_rot + (int64_t)tc * nq * 64 + hd * 64 + E * g : dk_rot + (int64_t)tc * nkv * 64 + (hd - nq) * 64 + E * g, d);
            const int pos = pos_ids ? pos_ids[tc] : tc % S;
            ld_f32(cos_t + pos * 64 + E * g, cs);
            ld_f32(sin_t + pos * 64 + E * g, sn);
            bwd_row<TA>(x, d, w, cs, sn, eps, sgn, cross, live ? 1.f : 0.f, dx, dwacc);
            if (live) {
                L::st(dqkv + (int64_t)t * ldqkv + hd * 64 + E * g, dx);
                if (F32) am = amax_row(am, dx);
            }
            if (cross) {
                const int a_l = live ? a_t : -1;
#pragma unroll
                for (int a = 0; a < NBR; ++a) {
                    const float m = (a_l == a) ? 1.f : 0.f;
#pragma unroll
                    for (int e = 0; e < E; ++e) dbacc[a][e] = __builtin_fmaf(m, dx[e], dbacc[a][e]);
                }
            }
        }
    } else {
        const int hv = hd - nq - nkv;
        for (int tb = w0 * ROWS; tb < T; tb += waves_per_head * ROWS) {
            const int t = tb + sub;
            const bool live = t < T;
            const int tc = live ? t : T - 1;
            float dv[E];
            L::ld(dqkv + (int64_t)tc * ldqkv + (nq + nkv + hv) * 64 + E * g, dv);
            const int a_t = live ? act_idx[t] : -1;
#pragma unroll
            for (int a = 0; a < NBR; ++a) {
                const float m = (a_t == a) ? 1.f : 0.f;
#pragma unroll
                for (int e = 0; e < E; ++e) dbacc[a][e] = __builtin_fmaf(m, dv[e], dbacc[a][e]);
            }
        }
    }
    if (F32) bwd_amax_commit(am, amax_out, lane, (uint32_t)wave);
    // fold the groups of lanes, then group 0 writes this wave's row of partial sums
    const int SL = 1 + (cross ? nb1 : 0);
    float* prow = partial + ((int64_t)w0 * NH + hd) * SL * 64 + E * g;
#pragma unroll
    for (int e = 0; e < E; ++e) dwacc[e] = rows_sum<L>(dwacc[e]);
    if (sub == 0) st_f32(prow, dwacc);                           // zeros for the v heads
    if (cross) {
#pragma unroll
        for (int a = 0; a < NBR; ++a) {
#pragma unroll
            for (int e = 0; e < E; ++e) dbacc[a][e] = rows_sum<L>(dbacc[a][e]);
            if (a < nb1 && sub == 0) st_f32(prow + (1 + a) * 64, dbacc[a]);
        }
    }
}

// token-major walk (the self calls: no behaviour biases), like qknorm_rope_fwd_tok_kernel: one group of lanes per token walks its q
// and k heads three at a time (six 16-byte loads in flight per lane), cos / sin once per token; the two norm-weight gradients
// accumulate in registers over all the heads of all the tokens of the wave and leave as ONE partial row [dwq | dwk] per wave
// (qknorm_partial_reduce_kernel with nq = nkv = 1 folds them).
template <typename TA>
__global__ void __launch_bounds__(EW_THREADS)
qknorm_rope_bwd_tok_kernel(const TA* __restrict__ qkv, const TA* __restrict__ dq_rot, const TA* __restrict__ dk_rot,
                           int T, int S, int nq, int nkv, const float* __restrict__ wq, const float* __restrict__ wk, float eps,
                           const float* __restrict__ cos_t, const float* __restrict__ sin_t, TA* __restrict__ dqkv,
                           float* __restrict__ partial, int n_waves, const int32_t* __restrict__ pos_ids,
                           uint32_t* __restrict__ amax_out) {
    using L = RowLanes<TA>;
    constexpr int E = L::E, ROWS = 64 / L::LANES;
    constexpr bool F32 = sizeof(TA) == 4;
    const int lane = threadIdx.x & 63;
    const int g = lane % L::LANES, sub = lane / L::LANES;
    const int wave = (int)(((int64_t)blockIdx.x * EW_THREADS + threadIdx.x) >> 6);
    if (wave >= n_waves) return;
    float am = 0.f;
    const int nqk = nq + nkv;
    const int ldqkv = (nq + 2 * nkv) * 64;
    float wqv[E], wkv[E], dwq[E], dwk[E];
    ld_f32(wq + E * g, wqv);
    ld_f32(wk + E * g, wkv);
#pragma unroll
    for (int e = 0; e < E; ++e) { dwq[e] = 0.f; dwk[e] = 0.f; }
    const float sgn = g < L::LANES / 2 ? 1.f : -1.f;
    for (int tb = wave * ROWS; tb < T; tb += n_waves * ROWS) {
        const int t = tb + sub;
        const bool live = t < T;
        const int tc = live ? t : T - 1;
        const int pos = pos_ids ? pos_ids[tc] : tc % S;
        float cs[E], sn[E];
        ld_f32(cos_t + pos * 64 + E * g, cs);
        ld_f32(sin_t + pos * 64 + E * g, sn);
        const TA* xrow = qkv + (int64_t)tc * ldqkv + E * g;
        const TA* dqrow = dq_rot + (int64_t)tc * nq * 64 + E * g;
        const TA* dkrow = dk_rot + (int64_t)tc * nkv * 64 + E * g;
        for (int h0 = 0; h0 < nqk; h0 += 3) {
            float xs[3][E], ds[3][E];
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const int hd = min(h0 + u, nqk - 1);
                L::ld(xrow + hd * 64, xs[u]);
                L::ld(hd < nq ? dqrow + hd * 64 : dkrow + (hd - nq) * 64, ds[u]);
            }
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const int hd = h0 + u;
                if (hd >= nqk) break;                       // (uniform over the wave)
                const bool isq = hd < nq;
                // bf16: the head's sum goes through bwd_row (one rounding per row, like the head-major walk).  fp32: this row's dy * x^ is
                // rounded on its own (added to -0: the product itself) and then added to the head's sum - two roundings: the bits the
                // fp32 self calls have had since this walk exists
                float dx[E], dwr[E];
#pragma unroll
                for (int e = 0; e < E; ++e) dwr[e] = F32 ? -0.f : (isq ? dwq[e] : dwk[e]);
                bwd_row<TA>(xs[u], ds[u], isq ? wqv : wkv, cs, sn, eps, sgn, false, live ? 1.f : 0.f, dx, dwr);
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    if (isq) dwq[e] = F32 ? dwq[e] + dwr[e] : dwr[e];
                    else dwk[e] = F32 ? dwk[e] + dwr[e] : dwr[e];
                }
                if (live) {
                    L::st(dqkv + (int64_t)t * ldqkv + hd * 64 + E * g, dx);
                    if (F32) am = amax_row(am, dx);
                }
            }
        }
    }
    if (F32) bwd_amax_commit(am, amax_out, lane, (uint32_t)wave);
    float* prow = partial + (int64_t)wave * 128 + E * g;
#pragma unroll
    for (int e = 0; e < E; ++e) { dwq[e] = rows_sum<L>(dwq[e]); dwk[e] = rows_sum<L>(dwk[e]); }
    if (sub == 0) {
        st_f32(prow, dwq);
        st_f32(prow + 64, dwk);
    }
}

// dwq[c] += sum over (row, q head) of slot 0; dwk likewise over the k heads; dbias_x[a][head*64 + c] += sum over rows of
// slot 1 + a.  One workgroup per 32 output columns, 32 row groups, fixed summation order (deterministic).
// QKR_CW output columns per workgroup, 1024 / QKR_CW row groups: with 32 columns per workgroup the self-attention call
// (128 output columns) ran on FOUR workgroups, every thread walking ~170 dependent-latency loads: 54 us per call at every
// batch size, 0.65 ms per step.  8 columns per workgroup = 16 (self) / 400 (cross) workgroups, ~43 / 7 loads per thread;
// 32-byte row segments out of a 2-MB, L2-resident buffer.  Fixed summation order (deterministic).
constexpr int QKR_CW = 8;
constexpr int QKR_RG = 1024 / QKR_CW;
__global__ void __launch_bounds__(1024)
qknorm_partial_reduce_kernel(const float* __restrict__ partial, int n_rows, int nq, int nkv, int cross, int nb1,
                             float* __restrict__ dwq, float* __restrict__ dwk, float* __restrict__ dbias_q,
                             float* __restrict__ dbias_k, float* __restrict__ dbias_v) {
    __shared__ float sh[16][QKR_CW];
    const int cl = threadIdx.x & (QKR_CW - 1), rg = threadIdx.x / QKR_CW;
    const int NH = nq + nkv + (cross ? nkv : 0);
    const int SL = 1 + (cross ? nb1 : 0);
    const int64_t row_stride = (int64_t)NH * SL * 64;
    const int col = blockIdx.x * QKR_CW + cl;        // [0,64): dwq, [64,128): dwk, then bias columns (head, a, c)
    int h0, h1, slot, c;
    float* dst;
    if (col < 64) { h0 = 0; h1 = nq; slot = 0; c = col; dst = dwq + c; }
    else if (col < 128) { h0 = nq; h1 = nq + nkv; slot = 0; c = col - 64; dst = dwk + c; }
    else {
        const int b = col - 128;
        const int hd = b / (nb1 * 64), a = (b / 64) % nb1;
        c = b % 64; h0 = hd; h1 = hd + 1; slot = 1 + a;
        if (hd < nq) dst = dbias_q + (int64_t)a * nq * 64 + hd * 64 + c;
        else if (hd < nq + nkv) dst = dbias_k + (int64_t)a * nkv * 64 + (hd - nq) * 64 + c;
        else dst = dbias_v + (int64_t)a * nkv * 64 + (hd - nq - nkv) * 64 + c;
    }
    const int nh = h1 - h0;
    const int64_t n_items = (int64_t)n_rows * nh;     // (row, head) pairs to add up
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    auto at = [&](int64_t it) { return partial[(it / nh) * row_stride + ((int64_t)(h0 + it % nh) * SL + slot) * 64 + c]; };
    int64_t it = rg;
    for (; it + 3 * QKR_RG < n_items; it += 4 * QKR_RG) {
        s0 += at(it); s1 += at(it + QKR_RG); s2 += at(it + 2 * QKR_RG); s3 += at(it + 3 * QKR_RG);
    }
    for (; it < n_items; it += QKR_RG) s0 += at(it);
    // a wave holds 8 row groups of the same 8 columns: fold them with three shuffles, then the 16 waves through LDS
    float t = (s0 + s1) + (s2 + s3);
    t += __shfl_xor(t, 8, 64); t += __shfl_xor(t, 16, 64); t += __shfl_xor(t, 32, 64);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane < QKR_CW) sh[w][lane] = t;
    __syncthreads();
    if (threadIdx.x < QKR_CW) {
        float tot = 0.f;
#pragma unroll
        for (int gi = 0; gi < 16; ++gi) tot += sh[gi][threadIdx.x];
        *dst += tot;
    }
}

// ---------------------------------------------------------------------------------------------
// host API
// ---------------------------------------------------------------------------------------------
static bool qknorm_row_major() {
    static EnvSwitch sw("GAMER_QKNORM_ROW_MAJOR");          // (the round-1 walks, kept for A/B runs and as the tests' bit reference)
    return sw.is_set();
}

template <typename TA>
static int qknorm_rope_fwd_impl(const char* name, TA* qkv, int T, int S, int nq, int nkv, const float* wq,
                                const float* wk, float eps, const float* cos_t, const float* sin_t, const float* bias_q,
                                const float* bias_k, const float* bias_v, const int32_t* act_idx, TA* q_rot, TA* k_rot,
                                const int32_t* pos_ids, void* stream) {
    GAMER_CHECK_ARG(qkv && wq && wk && cos_t && sin_t && q_rot && k_rot, "%s: null pointer", name);
    GAMER_CHECK_ARG(T > 0 && S > 0 && nq > 0 && nkv > 0 && T % S == 0, "%s: bad shape T=%d S=%d nq=%d nkv=%d", name, T, S, nq, nkv);
    const bool cross = bias_q != nullptr;
    GAMER_CHECK_ARG(!cross || (bias_k && bias_v && act_idx), "%s: cross needs bias_k, bias_v, act_idx", name);
    const int NH = nq + nkv + (cross ? nkv : 0);
    constexpr int ROWS = 64 / RowLanes<TA>::LANES;                 // rows per wave iteration
    AmaxSink sink = {};
    if constexpr (sizeof(TA) == 4) sink = take_amax_sink();
    const bool row_major = qknorm_row_major();
    const dim3 grid(grid_for_waves(((int64_t)T * (row_major ? NH : 1) + ROWS - 1) / ROWS));
    return with_flags([&](auto rm) {
        return launch<rm() ? qknorm_rope_fwd_row_kernel<TA> : qknorm_rope_fwd_tok_kernel<TA>>(
            name, grid, dim3(EW_THREADS), 0, ST(stream), qkv, T, S, nq, nkv, wq, wk, eps, cos_t, sin_t, bias_q, bias_k, bias_v, act_idx, q_rot,
            k_rot, pos_ids, sink.out[0], sink.out[1], sink.out[2]);
    }, row_major);
}
extern "C" int gamer_qknorm_rope_fwd(float* qkv, int T, int S, int nq, int nkv, const float* wq, const float* wk,
                                     float eps, const float* cos_t, const float* sin_t, const float* bias_q,
                                     const float* bias_k, const float* bias_v, const int32_t* act_idx, float* q_rot,
                                     float* k_rot, const int32_t* pos_ids, void* stream) {
    return qknorm_rope_fwd_impl<float>("gamer_qknorm_rope_fwd", qkv, T, S, nq, nkv, wq, wk, eps, cos_t, sin_t, bias_q,
                                       bias_k, bias_v, act_idx, q_rot, k_rot, pos_ids, stream);
}
extern "C" int gamer_qknorm_rope_fwd_bf16(gamer_bf16* qkv, int T, int S, int nq, int nkv, const float* wq,
                                          const float* wk, float eps, const float* cos_t, const float* sin_t,
                                          const float* bias_q, const float* bias_k, const float* bias_v,
                                          const int32_t* act_idx, gamer_bf16* q_rot, gamer_bf16* k_rot,
                                          const int32_t* pos_ids, void* stream) {
    return qknorm_rope_fwd_impl<bf16_t>("gamer_qknorm_rope_fwd_bf16", (bf16_t*)qkv, T, S, nq, nkv, wq, wk, eps, cos_t,
                                        sin_t, bias_q, bias_k, bias_v, act_idx, (bf16_t*)q_rot, (bf16_t*)k_rot, pos_ids,
                                        stream);
}

template <typename TA>
static int qknorm_rope_bwd_impl(const char* name, const TA* qkv, const TA* dq_rot, const TA* dk_rot, int T, int S,
                                int nq, int nkv, const float* wq, const float* wk, float eps, const float* cos_t,
                                const float* sin_t, const float* bias_q, const float* bias_k, const int32_t* act_idx,
                                int nb1, TA* dqkv, float* dwq, float* dwk, float* dbias_q, float* dbias_k,
                                float* dbias_v, const int32_t* pos_ids, float* partial, int64_t partial_numel,
                                void* stream) {
    GAMER_CHECK_ARG(qkv && dq_rot && dk_rot && wq && wk && cos_t && sin_t && dqkv && dwq && dwk && partial,
                    "%s: null pointer", name);
    GAMER_CHECK_ARG(T > 0 && S > 0 && nq > 0 && nkv > 0 && T % S == 0, "%s: bad shape", name);
    const int cross = bias_q != nullptr ? 1 : 0;
    GAMER_CHECK_ARG(!cross || (bias_k && act_idx && dbias_q && dbias_k && dbias_v && nb1 > 0 && nb1 <= TBL_MAXROWS),
                    "%s: cross needs bias_k, act_idx, dbias_*, 0<nb1<=8 (nb1=%d)", name, nb1);
    const int NH = nq + nkv + (cross ? nkv : 0);
    const int SL = 1 + (cross ? nb1 : 0);
    constexpr bool F32 = sizeof(TA) == 4;
    constexpr int ROWS = 64 / RowLanes<TA>::LANES;                 // token rows per wave iteration
    int waves_per_head = 8192 / NH;
    if (waves_per_head > (T + ROWS - 1) / ROWS) waves_per_head = (T + ROWS - 1) / ROWS;
    const int64_t cap = partial_numel / ((int64_t)NH * SL * 64);
    if (waves_per_head > cap) waves_per_head = (int)cap;
    GAMER_CHECK_ARG(waves_per_head >= 1 && aligned16(partial),
                    "%s: partial needs at least %d floats, 16-byte aligned (got %lld)", name, NH * SL * 64,
                    (long long)partial_numel);
    int n_waves = (T + ROWS - 1) / ROWS;
    if (n_waves > 8192) n_waves = 8192;
    if ((int64_t)n_waves * 128 > partial_numel) n_waves = (int)(partial_numel / 128);
    auto reduce = [&](int n_rows, int rq, int rkv, int rcross, int rnb1, int cols) {
        return launch<qknorm_partial_reduce_kernel>(name, dim3(cols / QKR_CW), dim3(1024), 0, ST(stream), (const float*)partial, n_rows, rq, rkv,
                                                    rcross, rnb1, dwq, dwk, dbias_q, dbias_k, dbias_v);
    };
    uint32_t* amax_out = nullptr;
    if (!cross && !qknorm_row_major() && n_waves >= 1) {
        // self attention: token-major (one partial row [dwq | dwk] per wave; the reduce sees one q and one k "head")
        if constexpr (F32) amax_out = take_amax_sink().out[0];
        GAMER_TRY(launch<qknorm_rope_bwd_tok_kernel<TA>>(name, dim3((n_waves + EW_WAVES - 1) / EW_WAVES), dim3(EW_THREADS), 0, ST(stream), qkv,
                                                         dq_rot, dk_rot, T, S, nq, nkv, wq, wk, eps, cos_t, sin_t, dqkv, partial, n_waves,
                                                         pos_ids, amax_out));
        return reduce(n_waves, 1, 1, 0, 0, 128);
    }
    const int64_t total_waves = (int64_t)NH * waves_per_head;
    const dim3 grid((int)((total_waves + EW_WAVES - 1) / EW_WAVES));
    if constexpr (F32) amax_out = take_amax_sink().out[0];
    GAMER_TRY(with_flags([&](auto four) {                    // (bf16 only: four bias rows hold the shipped three behaviours)
        return launch<qknorm_rope_bwd_head_kernel<TA, (!F32 && four()) ? 4 : TBL_MAXROWS>>(
            name, grid, dim3(EW_THREADS), 0, ST(stream), qkv, dq_rot, dk_rot, T, S, nq, nkv, wq, wk, eps, cos_t, sin_t, cross, bias_q, bias_k,
            act_idx, nb1, dqkv, partial, waves_per_head, pos_ids, amax_out);
    }, !cross || nb1 <= 4));
    return reduce(waves_per_head, nq, nkv, cross, nb1, 128 + (cross ? NH * nb1 * 64 : 0));
}
extern "C" int gamer_qknorm_rope_bwd(const float* qkv, const float* dq_rot, const float* dk_rot, int T, int S, int nq,
                                     int nkv, const float* wq, const float* wk, float eps, const float* cos_t,
                                     const float* sin_t, const float* bias_q, const float* bias_k,
                                     const int32_t* act_idx, int nb1, float* dqkv, float* dwq, float* dwk,
                                     float* dbias_q, float* dbias_k, float* dbias_v, const int32_t* pos_ids,
                                     float* partial, int64_t partial_numel, void* stream) {
    return qknorm_rope_bwd_impl<float>("gamer_qknorm_rope_bwd", qkv, dq_rot, dk_rot, T, S, nq, nkv, wq, wk, eps, cos_t,
                                       sin_t, bias_q, bias_k, act_idx, nb1, dqkv, dwq, dwk, dbias_q, dbias_k, dbias_v,
                                       pos_ids, partial, partial_numel, stream);
}
extern "C" int gamer_qknorm_rope_bwd_bf16(const gamer_bf16* qkv, const gamer_bf16* dq_rot, const gamer_bf16* dk_rot,
                                          int T, int S, int nq, int nkv, const float* wq, const float* wk, float eps,
                                          const float* cos_t, const float* sin_t, const float* bias_q,
                                          const float* bias_k, const int32_t* act_idx, int nb1, gamer_bf16* dqkv,
                                          float* dwq, float* dwk, float* dbias_q, float* dbias_k, float* dbias_v,
                                          const int32_t* pos_ids, float* partial, int64_t partial_numel, void* stream) {
    return qknorm_rope_bwd_impl<bf16_t>("gamer_qknorm_rope_bwd_bf16", (const bf16_t*)qkv, (const bf16_t*)dq_rot,
                                        (const bf16_t*)dk_rot, T, S, nq, nkv, wq, wk, eps, cos_t, sin_t, bias_q, bias_k,
                                        act_idx, nb1, (bf16_t*)dqkv, dwq, dwk, dbias_q, dbias_k, dbias_v, pos_ids,
                                        partial, partial_numel, stream);
}

}  // namespace gamer
