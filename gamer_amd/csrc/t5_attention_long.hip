// T5's attention for 1 <= Sq, Sk <= 512: the key-streaming family next to the resident kernels of t5_attention.hip, whose header
// states the semantics (scores without 1 / sqrt(d), the bias by relative offset, allowed keys, rows with no allowed key, the dropout
// element index, beam rows).  No buffer here is sized by the sequence: K / V (forward, row term, dQ) or Q / dO (dK, dV) pass through
// LDS in blocks of 64 rows, and nothing of size Sq x Sk reaches memory.  All products run on v_mfma_f32_16x16x4_f32 through the
// helpers of t5_attention_common.h.
//   forward   one workgroup per (row, head, block of 64 queries), a wave per 16 queries; the keys stream in blocks of 64 with an
//             online softmax (running maximum m, sum l, accumulator rescaled per block).  Sq <= 16 (decoding's cross attention):
//             all four waves take the one query tile and every fourth key tile, and (m, l, acc) are combined once through LDS in
//             wave order.
//   backward  three launches, every output element with one owner and every sum in a fixed order (no float atomics):
//             row terms per (row, head, query block), the keys in order, into the workspace [2][B][H][Sq]: c_i = 1 / sum_j exp(s_ij -
//                       lse_i), which takes the rounding of the saved lse (an ulp of a number of O(10), the same factor on every
//                       key of the row) out of the recomputed p = c_i exp(s_ij - lse_i), so that a row's dS sum to zero as they do
//                       for the forward's own p; and delta_i = sum_j dropout(p)[i, j] dP[i, j] - summed from the products it is
//                       subtracted from, as in the resident backward.  Both sums run over up to 512 keys and are kept in fp64
//             dK, dV    one workgroup per (row, head, block of 64 keys), a wave per 16 keys (K / V rows as register operands), the
//                       queries and dO stream through LDS: the tiles S = Q K^T and dP = dO V^T come out with the key on the lane,
//                       which is the A operand of dV += P^T dO and dK += dS^T Q
//             dQ, bias  a wave per 16 queries, K / V stream; with a bias workgroup (slab, head) walks the rows slab, slab + n_slab,
//                       ... and their query blocks, puts each 64 x 64 tile of dS into LDS and adds its diagonals, queries in order,
//                       to an LDS accumulator of Sq + Sk - 1 offsets that it writes to its slab at the end; without a bias one
//                       workgroup per (row, head, query block)
// The packed forms (PK = true, semantics at the top of t5_attention.hip): the grids keep the dense geometry (a.Sq, a.Sk); a workgroup whose
// query block (forward, row terms, dQ) or key block (dK, dV) lies past its row's end returns before it touches memory, and the key / query
// loops run to the row's own lengths.  The row terms are [2][H][Tq].
// Causal: key blocks wholly above the diagonal of a query block are skipped (every score there is masked).
#include "t5_attention_common.h"

namespace gamer {

constexpr int T5L_MAX_S = 512, T5L_QB = 64, T5L_KB = 64;
static_assert(T5L_QB == 16 * T5_WAVES && T5L_KB == 64 && T5L_MAX_S <= T5_BIAS_MAX_S, "a wave per 16 rows of a block");

// keep flags of the keys k0 .. k0 + 63 of row b
__device__ __forceinline__ void t5l_stage_keep(int* __restrict__ kp, const uint8_t* __restrict__ keep, int b, int Sk, int k0) {
    for (int j = threadIdx.x; j < T5L_KB; j += T5_THREADS) kp[j] = k0 + j < Sk && (!keep || keep[(int64_t)b * Sk + k0 + j]) ? 1 : 0;
}
// the value of query (lane & 15)'s lane for the accumulator row 4 (lane >> 4) + reg
__device__ __forceinline__ float t5l_row_value(float v, int reg, int lane) { return __shfl(v, 4 * (lane >> 4) + reg, 64); }

template <int D, bool PK>
__global__ void __launch_bounds__(T5_THREADS)
t5l_attn_fwd_kernel(const T5Args a, float* __restrict__ o, int ldo, float* __restrict__ lse) {
    constexpr int LD = D + 4;
    __shared__ __attribute__((aligned(16))) float Ks[T5L_KB * LD];
    __shared__ __attribute__((aligned(16))) float Vs[T5L_KB * LD];
    __shared__ int kp[T5L_KB];
    const int nqb = (a.Sq + T5L_QB - 1) / T5L_QB;                           // (the grid: query blocks of the dense geometry)
    const int qb = blockIdx.x % nqb, bh = blockIdx.x / nqb, b = bh / a.H, hh = bh % a.H;
    const int bk = a.kv_rows ? a.kv_rows[b] : b;
    const T5Row row = t5_row<PK>(a, b, bk, hh);
    const int Sq = row.Sq, Sk = row.Sk;
    if (PK && qb * T5L_QB >= Sq) return;                                    // a query block past the row's end
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool split = a.Sq <= 16;                                          // one query tile: the waves share its key tiles
    const int q0 = qb * T5L_QB + (split ? 0 : wave * 16);
    const bool active = q0 < Sq;
    const int i = q0 + (lane & 15);
    const bool iv = i < Sq;
    const int q_last = min(Sq, (qb + 1) * T5L_QB) - 1;
    const DropoutRng rng(a.p_drop, a.seed);
    float qr[D / 4];
    t5_row_operand<D>(qr, iv ? a.q + (row.q0 + i) * a.ldq + hh * D : nullptr, lane);
    const float* relrow = a.rel ? a.rel + (int64_t)hh * (a.Sq + a.Sk - 1) + (a.Sq - 1 - i) : nullptr;      // read at [j] for allowed (i, j) only
    float m = -INFINITY, l = 0.f;                                           // l: this lane's keys only until the end
    f32x4v acc[D / 16];
#pragma unroll
    for (int n = 0; n < D / 16; ++n) acc[n] = f32x4v{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < Sk; k0 += T5L_KB) {
        if (a.causal && k0 > q_last) break;
        const int rows = min(T5L_KB, Sk - k0), nt = (rows + 15) / 16;
        __syncthreads();                                                    // (the block before is consumed)
        t5_stage<D>(Ks, a.k + (row.k0 + k0) * a.ldk + hh * D, a.ldk, rows, nt * 16);
        t5_stage<D>(Vs, a.v + (row.k0 + k0) * a.ldv + hh * D, a.ldv, rows, nt * 16);
        t5l_stage_keep(kp, a.keep, bk, Sk, k0);
        __syncthreads();
        const int mine = !active ? 0 : split ? (wave < nt ? 1 : 0) : nt;      // key tiles of this wave in this block
        f32x4v s[4];
        float mb = -INFINITY;
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (t < mine) {
                const int kt = split ? wave : t;
                s[t] = t5_tile<D>(Ks + kt * 16 * LD, qr, lane);
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int jl = kt * 16 + 4 * (lane >> 4) + reg, j = k0 + jl;
                    const bool ok = iv && kp[jl] && (!a.causal || j <= i);
                    s[t][reg] = ok ? s[t][reg] + (relrow ? relrow[j] : 0.f) : -INFINITY;
                    mb = fmaxf(mb, s[t][reg]);
                }
            }
        const float mn = fmaxf(m, t5_xor_max(mb));
        const float ms = mn == -INFINITY ? 0.f : mn;
        const float alpha = expf(m - ms);                                   // (1 when the maximum stays, 0 from -inf)
        m = mn;
        l *= alpha;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const float ar = t5l_row_value(alpha, reg, lane);
#pragma unroll
            for (int n = 0; n < D / 16; ++n) acc[n][reg] *= ar;
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (t < mine) {
                const int kt = split ? wave : t;
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int j = k0 + kt * 16 + 4 * (lane >> 4) + reg;
                    float p = expf(s[t][reg] - ms);                         // (a key that is not allowed: exp(-inf) = 0)
                    l += p;
                    if (rng.on && iv && j < Sk) p *= rng.mult((((uint64_t)b * a.H + hh) * a.Sq + i) * a.Sk + j);
                    s[t][reg] = p;
                }
                t5_tile_out<D>(acc, s[t], Vs + kt * 16 * LD, lane);
            }
    }
    l = t5_xor_sum(l);
    float* ob = o + row.q0 * ldo + hh * D;
    float* lb = lse + row.l0;
    if (!split) {
        if (!active) return;
        if (iv && lane < 16) lb[i] = m + logf(l);                           // (no allowed key: -inf + -inf)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const float lr = t5l_row_value(l, reg, lane);
#pragma unroll
            for (int n = 0; n < D / 16; ++n) acc[n][reg] = lr > 0.f ? acc[n][reg] / lr : 0.f;
        }
        t5_store_rows<D>(ob, ldo, q0, Sq, acc, lane);
        return;
    }
    // ---- Sq <= 16: (m, l, acc) of the four waves through LDS, combined in wave order -------------------------------------------------
    float* cacc = Ks;                                                       // [wave][16][D]
    float* cm = Vs;                                                         // [wave][16]
    float* cl = Vs + T5_WAVES * 16;                                         // [wave][16]
    __syncthreads();                                                        // (the last block is consumed)
    if (lane < 16) {
        cm[wave * 16 + lane] = m;
        cl[wave * 16 + lane] = l;
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg)
#pragma unroll
        for (int n = 0; n < D / 16; ++n) cacc[(wave * 16 + 4 * (lane >> 4) + reg) * D + 16 * n + (lane & 15)] = acc[n][reg];
    __syncthreads();
    for (int e = threadIdx.x; e < Sq * D; e += T5_THREADS) {
        const int iq = e / D, c = e % D;
        float mm = -INFINITY;
        for (int w = 0; w < T5_WAVES; ++w) mm = fmaxf(mm, cm[w * 16 + iq]);
        const float ms = mm == -INFINITY ? 0.f : mm;
        float ls = 0.f, as = 0.f;
        for (int w = 0; w < T5_WAVES; ++w) {
            const float f = expf(cm[w * 16 + iq] - ms);
            ls += cl[w * 16 + iq] * f;
            as += cacc[(w * 16 + iq) * D + c] * f;
        }
        ob[(int64_t)iq * ldo + c] = ls > 0.f ? as / ls : 0.f;
        if (c == 0) lb[iq] = mm + logf(ls);
    }
}

// p and the dropout multiplier of one element in the backward: p from the saved log-sum-exp l and the row's normaliser c
struct T5lProb {
    float p, m;
};
__device__ __forceinline__ double t5l_xor_sum(double v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}
__device__ __forceinline__ T5lProb t5l_prob(const T5Args& a, const DropoutRng& rng, bool ok, float s, float relv, float l, float c, int b,
                                            int hh, int i, int j) {
    T5lProb r{0.f, 1.f};
    if (ok) {
        r.p = expf(s + relv - l) * c;
        if (rng.on) r.m = rng.mult((((uint64_t)b * a.H + hh) * a.Sq + i) * a.Sk + j);
    }
    return r;
}

// Query-side walk of the backward.  DQ = false: the row terms alone (grid B H nqb; row_ws = [delta | c], each [B][H][Sq]).  DQ = true: dQ and, with `drel_part`, the offset
// gradient (grid n_slab H, the workgroup walks its rows and their query blocks); without it grid B H nqb.
template <int D, bool DQ, bool BIAS, bool PK>
__global__ void __launch_bounds__(T5_THREADS)
t5l_attn_bwd_q_kernel(const T5Args a, const float* __restrict__ d_o, int ldo, const float* __restrict__ lse, float* __restrict__ row_ws,
                      float* __restrict__ dq, int lddq, float* __restrict__ drel_part, int n_slab) {
    constexpr int LD = D + 4, LDS_ = T5L_KB + 4;
    __shared__ __attribute__((aligned(16))) float Ks[T5L_KB * LD];
    __shared__ __attribute__((aligned(16))) float Vs[T5L_KB * LD];
    __shared__ __attribute__((aligned(16))) float dSs[BIAS ? T5L_QB * LDS_ : 4];      // one tile of dS [query][key]
    __shared__ float dacc[BIAS ? 2 * T5L_MAX_S : 1];                                    // the offset gradient of this workgroup
    __shared__ int kp[T5L_KB];
    const int nqb = (a.Sq + T5L_QB - 1) / T5L_QB, R = a.Sq + a.Sk - 1;      // (the dense geometry: the grid and the offsets)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const DropoutRng rng(a.p_drop, a.seed);
    float* delta = row_ws;
    float* norm = row_ws + (PK ? (int64_t)a.H * a.Tq : (int64_t)a.B * a.H * a.Sq);
    int hh, b_first, b_step, b_end, qb_first, qb_end;
    if (BIAS) {
        hh = blockIdx.x % a.H;
        b_first = blockIdx.x / a.H, b_step = n_slab, b_end = a.B, qb_first = 0, qb_end = nqb;
        for (int r = threadIdx.x; r < R; r += T5_THREADS) dacc[r] = 0.f;
    } else {
        const int bh = blockIdx.x / nqb;
        hh = bh % a.H;
        b_first = bh / a.H, b_step = 1, b_end = b_first + 1, qb_first = blockIdx.x % nqb, qb_end = qb_first + 1;
    }
    for (int b = b_first; b < b_end; b += b_step) {
        const T5Row row = t5_row<PK>(a, b, b, hh);
        const int Sq = row.Sq, Sk = row.Sk;
        for (int qb = qb_first; qb < qb_end && qb * T5L_QB < Sq; ++qb) {     // (packed: query blocks past the row's end have nothing to do)
            const int q0 = qb * T5L_QB + wave * 16;
            const bool active = q0 < Sq;
            const int i = q0 + (lane & 15);
            const bool iv = i < Sq;
            const int q_rows = min(T5L_QB, Sq - qb * T5L_QB), q_last = qb * T5L_QB + q_rows - 1;
            float qr[D / 4], gr[D / 4];
            t5_row_operand<D>(qr, iv ? a.q + (row.q0 + i) * a.ldq + hh * D : nullptr, lane);
            t5_row_operand<D>(gr, iv ? d_o + (row.q0 + i) * ldo + hh * D : nullptr, lane);
            const float* relrow = a.rel ? a.rel + (int64_t)hh * R + (a.Sq - 1 - i) : nullptr;
            const float l = iv ? lse[row.l0 + i] : 0.f;
            float dl = DQ && iv ? delta[row.l0 + i] : 0.f;
            const float cn = DQ && iv ? norm[row.l0 + i] : 1.f;
            double zs = 0.0, dls = 0.0;                                     // the row sums of 512 terms: fp64, a few adds per element
            f32x4v acc[D / 16];
#pragma unroll
            for (int n = 0; n < D / 16; ++n) acc[n] = f32x4v{0.f, 0.f, 0.f, 0.f};
            for (int k0 = 0; k0 < Sk; k0 += T5L_KB) {
                if (a.causal && k0 > q_last) break;
                const int rows = min(T5L_KB, Sk - k0), nt = (rows + 15) / 16;
                __syncthreads();                                            // (the block before is consumed, dS tile included)
                t5_stage<D>(Ks, a.k + (row.k0 + k0) * a.ldk + hh * D, a.ldk, rows, nt * 16);
                t5_stage<D>(Vs, a.v + (row.k0 + k0) * a.ldv + hh * D, a.ldv, rows, nt * 16);
                t5l_stage_keep(kp, a.keep, b, Sk, k0);
                __syncthreads();
                if (active)
                    for (int t = 0; t < nt; ++t) {
                        const f32x4v s = t5_tile<D>(Ks + t * 16 * LD, qr, lane);
                        const f32x4v dp = t5_tile<D>(Vs + t * 16 * LD, gr, lane);
                        f32x4v ds;
#pragma unroll
                        for (int reg = 0; reg < 4; ++reg) {
                            const int jl = t * 16 + 4 * (lane >> 4) + reg, j = k0 + jl;
                            const bool ok = iv && kp[jl] && (!a.causal || j <= i);
                            const T5lProb pr = t5l_prob(a, rng, ok, s[reg], ok && relrow ? relrow[j] : 0.f, l, cn, b, hh, i, j);
                            if (DQ) {
                                ds[reg] = pr.p * (pr.m * dp[reg] - dl);
                            } else {
                                dls += (double)(pr.p * pr.m * dp[reg]);
                                zs += (double)pr.p;
                            }
                        }
                        if (DQ) {
                            t5_tile_out<D>(acc, ds, Ks + t * 16 * LD, lane);
                            if (BIAS)
                                *reinterpret_cast<float4*>(dSs + (wave * 16 + (lane & 15)) * LDS_ + t * 16 + 4 * (lane >> 4)) =
                                    make_float4(ds[0], ds[1], ds[2], ds[3]);
                        }
                    }
                if (BIAS) {
                    // the diagonals j - i of this tile, queries in order, onto the offsets (only elements written above are read)
                    __syncthreads();
                    const int off = (int)threadIdx.x - (T5L_QB - 1);
                    if (off < T5L_KB) {
                        float sum = 0.f;
                        for (int il = max(0, -off); il < q_rows && il + off < rows; ++il) sum += dSs[il * LDS_ + il + off];
                        const int r = k0 - qb * T5L_QB + off + a.Sq - 1;
                        if (r >= 0 && r < R) dacc[r] += sum;
                    }
                }
            }
            if (!active) continue;
            if (DQ) {
                t5_store_rows<D>(dq + row.q0 * lddq + hh * D, lddq, q0, Sq, acc, lane);
            } else {
                zs = t5l_xor_sum(zs);
                dls = t5l_xor_sum(dls);
                if (iv && lane < 16) {                                      // (no allowed key: every p is 0 anyway)
                    delta[row.l0 + i] = zs > 0.0 ? (float)(dls / zs) : 0.f;
                    norm[row.l0 + i] = zs > 0.0 ? (float)(1.0 / zs) : 0.f;
                }
            }
        }
    }
    if (BIAS) {
        __syncthreads();
        float* slab = drel_part + ((int64_t)(blockIdx.x / a.H) * a.H + hh) * R;
        for (int r = threadIdx.x; r < R; r += T5_THREADS) slab[r] = dacc[r];
    }
}

// dK and dV of 64 keys: a wave per 16 keys, the queries and dO stream through LDS
template <int D, bool PK>
__global__ void __launch_bounds__(T5_THREADS)
t5l_attn_bwd_kv_kernel(const T5Args a, const float* __restrict__ d_o, int ldo, const float* __restrict__ lse, const float* __restrict__ row_ws,
                       float* __restrict__ dk, int lddk, float* __restrict__ dv, int lddv) {
    constexpr int LD = D + 4;
    __shared__ __attribute__((aligned(16))) float Qs[T5L_QB * LD];
    __shared__ __attribute__((aligned(16))) float Gs[T5L_QB * LD];
    __shared__ float ls[T5L_QB], dls[T5L_QB], cs[T5L_QB];
    const int nkb = (a.Sk + T5L_KB - 1) / T5L_KB, R = a.Sq + a.Sk - 1;      // (the dense geometry: the grid and the offsets)
    const int kb = blockIdx.x % nkb, bh = blockIdx.x / nkb, b = bh / a.H, hh = bh % a.H;
    const T5Row row = t5_row<PK>(a, b, b, hh);
    const int Sq = row.Sq, Sk = row.Sk;
    if (PK && kb * T5L_KB >= Sk) return;                                    // a key block past the row's end
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j0 = kb * T5L_KB + wave * 16, j = j0 + (lane & 15);
    const bool active = j0 < Sk, jv = j < Sk;
    const bool kept = jv && (!a.keep || a.keep[(int64_t)b * Sk + j]);
    const float* delta = row_ws;
    const float* norm = row_ws + (PK ? (int64_t)a.H * a.Tq : (int64_t)a.B * a.H * a.Sq);
    const DropoutRng rng(a.p_drop, a.seed);
    float kr[D / 4], vr[D / 4];
    t5_row_operand<D>(kr, jv ? a.k + (row.k0 + j) * a.ldk + hh * D : nullptr, lane);
    t5_row_operand<D>(vr, jv ? a.v + (row.k0 + j) * a.ldv + hh * D : nullptr, lane);
    const float* relcol = a.rel ? a.rel + (int64_t)hh * R + (j + a.Sq - 1) : nullptr;                  // read at [-i] for allowed (i, j) only
    f32x4v acck[D / 16], accv[D / 16];
#pragma unroll
    for (int n = 0; n < D / 16; ++n) acck[n] = accv[n] = f32x4v{0.f, 0.f, 0.f, 0.f};
    const int qb_first = a.causal ? kb * T5L_KB / T5L_QB : 0;               // (query blocks wholly before the key block see none of it)
    for (int q0 = qb_first * T5L_QB; q0 < Sq; q0 += T5L_QB) {
        const int rows = min(T5L_QB, Sq - q0), nt = (rows + 15) / 16;
        __syncthreads();                                                    // (the block before is consumed)
        t5_stage<D>(Qs, a.q + (row.q0 + q0) * a.ldq + hh * D, a.ldq, rows, nt * 16);
        t5_stage<D>(Gs, d_o + (row.q0 + q0) * ldo + hh * D, ldo, rows, nt * 16);
        for (int il = threadIdx.x; il < T5L_QB; il += T5_THREADS) {
            ls[il] = il < rows ? lse[row.l0 + q0 + il] : 0.f;
            dls[il] = il < rows ? delta[row.l0 + q0 + il] : 0.f;
            cs[il] = il < rows ? norm[row.l0 + q0 + il] : 0.f;
        }
        __syncthreads();
        if (active)
            for (int t = 0; t < nt; ++t) {
                const f32x4v s = t5_tile<D>(Qs + t * 16 * LD, kr, lane);    // [query 4 (lane >> 4) + reg][key lane & 15]
                const f32x4v dp = t5_tile<D>(Gs + t * 16 * LD, vr, lane);
                f32x4v pd, ds;
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int il = t * 16 + 4 * (lane >> 4) + reg, i = q0 + il;
                    const bool ok = kept && i < Sq && (!a.causal || j <= i);
                    const T5lProb pr = t5l_prob(a, rng, ok, s[reg], ok && relcol ? relcol[-i] : 0.f, ls[il], cs[il], b, hh, i, j);
                    pd[reg] = pr.p * pr.m;
                    ds[reg] = pr.p * (pr.m * dp[reg] - dls[il]);
                }
                t5_tile_out<D>(accv, pd, Gs + t * 16 * LD, lane);
                t5_tile_out<D>(acck, ds, Qs + t * 16 * LD, lane);
            }
    }
    if (!active) return;
    t5_store_rows<D>(dk + row.k0 * lddk + hh * D, lddk, j0, Sk, acck, lane);
    t5_store_rows<D>(dv + row.k0 * lddv + hh * D, lddv, j0, Sk, accv, lane);
}

}  // namespace gamer

using namespace gamer;
#define ST(s) ((hipStream_t)(s))

static int t5l_grid(const char* name, int B, int H, int blocks) {
    GAMER_CHECK_ARG((int64_t)B * H * blocks < (1LL << 31), "%s: bad shape B=%d H=%d (B H blocks of 64 rows < 2^31)", name, B, H);
    return 0;
}

extern "C" int gamer_t5_attn_long_fwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* rel,
                                      const uint8_t* keep, const int32_t* kv_rows, int B, int Sq, int Sk, int H, int head_dim, int causal,
                                      float p_drop, uint64_t seed, float* o, int ldo, float* lse, void* stream) {
    const char* name = "gamer_t5_attn_long_fwd";
    T5Args a;
    GAMER_TRY(t5_args(name, a, q, ldq, k, ldk, v, ldv, rel, keep, B, Sq, Sk, H, head_dim, causal, p_drop, seed, T5L_MAX_S));
    a.kv_rows = kv_rows;
    GAMER_CHECK_ARG(o && lse && ldo >= H * head_dim, "%s: bad output", name);
    const int nqb = (Sq + T5L_QB - 1) / T5L_QB;
    GAMER_TRY(t5l_grid(name, B, H, nqb));
    if (head_dim == 64) return launch<t5l_attn_fwd_kernel<64, false>>(name, dim3(B * H * nqb), dim3(T5_THREADS), 0, ST(stream), a, o, ldo, lse);
    return launch<t5l_attn_fwd_kernel<32, false>>(name, dim3(B * H * nqb), dim3(T5_THREADS), 0, ST(stream), a, o, ldo, lse);
}

template <int D, bool PK>
static int t5l_bwd(const char* name, const T5Args& a, const float* d_o, int ldo, const float* lse, float* dq, int lddq, float* dk, int lddk,
                   float* dv, int lddv, float* drel_partial, int n_slab, float* delta, hipStream_t st) {
    const int nqb = (a.Sq + T5L_QB - 1) / T5L_QB, nkb = (a.Sk + T5L_KB - 1) / T5L_KB, rows = a.B * a.H;
    GAMER_TRY(launch<t5l_attn_bwd_q_kernel<D, false, false, PK>>(name, dim3(rows * nqb), dim3(T5_THREADS), 0, st, a, d_o, ldo, lse, delta,
                                                              (float*)nullptr, 0, (float*)nullptr, 0));
    GAMER_TRY(launch<t5l_attn_bwd_kv_kernel<D, PK>>(name, dim3(rows * nkb), dim3(T5_THREADS), 0, st, a, d_o, ldo, lse, (const float*)delta, dk, lddk,
                                                dv, lddv));
    if (drel_partial)
        return launch<t5l_attn_bwd_q_kernel<D, true, true, PK>>(name, dim3(n_slab * a.H), dim3(T5_THREADS), 0, st, a, d_o, ldo, lse, delta, dq, lddq,
                                                            drel_partial, n_slab);
    return launch<t5l_attn_bwd_q_kernel<D, true, false, PK>>(name, dim3(rows * nqb), dim3(T5_THREADS), 0, st, a, d_o, ldo, lse, delta, dq, lddq,
                                                         (float*)nullptr, 0);
}

extern "C" int gamer_t5_attn_long_bwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* rel,
                                      const uint8_t* keep, int B, int Sq, int Sk, int H, int head_dim, int causal, float p_drop,
                                      uint64_t seed, const float* d_o, int ldo, const float* lse, float* dq, int lddq, float* dk, int lddk,
                                      float* dv, int lddv, float* drel_partial, int n_slab, float* row_ws, void* stream) {
    const char* name = "gamer_t5_attn_long_bwd";
    T5Args a;
    GAMER_TRY(t5_args(name, a, q, ldq, k, ldk, v, ldv, rel, keep, B, Sq, Sk, H, head_dim, causal, p_drop, seed, T5L_MAX_S));
    GAMER_CHECK_ARG(d_o && lse && dq && dk && dv && row_ws, "%s: null pointer", name);
    GAMER_CHECK_ARG(ldo >= H * head_dim && lddq >= H * head_dim && lddk >= H * head_dim && lddv >= H * head_dim, "%s: bad leading dims", name);
    GAMER_CHECK_ARG(n_slab > 0 && n_slab <= B, "%s: n_slab=%d (1 .. B: every slab is written by its workgroup)", name, n_slab);
    GAMER_CHECK_ARG(!rel == !drel_partial, "%s: drel_partial goes with the bias", name);
    GAMER_TRY(t5l_grid(name, B, H, ((Sq > Sk ? Sq : Sk) + T5L_QB - 1) / T5L_QB));
    if (head_dim == 64) return t5l_bwd<64, false>(name, a, d_o, ldo, lse, dq, lddq, dk, lddk, dv, lddv, drel_partial, n_slab, row_ws, ST(stream));
    return t5l_bwd<32, false>(name, a, d_o, ldo, lse, dq, lddq, dk, lddk, dv, lddv, drel_partial, n_slab, row_ws, ST(stream));
}

// ---- the packed forms: the grids keep the dense geometry (max_sq, max_sk); blocks past a row's end leave at once ---------------------------
extern "C" int gamer_t5_attn_long_packed_fwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* rel,
                                             const int32_t* q_start, const int32_t* k_start, const int32_t* q_start_host,
                                             const int32_t* k_start_host, const int32_t* kv_rows, int B, int kv_batch, int max_sq,
                                             int max_sk, int H, int head_dim, int causal, float p_drop, uint64_t seed, float* o, int ldo,
                                             float* lse, void* stream) {
    const char* name = "gamer_t5_attn_long_packed_fwd";
    T5Args a;
    GAMER_TRY(t5_packed_args(name, a, q, ldq, k, ldk, v, ldv, rel, q_start, k_start, q_start_host, k_start_host, B, kv_rows ? kv_batch : B,
                             max_sq, max_sk, H, head_dim, causal, p_drop, seed, T5L_MAX_S));
    a.kv_rows = kv_rows;
    GAMER_CHECK_ARG(o && lse && ldo >= H * head_dim, "%s: bad output", name);
    const int nqb = (max_sq + T5L_QB - 1) / T5L_QB;
    GAMER_TRY(t5l_grid(name, B, H, nqb));
    if (head_dim == 64) return launch<t5l_attn_fwd_kernel<64, true>>(name, dim3(B * H * nqb), dim3(T5_THREADS), 0, ST(stream), a, o, ldo, lse);
    return launch<t5l_attn_fwd_kernel<32, true>>(name, dim3(B * H * nqb), dim3(T5_THREADS), 0, ST(stream), a, o, ldo, lse);
}

extern "C" int gamer_t5_attn_long_packed_bwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* rel,
                                             const int32_t* q_start, const int32_t* k_start, const int32_t* q_start_host,
                                             const int32_t* k_start_host, int B, int max_sq, int max_sk, int H, int head_dim, int causal,
                                             float p_drop, uint64_t seed, const float* d_o, int ldo, const float* lse, float* dq, int lddq,
                                             float* dk, int lddk, float* dv, int lddv, float* drel_partial, int n_slab, float* row_ws,
                                             void* stream) {
    const char* name = "gamer_t5_attn_long_packed_bwd";
    T5Args a;
    GAMER_TRY(t5_packed_args(name, a, q, ldq, k, ldk, v, ldv, rel, q_start, k_start, q_start_host, k_start_host, B, B, max_sq, max_sk, H,
                             head_dim, causal, p_drop, seed, T5L_MAX_S));
    GAMER_CHECK_ARG(d_o && lse && dq && dk && dv && row_ws, "%s: null pointer", name);
    GAMER_CHECK_ARG(ldo >= H * head_dim && lddq >= H * head_dim && lddk >= H * head_dim && lddv >= H * head_dim, "%s: bad leading dims", name);
    GAMER_CHECK_ARG(n_slab > 0 && n_slab <= B, "%s: n_slab=%d (1 .. B: every slab is written by its workgroup)", name, n_slab);
    GAMER_CHECK_ARG(!rel == !drel_partial, "%s: drel_partial goes with the bias", name);
    GAMER_TRY(t5l_grid(name, B, H, ((max_sq > max_sk ? max_sq : max_sk) + T5L_QB - 1) / T5L_QB));
    if (head_dim == 64) return t5l_bwd<64, true>(name, a, d_o, ldo, lse, dq, lddq, dk, lddk, dv, lddv, drel_partial, n_slab, row_ws, ST(stream));
    return t5l_bwd<32, true>(name, a, d_o, ldo, lse, dq, lddq, dk, lddk, dv, lddv, drel_partial, n_slab, row_ws, ST(stream));
}
