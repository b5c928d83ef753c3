// Behaviour-aware attention of MBSTR (ref:SeqRec/modules/layers/mbs_transformer.py MBSMultiHeadAttention) and the small
// kernels around it.  With b behaviours, C = b b + 1 pair indices c(q, k) = 0 if t_q = 0 or t_k = 0, else (t_q - 1) b + t_k:
//   score[q, k] = Q_q^T W1m[c] K_k * scale + rel[c][bucket(k - q)][head]   (keys of type 0 are masked out)
//   ctx[q, m]   = sum_k dropout(softmax(score))[q, k] sum_n W2m[c][n, m] V_k[n]
// The reference forms [B, h, L, L, C] tensors for both.  Here the C axis is removed by grouping the KEYS by their type tau:
//   score[q, k] = (W1m[c(t_q, tau)]^T Q_q) . K_k          one [L, d] transform of Q per key type present in the row
//   ctx[q]      = sum_tau W2m[c(t_q, tau)]^T-contract (sum_{k of type tau} p[q, k] V_k)
// so the work is that of b dense attentions' operand transforms plus ONE dense attention's products, and nothing of size L^2
// leaves the workgroup.  One workgroup per (batch row, head); probabilities in LDS; plain fp32 FMA products (these models are
// small: d = 32, L = 50 in the shipped config), fp32-exact like the other discriminative kernels.
//   gamer_mbs_mix_fwd / _bwd      W1m, W2m from (W, alpha): Wm[c] = sum_j softmax_j(alpha[c, j, head]) W[j, head]
//   gamer_mbs_attn_fwd / _bwd     the attention; the backward recomputes p from the saved log-sum-exp, and its three parameter
//                                 gradients leave as per-workgroup partial slabs (each added to by its one workgroup, no float atomics)
//   gamer_mbs_bias_fold           relative-offset sums [C][2 L - 1][h] -> bucket table gradient [C][num_buckets][h]
//   gamer_mbs_gate_mix_fwd / _bwd the CGC head's gate softmax and expert mixture per row
#include "common.h"
#include <cfloat>

namespace gamer {

constexpr int MBS_THREADS = 256;
constexpr int MBS_MAX_L = 128, MBS_MAX_D = 64, MBS_MAX_B = 8, MBS_MAX_E = 16;
constexpr int MBS_ACC = MBS_MAX_L * MBS_MAX_D / MBS_THREADS;      // (query, column) elements per thread

struct MbsArgs {
    const float *q, *k, *v;        // [B*L, ld*]: head h at column h*dh
    int ldq, ldk, ldv;
    const int32_t* types;          // [B][L] in [0, nbeh]; 0 = padding
    const float *w1m, *w2m;        // [C][H][dh][dh]
    const float* rel;              // [C][nb][H], or nullptr: no position bias
    const int32_t* bucket;         // [2 L - 1]: bucket of k - q at index k - q + L - 1
    int nb, B, L, H, dh, nbeh, stage;
    float scale, p_drop;
    uint64_t seed;
};

struct MbsTile {
    const float* p;
    int ld;
    __device__ __forceinline__ float at(int r, int d) const { return p[(int64_t)r * ld + d]; }
};
__device__ __forceinline__ MbsTile mbs_tile(const float* g, int ld, int b, int h, int L, int dh, bool stage, float*& lds_top) {
    const float* base = g + (int64_t)b * L * ld + h * dh;
    if (!stage) return MbsTile{base, ld};
    float* dst = lds_top;
    lds_top += L * (dh + 1);
    for (int e = threadIdx.x; e < L * dh; e += MBS_THREADS) dst[(e / dh) * (dh + 1) + e % dh] = base[(int64_t)(e / dh) * ld + e % dh];
    return MbsTile{dst, dh + 1};
}

__device__ __forceinline__ int mbs_pair(int tq, int tk, int nbeh) { return (tq == 0 || tk == 0) ? 0 : (tq - 1) * nbeh + tk; }

// ty[i] = the row's types (clamped to [0, nbeh]); order = positions sorted by type (stable); toff[t] .. toff[t + 1] = type t's range
__device__ __forceinline__ void mbs_lists(const int32_t* __restrict__ types_row, int L, int nbeh, int* ty, int* order, int* toff) {
    __shared__ int cnt[MBS_MAX_B + 1];
    const int i = threadIdx.x;                                  // (L <= MBS_MAX_L < MBS_THREADS: one position per thread)
    if (i < L) ty[i] = min(max(types_row[i], 0), nbeh);
    __syncthreads();
    if (i <= nbeh) {
        int c = 0;
        for (int j = 0; j < L; ++j) c += ty[j] == i;
        cnt[i] = c;
    }
    __syncthreads();
    if (i == 0) {
        int acc = 0;
        for (int t = 0; t <= nbeh; ++t) { toff[t] = acc; acc += cnt[t]; }
        toff[nbeh + 1] = acc;
    }
    __syncthreads();
    if (i < L) {
        const int t = ty[i];
        int rank = 0;
        for (int j = 0; j < i; ++j) rank += ty[j] == t;
        order[toff[t] + rank] = i;
    }
    __syncthreads();
}

// out[q][n] = sum_m X[q][m] Wm[c(t_q, tau)][m][n]   (TRANS: Wm[c][n][m]) for every query q; wm: the head's [C][.][dh][dh] base
template <bool TRANS>
__device__ __forceinline__ void mbs_transform(float* __restrict__ out, const MbsTile& X, const float* __restrict__ wm, int64_t cstride,
                                              const int* ty, int tau, int L, int dh, int nbeh) {
    for (int e = threadIdx.x; e < L * dh; e += MBS_THREADS) {
        const int q = e / dh, n = e % dh;
        const float* w = wm + mbs_pair(ty[q], tau, nbeh) * cstride;
        float acc = 0.f;
        for (int m = 0; m < dh; ++m) acc += X.at(q, m) * (TRANS ? w[n * dh + m] : w[m * dh + n]);
        out[e] = acc;
    }
}

__device__ __forceinline__ float mbs_score(const MbsArgs& a, const float* qt, const MbsTile& K, const int* ty, int hh, int q, int k, int tau) {
    float s = 0.f;
    for (int d = 0; d < a.dh; ++d) s += qt[q * a.dh + d] * K.at(k, d);
    s *= a.scale;
    if (a.rel) {
        const int bk = min(max(a.bucket[k - q + a.L - 1], 0), a.nb - 1);          // (an index outside the table cannot leave it)
        s += a.rel[((int64_t)mbs_pair(ty[q], tau, a.nbeh) * a.nb + bk) * a.H + hh];
    }
    return s;
}

__global__ void __launch_bounds__(MBS_THREADS)
mbs_attn_fwd_kernel(const MbsArgs a, float* __restrict__ o, int ldo, float* __restrict__ lse) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int L = a.L, dh = a.dh, nbeh = a.nbeh;
    float* P = lds;                           // [L][L]
    float* T1 = P + L * L;                    // [L][dh]
    int* ty = (int*)(T1 + L * dh);
    int* order = ty + L;
    int* toff = order + L;                    // [nbeh + 2] (16 reserved)
    float* top = (float*)(toff + 16);
    const int b = blockIdx.x / a.H, hh = blockIdx.x % a.H;
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const DropoutRng rng(a.p_drop, a.seed);
    const int64_t cstride = (int64_t)a.H * dh * dh;
    const float* w1 = a.w1m + (int64_t)hh * dh * dh;
    const float* w2 = a.w2m + (int64_t)hh * dh * dh;
    const MbsTile Q = mbs_tile(a.q, a.ldq, b, hh, L, dh, a.stage, top);
    const MbsTile K = mbs_tile(a.k, a.ldk, b, hh, L, dh, a.stage, top);
    const MbsTile V = mbs_tile(a.v, a.ldv, b, hh, L, dh, a.stage, top);
    mbs_lists(a.types + (int64_t)b * L, L, nbeh, ty, order, toff);
    for (int e = threadIdx.x; e < L * L; e += MBS_THREADS)
        if (ty[e % L] == 0) P[e] = -FLT_MAX;                                     // the additive finfo.min key mask absorbs the score
    for (int tau = 1; tau <= nbeh; ++tau) {
        const int k0 = toff[tau], nk = toff[tau + 1] - k0;
        if (nk == 0) continue;
        mbs_transform<false>(T1, Q, w1, cstride, ty, tau, L, dh, nbeh);
        __syncthreads();
        for (int e = threadIdx.x; e < L * nk; e += MBS_THREADS) {
            const int q = e / nk, k = order[k0 + e % nk];
            P[q * L + k] = mbs_score(a, T1, K, ty, hh, q, k, tau);
        }
        __syncthreads();
    }
    __syncthreads();
    for (int i = wib; i < L; i += MBS_THREADS / 64) {
        float m = -INFINITY;
        for (int j = lane; j < L; j += 64) m = fmaxf(m, P[i * L + j]);
        m = wave_max(m);
        float sum = 0.f;
        for (int j = lane; j < L; j += 64) sum += __expf(P[i * L + j] - m);
        sum = wave_sum(sum);
        const float l = m + __logf(sum);
        for (int j = lane; j < L; j += 64) {
            const float p = __expf(P[i * L + j] - l);
            P[i * L + j] = p * rng.mult((((uint64_t)b * a.H + hh) * L + i) * L + j);
        }
        if (lane == 0) lse[((int64_t)b * a.H + hh) * L + i] = l;
    }
    __syncthreads();
    float acc[MBS_ACC];
#pragma unroll
    for (int i = 0; i < MBS_ACC; ++i) acc[i] = 0.f;
    for (int tau = 1; tau <= nbeh; ++tau) {
        const int k0 = toff[tau], nk = toff[tau + 1] - k0;
        if (nk == 0) continue;
        for (int e = threadIdx.x; e < L * dh; e += MBS_THREADS) {                // U[q][n] = sum over the keys of type tau of p V
            const int q = e / dh, n = e % dh;
            float u = 0.f;
            for (int kk = 0; kk < nk; ++kk) { const int k = order[k0 + kk]; u += P[q * L + k] * V.at(k, n); }
            T1[e] = u;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < MBS_ACC; ++i) {
            const int e = threadIdx.x + i * MBS_THREADS;
            if (e < L * dh) {
                const int q = e / dh, m = e % dh;
                const float* w = w2 + mbs_pair(ty[q], tau, nbeh) * cstride;
                float s = 0.f;
                for (int n = 0; n < dh; ++n) s += w[n * dh + m] * T1[q * dh + n];
                acc[i] += s;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < MBS_ACC; ++i) {
        const int e = threadIdx.x + i * MBS_THREADS;
        if (e < L * dh) o[((int64_t)b * L + e / dh) * ldo + hh * dh + e % dh] = acc[i];
    }
}

// P holds the probability with the SIGN bit as the dropout decision (set = dropped), so one [L][L] array serves both p and
// dropout(p); it is overwritten, key type by key type, with dS.
__device__ __forceinline__ float mbs_pd(float x, float keep_scale) { return (__float_as_uint(x) >> 31) ? 0.f : x * keep_scale; }

__global__ void __launch_bounds__(MBS_THREADS)
mbs_attn_bwd_kernel(const MbsArgs a, const float* __restrict__ o, const float* __restrict__ d_o, int ldo, const float* __restrict__ lse,
                    float* __restrict__ dq, int lddq, float* __restrict__ dk, int lddk, float* __restrict__ dv, int lddv,
                    float* __restrict__ dw1_part, float* __restrict__ dw2_part, float* __restrict__ drel_part, int n_partial) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int L = a.L, dh = a.dh, nbeh = a.nbeh, C = nbeh * nbeh + 1;
    float* P = lds;                           // [L][L]
    float* T1 = P + L * L;                    // [L][dh]
    float* T2 = T1 + L * dh;                  // [L][dh]
    float* delta = T2 + L * dh;               // [L]
    int* ty = (int*)(delta + L);
    int* order = ty + L;
    int* toff = order + L;
    float* const tiles = (float*)(toff + 16);
    const int hh = blockIdx.x % a.H, slot = blockIdx.x / a.H;
    const DropoutRng rng(a.p_drop, a.seed);
    const float keep_scale = rng.scale;
    const int64_t cstride = (int64_t)a.H * dh * dh;
    const float* w1 = a.w1m + (int64_t)hh * dh * dh;
    const float* w2 = a.w2m + (int64_t)hh * dh * dh;
    float* s1 = dw1_part + (int64_t)slot * C * cstride + (int64_t)hh * dh * dh;
    float* s2 = dw2_part + (int64_t)slot * C * cstride + (int64_t)hh * dh * dh;
    float* sr = drel_part ? drel_part + (int64_t)slot * C * (2 * L - 1) * a.H : nullptr;
    for (int b = slot; b < a.B; b += n_partial) {
        float* top = tiles;
        const MbsTile Q = mbs_tile(a.q, a.ldq, b, hh, L, dh, a.stage, top);
        const MbsTile K = mbs_tile(a.k, a.ldk, b, hh, L, dh, a.stage, top);
        const MbsTile V = mbs_tile(a.v, a.ldv, b, hh, L, dh, a.stage, top);
        const MbsTile G = mbs_tile(d_o, ldo, b, hh, L, dh, a.stage, top);
        mbs_lists(a.types + (int64_t)b * L, L, nbeh, ty, order, toff);
        // ---- p from the saved log-sum-exp --------------------------------------------------------------------------------
        for (int e = threadIdx.x; e < L * L; e += MBS_THREADS)
            if (ty[e % L] == 0) P[e] = 0.f;
        for (int i = threadIdx.x; i < L; i += MBS_THREADS) {
            const float* oi = o + ((int64_t)b * L + i) * ldo + hh * dh;
            float acc = 0.f;
            for (int d = 0; d < dh; ++d) acc += oi[d] * G.at(i, d);
            delta[i] = acc;
        }
        for (int tau = 1; tau <= nbeh; ++tau) {
            const int k0 = toff[tau], nk = toff[tau + 1] - k0;
            if (nk == 0) continue;
            mbs_transform<false>(T1, Q, w1, cstride, ty, tau, L, dh, nbeh);
            __syncthreads();
            for (int e = threadIdx.x; e < L * nk; e += MBS_THREADS) {
                const int q = e / nk, k = order[k0 + e % nk];
                const float p = __expf(mbs_score(a, T1, K, ty, hh, q, k, tau) - lse[((int64_t)b * a.H + hh) * L + q]);
                const float mlt = rng.mult((((uint64_t)b * a.H + hh) * L + q) * L + k);
                P[q * L + k] = mlt == 0.f ? -p : p;
            }
            __syncthreads();
        }
        __syncthreads();
        // ---- the value side: dV, dW2m, and dS in place ---------------------------------------------------------------------
        for (int tau = 1; tau <= nbeh; ++tau) {
            const int k0 = toff[tau], nk = toff[tau + 1] - k0;
            if (nk == 0) continue;
            mbs_transform<true>(T1, G, w2, cstride, ty, tau, L, dh, nbeh);      // T1[q][n] = sum_m W2m[c][n][m] dO[q][m]
            for (int e = threadIdx.x; e < L * dh; e += MBS_THREADS) {            // T2 = U[q][n]
                const int q = e / dh, n = e % dh;
                float u = 0.f;
                for (int kk = 0; kk < nk; ++kk) { const int k = order[k0 + kk]; u += mbs_pd(P[q * L + k], keep_scale) * V.at(k, n); }
                T2[e] = u;
            }
            __syncthreads();
            for (int e = threadIdx.x; e < nk * dh; e += MBS_THREADS) {
                const int k = order[k0 + e / dh], n = e % dh;
                float acc = 0.f;
                for (int q = 0; q < L; ++q) acc += mbs_pd(P[q * L + k], keep_scale) * T1[q * dh + n];
                dv[((int64_t)b * L + k) * lddv + hh * dh + n] = acc;
            }
            for (int sg = 0; sg <= nbeh; ++sg) {
                const int q0 = toff[sg], nq = toff[sg + 1] - q0;
                if (nq == 0) continue;
                float* slab = s2 + mbs_pair(sg, tau, nbeh) * cstride;
                for (int e = threadIdx.x; e < dh * dh; e += MBS_THREADS) {
                    const int n = e / dh, m = e % dh;
                    float acc = 0.f;
                    for (int qq = 0; qq < nq; ++qq) { const int q = order[q0 + qq]; acc += T2[q * dh + n] * G.at(q, m); }
                    slab[e] += acc;
                }
            }
            __syncthreads();
            for (int e = threadIdx.x; e < L * nk; e += MBS_THREADS) {
                const int q = e / nk, k = order[k0 + e % nk];
                float dp = 0.f;
                for (int d = 0; d < dh; ++d) dp += T1[q * dh + d] * V.at(k, d);
                const float x = P[q * L + k];
                P[q * L + k] = mbs_pd(x, keep_scale) * dp - fabsf(x) * delta[q];
            }
            __syncthreads();
        }
        // ---- the score side: dK, dQ, dW1m ------------------------------------------------------------------------------------
        float dqa[MBS_ACC];                                                      // (one thread owns (q, m) for every key type)
#pragma unroll
        for (int i = 0; i < MBS_ACC; ++i) dqa[i] = 0.f;
        for (int tau = 1; tau <= nbeh; ++tau) {
            const int k0 = toff[tau], nk = toff[tau + 1] - k0;
            if (nk == 0) continue;
            mbs_transform<false>(T1, Q, w1, cstride, ty, tau, L, dh, nbeh);
            for (int e = threadIdx.x; e < L * dh; e += MBS_THREADS) {            // T2[q][n] = scale sum_{k of tau} dS[q][k] K[k][n]
                const int q = e / dh, n = e % dh;
                float u = 0.f;
                for (int kk = 0; kk < nk; ++kk) { const int k = order[k0 + kk]; u += P[q * L + k] * K.at(k, n); }
                T2[e] = u * a.scale;
            }
            __syncthreads();
            for (int e = threadIdx.x; e < nk * dh; e += MBS_THREADS) {
                const int k = order[k0 + e / dh], n = e % dh;
                float acc = 0.f;
                for (int q = 0; q < L; ++q) acc += P[q * L + k] * T1[q * dh + n];
                dk[((int64_t)b * L + k) * lddk + hh * dh + n] = acc * a.scale;
            }
#pragma unroll
            for (int i = 0; i < MBS_ACC; ++i) {
                const int e = threadIdx.x + i * MBS_THREADS;
                if (e < L * dh) {
                    const int q = e / dh, m = e % dh;
                    const float* w = w1 + mbs_pair(ty[q], tau, nbeh) * cstride + m * dh;
                    float acc = 0.f;
                    for (int n = 0; n < dh; ++n) acc += w[n] * T2[q * dh + n];
                    dqa[i] += acc;
                }
            }
            for (int sg = 0; sg <= nbeh; ++sg) {
                const int q0 = toff[sg], nq = toff[sg + 1] - q0;
                if (nq == 0) continue;
                float* slab = s1 + mbs_pair(sg, tau, nbeh) * cstride;
                for (int e = threadIdx.x; e < dh * dh; e += MBS_THREADS) {
                    const int m = e / dh, n = e % dh;
                    float acc = 0.f;
                    for (int qq = 0; qq < nq; ++qq) { const int q = order[q0 + qq]; acc += Q.at(q, m) * T2[q * dh + n]; }
                    slab[e] += acc;
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < MBS_ACC; ++i) {
            const int e = threadIdx.x + i * MBS_THREADS;
            if (e < L * dh) dq[((int64_t)b * L + e / dh) * lddq + hh * dh + e % dh] = dqa[i];
        }
        // ---- position bias: sums of dS per (pair index, k - q); queries of type 0 meet pair index 0 for every key type ---------
        if (sr) {
            const int R = 2 * L - 1;
            for (int e = threadIdx.x; e < (nbeh * nbeh + 1) * R; e += MBS_THREADS) {
                const int c = e / R, r = e % R - (L - 1);
                const int sg = c == 0 ? 0 : (c - 1) / nbeh + 1, tau = c == 0 ? 0 : (c - 1) % nbeh + 1;
                const int q0 = toff[sg], nq = toff[sg + 1] - q0;
                float acc = 0.f;
                for (int qq = 0; qq < nq; ++qq) {
                    const int q = order[q0 + qq], k = q + r;
                    if (k >= 0 && k < L && (c == 0 ? ty[k] != 0 : ty[k] == tau)) acc += P[q * L + k];
                }
                if (nq) sr[(int64_t)e * a.H + hh] += acc;
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(MBS_THREADS)
mbs_bias_fold_kernel(const float* __restrict__ drel, const int32_t* __restrict__ bucket, int L, int C, int nb, int H,
                     float* __restrict__ dbias) {
    const int i = blockIdx.x * MBS_THREADS + threadIdx.x;
    if (i >= C * nb * H) return;
    const int hh = i % H, bk = (i / H) % nb, c = i / (H * nb);
    const int R = 2 * L - 1;
    float acc = 0.f;
    for (int r = 0; r < R; ++r)
        if (bucket[r] == bk) acc += drel[((int64_t)c * R + r) * H + hh];
    dbias[i] = acc;
}

// ---- W1m / W2m ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void mbs_alpha_softmax(const float* __restrict__ alpha, int c, int hh, int nbeh, int H, float (&s)[MBS_MAX_B]) {
    float m = -INFINITY;
    for (int j = 0; j < nbeh; ++j) m = fmaxf(m, alpha[((int64_t)c * nbeh + j) * H + hh]);
    float sum = 0.f;
    for (int j = 0; j < nbeh; ++j) { s[j] = expf(alpha[((int64_t)c * nbeh + j) * H + hh] - m); sum += s[j]; }
    for (int j = 0; j < nbeh; ++j) s[j] /= sum;
}

__global__ void __launch_bounds__(MBS_THREADS)
mbs_mix_fwd_kernel(const float* __restrict__ W, const float* __restrict__ alpha, int nbeh, int H, int dd, float* __restrict__ Wm) {
    const int64_t i = (int64_t)blockIdx.x * MBS_THREADS + threadIdx.x;
    const int C = nbeh * nbeh + 1;
    if (i >= (int64_t)C * H * dd) return;
    const int mn = i % dd, hh = (i / dd) % H, c = i / ((int64_t)dd * H);
    float s[MBS_MAX_B];
    mbs_alpha_softmax(alpha, c, hh, nbeh, H, s);
    float acc = 0.f;
    for (int j = 0; j < nbeh; ++j) acc += s[j] * W[((int64_t)j * H + hh) * dd + mn];
    Wm[i] = acc;
}

// dW[j][h] = sum_c s[c][j][h] dWm[c][h]   (pair indices in order)
__global__ void __launch_bounds__(MBS_THREADS)
mbs_mix_bwd_w_kernel(const float* __restrict__ alpha, const float* __restrict__ dWm, int nbeh, int H, int dd, float* __restrict__ dW) {
    const int64_t i = (int64_t)blockIdx.x * MBS_THREADS + threadIdx.x;
    const int C = nbeh * nbeh + 1;
    if (i >= (int64_t)nbeh * H * dd) return;
    const int mn = i % dd, hh = (i / dd) % H, j = i / ((int64_t)dd * H);
    float acc = 0.f;
    for (int c = 0; c < C; ++c) {
        float s[MBS_MAX_B];
        mbs_alpha_softmax(alpha, c, hh, nbeh, H, s);
        acc += s[j] * dWm[((int64_t)c * H + hh) * dd + mn];
    }
    dW[i] = acc;
}

// one workgroup per (c, head): ds_j = <dWm[c][h], W[j][h]>, dalpha_j = s_j (ds_j - sum_i s_i ds_i)
__global__ void __launch_bounds__(MBS_THREADS)
mbs_mix_bwd_alpha_kernel(const float* __restrict__ W, const float* __restrict__ alpha, const float* __restrict__ dWm, int nbeh, int H,
                         int dd, float* __restrict__ dalpha) {
    __shared__ float red[MBS_THREADS];
    __shared__ float ds[MBS_MAX_B];
    const int c = blockIdx.x / H, hh = blockIdx.x % H;
    const float* g = dWm + ((int64_t)c * H + hh) * dd;
    for (int j = 0; j < nbeh; ++j) {
        const float* w = W + ((int64_t)j * H + hh) * dd;
        float acc = 0.f;
        for (int e = threadIdx.x; e < dd; e += MBS_THREADS) acc += g[e] * w[e];
        red[threadIdx.x] = acc;
        __syncthreads();
        for (int o = MBS_THREADS / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) ds[j] = red[0];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        float s[MBS_MAX_B];
        mbs_alpha_softmax(alpha, c, hh, nbeh, H, s);
        float dot = 0.f;
        for (int j = 0; j < nbeh; ++j) dot += s[j] * ds[j];
        for (int j = 0; j < nbeh; ++j) dalpha[((int64_t)c * nbeh + j) * H + hh] = s[j] * (ds[j] - dot);
    }
}

// ---- CGC head: gates = softmax(logits[r][0 .. E)), mix[r] = sum_e gates_e outs[r][e]; a row of type 0 gives zeros ---------------------
__global__ void __launch_bounds__(MBS_THREADS)
mbs_gate_mix_fwd_kernel(const float* __restrict__ logits, int ldl, const float* __restrict__ outs, const int32_t* __restrict__ types,
                        int M, int E, int H, float* __restrict__ gates, float* __restrict__ mix) {
    const int lane = threadIdx.x & 63;
    const int r = (blockIdx.x * MBS_THREADS + threadIdx.x) >> 6;
    if (r >= M) return;
    float g[MBS_MAX_E];
    const bool live = types[r] != 0;
    float m = -INFINITY, sum = 0.f;
    for (int e = 0; e < E; ++e) m = fmaxf(m, logits[(int64_t)r * ldl + e]);
    for (int e = 0; e < E; ++e) { g[e] = expf(logits[(int64_t)r * ldl + e] - m); sum += g[e]; }
    for (int e = 0; e < E; ++e) {
        g[e] = live ? g[e] / sum : 0.f;
        if (lane == 0) gates[(int64_t)r * E + e] = g[e];
    }
    for (int col = lane; col < H; col += 64) {
        float acc = 0.f;
        for (int e = 0; e < E; ++e) acc += g[e] * outs[((int64_t)r * E + e) * H + col];
        mix[(int64_t)r * H + col] = live ? acc : 0.f;
    }
}

__global__ void __launch_bounds__(MBS_THREADS)
mbs_gate_mix_bwd_kernel(const float* __restrict__ gates, const float* __restrict__ outs, const float* __restrict__ dmix, int M, int E, int H,
                        float* __restrict__ douts, float* __restrict__ dlogits, int lddl) {
    const int lane = threadIdx.x & 63;
    const int r = (blockIdx.x * MBS_THREADS + threadIdx.x) >> 6;
    if (r >= M) return;
    float g[MBS_MAX_E], dg[MBS_MAX_E];
    for (int e = 0; e < E; ++e) { g[e] = gates[(int64_t)r * E + e]; dg[e] = 0.f; }
    for (int col = lane; col < H; col += 64) {
        const float d = dmix[(int64_t)r * H + col];
        for (int e = 0; e < E; ++e) {
            const int64_t i = ((int64_t)r * E + e) * H + col;
            dg[e] += d * outs[i];
            douts[i] = g[e] * d;
        }
    }
    float dot = 0.f;
    for (int e = 0; e < E; ++e) { dg[e] = wave_sum(dg[e]); dot += g[e] * dg[e]; }
    if (lane == 0)
        for (int e = 0; e < E; ++e) dlogits[(int64_t)r * lddl + e] = g[e] * (dg[e] - dot);
}

}  // namespace gamer

using namespace gamer;
#define ST(s) ((hipStream_t)(s))

constexpr size_t MBS_LDS_MAX = 150 * 1024;      // of the 160 KB per CU

static int mbs_args(const char* name, MbsArgs& a, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                    const int32_t* types, const float* w1m, const float* w2m, const float* rel, const int32_t* bucket, int nb, int B,
                    int L, int H, int dh, int nbeh, float scale, float p_drop, uint64_t seed) {
    GAMER_CHECK_ARG(q && k && v && types && w1m && w2m, "%s: null pointer", name);
    GAMER_CHECK_ARG(B > 0 && L > 0 && L <= MBS_MAX_L && H > 0 && dh > 0 && dh <= MBS_MAX_D && nbeh >= 1 && nbeh <= MBS_MAX_B,
                    "%s: bad shape B=%d L=%d H=%d head_dim=%d behaviours=%d (L <= %d, head_dim <= %d, behaviours <= %d)", name, B, L, H,
                    dh, nbeh, MBS_MAX_L, MBS_MAX_D, MBS_MAX_B);
    GAMER_CHECK_ARG(ldq >= H * dh && ldk >= H * dh && ldv >= H * dh, "%s: bad leading dims", name);
    GAMER_CHECK_ARG(!rel || (bucket && nb > 0), "%s: a bias table needs its bucket index and num_buckets", name);
    GAMER_CHECK_ARG(p_drop >= 0.f && p_drop < 1.f, "%s: p_drop=%f", name, p_drop);
    a.q = q; a.k = k; a.v = v; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.types = types; a.w1m = w1m; a.w2m = w2m;
    a.rel = rel; a.bucket = bucket; a.nb = nb; a.B = B; a.L = L; a.H = H; a.dh = dh; a.nbeh = nbeh; a.stage = 0;
    a.scale = scale; a.p_drop = p_drop; a.seed = seed;
    return 0;
}

extern "C" int gamer_mbs_attn_fwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const int32_t* types,
                                  const float* w1m, const float* w2m, const float* rel, const int32_t* bucket, int num_buckets, int B,
                                  int L, int H, int head_dim, int n_behaviors, float scale, float p_drop, uint64_t seed, float* o,
                                  int ldo, float* lse, void* stream) {
    MbsArgs a;
    int rc = mbs_args("gamer_mbs_attn_fwd", a, q, ldq, k, ldk, v, ldv, types, w1m, w2m, rel, bucket, num_buckets, B, L, H, head_dim,
                      n_behaviors, scale, p_drop, seed);
    if (rc) return rc;
    GAMER_CHECK_ARG(o && lse && ldo >= H * head_dim, "gamer_mbs_attn_fwd: bad output");
    size_t shmem = ((size_t)L * L + (size_t)L * head_dim + 2 * L + 16) * sizeof(float);
    const size_t staged = shmem + (size_t)3 * L * (head_dim + 1) * sizeof(float);
    a.stage = staged <= MBS_LDS_MAX ? 1 : 0;
    if (a.stage) shmem = staged;
    GAMER_TRY(ensure_dynamic_lds<mbs_attn_fwd_kernel>("gamer_mbs_attn_fwd", MBS_LDS_MAX));
    return launch<mbs_attn_fwd_kernel>("gamer_mbs_attn_fwd", dim3(B * H), dim3(MBS_THREADS), shmem, ST(stream), a, o, ldo, lse);
}

extern "C" int gamer_mbs_attn_bwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const int32_t* types,
                                  const float* w1m, const float* w2m, const float* rel, const int32_t* bucket, int num_buckets, int B,
                                  int L, int H, int head_dim, int n_behaviors, float scale, float p_drop, uint64_t seed, const float* o,
                                  const float* d_o, int ldo, const float* lse, float* dq, int lddq, float* dk, int lddk, float* dv,
                                  int lddv, float* dw1m_partial, float* dw2m_partial, float* drel_partial, int n_partial,
                                  void* stream) {
    MbsArgs a;
    int rc = mbs_args("gamer_mbs_attn_bwd", a, q, ldq, k, ldk, v, ldv, types, w1m, w2m, rel, bucket, num_buckets, B, L, H, head_dim,
                      n_behaviors, scale, p_drop, seed);
    if (rc) return rc;
    GAMER_CHECK_ARG(o && d_o && lse && dq && dk && dv && dw1m_partial && dw2m_partial, "gamer_mbs_attn_bwd: null pointer");
    GAMER_CHECK_ARG(ldo >= H * head_dim && lddq >= H * head_dim && lddk >= H * head_dim && lddv >= H * head_dim,
                    "gamer_mbs_attn_bwd: bad leading dims");
    GAMER_CHECK_ARG(n_partial > 0 && (int64_t)n_partial * H < (1LL << 31), "gamer_mbs_attn_bwd: n_partial=%d", n_partial);
    GAMER_CHECK_ARG(!rel == !drel_partial, "gamer_mbs_attn_bwd: drel_partial goes with the bias table");
    size_t shmem = ((size_t)L * L + (size_t)2 * L * head_dim + 3 * L + 16) * sizeof(float);
    const size_t staged = shmem + (size_t)4 * L * (head_dim + 1) * sizeof(float);
    a.stage = staged <= MBS_LDS_MAX ? 1 : 0;
    if (a.stage) shmem = staged;
    GAMER_TRY(ensure_dynamic_lds<mbs_attn_bwd_kernel>("gamer_mbs_attn_bwd", MBS_LDS_MAX));
    return launch<mbs_attn_bwd_kernel>("gamer_mbs_attn_bwd", dim3(n_partial * H), dim3(MBS_THREADS), shmem, ST(stream), a, o, d_o, ldo, lse, dq, lddq,
                                       dk, lddk, dv, lddv, dw1m_partial, dw2m_partial, drel_partial, n_partial);
}

extern "C" int gamer_mbs_bias_fold(const float* drel, const int32_t* bucket, int L, int n_pairs, int num_buckets, int H, float* dbias,
                                   void* stream) {
    GAMER_CHECK_ARG(drel && bucket && dbias && L > 0 && n_pairs > 0 && num_buckets > 0 && H > 0, "gamer_mbs_bias_fold: bad arguments");
    const int n = n_pairs * num_buckets * H;
    hipLaunchKernelGGL(mbs_bias_fold_kernel, dim3((n + MBS_THREADS - 1) / MBS_THREADS), dim3(MBS_THREADS), 0, ST(stream), drel, bucket, L,
                       n_pairs, num_buckets, H, dbias);
    GAMER_CHECK_LAUNCH("gamer_mbs_bias_fold");
    return 0;
}

static int mbs_mix_check(const char* name, int nbeh, int H, int dh) {
    GAMER_CHECK_ARG(nbeh >= 1 && nbeh <= MBS_MAX_B && H > 0 && dh > 0 && dh <= MBS_MAX_D, "%s: bad shape behaviours=%d H=%d head_dim=%d",
                    name, nbeh, H, dh);
    return 0;
}

extern "C" int gamer_mbs_mix_fwd(const float* W, const float* alpha, int n_behaviors, int H, int head_dim, float* Wm, void* stream) {
    GAMER_CHECK_ARG(W && alpha && Wm, "gamer_mbs_mix_fwd: null pointer");
    if (int rc = mbs_mix_check("gamer_mbs_mix_fwd", n_behaviors, H, head_dim)) return rc;
    const int dd = head_dim * head_dim;
    const int64_t n = (int64_t)(n_behaviors * n_behaviors + 1) * H * dd;
    hipLaunchKernelGGL(mbs_mix_fwd_kernel, dim3((unsigned)((n + MBS_THREADS - 1) / MBS_THREADS)), dim3(MBS_THREADS), 0, ST(stream), W,
                       alpha, n_behaviors, H, dd, Wm);
    GAMER_CHECK_LAUNCH("gamer_mbs_mix_fwd");
    return 0;
}

extern "C" int gamer_mbs_mix_bwd(const float* W, const float* alpha, const float* dWm, int n_behaviors, int H, int head_dim, float* dW,
                                 float* dalpha, void* stream) {
    GAMER_CHECK_ARG(W && alpha && dWm && dW && dalpha, "gamer_mbs_mix_bwd: null pointer");
    if (int rc = mbs_mix_check("gamer_mbs_mix_bwd", n_behaviors, H, head_dim)) return rc;
    const int dd = head_dim * head_dim;
    const int64_t n = (int64_t)n_behaviors * H * dd;
    hipLaunchKernelGGL(mbs_mix_bwd_w_kernel, dim3((unsigned)((n + MBS_THREADS - 1) / MBS_THREADS)), dim3(MBS_THREADS), 0, ST(stream), alpha,
                       dWm, n_behaviors, H, dd, dW);
    GAMER_CHECK_LAUNCH("gamer_mbs_mix_bwd/w");
    hipLaunchKernelGGL(mbs_mix_bwd_alpha_kernel, dim3((n_behaviors * n_behaviors + 1) * H), dim3(MBS_THREADS), 0, ST(stream), W, alpha,
                       dWm, n_behaviors, H, dd, dalpha);
    GAMER_CHECK_LAUNCH("gamer_mbs_mix_bwd/alpha");
    return 0;
}

extern "C" int gamer_mbs_gate_mix_fwd(const float* logits, int ldl, const float* outs, const int32_t* types, int M, int E, int H,
                                      float* gates, float* mix, void* stream) {
    GAMER_CHECK_ARG(logits && outs && types && gates && mix, "gamer_mbs_gate_mix_fwd: null pointer");
    GAMER_CHECK_ARG(M > 0 && E > 0 && E <= MBS_MAX_E && H > 0 && ldl >= E, "gamer_mbs_gate_mix_fwd: bad shape M=%d E=%d H=%d (E <= %d)", M, E,
                    H, MBS_MAX_E);
    const int64_t blocks = ((int64_t)M * 64 + MBS_THREADS - 1) / MBS_THREADS;
    hipLaunchKernelGGL(mbs_gate_mix_fwd_kernel, dim3((unsigned)blocks), dim3(MBS_THREADS), 0, ST(stream), logits, ldl, outs, types, M, E, H,
                       gates, mix);
    GAMER_CHECK_LAUNCH("gamer_mbs_gate_mix_fwd");
    return 0;
}

extern "C" int gamer_mbs_gate_mix_bwd(const float* gates, const float* outs, const float* dmix, int M, int E, int H, float* douts,
                                      float* dlogits, int lddl, void* stream) {
    GAMER_CHECK_ARG(gates && outs && dmix && douts && dlogits, "gamer_mbs_gate_mix_bwd: null pointer");
    GAMER_CHECK_ARG(M > 0 && E > 0 && E <= MBS_MAX_E && H > 0 && lddl >= E, "gamer_mbs_gate_mix_bwd: bad shape M=%d E=%d H=%d (E <= %d)", M, E,
                    H, MBS_MAX_E);
    const int64_t blocks = ((int64_t)M * 64 + MBS_THREADS - 1) / MBS_THREADS;
    hipLaunchKernelGGL(mbs_gate_mix_bwd_kernel, dim3((unsigned)blocks), dim3(MBS_THREADS), 0, ST(stream), gates, outs, dmix, M, E, H, douts,
                       dlogits, lddl);
    GAMER_CHECK_LAUNCH("gamer_mbs_gate_mix_bwd");
    return 0;
}
