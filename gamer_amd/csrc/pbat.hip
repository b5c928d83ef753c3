// Fused behaviour-aware attention of PBAT (ref:SeqRec/modules/layers/pbat.py FBAMultiHeadAttention) and the two elementwise halves
// of its Wasserstein head.  Two streams per token: a mean (q1, k1, v1) and a covariance (q2, k2, v2 = ELU(.) + 1).
//
// The reference fuses, for every pair (i, j), three Gaussians on each side (TriSAGP): the token's projection, the relation entry
// R[t_i, t_j] (through Wq1 / Wk1 on the mean side) and the position (through Wq2 / Wk2), and scores the pair with minus the
// Wasserstein distance of the two fused Gaussians.  Its ``key_1[:, :, :, None, :]`` puts the KEY projection on the query axis, so
// both fused Gaussians of (i, j) are built from token i's own projections and the key enters through its type alone:
//     score[i, j] = S[i, t_j],   S [L][b + 1]
// The [B, h, L, L, d] tensors of the reference (four fused, two gathered relation tensors) are never formed: the kernels work on
// S, and the softmax over keys reads S[i, t_j].  One workgroup per (batch row, head); one wave per query row with the head
// dimension across the lanes; plain fp32 (these models are small: d = 32, L = 50 in the shipped config).
//   gamer_pbat_attn_fwd / _bwd    the attention; the forward saves S and the rows' log-sum-exp only; the backward's parameter
//                                 gradients leave as per-workgroup slabs (each written by its one workgroup, no float atomics)
//   gamer_wass_rows_fwd / _bwd    x' = -2 [hm, sqrt(clamp hc)], a = |hm|^2 + sum hc                      (the head's rows)
//   gamer_wass_table_fwd / _bwd   E' = [em, sqrt(clamp ec)], c = |em|^2 + sum ec, ec = ELU(E_c) + 1       (the head's table)
// so that distance(r, v) = a_r + c_v + x'_r . E'_v runs on the biased catalogue kernels with H' = 2 H.
#include "common.h"
#include <cfloat>
#include <algorithm>

namespace gamer {

constexpr int PB_THREADS = 256, PB_WAVES = PB_THREADS / 64;
constexpr int PB_MAX_L = 128, PB_MAX_D = 64, PB_MAX_B = 8, PB_MAX_T = PB_MAX_B + 1;
constexpr float PB_EPS = 1e-24f;                      // the reference's clamp of every covariance

struct PbatArgs {
    const float *q1, *q2, *k1, *k2, *v1, *v2;         // [B*L, ld]: head h at column h*d
    int ld;
    const float *rel_m, *rel_c;                       // [B][(b + 1)^2][H*d]: entry (query type, key type)
    const float *pos_m, *pos_c;                       // [L][H*d]
    const float *wq1, *bq1, *wq2, *bq2, *wk1, *bk1, *wk2, *bk2;      // [d][d], [d]
    const float *uq, *uk;                             // [H][L][d]: Wq2 pos_m + bq2, Wk2 pos_m + bk2 (pbat_pos_kernel)
    const int32_t *types, *keep;                      // [B][L]: type in [0, b]; keep != 0 = a key that may be attended
    int B, L, H, d, nbeh;
    float scale, p_drop;
    uint64_t seed;
};

// ---- the fused Gaussians ---------------------------------------------------------------------------------------------------------
struct PbTri { float u1, u2, u3, cov, N, mean; };
__device__ __forceinline__ PbTri pb_tri(float m1, float m2, float m3, float c1, float c2, float c3) {
    PbTri t;
    t.u1 = 1.f / fmaxf(c1, PB_EPS);
    t.u2 = 1.f / fmaxf(c2, PB_EPS);
    t.u3 = 1.f / fmaxf(c3, PB_EPS);
    t.cov = 1.f / (t.u1 + t.u2 + t.u3);
    t.N = m1 * t.u1 + m2 * t.u2 + m3 * t.u3;
    t.mean = t.cov * t.N;
    return t;
}
// one dimension's share of the distance: (mQ - mK)^2 + cQ + cK - 2 sqrt(clamp cQ) sqrt(clamp cK)
__device__ __forceinline__ float pb_dist(const PbTri& Q, const PbTri& K) {
    const float dm = Q.mean - K.mean;
    const float sq = sqrtf(fmaxf(Q.cov, PB_EPS)), sk = sqrtf(fmaxf(K.cov, PB_EPS));
    const float ds = sq - sk;
    const float cv = (Q.cov >= PB_EPS && K.cov >= PB_EPS) ? ds * ds : Q.cov + K.cov - 2.f * sq * sk;
    return dm * dm + cv;
}
// gradients of one fused Gaussian's inputs from (gm, gc) = d / d(mean, cov); c1 .. c3 are the raw covariances (clamp: no gradient below)
struct PbTriGrad { float m1, m2, m3, c1, c2, c3; };
__device__ __forceinline__ PbTriGrad pb_tri_bwd(const PbTri& t, float m1, float m2, float m3, float c1, float c2, float c3, float gm,
                                                float gc) {
    const float dN = t.cov * gm;
    const float common = -t.cov * t.cov * (gc + t.N * gm);
    PbTriGrad g;
    g.m1 = t.u1 * dN; g.m2 = t.u2 * dN; g.m3 = t.u3 * dN;
    g.c1 = c1 >= PB_EPS ? -t.u1 * t.u1 * (m1 * dN + common) : 0.f;
    g.c2 = c2 >= PB_EPS ? -t.u2 * t.u2 * (m2 * dN + common) : 0.f;
    g.c3 = c3 >= PB_EPS ? -t.u3 * t.u3 * (m3 * dN + common) : 0.f;
    return g;
}

// uq / uk [H][L][d] = W2 pos_m[i][head] + b2: the position's mean through Wq2 / Wk2 (the same for every batch row)
__global__ void __launch_bounds__(PB_THREADS)
pbat_pos_kernel(const float* __restrict__ pos_m, const float* __restrict__ wq2, const float* __restrict__ bq2,
                const float* __restrict__ wk2, const float* __restrict__ bk2, int L, int H, int d, float* __restrict__ uq,
                float* __restrict__ uk) {
    const int e = blockIdx.x * PB_THREADS + threadIdx.x;
    if (e >= H * L * d) return;
    const int c = e % d, i = (e / d) % L, hh = e / (d * L);
    const float* x = pos_m + (int64_t)i * H * d + hh * d;
    float aq = bq2[c], ak = bk2[c];
    for (int k = 0; k < d; ++k) { aq += wq2[c * d + k] * x[k]; ak += wk2[c * d + k] * x[k]; }
    uq[e] = aq;
    uk[e] = ak;
}

// ty[i] = the query's type in [0, b]; tk[j] = the key's slot: its type, or b + 1 for a key that is masked out; returns "no key left"
__device__ __forceinline__ bool pb_types(const PbatArgs& a, int b, int* ty, int* tk, int* nvalid) {
    const int i = threadIdx.x;
    if (i == 0) *nvalid = 0;
    __syncthreads();
    if (i < a.L) {
        const int t = min(max(a.types[(int64_t)b * a.L + i], 0), a.nbeh);
        const bool kp = a.keep[(int64_t)b * a.L + i] != 0;
        ty[i] = t;
        tk[i] = kp ? t : a.nbeh + 1;
        if (kp) atomicAdd(nvalid, 1);
    }
    __syncthreads();
    return *nvalid == 0;
}

// T[p][c] = bias[c] + sum_e W[c][e] rel[p][e] for the (b + 1)^2 relation entries p; wt: [d][d + 1] scratch for W^T
__device__ __forceinline__ void pb_rel_transform(float* __restrict__ T, float* __restrict__ wt, const float* __restrict__ W,
                                                 const float* __restrict__ bias, const float* __restrict__ rel, int ldr, int NP, int d) {
    for (int e = threadIdx.x; e < d * d; e += PB_THREADS) wt[(e % d) * (d + 1) + e / d] = W[e];
    __syncthreads();
    for (int e = threadIdx.x; e < NP * d; e += PB_THREADS) {
        const int p = e / d, c = e % d;
        const float* r = rel + (int64_t)p * ldr;
        float acc = bias[c];
        for (int k = 0; k < d; ++k) acc += wt[k * (d + 1) + c] * r[k];
        T[e] = acc;
    }
    __syncthreads();
}

// what one lane holds of query row i: dimension c of the six inputs of both fused Gaussians that do not depend on the key type
struct PbRow { float q1, q2, k1, k2, uq, uk, pc; };
__device__ __forceinline__ PbRow pb_row(const PbatArgs& a, int b, int hh, int i, int c) {
    const int64_t o = ((int64_t)b * a.L + i) * a.ld + hh * a.d + c;
    const int64_t u = ((int64_t)hh * a.L + i) * a.d + c;
    return PbRow{a.q1[o], a.q2[o], a.k1[o], a.k2[o], a.uq[u], a.uk[u], a.pos_c[(int64_t)i * a.H * a.d + hh * a.d + c]};
}

__device__ __forceinline__ uint64_t pb_drop_index(const PbatArgs& a, int b, int hh, int i, int j) {
    return (((uint64_t)b * a.H + hh) * a.L + i) * a.L + j;
}

__global__ void __launch_bounds__(PB_THREADS)
pbat_attn_fwd_kernel(const PbatArgs a, float* __restrict__ o1, float* __restrict__ o2, int ldo, float* __restrict__ S,
                     float* __restrict__ lse) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int L = a.L, d = a.d, nbeh = a.nbeh, NT = nbeh + 1, NP = NT * NT, HD = a.H * d;
    float* Tq = lds;                          // [NP][d]
    float* Tk = Tq + NP * d;                  // [NP][d]
    float* Rc = Tk + NP * d;                  // [NP][d]
    float* wt = Rc + NP * d;                  // [d][d + 1]
    float* Pt = wt + d * (d + 1);             // [L][NT + 1]: probability of a key of each type; slot NT = masked keys
    int* ty = (int*)(Pt + L * (NT + 1));      // [L]
    int* tk = ty + L;                         // [L]
    int* cnt = tk + L;                        // [16]: valid keys per type; [15] = all of them
    const int b = blockIdx.x / a.H, hh = blockIdx.x % a.H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool allpad = pb_types(a, b, ty, tk, cnt + 15);
    if ((int)threadIdx.x <= nbeh) {
        int n = 0;
        for (int j = 0; j < L; ++j) n += tk[j] == (int)threadIdx.x;
        cnt[threadIdx.x] = n;
    }
    const float* rm = a.rel_m + (int64_t)b * NP * HD + hh * d;
    pb_rel_transform(Tq, wt, a.wq1, a.bq1, rm, HD, NP, d);
    pb_rel_transform(Tk, wt, a.wk1, a.bk1, rm, HD, NP, d);
    for (int e = threadIdx.x; e < NP * d; e += PB_THREADS) Rc[e] = a.rel_c[(int64_t)b * NP * HD + (int64_t)(e / d) * HD + hh * d + e % d];
    __syncthreads();
    const bool act = lane < d;
    const int c = act ? lane : d - 1;
    for (int i = wave; i < L; i += PB_WAVES) {
        const PbRow r = pb_row(a, b, hh, i, c);
        const int p0 = ty[i] * NT;
        float sc[PB_MAX_T];
#pragma unroll
        for (int t = 0; t < PB_MAX_T; ++t) {
            sc[t] = 0.f;
            if (t <= nbeh) {
                const int e = (p0 + t) * d + c;
                const PbTri Q = pb_tri(r.q1, Tq[e], r.uq, r.q2, Rc[e], r.pc);
                const PbTri K = pb_tri(r.k1, Tk[e], r.uk, r.k2, Rc[e], r.pc);
                sc[t] = -wave_sum(act ? pb_dist(Q, K) : 0.f) * a.scale;
            }
        }
        float m = -INFINITY, sum = 0.f;
#pragma unroll
        for (int t = 0; t < PB_MAX_T; ++t)
            if (t <= nbeh && cnt[t] > 0) m = fmaxf(m, sc[t]);
#pragma unroll
        for (int t = 0; t < PB_MAX_T; ++t)
            if (t <= nbeh && cnt[t] > 0) sum += (float)cnt[t] * expf(sc[t] - m);
        const float l = allpad ? 0.f : m + logf(sum);
        if (lane == 0) {
            const int64_t row = ((int64_t)b * a.H + hh) * L + i;
            lse[row] = l;
#pragma unroll
            for (int t = 0; t < PB_MAX_T; ++t)
                if (t <= nbeh) {
                    S[row * NT + t] = sc[t];
                    Pt[i * (NT + 1) + t] = allpad ? 0.f : expf(sc[t] - l);
                }
            Pt[i * (NT + 1) + NT] = allpad ? 1.f / (float)L : 0.f;      // (no key left: the additive mask gives every key 1 / L)
        }
    }
    __syncthreads();
    const DropoutRng rng(a.p_drop, a.seed);
    for (int i = wave; i < L; i += PB_WAVES) {
        float a1 = 0.f, a2 = 0.f;
        for (int j = 0; j < L; ++j) {
            const float p = Pt[i * (NT + 1) + tk[j]];
            if (p == 0.f) continue;
            const float w = p * rng.mult(pb_drop_index(a, b, hh, i, j));
            const int64_t o = ((int64_t)b * L + j) * a.ld + hh * d + c;
            a1 += w * a.v1[o];
            a2 += w * a.v2[o];
        }
        if (act) {
            const int64_t o = ((int64_t)b * L + i) * ldo + hh * d + c;
            o1[o] = a1;
            o2[o] = a2;
        }
    }
}

// slab of one (slot, head): [wq1 d d | bq1 d | wk1 d d | bk1 d | wq2 d d | bq2 d | wk2 d d | bk2 d] in w_part,
// [dpos_m L d | dpos_c L d | dUq L d | dUk L d] in pos_part (dUq / dUk: the gradients of uq / uk summed over the slot's rows,
// folded into wq2 / wk2 / dpos_m when the workgroup has done its rows)
__global__ void __launch_bounds__(PB_THREADS)
pbat_attn_bwd_kernel(const PbatArgs a, const float* __restrict__ S, const float* __restrict__ lse, const float* __restrict__ g1,
                     const float* __restrict__ g2, int ldo,
                     float* __restrict__ dq1, float* __restrict__ dq2, float* __restrict__ dk1, float* __restrict__ dk2,
                     float* __restrict__ dv1, float* __restrict__ dv2, int ldd, float* __restrict__ drel_m, float* __restrict__ drel_c,
                     float* __restrict__ w_part, float* __restrict__ pos_part, int n_partial) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int L = a.L, d = a.d, nbeh = a.nbeh, NT = nbeh + 1, NP = NT * NT, HD = a.H * d;
    const int region = max(3 * NP * d, 2 * L * (d + 1));
    float* Tq = lds;                          // [NP][d]      | v1s [L][d + 1]
    float* Tk = Tq + NP * d;                  // [NP][d]      | v2s [L][d + 1]
    float* Rc = Tk + NP * d;                  // [NP][d]
    float* v1s = lds;
    float* v2s = v1s + L * (d + 1);
    float* dTq = lds + region;                // [NP][d]
    float* dTk = dTq + NP * d;                // [NP][d]
    float* red = dTk + NP * d;                // [PB_WAVES][3 NT][d]   | W^T scratch [d][d + 1]
    float* Pt = red + max(PB_WAVES * 3 * NT * d, d * (d + 1));      // [L][NT + 1]
    float* dS = Pt + L * (NT + 1);            // [L][NT]
    int* ty = (int*)(dS + L * NT);
    int* tk = ty + L;
    int* order = tk + L;                      // query rows sorted by type
    int* toff = order + L;                    // [16]; [15] = valid keys
    const int hh = blockIdx.x % a.H, slot = blockIdx.x / a.H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool act = lane < d;
    const int c = act ? lane : d - 1;
    const DropoutRng rng(a.p_drop, a.seed);
    const int wsz = 4 * (d * d + d);
    float* ws = w_part + ((int64_t)slot * a.H + hh) * wsz;
    float* ps = pos_part + ((int64_t)slot * a.H + hh) * 4 * L * d;
    float* ps_c = ps + L * d;
    float* ps_uq = ps + 2 * L * d;
    float* ps_uk = ps + 3 * L * d;
    for (int b = slot; b < a.B; b += n_partial) {
        const bool allpad = pb_types(a, b, ty, tk, toff + 15);
        if ((int)threadIdx.x == 0) {
            int acc = 0;
            for (int t = 0; t <= nbeh; ++t) {
                toff[t] = acc;
                for (int i = 0; i < L; ++i)
                    if (ty[i] == t) order[acc++] = i;
            }
            toff[nbeh + 1] = acc;
        }
        for (int e = threadIdx.x; e < L * (NT + 1); e += PB_THREADS) {
            const int i = e / (NT + 1), t = e % (NT + 1);
            const int64_t row = ((int64_t)b * a.H + hh) * L + i;
            Pt[e] = t == NT ? (allpad ? 1.f / (float)L : 0.f) : (allpad ? 0.f : expf(S[row * NT + t] - lse[row]));
        }
        for (int e = threadIdx.x; e < L * d; e += PB_THREADS) {
            const int64_t o = ((int64_t)b * L + e / d) * a.ld + hh * d + e % d;
            v1s[(e / d) * (d + 1) + e % d] = a.v1[o];
            v2s[(e / d) * (d + 1) + e % d] = a.v2[o];
        }
        __syncthreads();
        // ---- dS[i][t] = sum over the keys j of type t of p_ij (drop_ij dP_ij - delta_i), delta_i = sum_j p_ij drop_ij dP_ij; lanes over
        //      the keys.  delta comes from the very products it is subtracted from, so a row with one key gets exactly zero --------------
        for (int i = wave; i < L; i += PB_WAVES) {
            const int64_t go = ((int64_t)b * L + i) * ldo + hh * d;
            float pj[2], dp[2];
            int tj[2];
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
                const int j = lane + 64 * h2;
                pj[h2] = dp[h2] = 0.f;
                tj[h2] = -1;
                if (j < L && tk[j] <= nbeh) {
                    float dot = 0.f;
                    for (int k = 0; k < d; ++k) dot += g1[go + k] * v1s[j * (d + 1) + k] + g2[go + k] * v2s[j * (d + 1) + k];
                    tj[h2] = tk[j];
                    pj[h2] = Pt[i * (NT + 1) + tj[h2]];
                    dp[h2] = rng.mult(pb_drop_index(a, b, hh, i, j)) * dot;
                }
            }
            const float delta = wave_sum(pj[0] * dp[0] + pj[1] * dp[1]);
#pragma unroll
            for (int t = 0; t < PB_MAX_T; ++t)
                if (t <= nbeh) {
                    const float s = wave_sum((tj[0] == t ? pj[0] * (dp[0] - delta) : 0.f) + (tj[1] == t ? pj[1] * (dp[1] - delta) : 0.f));
                    if (lane == 0) dS[i * NT + t] = s;
                }
        }
        // ---- dv[j] = sum_i p_ij drop_ij g[i]; one wave per key ------------------------------------------------------------------------
        for (int j = wave; j < L; j += PB_WAVES) {
            float a1 = 0.f, a2 = 0.f;
            for (int i = 0; i < L; ++i) {
                const float p = Pt[i * (NT + 1) + tk[j]];
                if (p == 0.f) continue;
                const float w = p * rng.mult(pb_drop_index(a, b, hh, i, j));
                const int64_t go = ((int64_t)b * L + i) * ldo + hh * d + c;
                a1 += w * g1[go];
                a2 += w * g2[go];
            }
            if (act) {
                const int64_t o = ((int64_t)b * L + j) * ldd + hh * d + c;
                dv1[o] = a1;
                dv2[o] = a2;
            }
        }
        __syncthreads();
        // ---- through the scores: rows of one query type at a time, so that a wave's registers hold the sums of that type's entries ----
        const float* rm = a.rel_m + (int64_t)b * NP * HD + hh * d;
        pb_rel_transform(Tq, red, a.wq1, a.bq1, rm, HD, NP, d);
        pb_rel_transform(Tk, red, a.wk1, a.bk1, rm, HD, NP, d);
        for (int e = threadIdx.x; e < NP * d; e += PB_THREADS) Rc[e] = a.rel_c[(int64_t)b * NP * HD + (int64_t)(e / d) * HD + hh * d + e % d];
        __syncthreads();
        for (int ta = 0; ta <= nbeh; ++ta) {
            float aq[PB_MAX_T], ak[PB_MAX_T], ar[PB_MAX_T];
#pragma unroll
            for (int t = 0; t < PB_MAX_T; ++t) aq[t] = ak[t] = ar[t] = 0.f;
            for (int s = toff[ta] + wave; s < toff[ta + 1]; s += PB_WAVES) {
                const int i = order[s];
                const PbRow r = pb_row(a, b, hh, i, c);
                float gq1 = 0.f, gq2 = 0.f, gk1 = 0.f, gk2 = 0.f, guq = 0.f, guk = 0.f, gpc = 0.f;
#pragma unroll
                for (int t = 0; t < PB_MAX_T; ++t)
                    if (t <= nbeh) {
                        const int e = (ta * NT + t) * d + c;
                        const float tq = Tq[e], tkk = Tk[e], rc = Rc[e];
                        const PbTri Q = pb_tri(r.q1, tq, r.uq, r.q2, rc, r.pc);
                        const PbTri K = pb_tri(r.k1, tkk, r.uk, r.k2, rc, r.pc);
                        const float gw = -a.scale * dS[i * NT + t];                 // d / d(distance)
                        const float sq = sqrtf(fmaxf(Q.cov, PB_EPS)), sk = sqrtf(fmaxf(K.cov, PB_EPS));
                        const float gmq = 2.f * (Q.mean - K.mean) * gw;
                        const float gcq = gw * (Q.cov >= PB_EPS ? 1.f - sk / sq : 1.f);
                        const float gck = gw * (K.cov >= PB_EPS ? 1.f - sq / sk : 1.f);
                        const PbTriGrad GQ = pb_tri_bwd(Q, r.q1, tq, r.uq, r.q2, rc, r.pc, gmq, gcq);
                        const PbTriGrad GK = pb_tri_bwd(K, r.k1, tkk, r.uk, r.k2, rc, r.pc, -gmq, gck);
                        gq1 += GQ.m1; gq2 += GQ.c1; gk1 += GK.m1; gk2 += GK.c1;
                        guq += GQ.m3; guk += GK.m3; gpc += GQ.c3 + GK.c3;
                        aq[t] += GQ.m2; ak[t] += GK.m2; ar[t] += GQ.c2 + GK.c2;
                    }
                if (act) {
                    const int64_t o = ((int64_t)b * L + i) * ldd + hh * d + c;
                    dq1[o] = gq1; dq2[o] = gq2; dk1[o] = gk1; dk2[o] = gk2;
                    ps_c[i * d + c] += gpc;
                    ps_uq[i * d + c] += guq;
                    ps_uk[i * d + c] += guk;
                }
            }
            if (act) {
#pragma unroll
                for (int t = 0; t < PB_MAX_T; ++t)
                    if (t <= nbeh) {
                        red[((wave * 3 + 0) * NT + t) * d + c] = aq[t];
                        red[((wave * 3 + 1) * NT + t) * d + c] = ak[t];
                        red[((wave * 3 + 2) * NT + t) * d + c] = ar[t];
                    }
            }
            __syncthreads();
            for (int e = threadIdx.x; e < 3 * NT * d; e += PB_THREADS) {
                const int which = e / (NT * d), t = (e / d) % NT, cc = e % d;
                float acc = 0.f;
                for (int w = 0; w < PB_WAVES; ++w) acc += red[((w * 3 + which) * NT + t) * d + cc];
                const int p = ta * NT + t;
                if (which == 0) dTq[p * d + cc] = acc;
                else if (which == 1) dTk[p * d + cc] = acc;
                else drel_c[(int64_t)b * NP * HD + (int64_t)p * HD + hh * d + cc] = acc;
            }
            __syncthreads();
        }
        // ---- relation means: dR_m = Wq1^T dTq + Wk1^T dTk; the slabs of Wq1 / Wk1 and their biases ------------------------------------
        for (int e = threadIdx.x; e < NP * d; e += PB_THREADS) {
            const int p = e / d, k = e % d;
            float acc = 0.f;
            for (int cc = 0; cc < d; ++cc) acc += dTq[p * d + cc] * a.wq1[cc * d + k] + dTk[p * d + cc] * a.wk1[cc * d + k];
            drel_m[(int64_t)b * NP * HD + (int64_t)p * HD + hh * d + k] = acc;
        }
        for (int e = threadIdx.x; e < d * d + d; e += PB_THREADS) {
            float sq = 0.f, sk = 0.f;
            if (e < d * d) {
                const int cc = e / d, k = e % d;
                for (int p = 0; p < NP; ++p) { const float x = rm[(int64_t)p * HD + k]; sq += dTq[p * d + cc] * x; sk += dTk[p * d + cc] * x; }
            } else {
                const int cc = e - d * d;
                for (int p = 0; p < NP; ++p) { sq += dTq[p * d + cc]; sk += dTk[p * d + cc]; }
            }
            ws[e] += sq;
            ws[d * d + d + e] += sk;
        }
        __syncthreads();
    }
    // ---- the positions: Wq2 / Wk2, their biases and dpos_m from the slot's summed dUq / dUk -----------------------------------------------
    __threadfence_block();
    __syncthreads();
    for (int e = threadIdx.x; e < d * d + d; e += PB_THREADS) {
        float sq = 0.f, sk = 0.f;
        if (e < d * d) {
            const int cc = e / d, k = e % d;
            for (int i = 0; i < L; ++i) { const float x = a.pos_m[(int64_t)i * HD + hh * d + k]; sq += ps_uq[i * d + cc] * x; sk += ps_uk[i * d + cc] * x; }
        } else {
            const int cc = e - d * d;
            for (int i = 0; i < L; ++i) { sq += ps_uq[i * d + cc]; sk += ps_uk[i * d + cc]; }
        }
        ws[2 * (d * d + d) + e] = sq;
        ws[3 * (d * d + d) + e] = sk;
    }
    for (int e = threadIdx.x; e < L * d; e += PB_THREADS) {
        const int i = e / d, k = e % d;
        float acc = 0.f;
        for (int cc = 0; cc < d; ++cc) acc += ps_uq[i * d + cc] * a.wq2[cc * d + k] + ps_uk[i * d + cc] * a.wk2[cc * d + k];
        ps[e] = acc;
    }
}

// ---- the Wasserstein head's elementwise halves: one wave per row ------------------------------------------------------------------
__device__ __forceinline__ float pb_elu1(float x) { return x > 0.f ? x + 1.f : expf(x); }          // ELU(x) + 1

__global__ void __launch_bounds__(PB_THREADS)
wass_rows_fwd_kernel(const float* __restrict__ hm, const float* __restrict__ hc, int R, int H, float* __restrict__ x, float* __restrict__ ar) {
    const int lane = threadIdx.x & 63;
    const int64_t r = ((int64_t)blockIdx.x * PB_THREADS + threadIdx.x) >> 6;
    if (r >= R) return;
    float acc = 0.f;
    for (int k = lane; k < H; k += 64) {
        const float m = hm[r * H + k], cv = hc[r * H + k];
        x[r * 2 * H + k] = -2.f * m;
        x[r * 2 * H + H + k] = -2.f * sqrtf(fmaxf(cv, PB_EPS));
        acc += m * m + cv;
    }
    acc = wave_sum(acc);
    if (lane == 0) ar[r] = acc;
}

__global__ void __launch_bounds__(PB_THREADS)
wass_rows_bwd_kernel(const float* __restrict__ hm, const float* __restrict__ hc, const float* __restrict__ dx, const float* __restrict__ da,
                     int R, int H, float* __restrict__ dhm, float* __restrict__ dhc) {
    const int64_t e = (int64_t)blockIdx.x * PB_THREADS + threadIdx.x;
    if (e >= (int64_t)R * H) return;
    const int64_t r = e / H;
    const int k = e % H;
    const float g = da ? da[r] : 0.f;
    const float cv = hc[e];
    dhm[e] = -2.f * dx[r * 2 * H + k] + 2.f * hm[e] * g;
    dhc[e] = (cv >= PB_EPS ? -dx[r * 2 * H + H + k] / sqrtf(cv) : 0.f) + g;
}

__global__ void __launch_bounds__(PB_THREADS)
wass_table_fwd_kernel(const float* __restrict__ Em, const float* __restrict__ Ec, int V, int H, float* __restrict__ E2, float* __restrict__ cv) {
    const int lane = threadIdx.x & 63;
    const int64_t v = ((int64_t)blockIdx.x * PB_THREADS + threadIdx.x) >> 6;
    if (v >= V) return;
    float acc = 0.f;
    for (int k = lane; k < H; k += 64) {
        const float m = Em[v * H + k], ec = pb_elu1(Ec[v * H + k]);
        E2[v * 2 * H + k] = m;
        E2[v * 2 * H + H + k] = sqrtf(fmaxf(ec, PB_EPS));
        acc += m * m + ec;
    }
    acc = wave_sum(acc);
    if (lane == 0) cv[v] = acc;
}

__global__ void __launch_bounds__(PB_THREADS)
wass_table_bwd_kernel(const float* __restrict__ Em, const float* __restrict__ Ec, const float* __restrict__ dE2, const float* __restrict__ dc,
                      int V, int H, float* __restrict__ dEm, float* __restrict__ dEc) {
    const int64_t e = (int64_t)blockIdx.x * PB_THREADS + threadIdx.x;
    if (e >= (int64_t)V * H) return;
    const int64_t v = e / H;
    const int k = e % H;
    const float g = dc ? dc[v] : 0.f;
    const float x = Ec[e], ec = pb_elu1(x);
    const float dec = (ec >= PB_EPS ? 0.5f * dE2[v * 2 * H + H + k] / sqrtf(ec) : 0.f) + g;
    dEm[e] = dE2[v * 2 * H + k] + 2.f * Em[e] * g;
    dEc[e] = dec * (x > 0.f ? 1.f : ec);
}

}  // namespace gamer

using namespace gamer;
#define ST(s) ((hipStream_t)(s))

constexpr size_t PB_LDS_MAX = 150 * 1024;      // of the 160 KB per CU

static int pbat_args(const char* name, PbatArgs& a, const float* q1, const float* q2, const float* k1, const float* k2, const float* v1,
                     const float* v2, int ld, const float* rel_m, const float* rel_c, const float* pos_m, const float* pos_c,
                     const float* wq1, const float* bq1, const float* wq2, const float* bq2, const float* wk1, const float* bk1,
                     const float* wk2, const float* bk2, const int32_t* types, const int32_t* keep, int B, int L, int H, int d, int nbeh,
                     float scale, float p_drop, uint64_t seed, float* pos_ws, hipStream_t st) {
    GAMER_CHECK_ARG(q1 && q2 && k1 && k2 && v1 && v2 && rel_m && rel_c && pos_m && pos_c && wq1 && bq1 && wq2 && bq2 && wk1 && bk1 && wk2 &&
                    bk2 && types && keep && pos_ws, "%s: null pointer", name);
    GAMER_CHECK_ARG(B > 0 && L > 0 && L <= PB_MAX_L && H > 0 && d > 0 && d <= PB_MAX_D && d % 4 == 0 && nbeh >= 1 && nbeh <= PB_MAX_B,
                    "%s: bad shape B=%d L=%d H=%d head_dim=%d behaviours=%d (L <= %d, head_dim <= %d and a multiple of 4, behaviours <= %d)",
                    name, B, L, H, d, nbeh, PB_MAX_L, PB_MAX_D, PB_MAX_B);
    GAMER_CHECK_ARG(ld >= H * d, "%s: bad leading dim", name);
    GAMER_CHECK_ARG((int64_t)B * H < (1LL << 31), "%s: B * H too large", name);
    GAMER_CHECK_ARG(p_drop >= 0.f && p_drop < 1.f, "%s: p_drop=%f", name, p_drop);
    a.q1 = q1; a.q2 = q2; a.k1 = k1; a.k2 = k2; a.v1 = v1; a.v2 = v2; a.ld = ld; a.rel_m = rel_m; a.rel_c = rel_c; a.pos_m = pos_m;
    a.pos_c = pos_c; a.wq1 = wq1; a.bq1 = bq1; a.wq2 = wq2; a.bq2 = bq2; a.wk1 = wk1; a.bk1 = bk1; a.wk2 = wk2; a.bk2 = bk2;
    a.uq = pos_ws; a.uk = pos_ws + (int64_t)H * L * d; a.types = types; a.keep = keep; a.B = B; a.L = L; a.H = H; a.d = d; a.nbeh = nbeh;
    a.scale = scale; a.p_drop = p_drop; a.seed = seed;
    const int n = H * L * d;
    return launch<pbat_pos_kernel>(name, dim3((n + PB_THREADS - 1) / PB_THREADS), dim3(PB_THREADS), 0, st, pos_m, wq2, bq2, wk2, bk2, L, H, d,
                                   pos_ws, pos_ws + (int64_t)H * L * d);
}

extern "C" int gamer_pbat_attn_fwd(const float* q1, const float* q2, const float* k1, const float* k2, const float* v1, const float* v2,
                                   int ld, const float* rel_m, const float* rel_c, const float* pos_m, const float* pos_c, const float* wq1,
                                   const float* bq1, const float* wq2, const float* bq2, const float* wk1, const float* bk1,
                                   const float* wk2, const float* bk2, const int32_t* types, const int32_t* keep, int B, int L, int H,
                                   int head_dim, int n_behaviors, float scale, float p_drop, uint64_t seed, float* o1, float* o2, int ldo,
                                   float* S, float* lse, float* pos_ws, void* stream) {
    PbatArgs a;
    GAMER_TRY(pbat_args("gamer_pbat_attn_fwd", a, q1, q2, k1, k2, v1, v2, ld, rel_m, rel_c, pos_m, pos_c, wq1, bq1, wq2, bq2, wk1, bk1, wk2,
                        bk2, types, keep, B, L, H, head_dim, n_behaviors, scale, p_drop, seed, pos_ws, ST(stream)));
    GAMER_CHECK_ARG(o1 && o2 && S && lse && ldo >= H * head_dim, "gamer_pbat_attn_fwd: bad output");
    const int d = head_dim, NT = n_behaviors + 1, NP = NT * NT;
    const size_t shmem = ((size_t)3 * NP * d + (size_t)d * (d + 1) + (size_t)L * (NT + 1) + 2 * L + 16) * sizeof(float);
    GAMER_CHECK_ARG(shmem <= PB_LDS_MAX, "gamer_pbat_attn_fwd: %zu bytes of LDS", shmem);
    return launch<pbat_attn_fwd_kernel>("gamer_pbat_attn_fwd", dim3(B * H), dim3(PB_THREADS), shmem, ST(stream), a, o1, o2, ldo, S, lse);
}

extern "C" int gamer_pbat_attn_bwd(const float* q1, const float* q2, const float* k1, const float* k2, const float* v1, const float* v2,
                                   int ld, const float* rel_m, const float* rel_c, const float* pos_m, const float* pos_c, const float* wq1,
                                   const float* bq1, const float* wq2, const float* bq2, const float* wk1, const float* bk1,
                                   const float* wk2, const float* bk2, const int32_t* types, const int32_t* keep, int B, int L, int H,
                                   int head_dim, int n_behaviors, float scale, float p_drop, uint64_t seed, const float* S, const float* lse,
                                   const float* do1, const float* do2, int ldo, float* dq1, float* dq2,
                                   float* dk1, float* dk2, float* dv1, float* dv2, int ldd, float* drel_m, float* drel_c, float* w_partial,
                                   float* pos_partial, int n_partial, float* pos_ws, void* stream) {
    PbatArgs a;
    GAMER_TRY(pbat_args("gamer_pbat_attn_bwd", a, q1, q2, k1, k2, v1, v2, ld, rel_m, rel_c, pos_m, pos_c, wq1, bq1, wq2, bq2, wk1, bk1, wk2,
                        bk2, types, keep, B, L, H, head_dim, n_behaviors, scale, p_drop, seed, pos_ws, ST(stream)));
    GAMER_CHECK_ARG(S && lse && do1 && do2 && dq1 && dq2 && dk1 && dk2 && dv1 && dv2 && drel_m && drel_c && w_partial &&
                    pos_partial, "gamer_pbat_attn_bwd: null pointer");
    GAMER_CHECK_ARG(ldo >= H * head_dim && ldd >= H * head_dim, "gamer_pbat_attn_bwd: bad leading dims");
    GAMER_CHECK_ARG(n_partial > 0 && n_partial <= B && (int64_t)n_partial * H < (1LL << 31), "gamer_pbat_attn_bwd: n_partial=%d", n_partial);
    const int d = head_dim, NT = n_behaviors + 1, NP = NT * NT;
    const size_t region = std::max((size_t)3 * NP * d, (size_t)2 * L * (d + 1));
    const size_t red = std::max((size_t)PB_WAVES * 3 * NT * d, (size_t)d * (d + 1));
    const size_t shmem = (region + (size_t)2 * NP * d + red + (size_t)L * (NT + 1) + (size_t)L * NT + 4 * L + 16) * sizeof(float);
    GAMER_CHECK_ARG(shmem <= PB_LDS_MAX, "gamer_pbat_attn_bwd: %zu bytes of LDS", shmem);
    return launch<pbat_attn_bwd_kernel>("gamer_pbat_attn_bwd", dim3(n_partial * H), dim3(PB_THREADS), shmem, ST(stream), a, S, lse, do1,
                                        do2, ldo, dq1, dq2, dk1, dk2, dv1, dv2, ldd, drel_m, drel_c, w_partial, pos_partial, n_partial);
}

static int wass_check(const char* name, int R, int H) {
    GAMER_CHECK_ARG(R > 0 && H > 0, "%s: bad shape rows=%d H=%d", name, R, H);
    return 0;
}

extern "C" int gamer_wass_rows_fwd(const float* hm, const float* hc, int R, int H, float* x, float* a, void* stream) {
    GAMER_CHECK_ARG(hm && hc && x && a, "gamer_wass_rows_fwd: null pointer");
    GAMER_TRY(wass_check("gamer_wass_rows_fwd", R, H));
    const int64_t blocks = ((int64_t)R * 64 + PB_THREADS - 1) / PB_THREADS;
    return launch<wass_rows_fwd_kernel>("gamer_wass_rows_fwd", dim3((unsigned)blocks), dim3(PB_THREADS), 0, ST(stream), hm, hc, R, H, x, a);
}

extern "C" int gamer_wass_rows_bwd(const float* hm, const float* hc, const float* dx, const float* da, int R, int H, float* dhm, float* dhc,
                                   void* stream) {
    GAMER_CHECK_ARG(hm && hc && dx && dhm && dhc, "gamer_wass_rows_bwd: null pointer");
    GAMER_TRY(wass_check("gamer_wass_rows_bwd", R, H));
    const int64_t blocks = ((int64_t)R * H + PB_THREADS - 1) / PB_THREADS;
    return launch<wass_rows_bwd_kernel>("gamer_wass_rows_bwd", dim3((unsigned)blocks), dim3(PB_THREADS), 0, ST(stream), hm, hc, dx, da, R, H, dhm,
                                        dhc);
}

extern "C" int gamer_wass_table_fwd(const float* Em, const float* Ec, int V, int H, float* E2, float* c, void* stream) {
    GAMER_CHECK_ARG(Em && Ec && E2 && c, "gamer_wass_table_fwd: null pointer");
    GAMER_TRY(wass_check("gamer_wass_table_fwd", V, H));
    const int64_t blocks = ((int64_t)V * 64 + PB_THREADS - 1) / PB_THREADS;
    return launch<wass_table_fwd_kernel>("gamer_wass_table_fwd", dim3((unsigned)blocks), dim3(PB_THREADS), 0, ST(stream), Em, Ec, V, H, E2, c);
}

extern "C" int gamer_wass_table_bwd(const float* Em, const float* Ec, const float* dE2, const float* dc, int V, int H, float* dEm, float* dEc,
                                    void* stream) {
    GAMER_CHECK_ARG(Em && Ec && dE2 && dEm && dEc, "gamer_wass_table_bwd: null pointer");
    GAMER_TRY(wass_check("gamer_wass_table_bwd", V, H));
    const int64_t blocks = ((int64_t)V * H + PB_THREADS - 1) / PB_THREADS;
    return launch<wass_table_bwd_kernel>("gamer_wass_table_bwd", dim3((unsigned)blocks), dim3(PB_THREADS), 0, ST(stream), Em, Ec, dE2, dc, V, H,
                                         dEm, dEc);
}
