// MBHT's own kernels (ref:SeqRec/models/discriminative/MBHT/model.py): the two pieces of its multi-scale encoder layer
// (ref:SeqRec/modules/layers/multi_scale_transformer.py) that the plain encoder kernels do not cover, and, further down, the
// hypergraph branch (build, convolution, sliding-window readout, fusion).  DESIGN.md section 10i.
//   gamer_msa_linear_fwd / _bwd   LinearAttention's core.  With keep[l] = item_l > 0 and c = scales[0] projected rows per head:
//                                   Kp[j] = sum_l F[j, l] keep_l K_l + Fb[j],   Vp[j] = sum_l E[j, l] keep_l V_l + Eb[j]   (j < c)
//                                   o_i   = sum_j dropout(softmax_j(scale Q_i . Kp[j])) Vp[j]
//                                 One workgroup per (batch row, head): masking, both sequence-axis projections, scores, softmax,
//                                 dropout and context in one launch; Kp, Vp [c, dh] and the probabilities [L, c] live in LDS only.
//                                 The backward recomputes them from q, k, v and the saved log-sum-exp.
//   gamer_seq_mix_fwd / _bwd      out_fc along the sequence axis, without the two transposes and without the cat:
//                                   Y[b] = W X[b] + bias[:, None],  X[b] = [X0[b]; X1[b]; X2[b]]  ([L0 + L1 + L2, H]), W [Lout, Lin]
// fp32 FMA products (L <= 128, c <= 16: these shapes are tiny), no float atomics: parameter gradients leave as per-workgroup slabs
// (each added to by its one workgroup in a fixed order) for gamer_colsum_reduce, so every result is bit-for-bit repeatable.
#include "common.h"
#include <cfloat>

namespace gamer {

constexpr int MBHT_THREADS = 256;
constexpr int MBHT_MAX_L = 128, MBHT_MAX_D = 64, MBHT_MAX_C = 16, MBHT_MAX_H = 256;
constexpr int MIX_TILE = 64, MIX_LD = MIX_TILE + 1;           // hidden columns per pass; the LDS row stride (odd: no bank conflicts)

struct MsaArgs {
    const float *q, *k, *v;        // [B*L, ld*]: head h at column h*dh
    int ldq, ldk, ldv;
    const int32_t* keep;           // [B][L]: non-zero = a real item
    const float *Ew, *Eb, *Fw, *Fb; // E (values) and F (keys): weight [c][L], bias [c]
    int B, L, H, dh, c;
    float scale, p_drop;
    uint64_t seed;
};

// Kp / Vp [c][dh] of (b, hh) into LDS
__device__ __forceinline__ void msa_project(const MsaArgs& a, int b, int hh, float* __restrict__ Kp, float* __restrict__ Vp) {
    const int L = a.L, dh = a.dh;
    const int32_t* keep = a.keep + (int64_t)b * L;
    for (int e = threadIdx.x; e < a.c * dh; e += MBHT_THREADS) {
        const int j = e / dh, d = e % dh;
        const float* kc = a.k + (int64_t)b * L * a.ldk + hh * dh + d;
        const float* vc = a.v + (int64_t)b * L * a.ldv + hh * dh + d;
        float ka = 0.f, va = 0.f;
        for (int l = 0; l < L; ++l) {
            if (keep[l] == 0) continue;
            ka += a.Fw[j * L + l] * kc[(int64_t)l * a.ldk];
            va += a.Ew[j * L + l] * vc[(int64_t)l * a.ldv];
        }
        Kp[e] = ka + a.Fb[j];
        Vp[e] = va + a.Eb[j];
    }
}

// the scores of query i against the c projected keys, scaled: s[0 .. c)
__device__ __forceinline__ void msa_scores(const MsaArgs& a, const float* __restrict__ qi, const float* __restrict__ Kp,
                                           float (&s)[MBHT_MAX_C]) {
#pragma unroll
    for (int j = 0; j < MBHT_MAX_C; ++j) s[j] = 0.f;
    for (int d = 0; d < a.dh; ++d) {
        const float x = qi[d];
#pragma unroll
        for (int j = 0; j < MBHT_MAX_C; ++j)
            if (j < a.c) s[j] += x * Kp[j * a.dh + d];
    }
#pragma unroll
    for (int j = 0; j < MBHT_MAX_C; ++j) s[j] *= a.scale;
}

__global__ void __launch_bounds__(MBHT_THREADS)
msa_linear_fwd_kernel(const MsaArgs a, float* __restrict__ o, int ldo, float* __restrict__ lse) {
    __shared__ float Kp[MBHT_MAX_C * MBHT_MAX_D], Vp[MBHT_MAX_C * MBHT_MAX_D];
    __shared__ float P[MBHT_MAX_L * MBHT_MAX_C];
    const int L = a.L, dh = a.dh, c = a.c;
    const int b = blockIdx.x / a.H, hh = blockIdx.x % a.H;
    const DropoutRng rng(a.p_drop, a.seed);
    msa_project(a, b, hh, Kp, Vp);
    __syncthreads();
    const int i = threadIdx.x;                                  // (L <= MBHT_MAX_L < MBHT_THREADS: one query per thread)
    if (i < L) {
        float s[MBHT_MAX_C];
        msa_scores(a, a.q + ((int64_t)b * L + i) * a.ldq + hh * dh, Kp, s);
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < MBHT_MAX_C; ++j)
            if (j < c) m = fmaxf(m, s[j]);
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < MBHT_MAX_C; ++j)
            if (j < c) sum += expf(s[j] - m);
        const float l = m + logf(sum);
        const uint64_t base = (((uint64_t)b * a.H + hh) * L + i) * c;
#pragma unroll
        for (int j = 0; j < MBHT_MAX_C; ++j)
            if (j < c) P[i * c + j] = expf(s[j] - l) * rng.mult(base + j);
        lse[((int64_t)b * a.H + hh) * L + i] = l;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < L * dh; e += MBHT_THREADS) {
        const int q = e / dh, d = e % dh;
        float acc = 0.f;
        for (int j = 0; j < c; ++j) acc += P[q * c + j] * Vp[j * dh + d];
        o[((int64_t)b * L + q) * ldo + hh * dh + d] = acc;
    }
}

// One workgroup walks the (row, head) pairs blockIdx.x, blockIdx.x + gridDim.x, ... in order and adds their parameter sums into its
// own slab: [dEw c L | dFw c L | dEb c | dFb c].
__global__ void __launch_bounds__(MBHT_THREADS)
msa_linear_bwd_kernel(const MsaArgs a, const float* __restrict__ d_o, int ldo, const float* __restrict__ lse, float* __restrict__ dq,
                      int lddq, float* __restrict__ dk, int lddk, float* __restrict__ dv, int lddv, float* __restrict__ partial) {
    __shared__ float Kp[MBHT_MAX_C * MBHT_MAX_D], Vp[MBHT_MAX_C * MBHT_MAX_D];
    __shared__ float dKp[MBHT_MAX_C * MBHT_MAX_D], dVp[MBHT_MAX_C * MBHT_MAX_D];
    __shared__ float PD[MBHT_MAX_L * MBHT_MAX_C], DS[MBHT_MAX_L * MBHT_MAX_C];     // dropout(p) and dS (scaled)
    const int L = a.L, dh = a.dh, c = a.c;
    const DropoutRng rng(a.p_drop, a.seed);
    float* slab = partial + (int64_t)blockIdx.x * (2 * c * L + 2 * c);
    for (int pair = blockIdx.x; pair < a.B * a.H; pair += gridDim.x) {
        const int b = pair / a.H, hh = pair % a.H;
        const int32_t* keep = a.keep + (int64_t)b * L;
        msa_project(a, b, hh, Kp, Vp);
        __syncthreads();
        const int i = threadIdx.x;
        if (i < L) {
            float s[MBHT_MAX_C], dp[MBHT_MAX_C];
            msa_scores(a, a.q + ((int64_t)b * L + i) * a.ldq + hh * dh, Kp, s);
            const float l = lse[((int64_t)b * a.H + hh) * L + i];
            const float* gi = d_o + ((int64_t)b * L + i) * ldo + hh * dh;
#pragma unroll
            for (int j = 0; j < MBHT_MAX_C; ++j) dp[j] = 0.f;
            for (int d = 0; d < dh; ++d) {
                const float g = gi[d];
#pragma unroll
                for (int j = 0; j < MBHT_MAX_C; ++j)
                    if (j < c) dp[j] += g * Vp[j * dh + d];
            }
            const uint64_t base = (((uint64_t)b * a.H + hh) * L + i) * c;
            float delta = 0.f;
#pragma unroll
            for (int j = 0; j < MBHT_MAX_C; ++j)
                if (j < c) {
                    const float mlt = rng.mult(base + j);
                    s[j] = expf(s[j] - l);                      // p
                    dp[j] *= mlt;                               // d p
                    PD[i * c + j] = s[j] * mlt;
                    delta += dp[j] * s[j];
                }
#pragma unroll
            for (int j = 0; j < MBHT_MAX_C; ++j)
                if (j < c) DS[i * c + j] = s[j] * (dp[j] - delta) * a.scale;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < L * dh; e += MBHT_THREADS) {               // dQ
            const int q = e / dh, d = e % dh;
            float acc = 0.f;
            for (int j = 0; j < c; ++j) acc += DS[q * c + j] * Kp[j * dh + d];
            dq[((int64_t)b * L + q) * lddq + hh * dh + d] = acc;
        }
        for (int e = threadIdx.x; e < c * dh; e += MBHT_THREADS) {               // dKp, dVp
            const int j = e / dh, d = e % dh;
            const float* qc = a.q + (int64_t)b * L * a.ldq + hh * dh + d;
            const float* gc = d_o + (int64_t)b * L * ldo + hh * dh + d;
            float ka = 0.f, va = 0.f;
            for (int q = 0; q < L; ++q) {
                ka += DS[q * c + j] * qc[(int64_t)q * a.ldq];
                va += PD[q * c + j] * gc[(int64_t)q * ldo];
            }
            dKp[e] = ka;
            dVp[e] = va;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < L * dh; e += MBHT_THREADS) {               // dK, dV (zero on padding)
            const int l = e / dh, d = e % dh;
            float ka = 0.f, va = 0.f;
            if (keep[l] != 0)
                for (int j = 0; j < c; ++j) {
                    ka += a.Fw[j * L + l] * dKp[j * dh + d];
                    va += a.Ew[j * L + l] * dVp[j * dh + d];
                }
            dk[((int64_t)b * L + l) * lddk + hh * dh + d] = ka;
            dv[((int64_t)b * L + l) * lddv + hh * dh + d] = va;
        }
        for (int e = threadIdx.x; e < c * L; e += MBHT_THREADS) {                // dE, dF
            const int j = e / L, l = e % L;
            if (keep[l] == 0) continue;
            const float* kr = a.k + ((int64_t)b * L + l) * a.ldk + hh * dh;
            const float* vr = a.v + ((int64_t)b * L + l) * a.ldv + hh * dh;
            float ea = 0.f, fa = 0.f;
            for (int d = 0; d < dh; ++d) {
                ea += dVp[j * dh + d] * vr[d];
                fa += dKp[j * dh + d] * kr[d];
            }
            slab[e] += ea;
            slab[c * L + e] += fa;
        }
        if ((int)threadIdx.x < c) {
            const int j = threadIdx.x;
            float ea = 0.f, fa = 0.f;
            for (int d = 0; d < dh; ++d) { ea += dVp[j * dh + d]; fa += dKp[j * dh + d]; }
            slab[2 * c * L + j] += ea;
            slab[2 * c * L + c + j] += fa;
        }
        __syncthreads();
    }
}

// ---- out_fc along the sequence axis ----------------------------------------------------------------------------------------------
struct MixSrc {
    const float* x[3];             // X0 [B][L0][H], X1 [B][L1][H], X2 [B][L2][H]
    int len[3];
};

// row i of the concatenation: its source pointer for batch row b (nullptr past the end)
template <typename T>
__device__ __forceinline__ T* mix_row(T* const (&x)[3], const int (&len)[3], int b, int i, int H) {
    int s = 0;
    if (i >= len[0]) { i -= len[0]; s = 1; }
    if (s == 1 && i >= len[1]) { i -= len[1]; s = 2; }
    return x[s] + ((int64_t)b * len[s] + i) * H;
}

// tile [rows][MIX_LD] <- columns [h0, h0 + MIX_TILE) of the rows (zero past H)
__device__ __forceinline__ void mix_stage_x(float* __restrict__ tile, const MixSrc& s, int b, int Lin, int H, int h0) {
    for (int e = threadIdx.x; e < Lin * MIX_TILE; e += MBHT_THREADS) {
        const int i = e / MIX_TILE, hc = e % MIX_TILE;
        tile[i * MIX_LD + hc] = h0 + hc < H ? mix_row(s.x, s.len, b, i, H)[h0 + hc] : 0.f;
    }
}

__global__ void __launch_bounds__(MBHT_THREADS)
seq_mix_fwd_kernel(const MixSrc s, const float* __restrict__ W, const float* __restrict__ bias, int H, int Lout, float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int Lin = s.len[0] + s.len[1] + s.len[2];
    const int b = blockIdx.x, h0 = blockIdx.y * MIX_TILE;
    mix_stage_x(lds, s, b, Lin, H, h0);
    __syncthreads();
    for (int e = threadIdx.x; e < Lout * MIX_TILE; e += MBHT_THREADS) {
        const int r = e / MIX_TILE, hc = e % MIX_TILE;
        if (h0 + hc >= H) continue;
        const float* w = W + (int64_t)r * Lin;
        float acc = 0.f;
        for (int i = 0; i < Lin; ++i) acc += w[i] * lds[i * MIX_LD + hc];
        y[((int64_t)b * Lout + r) * H + h0 + hc] = acc + bias[r];
    }
}

// One workgroup walks the rows blockIdx.x, blockIdx.x + gridDim.x, ... and every column tile of each in order, adding into its own
// slab [dW Lout Lin | dbias Lout].
__global__ void __launch_bounds__(MBHT_THREADS)
seq_mix_bwd_kernel(const MixSrc s, const float* __restrict__ W, const float* __restrict__ dy, int B, int H, int Lout,
                   float* __restrict__ dx0, float* __restrict__ dx1, float* __restrict__ dx2, float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int Lin = s.len[0] + s.len[1] + s.len[2];
    float* X = lds;                           // [Lin][MIX_LD]
    float* G = X + Lin * MIX_LD;              // [Lout][MIX_LD]
    float* const dx[3] = {dx0, dx1, dx2};
    float* slab = partial + (int64_t)blockIdx.x * ((int64_t)Lout * Lin + Lout);
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        for (int h0 = 0; h0 < H; h0 += MIX_TILE) {
            mix_stage_x(X, s, b, Lin, H, h0);
            for (int e = threadIdx.x; e < Lout * MIX_TILE; e += MBHT_THREADS) {
                const int r = e / MIX_TILE, hc = e % MIX_TILE;
                G[r * MIX_LD + hc] = h0 + hc < H ? dy[((int64_t)b * Lout + r) * H + h0 + hc] : 0.f;
            }
            __syncthreads();
            for (int e = threadIdx.x; e < Lin * MIX_TILE; e += MBHT_THREADS) {   // dX = W^T dY
                const int i = e / MIX_TILE, hc = e % MIX_TILE;
                if (h0 + hc >= H) continue;
                float acc = 0.f;
                for (int r = 0; r < Lout; ++r) acc += W[(int64_t)r * Lin + i] * G[r * MIX_LD + hc];
                mix_row(dx, s.len, b, i, H)[h0 + hc] = acc;
            }
            for (int e = threadIdx.x; e < Lout * Lin; e += MBHT_THREADS) {       // dW += dY X^T
                const int r = e / Lin, i = e % Lin;
                float acc = 0.f;
                for (int hc = 0; hc < MIX_TILE; ++hc) acc += G[r * MIX_LD + hc] * X[i * MIX_LD + hc];
                slab[e] += acc;
            }
            for (int r = threadIdx.x; r < Lout; r += MBHT_THREADS) {
                float acc = 0.f;
                for (int hc = 0; hc < MIX_TILE; ++hc) acc += G[r * MIX_LD + hc];
                slab[(int64_t)Lout * Lin + r] += acc;
            }
            __syncthreads();
        }
    }
}

// ---- the hypergraph branch ---------------------------------------------------------------------------------------------------------
// One row's hypergraph (ref:SeqRec/models/discriminative/MBHT/model.py build_Gs_unique) never exists as a dense incidence matrix: a
// row of H has at most hyper_len + 2 non-zeros (its self-loop, its multi-behaviour edge, its selected neighbours' items), so H is kept
// as (edge, value) lists per position in LDS.  An edge is named by its token; the multi-behaviour edge of an item carries HG_MULTI.
constexpr int HG_MAX_K = 8, HG_ENT = HG_MAX_K + 2, HG_DC = 32, HG_XLD = HG_DC + 1;
constexpr int HG_MULTI = 0x40000000;

struct HgLists {
    int* it;        // [L] the row's tokens
    int* nent;      // [L] entries of each position
    int* tok;       // [L][HG_ENT]
    float* val;     // [L][HG_ENT]
    float* de;      // [L][HG_ENT] the degree of the entry's edge
    float* dv;      // [L] the degree of the position
    float* cinv;    // [MBHT_MAX_H] 1 / max(|column d of x_m over all L positions|, 1e-12)
};

__device__ __forceinline__ int hg_find(const HgLists& h, int i, int tk) {
    for (int s = 0; s < h.nent[i]; ++s)
        if (h.tok[i * HG_ENT + s] == tk) return s;
    return -1;
}

// it[], n (returned), cinv[]: the reference's F.normalize(x_m) runs along dim 1 of [B, l, H], the SEQUENCE axis, so every hidden
// column is scaled by its norm over the l positions of the row, padding included
__device__ __forceinline__ int hg_prepare(const HgLists& h, const float* __restrict__ xm, const int32_t* __restrict__ items, int L, int H) {
    __shared__ int n_sh;
    for (int i = threadIdx.x; i < L; i += MBHT_THREADS) h.it[i] = items[i];
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int i = 0; i < L; ++i) n += h.it[i] != 0;
        n_sh = n;
    }
    __syncthreads();
    const int n = n_sh;
    for (int d = threadIdx.x; d < H; d += MBHT_THREADS) {
        float ss = 0.f;
        for (int l = 0; l < L; ++l) { const float x = xm[(int64_t)l * H + d]; ss += x * x; }
        h.cinv[d] = 1.f / fmaxf(sqrtf(ss), 1e-12f);
    }
    __syncthreads();
    return n;
}

// The entries of position i from its selected key positions js[0 .. k) with values vs[]: slot[t] = the entry the selection t wrote
// (-1: none - a <MASK> key (replaced by the position's own item at 1.0), the position's own item (the self-loop overwrites it), or
// an item an earlier selection already wrote: the values are equal).
__device__ __forceinline__ void hg_row_entries(const HgLists& h, int i, int n, int mask_token, const int* js, const float* vs, int k,
                                               int* slot) {
    const int me = h.it[i];
    int* tok = h.tok + i * HG_ENT;
    float* val = h.val + i * HG_ENT;
    int ne = 0;
    tok[ne] = me; val[ne] = 1.f; ++ne;                                           // the self-loop (every <MASK> shares one edge)
    if (me != mask_token) {
        int occ = 0;
        for (int j = 0; j < n; ++j) occ += h.it[j] == me;
        if (occ > 1) { tok[ne] = me | HG_MULTI; val[ne] = 1.f; ++ne; }           // the item's multi-behaviour edge
        for (int t = 0; t < k; ++t) {
            slot[t] = -1;
            const int j = js[t];
            if (j < 0) continue;
            const int tk = h.it[j];
            if (tk == mask_token || tk == me) continue;
            bool seen = false;
            for (int s = 0; s < ne; ++s) seen |= tok[s] == tk;
            if (seen) {                                                          // the same item again: the gradient goes to both
                for (int s = 0; s < ne; ++s)
                    if (tok[s] == tk) slot[t] = s;
                continue;
            }
            tok[ne] = tk; val[ne] = vs[t]; slot[t] = ne; ++ne;
        }
    } else {
        for (int t = 0; t < k; ++t) slot[t] = -1;
    }
    h.nent[i] = ne;
}

// de[][] and dv[] from the lists
__device__ __forceinline__ void hg_degrees(const HgLists& h, int n) {
    for (int e = threadIdx.x; e < n * HG_ENT; e += MBHT_THREADS) {
        const int i = e / HG_ENT, s = e % HG_ENT;
        if (s >= h.nent[i]) continue;
        const int tk = h.tok[e];
        float acc = 0.f;
        for (int r = 0; r < n; ++r) {
            const int sr = hg_find(h, r, tk);
            if (sr >= 0) acc += h.val[r * HG_ENT + sr];
        }
        h.de[e] = acc;
    }
    for (int i = threadIdx.x; i < n; i += MBHT_THREADS) {
        float acc = 0.f;
        for (int s = 0; s < h.nent[i]; ++s) acc += h.val[i * HG_ENT + s];
        h.dv[i] = acc;
    }
}

__device__ __forceinline__ HgLists hg_carve(float*& top, int L) {
    HgLists h;
    h.it = (int*)top; top += L;
    h.nent = (int*)top; top += L;
    h.tok = (int*)top; top += L * HG_ENT;
    h.val = top; top += L * HG_ENT;
    h.de = top; top += L * HG_ENT;
    h.dv = top; top += L;
    h.cinv = top; top += MBHT_MAX_H;
    return h;
}
static inline size_t hg_lists_floats(int L) { return (size_t)L * (3 + 3 * HG_ENT) + MBHT_MAX_H; }

// Xs [n][HG_XLD] <- columns [d0, d0 + HG_DC) of the scaled rows u = x_m cinv (zero past H)
__device__ __forceinline__ void hg_stage_unit(float* __restrict__ Xs, const HgLists& h, const float* __restrict__ xm, int n, int H, int d0) {
    for (int e = threadIdx.x; e < n * HG_DC; e += MBHT_THREADS) {
        const int i = e / HG_DC, dd = e % HG_DC;
        Xs[i * HG_XLD + dd] = d0 + dd < H ? xm[(int64_t)i * H + d0 + dd] * h.cinv[d0 + dd] : 0.f;
    }
}

__global__ void __launch_bounds__(MBHT_THREADS)
hg_build_fwd_kernel(const float* __restrict__ xm_all, const int32_t* __restrict__ items_all, int L, int H, int K, int mask_token,
                    float* __restrict__ G_all, int32_t* __restrict__ sel_all) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.x, SLD = L | 1;
    float* top = lds;
    HgLists h = hg_carve(top, L);
    float* S = top; top += L * SLD;
    float* Xs = top;
    const float* xm = xm_all + (int64_t)b * L * H;
    float* G = G_all + (int64_t)b * L * L;
    int32_t* sel = sel_all + (int64_t)b * L * K;
    const int n = hg_prepare(h, xm, items_all + (int64_t)b * L, L, H);
    // similarities u u^T, HG_DC columns at a time; negative ones become the constant 0.01
    for (int d0 = 0; d0 < H; d0 += HG_DC) {
        hg_stage_unit(Xs, h, xm, n, H, d0);
        __syncthreads();
        for (int e = threadIdx.x; e < n * n; e += MBHT_THREADS) {
            const int i = e / n, j = e % n;
            float acc = d0 == 0 ? 0.f : S[i * SLD + j];
            for (int dd = 0; dd < HG_DC; ++dd) acc += Xs[i * HG_XLD + dd] * Xs[j * HG_XLD + dd];
            if (d0 + HG_DC >= H && acc < 0.f) acc = 0.01f;
            S[i * SLD + j] = acc;
        }
        __syncthreads();
    }
    // top-k of every live row that is no <MASK> (the lower key position wins among equal values), then its entries
    const int k = min(K, n);
    for (int i = threadIdx.x; i < L; i += MBHT_THREADS) {
        int js[HG_MAX_K], slot[HG_MAX_K];
        float vs[HG_MAX_K];
        int kk = 0;
        if (i < n && h.it[i] != mask_token) {
            for (int t = 0; t < k; ++t) {
                int best = -1;
                float bv = -INFINITY;
                for (int j = 0; j < n; ++j) {
                    bool taken = false;
                    for (int u = 0; u < t; ++u) taken |= js[u] == j;
                    const float v = S[i * SLD + j];
                    if (!taken && v > bv) { bv = v; best = j; }
                }
                js[t] = best;
                vs[t] = bv;
            }
            kk = k;
        }
        for (int t = 0; t < K; ++t) sel[i * K + t] = t < kk ? js[t] : -1;
        if (i < n) hg_row_entries(h, i, n, mask_token, js, vs, kk, slot);
    }
    __syncthreads();
    hg_degrees(h, n);
    __syncthreads();
    // G = Dv^-1 H De^-1 H^T on the live block, zero outside
    for (int e = threadIdx.x; e < L * L; e += MBHT_THREADS) {
        const int i = e / L, r = e % L;
        float acc = 0.f;
        if (i < n && r < n) {
            for (int s = 0; s < h.nent[i]; ++s) {
                const int sr = hg_find(h, r, h.tok[i * HG_ENT + s]);
                if (sr >= 0) acc += h.val[i * HG_ENT + s] * h.val[r * HG_ENT + sr] / h.de[i * HG_ENT + s];
            }
            acc /= h.dv[i];
        }
        G[e] = acc;
    }
}

// dG -> dx_m along the forward's own selection.  With A = H De^-1 H^T, G = Dv^-1 A, g = dG / Dv (rows) and S = g + g^T:
//   T[i, e]  = sum_r S[i, r] H[r, e]
//   dH[i, e] = T[i, e] / De_e - (1 / 2 De_e^2) sum_r H[r, e] T[r, e] - (1 / Dv_i) sum_r dG[i, r] G[i, r]
// A selection passes dH of its entry on to its similarity (every selection of a repeated item passes the full value on, as the
// reference's indexed assignment differentiates); self-loops, replaced <MASK> keys and clamped values pass nothing.
__global__ void __launch_bounds__(MBHT_THREADS)
hg_build_bwd_kernel(const float* __restrict__ xm_all, const int32_t* __restrict__ items_all, const int32_t* __restrict__ sel_all,
                    const float* __restrict__ G_all, const float* __restrict__ dG_all, int L, int H, int K, int mask_token,
                    float* __restrict__ dxm_all) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.x, SLD = L | 1;
    float* top = lds;
    HgLists h = hg_carve(top, L);
    float* S = top; top += L * SLD;
    float* Xs = top; top += L * HG_XLD;
    float* tt = top; top += L * HG_ENT;
    float* dh = top; top += L * HG_ENT;
    float* ddv = top; top += L;
    float* cdot = top; top += MBHT_MAX_H;
    float* sv = top; top += L * HG_MAX_K;
    int* slot = (int*)top; top += L * HG_MAX_K;
    int* live = (int*)top;                     // [L][HG_MAX_K]: the selection passes a gradient on
    const float* xm = xm_all + (int64_t)b * L * H;
    const int32_t* sel = sel_all + (int64_t)b * L * K;
    const float* G = G_all + (int64_t)b * L * L;
    const float* dG = dG_all + (int64_t)b * L * L;
    float* dxm = dxm_all + (int64_t)b * L * H;
    const int n = hg_prepare(h, xm, items_all + (int64_t)b * L, L, H);
    // the similarities of the selected pairs
    for (int e = threadIdx.x; e < n * K; e += MBHT_THREADS) {
        const int i = e / K, t = e % K, j = sel[e];
        float v = 0.f;
        int lv = 0;
        if (j >= 0 && j < n) {
            for (int d = 0; d < H; ++d) v += (xm[(int64_t)i * H + d] * h.cinv[d]) * (xm[(int64_t)j * H + d] * h.cinv[d]);
            lv = v >= 0.f;
            if (v < 0.f) v = 0.01f;
        }
        sv[i * HG_MAX_K + t] = v;
        live[i * HG_MAX_K + t] = lv;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += MBHT_THREADS) {
        int js[HG_MAX_K], sl[HG_MAX_K];
        float vs[HG_MAX_K];
        for (int t = 0; t < K; ++t) { const int j = sel[i * K + t]; js[t] = j < n ? j : -1; vs[t] = sv[i * HG_MAX_K + t]; }
        hg_row_entries(h, i, n, mask_token, js, vs, K, sl);
        for (int t = 0; t < K; ++t) slot[i * HG_MAX_K + t] = sl[t];
    }
    __syncthreads();
    hg_degrees(h, n);
    for (int e = threadIdx.x; e < n * n; e += MBHT_THREADS) S[(e / n) * SLD + e % n] = dG[(e / n) * L + e % n];
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += MBHT_THREADS) {
        float acc = 0.f;
        for (int r = 0; r < n; ++r) acc += S[i * SLD + r] * G[i * L + r];
        ddv[i] = -acc / h.dv[i];
    }
    for (int e = threadIdx.x; e < n * HG_ENT; e += MBHT_THREADS) {
        const int i = e / HG_ENT, s = e % HG_ENT;
        if (s >= h.nent[i]) continue;
        const int tk = h.tok[e];
        float acc = 0.f;
        for (int r = 0; r < n; ++r) {
            const int sr = hg_find(h, r, tk);
            if (sr >= 0) acc += (S[i * SLD + r] / h.dv[i] + S[r * SLD + i] / h.dv[r]) * h.val[r * HG_ENT + sr];
        }
        tt[e] = acc;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < n * HG_ENT; e += MBHT_THREADS) {
        const int i = e / HG_ENT, s = e % HG_ENT;
        if (s >= h.nent[i]) continue;
        const int tk = h.tok[e];
        float acc = 0.f;
        for (int r = 0; r < n; ++r) {
            const int sr = hg_find(h, r, tk);
            if (sr >= 0) acc += h.val[r * HG_ENT + sr] * tt[r * HG_ENT + sr];
        }
        const float de = h.de[e];
        dh[e] = tt[e] / de - 0.5f * acc / (de * de) + ddv[i];
    }
    __syncthreads();
    // dS: the gradient of every similarity that reached H, as a dense block
    for (int e = threadIdx.x; e < n * n; e += MBHT_THREADS) S[(e / n) * SLD + e % n] = 0.f;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += MBHT_THREADS)
        for (int t = 0; t < K; ++t) {
            const int sl = slot[i * HG_MAX_K + t];
            if (sl >= 0 && live[i * HG_MAX_K + t]) S[i * SLD + sel[i * K + t]] = dh[i * HG_ENT + sl];      // (a row's keys are distinct)
        }
    __syncthreads();
    // d u_r = sum_j (dS[r, j] + dS[j, r]) u_j (r < n), then through the column scaling, which every position of the row feeds:
    // d x[l, d] = (d u[l, d] - u[l, d] sum_r d u[r, d] u[r, d]) cinv[d]
    for (int d0 = 0; d0 < H; d0 += HG_DC) {
        hg_stage_unit(Xs, h, xm, n, H, d0);
        __syncthreads();
        for (int e = threadIdx.x; e < n * HG_DC; e += MBHT_THREADS) {
            const int r = e / HG_DC, dd = e % HG_DC;
            float acc = 0.f;
            for (int j = 0; j < n; ++j) acc += (S[r * SLD + j] + S[j * SLD + r]) * Xs[j * HG_XLD + dd];
            if (d0 + dd < H) dxm[(int64_t)r * H + d0 + dd] = acc;
        }
        __syncthreads();
        if ((int)threadIdx.x < HG_DC && d0 + (int)threadIdx.x < H) {
            const int dd = threadIdx.x;
            float acc = 0.f;
            for (int r = 0; r < n; ++r) acc += dxm[(int64_t)r * H + d0 + dd] * Xs[r * HG_XLD + dd];
            cdot[d0 + dd] = acc;
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < L * H; e += MBHT_THREADS) {
        const int r = e / H, d = e % H;
        const float du = r < n ? dxm[e] : 0.f;
        dxm[e] = (du - xm[e] * h.cinv[d] * cdot[d]) * h.cinv[d];
    }
}

// Y[b] = G[b] X[b] on the padded layout: the block-diagonal matrix of the reference never exists
__global__ void __launch_bounds__(MBHT_THREADS)
hg_conv_fwd_kernel(const float* __restrict__ G, const float* __restrict__ x, int L, int H, float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Gs = lds;                          // [L][L]
    float* Xt = Gs + L * L;                   // [L][MIX_LD]
    const int b = blockIdx.x, h0 = blockIdx.y * MIX_TILE;
    for (int e = threadIdx.x; e < L * L; e += MBHT_THREADS) Gs[e] = G[(int64_t)b * L * L + e];
    for (int e = threadIdx.x; e < L * MIX_TILE; e += MBHT_THREADS) {
        const int j = e / MIX_TILE, hc = e % MIX_TILE;
        Xt[j * MIX_LD + hc] = h0 + hc < H ? x[((int64_t)b * L + j) * H + h0 + hc] : 0.f;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < L * MIX_TILE; e += MBHT_THREADS) {
        const int r = e / MIX_TILE, hc = e % MIX_TILE;
        if (h0 + hc >= H) continue;
        float acc = 0.f;
        for (int j = 0; j < L; ++j) acc += Gs[r * L + j] * Xt[j * MIX_LD + hc];
        y[((int64_t)b * L + r) * H + h0 + hc] = acc;
    }
}

// dX[b] = G[b]^T dY[b], dG[b] = dY[b] X[b]^T; one workgroup per row walks the column tiles in order
__global__ void __launch_bounds__(MBHT_THREADS)
hg_conv_bwd_kernel(const float* __restrict__ G, const float* __restrict__ x, const float* __restrict__ dy, int L, int H,
                   float* __restrict__ dx, float* __restrict__ dG) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Gs = lds;                          // [L][L]
    float* Xt = Gs + L * L;                   // [L][MIX_LD]
    float* Yt = Xt + L * MIX_LD;              // [L][MIX_LD]
    const int b = blockIdx.x;
    for (int e = threadIdx.x; e < L * L; e += MBHT_THREADS) Gs[e] = G[(int64_t)b * L * L + e];
    for (int h0 = 0; h0 < H; h0 += MIX_TILE) {
        for (int e = threadIdx.x; e < L * MIX_TILE; e += MBHT_THREADS) {
            const int j = e / MIX_TILE, hc = e % MIX_TILE;
            const bool in = h0 + hc < H;
            Xt[j * MIX_LD + hc] = in ? x[((int64_t)b * L + j) * H + h0 + hc] : 0.f;
            Yt[j * MIX_LD + hc] = in ? dy[((int64_t)b * L + j) * H + h0 + hc] : 0.f;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < L * MIX_TILE; e += MBHT_THREADS) {
            const int j = e / MIX_TILE, hc = e % MIX_TILE;
            if (h0 + hc >= H) continue;
            float acc = 0.f;
            for (int r = 0; r < L; ++r) acc += Gs[r * L + j] * Yt[r * MIX_LD + hc];
            dx[((int64_t)b * L + j) * H + h0 + hc] = acc;
        }
        for (int e = threadIdx.x; e < L * L; e += MBHT_THREADS) {
            const int r = e / L, j = e % L;
            float acc = h0 == 0 ? 0.f : dG[(int64_t)b * L * L + e];
            for (int hc = 0; hc < MIX_TILE; ++hc) acc += Yt[r * MIX_LD + hc] * Xt[j * MIX_LD + hc];
            dG[(int64_t)b * L * L + e] = acc;
        }
        __syncthreads();
    }
}

// The sliding-window readout: for the positions pos[b][0 .. P) in order (training: <= 0 skipped; evaluation: the one position given)
//   out[pos] = mean(out[max(pos - before, 0) : pos] ++ out[pos + 1 : end]),  end = pos + follow if pos + follow < n else n - 1
// in place, so a later readout sees earlier ones; the evaluation form has no second part.  A thread owns a hidden column: the walk
// needs no synchronisation.  An empty window gives NaN, as torch.mean of no rows does.
struct HgWindow { int lo, pos, hi0, hi1, cnt; bool skip; };
__device__ __forceinline__ HgWindow hg_window(int pos, int n, int L, int before, int follow, int eval) {
    HgWindow w;
    w.skip = pos >= L || pos < 0 || (!eval && pos == 0);
    w.pos = pos;
    w.lo = max(pos - before, 0);
    w.hi0 = pos + 1;
    w.hi1 = eval ? pos + 1 : min(pos + follow < n ? pos + follow : n - 1, L);
    if (w.hi1 < w.hi0) w.hi1 = w.hi0;
    w.cnt = (pos - w.lo) + (w.hi1 - w.hi0);
    return w;
}

__global__ void __launch_bounds__(MBHT_THREADS)
hg_readout_fwd_kernel(const float* __restrict__ x, const int32_t* __restrict__ pos, const int32_t* __restrict__ n_obj, int L, int H, int P,
                      int before, int follow, int eval, float* __restrict__ out) {
    const int b = blockIdx.x, d = threadIdx.x;
    if (d >= H) return;
    float* o = out + (int64_t)b * L * H + d;
    for (int r = 0; r < L; ++r) o[(int64_t)r * H] = x[((int64_t)b * L + r) * H + d];
    for (int t = 0; t < P; ++t) {
        const HgWindow w = hg_window(pos[(int64_t)b * P + t], n_obj[b], L, before, follow, eval);
        if (w.skip) continue;
        float acc = 0.f;
        for (int r = w.lo; r < w.pos; ++r) acc += o[(int64_t)r * H];
        for (int r = w.hi0; r < w.hi1; ++r) acc += o[(int64_t)r * H];
        o[(int64_t)w.pos * H] = acc / (float)w.cnt;
    }
}

__global__ void __launch_bounds__(MBHT_THREADS)
hg_readout_bwd_kernel(const float* __restrict__ dout, const int32_t* __restrict__ pos, const int32_t* __restrict__ n_obj, int L, int H,
                      int P, int before, int follow, int eval, float* __restrict__ dx) {
    const int b = blockIdx.x, d = threadIdx.x;
    if (d >= H) return;
    float* g = dx + (int64_t)b * L * H + d;
    for (int r = 0; r < L; ++r) g[(int64_t)r * H] = dout[((int64_t)b * L + r) * H + d];
    for (int t = P - 1; t >= 0; --t) {
        const HgWindow w = hg_window(pos[(int64_t)b * P + t], n_obj[b], L, before, follow, eval);
        if (w.skip) continue;
        const float gp = g[(int64_t)w.pos * H] / (float)w.cnt;
        g[(int64_t)w.pos * H] = 0.f;                                             // (the value it replaced reaches nothing)
        for (int r = w.lo; r < w.pos; ++r) g[(int64_t)r * H] += gp;
        for (int r = w.hi0; r < w.hi1; ++r) g[(int64_t)r * H] += gp;
    }
}

// The fusion of the two sources: p0 = softmax over the sources of x_s . w (w = attn_weights attn^T), out = p0 x0 + (1 - p0) x1.
// One wave per row.
__global__ void __launch_bounds__(MBHT_THREADS)
hg_fuse_fwd_kernel(const float* __restrict__ x0, const float* __restrict__ x1, const float* __restrict__ w, int T, int H,
                   float* __restrict__ out, float* __restrict__ p0) {
    const int lane = threadIdx.x & 63;
    const int64_t r = ((int64_t)blockIdx.x * MBHT_THREADS + threadIdx.x) >> 6;
    if (r >= T) return;
    float s0 = 0.f, s1 = 0.f;
    for (int d = lane; d < H; d += 64) { s0 += x0[r * H + d] * w[d]; s1 += x1[r * H + d] * w[d]; }
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    const float m = fmaxf(s0, s1), e0 = expf(s0 - m), e1 = expf(s1 - m);
    const float p = e0 / (e0 + e1);
    for (int d = lane; d < H; d += 64) out[r * H + d] = p * x0[r * H + d] + (1.f - p) * x1[r * H + d];
    if (lane == 0) p0[r] = p;
}

// dx0, dx1 and slabs of dw: workgroup g walks the rows 4 g + wave, + 4 gridDim.x, ... ; its four waves' sums are added in order
__global__ void __launch_bounds__(MBHT_THREADS)
hg_fuse_bwd_kernel(const float* __restrict__ x0, const float* __restrict__ x1, const float* __restrict__ w, const float* __restrict__ p0,
                   const float* __restrict__ dout, int T, int H, float* __restrict__ dx0, float* __restrict__ dx1,
                   float* __restrict__ partial) {
    __shared__ float red[MBHT_THREADS / 64][MBHT_MAX_H];
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    float dw[MBHT_MAX_H / 64];
#pragma unroll
    for (int i = 0; i < MBHT_MAX_H / 64; ++i) dw[i] = 0.f;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wib; r < T; r += (int64_t)gridDim.x * 4) {
        const float p = p0[r];
        float dp = 0.f;
        for (int d = lane; d < H; d += 64) dp += dout[r * H + d] * (x0[r * H + d] - x1[r * H + d]);
        dp = wave_sum(dp);
        const float ds = p * (1.f - p) * dp;                                     // d s0 = - d s1
#pragma unroll
        for (int i = 0; i < MBHT_MAX_H / 64; ++i) {
            const int d = lane + 64 * i;
            if (d < H) {
                const float g = dout[r * H + d], a = x0[r * H + d], c = x1[r * H + d];
                dx0[r * H + d] = p * g + ds * w[d];
                dx1[r * H + d] = (1.f - p) * g - ds * w[d];
                dw[i] += ds * (a - c);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < MBHT_MAX_H / 64; ++i) red[wib][lane + 64 * i] = dw[i];
    __syncthreads();
    for (int d = threadIdx.x; d < H; d += MBHT_THREADS)
        partial[(int64_t)blockIdx.x * H + d] = ((red[0][d] + red[1][d]) + red[2][d]) + red[3][d];
}

}  // namespace gamer

using namespace gamer;
#define ST(s) ((hipStream_t)(s))

static int msa_args(const char* name, MsaArgs& a, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                    const int32_t* keep, const float* Ew, const float* Eb, const float* Fw, const float* Fb, int B, int L, int H, int dh,
                    int c, float scale, float p_drop, uint64_t seed) {
    GAMER_CHECK_ARG(q && k && v && keep && Ew && Eb && Fw && Fb, "%s: null pointer", name);
    GAMER_CHECK_ARG(B > 0 && L > 0 && L <= MBHT_MAX_L && H > 0 && dh > 0 && dh <= MBHT_MAX_D && c > 0 && c <= MBHT_MAX_C &&
                        (int64_t)B * H < (1LL << 31),
                    "%s: bad shape B=%d L=%d H=%d head_dim=%d c=%d (L <= %d, head_dim <= %d, c <= %d)", name, B, L, H, dh, c, MBHT_MAX_L,
                    MBHT_MAX_D, MBHT_MAX_C);
    GAMER_CHECK_ARG(ldq >= H * dh && ldk >= H * dh && ldv >= H * dh, "%s: bad leading dims", name);
    GAMER_CHECK_ARG(p_drop >= 0.f && p_drop < 1.f, "%s: p_drop=%f", name, p_drop);
    a.q = q; a.k = k; a.v = v; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.keep = keep; a.Ew = Ew; a.Eb = Eb; a.Fw = Fw; a.Fb = Fb;
    a.B = B; a.L = L; a.H = H; a.dh = dh; a.c = c; a.scale = scale; a.p_drop = p_drop; a.seed = seed;
    return 0;
}

extern "C" int gamer_msa_linear_fwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const int32_t* keep,
                                    const float* Ew, const float* Eb, const float* Fw, const float* Fb, int B, int L, int H,
                                    int head_dim, int c, float scale, float p_drop, uint64_t seed, float* o, int ldo, float* lse,
                                    void* stream) {
    MsaArgs a;
    GAMER_TRY(msa_args("gamer_msa_linear_fwd", a, q, ldq, k, ldk, v, ldv, keep, Ew, Eb, Fw, Fb, B, L, H, head_dim, c, scale, p_drop, seed));
    GAMER_CHECK_ARG(o && lse && ldo >= H * head_dim, "gamer_msa_linear_fwd: bad output");
    return launch<msa_linear_fwd_kernel>("gamer_msa_linear_fwd", dim3(B * H), dim3(MBHT_THREADS), 0, ST(stream), a, o, ldo, lse);
}

extern "C" int gamer_msa_linear_bwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const int32_t* keep,
                                    const float* Ew, const float* Eb, const float* Fw, const float* Fb, int B, int L, int H,
                                    int head_dim, int c, float scale, float p_drop, uint64_t seed, const float* d_o, int ldo,
                                    const float* lse, float* dq, int lddq, float* dk, int lddk, float* dv, int lddv, float* partial,
                                    int n_partial, void* stream) {
    MsaArgs a;
    GAMER_TRY(msa_args("gamer_msa_linear_bwd", a, q, ldq, k, ldk, v, ldv, keep, Ew, Eb, Fw, Fb, B, L, H, head_dim, c, scale, p_drop, seed));
    GAMER_CHECK_ARG(d_o && lse && dq && dk && dv && partial, "gamer_msa_linear_bwd: null pointer");
    GAMER_CHECK_ARG(ldo >= H * head_dim && lddq >= H * head_dim && lddk >= H * head_dim && lddv >= H * head_dim,
                    "gamer_msa_linear_bwd: bad leading dims");
    GAMER_CHECK_ARG(n_partial > 0 && n_partial <= B * H, "gamer_msa_linear_bwd: n_partial=%d (1 .. B H)", n_partial);
    return launch<msa_linear_bwd_kernel>("gamer_msa_linear_bwd", dim3(n_partial), dim3(MBHT_THREADS), 0, ST(stream), a, d_o, ldo, lse, dq,
                                         lddq, dk, lddk, dv, lddv, partial);
}

constexpr size_t MIX_LDS_MAX = 150 * 1024;      // of the 160 KB per CU

static int mix_args(const char* name, MixSrc& s, const float* x0, int L0, const float* x1, int L1, const float* x2, int L2, const float* W,
                    int B, int H, int Lout) {
    GAMER_CHECK_ARG(x0 && W && L0 > 0 && L1 >= 0 && L2 >= 0 && !x1 == (L1 == 0) && !x2 == (L2 == 0),
                    "%s: three sources (the second and third may be empty: NULL with length 0)", name);
    GAMER_CHECK_ARG(B > 0 && H > 0 && H <= MBHT_MAX_H && Lout > 0 && Lout <= MBHT_MAX_L && L0 <= MBHT_MAX_L && L1 <= MBHT_MAX_L &&
                        L2 <= MBHT_MAX_L,
                    "%s: bad shape B=%d H=%d Lout=%d lengths %d %d %d (H <= %d, every length <= %d)", name, B, H, Lout, L0, L1, L2,
                    MBHT_MAX_H, MBHT_MAX_L);
    s.x[0] = x0; s.x[1] = x1 ? x1 : x0; s.x[2] = x2 ? x2 : x0; s.len[0] = L0; s.len[1] = L1; s.len[2] = L2;
    return 0;
}

extern "C" int gamer_seq_mix_fwd(const float* x0, int L0, const float* x1, int L1, const float* x2, int L2, const float* W,
                                 const float* bias, int B, int H, int Lout, float* y, void* stream) {
    MixSrc s;
    GAMER_TRY(mix_args("gamer_seq_mix_fwd", s, x0, L0, x1, L1, x2, L2, W, B, H, Lout));
    GAMER_CHECK_ARG(bias && y, "gamer_seq_mix_fwd: null pointer");
    const size_t shmem = (size_t)(L0 + L1 + L2) * MIX_LD * sizeof(float);
    GAMER_CHECK_ARG(shmem <= MIX_LDS_MAX, "gamer_seq_mix_fwd: %zu bytes of LDS", shmem);
    return launch<seq_mix_fwd_kernel>("gamer_seq_mix_fwd", dim3(B, (H + MIX_TILE - 1) / MIX_TILE), dim3(MBHT_THREADS), shmem, ST(stream), s,
                                      W, bias, H, Lout, y);
}

extern "C" int gamer_seq_mix_bwd(const float* x0, int L0, const float* x1, int L1, const float* x2, int L2, const float* W,
                                 const float* dy, int B, int H, int Lout, float* dx0, float* dx1, float* dx2, float* partial,
                                 int n_partial, void* stream) {
    MixSrc s;
    GAMER_TRY(mix_args("gamer_seq_mix_bwd", s, x0, L0, x1, L1, x2, L2, W, B, H, Lout));
    GAMER_CHECK_ARG(dy && dx0 && partial && !dx1 == (L1 == 0) && !dx2 == (L2 == 0), "gamer_seq_mix_bwd: null pointer");
    GAMER_CHECK_ARG(n_partial > 0 && n_partial <= B, "gamer_seq_mix_bwd: n_partial=%d (1 .. B)", n_partial);
    const size_t shmem = (size_t)(L0 + L1 + L2 + Lout) * MIX_LD * sizeof(float);
    GAMER_CHECK_ARG(shmem <= MIX_LDS_MAX, "gamer_seq_mix_bwd: %zu bytes of LDS", shmem);
    return launch<seq_mix_bwd_kernel>("gamer_seq_mix_bwd", dim3(n_partial), dim3(MBHT_THREADS), shmem, ST(stream), s, W, dy, B, H, Lout, dx0,
                                      dx1 ? dx1 : dx0, dx2 ? dx2 : dx0, partial);
}

constexpr size_t HG_LDS_MAX = 150 * 1024;

static int hg_shape(const char* name, int B, int L, int H, int K) {
    GAMER_CHECK_ARG(B > 0 && L > 0 && L <= MBHT_MAX_L && H > 0 && H <= MBHT_MAX_H && K > 0 && K <= HG_MAX_K,
                    "%s: bad shape B=%d L=%d H=%d hyper_len=%d (L <= %d, H <= %d, hyper_len <= %d)", name, B, L, H, K, MBHT_MAX_L,
                    MBHT_MAX_H, HG_MAX_K);
    return 0;
}

extern "C" int gamer_hg_build_fwd(const float* xm, const int32_t* items, int B, int L, int H, int hyper_len, int mask_token, float* G,
                                  int32_t* sel, void* stream) {
    GAMER_CHECK_ARG(xm && items && G && sel, "gamer_hg_build_fwd: null pointer");
    GAMER_TRY(hg_shape("gamer_hg_build_fwd", B, L, H, hyper_len));
    GAMER_CHECK_ARG(mask_token > 0 && mask_token < HG_MULTI, "gamer_hg_build_fwd: mask_token=%d", mask_token);
    const size_t shmem = (hg_lists_floats(L) + (size_t)L * (L | 1) + (size_t)L * HG_XLD) * sizeof(float);
    GAMER_CHECK_ARG(shmem <= HG_LDS_MAX, "gamer_hg_build_fwd: %zu bytes of LDS", shmem);
    return launch<hg_build_fwd_kernel>("gamer_hg_build_fwd", dim3(B), dim3(MBHT_THREADS), shmem, ST(stream), xm, items, L, H, hyper_len,
                                       mask_token, G, sel);
}

extern "C" int gamer_hg_build_bwd(const float* xm, const int32_t* items, const int32_t* sel, const float* G, const float* dG, int B,
                                  int L, int H, int hyper_len, int mask_token, float* dxm, void* stream) {
    GAMER_CHECK_ARG(xm && items && sel && G && dG && dxm, "gamer_hg_build_bwd: null pointer");
    GAMER_TRY(hg_shape("gamer_hg_build_bwd", B, L, H, hyper_len));
    GAMER_CHECK_ARG(mask_token > 0 && mask_token < HG_MULTI, "gamer_hg_build_bwd: mask_token=%d", mask_token);
    const size_t shmem = (hg_lists_floats(L) + (size_t)L * (L | 1) + (size_t)L * HG_XLD + (size_t)L * (2 * HG_ENT + 1 + 3 * HG_MAX_K) + MBHT_MAX_H) *
                         sizeof(float);
    GAMER_CHECK_ARG(shmem <= HG_LDS_MAX, "gamer_hg_build_bwd: %zu bytes of LDS", shmem);
    return launch<hg_build_bwd_kernel>("gamer_hg_build_bwd", dim3(B), dim3(MBHT_THREADS), shmem, ST(stream), xm, items, sel, G, dG, L, H,
                                       hyper_len, mask_token, dxm);
}

extern "C" int gamer_hg_conv_fwd(const float* G, const float* x, int B, int L, int H, float* y, void* stream) {
    GAMER_CHECK_ARG(G && x && y, "gamer_hg_conv_fwd: null pointer");
    GAMER_TRY(hg_shape("gamer_hg_conv_fwd", B, L, H, 1));
    const size_t shmem = ((size_t)L * L + (size_t)L * MIX_LD) * sizeof(float);
    return launch<hg_conv_fwd_kernel>("gamer_hg_conv_fwd", dim3(B, (H + MIX_TILE - 1) / MIX_TILE), dim3(MBHT_THREADS), shmem, ST(stream), G,
                                      x, L, H, y);
}

extern "C" int gamer_hg_conv_bwd(const float* G, const float* x, const float* dy, int B, int L, int H, float* dx, float* dG,
                                 void* stream) {
    GAMER_CHECK_ARG(G && x && dy && dx && dG, "gamer_hg_conv_bwd: null pointer");
    GAMER_TRY(hg_shape("gamer_hg_conv_bwd", B, L, H, 1));
    const size_t shmem = ((size_t)L * L + (size_t)2 * L * MIX_LD) * sizeof(float);
    return launch<hg_conv_bwd_kernel>("gamer_hg_conv_bwd", dim3(B), dim3(MBHT_THREADS), shmem, ST(stream), G, x, dy, L, H, dx, dG);
}

static int hg_readout_check(const char* name, const void* a, const void* pos, const void* n_obj, const void* out, int B, int L, int H,
                            int P, int before, int follow) {
    GAMER_CHECK_ARG(a && pos && n_obj && out, "%s: null pointer", name);
    GAMER_TRY(hg_shape(name, B, L, H, 1));
    GAMER_CHECK_ARG(P > 0 && before >= 0 && follow >= 0, "%s: P=%d before=%d follow=%d", name, P, before, follow);
    return 0;
}

extern "C" int gamer_hg_readout_fwd(const float* x, const int32_t* pos, const int32_t* n_obj, int B, int L, int H, int P, int before,
                                    int follow, int eval, float* out, void* stream) {
    GAMER_TRY(hg_readout_check("gamer_hg_readout_fwd", x, pos, n_obj, out, B, L, H, P, before, follow));
    return launch<hg_readout_fwd_kernel>("gamer_hg_readout_fwd", dim3(B), dim3(MBHT_THREADS), 0, ST(stream), x, pos, n_obj, L, H, P, before,
                                         follow, eval, out);
}

extern "C" int gamer_hg_readout_bwd(const float* dout, const int32_t* pos, const int32_t* n_obj, int B, int L, int H, int P, int before,
                                    int follow, int eval, float* dx, void* stream) {
    GAMER_TRY(hg_readout_check("gamer_hg_readout_bwd", dout, pos, n_obj, dx, B, L, H, P, before, follow));
    return launch<hg_readout_bwd_kernel>("gamer_hg_readout_bwd", dim3(B), dim3(MBHT_THREADS), 0, ST(stream), dout, pos, n_obj, L, H, P,
                                         before, follow, eval, dx);
}

extern "C" int gamer_hg_fuse_fwd(const float* x0, const float* x1, const float* w, int64_t T, int H, float* out, float* p0, void* stream) {
    GAMER_CHECK_ARG(x0 && x1 && w && out && p0, "gamer_hg_fuse_fwd: null pointer");
    GAMER_CHECK_ARG(T > 0 && T < (1LL << 29) && H > 0 && H <= MBHT_MAX_H, "gamer_hg_fuse_fwd: bad shape T=%lld H=%d (H <= %d)", (long long)T, H,
                    MBHT_MAX_H);
    const int64_t blocks = (T * 64 + MBHT_THREADS - 1) / MBHT_THREADS;
    return launch<hg_fuse_fwd_kernel>("gamer_hg_fuse_fwd", dim3((unsigned)blocks), dim3(MBHT_THREADS), 0, ST(stream), x0, x1, w, (int)T, H, out,
                                      p0);
}

extern "C" int gamer_hg_fuse_bwd(const float* x0, const float* x1, const float* w, const float* p0, const float* dout, int64_t T, int H,
                                 float* dx0, float* dx1, float* partial, int n_partial, void* stream) {
    GAMER_CHECK_ARG(x0 && x1 && w && p0 && dout && dx0 && dx1 && partial, "gamer_hg_fuse_bwd: null pointer");
    GAMER_CHECK_ARG(T > 0 && T < (1LL << 29) && H > 0 && H <= MBHT_MAX_H && n_partial > 0,
                    "gamer_hg_fuse_bwd: bad shape T=%lld H=%d n_partial=%d (H <= %d)", (long long)T, H, n_partial, MBHT_MAX_H);
    return launch<hg_fuse_bwd_kernel>("gamer_hg_fuse_bwd", dim3(n_partial), dim3(MBHT_THREADS), 0, ST(stream), x0, x1, w, p0, dout, (int)T, H,
                                      dx0, dx1, partial);
}
