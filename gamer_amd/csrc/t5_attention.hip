// T5's attention (HF T5Attention, the TIGER backbone of ref:SeqRec/models/generative/TIGER/model.py) and its bias kernels.
//   score[i, j] = q_i . k_j + rel[head][j - i + Sq - 1]        no 1 / sqrt(d); rel = nullptr: no bias (cross attention)
//   ctx[i]      = sum_j dropout(softmax_j(score over the allowed keys))[i, j] v_j
// A key j is allowed for query i when keep[b][j] != 0 (nullptr: all kept) and, with `causal`, j <= i.  A query row with no
// allowed key gives a zero context, lse = -inf and zero gradients (HF's additive finfo.min mask gives a softmax over the bias
// alone there; rows of real inputs always hold </s>).
// One workgroup per (batch row, head), four waves; K and V of the head live in LDS ([Sk16][d + 4]: the + 4 spreads a 16-row
// operand read over all 64 banks and keeps the rows 16-byte aligned).  Both products run on the exact fp32 MFMA
// v_mfma_f32_16x16x4_f32.  A wave owns tiles of 16 queries and forms the TRANSPOSED score tile S^T = K_tile Q_tile^T: its
// accumulator then has the query on lane & 15 and four keys in the registers, which is the A-operand form of the next product
// (P V, dS K) with the key order permuted the same way on the V / K side - the probabilities never leave the registers in the
// forward, and nothing of size Sq x Sk reaches memory in either direction.
// The backward recomputes p from the saved log-sum-exp into one LDS array P [Sq16][ldp] (sign bit = dropped), takes dV from it
// (waves own KEY tiles now, the sum runs over the queries), turns it into dS in place while forming dQ (the row term delta_i is
// summed from dropout(p) dP itself, so the forward's output is not read), takes dK from it, and
// sums dS along the diagonals for the bias gradient by relative offset.  A workgroup walks the rows slot, slot + n_slab, ...
// and owns slab `slot` of the offset gradient: written by that workgroup alone (no float atomics), reduced in slab order by
// gamer_t5_bias_fold.
// The packed forms (gamer_t5_attn_packed_fwd / _bwd; PK = true): the rows lie one behind the other without padding tokens and a workgroup
// looks its row up in the offset arrays (t5_row<PK> of t5_attention_common.h).  a.Sq, a.Sk are then the shape of the dense run that the
// call replaces: the bias offset j - i + a.Sq - 1 and the dropout counter ((b H + head) a.Sq + i) a.Sk + j are that run's, there is no
// keep, and the LDS arrays are laid out by the row's own lengths inside what the host sized by (a.Sq, a.Sk).
//   gamer_t5_bias_expand   table [num_buckets][h] -> rel [h][R] through the host's bucket-per-offset vector
//   gamer_t5_bias_fold     slabs [layers][n_slab][h][R] -> table gradient [num_buckets][h]: slabs in order, offsets in order,
//                          then the layers in order (the table of layer 0 serves every layer of its stack)
#include "t5_attention_common.h"

namespace gamer {

constexpr int T5_MAX_S = 128, T5_MAX_KT = T5_MAX_S / 16;

__host__ __device__ static inline int t5_ldp(int sk16) { return sk16 % 32 == 16 ? sk16 : sk16 + 16; }      // ldp % 32 == 16

__device__ __forceinline__ void t5_stage_keep(int* __restrict__ kp, const uint8_t* __restrict__ keep, int b, int Sk, int Sk16) {
    for (int j = threadIdx.x; j < Sk16; j += T5_THREADS) kp[j] = j < Sk && (!keep || keep[(int64_t)b * Sk + j]) ? 1 : 0;
}

template <int D, bool PK>
__global__ void __launch_bounds__(T5_THREADS)
t5_attn_fwd_kernel(const T5Args a, float* __restrict__ o, int ldo, float* __restrict__ lse) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int LD = D + 4;
    const int b = blockIdx.x / a.H, hh = blockIdx.x % a.H;
    const int bk = a.kv_rows ? a.kv_rows[b] : b;
    const T5Row row = t5_row<PK>(a, b, bk, hh);
    const int Sq = row.Sq, Sk = row.Sk, Sk16 = (Sk + 15) & ~15, nkt = Sk16 / 16, nqt = (Sq + 15) / 16;
    float* Ks = lds;                          // [Sk16][LD]
    float* Vs = Ks + Sk16 * LD;               // [Sk16][LD]
    int* kp = (int*)(Vs + Sk16 * LD);         // [Sk16]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    t5_stage<D>(Ks, a.k + row.k0 * a.ldk + hh * D, a.ldk, Sk, Sk16);
    t5_stage<D>(Vs, a.v + row.k0 * a.ldv + hh * D, a.ldv, Sk, Sk16);
    t5_stage_keep(kp, a.keep, bk, Sk, Sk16);
    __syncthreads();
    const DropoutRng rng(a.p_drop, a.seed);
    const float* qb = a.q + row.q0 * a.ldq + hh * D;
    float* ob = o + row.q0 * ldo + hh * D;
    for (int qt = wave; qt < nqt; qt += T5_WAVES) {
        const int i = qt * 16 + (lane & 15);
        const bool iv = i < Sq;
        float qr[D / 4];
        t5_row_operand<D>(qr, iv ? qb + (int64_t)i * a.ldq : nullptr, lane);
        const float* relrow = a.rel ? a.rel + (int64_t)hh * (a.Sq + a.Sk - 1) + (a.Sq - 1 - i) : nullptr;      // read at [j] for allowed (i, j) only
        f32x4v s[T5_MAX_KT];
        float m = -INFINITY;
#pragma unroll
        for (int nt = 0; nt < T5_MAX_KT; ++nt) {
            if (nt < nkt) {
                s[nt] = t5_tile<D>(Ks + nt * 16 * LD, qr, lane);
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int j = nt * 16 + 4 * (lane >> 4) + reg;
                    const bool ok = iv && kp[j] && (!a.causal || j <= i);
                    s[nt][reg] = ok ? s[nt][reg] + (relrow ? relrow[j] : 0.f) : -INFINITY;
                    m = fmaxf(m, s[nt][reg]);
                }
            }
        }
        m = t5_xor_max(m);
        const float ms = m == -INFINITY ? 0.f : m;
        float sum = 0.f;
#pragma unroll
        for (int nt = 0; nt < T5_MAX_KT; ++nt)
            if (nt < nkt) {
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) sum += expf(s[nt][reg] - ms);
            }
        sum = t5_xor_sum(sum);
        const float l = m + logf(sum);                          // (no allowed key: -inf + -inf)
        const float ls = m == -INFINITY ? 0.f : l;
        if (iv && lane < 16) lse[row.l0 + i] = l;
        f32x4v acc[D / 16];
#pragma unroll
        for (int n = 0; n < D / 16; ++n) acc[n] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int nt = 0; nt < T5_MAX_KT; ++nt)
            if (nt < nkt) {
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int j = nt * 16 + 4 * (lane >> 4) + reg;
                    float p = expf(s[nt][reg] - ls);            // (a key that is not allowed: exp(-inf) = 0)
                    if (rng.on && iv && j < Sk) p *= rng.mult((((uint64_t)b * a.H + hh) * a.Sq + i) * a.Sk + j);
                    s[nt][reg] = p;
                }
                t5_tile_out<D>(acc, s[nt], Vs + nt * 16 * LD, lane);
            }
        t5_store_rows<D>(ob, ldo, qt * 16, Sq, acc, lane);
    }
}

// P holds the probability with the SIGN bit as the dropout decision (set = dropped), so one array serves p and dropout(p)
__device__ __forceinline__ float t5_pd(float x, float keep_scale) { return (__float_as_uint(x) >> 31) ? 0.f : x * keep_scale; }

// acc[n] = sum_i f(P[i][key tile column lane & 15]) X[i][16 n + (lane & 15)] over the rows i < rows of a global [., D] head block
template <int D, bool PD>
__device__ __forceinline__ void t5_key_tile(f32x4v (&acc)[D / 16], const float* __restrict__ Pcol, int ldp, const float* __restrict__ x, int ldx,
                                            int rows, int rows16, float keep_scale, int lane) {
#pragma unroll
    for (int n = 0; n < D / 16; ++n) acc[n] = f32x4v{0.f, 0.f, 0.f, 0.f};
    for (int i4 = 0; i4 < rows16; i4 += 4) {
        const int i = i4 + (lane >> 4);
        const float pv = Pcol[i * ldp + (lane & 15)];
        const float av = PD ? t5_pd(pv, keep_scale) : pv;
        const float* xr = x + (int64_t)i * ldx + (lane & 15);
#pragma unroll
        for (int n = 0; n < D / 16; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, i < rows ? xr[16 * n] : 0.f, acc[n], 0, 0, 0);
    }
}

template <int D, bool PK>
__global__ void __launch_bounds__(T5_THREADS)
t5_attn_bwd_kernel(const T5Args a, const float* __restrict__ d_o, int ldo, const float* __restrict__ lse,
                   float* __restrict__ dq, int lddq, float* __restrict__ dk, int lddk, float* __restrict__ dv, int lddv,
                   float* __restrict__ drel_part, int n_slab) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int LD = D + 4;
    const int R = a.Sq + a.Sk - 1;
    const int hh = blockIdx.x % a.H, slot = blockIdx.x / a.H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const DropoutRng rng(a.p_drop, a.seed);
    const float keep_scale = rng.scale;
    float* slab = drel_part ? drel_part + ((int64_t)slot * a.H + hh) * R : nullptr;
    for (int b = slot; b < a.B; b += n_slab) {
        // (the LDS arrays are laid out by this row's lengths: within what the host sized by a.Sq, a.Sk)
        const T5Row row = t5_row<PK>(a, b, b, hh);
        const int Sq = row.Sq, Sk = row.Sk, Sk16 = (Sk + 15) & ~15, Sq16 = (Sq + 15) & ~15, nkt = Sk16 / 16, nqt = Sq16 / 16;
        const int ldp = t5_ldp(Sk16);
        float* Ks = lds;                          // [Sk16][LD]
        float* Vs = Ks + Sk16 * LD;               // [Sk16][LD]
        float* P = Vs + Sk16 * LD;                // [Sq16][ldp]
        int* kp = (int*)(P + Sq16 * ldp);         // [Sk16]
        const float* qb = a.q + row.q0 * a.ldq + hh * D;
        const float* gb = d_o + row.q0 * ldo + hh * D;
        __syncthreads();                                                         // (the row before is done with the LDS)
        t5_stage<D>(Ks, a.k + row.k0 * a.ldk + hh * D, a.ldk, Sk, Sk16);
        t5_stage<D>(Vs, a.v + row.k0 * a.ldv + hh * D, a.ldv, Sk, Sk16);
        t5_stage_keep(kp, a.keep, b, Sk, Sk16);
        __syncthreads();
        // ---- p from the saved log-sum-exp (query tiles) ----------------------------------------------------------------------
        for (int qt = wave; qt < nqt; qt += T5_WAVES) {
            const int i = qt * 16 + (lane & 15);
            const bool iv = i < Sq;
            float qr[D / 4];
            t5_row_operand<D>(qr, iv ? qb + (int64_t)i * a.ldq : nullptr, lane);
            const float* relrow = a.rel ? a.rel + (int64_t)hh * R + (a.Sq - 1 - i) : nullptr;
            const float l = iv ? lse[row.l0 + i] : 0.f;
            for (int nt = 0; nt < nkt; ++nt) {
                const f32x4v s = t5_tile<D>(Ks + nt * 16 * LD, qr, lane);
                float4 pv;
                float* pp = &pv.x;
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int j = nt * 16 + 4 * (lane >> 4) + reg;
                    const bool ok = iv && kp[j] && (!a.causal || j <= i);
                    float p = 0.f;
                    if (ok) {
                        p = expf(s[reg] + (relrow ? relrow[j] : 0.f) - l);
                        if (rng.on && rng.mult((((uint64_t)b * a.H + hh) * a.Sq + i) * a.Sk + j) == 0.f) p = -p;
                    }
                    pp[reg] = p;
                }
                *reinterpret_cast<float4*>(P + i * ldp + nt * 16 + 4 * (lane >> 4)) = pv;
            }
        }
        __syncthreads();
        // ---- dV = dropout(p)^T dO (key tiles) ----------------------------------------------------------------------------------
        for (int kt = wave; kt < nkt; kt += T5_WAVES) {
            f32x4v acc[D / 16];
            t5_key_tile<D, true>(acc, P + kt * 16, ldp, gb, ldo, Sq, Sq16, keep_scale, lane);
            t5_store_rows<D>(dv + row.k0 * lddv + hh * D, lddv, kt * 16, Sk, acc, lane);
        }
        __syncthreads();
        // ---- dS in place, dQ = dS K (query tiles).  delta_i = sum_j dropout(p)[i, j] dP[i, j] from the very products it is subtracted
        // from (not from O . dO): with one dominant key p (dP - delta) is then a difference of nearly the same fp32 number ------------
        for (int qt = wave; qt < nqt; qt += T5_WAVES) {
            const int i = qt * 16 + (lane & 15);
            float gr[D / 4];
            t5_row_operand<D>(gr, i < Sq ? gb + (int64_t)i * ldo : nullptr, lane);
            const float* prow = P + i * ldp + 4 * (lane >> 4);
            f32x4v dp[T5_MAX_KT];
            float dl = 0.f;
#pragma unroll
            for (int nt = 0; nt < T5_MAX_KT; ++nt)
                if (nt < nkt) {
                    dp[nt] = t5_tile<D>(Vs + nt * 16 * LD, gr, lane);
                    const float4 x = *reinterpret_cast<const float4*>(prow + nt * 16);
                    dl += t5_pd(x.x, keep_scale) * dp[nt][0] + t5_pd(x.y, keep_scale) * dp[nt][1] + t5_pd(x.z, keep_scale) * dp[nt][2] +
                          t5_pd(x.w, keep_scale) * dp[nt][3];
                }
            dl = t5_xor_sum(dl);
            f32x4v acc[D / 16];
#pragma unroll
            for (int n = 0; n < D / 16; ++n) acc[n] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int nt = 0; nt < T5_MAX_KT; ++nt)
                if (nt < nkt) {
                    float4* pp = reinterpret_cast<float4*>(P + i * ldp + nt * 16 + 4 * (lane >> 4));
                    const float4 x = *pp;
                    f32x4v ds;
                    ds[0] = t5_pd(x.x, keep_scale) * dp[nt][0] - fabsf(x.x) * dl;
                    ds[1] = t5_pd(x.y, keep_scale) * dp[nt][1] - fabsf(x.y) * dl;
                    ds[2] = t5_pd(x.z, keep_scale) * dp[nt][2] - fabsf(x.z) * dl;
                    ds[3] = t5_pd(x.w, keep_scale) * dp[nt][3] - fabsf(x.w) * dl;
                    *pp = make_float4(ds[0], ds[1], ds[2], ds[3]);
                    t5_tile_out<D>(acc, ds, Ks + nt * 16 * LD, lane);
                }
            t5_store_rows<D>(dq + row.q0 * lddq + hh * D, lddq, qt * 16, Sq, acc, lane);
        }
        __syncthreads();
        // ---- dK = dS^T Q (key tiles) -----------------------------------------------------------------------------------------------
        for (int kt = wave; kt < nkt; kt += T5_WAVES) {
            f32x4v acc[D / 16];
            t5_key_tile<D, false>(acc, P + kt * 16, ldp, qb, a.ldq, Sq, Sq16, 1.f, lane);
            t5_store_rows<D>(dk + row.k0 * lddk + hh * D, lddk, kt * 16, Sk, acc, lane);
        }
        // ---- the bias gradient by relative offset: sums of dS along the diagonals j - i = r - (Sq - 1), queries in order -----------
        if (slab)
            for (int r = threadIdx.x; r < R; r += T5_THREADS) {
                const int off = r - (a.Sq - 1);
                float acc = 0.f;
                for (int i = max(0, -off); i < Sq && i + off < Sk; ++i) acc += P[i * ldp + i + off];
                slab[r] = b == slot ? acc : slab[r] + acc;
            }
    }
}

__global__ void __launch_bounds__(T5_THREADS)
t5_bias_expand_kernel(const float* __restrict__ table, const int32_t* __restrict__ bucket, int nb, int H, int R, float* __restrict__ rel) {
    const int e = blockIdx.x * T5_THREADS + threadIdx.x;
    if (e >= H * R) return;
    const int hh = e / R, r = e % R;
    rel[e] = table[min(max(bucket[r], 0), nb - 1) * H + hh];                    // (an index outside the table cannot leave it)
}

// one wave per (bucket, head)
__global__ void __launch_bounds__(WAVE)
t5_bias_fold_kernel(const float* __restrict__ slabs, int n_layers, int n_slab, int H, int R, const int32_t* __restrict__ bucket,
                    float* __restrict__ dtable) {
    const int bk = blockIdx.x / H, hh = blockIdx.x % H, lane = threadIdx.x;
    float total = 0.f;
    for (int l = 0; l < n_layers; ++l) {
        float acc = 0.f;
        for (int r = lane; r < R; r += WAVE)
            if (bucket[r] == bk) {
                float v = 0.f;
                for (int s = 0; s < n_slab; ++s) v += slabs[(((int64_t)l * n_slab + s) * H + hh) * R + r];
                acc += v;
            }
        acc = wave_sum(acc);
        total = l == 0 ? acc : total + acc;
    }
    if (lane == 0) dtable[bk * H + hh] = total;
}

}  // namespace gamer

using namespace gamer;
#define ST(s) ((hipStream_t)(s))

constexpr size_t T5_LDS_MAX = 150 * 1024;       // of the 160 KB per CU

extern "C" int gamer_t5_attn_fwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* rel,
                                 const uint8_t* keep, const int32_t* kv_rows, int B, int Sq, int Sk, int H, int head_dim, int causal,
                                 float p_drop, uint64_t seed, float* o, int ldo, float* lse, void* stream) {
    T5Args a;
    GAMER_TRY(t5_args("gamer_t5_attn_fwd", a, q, ldq, k, ldk, v, ldv, rel, keep, B, Sq, Sk, H, head_dim, causal, p_drop, seed, T5_MAX_S));
    a.kv_rows = kv_rows;
    GAMER_CHECK_ARG(o && lse && ldo >= H * head_dim, "gamer_t5_attn_fwd: bad output");
    const int Sk16 = (Sk + 15) & ~15;
    const size_t shmem = ((size_t)2 * Sk16 * (head_dim + 4) + Sk16) * sizeof(float);
    if (head_dim == 64) return launch<t5_attn_fwd_kernel<64, false>>("gamer_t5_attn_fwd", dim3(B * H), dim3(T5_THREADS), shmem, ST(stream), a, o, ldo, lse);
    return launch<t5_attn_fwd_kernel<32, false>>("gamer_t5_attn_fwd", dim3(B * H), dim3(T5_THREADS), shmem, ST(stream), a, o, ldo, lse);
}

extern "C" int gamer_t5_attn_bwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* rel,
                                 const uint8_t* keep, int B, int Sq, int Sk, int H, int head_dim, int causal, float p_drop, uint64_t seed,
                                 const float* d_o, int ldo, const float* lse, float* dq, int lddq, float* dk, int lddk, float* dv, int lddv,
                                 float* drel_partial, int n_slab, void* stream) {
    T5Args a;
    GAMER_TRY(t5_args("gamer_t5_attn_bwd", a, q, ldq, k, ldk, v, ldv, rel, keep, B, Sq, Sk, H, head_dim, causal, p_drop, seed, T5_MAX_S));
    GAMER_CHECK_ARG(d_o && lse && dq && dk && dv, "gamer_t5_attn_bwd: null pointer");
    GAMER_CHECK_ARG(ldo >= H * head_dim && lddq >= H * head_dim && lddk >= H * head_dim &&
                        lddv >= H * head_dim,
                    "gamer_t5_attn_bwd: bad leading dims");
    GAMER_CHECK_ARG(n_slab > 0 && n_slab <= B, "gamer_t5_attn_bwd: n_slab=%d (1 .. B: every slab is written by its workgroup)", n_slab);
    GAMER_CHECK_ARG(!rel == !drel_partial, "gamer_t5_attn_bwd: drel_partial goes with the bias");
    const int Sk16 = (Sk + 15) & ~15, Sq16 = (Sq + 15) & ~15;
    const size_t shmem = ((size_t)2 * Sk16 * (head_dim + 4) + (size_t)Sq16 * t5_ldp(Sk16) + Sk16) * sizeof(float);
    GAMER_CHECK_ARG(shmem <= T5_LDS_MAX, "gamer_t5_attn_bwd: %zu bytes of LDS", shmem);
    if (head_dim == 64)
        return launch<t5_attn_bwd_kernel<64, false>>("gamer_t5_attn_bwd", dim3(n_slab * H), dim3(T5_THREADS), shmem, ST(stream), a, d_o, ldo, lse, dq,
                                              lddq, dk, lddk, dv, lddv, drel_partial, n_slab);
    return launch<t5_attn_bwd_kernel<32, false>>("gamer_t5_attn_bwd", dim3(n_slab * H), dim3(T5_THREADS), shmem, ST(stream), a, d_o, ldo, lse, dq, lddq,
                                          dk, lddk, dv, lddv, drel_partial, n_slab);
}

// ---- the packed forms: rows of q_start[b + 1] - q_start[b] queries and k_start[b + 1] - k_start[b] keys, no padding tokens ----------------
extern "C" int gamer_t5_attn_packed_fwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* rel,
                                        const int32_t* q_start, const int32_t* k_start, const int32_t* q_start_host,
                                        const int32_t* k_start_host, const int32_t* kv_rows, int B, int kv_batch, int max_sq, int max_sk,
                                        int H, int head_dim, int causal, float p_drop, uint64_t seed, float* o, int ldo, float* lse,
                                        void* stream) {
    const char* name = "gamer_t5_attn_packed_fwd";
    T5Args a;
    GAMER_TRY(t5_packed_args(name, a, q, ldq, k, ldk, v, ldv, rel, q_start, k_start, q_start_host, k_start_host, B, kv_rows ? kv_batch : B,
                             max_sq, max_sk, H, head_dim, causal, p_drop, seed, T5_MAX_S));
    a.kv_rows = kv_rows;
    GAMER_CHECK_ARG(o && lse && ldo >= H * head_dim, "%s: bad output", name);
    const int Sk16 = (max_sk + 15) & ~15;
    const size_t shmem = ((size_t)2 * Sk16 * (head_dim + 4) + Sk16) * sizeof(float);
    if (head_dim == 64) return launch<t5_attn_fwd_kernel<64, true>>(name, dim3(B * H), dim3(T5_THREADS), shmem, ST(stream), a, o, ldo, lse);
    return launch<t5_attn_fwd_kernel<32, true>>(name, dim3(B * H), dim3(T5_THREADS), shmem, ST(stream), a, o, ldo, lse);
}

extern "C" int gamer_t5_attn_packed_bwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* rel,
                                        const int32_t* q_start, const int32_t* k_start, const int32_t* q_start_host,
                                        const int32_t* k_start_host, int B, int max_sq, int max_sk, int H, int head_dim, int causal,
                                        float p_drop, uint64_t seed, const float* d_o, int ldo, const float* lse, float* dq, int lddq,
                                        float* dk, int lddk, float* dv, int lddv, float* drel_partial, int n_slab, void* stream) {
    const char* name = "gamer_t5_attn_packed_bwd";
    T5Args a;
    GAMER_TRY(t5_packed_args(name, a, q, ldq, k, ldk, v, ldv, rel, q_start, k_start, q_start_host, k_start_host, B, B, max_sq, max_sk, H,
                             head_dim, causal, p_drop, seed, T5_MAX_S));
    GAMER_CHECK_ARG(d_o && lse && dq && dk && dv, "%s: null pointer", name);
    GAMER_CHECK_ARG(ldo >= H * head_dim && lddq >= H * head_dim && lddk >= H * head_dim && lddv >= H * head_dim, "%s: bad leading dims", name);
    GAMER_CHECK_ARG(n_slab > 0 && n_slab <= B, "%s: n_slab=%d (1 .. B: every slab is written by its workgroup)", name, n_slab);
    GAMER_CHECK_ARG(!rel == !drel_partial, "%s: drel_partial goes with the bias", name);
    const int Sk16 = (max_sk + 15) & ~15, Sq16 = (max_sq + 15) & ~15;
    const size_t shmem = ((size_t)2 * Sk16 * (head_dim + 4) + (size_t)Sq16 * t5_ldp(Sk16) + Sk16) * sizeof(float);
    GAMER_CHECK_ARG(shmem <= T5_LDS_MAX, "%s: %zu bytes of LDS", name, shmem);
    if (head_dim == 64)
        return launch<t5_attn_bwd_kernel<64, true>>(name, dim3(n_slab * H), dim3(T5_THREADS), shmem, ST(stream), a, d_o, ldo, lse, dq, lddq, dk,
                                                    lddk, dv, lddv, drel_partial, n_slab);
    return launch<t5_attn_bwd_kernel<32, true>>(name, dim3(n_slab * H), dim3(T5_THREADS), shmem, ST(stream), a, d_o, ldo, lse, dq, lddq, dk, lddk,
                                                dv, lddv, drel_partial, n_slab);
}

extern "C" int gamer_t5_bias_expand(const float* table, const int32_t* bucket, int num_buckets, int H, int R, float* rel, void* stream) {
    GAMER_CHECK_ARG(table && bucket && rel && num_buckets > 0 && H > 0 && H <= T5_MAX_H && R > 0 && R < 2 * T5_BIAS_MAX_S,
                    "gamer_t5_bias_expand: bad arguments (num_buckets=%d H=%d offsets=%d)", num_buckets, H, R);
    return launch<t5_bias_expand_kernel>("gamer_t5_bias_expand", dim3((H * R + T5_THREADS - 1) / T5_THREADS), dim3(T5_THREADS), 0, ST(stream),
                                         table, bucket, num_buckets, H, R, rel);
}

extern "C" int gamer_t5_bias_fold(const float* drel_partial, int n_layers, int n_slab, int H, int R, const int32_t* bucket, int num_buckets,
                                  float* dtable, void* stream) {
    GAMER_CHECK_ARG(drel_partial && bucket && dtable && n_layers > 0 && n_slab > 0 && num_buckets > 0 && H > 0 && H <= T5_MAX_H && R > 0 &&
                        R < 2 * T5_BIAS_MAX_S && (int64_t)num_buckets * H < (1LL << 24),
                    "gamer_t5_bias_fold: bad arguments (layers=%d slabs=%d num_buckets=%d H=%d offsets=%d)", n_layers, n_slab, num_buckets, H, R);
    return launch<t5_bias_fold_kernel>("gamer_t5_bias_fold", dim3(num_buckets * H), dim3(WAVE), 0, ST(stream), drel_partial, n_layers, n_slab, H, R,
                                       bucket, dtable);
}
