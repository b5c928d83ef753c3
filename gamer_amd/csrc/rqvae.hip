// Residual quantiser of the RQ-VAE item tokenizer (ref:SeqRec/models/tokenizer/RQVAE/{vector_quantizer,resiual_vector_quantizer}.py).
//   gamer_rvq_fwd   levels [level_begin, level_end) of the residual quantiser in one launch: per level the squared distances
//                   d = |r|^2 + |e|^2 - 2 r.e (the reference's expanded form, fp32 FMA chains), the argmin (lowest index on a tie)
//                   or an index handed in (mode 1), x_res = r + (e - r), x_q += x_res, r -= x_res, and the row sum of |e - r|^2
//   gamer_rvq_bwd   dz and dE of  sum_l g_l (mse(e, sg r) + mu mse(sg e, r)) + <g_xq, x_q>  from the saved indices and residuals
//
// Forward layout.  A workgroup of 256 threads carries RVQ_ROWS = 16 rows through every level of the call; a row belongs to 16
// consecutive lanes of one wave.  Each of the 16 lanes keeps the WHOLE residual and running sum of its row in registers (D <= 64:
// 2 x 16 float4) from one level to the next and scores the codes k = lane, lane + 16, ... of the level: the 16 lanes of a row read
// 16 different codes, the four rows of a wave read the same 16 (LDS broadcast).  A level's codebook is staged in LDS as [code][LD]
// with LD = D + 4 floats when D / 4 is even (D when odd): LD / 4 odd makes the 16 ds_read_b128 addresses of a lane group fall on
// 16 different 4-bank slots.  |e|^2 is computed once per staged code.  A codebook larger than the 64 KiB the kernel takes (K = 1024
// at D = 64 is 256 KiB, more than a CU has) is staged in chunks of whole codes; the running minimum goes across the chunks.
// The argmin of a row is a 4-step xor butterfly over its 16 lanes on (d, index) - smaller d, then smaller index -, so the result
// does not depend on which lane saw a code.  The chosen code is read back from global memory (the 16 lanes read one address).
//
// Fixed-order sums, no float atomics: |r|^2, |e|^2 and r.e are four fp32 FMA chains (one per float4 component) summed as
// (x + y) + (z + w); |e - r|^2 of a row is one fp64 FMA chain over D; a workgroup adds its 16 rows in row order (fp64) into the fp32
// loss_partial[block][level]; rvq_loss_reduce_kernel (one wave per level) adds the partials lane-strided and then by the xor
// butterfly, in fp64, and rounds once.  The same input gives the same bits on every call, and a row's outputs do not depend on the other rows.
//
// Backward layout.  dE is a scatter of rows into codes, done in a fixed order: one wave per (level, code) scans idx[:, level] 64 rows
// at a time (ballot), and adds scale_l (e - r_l[row]) for the rows that chose the code in row order (an fp64 sum), lane = column.  A code nobody
// chose gets exact zeros.  The remaining workgroups write dz = g_xq + mu scale_0 (r_0 - e_0) per element: x_res = r + sg(e - r) has an
// identity gradient into r, so r_{l+1} = r_l - x_res_l carries none back, and only level 0's commitment term reaches z.
#include "common.h"

namespace gamer {

#define ST(s) ((hipStream_t)(s))
constexpr int RVQ_MAX_LEVELS = 8, RVQ_MAX_D = 64, RVQ_MAX_K = 1024;
constexpr int RVQ_LPR = 16;                                    // lanes per row
constexpr int RVQ_THREADS = 256, RVQ_ROWS = RVQ_THREADS / RVQ_LPR;
constexpr int RVQ_LDS_BYTES = 64 * 1024;

struct RvqFwdArgs {
    const float* r;
    int64_t ldr;
    const float* E;
    int32_t* idx;
    float* xq;
    float* res;
    float* r_levels;
    float* dist;
    float* loss_partial;
    int off[RVQ_MAX_LEVELS + 1];
    int mode[RVQ_MAX_LEVELS];
    int n_levels, lvl0, lvl1, B, D, kc, ld;
};

// four FMA chains, one per component (independent: they issue back to back), summed as (x + y) + (z + w)
__device__ __forceinline__ void rvq_fma4(float4& acc, const float4 a, const float4 b) {
    acc.x = fmaf(a.x, b.x, acc.x);
    acc.y = fmaf(a.y, b.y, acc.y);
    acc.z = fmaf(a.z, b.z, acc.z);
    acc.w = fmaf(a.w, b.w, acc.w);
}
__device__ __forceinline__ float rvq_sum4(const float4 v) { return (v.x + v.y) + (v.z + v.w); }

// a row's D values leave from the first of its 16 lanes (every lane holds the same values)
template <int DV>
__device__ __forceinline__ void rvq_store_row(float* __restrict__ dst, const float4 (&v)[DV], int dv) {
#pragma unroll
    for (int i = 0; i < DV; ++i)
        if (i < dv) *reinterpret_cast<float4*>(dst + 4 * i) = v[i];
}

template <int DV>
__global__ void __launch_bounds__(RVQ_THREADS) rvq_fwd_kernel(RvqFwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) char rvq_smem[];
    const int D = a.D, dv = D >> 2, LD = a.ld;
    float* cb = reinterpret_cast<float*>(rvq_smem);            // [kc][LD]
    float* en = cb + (size_t)a.kc * LD;                        // [kc]
    double* rowsq = reinterpret_cast<double*>(en + a.kc);      // [RVQ_ROWS][RVQ_MAX_LEVELS] (kc % 16 == 0: 8-byte aligned)
    const int tid = threadIdx.x, sub = tid & (RVQ_LPR - 1), rl = tid / RVQ_LPR;
    const int64_t row = (int64_t)blockIdx.x * RVQ_ROWS + rl;
    const bool live = row < a.B;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 r[DV], xq[DV];
#pragma unroll
    for (int i = 0; i < DV; ++i) {
        const bool in = live && i < dv;
        r[i] = in ? *reinterpret_cast<const float4*>(a.r + row * a.ldr + 4 * i) : zero4;
        xq[i] = in && a.lvl0 > 0 ? *reinterpret_cast<const float4*>(a.xq + row * D + 4 * i) : zero4;
    }
    for (int l = a.lvl0; l < a.lvl1; ++l) {
        const int K = a.off[l + 1] - a.off[l];
        const float* __restrict__ El = a.E + (int64_t)a.off[l] * D;
        const bool dist_only = a.dist != nullptr && l == a.lvl1 - 1;
        if (a.r_levels && live && sub == 0) rvq_store_row<DV>(a.r_levels + ((int64_t)l * a.B + row) * D, r, dv);
        int bidx = 0;
        if (a.mode[l] == 0 || dist_only) {
            float4 rn4 = zero4;
#pragma unroll
            for (int i = 0; i < DV; ++i)
                if (i < dv) rvq_fma4(rn4, r[i], r[i]);
            const float rn = rvq_sum4(rn4);
            float best = __builtin_inff();
            bidx = 0x7fffffff;
            for (int k0 = 0; k0 < K; k0 += a.kc) {
                const int kn = min(a.kc, K - k0);
                __syncthreads();                                               // the previous chunk (or level) is read
                for (int c = rl; c < kn; c += RVQ_ROWS)
                    if (sub < dv)
                        *reinterpret_cast<float4*>(cb + (size_t)c * LD + 4 * sub) =
                            *reinterpret_cast<const float4*>(El + (int64_t)(k0 + c) * D + 4 * sub);
                __syncthreads();
                for (int c = tid; c < kn; c += RVQ_THREADS) {
                    const float* e = cb + (size_t)c * LD;
                    float4 s = zero4;
                    for (int i = 0; i < dv; ++i) {
                        const float4 v = *reinterpret_cast<const float4*>(e + 4 * i);
                        rvq_fma4(s, v, v);
                    }
                    en[c] = rvq_sum4(s);
                }
                __syncthreads();
                for (int c = sub; c < kn; c += RVQ_LPR) {
                    const float* e = cb + (size_t)c * LD;
                    float4 dot = zero4;
#pragma unroll
                    for (int i = 0; i < DV; ++i)
                        if (i < dv) rvq_fma4(dot, r[i], *reinterpret_cast<const float4*>(e + 4 * i));
                    const float d = (rn + en[c]) - 2.f * rvq_sum4(dot);
                    if (dist_only && live) a.dist[row * K + k0 + c] = d;
                    if (d < best) {
                        best = d;
                        bidx = k0 + c;
                    }
                }
            }
            if (dist_only) break;
#pragma unroll
            for (int o = 1; o < RVQ_LPR; o <<= 1) {
                const float od = __shfl_xor(best, o, 64);
                const int oi = __shfl_xor(bidx, o, 64);
                if (od < best || (od == best && oi < bidx)) {
                    best = od;
                    bidx = oi;
                }
            }
            if (bidx >= K) bidx = 0;                                           // every distance NaN
        } else {
            bidx = live ? a.idx[row * a.n_levels + l] : 0;
        }
        bidx = min(max(bidx, 0), K - 1);
        const float* __restrict__ ec = El + (int64_t)bidx * D;
        double sq = 0.0;                                                       // (fp64: the row's sum is rounded once)
#pragma unroll
        for (int i = 0; i < DV; ++i)
            if (i < dv) {
                const float4 e = *reinterpret_cast<const float4*>(ec + 4 * i);
                float4 df = make_float4(e.x - r[i].x, e.y - r[i].y, e.z - r[i].z, e.w - r[i].w);
                sq = fma((double)df.x, (double)df.x, sq);
                sq = fma((double)df.y, (double)df.y, sq);
                sq = fma((double)df.z, (double)df.z, sq);
                sq = fma((double)df.w, (double)df.w, sq);
                df = make_float4(r[i].x + df.x, r[i].y + df.y, r[i].z + df.z, r[i].w + df.w);      // x_res = r + (e - r)
                xq[i] = make_float4(xq[i].x + df.x, xq[i].y + df.y, xq[i].z + df.z, xq[i].w + df.w);
                r[i] = make_float4(r[i].x - df.x, r[i].y - df.y, r[i].z - df.z, r[i].w - df.w);
            }
        if (sub == 0) {
            rowsq[rl * RVQ_MAX_LEVELS + (l - a.lvl0)] = live ? sq : 0.0;
            if (live && a.mode[l] == 0) a.idx[row * a.n_levels + l] = bidx;
        }
    }
    if (live && sub == 0) {
        rvq_store_row<DV>(a.xq + row * D, xq, dv);
        rvq_store_row<DV>(a.res + row * D, r, dv);
    }
    if (a.loss_partial) {
        const int n_full = a.lvl1 - a.lvl0 - (a.dist ? 1 : 0);
        __syncthreads();
        if (tid < n_full) {
            double s = 0.0;
            for (int i = 0; i < RVQ_ROWS; ++i) s += rowsq[i * RVQ_MAX_LEVELS + tid];
            a.loss_partial[(int64_t)blockIdx.x * RVQ_MAX_LEVELS + tid] = (float)s;
        }
    }
}

// loss_sums[lvl0 + j] = the sum over workgroups of loss_partial[block][j]: lane-strided, then the xor butterfly (a fixed order)
__global__ void __launch_bounds__(WAVE) rvq_loss_reduce_kernel(const float* __restrict__ partial, int nblocks, int lvl0,
                                                               float* __restrict__ loss_sums) {
    const int j = blockIdx.x;
    double s = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += WAVE) s += (double)partial[(int64_t)b * RVQ_MAX_LEVELS + j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (threadIdx.x == 0) loss_sums[lvl0 + j] = (float)s;
}

struct RvqBwdArgs {
    const int32_t* idx;
    const float* r_levels;
    const float* E;
    const float* g_xq;
    const float* g_level;
    float* dz;
    float* dE;
    int off[RVQ_MAX_LEVELS + 1];
    int n_levels, B, D, code_blocks;
    float mu, inv_n;
};

__global__ void __launch_bounds__(RVQ_THREADS) rvq_bwd_kernel(RvqBwdArgs a) {
    const int D = a.D, tid = threadIdx.x;
    if ((int)blockIdx.x < a.code_blocks) {
        const int code = blockIdx.x * (RVQ_THREADS / WAVE) + (tid >> 6), lane = tid & 63;
        if (code >= a.off[a.n_levels]) return;
        int l = 0;
        while (code >= a.off[l + 1]) ++l;
        const int k = code - a.off[l];
        const bool col = lane < D;
        const float scale = 2.f * a.g_level[l] * a.inv_n;
        const float e = col ? a.E[(int64_t)code * D + lane] : 0.f;
        const float* __restrict__ rl = a.r_levels + (int64_t)l * a.B * D;
        double acc = 0.0;                                                      // (fp64: rounded once, when stored)
        for (int row0 = 0; row0 < a.B; row0 += WAVE) {
            const int row = row0 + lane;
            const int v = row < a.B ? a.idx[(int64_t)row * a.n_levels + l] : -1;
            unsigned long long m = __ballot(v == k);
            while (m) {
                const int j = __builtin_ctzll(m);
                m &= m - 1;
                if (col) acc = fma((double)scale, (double)(e - rl[(int64_t)(row0 + j) * D + lane]), acc);
            }
        }
        if (col) a.dE[(int64_t)code * D + lane] = (float)acc;
        return;
    }
    const int dv = D >> 2;
    const int64_t t = (int64_t)(blockIdx.x - a.code_blocks) * RVQ_THREADS + tid;
    if (t >= (int64_t)a.B * dv) return;
    const int64_t row = t / dv;
    const int c = (int)(t - row * dv) * 4;
    const int K0 = a.off[1] - a.off[0];
    const int i0 = min(max(a.idx[row * a.n_levels], 0), K0 - 1);
    const float4 e = *reinterpret_cast<const float4*>(a.E + (int64_t)(a.off[0] + i0) * D + c);
    const float4 r = *reinterpret_cast<const float4*>(a.r_levels + row * D + c);
    const float4 g = a.g_xq ? *reinterpret_cast<const float4*>(a.g_xq + row * D + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float s = a.mu * (2.f * a.g_level[0] * a.inv_n);
    *reinterpret_cast<float4*>(a.dz + row * D + c) =
        make_float4(fmaf(s, r.x - e.x, g.x), fmaf(s, r.y - e.y, g.y), fmaf(s, r.z - e.z, g.z), fmaf(s, r.w - e.w, g.w));
}

// the limits shared by both entry points; fills off[]
static int rvq_check(const char* name, const int32_t* level_offsets, int n_levels, int B, int D, int* off) {
    GAMER_CHECK_ARG(level_offsets, "%s: null pointer", name);
    GAMER_CHECK_ARG(n_levels >= 1 && n_levels <= RVQ_MAX_LEVELS, "%s: %d levels (1 to %d)", name, n_levels, RVQ_MAX_LEVELS);
    GAMER_CHECK_ARG(D >= 4 && D <= RVQ_MAX_D && D % 4 == 0, "%s: D=%d (a multiple of 4, at most %d)", name, D, RVQ_MAX_D);
    GAMER_CHECK_ARG(B >= 1 && (int64_t)B * RVQ_MAX_K < ((int64_t)1 << 40), "%s: B=%d", name, B);
    GAMER_CHECK_ARG(level_offsets[0] == 0, "%s: level_offsets[0] must be 0", name);
    for (int l = 0; l < n_levels; ++l) {
        const int K = level_offsets[l + 1] - level_offsets[l];
        GAMER_CHECK_ARG(K >= 1 && K <= RVQ_MAX_K, "%s: level %d has K=%d codes (1 to %d)", name, l, K, RVQ_MAX_K);
    }
    for (int l = 0; l <= n_levels; ++l) off[l] = level_offsets[l];
    for (int l = n_levels + 1; l <= RVQ_MAX_LEVELS; ++l) off[l] = level_offsets[n_levels];
    return 0;
}

static inline int rvq_blocks(int B) { return (B + RVQ_ROWS - 1) / RVQ_ROWS; }

}  // namespace gamer

using namespace gamer;

extern "C" int64_t gamer_rvq_ws_floats(int B) {
    if (B <= 0) return -1;
    return (int64_t)rvq_blocks(B) * RVQ_MAX_LEVELS;
}

extern "C" int gamer_rvq_fwd(const float* r, int64_t ldr, const float* codebooks, const int32_t* level_offsets, const int32_t* modes,
                             int n_levels, int level_begin, int level_end, int B, int D, int32_t* idx, float* x_q, float* residual,
                             float* r_levels, float* dist, float* loss_partial, float* loss_sums, void* stream) {
    RvqFwdArgs a = {};
    GAMER_CHECK_ARG(r && codebooks && level_offsets && modes && idx && x_q && residual, "gamer_rvq_fwd: null pointer");
    if (rvq_check("gamer_rvq_fwd", level_offsets, n_levels, B, D, a.off)) return -1;
    GAMER_CHECK_ARG(level_begin >= 0 && level_begin < level_end && level_end <= n_levels, "gamer_rvq_fwd: levels [%d, %d) of %d",
                    level_begin, level_end, n_levels);
    GAMER_CHECK_ARG(ldr >= D && ldr % 4 == 0, "gamer_rvq_fwd: row stride %lld (a multiple of 4, at least D=%d)", (long long)ldr, D);
    GAMER_CHECK_ARG(aligned16(r) && aligned16(codebooks) && aligned16(x_q) && aligned16(residual) && aligned16(r_levels),
                    "gamer_rvq_fwd: r, codebooks, x_q, residual and r_levels must be 16-byte aligned");
    GAMER_CHECK_ARG(!loss_sums == !loss_partial, "gamer_rvq_fwd: loss_sums goes with the loss_partial workspace");
    int kmax = 0;
    for (int l = 0; l < n_levels; ++l) {
        GAMER_CHECK_ARG(modes[l] == 0 || modes[l] == 1, "gamer_rvq_fwd: mode %d of level %d (0 = argmin, 1 = given index)", modes[l], l);
        a.mode[l] = modes[l];
        if (l >= level_begin && l < level_end) kmax = max(kmax, a.off[l + 1] - a.off[l]);
    }
    const int dv = D / 4;
    a.ld = 4 * (dv | 1);
    const int fixed = RVQ_ROWS * RVQ_MAX_LEVELS * (int)sizeof(double);
    const int per_code = (a.ld + 1) * (int)sizeof(float);
    a.kc = min((kmax + RVQ_LPR - 1) / RVQ_LPR * RVQ_LPR, (RVQ_LDS_BYTES - fixed) / per_code / RVQ_LPR * RVQ_LPR);
    const size_t lds = (size_t)a.kc * per_code + fixed;
    a.r = r, a.ldr = ldr, a.E = codebooks, a.idx = idx, a.xq = x_q, a.res = residual, a.r_levels = r_levels, a.dist = dist;
    a.loss_partial = loss_partial;
    a.n_levels = n_levels, a.lvl0 = level_begin, a.lvl1 = level_end, a.B = B, a.D = D;
    const dim3 grid(rvq_blocks(B)), block(RVQ_THREADS);
    if (dv <= 4) GAMER_TRY(launch<rvq_fwd_kernel<4>>("gamer_rvq_fwd", grid, block, lds, ST(stream), a));
    else if (dv <= 8) GAMER_TRY(launch<rvq_fwd_kernel<8>>("gamer_rvq_fwd", grid, block, lds, ST(stream), a));
    else GAMER_TRY(launch<rvq_fwd_kernel<16>>("gamer_rvq_fwd", grid, block, lds, ST(stream), a));
    const int n_full = level_end - level_begin - (dist ? 1 : 0);
    if (loss_sums && n_full > 0)
        GAMER_TRY(launch<rvq_loss_reduce_kernel>("gamer_rvq_fwd", dim3(n_full), dim3(WAVE), 0, ST(stream), (const float*)loss_partial,
                                                 (int)grid.x, level_begin, loss_sums));
    return 0;
}

extern "C" int gamer_rvq_bwd(const int32_t* idx, const float* r_levels, const float* codebooks, const int32_t* level_offsets,
                             int n_levels, int B, int D, const float* g_xq, const float* g_level, float mu, float* dz, float* dE,
                             void* stream) {
    RvqBwdArgs a = {};
    GAMER_CHECK_ARG(idx && r_levels && codebooks && level_offsets && g_level && dz && dE, "gamer_rvq_bwd: null pointer");
    if (rvq_check("gamer_rvq_bwd", level_offsets, n_levels, B, D, a.off)) return -1;
    GAMER_CHECK_ARG(aligned16(r_levels) && aligned16(codebooks) && aligned16(g_xq) && aligned16(dz),
                    "gamer_rvq_bwd: r_levels, codebooks, g_xq and dz must be 16-byte aligned");
    a.idx = idx, a.r_levels = r_levels, a.E = codebooks, a.g_xq = g_xq, a.g_level = g_level, a.dz = dz, a.dE = dE;
    a.n_levels = n_levels, a.B = B, a.D = D, a.mu = mu;
    a.inv_n = 1.f / ((float)B * (float)D);
    const int waves = RVQ_THREADS / WAVE;
    a.code_blocks = (a.off[n_levels] + waves - 1) / waves;
    const int64_t dz_blocks = ((int64_t)B * (D / 4) + RVQ_THREADS - 1) / RVQ_THREADS;
    return launch<rvq_bwd_kernel>("gamer_rvq_bwd", dim3((unsigned)(a.code_blocks + dz_blocks)), dim3(RVQ_THREADS), 0, ST(stream), a);
}
