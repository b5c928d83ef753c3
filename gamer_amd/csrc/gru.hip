// GRU recurrence of GRU4Rec (ref:SeqRec/models/discriminative/GRU4Rec/model.py: nn.GRU(bias=False, batch_first=True)).
//   gamer_gru_fwd   all L steps of one layer in one launch: r = sigma(gi_r + W_hr h), z = sigma(gi_z + W_hz h),
//                   n = tanh(gi_n + r (W_hn h)), h' = (1 - z) n + z h, from h_{-1} = 0 (PyTorch's gate order r, z, n)
//   gamer_gru_bwd   all L steps backwards in one launch: dgi, and dgh shifted one step for the dW_hh GEMM
// The input projection gi = x W_ih^T and the weight / input gradients are GEMMs over B L rows outside (gamer_amd/gru4rec.py).
//
// Batch rows are independent: a workgroup carries GRU_ROWS = 16 rows (one MFMA M tile) through every step, with no grid barrier.
// Wave w owns hidden units [16 w, 16 w + 16); lane l = (q = l >> 4, c = l & 15) owns rows 4 q + i (i = 0..3) of unit 16 w + c, the
// C/D layout of v_mfma_f32_16x16x4_f32, so a lane finishes its gates with no data exchange.  Per step:
//   forward   [16, H] h_{t-1} (LDS) x W_hh^T [H, 3H] -> the wave's three 16 x 16 tiles (r, z, n), K = H
//   backward  [16, 3H] dgh_t (LDS) x W_hh [3H, H] -> the wave's 16 x 16 tile of dh_{t-1}, K = 3H (three gate chains, summed)
// h_t / dgh_t go through LDS, double-buffered: one barrier per step.  Row stride H + 4 (3H + 4) floats: the 16 x 4 lanes of one
// A-operand read hit 64 different banks.  For H <= 128 the wave keeps its 3 x 16 rows (columns) of W_hh in registers, 3 H / 4
// per lane (96 at H = 128, 8 waves: 2 per SIMD); for H > 128 that does not fit, and the operand is read from W_hh (L2) every step.
// fp32 end to end: the products are exact fp32 fma chains (MFMA), the gates use expf / tanhf.  No atomics: the same bits on every
// call, and a row's values do not depend on which other rows share its workgroup.
//
// lens (optional, int64 [B]): a row block stops after its longest row (outputs past seq_len - 1 are never read); h is zero past
// that step, and the backward ignores dy at t >= lens[row] (so dgi, dgh are exactly zero there).
//
// Bound (MI355X: fp32 MFMA 157 TFLOP/s, 256 CUs): 6 B H^2 L FLOP per direction in the recurrence - 8.1 GFLOP forward at B = 4096,
// H = 128, L = 20, 52 us at peak with one workgroup per CU; the L dependent steps (a barrier and an MFMA chain of H / 4 each)
// make it latency-bound.  DESIGN.md section 10d.
#include "common.h"

namespace gamer {

#define ST(s) ((hipStream_t)(s))
constexpr int GRU_ROWS = 16;
constexpr int GRU_WREG_MAX_WAVES = 8;        // H <= 128: W_hh in registers

__device__ __forceinline__ float gru_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// the longest row of the block (rows >= B excluded), clamped to [0, L]; L without lens
__device__ __forceinline__ int gru_block_len(const int64_t* __restrict__ lens, int B, int L, int b0) {
    if (!lens) return L;
    int64_t m = 0;
    for (int i = 0; i < GRU_ROWS && b0 + i < B; ++i) m = max(m, lens[b0 + i]);
    return (int)min(m, (int64_t)L);
}

// zero rows [b0, b0 + 16) (< B) of a [B][L][n] tensor at steps [t0, L)
__device__ __forceinline__ void gru_zero_tail(float* __restrict__ p, int B, int L, int n, int b0, int t0, int nthreads) {
    if (t0 >= L) return;
    const int per_row = (L - t0) * n;
    for (int i = 0; i < GRU_ROWS && b0 + i < B; ++i) {
        float* row = p + ((int64_t)(b0 + i) * L + t0) * n;
        for (int e = threadIdx.x; e < per_row; e += nthreads) row[e] = 0.f;
    }
}

template <int NW>
__global__ void __launch_bounds__(NW * 64)
gru_fwd_kernel(const float* __restrict__ gi, const float* __restrict__ W, const int64_t* __restrict__ lens, int B, int L,
               float* __restrict__ hseq, float* __restrict__ gates) {
    constexpr int H = 16 * NW, KS = H / 4, LD = H + 4, NT = NW * 64;
    constexpr bool WREG = NW <= GRU_WREG_MAX_WAVES;
    constexpr int UNROLL = WREG ? KS : 4;              // (streamed operands: a full unroll hoists every load and spills)
    __shared__ float lds[2][GRU_ROWS * LD];
    const int lane = threadIdx.x & 63, q = lane >> 4, c = lane & 15, u = 16 * (threadIdx.x >> 6) + c;
    const int b0 = blockIdx.x * GRU_ROWS;
    const int Lb = gru_block_len(lens, B, L, b0);
    // B operand of gate g, k step kk: W_hh^T[4 kk + q][u] = W[g H + u][4 kk + q]
    const float* wr = W + (int64_t)u * H + q;
    float w[WREG ? 3 * KS : 1];
    if constexpr (WREG) {
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) w[g * KS + kk] = wr[(int64_t)g * H * H + 4 * kk];
    }
    for (int e = threadIdx.x; e < GRU_ROWS * LD; e += NT) lds[0][e] = 0.f;          // h_{-1} = 0
    gru_zero_tail(hseq, B, L, H, b0, Lb, NT);
    float hp[4] = {0.f, 0.f, 0.f, 0.f};
    __syncthreads();
    for (int t = 0; t < Lb; ++t) {
        const float* hl = lds[t & 1];
        float xr[4], xz[4], xn[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = b0 + 4 * q + i;
            const float* g = gi + ((int64_t)row * L + t) * (3 * H) + u;
            xr[i] = row < B ? g[0] : 0.f;
            xz[i] = row < B ? g[H] : 0.f;
            xn[i] = row < B ? g[2 * H] : 0.f;
        }
        f32x4v ar = {0.f, 0.f, 0.f, 0.f}, az = ar, an = ar;
#pragma unroll UNROLL
        for (int kk = 0; kk < KS; ++kk) {
            const float a = hl[c * LD + 4 * kk + q];
            float w0, w1, w2;
            if constexpr (WREG) {
                w0 = w[kk], w1 = w[KS + kk], w2 = w[2 * KS + kk];
            } else {
                w0 = wr[4 * kk], w1 = wr[(int64_t)H * H + 4 * kk], w2 = wr[(int64_t)2 * H * H + 4 * kk];
            }
            ar = __builtin_amdgcn_mfma_f32_16x16x4f32(a, w0, ar, 0, 0, 0);
            az = __builtin_amdgcn_mfma_f32_16x16x4f32(a, w1, az, 0, 0, 0);
            an = __builtin_amdgcn_mfma_f32_16x16x4f32(a, w2, an, 0, 0, 0);
        }
        float* hn = lds[(t + 1) & 1];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int rl = 4 * q + i, row = b0 + rl;
            const float r = gru_sigmoid(xr[i] + ar[i]);
            const float z = gru_sigmoid(xz[i] + az[i]);
            const float n = tanhf(xn[i] + r * an[i]);
            const float h = (1.f - z) * n + z * hp[i];
            hp[i] = h;
            hn[rl * LD + u] = h;
            if (row < B) {
                const int64_t pos = (int64_t)row * L + t;
                hseq[pos * H + u] = h;
                if (gates) {
                    float* gs = gates + pos * (4 * H) + u;
                    gs[0] = r;
                    gs[H] = z;
                    gs[2 * H] = n;
                    gs[3 * H] = an[i];
                }
            }
        }
        __syncthreads();
    }
}

template <int NW>
__global__ void __launch_bounds__(NW * 64)
gru_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ hseq, const float* __restrict__ gates,
               const float* __restrict__ W, const int64_t* __restrict__ lens, int B, int L, float* __restrict__ dgi,
               float* __restrict__ dghs) {
    constexpr int H = 16 * NW, KG = H / 4, LD = 3 * H + 4, NT = NW * 64;
    constexpr bool WREG = NW <= GRU_WREG_MAX_WAVES;
    constexpr int UNROLL = WREG ? KG : 4;
    __shared__ float lds[2][GRU_ROWS * LD];
    const int lane = threadIdx.x & 63, q = lane >> 4, c = lane & 15, u = 16 * (threadIdx.x >> 6) + c;
    const int b0 = blockIdx.x * GRU_ROWS;
    const int Lb = gru_block_len(lens, B, L, b0);
    // B operand of gate block g, k step kk: W[g H + 4 kk + q][u]
    const float* wc = W + (int64_t)q * H + u;
    float w[WREG ? 3 * KG : 1];
    if constexpr (WREG) {
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int kk = 0; kk < KG; ++kk) w[g * KG + kk] = wc[(int64_t)(g * H + 4 * kk) * H];
    }
    gru_zero_tail(dgi, B, L, 3 * H, b0, Lb, NT);
    gru_zero_tail(dghs, B, L, 3 * H, b0, Lb > 0 ? Lb - 1 : 0, NT);
    int len[4];
    float dh[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = b0 + 4 * q + i;
        len[i] = row >= B ? 0 : (lens ? (int)min(lens[row], (int64_t)L) : L);
        dh[i] = 0.f;
    }
    for (int t = Lb - 1; t >= 0; --t) {
        float* gl = lds[t & 1];
        float dhz[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int rl = 4 * q + i, row = b0 + rl;
            const int64_t pos = (int64_t)row * L + t;
            float d = dh[i], r = 0.f, z = 0.f, n = 0.f, hn = 0.f, hprev = 0.f;
            if (row < B) {
                if (t < len[i]) d += dy[pos * H + u];
                const float* gs = gates + pos * (4 * H) + u;
                r = gs[0];
                z = gs[H];
                n = gs[2 * H];
                hn = gs[3 * H];
                hprev = t > 0 ? hseq[(pos - 1) * H + u] : 0.f;
            }
            const float dnp = d * (1.f - z) * (1.f - n * n);               // d(gi_n + r hn)
            const float drp = dnp * hn * r * (1.f - r);                     // d(gi_r + W_hr h)
            const float dzp = d * (hprev - n) * z * (1.f - z);              // d(gi_z + W_hz h)
            dhz[i] = d * z;
            gl[rl * LD + u] = drp;
            gl[rl * LD + H + u] = dzp;
            gl[rl * LD + 2 * H + u] = dnp * r;                              // d(W_hn h)
            if (row < B) {
                float* o = dgi + pos * (3 * H) + u;
                o[0] = drp;
                o[H] = dzp;
                o[2 * H] = dnp;
                if (t > 0) {
                    float* s = dghs + (pos - 1) * (3 * H) + u;
                    s[0] = drp;
                    s[H] = dzp;
                    s[2 * H] = dnp * r;
                }
            }
        }
        __syncthreads();
        if (t == 0) break;
        f32x4v a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0;
#pragma unroll UNROLL
        for (int kk = 0; kk < KG; ++kk) {
            const float* ar = gl + c * LD + 4 * kk + q;
            float w0, w1, w2;
            if constexpr (WREG) {
                w0 = w[kk], w1 = w[KG + kk], w2 = w[2 * KG + kk];
            } else {
                w0 = wc[(int64_t)(4 * kk) * H], w1 = wc[(int64_t)(H + 4 * kk) * H], w2 = wc[(int64_t)(2 * H + 4 * kk) * H];
            }
            a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[0], w0, a0, 0, 0, 0);
            a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[H], w1, a1, 0, 0, 0);
            a2 = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[2 * H], w2, a2, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) dh[i] = dhz[i] + ((a0[i] + a1[i]) + a2[i]);
    }
}

static int gru_shape_ok(const char* name, int B, int L, int H) {
    GAMER_CHECK_ARG(B > 0 && L > 0 && H >= 16 && H <= 256 && H % 16 == 0 && (int64_t)B * L * 4 * H < ((int64_t)1 << 40),
                    "%s: bad shape B=%d L=%d H=%d (H %% 16 == 0, 16 <= H <= 256)", name, B, L, H);
    return 0;
}

#define GRU_DISPATCH(NW_, KERNEL, GRID, ...)                                                                           \
    do {                                                                                                                \
        switch (NW_) {                                                                                                  \
            case 1: hipLaunchKernelGGL(KERNEL<1>, GRID, dim3(64), 0, st, __VA_ARGS__); break;                           \
            case 2: hipLaunchKernelGGL(KERNEL<2>, GRID, dim3(128), 0, st, __VA_ARGS__); break;                          \
            case 3: hipLaunchKernelGGL(KERNEL<3>, GRID, dim3(192), 0, st, __VA_ARGS__); break;                          \
            case 4: hipLaunchKernelGGL(KERNEL<4>, GRID, dim3(256), 0, st, __VA_ARGS__); break;                          \
            case 5: hipLaunchKernelGGL(KERNEL<5>, GRID, dim3(320), 0, st, __VA_ARGS__); break;                          \
            case 6: hipLaunchKernelGGL(KERNEL<6>, GRID, dim3(384), 0, st, __VA_ARGS__); break;                          \
            case 7: hipLaunchKernelGGL(KERNEL<7>, GRID, dim3(448), 0, st, __VA_ARGS__); break;                          \
            case 8: hipLaunchKernelGGL(KERNEL<8>, GRID, dim3(512), 0, st, __VA_ARGS__); break;                          \
            case 9: hipLaunchKernelGGL(KERNEL<9>, GRID, dim3(576), 0, st, __VA_ARGS__); break;                          \
            case 10: hipLaunchKernelGGL(KERNEL<10>, GRID, dim3(640), 0, st, __VA_ARGS__); break;                        \
            case 11: hipLaunchKernelGGL(KERNEL<11>, GRID, dim3(704), 0, st, __VA_ARGS__); break;                        \
            case 12: hipLaunchKernelGGL(KERNEL<12>, GRID, dim3(768), 0, st, __VA_ARGS__); break;                        \
            case 13: hipLaunchKernelGGL(KERNEL<13>, GRID, dim3(832), 0, st, __VA_ARGS__); break;                        \
            case 14: hipLaunchKernelGGL(KERNEL<14>, GRID, dim3(896), 0, st, __VA_ARGS__); break;                        \
            case 15: hipLaunchKernelGGL(KERNEL<15>, GRID, dim3(960), 0, st, __VA_ARGS__); break;                        \
            default: hipLaunchKernelGGL(KERNEL<16>, GRID, dim3(1024), 0, st, __VA_ARGS__); break;                       \
        }                                                                                                               \
    } while (0)

}  // namespace gamer

using namespace gamer;

extern "C" int64_t gamer_gru_gates_floats(int B, int L, int H) {
    if (B <= 0 || L <= 0 || H <= 0) return -1;
    return (int64_t)B * L * 4 * H;
}

extern "C" int gamer_gru_fwd(const float* gi, const float* w_hh, const int64_t* lens, int B, int L, int H, float* h, float* gates,
                             void* stream) {
    GAMER_CHECK_ARG(gi && w_hh && h, "gamer_gru_fwd: null pointer");
    if (gru_shape_ok("gamer_gru_fwd", B, L, H)) return -1;
    hipStream_t st = ST(stream);
    GRU_DISPATCH(H / 16, gru_fwd_kernel, dim3((B + GRU_ROWS - 1) / GRU_ROWS), gi, w_hh, lens, B, L, h, gates);
    GAMER_CHECK_LAUNCH("gamer_gru_fwd");
    return 0;
}

extern "C" int gamer_gru_bwd(const float* dy, const float* h, const float* gates, const float* w_hh, const int64_t* lens, int B, int L,
                             int H, float* dgi, float* dgh_next, void* stream) {
    GAMER_CHECK_ARG(dy && h && gates && w_hh && dgi && dgh_next, "gamer_gru_bwd: null pointer");
    if (gru_shape_ok("gamer_gru_bwd", B, L, H)) return -1;
    hipStream_t st = ST(stream);
    GRU_DISPATCH(H / 16, gru_bwd_kernel, dim3((B + GRU_ROWS - 1) / GRU_ROWS), dy, h, gates, w_hh, lens, B, L, dgi, dgh_next);
    GAMER_CHECK_LAUNCH("gamer_gru_bwd");
    return 0;
}
