// Scoring GIVEN items on the T5 backbones (gfx950): the decoder's cross attention for ANY number R of query rows per user.
//
// gamer_t5_attn_fwd (csrc/t5_attention.hip) runs one workgroup per (row, head) and stages the K / V of that row's user into LDS - the
// decoder has at most 8 query rows, so one wave works on one half-empty 16-query tile, three waves idle, and with the kv_rows map
// every beam row of a user stages that user's K / V again.  A thousand candidates per user turn that shape round, the way
// gamer_attn_candidates (csrc/candidates.hip) did for the cached decode path: one workgroup = (user, head, block of 64 query rows);
// the K and V of the (user, head) are staged ONCE per workgroup ([Sk16][d + 4], the image of the resident kernels) and each of the
// four waves owns one 16-query tile of the block.
//   semantics   gamer_t5_attn_fwd's without a bias, causality or dropout: score = q . k (no 1 / sqrt(d)), softmax over the keys with
//               keep[user][j] != 0 (nullptr: all; packed keys: all of the user's own), a row with no allowed key gives a zero context.
//               No lse output: nothing reads it.
//   arithmetic  v_mfma_f32_16x16x4_f32 through the tile helpers of t5_attention_common.h, in the resident kernel's order: S^T = K Q^T
//               with the query on lane & 15, the probabilities stay in the registers as the A operand of P V.  A query is a column of
//               its tile in every product and a lane group in every reduction, so its result depends on its own row and its user's
//               K / V only, not on the rows that share its tile or block.
//   traffic     LDS: 2 Sk16 (d + 4) floats written once per 64 query rows (the row map: once per decoder sequence of <= 8 rows).
//               HBM / L2: a (user, head)'s K / V is read by each of its ceil(R / 64) blocks, neighbours in the grid.
// No atomics: every output element is written once by one lane.
#include "t5_attention_common.h"

namespace gamer {

constexpr int T5C_MAX_S = 128, T5C_MAX_KT = T5C_MAX_S / 16;
constexpr int T5C_ROWS = 16 * T5_WAVES;                      // query rows of a workgroup: one 16-query tile per wave

template <int D, bool PK>
__global__ void __launch_bounds__(T5_THREADS)
t5_attn_candidates_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ k, int ldk, const float* __restrict__ v, int ldv,
                          const uint8_t* __restrict__ keep, const int32_t* __restrict__ k_start, int R, int Sk_dense, int H, int nblk,
                          float* __restrict__ o, int ldo) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int LD = D + 4;
    const int blk = blockIdx.x % nblk, bh = blockIdx.x / nblk;
    const int b = bh / H, hh = bh % H;
    const int64_t k0 = PK ? k_start[b] : (int64_t)b * Sk_dense;
    const int Sk = PK ? k_start[b + 1] - (int)k0 : Sk_dense;
    const int Sk16 = (Sk + 15) & ~15, nkt = Sk16 / 16;
    float* Ks = lds;                          // [Sk16][LD]
    float* Vs = Ks + Sk16 * LD;               // [Sk16][LD]
    int* kp = (int*)(Vs + Sk16 * LD);         // [Sk16]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    t5_stage<D>(Ks, k + k0 * ldk + hh * D, ldk, Sk, Sk16);
    t5_stage<D>(Vs, v + k0 * ldv + hh * D, ldv, Sk, Sk16);
    for (int j = threadIdx.x; j < Sk16; j += T5_THREADS) kp[j] = j < Sk && (PK || !keep || keep[(int64_t)b * Sk_dense + j]) ? 1 : 0;
    __syncthreads();
    const int i0 = blk * T5C_ROWS + wave * 16;                // this wave's first row of the user's R
    if (i0 >= R) return;                                      // (after the only barrier)
    const float* qb = q + (int64_t)b * R * ldq + hh * D;
    float* ob = o + (int64_t)b * R * ldo + hh * D;
    const int i = i0 + (lane & 15);
    const bool iv = i < R;
    float qr[D / 4];
    t5_row_operand<D>(qr, iv ? qb + (int64_t)i * ldq : nullptr, lane);
    f32x4v s[T5C_MAX_KT];
    float m = -INFINITY;
#pragma unroll
    for (int nt = 0; nt < T5C_MAX_KT; ++nt) {
        if (nt < nkt) {
            s[nt] = t5_tile<D>(Ks + nt * 16 * LD, qr, lane);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int j = nt * 16 + 4 * (lane >> 4) + reg;
                s[nt][reg] = iv && kp[j] ? s[nt][reg] + 0.f : -INFINITY;      // (+ 0.f: the resident kernel's sum with no bias)
                m = fmaxf(m, s[nt][reg]);
            }
        }
    }
    m = t5_xor_max(m);
    const float ms = m == -INFINITY ? 0.f : m;
    float sum = 0.f;
#pragma unroll
    for (int nt = 0; nt < T5C_MAX_KT; ++nt)
        if (nt < nkt) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) sum += expf(s[nt][reg] - ms);
        }
    sum = t5_xor_sum(sum);
    const float ls = m == -INFINITY ? 0.f : m + logf(sum);
    f32x4v acc[D / 16];
#pragma unroll
    for (int n = 0; n < D / 16; ++n) acc[n] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int nt = 0; nt < T5C_MAX_KT; ++nt)
        if (nt < nkt) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) s[nt][reg] = expf(s[nt][reg] - ls);      // (a key that is not allowed: exp(-inf) = 0)
            t5_tile_out<D>(acc, s[nt], Vs + nt * 16 * LD, lane);
        }
    t5_store_rows<D>(ob, ldo, i0, R, acc, lane);
}

}  // namespace gamer

using namespace gamer;

extern "C" int gamer_t5_attn_candidates(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const uint8_t* keep,
                                        const int32_t* k_start, const int32_t* k_start_host, int B, int R, int Sk, int H, int head_dim,
                                        float* o, int ldo, void* stream) {
    const char* name = "gamer_t5_attn_candidates";
    GAMER_CHECK_ARG(q && k && v && o, "%s: null pointer", name);
    GAMER_CHECK_ARG(B > 0 && R > 0 && Sk > 0 && Sk <= T5C_MAX_S && H > 0 && H <= T5_MAX_H && (head_dim == 32 || head_dim == 64),
                    "%s: bad shape B=%d R=%d Sk=%d H=%d head_dim=%d (Sk <= %d, H <= %d, head_dim 32 or 64)", name, B, R, Sk, H, head_dim,
                    T5C_MAX_S, T5_MAX_H);
    const int I = H * head_dim;
    GAMER_CHECK_ARG(ldq >= I && ldk >= I && ldv >= I && ldo >= I && ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && aligned16(q) &&
                        aligned16(k) && aligned16(v),
                    "%s: bad leading dims (>= H head_dim, multiples of 4, 16-byte aligned bases)", name);
    GAMER_CHECK_ARG(!k_start == !k_start_host, "%s: k_start goes with its host copy", name);
    GAMER_CHECK_ARG(!(k_start && keep), "%s: packed keys take no keep (every key of a packed row is real)", name);
    if (k_start) GAMER_TRY(t5_offsets(name, "k_start", k_start_host, B, Sk));
    const int64_t nblk = ((int64_t)R + T5C_ROWS - 1) / T5C_ROWS;
    const int64_t blocks = (int64_t)B * H * nblk;
    GAMER_CHECK_ARG(blocks <= 0x7fffffff && (int64_t)B * R <= 0x7fffffff, "%s: B * R = %lld rows are too many", name, (long long)B * R);
    const int Sk16 = (Sk + 15) & ~15;
    const size_t shmem = ((size_t)2 * Sk16 * (head_dim + 4) + Sk16) * sizeof(float);
    const dim3 grid((unsigned)blocks), block(T5_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (k_start) {
        if (head_dim == 64)
            return launch<t5_attn_candidates_kernel<64, true>>(name, grid, block, shmem, st, q, ldq, k, ldk, v, ldv, keep, k_start, R, Sk, H,
                                                               (int)nblk, o, ldo);
        return launch<t5_attn_candidates_kernel<32, true>>(name, grid, block, shmem, st, q, ldq, k, ldk, v, ldv, keep, k_start, R, Sk, H,
                                                           (int)nblk, o, ldo);
    }
    if (head_dim == 64)
        return launch<t5_attn_candidates_kernel<64, false>>(name, grid, block, shmem, st, q, ldq, k, ldk, v, ldv, keep, k_start, R, Sk, H,
                                                            (int)nblk, o, ldo);
    return launch<t5_attn_candidates_kernel<32, false>>(name, grid, block, shmem, st, q, ldq, k, ldk, v, ldv, keep, k_start, R, Sk, H,
                                                        (int)nblk, o, ldo);
}
