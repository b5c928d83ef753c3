// Scoring GIVEN items on the cached decode path (gfx950): the attention of one new token per candidate row against a prompt
// K/V cache stored once per sample, for ANY number of rows per sample, and the log-probability of a row's own token.
//
// gamer_attn_decode (csrc/decode.hip) holds all rows of a (sample, kv head) in one workgroup - num_beams * G <= 64 query columns, the
// KEY range split over the four waves, every wave streaming private K / V tiles.  A thousand candidates per user do not fit that
// shape, so this kernel turns it round: one workgroup = (sample, kv head, block of 128 query rows); the four waves own 32 query
// columns each (rows are G heads x consecutive candidates, the decode kernel's row -> (candidate, head) mapping) and SHARE every
// 32-key prompt tile, which the 256 threads stage into LDS once per workgroup - double-buffered, the next tile's global loads in
// flight while the current one is multiplied, one barrier per tile.
//   traffic   LDS: a K / V tile is written once and read by four waves per 128 query rows (the decode kernel: once per 64).
//             HBM / L2: the prompt cache of a (sample, kv head), L0 * 64 * 2 * 4 bytes, is read by each of its ceil(nb * G / 128)
//             blocks; the blocks of a (sample, kv head) are neighbours in the grid, so all but the first read come out of L2.
//   arithmetic  fp32, head size 64: S^T = K Q^T with the query on the lane and the scores straight into O^T += V^T P^T
//             (v_mfma_f32_32x32x2_f32), the online softmax in the log2 domain - the decode kernel's inner loop on one query tile
//             per wave.  No partial states to merge: a wave sees every key of its columns in order.
//   tail      the wave's state goes through LDS once (the tile buffers, free by then) to the lane = d layout; the <= tmax
//             generated keys of a row - its own, the new token included - are added on the vector unit as in the decode kernel.
//   semantics gamer_attn_decode's: gen_ok = 1 (a self block) the generated keys are allowed, gen_ok = 0 (a cross block) masked;
//             uniform[b] = 1: the row is the mean of V over all L0 + t keys (the finfo.min rule, csrc/decode.hip); a row with no
//             allowed key and no uniform flag gives zeros.  No atomics: every call gives the same bits.
// There is no three-piece fp16 form of this kernel: in every fp32 matmul form (f32, split3, ...) the candidate attention runs these
// fp32 MFMAs and only the GEMMs around it follow the engine's form.
#include "attention_common.h"
#include "decode_common.h"

namespace gamer {

constexpr int CAND_ROWS = 128;                                   // query rows of a workgroup: 32 per wave
constexpr int CAND_TILE = 32 * DEC_KLD + 32 * 64;                // floats of one staged tile: K image | V rows
constexpr int CAND_ML = 256;                                     // [4][32] running max | [4][32] running sum (uniform: [4][64] V sums)
constexpr int CAND_FIXED_FLOATS = 2 * CAND_TILE + CAND_ML;       // + key_ok of the whole prompt, padded to whole tiles
constexpr int CAND_MAX_L0 = (65536 / 4 - CAND_FIXED_FLOATS) / 32 * 32;      // 64 KB of LDS per workgroup at the most
static_assert(4 * 32 * DEC_OLD <= 2 * CAND_TILE, "the four waves' state images reuse the tile buffers");

template <int G>
__global__ void __launch_bounds__(256, 2)
attn_candidates_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ kp, int ldkp,
                       const float* __restrict__ vp, int ldvp, const int32_t* __restrict__ key_ok,
                       const float* __restrict__ kg, const float* __restrict__ vg, int ldg, int tmax, int t, int gen_ok,
                       const int32_t* __restrict__ uniform, int nb, int L0, int nq, int nkv, int nblk, float scale,
                       float* __restrict__ o) {
    extern __shared__ __attribute__((aligned(16))) float cand_lds[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int blk = blockIdx.x % nblk, bk = blockIdx.x / nblk;
    const int b = bk / nkv, kvh = bk % nkv;
    const int Qn = nb * G;
    const int q0 = blk * CAND_ROWS + w * 32;                    // this wave's first query row of the (sample, kv head)
    const bool uni = uniform != nullptr && uniform[b] != 0;
    const float c2 = scale * 1.4426950408889634f;               // scores live in the log2 domain
    float* tiles = cand_lds;                                    // two staged tiles; after the key loop: [4][32][DEC_OLD] states
    float* ml = cand_lds + 2 * CAND_TILE;
    int32_t* okl = reinterpret_cast<int32_t*>(ml + CAND_ML);    // key_ok of the sample, zero past L0
    float* Ow = tiles + w * 32 * DEC_OLD;

    if (uni) {
        // mean of V over the prompt keys (+ the generated ones in the tail): wave w sums keys w, w+4, ...
        float vsum = 0.f;
        for (int j = w; j < L0; j += 4) vsum += vp[((int64_t)b * L0 + j) * ldvp + kvh * 64 + lane];
        ml[w * 64 + lane] = vsum;
        __syncthreads();
    } else {
        const int n_tiles = (L0 + 31) >> 5;
        for (int j = tid; j < n_tiles * 32; j += 256) okl[j] = j < L0 ? key_ok[(int64_t)b * L0 + j] : 0;
        // the wave's query fragments (columns past Qn are zero and never stored)
        const bool wave_live = q0 < Qn;
        float qf[8][4];
        {
            const int qi = q0 + r;
            const bool live = qi < Qn;
            const int qc = live ? qi : 0;
            const float* qrow = q + (int64_t)(b * nb + qc / G) * ldq + (kvh * G + qc % G) * 64;
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) {
                const float4 t4 = *reinterpret_cast<const float4*>(qrow + 8 * kk + 4 * h);
                qf[kk][0] = live ? t4.x * c2 : 0.f; qf[kk][1] = live ? t4.y * c2 : 0.f;
                qf[kk][2] = live ? t4.z * c2 : 0.f; qf[kk][3] = live ? t4.w * c2 : 0.f;
            }
        }
        // a tile is 512 float4 of K and of V: two of each per thread; rows past the prompt are zero
        float4 kr[2], vr[2];
        auto request = [&](int jt) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int f = tid + 256 * i, row = f >> 4, c4 = (f & 15) << 2;
                const int j = jt * 32 + row;
                kr[i] = make_float4(0.f, 0.f, 0.f, 0.f); vr[i] = kr[i];
                if (j < L0) {
                    kr[i] = *reinterpret_cast<const float4*>(kp + ((int64_t)b * L0 + j) * ldkp + kvh * 64 + c4);
                    vr[i] = *reinterpret_cast<const float4*>(vp + ((int64_t)b * L0 + j) * ldvp + kvh * 64 + c4);
                }
            }
        };
        auto commit = [&](float* Kt) {
            float* Vt = Kt + 32 * DEC_KLD;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int f = tid + 256 * i, row = f >> 4, c4 = (f & 15) << 2;
                *reinterpret_cast<float4*>(&Kt[row * DEC_KLD + c4]) = kr[i];
                *reinterpret_cast<float4*>(&Vt[row * 64 + c4]) = vr[i];
            }
        };
        float m_run = -INFINITY, l_run = 0.f;
        dec_f32x16 oacc[2];
#pragma unroll
        for (int i = 0; i < 16; ++i) { oacc[0][i] = 0.f; oacc[1][i] = 0.f; }
        request(0);
        commit(tiles);
        __syncthreads();                                      // tile 0 and key_ok are in LDS
        for (int jt = 0; jt < n_tiles; ++jt) {
            const float* Kt = tiles + (jt & 1) * CAND_TILE;
            const float* Vt = Kt + 32 * DEC_KLD;
            const bool more = jt + 1 < n_tiles;
            if (more) request(jt + 1);                        // in flight while this tile is multiplied
            if (wave_live) {
                int okv[16];
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const int4 t4 = *reinterpret_cast<const int4*>(okl + jt * 32 + 8 * g4 + 4 * h);
                    okv[4 * g4] = t4.x; okv[4 * g4 + 1] = t4.y; okv[4 * g4 + 2] = t4.z; okv[4 * g4 + 3] = t4.w;
                }
                dec_f32x16 st;
#pragma unroll
                for (int i = 0; i < 16; ++i) st[i] = 0.f;
#pragma unroll
                for (int kk = 0; kk < 8; ++kk) {
                    const float4 kf = *reinterpret_cast<const float4*>(&Kt[r * DEC_KLD + 8 * kk + 4 * h]);
                    st = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, qf[kk][0], st, 0, 0, 0);
                    st = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, qf[kk][1], st, 0, 0, 0);
                    st = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, qf[kk][2], st, 0, 0, 0);
                    st = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, qf[kk][3], st, 0, 0, 0);
                }
                // register reg of lane (r, h) = score of key (reg&3) + 8*(reg>>2) + 4*h for query column r
                float mloc = -INFINITY;
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    st[reg] = okv[reg] != 0 ? st[reg] : -INFINITY;
                    mloc = fmaxf(mloc, st[reg]);
                }
                mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
                const float mn = fmaxf(m_run, mloc);
                const float base = mn == -INFINITY ? 0.f : mn;               // nothing allowed so far: p = 0
                const float alpha = __builtin_amdgcn_exp2f(m_run - base);    // m = -inf -> 0
                float rowsum = 0.f;
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    st[reg] = __builtin_amdgcn_exp2f(st[reg] - base);
                    rowsum += st[reg];
                }
                rowsum += __shfl_xor(rowsum, 32, 64);
                l_run = l_run * alpha + rowsum;
                m_run = mn;
#pragma unroll
                for (int i = 0; i < 16; ++i) { oacc[0][i] *= alpha; oacc[1][i] *= alpha; }
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int key = (reg & 3) + 8 * (reg >> 2) + 4 * h;
                    oacc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vt[key * 64 + r], st[reg], oacc[0], 0, 0, 0);
                    oacc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vt[key * 64 + 32 + r], st[reg], oacc[1], 0, 0, 0);
                }
            }
            // the other buffer was last read for tile jt - 1, before the barrier every wave passed at the end of that iteration
            if (more) commit(tiles + ((jt + 1) & 1) * CAND_TILE);
            __syncthreads();                                  // tile jt + 1 is staged and tile jt is consumed (last: the tiles are free)
        }
        // publish the wave's state for the tail: O[query r][d = 32*dh + (reg&3) + 8*(reg>>2) + 4*h]
        if (h == 0) { ml[w * 32 + r] = m_run; ml[128 + w * 32 + r] = l_run; }
#pragma unroll
        for (int dh = 0; dh < 2; ++dh)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg)
                Ow[r * DEC_OLD + 32 * dh + (reg & 3) + 8 * (reg >> 2) + 4 * h] = oacc[dh][reg];
        __syncthreads();
    }
    // tail: the wave's own 32 query rows one after the other, lane = d: the generated positions of the row (its own prefix and
    // the new token), normalise and store.  (Measured and not kept: the loads of eight rows requested together before the first dot
    // product - 0.651 against 0.656 ms per self-block call at 64 k rows; the tail is not what the call waits for.)
#pragma unroll 1
    for (int i = 0; i < 32; ++i) {
        const int qi = q0 + i;
        if (qi >= Qn) break;
        const int n = b * nb + qi / G, head = kvh * G + qi % G;
        float res;
        if (uni) {
            float a = ml[lane] + ml[64 + lane] + ml[128 + lane] + ml[192 + lane];
            for (int g = 0; g < t; ++g) a += vg[((int64_t)n * tmax + g) * ldg + kvh * 64 + lane];
            res = a / (float)(L0 + t);
        } else {
            float mi = ml[w * 32 + i], li = ml[128 + w * 32 + i];
            float a = Ow[i * DEC_OLD + lane];
            if (gen_ok) {
                // the row's generated key / value rows, four at a time, all requested before the first dot product waits for one
                const float qd = q[(int64_t)n * ldq + head * 64 + lane] * c2;
                for (int g0 = 0; g0 < t; g0 += 4) {
                    float kv4[4], vv4[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int64_t row = ((int64_t)n * tmax + min(g0 + u, t - 1)) * ldg + kvh * 64 + lane;
                        kv4[u] = kg[row];
                        vv4[u] = vg[row];
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        if (g0 + u < t) {
                            const float s = wave_sum_x(qd * kv4[u]);
                            const float mn = fmaxf(mi, s);
                            const float alpha = __builtin_amdgcn_exp2f(mi - mn), pe = __builtin_amdgcn_exp2f(s - mn);
                            li = li * alpha + pe;
                            a = a * alpha + pe * vv4[u];
                            mi = mn;
                        }
                    }
                }
            }
            res = li > 0.f ? a / li : 0.f;
        }
        o[(int64_t)n * nq * 64 + head * 64 + lane] = res;
    }
}

// out[n] (+)= log_softmax(logits[row_n][0..V))[token[n]]: one wave per row, one pass for the maximum and one for the sum - the
// [N, V] log-softmax is never written.  row_n = row_index[n] (NULL: n).  A token outside [0, V) gives -inf.
__global__ void __launch_bounds__(256)
token_logprob_kernel(const float* __restrict__ logits, int64_t ld, const int32_t* __restrict__ row_index,
                     const int64_t* __restrict__ token, int N, int V, int accumulate, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int n = (int)((blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6);
    if (n >= N) return;
    const float* row = logits + (int64_t)(row_index ? row_index[n] : n) * ld;
    float m = -INFINITY;
    for (int v = lane; v < V; v += 64) m = fmaxf(m, row[v]);
    m = wave_max(m);
    float s = 0.f;
    for (int v = lane; v < V; v += 64) s += __expf(row[v] - m);
    s = wave_sum(s);
    if (lane != 0) return;
    const int64_t tok = token[n];
    const float lp = (tok >= 0 && tok < V) ? row[tok] - (m + __logf(s)) : -INFINITY;
    out[n] = accumulate ? out[n] + lp : lp;
}

}  // namespace gamer

using namespace gamer;

extern "C" int gamer_attn_candidates(const float* q, int ldq, const float* kp, int ldkp, const float* vp, int ldvp,
                                     const int32_t* key_ok, const float* kg, const float* vg, int ldg, int tmax, int t,
                                     int gen_ok, const int32_t* uniform, int B, int nb, int L0, int nq, int nkv,
                                     float scale, float* o, void* stream) {
    GAMER_CHECK_ARG(q && kp && vp && key_ok && kg && vg && o, "gamer_attn_candidates: null pointer");
    GAMER_CHECK_ARG(B > 0 && nb > 0 && L0 > 0 && nq > 0 && nkv > 0 && nq % nkv == 0 && t >= 0 && t <= tmax,
                    "gamer_attn_candidates: bad shape B=%d nb=%d L0=%d nq=%d nkv=%d t=%d tmax=%d", B, nb, L0, nq, nkv, t, tmax);
    const int G = nq / nkv;
    GAMER_CHECK_ARG(G == 1 || G == 2, "gamer_attn_candidates: nq / nkv = %d (1 or 2 are built)", G);
    GAMER_CHECK_ARG(L0 <= CAND_MAX_L0, "gamer_attn_candidates: L0 = %d > %d (key_ok of a sample is held in LDS)", L0, CAND_MAX_L0);
    GAMER_CHECK_ARG(ldq % 4 == 0 && ldkp % 4 == 0 && ldvp % 4 == 0 && aligned16(q) && aligned16(kp) && aligned16(vp),
                    "gamer_attn_candidates: q / prompt K / V need 16-byte alignment and leading dims %% 4 == 0");
    const int64_t nblk = ((int64_t)nb * G + CAND_ROWS - 1) / CAND_ROWS;
    const int64_t blocks = (int64_t)B * nkv * nblk;
    GAMER_CHECK_ARG(blocks <= 0x7fffffff && (int64_t)B * nb <= 0x7fffffff, "gamer_attn_candidates: B * nb = %lld rows are too many",
                    (long long)B * nb);
    const size_t shmem = ((size_t)CAND_FIXED_FLOATS + (size_t)((L0 + 31) / 32) * 32) * sizeof(float);
    return with_group(nq, nkv, [&](auto g) {
        return launch<attn_candidates_kernel<g()>>("gamer_attn_candidates", dim3((unsigned)blocks), dim3(256), shmem, (hipStream_t)stream, q,
                                                   ldq, kp, ldkp, vp, ldvp, key_ok, kg, vg, ldg, tmax, t, gen_ok, uniform, nb, L0, nq, nkv,
                                                   (int)nblk, scale, o);
    });
}

extern "C" int gamer_token_logprob(const float* logits, int64_t ld, const int32_t* row_index, const int64_t* token, int N, int V,
                                   int accumulate, float* out, void* stream) {
    GAMER_CHECK_ARG(logits && token && out, "gamer_token_logprob: null pointer");
    GAMER_CHECK_ARG(N > 0 && V > 0 && ld >= V, "gamer_token_logprob: bad shape N=%d V=%d ld=%lld", N, V, (long long)ld);
    hipLaunchKernelGGL(token_logprob_kernel, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream, logits, ld, row_index, token, N, V,
                       accumulate, out);
    GAMER_CHECK_LAUNCH("gamer_token_logprob");
    return 0;
}
