// Catalogue-wide kernels of the discriminative baselines (SASRec: ref:SeqRec/modules/model_base/seq_model.py:67-122).
//   gamer_catalog_ce_fwd / _bwd   nn.CrossEntropyLoss over h @ E^T ([R, V] scores) without writing the scores to HBM
//   gamer_catalog_topk            top K of h @ E[start:end]^T per row (full_sort_predict + argsort, first K columns)
//   gamer_catalog_*_bias          the three above with a per-item bias added to every score (BERT4Rec's head) and its gradient
//   gamer_cloze_mask              BERT4Rec's cloze masking and the row-major compaction of the masked positions
//   gamer_embedding_bwd_large     item-embedding gradient without float atomics, tables of up to 2^31 - 1 rows
//   gamer_position_bwd            position-embedding gradient (per-position sums over the batch)
//   gamer_seq_embed_ln_fwd        dropout(LayerNorm(E[ids] + P[s])), the model's input block
//
// Score tiles: v_mfma_f32_16x16x4_f32 (exact fp32 products, a k-ordered fma chain), 16 x 16 per wave and instruction, H padded
// with zeros to HP = 64 / 128 / 256 (an fma with a zero product returns its addend unchanged, so the padding changes no bit).
// Every kernel that forms a score tile runs the same chain, so the backward's recompute reproduces the forward's scores bit for bit.
// A workgroup = 4 waves x 16 rows = 64 rows; items come in blocks of 64 through LDS (row stride HP + 4 floats: the 16 x 4 lanes
// of one operand read hit 64 different banks).  Lane l = (g = l >> 4, c = l & 15).
//
// Bounds (MI355X_MICROARCH.md: fp32 MFMA 157 TFLOP/s): a training step's head is 8 R H V FLOP - forward 2 R H V, the backward
// recomputes the scores twice (dE and dh kernels, 4 R H V) and forms dE and dh (4 R H V) - 0.43 TFLOP at R = 4096, H = 128,
// V = 100k: 2.7 ms at peak.  Its HBM traffic is the item table read ~3 + R / 64 / (items per chunk) times and dE written
// once (V H 4 bytes each); the materialised form moves the [R, V] fp32 scores ~5 times (8 GB at that shape, 1.6 ms at 5 TB/s).
// No float atomics anywhere: every sum has one fixed order, so two calls give the same bits.
#include "common.h"

namespace gamer {

#define ST(s) ((hipStream_t)(s))
constexpr int CAT_THREADS = 256;
constexpr int CAT_ROWS = 64;                 // rows per workgroup
constexpr int CAT_ITEMS = 64;                // items per LDS block
constexpr int CAT_KMAX = 64;                 // top-K limit

__device__ __forceinline__ int64_t cat_row(const void* idx, int idx64, int r) {
    if (!idx) return r;
    return idx64 ? ((const int64_t*)idx)[r] : (int64_t)((const int32_t*)idx)[r];
}
static inline int cat_hp(int H) { return H <= 64 ? 64 : (H <= 128 ? 128 : 256); }

// Chunking of the item axis: a fixed function of the shape (so of nothing that changes between two calls).
static inline int cat_chunks(int R, int n_items, int target_wgs, int max_chunks) {
    const int rb = (R + CAT_ROWS - 1) / CAT_ROWS;
    const int nblk = (n_items + CAT_ITEMS - 1) / CAT_ITEMS;
    int c = (target_wgs + rb - 1) / rb;
    c = c < 1 ? 1 : c;
    c = c > nblk ? nblk : c;
    return c > max_chunks ? max_chunks : c;
}
// items of chunk k: [item0 + k * per, min(item0 + (k + 1) * per, item_end)), per a multiple of CAT_ITEMS
static inline int cat_per_chunk(int n_items, int chunks) {
    const int nblk = (n_items + CAT_ITEMS - 1) / CAT_ITEMS;
    return ((nblk + chunks - 1) / chunks) * CAT_ITEMS;
}

// E rows [v0, v0 + 64) -> LDS [64][HP + 4], zeros past v_end and past H
template <int HP>
__device__ __forceinline__ void load_items(float* __restrict__ lds, const float* __restrict__ E, int H, int v0, int v_end) {
    constexpr int LD = HP + 4, C4 = HP / 4;
    for (int e = threadIdx.x; e < CAT_ITEMS * C4; e += CAT_THREADS) {
        const int it = e / C4, c4 = e % C4, v = v0 + it;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (v < v_end && 4 * c4 < H) x = *reinterpret_cast<const float4*>(E + (int64_t)v * H + 4 * c4);
        *reinterpret_cast<float4*>(lds + it * LD + 4 * c4) = x;
    }
}

// B operand of the S^T tiles for the wave's 16 rows: hreg[k] = h[row c][4k + g] (0 past H and for rows >= R)
template <int HP>
__device__ __forceinline__ void load_hreg(float (&hreg)[HP / 4], const float* __restrict__ h, int64_t ldh, const void* idx, int idx64,
                                          int R, int r, int H) {
    const int g = (threadIdx.x & 63) >> 4;
    const int64_t hr = r < R ? cat_row(idx, idx64, r) : 0;
#pragma unroll
    for (int k = 0; k < HP / 4; ++k) hreg[k] = (r < R && 4 * k + g < H) ? h[hr * ldh + 4 * k + g] : 0.f;
}

// S^T tiles of one 64-item LDS block: s[j][i] = score(row c, item 16 j + 4 g + i)
template <int HP>
__device__ __forceinline__ void score_tiles_t(f32x4v (&s)[4], const float (&hreg)[HP / 4], const float* __restrict__ lds) {
    constexpr int LD = HP + 4;
    const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < HP / 4; ++k) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            s[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(lds[(16 * j + c) * LD + 4 * k + g], hreg[k], s[j], 0, 0, 0);
    }
}

// BIAS instantiations: score(row, item v) += bias[v] for the S^T tiles of the block at v0 (the plain instantiations are the code
// without it: same instructions, same bits as before the bias existed)
template <bool BIAS>
__device__ __forceinline__ void add_bias_t(f32x4v (&s)[4], const float* __restrict__ bias, int v0, int v_end) {
    if (!BIAS || !bias) return;
    const int g = (threadIdx.x & 63) >> 4;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int v = v0 + 16 * j + 4 * g + i;
            if (v < v_end) s[j][i] += bias[v];
        }
}

// ---- cross entropy, forward: per (row block, chunk) running max / sum of exp -> ws; then the fixed-order merge -------------
template <int HP, bool BIAS>
__global__ void __launch_bounds__(CAT_THREADS)
cat_ce_partial_kernel(const float* __restrict__ h, int64_t ldh, const void* idx, int idx64, int R, const float* __restrict__ E,
                      int V, int H, int per_chunk, float* __restrict__ pmax, float* __restrict__ psum,
                      const float* __restrict__ bias) {
    __shared__ float lds[CAT_ITEMS * (HP + 4)];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
    const int r = blockIdx.x * CAT_ROWS + 16 * w + c;
    const int chunk = blockIdx.y, v_begin = chunk * per_chunk, v_end = min(V, v_begin + per_chunk);
    float hreg[HP / 4];
    load_hreg<HP>(hreg, h, ldh, idx, idx64, R, r, H);
    float m = -INFINITY, s = 0.f;
    for (int v0 = v_begin; v0 < v_end; v0 += CAT_ITEMS) {
        __syncthreads();
        load_items<HP>(lds, E, H, v0, v_end);
        __syncthreads();
        f32x4v t[4];
        score_tiles_t<HP>(t, hreg, lds);
        add_bias_t<BIAS>(t, bias, v0, v_end);
        float bm = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (v0 + 16 * j + 4 * g + i < v_end) bm = fmaxf(bm, t[j][i]);
        if (bm == -INFINITY) continue;
        const float nm = fmaxf(m, bm);
        float add = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (v0 + 16 * j + 4 * g + i < v_end) add += __expf(t[j][i] - nm);
        s = (m == -INFINITY ? 0.f : s * __expf(m - nm)) + add;
        m = nm;
    }
    // the four lanes of row c (g = 0..3): xor 16, then xor 32
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
        const float om = __shfl_xor(m, o, 64), os = __shfl_xor(s, o, 64);
        const float nm = fmaxf(m, om);
        if (nm != -INFINITY) s = (m == -INFINITY ? 0.f : s * __expf(m - nm)) + (om == -INFINITY ? 0.f : os * __expf(om - nm));
        m = nm;
    }
    if (g == 0 && r < R) {
        pmax[(int64_t)chunk * R + r] = m;
        psum[(int64_t)chunk * R + r] = s;
    }
}

// one thread per row: chunks merged in order; lse, the row's loss; bad targets counted
template <int HP, bool BIAS>
__global__ void __launch_bounds__(CAT_THREADS)
cat_ce_merge_kernel(const float* __restrict__ h, int64_t ldh, const void* idx, int idx64, int R, const float* __restrict__ E, int V,
                    int H, const int64_t* __restrict__ target, int chunks, const float* __restrict__ pmax,
                    const float* __restrict__ psum, float* __restrict__ lse, float* __restrict__ row_loss, int* __restrict__ bad,
                    const float* __restrict__ bias) {
    const int r = blockIdx.x * CAT_THREADS + threadIdx.x;
    if (r >= R) return;
    float m = -INFINITY, s = 0.f;
    for (int k = 0; k < chunks; ++k) {
        const float om = pmax[(int64_t)k * R + r], os = psum[(int64_t)k * R + r];
        const float nm = fmaxf(m, om);
        if (nm != -INFINITY) s = (m == -INFINITY ? 0.f : s * __expf(m - nm)) + (om == -INFINITY ? 0.f : os * __expf(om - nm));
        m = nm;
    }
    const float l = m + __logf(s);
    lse[r] = l;
    const int64_t t = target[r];
    if (t < 0 || t >= V) {
        atomicAdd(bad, 1);
        row_loss[r] = 0.f;
        return;
    }
    // the target's score by the MFMA's chain: k in order, one fma each, from +0
    const float* hr = h + cat_row(idx, idx64, r) * ldh;
    const float* er = E + t * H;
    float z = 0.f;
    for (int k = 0; k < H; ++k) z = fmaf(er[k], hr[k], z);
    if (BIAS && bias) z += bias[t];
    row_loss[r] = l - z;
}

// mean over R rows in one fixed order (one workgroup: strided partials, then a fixed tree)
__global__ void __launch_bounds__(CAT_THREADS)
cat_mean_kernel(const float* __restrict__ x, int R, float* __restrict__ out) {
    __shared__ float red[CAT_THREADS];
    float a = 0.f;
    for (int r = threadIdx.x; r < R; r += CAT_THREADS) a += x[r];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int o = CAT_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0] / (float)R;
}

// ---- cross entropy, backward ------------------------------------------------------------------------------------------------
// G[r, v] = (exp(score - lse[r]) - [v == target[r]]) * coef, coef = dloss / R (0 for rows past R and items past V)
__device__ __forceinline__ float cat_grad(float s, float lse, int v, int64_t tgt, float coef) {
    return (__expf(s - lse) - (v == tgt ? 1.f : 0.f)) * coef;
}

// dE: one workgroup per 64 items (16 per wave), sweeping every row in order; dE += G^T h, the row sum an MFMA chain.
// Score tiles here are S (A = h rows from LDS, B = the wave's items from registers): s[t][i] = score(row 16 t + 4 g + i, item c).
// The k-step (t, i) of dE^T = h^T G takes rows 16 t + 4 g + i, so G's register i is the B operand as it stands.
// BIAS: dbias[item] = the column sum of G: every lane adds its 16 rows of each row block in (t, i) order as the blocks go by, then the
// four lanes of an item in g order - one fixed order, written (not accumulated).  dE may be NULL then (dbias alone).
template <int HP, bool BIAS>
__global__ void __launch_bounds__(CAT_THREADS)
cat_ce_bwd_de_kernel(const float* __restrict__ h, int64_t ldh, const void* idx, int idx64, int R, const float* __restrict__ E, int V,
                     int H, const int64_t* __restrict__ target, const float* __restrict__ lse, const float* __restrict__ dloss,
                     float scale, float* __restrict__ dE, const float* __restrict__ bias, float* __restrict__ dbias) {
    constexpr int LD = HP + 4, C4 = HP / 4;
    __shared__ float hl[CAT_ROWS * LD];
    __shared__ float lse_l[CAT_ROWS];
    __shared__ int64_t tgt_l[CAT_ROWS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
    const int v = blockIdx.x * CAT_ITEMS + 16 * w + c;
    const float coef = (dloss ? dloss[0] : 1.f) * scale;
    float ereg[C4];
#pragma unroll
    for (int k = 0; k < C4; ++k) ereg[k] = (v < V && 4 * k + g < H) ? E[(int64_t)v * H + 4 * k + g] : 0.f;
    const float bv = (BIAS && bias && v < V) ? bias[v] : 0.f;
    float gsum = 0.f;
    f32x4v acc[HP / 16];
#pragma unroll
    for (int m = 0; m < HP / 16; ++m) acc[m] = f32x4v{0.f, 0.f, 0.f, 0.f};
    for (int r0 = 0; r0 < R; r0 += CAT_ROWS) {
        __syncthreads();
        for (int e = threadIdx.x; e < CAT_ROWS * C4; e += CAT_THREADS) {
            const int rr = e / C4, c4 = e % C4, r = r0 + rr;
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < R && 4 * c4 < H) {
                const float* hr = h + cat_row(idx, idx64, r) * ldh + 4 * c4;
                x = make_float4(hr[0], hr[1], hr[2], hr[3]);
            }
            *reinterpret_cast<float4*>(hl + rr * LD + 4 * c4) = x;
        }
        if (threadIdx.x < CAT_ROWS) {
            const int r = r0 + threadIdx.x;
            lse_l[threadIdx.x] = r < R ? lse[r] : 0.f;
            tgt_l[threadIdx.x] = r < R ? target[r] : -1;
        }
        __syncthreads();
        f32x4v s[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) s[t] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < C4; ++k)
#pragma unroll
            for (int t = 0; t < 4; ++t)
                s[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(hl[(16 * t + c) * LD + 4 * k + g], ereg[k], s[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int rr = 16 * t + 4 * g + i;
                s[t][i] = (r0 + rr < R && v < V) ? cat_grad(BIAS ? s[t][i] + bv : s[t][i], lse_l[rr], v, tgt_l[rr], coef) : 0.f;
                if (BIAS) gsum += s[t][i];
            }
        if (BIAS && !dE) continue;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int m = 0; m < HP / 16; ++m)
                    acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(hl[(16 * t + 4 * g + i) * LD + 16 * m + c], s[t][i], acc[m], 0, 0, 0);
    }
    if (BIAS && dbias) {
        const float g1 = __shfl(gsum, c + 16, 64), g2 = __shfl(gsum, c + 32, 64), g3 = __shfl(gsum, c + 48, 64);
        if (g == 0 && v < V) dbias[v] = ((gsum + g1) + g2) + g3;
    }
    // lane (g, c), register i: dE[item c][16 m + 4 g + i]
    if (v < V && (!BIAS || dE)) {
#pragma unroll
        for (int m = 0; m < HP / 16; ++m) {
            const int col = 16 * m + 4 * g;
            if (col < H) {
                float4* p = reinterpret_cast<float4*>(dE + (int64_t)v * H + col);
                float4 o = *p;
                o.x += acc[m][0]; o.y += acc[m][1]; o.z += acc[m][2]; o.w += acc[m][3];
                *p = o;
            }
        }
    }
}

// dh partials: per (row block, chunk), dh^T = E^T G^T over the chunk's items (k-step (j, i) = items 16 j + 4 g + i of a block)
template <int HP, bool BIAS>
__global__ void __launch_bounds__(CAT_THREADS)
cat_ce_bwd_dh_kernel(const float* __restrict__ h, int64_t ldh, const void* idx, int idx64, int R, const float* __restrict__ E, int V,
                     int H, const int64_t* __restrict__ target, const float* __restrict__ lse, const float* __restrict__ dloss,
                     float scale, int per_chunk, float* __restrict__ part, const float* __restrict__ bias) {
    constexpr int LD = HP + 4;
    __shared__ float lds[CAT_ITEMS * LD];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
    const int r = blockIdx.x * CAT_ROWS + 16 * w + c;
    const int chunk = blockIdx.y, v_begin = chunk * per_chunk, v_end = min(V, v_begin + per_chunk);
    const float coef = (dloss ? dloss[0] : 1.f) * scale;
    const float l = r < R ? lse[r] : 0.f;
    const int64_t tgt = r < R ? target[r] : -1;
    float hreg[HP / 4];
    load_hreg<HP>(hreg, h, ldh, idx, idx64, R, r, H);
    f32x4v acc[HP / 16];
#pragma unroll
    for (int m = 0; m < HP / 16; ++m) acc[m] = f32x4v{0.f, 0.f, 0.f, 0.f};
    for (int v0 = v_begin; v0 < v_end; v0 += CAT_ITEMS) {
        __syncthreads();
        load_items<HP>(lds, E, H, v0, v_end);
        __syncthreads();
        f32x4v s[4];
        score_tiles_t<HP>(s, hreg, lds);
        add_bias_t<BIAS>(s, bias, v0, v_end);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int v = v0 + 16 * j + 4 * g + i;
                s[j][i] = (r < R && v < v_end) ? cat_grad(s[j][i], l, v, tgt, coef) : 0.f;
            }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int m = 0; m < HP / 16; ++m)
                    acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(lds[(16 * j + 4 * g + i) * LD + 16 * m + c], s[j][i], acc[m], 0, 0, 0);
    }
    // lane (g, c), register i: dh[row c][16 m + 4 g + i]
    if (r < R) {
        float* p = part + ((int64_t)chunk * R + r) * HP;
#pragma unroll
        for (int m = 0; m < HP / 16; ++m)
            *reinterpret_cast<float4*>(p + 16 * m + 4 * g) = make_float4(acc[m][0], acc[m][1], acc[m][2], acc[m][3]);
    }
}

// dh[row_idx[r]][:H] = sum over chunks in order
__global__ void __launch_bounds__(CAT_THREADS)
cat_dh_reduce_kernel(const float* __restrict__ part, int R, int H, int HP, int chunks, const void* idx, int idx64,
                     float* __restrict__ dh, int64_t lddh) {
    const int64_t e = (int64_t)blockIdx.x * CAT_THREADS + threadIdx.x;
    if (e >= (int64_t)R * H) return;
    const int r = (int)(e / H), col = (int)(e % H);
    float a = 0.f;
    for (int k = 0; k < chunks; ++k) a += part[((int64_t)k * R + r) * HP + col];
    dh[cat_row(idx, idx64, r) * lddh + col] = a;
}

// ---- top K ------------------------------------------------------------------------------------------------------------------
// (score desc, index asc): a total order, so the top K of a set does not depend on the order candidates arrive in
__device__ __forceinline__ bool cat_better(float s1, int i1, float s2, int i2) { return s1 > s2 || (s1 == s2 && i1 < i2); }

// insert (s, i) into the sorted list (ls, li) of n <= K entries
__device__ __forceinline__ void cat_insert(float* ls, int* li, int& n, int K, float s, int i) {
    if (n == K && !cat_better(s, i, ls[K - 1], li[K - 1])) return;
    int p = n < K ? n : K - 1;
    while (p > 0 && cat_better(s, i, ls[p - 1], li[p - 1])) {
        ls[p] = ls[p - 1];
        li[p] = li[p - 1];
        --p;
    }
    ls[p] = s;
    li[p] = i;
    if (n < K) ++n;
}

// per (row block, chunk of [start, end)): every lane offers its 16 scores of row c to the row's list, the four lanes of a row in turn
template <int HP, bool BIAS>
__global__ void __launch_bounds__(CAT_THREADS)
cat_topk_partial_kernel(const float* __restrict__ h, int64_t ldh, const void* idx, int idx64, int R, const float* __restrict__ E, int H,
                        int start, int end, int per_chunk, int K, float* __restrict__ cs, int* __restrict__ ci,
                        const float* __restrict__ bias) {
    __shared__ float lds[CAT_ITEMS * (HP + 4)];
    __shared__ float ls[CAT_ROWS * CAT_KMAX];
    __shared__ int li[CAT_ROWS * CAT_KMAX];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
    const int r = blockIdx.x * CAT_ROWS + 16 * w + c;
    const int chunk = blockIdx.y, v_begin = start + chunk * per_chunk, v_end = min(end, v_begin + per_chunk);
    float* my_s = ls + (16 * w + c) * CAT_KMAX;
    int* my_i = li + (16 * w + c) * CAT_KMAX;
    int n = 0;                               // (kept equal in the four lanes of a row)
    float hreg[HP / 4];
    load_hreg<HP>(hreg, h, ldh, idx, idx64, R, r, H);
    for (int v0 = v_begin; v0 < v_end; v0 += CAT_ITEMS) {
        __syncthreads();
        load_items<HP>(lds, E, H, v0, v_end);
        __syncthreads();
        f32x4v s[4];
        score_tiles_t<HP>(s, hreg, lds);
        add_bias_t<BIAS>(s, bias, v0, v_end);
        for (int gg = 0; gg < 4; ++gg) {
            if (g == gg) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int v = v0 + 16 * j + 4 * g + i;
                        if (v < v_end) cat_insert(my_s, my_i, n, K, s[j][i], v);
                    }
            }
            n = __shfl(n, (lane & 15) + 16 * gg, 64);
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        }
    }
    if (g == 0 && r < R) {
        float* os = cs + ((int64_t)chunk * R + r) * K;
        int* oi = ci + ((int64_t)chunk * R + r) * K;
        for (int q = 0; q < K; ++q) {
            os[q] = q < n ? my_s[q] : -INFINITY;
            oi[q] = q < n ? my_i[q] : -1;
        }
    }
}

// one thread per row: the chunk lists merged (each sorted; a chunk's entries past its count are index -1)
__global__ void __launch_bounds__(CAT_THREADS)
cat_topk_merge_kernel(int R, int K, int chunks, const float* __restrict__ cs, const int* __restrict__ ci, int64_t* __restrict__ out_i,
                      float* __restrict__ out_s, float* __restrict__ scratch_s, int* __restrict__ scratch_i) {
    const int r = blockIdx.x * CAT_THREADS + threadIdx.x;
    if (r >= R) return;
    float* ls = scratch_s + (int64_t)r * K;
    int* li = scratch_i + (int64_t)r * K;
    int n = 0;
    for (int k = 0; k < chunks; ++k) {
        const float* s = cs + ((int64_t)k * R + r) * K;
        const int* i = ci + ((int64_t)k * R + r) * K;
        for (int q = 0; q < K; ++q) {
            if (i[q] < 0) break;
            if (n == K && !cat_better(s[q], i[q], ls[K - 1], li[K - 1])) break;     // the chunk's list is sorted
            cat_insert(ls, li, n, K, s[q], i[q]);
        }
    }
    for (int q = 0; q < K; ++q) {
        out_i[(int64_t)r * K + q] = q < n ? (int64_t)li[q] : -1;
        out_s[(int64_t)r * K + q] = q < n ? ls[q] : -INFINITY;
    }
}

// ---- item-embedding gradient for large tables ------------------------------------------------------------------------------
// Tokens are grouped by id with integer atomics only (counts, segment placement), each segment is put in token order by ranks
// (rank = number of the segment's tokens before this one, from 64-token chunks), then one wave sums a segment's rows in that
// order into dW.
__device__ __forceinline__ bool emb_ok(int64_t id, int V, int pad) { return id >= 0 && id < V && id != pad; }

__global__ void embl_init_kernel(const int64_t* __restrict__ ids, int T, int V, int pad, int* __restrict__ cnt) {
    const int t = blockIdx.x * CAT_THREADS + threadIdx.x;
    if (t < T && emb_ok(ids[t], V, pad)) cnt[ids[t]] = 0;
}
__global__ void embl_count_kernel(const int64_t* __restrict__ ids, int T, int V, int pad, int* __restrict__ cnt, int* __restrict__ claim) {
    const int t = blockIdx.x * CAT_THREADS + threadIdx.x;
    if (t >= T) return;
    claim[t] = 0;
    if (emb_ok(ids[t], V, pad)) claim[t] = atomicAdd(cnt + ids[t], 1) == 0;
}
__global__ void embl_place_kernel(const int64_t* __restrict__ ids, int T, const int* __restrict__ claim, const int* __restrict__ cnt,
                                  int* __restrict__ segk, int* __restrict__ counters, int* __restrict__ seg_start,
                                  int* __restrict__ seg_n, int* __restrict__ seg_id) {
    const int t = blockIdx.x * CAT_THREADS + threadIdx.x;
    if (t >= T || !claim[t]) return;
    const int64_t id = ids[t];
    const int n = cnt[id];
    const int k = atomicAdd(counters + 1, 1);
    seg_start[k] = atomicAdd(counters, n);
    seg_n[k] = n;
    seg_id[k] = (int)id;
    segk[id] = k;
}
// A token's rank in its id's segment = the id's tokens in earlier 64-token chunks + those before it in its own chunk.  One wave per
// chunk finds the in-chunk rank and count (64 shuffles); the first token of an id in a chunk (its leader) files (chunk, count)
// in the segment's pair list; each leader sums the counts of the pairs of earlier chunks; every token adds its leader's sum.
// Work per token: 64 steps, per leader: the segment's pairs (at most T / 64) - bounded however skewed the ids are.
constexpr int EMB_CHUNK = 64;
__global__ void __launch_bounds__(CAT_THREADS)
embl_chunk_kernel(const int64_t* __restrict__ ids, int T, int V, int pad, const int* __restrict__ segk, const int* __restrict__ seg_start,
                  int* __restrict__ pcount, int* __restrict__ pair_chunk, int* __restrict__ pair_cnt, int* __restrict__ rin,
                  int* __restrict__ lead) {
    const int lane = threadIdx.x & 63;
    const int chunk = (blockIdx.x * CAT_THREADS + threadIdx.x) >> 6;
    const int t = chunk * EMB_CHUNK + lane;
    const bool ok = t < T && emb_ok(ids[t], V, pad);
    const int key = ok ? (int)ids[t] : -1;
    int r = 0, n = 0, first = lane;
    for (int j = 0; j < EMB_CHUNK; ++j) {
        const int kj = __shfl(key, j, 64);
        if (ok && kj == key) {
            if (j < lane && r++ == 0) first = j;
            ++n;
        }
    }
    if (!ok) return;
    rin[t] = r;
    lead[t] = chunk * EMB_CHUNK + first;
    if (r == 0) {
        const int k = segk[key];
        const int q = seg_start[k] + atomicAdd(pcount + k, 1);
        pair_chunk[q] = chunk;
        pair_cnt[q] = n;
    }
}
__global__ void embl_prefix_kernel(const int64_t* __restrict__ ids, int T, int V, int pad, const int* __restrict__ segk,
                                   const int* __restrict__ seg_start, const int* __restrict__ pcount, const int* __restrict__ pair_chunk,
                                   const int* __restrict__ pair_cnt, const int* __restrict__ rin, int* __restrict__ cprefix) {
    const int t = blockIdx.x * CAT_THREADS + threadIdx.x;
    if (t >= T || !emb_ok(ids[t], V, pad) || rin[t] != 0) return;
    const int k = segk[ids[t]], s = seg_start[k], np = pcount[k], chunk = t / EMB_CHUNK;
    int p = 0;
    for (int q = 0; q < np; ++q) p += pair_chunk[s + q] < chunk ? pair_cnt[s + q] : 0;
    cprefix[t] = p;
}
__global__ void embl_rank_kernel(const int64_t* __restrict__ ids, int T, int V, int pad, const int* __restrict__ segk,
                                 const int* __restrict__ seg_start, const int* __restrict__ rin, const int* __restrict__ lead,
                                 const int* __restrict__ cprefix, int* __restrict__ sorted, int* __restrict__ posseg) {
    const int t = blockIdx.x * CAT_THREADS + threadIdx.x;
    if (t >= T || !emb_ok(ids[t], V, pad)) return;
    const int k = segk[ids[t]], pos = seg_start[k] + cprefix[lead[t]] + rin[t];
    sorted[pos] = t;
    posseg[pos] = k;
}
// segments longer than EMB_CHUNK: the rows of each 64-position piece summed in order into part[piece start] (one wave per piece),
// so that a hot item is not one wave's sequential sweep; embl_sum_kernel then adds the pieces in order
__global__ void __launch_bounds__(CAT_THREADS)
embl_piece_kernel(const float4* __restrict__ dx, int T, int H4, const int* __restrict__ counters, const int* __restrict__ posseg,
                  const int* __restrict__ seg_start, const int* __restrict__ seg_n, const int* __restrict__ sorted,
                  float4* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const int p = (blockIdx.x * CAT_THREADS + threadIdx.x) >> 6;
    if (p >= T || p >= counters[0]) return;
    const int k = posseg[p], s = seg_start[k], n = seg_n[k];
    if (n <= EMB_CHUNK || (p - s) % EMB_CHUNK) return;
    const int e = min(p + EMB_CHUNK, s + n);
    for (int c = lane; c < H4; c += 64) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int q = p; q < e; ++q) {
            const float4 x = dx[(int64_t)sorted[q] * H4 + c];
            a.x += x.x; a.y += x.y; a.z += x.z; a.w += x.w;
        }
        part[(int64_t)p * H4 + c] = a;
    }
}
__global__ void __launch_bounds__(CAT_THREADS)
embl_sum_kernel(const float4* __restrict__ dx, int T, int H4, const int* __restrict__ counters, const int* __restrict__ seg_start,
                const int* __restrict__ seg_n, const int* __restrict__ seg_id, const int* __restrict__ sorted,
                const float4* __restrict__ part, float4* __restrict__ dW) {
    const int lane = threadIdx.x & 63;
    const int k = (blockIdx.x * CAT_THREADS + threadIdx.x) >> 6;
    if (k >= T || k >= counters[1]) return;
    const int s = seg_start[k], n = seg_n[k];
    float4* out = dW + (int64_t)seg_id[k] * H4;
    for (int c = lane; c < H4; c += 64) {
        float4 a = out[c];
        if (n <= EMB_CHUNK) {
            for (int q = 0; q < n; ++q) {
                const float4 x = dx[(int64_t)sorted[s + q] * H4 + c];
                a.x += x.x; a.y += x.y; a.z += x.z; a.w += x.w;
            }
        } else {
            for (int q = 0; q < n; q += EMB_CHUNK) {
                const float4 x = part[(int64_t)(s + q) * H4 + c];
                a.x += x.x; a.y += x.y; a.z += x.z; a.w += x.w;
            }
        }
        out[c] = a;
    }
}

// ---- position-embedding gradient: dP[s] += sum_b dx[b, s] (batch chunks of 64 in order, then the chunks in order) -------------
constexpr int POS_BCH = 64;
__global__ void __launch_bounds__(CAT_THREADS)
pos_partial_kernel(const float4* __restrict__ dx, int B, int S4H, float4* __restrict__ part) {
    const int e = blockIdx.x * CAT_THREADS + threadIdx.x;
    if (e >= S4H) return;
    const int b0 = blockIdx.y * POS_BCH, b1 = min(B, b0 + POS_BCH);
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int b = b0; b < b1; ++b) {
        const float4 x = dx[(int64_t)b * S4H + e];
        a.x += x.x; a.y += x.y; a.z += x.z; a.w += x.w;
    }
    part[(int64_t)blockIdx.y * S4H + e] = a;
}
__global__ void __launch_bounds__(CAT_THREADS)
pos_reduce_kernel(const float4* __restrict__ part, int nb, int S4H, float4* __restrict__ dP) {
    const int e = blockIdx.x * CAT_THREADS + threadIdx.x;
    if (e >= S4H) return;
    float4 a = dP[e];
    for (int k = 0; k < nb; ++k) {
        const float4 x = part[(int64_t)k * S4H + e];
        a.x += x.x; a.y += x.y; a.z += x.z; a.w += x.w;
    }
    dP[e] = a;
}

// ---- input block: y = dropout(LayerNorm(E[ids[t]] + P[t % S])), one wave per token, one float4 per lane (H <= 256) ------------
// v (the LayerNorm input), mean and rstd are kept for gamer_layernorm_bwd; the dropout word of float4 (t, c) is that of the flat
// index t * H / 4 + c, the mask gamer_residual_dropout_bwd regenerates with the same seed.
__global__ void __launch_bounds__(CAT_THREADS)
seq_embed_ln_kernel(const int64_t* __restrict__ ids, const float* __restrict__ E, int V, const float* __restrict__ P, int T, int S,
                    int H, const float* __restrict__ w, const float* __restrict__ b, float eps, float p, uint64_t seed,
                    float* __restrict__ v_out, float* __restrict__ y, float* __restrict__ mean_out, float* __restrict__ rstd_out) {
    const DropoutRng rng(p, seed);
    const int lane = threadIdx.x & 63, H4 = H / 4;
    const int t = (blockIdx.x * CAT_THREADS + threadIdx.x) >> 6;
    if (t >= T) return;
    const int64_t id = ids[t];
    const int s = t % S;
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane < H4) {
        const float4 e = (id >= 0 && id < V) ? *reinterpret_cast<const float4*>(E + id * H + 4 * lane) : x;
        const float4 q = *reinterpret_cast<const float4*>(P + (int64_t)s * H + 4 * lane);
        x = make_float4(e.x + q.x, e.y + q.y, e.z + q.z, e.w + q.w);
    }
    const float mean = wave_sum(x.x + x.y + x.z + x.w) / (float)H;
    const float dx0 = x.x - mean, dx1 = x.y - mean, dx2 = x.z - mean, dx3 = x.w - mean;
    const float var = wave_sum(lane < H4 ? dx0 * dx0 + dx1 * dx1 + dx2 * dx2 + dx3 * dx3 : 0.f) / (float)H;
    const float rstd = rsqrtf(var + eps);
    if (lane < H4) {
        const float4 wv = *reinterpret_cast<const float4*>(w + 4 * lane), bv = *reinterpret_cast<const float4*>(b + 4 * lane);
        float m[4];
        rng.mult4((uint32_t)((int64_t)t * H4 + lane), m);
        const float4 o = make_float4(m[0] * (dx0 * rstd * wv.x + bv.x), m[1] * (dx1 * rstd * wv.y + bv.y),
                                     m[2] * (dx2 * rstd * wv.z + bv.z), m[3] * (dx3 * rstd * wv.w + bv.w));
        *reinterpret_cast<float4*>(v_out + (int64_t)t * H + 4 * lane) = x;
        *reinterpret_cast<float4*>(y + (int64_t)t * H + 4 * lane) = o;
    }
    if (lane == 0) {
        mean_out[t] = mean;
        rstd_out[t] = rstd;
    }
}

// ---- BERT4Rec's cloze masking (ref:SeqRec/models/discriminative/BERT4Rec/model.py reconstruct_train_data) ----------------------
// ft[b] = word(B L + b) < ft_ratio 2^32; m[b, s] = word(b L + s) < mask_ratio 2^32 and ids != 0 and not ft[b]; m[b, p_b] |= ft[b],
// p_b = min(seq_len[b], max_seq_length - 1); labels = ids * m; masked = m ? mask_token : ids.  word(i) is the 32-bit word of
// DropoutRng::mult(i) (a ratio >= 1 always masks).  The masked positions with a label (labels != 0) are compacted in row-major
// order without atomics: a wave per 64-token chunk counts them (ballot), one workgroup turns the chunk counts into offsets, a
// wave per chunk places its tokens at offset + rank.
struct ClozeRng {
    uint32_t k0, k1;
    __device__ __forceinline__ explicit ClozeRng(uint64_t seed) {
        const DropoutRng r(0.f, seed);
        k0 = r.k0;
        k1 = r.k1;
    }
    __device__ __forceinline__ uint32_t word(uint32_t idx) const { return mix32(mix32(idx ^ k0) + k1); }
};
static inline uint32_t cloze_thr(float ratio) {
    const float t = ratio * 4294967296.f;
    return t >= 4294967040.f ? 0xffffffffU : (t <= 0.f ? 0u : (uint32_t)t);
}
constexpr int CLOZE_CHUNK = 64;

__global__ void __launch_bounds__(CAT_THREADS)
cloze_mask_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ seq_len, int B, int L, uint32_t thr_mask, int all_mask,
                  uint32_t thr_ft, int all_ft, int64_t mask_token, int max_seq_length, uint64_t seed, int64_t* __restrict__ masked,
                  int64_t* __restrict__ labels, int* __restrict__ chunk_count, int64_t* __restrict__ words) {
    const ClozeRng rng(seed);
    const int T = B * L;
    const int lane = threadIdx.x & 63;
    const int chunk = (blockIdx.x * CAT_THREADS + threadIdx.x) >> 6;
    const int t = chunk * CLOZE_CHUNK + lane;
    bool has = false;
    if (t < T) {
        const int b = t / L, s = t % L;
        const uint32_t wr = rng.word((uint32_t)(T + b)), wp = rng.word((uint32_t)t);
        const bool ft = all_ft || wr < thr_ft;
        const int64_t n = seq_len[b], id = ids[t];
        const int64_t p = n < max_seq_length - 1 ? n : max_seq_length - 1;
        const bool m = ((all_mask || wp < thr_mask) && id != 0 && !ft) || (ft && s == p);
        masked[t] = m ? mask_token : id;
        labels[t] = m ? id : 0;
        has = m && id != 0;
        if (words) {
            words[t] = (int64_t)wp;
            if (s == 0) words[T + b] = (int64_t)wr;
        }
    }
    const uint64_t bal = __ballot(has);
    if (lane == 0 && chunk * CLOZE_CHUNK < T) chunk_count[chunk] = __popcll(bal);
}

// one workgroup: chunk counts -> exclusive offsets (in place), the total -> count[0]
__global__ void __launch_bounds__(CAT_THREADS)
cloze_scan_kernel(int* __restrict__ chunk_count, int nchunks, int* __restrict__ count) {
    __shared__ int part[CAT_THREADS];
    const int per = (nchunks + CAT_THREADS - 1) / CAT_THREADS;
    const int c0 = min(nchunks, (int)threadIdx.x * per), c1 = min(nchunks, c0 + per);
    int a = 0;
    for (int c = c0; c < c1; ++c) a += chunk_count[c];
    part[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int i = 0; i < CAT_THREADS; ++i) {
            const int x = part[i];
            part[i] = run;
            run += x;
        }
        count[0] = run;
    }
    __syncthreads();
    int run = part[threadIdx.x];
    for (int c = c0; c < c1; ++c) {
        const int x = chunk_count[c];
        chunk_count[c] = run;
        run += x;
    }
}

__global__ void __launch_bounds__(CAT_THREADS)
cloze_place_kernel(const int64_t* __restrict__ labels, int T, const int* __restrict__ chunk_off, int64_t* __restrict__ rows,
                   int64_t* __restrict__ targets) {
    const int lane = threadIdx.x & 63;
    const int chunk = (blockIdx.x * CAT_THREADS + threadIdx.x) >> 6;
    const int t = chunk * CLOZE_CHUNK + lane;
    const int64_t lab = t < T ? labels[t] : 0;
    const uint64_t bal = __ballot(lab != 0);
    if (lab != 0) {
        const int q = chunk_off[chunk] + __popcll(bal & ((1ull << lane) - 1ull));
        if (q < T) {
            rows[q] = t;
            targets[q] = lab;
        }
    }
}

}  // namespace gamer

using namespace gamer;

// ---- C ABI ------------------------------------------------------------------------------------------------------------------
static int cat_shape_ok(const char* name, int R, int V, int H, int64_t ldh) {
    GAMER_CHECK_ARG(R > 0 && V > 0 && H > 0 && H % 4 == 0 && H <= 256 && ldh >= H,
                    "%s: bad shape R=%d V=%d H=%d ldh=%lld (H %% 4 == 0, H <= 256, ldh >= H)", name, R, V, H, (long long)ldh);
    return 0;
}
static int ce_chunks(int R, int V) { return cat_chunks(R, V, 1024, 1 << 20); }
static int topk_chunks(int R, int n) { return cat_chunks(R, n, 512, 64); }

extern "C" int64_t gamer_catalog_ws_bytes(int R, int V, int H, int K) {
    if (R <= 0 || V <= 0 || H <= 0 || H > 256 || K < 0 || K > CAT_KMAX) return -1;
    if (K > 0) {
        const int64_t ch = topk_chunks(R, V);
        return ch * R * K * 8 + (int64_t)R * K * 8;
    }
    const int64_t ch = ce_chunks(R, V);
    const int64_t a = 2 * ch * R + R;                              // pmax, psum, row_loss
    const int64_t b = ch * R * cat_hp(H);                          // dh partials
    return ((a > b ? a : b) * 4 + 15) / 16 * 16 + 16;
}

#define CAT_DISPATCH_B(HP_, B_, KERNEL, GRID, ...)                                                                       \
    do {                                                                                                                  \
        if ((HP_) == 64) hipLaunchKernelGGL((KERNEL<64, B_>), GRID, dim3(CAT_THREADS), 0, st, __VA_ARGS__);               \
        else if ((HP_) == 128) hipLaunchKernelGGL((KERNEL<128, B_>), GRID, dim3(CAT_THREADS), 0, st, __VA_ARGS__);        \
        else hipLaunchKernelGGL((KERNEL<256, B_>), GRID, dim3(CAT_THREADS), 0, st, __VA_ARGS__);                          \
    } while (0)
// BIAS_: whether the call has a bias (or a bias gradient); without one the plain instantiation runs
#define CAT_DISPATCH(HP_, BIAS_, KERNEL, GRID, ...)                                  \
    do {                                                                             \
        if (BIAS_) CAT_DISPATCH_B(HP_, true, KERNEL, GRID, __VA_ARGS__);             \
        else CAT_DISPATCH_B(HP_, false, KERNEL, GRID, __VA_ARGS__);                  \
    } while (0)

// (the entry points without a bias call these with bias = NULL: the plain instantiations, the launches they always made)
static int catalog_ce_fwd(const char* name, const float* h, int64_t ldh, const void* row_idx, int idx64, int R, const float* E, int V,
                          int H, const float* bias, const int64_t* target, float* lse, float* loss, int* bad, void* ws,
                          int64_t ws_bytes, void* stream) {
    GAMER_CHECK_ARG(h && E && target && lse && loss && bad && ws, "%s: null pointer", name);
    if (cat_shape_ok(name, R, V, H, ldh)) return -1;
    GAMER_CHECK_ARG(aligned16(E) && aligned16(ws) && ws_bytes >= gamer_catalog_ws_bytes(R, V, H, 0),
                    "%s: E / ws must be 16-byte aligned and ws hold %lld bytes", name,
                    (long long)gamer_catalog_ws_bytes(R, V, H, 0));
    const bool hb = bias != nullptr;
    const int ch = ce_chunks(R, V), per = cat_per_chunk(V, ch), hp = cat_hp(H);
    float* pmax = (float*)ws;
    float* psum = pmax + (int64_t)ch * R;
    float* row_loss = psum + (int64_t)ch * R;
    hipStream_t st = ST(stream);
    CAT_DISPATCH(hp, hb, cat_ce_partial_kernel, dim3((R + CAT_ROWS - 1) / CAT_ROWS, ch), h, ldh, row_idx, idx64, R, E, V, H, per, pmax,
                 psum, bias);
    GAMER_CHECK_LAUNCH("gamer_catalog_ce_fwd/partial");
    CAT_DISPATCH(hp, hb, cat_ce_merge_kernel, dim3((R + CAT_THREADS - 1) / CAT_THREADS), h, ldh, row_idx, idx64, R, E, V, H, target, ch,
                 pmax, psum, lse, row_loss, bad, bias);
    GAMER_CHECK_LAUNCH("gamer_catalog_ce_fwd/merge");
    hipLaunchKernelGGL(cat_mean_kernel, dim3(1), dim3(CAT_THREADS), 0, st, row_loss, R, loss);
    GAMER_CHECK_LAUNCH("gamer_catalog_ce_fwd/mean");
    return 0;
}
extern "C" int gamer_catalog_ce_fwd(const float* h, int64_t ldh, const void* row_idx, int idx64, int R, const float* E, int V, int H,
                                    const int64_t* target, float* lse, float* loss, int* bad, void* ws, int64_t ws_bytes,
                                    void* stream) {
    return catalog_ce_fwd("gamer_catalog_ce_fwd", h, ldh, row_idx, idx64, R, E, V, H, nullptr, target, lse, loss, bad, ws, ws_bytes,
                          stream);
}
extern "C" int gamer_catalog_ce_bias_fwd(const float* h, int64_t ldh, const void* row_idx, int idx64, int R, const float* E, int V,
                                         int H, const float* bias, const int64_t* target, float* lse, float* loss, int* bad, void* ws,
                                         int64_t ws_bytes, void* stream) {
    return catalog_ce_fwd("gamer_catalog_ce_bias_fwd", h, ldh, row_idx, idx64, R, E, V, H, bias, target, lse, loss, bad, ws, ws_bytes,
                          stream);
}

static int catalog_ce_bwd(const char* name, const float* h, int64_t ldh, const void* row_idx, int idx64, int R, const float* E, int V,
                          int H, const float* bias, const int64_t* target, const float* lse, const float* dloss, float scale,
                          float* dE, float* dh, int64_t lddh, float* dbias, void* ws, int64_t ws_bytes, void* stream) {
    GAMER_CHECK_ARG(h && E && target && lse && ws && (dE || dh || dbias), "%s: null pointer", name);
    if (cat_shape_ok(name, R, V, H, ldh)) return -1;
    GAMER_CHECK_ARG(!dh || lddh >= H, "%s: lddh=%lld < H=%d", name, (long long)lddh, H);
    GAMER_CHECK_ARG(aligned16(E) && aligned16(ws) && (!dE || aligned16(dE)) && ws_bytes >= gamer_catalog_ws_bytes(R, V, H, 0),
                    "%s: E / dE / ws must be 16-byte aligned and ws hold %lld bytes", name,
                    (long long)gamer_catalog_ws_bytes(R, V, H, 0));
    const int ch = ce_chunks(R, V), per = cat_per_chunk(V, ch), hp = cat_hp(H);
    const bool hb = bias != nullptr;
    hipStream_t st = ST(stream);
    if (dE || dbias) {
        CAT_DISPATCH(hp, hb || dbias, cat_ce_bwd_de_kernel, dim3((V + CAT_ITEMS - 1) / CAT_ITEMS), h, ldh, row_idx, idx64, R, E, V, H,
                     target, lse, dloss, scale, dE, bias, dbias);
        GAMER_CHECK_LAUNCH("gamer_catalog_ce_bwd/dE");
    }
    if (dh) {
        float* part = (float*)ws;
        CAT_DISPATCH(hp, hb, cat_ce_bwd_dh_kernel, dim3((R + CAT_ROWS - 1) / CAT_ROWS, ch), h, ldh, row_idx, idx64, R, E, V, H, target,
                     lse, dloss, scale, per, part, bias);
        GAMER_CHECK_LAUNCH("gamer_catalog_ce_bwd/dh");
        const int64_t n = (int64_t)R * H;
        hipLaunchKernelGGL(cat_dh_reduce_kernel, dim3((unsigned)((n + CAT_THREADS - 1) / CAT_THREADS)), dim3(CAT_THREADS), 0, st, part,
                           R, H, hp, ch, row_idx, idx64, dh, lddh);
        GAMER_CHECK_LAUNCH("gamer_catalog_ce_bwd/dh_reduce");
    }
    return 0;
}
extern "C" int gamer_catalog_ce_bwd(const float* h, int64_t ldh, const void* row_idx, int idx64, int R, const float* E, int V, int H,
                                    const int64_t* target, const float* lse, const float* dloss, float scale, float* dE, float* dh,
                                    int64_t lddh, void* ws, int64_t ws_bytes, void* stream) {
    GAMER_CHECK_ARG(dE || dh, "gamer_catalog_ce_bwd: null pointer");
    return catalog_ce_bwd("gamer_catalog_ce_bwd", h, ldh, row_idx, idx64, R, E, V, H, nullptr, target, lse, dloss, scale, dE, dh, lddh,
                          nullptr, ws, ws_bytes, stream);
}
extern "C" int gamer_catalog_ce_bias_bwd(const float* h, int64_t ldh, const void* row_idx, int idx64, int R, const float* E, int V,
                                         int H, const float* bias, const int64_t* target, const float* lse, const float* dloss,
                                         float scale, float* dE, float* dh, int64_t lddh, float* dbias, void* ws, int64_t ws_bytes,
                                         void* stream) {
    return catalog_ce_bwd("gamer_catalog_ce_bias_bwd", h, ldh, row_idx, idx64, R, E, V, H, bias, target, lse, dloss, scale, dE, dh, lddh,
                          dbias, ws, ws_bytes, stream);
}

static int catalog_topk(const char* name, const float* h, int64_t ldh, const void* row_idx, int idx64, int R, const float* E, int V,
                        int H, const float* bias, int start, int end, int K, int64_t* out_idx, float* out_score, void* ws,
                        int64_t ws_bytes, void* stream) {
    GAMER_CHECK_ARG(h && E && out_idx && out_score && ws, "%s: null pointer", name);
    if (cat_shape_ok(name, R, V, H, ldh)) return -1;
    GAMER_CHECK_ARG(K > 0 && K <= CAT_KMAX && start >= 0 && start < end && end <= V, "%s: K=%d (1..%d), range [%d, %d) of V=%d", name,
                    K, CAT_KMAX, start, end, V);
    const int n = end - start;
    GAMER_CHECK_ARG(aligned16(E) && aligned16(ws) && ws_bytes >= gamer_catalog_ws_bytes(R, n, H, K),
                    "%s: E / ws must be 16-byte aligned and ws hold %lld bytes", name, (long long)gamer_catalog_ws_bytes(R, n, H, K));
    const bool hb = bias != nullptr;
    const int ch = topk_chunks(R, n), per = cat_per_chunk(n, ch), hp = cat_hp(H);
    float* cs = (float*)ws;
    int* ci = (int*)(cs + (int64_t)ch * R * K);
    float* ms = (float*)(ci + (int64_t)ch * R * K);
    int* mi = (int*)(ms + (int64_t)R * K);
    hipStream_t st = ST(stream);
    CAT_DISPATCH(hp, hb, cat_topk_partial_kernel, dim3((R + CAT_ROWS - 1) / CAT_ROWS, ch), h, ldh, row_idx, idx64, R, E, H, start, end,
                 per, K, cs, ci, bias);
    GAMER_CHECK_LAUNCH("gamer_catalog_topk/partial");
    hipLaunchKernelGGL(cat_topk_merge_kernel, dim3((R + CAT_THREADS - 1) / CAT_THREADS), dim3(CAT_THREADS), 0, st, R, K, ch, cs, ci,
                       out_idx, out_score, ms, mi);
    GAMER_CHECK_LAUNCH("gamer_catalog_topk/merge");
    return 0;
}
extern "C" int gamer_catalog_topk(const float* h, int64_t ldh, const void* row_idx, int idx64, int R, const float* E, int V, int H,
                                  int start, int end, int K, int64_t* out_idx, float* out_score, void* ws, int64_t ws_bytes,
                                  void* stream) {
    return catalog_topk("gamer_catalog_topk", h, ldh, row_idx, idx64, R, E, V, H, nullptr, start, end, K, out_idx, out_score, ws,
                        ws_bytes, stream);
}
extern "C" int gamer_catalog_topk_bias(const float* h, int64_t ldh, const void* row_idx, int idx64, int R, const float* E, int V, int H,
                                       const float* bias, int start, int end, int K, int64_t* out_idx, float* out_score, void* ws,
                                       int64_t ws_bytes, void* stream) {
    return catalog_topk("gamer_catalog_topk_bias", h, ldh, row_idx, idx64, R, E, V, H, bias, start, end, K, out_idx, out_score, ws,
                        ws_bytes, stream);
}

extern "C" int64_t gamer_embedding_bwd_large_ws_bytes(int V, int T, int H) {
    if (V <= 0 || T <= 0 || H <= 0) return -1;
    return ((2 * (int64_t)V + 11 * (int64_t)T + 2) * 4 + 15) / 16 * 16 + (int64_t)T * H * 4;
}
extern "C" int gamer_embedding_bwd_large(const int64_t* ids, const float* dx, int V, int T, int H, int pad_id, float* dW, void* ws,
                                         int64_t ws_bytes, void* stream) {
    GAMER_CHECK_ARG(ids && dx && dW && ws, "gamer_embedding_bwd_large: null pointer");
    GAMER_CHECK_ARG(T > 0 && H > 0 && H % 4 == 0 && V > 0, "gamer_embedding_bwd_large: bad shape T=%d H=%d V=%d", T, H, V);
    GAMER_CHECK_ARG(aligned16(dx) && aligned16(dW) && aligned16(ws) && ws_bytes >= gamer_embedding_bwd_large_ws_bytes(V, T, H),
                    "gamer_embedding_bwd_large: dx / dW must be 16-byte aligned and ws hold %lld bytes",
                    (long long)gamer_embedding_bwd_large_ws_bytes(V, T, H));
    int* p = (int*)ws;
    int* cnt = p; p += V;
    int* segk = p; p += V;
    int* claim = p; p += T;
    int* seg_start = p; p += T;
    int* seg_n = p; p += T;
    int* seg_id = p; p += T;
    int* sorted = p; p += T;
    int* pcount = p; p += T;                 // pairs filed per segment
    int* pair_chunk = p; p += T;
    int* pair_cnt = p; p += T;
    int* rin = p; p += T;                    // rank inside the token's chunk
    int* lead = p; p += T;                   // the token's chunk leader
    int* cprefix = claim;                    // (claim is dead once the segments are placed)
    int* posseg = pair_chunk;                // (pair_chunk is dead once the prefixes are summed): segment of a sorted position
    int* counters = p;                       // [0] next free position, [1] segments
    float4* part = (float4*)((char*)ws + ((2 * (int64_t)V + 11 * (int64_t)T + 2) * 4 + 15) / 16 * 16);
    hipStream_t st = ST(stream);
    const dim3 g((T + CAT_THREADS - 1) / CAT_THREADS), b(CAT_THREADS);
    const dim3 gc((unsigned)(((int64_t)(T + EMB_CHUNK - 1) / EMB_CHUNK * 64 + CAT_THREADS - 1) / CAT_THREADS));
    if (hipMemsetAsync(counters, 0, 2 * sizeof(int), st) != hipSuccess || hipMemsetAsync(pcount, 0, (size_t)T * sizeof(int), st) != hipSuccess) {
        set_error("gamer_embedding_bwd_large: memset failed");
        return -1;
    }
    hipLaunchKernelGGL(embl_init_kernel, g, b, 0, st, ids, T, V, pad_id, cnt);
    hipLaunchKernelGGL(embl_count_kernel, g, b, 0, st, ids, T, V, pad_id, cnt, claim);
    hipLaunchKernelGGL(embl_place_kernel, g, b, 0, st, ids, T, claim, cnt, segk, counters, seg_start, seg_n, seg_id);
    hipLaunchKernelGGL(embl_chunk_kernel, gc, b, 0, st, ids, T, V, pad_id, segk, seg_start, pcount, pair_chunk, pair_cnt, rin, lead);
    hipLaunchKernelGGL(embl_prefix_kernel, g, b, 0, st, ids, T, V, pad_id, segk, seg_start, pcount, pair_chunk, pair_cnt, rin, cprefix);
    hipLaunchKernelGGL(embl_rank_kernel, g, b, 0, st, ids, T, V, pad_id, segk, seg_start, rin, lead, cprefix, sorted, posseg);
    GAMER_CHECK_LAUNCH("gamer_embedding_bwd_large/sort");
    const dim3 gw((unsigned)(((int64_t)T * 64 + CAT_THREADS - 1) / CAT_THREADS));
    hipLaunchKernelGGL(embl_piece_kernel, gw, b, 0, st, (const float4*)dx, T, H / 4, counters, posseg, seg_start, seg_n, sorted, part);
    hipLaunchKernelGGL(embl_sum_kernel, dim3((unsigned)(((int64_t)T * 64 + CAT_THREADS - 1) / CAT_THREADS)), b, 0, st, (const float4*)dx,
                       T, H / 4, counters, seg_start, seg_n, seg_id, sorted, (const float4*)part, (float4*)dW);
    GAMER_CHECK_LAUNCH("gamer_embedding_bwd_large/sum");
    return 0;
}

extern "C" int64_t gamer_position_bwd_ws_floats(int B, int S, int H) {
    if (B <= 0 || S <= 0 || H <= 0) return -1;
    return (int64_t)((B + POS_BCH - 1) / POS_BCH) * S * H;
}
extern "C" int gamer_position_bwd(const float* dx, int B, int S, int H, float* dP, float* ws, int64_t ws_floats, void* stream) {
    GAMER_CHECK_ARG(dx && dP && ws, "gamer_position_bwd: null pointer");
    GAMER_CHECK_ARG(B > 0 && S > 0 && H > 0 && H % 4 == 0, "gamer_position_bwd: bad shape B=%d S=%d H=%d", B, S, H);
    GAMER_CHECK_ARG(aligned16(dx) && aligned16(dP) && aligned16(ws) && ws_floats >= gamer_position_bwd_ws_floats(B, S, H),
                    "gamer_position_bwd: pointers must be 16-byte aligned and ws hold %lld floats",
                    (long long)gamer_position_bwd_ws_floats(B, S, H));
    const int s4h = S * H / 4, nb = (B + POS_BCH - 1) / POS_BCH;
    hipStream_t st = ST(stream);
    hipLaunchKernelGGL(pos_partial_kernel, dim3((s4h + CAT_THREADS - 1) / CAT_THREADS, nb), dim3(CAT_THREADS), 0, st, (const float4*)dx,
                       B, s4h, (float4*)ws);
    hipLaunchKernelGGL(pos_reduce_kernel, dim3((s4h + CAT_THREADS - 1) / CAT_THREADS), dim3(CAT_THREADS), 0, st, (const float4*)ws, nb,
                       s4h, (float4*)dP);
    GAMER_CHECK_LAUNCH("gamer_position_bwd");
    return 0;
}

extern "C" int gamer_seq_embed_ln_fwd(const int64_t* ids, const float* E, int V, const float* P, int B, int S, int H, const float* w,
                                      const float* b, float eps, float p_drop, uint64_t seed, float* v, float* y, float* mean,
                                      float* rstd, void* stream) {
    GAMER_CHECK_ARG(ids && E && P && w && b && v && y && mean && rstd, "gamer_seq_embed_ln_fwd: null pointer");
    GAMER_CHECK_ARG(B > 0 && S > 0 && V > 0 && H > 0 && H % 4 == 0 && H <= 256 && p_drop >= 0.f && p_drop < 1.f,
                    "gamer_seq_embed_ln_fwd: bad arguments B=%d S=%d V=%d H=%d p=%f (H %% 4 == 0, H <= 256)", B, S, V, H, p_drop);
    GAMER_CHECK_ARG(aligned16(E) && aligned16(P) && aligned16(w) && aligned16(b) && aligned16(v) && aligned16(y),
                    "gamer_seq_embed_ln_fwd: pointers must be 16-byte aligned");
    const int T = B * S;
    hipLaunchKernelGGL(seq_embed_ln_kernel, dim3((unsigned)(((int64_t)T * 64 + CAT_THREADS - 1) / CAT_THREADS)), dim3(CAT_THREADS), 0,
                       ST(stream), ids, E, V, P, T, S, H, w, b, eps, p_drop, seed, v, y, mean, rstd);
    GAMER_CHECK_LAUNCH("gamer_seq_embed_ln_fwd");
    return 0;
}

extern "C" int64_t gamer_cloze_mask_ws_bytes(int B, int L) {
    if (B <= 0 || L <= 0 || (int64_t)B * L > (int64_t)1 << 30) return -1;
    return ((int64_t)((B * L + CLOZE_CHUNK - 1) / CLOZE_CHUNK) * 4 + 15) / 16 * 16;
}
extern "C" int gamer_cloze_mask(const int64_t* ids, const int64_t* seq_len, int B, int L, float mask_ratio, float ft_ratio,
                                int64_t mask_token, int max_seq_length, uint64_t seed, int64_t* masked, int64_t* labels, int64_t* rows,
                                int64_t* targets, int* count, int64_t* words, void* ws, int64_t ws_bytes, void* stream) {
    GAMER_CHECK_ARG(ids && seq_len && masked && labels && rows && targets && count && ws, "gamer_cloze_mask: null pointer");
    GAMER_CHECK_ARG(B > 0 && L > 0 && (int64_t)B * L <= (int64_t)1 << 30 && max_seq_length >= 1 && mask_ratio >= 0.f && ft_ratio >= 0.f,
                    "gamer_cloze_mask: bad arguments B=%d L=%d max_seq_length=%d mask_ratio=%f ft_ratio=%f", B, L, max_seq_length,
                    mask_ratio, ft_ratio);
    GAMER_CHECK_ARG(ws_bytes >= gamer_cloze_mask_ws_bytes(B, L), "gamer_cloze_mask: ws must hold %lld bytes",
                    (long long)gamer_cloze_mask_ws_bytes(B, L));
    const int T = B * L, nchunks = (T + CLOZE_CHUNK - 1) / CLOZE_CHUNK;
    int* chunk_count = (int*)ws;
    hipStream_t st = ST(stream);
    const dim3 g((unsigned)(((int64_t)nchunks * 64 + CAT_THREADS - 1) / CAT_THREADS)), b(CAT_THREADS);
    hipLaunchKernelGGL(cloze_mask_kernel, g, b, 0, st, ids, seq_len, B, L, cloze_thr(mask_ratio), (int)(mask_ratio >= 1.f),
                       cloze_thr(ft_ratio), (int)(ft_ratio >= 1.f), mask_token, max_seq_length, seed, masked, labels, chunk_count, words);
    GAMER_CHECK_LAUNCH("gamer_cloze_mask/mask");
    hipLaunchKernelGGL(cloze_scan_kernel, dim3(1), b, 0, st, chunk_count, nchunks, count);
    GAMER_CHECK_LAUNCH("gamer_cloze_mask/scan");
    hipLaunchKernelGGL(cloze_place_kernel, g, b, 0, st, (const int64_t*)labels, T, (const int*)chunk_count, rows, targets);
    GAMER_CHECK_LAUNCH("gamer_cloze_mask/place");
    return 0;
}
