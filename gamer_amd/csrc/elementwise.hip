// HBM-bound pieces of the Qwen3Multi decoder layer: embedding, RMSNorm, behaviour tables,
// residual/dropout, output gate, temperature cross-entropy (the per-head q/k norm + RoPE and the FFN activations have files of
// their own: qknorm_rope.hip, ffn_act.hip).
// Every kernel moves 16 B per lane and reduces with wave shuffles (wave = 64).
#include "common.h"

namespace gamer {

// ---------------------------------------------------------------------------------------------
// embedding
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(EW_THREADS)
embedding_fwd_kernel(const int64_t* __restrict__ ids, const float4* __restrict__ W, int V, int T, int H4,
                     float4* __restrict__ x) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * EW_THREADS + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * EW_THREADS) >> 6;
    for (int t = wave; t < T; t += nwaves) {
        const int64_t id = ids[t];
        const bool ok = id >= 0 && id < V;
        for (int c = lane; c < H4; c += 64) {
            float4 v = ok ? W[id * H4 + c] : make_float4(0.f, 0.f, 0.f, 0.f);
            x[(int64_t)t * H4 + c] = v;
        }
    }
}

// Scatter-add of d(embedding output) into the table gradient.  A few rows are hot (the behaviour tokens: every fifth
// token of the batch lands on one of NB rows) and same-address float atomics serialise in L2: 2.06 ms at T = 517k with
// one global atomic per element.  Each workgroup therefore takes a contiguous chunk of tokens, caches the first
// EMB_CACHE distinct ids of its chunk in LDS (the hot ids are among them: a chunk starts with a behaviour token),
// accumulates those rows with LDS atomics and flushes them once; every other row goes straight to global atomics.
constexpr int EMB_CACHE = 8;
constexpr int EMB_CHUNK = 1024;          // tokens per workgroup at large T; smaller chunks keep >= ~512 workgroups at small T
__global__ void __launch_bounds__(EW_THREADS)
embedding_bwd_kernel(const int64_t* __restrict__ ids, const float* __restrict__ dx, int V, int T, int H,
                     int pad_id, float* __restrict__ dW, const int chunk) {
    extern __shared__ __attribute__((aligned(16))) float emb_cache[];       // [EMB_CACHE][H]
    __shared__ int64_t cache_id[EMB_CACHE];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int t0 = blockIdx.x * chunk, t1 = min(T, t0 + chunk);
    for (int e = threadIdx.x; e < EMB_CACHE * H; e += EW_THREADS) emb_cache[e] = 0.f;
    if (threadIdx.x == 0) {
        int n = 0;
        for (int i = 0; i < EMB_CACHE; ++i) cache_id[i] = -1;
        for (int t = t0; t < t1 && t < t0 + 64 && n < EMB_CACHE; ++t) {
            const int64_t id = ids[t];
            if (id == pad_id || id < 0 || id >= V) continue;
            bool seen = false;
            for (int i = 0; i < n; ++i) seen |= cache_id[i] == id;
            if (!seen) cache_id[n++] = id;
        }
    }
    __syncthreads();
    for (int t = t0 + w; t < t1; t += EW_THREADS / 64) {
        const int64_t id = ids[t];
        if (id == pad_id || id < 0 || id >= V) continue;   // wave-uniform
        int slot = -1;
#pragma unroll
        for (int i = 0; i < EMB_CACHE; ++i) slot = cache_id[i] == id ? i : slot;
        if (slot >= 0) {
            for (int c = lane; c < H; c += 64) atomicAdd(&emb_cache[slot * H + c], dx[(int64_t)t * H + c]);
        } else {
            for (int c = lane; c < H; c += 64) atomicAdd(&dW[id * H + c], dx[(int64_t)t * H + c]);
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < EMB_CACHE * H; e += EW_THREADS) {
        const int64_t id = cache_id[e / H];
        const float v = emb_cache[e];
        if (id >= 0 && v != 0.f) atomicAdd(&dW[id * H + e % H], v);
    }
}

// ---- the same gradient without float atomics: a stable counting sort of the tokens by id, then sums in sorted order ----
// (1) per-chunk histograms of the ids (integer LDS atomics: the counts do not depend on their order), (2) one workgroup turns
// them into every chunk's write cursors (rows ascending, chunks ascending inside a row: a STABLE order) and cuts every row's
// token list into pieces of EMB_PIECE tokens, (3) every chunk writes its token indices to their sorted positions in token
// order, (4) one workgroup per piece adds its <= EMB_PIECE rows of dx in sorted order, (5) one workgroup per table row adds its
// pieces in order into dW.  Same bits on every run; 517k tokens x 256: five launches, ~0.3 ms (the atomic form: 0.75 ms).
constexpr int EMB_SORT_CHUNK = 1024;
constexpr int EMB_PIECE = 256;
constexpr int EMB_MAX_V = 8191;          // (V + 1 counters in LDS)
struct EmbSortWs { int* hist; int* row_start; int* row_count; int* piece_start; int* perm; float* partial; };

__global__ void __launch_bounds__(EW_THREADS)
emb_hist_kernel(const int64_t* __restrict__ ids, int V, int T, int pad_id, int* __restrict__ hist) {
    extern __shared__ int emb_cnt[];                             // [V + 1]: bucket V = padding / out-of-range ids
    for (int v = threadIdx.x; v <= V; v += EW_THREADS) emb_cnt[v] = 0;
    __syncthreads();
    const int t0 = blockIdx.x * EMB_SORT_CHUNK, t1 = min(T, t0 + EMB_SORT_CHUNK);
    for (int t = t0 + threadIdx.x; t < t1; t += EW_THREADS) {
        const int64_t id = ids[t];
        atomicAdd(&emb_cnt[(id == pad_id || id < 0 || id >= V) ? V : (int)id], 1);
    }
    __syncthreads();
    for (int v = threadIdx.x; v <= V; v += EW_THREADS) hist[(int64_t)blockIdx.x * (V + 1) + v] = emb_cnt[v];
}

// one wave per table row v: hist[c][v] -> exclusive prefix over the chunks c, row_count[v] = the row's total
__global__ void __launch_bounds__(64)
emb_chunk_scan_kernel(int V, int n_chunks, int* __restrict__ hist, int* __restrict__ row_count) {
    const int v = blockIdx.x, lane = threadIdx.x;
    int carry = 0;
    for (int c0 = 0; c0 < n_chunks; c0 += 64) {
        const int c = c0 + lane;
        const int h = c < n_chunks ? hist[(int64_t)c * (V + 1) + v] : 0;
        int incl = h;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (c < n_chunks) hist[(int64_t)c * (V + 1) + v] = carry + incl - h;
        carry += __shfl(incl, 63, 64);
    }
    if (lane == 0) row_count[v] = carry;
}
// one workgroup: row_start[v] = tokens in front of row v, piece_start[v] = pieces in front of it (v = 0 .. V; [V + 1] = the end)
__global__ void __launch_bounds__(1024)
emb_row_scan_kernel(int V, const int* __restrict__ row_count, int* __restrict__ row_start, int* __restrict__ piece_start) {
    __shared__ int s_tok[1024], s_pc[1024];
    const int tid = threadIdx.x;
    const int per = (V + 1 + 1023) / 1024;                        // rows per thread (<= 8)
    int tok = 0, pc = 0;
    for (int i = 0; i < per; ++i) {
        const int v = tid * per + i;
        if (v <= V) {
            const int n = row_count[v];
            tok += n;
            if (v < V) pc += (n + EMB_PIECE - 1) / EMB_PIECE;
        }
    }
    s_tok[tid] = tok; s_pc[tid] = pc;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {                          // inclusive scans of the per-thread sums
        const int a = tid >= o ? s_tok[tid - o] : 0, b = tid >= o ? s_pc[tid - o] : 0;
        __syncthreads();
        s_tok[tid] += a; s_pc[tid] += b;
        __syncthreads();
    }
    int t_run = s_tok[tid] - tok, p_run = s_pc[tid] - pc;
    for (int i = 0; i < per; ++i) {
        const int v = tid * per + i;
        if (v <= V) {
            row_start[v] = t_run;
            piece_start[v] = p_run;
            const int n = row_count[v];
            t_run += n;
            if (v < V) p_run += (n + EMB_PIECE - 1) / EMB_PIECE;
        }
    }
    if (tid == 1023) piece_start[V + 1] = s_pc[1023];
}

__global__ void __launch_bounds__(EW_THREADS)
emb_scatter_kernel(const int64_t* __restrict__ ids, int V, int T, int pad_id, const int* __restrict__ hist,
                   const int* __restrict__ row_start, int* __restrict__ perm) {
    extern __shared__ int emb_cur[];                             // [V + 1] write cursors of this chunk, then its [1024] buckets
    int* bucket = emb_cur + V + 1;
    const int t0 = blockIdx.x * EMB_SORT_CHUNK, t1 = min(T, t0 + EMB_SORT_CHUNK);
    for (int v = threadIdx.x; v <= V; v += EW_THREADS) emb_cur[v] = row_start[v] + hist[(int64_t)blockIdx.x * (V + 1) + v];
    for (int t = t0 + threadIdx.x; t < t1; t += EW_THREADS) {
        const int64_t id = ids[t];
        bucket[t - t0] = (id == pad_id || id < 0 || id >= V) ? -1 : (int)id;
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        // token order inside the chunk: ONE wave walks it 64 tokens at a time.  A lane's position = its row's cursor + the number of
        // earlier lanes of the batch with the same id; the last lane of every id moves the cursor on.  (A single thread walking
        // the 1024 tokens took 120-150 us per launch - every step a dependent LDS round trip.)
        const int lane = threadIdx.x;
        for (int tb = t0; tb < t1; tb += 64) {
            const int t = tb + lane;
            const int b = t < t1 ? bucket[t - t0] : -1;
            int rank = 0, cnt = 0;
            for (int j = 0; j < 64; ++j) {
                const int bj = __shfl(b, j, 64);
                const bool same = bj == b;
                rank += (same && j < lane) ? 1 : 0;
                cnt += same ? 1 : 0;
            }
            if (b >= 0) {
                const int pos = emb_cur[b] + rank;               // (every lane reads before any lane of this batch writes)
                perm[pos] = t;
                __builtin_amdgcn_wave_barrier();
                if (rank == cnt - 1) emb_cur[b] = pos + 1;
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}

__global__ void __launch_bounds__(EW_THREADS)
emb_piece_sum_kernel(const float4* __restrict__ dx, int V, int H4, const int* __restrict__ row_start, const int* __restrict__ row_count,
                     const int* __restrict__ piece_start, const int* __restrict__ perm, float4* __restrict__ partial) {
    __shared__ float4 red[3][256];
    const int p = blockIdx.x;
    if (p >= piece_start[V]) return;
    int lo = 0, hi = V;                                          // the row of piece p: last v with piece_start[v] <= p
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (piece_start[mid] <= p) lo = mid; else hi = mid; }
    const int v = lo, k = p - piece_start[v];
    const int begin = row_start[v] + k * EMB_PIECE;
    const int count = min(EMB_PIECE, row_count[v] - k * EMB_PIECE);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // wave w adds tokens [w * 64, w * 64 + 64) of the piece in order; the four sums are then combined in a fixed order
    for (int c0 = 0; c0 < H4; c0 += 64) {
        const int c = c0 + lane;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < H4) {
            const int j1 = min(count, (w + 1) * (EMB_PIECE / 4));
            int j = w * (EMB_PIECE / 4);
            for (; j + 4 <= j1; j += 4) {
                const int r0 = perm[begin + j], r1 = perm[begin + j + 1], r2 = perm[begin + j + 2], r3 = perm[begin + j + 3];
                const float4 a0 = dx[(int64_t)r0 * H4 + c], a1 = dx[(int64_t)r1 * H4 + c], a2 = dx[(int64_t)r2 * H4 + c],
                             a3 = dx[(int64_t)r3 * H4 + c];
                acc.x = (((acc.x + a0.x) + a1.x) + a2.x) + a3.x; acc.y = (((acc.y + a0.y) + a1.y) + a2.y) + a3.y;
                acc.z = (((acc.z + a0.z) + a1.z) + a2.z) + a3.z; acc.w = (((acc.w + a0.w) + a1.w) + a2.w) + a3.w;
            }
            for (; j < j1; ++j) {
                const float4 a0 = dx[(int64_t)perm[begin + j] * H4 + c];
                acc.x += a0.x; acc.y += a0.y; acc.z += a0.z; acc.w += a0.w;
            }
        }
        if (w > 0 && c < H4) red[w - 1][lane] = acc;
        __syncthreads();
        if (w == 0 && c < H4) {
            const float4 b = red[0][lane], d = red[1][lane], e = red[2][lane];
            float4 o;
            o.x = (acc.x + b.x) + (d.x + e.x); o.y = (acc.y + b.y) + (d.y + e.y);
            o.z = (acc.z + b.z) + (d.z + e.z); o.w = (acc.w + b.w) + (d.w + e.w);
            partial[(int64_t)p * H4 + c] = o;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(64)
emb_row_sum_kernel(int H4, const int* __restrict__ piece_start, const float4* __restrict__ partial, float4* __restrict__ dW) {
    const int v = blockIdx.x;
    const int p0 = piece_start[v], p1 = piece_start[v + 1];
    if (p0 == p1) return;
    for (int c = threadIdx.x; c < H4; c += 64) {
        float4 s = partial[(int64_t)p0 * H4 + c];
        for (int p = p0 + 1; p < p1; ++p) {
            const float4 a = partial[(int64_t)p * H4 + c];
            s.x += a.x; s.y += a.y; s.z += a.z; s.w += a.w;
        }
        float4 o = dW[(int64_t)v * H4 + c];
        o.x += s.x; o.y += s.y; o.z += s.z; o.w += s.w;
        dW[(int64_t)v * H4 + c] = o;
    }
}

// ---------------------------------------------------------------------------------------------
// RMSNorm (hidden dim H <= 1024, H % 4 == 0); one wave per row, row cached in registers
// ---------------------------------------------------------------------------------------------
// float4 chunks per lane: 1 for H <= 256 (the shipped hidden size: one chunk per lane, 4x fewer registers - the
// 4-chunk form sat at 134 VGPRs = 3 waves per SIMD after the dtype templating, 9.2 -> 12.3 ms per step), 4 for H <= 1024
constexpr int RMS_MAXC_BIG = 4;

template <typename TY, int RMS_MAXC>
__global__ void __launch_bounds__(EW_THREADS)
rmsnorm_fwd_kernel(const float4* __restrict__ x, const float4* __restrict__ w, int T, int H4, float inv_h,
                   float eps, const int32_t* __restrict__ dst_rows, TY* __restrict__ y, int ldy, uint32_t* __restrict__ amax_out) {
    __shared__ uint32_t amax_lds[4];
    uint32_t am = 0;
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * EW_THREADS + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * EW_THREADS) >> 6;
    float4 wv[RMS_MAXC];
#pragma unroll
    for (int i = 0; i < RMS_MAXC; ++i) {
        const int c = lane + 64 * i;
        wv[i] = (c < H4) ? w[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int t = wave; t < T; t += nwaves) {
        float4 v[RMS_MAXC];
        float ss = 0.f;
#pragma unroll
        for (int i = 0; i < RMS_MAXC; ++i) {
            const int c = lane + 64 * i;
            v[i] = (c < H4) ? x[(int64_t)t * H4 + c] : make_float4(0.f, 0.f, 0.f, 0.f);
            ss += v[i].x * v[i].x + v[i].y * v[i].y + v[i].z * v[i].z + v[i].w * v[i].w;
        }
        ss = wave_sum(ss);
        const float rstd = rsqrtf(ss * inv_h + eps);
        const int64_t r = dst_rows ? dst_rows[t] : t;
        TY* yrow = y + r * ldy;
#pragma unroll
        for (int i = 0; i < RMS_MAXC; ++i) {
            const int c = lane + 64 * i;
            if (c < H4) {
                float4 o;
                o.x = wv[i].x * (v[i].x * rstd);
                o.y = wv[i].y * (v[i].y * rstd);
                o.z = wv[i].z * (v[i].z * rstd);
                o.w = wv[i].w * (v[i].w * rstd);
                st4(yrow + 4 * c, o);
                am = amax_f4(am, o);
            }
        }
    }
    amax_block_commit(am, amax_out, amax_lds);
}

// dx (+)= rstd*(w*dy - xhat*mean(w*dy*xhat)); per-workgroup dw partial sums (deterministic).
template <typename TG, int RMS_MAXC>
__global__ void __launch_bounds__(EW_THREADS)
rmsnorm_bwd_kernel(const float4* __restrict__ x, const float4* __restrict__ w, const TG* __restrict__ dy,
                   int lddy, const int32_t* __restrict__ dy_rows, int T, int H4, float inv_h, float eps,
                   int accumulate_dx, float4* __restrict__ dx, float* __restrict__ dw_partial,
                   TG* __restrict__ mask_out, const int32_t* __restrict__ mask_rows, float p_drop, uint64_t seed,
                   uint32_t* __restrict__ amax_out) {
    // mask_out != nullptr: the next consumer of dx is a residual branch with dropout; its input gradient
    // mask(seed) * dx is written here (what gamer_residual_dropout_bwd would compute in a second pass over dx)
    // amax_out: max |mask_out| (the GEMM operand of that branch)
    const DropoutRng rng(mask_out ? p_drop : 0.f, seed);
    __shared__ float4 red[EW_WAVES][64 * RMS_MAXC];
    __shared__ uint32_t amax_lds[4];
    uint32_t am = 0;
    const int lane = threadIdx.x & 63;
    const int wib = threadIdx.x >> 6;
    const int wave = (blockIdx.x * EW_THREADS + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * EW_THREADS) >> 6;
    float4 wv[RMS_MAXC], dwacc[RMS_MAXC];
#pragma unroll
    for (int i = 0; i < RMS_MAXC; ++i) {
        const int c = lane + 64 * i;
        wv[i] = (c < H4) ? w[c] : make_float4(0.f, 0.f, 0.f, 0.f);
        dwacc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // (Measured and not kept: two rows per iteration with the dx read hoisted in front of the reductions - 0.58 -> 0.39 ms on a
    // 512-workgroup grid, but the engine launches 2048 workgroups (8 waves per SIMD, 5.9 TB/s with the mask output) and there the
    // extra registers cost occupancy: 0.45 -> 0.51 ms per call.)
    for (int t = wave; t < T; t += nwaves) {
        float4 v[RMS_MAXC], g[RMS_MAXC];
        float ss = 0.f;
        const int64_t r = dy_rows ? dy_rows[t] : t;
        const TG* dyrow = dy + r * lddy;
#pragma unroll
        for (int i = 0; i < RMS_MAXC; ++i) {
            const int c = lane + 64 * i;
            v[i] = (c < H4) ? x[(int64_t)t * H4 + c] : make_float4(0.f, 0.f, 0.f, 0.f);
            g[i] = (c < H4) ? ld4(dyrow + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
            ss += v[i].x * v[i].x + v[i].y * v[i].y + v[i].z * v[i].z + v[i].w * v[i].w;
        }
        ss = wave_sum(ss);
        const float rstd = rsqrtf(ss * inv_h + eps);
        float dot = 0.f;
#pragma unroll
        for (int i = 0; i < RMS_MAXC; ++i) {
            // xhat
            v[i].x *= rstd; v[i].y *= rstd; v[i].z *= rstd; v[i].w *= rstd;
            dwacc[i].x += g[i].x * v[i].x; dwacc[i].y += g[i].y * v[i].y;
            dwacc[i].z += g[i].z * v[i].z; dwacc[i].w += g[i].w * v[i].w;
            g[i].x *= wv[i].x; g[i].y *= wv[i].y; g[i].z *= wv[i].z; g[i].w *= wv[i].w;
            dot += g[i].x * v[i].x + g[i].y * v[i].y + g[i].z * v[i].z + g[i].w * v[i].w;
        }
        dot = wave_sum(dot) * inv_h;
#pragma unroll
        for (int i = 0; i < RMS_MAXC; ++i) {
            const int c = lane + 64 * i;
            if (c < H4) {
                float4 o;
                o.x = rstd * (g[i].x - v[i].x * dot);
                o.y = rstd * (g[i].y - v[i].y * dot);
                o.z = rstd * (g[i].z - v[i].z * dot);
                o.w = rstd * (g[i].w - v[i].w * dot);
                if (accumulate_dx) {
                    float4 p = dx[(int64_t)t * H4 + c];
                    o.x += p.x; o.y += p.y; o.z += p.z; o.w += p.w;
                }
                dx[(int64_t)t * H4 + c] = o;
                if (mask_out) {
                    float m[4];
                    rng.mult4((uint32_t)((int64_t)t * H4 + c), m);
                    const int64_t mr = mask_rows ? mask_rows[t] : t;
                    const float4 mo = make_float4(m[0] * o.x, m[1] * o.y, m[2] * o.z, m[3] * o.w);
                    st4(mask_out + (mr * H4 + c) * 4, mo);
                    am = amax_f4(am, mo);
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < RMS_MAXC; ++i) red[wib][lane + 64 * i] = dwacc[i];
    __syncthreads();
    if (wib == 0) {
#pragma unroll
        for (int i = 0; i < RMS_MAXC; ++i) {
            const int c = lane + 64 * i;
            if (c < H4) {
                float4 s = red[0][c];
                for (int ww = 1; ww < EW_WAVES; ++ww) {
                    float4 o = red[ww][c];
                    s.x += o.x; s.y += o.y; s.z += o.z; s.w += o.w;
                }
                reinterpret_cast<float4*>(dw_partial + (int64_t)blockIdx.x * H4 * 4)[c] = s;
            }
        }
    }
    amax_block_commit(am, mask_out ? amax_out : nullptr, amax_lds);
}

// out[c] (+)= sum_r partial[r][c]; one workgroup per 32 columns, 32 row groups per workgroup, four independent
// loads in flight per thread, fixed summation order (deterministic).  (With 8 row groups and one load at a time
// the 2048-row partial tables of the norm backward took 82 us per call, 21 calls per step.)
constexpr int COLSUM_RG = 32;
__global__ void __launch_bounds__(32 * COLSUM_RG)
colsum_reduce_kernel(const float* __restrict__ partial, int rows, int cols, int accumulate,
                     float* __restrict__ out) {
    __shared__ float sh[COLSUM_RG][32];
    const int cl = threadIdx.x & 31, rg = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (c < cols) {
        int r = rg;
        for (; r + 3 * COLSUM_RG < rows; r += 4 * COLSUM_RG) {
            s0 += partial[(int64_t)r * cols + c];
            s1 += partial[(int64_t)(r + COLSUM_RG) * cols + c];
            s2 += partial[(int64_t)(r + 2 * COLSUM_RG) * cols + c];
            s3 += partial[(int64_t)(r + 3 * COLSUM_RG) * cols + c];
        }
        for (; r < rows; r += COLSUM_RG) s0 += partial[(int64_t)r * cols + c];
    }
    sh[rg][cl] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (rg == 0 && c < cols) {
        float t = 0.f;
#pragma unroll
        for (int g = 0; g < COLSUM_RG; ++g) t += sh[g][cl];
        out[c] = accumulate ? out[c] + t : t;
    }
}

// n tables [rows][cols] `stride` floats apart, each summed into its own output vector outs[i]: the RMSNorm weight gradients of
// a whole backward pass in ONE launch at its end (they belong to the tail bucket of the gradient all-reduce) instead of one
// 7-us launch behind every norm backward - 25 launches per step, 0.6 % of the step at per-GPU batch 128.
__global__ void __launch_bounds__(32 * COLSUM_RG)
colsum_reduce_batched_kernel(const float* __restrict__ partial, int64_t stride, int rows, int cols, int accumulate,
                             float* const* __restrict__ outs) {
    __shared__ float sh[COLSUM_RG][32];
    const int cl = threadIdx.x & 31, rg = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl;
    const float* pt = partial + (int64_t)blockIdx.y * stride;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (c < cols) {
        int r = rg;
        for (; r + 3 * COLSUM_RG < rows; r += 4 * COLSUM_RG) {
            s0 += pt[(int64_t)r * cols + c];
            s1 += pt[(int64_t)(r + COLSUM_RG) * cols + c];
            s2 += pt[(int64_t)(r + 2 * COLSUM_RG) * cols + c];
            s3 += pt[(int64_t)(r + 3 * COLSUM_RG) * cols + c];
        }
        for (; r < rows; r += COLSUM_RG) s0 += pt[(int64_t)r * cols + c];
    }
    sh[rg][cl] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (rg == 0 && c < cols) {
        float t = 0.f;
#pragma unroll
        for (int g = 0; g < COLSUM_RG; ++g) t += sh[g][cl];
        float* out = outs[blockIdx.y];
        out[c] = accumulate ? out[c] + t : t;
    }
}

// ---------------------------------------------------------------------------------------------
// small-table rows (behaviour embeddings)
// ---------------------------------------------------------------------------------------------
template <typename TY>
__global__ void __launch_bounds__(EW_THREADS)
rowtable_fwd_kernel(const float4* __restrict__ table, const int32_t* __restrict__ idx,
                    const int32_t* __restrict__ dst_rows, int T, int E4, TY* __restrict__ y, int ldy, int col0,
                    uint32_t* __restrict__ amax_out) {
    __shared__ uint32_t amax_lds[4];
    uint32_t am = 0;
    const int64_t total = (int64_t)T * E4;
    for (int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * EW_THREADS) {
        const int t = (int)(i / E4);
        const int c = (int)(i % E4);
        const int64_t r = dst_rows ? dst_rows[t] : t;
        const float4 v = table[(int64_t)idx[t] * E4 + c];
        st4(y + r * ldy + col0 + 4 * c, v);
        am = amax_f4(am, v);
    }
    amax_block_commit(am, amax_out, amax_lds);
}


// dtable[idx[t]][c] += dy[src(t)][col0+c]; per-thread predicated accumulators, LDS combine, one
// atomic per workgroup per table element.
// DET (a `partial` workspace was given): no atomics at all - the row groups of a workgroup are added in row-group order through
// LDS, the workgroup's table goes to partial[block] and gamer_colsum_reduce's kernel folds the blocks in block order.
template <typename TG, bool DET>
__global__ void __launch_bounds__(EW_THREADS)
rowtable_bwd_kernel(const TG* __restrict__ dy, int lddy, int col0, const int32_t* __restrict__ idx,
                    const int32_t* __restrict__ dy_rows, int T, int E4, int nrows, float* __restrict__ dtable,
                    float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float lds_tbl[];   // [nrows][E4*4]; DET: [row groups][nrows][E4*4]
    const int E = E4 * 4;
    if (!DET) {
        for (int i = threadIdx.x; i < nrows * E; i += EW_THREADS) lds_tbl[i] = 0.f;
        __syncthreads();
    }
    const int c = threadIdx.x % E4;
    const int rl = threadIdx.x / E4;
    const int rows_per_block = EW_THREADS / E4;
    float4 acc[TBL_MAXROWS];
#pragma unroll
    for (int a = 0; a < TBL_MAXROWS; ++a) acc[a] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (rl < rows_per_block) {
        for (int64_t t = (int64_t)blockIdx.x * rows_per_block + rl; t < T; t += (int64_t)gridDim.x * rows_per_block) {
            const int64_t r = dy_rows ? dy_rows[t] : t;
            const float4 g = ld4(dy + r * lddy + col0 + 4 * c);
            const int a_t = idx[t];
#pragma unroll
            for (int a = 0; a < TBL_MAXROWS; ++a) {
                const float m = (a_t == a) ? 1.f : 0.f;
                acc[a].x += m * g.x; acc[a].y += m * g.y; acc[a].z += m * g.z; acc[a].w += m * g.w;
            }
        }
#pragma unroll
        for (int a = 0; a < TBL_MAXROWS; ++a) {
            if (a < nrows) {
                if (DET) {
                    *reinterpret_cast<float4*>(&lds_tbl[(rl * nrows + a) * E + c * 4]) = acc[a];
                } else {
                    atomicAdd(&lds_tbl[a * E + c * 4 + 0], acc[a].x);
                    atomicAdd(&lds_tbl[a * E + c * 4 + 1], acc[a].y);
                    atomicAdd(&lds_tbl[a * E + c * 4 + 2], acc[a].z);
                    atomicAdd(&lds_tbl[a * E + c * 4 + 3], acc[a].w);
                }
            }
        }
    }
    __syncthreads();
    if (DET) {
        for (int i = threadIdx.x; i < nrows * E; i += EW_THREADS) {
            float t = 0.f;
            for (int g = 0; g < rows_per_block; ++g) t += lds_tbl[g * nrows * E + i];
            partial[(int64_t)blockIdx.x * nrows * E + i] = t;
        }
    } else {
        for (int i = threadIdx.x; i < nrows * E; i += EW_THREADS) atomicAdd(&dtable[i], lds_tbl[i]);
    }
}

// ---------------------------------------------------------------------------------------------
// residual + dropout, SwiGLU, SiLU gate
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(EW_THREADS)
residual_dropout_fwd_kernel(const float4* x_in, const float4* __restrict__ delta,
                            const int32_t* __restrict__ src_rows, int T, int H4, float p, uint64_t seed,
                            float4* x_out) {
    const DropoutRng rng(p, seed);
    const int64_t total = (int64_t)T * H4;
    for (int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * EW_THREADS) {
        const int t = (int)(i / H4);
        const int c = (int)(i % H4);
        const int64_t r = src_rows ? src_rows[t] : t;
        const float4 d = delta[r * H4 + c];
        float4 v = x_in[i];
        float m[4];
        rng.mult4((uint32_t)i, m);
        v.x += m[0] * d.x; v.y += m[1] * d.y; v.z += m[2] * d.z; v.w += m[3] * d.w;
        x_out[i] = v;
    }
}

__global__ void __launch_bounds__(EW_THREADS)
residual_dropout_bwd_kernel(const float4* __restrict__ dx, const int32_t* __restrict__ src_rows, int T, int H4,
                            float p, uint64_t seed, float4* __restrict__ ddelta) {
    const DropoutRng rng(p, seed);
    const int64_t total = (int64_t)T * H4;
    for (int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * EW_THREADS) {
        const int t = (int)(i / H4);
        const int c = (int)(i % H4);
        const int64_t r = src_rows ? src_rows[t] : t;
        const float4 g = dx[i];
        float m[4];
        rng.mult4((uint32_t)i, m);
        float4 o;
        o.x = m[0] * g.x; o.y = m[1] * g.y; o.z = m[2] * g.z; o.w = m[3] * g.w;
        ddelta[r * H4 + c] = o;
    }
}

// TO = type of `out`: the residual stream (fp32) when resid is given, otherwise the activation type
template <typename TA, typename TO>
__global__ void __launch_bounds__(EW_THREADS)
silu_gate_fwd_kernel(const TA* __restrict__ a, const TA* __restrict__ gate, int64_t n4,
                     TO* __restrict__ out, const float4* __restrict__ resid, float p, uint64_t seed) {
    // resid != nullptr: out = resid + dropout(a * silu(gate)) - the residual add of the cross-attention block fused
    // in (same mask as gamer_residual_dropout_fwd with this seed: element index -> mult4)
    const DropoutRng rng(resid ? p : 0.f, seed);
    for (int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; i < n4; i += (int64_t)gridDim.x * EW_THREADS) {
        const float4 x = ld4(a + 4 * i), g = ld4(gate + 4 * i);
        float4 o;
        o.x = x.x * silu_f(g.x); o.y = x.y * silu_f(g.y); o.z = x.z * silu_f(g.z); o.w = x.w * silu_f(g.w);
        if (resid) {
            const float4 r = resid[i];
            float m[4];
            rng.mult4((uint32_t)i, m);
            o.x = r.x + m[0] * o.x; o.y = r.y + m[1] * o.y; o.z = r.z + m[2] * o.z; o.w = r.w + m[3] * o.w;
        }
        st4(out + 4 * i, o);
    }
}

template <typename TA>
__global__ void __launch_bounds__(EW_THREADS)
silu_gate_bwd_kernel(const TA* __restrict__ a, const TA* __restrict__ gate, const float4* __restrict__ dout,
                     int64_t n4, TA* __restrict__ da, TA* __restrict__ dgate, float p, uint64_t seed,
                     uint32_t* __restrict__ amax_a, uint32_t* __restrict__ amax_gate) {
    // p > 0: dout is the gradient of the residual stream; the dropout mask of the fused forward is applied first
    __shared__ uint32_t amax_lds[2][4];
    uint32_t ama = 0, amg = 0;
    const DropoutRng rng(p, seed);
    for (int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; i < n4; i += (int64_t)gridDim.x * EW_THREADS) {
        const float4 x = ld4(a + 4 * i), g = ld4(gate + 4 * i);
        float4 d = dout[i];
        float m[4];
        rng.mult4((uint32_t)i, m);
        d.x *= m[0]; d.y *= m[1]; d.z *= m[2]; d.w *= m[3];
        float4 oa, og;
        oa.x = d.x * silu_f(g.x); og.x = d.x * x.x * dsilu_f(g.x);
        oa.y = d.y * silu_f(g.y); og.y = d.y * x.y * dsilu_f(g.y);
        oa.z = d.z * silu_f(g.z); og.z = d.z * x.z * dsilu_f(g.z);
        oa.w = d.w * silu_f(g.w); og.w = d.w * x.w * dsilu_f(g.w);
        st4(da + 4 * i, oa);
        st4(dgate + 4 * i, og);
        ama = amax_f4(ama, oa);
        amg = amax_f4(amg, og);
    }
    amax_block_commit(ama, amax_a, amax_lds[0]);
    amax_block_commit(amg, amax_gate, amax_lds[1]);
}

// ---------------------------------------------------------------------------------------------
// temperature + shifted cross entropy; one wave per row of logits (TL = fp32, or bf16 as the reference's autocast
// lm_head produces them; the statistics are fp32 either way, loss_utils.py upcasts)
// ---------------------------------------------------------------------------------------------
constexpr int CE_MAXC = 20;              // register-resident rows up to V = 1280 (the shipped vocabulary is 1041)
template <typename T> constexpr int CE_EPL = 16 / (int)sizeof(T);      // elements per 16 bytes
// ... as 16-byte groups per lane: five cover 1280 fp32 values, three 1536 bf16 values (five for bf16 too meant 40 exponentials per
// lane for the 17 values it owns at V = 1041)
template <typename T> constexpr int CE_MAXQ = sizeof(T) == 2 ? 3 : 5;
__device__ __forceinline__ void ce_load16(const float* p, float (&x)[4]) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
}
__device__ __forceinline__ void ce_store16(float* p, const float (&x)[4]) { *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]); }
__device__ __forceinline__ void ce_load16(const bf16_t* p, float (&x)[8]) {
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = (float)v[e];
}
__device__ __forceinline__ void ce_store16(bf16_t* p, const float (&x)[8]) {
    bf16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (bf16_t)x[e];
    *reinterpret_cast<bf16x8*>(p) = v;
}
template <typename TL>
__global__ void __launch_bounds__(EW_THREADS)
ce_fwd_kernel(TL* __restrict__ logits, int ldl, const int64_t* __restrict__ labels, int T, int S, int V,
              float inv_temp, int ignore_index, float* __restrict__ lse_out, float* __restrict__ row_loss, int vec4) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * EW_THREADS + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * EW_THREADS) >> 6;
    for (int t = wave; t < T; t += nwaves) {
        TL* row = logits + (int64_t)t * ldl;
        const int s = t % S;
        const int64_t tgt = (s + 1 < S) ? labels[t + 1] : (int64_t)ignore_index;
        const bool valid = tgt != ignore_index && tgt >= 0 && tgt < V;
        float mx = -INFINITY;
        float zt = 0.f;
        if (vec4 && V <= 64 * CE_EPL<TL> * CE_MAXQ<TL>) {
            // rows with 16-byte aligned starts: the row in registers as 16-byte groups per lane (four fp32 / eight bf16 values; one wave
            // instruction moves 1 KB instead of 256 / 128 bytes: fp32 3.6 -> 5 TB/s, bf16 2.2 -> ...); the group that straddles V is
            // stored element by element - the padding columns of the row stay as they are
            constexpr int EPL = CE_EPL<TL>;
            float z[CE_MAXQ<TL>][EPL];
            const int c_last = ((V - 1) / EPL) * EPL;      // every load is unconditional (a group past the row reads the row's last group and
#pragma unroll                                            // is masked): loads under `if (c < V)` were each waited for right behind the load
            for (int i = 0; i < CE_MAXQ<TL>; ++i) {
                const int c = EPL * (lane + 64 * i);
                float x[EPL];
                ce_load16(row + min(c, c_last), x);
#pragma unroll
                for (int e = 0; e < EPL; ++e) z[i][e] = c + e < V ? round_as<TL>(x[e] * inv_temp) : -INFINITY;
            }
#pragma unroll
            for (int i = 0; i < CE_MAXQ<TL>; ++i) {
                const int c = EPL * (lane + 64 * i);
                if (inv_temp == 1.f) {
                    // the producer already divided by the temperature (the head GEMM's alpha): nothing to write back
                } else if (c + EPL <= V) {
                    ce_store16(row + c, z[i]);
                } else if (c < V) {
#pragma unroll
                    for (int e = 0; e < EPL; ++e)
                        if (c + e < V) st1(row + c + e, z[i][e]);
                }
#pragma unroll
                for (int e = 0; e < EPL; ++e) {
                    mx = fmaxf(mx, z[i][e]);
                    if (valid && c + e == (int)tgt) zt = z[i][e];
                }
            }
            mx = wave_max(mx);
            zt = wave_sum(zt);
            float se = 0.f;
#pragma unroll
            for (int i = 0; i < CE_MAXQ<TL>; ++i)
#pragma unroll
                for (int e = 0; e < EPL; ++e) se += expf(z[i][e] - mx);           // exp(-inf) = 0 past the row
            se = wave_sum(se);
            const float lse = mx + logf(se);
            if (lane == 0) {
                lse_out[t] = lse;
                row_loss[t] = valid ? (lse - zt) : 0.f;
            }
            continue;
        }
        if (V <= 64 * CE_MAXC) {
            // the whole row in registers: one read (all loads in flight together), one write, no second pass
            float z[CE_MAXC];
#pragma unroll
            for (int i = 0; i < CE_MAXC; ++i) {
                const int c = lane + 64 * i;
                z[i] = c < V ? round_as<TL>(ld1(row + c) * inv_temp) : -INFINITY;
            }
#pragma unroll
            for (int i = 0; i < CE_MAXC; ++i) {
                const int c = lane + 64 * i;
                if (c < V) st1(row + c, z[i]);
                mx = fmaxf(mx, z[i]);
                if (valid && c == (int)tgt) zt = z[i];
            }
            mx = wave_max(mx);
            zt = wave_sum(zt);
            float se = 0.f;
#pragma unroll
            for (int i = 0; i < CE_MAXC; ++i) se += expf(z[i] - mx);           // exp(-inf) = 0 past the row
            se = wave_sum(se);
            const float lse = mx + logf(se);
            if (lane == 0) {
                lse_out[t] = lse;
                row_loss[t] = valid ? (lse - zt) : 0.f;
            }
            continue;
        }
        for (int c = lane; c < V; c += 64) {
            const float z = round_as<TL>(ld1(row + c) * inv_temp);
            st1(row + c, z);
            mx = fmaxf(mx, z);
            if (valid && c == (int)tgt) zt = z;
        }
        mx = wave_max(mx);
        zt = wave_sum(zt);
        float se = 0.f;
        for (int c = lane; c < V; c += 64) se += expf(ld1(row + c) - mx);
        se = wave_sum(se);
        const float lse = mx + logf(se);
        if (lane == 0) {
            lse_out[t] = lse;
            row_loss[t] = valid ? (lse - zt) : 0.f;
        }
    }
}

// deterministic single-workgroup reduction: out[0] = sum(row_loss), out[1] = #valid targets
__global__ void __launch_bounds__(1024)
ce_reduce_kernel(const float* __restrict__ row_loss, const int64_t* __restrict__ labels, int T, int S, int V,
                 int ignore_index, float* __restrict__ loss_sum, float* __restrict__ count) {
    __shared__ float sh_l[1024];
    __shared__ float sh_c[1024];
    float l = 0.f, c = 0.f;
    // eight independent loads in flight per thread (one workgroup: the loop is latency-bound, 0.30 ms at T = 517k
    // with one load at a time); the summation order stays fixed
    int t = threadIdx.x;
    for (; t + 7 * 1024 < T; t += 8 * 1024) {
        float lv[8];
        int64_t tg[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int tt = t + u * 1024;
            lv[u] = row_loss[tt];
            tg[u] = (tt % S) + 1 < S ? labels[tt + 1] : (int64_t)ignore_index;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            l += lv[u];
            if (tg[u] != ignore_index && tg[u] >= 0 && tg[u] < V) c += 1.f;
        }
    }
    for (; t < T; t += 1024) {
        l += row_loss[t];
        const int s = t % S;
        if (s + 1 < S) {
            const int64_t tgt = labels[t + 1];
            if (tgt != ignore_index && tgt >= 0 && tgt < V) c += 1.f;
        }
    }
    sh_l[threadIdx.x] = l;
    sh_c[threadIdx.x] = c;
    __syncthreads();
    for (int off = 512; off > 0; off >>= 1) {
        if (threadIdx.x < off) {
            sh_l[threadIdx.x] += sh_l[threadIdx.x + off];
            sh_c[threadIdx.x] += sh_c[threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        loss_sum[0] = sh_l[0];
        count[0] = sh_c[0];
    }
}

template <typename TL>
__global__ void __launch_bounds__(EW_THREADS)
ce_bwd_kernel(TL* __restrict__ logits, int ldl, const int64_t* __restrict__ labels, int T, int S, int V,
              int ignore_index, const float* __restrict__ lse, const float* __restrict__ count_dev,
              float denom_host, float dloss_over_temp, const float* __restrict__ dloss_dev, uint32_t* __restrict__ amax_out,
              int vec4) {
    __shared__ uint32_t amax_lds[4];
    uint32_t am = 0;
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * EW_THREADS + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * EW_THREADS) >> 6;
    const float denom = count_dev ? count_dev[0] : denom_host;
    const float gs = dloss_over_temp * (dloss_dev ? dloss_dev[0] : 1.f) / denom;
    for (int t = wave; t < T; t += nwaves) {
        TL* row = logits + (int64_t)t * ldl;
        const int s = t % S;
        const int64_t tgt = (s + 1 < S) ? labels[t + 1] : (int64_t)ignore_index;
        const bool valid = tgt != ignore_index && tgt >= 0 && tgt < V;
        const float l = lse[t];
        if (vec4 && V <= 64 * CE_EPL<TL> * CE_MAXQ<TL>) {       // 16 bytes per lane, the row's loads all in flight (see ce_fwd_kernel)
            constexpr int EPL = CE_EPL<TL>;
            const int c_last = ((V - 1) / EPL) * EPL;
            float xs[CE_MAXQ<TL>][EPL];
#pragma unroll
            for (int i = 0; i < CE_MAXQ<TL>; ++i) ce_load16(row + min(EPL * (lane + 64 * i), c_last), xs[i]);
#pragma unroll
            for (int i = 0; i < CE_MAXQ<TL>; ++i) {
                const int c = EPL * (lane + 64 * i);
                if (c >= V) continue;
                float g[EPL];
#pragma unroll
                for (int e = 0; e < EPL; ++e) {
                    float v = (valid && c + e < V) ? expf(xs[i][e] - l) : 0.f;
                    if (valid && c + e == (int)tgt) v -= 1.f;
                    g[e] = (valid && c + e < V) ? v * gs : 0.f;
                }
                if (c + EPL <= V) {
                    ce_store16(row + c, g);
                } else {
#pragma unroll
                    for (int e = 0; e < EPL; ++e)
                        if (c + e < V) st1(row + c + e, g[e]);
                }
#pragma unroll
                for (int e = 0; e < EPL; ++e) am = __float_as_uint(fmaxf(__uint_as_float(am), fabsf(g[e])));
            }
            continue;
        }
        for (int c = lane; c < V; c += 64) {
            float g = 0.f;
            if (valid) {
                g = expf(ld1(row + c) - l);
                if (c == (int)tgt) g -= 1.f;
                g *= gs;
            }
            st1(row + c, g);
            am = __float_as_uint(fmaxf(__uint_as_float(am), fabsf(g)));
        }
    }
    amax_block_commit(am, amax_out, amax_lds);
}

__global__ void __launch_bounds__(EW_THREADS)
fill_kernel(float* __restrict__ p, int64_t n, float value) {
    for (int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * EW_THREADS)
        p[i] = value;
}

}  // namespace gamer

namespace gamer {
static thread_local AmaxSink g_amax_sink = {{nullptr, nullptr, nullptr}};
AmaxSink take_amax_sink() {
    const AmaxSink s = g_amax_sink;
    g_amax_sink.out[0] = g_amax_sink.out[1] = g_amax_sink.out[2] = nullptr;
    return s;
}
}  // namespace gamer

using namespace gamer;

extern "C" int gamer_amax_sink(uint32_t* out0, uint32_t* out1) {
    g_amax_sink.out[0] = out0;
    g_amax_sink.out[1] = out1;
    g_amax_sink.out[2] = nullptr;
    return 0;
}
extern "C" int gamer_amax_sink3(uint32_t* out0, uint32_t* out1, uint32_t* out2) {
    g_amax_sink.out[0] = out0;
    g_amax_sink.out[1] = out1;
    g_amax_sink.out[2] = out2;
    return 0;
}

extern "C" int gamer_embedding_fwd(const int64_t* ids, const float* W, int V, int T, int H, float* x, void* stream) {
    GAMER_CHECK_ARG(ids && W && x, "gamer_embedding_fwd: null pointer");
    GAMER_CHECK_ARG(T > 0 && H > 0 && H % 4 == 0 && V > 0, "gamer_embedding_fwd: bad shape T=%d H=%d V=%d", T, H, V);
    GAMER_CHECK_ARG(aligned16(W) && aligned16(x), "gamer_embedding_fwd: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(embedding_fwd_kernel, dim3(grid_for_waves(T)), dim3(EW_THREADS), 0, ST(stream),
                       ids, (const float4*)W, V, T, H / 4, (float4*)x);
    GAMER_CHECK_LAUNCH("gamer_embedding_fwd");
    return 0;
}

extern "C" int gamer_embedding_bwd(const int64_t* ids, const float* dx, int V, int T, int H, int pad_id, float* dW,
                                   void* stream) {
    GAMER_CHECK_ARG(ids && dx && dW, "gamer_embedding_bwd: null pointer");
    GAMER_CHECK_ARG(T > 0 && H > 0 && V > 0, "gamer_embedding_bwd: bad shape T=%d H=%d V=%d", T, H, V);
    GAMER_CHECK_ARG(H <= 1024, "gamer_embedding_bwd: H=%d > 1024 unsupported", H);
    // 1024-token chunks at T = 517k (505 workgroups); at the 8-GPU per-rank shape (T = 64,640) that would be 64 workgroups
    // walking 256 dependent iterations each (0.44 ms): chunks of >= 128 tokens sized for ~512 workgroups instead
    int chunk = EMB_CHUNK;
    while (chunk > 128 && (T + chunk - 1) / chunk < 512) chunk >>= 1;
    hipLaunchKernelGGL(embedding_bwd_kernel, dim3((T + chunk - 1) / chunk), dim3(EW_THREADS),
                       (size_t)EMB_CACHE * H * sizeof(float), ST(stream), ids, dx, V, T, H, pad_id, dW, chunk);
    GAMER_CHECK_LAUNCH("gamer_embedding_bwd");
    return 0;
}

// bytes of the workspace gamer_embedding_bwd_ordered needs
extern "C" int64_t gamer_embedding_bwd_ordered_ws_bytes(int V, int T, int H) {
    if (V <= 0 || T <= 0 || H <= 0) return -1;
    const int64_t chunks = (T + EMB_SORT_CHUNK - 1) / EMB_SORT_CHUNK;
    const int64_t pieces = (int64_t)T / EMB_PIECE + V + 1;
    const int64_t ints = chunks * (V + 1) + 2 * (int64_t)(V + 1) + (V + 2) + T;
    return ((ints * 4 + 15) / 16) * 16 + pieces * H * 4;
}
extern "C" int gamer_embedding_bwd_ordered(const int64_t* ids, const float* dx, int V, int T, int H, int pad_id, float* dW,
                                           void* ws, int64_t ws_bytes, void* stream) {
    GAMER_CHECK_ARG(ids && dx && dW && ws, "gamer_embedding_bwd_ordered: null pointer");
    GAMER_CHECK_ARG(T > 0 && H > 0 && H % 4 == 0 && V > 0 && V <= EMB_MAX_V,
                    "gamer_embedding_bwd_ordered: bad shape T=%d H=%d V=%d (H %% 4 == 0, V <= %d)", T, H, V, EMB_MAX_V);
    GAMER_CHECK_ARG(aligned16(dx) && aligned16(dW) && aligned16(ws) && ws_bytes >= gamer_embedding_bwd_ordered_ws_bytes(V, T, H),
                    "gamer_embedding_bwd_ordered: dx / dW / ws must be 16-byte aligned and ws hold %lld bytes (got %lld)",
                    (long long)gamer_embedding_bwd_ordered_ws_bytes(V, T, H), (long long)ws_bytes);
    const int chunks = (T + EMB_SORT_CHUNK - 1) / EMB_SORT_CHUNK;
    const int pieces_max = T / EMB_PIECE + V + 1;
    int* ip = (int*)ws;
    EmbSortWs w;
    w.hist = ip; ip += (int64_t)chunks * (V + 1);
    w.row_start = ip; ip += V + 1;
    w.row_count = ip; ip += V + 1;
    w.piece_start = ip; ip += V + 2;
    w.perm = ip; ip += T;
    const int64_t ints = (int64_t)chunks * (V + 1) + 2 * (int64_t)(V + 1) + (V + 2) + T;
    w.partial = (float*)((char*)ws + ((ints * 4 + 15) / 16) * 16);
    hipStream_t st = ST(stream);
    const size_t lds = (size_t)(V + 1) * sizeof(int);
    hipLaunchKernelGGL(emb_hist_kernel, dim3(chunks), dim3(EW_THREADS), lds, st, ids, V, T, pad_id, w.hist);
    GAMER_CHECK_LAUNCH("gamer_embedding_bwd_ordered/hist");
    hipLaunchKernelGGL(emb_chunk_scan_kernel, dim3(V + 1), dim3(64), 0, st, V, chunks, w.hist, w.row_count);
    GAMER_CHECK_LAUNCH("gamer_embedding_bwd_ordered/chunk_scan");
    hipLaunchKernelGGL(emb_row_scan_kernel, dim3(1), dim3(1024), 0, st, V, w.row_count, w.row_start, w.piece_start);
    GAMER_CHECK_LAUNCH("gamer_embedding_bwd_ordered/row_scan");
    hipLaunchKernelGGL(emb_scatter_kernel, dim3(chunks), dim3(EW_THREADS), lds + EMB_SORT_CHUNK * sizeof(int), st, ids, V, T, pad_id,
                       w.hist, w.row_start, w.perm);
    GAMER_CHECK_LAUNCH("gamer_embedding_bwd_ordered/scatter");
    hipLaunchKernelGGL(emb_piece_sum_kernel, dim3(pieces_max), dim3(EW_THREADS), 0, st, (const float4*)dx, V, H / 4, w.row_start,
                       w.row_count, w.piece_start, w.perm, (float4*)w.partial);
    GAMER_CHECK_LAUNCH("gamer_embedding_bwd_ordered/pieces");
    hipLaunchKernelGGL(emb_row_sum_kernel, dim3(V), dim3(64), 0, st, H / 4, w.piece_start, (const float4*)w.partial, (float4*)dW);
    GAMER_CHECK_LAUNCH("gamer_embedding_bwd_ordered/rows");
    return 0;
}

template <typename TY>
static int rmsnorm_fwd_impl(const char* name, const float* x, const float* w, int T, int H, float eps,
                            const int32_t* dst_rows, TY* y, int ldy, void* stream) {
    GAMER_CHECK_ARG(x && w && y, "%s: null pointer", name);
    GAMER_CHECK_ARG(T > 0 && H > 0 && H % 4 == 0 && H <= 256 * RMS_MAXC_BIG && ldy >= H && ldy % 4 == 0,
                    "%s: bad shape T=%d H=%d ldy=%d (H%%4==0, H<=1024, ldy%%4==0)", name, T, H, ldy);
    GAMER_CHECK_ARG(aligned16(x) && aligned16(w) && aligned_vec4<TY>(y), "%s: pointers must be 16-byte aligned", name);
    const AmaxSink sink = take_amax_sink();
    if (H <= 256)
        hipLaunchKernelGGL((rmsnorm_fwd_kernel<TY, 1>), dim3(grid_for_waves(T)), dim3(EW_THREADS), 0, ST(stream),
                           (const float4*)x, (const float4*)w, T, H / 4, 1.f / (float)H, eps, dst_rows, y, ldy, sink.out[0]);
    else
        hipLaunchKernelGGL((rmsnorm_fwd_kernel<TY, RMS_MAXC_BIG>), dim3(grid_for_waves(T)), dim3(EW_THREADS), 0, ST(stream),
                           (const float4*)x, (const float4*)w, T, H / 4, 1.f / (float)H, eps, dst_rows, y, ldy, sink.out[0]);
    GAMER_CHECK_LAUNCH(name);
    return 0;
}
extern "C" int gamer_rmsnorm_fwd(const float* x, const float* w, int T, int H, float eps, const int32_t* dst_rows,
                                 float* y, int ldy, void* stream) {
    return rmsnorm_fwd_impl<float>("gamer_rmsnorm_fwd", x, w, T, H, eps, dst_rows, y, ldy, stream);
}
extern "C" int gamer_rmsnorm_fwd_bf16(const float* x, const float* w, int T, int H, float eps, const int32_t* dst_rows,
                                      gamer_bf16* y, int ldy, void* stream) {
    return rmsnorm_fwd_impl<bf16_t>("gamer_rmsnorm_fwd_bf16", x, w, T, H, eps, dst_rows, (bf16_t*)y, ldy, stream);
}

template <typename TG>
static int rmsnorm_bwd_impl(const char* name, const float* x, const float* w, const TG* dy, int lddy,
                            const int32_t* dy_rows, int T, int H, float eps, int accumulate_dx, float* dx,
                            float* dw_partial, int n_partial, TG* mask_out, const int32_t* mask_rows, float p_drop,
                            uint64_t seed, void* stream) {
    GAMER_CHECK_ARG(x && w && dy && dx && dw_partial, "%s: null pointer", name);
    GAMER_CHECK_ARG(T > 0 && H > 0 && H % 4 == 0 && H <= 256 * RMS_MAXC_BIG && lddy >= H && lddy % 4 == 0 && n_partial > 0,
                    "%s: bad shape T=%d H=%d lddy=%d n_partial=%d", name, T, H, lddy, n_partial);
    GAMER_CHECK_ARG(aligned16(x) && aligned16(w) && aligned_vec4<TG>(dy) && aligned16(dx) && aligned16(dw_partial) &&
                    aligned_vec4<TG>(mask_out), "%s: pointers must be 16-byte aligned", name);
    const AmaxSink sink = take_amax_sink();
    if (H <= 256)
        hipLaunchKernelGGL((rmsnorm_bwd_kernel<TG, 1>), dim3(n_partial), dim3(EW_THREADS), 0, ST(stream),
                           (const float4*)x, (const float4*)w, dy, lddy, dy_rows, T, H / 4, 1.f / (float)H, eps,
                           accumulate_dx, (float4*)dx, dw_partial, mask_out, mask_rows, p_drop, seed, sink.out[0]);
    else
        hipLaunchKernelGGL((rmsnorm_bwd_kernel<TG, RMS_MAXC_BIG>), dim3(n_partial), dim3(EW_THREADS), 0, ST(stream),
                           (const float4*)x, (const float4*)w, dy, lddy, dy_rows, T, H / 4, 1.f / (float)H, eps,
                           accumulate_dx, (float4*)dx, dw_partial, mask_out, mask_rows, p_drop, seed, sink.out[0]);
    GAMER_CHECK_LAUNCH(name);
    return 0;
}
extern "C" int gamer_rmsnorm_bwd(const float* x, const float* w, const float* dy, int lddy, const int32_t* dy_rows,
                                 int T, int H, float eps, int accumulate_dx, float* dx, float* dw_partial,
                                 int n_partial, float* mask_out, const int32_t* mask_rows, float p_drop,
                                 uint64_t seed, void* stream) {
    return rmsnorm_bwd_impl<float>("gamer_rmsnorm_bwd", x, w, dy, lddy, dy_rows, T, H, eps, accumulate_dx, dx, dw_partial,
                                   n_partial, mask_out, mask_rows, p_drop, seed, stream);
}
extern "C" int gamer_rmsnorm_bwd_bf16(const float* x, const float* w, const gamer_bf16* dy, int lddy,
                                      const int32_t* dy_rows, int T, int H, float eps, int accumulate_dx, float* dx,
                                      float* dw_partial, int n_partial, gamer_bf16* mask_out, const int32_t* mask_rows,
                                      float p_drop, uint64_t seed, void* stream) {
    return rmsnorm_bwd_impl<bf16_t>("gamer_rmsnorm_bwd_bf16", x, w, (const bf16_t*)dy, lddy, dy_rows, T, H, eps,
                                    accumulate_dx, dx, dw_partial, n_partial, (bf16_t*)mask_out, mask_rows, p_drop, seed,
                                    stream);
}

extern "C" int gamer_colsum_reduce(const float* partial, int rows, int cols, int accumulate, float* out, void* stream) {
    GAMER_CHECK_ARG(partial && out && rows > 0 && cols > 0, "gamer_colsum_reduce: bad arguments");
    hipLaunchKernelGGL(colsum_reduce_kernel, dim3((cols + 31) / 32), dim3(32 * COLSUM_RG), 0, ST(stream), partial, rows,
                       cols, accumulate, out);
    GAMER_CHECK_LAUNCH("gamer_colsum_reduce");
    return 0;
}

extern "C" int gamer_colsum_reduce_batched(const float* partial, int64_t stride, int rows, int cols, int n, float* const* outs,
                                           int accumulate, void* stream) {
    GAMER_CHECK_ARG(partial && outs && rows > 0 && cols > 0 && n > 0 && n <= 65535 && stride >= (int64_t)rows * cols,
                    "gamer_colsum_reduce_batched: bad arguments (rows=%d cols=%d n=%d stride=%lld)", rows, cols, n, (long long)stride);
    hipLaunchKernelGGL(colsum_reduce_batched_kernel, dim3((cols + 31) / 32, n), dim3(32 * COLSUM_RG), 0, ST(stream), partial, stride,
                       rows, cols, accumulate, outs);
    GAMER_CHECK_LAUNCH("gamer_colsum_reduce_batched");
    return 0;
}

template <typename TY>
static int rowtable_fwd_impl(const char* name, const float* table, const int32_t* idx, const int32_t* dst_rows, int T,
                             int E, TY* y, int ldy, int col0, void* stream) {
    GAMER_CHECK_ARG(table && idx && y, "%s: null pointer", name);
    GAMER_CHECK_ARG(T > 0 && E > 0 && E % 4 == 0 && ldy % 4 == 0 && col0 % 4 == 0 && col0 + E <= ldy,
                    "%s: bad shape T=%d E=%d ldy=%d col0=%d", name, T, E, ldy, col0);
    hipLaunchKernelGGL(rowtable_fwd_kernel<TY>, dim3(grid_for_threads((int64_t)T * E / 4)), dim3(EW_THREADS), 0,
                       ST(stream), (const float4*)table, idx, dst_rows, T, E / 4, y, ldy, col0, take_amax_sink().out[0]);
    GAMER_CHECK_LAUNCH(name);
    return 0;
}
extern "C" int gamer_rowtable_fwd(const float* table, const int32_t* idx, const int32_t* dst_rows, int T, int E,
                                  float* y, int ldy, int col0, void* stream) {
    return rowtable_fwd_impl<float>("gamer_rowtable_fwd", table, idx, dst_rows, T, E, y, ldy, col0, stream);
}
extern "C" int gamer_rowtable_fwd_bf16(const float* table, const int32_t* idx, const int32_t* dst_rows, int T, int E,
                                       gamer_bf16* y, int ldy, int col0, void* stream) {
    return rowtable_fwd_impl<bf16_t>("gamer_rowtable_fwd_bf16", table, idx, dst_rows, T, E, (bf16_t*)y, ldy, col0, stream);
}

template <typename TG>
static int rowtable_bwd_impl(const char* name, const TG* dy, int lddy, int col0, const int32_t* idx,
                             const int32_t* dy_rows, int T, int E, int n_rows_table, float* dtable, float* partial,
                             int64_t partial_numel, void* stream) {
    GAMER_CHECK_ARG(dy && idx && dtable, "%s: null pointer", name);
    GAMER_CHECK_ARG(T > 0 && E > 0 && E % 4 == 0 && E / 4 <= EW_THREADS && lddy % 4 == 0 && col0 % 4 == 0 &&
                    n_rows_table > 0 && n_rows_table <= TBL_MAXROWS,
                    "%s: bad shape T=%d E=%d lddy=%d col0=%d rows=%d (rows<=8)", name, T, E, lddy, col0, n_rows_table);
    const int rows_per_block = EW_THREADS / (E / 4);
    int blocks = (T + rows_per_block - 1) / rows_per_block;
    if (blocks > 1024) blocks = 1024;
    if (partial) {
        const int64_t per_block = (int64_t)n_rows_table * E;
        if (blocks * per_block > partial_numel) blocks = (int)(partial_numel / per_block);
        GAMER_CHECK_ARG(blocks >= 1, "%s: partial holds %lld floats, one workgroup's table needs %lld", name, (long long)partial_numel,
                        (long long)per_block);
        const size_t lds = (size_t)rows_per_block * per_block * sizeof(float);
        GAMER_CHECK_ARG(lds <= 64 * 1024, "%s: the ordered form needs %zu bytes of LDS (E=%d, rows=%d)", name, lds, E, n_rows_table);
        hipLaunchKernelGGL((rowtable_bwd_kernel<TG, true>), dim3(blocks), dim3(EW_THREADS), lds, ST(stream), dy, lddy, col0, idx,
                           dy_rows, T, E / 4, n_rows_table, dtable, partial);
        GAMER_CHECK_LAUNCH(name);
        hipLaunchKernelGGL(colsum_reduce_kernel, dim3(((int)per_block + 31) / 32), dim3(32 * COLSUM_RG), 0, ST(stream), partial, blocks,
                           (int)per_block, 1, dtable);
        GAMER_CHECK_LAUNCH(name);
        return 0;
    }
    hipLaunchKernelGGL((rowtable_bwd_kernel<TG, false>), dim3(blocks), dim3(EW_THREADS), (size_t)n_rows_table * E * sizeof(float),
                       ST(stream), dy, lddy, col0, idx, dy_rows, T, E / 4, n_rows_table, dtable, (float*)nullptr);
    GAMER_CHECK_LAUNCH(name);
    return 0;
}
extern "C" int gamer_rowtable_bwd(const float* dy, int lddy, int col0, const int32_t* idx, const int32_t* dy_rows,
                                  int T, int E, int n_rows_table, float* dtable, float* partial, int64_t partial_numel,
                                  void* stream) {
    return rowtable_bwd_impl<float>("gamer_rowtable_bwd", dy, lddy, col0, idx, dy_rows, T, E, n_rows_table, dtable, partial,
                                    partial_numel, stream);
}
extern "C" int gamer_rowtable_bwd_bf16(const gamer_bf16* dy, int lddy, int col0, const int32_t* idx,
                                       const int32_t* dy_rows, int T, int E, int n_rows_table, float* dtable,
                                       float* partial, int64_t partial_numel, void* stream) {
    return rowtable_bwd_impl<bf16_t>("gamer_rowtable_bwd_bf16", (const bf16_t*)dy, lddy, col0, idx, dy_rows, T, E,
                                     n_rows_table, dtable, partial, partial_numel, stream);
}

extern "C" int gamer_residual_dropout_fwd(const float* x_in, const float* delta, const int32_t* src_rows, int T, int H,
                                          float p_drop, uint64_t seed, float* x_out, void* stream) {
    GAMER_CHECK_ARG(x_in && x_out && delta && T > 0 && H > 0 && H % 4 == 0 && p_drop >= 0.f && p_drop < 1.f,
                    "gamer_residual_dropout_fwd: bad arguments T=%d H=%d p=%f", T, H, p_drop);
    hipLaunchKernelGGL(residual_dropout_fwd_kernel, dim3(grid_for_threads((int64_t)T * H / 4)), dim3(EW_THREADS), 0,
                       ST(stream), (const float4*)x_in, (const float4*)delta, src_rows, T, H / 4, p_drop, seed,
                       (float4*)x_out);
    GAMER_CHECK_LAUNCH("gamer_residual_dropout_fwd");
    return 0;
}

extern "C" int gamer_residual_dropout_bwd(const float* dx, const int32_t* src_rows, int T, int H, float p_drop,
                                          uint64_t seed, float* ddelta, void* stream) {
    GAMER_CHECK_ARG(dx && ddelta && T > 0 && H > 0 && H % 4 == 0 && p_drop >= 0.f && p_drop < 1.f,
                    "gamer_residual_dropout_bwd: bad arguments T=%d H=%d p=%f", T, H, p_drop);
    hipLaunchKernelGGL(residual_dropout_bwd_kernel, dim3(grid_for_threads((int64_t)T * H / 4)), dim3(EW_THREADS), 0,
                       ST(stream), (const float4*)dx, src_rows, T, H / 4, p_drop, seed, (float4*)ddelta);
    GAMER_CHECK_LAUNCH("gamer_residual_dropout_bwd");
    return 0;
}

extern "C" int gamer_silu_gate_fwd(const float* a, const float* gate, int64_t n, float* out, const float* resid,
                                   float p_drop, uint64_t seed, void* stream) {
    GAMER_CHECK_ARG(a && gate && out && n > 0 && n % 4 == 0 && p_drop >= 0.f && p_drop < 1.f, "gamer_silu_gate_fwd: bad arguments");
    hipLaunchKernelGGL((silu_gate_fwd_kernel<float, float>), dim3(grid_for_threads(n / 4)), dim3(EW_THREADS), 0, ST(stream),
                       a, gate, n / 4, out, (const float4*)resid, p_drop, seed);
    GAMER_CHECK_LAUNCH("gamer_silu_gate_fwd");
    return 0;
}
extern "C" int gamer_silu_gate_fwd_bf16(const gamer_bf16* a, const gamer_bf16* gate, int64_t n, float* out,
                                        const float* resid, float p_drop, uint64_t seed, void* stream) {
    GAMER_CHECK_ARG(a && gate && out && resid && n > 0 && n % 4 == 0 && p_drop >= 0.f && p_drop < 1.f,
                    "gamer_silu_gate_fwd_bf16: bad arguments (resid is required: out is the fp32 residual stream)");
    hipLaunchKernelGGL((silu_gate_fwd_kernel<bf16_t, float>), dim3(grid_for_threads(n / 4)), dim3(EW_THREADS), 0, ST(stream),
                       (const bf16_t*)a, (const bf16_t*)gate, n / 4, out, (const float4*)resid, p_drop, seed);
    GAMER_CHECK_LAUNCH("gamer_silu_gate_fwd_bf16");
    return 0;
}

template <typename TA>
static int silu_gate_bwd_impl(const char* name, const TA* a, const TA* gate, const float* dout, int64_t n, TA* da,
                              TA* dgate, float p_drop, uint64_t seed, void* stream) {
    GAMER_CHECK_ARG(a && gate && dout && da && dgate && n > 0 && n % 4 == 0 && p_drop >= 0.f && p_drop < 1.f,
                    "%s: bad arguments", name);
    const AmaxSink sink = take_amax_sink();
    hipLaunchKernelGGL(silu_gate_bwd_kernel<TA>, dim3(grid_for_threads(n / 4)), dim3(EW_THREADS), 0, ST(stream), a, gate,
                       (const float4*)dout, n / 4, da, dgate, p_drop, seed, sink.out[0], sink.out[1]);
    GAMER_CHECK_LAUNCH(name);
    return 0;
}
extern "C" int gamer_silu_gate_bwd(const float* a, const float* gate, const float* dout, int64_t n, float* da,
                                   float* dgate, float p_drop, uint64_t seed, void* stream) {
    return silu_gate_bwd_impl<float>("gamer_silu_gate_bwd", a, gate, dout, n, da, dgate, p_drop, seed, stream);
}
extern "C" int gamer_silu_gate_bwd_bf16(const gamer_bf16* a, const gamer_bf16* gate, const float* dout, int64_t n,
                                        gamer_bf16* da, gamer_bf16* dgate, float p_drop, uint64_t seed, void* stream) {
    return silu_gate_bwd_impl<bf16_t>("gamer_silu_gate_bwd_bf16", (const bf16_t*)a, (const bf16_t*)gate, dout, n,
                                      (bf16_t*)da, (bf16_t*)dgate, p_drop, seed, stream);
}

template <typename TL>
static int ce_fwd_impl(const char* name, TL* logits, int ldl, const int64_t* labels, int B, int S, int V,
                       float temperature, int ignore_index, float* lse_out, float* row_loss, float* loss_sum,
                       float* count, void* stream) {
    GAMER_CHECK_ARG(logits && labels && lse_out && row_loss && loss_sum && count, "%s: null pointer", name);
    GAMER_CHECK_ARG(B > 0 && S > 0 && V > 0 && ldl >= V && temperature > 0.f, "%s: bad shape B=%d S=%d V=%d ldl=%d", name, B, S, V, ldl);
    const int T = B * S;
    const int vec4 = (ldl % (16 / (int)sizeof(TL)) == 0 && aligned16(logits)) ? 1 : 0;
    hipLaunchKernelGGL(ce_fwd_kernel<TL>, dim3(grid_for_waves(T)), dim3(EW_THREADS), 0, ST(stream), logits, ldl, labels, T,
                       S, V, 1.f / temperature, ignore_index, lse_out, row_loss, vec4);
    GAMER_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(ce_reduce_kernel, dim3(1), dim3(1024), 0, ST(stream), row_loss, labels, T, S, V, ignore_index,
                       loss_sum, count);
    GAMER_CHECK_LAUNCH(name);
    return 0;
}
extern "C" int gamer_ce_fwd(float* logits, int ldl, const int64_t* labels, int B, int S, int V, float temperature,
                            int ignore_index, float* lse_out, float* row_loss, float* loss_sum, float* count,
                            void* stream) {
    return ce_fwd_impl<float>("gamer_ce_fwd", logits, ldl, labels, B, S, V, temperature, ignore_index, lse_out, row_loss,
                              loss_sum, count, stream);
}
extern "C" int gamer_ce_fwd_bf16(gamer_bf16* logits, int ldl, const int64_t* labels, int B, int S, int V,
                                 float temperature, int ignore_index, float* lse_out, float* row_loss, float* loss_sum,
                                 float* count, void* stream) {
    return ce_fwd_impl<bf16_t>("gamer_ce_fwd_bf16", (bf16_t*)logits, ldl, labels, B, S, V, temperature, ignore_index,
                               lse_out, row_loss, loss_sum, count, stream);
}

template <typename TL>
static int ce_bwd_impl(const char* name, TL* logits, int ldl, const int64_t* labels, int B, int S, int V,
                       float temperature, int ignore_index, const float* lse, const float* count_dev, float denom_host,
                       float dloss, const float* dloss_dev, void* stream) {
    GAMER_CHECK_ARG(logits && labels && lse, "%s: null pointer", name);
    GAMER_CHECK_ARG(B > 0 && S > 0 && V > 0 && ldl >= V && temperature > 0.f, "%s: bad shape", name);
    GAMER_CHECK_ARG(count_dev || denom_host > 0.f, "%s: need count_dev or a positive denom_host", name);
    const int T = B * S;
    hipLaunchKernelGGL(ce_bwd_kernel<TL>, dim3(grid_for_waves(T)), dim3(EW_THREADS), 0, ST(stream), logits, ldl, labels, T,
                       S, V, ignore_index, lse, count_dev, denom_host, dloss / temperature, dloss_dev, take_amax_sink().out[0],
                       (ldl % (16 / (int)sizeof(TL)) == 0 && aligned16(logits)) ? 1 : 0);
    GAMER_CHECK_LAUNCH(name);
    return 0;
}
extern "C" int gamer_ce_bwd(float* logits, int ldl, const int64_t* labels, int B, int S, int V, float temperature,
                            int ignore_index, const float* lse, const float* count_dev, float denom_host, float dloss,
                            const float* dloss_dev, void* stream) {
    return ce_bwd_impl<float>("gamer_ce_bwd", logits, ldl, labels, B, S, V, temperature, ignore_index, lse, count_dev,
                              denom_host, dloss, dloss_dev, stream);
}
extern "C" int gamer_ce_bwd_bf16(gamer_bf16* logits, int ldl, const int64_t* labels, int B, int S, int V,
                                 float temperature, int ignore_index, const float* lse, const float* count_dev,
                                 float denom_host, float dloss, const float* dloss_dev, void* stream) {
    return ce_bwd_impl<bf16_t>("gamer_ce_bwd_bf16", (bf16_t*)logits, ldl, labels, B, S, V, temperature, ignore_index, lse,
                               count_dev, denom_host, dloss, dloss_dev, stream);
}

extern "C" int gamer_fill_f32(float* p, int64_t n, float value, void* stream) {
    GAMER_CHECK_ARG(p && n >= 0, "gamer_fill_f32: bad arguments");
    if (n == 0) return 0;
    hipLaunchKernelGGL(fill_kernel, dim3(grid_for_threads(n)), dim3(EW_THREADS), 0, ST(stream), p, n, value);
    GAMER_CHECK_LAUNCH("gamer_fill_f32");
    return 0;
}
