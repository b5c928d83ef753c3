// Cached decode attention of the bf16 engine (gfx950): ONE new token per beam against a bf16 K/V cache whose prompt part is stored
// once per sample and whose generated part is stored per beam - the bf16 twin of gamer_attn_decode (csrc/decode.hip), with the
// semantics and arithmetic of the bf16 train / scoring attention (csrc/attention_bf16.hip:5-11):
//   * a query row with no allowed key gives an all-zero output (l = 0): there is no "uniform average" row in bf16, hence no
//     `uniform` argument, and a cross block's generated keys - masked for every row - are never read (gen_ok = 0);
//   * bf16 q / k / v, fp32 scores and softmax statistics, un-normalised probabilities rounded to bf16 for the P V product, fp32
//     accumulation, bf16 output.
// Shape of the kernel (the one decode.hip proved): one workgroup = (sample, kv head); its nb * G <= 64 query rows are two 32-column
// tiles; the prompt keys are split over the four waves in 32-key tiles, each wave streaming its own tiles through a private LDS
// region (no workgroup barrier in the loop): S^T = K Q^T on v_mfma_f32_32x32x16_bf16 with the query on the lane, the score registers
// rounded pairwise to bf16 ARE the B operand of O^T += V^T P^T, V^T fragments through ds_read_b64_tr_b16 from the swizzled row-major
// image.  The four partial (reference, sum, O) states are merged through LDS, flash-decoding style; the <= tmax generated positions
// of each beam are added in the merge on the vector unit (products of two bf16 are exact in fp32).  No atomics: the same bits on
// every call.
// THE SOFTMAX REFERENCE IS THE SCORING FORWARD'S.  Rounding an un-normalised probability to bf16 depends on what it is relative to,
// and a cached step is held to the scoring forward of the same tokens (tests/test_decode_bf16_gpu.py), so a key's probability is
// taken relative to what attn_fwd_b_tile (csrc/attention_bf16.hip) would use for it: the maximum of the first 32-key sub-tile of the
// sequence that has an allowed key, replaced when a later sub-tile's maximum exceeds it by more than 2^16.  That rule is sequential
// in the keys, the waves are not: pass 1 computes S^T = K Q^T alone and leaves every sub-tile's maximum per query row in LDS (the
// generated keys join the sub-tile of their position L0 + g), 64 threads run the rule over the sub-tiles, pass 2 computes S^T again
// and the probabilities relative to its sub-tile's reference.  With equal probabilities what is left between the two kernels is the
// order of fp32 sums.  Cost: K is read twice (the second time from L2) and S^T computed twice.
// Traffic per call: the prompt cache from HBM once, B * nkv * L0 * 64 * 2 (K, V) * 2 bytes, half of the fp32 kernel's.  LDS: the
// tile / merge region + 256 bytes per sub-tile, so L0 + t <= 11,904 keys (checked on the host).
#include "attention_split_common.h"      // SlOffsets / read_row8 / read_tr8: the swizzled [32][64] 16-bit image and its two read patterns

namespace gamer {

constexpr int DB_MAXQ = 16;                                   // query rows per wave in the merge (4 waves): nb * G <= 64
constexpr int DB_WAVE_BYTES = 2 * SIMG * (int)sizeof(bf16_t) + 32 * (int)sizeof(int32_t);        // K tile | V tile | key_ok tile
constexpr int DB_OLD = 65;                                    // row stride of the merged-state image [64 queries][64 d]
constexpr int DB_MERGE_BYTES = 4 * (64 * DB_OLD + 128) * (int)sizeof(float);
constexpr int DB_LDS_BYTES = DB_MERGE_BYTES > 4 * DB_WAVE_BYTES ? DB_MERGE_BYTES : 4 * DB_WAVE_BYTES;

// two fp32 -> one register of two bf16, round to nearest even (attention_bf16.hip: cvt_pk_bf16)
__device__ __forceinline__ uint32_t db_cvt_pk(float lo, float hi) {
    uint32_t r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}
typedef uint32_t db_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ bf16x8 db_pack8(const f32x16& a, int s2) {
    db_u32x4 u;
#pragma unroll
    for (int j = 0; j < 4; ++j) u[j] = db_cvt_pk(a[8 * s2 + 2 * j], a[8 * s2 + 2 * j + 1]);
    return __builtin_bit_cast(bf16x8, u);
}
// sum over the 64 lanes without the LDS crossbar (decode.hip: wave_sum_x; the pairs of the xor 32, 16, 8, 4, 2, 1 butterfly)
__device__ __forceinline__ float db_wave_sum(float v) {
#define GAMER_DB_DPP(ctrl) __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), ctrl, 0xf, 0xf, false))
    const auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    const auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(b[0]) + __uint_as_float(b[1]);
    v += GAMER_DB_DPP(0x128);            // row_ror:8
    v += GAMER_DB_DPP(0x124);            // row_ror:4
    v += GAMER_DB_DPP(0x4E);             // quad_perm [2,3,0,1]
    v += GAMER_DB_DPP(0xB1);             // quad_perm [1,0,3,2]
#undef GAMER_DB_DPP
    return v;
}

template <int G>
__global__ void __launch_bounds__(256, 2)
attn_decode_b_kernel(const bf16_t* __restrict__ q, int ldq, const bf16_t* __restrict__ kp, int ldkp,
                     const bf16_t* __restrict__ vp, int ldvp, const int32_t* __restrict__ key_ok,
                     const bf16_t* __restrict__ kg, const bf16_t* __restrict__ vg, int ldg, int tmax, int t, int gen_ok,
                     int nb, int L0, int nq, int nkv, float scale, int nsub, bf16_t* __restrict__ o) {
    extern __shared__ __attribute__((aligned(16))) unsigned char db_raw[];
    float* lds_f = reinterpret_cast<float*>(db_raw);
    float* ref_tab = reinterpret_cast<float*>(db_raw + DB_LDS_BYTES);      // [nsub][64]: sub-tile maxima, then softmax references
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int b = blockIdx.x / nkv, kvh = blockIdx.x % nkv;
    const int Qn = nb * G;
    const float c2 = scale * 1.4426950408889634f;               // scores live in the log2 domain
    float* mrg_m = lds_f;                                       // [4][64] softmax reference of every wave's partial state
    float* mrg_l = lds_f + 256;                                 // [4][64] running sum
    float* mrg_o = lds_f + 512;                                 // [4][64][DB_OLD] partial O
    const int n_tiles = (L0 + 31) >> 5;
    const int n_qt = Qn > 32 ? 2 : 1;
    const bool gen = gen_ok != 0 && t > 0;

    bf16_t* Kw = reinterpret_cast<bf16_t*>(db_raw + (size_t)w * DB_WAVE_BYTES);
    bf16_t* Vw = Kw + SIMG;
    int32_t* okw = reinterpret_cast<int32_t*>(Vw + SIMG);
    const SlOffsets lo(lane);
    // query fragments of the two 32-column tiles: B operands, lane = query column, 8 d-values per k-step (the columns past Qn
    // repeat row 0 and are never stored)
    bf16x8 qf[2][4];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int qi = qt * 32 + r;
        const int qc = qi < Qn ? qi : 0;
        const bf16_t* qrow = q + (int64_t)(b * nb + qc / G) * ldq + (kvh * G + qc % G) * 64 + 8 * h;
#pragma unroll
        for (int s = 0; s < 4; ++s) qf[qt][s] = *reinterpret_cast<const bf16x8*>(qrow + 16 * s);
    }
    // this wave's K (and V) tile of 32 keys: 256 chunks of 16 bytes per tensor, 4 per lane; every load is unconditional (clamped
    // row) and requested before the first store; rows past the prompt are stored as zeros.  Returns the tile's key_ok quads.
    auto stage = [&](int j0, auto with_v_t, int (&okv)[16]) __attribute__((always_inline)) {
        constexpr bool with_v = decltype(with_v_t)::value;
        uint4 kr[4], vr[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = lane + 64 * i, row = f >> 3, c8 = (f & 7) << 3;
            const int j = min(j0 + row, L0 - 1);
            kr[i] = *reinterpret_cast<const uint4*>(kp + ((int64_t)b * L0 + j) * ldkp + kvh * 64 + c8);
            if constexpr (with_v) vr[i] = *reinterpret_cast<const uint4*>(vp + ((int64_t)b * L0 + j) * ldvp + kvh * 64 + c8);
        }
        const int okv_g = key_ok[(int64_t)b * L0 + min(j0 + r, L0 - 1)];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = lane + 64 * i, row = f >> 3, c8 = (f & 7) << 3;
            const bool in = j0 + row < L0;
            const uint4 z = make_uint4(0u, 0u, 0u, 0u);
            *reinterpret_cast<uint4*>(Kw + sl_off(row, c8)) = in ? kr[i] : z;
            if constexpr (with_v) *reinterpret_cast<uint4*>(Vw + sl_off(row, c8)) = in ? vr[i] : z;
        }
        if (lane < 32) okw[lane] = (j0 + lane < L0) ? okv_g : 0;
        __builtin_amdgcn_s_waitcnt(0xc07f);               // lgkmcnt(0): the wave's own LDS writes landed
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int4 t4 = *reinterpret_cast<const int4*>(okw + 8 * g4 + 4 * h);
            okv[4 * g4] = t4.x; okv[4 * g4 + 1] = t4.y; okv[4 * g4 + 2] = t4.z; okv[4 * g4 + 3] = t4.w;
        }
    };
    // raw scores of the staged tile for query tile qt, masked keys at -inf: register reg of lane (r, h) = key (reg&3) + 8*(reg>>2) + 4*h
#define GAMER_DB_SCORES(st, kf, qt, okv)                                                                                   \
    f32x16 st;                                                                                                             \
    _Pragma("unroll") for (int i_ = 0; i_ < 16; ++i_) st[i_] = 0.f;                                                        \
    _Pragma("unroll") for (int s_ = 0; s_ < 4; ++s_) st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[s_], qf[qt][s_], st, 0, 0, 0); \
    _Pragma("unroll") for (int reg_ = 0; reg_ < 16; ++reg_) st[reg_] = okv[reg_] != 0 ? st[reg_] : -INFINITY;

    // ---- pass 1: the maximum of every 32-key sub-tile, per query row (log2 domain) ----------------------------------------
    for (int i = n_tiles * 64 + tid; i < nsub * 64; i += 256) ref_tab[i] = -INFINITY;      // sub-tiles of generated keys alone
    for (int jt = w; jt < n_tiles; jt += 4) {
        int okv[16];
        stage(jt * 32, std::false_type{}, okv);
        bf16x8 kf[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) kf[s] = read_row8(Kw, lo, 0, s);
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            if (qt >= n_qt) continue;                     // (workgroup-uniform)
            GAMER_DB_SCORES(st, kf, qt, okv)
            float mloc = st[0];
#pragma unroll
            for (int reg = 1; reg < 16; ++reg) mloc = fmaxf(mloc, st[reg]);
            mloc = xor32_max(mloc) * c2;
            if (h == 0) ref_tab[jt * 64 + qt * 32 + r] = mloc;
        }
        __builtin_amdgcn_wave_barrier();                  // the tile is consumed before the next one overwrites it
    }
    __syncthreads();
    if (gen) {
        // the generated keys (own ancestors + the new token) sit at positions L0 + g: they join the maximum of their sub-tile
#pragma unroll 1
        for (int i = 0; i < DB_MAXQ; ++i) {
            const int qi = w + 4 * i;
            if (qi >= Qn) break;
            const int n = b * nb + qi / G, head = kvh * G + qi % G;
            const float qd = (float)q[(int64_t)n * ldq + head * 64 + lane];
            for (int g = 0; g < t; ++g) {
                const float s = db_wave_sum(qd * (float)kg[((int64_t)n * tmax + g) * ldg + kvh * 64 + lane]) * c2;
                const int idx = ((L0 + g) >> 5) * 64 + qi;
                if (lane == 0) ref_tab[idx] = fmaxf(ref_tab[idx], s);
            }
        }
        __syncthreads();
    }
    // the softmax reference in effect at every sub-tile, by attn_fwd_b_tile's rule (csrc/attention_bf16.hip): the maximum of the
    // first sub-tile with an allowed key, replaced when a later sub-tile's maximum exceeds it by more than 2^16 (0 before any key)
    if (tid < Qn) {
        float m_ref = 0.f;
        bool seen = false;
        for (int k = 0; k < nsub; ++k) {
            const float mk = ref_tab[k * 64 + tid];
            const bool need = seen ? (mk > m_ref + 16.f) : (mk > -INFINITY);
            if (need) { m_ref = mk; seen = true; }
            ref_tab[k * 64 + tid] = m_ref;
        }
    }
    __syncthreads();

    // ---- pass 2: probabilities relative to the sub-tile's reference, O^T += V^T P^T ------------------------------------------
    {
        float m_cur[2] = {-INFINITY, -INFINITY}, l_run[2] = {0.f, 0.f};
        f32x16 oacc[2][2];
#pragma unroll
        for (int i = 0; i < 16; ++i) { oacc[0][0][i] = 0.f; oacc[0][1][i] = 0.f; oacc[1][0][i] = 0.f; oacc[1][1][i] = 0.f; }
        for (int jt = w; jt < n_tiles; jt += 4) {
            int okv[16];
            stage(jt * 32, std::true_type{}, okv);
            // the tile's K row fragments (A operands: lane = key) serve both query tiles
            bf16x8 kf[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) kf[s] = read_row8(Kw, lo, 0, s);
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
                if (qt >= n_qt) continue;                     // (workgroup-uniform)
                GAMER_DB_SCORES(st, kf, qt, okv)
                const float ref = ref_tab[jt * 64 + qt * 32 + r];
                const float alpha = __builtin_amdgcn_exp2f(m_cur[qt] - ref);      // first tile: 0 (nothing accumulated); same reference: 1
                float rowsum = 0.f;
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    st[reg] = __builtin_amdgcn_exp2f(__builtin_fmaf(st[reg], c2, -ref));      // masked: exp2(-inf) = 0
                    rowsum += st[reg];
                }
                rowsum = xor32_sum(rowsum);
                l_run[qt] = l_run[qt] * alpha + rowsum;
                m_cur[qt] = ref;
#pragma unroll
                for (int i = 0; i < 16; ++i) { oacc[qt][0][i] *= alpha; oacc[qt][1][i] *= alpha; }
                // O^T[d][query] += sum_key V[key][d] * bf16(P[query][key])
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    const bf16x8 pf = db_pack8(st, s2);
#pragma unroll
                    for (int db = 0; db < 2; ++db)
                        oacc[qt][db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(read_tr8(Vw, lo, 16 * s2, db), pf, oacc[qt][db], 0, 0, 0);
                }
            }
            __builtin_amdgcn_wave_barrier();                  // the tile is consumed before the next one overwrites it
        }
        __syncthreads();                                      // every wave is done with its tile region
        // publish this wave's state: O[query qt*32 + r][d = 32*dh + (reg&3) + 8*(reg>>2) + 4*h]
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            if (h == 0) { mrg_m[w * 64 + qt * 32 + r] = m_cur[qt]; mrg_l[w * 64 + qt * 32 + r] = l_run[qt]; }
#pragma unroll
            for (int dh = 0; dh < 2; ++dh)
#pragma unroll
                for (int reg = 0; reg < 16; ++reg)
                    mrg_o[(w * 64 + qt * 32 + r) * DB_OLD + 32 * dh + (reg & 3) + 8 * (reg >> 2) + 4 * h] = oacc[qt][dh][reg];
        }
        __syncthreads();
    }
    // merge the four key ranges at the row's last reference, add the generated positions of each beam, normalise and store.
    // Wave w takes query rows w, w + 4, ...; lane = d.
#pragma unroll 1
    for (int i = 0; i < DB_MAXQ; ++i) {
        const int qi = w + 4 * i;
        if (qi >= Qn) break;
        const int n = b * nb + qi / G, head = kvh * G + qi % G;
        const float R = ref_tab[(nsub - 1) * 64 + qi];          // (finite: 0 when the row has no allowed key)
        float li = 0.f, a = 0.f;
#pragma unroll
        for (int ww = 0; ww < 4; ++ww) {
            const float sc = __builtin_amdgcn_exp2f(mrg_m[ww * 64 + qi] - R);             // a wave without a tile: -inf -> 0
            li += mrg_l[ww * 64 + qi] * sc;
            a += mrg_o[(ww * 64 + qi) * DB_OLD + lane] * sc;
        }
        if (gen) {
            // the generated positions' key / value rows of this beam, four at a time, all requested before the first dot product
            const float qd = (float)q[(int64_t)n * ldq + head * 64 + lane];
            for (int g0 = 0; g0 < t; g0 += 4) {
                float kv4[4], vv4[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int64_t row = ((int64_t)n * tmax + min(g0 + u, t - 1)) * ldg + kvh * 64 + lane;
                    kv4[u] = (float)kg[row];
                    vv4[u] = (float)vg[row];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (g0 + u < t) {
                        const float rg = ref_tab[((L0 + g0 + u) >> 5) * 64 + qi];
                        const float pe = __builtin_amdgcn_exp2f(__builtin_fmaf(db_wave_sum(qd * kv4[u]), c2, -rg));
                        const float sg = __builtin_amdgcn_exp2f(rg - R);
                        li += pe * sg;
                        a += round_as<bf16_t>(pe) * vv4[u] * sg;
                    }
                }
            }
        }
        const float res = li > 0.f ? a * (1.f / li) : 0.f;      // no allowed key: exact zeros
        o[(int64_t)n * nq * 64 + head * 64 + lane] = (bf16_t)res;
    }
}

#undef GAMER_DB_SCORES
// the new token's rotated keys and (biased) values join the generated part of the cache: kg / vg [N][tmax][C] <- k / v rows, position g
// (16-byte chunks of eight bf16)
__global__ void __launch_bounds__(256)
kv_append_b_kernel(const uint4* __restrict__ k, int ldk8, const uint4* __restrict__ v, int ldv8, uint4* __restrict__ kg,
                   uint4* __restrict__ vg, int ldg8, int tmax, int g, int N, int C8) {
    const int64_t total = (int64_t)N * C8;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int n = (int)(i / C8), c = (int)(i % C8);
        const int64_t dst = ((int64_t)n * tmax + g) * ldg8 + c;
        kg[dst] = k[(int64_t)n * ldk8 + c];
        vg[dst] = v[(int64_t)n * ldv8 + c];
    }
}

}  // namespace gamer

using namespace gamer;

extern "C" int gamer_kv_append_bf16(const gamer_bf16* k, int ldk, const gamer_bf16* v, int ldv, gamer_bf16* kg, gamer_bf16* vg, int ldg,
                                    int tmax, int g, int N, int C, void* stream) {
    GAMER_CHECK_ARG(k && v && kg && vg, "gamer_kv_append_bf16: null pointer");
    GAMER_CHECK_ARG(N > 0 && C > 0 && C % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldg % 8 == 0 && ldk >= C && ldv >= C && ldg >= C &&
                    tmax > 0 && g >= 0 && g < tmax,
                    "gamer_kv_append_bf16: bad shape N=%d C=%d ldk=%d ldv=%d ldg=%d tmax=%d g=%d (multiples of 8)", N, C, ldk, ldv, ldg, tmax, g);
    GAMER_CHECK_ARG(aligned16(k) && aligned16(v) && aligned16(kg) && aligned16(vg), "gamer_kv_append_bf16: pointers must be 16-byte aligned");
    const int64_t total = (int64_t)N * (C / 8);
    const int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    return launch<kv_append_b_kernel>("gamer_kv_append_bf16", dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                                      reinterpret_cast<const uint4*>(k), ldk / 8, reinterpret_cast<const uint4*>(v), ldv / 8,
                                      reinterpret_cast<uint4*>(kg), reinterpret_cast<uint4*>(vg), ldg / 8, tmax, g, N, C / 8);
}

extern "C" int gamer_attn_decode_bf16(const gamer_bf16* q, int ldq, const gamer_bf16* kp, int ldkp, const gamer_bf16* vp, int ldvp,
                                      const int32_t* key_ok, const gamer_bf16* kg, const gamer_bf16* vg, int ldg, int tmax, int t,
                                      int gen_ok, int B, int nb, int L0, int nq, int nkv, float scale, gamer_bf16* o, void* stream) {
    // every check comes before the launch: a bad call leaves o untouched
    GAMER_CHECK_ARG(q && kp && vp && key_ok && kg && vg && o, "gamer_attn_decode_bf16: null pointer");
    GAMER_CHECK_ARG(B > 0 && nb > 0 && L0 > 0 && nq > 0 && nkv > 0 && nq % nkv == 0 && tmax > 0 && t >= 0 && t <= tmax,
                    "gamer_attn_decode_bf16: bad shape B=%d nb=%d L0=%d nq=%d nkv=%d t=%d tmax=%d", B, nb, L0, nq, nkv, t, tmax);
    const int G = nq / nkv;
    GAMER_CHECK_ARG((G == 1 || G == 2) && nb * G <= 4 * DB_MAXQ, "gamer_attn_decode_bf16: nq / nkv = %d (1 or 2), num_beams * (nq/nkv) = %d > %d",
                    G, nb * G, 4 * DB_MAXQ);
    GAMER_CHECK_ARG(ldq % 8 == 0 && ldkp % 8 == 0 && ldvp % 8 == 0 && ldg % 8 == 0 && ldq >= nq * 64 && ldkp >= nkv * 64 &&
                    ldvp >= nkv * 64 && ldg >= nkv * 64,
                    "gamer_attn_decode_bf16: leading dims ldq=%d ldkp=%d ldvp=%d ldg=%d must be multiples of 8 and cover the heads", ldq, ldkp,
                    ldvp, ldg);
    GAMER_CHECK_ARG(aligned16(q) && aligned16(kp) && aligned16(vp) && aligned16(kg) && aligned16(vg) && aligned16(o),
                    "gamer_attn_decode_bf16: q / k / v / o need 16-byte aligned bases");
    GAMER_CHECK_ARG((int64_t)B * nkv <= 0x7fffffff, "gamer_attn_decode_bf16: B * nkv = %lld workgroups", (long long)B * nkv);
    // one softmax reference per (32-key sub-tile, query row) lives in LDS behind the tile / merge region
    const int64_t nsub = gen_ok && t > 0 ? ((int64_t)L0 + t + 31) / 32 : ((int64_t)L0 + 31) / 32;
    const int64_t lds_bytes = DB_LDS_BYTES + nsub * 64 * (int64_t)sizeof(float);
    GAMER_CHECK_ARG(lds_bytes <= 160 * 1024, "gamer_attn_decode_bf16: L0 + t = %lld keys need %lld bytes of LDS (at most %d keys)",
                    (long long)L0 + t, (long long)lds_bytes, (160 * 1024 - DB_LDS_BYTES) / 256 * 32);
    const dim3 grid(B * nkv);
    return with_group(nq, nkv, [&](auto g) {
        return launch<attn_decode_b_kernel<g()>>("gamer_attn_decode_bf16", grid, dim3(256), (size_t)lds_bytes, (hipStream_t)stream,
                                                 reinterpret_cast<const bf16_t*>(q), ldq, reinterpret_cast<const bf16_t*>(kp), ldkp,
                                                 reinterpret_cast<const bf16_t*>(vp), ldvp, key_ok, reinterpret_cast<const bf16_t*>(kg),
                                                 reinterpret_cast<const bf16_t*>(vg), ldg, tmax, t, gen_ok, nb, L0, nq, nkv, scale,
                                                 (int)nsub, reinterpret_cast<bf16_t*>(o));
    });
}
