// PBATransformer (the position- and behaviour-aware T5; ref:SeqRec/models/generative/PBATransformer): the two routers as one launch
// per stack call, and the activation of its routed, injected ReLU feed-forward layer in one pass each way.
//
// Routers (ref:.../PBATransformer/router.py): pure functions of the ids.  With P = num_positions,
//   encoder  token s of a right-padded row: position (s mod P) + 1 - [1, 2, 2, ..] per item under Moe_behavior_only with behaviour
//            tokens, all 1 without them - and 0 from slot n_items * P on (the reference's </s> entry); behaviour =
//            lut[token at s - (s mod P)] + 1 for s mod P != 0, else 0, and 0 from (S / P) * P on; both 0 at pad / eos
//   decoder  position [0, 1 .. P, 0][s] (Moe_behavior_only: [0, 1, 2, 2, .., 0] / [0, 1, 1, .., 0]); behaviour 0 for s <= 1 and
//            s > P, lut[token at 1] + 1 between; both 0 at pad / eos
// key[t] = expert * NB1 + behaviour, the row's (expert, behaviour) group of the injection table, -1 where no expert owns the position
// (the reference leaves such rows' feed-forward output at zero).  bad_token counts the positions whose behaviour is USED (not pad,
// not eos, not a behaviour slot itself) and whose slot token the table does not map; the reference indexes its embedding out of
// range there.  It is incremented, never cleared (as gamer_moe_router_prep's).
//
// relu_tbl: act[t, j] = drop(relu(pre[t, j] + tbl[row_group[t], j])) (a row whose group lies outside [0, n_groups) adds nothing);
// backward in place pre <- mask * scale * dact * (pre + tbl > 0).
// tbl = the behaviour-embedding share of wi per (expert, behaviour) (gamer_inject_table_fwd), so the [T, d_model + behaviour_dim]
// concatenation of the reference never exists.  One wave per row, 16-byte accesses, the mask of element (t, j) from the counter
// hash at index t * (I / 4) + j / 4: the bytes are read once and written once, the kernels are bound by HBM.
#include "common.h"

namespace gamer {

__global__ void __launch_bounds__(256)
pba_router_kernel(const int64_t* __restrict__ ids, int S, int decoder, int P, int n_items, int moe_only, int use_beh,
                  const int32_t* __restrict__ lut, int vocab, int NB1, int num_experts, int pad_id, int eos_id,
                  int32_t* __restrict__ expert, int32_t* __restrict__ beh_idx, int32_t* __restrict__ key,
                  int32_t* __restrict__ bad_token) {
    const int64_t base = (int64_t)blockIdx.x * S;
    int bad = 0;
    for (int s = threadIdx.x; s < S; s += blockDim.x) {
        const int64_t id = ids[base + s];
        const bool special = (id == pad_id) || (id == eos_id);
        int r, slot;                 // the place inside the item, and where the item's behaviour token sits
        bool item;                   // s lies inside an item
        bool beh_range;              // ... and inside the range the reference fills with behaviour indices
        if (decoder) {
            r = s - 1; slot = 1;
            item = s >= 1 && s <= P;
            beh_range = item && S > 1;
        } else {
            r = s % P; slot = s - r;
            item = s < n_items * P;
            beh_range = s < (S / P) * P;
        }
        int e = 0, bi = 0;
        if (item && !special) e = moe_only ? (use_beh ? (r == 0 ? 1 : 2) : 1) : r + 1;
        if (use_beh && beh_range && r != 0 && !special) {
            const int64_t btok = ids[base + slot];
            if (btok >= 0 && btok < vocab && lut[btok] >= 0 && lut[btok] + 1 < NB1) bi = lut[btok] + 1;
            else ++bad;
        }
        expert[base + s] = e;
        beh_idx[base + s] = bi;
        if (key) key[base + s] = e < num_experts ? e * NB1 + bi : -1;
    }
    if (bad) atomicAdd(bad_token, bad);
}

template <bool TBL>
__global__ void __launch_bounds__(EW_THREADS)
relu_tbl_fwd_kernel(const float* __restrict__ pre, int64_t ld, int T, int I4, float p, uint64_t seed, float* __restrict__ act,
                    const float* __restrict__ tbl, const int32_t* __restrict__ row_group, int n_groups) {
    const DropoutRng rng(p, seed);
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * EW_THREADS + threadIdx.x) >> 6, nwaves = (gridDim.x * EW_THREADS) >> 6;
    for (int t = wave; t < T; t += nwaves) {
        const float* row = pre + (int64_t)t * ld;
        const int g = TBL ? row_group[t] : 0;
        const bool add = TBL && (unsigned)g < (unsigned)n_groups;       // (a row of no group reads no table row)
        const float* trow = add ? tbl + (int64_t)g * (4 * I4) : nullptr;
        for (int c = lane; c < I4; c += 64) {
            float4 a = ld4(row + 4 * c);
            if (add) {
                const float4 b = *reinterpret_cast<const float4*>(trow + 4 * c);
                a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
            }
            const int64_t i = (int64_t)t * I4 + c;
            float m[4];
            rng.mult4((uint32_t)i, m);
            float4 o;
            o.x = a.x > 0.f ? m[0] * a.x : 0.f;
            o.y = a.y > 0.f ? m[1] * a.y : 0.f;
            o.z = a.z > 0.f ? m[2] * a.z : 0.f;
            o.w = a.w > 0.f ? m[3] * a.w : 0.f;
            st4(act + 4 * i, o);
        }
    }
}

template <bool TBL>
__global__ void __launch_bounds__(EW_THREADS)
relu_tbl_bwd_kernel(float* __restrict__ pre, int64_t ld, int T, int I4, const float* __restrict__ dact, float p, uint64_t seed,
                    const float* __restrict__ tbl, const int32_t* __restrict__ row_group, int n_groups) {
    const DropoutRng rng(p, seed);
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * EW_THREADS + threadIdx.x) >> 6, nwaves = (gridDim.x * EW_THREADS) >> 6;
    for (int t = wave; t < T; t += nwaves) {
        float* row = pre + (int64_t)t * ld;
        const int g = TBL ? row_group[t] : 0;
        const bool add = TBL && (unsigned)g < (unsigned)n_groups;       // (a row of no group reads no table row)
        const float* trow = add ? tbl + (int64_t)g * (4 * I4) : nullptr;
        for (int c = lane; c < I4; c += 64) {
            float4 a = ld4(row + 4 * c);
            if (add) {
                const float4 b = *reinterpret_cast<const float4*>(trow + 4 * c);
                a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
            }
            const int64_t i = (int64_t)t * I4 + c;
            const float4 d = ld4(dact + 4 * i);
            float m[4];
            rng.mult4((uint32_t)i, m);
            float4 o;
            o.x = a.x > 0.f ? m[0] * d.x : 0.f;
            o.y = a.y > 0.f ? m[1] * d.y : 0.f;
            o.z = a.z > 0.f ? m[2] * d.z : 0.f;
            o.w = a.w > 0.f ? m[3] * d.w : 0.f;
            st4(row + 4 * c, o);
        }
    }
}

}  // namespace gamer

using namespace gamer;

extern "C" int gamer_pba_router(const int64_t* ids, int B, int S, int decoder, int num_positions, int n_items, int moe_behavior_only,
                                int use_behavior_token, const int32_t* behavior_lut, int vocab, int nb1, int num_experts, int pad_id,
                                int eos_id, int32_t* expert, int32_t* beh_idx, int32_t* key, int32_t* bad_token, void* stream) {
    GAMER_CHECK_ARG(ids && expert && beh_idx && bad_token, "gamer_pba_router: null pointer");
    GAMER_CHECK_ARG(B > 0 && S > 0 && num_positions > 0 && n_items > 0 && nb1 > 0 && num_experts > 0,
                    "gamer_pba_router: bad shape B=%d S=%d P=%d n_items=%d NB1=%d E=%d", B, S, num_positions, n_items, nb1, num_experts);
    GAMER_CHECK_ARG(!use_behavior_token || (behavior_lut && vocab > 0), "gamer_pba_router: behaviour tokens need the lookup table");
    hipLaunchKernelGGL(pba_router_kernel, dim3(B), dim3(256), 0, ST(stream), ids, S, decoder ? 1 : 0, num_positions, n_items,
                       moe_behavior_only ? 1 : 0, use_behavior_token ? 1 : 0, behavior_lut, vocab, nb1, num_experts, pad_id, eos_id,
                       expert, beh_idx, key, bad_token);
    GAMER_CHECK_LAUNCH("gamer_pba_router");
    return 0;
}

static int relu_tbl_check(const char* name, const float* pre, int64_t ld, int T, int I, float p_drop, const float* other, const float* tbl,
                          const int32_t* row_group) {
    GAMER_CHECK_ARG((tbl == nullptr) == (row_group == nullptr) && aligned16(tbl), "%s: tbl (16-byte aligned) and row_group come together",
                    name);
    GAMER_CHECK_ARG(pre && other && T > 0 && I > 0 && I % 4 == 0 && ld >= (int64_t)I && ld % 4 == 0 && p_drop >= 0.f && p_drop < 1.f,
                    "%s: bad arguments (T=%d I=%d ld=%lld)", name, T, I, (long long)ld);
    GAMER_CHECK_ARG((int64_t)T * (I / 4) <= 0xffffffffLL, "%s: T * I / 4 = %lld exceeds the 32-bit dropout counter", name,
                    (long long)T * (I / 4));
    GAMER_CHECK_ARG(aligned16(pre) && aligned16(other), "%s: pointers must be 16-byte aligned", name);
    return 0;
}

extern "C" int gamer_relu_tbl_fwd(const float* pre, int64_t ld, int T, int I, float p_drop, uint64_t seed, float* act, const float* tbl,
                                  const int32_t* row_group, int n_groups, void* stream) {
    GAMER_TRY(relu_tbl_check("gamer_relu_tbl_fwd", pre, ld, T, I, p_drop, act, tbl, row_group));
    if (tbl)
        hipLaunchKernelGGL(relu_tbl_fwd_kernel<true>, dim3(grid_for_waves(T)), dim3(EW_THREADS), 0, ST(stream), pre, ld, T, I / 4, p_drop,
                           seed, act, tbl, row_group, n_groups);
    else
        hipLaunchKernelGGL(relu_tbl_fwd_kernel<false>, dim3(grid_for_waves(T)), dim3(EW_THREADS), 0, ST(stream), pre, ld, T, I / 4, p_drop,
                           seed, act, tbl, row_group, n_groups);
    GAMER_CHECK_LAUNCH("gamer_relu_tbl_fwd");
    return 0;
}

extern "C" int gamer_relu_tbl_bwd(float* pre, int64_t ld, int T, int I, const float* dact, float p_drop, uint64_t seed, const float* tbl,
                                  const int32_t* row_group, int n_groups, void* stream) {
    GAMER_TRY(relu_tbl_check("gamer_relu_tbl_bwd", pre, ld, T, I, p_drop, dact, tbl, row_group));
    if (tbl)
        hipLaunchKernelGGL(relu_tbl_bwd_kernel<true>, dim3(grid_for_waves(T)), dim3(EW_THREADS), 0, ST(stream), pre, ld, T, I / 4, dact,
                           p_drop, seed, tbl, row_group, n_groups);
    else
        hipLaunchKernelGGL(relu_tbl_bwd_kernel<false>, dim3(grid_for_waves(T)), dim3(EW_THREADS), 0, ST(stream), pre, ld, T, I / 4, dact,
                           p_drop, seed, tbl, row_group, n_groups);
    GAMER_CHECK_LAUNCH("gamer_relu_tbl_bwd");
    return 0;
}
