// The feed-forward activation step hm = dropout(act(pre [+ table row])) and its in-place backward, for every FFN of the package:
//   SwiGLU  hm = drop(silu(g) * u)   gate | up in two arrays (gamer_swiglu_fwd / _bwd) or in columns 0 .. I - 1 | I .. 2 I - 1 of the
//                                    rows of the fused projection's output (_ld; _ld_tbl adds tbl[row_group[t]], [groups][2 I], first:
//                                    the share of the projection that depends on the row's group only - gamer_inject_table_fwd)
//   SiLU    hm = drop(silu(h))       the non-gated FFN (mlp_type "PBATransformer": T5DenseActDense,
//                                    ref:SeqRec/models/generative/Qwen3Moe/FFN.py:75-86)
//   ReLU    act = drop(relu(pre + tbl[row_group[t]]))   PBATransformer's routed, injected layer ([groups][I]; a row whose group lies
//                                    outside [0, n_groups) adds nothing): tbl = the behaviour-embedding share of wi per (expert,
//                                    behaviour), so the [T, d_model + behaviour_dim] concatenation of the reference never exists
// The arithmetic is the rule's (common.h: SwigluRule, SiluRule, ReluRule); this file owns the walk.  Row forms: x is [T][ld] with
// the rule's inputs in columns 0 .. NIN I - 1, hm / dhm are [T][I] contiguous, one wave per row, 16-byte accesses; the backward
// writes the input gradients over the inputs and leaves the columns past them alone.  The dropout word of element (t, c) is that
// of the flat index t * I + c in every form, so the flat and the row forms, and SiLU and SwiGLU, draw the same masks from one seed.
// The bytes are read once and written once: the kernels are bound by HBM.
#include <limits.h>

#include "common.h"

namespace gamer {

// what a walk reads and what it writes: forward x -> other (= hm), backward (x, other = dhm) -> x
template <typename TA, bool BWD> using act_x_t = std::conditional_t<BWD, TA, const TA>;
template <typename TA, bool BWD> using act_other_t = std::conditional_t<BWD, const TA, TA>;

// The row walk: a wave per row t, a quad c of the row's I4 = I / 4 per lane and trip.  TBL: the table row of the row's group is
// added to the inputs first (the sums are used, not stored).  AMAX: the maxima of what is stored go to the armed sink
// (gamer_amax_sink: forward hm -> amax0; backward the first / second input gradient -> amax0 / amax1); without it, no LDS.
template <class R, typename TA, bool BWD, bool TBL, bool AMAX>
__global__ void __launch_bounds__(EW_THREADS)
act_row_kernel(act_x_t<TA, BWD>* __restrict__ x, int64_t ld, int T, int I4, act_other_t<TA, BWD>* __restrict__ other, float p, uint64_t seed,
               uint32_t* __restrict__ amax0, uint32_t* __restrict__ amax1, const float* __restrict__ tbl,
               const int32_t* __restrict__ row_group, int n_groups) {
    constexpr bool TWO = R::NIN == 2;
    uint32_t am0 = 0, am1 = 0;
    const DropoutRng rng(p, seed);
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * EW_THREADS + threadIdx.x) >> 6, nwaves = (gridDim.x * EW_THREADS) >> 6;
    for (int t = wave; t < T; t += nwaves) {
        auto* row = x + (int64_t)t * ld;
        const int g = TBL ? row_group[t] : 0;
        const bool add = TBL && (unsigned)g < (unsigned)n_groups;       // (a row of no group reads no table row)
        const float* trow = add ? tbl + (int64_t)g * (R::NIN * 4 * I4) : nullptr;
        for (int c = lane; c < I4; c += 64) {
            const int64_t i = (int64_t)t * I4 + c;
            float4 a = ld4(row + 4 * c), b = TWO ? ld4(row + 4 * (I4 + c)) : a, d;
            if (add) {
                const float4 ta = *reinterpret_cast<const float4*>(trow + 4 * c);
                a.x += ta.x; a.y += ta.y; a.z += ta.z; a.w += ta.w;
                if constexpr (TWO) {
                    const float4 tb = *reinterpret_cast<const float4*>(trow + 4 * (I4 + c));
                    b.x += tb.x; b.y += tb.y; b.z += tb.z; b.w += tb.w;
                }
            }
            // (the gradient after the table row: the wait for that row counts every load issued before it, and this one can
            // stay in flight over the mask's hash instead)
            if constexpr (BWD) d = ld4(other + 4 * i);
            float m[4];
            rng.mult4((uint32_t)i, m);
            if constexpr (BWD) {
                float4 da, db;
                act_bwd4<R>(a, b, d, m, da, db);
                st4(row + 4 * c, da);
                if (AMAX) am0 = amax_f4(am0, da);
                if constexpr (TWO) {
                    st4(row + 4 * (I4 + c), db);
                    if (AMAX) am1 = amax_f4(am1, db);
                }
            } else {
                const float4 o = act_fwd4<R>(a, b, m);
                st4(other + 4 * i, o);
                if (AMAX) am0 = amax_f4(am0, o);
            }
        }
    }
    if constexpr (AMAX) {
        __shared__ uint32_t amax_lds[BWD && TWO ? 2 : 1][4];
        amax_block_commit(am0, amax0, amax_lds[0]);
        if constexpr (BWD && TWO) amax_block_commit(am1, amax1, amax_lds[1]);
    }
}

// The flat walk of the contiguous SwiGLU pair: gate and up in two arrays of n = 4 n4 elements, thread-strided over the quads.
template <typename TA, bool BWD>
__global__ void __launch_bounds__(EW_THREADS)
swiglu_flat_kernel(act_x_t<TA, BWD>* __restrict__ g, act_x_t<TA, BWD>* __restrict__ u, act_other_t<TA, BWD>* __restrict__ other, int64_t n4,
                   float p, uint64_t seed, uint32_t* __restrict__ amax0, uint32_t* __restrict__ amax1) {
    __shared__ uint32_t amax_lds[BWD ? 2 : 1][4];
    uint32_t am0 = 0, am1 = 0;
    const DropoutRng rng(p, seed);
    for (int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; i < n4; i += (int64_t)gridDim.x * EW_THREADS) {
        const float4 a = ld4(g + 4 * i), b = ld4(u + 4 * i);
        float4 d;
        if constexpr (BWD) d = ld4(other + 4 * i);
        float m[4];
        rng.mult4((uint32_t)i, m);
        if constexpr (BWD) {
            float4 dg, du;
            act_bwd4<SwigluRule>(a, b, d, m, dg, du);
            st4(g + 4 * i, dg);
            st4(u + 4 * i, du);
            am0 = amax_f4(am0, dg);
            am1 = amax_f4(am1, du);
        } else {
            const float4 o = act_fwd4<SwigluRule>(a, b, m);
            st4(other + 4 * i, o);
            am0 = amax_f4(am0, o);
        }
    }
    amax_block_commit(am0, amax0, amax_lds[0]);
    if constexpr (BWD) amax_block_commit(am1, amax1, amax_lds[1]);
}

}  // namespace gamer

using namespace gamer;

// the dropout word of a quad is a 32-bit counter: a longer tensor would see its masks repeat
static constexpr long long DROP_MAX_QUADS = 0xffffffffLL;

// Every row form: check, take the sink, launch.  x [T][ld] holds the rule's NIN * I input columns, other = hm or dhm [T][I]; a table
// form takes tbl and row_group, any other form neither.
template <class R, typename TA, bool BWD, bool TBL, bool AMAX = true>
static int act_row(const char* name, act_x_t<TA, BWD>* x, int64_t ld, int T, int I, act_other_t<TA, BWD>* other, float p_drop, uint64_t seed,
                   void* stream, const float* tbl = nullptr, const int32_t* row_group = nullptr, int n_groups = INT_MAX) {
    GAMER_CHECK_ARG(TBL ? tbl && row_group && aligned16(tbl) : !tbl && !row_group, "%s: tbl (16-byte aligned) and row_group come together",
                    name);
    GAMER_CHECK_ARG(x && other && T > 0 && I > 0 && I % 4 == 0 && ld >= R::NIN * (int64_t)I && ld % 4 == 0 && p_drop >= 0.f && p_drop < 1.f,
                    "%s: bad arguments (T=%d I=%d ld=%lld)", name, T, I, (long long)ld);
    GAMER_CHECK_ARG((int64_t)T * (I / 4) <= DROP_MAX_QUADS, "%s: T * I / 4 = %lld exceeds the 32-bit dropout counter", name,
                    (long long)T * (I / 4));
    GAMER_CHECK_ARG(aligned_vec4<TA>(x) && aligned_vec4<TA>(other), "%s: pointers must be aligned to four elements", name);
    const AmaxSink sink = AMAX ? take_amax_sink() : AmaxSink{};
    return launch<act_row_kernel<R, TA, BWD, TBL, AMAX>>(name, dim3(grid_for_waves(T)), dim3(EW_THREADS), 0, ST(stream), x, ld, T, I / 4,
                                                         other, p_drop, seed, sink.out[0], sink.out[1], tbl, row_group, n_groups);
}

template <typename TA, bool BWD>
static int swiglu_flat(const char* name, act_x_t<TA, BWD>* g, act_x_t<TA, BWD>* u, int64_t n, act_other_t<TA, BWD>* other, float p_drop,
                       uint64_t seed, void* stream) {
    GAMER_CHECK_ARG(g && u && other && n > 0 && n % 4 == 0 && p_drop >= 0.f && p_drop < 1.f, "%s: bad arguments", name);
    GAMER_CHECK_ARG(n / 4 <= DROP_MAX_QUADS, "%s: n / 4 = %lld exceeds the 32-bit dropout counter", name, (long long)(n / 4));
    const AmaxSink sink = take_amax_sink();
    return launch<swiglu_flat_kernel<TA, BWD>>(name, dim3(grid_for_threads(n / 4)), dim3(EW_THREADS), 0, ST(stream), g, u, other, n / 4,
                                               p_drop, seed, sink.out[0], sink.out[1]);
}

extern "C" int gamer_swiglu_fwd(const float* g, const float* u, int64_t n, float p_drop, uint64_t seed, float* hm, void* stream) {
    return swiglu_flat<float, false>("gamer_swiglu_fwd", g, u, n, hm, p_drop, seed, stream);
}
extern "C" int gamer_swiglu_fwd_bf16(const gamer_bf16* g, const gamer_bf16* u, int64_t n, float p_drop, uint64_t seed, gamer_bf16* hm,
                                     void* stream) {
    return swiglu_flat<bf16_t, false>("gamer_swiglu_fwd_bf16", (const bf16_t*)g, (const bf16_t*)u, n, (bf16_t*)hm, p_drop, seed, stream);
}
extern "C" int gamer_swiglu_bwd(float* g, float* u, const float* dhm, int64_t n, float p_drop, uint64_t seed, void* stream) {
    return swiglu_flat<float, true>("gamer_swiglu_bwd", g, u, n, dhm, p_drop, seed, stream);
}
extern "C" int gamer_swiglu_bwd_bf16(gamer_bf16* g, gamer_bf16* u, const gamer_bf16* dhm, int64_t n, float p_drop, uint64_t seed,
                                     void* stream) {
    return swiglu_flat<bf16_t, true>("gamer_swiglu_bwd_bf16", (bf16_t*)g, (bf16_t*)u, n, (const bf16_t*)dhm, p_drop, seed, stream);
}

extern "C" int gamer_swiglu_fwd_ld(const float* gu, int64_t ld, int T, int I, float p_drop, uint64_t seed, float* hm, void* stream) {
    return act_row<SwigluRule, float, false, false>("gamer_swiglu_fwd_ld", gu, ld, T, I, hm, p_drop, seed, stream);
}
extern "C" int gamer_swiglu_fwd_ld_bf16(const gamer_bf16* gu, int64_t ld, int T, int I, float p_drop, uint64_t seed, gamer_bf16* hm,
                                        void* stream) {
    return act_row<SwigluRule, bf16_t, false, false>("gamer_swiglu_fwd_ld_bf16", (const bf16_t*)gu, ld, T, I, (bf16_t*)hm, p_drop, seed, stream);
}
extern "C" int gamer_swiglu_bwd_ld(float* gu, int64_t ld, int T, int I, const float* dhm, float p_drop, uint64_t seed, void* stream) {
    return act_row<SwigluRule, float, true, false>("gamer_swiglu_bwd_ld", gu, ld, T, I, dhm, p_drop, seed, stream);
}
extern "C" int gamer_swiglu_bwd_ld_bf16(gamer_bf16* gu, int64_t ld, int T, int I, const gamer_bf16* dhm, float p_drop, uint64_t seed,
                                        void* stream) {
    return act_row<SwigluRule, bf16_t, true, false>("gamer_swiglu_bwd_ld_bf16", (bf16_t*)gu, ld, T, I, (const bf16_t*)dhm, p_drop, seed, stream);
}
// (this ABI carries no group count: every group from 0 on reads its table row)
extern "C" int gamer_swiglu_fwd_ld_tbl(const float* gu, int64_t ld, int T, int I, float p_drop, uint64_t seed, float* hm,
                                       const float* tbl, const int32_t* row_group, void* stream) {
    GAMER_CHECK_ARG(tbl && row_group, "gamer_swiglu_fwd_ld_tbl: null table");
    return act_row<SwigluRule, float, false, true>("gamer_swiglu_fwd_ld_tbl", gu, ld, T, I, hm, p_drop, seed, stream, tbl, row_group);
}
extern "C" int gamer_swiglu_bwd_ld_tbl(float* gu, int64_t ld, int T, int I, const float* dhm, float p_drop, uint64_t seed,
                                       const float* tbl, const int32_t* row_group, void* stream) {
    GAMER_CHECK_ARG(tbl && row_group, "gamer_swiglu_bwd_ld_tbl: null table");
    return act_row<SwigluRule, float, true, true>("gamer_swiglu_bwd_ld_tbl", gu, ld, T, I, dhm, p_drop, seed, stream, tbl, row_group);
}

extern "C" int gamer_silu_fwd_ld(const float* h, int64_t ld, int T, int I, float p_drop, uint64_t seed, float* hm, void* stream) {
    return act_row<SiluRule, float, false, false>("gamer_silu_fwd_ld", h, ld, T, I, hm, p_drop, seed, stream);
}
extern "C" int gamer_silu_fwd_ld_bf16(const gamer_bf16* h, int64_t ld, int T, int I, float p_drop, uint64_t seed, gamer_bf16* hm,
                                      void* stream) {
    return act_row<SiluRule, bf16_t, false, false>("gamer_silu_fwd_ld_bf16", (const bf16_t*)h, ld, T, I, (bf16_t*)hm, p_drop, seed, stream);
}
extern "C" int gamer_silu_bwd_ld(float* h, int64_t ld, int T, int I, const float* dhm, float p_drop, uint64_t seed, void* stream) {
    return act_row<SiluRule, float, true, false>("gamer_silu_bwd_ld", h, ld, T, I, dhm, p_drop, seed, stream);
}
extern "C" int gamer_silu_bwd_ld_bf16(gamer_bf16* h, int64_t ld, int T, int I, const gamer_bf16* dhm, float p_drop, uint64_t seed,
                                      void* stream) {
    return act_row<SiluRule, bf16_t, true, false>("gamer_silu_bwd_ld_bf16", (bf16_t*)h, ld, T, I, (const bf16_t*)dhm, p_drop, seed, stream);
}

// (tbl and row_group both null: no table; what these two store feeds no split GEMM, so they leave an armed amax sink alone)
extern "C" int gamer_relu_tbl_fwd(const float* pre, int64_t ld, int T, int I, float p_drop, uint64_t seed, float* act, const float* tbl,
                                  const int32_t* row_group, int n_groups, void* stream) {
    return with_flags([&](auto t) {
        return act_row<ReluRule, float, false, t(), false>("gamer_relu_tbl_fwd", pre, ld, T, I, act, p_drop, seed, stream, tbl, row_group, n_groups);
    }, tbl || row_group);
}
extern "C" int gamer_relu_tbl_bwd(float* pre, int64_t ld, int T, int I, const float* dact, float p_drop, uint64_t seed, const float* tbl,
                                  const int32_t* row_group, int n_groups, void* stream) {
    return with_flags([&](auto t) {
        return act_row<ReluRule, float, true, t(), false>("gamer_relu_tbl_bwd", pre, ld, T, I, dact, p_drop, seed, stream, tbl, row_group, n_groups);
    }, tbl || row_group);
}
