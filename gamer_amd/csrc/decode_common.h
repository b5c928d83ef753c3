// What the cached decode attention kernels share (csrc/decode.hip: one workgroup per (sample, kv head), the key range split over the
// waves; csrc/candidates.hip: one workgroup per (sample, kv head, block of query rows), the query columns split over the waves): the
// K tile image, the row stride of the O^T state image the tails read, and the tail's 64-lane sum.
#pragma once
#include "common.h"

namespace gamer {

// Sum over the 64 lanes for the tail's dot products with the generated keys (up to tmax per query row, one after the other): the pairs of
// the xor 32, 16, 8, 4, 2, 1 butterfly in that order - v_permlane32_swap / v_permlane16_swap exchange the halves / the odd and even rows
// of 16, the rest are DPP row rotations and quad permutations (their partners hold the xor partner's VALUE once the earlier steps have
// made the lanes 8- and 4-periodic) - so the bits are those of wave_sum's __shfl_xor chain (checked on random data), without its six
// dependent ds_bpermute round trips per dot product.
__device__ __forceinline__ float wave_sum_x(float v) {
#define GAMER_DEC_DPP(ctrl) __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), ctrl, 0xf, 0xf, false))
    const auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    const auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(b[0]) + __uint_as_float(b[1]);
    v += GAMER_DEC_DPP(0x128);            // row_ror:8
    v += GAMER_DEC_DPP(0x124);            // row_ror:4
    v += GAMER_DEC_DPP(0x4E);             // quad_perm [2,3,0,1]
    v += GAMER_DEC_DPP(0xB1);             // quad_perm [1,0,3,2]
#undef GAMER_DEC_DPP
    return v;
}
constexpr int DEC_KLD = 68;             // floats per row of the K tile image (16-byte aligned rows, conflict-free)
constexpr int DEC_OLD = 65;             // row stride of the state image [query][64 d] the tail reads with lane = d

typedef float dec_f32x16 __attribute__((ext_vector_type(16)));

}  // namespace gamer
