// PBATransformer (the position- and behaviour-aware T5; ref:SeqRec/models/generative/PBATransformer): the two routers as one launch
// per stack call (the activation of its routed, injected ReLU feed-forward layer, gamer_relu_tbl_*, is one of ffn_act.hip's forms).
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
