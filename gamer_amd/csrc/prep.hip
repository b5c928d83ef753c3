// Router maps, mask-predicate levels, empty-row flags and expert token lists (integer work).
// Reference behaviour restated: ref:SeqRec/models/generative/Qwen3Multi/router.py:74-201,
// ref:SeqRec/models/generative/Qwen3Multi/model.py:573-630,691-741,
// ref:SeqRec/models/generative/Qwen3Moe/FFN.py:63-68.
#include "common.h"
#include <atomic>

namespace gamer {

static thread_local char g_err[512] = {0};
static std::atomic<unsigned> g_env_epoch{1};
unsigned env_epoch() { return g_env_epoch.load(std::memory_order_acquire); }
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    // every failing entry point comes through here: whatever the caller armed for "the next launch" (gamer_amax_sink,
    // gamer_attn_split_amax) must not survive a rejected call and attach itself to a later launch of another tensor
    take_amax_sink();
    disarm_attn_amax();
}

constexpr int ROUTER_THREADS = 256;
constexpr int INT_BIG = 0x7fffffff;

// One workgroup per sequence.  LDS prefix-min scan gives min_{j<=i} klevel[j] for the empty flags.
__global__ void __launch_bounds__(ROUTER_THREADS)
router_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ attn_mask,
              const int64_t* __restrict__ actions, const int32_t* __restrict__ lut, int vocab,
              int S, int P, int pad_id, int eos_id,
              int32_t* __restrict__ expert, int32_t* __restrict__ beh_idx, int32_t* __restrict__ act_idx,
              int32_t* __restrict__ kl_self, int32_t* __restrict__ kl_cross, int32_t* __restrict__ ql_cross,
              int32_t* __restrict__ empty_self, int32_t* __restrict__ empty_cross,
              int32_t* __restrict__ tile_empty_self, int32_t* __restrict__ tile_empty_cross,
              int32_t* __restrict__ bad_token) {
    extern __shared__ __attribute__((aligned(16))) int32_t smem[];
    int32_t* pm_self = smem;            // [S] running min of kl_self
    int32_t* pm_cross = smem + S;       // [S]
    int32_t* tmp_a = smem + 2 * S;      // [S] scan ping-pong
    int32_t* tmp_b = smem + 3 * S;      // [S]
    const int b = blockIdx.x;
    const int64_t base = (int64_t)b * S;
    const int n_tiles = (S + 31) / 32;

    for (int t = threadIdx.x; t < S; t += blockDim.x) {
        const int64_t id = ids[base + t];
        const bool special = (id == pad_id) || (id == eos_id);
        const int e = special ? 0 : (t % P) + 1;
        // behaviour token of this token's item
        const int first = (t / P) * P;
        const int64_t btok = ids[base + first];
        int a;
        if (btok >= 0 && btok < vocab && lut[btok] >= 0) {
            a = lut[btok] + 1;
        } else {
            a = 0;
            if (!special && t == first) atomicAdd(bad_token, 1);
        }
        if (special) a = 0;
        expert[base + t] = e;
        act_idx[base + t] = a;
        beh_idx[base + t] = (t % P == 0) ? 0 : a;
        const bool keep = attn_mask ? (attn_mask[base + t] != 0) : true;
        int64_t lv64 = actions ? actions[base + t] : 0;
        if (lv64 > 0x3fffffff) lv64 = 0x3fffffff;
        if (lv64 < -0x3fffffff) lv64 = -0x3fffffff;
        const int lv = (int)lv64;
        const int ks = keep ? 0 : INT_BIG;
        const int kc = keep ? lv : INT_BIG;
        kl_self[base + t] = ks;
        kl_cross[base + t] = kc;
        ql_cross[base + t] = lv;
        pm_self[t] = ks;
        pm_cross[t] = kc;
    }
    __syncthreads();
    // inclusive prefix-min (Hillis-Steele) for both arrays
    for (int which = 0; which < 2; ++which) {
        int32_t* src = which ? pm_cross : pm_self;
        int32_t* a = src;
        int32_t* bb = tmp_a;
        for (int off = 1; off < S; off <<= 1) {
            for (int t = threadIdx.x; t < S; t += blockDim.x) {
                int v = a[t];
                if (t >= off) v = min(v, a[t - off]);
                bb[t] = v;
            }
            __syncthreads();
            int32_t* nx = (bb == tmp_a) ? tmp_b : tmp_a;
            a = bb;
            bb = nx;
        }
        // copy back if result is not in src
        if (a != src) {
            for (int t = threadIdx.x; t < S; t += blockDim.x) src[t] = a[t];
        }
        __syncthreads();
    }
    for (int t = threadIdx.x; t < S; t += blockDim.x) {
        const int lv = ql_cross[base + t];      // written by this same thread above
        const int es = (pm_self[t] < 1) ? 0 : 1;
        const int ec = (pm_cross[t] < lv) ? 0 : 1;
        empty_self[base + t] = es;
        empty_cross[base + t] = ec;
        tmp_a[t] = es;
        tmp_b[t] = ec;
    }
    __syncthreads();
    for (int qt = threadIdx.x; qt < n_tiles; qt += blockDim.x) {
        int es = 0, ec = 0;
        for (int t = qt * 32; t < min(S, qt * 32 + 32); ++t) {
            es |= tmp_a[t];
            ec |= tmp_b[t];
        }
        tile_empty_self[(int64_t)b * n_tiles + qt] = es;
        tile_empty_cross[(int64_t)b * n_tiles + qt] = ec;
    }
}

// ---- session spans (Qwen3SessionMulti) ------------------------------------------------------
// ref:SeqRec/models/generative/Qwen3SessionMulti/model.py:545-551 (in-item mask), :556-613 (cross mask),
// :676-728 (self mask), :983-984 (RoPE positions = extended_session_ids).
// The reference masks key j for query i unless sess[j] < sess[i] (plus, for the self attention, the keys of the
// query's own item up to the query).  Session ids that do not decrease along the kept tokens make
// {kept j : sess[j] < sess[i]} a prefix of the kept keys, so the masks become per-query spans:
//   lim_i = 1 + last kept j with sess[j] < sess[i]   (0 if none)
//   self : j <= i, minus the hole [lim_i, first token of i's item)        cross: j <= lim_i - 1 (and kl[j] < ql[i])
// One workgroup per sequence; each row scans the sequence in LDS (S^2 integer compares, ~0.1 ms at B = 1024).
// Rows whose span would not be causal / not a prefix (ids out of order) are counted in `violations` and clamped.
// CROSS = true: Qwen3SessionMulti, after the router (kl_cross / ql_cross in, the cross span and empty flags out).
// CROSS = false: Qwen3Session (HF Qwen3ForCausalLM with the same self mask, no router): kl_self is written here, 0 for a
// kept key and INT_BIG for a padded one, as causal_prep_kernel does; no cross input or output is touched.
// The work of one workgroup (= one sequence b) is session_spans_row; ``sraw`` is its LDS, S (8 + 4 (CROSS ? 4 : 2)) bytes
// (session_span_lds).  The kernels of gamer_session_spans / gamer_session_prep are this function alone;
// session_moe_prep_kernel runs it behind Qwen3Moe's routing.
template <bool CROSS>
constexpr size_t session_span_lds(int S) { return (size_t)S * (sizeof(int64_t) + (CROSS ? 4 : 2) * sizeof(int32_t)); }

template <bool CROSS>
__device__ __forceinline__ void
session_spans_row(unsigned char* sraw, const int64_t* __restrict__ sess, const int64_t* __restrict__ ext_ids,
                  const int64_t* __restrict__ attn_mask, const int32_t* __restrict__ kl_cross,
                  const int32_t* __restrict__ ql_cross, int S, int P, int n_pos, int32_t* __restrict__ kl_self,
                  int32_t* __restrict__ span_self, int32_t* __restrict__ span_cross, int32_t* __restrict__ pos_ids,
                  int32_t* __restrict__ empty_self, int32_t* __restrict__ empty_cross,
                  int32_t* __restrict__ tile_empty_self, int32_t* __restrict__ tile_empty_cross,
                  int32_t* __restrict__ violations) {
    int64_t* sess_s = reinterpret_cast<int64_t*>(sraw);                 // [S]
    int32_t* keep_s = reinterpret_cast<int32_t*>(sess_s + S);           // [S]
    int32_t* klc_s = keep_s + S;                                        // [S] cross key level (INT_MAX if padded; CROSS only)
    int32_t* es_s = klc_s + (CROSS ? S : 0);                            // [S] empty flags for the tile reduction
    int32_t* ec_s = es_s + S;                                           // [S] (CROSS only)
    const int b = blockIdx.x;
    const int64_t base = (int64_t)b * S;
    for (int t = threadIdx.x; t < S; t += blockDim.x) {
        sess_s[t] = sess[base + t];
        const int keep = attn_mask ? (attn_mask[base + t] != 0 ? 1 : 0) : 1;
        keep_s[t] = keep;
        if constexpr (CROSS) klc_s[t] = kl_cross[base + t];
        else kl_self[base + t] = keep ? 0 : INT_BIG;
    }
    __syncthreads();
    int bad = 0;
    for (int i = threadIdx.x; i < S; i += blockDim.x) {
        const int64_t si = sess_s[i];
        int last_lt = -1, first_ge = INT_BIG;
        for (int j = 0; j < S; ++j) {
            if (keep_s[j]) {
                if (sess_s[j] < si) last_lt = j;
                else first_ge = min(first_ge, j);
            }
        }
        if (last_lt > first_ge || last_lt >= i) ++bad;            // not a prefix of the kept keys / not causal
        const int lim = min(last_lt + 1, i);
        const int istart = i - i % P;
        bool any_before = false;
        int klmin = INT_BIG;
        for (int j = 0; j < lim; ++j) {
            any_before |= keep_s[j] != 0;
            if constexpr (CROSS) klmin = min(klmin, klc_s[j]);
        }
        bool any_item = false;
        for (int j = istart; j <= i; ++j) any_item |= keep_s[j] != 0;
        const int es = (any_before || any_item) ? 0 : 1;
        const bool hole = lim < istart;
        reinterpret_cast<int4*>(span_self)[base + i] = make_int4(i, hole ? lim : INT_BIG, hole ? istart : 0, 0);
        empty_self[base + i] = es;
        es_s[i] = es;
        if constexpr (CROSS) {
            const int ec = (klmin < ql_cross[base + i]) ? 0 : 1;
            reinterpret_cast<int4*>(span_cross)[base + i] = make_int4(lim - 1, INT_BIG, 0, 0);
            empty_cross[base + i] = ec;
            ec_s[i] = ec;
        }
        int64_t p = ext_ids ? ext_ids[base + i] : (int64_t)i;
        if (p < 0 || p >= n_pos) { ++bad; p = p < 0 ? 0 : n_pos - 1; }
        pos_ids[base + i] = (int32_t)p;
    }
    if (bad) atomicAdd(violations, bad);
    __syncthreads();
    const int n_tiles = (S + 31) / 32;
    for (int qt = threadIdx.x; qt < n_tiles; qt += blockDim.x) {
        int es = 0, ec = 0;
        for (int t = qt * 32; t < min(S, qt * 32 + 32); ++t) {
            es |= es_s[t];
            if constexpr (CROSS) ec |= ec_s[t];
        }
        tile_empty_self[(int64_t)b * n_tiles + qt] = es;
        if constexpr (CROSS) tile_empty_cross[(int64_t)b * n_tiles + qt] = ec;
    }
}

template <bool CROSS>
__global__ void __launch_bounds__(ROUTER_THREADS)
session_span_kernel(const int64_t* __restrict__ sess, const int64_t* __restrict__ ext_ids,
                    const int64_t* __restrict__ attn_mask, const int32_t* __restrict__ kl_cross,
                    const int32_t* __restrict__ ql_cross, int S, int P, int n_pos, int32_t* __restrict__ kl_self,
                    int32_t* __restrict__ span_self, int32_t* __restrict__ span_cross, int32_t* __restrict__ pos_ids,
                    int32_t* __restrict__ empty_self, int32_t* __restrict__ empty_cross,
                    int32_t* __restrict__ tile_empty_self, int32_t* __restrict__ tile_empty_cross,
                    int32_t* __restrict__ violations) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sraw[];
    session_spans_row<CROSS>(sraw, sess, ext_ids, attn_mask, kl_cross, ql_cross, S, P, n_pos, kl_self, span_self, span_cross,
                             pos_ids, empty_self, empty_cross, tile_empty_self, tile_empty_cross, violations);
}

// ---- expert lists ---------------------------------------------------------------------------
// pass 1: per-sequence member counts   work[b*E + e]
__global__ void expert_count_kernel(const int32_t* __restrict__ expert, int S, int E,
                                    int32_t* __restrict__ work) {
    __shared__ int cnt[64];
    const int b = blockIdx.x;
    if (threadIdx.x < 64) cnt[threadIdx.x] = 0;
    __syncthreads();
    for (int t = threadIdx.x; t < S; t += blockDim.x) {
        const int e = expert[(int64_t)b * S + t];
        if ((unsigned)e < (unsigned)E) atomicAdd(&cnt[e], 1);     // rows past the last expert are in no group
    }
    __syncthreads();
    if (threadIdx.x < E) work[(int64_t)b * E + threadIdx.x] = cnt[threadIdx.x];
}

// pass 2 (single workgroup): exclusive scan over sequences per expert, then expert bases.
// work[b*E+e] <- global start slot of (sequence b, expert e); offsets[e] = segment starts.
__global__ void __launch_bounds__(1024)
expert_scan_kernel(int B, int E, int T, int32_t* __restrict__ work, int32_t* __restrict__ offsets) {
    __shared__ int32_t sh[1024];
    __shared__ int32_t carry;
    __shared__ int32_t totals[65];
    const int tid = threadIdx.x;
    for (int e = 0; e < E; ++e) {
        if (tid == 0) carry = 0;
        __syncthreads();
        for (int b0 = 0; b0 < B; b0 += 1024) {
            const int b = b0 + tid;
            const int v = (b < B) ? work[(int64_t)b * E + e] : 0;
            sh[tid] = v;
            __syncthreads();
            for (int off = 1; off < 1024; off <<= 1) {
                int add = (tid >= off) ? sh[tid - off] : 0;
                __syncthreads();
                sh[tid] += add;
                __syncthreads();
            }
            const int incl = sh[tid];
            const int c = carry;
            if (b < B) work[(int64_t)b * E + e] = c + incl - v;   // exclusive, within this expert
            __syncthreads();
            if (tid == 1023) carry = c + incl;
            __syncthreads();
        }
        if (tid == 0) totals[e] = carry;
        __syncthreads();
    }
    __shared__ int32_t sbase[65];
    if (tid == 0) {
        int acc = 0;
        for (int e = 0; e < E; ++e) {
            offsets[e] = acc;
            sbase[e] = acc;
            acc += totals[e];
        }
        offsets[E] = acc;   // == T
    }
    __syncthreads();
    // add the expert base
    for (int i = tid; i < B * E; i += 1024) {
        work[i] += sbase[i % E];
    }
}

// pass 3: one wave per sequence; lane e (< E) walks the sequence in token order and emits slots.  Lane E emits the rows whose
// expert index is outside [0, E) - in no group - behind the last group, in token order: slots offsets[E] .. T - 1, so that perm
// and slot stay permutations of [0, T).  Its base is offsets[E] plus the ungrouped rows of the sequences before b (b S minus
// their grouped rows, which the scanned work table gives per expert).
__global__ void expert_emit_kernel(const int32_t* __restrict__ expert, int S, int E,
                                   const int32_t* __restrict__ work, const int32_t* __restrict__ offsets,
                                   int32_t* __restrict__ perm, int32_t* __restrict__ slot) {
    const int b = blockIdx.x;
    const int e = threadIdx.x;
    if (e > E) return;
    const int64_t base = (int64_t)b * S;
    if (e == E) {
        int64_t grouped_before = 0;
        for (int g = 0; g < E; ++g) grouped_before += work[(int64_t)b * E + g] - offsets[g];
        int next = (int)(offsets[E] + base - grouped_before);
        for (int t = 0; t < S; ++t) {
            if ((unsigned)expert[base + t] >= (unsigned)E) {
                perm[next] = (int32_t)(base + t);
                slot[base + t] = next;
                ++next;
            }
        }
        return;
    }
    int next = work[(int64_t)b * E + e];
    for (int t = 0; t < S; ++t) {
        if (expert[base + t] == e) {
            perm[next] = (int32_t)(base + t);
            slot[base + t] = next;
            ++next;
        }
    }
}

// The router's position table (router.py:28-54): expert[i] <- table[expert[i]] for 0 <= expert[i] < n_table.
__global__ void __launch_bounds__(256)
position_table_kernel(int32_t* __restrict__ expert, int64_t n, const int32_t* __restrict__ table, int n_table) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int e = expert[i];
        if ((unsigned)e < (unsigned)n_table) expert[i] = table[e];
    }
}

// Labels outside [0, V) that are not ignore_index: torch's CrossEntropyLoss raises on them (a tokenizer / vocab_size
// mismatch); the CE kernels skip such rows, so they are counted here and the host raises (Engine.check_inputs).
__global__ void __launch_bounds__(256)
check_labels_kernel(const int64_t* __restrict__ labels, int64_t n, int V, int ignore_index, int32_t* __restrict__ bad) {
    int cnt = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t y = labels[i];
        cnt += (y != ignore_index && (y < 0 || y >= V)) ? 1 : 0;
    }
    if (__any(cnt)) {
        cnt = wave_sum_i32(cnt);
        if ((threadIdx.x & 63) == 0) atomicAdd(bad, cnt);
    }
}

}  // namespace gamer

using namespace gamer;

extern "C" int gamer_abi_version(void) { return GAMER_ABI_VERSION; }
extern "C" int gamer_reload_env(void) { gamer::g_env_epoch.fetch_add(1, std::memory_order_acq_rel); return 0; }
extern "C" const char* gamer_last_error(void) { return gamer::g_err; }

extern "C" int gamer_router_fwd(const int64_t* ids, const int64_t* attn_mask, const int64_t* actions,
                                const int32_t* behavior_lut, int vocab, int B, int S, int num_positions,
                                int pad_id, int eos_id,
                                int32_t* expert, int32_t* beh_idx, int32_t* act_idx,
                                int32_t* kl_self, int32_t* kl_cross, int32_t* ql_cross,
                                int32_t* empty_self, int32_t* empty_cross,
                                int32_t* tile_empty_self, int32_t* tile_empty_cross,
                                int32_t* bad_token, void* stream) {
    GAMER_CHECK_ARG(ids && behavior_lut && expert && beh_idx && act_idx && kl_self && kl_cross &&
                    ql_cross && empty_self && empty_cross && tile_empty_self && tile_empty_cross && bad_token,
                    "gamer_router_fwd: null pointer");
    GAMER_CHECK_ARG(B > 0 && S > 0 && num_positions > 0, "gamer_router_fwd: bad shape B=%d S=%d P=%d", B, S, num_positions);
    GAMER_CHECK_ARG(S <= 8192, "gamer_router_fwd: S=%d > 8192 unsupported", S);
    const size_t shmem = (size_t)4 * S * sizeof(int32_t);
    hipLaunchKernelGGL(router_kernel, dim3(B), dim3(ROUTER_THREADS), shmem, (hipStream_t)stream,
                       ids, attn_mask, actions, behavior_lut, vocab, S, num_positions, pad_id, eos_id,
                       expert, beh_idx, act_idx, kl_self, kl_cross, ql_cross, empty_self, empty_cross,
                       tile_empty_self, tile_empty_cross, bad_token);
    GAMER_CHECK_LAUNCH("gamer_router_fwd");
    return 0;
}

extern "C" int gamer_session_spans(const int64_t* session_ids, const int64_t* extended_session_ids,
                                   const int64_t* attn_mask, const int32_t* kl_cross, const int32_t* ql_cross,
                                   int B, int S, int num_positions, int n_rope_positions,
                                   int32_t* span_self, int32_t* span_cross, int32_t* pos_ids,
                                   int32_t* empty_self, int32_t* empty_cross,
                                   int32_t* tile_empty_self, int32_t* tile_empty_cross, int32_t* violations,
                                   void* stream) {
    GAMER_CHECK_ARG(session_ids && kl_cross && ql_cross && span_self && span_cross && pos_ids && empty_self &&
                    empty_cross && tile_empty_self && tile_empty_cross && violations,
                    "gamer_session_spans: null pointer");
    GAMER_CHECK_ARG(B > 0 && S > 0 && num_positions > 0 && n_rope_positions > 0,
                    "gamer_session_spans: bad shape B=%d S=%d P=%d n_pos=%d", B, S, num_positions, n_rope_positions);
    GAMER_CHECK_ARG(S <= 2048, "gamer_session_spans: S=%d > 2048 unsupported", S);
    const size_t shmem = session_span_lds<true>(S);
    hipLaunchKernelGGL(session_span_kernel<true>, dim3(B), dim3(ROUTER_THREADS), shmem, (hipStream_t)stream,
                       session_ids, extended_session_ids, attn_mask, kl_cross, ql_cross, S, num_positions,
                       n_rope_positions, nullptr, span_self, span_cross, pos_ids, empty_self, empty_cross,
                       tile_empty_self, tile_empty_cross, violations);
    GAMER_CHECK_LAUNCH("gamer_session_spans");
    return 0;
}

extern "C" int gamer_session_prep(const int64_t* session_ids, const int64_t* extended_session_ids,
                                  const int64_t* attn_mask, int B, int S, int num_positions, int n_rope_positions,
                                  int32_t* kl_self, int32_t* span_self, int32_t* pos_ids, int32_t* empty_self,
                                  int32_t* tile_empty_self, int32_t* violations, void* stream) {
    GAMER_CHECK_ARG(session_ids && kl_self && span_self && pos_ids && empty_self && tile_empty_self && violations,
                    "gamer_session_prep: null pointer");
    GAMER_CHECK_ARG(B > 0 && S > 0 && num_positions > 0 && n_rope_positions > 0,
                    "gamer_session_prep: bad shape B=%d S=%d P=%d n_pos=%d", B, S, num_positions, n_rope_positions);
    GAMER_CHECK_ARG(S <= 2048, "gamer_session_prep: S=%d > 2048 unsupported", S);
    const size_t shmem = session_span_lds<false>(S);
    hipLaunchKernelGGL(session_span_kernel<false>, dim3(B), dim3(ROUTER_THREADS), shmem, (hipStream_t)stream,
                       session_ids, extended_session_ids, attn_mask, nullptr, nullptr, S, num_positions,
                       n_rope_positions, kl_self, span_self, nullptr, pos_ids, empty_self, nullptr,
                       tile_empty_self, nullptr, violations);
    GAMER_CHECK_LAUNCH("gamer_session_prep");
    return 0;
}

extern "C" int gamer_expert_lists(const int32_t* expert, int B, int S, int num_experts,
                                  int32_t* perm, int32_t* slot, int32_t* offsets, int32_t* work, void* stream) {
    GAMER_CHECK_ARG(expert && perm && slot && offsets && work, "gamer_expert_lists: null pointer");
    GAMER_CHECK_ARG(B > 0 && S > 0 && num_experts > 0 && num_experts <= 64,
                    "gamer_expert_lists: bad shape B=%d S=%d E=%d", B, S, num_experts);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(expert_count_kernel, dim3(B), dim3(256), 0, st, expert, S, num_experts, work);
    GAMER_CHECK_LAUNCH("gamer_expert_lists/count");
    hipLaunchKernelGGL(expert_scan_kernel, dim3(1), dim3(1024), 0, st, B, num_experts, B * S, work, offsets);
    GAMER_CHECK_LAUNCH("gamer_expert_lists/scan");
    hipLaunchKernelGGL(expert_emit_kernel, dim3(B), dim3(num_experts < 64 ? 64 : 128), 0, st, expert, S, num_experts, work,
                       offsets, perm, slot);
    GAMER_CHECK_LAUNCH("gamer_expert_lists/emit");
    return 0;
}

extern "C" int gamer_router_position_table(int32_t* expert, int64_t n, const int32_t* table, int n_table, void* stream) {
    GAMER_CHECK_ARG(expert && table && n > 0 && n_table > 0 && n_table <= 4096,
                    "gamer_router_position_table: bad arguments n=%lld n_table=%d", (long long)n, n_table);
    int64_t blocks = (n + 256 * 4 - 1) / (256 * 4);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(position_table_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, expert, n, table, n_table);
    GAMER_CHECK_LAUNCH("gamer_router_position_table");
    return 0;
}

extern "C" int gamer_check_labels(const int64_t* labels, int64_t n, int V, int ignore_index, int32_t* bad_label,
                                  void* stream) {
    GAMER_CHECK_ARG(labels && bad_label && n > 0 && V > 0, "gamer_check_labels: bad arguments");
    int64_t blocks = (n + 256 * 8 - 1) / (256 * 8);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(check_labels_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, labels, n, V,
                       ignore_index, bad_label);
    GAMER_CHECK_LAUNCH("gamer_check_labels");
    return 0;
}

// ---- causal + key-padding mask and per-row RoPE positions (the Qwen3 baseline) ----------------------------------------
// HF Qwen3ForCausalLM's mask is causal plus key padding: allowed(i,j) = j <= i && attention_mask[j] != 0, i.e. the
// attention kernels' predicate with kl[j] = 0 / INT_MAX and query level 1.  generate() rotates row b's token i by
// cumsum(attention_mask[b])[i] - 1, 0 at pads (transformers/generation/utils.py, _prepare_position_ids_for_generation),
// and every generated token by one more: the first one by the number of kept prompt tokens.
// One workgroup per sequence; an inclusive prefix sum of the kept flags in LDS gives the positions and the empty rows
// (no kept key at or before the row).
__global__ void __launch_bounds__(ROUTER_THREADS)
causal_prep_kernel(const int64_t* __restrict__ attn_mask, int S, int32_t* __restrict__ kl_self,
                   int32_t* __restrict__ empty_self, int32_t* __restrict__ tile_empty_self,
                   int32_t* __restrict__ pos_ids, int32_t* __restrict__ next_pos) {
    extern __shared__ __attribute__((aligned(16))) int32_t cs[];
    int32_t* a = cs;            // [S] scan ping-pong
    int32_t* bb = cs + S;       // [S]
    const int b = blockIdx.x;
    const int64_t base = (int64_t)b * S;
    const int n_tiles = (S + 31) / 32;
    for (int t = threadIdx.x; t < S; t += blockDim.x) {
        const int keep = attn_mask ? (attn_mask[base + t] != 0 ? 1 : 0) : 1;
        kl_self[base + t] = keep ? 0 : INT_BIG;
        a[t] = keep;
    }
    __syncthreads();
    // inclusive prefix sum (Hillis-Steele)
    for (int off = 1; off < S; off <<= 1) {
        for (int t = threadIdx.x; t < S; t += blockDim.x) bb[t] = a[t] + (t >= off ? a[t - off] : 0);
        __syncthreads();
        int32_t* sw = a; a = bb; bb = sw;
    }
    for (int t = threadIdx.x; t < S; t += blockDim.x) {
        const int c = a[t];
        empty_self[base + t] = c == 0 ? 1 : 0;
        if (pos_ids) {
            const int keep = attn_mask ? (attn_mask[base + t] != 0 ? 1 : 0) : 1;
            pos_ids[base + t] = keep ? c - 1 : 0;
        }
    }
    for (int qt = threadIdx.x; qt < n_tiles; qt += blockDim.x) {
        // rows are empty exactly up to the first kept token: the tile has an empty row iff its first row is empty
        tile_empty_self[(int64_t)b * n_tiles + qt] = a[qt * 32] == 0 ? 1 : 0;
    }
    if (next_pos && threadIdx.x == 0) next_pos[b] = a[S - 1];
}

extern "C" int gamer_causal_prep(const int64_t* attn_mask, int B, int S, int32_t* kl_self, int32_t* empty_self,
                                 int32_t* tile_empty_self, int32_t* pos_ids, int32_t* next_pos, void* stream) {
    GAMER_CHECK_ARG(kl_self && empty_self && tile_empty_self, "gamer_causal_prep: null pointer");
    GAMER_CHECK_ARG(B > 0 && S > 0, "gamer_causal_prep: bad shape B=%d S=%d", B, S);
    GAMER_CHECK_ARG(S <= 8192, "gamer_causal_prep: S=%d > 8192 unsupported", S);
    const size_t shmem = (size_t)2 * S * sizeof(int32_t);
    hipLaunchKernelGGL(causal_prep_kernel, dim3(B), dim3(ROUTER_THREADS), shmem, (hipStream_t)stream,
                       attn_mask, S, kl_self, empty_self, tile_empty_self, pos_ids, next_pos);
    GAMER_CHECK_LAUNCH("gamer_causal_prep");
    return 0;
}

// ---- Qwen3Moe router + causal mask (one launch) -----------------------------------------------------------------------
// ref:SeqRec/models/generative/Qwen3Moe/router.py (Qwen3Multi's router without action indices) with the model's
// cache_position = arange(S) (model.py:222-230), and its causal + key-padding mask (model.py:310-460).  Per token t of row b:
//   expert[t]  = table[t % P] for t < n_items P, 0 for the trailing eos slot t = n_items P (router.py:28-60);
//                0 at pad / eos tokens.  table == NULL: t % P + 1 (the shipped table, and that of use_behavior_token = False)
//   beh_idx[t] = behaviour tokens (use_beh != 0): lut[ids[item start]] + 1, 0 on the behaviour token itself, at pad / eos and
//                in the eos slot (router.py:97-154); a non-special item start outside behavior_maps is counted in bad_token
//                (the reference fails in its embedding there) and gets 0.  use_beh == 0: 0 everywhere.
//   kl_self / empty_self / tile_empty_self / pos_ids / next_pos: as causal_prep_kernel.
// One workgroup per sequence; LDS holds the kept-flag prefix sum (2 S int32).
// Position expert ``e`` and behaviour index ``bi`` of token t of one row (``ids``: the row's); returns 1 for a non-special item
// start outside behavior_maps (the row's share of bad_token), else 0.
__device__ __forceinline__ int
moe_route_indices(const int64_t* __restrict__ ids, int t, const int32_t* __restrict__ lut, int vocab,
                  const int32_t* __restrict__ table, int P, int slots, int use_beh, int pad_id, int eos_id, int& e, int& bi) {
    const int64_t id = ids[t];
    const bool special = (id == pad_id) || (id == eos_id);
    const int p = t % P;
    e = 0;
    bi = 0;
    if (!special && t < slots) {
        e = table ? table[p] : p + 1;
        if (use_beh && p != 0) {
            const int64_t btok = ids[t - p];
            if (btok >= 0 && btok < vocab && lut[btok] >= 0) bi = lut[btok] + 1;
        }
    }
    return (use_beh && p == 0 && !special && t < slots && !(id >= 0 && id < vocab && lut[id] >= 0)) ? 1 : 0;
}

// expert[t] and beh_idx[t] of token t of one row (``expert`` / ``beh_idx``: the row's): Qwen3Moe's routing.
__device__ __forceinline__ int
moe_route_token(const int64_t* __restrict__ ids, int t, const int32_t* __restrict__ lut, int vocab,
                const int32_t* __restrict__ table, int P, int slots, int use_beh, int pad_id, int eos_id,
                int32_t* __restrict__ expert, int32_t* __restrict__ beh_idx) {
    int e, bi;
    const int bad = moe_route_indices(ids, t, lut, vocab, table, P, slots, use_beh, pad_id, eos_id, e, bi);
    expert[t] = e;
    beh_idx[t] = bi;
    return bad;
}

// Qwen3MoeAction's routing of token t (ref:SeqRec/models/generative/Qwen3Multi/router.py:154-199 with cache_position = arange(S),
// Qwen3MoeAction/FFN.py:43-44): the action index is lut[ids[item start]] + 1 on every token of the item, the behaviour token
// included; 0 at pad / eos, in the action table's own eos slot - column ((S + P - 2) / P) P, inside the sequence only as the
// last column of S = n P + 1 tokens -, in column ``act_zero_col`` (a generation's re-run: what the cache holds for the
// prompt's last column; -1: none), and for an item start outside behavior_maps.  expert[t] is the FFN's index
// max(0, pos_experts (action - 1) + position expert).
__device__ __forceinline__ int
moe_action_route_token(const int64_t* __restrict__ ids, int t, const int32_t* __restrict__ lut, int vocab,
                       const int32_t* __restrict__ table, int S, int P, int slots, int use_beh, int pad_id, int eos_id,
                       int pos_experts, int act_zero_col, int32_t* __restrict__ expert, int32_t* __restrict__ beh_idx,
                       int32_t* __restrict__ act_idx) {
    int e, bi;
    const int bad = moe_route_indices(ids, t, lut, vocab, table, P, slots, use_beh, pad_id, eos_id, e, bi);
    const int64_t id = ids[t];
    int act = 0;
    if (use_beh && id != pad_id && id != eos_id && t < slots && t != ((S + P - 2) / P) * P && t != act_zero_col) {
        const int64_t btok = ids[t - t % P];
        if (btok >= 0 && btok < vocab && lut[btok] >= 0) act = lut[btok] + 1;
    }
    const int idx = pos_experts * (act - 1) + e;
    expert[t] = idx < 0 ? 0 : idx;
    beh_idx[t] = bi;
    act_idx[t] = act;
    return bad;
}

// ACTION = true: Qwen3MoeAction (moe_action_route_token: ``expert`` is the FFN's index, ``act_idx`` is written); the mask half
// is the same code.
template <bool ACTION>
__global__ void __launch_bounds__(ROUTER_THREADS)
moe_router_prep_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ attn_mask,
                       const int32_t* __restrict__ lut, int vocab, const int32_t* __restrict__ table, int S, int P,
                       int n_items, int use_beh, int pad_id, int eos_id, int pos_experts, int act_zero_col,
                       int32_t* __restrict__ expert, int32_t* __restrict__ beh_idx, int32_t* __restrict__ act_idx,
                       int32_t* __restrict__ kl_self,
                       int32_t* __restrict__ empty_self, int32_t* __restrict__ tile_empty_self,
                       int32_t* __restrict__ pos_ids, int32_t* __restrict__ next_pos, int32_t* __restrict__ bad_token) {
    extern __shared__ __attribute__((aligned(16))) int32_t ms[];
    int32_t* a = ms;            // [S] scan ping-pong
    int32_t* bb = ms + S;       // [S]
    const int b = blockIdx.x;
    const int64_t base = (int64_t)b * S;
    const int n_tiles = (S + 31) / 32;
    const int slots = n_items * P;
    int bad = 0;
    for (int t = threadIdx.x; t < S; t += blockDim.x) {
        if (ACTION)
            bad += moe_action_route_token(ids + base, t, lut, vocab, table, S, P, slots, use_beh, pad_id, eos_id, pos_experts,
                                          act_zero_col, expert + base, beh_idx + base, act_idx + base);
        else
            bad += moe_route_token(ids + base, t, lut, vocab, table, P, slots, use_beh, pad_id, eos_id, expert + base, beh_idx + base);
        const int keep = attn_mask ? (attn_mask[base + t] != 0 ? 1 : 0) : 1;
        kl_self[base + t] = keep ? 0 : INT_BIG;
        a[t] = keep;
    }
    if (bad) atomicAdd(bad_token, bad);
    __syncthreads();
    for (int off = 1; off < S; off <<= 1) {
        for (int t = threadIdx.x; t < S; t += blockDim.x) bb[t] = a[t] + (t >= off ? a[t - off] : 0);
        __syncthreads();
        int32_t* sw = a; a = bb; bb = sw;
    }
    for (int t = threadIdx.x; t < S; t += blockDim.x) {
        const int c = a[t];
        empty_self[base + t] = c == 0 ? 1 : 0;
        if (pos_ids) {
            const int keep = attn_mask ? (attn_mask[base + t] != 0 ? 1 : 0) : 1;
            pos_ids[base + t] = keep ? c - 1 : 0;
        }
    }
    for (int qt = threadIdx.x; qt < n_tiles; qt += blockDim.x)
        tile_empty_self[(int64_t)b * n_tiles + qt] = a[qt * 32] == 0 ? 1 : 0;
    if (next_pos && threadIdx.x == 0) next_pos[b] = a[S - 1];
}

extern "C" int gamer_moe_router_prep(const int64_t* ids, const int64_t* attn_mask, const int32_t* behavior_lut, int vocab,
                                     const int32_t* position_table, int B, int S, int num_positions, int n_items,
                                     int use_behavior_token, int pad_id, int eos_id, int32_t* expert, int32_t* beh_idx,
                                     int32_t* kl_self, int32_t* empty_self, int32_t* tile_empty_self, int32_t* pos_ids,
                                     int32_t* next_pos, int32_t* bad_token, void* stream) {
    GAMER_CHECK_ARG(ids && expert && beh_idx && kl_self && empty_self && tile_empty_self && bad_token,
                    "gamer_moe_router_prep: null pointer");
    GAMER_CHECK_ARG(!use_behavior_token || (behavior_lut && vocab > 0),
                    "gamer_moe_router_prep: use_behavior_token needs the behaviour table");
    GAMER_CHECK_ARG(B > 0 && S > 0 && num_positions > 0 && n_items > 0,
                    "gamer_moe_router_prep: bad shape B=%d S=%d P=%d n_items=%d", B, S, num_positions, n_items);
    GAMER_CHECK_ARG(S <= 8192, "gamer_moe_router_prep: S=%d > 8192 unsupported", S);
    GAMER_CHECK_ARG((int64_t)n_items * num_positions + 1 >= S,
                    "gamer_moe_router_prep: S=%d is longer than the router's table (n_items * P + 1 = %lld)", S,
                    (long long)n_items * num_positions + 1);
    const size_t shmem = (size_t)2 * S * sizeof(int32_t);
    hipLaunchKernelGGL(moe_router_prep_kernel<false>, dim3(B), dim3(ROUTER_THREADS), shmem, (hipStream_t)stream,
                       ids, attn_mask, behavior_lut, vocab, position_table, S, num_positions, n_items,
                       use_behavior_token ? 1 : 0, pad_id, eos_id, 0, -1, expert, beh_idx, nullptr, kl_self, empty_self,
                       tile_empty_self, pos_ids, next_pos, bad_token);
    GAMER_CHECK_LAUNCH("gamer_moe_router_prep");
    return 0;
}

// ---- Qwen3MoeAction router + causal mask (one launch) -----------------------------------------------------------------
// gamer_moe_router_prep with the action index and the (action, position) FFN index of moe_action_route_token.
extern "C" int gamer_moe_action_router_prep(const int64_t* ids, const int64_t* attn_mask, const int32_t* behavior_lut, int vocab,
                                            const int32_t* position_table, int B, int S, int num_positions, int n_items,
                                            int use_behavior_token, int pad_id, int eos_id, int num_position_experts,
                                            int act_zero_col, int32_t* expert, int32_t* beh_idx, int32_t* act_idx,
                                            int32_t* kl_self, int32_t* empty_self, int32_t* tile_empty_self, int32_t* pos_ids,
                                            int32_t* next_pos, int32_t* bad_token, void* stream) {
    GAMER_CHECK_ARG(ids && expert && beh_idx && act_idx && kl_self && empty_self && tile_empty_self && bad_token,
                    "gamer_moe_action_router_prep: null pointer");
    GAMER_CHECK_ARG(!use_behavior_token || (behavior_lut && vocab > 0),
                    "gamer_moe_action_router_prep: use_behavior_token needs the behaviour table");
    GAMER_CHECK_ARG(B > 0 && S > 0 && num_positions > 0 && n_items > 0 && num_position_experts > 0,
                    "gamer_moe_action_router_prep: bad shape B=%d S=%d P=%d n_items=%d position experts=%d", B, S,
                    num_positions, n_items, num_position_experts);
    GAMER_CHECK_ARG(act_zero_col >= -1 && act_zero_col < S, "gamer_moe_action_router_prep: act_zero_col=%d outside [-1, S=%d)",
                    act_zero_col, S);
    GAMER_CHECK_ARG(S <= 8192, "gamer_moe_action_router_prep: S=%d > 8192 unsupported", S);
    GAMER_CHECK_ARG((int64_t)n_items * num_positions + 1 >= S,
                    "gamer_moe_action_router_prep: S=%d is longer than the router's table (n_items * P + 1 = %lld)", S,
                    (long long)n_items * num_positions + 1);
    const size_t shmem = (size_t)2 * S * sizeof(int32_t);
    hipLaunchKernelGGL(moe_router_prep_kernel<true>, dim3(B), dim3(ROUTER_THREADS), shmem, (hipStream_t)stream,
                       ids, attn_mask, behavior_lut, vocab, position_table, S, num_positions, n_items,
                       use_behavior_token ? 1 : 0, pad_id, eos_id, num_position_experts, act_zero_col, expert, beh_idx, act_idx,
                       kl_self, empty_self, tile_empty_self, pos_ids, next_pos, bad_token);
    GAMER_CHECK_LAUNCH("gamer_moe_action_router_prep");
    return 0;
}

// ---- Qwen3SessionMoe: Qwen3Moe's router + Qwen3Session's mask (one launch) ---------------------------------------------
// ref:SeqRec/models/generative/Qwen3SessionMoe/model.py: the layers and router of Qwen3Moe (:23-93) under the self mask and
// RoPE positions of Qwen3Session (:402-468, :680-703).  One workgroup per sequence: moe_route_token per token (expert, beh_idx,
// bad_token as moe_router_prep_kernel), then session_spans_row<false> (kl_self, span_self, pos_ids, empty flags, violations as
// gamer_session_prep's kernel).  The two halves share no output, so no barrier stands between them.
__global__ void __launch_bounds__(ROUTER_THREADS)
session_moe_prep_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ attn_mask,
                        const int64_t* __restrict__ sess, const int64_t* __restrict__ ext_ids,
                        const int32_t* __restrict__ lut, int vocab, const int32_t* __restrict__ table, int S, int P,
                        int n_items, int use_beh, int pad_id, int eos_id, int n_pos,
                        int32_t* __restrict__ expert, int32_t* __restrict__ beh_idx, int32_t* __restrict__ bad_token,
                        int32_t* __restrict__ kl_self, int32_t* __restrict__ span_self, int32_t* __restrict__ pos_ids,
                        int32_t* __restrict__ empty_self, int32_t* __restrict__ tile_empty_self,
                        int32_t* __restrict__ violations) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sraw[];
    const int64_t base = (int64_t)blockIdx.x * S;
    const int slots = n_items * P;
    int bad = 0;
    for (int t = threadIdx.x; t < S; t += blockDim.x)
        bad += moe_route_token(ids + base, t, lut, vocab, table, P, slots, use_beh, pad_id, eos_id, expert + base, beh_idx + base);
    if (bad) atomicAdd(bad_token, bad);
    session_spans_row<false>(sraw, sess, ext_ids, attn_mask, nullptr, nullptr, S, P, n_pos, kl_self, span_self, nullptr, pos_ids,
                             empty_self, nullptr, tile_empty_self, nullptr, violations);
}

extern "C" int gamer_session_moe_prep(const int64_t* ids, const int64_t* attn_mask, const int64_t* session_ids,
                                      const int64_t* extended_session_ids, const int32_t* behavior_lut, int vocab,
                                      const int32_t* position_table, int B, int S, int num_positions, int n_items,
                                      int use_behavior_token, int pad_id, int eos_id, int n_rope_positions,
                                      int32_t* expert, int32_t* beh_idx, int32_t* bad_token, int32_t* kl_self,
                                      int32_t* span_self, int32_t* pos_ids, int32_t* empty_self, int32_t* tile_empty_self,
                                      int32_t* violations, void* stream) {
    GAMER_CHECK_ARG(ids && session_ids && expert && beh_idx && bad_token && kl_self && span_self && pos_ids && empty_self &&
                    tile_empty_self && violations, "gamer_session_moe_prep: null pointer");
    GAMER_CHECK_ARG(!use_behavior_token || (behavior_lut && vocab > 0),
                    "gamer_session_moe_prep: use_behavior_token needs the behaviour table");
    GAMER_CHECK_ARG(B > 0 && S > 0 && num_positions > 0 && n_items > 0 && n_rope_positions > 0,
                    "gamer_session_moe_prep: bad shape B=%d S=%d P=%d n_items=%d n_pos=%d", B, S, num_positions, n_items,
                    n_rope_positions);
    GAMER_CHECK_ARG(S <= 2048, "gamer_session_moe_prep: S=%d > 2048 unsupported", S);
    GAMER_CHECK_ARG((int64_t)n_items * num_positions + 1 >= S,
                    "gamer_session_moe_prep: S=%d is longer than the router's table (n_items * P + 1 = %lld)", S,
                    (long long)n_items * num_positions + 1);
    hipLaunchKernelGGL(session_moe_prep_kernel, dim3(B), dim3(ROUTER_THREADS), session_span_lds<false>(S), (hipStream_t)stream,
                       ids, attn_mask, session_ids, extended_session_ids, behavior_lut, vocab, position_table, S,
                       num_positions, n_items, use_behavior_token ? 1 : 0, pad_id, eos_id, n_rope_positions, expert, beh_idx,
                       bad_token, kl_self, span_self, pos_ids, empty_self, tile_empty_self, violations);
    GAMER_CHECK_LAUNCH("gamer_session_moe_prep");
    return 0;
}
