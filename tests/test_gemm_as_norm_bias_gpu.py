"""RMSNorm as the prologue and the cross block's behaviour biases as the epilogue of the activation-stationary Linear forward
(csrc/gemm_as.hip; gamer_gemm_desc.norm_x / .bias_idx): the norms in front of the q|k|v projections, the experts' gate|up projection and
the tied head, and the bias rows qknorm_rope_fwd used to add in place (ref:SeqRec/models/generative/Qwen3Multi/model.py:93-99, 204,
220, 238, 869).  References: fp64 for the norm and the product, the separate launches for everything that has to keep its bits."""
import ctypes
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gamer_amd import _lib, ops, synthetic  # noqa: E402
from gamer_amd.config import synthetic_config  # noqa: E402

DEV = "cuda"
NAN = float("nan")
EPS = 1e-6
_env = ops.env_switches


def _launches():
    """(all launches of the activation-stationary kernel, those with a norm prologue / bias epilogue) by this process so far"""
    lib = _lib.load()
    out = []
    for name in ("gamer_debug_gemm_as_launches", "gamer_debug_gemm_as_fused_launches"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = ctypes.c_longlong, []
        out.append(int(fn()))
    return out


def _param_cache(flat, everything=False):
    cache = ops.amax_reuse(everything=everything)
    cache.stable_range(flat.data_ptr(), flat.numel() * 4)
    cache.planes = torch.zeros(flat.numel(), dtype=torch.float32, device=DEV)
    return cache


def _weights(rows, K, seed, scale=0.05):
    g = torch.Generator().manual_seed(seed)
    flat = (torch.randn(rows * K + 8, generator=g) * scale).to(DEV)
    return flat, flat[:rows * K].view(rows, K)


def _rms64(x, w):
    xd = x.double().cpu()
    return xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + EPS) * w.double().cpu()


def _slot_value(ptr_):
    from test_ops_gpu import _slot_value as sv
    return sv(ptr_)


def _norm_inputs(M, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) * 2
    zero_row = big_row = None
    if M >= 8:
        zero_row, big_row = 5, 7
        x[zero_row] = 0                                  # rstd = 1 / sqrt(eps), h = 0
        x[big_row] *= 2.0 ** 30                          # 2^30 times the others: its squares are 2^60 times theirs
    w = 1 + 0.1 * torch.randn(K, generator=g)
    return x.to(DEV), w.to(DEV), zero_row, big_row


# ---- 1. the norm prologue against fp64, and its product against a plain launch on the h it stored ---------------------------------
@pytest.mark.parametrize("K", [64, 128, 192, 256])
@pytest.mark.parametrize("N,ldc", [(32, 32), (100, 128), (768, 768), (1041, 1056)])
def test_norm_prologue_against_fp64_and_a_plain_launch_on_its_h(N, ldc, K):
    """M = 1 (one live lane), 33 (a second wave with one row), 517, 1000 (ragged last workgroups); every K the kernel instantiates; N
    with partial slabs and a padded C; h with row stride K and K + 64 over NaN (the padding stays NaN); one all-zero row and one row
    2^30 times the others.  Bars: h as tests/test_rowwise_paths_gpu.py::test_rmsnorm_on_both_instantiations (2e-6 of the largest
    value), C as tests/test_gemm_as_gpu.py::test_gemm_as_against_fp64_and_the_tile_kernel (1e-6 max, 6e-8 rms of sum |a| |w|) against
    the fp64 product of the fp64-normalised rows.  Exact: C has the bits of a plain launch on the stored h, and the published maximum is
    max |h|."""
    flat, W = _weights(N, K, seed=N + K)
    cache = _param_cache(flat)
    for M in (1, 33, 517, 1000):
        x, wn, zero_row, big_row = _norm_inputs(M, K, seed=1000 * K + M)
        href = _rms64(x, wn)
        wd = W.double().cpu()
        ref, sc = href @ wd.T, href.abs() @ wd.abs().T
        for ldh in (K, K + 64):
            where = f"M={M} N={N} K={K} ldh={ldh}"
            n0 = _launches()
            with _env(GAMER_GEMM_AS=1, GAMER_GEMM_AS_MIN_M=1), ops.f32_matmul("split3"), cache:
                for _ in range(2):                       # (the packed weight pieces exist from the second pass on)
                    cache.reset()
                    y = torch.full((M, ldc), NAN, device=DEV)
                    h = torch.full((M, ldh), NAN, device=DEV)
                    with cache.hold(h):
                        ops.linear_fwd(h, ldh, W, K, y, ldc, M, N, K, norm=dict(x=x, w=wn, eps=EPS))
                        key = cache._key(h.data_ptr(), (1, 0, M, K, ldh))
                        assert key in cache.slots, "the call did not leave a slot for max |h|"
                        torch.cuda.synchronize()
                        published = _slot_value(cache.slots[key])
                y_plain = torch.full((M, ldc), NAN, device=DEV)
                ops.linear_fwd(h, ldh, W, K, y_plain, ldc, M, N, K)
                torch.cuda.synchronize()
            n1 = _launches()
            # (every pass that has the packed pieces runs fused - the very first pass of the cache does not -, then the one plain launch)
            assert n1[1] - n0[1] in (1, 2) and (n1[0] - n0[0]) - (n1[1] - n0[1]) == 1, (where, n0, n1)
            hc = h.cpu()
            e_h = float((hc[:, :K].double() - href).abs().max() / href.abs().max().clamp_min(1e-30))
            e = (y[:, :N].double().cpu() - ref).abs() / sc.clamp_min(1e-300)
            e_max, e_rms = float(e.max()), float(e.pow(2).mean().sqrt())
            print(f"{where}: h {e_h:.3g}  C max {e_max:.3g} rms {e_rms:.3g}")
            assert e_h < 2e-6, (where, e_h)
            if ldh > K:
                assert torch.isnan(hc[:, K:]).all(), where
            if ldc > N:
                assert torch.isnan(y[:, N:]).all(), where
            if zero_row is not None:
                assert bool((hc[zero_row, :K] == 0).all()) and bool((y[zero_row, :N] == 0).all()), where
                assert torch.isfinite(hc[big_row, :K]).all(), where
            assert e_max < 1e-6 and e_rms < 6e-8, (where, e_max, e_rms)
            assert torch.equal(y[:, :N], y_plain[:, :N]), where
            assert published == float(hc[:, :K].abs().max()), (where, published)


# ---- 2. the grouped form with the row map (the experts' gate|up projection) --------------------------------------------------------
@pytest.mark.parametrize("p_drop", [0.0, 0.2])
@pytest.mark.parametrize("table", [False, True])
def test_norm_prologue_grouped_with_the_row_map(table, p_drop):
    """Six row groups - an empty one, one of 5 rows, one of 128 + 37 - whose rows are a random permutation of the tokens: the launch reads
    token perm[m] for sorted row m and leaves h in sorted order.  Plain store and SwiGLU-forward epilogue (row table and dropout on and
    off): gate|up and hm are the bits of the same launch without the norm on that h."""
    K, I, G = 256, 64, 6
    N = 2 * I
    sizes = [40, 0, 5, 128 + 37, 90, 63]
    T = sum(sizes)
    offs = torch.tensor([0] + torch.tensor(sizes).cumsum(0).tolist(), dtype=torch.int32, device=DEV)
    div = 2 if table else 1
    flat, W = _weights((G // div) * N, K, seed=31 + int(table))
    g = torch.Generator().manual_seed(5)
    x, wn, _, _ = _norm_inputs(T, K, seed=77)
    perm = torch.randperm(T, generator=g).to(torch.int32)                # sorted row -> token
    slot = torch.empty(T, dtype=torch.int32)
    slot[perm.long()] = torch.arange(T, dtype=torch.int32)               # token -> sorted row
    perm_d, slot_d = perm.to(DEV), slot.to(DEV)
    tbl = torch.randn(G, N, generator=g).to(DEV) if table else None
    row_group = torch.cat([torch.full((s,), i, dtype=torch.int32) for i, s in enumerate(sizes)]).to(DEV) if table else None
    grp = dict(strideB=N * K, groups=G, group_offsets=offs, group_div=div if table else 0)
    nrm = dict(x=x, w=wn, eps=EPS, dst_rows=slot_d, src_rows=perm_d)
    cache = _param_cache(flat)
    href = _rms64(x, wn)[perm.long()]
    n0 = _launches()
    with _env(GAMER_GEMM_AS=1, GAMER_GEMM_AS_MIN_M=1), ops.f32_matmul("split3"), cache:
        for _ in range(2):
            cache.reset()
            h = torch.full((T, K), NAN, device=DEV)
            gu, hm = torch.full((T, N), NAN, device=DEV), torch.full((T, I), NAN, device=DEV)
            ops.gemm(h, K, 1, W, K, 1, gu, N, T, N, K, p_drop=p_drop, seed=77, swiglu_fwd=(hm, tbl, row_group), norm=nrm, **grp)
        n1 = _launches()
        gu2, hm2 = torch.full((T, N), NAN, device=DEV), torch.full((T, I), NAN, device=DEV)
        ops.gemm(h, K, 1, W, K, 1, gu2, N, T, N, K, p_drop=p_drop, seed=77, swiglu_fwd=(hm2, tbl, row_group), **grp)
        n2 = _launches()
        out = {}
        if not table:
            # the plain store, grouped (the projection when the SwiGLU forward runs on its own)
            h3, y3, y4 = torch.full((T, K), NAN, device=DEV), torch.full((T, N), NAN, device=DEV), torch.full((T, N), NAN, device=DEV)
            ops.linear_fwd(h3, K, W, K, y3, N, T, N, K, norm=nrm, **grp)
            ops.linear_fwd(h3, K, W, K, y4, N, T, N, K, **grp)
            out = dict(h3=h3, y3=y3, y4=y4)
        torch.cuda.synchronize()
    assert n1[1] - n0[1] == 1, (n0, n1)
    assert n2[0] - n1[0] == 1 and n2[1] == n1[1], (n1, n2)
    e_h = float((h.double().cpu() - href).abs().max() / href.abs().max())
    print(f"table={table} p={p_drop}: h {e_h:.3g}")
    assert e_h < 2e-6
    assert torch.equal(gu, gu2) and torch.equal(hm, hm2)
    assert torch.isfinite(hm).all()
    if out:
        assert torch.equal(out["h3"], h) and torch.equal(out["y3"], out["y4"]) and torch.equal(out["y3"], gu)


# ---- 3. the bias epilogue ----------------------------------------------------------------------------------------------------------
def _bias_inputs(M, seed=3):
    H, nq, nkv, NB1 = 256, 6, 3, 4
    S = 10 if M % 10 == 0 else 1                         # (qknorm_rope_fwd takes whole sequences)
    g = torch.Generator().manual_seed(seed + M)
    x = torch.randn(M, H, generator=g).to(DEV)
    idx = torch.randint(0, NB1, (M,), generator=g)
    if M >= NB1:
        idx[:NB1] = torch.arange(NB1)                    # every row of the tables is used
    tabs = [torch.randn(NB1, n * 64, generator=g).to(DEV) * 0.5 for n in (nq, nkv, nkv)]
    wq, wk = (1 + 0.1 * torch.randn(64, generator=g)).to(DEV), (1 + 0.1 * torch.randn(64, generator=g)).to(DEV)
    ang = torch.rand(S, 32, generator=g) * 6.28
    cos, sin = torch.cat([ang.cos(), ang.cos()], 1).to(DEV).contiguous(), torch.cat([ang.sin(), ang.sin()], 1).to(DEV).contiguous()
    return H, nq, nkv, S, x, idx.to(torch.int32).to(DEV), tabs, wq, wk, cos, sin


def _qkv_call(cache, fused, M, W, inp, env=None, passes=2, mode="split3"):
    """The cross block's q|k|v projection + q/k-norm + RoPE: `fused` = the biases in the GEMM's descriptor and a bias-free
    qknorm_rope_fwd, else today's linear_fwd + biased qknorm_rope_fwd.  Returns q|k|v, q_rot, k_rot and the slot value of max |v|."""
    H, nq, nkv, S, x, idx, (bq, bk, bv), wq, wk, cos, sin = inp
    QKV, col0 = (nq + 2 * nkv) * 64, (nq + nkv) * 64
    env = dict(GAMER_GEMM_AS=1, **(dict(GAMER_GEMM_AS_MIN_M=1) if env is None else env))
    with _env(**env), ops.f32_matmul(mode), cache:
        for _ in range(passes):
            cache.reset()
            qkv =torch.full((M, QKV), NAN, device=DEV)
            q_rot, k_rot = torch.full((M, nq * 64), NAN, device=DEV), torch.full((M, nkv * 64), NAN, device=DEV)
            v = qkv[:, col0:]
            if fused:
                ops.linear_fwd(x, H, W, H, qkv, QKV, M, QKV, H, bias=dict(idx=idx, q=bq, k=bk, v=bv), c_amax=(v, col0))
                ops.qknorm_rope_fwd(qkv, S, nq, nkv, wq, wk, EPS, cos, sin, q_rot, k_rot)
            else:
                ops.linear_fwd(x, H, W, H, qkv, QKV, M, QKV, H)
                ops.qknorm_rope_fwd(qkv, S, nq, nkv, wq, wk, EPS, cos, sin, q_rot, k_rot, bias_q=bq, bias_k=bk, bias_v=bv, act_idx=idx)
        smax = None
        if mode == "split3":
            key = cache._key(v.data_ptr(), (1, 0, M, nkv * 64, QKV))
            assert key in cache.pending, "no producer opened a slot for max |v|"
            torch.cuda.synchronize()
            smax = _slot_value(cache.pending[key])
        torch.cuda.synchronize()
    return qkv, q_rot, k_rot, smax


@pytest.mark.parametrize("M", [1, 130, 1000])
def test_bias_epilogue_has_the_bits_of_the_in_place_add(M):
    """N = 768 = 384 | 192 | 192, four table rows: q|k|v leaves the GEMM with the bits linear_fwd + the biased qknorm_rope_fwd leave in
    place, the bias-free q/k-norm + RoPE on it returns the same q_rot / k_rot, and the reported maximum of the v columns is today's."""
    inp = _bias_inputs(M)
    flat, W = _weights(768, 256, seed=9, scale=0.3)
    cache = _param_cache(flat)
    n0 = _launches()
    qkv_f, q_f, k_f, s_f = _qkv_call(cache, True, M, W, inp)
    n1 = _launches()
    qkv_r, q_r, k_r, s_r = _qkv_call(cache, False, M, W, inp)
    n2 = _launches()
    assert n1[1] - n0[1] == 1 and n2[1] == n1[1] and n2[0] - n1[0] >= 1, (n0, n1, n2)
    assert torch.equal(qkv_f, qkv_r)
    assert torch.equal(q_f, q_r) and torch.equal(k_f, k_r)
    assert s_f == s_r == float(qkv_r[:, 576:].abs().max())
    # (and the biases are really there)
    bq = inp[6][0]
    plain = inp[4].double().cpu() @ W.double().cpu().T
    want = plain[:, :384] + bq.double().cpu()[inp[5].long().cpu()]
    assert float((qkv_f[:, :384].double().cpu() - want).abs().max()) < 2e-6 * float(want.abs().max())


# ---- 4. every fallback returns the bits of the separate launches ---------------------------------------------------------------------
def _norm_call(cache, fused, M, K, N, W, x, wn, env=None, passes=2, mode="split3"):
    env = dict(GAMER_GEMM_AS=1, **(dict(GAMER_GEMM_AS_MIN_M=1) if env is None else env))
    with _env(**env), ops.f32_matmul(mode), cache:
        for _ in range(passes):
            cache.reset()
            h, y = torch.full((M, K), NAN, device=DEV), torch.full((M, N), NAN, device=DEV)
            if fused:
                ops.linear_fwd(h, K, W, K, y, N, M, N, K, norm=dict(x=x, w=wn, eps=EPS))
            else:
                ops.rmsnorm_fwd(x, wn, EPS, h)
                ops.linear_fwd(h, K, W, K, y, N, M, N, K)
        torch.cuda.synchronize()
    return h, y


@pytest.mark.parametrize("case", ["first_pass", "few_rows", "split6", "f32", "K320", "switch_off"])
def test_fallbacks_return_the_bits_of_the_separate_launches(case):
    """A call that carries a norm or a bias and is not taken by the activation-stationary kernel - no packed pieces yet (first pass of a
    cache), M below the bar, another product form, K = 320 (the injecting layers' concatenated input), its switch off - runs as
    gamer_rmsnorm_fwd / the plain product / the bias pass inside the library: the bits of those launches made by the caller, and
    gamer_debug_gemm_as_fused_launches does not move."""
    M, N = 300, 768
    K = 320 if case == "K320" else 256
    low_bar = dict(GAMER_GEMM_AS_MIN_M=1)
    env_n, env_b, passes, mode = dict(low_bar), dict(low_bar), 2, "split3"
    if case == "first_pass":
        passes = 1
    elif case == "few_rows":
        env_n, env_b = {}, {}                            # production bar: 16 k rows
    elif case in ("split6", "f32"):
        mode = case
    elif case == "switch_off":
        env_n, env_b = dict(low_bar, GAMER_GEMM_AS_NORM=0), dict(low_bar, GAMER_GEMM_AS_BIAS=0)
    flat, W = _weights(N, K, seed=2)
    x, wn, _, _ = _norm_inputs(M, K, seed=4)
    n0 = _launches()
    h_f, y_f = _norm_call(_param_cache(flat), True, M, K, N, W, x, wn, env_n, passes, mode)
    h_r, y_r = _norm_call(_param_cache(flat), False, M, K, N, W, x, wn, env_n, passes, mode)
    assert torch.equal(h_f, h_r) and torch.equal(y_f, y_r), case
    if K == 256:
        inp = _bias_inputs(M)
        qkv_f, q_f, k_f, s_f = _qkv_call(_param_cache(flat), True, M, W, inp, env_b, passes, mode)
        qkv_r, q_r, k_r, s_r = _qkv_call(_param_cache(flat), False, M, W, inp, env_b, passes, mode)
        assert torch.equal(qkv_f, qkv_r) and torch.equal(q_f, q_r) and torch.equal(k_f, k_r), case
        assert s_f == s_r, case
    n1 = _launches()
    assert n1[1] == n0[1], (case, n0, n1)
    if case == "switch_off":
        assert n1[0] > n0[0]                             # (the plain activation-stationary launch took the products)
        # ... and with the switches on the same calls are taken
        _norm_call(_param_cache(flat), True, M, K, N, W, x, wn, low_bar)
        _qkv_call(_param_cache(flat), True, M, W, _bias_inputs(M), low_bar)
        assert _launches()[1] == n1[1] + 2


# ---- 5. a two-layer engine, switches on and off --------------------------------------------------------------------------------------
def _engine_run(cfg, sd, batch, on):
    from gamer_amd.engine import Engine
    eng = Engine(cfg, temperature=0.7, matmul="split3")
    eng.load_state_dict(sd)
    eng.base_seed = 5
    n0 = _launches()
    with _env(GAMER_GEMM_AS_MIN_M=1, GAMER_GEMM_OS_MIN_M=1, GAMER_GEMM_AS_NORM=int(on), GAMER_GEMM_AS_BIAS=int(on)):
        for _ in range(2):                                   # (second pass: the packed weight pieces exist)
            eng.dropout_step = 0
            loss, _ = eng.forward(batch["input_ids"], batch["attention_mask"], batch["actions"], labels=batch["labels"],
                                  train=True, dropout=True)
            eng.zero_grad()
            eng.backward(1.0)
        torch.cuda.synchronize()
    return float(loss), {k: v.clone() for k, v in eng.grads.items()}, _launches()[1] - n0[1]


def test_engine_with_the_fused_norm_and_bias_matches_the_separate_launches():
    """Hidden size 64 (K = 64 is an instantiated shape), two layers - the second with behaviour injection and the cross block -,
    B = 4, S = 10, dropout on, split3: the step with GAMER_GEMM_AS_NORM / _BIAS on against off, same weights, batch and dropout seeds.
    Bars: those tests/test_model_gpu.py holds the split3 engine to against the reference - loss 1e-5 relative, every gradient tensor
    1e-3 of its largest entry, the global gradient norm 1e-4 - and every run repeats itself bit for bit."""
    from oracle import qwen3multi_oracle as orc
    cfg = synthetic_config(hidden_size=64, moe_intermediate_size=64, intermediate_size=128, num_attention_heads=2,
                           num_key_value_heads=1, num_hidden_layers=2, behavior_injection_decoder=[1], cross_attention_decoder=[1])
    sd = orc.init_state_dict(orc.OracleConfig.from_dict(cfg.to_dict()), seed=4)
    batch = synthetic.make_batch(4, 2, 256, 3, seed=9, behavior_probs=[0.5, 0.3, 0.2])
    assert batch["input_ids"].shape == (4, 10)
    l_on, g_on, fused_on = _engine_run(cfg, sd, batch, True)
    l_on2, g_on2, _ = _engine_run(cfg, sd, batch, True)
    l_off, g_off, fused_off = _engine_run(cfg, sd, batch, False)
    l_off2, g_off2, _ = _engine_run(cfg, sd, batch, False)
    assert fused_on > 0 and fused_off == 0, (fused_on, fused_off)
    assert l_on == l_on2 and l_off == l_off2
    for k in g_on:
        assert torch.equal(g_on[k], g_on2[k]) and torch.equal(g_off[k], g_off2[k]), k
    worst = max((float((g_on[k] - g_off[k]).abs().max()) / max(float(g_off[k].abs().max()), 1e-20), k) for k in g_on)
    gn_on = float(torch.sqrt(sum((g.double() ** 2).sum() for g in g_on.values())))
    gn_off = float(torch.sqrt(sum((g.double() ** 2).sum() for g in g_off.values())))
    print(f"loss {l_on} / {l_off}  worst gradient {worst}  global norm {gn_on} / {gn_off}")
    assert abs(l_on - l_off) < 1e-5 * abs(l_off)
    assert worst[0] < 1e-3, worst
    assert abs(gn_on - gn_off) < 1e-4 * gn_off
