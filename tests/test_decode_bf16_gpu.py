"""Generation on the bf16 engine: gamer_attn_decode_bf16, the bf16 DecodeSession and the trie-constrained beam search over it.

Weights and prompts are those of tests/golden/decode_small.npz; its fp32 expected beams are NOT used: the bf16 attention gives 0
for a row without an allowed key where the fp32 one gives a uniform average (csrc/attention_bf16.hip), and bf16 rounding moves
near-ties, so "the same beams as a reference" is not a property this search can be held to.  The chain that anchors it instead:
the reference under autocast -> the bf16 scoring forward (tests/test_bf16_gpu.py::test_model_bf16_against_reference_autocast_fixture)
-> the cached step (here, teacher forced) -> the search (here: every pruning decision justified by the scoring forward).

ERROR BAR, the project's own: two implementations of this bf16 arithmetic agree on the logits within delta = 1e-2 * max |logits|
(tests/test_bf16_gpu.py::test_model_bf16_against_reference_autocast_fixture; 4e-3 measured).  A log-probability (logit - logsumexp)
then moves by at most eps = 2 delta.  max |logits| is that of the scoring forward's rows a test compares against.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

from gamer_amd import synthetic
from gamer_amd.decode import ItemTrie
from oracle import qwen3multi_oracle as orc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from beam_trace_check import check_trace  # noqa: E402

FX = os.path.join(os.path.dirname(__file__), "golden", "decode_small.npz")
BF = torch.bfloat16


# ---- the helper alone (CPU): an exact synthetic scorer ---------------------------------------------------------------------
def _synthetic_search(items, first, B, nb, steps, scorer):
    """A plain host beam search over ``scorer`` with the product's slot conventions (dead slots at about -1e9)."""
    trie = ItemTrie(items, device="cpu")
    prefixes = torch.zeros(B, 1, 0, dtype=torch.int64)
    prev = torch.zeros(B, 1, dtype=torch.float64)
    trace = []
    for s in range(steps):
        logp = scorer(s, prefixes)
        parent, token, score = (torch.zeros(B, nb, dtype=torch.int64), torch.zeros(B, nb, dtype=torch.int64),
                                torch.full((B, nb), -1e9, dtype=torch.float64))
        for b in range(B):
            cand = [(float(prev[b, i]) + float(logp[b, i, t]), i, t) for i in range(prefixes.shape[1]) if float(prev[b, i]) > -1e8
                    for t in trie.get([first] + prefixes[b, i].tolist())]
            cand.sort(key=lambda c: -c[0])
            for j, (v, i, t) in enumerate(cand[:nb]):
                parent[b, j], token[b, j], score[b, j] = i, t, v
        trace.append((parent, token, score.to(torch.float32)))
        prefixes = torch.cat([torch.gather(prefixes, 1, parent.clamp(0, prefixes.shape[1] - 1)[:, :, None].expand(B, nb, s)),
                              token[:, :, None]], 2)
        prev = score.to(torch.float32).double()
    return trie, trace, (trace[-1][2] / steps).reshape(-1)


def test_beam_trace_check_accepts_a_valid_trace_and_rejects_an_unjustified_pruning():
    B, nb, steps, V, first = 2, 3, 4, 40, 39
    g = torch.Generator().manual_seed(0)
    codes = torch.unique(torch.randint(0, 4, (30, 4), generator=g), dim=0)
    items = [[first] + [8 * l + int(c) for l, c in enumerate(row)] for row in codes]
    table = {}

    def scorer(step, prefixes):                          # exact: a fixed pseudo-random distribution per (user, prefix)
        out = torch.empty(*prefixes.shape[:2], V, dtype=torch.float64)
        for b in range(prefixes.shape[0]):
            for i in range(prefixes.shape[1]):
                key = (b, tuple(prefixes[b, i].tolist()))
                if key not in table:
                    table[key] = torch.log_softmax(torch.randn(V, generator=g, dtype=torch.float64), 0)
                out[b, i] = table[key]
        return out
    trie, trace, final = _synthetic_search(items, first, B, nb, steps, scorer)
    eps = 1e-5                                           # (the trace's scores are fp32 roundings of the scorer's sums)
    stats = check_trace(trace, final, trie, [first] * B, scorer, eps)
    assert stats["pruned_steps"] > 0 and stats["max_candidates"] > nb and stats["max_score_err"] <= eps
    assert stats["prefixes"].shape == (B, nb, steps)
    # user 0, last step: the worst kept beam gives its slot to the worst dropped candidate (with that candidate's exact score, so
    # every other property still holds): the candidate it displaced is now dropped by more than 2 eps
    parent, token, score = (t.clone() for t in trace[-1])
    pre = torch.zeros(B, 1, 0, dtype=torch.int64)            # the prefixes the last step extends, rebuilt from the trace
    for s in range(steps - 1):
        p, t, _ = trace[s]
        pre = torch.cat([torch.gather(pre, 1, p.clamp(0, pre.shape[1] - 1)[:, :, None].expand(B, nb, s)), t[:, :, None]], 2)
    logp = scorer(steps - 1, pre)
    kept = {(int(parent[0, j]), int(token[0, j])) for j in range(nb)}
    cand = [(float(trace[-2][2][0, i]) + float(logp[0, i, t]), i, t) for i in range(nb)
            for t in trie.get([first] + pre[0, i].tolist()) if (i, t) not in kept]
    worst = min(cand)
    gap = float(score[0, nb - 1]) - worst[0]
    assert gap > 1e-3
    score[0, nb - 1], parent[0, nb - 1], token[0, nb - 1] = worst[0], worst[1], worst[2]
    bad = trace[:-1] + [(parent, token, score)]
    with pytest.raises(AssertionError, match="dropped candidate"):
        check_trace(bad, (score / steps).reshape(-1), trie, [first] * B, scorer, eps)
    # ... and inside the noise the same trace is a legitimate outcome
    check_trace(bad, (score / steps).reshape(-1), trie, [first] * B, scorer, gap)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
def _load():
    fx = np.load(FX)
    meta = json.loads(str(fx["meta_json"]))
    ocfg = orc.OracleConfig.from_dict(meta["config"])
    sd = orc.init_state_dict(ocfg, seed=meta["weight_seed"])
    for k, v in sd.items():
        if v.dim() == 2:
            sd[k] = v * meta["weight_scale"]
    sd["model.embed_tokens.weight"][synthetic.PAD_ID] = 0
    return fx, meta, sd


def _case(fx, tb):
    t = lambda k: torch.from_numpy(fx[f"b{tb}_{k}"])
    return t("input_ids"), t("attention_mask"), t("actions")


@pytest.fixture(scope="module")
def small16():
    """The fixture's model on a bf16 engine (one engine for the module: the searches of a shape share its decode buffers)."""
    from gamer_amd.config import Qwen3MultiConfig
    from gamer_amd.engine import Engine
    fx, meta, sd = _load()
    eng = Engine(Qwen3MultiConfig(**meta["config"]), temperature=0.7, dtype="bf16")
    eng.load_state_dict(sd)
    return fx, meta, sd, eng


class ForwardScorer:
    """Teacher-forced next-token log-probabilities from the bf16 SCORING forward (the pinned link of the chain): the prompt
    followed by a prefix of generated tokens, which take the behaviour level of the target item's behaviour token."""

    def __init__(self, eng, ids, am, act):
        self.eng, self.ids, self.am, self.act = eng, ids, am, act
        self.amax = 0.0

    def logits(self, prefixes):
        """prefixes int64 [B, n, s] -> the last position's logits [B, n, V] (bf16 values as fp32, on the host)."""
        B, n, s = prefixes.shape
        L0 = self.ids.shape[1]
        full = torch.cat([self.ids[:, None, :].expand(B, n, L0), prefixes.cpu()], 2).reshape(B * n, L0 + s)
        am = torch.cat([self.am, self.am.new_ones(B, s)], 1).repeat_interleave(n, 0)
        act = torch.cat([self.act, self.act[:, -1:].expand(B, s)], 1).repeat_interleave(n, 0)
        _, lg = self.eng.forward(full, am, act, train=False, act_zero_col=L0 - 1)
        assert lg.dtype == BF
        out = lg[:, -1, :].float().cpu().view(B, n, -1)
        self.amax = max(self.amax, float(out.abs().max()))
        return out

    def __call__(self, step, prefixes):
        return torch.log_softmax(self.logits(prefixes).double(), -1)

    def delta(self):
        return 1e-2 * self.amax

    def eps(self):
        return 2 * self.delta()


def _dense_ref(q, kp, vp, kg, vg, kok, gen_ok, B, nb, L0, t, nq, nkv):
    """fp64 softmax attention of the bf16-rounded inputs; a row with no allowed key gives 0."""
    N, G = B * nb, nq // nkv
    ref = torch.zeros(N, nq, 64, dtype=torch.float64)
    for n in range(N):
        b = n // nb
        for hd in range(nq):
            kv = hd // G
            keys = torch.cat([kp[b * L0:(b + 1) * L0, kv * 64:(kv + 1) * 64], kg[n, :t, kv * 64:(kv + 1) * 64]]).double()
            vals = torch.cat([vp[b * L0:(b + 1) * L0, kv * 64:(kv + 1) * 64], vg[n, :t, kv * 64:(kv + 1) * 64]]).double()
            allowed = torch.cat([kok[b].bool(), torch.full((t,), bool(gen_ok))])
            if not allowed.any():
                continue
            s = (keys @ q[n, hd * 64:(hd + 1) * 64].double()) * 0.125
            s[~allowed] = float("-inf")
            ref[n, hd] = torch.softmax(s, 0) @ vals
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("nq,nkv,nb,L0,t", [(2, 1, 6, 31, 1), (6, 3, 20, 130, 3), (2, 2, 5, 64, 4), (6, 3, 1, 130, 0), (2, 1, 1, 40, 0),
                                            (2, 1, 3, 1, 2)])
def test_attn_decode_bf16_kernel_against_dense(nq, nkv, nb, L0, t):
    """gamer_attn_decode_bf16 against fp64 attention of the same bf16 values, self (generated keys attended) and cross (masked):
    relative error < 2e-2, tests/test_bf16_gpu.py::test_attention_bf16_fwd_bwd's bar for the same two roundings (probabilities to
    bf16 before P V, the output once more).  Sample 1 has no allowed prompt key: exact zeros in the cross form.  Prompt lengths
    on both sides of the 32-key tile and of the four waves' split (1, 31, 40, 64, 130), one and two query tiles (nb * G = 1 .. 40),
    G = 1 and 2, V inside a wider buffer (row stride != width).  Two calls give the same bits."""
    from gamer_amd import ops
    dev, B, tmax = "cuda", 3, 4
    N = B * nb
    g = torch.Generator().manual_seed(L0 + t)
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(BF)
    q, kp, vp, kg, vg = rnd(N, nq * 64), rnd(B * L0, nkv * 64), rnd(B * L0, nkv * 64), rnd(N, tmax, nkv * 64), rnd(N, tmax, nkv * 64)
    ok = (torch.rand(B, L0, generator=g) < 0.6).to(torch.int32)
    ok[0, :5] = 0                                            # left padding
    ok[0, -1] = 1                                            # (sample 0 keeps a key at every L0)
    ok[1] = 0                                                # sample 1: nothing allowed
    vbuf = torch.zeros(B * L0, (nq + 2 * nkv) * 64, dtype=BF)
    vbuf[:, (nq + nkv) * 64:] = vp
    kp_d, v_d = kp.to(dev), vbuf.to(dev)[:, (nq + nkv) * 64:]
    for gen_ok in (True, False):
        o = torch.full((N, nq * 64), 7.0, dtype=BF, device=dev)
        args = (q.to(dev), kp_d, v_d, ok.to(dev), kg.to(dev), vg.to(dev), t, gen_ok, B, nb, L0, nq, nkv, 0.125)
        ops.attn_decode_bf16(*args, o)
        ref = _dense_ref(q, kp, vp, kg, vg, ok, gen_ok, B, nb, L0, t, nq, nkv)
        got = o.float().cpu().double().view(N, nq, 64)
        err = float((got - ref).abs().max() / ref.abs().max())
        print(f"attn_decode_bf16 nq={nq} nkv={nkv} nb={nb} L0={L0} t={t} gen_ok={gen_ok}: rel err {err:.3e}")
        assert err < 2e-2, (gen_ok, err)
        if not gen_ok or t == 0:
            assert bool((o[nb:2 * nb] == 0).all()), "rows without an allowed key must be exact zeros"
        o2 = torch.full_like(o, -3.0)
        ops.attn_decode_bf16(*args, o2)
        assert torch.equal(o, o2)


@pytest.mark.gpu
@pytest.mark.parametrize("gen_ok", [True, False])
def test_attn_decode_bf16_when_the_softmax_reference_moves(gen_ok):
    """The kernel takes probabilities relative to the first allowed sub-tile's maximum and replaces that reference when a later
    sub-tile exceeds it by more than 2^16 (the scoring forward's rule).  Random scores never do; here the keys from position 70 on
    score about 2^23 above the first ones, and the generated keys 2^23 above those, so the reference moves inside a wave's own
    tiles, between the waves, and in the merge's generated positions: still fp64 attention of the same values within 2e-2."""
    from gamer_amd import ops
    dev, B, nb, L0, t, tmax, nq, nkv = "cuda", 2, 5, 200, 2, 4, 2, 1
    N = B * nb
    g = torch.Generator().manual_seed(11)
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(BF)
    u = rnd(64).float()
    q = (u[None, :] + 0.1 * torch.randn(N, nq, 64, generator=g)).reshape(N, nq * 64).to(BF)
    kp, vp, kg, vg = rnd(B * L0, 64), rnd(B * L0, 64), rnd(N, tmax, 64), rnd(N, tmax, 64)
    late = (torch.arange(B * L0) % L0) >= 70
    kp[late] = (2.0 * u[None, :] + 0.3 * kp[late].float()).to(BF)
    kg = (4.0 * u[None, None, :] + 0.3 * kg.float()).to(BF)
    ok = torch.ones(B, L0, dtype=torch.int32)
    ok[:, :3] = 0
    o = torch.empty(N, nq * 64, dtype=BF, device=dev)
    ops.attn_decode_bf16(q.to(dev), kp.to(dev), vp.to(dev), ok.to(dev), kg.to(dev), vg.to(dev), t, gen_ok, B, nb, L0, nq, nkv, 0.125, o)
    ref = _dense_ref(q, kp, vp, kg, vg, ok, gen_ok, B, nb, L0, t, nq, nkv)
    err = float((o.float().cpu().double().view(N, nq, 64) - ref).abs().max() / ref.abs().max())
    print(f"moving reference, gen_ok={gen_ok}: rel err {err:.3e}")
    assert err < 2e-2, err


@pytest.mark.gpu
def test_attn_decode_bf16_rejects_bad_arguments_before_any_launch():
    from gamer_amd import _lib, ops
    dev, B, L0, nq, nkv, tmax = "cuda", 2, 40, 2, 1, 4
    lib = _lib.load()

    def run(nb, t, ldq=None, q_off=0):
        N = B * nb
        q = torch.zeros(N * (nq * 64 + 8) + 8, dtype=BF, device=dev)
        kp, vp = torch.zeros(B * L0, nkv * 64, dtype=BF, device=dev), torch.zeros(B * L0, nkv * 64, dtype=BF, device=dev)
        kg, vg = torch.zeros(N, tmax, nkv * 64, dtype=BF, device=dev), torch.zeros(N, tmax, nkv * 64, dtype=BF, device=dev)
        ok = torch.ones(B, L0, dtype=torch.int32, device=dev)
        o = torch.full((N, nq * 64), 7.0, dtype=BF, device=dev)
        rc = lib.gamer_attn_decode_bf16(q.data_ptr() + 2 * q_off, ldq or nq * 64, kp.data_ptr(), nkv * 64, vp.data_ptr(), nkv * 64,
                                        ok.data_ptr(), kg.data_ptr(), vg.data_ptr(), nkv * 64, tmax, t, 1, B, nb, L0, nq, nkv, 0.125,
                                        o.data_ptr(), _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc, bool((o == 7.0).all())
    rc, untouched = run(4, 2)
    assert rc == 0 and not untouched                         # (the good call, for contrast)
    for kw in (dict(nb=33, t=2),                             # nb * G = 66 > 64
               dict(nb=4, t=tmax + 1), dict(nb=4, t=-1),     # t outside [0, tmax]
               dict(nb=4, t=2, ldq=nq * 64 + 4),             # leading dim % 8 != 0
               dict(nb=4, t=2, q_off=4)):                    # base not 16-byte aligned
        rc, untouched = run(**kw)
        assert rc != 0 and untouched, kw
    assert b"gamer_attn_decode_bf16" in lib.gamer_last_error()
    with pytest.raises(RuntimeError):                        # G = 4
        z = lambda *s: torch.zeros(*s, dtype=BF, device=dev)
        ops.attn_decode_bf16(z(2, 256), z(8, 64), z(8, 64), torch.ones(2, 4, dtype=torch.int32, device=dev), z(2, 4, 64), z(2, 4, 64),
                             1, True, 2, 1, 4, 4, 1, 0.125, z(2, 256))
    # nb * G = 65 exactly: G = 1, 65 beams
    N = 65
    z = lambda *s: torch.zeros(*s, dtype=BF, device=dev)
    o = torch.full((N, 64), 7.0, dtype=BF, device=dev)
    with pytest.raises(RuntimeError, match="num_beams"):
        ops.attn_decode_bf16(z(N, 64), z(8, 64), z(8, 64), torch.ones(1, 8, dtype=torch.int32, device=dev), z(N, 4, 64), z(N, 4, 64),
                             1, True, 1, 65, 8, 1, 1, 0.125, o)
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())


@pytest.mark.gpu
def test_kv_append_bf16():
    from gamer_amd import ops
    g = torch.Generator().manual_seed(3)
    N, C, tmax = 37, 192, 4
    k = torch.randn(N, C, generator=g).to(BF).cuda()
    wide = torch.randn(N, 2 * C + 64, generator=g).to(BF).cuda()
    v = wide[:, C + 64:]                                     # a column slice: row stride != width
    kg, vg = torch.zeros(N, tmax, C, dtype=BF, device="cuda"), torch.zeros(N, tmax, C, dtype=BF, device="cuda")
    ops.kv_append_bf16(k, v, kg, vg, 2)
    assert torch.equal(kg[:, 2], k) and torch.equal(vg[:, 2], v)
    assert bool((kg[:, [0, 1, 3]] == 0).all()) and bool((vg[:, [0, 1, 3]] == 0).all())
    with pytest.raises(RuntimeError):
        ops.kv_append_bf16(k, v, kg, vg, tmax)


def _empty_target_rows(am, act):
    lv = act[:, -1:]
    return ~(((act[:, :-1] < lv) & (am[:, :-1] == 1)).any(1))


@pytest.mark.gpu
@pytest.mark.parametrize("tb", [0, 1, 2])
def test_teacher_forced_bf16_step_matches_the_scoring_forward(tb, small16):
    """A bf16 DecodeSession driven with fixed tokens (catalogue items) and parents (a non-identity permutation of every user's
    beams in front of steps 2 and 3): the prompt pass's and every step's logits against the last row of the bf16 scoring forward
    of prompt + tokens, per beam, within delta.  Behaviour 0: every user's cross rows are empty (zeros, where fp32 averages).
    ``reorder_cross_cache`` False and True give the same bits: there is no generated cross cache to re-order.

    MEASURED on MI355X (max |cached - forward| per step 0..4; delta is .025 - .043):
      behaviour 0:  0  0  0  0  0          behaviour 1:  0  0  .0078  .0078  .0156          behaviour 2:  0  0  0  0  0
    The step is the forward's arithmetic to the bit in most cases because gamer_attn_decode_bf16 rounds every probability
    relative to the softmax reference the scoring forward's kernel would use for that key (csrc/decode_bf16.hip); what is left is
    the order of fp32 sums.  A first form of the kernel, with each wave's own running maximum as the reference, gave
    .010 - .039 here and missed delta in one of the 15 cases (behaviour 2, step 3: .0391 against .0302) - on this fixture
    (matrices scaled by 4) two roundings of the same mathematics lie .037 - .055 apart (the scoring forward against itself with the
    prompt shifted by 35 pad columns), more than delta."""
    from gamer_amd.decode import DecodeSession
    fx, meta, sd, eng = small16
    nb, cb, V = 6, meta["codebook"], meta["config"]["vocab_size"]
    ids, am, act = _case(fx, tb)
    B, L0 = ids.shape
    N = B * nb
    if tb == 0:
        assert bool(_empty_target_rows(am, act).all())
    items = synthetic.item_tokens(torch.from_numpy(fx["catalogue"]), tb, cb)[:, 1:]
    sel = (7 * torch.arange(N) + 3) % items.shape[0]
    beam, base = torch.arange(N) % nb, torch.arange(N) // nb * nb
    parents = {2: base + (nb - 1 - beam), 3: base + (beam + 1) % nb}
    scorer = ForwardScorer(eng, ids, am, act)
    runs = []
    for reorder in (False, True):
        s = DecodeSession(eng, ids, am, act, nb, 4, reorder_cross_cache=reorder)
        got = [s.prefill_logits[:, :V].clone()]
        prefixes = torch.zeros(N, 0, dtype=torch.int64)
        history = [prefixes]
        for step in range(1, 5):
            if step in parents:
                s.reorder(parents[step].cuda())
                prefixes, sel = prefixes[parents[step]], sel[parents[step]]
            tok = items[sel, step - 1]
            got.append(s.step(tok.cuda())[:, :V].clone())
            prefixes = torch.cat([prefixes, tok[:, None]], 1)
            history.append(prefixes)
        sel = (7 * torch.arange(N) + 3) % items.shape[0]
        torch.cuda.synchronize()
        runs.append([g.cpu() for g in got])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    worst = 0.0
    for step, (got, pre) in enumerate(zip(runs[0], history)):
        ref = scorer.logits(pre.view(B, nb, step) if step else torch.zeros(B, 1, 0, dtype=torch.int64))
        ref = ref.reshape(-1, V)
        delta = 1e-2 * float(ref.abs().max())
        err = float((got - ref).abs().max())
        worst = max(worst, err / delta)
        print(f"behaviour {tb} step {step}: max |cached - scoring forward| = {err:.4e}, delta = {delta:.4e}")
        assert err < delta, (step, err, delta)


def _search_case(small16, tb, nb, **kw):
    from gamer_amd.decode import beam_search
    fx, meta, sd, eng = small16
    ids, am, act = _case(fx, tb)
    items = synthetic.item_tokens(torch.from_numpy(fx["catalogue"]), tb, meta["codebook"]).tolist()
    trie = ItemTrie(items)
    seq, sc, trace = beam_search(eng, ids, am, act, trie, nb, 4, return_trace=True, **kw)
    return eng, ids, am, act, trie, seq, sc, trace


def _check_search(eng, ids, am, act, trie, seq, sc, trace, nb):
    scorer = ForwardScorer(eng, ids, am, act)
    stats = check_trace([tuple(t.cpu() for t in st) for st in trace], sc, trie, ids[:, -1].tolist(), scorer, scorer.eps)
    B, L0 = ids.shape
    live = trace[-1][2].cpu() > -1e8
    assert torch.equal(seq.cpu()[:, L0:].view(B, nb, 4)[live], stats["prefixes"][live])
    assert torch.equal(seq.cpu()[:, :L0], ids.repeat_interleave(nb, 0))
    print(f"search: eps = {stats['eps']:.4e}, max |running - rescored| = {stats['max_score_err']:.4e}, smallest kept - dropped margin = "
          f"{stats['min_margin']:.4e}, pruned (step, user) pairs = {stats['pruned_steps']}, most candidates = {stats['max_candidates']}")
    return stats


@pytest.mark.gpu
@pytest.mark.parametrize("tb", [0, 1, 2])
def test_bf16_beam_search_prunes_only_within_noise(tb, small16):
    """20 beams, 4 tokens over the fixture's 48-item catalogue: every kept beam is a trie child of a kept prefix with the running
    score the scoring forward gives it within eps, and no dropped candidate beats a kept one by more than 2 eps
    (tests/helpers/beam_trace_check.py).  The catalogue has more 2-token prefixes than beams, so the search does prune."""
    nb = 20
    eng, ids, am, act, trie, seq, sc, trace = _search_case(small16, tb, nb)
    stats = _check_search(eng, ids, am, act, trie, seq, sc, trace, nb)
    assert stats["pruned_steps"] > 0 and stats["max_candidates"] > nb


@pytest.mark.gpu
@pytest.mark.parametrize("tb", [0, 2])
def test_bf16_beam_search_without_pruning_returns_the_catalogue_in_rescored_order(tb, small16):
    """A catalogue of exactly nb = 4 items with distinct first tokens: nothing is ever pruned, so the search returns exactly those
    items, ordered by its score = sum of 4 log-probs / 4.  Each log-prob is within eps of the scoring forward's, so the score is
    too, and beam i ranked above beam j means rescored(i) >= rescored(j) - 2 eps: the rescored order, up to swaps of
    neighbours that lie within 2 eps of each other."""
    from gamer_amd.decode import beam_search
    fx, meta, sd, eng = small16
    nb, cb = 4, meta["codebook"]
    ids, am, act = _case(fx, tb)
    B, L0 = ids.shape
    cat = torch.from_numpy(fx["catalogue"])
    rows = [int((cat[:, 0] == c).nonzero()[0]) for c in torch.unique(cat[:, 0])[:nb].tolist()]
    assert len(rows) == nb
    items = synthetic.item_tokens(cat[rows], tb, cb)
    seq, sc = beam_search(eng, ids, am, act, ItemTrie(items.tolist()), nb, 4)
    tails = seq.cpu()[:, L0:].view(B, nb, 4)
    scorer = ForwardScorer(eng, ids, am, act)
    resc = torch.zeros(B, nb, dtype=torch.float64)
    for s in range(4):
        logp = scorer(s, tails[:, :, :s] if s else torch.zeros(B, 1, 0, dtype=torch.int64))
        resc += torch.gather(logp.expand(B, nb, -1), 2, tails[:, :, s:s + 1])[:, :, 0]
    resc /= 4
    eps = scorer.eps()
    for b in range(B):
        assert sorted(tails[b].tolist()) == sorted(items[:, 1:].tolist()), b
        print(f"behaviour {tb} user {b}: search scores {sc.view(B, nb)[b].tolist()}, rescored {resc[b].tolist()}, eps {eps:.4e}")
        assert float((sc.cpu().view(B, nb)[b].double() - resc[b]).abs().max()) <= eps
        for i in range(nb):
            for j in range(i + 1, nb):
                assert float(resc[b, i]) >= float(resc[b, j]) - 2 * eps, (b, i, j)


@pytest.mark.gpu
def test_bf16_rerun_path_module_generate_and_repeatability(small16):
    """``use_cache=False`` (the whole sequence again every step) is the same computation in bf16 and passes the same check; the
    same search twice gives the same bits; ``generate()`` of a module built with dtype="bf16" returns what beam_search returns."""
    from gamer_amd.config import Qwen3MultiConfig
    from gamer_amd.decode import beam_search, prefix_allowed_tokens
    from gamer_amd.modeling import Qwen3MultiWithTemperature
    fx, meta, sd, _ = small16
    tb, nb = 1, 20
    eng, ids, am, act, trie, seq, sc, trace = _search_case(small16, tb, nb, use_cache=False, reorder_cross_cache=True)
    stats = _check_search(eng, ids, am, act, trie, seq, sc, trace, nb)
    assert stats["pruned_steps"] > 0
    a = beam_search(eng, ids, am, act, trie, nb, 4)
    b = beam_search(eng, ids, am, act, trie, nb, 4)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    model = Qwen3MultiWithTemperature(Qwen3MultiConfig(**meta["config"]), dtype="bf16")
    model.set_hyper(0.7)
    model.load_state_dict(sd)
    assert model.engine.dtype == "bf16"
    out = model.generate(input_ids=ids, attention_mask=am, actions=act, max_new_tokens=4, num_beams=nb, num_return_sequences=nb,
                         prefix_allowed_tokens_fn=prefix_allowed_tokens(trie))
    seq_m, sc_m = beam_search(model.engine, ids, am, act, trie, nb, 4)
    assert torch.equal(out.sequences, seq_m) and torch.equal(out.sequences_scores, sc_m)
    assert torch.equal(seq_m, a[0]) and torch.equal(sc_m, a[1])          # (the same weights on another engine: the same search)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["session", "qwen3", "qwen3_session", "qwen3moe"])
def test_bf16_generation_of_the_other_variants_is_refused_by_name(variant, small16):
    from gamer_amd.config import Qwen3Config, Qwen3MoeConfig, Qwen3MultiConfig, Qwen3SessionConfig
    from gamer_amd.decode import beam_search
    from gamer_amd.engine import Engine
    fx, meta, sd, _ = small16
    small = dict(vocab_size=49, pad_token_id=synthetic.PAD_ID, hidden_size=128, num_hidden_layers=1, num_attention_heads=2,
                 num_key_value_heads=1, intermediate_size=256)
    if variant == "session":
        cfg = Qwen3MultiConfig(**meta["config"])
    elif variant == "qwen3":
        cfg = Qwen3Config(**small)
    elif variant == "qwen3_session":
        cfg = Qwen3SessionConfig(num_positions=5, model_max_length=1024, **small)
    else:
        moe = np.load(os.path.join(os.path.dirname(FX), "moe_small.npz"))
        cfg = Qwen3MoeConfig(**json.loads(str(moe["meta_json"]))["config"])
    eng = Engine(cfg, variant=variant, dtype="bf16")
    ids, am, act = _case(fx, 2)
    trie = ItemTrie(synthetic.item_tokens(torch.from_numpy(fx["catalogue"]), 2, meta["codebook"]).tolist())
    kw = dict(session_ids=torch.zeros_like(ids), extended_session_ids=torch.zeros_like(ids)) if "session" in variant else {}
    for use_cache in (True, False):
        with pytest.raises(NotImplementedError, match=f"'{variant}'"):
            beam_search(eng, ids, am, act, trie, 4, 4, use_cache=use_cache, reorder_cross_cache=True, **kw)
