"""Qwen3Multi's FFN ablation configurations on the HIP engine against the real reference (tests/golden/ablate_*.npz,
decode_ablate_small.npz from tools/make_golden_ffn_ablation.py): dense layers, PBATransformer experts and behaviour-only routing
in the fp32 forms and bf16, the cached decode, the new kernels against fp64 and a short ``train.py --base_model`` run.
Bars: those of the ``small`` / ``small_bf16`` fixtures (tests/test_model_gpu.py, tests/test_bf16_gpu.py)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gamer_amd import ops, synthetic  # noqa: E402
from gamer_amd.config import Qwen3MultiConfig  # noqa: E402
from gamer_amd.decode import ItemTrie, beam_search  # noqa: E402
from gamer_amd.engine import Engine  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import ffn_ablation_weights as fw  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"
F32_CASES = ["ablate_dense_small", "ablate_pba_small", "ablate_behonly_small", "ablate_session_small"]


def _load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    meta = json.loads(str(z["meta_json"]))
    sd = fw.init_state_dict(meta["config"], meta["weight_seed"], meta.get("weight_scale", 1.0))
    return z, meta, sd


def _engine(name, **kw):
    z, meta, sd = _load(name)
    cfg = Qwen3MultiConfig(**meta["config"])
    cfg.dropout_rate = 0.2                  # (the kernels get p = 0 through dropout=False)
    variant = "session" if "Session" in meta["model"] else "multi"
    eng = Engine(cfg, temperature=meta["temperature"], variant=variant, **kw)
    eng.load_state_dict(sd)
    batch = {k: torch.from_numpy(z[k]) for k in ("input_ids", "attention_mask", "actions", "labels")}
    if variant == "session":
        batch.update(session_ids=torch.from_numpy(z["session_ids"]), extended_session_ids=torch.from_numpy(z["extended_session_ids"]))
    return z, eng, batch


def _fwd(eng, batch, **kw):
    return eng.forward(batch["input_ids"], batch["attention_mask"], batch["actions"], session_ids=batch.get("session_ids"),
                       extended_session_ids=batch.get("extended_session_ids"), **kw)


def _relmax(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


def _grad_errors(eng, z):
    gkeys = [str(k) for k in z["grad_keys"]]
    assert sorted(eng.grads) == gkeys
    norms = np.array([float(eng.grads[k].double().norm()) for k in gkeys])
    rel = np.abs(norms - z["grad_norms"]) / np.maximum(z["grad_norms"], 1e-12)
    samples = {}
    for k in z.files:
        if k.startswith("grad::"):
            samples[k[6:]] = _relmax(eng.grads[k[6:]].cpu().numpy(), z[k])
        elif k.startswith("gradsample::"):
            g = eng.grads[k[12:]]
            samples[k[12:]] = _relmax(g[::max(1, g.shape[0] // 8), ::max(1, g.shape[1] // 8)].cpu().numpy(), z[k])
    return gkeys, norms, rel, samples


@pytest.mark.parametrize("matmul", ["f32", "split3", "split6"])
@pytest.mark.parametrize("name", F32_CASES)
def test_ablation_against_reference_fixture(name, matmul):
    z, eng, batch = _engine(name, matmul=matmul)
    _, logits = _fwd(eng, batch, train=False)
    e_raw = _relmax(logits.cpu().numpy(), z["logits_raw"])
    loss, logits_s = _fwd(eng, batch, labels=batch["labels"], train=False)
    e_scaled = _relmax(logits_s.cpu().numpy(), z["logits_scaled"])
    assert e_raw < 2e-5 and e_scaled < 2e-5, (e_raw, e_scaled)
    assert abs(float(loss) - float(z["loss_mean"])) < 1e-5 * float(z["loss_mean"])
    loss, _ = _fwd(eng, batch, labels=batch["labels"], train=True, dropout=False)
    assert abs(float(loss) - float(z["loss_train_mode"])) < 1e-5 * float(z["loss_train_mode"])
    eng.zero_grad()
    eng.backward(1.0)
    eng.check_inputs()
    gkeys, norms, rel, samples = _grad_errors(eng, z)
    gn = float(np.sqrt((norms ** 2).sum()))
    assert abs(gn - float(z["global_grad_norm"])) < 1e-4 * float(z["global_grad_norm"])
    assert float(rel.max()) < 1e-3, gkeys[int(rel.argmax())]
    wk = max(samples, key=samples.get)
    assert samples[wk] < 1e-3, (wk, samples[wk])
    assert all(bool(torch.isfinite(g).all()) for g in eng.grads.values())


def test_ablation_bf16_against_reference_autocast_fixture():
    z, eng, batch = _engine("ablate_pba_small_bf16", dtype="bf16")
    _, logits = _fwd(eng, batch, train=False)
    assert logits.dtype == torch.bfloat16
    ref = z["logits_raw"]
    assert float(np.abs(logits.float().cpu().numpy() - ref).max()) < 1e-2 * float(np.abs(ref).max())
    loss, _ = _fwd(eng, batch, labels=batch["labels"], train=True, dropout=False)
    assert abs(float(loss) - float(z["loss_train_mode"])) < 1e-3
    eng.zero_grad()
    eng.backward(1.0)
    torch.cuda.synchronize()
    gkeys, norms, rel, _ = _grad_errors(eng, z)
    np.testing.assert_allclose(norms, z["grad_norms"], rtol=3e-2, atol=1e-9)
    gn = float(np.sqrt((norms ** 2).sum()))
    assert abs(gn - float(z["global_grad_norm"])) < 5e-3 * float(z["global_grad_norm"])
    for k in z.files:
        if k.startswith("grad::") or k.startswith("gradsample::"):
            gt = eng.grads[k.split("::")[1]].cpu()
            got = gt.numpy() if k.startswith("grad::") else gt[::max(1, gt.shape[0] // 8), ::max(1, gt.shape[1] // 8)].numpy()
            assert np.abs(got - z[k]).max() <= 8e-2 * max(np.abs(z[k]).max(), 1e-12), k


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_silu_kernels_against_fp64_and_the_swiglu_dropout_mask(dtype):
    # (5, 260, 520): 65 quads per row, a second trip of the lane loop with one lane
    for T, I, ld in ((300, 192, 200), (5, 260, 520)):
        _silu_kernels_case(T, I, ld, dtype)


def _silu_kernels_case(T, I, ld, dtype):
    p, seed = 0.25, 1234
    g = torch.Generator().manual_seed(5)
    h = (torch.randn(T, ld, generator=g) * 3).to(dtype)
    dhm = torch.randn(T, I, generator=g).to(dtype)
    hd, dd = h[:, :I].double(), dhm.double()
    s = torch.sigmoid(hd)
    # no dropout: exact formulas
    hg, hm = h.to(DEV), torch.empty(T, I, dtype=dtype, device=DEV)
    ops.silu_fwd_ld(hg, ld, T, I, 0.0, seed, hm)
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    assert float((hm.cpu().double() - hd * s).abs().max()) < tol * float((hd * s).abs().max())
    ops.silu_bwd_ld(hg, ld, T, I, dhm.to(DEV), 0.0, seed)
    ref = dd * (s * (1 + hd * (1 - s)))
    assert float((hg[:, :I].cpu().double() - ref).abs().max()) < tol * float(ref.abs().max())
    assert torch.equal(hg[:, I:].cpu(), h[:, I:])                       # columns past I untouched
    # dropout: the mask of gamer_swiglu_fwd_ld under the same seed (up = 1, so the SwiGLU output is drop(silu(gate)))
    gu = torch.cat([h[:, :I], torch.ones(T, I, dtype=dtype)], 1).to(DEV)
    hm_sw = torch.empty(T, I, dtype=dtype, device=DEV)
    ops.swiglu_fwd_ld(gu, 2 * I, T, I, p, seed, hm_sw)
    hg = h.to(DEV)
    ops.silu_fwd_ld(hg, ld, T, I, p, seed, hm)
    assert torch.equal(hm.cpu(), hm_sw.cpu())
    kept = hm.cpu().double() != 0
    assert abs(float(kept.double().mean()) - (1 - p)) < max(0.02, 4 * (p * (1 - p) / (T * I)) ** 0.5)    # (four sigma of T * I draws)
    ops.silu_bwd_ld(hg, ld, T, I, dhm.to(DEV), p, seed)
    ref = torch.where(kept, ref / (1 - p), torch.zeros_like(ref))
    assert float((hg[:, :I].cpu().double() - ref).abs().max()) < tol * float(ref.abs().max())


def test_expert_lists_put_rows_past_the_last_expert_in_no_group():
    B, S, E = 5, 37, 2
    g = torch.Generator().manual_seed(2)
    expert = torch.randint(0, 4, (B, S), generator=g, dtype=torch.int32).to(DEV)       # 2, 3: no such expert
    table = torch.tensor([0, 1, 2, 2, 2, 2], dtype=torch.int32, device=DEV)
    ops.router_position_table(expert, table)
    T = B * S
    perm, slot = torch.full((T,), -1, dtype=torch.int32, device=DEV), torch.full((T,), -1, dtype=torch.int32, device=DEV)
    offsets, work = torch.empty(E + 1, dtype=torch.int32, device=DEV), torch.empty((B + 1) * E, dtype=torch.int32, device=DEV)
    ops.expert_lists(expert, E, perm, slot, offsets, work)
    ex, pm, sl, off = expert.view(-1).cpu(), perm.cpu().long(), slot.cpu().long(), offsets.cpu().tolist()
    assert torch.equal(torch.sort(pm).values, torch.arange(T)) and torch.equal(pm[sl], torch.arange(T))
    assert off == [0, int((ex == 0).sum()), int((ex <= 1).sum())]
    tail = pm[off[E]:]
    assert bool((ex[tail] >= E).all()) and bool((tail[1:] > tail[:-1]).all())         # no group, token order


def test_behaviour_only_semantic_rows_pass_the_residual_bit_for_bit():
    z, eng, batch = _engine("ablate_behonly_small", matmul="split3")
    _fwd(eng, batch, labels=batch["labels"], train=True, dropout=False)
    ws, cfg = eng.ws, eng.cfg
    semantic = (ws.router["expert"].view(-1) >= cfg.num_experts)
    assert bool(semantic.any())
    for l in range(cfg.num_hidden_layers):
        xin = ws.x[l][2] if l in cfg.cross_attention_decoder else ws.x[l][1]
        xout = ws.x[l + 1][0] if l + 1 < cfg.num_hidden_layers else ws.x_final
        assert torch.equal(xout[semantic], xin[semantic]), l
        assert not torch.equal(xout[~semantic], xin[~semantic])


def test_non_gated_kernels_run(monkeypatch):
    seen = []
    real = ops.call

    def record(name, *a):
        seen.append(name)
        return real(name, *a)
    monkeypatch.setattr(ops, "call", record)
    for dtype, sfx in (("f32", ""), ("bf16", "_bf16")):
        seen.clear()
        z, eng, batch = _engine("ablate_pba_small", dtype=dtype)
        _fwd(eng, batch, labels=batch["labels"], train=True, dropout=False)
        eng.zero_grad()
        eng.backward(1.0)
        torch.cuda.synchronize()
        assert seen.count("gamer_silu_fwd_ld" + sfx) == 4 and seen.count("gamer_silu_bwd_ld" + sfx) == 4
        assert not [n for n in seen if n.startswith("gamer_swiglu")]


@pytest.mark.parametrize("tb", [0, 1, 2])
def test_decode_beams_match_reference_generate(tb):
    z, meta, sd = _load("decode_ablate_small")
    cfg = Qwen3MultiConfig(**meta["config"])
    eng = Engine(cfg, temperature=0.7)
    eng.load_state_dict(sd)
    ids, am, act = (torch.from_numpy(z[f"b{tb}_{k}"]) for k in ("input_ids", "attention_mask", "actions"))
    trie = ItemTrie(synthetic.item_tokens(torch.from_numpy(z["catalogue"]), tb, meta["codebook"]).tolist())
    beams = meta["beams"]
    seq, sc = beam_search(eng, ids, am, act, trie, beams, 4)
    assert torch.equal(seq.cpu(), torch.from_numpy(z[f"b{tb}_sequences"]))
    assert float((sc.cpu().double() - torch.from_numpy(z[f"b{tb}_scores"])).abs().max()) < 1e-4
    seq_f, sc_f = beam_search(eng, ids, am, act, trie, beams, 4, reorder_cross_cache=True)
    seq_nc, sc_nc = beam_search(eng, ids, am, act, trie, beams, 4, use_cache=False, reorder_cross_cache=True)
    assert torch.equal(seq_f, seq_nc) and float((sc_f - sc_nc).abs().max()) < 2e-5


def test_module_trains_under_autocast():
    from gamer_amd.modeling import Qwen3MultiWithTemperature, Qwen3SessionMultiWithTemperature
    z, meta, sd = _load("ablate_pba_small")
    for cls in (Qwen3MultiWithTemperature, Qwen3SessionMultiWithTemperature):
        model = cls(Qwen3MultiConfig(**meta["config"]))
        model.set_hyper(0.7)
        model.load_state_dict(sd)
        kw = {k: torch.from_numpy(z[k]).to(DEV) for k in ("input_ids", "attention_mask", "actions", "labels",
                                                          "session_ids", "extended_session_ids")}
        for autocast in (False, True):
            model.zero_grad()
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                out = model(**kw)
            out.loss.backward()
            assert torch.isfinite(out.loss) and all(bool(torch.isfinite(p.grad).all()) for p in model.parameters())


def test_train_base_model_loss_falls(tmp_path):
    from gamer_amd import train
    d = tmp_path / "base"
    Qwen3MultiConfig(mlp_type="PBATransformer", sparse_layers_decoder=[0, 2, 4, 6], Moe_behavior_only=True).save_pretrained(str(d))
    state = train.main(["--base_model", str(d), "--max_his_len", "20", "--per_device_batch_size", "16",
                        "--gradient_accumulation_steps", "2", "--epochs", "2", "--steps_per_epoch", "12", "--logging_step", "4",
                        "--learning_rate", "2e-3"])
    losses = [r["loss"] for r in state["log_history"] if "loss" in r]
    assert losses[-1] < losses[0] - 0.3, losses
