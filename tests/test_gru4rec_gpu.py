"""GRU4Rec on the GPU: the recurrence kernels (gamer_gru_fwd / _bwd and the GEMMs around them) against fp64 torch.nn.GRU, and
the model against the real reference class (tests/golden/gru4rec_small.npz, tools/make_golden_gru4rec.py)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import gru4rec_weights as gw  # noqa: E402

pytestmark = pytest.mark.gpu
FX = os.path.join(os.path.dirname(__file__), "golden", "gru4rec_small.npz")
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    from gamer_amd import build
    build.build()


def _rel(got, ref):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _inputs(E, H, L, B, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, L, E, generator=g)
    w_ih = torch.randn(3 * H, E, generator=g) / E ** 0.5
    w_hh = torch.randn(3 * H, H, generator=g) / H ** 0.5
    dy = torch.randn(B, L, H, generator=g)
    return x, w_ih, w_hh, dy


def _gpu_layer(x, w_ih, w_hh, dy, lens=None):
    """h, dx, dW_ih, dW_hh of one layer on the HIP path"""
    from gamer_amd.gru4rec import _GRULayerFn
    xd = x.to(DEV).requires_grad_(True)
    wi, wh = w_ih.to(DEV).requires_grad_(True), w_hh.to(DEV).requires_grad_(True)
    h = _GRULayerFn.apply(xd, wi, wh, lens, True)
    h.backward(dy.to(DEV))
    torch.cuda.synchronize()
    return h.detach(), xd.grad, wi.grad, wh.grad


def _fp64_layer(x, w_ih, w_hh, dy):
    E, H = x.shape[-1], w_hh.shape[1]
    gru = torch.nn.GRU(E, H, bias=False, batch_first=True).double()
    with torch.no_grad():
        gru.weight_ih_l0.copy_(w_ih.double())
        gru.weight_hh_l0.copy_(w_hh.double())
    x64 = x.double().requires_grad_(True)
    h, _ = gru(x64)
    h.backward(dy.double())
    return h.detach(), x64.grad, gru.weight_ih_l0.grad, gru.weight_hh_l0.grad


# (E, H, L, B): every (E, H) at L = 1, 20, 200; B = 1, 17 and 4096 (the fp64 CPU reference bounds the largest shapes)
CASES = [(64, 128, 1, 17), (64, 128, 20, 17), (64, 128, 200, 17), (64, 128, 20, 4096), (64, 128, 200, 1),
         (32, 64, 1, 1), (32, 64, 20, 17), (32, 64, 200, 17), (32, 64, 20, 4096),
         (64, 16, 1, 17), (64, 16, 20, 4096), (64, 16, 200, 17),
         (128, 256, 1, 17), (128, 256, 20, 17), (128, 256, 200, 1), (128, 256, 20, 4096)]


@pytest.mark.parametrize("E,H,L,B", CASES)
def test_gru_layer_against_fp64_torch(E, H, L, B):
    x, w_ih, w_hh, dy = _inputs(E, H, L, B, seed=E * 131 + H * 7 + L + B)
    got = _gpu_layer(x, w_ih, w_hh, dy)
    ref = _fp64_layer(x, w_ih, w_hh, dy)
    bar = 1e-5 if L <= 20 else 1e-4
    for name, a, r in zip(("h", "dx", "dW_ih", "dW_hh"), got, ref):
        assert _rel(a, r) < bar, (name, _rel(a, r))
    for t in (0, L // 2, L - 1):                        # every step on its own scale, too
        assert _rel(got[0][:, t], ref[0][:, t]) < bar, t


def test_gru_layer_is_deterministic():
    x, w_ih, w_hh, dy = _inputs(64, 128, 20, 4096, seed=1)
    a = _gpu_layer(x, w_ih, w_hh, dy)
    b = _gpu_layer(x, w_ih, w_hh, dy)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize("H", [128, 256])
def test_gru_rows_are_independent(H):
    from gamer_amd import ops
    B, L = 4096, 20
    g = torch.Generator().manual_seed(H)
    gi = (torch.randn(B, L, 3 * H, generator=g)).to(DEV)
    w_hh = (torch.randn(3 * H, H, generator=g) / H ** 0.5).to(DEV)
    h = torch.empty(B, L, H, device=DEV)
    ops.gru_fwd(gi, w_hh, h)
    for r in (0, 5, 17, 2049, 4095):
        for n in (1, 3, 16, 33):
            sub = torch.zeros(n, L, 3 * H, device=DEV)
            at = (r * 7) % n                              # the row at another place of a smaller batch
            sub[at] = gi[r]
            hs = torch.empty(n, L, H, device=DEV)
            ops.gru_fwd(sub, w_hh, hs)
            assert torch.equal(hs[at], h[r]), (r, n)


def test_gru_lens_stop_early_and_zero_the_rest():
    from gamer_amd import ops
    B, L, H = 40, 30, 64
    g = torch.Generator().manual_seed(9)
    gi = torch.randn(B, L, 3 * H, generator=g).to(DEV)
    w_hh = (torch.randn(3 * H, H, generator=g) / 8).to(DEV)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[16:32] = 4                                       # a whole block stops after step 4
    lens = lens.to(DEV)
    full, part = torch.empty(B, L, H, device=DEV), torch.full((B, L, H), float("nan"), device=DEV)
    gates_f = torch.empty(ops.gru_gates_floats(B, L, H), device=DEV)
    gates_p = torch.empty_like(gates_f)
    ops.gru_fwd(gi, w_hh, full, gates_f)
    ops.gru_fwd(gi, w_hh, part, gates_p, lens=lens)
    for b in range(B):
        n = int(lens[b])
        assert torch.equal(part[b, :n], full[b, :n]), b
    assert bool(torch.isfinite(part).all()) and float(part[16:32, 4:].abs().max()) == 0
    dy = torch.randn(B, L, H, generator=g).to(DEV)
    keep = (torch.arange(L, device=DEV)[None, :] < lens[:, None]).float()[..., None]
    res = []
    for gates, hh, ln, d in ((gates_f, full, None, dy * keep), (gates_p, part, lens, dy)):
        dgi = torch.full((B, L, 3 * H), float("nan"), device=DEV)
        dgh = torch.full((B, L, 3 * H), float("nan"), device=DEV)
        ops.gru_bwd(d.contiguous(), hh, gates, w_hh, dgi, dgh, lens=ln)
        res.append((dgi, dgh))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_wrappers_refuse_bad_shapes():
    from gamer_amd import ops
    with pytest.raises(RuntimeError, match="H % 16"):
        ops.gru_fwd(torch.zeros(2, 3, 72, device=DEV), torch.zeros(72, 24, device=DEV), torch.empty(2, 3, 24, device=DEV))
    with pytest.raises(RuntimeError, match="gi must be"):
        ops.gru_fwd(torch.zeros(2, 3, 47, device=DEV), torch.zeros(48, 16, device=DEV), torch.empty(2, 3, 16, device=DEV))
    with pytest.raises(RuntimeError, match="lens"):
        ops.gru_fwd(torch.zeros(2, 3, 48, device=DEV), torch.zeros(48, 16, device=DEV), torch.empty(2, 3, 16, device=DEV),
                    lens=torch.ones(2, dtype=torch.int32, device=DEV))


# ---- the model against the real reference class ------------------------------------------------------------------------------
def _model(tag):
    from gamer_amd.gru4rec import GRU4Rec, GRU4RecConfig
    z = np.load(FX)
    m = json.loads(str(z["meta_json"]))
    c = m["configs"][tag]
    model = GRU4Rec(GRU4RecConfig(**c["config"]), m["n_items"], max_his_len=m["max_his_len"])
    model.load_state_dict(gw.init_state_dict({k: tuple(s) for k, s in zip(c["keys"], c["shapes"])}, c["weight_seed"]))
    p = tag + "/"
    inter = dict(inputs=torch.from_numpy(z[p + "inputs"]).to(DEV), seq_len=torch.from_numpy(z[p + "seq_len"]).to(DEV),
                 target=torch.from_numpy(z[p + "target"]).to(DEV))
    return model.to(DEV), z, m, inter, p


@pytest.mark.parametrize("tag", ["a", "b"])
def test_gru4rec_forward_loss_and_grads_match_reference(tag):
    model, z, m, inter, p = _model(tag)
    model.eval()
    with torch.no_grad():
        out = model(inter["inputs"], inter["seq_len"])
    assert _rel(out, z[p + "out"]) < 2e-5
    model.train()
    model.zero_grad()
    loss = model.calculate_loss(inter)
    loss.backward()
    assert abs(float(loss.detach()) - float(z[p + "loss"])) <= 1e-5 * abs(float(z[p + "loss"]))
    for k, prm in model.named_parameters():
        if k == "item_embedding.weight":
            continue
        assert prm.grad is not None, k
        if p + "grad/" + k in z.files:
            assert _rel(prm.grad, z[p + "grad/" + k]) < 2e-4, k
        else:
            ref = z[p + "grad4/" + k]
            assert _rel(prm.grad.cpu()[::4], ref) < 2e-4, k
            ck, rck = gw.checksums({k: prm.grad.cpu()})[0], z[p + "grad_checksum/" + k]
            assert abs(ck[1] - rck[1]) < 1e-3 * rck[1], k
    gi = model.item_embedding.weight.grad
    rows = torch.from_numpy(z[p + "rows"])
    assert _rel(gi.cpu()[rows], z[p + "grad_item_rows"]) < 2e-4
    assert float(gi[0].abs().sum()) > 0                  # the head reaches the padding row
    ck, ref = gw.checksums({"g": gi.cpu()})[0], z[p + "grad_item_checksum"]
    assert abs(ck[0] - ref[0]) < 2e-4 * np.sqrt(ref[1]) * 10 and abs(ck[1] - ref[1]) < 1e-3 * ref[1]


@pytest.mark.parametrize("tag", ["a", "b"])
@pytest.mark.parametrize("ranged", [False, True])
def test_gru4rec_full_sort_matches_reference(tag, ranged):
    model, z, m, inter, p = _model(tag)
    model.eval()
    if ranged:
        inter = dict(inter, item_range=tuple(m["item_range"]))
    with torch.no_grad():
        scores = model.full_sort_predict(dict(inter))
    cols = torch.from_numpy(z[p + "cols"])
    ref = torch.from_numpy(z[p + ("scores_r_cols" if ranged else "scores_cols")])
    got = scores.cpu()[:, cols]
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(got), fin)
    assert _rel(got[fin], ref[fin]) < 2e-5
    idx, _ = model.full_sort_topk(dict(inter), 10)
    ref_top = torch.from_numpy(z[p + ("top10_r" if ranged else "top10")])
    full = scores.cpu()
    for b in range(idx.shape[0]):
        for q in range(10):
            a, r = int(idx[b, q]), int(ref_top[b, q])
            # identical ranks unless two neighbours' scores lie within fp32 noise of each other
            assert a == r or abs(float(full[b, a]) - float(full[b, r])) < 1e-5, (b, q, a, r)


def test_gru4rec_topk_is_a_stable_argsort_of_full_sort_predict():
    from gamer_amd.gru4rec import GRU4Rec, GRU4RecConfig
    torch.manual_seed(4)
    model = GRU4Rec(GRU4RecConfig(), 5000).to(DEV).eval()
    g = torch.Generator().manual_seed(4)
    B, L = 37, 9
    lens = torch.randint(1, L + 1, (B,), generator=g)
    inputs = torch.randint(1, 5001, (B, L), generator=g) * (torch.arange(L)[None, :] < lens[:, None])
    inter = dict(inputs=inputs.to(DEV), seq_len=lens.to(DEV))
    for rng in (None, (100, 2100)):
        it = dict(inter, item_range=rng) if rng else inter
        scores = model.full_sort_predict(dict(it)).cpu()
        idx, sc = model.full_sort_topk(dict(it), 20)
        ref = torch.argsort(-scores, dim=1, stable=True)[:, :20]
        close = (scores.gather(1, idx.cpu()) - scores.gather(1, ref)).abs() < 1e-5
        assert bool(((idx.cpu() == ref) | close).all())
        assert torch.allclose(sc.cpu(), scores.gather(1, idx.cpu()), atol=1e-5)


def test_gru4rec_dropout_is_repeatable_and_equals_fp64_with_its_mask():
    from gamer_amd import ops, rec_common
    model, z, m, inter, p = _model("b")
    model.dropout_prob = 0.3
    model.train()
    res = []
    for _ in range(2):
        rec_common._Seeds.value = 77
        model.zero_grad()
        loss = model.calculate_loss(inter)
        loss.backward()
        res.append([loss.detach().clone()] + [q.grad.clone() for q in model.parameters()])
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)
    # the kernel's own mask: the same dropout (seed 78, the next seed after 77) run on ones
    ids = inter["inputs"]
    B, L = ids.shape
    E = model.embedding_size
    ones = torch.ones(B * L, E, device=DEV)
    mask = torch.zeros_like(ones)
    ops.residual_dropout_fwd(mask, ones, 0.3, 78)
    assert 0.5 < float((mask == 0).float().mean()) / 0.3 < 1.5
    # fp64 composition of the reference's forward with that mask
    sd = {k: v.detach().double().cpu().requires_grad_(True) for k, v in model.state_dict().items()}
    Et = sd["item_embedding.weight"]
    x = (Et[ids.cpu()] * mask.double().cpu().view(B, L, E))
    gru = torch.nn.GRU(E, model.hidden_size, num_layers=2, bias=False, batch_first=True).double()
    for k in range(2):
        setattr(gru, f"weight_ih_l{k}", torch.nn.Parameter(sd[f"gru_layers.weight_ih_l{k}"]))
        setattr(gru, f"weight_hh_l{k}", torch.nn.Parameter(sd[f"gru_layers.weight_hh_l{k}"]))
    gru._flat_weights = [getattr(gru, n) for n in gru._flat_weights_names]
    h, _ = gru(x)
    n = inter["seq_len"].cpu().long()
    hl = h[torch.arange(B), n - 1]
    out = hl @ sd["dense.weight"].t() + sd["dense.bias"]
    ref_loss = torch.nn.functional.cross_entropy(out @ Et.t(), inter["target"].cpu())
    grads = torch.autograd.grad(ref_loss, [sd[k] for k in ("item_embedding.weight", "dense.weight", "dense.bias")] +
                                [getattr(gru, f"weight_{a}_l{k}") for k in range(2) for a in ("ih", "hh")])
    ref_loss = ref_loss.detach()
    assert abs(float(res[0][0]) - float(ref_loss)) <= 1e-5 * abs(float(ref_loss))
    got = dict(model.named_parameters())
    names = ["item_embedding.weight", "dense.weight", "dense.bias"] + [f"gru_layers.weight_{a}_l{k}" for k in range(2)
                                                                        for a in ("ih", "hh")]
    for name, gref in zip(names, grads):
        assert _rel(got[name].grad, gref) < 2e-4, name


def test_training_step_memory_is_bounded():
    from gamer_amd.gru4rec import GRU4Rec, GRU4RecConfig
    R, V, S = 4096, 200_000, 20
    limit = R * V * 4                               # one [R, V] fp32 logits tensor: 3.3 GB
    torch.manual_seed(0)
    model = GRU4Rec(GRU4RecConfig(dropout=0.0), V - 1).to(DEV)
    g = torch.Generator().manual_seed(1)
    inter = dict(inputs=torch.randint(1, V, (R, S), generator=g).to(DEV), seq_len=torch.full((R,), S, device=DEV),
                 target=torch.randint(1, V, (R,), generator=g).to(DEV))
    model.train()

    def step():
        model.zero_grad(set_to_none=True)
        loss = model.calculate_loss(inter)
        loss.backward()
        assert torch.isfinite(loss)
    step()                                            # warm the cached workspaces
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < 0.2 * limit, peak                   # the whole step: activations, gates, dE, GEMM workspaces


def test_train_rec_gru4rec_two_epochs_and_only_test(tmp_path):
    import subprocess
    from gamer_amd import synthetic
    from gamer_amd.gru4rec import GRU4Rec, GRU4RecConfig
    synthetic.write_smb_dataset(str(tmp_path), "syn", n_users=60, n_items=40, seed=5, min_sessions=3)
    cfg = tmp_path / "cfg"
    cfg.mkdir()
    (cfg / "config.json").write_text(json.dumps(dict(embedding_size=64, hidden_size=64, dropout=0.1)))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--backbone", "GRU4Rec", "--base_model", str(cfg), "--data_path", str(tmp_path), "--dataset", "syn",
              "--tasks", "smb_dis_diff", "--test_task", "smb_dis_diff", "--max_his_len", "8", "--batch_size", "32",
              "--learning_rate", "3e-3", "--output_dir", str(tmp_path / "out"), "--result_dir", str(tmp_path / "res"),
              "--seed", "1"]
    run = lambda extra: subprocess.run([sys.executable, "-m", "gamer_amd.train_rec", *common, *extra], cwd=root, capture_output=True,
                                       text=True, timeout=300)
    r = run(["--epochs", "2"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    losses = [float(l.split(" loss ")[1].split()[0]) for l in r.stdout.splitlines() if " loss " in l]
    assert len(losses) == 2 and losses[1] < losses[0], r.stdout
    sd = torch.load(tmp_path / "out" / "best_model.pth", map_location="cpu")
    fresh = GRU4Rec(GRU4RecConfig(embedding_size=64, hidden_size=64), n_items=sd["item_embedding.weight"].shape[0] - 1)
    fresh.load_state_dict(sd)                          # strict
    res = json.load(open(tmp_path / "res" / "result-smb_dis_diff.json"))
    metrics = "hit@1,hit@5,hit@10,recall@1,recall@5,recall@10,ndcg@5,ndcg@10".split(",")
    assert [e["eval_type"] for e in res] == ["Behavior click", "Behavior cart", "Behavior buy", "Merged Behavior"]
    assert all(all(m in e for m in metrics) for e in res)
    r2 = run(["--only_test"])
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-2000:]
    assert json.load(open(tmp_path / "res" / "result-smb_dis_diff.json")) == res
