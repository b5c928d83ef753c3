"""gamer_amd.layer_blocks on the GPU: the post-LN residual step, the dense FFN and the behaviour-grouped FFN against the same
computation in fp64 torch autograd, and rec_common.EmbedDropoutFn's padding id and gradient hand-over.  The bar is
test_rec_common_gpu.py's: max error below 1e-5 of the largest reference value (same fp32 GEMM path, reductions of at most 12
terms)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
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


def _check(tag, pairs):
    for name, a, r in pairs:
        print(f"{tag}: {name} {_rel(a, r):.2e}")
        assert a.shape == r.shape and _rel(a, r) < 1e-5, (tag, name, _rel(a, r))


def _dev(*ts):
    return [t.to(DEV).contiguous() for t in ts]


def test_post_ln_against_fp64_autograd():
    from gamer_amd import layer_blocks as lb
    # T = 5 rows: not a multiple of 4; H = 8: the smallest multiple of 4 with more than one vector
    g = torch.Generator().manual_seed(5)
    x, h, dy = (torch.randn(5, 8, generator=g) for _ in range(3))
    lnw, lnb = torch.rand(8, generator=g) + 0.5, torch.randn(8, generator=g)
    eps = 1e-5
    xd, hd, dyd, wd, bd = _dev(x, h, dy, lnw, lnb)
    y, saved = lb.post_ln_fwd(xd, hd, wd, bd, eps, 0.0, 0)
    dxr, dh, dw, db = lb.post_ln_bwd(dyd, saved, wd, 0.0, 0)
    x64, h64, w64, b64 = (t.double().requires_grad_(True) for t in (x, h, lnw, lnb))
    ref = F.layer_norm(x64 + h64, (8,), w64, b64, eps)
    ref.backward(dy.double())
    _check("post_ln", (("y", y, ref), ("dx_residual", dxr, x64.grad), ("dh", dh, h64.grad), ("dlnw", dw, w64.grad),
                       ("dlnb", db, b64.grad)))


def test_post_ln_with_dropout_is_the_explicit_op_sequence():
    """p = 0.5 under a fixed seed: the block's outputs are bit-equal to residual_dropout_fwd / layernorm_fwd and layernorm_bwd /
    residual_dropout_bwd written out here (the seed and argument plumbing; the mask itself is the ops tests' business)."""
    from gamer_amd import layer_blocks as lb, ops
    g = torch.Generator().manual_seed(6)
    x, h, dy = (torch.randn(5, 8, generator=g) for _ in range(3))
    lnw, lnb = torch.rand(8, generator=g) + 0.5, torch.randn(8, generator=g)
    eps, p, seed = 1e-5, 0.5, 4242
    xd, hd, dyd, wd, bd = _dev(x, h, dy, lnw, lnb)
    y, saved = lb.post_ln_fwd(xd, hd, wd, bd, eps, p, seed)
    dxr, dh, dw, db = lb.post_ln_bwd(dyd, saved, wd, p, seed)
    f32 = dict(dtype=torch.float32, device=DEV)
    v, y2, mean, rstd = torch.empty(5, 8, **f32), torch.empty(5, 8, **f32), torch.empty(5, **f32), torch.empty(5, **f32)
    ops.residual_dropout_fwd(xd, hd, p, seed, None, v)
    ops.layernorm_fwd(v, None, wd, bd, eps, None, y2, mean, rstd)
    dv, dh2 = torch.empty(5, 8, **f32), torch.empty(5, 8, **f32)
    pw, pb = torch.empty(lb._N_PARTIAL, 8, **f32), torch.empty(lb._N_PARTIAL, 8, **f32)
    ops.layernorm_bwd(v, wd, mean, rstd, dyd, dv, pw, pb)
    dw2, db2 = torch.empty(8, **f32), torch.empty(8, **f32)
    ops.colsum_reduce(pw, dw2)
    ops.colsum_reduce(pb, db2)
    ops.residual_dropout_bwd(dv, p, seed, dh2)
    for name, a, r in (("v", saved[0], v), ("y", y, y2), ("dx_residual", dxr, dv), ("dh", dh, dh2), ("dlnw", dw, dw2), ("dlnb", db, db2)):
        assert torch.equal(a, r), name
    dropped = (dh2 == 0) & (dv != 0)
    assert 0 < int(dropped.sum()) < dh2.numel()                                 # the mask was on: some kept, some dropped


@pytest.mark.parametrize("act,ref_act", [("relu", F.relu), ("gelu", F.gelu)])
def test_ffn_against_fp64_autograd(act, ref_act):
    from gamer_amd import layer_blocks as lb, ops
    # dff = 12 != H = 8
    g = torch.Generator().manual_seed(7)
    x, w1, b1 = torch.randn(5, 8, generator=g), torch.randn(12, 8, generator=g) / 8 ** 0.5, torch.randn(12, generator=g)
    w2, b2, df = torch.randn(8, 12, generator=g) / 12 ** 0.5, torch.randn(8, generator=g), torch.randn(5, 8, generator=g)
    xd, w1d, b1d, w2d, b2d, dfd = _dev(x, w1, b1, w2, b2, df)
    with ops.f32_matmul("f32"):
        f, saved = lb.ffn_fwd(xd, w1d, b1d, w2d, b2d, ops.ACTIVATIONS[act])
        dx, dw1, db1, dw2, db2 = lb.ffn_bwd(dfd.clone(), saved, w1d, w2d, ops.ACTIVATIONS[act])
    x64, w164, b164, w264, b264 = (t.double().requires_grad_(True) for t in (x, w1, b1, w2, b2))
    ref = ref_act(x64 @ w164.t() + b164) @ w264.t() + b264
    ref.backward(df.double())
    _check(f"ffn {act}", (("f", f, ref), ("dx", dx, x64.grad), ("dw1", dw1, w164.grad), ("db1", db1, b164.grad),
                          ("dw2", dw2, w264.grad), ("db2", db2, b264.grad)))


def test_grouped_ffn_against_fp64_per_row_loop():
    from gamer_amd import layer_blocks as lb, ops
    B, L, H, dff, b = 2, 5, 8, 12, 3
    g = torch.Generator().manual_seed(9)
    types = torch.tensor([[1, 3, 0, 1, 3], [0, 0, 3, 1, 1]], dtype=torch.int32)          # padding; behaviour 2 has no row
    y, df = torch.randn(B * L, H, generator=g), torch.randn(B * L, H, generator=g)
    w1, b1 = torch.randn(b, dff, H, generator=g) / H ** 0.5, torch.randn(b, dff, generator=g)
    w2, b2 = torch.randn(b, H, dff, generator=g) / dff ** 0.5, torch.randn(b, H, generator=g)
    relu = ops.ACTIVATIONS["relu"]
    yd, dfd, w1d, b1d, w2d, b2d = _dev(y, df, w1, b1, w2, b2)
    lists = lb._TypeLists(types.to(DEV), b)
    perm, grp = lists.perm, dict(groups=b, group_offsets=lists.offsets[1:])
    w1a, w2a = lb._aug_weights(w1d, b1d), lb._aug_weights(w2d, b2d)
    dw1a, dw2a = torch.zeros_like(w1a), torch.zeros_like(w2a)
    with ops.f32_matmul("f32"):
        f, saved = lb.grouped_ffn_fwd(yd, perm, grp, w1a, w2a, relu, torch.zeros(dff, device=DEV))
        dys = lb.grouped_ffn_bwd(dfd, saved, perm, grp, w1a, w2a, relu, dw1a, dw2a)
        once = [t.clone() for t in lb.split_aug_grads(dw1a, dw2a)]
        dys_again = lb.grouped_ffn_bwd(dfd, saved, perm, grp, w1a, w2a, relu, dw1a, dw2a)      # PBAT: the second stream adds
    # fp64: every row through its own expert, padding rows zero
    y64, w164, b164, w264, b264 = (t.double().requires_grad_(True) for t in (y, w1, b1, w2, b2))
    flat = types.flatten().tolist()
    rows = []
    for r, t in enumerate(flat):
        e = t - 1
        rows.append(torch.zeros(H, dtype=torch.float64) if t == 0
                    else w264[e] @ F.relu(w164[e] @ y64[r] + b164[e]) + b264[e])
    ref = torch.stack(rows)
    ref.backward(df.double())
    pad = torch.tensor([t == 0 for t in flat])
    perm_c = perm.cpu()
    assert sorted(perm_c.tolist()) == list(range(B * L))
    _check("grouped_ffn", (("f", f, ref), ("dys", dys, y64.grad[perm_c])))
    assert float(f[pad.to(DEV)].abs().max()) == 0                                # padding rows: exactly zero
    assert float(dys[pad[perm_c].to(DEV)].abs().max()) == 0
    assert torch.equal(dys_again, dys)
    ref_grads = []
    for i in range(b):
        ref_grads += [w164.grad[i], b164.grad[i], w264.grad[i], b264.grad[i]]
    names = [f"{n}[{i}]" for i in range(b) for n in ("dw1", "db1", "dw2", "db2")]
    for name, a, r in zip(names, once, ref_grads):
        if name.endswith("[1]"):                                                 # behaviour 2, no rows: exactly zero
            assert float(a.abs().max()) == 0 and float(r.abs().max()) == 0, name
        else:
            _check("grouped_ffn", ((name, a, r),))
    for name, a, r in zip(names, lb.split_aug_grads(dw1a, dw2a), ref_grads):
        if name.endswith("[1]"):
            assert float(a.abs().max()) == 0, name
        else:
            _check("grouped_ffn twice", ((name, a, 2 * r),))


def test_embed_dropout_pad_id_and_shared_gradient_hand_over():
    from gamer_amd.rec_common import EmbedDropoutFn, _SharedGrad
    g = torch.Generator().manual_seed(10)
    V, D = 6, 8
    E = torch.randn(V, D, generator=g)
    ids_a, ids_b = torch.tensor([[0, 2, 5], [2, 0, 1]]), torch.tensor([[3, 0, 0], [5, 4, 3]])
    da, db = torch.randn(2, 3, D, generator=g), torch.randn(2, 3, D, generator=g)

    def scatter(pairs, skip):
        out = torch.zeros(V, D, dtype=torch.float64)
        for ids, d in pairs:
            keep = ids.flatten() != skip
            out.index_add_(0, ids.flatten()[keep], d.double().reshape(-1, D)[keep])
        return out
    # TIGER's use: no padding row, two gathers share the buffer - the first backward hands it on, the second returns it
    Ed = E.to(DEV).requires_grad_(True)
    shared = _SharedGrad(gathers=2)
    xa = EmbedDropoutFn.apply(ids_a.to(DEV), Ed, 0.0, 1, shared, -1)
    xb = EmbedDropoutFn.apply(ids_b.to(DEV), Ed, 0.0, 2, shared, -1)
    assert torch.equal(xa.cpu(), E[ids_a]) and torch.equal(xb.cpu(), E[ids_b])
    first, = torch.autograd.grad(xa, Ed, da.to(DEV), allow_unused=True)
    assert first is None
    second, = torch.autograd.grad(xb, Ed, db.to(DEV))
    ref = scatter([(ids_a, da), (ids_b, db)], skip=-1)
    assert float(ref[0].abs().max()) > 0
    _check("embed pad_id=-1", (("dE", second, ref), ("dE[0]", second[0], ref[0])))
    # the default: row 0 is padding and gets nothing; one gather returns its gradient, with or without a shared buffer
    for shared in (None, _SharedGrad()):
        Ed = E.to(DEV).requires_grad_(True)
        x = EmbedDropoutFn.apply(ids_a.to(DEV), Ed, 0.0, 1, shared)
        dE, = torch.autograd.grad(x, Ed, da.to(DEV))
        _check("embed default", (("dE", dE, scatter([(ids_a, da)], skip=0)),))
        assert float(dE[0].abs().max()) == 0
