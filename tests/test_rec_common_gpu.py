"""gamer_amd.rec_common on the GPU: GatherLinearFn, the shared block under GRU4Rec's dense layer, MBSTR's dot-product head and
(through linear_act_bwd) BERT4Rec's output chain, against the same computation in fp64 torch autograd."""
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


@pytest.mark.parametrize("act,ref_act", [("none", lambda t: t), ("relu", F.relu), ("gelu", F.gelu)])
def test_gather_linear_against_fp64_autograd(act, ref_act):
    from gamer_amd import ops
    from gamer_amd.rec_common import GatherLinearFn
    # H = 8: the smallest multiple of 4 with more than one vector; 12 outputs != 8 inputs; one gathered row per sequence
    g = torch.Generator().manual_seed(8)
    x, w, b = torch.randn(3, 5, 8, generator=g), torch.randn(12, 8, generator=g) / 8 ** 0.5, torch.randn(12, generator=g)
    dout = torch.randn(3, 12, generator=g)
    rows = torch.tensor([0, 7, 14])
    xd, wd, bd = (t.to(DEV).requires_grad_(True) for t in (x, w, b))
    out = GatherLinearFn.apply(xd, rows.to(DEV), wd, bd, ops.ACTIVATIONS[act])
    out.backward(dout.to(DEV))
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
    ref = ref_act(x64.view(-1, 8)[rows] @ w64.t() + b64)
    ref.backward(dout.double())
    # the bar test_gru4rec_gpu.py::test_gru_layer_against_fp64_torch holds _GRULayerFn to on the same fp32 GEMM path (its L <= 20
    # cases: reductions no longer than these): max error below 1e-5 of the largest reference value
    for name, a, r in (("out", out, ref), ("dx", xd.grad, x64.grad), ("dw", wd.grad, w64.grad), ("db", bd.grad, b64.grad)):
        print(f"{act}: {name} {_rel(a, r):.2e}")
        assert a.shape == r.shape and _rel(a, r) < 1e-5, (name, _rel(a, r))
    rest = torch.ones(15, dtype=torch.bool)
    rest[rows] = False
    assert float(xd.grad.view(15, 8)[rest.to(DEV)].abs().max()) == 0            # the twelve rows not gathered: exactly zero
