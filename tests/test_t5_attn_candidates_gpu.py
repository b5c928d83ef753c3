"""gamer_t5_attn_candidates (csrc/t5_candidates.hip), the decoder's cross attention for any number of query rows per user: against a
dense fp64 restatement on the fp32-rounded inputs, against gamer_t5_attn_fwd with its row map on the same tensors, row independence,
repeatability and the refusals.

Bar (that of the T5 attention grid of tests/test_tiger_gpu.py): every case also runs the restatement as fp32 torch ops on the GPU; the
kernel may err by at most twice the restatement's worst relative error over the grid (only the order of the sums differs), and never
by more than 1e-4.  The factor 2 is taken against the grid's worst fp32 torch error, deliberately not the same case's: at Sk = 1 and
for a user without a kept key the fp32 restatement is exact and a per-case bar would be 0.  Relative error = largest absolute
difference over the largest reference magnitude of the tensor."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RS, SKS = (1, 15, 17, 63, 65, 70), (1, 15, 16, 17, 37, 128)
MASKS = ("none", "right", "left", "holes", "single", "empty", "packed")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    from gamer_amd import build
    build.build()


def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _grid():
    """every (R, Sk) pair once and 24 pairs a second time; d, h, B and the masks rotate with different periods so that each value of
    each meets every R and every Sk.  (R, Sk, h, d, B, mask)"""
    cases = []
    for n in range(60):
        R, Sk = RS[n % 6], SKS[(n // 6 + (n // 36) * (n % 6)) % 6]
        d, h, B = (32, 64)[(n // 2) % 2], (1, 3)[(n // 4 + n) % 2], (1, 3)[(n // 3) % 2]
        mask = MASKS[n % 7]
        if mask == "packed" and Sk == 1:
            mask = "none"                                                     # (users of different lengths need Sk > 1)
        cases.append((R, Sk, h, d, B, mask))
    cases += [(70, 37, 3, 64, 3, "packed"), (17, 128, 1, 32, 3, "packed")]
    return cases


def _inputs(R, Sk, h, d, B, mask):
    """(q [B, R, I], k, v [B, Sk, I], keep bool [B, Sk]) on the CPU; packed: keep is a right-padded mask of different lengths"""
    g = torch.Generator().manual_seed(100003 * R + 1009 * Sk + 101 * h + 7 * d + B + MASKS.index(mask))
    I = h * d
    q = torch.randn(B, R, I, generator=g) * (10.0 / d) ** 0.5                 # scores of O(10): T5 does not scale them
    k, v = torch.randn(B, Sk, I, generator=g), torch.randn(B, Sk, I, generator=g)
    keep = torch.ones(B, Sk, dtype=torch.bool)
    for b in range(B):
        n = int(torch.randint(1, Sk + 1, (1,), generator=g))
        if mask == "right":
            keep[b, n:] = False
        elif mask == "left":
            keep[b, :Sk - n] = False
        elif mask in ("holes", "single", "empty"):
            keep[b] = torch.rand(Sk, generator=g) < 0.6
            keep[b, int(torch.randint(0, Sk, (1,), generator=g))] = True
        elif mask == "packed":
            keep[b, (Sk, max(1, Sk // 2), max(1, Sk - 3))[b % 3]:] = False
    if mask == "single":
        keep[B - 1] = False
        keep[B - 1, int(torch.randint(0, Sk, (1,), generator=g))] = True      # one user with a single kept key
    if mask == "empty":
        keep[B - 1] = False                                                   # one user with no kept key
    return q, k, v, keep


def _dense(q, k, v, keep, h, d, dtype, dev):
    B, R, I = q.shape
    heads = lambda x: x.to(dev).to(dtype).view(B, x.shape[1], h, d).permute(0, 2, 1, 3)
    s = heads(q) @ heads(k).transpose(-1, -2)
    s = s.masked_fill(~keep.to(dev)[:, None, None, :], float("-inf"))
    mx = s.amax(-1, keepdim=True)
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
    e = torch.exp(s - mx)
    p = e / e.sum(-1, keepdim=True).clamp_min(1e-300 if dtype == torch.float64 else 1e-37)
    return (p @ heads(v)).permute(0, 2, 1, 3).reshape(B * R, I)


def _run(q, k, v, keep, h, d, mask, old=False):
    """the kernel (or, ``old``, gamer_t5_attn_fwd / _packed_fwd with one query per row and the row -> user map) on the device"""
    from gamer_amd import ops
    B, R, I = q.shape
    Sk = k.shape[1]
    qd = q.reshape(B * R, I).to(DEV)
    if mask == "packed":
        lens = keep.sum(1)
        rows = keep.reshape(-1).nonzero()[:, 0]
        kvb = torch.cat([k, v], 2).reshape(B * Sk, 2 * I)[rows].contiguous().to(DEV)      # column blocks of one k|v buffer
        k_off, keepd = ops.T5Offsets.from_lengths(lens, DEV), None
    else:
        kvb = torch.cat([k, v], 2).reshape(B * Sk, 2 * I).to(DEV)
        k_off, keepd = None, (None if mask == "none" else keep.to(torch.uint8).to(DEV))
    kd, vd = kvb[:, :I], kvb[:, I:]
    o = torch.full((B * R, I), float("nan"), device=DEV)
    if not old:
        ops.t5_attn_candidates(qd, kd, vd, keepd, B, R, Sk, h, d, o, k_off=k_off)
    else:
        N = B * R
        kv_rows = (torch.arange(N, dtype=torch.int32, device=DEV) // R).contiguous()
        lse = torch.empty(N, h, 1, device=DEV)
        if k_off is not None:
            ops.t5_attn_packed_fwd(qd, kd, vd, None, ops.T5Offsets.uniform(N, 1, DEV), k_off, N, 1, Sk, h, d, False, 0.0, 0, o, lse,
                                   kv_rows=kv_rows, kv_batch=B)
        else:
            ops.t5_attn_fwd(qd, kd, vd, None, keepd, N, 1, Sk, h, d, False, 0.0, 0, o, lse, kv_rows=kv_rows, kv_batch=B)
    torch.cuda.synchronize()
    return o


@pytest.fixture(scope="module")
def grid():
    """[(case, kernel error, fp32 torch error, kernel vs gamer_t5_attn_fwd, bit-equal to it)] over the grid, computed once"""
    rows = []
    for case in _grid():
        R, Sk, h, d, B, mask = case
        q, k, v, keep = _inputs(*case)
        ref = _dense(q, k, v, keep, h, d, torch.float64, "cpu")
        t32 = _dense(q, k, v, keep, h, d, torch.float32, DEV)
        got, old = _run(q, k, v, keep, h, d, mask), _run(q, k, v, keep, h, d, mask, old=True)
        assert not bool(torch.isnan(got).any()), case                         # (the output was poisoned with NaN before the launch)
        if mask == "empty":
            assert float(got.view(B, R, -1)[B - 1].abs().max()) == 0.0, case  # the user with no kept key: exactly 0
        rows.append((case, _rel(got, ref), _rel(t32, ref), _rel(got, old), bool(torch.equal(got, old))))
    return rows


def test_against_fp64_within_twice_the_fp32_torch_error(grid):
    assert 55 <= len(grid) <= 65
    worst_kernel, worst_torch = max(r[1] for r in grid), max(r[2] for r in grid)
    print(f"t5_attn_candidates vs fp64: kernel worst {worst_kernel:.3e}  fp32 torch worst {worst_torch:.3e}  ({len(grid)} cases)")
    for case, ek, et, _, _ in grid:
        assert ek <= 2.0 * worst_torch and ek <= 1e-4, (case, ek, worst_torch)


def test_against_the_resident_kernel_with_its_row_map(grid):
    worst_torch = max(r[2] for r in grid)
    worst = max(r[3] for r in grid)
    print(f"t5_attn_candidates vs t5_attn_fwd(kv_rows): worst {worst:.3e}; bit-equal in {sum(r[4] for r in grid)} of {len(grid)} cases")
    for case, _, _, eo, _ in grid:
        assert eo <= 2.0 * worst_torch and eo <= 1e-4, (case, eo)


def test_the_grid_covers_every_value():
    cases = _grid()
    assert {c[0] for c in cases} == set(RS) and {c[1] for c in cases} == set(SKS)
    assert {(c[0], c[1]) for c in cases} >= {(R, Sk) for R in RS for Sk in SKS}
    assert {(c[3], c[2], c[4]) for c in cases} == {(d, h, B) for d in (32, 64) for h in (1, 3) for B in (1, 3)}
    assert {c[5] for c in cases} == set(MASKS)
    for R in RS:
        assert {c[3] for c in cases if c[0] == R} == {32, 64} and len({c[5] for c in cases if c[0] == R}) >= 5
    for Sk in SKS:
        assert {c[3] for c in cases if c[1] == Sk} == {32, 64} and {c[4] for c in cases if c[1] == Sk} == {1, 3}
    packed = [c for c in cases if c[5] == "packed"]
    assert len(packed) >= 2
    for c in packed:
        keep = _inputs(*c)[3]
        assert c[4] == 1 or len(set(keep.sum(1).tolist())) > 1               # users of different lengths
    assert any(c[4] == 3 for c in packed)


@pytest.mark.parametrize("d,mask", [(64, "holes"), (32, "packed")])
def test_a_row_alone_has_the_bits_it_has_among_70(d, mask):
    case = (70, 37, 3, d, 3, mask)
    q, k, v, keep = _inputs(*case)
    whole = _run(q, k, v, keep, 3, d, mask).view(3, 70, -1)
    alone = _run(q[1:2, 3:4].clone(), k[1:2], v[1:2], keep[1:2], 3, d, mask)
    assert torch.equal(alone[0], whole[1, 3])
    assert torch.equal(whole.reshape(210, -1), _run(q, k, v, keep, 3, d, mask))          # two calls: the same bits


def test_refusals_name_the_entry_point_and_the_process_goes_on():
    from gamer_amd import _lib, ops
    lib = _lib.load()

    def call(R, Sk, h, d, misalign=False):
        I = h * d
        q = torch.zeros(R * I + 4, device=DEV)
        q = (q[1:1 + R * I] if misalign else q[:R * I]).view(R, I)
        kv = torch.zeros(Sk, 2 * I, device=DEV)
        o = torch.full((R, I), float("nan"), device=DEV)
        ops.t5_attn_candidates(q, kv[:, :I], kv[:, I:], None, 1, R, Sk, h, d, o)
        torch.cuda.synchronize()
        return o

    for kw in (dict(Sk=129, h=2, d=32), dict(Sk=16, h=1, d=48), dict(Sk=16, h=17, d=32), dict(Sk=16, h=2, d=32, misalign=True)):
        with pytest.raises(RuntimeError, match="gamer_t5_attn_candidates"):
            call(5, **kw)
        assert b"gamer_t5_attn_candidates" in lib.gamer_last_error(), kw
    assert float(call(5, 16, 2, 32).abs().max()) == 0.0                       # v = 0: the next good call runs
    with pytest.raises(RuntimeError, match="device"):
        ops.t5_attn_candidates(torch.zeros(5, 64), torch.zeros(16, 64), torch.zeros(16, 64), None, 1, 5, 16, 2, 32, torch.zeros(5, 64))
