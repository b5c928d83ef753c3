"""CPU side of tests/test_rowwise_paths_gpu.py: the case lists, the inputs, the fp64 references and a plain fp32 restatement
of the cross entropy and of the AdamW update in the kernels' operation order.

Nothing here touches the GPU or imports gamer_amd.  `python tests/helpers/rowwise_ref.py` runs the fp32 restatements over every
listed case against the fp64 references and prints the worst value of each elementwise metric: the numbers quoted in the
docstring of the test module, from which its bars are taken (four times the worst value, see there).
"""
import math

import torch

IGN = -100
F32, F64, BF = torch.float32, torch.float64, torch.bfloat16

# ---------------------------------------------------------------------------------------------------------------------------
# cross entropy
# ---------------------------------------------------------------------------------------------------------------------------
CE_VS = (1, 3, 4, 5, 8, 9, 64, 255, 256, 257, 1041, 1279, 1280, 1281, 1535, 1536, 1537, 4099)
CE_LAYOUTS = ("a", "b", "c")
CE_TEMPS = (0.7, 1.0, 2.0)
# (6, 7): 36 rows with a target, the smallest number of sequences of 7 that holds every planted row of a case at once; the
# shorter shapes take a window of the list that moves with the case (see ce_case)
CE_SHAPES = ((2, 3), (5, 7), (1, 1), (6, 7))
CE_LOOP_SHAPES = ((1025, 8), (4100, 8))          # T = 8200: the reduce kernel's unrolled loop; T = 32800 > 32768: row grid-stride
# (name, count_dev given, denom_host, dloss, dloss_dev)
CE_BWD_VARIANTS = (("count_dev", True, 0.0, 1.0, None), ("denom_host", False, 123.0, 1.0, None),
                   ("dloss", True, 0.0, 0.37, None), ("dloss_dev", True, 0.0, 1.0, 2.5))


def ce_epl(dtype):
    """elements per 16 bytes"""
    return 4 if dtype == F32 else 8


def ce_ldl(V, layout):
    return V if layout == "a" else (V + 15) // 16 * 16 + 16


def ce_paths(dtype, V, layout):
    """(forward path, backward path) that gamer_ce_fwd / gamer_ce_bwd take: "vec" = the row in registers as 16-byte groups,
    "reg" = the row in registers one value at a time, "stream" = two passes over memory, "scalar" = the backward's plain loop."""
    epl = ce_epl(dtype)
    vec = layout != "c" and ce_ldl(V, layout) % epl == 0 and V <= 64 * epl * (5 if dtype == F32 else 3)
    return ("vec" if vec else "reg" if V <= 1280 else "stream"), ("vec" if vec else "scalar")


def ce_planted_columns(V, dtype):
    epl = ce_epl(dtype)
    last = (V - 1) // epl * epl                     # first column of the last 16-byte group
    return sorted({c for c in (0, 1, epl - 1, epl, 63, 64, 255, 256, last, last - 1, V - 2, V - 1) if 0 <= c < V})


def ce_row_specs(V, dtype):
    """(logits, label) recipes of the rows that are not plain random: labels that must act as ignored, the three special rows,
    and the planted rows - peak and target in the same column, then apart."""
    specs = [("rand", "ignore"), ("rand", "-1"), ("rand", "V"), ("rand", "V+5"), ("equal", None), ("big", None), ("ninf", None)]
    cols = ce_planted_columns(V, dtype)
    specs += [("same", c) for c in cols]
    if V > 1:
        specs += [("apart", c) for c in cols]
    return specs


class CeCase:
    """One forward input: x [T, V] (values of `dtype`, held as fp32), labels [B, S], and the buffer layout."""

    def __init__(self, dtype, V, layout, B, S, x, labels):
        self.dtype, self.V, self.layout, self.B, self.S, self.T = dtype, V, layout, B, S, B * S
        self.x, self.labels = x, labels
        self.ldl = ce_ldl(V, layout)
        self.off = 1 if layout == "c" else 0
        tgt = torch.nn.functional.pad(labels, (0, 1), value=IGN)[:, 1:].reshape(-1)
        self.valid = (tgt != IGN) & (tgt >= 0) & (tgt < V)
        self.tgt = torch.where(self.valid, tgt, torch.zeros_like(tgt))
        self.count = int(self.valid.sum())

    def flat(self):
        """The whole allocation as the kernel's caller holds it: NaN wherever no logit lives (padding columns, the element in
        front of a moved base and the tail behind it)."""
        n = self.off + self.T * self.ldl + (7 if self.layout == "c" else 0)
        buf = torch.full((n,), float("nan"), dtype=self.dtype)
        self.rows(buf)[:, :self.V] = self.x.to(self.dtype)
        return buf

    def rows(self, flat):
        return flat[self.off:self.off + self.T * self.ldl].view(self.T, self.ldl)

    def scaled(self, temp):
        """The bits the forward must leave: x * float32(1 / temp), rounded once to the activation type."""
        inv = torch.tensor(1.0, dtype=F32) / torch.tensor(temp, dtype=F32)
        return (self.x * inv).to(self.dtype)


def ce_case(dtype, V, layout, B, S, seed, plain=False, all_ignored=False):
    g = torch.Generator().manual_seed(seed)
    T = B * S
    x = torch.randn(T, V, generator=g) * 3
    labels = torch.randint(0, V, (B, S), generator=g)
    if plain:                                       # the loop shapes: random rows, one label in 16 not a target
        bad = torch.tensor([IGN, -1, V, V + 5])[torch.randint(0, 4, (B, S), generator=g)]
        labels = torch.where(torch.randint(0, 16, (B, S), generator=g) == 0, bad, labels)
    else:
        specs = ce_row_specs(V, dtype)
        slots = [(b, s) for b in range(B) for s in range(S - 1)]          # rows with a target: labels[b][s + 1]
        if len(slots) < len(specs):
            rot = seed % len(specs)
            specs = specs[rot:] + specs[:rot]
            # ... and the last row with a target stays random with its SMALLEST logit as the target (loss >= log V): a window of
            # peak-is-target rows alone has a loss sum of a few 1e-4, and 1e-4 relative of that is 1e-8 absolute on lse - z_t at
            # lse ~ 10 - below what fp32 resolves, whatever the kernel
            if slots:
                (b, s), slots = slots[-1], slots[:-1]
                labels[b, s + 1] = int(x[b * S + s].argmin())
        for (b, s), (kind, arg) in zip(slots, specs):
            t = b * S + s
            if kind == "rand":
                labels[b, s + 1] = {"ignore": IGN, "-1": -1, "V": V, "V+5": V + 5}[arg]
            elif kind == "equal":
                x[t] = 1.5
            elif kind == "big":
                x[t, 0], x[t, V - 1] = 3e4, -3e4
                if V == 1:
                    x[t, 0] = 3e4
            elif kind == "ninf":
                if V > 1:
                    x[t, (int(labels[b, s + 1]) + 1) % V] = float("-inf")
            else:
                x[t] = torch.randn(V, generator=g) * 0.5
                peak = arg if kind == "same" else (arg + V // 2) % V
                x[t, peak] = float("-inf")
                x[t, peak] = x[t].max() + 20.0 if V > 1 else 20.0
                labels[b, s + 1] = arg
    if all_ignored:
        labels = torch.tensor([IGN, -1, V, V + 5])[torch.randint(0, 4, (B, S), generator=g)]
    return CeCase(dtype, V, layout, B, S, x.to(dtype).float(), labels)


def ce_cases(dtype, V, layouts=CE_LAYOUTS):
    """Every (case, temperature) of one (dtype, V)."""
    for li, layout in enumerate(layouts):
        for si, (B, S) in enumerate(CE_SHAPES):
            for ti, temp in enumerate(CE_TEMPS):
                yield ce_case(dtype, V, layout, B, S, seed=1000 * V + 100 * li + 10 * si + ti), temp
        yield ce_case(dtype, V, layout, 5, 7, seed=1000 * V + 100 * li + 99, all_ignored=True), 0.7


def ce_ref(z, case):
    """fp64 log-softmax statistics of the scaled logits z [T, V]: lse, max, row loss, and softmax - onehot (zero rows where the
    row has no target)."""
    zd = z.double()
    lse = torch.logsumexp(zd, 1)
    mx = zd.max(1).values
    zt = zd.gather(1, case.tgt[:, None])[:, 0]
    row_loss = torch.where(case.valid, lse - zt, torch.zeros_like(lse))
    onehot = torch.zeros_like(zd)
    onehot[torch.arange(case.T), case.tgt] = 1.0
    onehot = onehot * case.valid[:, None]
    G = (torch.exp(zd - lse[:, None]) - onehot) * case.valid[:, None]
    return lse, mx, row_loss, G, onehot


def ce_gs(temp, denom, dloss, dloss_dev):
    """the backward's scale, fp64, from the fp32 values the kernel is handed"""
    return dloss * (dloss_dev if dloss_dev is not None else 1.0) / (denom * float(torch.tensor(temp, dtype=F32)))


def ce_emu32(z, case, temp, denom, dloss, dloss_dev):
    """The kernels' formulas in plain fp32 torch, same operation order: max, sum of exp(z - max), lse = max + log(sum);
    gradient (exp(z - lse) - onehot) * gs with gs = (dloss / temp) * dloss_dev / denom, rounded to the activation type."""
    zf = z.float()
    mx = zf.max(1).values
    se = torch.exp(zf - mx[:, None]).sum(1, dtype=F32)
    lse = mx + torch.log(se)
    onehot = torch.zeros_like(zf)
    onehot[torch.arange(case.T), case.tgt] = 1.0
    gs = (torch.tensor(dloss, dtype=F32) / torch.tensor(temp, dtype=F32)) * torch.tensor(1.0 if dloss_dev is None else dloss_dev, dtype=F32) \
        / torch.tensor(denom, dtype=F32)
    G = ((torch.exp(zf - lse[:, None]) - onehot) * gs * case.valid[:, None]).to(case.dtype).float()
    return lse, G


def ce_lse_metric(got, ref, lse, mx):
    """|got - ref| of a row's lse (or row loss) over |lse| + |lse - max| + 1: the rounding of max + log(sum) is relative to |lse|,
    that of logf to |log(sum)| = |lse - max|, and a relative error of the sum moves its logarithm by that much absolutely."""
    return float(((got.double() - ref).abs() / (lse.abs() + (lse - mx).abs() + 1.0)).max())


def ce_grad_metric(got, G, onehot, gs):
    """max of |error| / (|ref| + max_row |ref| + |gs| onehot) over the rows with a target.  The last term is the operand that
    cancels at the target column, (p - 1) * gs: in a row whose peak is its target, p - 1 is some 1e-8 and every other entry
    smaller still, so without it the 2^-24 rounding of expf's result alone would be a relative error of order one."""
    ref = G * gs
    scale = ref.abs() + ref.abs().max(1, keepdim=True).values + abs(gs) * onehot
    ok = scale > 0
    if not bool(ok.any()):
        return 0.0
    return float(((got.double() - ref).abs()[ok] / scale[ok]).max())


# ---------------------------------------------------------------------------------------------------------------------------
# sumsq + AdamW
# ---------------------------------------------------------------------------------------------------------------------------
ADAMW_NS = (1, 3, 4, 5, 1023, 1024, 1025, 100003, 4 * 4096 * 256 + 1029)
ADAMW_NPARTIAL = (1, 256, 1024, 4096)
ADAMW_HYPER = dict(lr=0.1, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.5)
# (name, step, max_norm, grad_scale, gradient magnitude): |g| ~ 0.05 per element, so the norm passes 1 from n ~ 400 on; the
# "clip" variants use a gradient large enough to clip at every n
ADAMW_VARIANTS = (("clip_step1", 1, 1.0, 1.0, 50.0), ("noclip_step2", 2, 1e9, 1.0, 0.05), ("maxnorm0_step1000", 1000, 0.0, 1.0, 0.05),
                  ("gradscale_step2", 2, 1.0, 0.125, 50.0), ("zero_grad_step1", 1, 1.0, 1.0, 0.0))


def adamw_decays(n):
    return sorted({d for d in (0, 1, 2, 5, n - 1, n) if 0 <= d <= n})


def adamw_cases(n):
    """(n_decay, variant, n_partial): the full cross for the small sizes; for the two large ones every n_decay and every variant
    at least once (each case moves seven arrays of n elements)."""
    decays = adamw_decays(n)
    if n <= 2048:
        k = 0
        for d in decays:
            for var in ADAMW_VARIANTS:
                for npart in ADAMW_NPARTIAL:
                    yield d, var, npart
    else:
        k = 0
        for d in decays:
            yield d, ADAMW_VARIANTS[k % len(ADAMW_VARIANTS)], ADAMW_NPARTIAL[k % 4]
            k += 1
        for var in ADAMW_VARIANTS:
            yield decays[-2], var, ADAMW_NPARTIAL[k % 4]
            k += 1


def adamw_inputs(n, seed=3):
    g = torch.Generator().manual_seed(seed + n)
    p0 = torch.randn(n, generator=g)
    m0 = torch.randn(n, generator=g) * 0.01
    v0 = torch.rand(n, generator=g) * 1e-4
    gr = torch.randn(n, generator=g)
    big = torch.sign(p0) * (1 + p0.abs())
    return p0, m0, v0, gr, torch.where(big == 0, torch.ones_like(big), big)


def adamw_p0(p0, big, n_decay):
    """|p| >= 1 on the four elements on each side of the decay boundary: a misplaced boundary moves one of them by
    lr * weight_decay = 5 %."""
    p = p0.clone()
    a, b = max(0, n_decay - 4), min(p.numel(), n_decay + 4)
    p[a:b] = big[a:b]
    return p


def _f32(v):
    return float(torch.tensor(v, dtype=F32))


def adamw_ref(p, g, m, v, n_decay, step, max_norm, grad_scale, lr, beta1, beta2, eps, weight_decay):
    """fp64, after oracle.clip_and_adamw: grad_scale, clip_grad_norm_ (with its 1e-6; max_norm = 0: no clipping), then
    torch.optim.AdamW.  Hyperparameters as the fp32 values the kernel receives.  Returns norm, p, m, v and the elementwise scales:
    of m the magnitudes of its two terms, |beta1 m| + |(1 - beta1) g| (they can cancel); of p the magnitude of the decayed
    parameter plus the update formed with that scale of m in place of m (the update inherits m's cancellation); of v itself."""
    lr, beta1, beta2, eps, weight_decay, max_norm, grad_scale = map(_f32, (lr, beta1, beta2, eps, weight_decay, max_norm, grad_scale))
    p, g, m, v = p.double(), g.double() * grad_scale, m.double(), v.double()
    total = torch.sqrt((g * g).sum())
    coef = min(1.0, max_norm / (float(total) + 1e-6)) if max_norm > 0 else 1.0
    g = g * coef
    wd = torch.where(torch.arange(p.numel()) < n_decay, weight_decay, 0.0).double()
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    pd = p * (1.0 - lr * wd)
    m1 = beta1 * m + (1.0 - beta1) * g
    v1 = beta2 * v + (1.0 - beta2) * g * g
    denom = v1.sqrt() / math.sqrt(bc2) + eps
    sm = (beta1 * m).abs() + ((1.0 - beta1) * g).abs()
    return float(total), pd - (lr / bc1) * m1 / denom, m1, v1, pd.abs() + (lr / bc1) * sm / denom, sm, v1.abs()


def adamw_emu32(p, g, m, v, n_decay, step, max_norm, grad_scale, lr, beta1, beta2, eps, weight_decay):
    """adamw_kernel's arithmetic in plain fp32 torch (scalars as fp32 tensors, the kernel's operation order)."""
    t = lambda x: torch.tensor(x, dtype=F32)
    lr, beta1, beta2, eps, weight_decay, max_norm, grad_scale, one = map(t, (lr, beta1, beta2, eps, weight_decay, max_norm, grad_scale, 1.0))
    inv_bc1 = t(1.0 / (1.0 - float(beta1.double()) ** step))
    inv_sqrt_bc2 = t(1.0 / math.sqrt(1.0 - float(beta2.double()) ** step))
    norm = torch.sqrt((g * g).sum(dtype=F32)) * grad_scale
    c = torch.minimum(max_norm / (norm + t(1e-6)), one) if float(max_norm) > 0 else one
    gg = g * (c * grad_scale)
    wd = torch.where(torch.arange(p.numel()) < n_decay, weight_decay, t(0.0))
    x = p * (one - lr * wd)
    m1 = beta1 * m + (one - beta1) * gg
    v1 = beta2 * v + (one - beta2) * gg * gg
    x = x - lr * inv_bc1 * (m1 / (torch.sqrt(v1) * inv_sqrt_bc2 + eps))
    return x, m1, v1


def scaled_err(got, ref, scale):
    """max |got - ref| / scale over the elements with a non-zero scale; the others must be exact"""
    err = (got.double() - ref).abs()
    ok = scale > 0
    assert bool((err[~ok] == 0).all())
    return float((err[ok] / scale[ok]).max()) if bool(ok.any()) else 0.0


# ---------------------------------------------------------------------------------------------------------------------------
def calibrate():
    worst = {}

    def note(k, val):
        worst[k] = max(worst.get(k, 0.0), val)

    for dtype, name in ((F32, "f32"), (BF, "bf16")):
        for V in CE_VS:
            cases = list(ce_cases(dtype, V, layouts=("b",)))          # (the layout does not enter the arithmetic)
            if V == 5:
                cases += [(ce_case(dtype, 5, "b", B, S, seed=7 + B, plain=True), 0.7) for B, S in CE_LOOP_SHAPES]
            for case, temp in cases:
                z = case.scaled(temp)
                lse, mx, row_loss, G, onehot = ce_ref(z, case)
                for _, use_count, denom_host, dloss, dloss_dev in CE_BWD_VARIANTS:
                    denom = float(case.count) if use_count else denom_host
                    if denom == 0:
                        continue
                    lse32, G32 = ce_emu32(z, case, temp, denom, dloss, dloss_dev)
                    note(f"ce_lse_{name}", ce_lse_metric(lse32, lse, lse, mx))
                    note(f"ce_grad_{name}", ce_grad_metric(G32, G, onehot, ce_gs(temp, denom, dloss, dloss_dev)))
    for n in ADAMW_NS:
        p0, m0, v0, gr, big = adamw_inputs(n)
        for n_decay, (_, step, max_norm, gscale, gmag), _ in adamw_cases(n):
            p, g = adamw_p0(p0, big, n_decay), gr * gmag
            _, pr, mr, vr, sp, sm, sv = adamw_ref(p, g, m0, v0, n_decay, step, max_norm, gscale, **ADAMW_HYPER)
            pe, me, ve = adamw_emu32(p, g, m0, v0, n_decay, step, max_norm, gscale, **ADAMW_HYPER)
            note("adamw_p", scaled_err(pe, pr, sp))
            note("adamw_m", scaled_err(me, mr, sm))
            note("adamw_v", scaled_err(ve, vr, sv))
    for k, val in worst.items():
        print(f"{k:14s} worst {val:.3e}   x4 = {4 * val:.3e}")


if __name__ == "__main__":
    calibrate()
