"""Float64 yardstick of the optimizer step: ``torch.nn.utils.clip_grad_norm_(norm_type=2)`` followed by torch's
single-tensor AdamW (torch/optim/adamw.py, ``_single_tensor_adamw`` without amsgrad / maximize), restated statement by
statement on float64 CPU tensors — per-parameter step counts, parameters without a gradient skipped (they keep their state
and their step).  tests/test_optim_cpu.py pins it to torch's own float64 run; the GPU tests measure against it.

Also the shared test problem (parameters of every size class, three groups, four steps of gradients whose magnitudes span ten
decades) and the tolerance of the issue: per tensor, ``max|got - fp64| <= 4 * e_ref + 2^-22 * max|tensor|`` with ``e_ref`` the
distance of torch's own fp32 CPU AdamW from this yardstick on the same inputs."""
import math

import torch


class Yardstick:
    """``params``: list of tensors (any dtype; copied to float64); ``groups``: list of dicts with ``params`` (indices into
    the list) and ``lr``, ``betas``, ``eps``, ``weight_decay``; ``max_norm``: ``None`` = no clipping."""

    def __init__(self, params, groups, max_norm=None, skip_nonfinite=False):
        self.p = [t.detach().double().cpu().clone() for t in params]
        self.groups = groups
        self.max_norm = max_norm
        self.skip_nonfinite = skip_nonfinite
        self.m = [None] * len(self.p)
        self.v = [None] * len(self.p)
        self.t = [0] * len(self.p)
        self.total_norm = None
        self.skipped = 0

    def step(self, grads):
        grads = [None if g is None else g.detach().double().cpu() for g in grads]
        present = [g for g in grads if g is not None]
        # clip_grad_norm_'s own definition: the 2-norm of the per-tensor 2-norms
        total = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g, 2.0) for g in present]), 2.0)) \
            if present else 0.0
        self.total_norm = total
        if self.skip_nonfinite and not math.isfinite(total):
            self.skipped += 1
            return
        coef = 1.0
        if self.max_norm is not None:
            coef = self.max_norm / (total + 1e-6)
            coef = 1.0 if coef > 1.0 else coef                    # torch.clamp(max=1.0): a NaN stays
        for grp in self.groups:
            lr, (b1, b2), eps, wd = grp["lr"], grp["betas"], grp["eps"], grp["weight_decay"]
            for i in grp["params"]:
                if grads[i] is None:
                    continue
                g = grads[i] * coef if self.max_norm is not None else grads[i]
                if self.m[i] is None:
                    self.m[i], self.v[i] = torch.zeros_like(self.p[i]), torch.zeros_like(self.p[i])
                self.t[i] += 1
                t = self.t[i]
                self.p[i] = self.p[i] * (1 - lr * wd)
                self.m[i] = self.m[i] + (g - self.m[i]) * (1 - b1)
                self.v[i] = self.v[i] * b2 + (1 - b2) * g * g
                denom = self.v[i].sqrt() / ((1 - b2 ** t) ** 0.5) + eps
                self.p[i] = self.p[i] - (lr / (1 - b1 ** t)) * (self.m[i] / denom)

    def snapshot(self):
        return dict(p=[t.clone() for t in self.p], m=[None if t is None else t.clone() for t in self.m],
                    v=[None if t is None else t.clone() for t in self.v], t=list(self.t), norm=self.total_norm)


def run_torch(params, groups, grads_per_step, max_norm, dtype):
    """torch's own CPU run in ``dtype``: ``clip_grad_norm_`` + ``torch.optim.AdamW(foreach=False)`` -> one snapshot (as
    ``Yardstick.snapshot``, float64 copies) per step."""
    ps = [torch.nn.Parameter(t.detach().to(dtype).cpu().clone()) for t in params]
    opt = torch.optim.AdamW([dict(g, params=[ps[i] for i in g["params"]]) for g in groups], foreach=False)
    out = []
    for grads in grads_per_step:
        for p, g in zip(ps, grads):
            p.grad = None if g is None else g.detach().to(dtype).cpu().clone()
        norm = None
        if max_norm is not None:
            norm = torch.nn.utils.clip_grad_norm_([p for p in ps if p.grad is not None], max_norm, norm_type=2, foreach=False)
        opt.step()
        st = [opt.state.get(p, {}) for p in ps]
        out.append(dict(p=[p.detach().double().clone() for p in ps],
                        m=[s["exp_avg"].double().clone() if "exp_avg" in s else None for s in st],
                        v=[s["exp_avg_sq"].double().clone() if "exp_avg_sq" in s else None for s in st],
                        t=[int(s["step"]) if "step" in s else 0 for s in st], norm=None if norm is None else float(norm)))
    return out


def run_yardstick(params, groups, grads_per_step, max_norm, skip_nonfinite=False):
    y = Yardstick(params, groups, max_norm, skip_nonfinite)
    out = []
    for grads in grads_per_step:
        y.step(grads)
        out.append(y.snapshot())
    return out


def log_uniform_grad(shape, gen, lo=1e-8, hi=1e2):
    """Signs at random, magnitudes log-uniform in [lo, hi], drawn per element."""
    n = int(torch.Size(shape).numel())
    mag = torch.exp(torch.rand(n, generator=gen, dtype=torch.float64) * (math.log(hi) - math.log(lo)) + math.log(lo))
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    return (mag * sign).float().reshape(shape)


# numel classes of the update kernel: below / at / above a 16-byte lane, the 4096-element block and its neighbours, two
# blocks and a tail; a matrix; 300 jobs of 1 .. 7 elements (the job search); an empty tensor
SIZES = [(1,), (3,), (4,), (5,), (4095,), (4096,), (4097,), (2 * 4096 + 13,), (256, 256)]
GROUP_HYPER = [dict(lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01),
               dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1),      # a dropped term shows here
               dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)]
STEPS = 4


def make_problem(seed=0, small=300):
    """-> dict(shapes, params (fp32 CPU), groups (with ``params`` = indices), grads (STEPS lists; ``None`` = no gradient),
    names).  Index ``view`` is the bias to be laid out at a 4-byte offset of a flat buffer, ``empty`` the zero-element
    parameter, ``sometimes`` the parameter without a gradient on steps 2 and 3, ``zero`` the one whose gradient is all zero."""
    gen = torch.Generator().manual_seed(seed)
    shapes = list(SIZES) + [(64,), (0,), (37,), (129,)]
    special = dict(view=len(SIZES), empty=len(SIZES) + 1, sometimes=len(SIZES) + 2, zero=len(SIZES) + 3)
    shapes += [(1 + int(k) % 7,) for k in torch.randperm(small, generator=gen).tolist()]
    params = [torch.randn(s, generator=gen) for s in shapes]
    groups = [dict(GROUP_HYPER[k], params=[i for i in range(len(shapes)) if i % 3 == k]) for k in range(3)]
    grads = []
    for step in range(STEPS):
        gs = [log_uniform_grad(s, gen) for s in shapes]
        gs[special["zero"]] = torch.zeros(shapes[special["zero"]])
        if step in (1, 2):
            gs[special["sometimes"]] = None
        grads.append(gs)
    return dict(shapes=shapes, params=params, groups=groups, grads=grads, special=special)


def bound(ref32, ref64, key, i):
    """The issue's bound for tensor ``i`` of kind ``key`` (``p`` / ``m`` / ``v``) at one step: ``4 * e_ref + 2^-22 * max|t|``
    (absolute, per tensor), ``e_ref = max|torch fp32 - fp64|`` over the FINITE elements of the fp64 result."""
    a, b = ref32[key][i], ref64[key][i]
    if b is None or b.numel() == 0:
        return 0.0, 0.0
    ok = torch.isfinite(b)
    if not bool(ok.any()):
        return 0.0, 0.0
    e_ref = float((a[ok] - b[ok]).abs().max())
    return 4 * e_ref + 2.0 ** -22 * float(b[ok].abs().max()), e_ref


def check_snapshot(got, ref32, ref64, what, lines=None):
    """``got``: dict(p, m, v, t) of lists (tensors on any device / dtype).  Asserts the step counts exactly and every tensor
    within ``bound``; returns (and appends to ``lines``) the worst ratio ``max|got - fp64| / e_ref`` per kind."""
    assert list(got["t"]) == list(ref64["t"]), f"{what}: step counts {got['t'][:12]} ... != {ref64['t'][:12]} ..."
    worst = {}
    for key in ("p", "m", "v"):
        for i, want in enumerate(ref64[key]):
            g = got[key][i]
            if want is None:
                assert g is None or not bool(g.abs().sum() != 0), f"{what}: {key}[{i}] has a state torch does not have"
                continue
            if want.numel() == 0:
                continue
            g = g.detach().double().cpu().reshape(want.shape)
            ok = torch.isfinite(want)
            assert torch.equal(torch.isnan(g), torch.isnan(ref32[key][i])), f"{what}: {key}[{i}] NaN mask differs from torch fp32's"
            if not bool(ok.any()):
                continue
            err = float((g[ok] - want[ok]).abs().max())
            b, e_ref = bound(ref32, ref64, key, i)
            ratio = err / e_ref if e_ref > 0 else (0.0 if err == 0 else float("inf"))
            if e_ref > 0 or err > 0:
                worst[key] = max(worst.get(key, 0.0), ratio if math.isfinite(ratio) else 0.0)
            assert err <= b, f"{what}: {key}[{i}] {tuple(want.shape)}: max|hip - fp64| {err:.3e} > 4 * {e_ref:.3e} + 2^-22 * max = {b:.3e}"
    line = f"{what}: max|hip - fp64| / e_ref  p {worst.get('p', 0):.2f}  exp_avg {worst.get('m', 0):.2f}  exp_avg_sq {worst.get('v', 0):.2f}"
    print(line)
    if lines is not None:
        lines.append(line)
    return worst
