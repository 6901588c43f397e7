"""Shared by tests/test_optimizer_host.py and tests/test_optimizer_gpu.py: the input recipe of the optimizer tests, a float64
model of torch's Adam and SGD update rules, and the error measures the parity bar is stated in.

The model follows torch's single-tensor rules operation by operation (torch/optim/adam.py `_single_tensor_adam`,
torch/optim/sgd.py `_single_tensor_sgd`), in float64 on the fp32 inputs:

    Adam   g' = g + wd p;  m += (g' - m)(1 - b1);  v = b2 v + (1 - b2) g'^2;
           p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)          t: this tensor's own step count
    SGD    g' = g + wd p;  buf = g' on the tensor's first step, else mu buf + (1 - dampening) g';
           p -= lr (g' + mu buf) with Nesterov, else p -= lr buf  (p -= lr g' without momentum)
"""
import functools

import torch

CHUNK = 4096            # elements of one tensor a block of the HIP kernels works on (OPT_CHUNK)
SIZES = [1, 3, 4, 5, 1023, 1025, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7, 70000]
STEPS = 10
LR = 1e-3
LR_FACTOR, LR_DROP_AFTER = 0.2, 5      # lr is multiplied by 0.2 after step 5
NONE_PARAM, NONE_STEPS = 5, (3, 4)     # the 1025-element parameter has grad = None on steps 3 and 4 (1-based)
BETAS, EPS = (0.9, 0.999), 1e-8


def lr_at(step: int) -> float:
    return LR if step <= LR_DROP_AFTER else LR * LR_FACTOR


def params0(sizes=tuple(SIZES), seed=0):
    gen = torch.Generator().manual_seed(1000 + seed)
    return [torch.randn(n, generator=gen, dtype=torch.float32) for n in sizes]


def grads(step: int, sizes=tuple(SIZES), seed=0):
    """Seeded fp32 gradients with magnitudes log-uniform over 1e-8 .. 1e2 and random signs: sqrt(v) crosses eps = 1e-8."""
    gen = torch.Generator().manual_seed(7919 * step + seed)
    out = []
    for n in sizes:
        mag = torch.pow(10.0, torch.rand(n, generator=gen, dtype=torch.float64) * 10.0 - 8.0)
        sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
        out.append((mag * sign).float())
    return out


class Adam64:
    def __init__(self, params, betas=BETAS, eps=EPS, weight_decay=0.0):
        self.p = [p.detach().double().clone() for p in params]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        self.t = [0] * len(self.p)
        self.betas, self.eps, self.wd = betas, eps, weight_decay

    def step(self, grads_, lr):
        b1, b2 = self.betas
        for i, g in enumerate(grads_):
            if g is None:
                continue
            g = g.detach().double()
            self.t[i] += 1
            t = self.t[i]
            if self.wd != 0:
                g = g + self.wd * self.p[i]
            self.m[i] = self.m[i] + (g - self.m[i]) * (1 - b1)
            self.v[i] = self.v[i] * b2 + (1 - b2) * g * g
            step_size = lr / (1 - b1 ** t)
            denom = self.v[i].sqrt() / (1 - b2 ** t) ** 0.5 + self.eps
            self.p[i] = self.p[i] - step_size * (self.m[i] / denom)

    def states(self):
        return {"exp_avg": self.m, "exp_avg_sq": self.v}


class Sgd64:
    def __init__(self, params, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
        self.p = [p.detach().double().clone() for p in params]
        self.buf = [None] * len(self.p)
        self.mu, self.damp, self.wd, self.nesterov = momentum, dampening, weight_decay, nesterov

    def step(self, grads_, lr):
        for i, g in enumerate(grads_):
            if g is None:
                continue
            g = g.detach().double()
            if self.wd != 0:
                g = g + self.wd * self.p[i]
            if self.mu != 0:
                self.buf[i] = g.clone() if self.buf[i] is None else self.mu * self.buf[i] + (1 - self.damp) * g
                g = g + self.mu * self.buf[i] if self.nesterov else self.buf[i]
            self.p[i] = self.p[i] - lr * g

    def states(self):
        return {"momentum_buffer": self.buf} if self.mu != 0 else {}


def schedule(step: int, sizes=tuple(SIZES), seed=0):
    """(lr, gradients) of step 1 .. STEPS of the shared scenario; None for the parameter that sits a step out."""
    gs = grads(step, sizes, seed)
    if len(gs) > NONE_PARAM and step in NONE_STEPS:
        gs[NONE_PARAM] = None
    return lr_at(step), gs


def run_torch_like(make_opt, device, sizes=tuple(SIZES), seed=0, steps=STEPS):
    """The scenario through a torch.optim-style optimizer: (parameters, {state name: list of tensors}) on the CPU."""
    ps = [torch.nn.Parameter(p.to(device)) for p in params0(sizes, seed)]
    opt = make_opt(ps)
    for s in range(1, steps + 1):
        lr, gs = schedule(s, sizes, seed)
        for group in opt.param_groups:
            group["lr"] = lr
        for p, g in zip(ps, gs):
            p.grad = None if g is None else g.to(device)
        opt.step()
    names = [k for k in ("exp_avg", "exp_avg_sq", "momentum_buffer") if k in opt.state[ps[0]]]
    return [p.detach().cpu() for p in ps], {k: [opt.state[p][k].detach().cpu() for p in ps] for k in names}


def run_model64(kind: str, sizes=tuple(SIZES), seed=0, steps=STEPS, **hyper):
    model = (Adam64 if kind == "adam" else Sgd64)(params0(sizes, seed), **hyper)
    for s in range(1, steps + 1):
        lr, gs = schedule(s, sizes, seed)
        model.step(gs, lr)
    return model.p, model.states()


def p_error(ps, ps64) -> float:
    """Largest |p - p64| in units of the base learning rate."""
    return max(float((p.double() - q).abs().max()) for p, q in zip(ps, ps64)) / LR


def state_error(name: str, ss, ss64) -> float:
    """exp_avg_sq (a sum of non-negative terms): largest element-wise relative error.  exp_avg and momentum_buffer (sums of
    both signs, which cancel): largest error of a tensor relative to that tensor's largest magnitude."""
    worst = 0.0
    for s, q in zip(ss, ss64):
        d = (s.double() - q).abs()
        if name == "exp_avg_sq":
            worst = max(worst, float((d / q.abs().clamp_min(1e-300)).max()))
        else:
            worst = max(worst, float(d.max() / q.abs().max().clamp_min(1e-300)))
    return worst


@functools.lru_cache(maxsize=None)
def reference(kind: str, hyper: tuple):
    """(p64, states64, the errors of torch's own fp32 CPU optimizer (foreach=False) against them): computed once per case."""
    kw = dict(hyper)
    p64, s64 = run_model64(kind, **kw)
    if kind == "adam":
        make = lambda ps: torch.optim.Adam(ps, lr=LR, betas=BETAS, eps=EPS, foreach=False, **kw)
    else:
        make = lambda ps: torch.optim.SGD(ps, lr=LR, foreach=False, **kw)
    pt, st = run_torch_like(make, "cpu")
    errs = {"p": p_error(pt, p64)}
    for k in s64:
        errs[k] = state_error(k, st[k], s64[k])
    return p64, s64, errs


ADAM_CASES = [(("weight_decay", 0.0),), (("weight_decay", 1e-2),)]
SGD_CASES = [(("momentum", mu), ("nesterov", nest), ("weight_decay", wd))
             for mu, nest in ((0.0, False), (0.9, False), (0.9, True)) for wd in (0.0, 1e-2)]
