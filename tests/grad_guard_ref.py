"""References for the guard of the training step (include/wavedm.h: wdm_grad_guard and the _guarded optimizer entries).

  norm_f64 / coef_f32     the float64 global norm of a buffer and torch.nn.utils.clip_grad_norm_'s coefficient min(1, max_norm / (norm + 1e-6)) in fp32
  TorchGuarded            the guarded step stated over torch.optim (foreach=False, the caller's device) the way the optimizer tests state the unguarded one
                          (training.torch_optimizer): clip_grad_norm_ gives the scaling, a skipped step is a call that is not made -- with the per-parameter
                          `step` of Adam / RMSprop advanced by one, because the trainer's count advances over a skipped step too
  guarded_step_f64        the same step written out in float64, every rule, for the cases torch cannot state directly (a skipped FIRST step) and for the host tests

Bounds (tests/test_gpu_grad_guard.py): the norm is off by at most 2^-23 relative (exact squares, an fp64 sum of up to 2^28 terms below 2^-25, one rounding to fp32);
the coefficient can differ from torch's by that plus two fp32 roundings, 3 * 2^-23 in all -- a first moment inherits it once, a second moment twice."""
import numpy as np
import torch

from wavedm_amd.training import STATE_NAMES, torch_optimizer

EPS_F32 = np.float32(1e-6)
U = 2.0 ** -23
NORM_TOL = U                       # |norm - ref| <= 2^-23 ref
COEF_SHARE = {"exp_avg": 3 * U, "momentum_buffer": 3 * U, "exp_avg_sq": 6 * U, "max_exp_avg_sq": 6 * U, "square_avg": 6 * U}


def norm_f64(g):
    """2-norm of the buffer in float64, on the host (no flush of subnormals there)."""
    return float(torch.linalg.vector_norm(g.detach().cpu().double()))


def coef_f32(norm, max_norm):
    """The record's coefficient from the record's norm, in fp32 arithmetic: 1 with clipping off, else min(1, max_norm / (norm + 1e-6f)) with torch.clamp's
    treatment of NaN (it stays)."""
    if not max_norm > 0.0:
        return np.float32(1.0)
    with np.errstate(all="ignore"):
        c = np.float32(max_norm) / (np.float32(norm) + EPS_F32)
    return np.float32(1.0) if c > np.float32(1.0) else np.float32(c)


def _advance_step(opt, p):
    """What a skipped call leaves behind in torch's terms: the per-parameter state as its first step creates it, with `step` one further."""
    st, group = opt.state[p], opt.param_groups[0]
    if isinstance(opt, torch.optim.SGD):
        return                                                    # no count; the momentum buffer is created by the first step that runs
    if len(st) == 0:
        st["step"] = torch.tensor(0.0)
        if isinstance(opt, torch.optim.Adam):
            st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(p), torch.zeros_like(p)
            if group["amsgrad"]:
                st["max_exp_avg_sq"] = torch.zeros_like(p)
        else:
            st["square_avg"] = torch.zeros_like(p)
    st["step"] += 1


class TorchGuarded:
    """clip_grad_norm_ + torch.optim + EMAHelper.update over copies of `params` (a list of tensors), with the skip rule."""

    def __init__(self, spec, params, mu, max_norm=0.0, skip_nonfinite=False):
        self.ps = [torch.nn.Parameter(p.detach().clone()) for p in params]
        self.ema = [p.detach().clone() for p in params]
        self.opt = torch_optimizer(spec, self.ps, foreach=False)
        self.mu, self.max_norm, self.skip_nonfinite, self.skipped = float(mu), float(max_norm), bool(skip_nonfinite), 0

    def step(self, grads):
        for p, g in zip(self.ps, grads):
            p.grad = g.detach().clone()
        if self.skip_nonfinite and not all(bool(torch.isfinite(g).all()) for g in grads):
            for p in self.ps:
                _advance_step(self.opt, p)
            self.skipped += 1
            return True
        if self.max_norm > 0.0:
            torch.nn.utils.clip_grad_norm_(self.ps, self.max_norm, foreach=False)
        self.opt.step()
        self.ema = [self.mu * e + (1.0 - self.mu) * p.detach() for e, p in zip(self.ema, self.ps)]
        return False

    def state(self, name, i=0):
        return self.opt.state[self.ps[i]][name]


def fresh_state_f64(rule, p0):
    """{p, ema, <state tensors of the rule>} in float64, as a trainer starts: zeroed state, the shadow equal to the parameters."""
    st = {"p": p0.double().clone(), "ema": p0.double().clone()}
    for k in STATE_NAMES[rule]:
        st[k] = torch.zeros_like(st["p"])
    return st


def guarded_step_f64(rule, st, g, step, h, max_norm=0.0, skip_nonfinite=False, first=None):
    """One guarded call in float64 on the dict of fresh_state_f64, in place.  step: the count of CALLS, from 1 (it enters the bias corrections whether or not
    earlier calls were skipped); h: {lr, betas, eps, weight_decay, alpha, momentum, mu}; first (SGD): this call creates the momentum buffer -- torch's rule, the
    first call that RUNS (default: decided from a buffer that is still all zero, which is what the kernel's beta1 * 0 + g amounts to).
    -> {"norm", "coef", "skip"}."""
    g = g.double()
    norm = float(torch.linalg.vector_norm(g))
    coef = 1.0
    if max_norm > 0.0:
        c = max_norm / (norm + float(EPS_F32))
        coef = 1.0 if c > 1.0 else c
    skip = bool(skip_nonfinite and not np.isfinite(norm))
    if skip:
        return {"norm": norm, "coef": coef, "skip": True}
    p = st["p"]
    g = g * coef                                                  # scaled first: torch scales .grad in place before the optimizer adds weight decay
    if h["weight_decay"] != 0.0:
        g = g + h["weight_decay"] * p
    b1, b2 = h["betas"]
    if rule in ("adam", "amsgrad"):
        st["exp_avg"].mul_(b1).add_(g, alpha=1.0 - b1)
        st["exp_avg_sq"].mul_(b2).add_(g * g, alpha=1.0 - b2)
        v = st["exp_avg_sq"]
        if rule == "amsgrad":
            torch.maximum(st["max_exp_avg_sq"], v, out=st["max_exp_avg_sq"])
            v = st["max_exp_avg_sq"]
        bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
        p.sub_((h["lr"] / bc1) * st["exp_avg"] / (v.sqrt() / bc2 ** 0.5 + h["eps"]))
    elif rule == "rmsprop":
        st["square_avg"].mul_(h["alpha"]).add_(g * g, alpha=1.0 - h["alpha"])
        p.sub_(h["lr"] * g / (st["square_avg"].sqrt() + h["eps"]))
    else:
        buf = st["momentum_buffer"]
        create = (not bool(buf.any())) if first is None else first
        st["momentum_buffer"] = g.clone() if create else buf * h["momentum"] + g
        p.sub_(h["lr"] * st["momentum_buffer"])
    st["ema"] = h["mu"] * st["ema"] + (1.0 - h["mu"]) * p
    return {"norm": norm, "coef": coef, "skip": False}


def hyper(spec, mu):
    return {"lr": spec["lr"], "betas": tuple(spec["betas"]), "eps": spec["eps"], "weight_decay": spec["weight_decay"], "alpha": spec["alpha"],
            "momentum": spec["momentum"], "mu": mu}
