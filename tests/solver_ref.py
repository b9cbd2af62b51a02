"""Host reference of the sampler's two integrators (wavedm_amd/sampling.py), restated in float64: the DDIM step of
ddm_wavelet.py:497-502 (eta = 0) and the DPM-Solver++(2M) multistep rule with first-order ends, on the reference's grid `seq = range(0, T, T // S)`.

Notation: step k = 0 ... S-1 walks reversed(seq), i = t_k, j = t_{k+1} (-1 behind the last: abar = 1).  abar is the fp32 cumprod the device path uses,
widened; alpha = sqrt(abar), sigma = sqrt(1 - abar), lambda = ln(alpha / sigma).
    x0     = (x_t - eps * sigma_i) / alpha_i
    DDIM   : x_next = alpha_j * x0 + sigma_j * eps
    2M     : x_next = cx * x_t + c0 * x0 + cp * x0_prev,  h = lambda_j - lambda_i,  r = (lambda_i - lambda_{t_{k-1}}) / h,  g = alpha_j * (1 - exp(-h)),
             cx = sigma_j / sigma_i,  c0 = g * (1 + 1 / (2 r)),  cp = -g / (2 r)
A step is second-order iff 1 <= k <= S - 1 - ends; ends = 2 is the shipped rule (the update that lands on t = 0 and the one onto abar = 1 stay DDIM), ends = 1
the textbook one (only the update onto abar = 1, where lambda is infinite, stays first-order).

Also here: an exactly solvable model.  Data x0 ~ N(mu, s^2) gives eps(x, t) = sigma_t (x - alpha_t mu) / (alpha_t^2 s^2 + sigma_t^2), and the
probability-flow ODE keeps every sample's quantile: x_t = alpha_t mu + sqrt(v_t / v_T) (x_T - alpha_T mu), v = alpha^2 s^2 + sigma^2."""
import numpy as np
import torch

SOLVERS = ("ddim", "dpmpp2m")


def abar_table(betas):
    """float64 array A[t + 1] = abar(t), A[0] = 1: the cumprod in fp32 (utils/sampling.py:11-12), widened."""
    b = torch.as_tensor(np.asarray(betas.detach().cpu() if isinstance(betas, torch.Tensor) else betas)).float()
    return (1 - torch.cat([torch.zeros(1), b])).cumprod(dim=0).double().numpy()


def linear_betas(T=1000, beta_start=1e-4, beta_end=2e-2):
    return torch.from_numpy(np.linspace(beta_start, beta_end, T, dtype=np.float64)).float()


def grid(S, T=1000):
    return list(range(0, T, T // S))


def _asl(A, t):
    a = float(A[t + 1])
    al, sg = np.sqrt(a), np.sqrt(1.0 - a)
    return al, sg, (np.log(al / sg) if sg > 0 else np.inf)


def coefficients(seq, betas, solver, ends=2):
    """One entry per step: None (first-order) or (cx, c0, cp) in float64, unrounded."""
    assert solver in SOLVERS
    A, ts, S = abar_table(betas), list(reversed([int(t) for t in seq])), len(seq)
    out = []
    for k in range(S):
        if solver == "ddim" or not 1 <= k <= S - 1 - ends:
            out.append(None)
            continue
        (ai, si, li), (aj, sj, lj), (_, _, lp) = _asl(A, ts[k]), _asl(A, ts[k + 1]), _asl(A, ts[k - 1])
        h = lj - li
        r = (li - lp) / h
        g = aj * (1.0 - np.exp(-h))
        out.append((sj / si, g * (1.0 + 0.5 / r), -g * 0.5 / r))
    return out


def sample(model, x, seq, betas, solver, ends=2, fp32_coefficients=True):
    """The whole-image sampler in float64: model(x, t) -> eps, x a float64 array.  -> (xs, x0_preds) like ddim_sample.  fp32_coefficients: the three 2M
    coefficients and the four DDIM ones rounded to fp32 first, as the device is given them."""
    A, ts, S = abar_table(betas), list(reversed([int(t) for t in seq])), len(seq)
    coef = coefficients(seq, betas, solver, ends)
    rnd = (lambda v: float(np.float32(v))) if fp32_coefficients else float
    xs, x0s = [np.asarray(x, dtype=np.float64)], []
    for k in range(S):
        i, j = ts[k], (ts[k + 1] if k + 1 < S else -1)
        xt = xs[-1]
        eps = np.asarray(model(xt, i), dtype=np.float64)
        if fp32_coefficients:           # sqrt of fp32 scalars in fp32, like compute_alpha's tensors
            ai, si = float(np.sqrt(np.float32(A[i + 1]))), float(np.sqrt(np.float32(1.0) - np.float32(A[i + 1])))
            aj, sj = float(np.sqrt(np.float32(A[j + 1]))), float(np.sqrt(np.float32(1.0) - np.float32(A[j + 1])))
        else:
            (ai, si, _), (aj, sj, _) = _asl(A, i), _asl(A, j)
        x0 = (xt - eps * si) / ai
        if coef[k] is None:
            xn = aj * x0 + sj * eps
        else:
            cx, c0, cp = (rnd(v) for v in coef[k])
            xn = cx * xt + c0 * x0 + cp * x0s[-1]
        x0s.append(x0)
        xs.append(xn)
    return xs, x0s


class GaussianModel:
    """eps of data x0 ~ N(mu, s^2) under the schedule `betas`, and the closed-form solution of its probability-flow ODE."""

    def __init__(self, betas, mu=0.3, s=0.5):
        self.A, self.mu, self.s = abar_table(betas), float(mu), float(s)

    def _av(self, t):
        a = float(self.A[t + 1])
        return np.sqrt(a), np.sqrt(1.0 - a), a * self.s ** 2 + (1.0 - a)

    def __call__(self, x, t):
        al, sg, v = self._av(t)
        return sg * (x - al * self.mu) / v

    def exact(self, x_T, t_T, t):
        """x_t of the trajectory through x_T at t_T."""
        aT, _, vT = self._av(t_T)
        al, _, v = self._av(t)
        return al * self.mu + np.sqrt(v / vT) * (x_T - aT * self.mu)

    def exact_x0(self, x_T, t_T, t):
        """The x0 prediction (x_t - sigma_t eps) / alpha_t on the exact trajectory."""
        al, sg, _ = self._av(t)
        xt = self.exact(x_T, t_T, t)
        return (xt - sg * self(xt, t)) / al


def rel_linf(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def last_step_at_or_above(seq, t_min=160):
    """The step k of the walk over reversed(seq) with the last t_k >= t_min."""
    ts = list(reversed(list(seq)))
    return max(k for k, t in enumerate(ts) if t >= t_min)


def gaussian_errors(S, solver, ends=2, n=4096, seed=0, T=1000):
    """(error of the x0 prediction at the grid's last t >= 160, error of x at t = 0), relative L-inf against the closed form, for S steps."""
    betas = linear_betas(T)
    m = GaussianModel(betas)
    seq = grid(S, T)
    x_T = np.random.default_rng(seed).standard_normal(n)
    xs, x0s = sample(m, x_T, seq, betas, solver, ends=ends, fp32_coefficients=False)
    ts = list(reversed(seq))
    k = last_step_at_or_above(seq)
    assert ts[-1] == 0
    return rel_linf(x0s[k], m.exact_x0(x_T, ts[0], ts[k])), rel_linf(xs[S - 1], m.exact(x_T, ts[0], 0))
