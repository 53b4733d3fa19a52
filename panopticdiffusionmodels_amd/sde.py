"""VP-SDE bookkeeping, ScoreModel and the Euler-Maruyama sampler of sde.py (VPSDE 72-113, ScoreModel 155-199,
ReverseSDE / ODE 202-236, euler_maruyama 243-267).

`ScoreModel.predict` feeds the net `t * 999` (sde.py:174); `noise_pred` is what eval_ldm.py / eval.py hand
to dpm_solver_pytorch.model_wrapper.  `euler_maruyama` here is the reference's loop in plain torch ops: it takes
any callable net, runs on the CPU or the GPU and draws its noise with torch.randn_like in the reference's order.
The fused GPU loop for a U-ViT (one captured step, noise generated on the device) is
sampler.EulerMaruyamaSampler; LSimple (training) is train.py.
"""
import numpy as np
import torch

try:
    from tqdm import tqdm
except ImportError:   # progress bar only (verbose=True); not a dependency
    def tqdm(it, **_kw):
        return it


def stp(s, ts):
    """scalar-tensor product broadcasting s [B] over ts [B, ...] (sde.py:18-22)."""
    if isinstance(s, np.ndarray):
        s = torch.from_numpy(s).type_as(ts)
    return s.view(-1, *([1] * (ts.dim() - 1))) * ts


def mos(a, start_dim=1):
    return a.pow(2).flatten(start_dim=start_dim).mean(dim=-1)


def duplicate(tensor, *size):
    return tensor.unsqueeze(dim=0).expand(*size, *tensor.shape)


class VPSDE:
    """Linear VP-SDE, beta(t) = beta_0 + t (beta_1 - beta_0)."""

    def __init__(self, beta_min=0.1, beta_max=20):
        self.beta_0, self.beta_1 = beta_min, beta_max

    def squared_diffusion(self, t):
        return self.beta_0 + t * (self.beta_1 - self.beta_0)

    def diffusion(self, t):
        return self.squared_diffusion(t) ** 0.5

    def drift(self, x, t):
        return -0.5 * stp(self.squared_diffusion(t), x)

    def squared_diffusion_integral(self, s, t):
        return self.beta_0 * (t - s) + (self.beta_1 - self.beta_0) * (t ** 2 - s ** 2) * 0.5

    def skip_alpha(self, s, t):
        return (-self.squared_diffusion_integral(s, t)).exp()

    def skip_beta(self, s, t):
        return 1. - self.skip_alpha(s, t)

    def cum_alpha(self, t):
        return self.skip_alpha(0, t)

    def cum_beta(self, t):
        return self.skip_beta(0, t)

    def nsr(self, t):
        return self.squared_diffusion_integral(0, t).expm1()

    def snr(self, t):
        return 1. / self.nsr(t)

    def marginal_prob(self, x0, t):
        return stp(self.cum_alpha(t) ** 0.5, x0), self.cum_beta(t) ** 0.5

    def __repr__(self):
        return f'vpsde beta_0={self.beta_0} beta_1={self.beta_1}'

    __str__ = __repr__


class ScoreModel:
    def __init__(self, nnet, pred, sde, T=1):
        assert T == 1
        self.nnet, self.pred, self.sde, self.T = nnet, pred, sde, T

    def predict(self, xt, t, **kwargs):
        if not isinstance(t, torch.Tensor):
            t = torch.tensor(t)
        t = t.to(xt.device)
        if t.dim() == 0:
            t = duplicate(t, xt.size(0))
        return self.nnet(xt, t * 999, **kwargs)

    def noise_pred(self, xt, t, **kwargs):
        pred = self.predict(xt, t, **kwargs)
        if self.pred == 'noise_pred':
            return pred
        if self.pred == 'x0_pred':
            return -stp(self.sde.snr(t).sqrt(), pred) + stp(self.sde.cum_beta(t).rsqrt(), xt)
        raise NotImplementedError(self.pred)

    def x0_pred(self, xt, t, **kwargs):
        pred = self.predict(xt, t, **kwargs)
        if self.pred == 'noise_pred':
            return stp(self.sde.cum_alpha(t).rsqrt(), xt) - stp(self.sde.nsr(t).sqrt(), pred)
        if self.pred == 'x0_pred':
            return pred
        raise NotImplementedError(self.pred)

    def score(self, xt, t, **kwargs):
        return stp(-self.sde.cum_beta(t).rsqrt(), self.noise_pred(xt, t, **kwargs))


class ReverseSDE:
    r"""dx = [f(x, t) - g(t)^2 s(x, t)] dt + g(t) dw   (sde.py:202-217)"""

    def __init__(self, score_model):
        self.sde = score_model.sde  # the forward sde
        self.score_model = score_model

    def drift(self, x, t, **kwargs):
        drift = self.sde.drift(x, t)  # f(x, t)
        diffusion = self.sde.diffusion(t)  # g(t)
        score = self.score_model.score(x, t, **kwargs)
        return drift - stp(diffusion ** 2, score)

    def diffusion(self, t):
        return self.sde.diffusion(t)


class ODE:
    r"""dx = [f(x, t) - 0.5 g(t)^2 s(x, t)] dt   (sde.py:220-236)"""

    def __init__(self, score_model):
        self.sde = score_model.sde  # the forward sde
        self.score_model = score_model

    def drift(self, x, t, **kwargs):
        drift = self.sde.drift(x, t)  # f(x, t)
        diffusion = self.sde.diffusion(t)  # g(t)
        score = self.score_model.score(x, t, **kwargs)
        return drift - 0.5 * stp(diffusion ** 2, score)

    def diffusion(self, t):
        return 0


@torch.no_grad()
def euler_maruyama(rsde, x_init, sample_steps, eps=1e-3, T=1, trace=None, verbose=False, **kwargs):
    r"""The Euler-Maruyama sampler for the reverse SDE / ODE (sde.py:243-267): the grid is
    [0, linspace(eps, T, sample_steps)] walked backwards, the last step (s == 0) adds no noise, **kwargs go to the
    net.  torch.randn_like is called once per step with s != 0, for the ODE too (its sigma is 0), exactly where the
    reference calls it, so the same torch seed draws the same noise."""
    assert isinstance(rsde, ReverseSDE) or isinstance(rsde, ODE)
    timesteps = np.append(0., np.linspace(eps, T, sample_steps))
    timesteps = torch.tensor(timesteps).to(x_init)
    x = x_init
    if trace is not None:
        trace.append(x)
    pairs = list(zip(timesteps, timesteps[1:]))[::-1]
    for s, t in (tqdm(pairs, desc='euler_maruyama') if verbose else pairs):
        drift = rsde.drift(x, t, **kwargs)
        diffusion = rsde.diffusion(t)
        dt = s - t
        mean = x + drift * dt
        sigma = diffusion * (-dt).sqrt()
        x = mean + stp(sigma, torch.randn_like(x)) if s != 0 else mean
        if trace is not None:
            trace.append(x)
    return x
