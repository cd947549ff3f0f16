"""Times Engine.refine_posterior against a torch.autograd + torch.optim.Adam implementation of the same ascent on the same device
(profiles/refine_notes.md): the GMVAE at the default sizes (784 pixels, L = 64, K = 10, one hidden layer of 64), 1024 examples x 4
samples x 500 steps.  One warm-up run each, then the two alternate REPEATS times; a host clock around work that ends in a device
synchronise; the medians and the spread are printed.  `python profiles/refine_timing.py [examples steps]`."""
import math
import statistics
import sys
import time

import torch

from gmvae_amd import _lib as L
from gmvae_amd.engine import Engine

B, STEPS = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (1024, 500)
S, N_EVAL, LR, REPEATS = 4, 256, 0.05, 3
e = Engine("gmvae", 784, 64, 10, [64], random_seed=1)
x = (torch.rand(B, 784, device="cuda") < 0.13).to(torch.uint8)
v = e.views()
W = [v[f"decoder_fcnet/linear_{i}/w"] for i in range(2)]
b = [v[f"decoder_fcnet/linear_{i}/b"] for i in range(2)]
pp = v["prior_gmm_fcnet/linear_0/w"] + v["prior_gmm_fcnet/linear_0/b"]
p_mu, p_sg = e._normal_head(pp)
logpi, mu, sigma = e._latent_components(x)
k = torch.argmax(logpi, dim=1) + 10 * torch.arange(B, device="cuda")
mu0, sg0 = mu[k].clone(), sigma[k].clone()
xf = x.float()


def log_joint(z):
    """log p(z) + log p(x|z) of z [B, S, L]: the 10-component prior with y summed out, the Bernoulli decoder."""
    t = (z[:, :, None, :] - p_mu) / p_sg
    comp = -0.5 * (t * t).sum(-1) - torch.log(p_sg).sum(-1) - 0.5 * 64 * math.log(2 * math.pi) - math.log(10)
    lam = torch.relu(z @ W[0] + b[0]) @ W[1] + b[1] + e.hp["gen_bias_init"]
    return torch.logsumexp(comp, dim=2) + (xf[:, None, :] * lam - torch.nn.functional.softplus(lam)).sum(-1)


def torch_refine():
    m, s = mu0.clone().requires_grad_(), sg0.log().requires_grad_()
    opt = torch.optim.Adam([m, s], lr=LR, maximize=True)
    for _ in range(STEPS):
        opt.zero_grad(set_to_none=True)
        z = m[:, None, :] + s.exp()[:, None, :] * torch.randn(B, S, 64, device="cuda")
        (log_joint(z).mean(dim=1) + s.sum(dim=1)).sum().backward()
        opt.step()
        with torch.no_grad():
            s.clamp_(-20.0, 5.0)
    with torch.no_grad():
        ep = torch.randn(B, N_EVAL, 64, device="cuda")
        out = []
        for mm, ss in ((mu0, sg0.log()), (m, s)):
            lw = log_joint(mm[:, None, :] + ss.exp()[:, None, :] * ep) + ss.sum(dim=1, keepdim=True) + 32 * math.log(2 * math.pi) \
                + 0.5 * (ep * ep).sum(-1)
            out.append(lw.mean().item())
    return out


def hip_refine():
    r = e.refine_posterior(x, n_steps=STEPS, n_samples=S, n_eval=N_EVAL, lr=LR)
    return [r["elbo_start"].double().mean().item(), r["elbo_refined"].double().mean().item()]


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


timed(hip_refine), timed(torch_refine)
th, tt = [], []
for _ in range(REPEATS):
    d, oh = timed(hip_refine)
    th.append(d)
    d, ot = timed(torch_refine)
    tt.append(d)
mh, mt = statistics.median(th), statistics.median(tt)
print(f"{B} examples x {S} samples x {STEPS} steps + {N_EVAL} evaluation draws")
print(f"gmvae_refine   {mh:.3f} s (runs {', '.join(f'{t:.3f}' for t in th)}): elbo {oh[0]:.3f} -> {oh[1]:.3f}")
print(f"torch.autograd {mt:.3f} s (runs {', '.join(f'{t:.3f}' for t in tt)}): elbo {ot[0]:.3f} -> {ot[1]:.3f}")
print(f"ratio {mt / mh:.2f}; {mh / max(STEPS + 2 * N_EVAL / S, 1) * 1e6:.1f} us per evaluation of {B * S // 16} panels")
