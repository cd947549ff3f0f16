"""Conditional distributions: MLP -> distribution (mirror of scripts/base.py).

Same class names, constructor arguments and methods as the reference
(``ConditionalNormal`` scripts/base.py:15-83, ``ConditionalBernoulli``
scripts/base.py:86-146, ``ConditionalCategorical`` scripts/base.py:149-209).
The MLP runs in the HIP library (Engine.mlp -> gmvae_mlp_forward); the light
distribution objects below play the role of the tfd.* objects the reference
returns and are used only by the forward-only auxiliary methods.  The training
loss does not go through them: it is the fused gmvae_step.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn.functional as F

from . import _lib as L

TINY = 1.1754943508222875e-38


def activation_name(fn) -> str:
    """hidden_activation_fn (scripts/base.py:19,90,153: any callable; the factories pass ONE to every network, gmvae.py:282,
    vae.py:196) -> the kind the kernels implement: relu (the reference's default tf.nn.relu), tanh, sigmoid, elu.  A name
    or the torch / torch.nn.functional callable; anything else raises (an arbitrary Python callable cannot run in a kernel)."""
    if fn is None:
        return "relu"
    table = {"relu": (torch.relu, F.relu), "tanh": (torch.tanh, F.tanh), "sigmoid": (torch.sigmoid, F.sigmoid), "elu": (F.elu,)}
    for name, fns in table.items():
        # by NAME only for the libraries' own functions (tf.nn.relu, tf.tanh, tf.nn.elu ... of a caller that still imports
        # TensorFlow): a user function that happens to be called `elu` may compute anything (another alpha)
        lib_fn = getattr(fn, "__name__", "") == name and (getattr(fn, "__module__", "") or "").split(".")[0] in ("torch", "tensorflow")
        if (isinstance(fn, str) and fn == name) or any(fn is f for f in fns) or lib_fn:
            return name
    raise NotImplementedError(f"hidden_activation_fn={fn!r}: the HIP kernels implement relu (the reference default, "
                              f"scripts/vae.py:196), tanh, sigmoid and elu")


def _check_relu(fn):          # (kept name: validates, returns nothing)
    activation_name(fn)


# scripts/base.py:12 DEFAULT_INITIALIZERS = {'w': xavier, 'b': zeros}: what Engine.init_parameters draws.  A custom
# `initializers` dict maps 'w' and/or 'b' to a callable shape -> array-like (the stand-in for a TF initializer op, which
# cannot exist here); it is applied to the network's tensors of the flat parameter buffer when the conditional is bound.
DEFAULT_INITIALIZERS = {"w": "xavier_uniform", "b": "zeros"}


def _check_initializers(init):
    if init is None or init is DEFAULT_INITIALIZERS or init == DEFAULT_INITIALIZERS:
        return None
    if not isinstance(init, dict) or not init or any(k not in ("w", "b") or not callable(v) for k, v in init.items()):
        raise TypeError("initializers must be None, base.DEFAULT_INITIALIZERS or a dict mapping 'w' / 'b' to callables "
                        f"shape -> array (scripts/base.py:18,49-50); got {init!r}")
    return dict(init)


def _gen(seed, device):
    if seed is None:
        return None
    g = torch.Generator(device=device)
    g.manual_seed(int(seed))
    return g


# ----------------------------------------------------------- distributions
class MultivariateNormalDiag:
    """tfd.MultivariateNormalDiag(loc, scale_diag) subset: sample / log_prob / mean."""

    def __init__(self, loc, scale_diag, name="MultivariateNormalDiag"):
        self.loc, self.scale_diag, self.name = loc, scale_diag, name

    def mean(self, name=None):
        return self.loc

    def sample(self, sample_shape=(), seed=None, name=None):
        shape = (sample_shape,) if isinstance(sample_shape, int) else tuple(sample_shape)
        full = shape + tuple(torch.broadcast_shapes(self.loc.shape, self.scale_diag.shape))
        eps = torch.randn(full, device=self.loc.device, generator=_gen(seed, self.loc.device))
        return self.loc + self.scale_diag * eps

    def log_prob(self, z):
        e = (z - self.loc) / self.scale_diag
        return (-0.5 * e * e - 0.5 * math.log(2 * math.pi) - torch.log(self.scale_diag)).sum(-1)


class IndependentBernoulli:
    """tfd.Independent(tfd.Bernoulli(logits), 1) subset."""

    def __init__(self, logits, name="Bernoulli"):
        self.logits, self.name = logits, name

    def mean(self, name=None):
        return torch.sigmoid(self.logits)

    def sample(self, seed=None):
        p = torch.sigmoid(self.logits)
        return torch.rand(p.shape, device=p.device, generator=_gen(seed, p.device)) < p

    def log_prob(self, x):
        """x in {0, 1}, or soft targets in [0, 1] (the grey Bernoulli's cross-entropy: no normalised density there)."""
        x = x.to(self.logits.dtype)
        return (x * self.logits - F.softplus(self.logits)).sum(-1)


Bernoulli = IndependentBernoulli


def _cb_terms(logits):
    """(A, A') of the continuous Bernoulli, A = log((e^l - 1) / l): series in h = l / 2 below |l| = 1 (both closed forms cancel
    around 0; 0 itself is 0 / 0), forms in exp(-|l|) above -- finite at l = 0 and at |l| = 100 and beyond, no inf - inf."""
    l = logits
    h = 0.5 * l
    h2 = h * h
    a_s = h + h2 * (1.0 / 6.0 + h2 * (-1.0 / 180.0 + h2 * (1.0 / 2835.0 + h2 * (-1.0 / 37800.0))))
    m_s = 0.5 + 0.5 * h * (1.0 / 3.0 + h2 * (-1.0 / 45.0 + h2 * (2.0 / 945.0 + h2 * (-1.0 / 4725.0))))
    a = l.abs().clamp(min=1.0)                     # (the closed forms' argument where the series is taken: finite)
    om = -torch.expm1(-a)
    a_c = l.clamp(min=0.0) + torch.log(om / a)
    p = 1.0 / om - 1.0 / a
    m_c = torch.where(l > 0, p, 1.0 - p)
    small = l.abs() < 1.0
    return torch.where(small, a_s, a_c), torch.where(small, m_s, m_c)


class ContinuousBernoulli:
    """Independent continuous Bernoulli on [0, 1]^D (Loaiza-Ganem & Cunningham 2019): p(t | l) = exp(t l - A(l))."""

    def __init__(self, logits, name="ContinuousBernoulli"):
        self.logits, self.name = logits, name

    def mean(self, name=None):
        return _cb_terms(self.logits)[1]

    def sample(self, seed=None):
        """Inverse CDF: t = log1p(u (e^l - 1)) / l, written in exp(-|l|); t = u around l = 0."""
        l = self.logits
        u = torch.rand(l.shape, device=l.device, dtype=l.dtype, generator=_gen(seed, l.device))
        a = l.abs().clamp(min=1e-3)
        v = torch.where(l > 0, u, 1.0 - u)                            # (l < 0: the mirrored draw, t -> 1 - t)
        t = 1.0 + torch.log(v + (1.0 - v) * torch.exp(-a)) / a        # log(1 + v (e^a - 1)) / a
        t = torch.where(l > 0, t, 1.0 - t)
        return torch.where(l.abs() < 1e-3, u, t).clamp(0.0, 1.0)

    def log_prob(self, x):
        x = x.to(self.logits.dtype)
        return (x * self.logits - _cb_terms(self.logits)[0]).sum(-1)


class NormalFixedScale:
    """Independent Normal(loc, sigma) with one fixed scale: the Gaussian likelihood's decoder distribution."""

    def __init__(self, loc, sigma, name="NormalFixedScale"):
        self.loc, self.sigma, self.name = loc, float(sigma), name

    def mean(self, name=None):
        return self.loc

    def sample(self, seed=None):
        return self.loc + self.sigma * torch.randn(self.loc.shape, device=self.loc.device, dtype=self.loc.dtype,
                                                   generator=_gen(seed, self.loc.device))

    def log_prob(self, x):
        e = (x.to(self.loc.dtype) - self.loc) / self.sigma
        return (-0.5 * e * e - math.log(self.sigma) - 0.5 * math.log(2 * math.pi)).sum(-1)


class NormalDiagScale:
    """Independent Normal(loc, sigma_d) with one scale per dimension: the Gaussian likelihood's decoder distribution under
    likelihood_scale="learned" (sigma = exp of the parameter decoder/log_sigma, a tensor [D])."""

    def __init__(self, loc, sigma, name="NormalDiagScale"):
        self.loc, self.sigma, self.name = loc, sigma.to(loc.device, loc.dtype), name

    def mean(self, name=None):
        return self.loc

    def sample(self, seed=None):
        return self.loc + self.sigma * torch.randn(self.loc.shape, device=self.loc.device, dtype=self.loc.dtype,
                                                   generator=_gen(seed, self.loc.device))

    def log_prob(self, x):
        e = (x.to(self.loc.dtype) - self.loc) / self.sigma
        return (-0.5 * e * e - torch.log(self.sigma) - 0.5 * math.log(2 * math.pi)).sum(-1)


class Poisson:
    """Independent Poisson with the LOG-mean as its parameter: the decoder's distribution under likelihood="poisson".
    log p(x) = x l - exp(l) - lgamma(x + 1) summed over the last dimension; x >= 0, real values allowed."""

    def __init__(self, log_rate, name="Poisson"):
        self.log_rate, self.name = log_rate, name

    def mean(self, name=None):
        return torch.exp(self.log_rate)

    def sample(self, seed=None):
        return torch.poisson(self.mean(), generator=_gen(seed, self.log_rate.device))

    def log_prob(self, x):
        x = x.to(self.log_rate.dtype)
        return (x * self.log_rate - torch.exp(self.log_rate) - torch.lgamma(x + 1.0)).sum(-1)


class NegativeBinomial:
    """Independent negative binomial with mean exp(l) and inverse dispersion r_d = exp(rho_d) (variance mean + mean^2 / r): the
    decoder's distribution under likelihood="negative_binomial".  With u = l - rho and sp = softplus,
    log p(x) = lgamma(x + r) - lgamma(r) - lgamma(x + 1) - x sp(-u) - r sp(u): l is never exponentiated alone."""

    def __init__(self, log_mean, log_dispersion, name="NegativeBinomial"):
        self.log_mean, self.name = log_mean, name
        self.log_dispersion = log_dispersion.to(log_mean.device, log_mean.dtype)

    def mean(self, name=None):
        return torch.exp(self.log_mean)

    def sample(self, seed=None):
        """The gamma-Poisson mixture: rate ~ Gamma(r, r / mean), x ~ Poisson(rate)."""
        g = _gen(seed, self.log_mean.device)
        r = torch.exp(self.log_dispersion).expand_as(self.log_mean)
        rate = torch._standard_gamma(r, generator=g) * torch.exp(self.log_mean - self.log_dispersion)
        return torch.poisson(rate, generator=g)

    def log_prob(self, x):
        x = x.to(self.log_mean.dtype)
        r, u = torch.exp(self.log_dispersion), self.log_mean - self.log_dispersion
        sp = torch.nn.functional.softplus
        return (torch.lgamma(x + r) - torch.lgamma(r) - torch.lgamma(x + 1.0) - x * sp(-u) - r * sp(u)).sum(-1)


class _Categorical:
    def __init__(self, logits):
        self.logits = logits


class RelaxedOneHotCategorical:
    """tfd.RelaxedOneHotCategorical(temperature, logits) subset; ``.distribution.logits``
    is what scripts/gmvae.py:263,271 reads."""

    def __init__(self, temperature, logits, name="RelaxedOneHotCategorical", straight_through=False):
        self.temperature, self.logits, self.name = temperature, logits, name
        self.straight_through = bool(straight_through)
        self.distribution = _Categorical(logits)

    def sample(self, seed=None, uniform=None):
        """softmax((logits + g) / temperature); with straight_through the one-hot row at the argmax of logits + g (lowest
        index on ties) -- what a step under GMVAE_Y_STRAIGHT_THROUGH consumes (include/gmvae_hip.h)."""
        if uniform is None:
            uniform = torch.rand(self.logits.shape, device=self.logits.device,
                                 generator=_gen(seed, self.logits.device)).clamp_min(TINY)
        g = -torch.log(-torch.log(uniform))
        if self.straight_through:
            k = (self.logits + g).argmax(-1)        # (the first maximal index on ties)
            return F.one_hot(k, self.logits.shape[-1]).to(self.logits.dtype)
        return torch.softmax((self.logits + g) / self.temperature, -1)


class MixtureSameFamily:
    """tfd.MixtureSameFamily(Categorical(logits), MVNDiag(loc[K,L], scale[K,L])) subset (scripts/vae.py:240-244)."""

    def __init__(self, mixture_logits, loc, scale_diag, name="prior"):
        self.mixture_logits, self.loc, self.scale_diag, self.name = mixture_logits, loc, scale_diag, name

    def log_prob(self, z):
        t = (z[..., None, :] - self.loc) / self.scale_diag
        ln = (-0.5 * t * t - 0.5 * math.log(2 * math.pi) - torch.log(self.scale_diag)).sum(-1)
        return torch.logsumexp(torch.log_softmax(self.mixture_logits, -1) + ln, -1)

    def sample(self, sample_shape=(), seed=None, name=None):
        n = sample_shape if isinstance(sample_shape, int) else int(torch.tensor(tuple(sample_shape)).prod())
        g = _gen(seed, self.loc.device)
        k = torch.multinomial(torch.softmax(self.mixture_logits, -1), n, replacement=True, generator=g)
        eps = torch.randn((n, self.loc.shape[1]), device=self.loc.device, generator=g)
        return self.loc[k] + self.scale_diag[k] * eps

    def mean(self, name=None):
        return (torch.softmax(self.mixture_logits, -1)[:, None] * self.loc).sum(0)


# -------------------------------------------------- conditional networks
class _Conditional:
    def __init__(self, size, hidden_layer_sizes, hidden_activation_fn, name, initializers=None):
        self._act = activation_name(hidden_activation_fn)
        self._initializers = _check_initializers(initializers)
        self._name, self._size = name, size
        self._hidden = None if hidden_layer_sizes is None else list(hidden_layer_sizes)
        self._engine = None
        self._net = None

    def bind(self, engine, net_id):
        """Attach to the flat parameter buffer (the factories do this; it stands in
        for Sonnet's lazy variable creation, scripts/base.py:47-60)."""
        # the activation is a field of the ENGINE's dims (one for every network, as the factories pass one): a conditional built
        # with another one would silently evaluate with the engine's
        if self._hidden and self._act != engine.hidden_act:
            raise ValueError(f"{self._name}: hidden_activation_fn is {self._act!r} but the Engine it is bound to was created "
                             f"with hidden_act={engine.hidden_act!r}")
        self._engine, self._net = engine, net_id
        if self._initializers:                      # custom initializers: re-draw this network's tensors
            prefix = self._name + "_fcnet/"
            hit = False
            with torch.no_grad():
                for name, view in engine.views().items():
                    fn = self._initializers.get(name[-1]) if name.startswith(prefix) else None
                    if fn is not None:
                        val = torch.as_tensor(fn(tuple(view.shape)), dtype=torch.float32).reshape(view.shape)
                        view.copy_(val.to(view.device))
                        hit = True
            if not hit:
                raise ValueError(f"{self._name}: no variables named {prefix}* in the engine's parameter layout")
            engine.drop_graphs()                    # (captured graphs hold weight images of the old values)
        return self

    def _mlp(self, tensor_list):
        if self._engine is None:
            raise RuntimeError(f"{self._name}: not bound to an Engine; build models with create_vae/create_gmvae")
        tensors = list(tensor_list)
        if self._net == L.NET_ENCODER_GMM:
            if len(tensors) != 2:
                raise ValueError("encoder_gmm expects (x, y)")      # concat([x, y], 1), scripts/base.py:66
            return self._engine.mlp(self._net, tensors[0], tensors[1])
        if len(tensors) != 1:
            raise ValueError(f"{self._name} expects one input tensor")
        return self._engine.mlp(self._net, tensors[0])


class ConditionalNormal(_Conditional):
    def __init__(self, size, hidden_layer_sizes=None, initializers=None, sigma_min=0.0, raw_sigma_bias=0.25,
                 hidden_activation_fn=torch.relu, name="cond_normal"):
        super().__init__(size, hidden_layer_sizes, hidden_activation_fn, name, initializers)
        self._sigma_min, self._raw_sigma_bias = sigma_min, raw_sigma_bias

    def condition(self, tensor_list, **unused_kwargs):
        outs = self._mlp(tensor_list)
        mu, raw = outs[:, :self._size], outs[:, self._size:]            # tf.split(outs, 2, axis=1)
        sigma = torch.clamp_min(F.softplus(raw + self._raw_sigma_bias), self._sigma_min)
        return mu, sigma

    def __call__(self, *args, **kwargs):
        mu, sigma = self.condition(args, **kwargs)
        return MultivariateNormalDiag(loc=mu, scale_diag=sigma, name=self._name)


class ConditionalBernoulli(_Conditional):
    def __init__(self, size, hidden_layer_sizes=None, initializers=None, bias_init=0.0,
                 hidden_activation_fn=torch.relu, name="cond_bernoulli"):
        super().__init__(size, hidden_layer_sizes, hidden_activation_fn, name, initializers)
        self._bias_init = bias_init

    def condition(self, tensor_list, **unused_kwargs):
        # + bias_init (scalar or vector, scripts/base.py:135) is applied inside gmvae_mlp_forward: the Engine this
        # conditional is bound to was created with the same value (gen_bias_init / gen_bias_vec of GmvaeDims)
        return self._mlp(tensor_list)

    def __call__(self, *args, **kwargs):
        # the distribution of the model's likelihood (Engine(likelihood=)): its mean() is A'(lambda), so reconstruct_images and
        # generate_sample_images return the mean image under every likelihood
        lam = self.condition(args, **kwargs)
        lik = "bernoulli" if self._engine is None else self._engine.likelihood
        if lik == "continuous_bernoulli":
            return ContinuousBernoulli(lam, name=self._name)
        if lik == "gaussian" and self._engine.likelihood_scale == "learned":
            return NormalDiagScale(lam, torch.exp(self._engine.views()["decoder/log_sigma"]), name=self._name)
        if lik == "gaussian":
            return NormalFixedScale(lam, self._engine.likelihood_sigma, name=self._name)
        if lik == "poisson":
            return Poisson(lam, name=self._name)
        if lik == "negative_binomial":
            return NegativeBinomial(lam, self._engine.views()["decoder/log_dispersion"], name=self._name)
        return IndependentBernoulli(lam, name=self._name)


class ConditionalCategorical(_Conditional):
    def __init__(self, size, hidden_layer_sizes=None, temperature=1.0, initializers=None,
                 hidden_activation_fn=torch.relu, name="cond_categorical"):
        super().__init__(size, hidden_layer_sizes, hidden_activation_fn, name, initializers)
        self._temperature = temperature

    def condition(self, tensor_list, **unused_kwargs):
        return self._mlp(tensor_list)

    def __call__(self, *args, **kwargs):
        # bound to an Engine: its CURRENT temperature (Engine.set_temperature) and its y estimator, so that transform and
        # reconstruct_images draw y as the training step does
        e = self._engine
        t = self._temperature if e is None else e.temperature
        st = e is not None and e.y_estimator == "straight_through"
        return RelaxedOneHotCategorical(t, logits=self.condition(args, **kwargs), name=self._name, straight_through=st)


def _targets_guard(loss, images, targets):
    """Every reference call site passes targets = images (scripts/runners.py:127-130).  A distinct tensor is compared ON
    THE DEVICE and a mismatch turns the loss into NaN: loud, and without the device-to-host sync a torch.equal costs."""
    if targets is images or (targets.data_ptr() == images.data_ptr() and targets.shape == images.shape):
        return loss
    if targets.numel() != images.numel():
        raise NotImplementedError("targets != images is not used by the reference and not supported")
    bad = (targets.reshape(images.shape).to(images.device) != images).any()
    return loss + torch.where(bad, torch.full_like(loss, float("nan")), torch.zeros_like(loss))


def impute(model, images, mask):
    """mask * images + (1 - mask) * model.reconstruct_images(mask * images): the one imputation rule of VAE.impute and
    GMVAE.impute (mask: uint8 / bool of the images' shape, non-zero = observed)."""
    m = (torch.as_tensor(mask).to(images.device) != 0).reshape(images.shape)
    xm = torch.where(m, images, torch.zeros_like(images))
    rec = model.reconstruct_images(xm).reshape(images.shape)
    return torch.where(m, images.to(rec.dtype), rec)


def _bound_engine(model, what):
    if model._engine is None:
        raise ValueError(f"{what} runs on the model's Engine: create the model through the runners / bind an Engine first")
    return model._engine


def impute_posterior(model, images, mask, n_samples, n_draws=0, seed=None):
    """VAE.impute / GMVAE.impute with n_samples given: Engine.impute_posterior's posterior-mean imputation (a float tensor of
    the images' shape), or with n_draws = M > 0 the M completed images [B, M, ...] as uint8: the decoder (Engine.mlp) on the
    sampling-importance-resampling draws of z, Bernoulli draws from a torch generator seeded with `seed` (None: the engine's
    noise seed) at the missing pixels, the observed pixels copied."""
    from . import _lib as L
    eng = _bound_engine(model, "impute(n_samples=)")
    B = images.shape[0]
    x = images.reshape(B, -1)
    m = torch.as_tensor(mask).reshape(B, -1)
    o = eng.impute_posterior(x, n_samples, mask=m, n_draws=n_draws)
    if not n_draws:
        return o["imputed"].reshape(images.shape)
    M = int(n_draws)
    lam = eng.mlp(L.NET_DECODER, o["draw_z"].reshape(B * M, -1))
    gen = torch.Generator(device=lam.device)
    gen.manual_seed(int(eng.noise_seed if seed is None else seed) & (2 ** 63 - 1))
    draws = (torch.rand(lam.shape, generator=gen, device=lam.device) < torch.sigmoid(lam)).to(torch.uint8).view(B, M, -1)
    obs = (m.to(lam.device) != 0)[:, None, :]
    xs = (x.to(lam.device) != 0).to(torch.uint8)[:, None, :]
    return torch.where(obs, xs, draws).reshape(B, M, *images.shape[1:])


def imputation_scores(model, images, mask, n_samples):
    """VAE.imputation_scores / GMVAE.imputation_scores: the importance-sampling imputation p^ (Engine.impute_posterior, the
    encoders fed mask * images) scored against the truth in `images` at the missing pixels: dict(nll = the cross-entropy per
    missing pixel, error_rate = the share of missing pixels where round(p^) != x, cond_loglik = the mean over the examples of
    log p^(x_missing | x_observed), ess = the mean effective sample size, n_missing), Python floats."""
    eng = _bound_engine(model, "imputation_scores")
    B = images.shape[0]
    x = images.reshape(B, -1).to(eng.device)
    m = torch.as_tensor(mask).reshape(B, -1).to(eng.device) != 0
    o = eng.impute_posterior(x, n_samples, mask=m)
    t = (x != 0).double()
    p = o["mean"].double().clamp(1e-12, 1.0 - 1e-12)
    miss = (~m).double()
    n_missing = miss.sum().item()
    ce = -(miss * (t * p.log() + (1.0 - t) * (-p).log1p())).sum().item()
    wrong = (miss * ((p >= 0.5).double() != t).double()).sum().item()
    return dict(nll=ce / max(n_missing, 1.0), error_rate=wrong / max(n_missing, 1.0), cond_loglik=o["cond_loglik"].double().mean().item(),
                ess=o["ess"].double().mean().item(), n_missing=n_missing)
