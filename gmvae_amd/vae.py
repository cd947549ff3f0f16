"""VAE / VAE with a learned Gaussian-mixture prior (mirror of scripts/vae.py).

``VAE`` (scripts/vae.py:11-123), ``TrainableVAE`` (126-188), ``create_vae``
(191-271) keep the reference's names, argument orders and semantics;
``run_model`` is served by the fused HIP step (gmvae_step) and returns a scalar
torch tensor whose ``.backward()`` fills ``model.params.grad``.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _lib as L
from . import base
from .engine import Engine


class VAE:
    def __init__(self, prior, decoder, encoder, mix_components, random_seed):
        self._prior, self._decoder, self._encoder = prior, decoder, encoder
        self.mix_components = mix_components
        self.random_seed = random_seed
        self._engine = None

    def prior(self):
        """p(z): fixed N(0,I) or the learned mixture (scripts/vae.py:41-48)."""
        return self._prior() if callable(self._prior) else self._prior

    def decoder(self, z):
        return self._decoder(z)

    def encoder(self, x):
        return self._encoder(x)      # the uint8 -> fp32 cast of scripts/vae.py:75 happens in the GEMM loader

    def reconstruct_images(self, images):
        q_z = self.encoder(images)
        z = q_z.sample(seed=self.random_seed)
        return self.decoder(z).mean(name="reconstructions")

    def generate_sample_images(self, z=None, num_samples=1):
        if z is None:
            z = self.generate_samples(num_samples)
        return self.decoder(z).mean(name="sample_images")

    def impute(self, images, mask, n_samples=None, n_draws=0, seed=None):
        """Fills in the missing pixels: mask * images + (1 - mask) * reconstruct_images(mask * images) -- the observed pixels
        exactly as given, the others the decoder's mean from the zero-imputed input the networks were trained on (a model
        created with pixel_mask=True).  A float tensor of the images' shape.
        n_samples = N: the missing pixels are the importance-sampling estimate of E[x_missing | x_observed] at N samples
        (Engine.impute_posterior) in place of one draw's decoder mean; with n_draws = M > 0, M completed images [B, M, ...]
        (uint8) by sampling-importance-resampling, the Bernoulli draws seeded by `seed` (base.impute_posterior)."""
        if n_samples is None:
            return base.impute(self, images, mask)
        return base.impute_posterior(self, images, mask, n_samples, n_draws, seed)

    def imputation_scores(self, images, mask, n_samples):
        """The importance-sampling imputation scored against the truth in `images` at the missing pixels: dict(nll,
        error_rate, cond_loglik, ess, n_missing) (base.imputation_scores)."""
        return base.imputation_scores(self, images, mask, n_samples)

    def transform(self, inputs):
        """MEAN latent code (scripts/vae.py:108-114)."""
        return self.encoder(inputs).mean(name="code")

    def embed_latent(self, images, **kw):
        """The 2-D t-SNE embedding of the latent codes of `images`: transform, then gmvae_amd.tsne.embed(**kw) -- its dict
        (embedding [N, 2], kl, kl_history, beta, entropy)."""
        from . import tsne
        return tsne.embed(self.transform(images), **kw)

    def generate_samples(self, num_samples):
        z = self.prior().sample(num_samples, seed=self.random_seed, name="samples")
        return z.reshape(num_samples, -1)

    # north_star aliases
    encode = encoder
    decode = decoder


class TrainableVAE(VAE):
    def __init__(self, prior, decoder, encoder, mix_components=1, random_seed=None):
        super().__init__(prior, decoder, encoder, mix_components, random_seed)

    def _need_engine(self):
        if self._engine is None:
            raise RuntimeError("run_model needs the fused HIP engine: build the model with create_vae()")
        return self._engine

    def run_model(self, images, targets, eps=None, mask=None):
        """Batch-mean loss = nll + kl_div_z (scripts/vae.py:153-188); ELBO = -loss.
        ``targets`` must be ``images`` (every reference call site passes the same
        tensor, scripts/runners.py:130).  eps: optional N(0,1) noise [B*S, L].  mask (a model created with pixel_mask=True):
        uint8 / bool [B, D], non-zero = observed; the loss counts the observed pixels alone (Engine)."""
        return base._targets_guard(self._need_engine().loss(images, eps, None, mask=mask), images, targets)

    def compute_loss(self, images, n_samples=None, eps=None, mask=None):
        e = self._need_engine()
        if n_samples is not None and n_samples != e.S:
            raise ValueError(f"model was created with n_samples={e.S}")
        return e.loss(images, eps, None, mask=mask)

    def iw_bound(self, images, n_samples, chunk=None, mask=None):
        """Per-example IWAE estimate of log p(x) at n_samples samples (Burda et al.), streamed in chunks of `chunk` samples:
        a [B] device tensor (Engine.iw_bound).  mask: the bound on log p(x_observed)."""
        return self._need_engine().iw_bound(images, n_samples, chunk, mask=mask)["bound"]

    def ais_bound(self, images, n_chains=16, n_temps=1000, **kw):
        """log p(x) per example by annealed importance sampling with HMC transitions, from the generative model alone -- its gap
        does not depend on the inference network, unlike iw_bound's --: Engine.ais_bound's dict (bound [B], logw [B, n_chains],
        stats [B, 4] = bound, ESS, acceptance rate, step size; z; tail).  **kw: schedule, n_leapfrog, step_size, init, adapt."""
        return self._need_engine().ais_bound(images, n_chains, n_temps, **kw)

    def simulate(self, num_samples, **kw):
        """num_samples ancestral samples (z*, x) from the generative model on the device: Engine.simulate's dict (z, k, x, prob);
        z* is an exact posterior sample for x.  generate_samples stays the reference's sampler; this one is what bdmc_gap needs."""
        return self._need_engine().simulate(num_samples, **kw)

    def bdmc_gap(self, n_examples, n_chains=16, n_temps=1000, **kw):
        """Bidirectional Monte Carlo: lower (ais_bound) and upper (reverse chains from the exact posterior sample) bounds on
        log p(x) of n_examples SIMULATED examples -- Engine.bdmc_gap's dict (lower, upper, gap, ...).  The upper bound exists only
        for simulated data; the gap bounds the bias of ais_bound at these settings on data distributed as the model's samples."""
        return self._need_engine().bdmc_gap(n_examples, n_chains, n_temps, **kw)

    def inference_gaps(self, images, n_steps=500, n_samples=4, n_eval=256, ais=None, **kw):
        """The inference gap log p(x) - L[q(z|x)] split into its amortisation and approximation parts by refining q(z|x) per
        example (Cremer, Li & Duvenaud 2018): Engine.inference_gaps's dict (elbo_amortised, elbo_refined, iw_bound_refined,
        log_px, amortisation_gap, approximation_gap as batch means; ais = a dict of ais_bound's arguments adds ais_log_px).
        **kw: lr, betas, adam_eps, row0."""
        return self._need_engine().inference_gaps(images, n_steps, n_samples, n_eval, ais=ais, **kw)

    def posterior_component(self, images, n_samples, chunk=None):
        """ln p(k | x) over the components of the learned mixture prior (mixture_components > 1), by importance sampling with
        n_samples samples of z, streamed in chunks of `chunk`: a [B, K] device tensor (Engine.posterior_component)."""
        return self._need_engine().posterior_component(images, n_samples, chunk)["log_post"]

    def latent_diagnostics(self, images, queries=None, per_dim=True):
        """The aggregate posterior's diagnostics over `images` (Engine.aggregate_posterior): the dict of per-query log-densities
        and of kl_avg = mi + kl_marginal, tc, dim_kl, active_units."""
        return self._need_engine().aggregate_posterior(images, queries=queries, per_dim=per_dim)

    def fit_latent_mixture(self, images, n_components=None, **kw):
        """A diagonal Gaussian mixture fitted by EM on the device to the codes self.transform(images) -- the "VAE + GMM" baseline
        (gmvae_amd.mixfit.fit(**kw): n_iter, n_init, reg_covar, seed, init, covariance).  n_components defaults to the mixture prior's size
        and is required for the plain VAE.  Returns fit's dict plus `log_resp` [N, K], the responsibilities of those images."""
        from . import mixfit
        if n_components is None and self.mix_components > 1:
            n_components = self.mix_components
        return mixfit.fit_latent(self, images, n_components, **kw)

    def neighbour_scores(self, images, labels=None, clusters=None, k=10, n_labels=10, **kw):
        """The neighbourhood scores of the codes self.transform(images) (gmvae_amd.neighbours.scores): with `labels` knn_acc_loo (the
        leave-one-out k-NN accuracy), silhouette_labels and their per-example tensors knn_pred and silhouette_labels_samples; with
        `clusters` (an int tensor [N]) silhouette_clusters and silhouette_clusters_samples; with both nmi and ari.  clusters None: the
        model's own clustering -- the mixture-prior VAE's predict_clusters(images, cluster_samples), 16 samples unless given, over
        its mixture components; the plain VAE has none.  The scores are 0-d device tensors; nothing synchronises."""
        from . import neighbours
        return neighbours.model_scores(self, images, labels, clusters, k=k, n_labels=n_labels, **kw)

    def linear_probe(self, train_images, train_labels, test_images=None, test_labels=None, n_classes=10, labelled_per_class=0,
                     seed=0, **fit_kw):
        """A linear classifier fitted on the device to the frozen codes self.transform(train_images) (gmvae_amd.linprobe.fit(**fit_kw):
        l2, n_iter, standardize) and scored there and on the test images: `train_accuracy`, `train_nll`, `test_accuracy`, `test_nll`
        (0-d device tensors), `n_labelled` and `fit`.  labelled_per_class > 0 fits on the labels runners.select_labelled picks with
        `seed` -- the "M1" baseline of a semi-supervised run with the same flag."""
        from . import linprobe
        return linprobe.model_probe(self, train_images, train_labels, test_images, test_labels, n_classes=n_classes,
                                    labelled_per_class=labelled_per_class, seed=seed, **fit_kw)

    def latent_pca(self, images, **kw):
        """The principal components and the spectrum of the codes self.transform(images) on the device (gmvae_amd.pca.fit(**kw)), with
        spectrum_summary's rotation-invariant readouts `dim90`, `participation` and `top_ratio` in the same dict."""
        from . import pca
        return pca.model_latent_pca(self, images, **kw)

    def sample_test(self, images, n_generations=None, space="data", **kw):
        """The kernel two-sample test of the model's samples against `images` on the device (gmvae_amd.twosample.mmd_test(**kw):
        n_perms, kernel, bandwidth, scales, seed): space "data" -- simulate(n_generations)["x"] against the binarised images
        (Bernoulli likelihood only) --, "code" -- one draw of encoder(x).sample() per image against the prior draws z* of simulate:
        does the aggregate posterior match the prior, with a p-value, next to latent_diagnostics' KL -- or "both".  A dict per
        space asked for, each mmd_test's (mmd2, p_value, null, witness_x, witness_y, sigma, n_perms, kscale)."""
        from . import twosample
        return twosample.model_test(self, images, n_generations, space, **kw)

    def sample_distance(self, images, n_generations=None, space="data", n_perms=0, **kw):
        """The debiased Sinkhorn divergence between the model's samples and `images` on the device (gmvae_amd.sinkhorn.divergence(**kw):
        blur, blur_rel, n_iter, n_final; with n_perms > 0 divergence_test, which adds a permutation null and p_value and takes seed)
        on the pairs of samples sample_test compares, with its seeds and refusals: a transport distance in the space's own units
        next to sample_test's verdict.  A dict per space asked for; read marginal_err -- convergence depends on the data -- and
        compare values only at equal sample sizes and blur (gmvae_amd.sinkhorn)."""
        from . import sinkhorn
        return sinkhorn.model_distance(self, images, n_generations, space, n_perms, **kw)

    def init_prior_from_mixture(self, fit):
        """Starts the learned mixture prior (mixture_components > 1) from a fitted mixture (fit_latent_mixture's or
        gmvae_amd.mixfit.fit's dict, or (logw, mu, sigma)): mixture_logits = logw, loc = mu, raw_scale_diag = softplus^-1(sigma) =
        sigma + ln(-expm1(-sigma)).  Written through state_dict() / load_state_dict(), so whatever the engine derives from its
        parameters is rebuilt.  Adam's slots are left as they are: the call is meant before training or between phases.
        ValueError for the plain VAE (it has no mixture prior) and for a fit whose K or L is not the prior's."""
        from . import mixfit
        e = self._need_engine()
        if self.mix_components <= 1:
            raise ValueError("the plain VAE has no mixture prior to initialise (create_vae(mixture_components > 1))")
        logw, mu, sigma = mixfit.checked_fit(fit, e.K, e.Lz, e.device)
        sd = self.state_dict()
        sd["mixture_logits"], sd["loc"], sd["raw_scale_diag"] = logw, mu, mixfit.softplus_inverse(sigma)
        self.load_state_dict(sd)

    def predict_clusters(self, images, n_samples):
        """The component the model's posterior p(k | x) assigns each example to: an int64 [B] device tensor."""
        return self.posterior_component(images, n_samples).argmax(dim=1)

    @property
    def summaries(self):
        """nll_scalar / kl_div_z / elbo of the last run_model (scripts/vae.py:178,182,186)."""
        e = self._need_engine()
        t = e.grads[e.P:].detach()
        out = {"nll_scalar": t[1] / t[4], "kl_div_z": t[2] / t[4], "elbo": -t[0] / t[4]}
        if e.weighted_objective:                   # (nll_scalar and kl_div_z stay unweighted; elbo = -loss carries the weights)
            out["kl_weight"], out["y_weight"], out["y_floor_share"] = t[5] / t[4], t[6] / t[4], t[7] / t[4]
        if e.pixel_mask:                           # (nll_scalar counts the observed pixels; the held-out ones per missing pixel)
            if t[6].item() > 0:
                out["imputation_nll"] = t[5] / t[6]
            out["observed_share"] = t[7] / (t[6] + t[7])
        if e.likelihood != "bernoulli":            # (the per-pixel squared error of the mean image A'(lambda) against t = x / 255)
            out["recon_mse"] = t[5] / t[6]
        if e.likelihood_scale == "learned":        # (the mean of the learned per-dimension scales sigma_d = exp(rho_d))
            out["sigma_mean"] = torch.exp(e.views()["decoder/log_sigma"]).mean()
        if e.likelihood == "negative_binomial":    # (the mean of the learned inverse dispersions r_d = exp(rho_d))
            out["dispersion_mean"] = torch.exp(e.views()["decoder/log_dispersion"]).mean()
        if e.clip_norm is not None:                # (of the last eager optimizer step: the norm before clipping, clipped 0 / 1)
            out["grad_norm"], out["clipped"] = e.grad_clip[0], e.grad_clip[2]
        return out

    @property
    def params(self):
        return self._need_engine().params

    def state_dict(self):
        return self._need_engine().state_dict()

    def load_state_dict(self, sd):
        self._need_engine().load_state_dict(sd)


def create_vae(data_size, latent_size, mixture_components=1, fcnet_hidden_sizes=None,
               hidden_activation_fn=torch.relu, sigma_min=0.001, raw_sigma_bias=0.25, gen_bias_init=0.0,
               random_seed=None, n_samples=1, grad_estimator="standard", weighted_objective=False, kl_weight=1.0,
               y_weight=1.0, y_free_nats=0.0, pixel_mask=False, clip_norm=None, likelihood="bernoulli", likelihood_sigma=1.0,
               real_valued=None, likelihood_scale="fixed"):
    """Factory with the signature of scripts/vae.py:191-200 (+ pixel_mask: run_model / compute_loss / iw_bound take mask=,
    Engine; + n_samples, the
    IWAE extension of SURVEY.md A15; 1 == the reference; + grad_estimator: "dreg" = the doubly
    reparameterised gradient for the encoder, Engine; + weighted_objective, kl_weight, y_weight, y_free_nats: the KL weight of
    Engine's weighted objective -- the VAE family has no y term, so y_weight and y_free_nats are ignored; + clip_norm: the
    gradient clipped by its global norm in front of Adam, Engine; summaries then carry grad_norm and clipped; + likelihood,
    likelihood_sigma: "grey_bernoulli", "continuous_bernoulli" or "gaussian" on grey levels t = x / 255, Engine; the decoder
    then returns that distribution, reconstruct_images its mean, and summaries carry recon_mse; + real_valued,
    likelihood_scale: float feature rows under the Gaussian, with a fixed or a learned per-dimension scale, Engine; likelihood
    "poisson" / "negative_binomial": float count rows, the decoder returns base.Poisson / base.NegativeBinomial with mean
    exp(lambda), summaries carry dispersion_mean under the latter, Engine)."""
    if fcnet_hidden_sizes is None:
        fcnet_hidden_sizes = [latent_size]                     # scripts/vae.py:228-229
    name = "vae_gmp" if mixture_components > 1 else "vae"
    engine = Engine(name, data_size, latent_size, mixture_components, fcnet_hidden_sizes, n_samples=n_samples,
                    sigma_min=sigma_min, raw_sigma_bias=raw_sigma_bias, gen_bias_init=gen_bias_init,
                    random_seed=random_seed, hidden_act=base.activation_name(hidden_activation_fn),
                    grad_estimator=grad_estimator, weighted_objective=weighted_objective, kl_weight=kl_weight,
                    y_weight=y_weight, y_free_nats=y_free_nats, pixel_mask=pixel_mask, clip_norm=clip_norm, likelihood=likelihood, likelihood_sigma=likelihood_sigma,
                    real_valued=real_valued, likelihood_scale=likelihood_scale)
    if mixture_components > 1:
        def prior():
            v = engine.views()
            return base.MixtureSameFamily(v["mixture_logits"], v["loc"], F.softplus(v["raw_scale_diag"]), name="prior")
    else:
        def prior():
            return base.MultivariateNormalDiag(torch.zeros(latent_size, device=engine.device),
                                               torch.ones(latent_size, device=engine.device), name="prior")
    decoder = base.ConditionalBernoulli(size=data_size, hidden_layer_sizes=fcnet_hidden_sizes,
                                        hidden_activation_fn=hidden_activation_fn, bias_init=gen_bias_init,
                                        name="decoder").bind(engine, L.NET_DECODER)
    encoder = base.ConditionalNormal(size=latent_size, hidden_layer_sizes=fcnet_hidden_sizes,
                                     hidden_activation_fn=hidden_activation_fn, sigma_min=sigma_min,
                                     raw_sigma_bias=raw_sigma_bias, name="encoder").bind(engine, L.NET_ENCODER)
    model = TrainableVAE(prior, decoder, encoder, mixture_components, random_seed=random_seed)
    model._engine = engine
    return model
