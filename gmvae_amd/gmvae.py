"""Gaussian Mixture VAE (mirror of scripts/gmvae.py).

``GMVAE`` (scripts/gmvae.py:12-188), ``TrainableGMVAE`` (191-274),
``create_gmvae`` (277-356): same names, argument orders and semantics.
``run_model`` is the fused HIP step.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _lib as L
from . import base
from . import utils
from .engine import Engine


class GMVAE:
    def __init__(self, mix_components, prior_gmm, decoder, encoder_y, encoder_gmm, random_seed):
        self._prior_gmm, self._decoder = prior_gmm, decoder
        self._encoder_y, self._encoder_gmm = encoder_y, encoder_gmm
        self.mix_components = mix_components
        self.random_seed = random_seed
        self._engine = None

    def prior_gmm(self, y):
        return self._prior_gmm(y)

    def decoder(self, z):
        return self._decoder(z)

    def encoder_y(self, x):
        return self._encoder_y(x)

    def encoder_gmm(self, x, y):
        return self._encoder_gmm(x, y)

    def reconstruct_images(self, images):
        y = self.encoder_y(images).sample(seed=self.random_seed)
        z = self.encoder_gmm(images, y).sample(seed=self.random_seed)
        return self.decoder(z).mean(name="reconstructions")

    def generate_sample_images(self, z=None, num_samples=1, name="sample_images"):
        if z is None:
            z = self.generate_samples(num_samples)
        return self.decoder(z).mean(name=name)

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
        """SAMPLED latent code (scripts/gmvae.py:140-149; the VAE returns the mean)."""
        y = self.encoder_y(inputs).sample(seed=self.random_seed)
        return self.encoder_gmm(inputs, y).sample(seed=self.random_seed, name="code")

    def embed_latent(self, images, **kw):
        """The 2-D t-SNE embedding of the latent codes of `images`: transform, then gmvae_amd.tsne.embed(**kw) -- its dict
        (embedding [N, 2], kl, kl_history, beta, entropy)."""
        from . import tsne
        return tsne.embed(self.transform(images), **kw)

    def generate_samples(self, num_samples, clusters=None):
        """[num_samples * K, L] draws from every p(z|y=k), or from the given clusters
        (scripts/gmvae.py:152-188)."""
        dev = self._engine.device if self._engine is not None else None
        if clusters is None:
            y = F.one_hot(torch.arange(self.mix_components, device=dev), self.mix_components).float()
        else:
            clusters = torch.as_tensor(clusters, device=dev).long()
            y = F.one_hot(clusters, self.mix_components).float()
        z = self.prior_gmm(y).sample(num_samples, seed=self.random_seed)
        return z.reshape(num_samples * y.shape[0], -1)

    def encode(self, x):
        q_y = self.encoder_y(x)
        return q_y, self.encoder_gmm(x, q_y.sample(seed=self.random_seed))

    decode = decoder


class TrainableGMVAE(GMVAE):
    def __init__(self, mix_components, prior_gmm, decoder, encoder_y, encoder_gmm, random_seed=None):
        super().__init__(mix_components, prior_gmm, decoder, encoder_y, encoder_gmm, random_seed=random_seed)
        self._last_labels = None

    def _need_engine(self):
        if self._engine is None:
            raise RuntimeError("run_model needs the fused HIP engine: build the model with create_gmvae()")
        return self._engine

    def run_model(self, images, targets, labels=None, eps=None, u=None, y_observed=None, mask=None):
        """Batch-mean loss = nll + kl_div_z + nent (scripts/gmvae.py:223-274); ELBO = -loss
        (the +ln K constant is omitted, as in the reference).  eps [B*S,L] / u [B*S,K]:
        optional explicit noise (parity mode); default is in-kernel Philox.  labels: the ground truth cluster_acc is
        scored against, never seen by the objective.  y_observed (a model created with semi_supervised=True): int [B],
        the observed component of each example or -1 -- those examples' y is clamped in the loss (Engine).  mask (a model
        created with pixel_mask=True): uint8 / bool [B, D], non-zero = observed; the loss counts the observed pixels alone."""
        self._last_labels = labels
        return base._targets_guard(self._need_engine().loss(images, eps, u, y_observed, mask), images, targets)

    def compute_loss(self, images, n_samples=None, labels=None, eps=None, u=None, y_observed=None, mask=None):
        e = self._need_engine()
        if n_samples is not None and n_samples != e.S:
            raise ValueError(f"model was created with n_samples={e.S}")
        self._last_labels = labels
        return e.loss(images, eps, u, y_observed, mask)

    def iw_bound(self, images, n_samples, chunk=None, mask=None):
        """Per-example importance-weighted bound at n_samples samples (the A15 bound compute_loss(n_samples=S) reports),
        streamed in chunks of `chunk` samples: a [B] device tensor (Engine.iw_bound).  mask: the bound on log p(x_observed)."""
        return self._need_engine().iw_bound(images, n_samples, chunk, mask=mask)["bound"]

    def iw_bound_enum_y(self, images, n_samples, chunk=None):
        """Per-example importance-weighted bound with y summed out exactly over the K components (log p(x) + ln K for a
        uniform p(y); the same for either y_inference), n_samples samples of z per component, streamed in chunks of `chunk`:
        a [B] device tensor (Engine.iw_bound_enum_y)."""
        return self._need_engine().iw_bound_enum_y(images, n_samples, chunk)["bound"]

    def ais_bound(self, images, n_chains=16, n_temps=1000, **kw):
        """log p(x) per example by annealed importance sampling with HMC transitions, from the generative model alone -- its gap
        does not depend on the inference network, unlike iw_bound's --: Engine.ais_bound's dict (bound [B], logw [B, n_chains],
        stats [B, 4] = bound, ESS, acceptance rate, step size; z; tail).  **kw: schedule, n_leapfrog, step_size, init, adapt.
        The bound is of log p(x) itself, the uniform p(y) inside: iw_bound_enum_y's bound minus ln K; the same for every y_inference."""
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

    def posterior_y(self, images, n_samples, chunk=None):
        """ln p(y = k | x) of the model itself (not the inference network's q(y|x)), by importance sampling with n_samples
        samples of z per component, streamed in chunks of `chunk`: a [B, K] device tensor (Engine.posterior_y)."""
        return self._need_engine().posterior_y(images, n_samples, chunk)["log_post"]

    def latent_diagnostics(self, images, queries=None, per_dim=True):
        """The aggregate posterior's diagnostics over `images` (Engine.aggregate_posterior): the dict of per-query log-densities
        and of kl_avg = mi + kl_marginal, tc, dim_kl, active_units, q_y, q_y_entropy and mi_xy."""
        return self._need_engine().aggregate_posterior(images, queries=queries, per_dim=per_dim)

    def fit_latent_mixture(self, images, n_components=None, **kw):
        """A diagonal Gaussian mixture fitted by EM on the device to the codes self.transform(images) -- the sampled code run_eval
        stores in latent_state -- (gmvae_amd.mixfit.fit(**kw): n_iter, n_init, reg_covar, seed, init, covariance).  n_components defaults to
        the model's mixture size.  Returns fit's dict plus `log_resp` [N, K], the responsibilities of those images."""
        from . import mixfit
        return mixfit.fit_latent(self, images, self.mix_components if n_components is None else n_components, **kw)

    def neighbour_scores(self, images, labels=None, clusters=None, k=10, n_labels=10, **kw):
        """The neighbourhood scores of the codes self.transform(images) (gmvae_amd.neighbours.scores): with `labels` knn_acc_loo (the
        leave-one-out k-NN accuracy), silhouette_labels and their per-example tensors knn_pred and silhouette_labels_samples; with
        `clusters` (an int tensor [N]) silhouette_clusters and silhouette_clusters_samples; with both nmi and ari.  clusters None: the
        model's own clustering -- argmax q(y | x) over the mixture components.  The scores are 0-d device tensors; nothing
        synchronises."""
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
        (Bernoulli likelihood only) --, "code" -- the sampled code transform(images) against the prior draws z* of simulate: does
        the aggregate posterior match the prior, with a p-value, next to latent_diagnostics' KL -- or "both".  A dict per space
        asked for, each mmd_test's (mmd2, p_value, null, witness_x, witness_y, sigma, n_perms, kscale)."""
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
        """Starts p(z | y = k) from a fitted mixture (fit_latent_mixture's or gmvae_amd.mixfit.fit's dict, or (logw, mu, sigma)).
        prior_gmm is a Linear on the one-hot y with no hidden layer, so a table: its bias becomes 0 and row k of its weight (mu_k,
        softplus^-1(max(sigma_k, sigma_min)) - raw_sigma_bias), so that prior_gmm(e_k) = N(mu_k, max(sigma_k, sigma_min)).  p(y)
        STAYS UNIFORM: the fitted weights logw are not used.  Written through state_dict() / load_state_dict(), so whatever the
        engine derives from its parameters is rebuilt.  Adam's slots are left as they are: the call is meant before training or
        between phases.  ValueError for a fit whose K or L is not the model's."""
        from . import mixfit
        e = self._need_engine()
        _, mu, sigma = mixfit.checked_fit(fit, e.K, e.Lz, e.device)
        raw = mixfit.softplus_inverse(sigma.clamp_min(float(e.hp["sigma_min"]))) - float(e.hp["raw_sigma_bias"])
        sd = self.state_dict()
        sd["prior_gmm_fcnet/linear_0/w"] = torch.cat([mu, raw], dim=1)
        sd["prior_gmm_fcnet/linear_0/b"] = torch.zeros(2 * e.Lz, dtype=torch.float32, device=e.device)
        self.load_state_dict(sd)

    def predict_clusters(self, images, n_samples=None):
        """The component the model's posterior p(y | x) assigns each example to: an int64 [B] device tensor.  A model on
        real-valued rows (real_valued=True), whose likelihood the enumerating evaluators refuse, assigns by the inference
        network's q(y | x) instead and takes no n_samples."""
        if self._need_engine().real_valued:
            return self.encoder_y(images).distribution.logits.argmax(dim=1)
        return self.posterior_y(images, n_samples).argmax(dim=1)

    @property
    def summaries(self):
        """nll_scalar, kl_div_z, nent, elbo, cluster_acc of the last run_model
        (scripts/gmvae.py:255,259,264,268,272).  cluster_acc is evaluated lazily,
        like TF evaluates it only when the summary is fetched.  A semi-supervised step with labelled examples adds
        sup_ce (their mean -ln q(y|x)) and sup_acc (the share whose argmax q(y|x) is the observed component); a weighted
        objective adds kl_weight, y_weight and y_floor_share (the share of examples whose y term sits on its free-bits floor);
        clip_norm adds grad_norm and clipped (0 / 1) of the last optimizer step; a likelihood on grey levels adds recon_mse."""
        e = self._need_engine()
        t = e.grads[e.P:].detach()
        out = {"nll_scalar": t[1] / t[4], "kl_div_z": t[2] / t[4], "nent": t[3] / t[4], "elbo": -t[0] / t[4]}
        if e.semi_supervised and t[6].item() > 0:
            out["sup_ce"], out["sup_acc"] = t[5] / t[6], t[7] / t[6]
        if e.weighted_objective:                   # (nll_scalar, kl_div_z and nent stay unweighted; elbo = -loss carries the weights)
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
        if self._last_labels is not None:
            d, ws = e._workspace(int(t[4].item()))
            out["cluster_acc"] = utils.cluster_acc(self.last_logits(), self._last_labels, self.mix_components)
        return out

    def last_logits(self):
        """q_y.distribution.logits of the last run_model batch (read from the step's workspace)."""
        e = self._need_engine()
        x = e._keep[0]
        return e.mlp(L.NET_ENCODER_Y, x)

    @property
    def params(self):
        return self._need_engine().params

    def state_dict(self):
        return self._need_engine().state_dict()

    def load_state_dict(self, sd):
        self._need_engine().load_state_dict(sd)


def create_gmvae(data_size, latent_size, mixture_components=1, fcnet_hidden_sizes=None,
                 hidden_activation_fn=torch.relu, sigma_min=0.001, raw_sigma_bias=0.25, gen_bias_init=0.0,
                 temperature=1.0, random_seed=None, n_samples=1, y_inference="gumbel", grad_estimator="standard",
                 semi_supervised=False, sup_weight=1.0, weighted_objective=False, kl_weight=1.0, y_weight=1.0, y_free_nats=0.0,
                 temperature_on_device=False, y_estimator="relaxed", pixel_mask=False, clip_norm=None, likelihood="bernoulli",
                 likelihood_sigma=1.0, real_valued=None, likelihood_scale="fixed"):
    """Factory with the signature of scripts/gmvae.py:277-287 (+ n_samples, y_inference, grad_estimator, semi_supervised,
    sup_weight, weighted_objective, kl_weight, y_weight, y_free_nats, temperature_on_device, y_estimator, pixel_mask, clip_norm, likelihood, likelihood_sigma, real_valued, likelihood_scale: Engine).  y_inference="marginal" trains and
    evaluates the objective with y summed out exactly over the K components (Engine); "marginal_iw" the same with z
    importance-weighted over n_samples samples per component.  The parameters and their names are the same in every mode, so
    a checkpoint of any loads in the others."""
    if fcnet_hidden_sizes is None:
        fcnet_hidden_sizes = [latent_size]                     # scripts/gmvae.py:316-317
    engine = Engine("gmvae", data_size, latent_size, mixture_components, fcnet_hidden_sizes, n_samples=n_samples,
                    sigma_min=sigma_min, raw_sigma_bias=raw_sigma_bias, temperature=temperature,
                    gen_bias_init=gen_bias_init, random_seed=random_seed, hidden_act=base.activation_name(hidden_activation_fn),
                    y_inference=y_inference, grad_estimator=grad_estimator, semi_supervised=semi_supervised,
                    sup_weight=sup_weight, weighted_objective=weighted_objective, kl_weight=kl_weight, y_weight=y_weight,
                    y_free_nats=y_free_nats, temperature_on_device=temperature_on_device, y_estimator=y_estimator,
                    pixel_mask=pixel_mask, clip_norm=clip_norm, likelihood=likelihood, likelihood_sigma=likelihood_sigma,
                    real_valued=real_valued, likelihood_scale=likelihood_scale)
    prior_gmm = base.ConditionalNormal(size=latent_size, hidden_layer_sizes=None,
                                       hidden_activation_fn=hidden_activation_fn, sigma_min=sigma_min,
                                       raw_sigma_bias=raw_sigma_bias, name="prior_gmm").bind(engine, L.NET_PRIOR_GMM)
    decoder = base.ConditionalBernoulli(size=data_size, hidden_layer_sizes=fcnet_hidden_sizes,
                                        hidden_activation_fn=hidden_activation_fn, bias_init=gen_bias_init,
                                        name="decoder").bind(engine, L.NET_DECODER)
    encoder_y = base.ConditionalCategorical(size=mixture_components, temperature=temperature,
                                            hidden_layer_sizes=fcnet_hidden_sizes,
                                            hidden_activation_fn=hidden_activation_fn,
                                            name="encoder_y").bind(engine, L.NET_ENCODER_Y)
    encoder_gmm = base.ConditionalNormal(size=latent_size, hidden_layer_sizes=fcnet_hidden_sizes,
                                         hidden_activation_fn=hidden_activation_fn, sigma_min=sigma_min,
                                         raw_sigma_bias=raw_sigma_bias, name="encoder_gmm").bind(engine, L.NET_ENCODER_GMM)
    model = TrainableGMVAE(mixture_components, prior_gmm, decoder, encoder_y, encoder_gmm, random_seed=random_seed)
    model._engine = engine
    return model
