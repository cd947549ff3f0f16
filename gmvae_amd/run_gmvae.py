"""`python -m gmvae_amd.run_gmvae` -- the flag table of scripts/run_gmvae.py:11-58 (same names, defaults)."""
import argparse
import os

from . import runners


def build_parser():
    p = argparse.ArgumentParser(description=__doc__)
    a = p.add_argument
    a("--mode", default="train", choices=["train", "eval"])
    a("--model", default="gmvae", choices=["gmvae", "vae", "vae_gmp"])
    a("--latent_size", type=int, default=8)
    a("--hidden_size", type=int, default=64)
    a("--num_layers", type=int, default=1)
    a("--mixture_components", type=int, default=10)
    a("--batch_size", type=int, default=16)
    a("--logdir", default="/tmp/smc_vi")
    a("--random_seed", type=int, default=None)          # any int, including 0, is honoured (the reference drops 0)
    a("--learning_rate", type=float, default=0.001)
    a("--max_steps", type=int, default=int(1e9))
    a("--early_stop_rounds", type=int, default=1000)
    a("--early_stop_threshold", type=float, default=0.001)
    a("--summarise_every", type=int, default=50)
    a("--gpu_id", default="0")                          # index INTO --gpu_num's list (runners.select_device); a launcher's
    a("--gpu_num", default="0")                         # LOCAL_RANK takes precedence (one process per GPU)
    a("--num_samples", type=int, default=10)            # eval prior draws (NOT IWAE samples)
    a("--num_generations", type=int, default=10)
    a("--split", default="train", choices=["train", "test"])
    # build-side additions
    a("--n_samples", type=int, default=1, help="IWAE samples per x (SURVEY.md A15); 1 == the reference")
    a("--data_dim", type=int, default=784)
    a("--data_dir", default=None, help="directory with mnist.npz or the IDX files; synthetic data otherwise")
    a("--synthetic_size", type=int, default=8192)
    a("--eager", action="store_true", help="eager launches instead of summarise_every-aligned train graphs")
    a("--checkpoint_poll_seconds", type=float, default=60.0)     # eval: scripts/utils.py:100-111 sleeps 60 s
    a("--checkpoint_max_wait", type=float, default=None, help="eval: give up waiting after this many seconds")
    a("--iw_samples", type=int, default=0, help="eval: also report the importance-weighted bound at this many samples per "
      "example, streamed in chunks (Engine.iw_bound); 0 = off")
    a("--iw_chunk", type=int, default=None, help="eval: samples per chunk of --iw_samples, --iw_enum_samples, "
      "--posterior_samples and --component_posterior_samples (default: ~51,200 rows per pass)")
    a("--iw_enum_samples", type=int, default=0, help="eval, gmvae (either --y_inference): also report the importance-weighted "
      "bound with y summed out over the mixture components at this many samples per example and component "
      "(Engine.iw_bound_enum_y); 0 = off")
    a("--ais_chains", type=int, default=0, help="eval: also estimate log p(x) by annealed importance sampling with HMC transitions "
      "from the generative model alone (Engine.ais_bound), this many chains per example; reports ais_log_px, the chains' "
      "effective sample size and acceptance rate, and the gap to the importance-weighted bound when --iw_samples (gmvae: "
      "--iw_enum_samples) is given too; needs --ais_temps; 0 = off")
    a("--ais_temps", type=int, default=0, help="--ais_chains: the number of temperatures of the annealing path")
    a("--ais_leapfrog", type=int, default=10, help="--ais_chains: leapfrog steps per HMC transition")
    a("--ais_step_size", type=float, default=0.05, help="--ais_chains: the initial leapfrog step size (adapted per chain)")
    a("--ais_init", default="prior", choices=["prior", "encoder"], help="--ais_chains: the chains' base distribution")
    a("--ais_schedule", default="sigmoid", choices=["sigmoid", "linear"], help="--ais_chains: the annealing path")
    a("--bdmc_examples", type=int, default=0, help="eval, with --ais_chains / --ais_temps: bidirectional Monte Carlo (Engine.bdmc_gap) on "
      "this many examples SIMULATED from the model, at the --ais_* settings: reverse AIS chains from each example's exact "
      "posterior sample give an upper bound on log p(x) beside ais_bound's lower one; reports bdmc_lower, bdmc_upper, bdmc_gap and "
      "the reverse chains' effective sample size and acceptance rate.  The upper bound exists only for simulated data; the gap "
      "bounds the bias of ais_log_px at these settings on data distributed as the model's own samples; 0 = off")
    a("--refine_steps", type=int, default=0, help="eval: also split the inference gap by refining q(z|x) per example with this many "
      "steps of Adam ascent on the example's own ELBO (Engine.inference_gaps); reports elbo_amortised, elbo_refined, "
      "iw_bound_refined, amortisation_gap and approximation_gap over the split (--ais_chains: ais_log_px joins log_px); 0 = off")
    a("--refine_samples", type=int, default=4, help="--refine_steps: Monte-Carlo samples per step (1, 2, 4, 8 or 16)")
    a("--refine_lr", type=float, default=0.05, help="--refine_steps: Adam's learning rate")
    a("--refine_eval_samples", type=int, default=256, help="--refine_steps: samples per example of the closing evaluation")
    a("--posterior_samples", type=int, default=0, help="eval, gmvae (either --y_inference): also report the model's own "
      "posterior p(y|x) by importance sampling at this many samples per example and component (Engine.posterior_y) -- its "
      "clustering accuracy next to q(y|x)'s, its entropy, KL(q(y|x) || p(y|x)) and the effective sample size; 0 = off")
    a("--component_posterior_samples", type=int, default=0, help="eval, vae_gmp: also report the model's own posterior "
      "p(k|x) over the components of its mixture prior by importance sampling at this many samples per example "
      "(Engine.posterior_component) -- its clustering accuracy, its entropy, KL(p(k|x) || pi) and the effective sample size; "
      "0 = off")
    a("--latent_diagnostics", type=int, default=0, help="eval: also report the aggregate posterior's diagnostics over the first "
      "N examples of the split (Engine.aggregate_posterior) -- the mutual information I(x; z), KL(q(z) || p(z)), the total "
      "correlation of q(z), their sum kl_avg, the active units, and for gmvae I(x; y) and the entropy of q(y); 0 = off")
    a("--embed_latent", type=int, default=0, help="eval: also embed the latent code of the first N examples of the split in two "
      "dimensions by exact t-SNE on the device (gmvae_amd.tsne.embed; the reference's utils.reduce_dimensionality) -- "
      "latent_embedding, samples_embedding (the prior draws, where --num_samples allows the perplexity) and embedding_kl; 0 = off")
    a("--tsne_perplexity", type=float, default=40.0, help="--embed_latent: the perplexity (the reference's 40)")
    a("--tsne_iters", type=int, default=300, help="--embed_latent: the iterations (the reference's 300)")
    a("--embedding_out", default=None, help="--embed_latent: write latent_embedding to this .npy file")
    a("--fit_latent_mixture", type=int, default=0, help="eval: also fit a diagonal Gaussian mixture of --mixture_components "
      "components by EM on the device to the latent code of the first N examples of the split (gmvae_amd.mixfit.fit; seed "
      "--random_seed, or 0) and assign the whole split -- latent_mixture_loglik, cluster_acc_latent_mixture (the VAE + GMM "
      "baseline) and latent_mixture; 0 = off")
    a("--mixture_fit_iters", type=int, default=100, help="--fit_latent_mixture: the EM iterations")
    a("--mixture_fit_inits", type=int, default=1, help="--fit_latent_mixture: the seedings tried; the fit with the largest "
      "log-likelihood is kept")
    a("--mixture_covariance", default="diag", choices=["diag", "full"], help="--fit_latent_mixture: axis-aligned components, or "
      "one full covariance per component (scikit-learn's GaussianMixture default; needs --latent_size <= 128); full: "
      "latent_mixture carries cov and info in place of sigma")
    a("--mixture_bic", action="store_true", help="--fit_latent_mixture: also report latent_mixture_bic, the Bayesian information "
      "criterion of the fit on the examples it was fitted to (scikit-learn's definition; smaller is better)")
    a("--neighbour_scores", type=int, default=0, help="eval: also score the latent code of the first N examples of the split by "
      "its neighbourhoods on the device (gmvae_amd.neighbours) -- knn_acc_loo_{k}, silhouette_labels, and for a clustering the run "
      "has in hand -- gmvae: argmax q(y|x); vae_gmp: the posterior over the prior's components, ONLY together with "
      "--component_posterior_samples; vae: none -- silhouette_clusters, nmi_clusters and ari_clusters; with --fit_latent_mixture the same three for the fitted "
      "mixture's assignment, with --embed_latent embedding_trustworthiness_{k} and embedding_continuity_{k}; 0 = off")
    a("--knn_k", type=int, default=10, help="--neighbour_scores: the number of neighbours k")
    a("--linear_probe", type=int, default=0, help="eval: also fit a linear classifier (softmax regression) on the device to the latent "
      "code of the first N examples of the split and score it on the next --probe_test (gmvae_amd.linprobe) -- linear_probe_acc, "
      "linear_probe_nll, linear_probe_train_acc and linear_probe_grad_max (the convergence readout); 0 = off")
    a("--probe_test", type=int, default=0, help="--linear_probe: the examples scored, those behind the N fitted (0: what is left of "
      "the split, N at most)")
    a("--probe_l2", type=float, default=1e-3, help="--linear_probe: the l2 penalty on the weights")
    a("--probe_iters", type=int, default=300, help="--linear_probe: the iterations")
    a("--probe_labelled_per_class", type=int, default=0, help="--linear_probe: fit on this many labels per class of the N examples, "
      "chosen as --labelled_per_class chooses with --random_seed (the M1 baseline of Kingma et al. 2014); 0 = every label")
    a("--probe_standardize", action="store_true", help="--linear_probe: centre and scale the code per dimension by the fitted rows")
    a("--sample_test", type=int, default=0, help="eval: also run the kernel two-sample test (MMD with a permutation null, on the "
      "device; gmvae_amd.twosample) of N samples of the model against the first N examples of the split -- mmd2_data and mmd_p_data "
      "(the simulated images against the data), mmd2_code and mmd_p_code (the prior's draws against one draw of q(z|x) per example: "
      "does the aggregate posterior match the prior); 0 = off")
    a("--sample_test_perms", type=int, default=1000, help="--sample_test: the splits, the observed one included (the smallest p-value "
      "is 1 / this)")
    a("--sample_test_kernel", default="rbf", choices=["rbf", "energy"], help="--sample_test: the rbf kernel at the median distance "
      "and half and twice it, or the energy distance's kernel -|x - y|")
    a("--sample_test_space", default="data", choices=["data", "code", "both"], help="--sample_test: what is compared")
    a("--sample_distance", type=int, default=0, help="eval: also measure the debiased Sinkhorn divergence (a transport distance under "
      "the cost |u - v|^2 / 2, on the device; gmvae_amd.sinkhorn) between N samples of the model and the first N examples of the "
      "split, on the pairs of samples --sample_test compares -- sinkhorn_data and sinkhorn_code, with sinkhorn_marginal_err_data and "
      "sinkhorn_marginal_err_code (the convergence readout: the divergence is low until it is small); 0 = off")
    a("--sample_distance_space", default="data", choices=["data", "code", "both"], help="--sample_distance: what is compared")
    a("--sinkhorn_blur_rel", type=float, default=0.1, help="--sample_distance: the blur as a fraction of the root-mean-square "
      "distance of the pooled sample (the final temperature is its square); values compare only at equal N and blur")
    a("--sinkhorn_iters", type=int, default=200, help="--sample_distance: the iterations")
    a("--sample_distance_perms", type=int, default=0, help="--sample_distance: with P > 0 also a permutation null of P splits, the "
      "observed one included -- sinkhorn_p_data and sinkhorn_p_code (one library call a split)")
    a("--latent_pca", type=int, default=0, help="eval: also report the principal component spectrum of the latent code of the first N "
      "examples of the split (gmvae_amd.pca.fit on the device) -- latent_pca_dim90 (the components that reach 90 %% of the variance), "
      "latent_pca_participation ((sum lambda)^2 / sum lambda^2), latent_pca_top_ratio, latent_pca_offdiag (the solver's convergence "
      "readout) and latent_pca; 0 = off")
    a("--tsne_init", default="random", choices=["random", "pca"], help="--embed_latent: start from 1e-4 x normals (the default), or "
      "from the code's first two principal components (scikit-learn's default since 1.2)")
    a("--pca_baseline", type=int, default=0, help="--fit_latent_mixture: also the PCA + GMM baseline -- the first N examples as the "
      "encoder reads them, projected on their first k principal components (gmvae_amd.pca), fitted with the same mixture settings -- "
      "pca_mixture_loglik, cluster_acc_pca_mixture and pca_residual_max (the subspace iteration's convergence readout); 0 = off")
    a("--sample_frechet", type=int, default=0, help="eval: also report frechet_code, the Frechet distance (gmvae_amd.pca) between the "
      "Gaussians fitted to the two code samples --sample_test --sample_test_space=code compares, N examples each; needs "
      "--latent_size <= 128; 0 = off")
    a("--y_inference", default="gumbel", choices=["gumbel", "marginal", "marginal_iw"], help="gmvae: one Gumbel-softmax draw "
      "of y (the reference), y summed out exactly over the mixture components, or y summed out with --n_samples importance "
      "samples of z per component (marginal_iw)")
    a("--grad_estimator", default="standard", choices=["standard", "dreg"], help="gradient of the inference network: the "
      "reparameterised one, or the doubly reparameterised one (dreg: Tucker et al. 2018; vae, vae_gmp, and gmvae with "
      "--y_inference=marginal or marginal_iw)")
    a("--labelled_per_class", type=int, default=0, help="gmvae with --y_inference=marginal or marginal_iw: train "
      "semi-supervised -- this many training examples per class show their label to the objective (0 = off)")
    a("--sup_weight", type=float, default=1.0, help="--labelled_per_class: weight of the classification term -ln q(y|x) "
      "of a labelled example")
    a("--kl_weight", type=float, default=1.0, help="train, --n_samples=1: weight of the z term KL(q(z|.) || p(z|.)) of the "
      "objective (beta-VAE)")
    a("--y_weight", type=float, default=1.0, help="train, gmvae, --n_samples=1: weight of the y term KL(q(y|x) || p(y))")
    a("--y_free_nats", type=float, default=0.0, help="train, gmvae, --n_samples=1: free bits on the y term -- an example "
      "whose KL(q(y|x) || p(y)) is below this many nats pays the floor and sends no gradient through it (0 = off)")
    a("--kl_warmup_steps", type=int, default=0, help="train, --n_samples=1: both weights are multiplied by "
      "min(1, (t + 1) / N) during the step with 0-based index t (0 = off)")
    a("--temperature", type=float, default=1.0, help="gmvae, --y_inference=gumbel: the Gumbel-softmax temperature (tau_0 of "
      "the annealing schedule)")
    a("--temperature_min", type=float, default=0.0, help="the schedule's floor tau_min")
    a("--temperature_anneal_rate", type=float, default=0.0, help="r of tau = max(tau_min, tau_0 exp(-r N floor(t / N))) during "
      "the step with 0-based index t (Jang et al. 2017)")
    a("--temperature_anneal_every", type=int, default=0, help="N of the schedule: the temperature changes every N steps "
      "(0 = no annealing)")
    a("--y_estimator", default="relaxed", choices=["relaxed", "straight_through"], help="gmvae, --y_inference=gumbel: the "
      "step consumes the relaxed sample of y, or (straight_through) its one-hot argmax with the relaxed sample's gradient")
    a("--missing_rate", type=float, default=0.0, help="train and eval with missing pixels: every pixel of every dataset row is "
      "missing independently with this probability -- ONE fixed mask per row, the same in train and eval; the loss, the "
      "gradients and --iw_samples count the observed pixels alone, the missing ones are scored as imputation_nll (0 = off)")
    a("--missing_seed", type=int, default=0, help="seed of --missing_rate's masks")
    a("--impute_samples", type=int, default=0, help="eval with --missing_rate: impute the missing pixels by importance sampling "
      "at this many samples per example (Mattei & Frellsen 2019) and report imputation_nll_is, imputation_error_rate_is, "
      "imputation_cond_loglik and imputation_ess next to the one-draw imputation_nll (0 = off)")
    a("--impute_draws", type=int, default=0, help="with --impute_samples: also draw this many multiple imputations per example "
      "by sampling-importance-resampling (0 .. 16) and report the share of distinct draws")
    a("--clip_norm", type=float, default=0.0, help="train: clip the batch-mean gradient by its global norm to this threshold "
      "in front of Adam and skip the steps whose gradient or loss is not finite; the log reports the norm's mean and maximum "
      "and the clipped and skipped shares per summary window (inf: report only; 0 = off)")
    a("--likelihood", default="bernoulli", choices=["bernoulli", "grey_bernoulli", "continuous_bernoulli", "gaussian", "poisson", "negative_binomial"],
      help="the decoder's likelihood: bernoulli on binarised pixels (the reference), or on the GREY levels t = pixel / 255 the "
      "Bernoulli cross-entropy on soft targets (grey_bernoulli), the continuous Bernoulli or a Gaussian with the fixed scale "
      "--likelihood_sigma; train and eval then report recon_mse, the per-pixel squared error of the mean image.  poisson / "
      "negative_binomial: the rows are COUNTS (float32 >= 0 from --data_npy, which is then required), "
      "the decoder's output is the log-mean, the networks read log1p(count); --real_valued is implied, --standardize refused; "
      "recon_mse is then the squared error of log1p(mean) against log1p(count), and the negative binomial learns an inverse "
      "dispersion per dimension (the parameter decoder/log_dispersion, reported as dispersion_mean)")
    a("--likelihood_sigma", type=float, default=1.0, help="--likelihood=gaussian: the fixed scale sigma (with "
      "--likelihood_scale=learned: where every dimension's scale starts)")
    a("--real_valued", action="store_true", help="--likelihood=gaussian: the rows are float feature vectors (embeddings, sensor "
      "vectors, tabular data) fed as they are -- from --data_npy, or a synthetic mixture of Gaussian blobs with labels")
    a("--likelihood_scale", default="fixed", choices=["fixed", "learned"], help="--likelihood=gaussian: one fixed scale, or a "
      "scale per dimension learned with the model (the parameter decoder/log_sigma)")
    a("--data_npy", default=None, help="--real_valued: a .npy file holding the float32 [N, D] rows (train and eval read the same "
      "file); --data_dim follows it")
    a("--labels_npy", default=None, help="--data_npy: a .npy file holding the N integer labels (clustering accuracy only)")
    a("--standardize", action="store_true", help="--real_valued: subtract the per-feature mean and divide by the per-feature "
      "standard deviation of the train rows; both are saved in the checkpoint and applied in eval")
    return p


def check_args(p, cfg):
    """Flag combinations the marginal objective does not take (argument errors, before any device work)."""
    if cfg.iw_enum_samples and cfg.model != "gmvae":
        p.error("--iw_enum_samples sums y out over the mixture components: it needs --model=gmvae")
    if cfg.posterior_samples and cfg.model != "gmvae":
        p.error("--posterior_samples is the posterior over the mixture components: it needs --model=gmvae")
    if cfg.component_posterior_samples:
        if cfg.model != "vae_gmp":
            p.error("--component_posterior_samples is the posterior over the VAE's mixture prior: it needs --model=vae_gmp")
        if cfg.mode != "eval":
            p.error("--component_posterior_samples needs --mode=eval")
    if cfg.latent_diagnostics < 0:
        p.error("--latent_diagnostics must be >= 0 (0 = off)")
    if cfg.latent_diagnostics:
        if cfg.mode != "eval":
            p.error("--latent_diagnostics needs --mode=eval")
        if cfg.missing_rate > 0:
            p.error("--latent_diagnostics is not available with --missing_rate (the encoders it runs take no mask)")
    if cfg.embed_latent < 0:
        p.error("--embed_latent must be >= 0 (0 = off)")
    if cfg.embed_latent:
        if cfg.mode != "eval":
            p.error("--embed_latent needs --mode=eval")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            p.error("--embed_latent embeds one rank's codes: it is not available with more than one rank")
        if cfg.embed_latent < 4 or not 1.0 < cfg.tsne_perplexity < cfg.embed_latent - 1:
            p.error("--embed_latent N needs N >= 4 and --tsne_perplexity in (1, N - 1)")
        if cfg.tsne_iters < 0:
            p.error("--tsne_iters must be >= 0")
    elif cfg.embedding_out:
        p.error("--embedding_out needs --embed_latent")
    if cfg.fit_latent_mixture < 0:
        p.error("--fit_latent_mixture must be >= 0 (0 = off)")
    if cfg.fit_latent_mixture:
        if cfg.mode != "eval":
            p.error("--fit_latent_mixture needs --mode=eval")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            p.error("--fit_latent_mixture fits one rank's codes: it is not available with more than one rank")
        if cfg.fit_latent_mixture < cfg.mixture_components:
            p.error("--fit_latent_mixture N needs N >= --mixture_components")
        if cfg.mixture_fit_iters < 0:
            p.error("--mixture_fit_iters must be >= 0")
        if cfg.mixture_fit_inits < 1:
            p.error("--mixture_fit_inits must be >= 1")
    if cfg.mixture_covariance != "diag":
        if not cfg.fit_latent_mixture:
            p.error("--mixture_covariance needs --fit_latent_mixture")
        if cfg.latent_size > 128:
            p.error("--mixture_covariance=full needs --latent_size <= 128")
        if cfg.mixture_components * cfg.latent_size ** 2 > 1 << 20:
            p.error("--mixture_covariance=full needs --mixture_components * --latent_size^2 <= 2^20")
    if cfg.mixture_bic and not cfg.fit_latent_mixture:
        p.error("--mixture_bic needs --fit_latent_mixture")
    if cfg.neighbour_scores < 0:
        p.error("--neighbour_scores must be >= 0 (0 = off)")
    if cfg.neighbour_scores:
        if cfg.mode != "eval":
            p.error("--neighbour_scores needs --mode=eval")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            p.error("--neighbour_scores scores one rank's codes: it is not available with more than one rank")
        if not 1 <= cfg.knn_k <= 256 or not cfg.neighbour_scores > 2 * cfg.knn_k:
            p.error("--neighbour_scores N needs --knn_k in [1, 256] and N > 2 * --knn_k")
    if cfg.linear_probe < 0:
        p.error("--linear_probe must be >= 0 (0 = off)")
    if cfg.linear_probe:
        if cfg.mode != "eval":
            p.error("--linear_probe needs --mode=eval")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            p.error("--linear_probe fits one rank's codes: it is not available with more than one rank")
        if cfg.latent_size > 128:
            p.error("--linear_probe needs --latent_size <= 128")
        if cfg.probe_test < 0 or cfg.probe_iters < 0 or cfg.probe_labelled_per_class < 0:
            p.error("--probe_test, --probe_iters and --probe_labelled_per_class must be >= 0")
        if not (cfg.probe_l2 > 0 and cfg.probe_l2 < float("inf")):
            p.error("--probe_l2 must be a finite number > 0")
    elif (cfg.probe_test, cfg.probe_l2, cfg.probe_iters, cfg.probe_labelled_per_class, cfg.probe_standardize) != (0, 1e-3, 300, 0, False):
        p.error("--probe_test, --probe_l2, --probe_iters, --probe_labelled_per_class and --probe_standardize need --linear_probe")
    if cfg.sample_test < 0 or cfg.sample_test == 1:
        p.error("--sample_test must be 0 (off) or >= 2")
    if cfg.sample_test:
        if cfg.mode != "eval":
            p.error("--sample_test needs --mode=eval")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            p.error("--sample_test tests one rank's examples: it is not available with more than one rank")
        if not 1 <= cfg.sample_test_perms <= 4096:
            p.error("--sample_test_perms must lie in [1, 4096]")
        if 2 * cfg.sample_test > 1 << 20:
            p.error("--sample_test N needs 2 N <= 2^20")
        if cfg.missing_rate > 0:
            p.error("--sample_test is not available with --missing_rate (the samples have every pixel, and the encoders that draw "
                    "the code take no mask)")
        if cfg.sample_test_space != "code" and cfg.likelihood != "bernoulli":
            p.error("--sample_test compares simulated binary images: --sample_test_space=data and both need the Bernoulli likelihood")
    elif (cfg.sample_test_perms, cfg.sample_test_kernel, cfg.sample_test_space) != (1000, "rbf", "data"):
        p.error("--sample_test_perms, --sample_test_kernel and --sample_test_space need --sample_test")
    if cfg.sample_distance < 0 or cfg.sample_distance == 1:
        p.error("--sample_distance must be 0 (off) or >= 2")
    if cfg.sample_distance:
        if cfg.mode != "eval":
            p.error("--sample_distance needs --mode=eval")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            p.error("--sample_distance compares one rank's examples: it is not available with more than one rank")
        if not 0 <= cfg.sample_distance_perms <= 4096:
            p.error("--sample_distance_perms must lie in [0, 4096]")
        if cfg.sample_distance > 1 << 20:
            p.error("--sample_distance N needs N <= 2^20")
        if not 1 <= cfg.sinkhorn_iters <= 100000:
            p.error("--sinkhorn_iters must lie in [1, 100000]")
        if not (cfg.sinkhorn_blur_rel > 0 and cfg.sinkhorn_blur_rel < float("inf")):
            p.error("--sinkhorn_blur_rel must be a finite number > 0")
        if cfg.missing_rate > 0:
            p.error("--sample_distance is not available with --missing_rate (the samples have every pixel, and the encoders that "
                    "draw the code take no mask)")
        if cfg.sample_distance_space != "code" and cfg.likelihood != "bernoulli":
            p.error("--sample_distance compares simulated binary images: --sample_distance_space=data and both need the Bernoulli "
                    "likelihood")
    elif (cfg.sample_distance_space, cfg.sinkhorn_blur_rel, cfg.sinkhorn_iters, cfg.sample_distance_perms) != ("data", 0.1, 200, 0):
        p.error("--sample_distance_space, --sinkhorn_blur_rel, --sinkhorn_iters and --sample_distance_perms need --sample_distance")
    if cfg.latent_pca < 0 or cfg.latent_pca == 1:
        p.error("--latent_pca must be 0 (off) or >= 2")
    if cfg.latent_pca:
        if cfg.mode != "eval":
            p.error("--latent_pca needs --mode=eval")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            p.error("--latent_pca fits one rank's codes: it is not available with more than one rank")
        if cfg.latent_size > 4096:
            p.error("--latent_pca needs --latent_size <= 4096")
    if cfg.tsne_init != "random" and not cfg.embed_latent:
        p.error("--tsne_init needs --embed_latent")
    if cfg.pca_baseline < 0:
        p.error("--pca_baseline must be >= 0 (0 = off)")
    if cfg.pca_baseline:
        if not cfg.fit_latent_mixture:
            p.error("--pca_baseline needs --fit_latent_mixture")
        if cfg.pca_baseline > 128:
            p.error("--pca_baseline k needs k <= 128")
        if cfg.fit_latent_mixture < 2:
            p.error("--pca_baseline needs --fit_latent_mixture N with N >= 2")
        if cfg.missing_rate > 0:
            p.error("--pca_baseline is not available with --missing_rate (it projects every pixel)")
    if cfg.sample_frechet < 0 or cfg.sample_frechet == 1:
        p.error("--sample_frechet must be 0 (off) or >= 2")
    if cfg.sample_frechet:
        if cfg.mode != "eval":
            p.error("--sample_frechet needs --mode=eval")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            p.error("--sample_frechet compares one rank's examples: it is not available with more than one rank")
        if cfg.latent_size > 128:
            p.error("--sample_frechet needs --latent_size <= 128")
        if cfg.missing_rate > 0:
            p.error("--sample_frechet is not available with --missing_rate (the encoders that draw the code take no mask)")
    if cfg.ais_chains < 0 or cfg.ais_temps < 0:
        p.error("--ais_chains and --ais_temps must be >= 0 (0 = off)")
    if bool(cfg.ais_chains) != bool(cfg.ais_temps):
        p.error("--ais_chains and --ais_temps go together")
    if cfg.ais_chains:
        if cfg.mode != "eval":
            p.error("--ais_chains needs --mode=eval")
        if cfg.ais_leapfrog < 1 or not (cfg.ais_step_size > 0 and cfg.ais_step_size < float("inf")):
            p.error("--ais_leapfrog must be >= 1 and --ais_step_size a finite number > 0")
        if cfg.missing_rate > 0 or cfg.likelihood != "bernoulli":
            p.error("--ais_chains scores the Bernoulli likelihood on every pixel: not available with --missing_rate or --likelihood")
    if cfg.bdmc_examples < 0:
        p.error("--bdmc_examples must be >= 0 (0 = off)")
    if cfg.bdmc_examples and not cfg.ais_chains:
        p.error("--bdmc_examples runs at the --ais_* settings: it needs --ais_chains and --ais_temps")
    if cfg.refine_steps < 0:
        p.error("--refine_steps must be >= 0 (0 = off)")
    if not cfg.refine_steps and (cfg.refine_samples, cfg.refine_lr, cfg.refine_eval_samples) != (4, 0.05, 256):
        p.error("--refine_samples, --refine_lr and --refine_eval_samples need --refine_steps")
    if cfg.refine_steps:
        if cfg.mode != "eval":
            p.error("--refine_steps needs --mode=eval")
        if cfg.refine_samples not in (1, 2, 4, 8, 16) or cfg.refine_eval_samples < 1:
            p.error("--refine_samples must be 1, 2, 4, 8 or 16 and --refine_eval_samples >= 1")
        if not (cfg.refine_lr > 0 and cfg.refine_lr < float("inf")):
            p.error("--refine_lr must be a finite number > 0")
        if cfg.missing_rate > 0 or cfg.likelihood != "bernoulli":
            p.error("--refine_steps scores the Bernoulli likelihood on every pixel: not available with --missing_rate or --likelihood")
    if cfg.y_inference == "marginal":
        if cfg.model != "gmvae":
            p.error("--y_inference=marginal needs --model=gmvae")
        if cfg.n_samples != 1:
            p.error("--y_inference=marginal enumerates y: --n_samples must be 1")
        if cfg.iw_samples:
            p.error("--iw_samples is not available with --y_inference=marginal")
    if cfg.y_inference == "marginal_iw":
        if cfg.model != "gmvae":
            p.error("--y_inference=marginal_iw needs --model=gmvae")
        if cfg.n_samples < 1:
            p.error("--y_inference=marginal_iw: --n_samples must be >= 1")
        if cfg.iw_samples:
            p.error("--iw_samples is not available with --y_inference=marginal_iw (use --iw_enum_samples)")
    if cfg.grad_estimator == "dreg" and cfg.model == "gmvae" and cfg.y_inference == "gumbel":
        p.error("--grad_estimator=dreg is not available for --model=gmvae with --y_inference=gumbel: use "
                "--y_inference=marginal or marginal_iw")
    if cfg.labelled_per_class < 0 or cfg.sup_weight < 0:
        p.error("--labelled_per_class and --sup_weight must be >= 0")
    if cfg.labelled_per_class > 0 and (cfg.model != "gmvae" or cfg.y_inference == "gumbel"):
        p.error("--labelled_per_class needs --model=gmvae with --y_inference=marginal or marginal_iw")
    if cfg.kl_weight < 0 or cfg.y_weight < 0 or cfg.y_free_nats < 0 or cfg.kl_warmup_steps < 0:
        p.error("--kl_weight, --y_weight, --y_free_nats and --kl_warmup_steps must be >= 0")
    if runners.weighted_flags(cfg):
        if cfg.n_samples > 1:
            p.error("--kl_weight / --y_weight / --y_free_nats / --kl_warmup_steps weight the one-sample bound: --n_samples must be 1")
        if cfg.y_inference == "marginal_iw":
            p.error("--kl_weight / --y_weight / --y_free_nats / --kl_warmup_steps are not available with --y_inference=marginal_iw")
        if cfg.grad_estimator == "dreg":
            p.error("--kl_weight / --y_weight / --y_free_nats / --kl_warmup_steps are not available with --grad_estimator=dreg")
        if cfg.labelled_per_class > 0:
            p.error("--kl_weight / --y_weight / --y_free_nats / --kl_warmup_steps are not available with --labelled_per_class")
    if runners.temperature_flags(cfg) or cfg.y_estimator != "relaxed":
        if cfg.model != "gmvae" or cfg.y_inference != "gumbel":
            p.error("--temperature, --temperature_min, --temperature_anneal_rate, --temperature_anneal_every and --y_estimator "
                    "belong to the Gumbel-softmax draw of y: they need --model=gmvae with --y_inference=gumbel")
    if not cfg.temperature > 0 or cfg.temperature_min < 0 or cfg.temperature_anneal_rate < 0 or cfg.temperature_anneal_every < 0:
        p.error("--temperature must be > 0; --temperature_min, --temperature_anneal_rate and --temperature_anneal_every >= 0")
    if cfg.temperature_anneal_rate > 0 and cfg.temperature_anneal_every > 0 and not cfg.temperature_min > 0:
        p.error("an annealed temperature needs a floor: --temperature_min must be > 0")
    if not cfg.clip_norm >= 0:
        p.error("--clip_norm must be >= 0 (0 = off)")
    if not 0.0 <= cfg.missing_rate < 1.0:
        p.error("--missing_rate must be in [0, 1)")
    if cfg.missing_rate > 0:
        if cfg.model == "gmvae" and cfg.y_inference != "gumbel":
            p.error("--missing_rate is not available with --y_inference=marginal or marginal_iw")
        if cfg.grad_estimator == "dreg":
            p.error("--missing_rate is not available with --grad_estimator=dreg")
        if cfg.labelled_per_class > 0:
            p.error("--missing_rate is not available with --labelled_per_class")
        if runners.weighted_flags(cfg):
            p.error("--missing_rate is not available with --kl_weight / --y_weight / --y_free_nats / --kl_warmup_steps")
        if runners.temperature_flags(cfg) or cfg.y_estimator != "relaxed":
            p.error("--missing_rate is not available with --temperature* or --y_estimator=straight_through")
        if cfg.iw_enum_samples or cfg.posterior_samples or cfg.component_posterior_samples:
            p.error("--missing_rate is not available with --iw_enum_samples, --posterior_samples or "
                    "--component_posterior_samples (they would score the unobserved pixels): use --iw_samples")
    if cfg.impute_samples < 0 or not 0 <= cfg.impute_draws <= 16:
        p.error("--impute_samples must be >= 0 and --impute_draws in 0 .. 16")
    if cfg.impute_draws and not cfg.impute_samples:
        p.error("--impute_draws needs --impute_samples")
    if cfg.impute_samples and not (cfg.mode == "eval" and cfg.missing_rate > 0):
        p.error("--impute_samples needs --mode=eval and --missing_rate > 0")
    if not (cfg.likelihood_sigma > 0 and cfg.likelihood_sigma < float("inf")):
        p.error("--likelihood_sigma must be a finite number > 0")
    if cfg.likelihood != "bernoulli":
        what = f"--likelihood={cfg.likelihood}"
        if cfg.model == "gmvae" and cfg.y_inference != "gumbel":
            p.error(f"{what} is not available with --y_inference=marginal or marginal_iw")
        if cfg.grad_estimator == "dreg":
            p.error(f"{what} is not available with --grad_estimator=dreg")
        if cfg.labelled_per_class > 0:
            p.error(f"{what} is not available with --labelled_per_class")
        if runners.weighted_flags(cfg):
            p.error(f"{what} is not available with --kl_weight / --y_weight / --y_free_nats / --kl_warmup_steps")
        if runners.temperature_flags(cfg) or cfg.y_estimator != "relaxed":
            p.error(f"{what} is not available with --temperature* or --y_estimator=straight_through")
        if cfg.missing_rate > 0:
            p.error(f"{what} is not available with --missing_rate")
        if cfg.iw_enum_samples or cfg.posterior_samples or cfg.component_posterior_samples:
            p.error(f"{what} is not available with --iw_enum_samples, --posterior_samples or --component_posterior_samples "
                    "(they would score Bernoulli): use --iw_samples")
    if cfg.likelihood in ("poisson", "negative_binomial"):
        if cfg.standardize:
            p.error(f"--standardize is not available with --likelihood={cfg.likelihood}: counts are fed as they are")
        if not cfg.data_npy:
            p.error(f"--likelihood={cfg.likelihood} needs --data_npy: a float32 [N, D] file of counts (runners.synthetic_counts "
                    "makes a stand-in)")
        cfg.real_valued = True      # (implied: float rows)
    if cfg.real_valued and cfg.likelihood not in ("gaussian", "poisson", "negative_binomial"):
        p.error("--real_valued needs --likelihood=gaussian")
    if cfg.likelihood_scale == "learned" and cfg.likelihood != "gaussian":
        p.error("--likelihood_scale=learned needs --likelihood=gaussian")
    if (cfg.data_npy or cfg.standardize) and not cfg.real_valued:
        p.error("--data_npy and --standardize need --real_valued")
    if cfg.labels_npy and not cfg.data_npy:
        p.error("--labels_npy needs --data_npy")
    if cfg.data_npy:
        try:
            shape = runners.npy_shape(cfg.data_npy)
        except (OSError, ValueError) as e:
            p.error(f"--data_npy: {e}")
        if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
            p.error(f"--data_npy must hold a float32 [N, D] array, got shape {shape}")
        cfg.data_dim = int(shape[1])
    return cfg


def main(argv=None):
    p = build_parser()
    cfg = check_args(p, p.parse_args(argv))
    return runners.run_train(cfg) if cfg.mode == "train" else runners.run_eval(cfg)


if __name__ == "__main__":
    main()
