"""Host-side owner of the flat parameter buffer and driver of the HIP step.

Python / PyTorch here is plumbing only (device memory, streams, RCCL via
torch.distributed, hipGraph capture through torch.cuda.graph).  All arithmetic
of the hot path happens inside libgmvae_hip.so; there is no CPU fallback.

Replaces, for one device: the TF graph that scripts/runners.py:162-185 builds
(model -> loss -> AdamOptimizer.compute_gradients / apply_gradients) and the
``sess.run([train_op, global_step])`` of scripts/runners.py:231-232.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Dict, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib as L


class _ElboFn(torch.autograd.Function):
    """loss = mean_b loss_b with d loss / d params delivered by the fused HIP
    forward+backward (the backward pass has already run when this returns)."""

    @staticmethod
    def forward(ctx, params, engine, x, eps, u, y_observed=None, mask=None):
        buf = engine.step(x, eps, u, y_observed=y_observed, mask=mask)
        P = engine.P
        ctx.engine_buf = buf
        ctx.P = P
        return buf[P] / buf[P + 4]

    @staticmethod
    def backward(ctx, grad_out):
        buf, P = ctx.engine_buf, ctx.P
        return buf[:P] * (grad_out / buf[P + 4]), None, None, None, None, None, None


def check_semi_supervised(model, y_inference, semi_supervised, sup_weight):
    """The argument check of Engine(semi_supervised=, sup_weight=) (no device needed)."""
    if not semi_supervised:
        return
    if L.MODEL_IDS.get(model) != L.MODEL_GMVAE:
        raise ValueError("semi_supervised=True clamps the GMVAE's y to observed components: it needs the GMVAE model")
    if y_inference == "gumbel":
        raise ValueError("semi_supervised=True needs y summed out: use y_inference='marginal' or 'marginal_iw'")
    if not float(sup_weight) >= 0.0:
        raise ValueError(f"sup_weight must be >= 0, got {sup_weight!r}")


def check_weighted_objective(model, y_inference, n_samples, grad_estimator, semi_supervised, weighted_objective,
                             kl_weight, y_weight, y_free_nats):
    """The argument check of Engine(weighted_objective=, kl_weight=, y_weight=, y_free_nats=) (no device needed)."""
    for name, v in (("kl_weight", kl_weight), ("y_weight", y_weight), ("y_free_nats", y_free_nats)):
        if not (float(v) >= 0.0 and math.isfinite(float(v))):
            raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
    if not weighted_objective:
        if (float(kl_weight), float(y_weight), float(y_free_nats)) != (1.0, 1.0, 0.0):
            raise ValueError("kl_weight, y_weight and y_free_nats need weighted_objective=True")
        return
    if int(n_samples) != 1:
        raise ValueError("weighted_objective=True weights the terms of the one-sample bound: n_samples must be 1")
    if y_inference == "marginal_iw":
        raise ValueError("weighted_objective=True is not available with y_inference='marginal_iw': use 'gumbel' or 'marginal'")
    if grad_estimator == "dreg":
        raise ValueError("weighted_objective=True is not available with grad_estimator='dreg'")
    if semi_supervised:
        raise ValueError("weighted_objective=True is not available with semi_supervised=True")


def check_y_head(model, y_inference, temperature, temperature_on_device, y_estimator):
    """The argument check of Engine(temperature=, temperature_on_device=, y_estimator=) (no device needed)."""
    if y_estimator not in L.Y_ESTIMATORS:
        raise ValueError(f"y_estimator must be one of {L.Y_ESTIMATORS}, got {y_estimator!r}")
    t = float(temperature)
    if not (t > 0.0 and math.isfinite(t)):
        raise ValueError(f"temperature must be a finite number > 0, got {temperature!r}")
    if not temperature_on_device and y_estimator == "relaxed":
        return
    what = "temperature_on_device=True" if temperature_on_device else f"y_estimator={y_estimator!r}"
    if L.MODEL_IDS.get(model) != L.MODEL_GMVAE:
        raise ValueError(f"{what} belongs to the GMVAE's Gumbel-softmax draw of y: it needs the GMVAE model")
    if y_inference != "gumbel":
        raise ValueError(f"{what} needs y_inference='gumbel': y_inference={y_inference!r} sums y out and draws none")


def check_pixel_mask(model, y_inference, grad_estimator, semi_supervised, weighted_objective, temperature_on_device,
                     y_estimator, pixel_mask):
    """The argument check of Engine(pixel_mask=) (no device needed): the library's refusals of GMVAE_OBJ_PIXEL_MASK."""
    if not pixel_mask:
        return
    if L.MODEL_IDS.get(model) == L.MODEL_GMVAE and y_inference != "gumbel":
        raise ValueError(f"pixel_mask=True is not available with y_inference={y_inference!r}: use 'gumbel'")
    if grad_estimator == "dreg":
        raise ValueError("pixel_mask=True is not available with grad_estimator='dreg'")
    if semi_supervised:
        raise ValueError("pixel_mask=True is not available with semi_supervised=True")
    if weighted_objective:
        raise ValueError("pixel_mask=True is not available with weighted_objective=True")
    if temperature_on_device:
        raise ValueError("pixel_mask=True is not available with temperature_on_device=True")
    if y_estimator != "relaxed":
        raise ValueError(f"pixel_mask=True is not available with y_estimator={y_estimator!r}")


def check_likelihood(model, y_inference, grad_estimator, semi_supervised, weighted_objective, temperature_on_device,
                     y_estimator, pixel_mask, likelihood, likelihood_sigma=1.0):
    """The argument check of Engine(likelihood=, likelihood_sigma=) and set_likelihood_sigma (no device needed): the library's
    refusals of GMVAE_LIK_*.  Returns sigma as a float."""
    if likelihood not in L.LIKELIHOODS:
        raise ValueError(f"likelihood must be one of {tuple(L.LIKELIHOODS)}, got {likelihood!r}")
    try:
        sigma = float(likelihood_sigma)
    except (TypeError, ValueError):
        raise ValueError(f"likelihood_sigma must be a finite number > 0, got {likelihood_sigma!r}") from None
    if not (sigma > 0.0 and math.isfinite(sigma)):
        raise ValueError(f"likelihood_sigma must be a finite number > 0, got {likelihood_sigma!r}")
    if likelihood == "bernoulli":
        return sigma
    _check_likelihood_alone(model, y_inference, grad_estimator, semi_supervised, weighted_objective, temperature_on_device,
                            y_estimator, pixel_mask, likelihood)
    return sigma


def check_count_likelihood(model, y_inference, grad_estimator, semi_supervised, weighted_objective, temperature_on_device,
                           y_estimator, pixel_mask, likelihood):
    """The argument check of Engine(likelihood="poisson" | "negative_binomial") (no device needed): the library's refusals of
    GMVAE_LIK_POISSON / GMVAE_LIK_NEG_BINOMIAL -- those of GMVAE_LIK_*."""
    if likelihood not in L.COUNT_LIKELIHOODS:
        raise ValueError(f"likelihood must be one of {tuple(L.COUNT_LIKELIHOODS)}, got {likelihood!r}")
    _check_likelihood_alone(model, y_inference, grad_estimator, semi_supervised, weighted_objective, temperature_on_device,
                            y_estimator, pixel_mask, likelihood)


def _check_likelihood_alone(model, y_inference, grad_estimator, semi_supervised, weighted_objective, temperature_on_device,
                            y_estimator, pixel_mask, likelihood):
    what = f"likelihood={likelihood!r}"
    if L.MODEL_IDS.get(model) == L.MODEL_GMVAE and y_inference != "gumbel":
        raise ValueError(f"{what} is not available with y_inference={y_inference!r}: use 'gumbel'")
    if grad_estimator == "dreg":
        raise ValueError(f"{what} is not available with grad_estimator='dreg'")
    if semi_supervised:
        raise ValueError(f"{what} is not available with semi_supervised=True")
    if weighted_objective:
        raise ValueError(f"{what} is not available with weighted_objective=True")
    if temperature_on_device:
        raise ValueError(f"{what} is not available with temperature_on_device=True")
    if y_estimator != "relaxed":
        raise ValueError(f"{what} is not available with y_estimator={y_estimator!r}")
    if pixel_mask:
        raise ValueError(f"{what} is not available with pixel_mask=True")


IMPUTE_MAX_DRAWS = 16


def check_impute_args(model, y_inference, likelihood, pixel_mask, n_samples, n_draws=0, has_mask=False):
    """The argument check of Engine.impute_posterior (no device needed): the library's refusals of gmvae_impute.  Returns
    (n_samples, n_draws) as ints."""
    if L.MODEL_IDS.get(model) == L.MODEL_GMVAE and y_inference != "gumbel":
        raise ValueError(f"impute_posterior is not available with y_inference={y_inference!r} (its weights are the Gumbel "
                         "objective's, as iw_bound's)")
    if likelihood != "bernoulli":
        raise ValueError(f"impute_posterior is not available with likelihood={likelihood!r} (it imputes Bernoulli pixels)")
    try:
        n, m = int(n_samples), int(n_draws)
    except (TypeError, ValueError):
        raise ValueError(f"n_samples and n_draws must be integers, got {n_samples!r}, {n_draws!r}") from None
    if n < 1:
        raise ValueError(f"n_samples must be >= 1, got {n}")
    if not 0 <= m <= IMPUTE_MAX_DRAWS:
        raise ValueError(f"n_draws must be in 0 .. {IMPUTE_MAX_DRAWS}, got {m}")
    if has_mask and not pixel_mask:
        raise ValueError("impute_posterior(mask=) needs an engine created with pixel_mask=True")
    return n, m


LIKELIHOOD_SCALES = ("fixed", "learned")


def check_real_valued(likelihood, real_valued=None, likelihood_scale="fixed"):
    """The argument check of Engine(real_valued=, likelihood_scale=) (no device needed): the library's refusals of GMVAE_X_F32
    and GMVAE_LIK_SCALE_LEARNED -- both need the Gaussian likelihood (whose own refusals check_likelihood holds)."""
    if likelihood_scale not in LIKELIHOOD_SCALES:
        raise ValueError(f"likelihood_scale must be one of {LIKELIHOOD_SCALES}, got {likelihood_scale!r}")
    if likelihood in L.COUNT_LIKELIHOODS:
        # counts (GMVAE_LIK_POISSON / GMVAE_LIK_NEG_BINOMIAL): float rows are implied -- an explicit False contradicts it
        if real_valued is not None and not real_valued:
            raise ValueError(f"likelihood={likelihood!r} takes float count rows: real_valued=False contradicts it")
        if likelihood_scale == "learned":
            raise ValueError(f"likelihood_scale='learned' needs likelihood='gaussian', got likelihood={likelihood!r}")
        return
    if real_valued and likelihood != "gaussian":
        raise ValueError(f"real_valued=True needs likelihood='gaussian', got likelihood={likelihood!r}")
    if likelihood_scale == "learned" and likelihood != "gaussian":
        raise ValueError(f"likelihood_scale='learned' needs likelihood='gaussian', got likelihood={likelihood!r}")


def check_clip_norm(clip_norm):
    """The argument check of Engine(clip_norm=) and set_clip_norm (no device needed): None (off) or a threshold > 0; inf reports
    the norm and never clips.  Returns the value as a float, or None."""
    if clip_norm is None:
        return None
    try:
        c = float(clip_norm)
    except (TypeError, ValueError):
        raise ValueError(f"clip_norm must be None or a number > 0, got {clip_norm!r}") from None
    if not c > 0.0:                              # (NaN fails the comparison too)
        raise ValueError(f"clip_norm must be None or a number > 0 (inf: report only), got {clip_norm!r}")
    return c


AIS_SCHEDULES = ("sigmoid", "linear")


def ais_schedule(schedule, n_temps: int) -> torch.Tensor:
    """The annealing path of Engine.ais_bound as a float64 CPU tensor beta_0 = 0 < ... < beta_T = 1: "linear" -- t / T --,
    "sigmoid" -- (s(4 (2 t / T - 1)) - s(-4)) / (s(4) - s(-4)), s the logistic function (Wu et al. 2017: more temperatures near
    both ends) -- or a tensor of n_temps + 1 values, which is checked."""
    T = int(n_temps)
    if isinstance(schedule, str):
        if schedule not in AIS_SCHEDULES:
            raise ValueError(f"schedule must be one of {AIS_SCHEDULES} or a tensor, got {schedule!r}")
        t = torch.arange(T + 1, dtype=torch.float64)
        if schedule == "linear":
            b = t / T
        else:
            s = lambda v: torch.sigmoid(torch.as_tensor(v, dtype=torch.float64))
            b = (s(4.0 * (2.0 * t / T - 1.0)) - s(-4.0)) / (s(4.0) - s(-4.0))
        b[0], b[-1] = 0.0, 1.0
        return b
    b = torch.as_tensor(schedule).detach().to("cpu", torch.float64).reshape(-1)
    if b.numel() != T + 1 or float(b[0]) != 0.0 or float(b[-1]) != 1.0 or not bool((b[1:] > b[:-1]).all()):
        raise ValueError(f"a schedule tensor holds n_temps + 1 = {T + 1} increasing values from 0 to 1")
    return b


def _check_labels(engine, y_observed, B):
    if y_observed.dtype.is_floating_point or y_observed.dtype == torch.bool or y_observed.numel() != B:
        raise ValueError(f"y_observed must be an int tensor of {B} observed components (-1: unlabelled)")
    return y_observed


def _check_mask(engine, mask, B):
    mask = mask.to(engine.device)
    if mask.dtype.is_floating_point or mask.numel() != B * engine.D:
        raise ValueError(f"mask must be a uint8 / bool tensor [{B}, {engine.D}] (non-zero: observed)")
    return mask != 0


class StepInput(NamedTuple):
    """A per-step side input of the training step (DESIGN.md "Per-step inputs"): a read-only workspace region of LABEL_SLOTS
    slots.  Step i of a train graph reads slot i; every eager entry writes slot 0 before it runs; a captured graph hands the
    caller the view [:n_steps] of the region as replay.<replay>."""
    option: str                             # the Engine attribute (and constructor argument) that enables it
    bit: int                                # the sched_flags bit the dims carry for a step to read it
    region: str                             # the workspace region (gmvae_workspace_offset)
    replay: str                             # the attribute of a captured graph's replay
    dtype: torch.dtype
    stride: Callable[[int, int], int]       # (B, D) -> elements from one slot to the next
    shape: Callable[[int, int], tuple]      # (B, D) -> the visible part of a slot
    held: Optional[str]                     # an eager call's slot 0: this engine-held device tensor (also a fresh region's value)
    arg: Optional[str]                      # ... or this call argument,
    check: Optional[Callable]               #     validated by check(engine, value, B),
    absent: Optional[int]                   #     None (and a fresh region) meaning this value
    noun: str                               # what a slot holds, for the refusals
    tag: str                                # gmvae_step_schedule's suffix, run_train.last_path's "graph+<tag>"


STEP_INPUTS: Tuple[StepInput, ...] = (
    StepInput(option="semi_supervised", bit=L.OBJ_LABELS, region="labels", replay="y_observed", dtype=torch.int32,
              stride=lambda B, D: (B + 3) // 4 * 4, shape=lambda B, D: (B,),
              held=None, arg="y_observed", check=_check_labels, absent=-1, noun="label set", tag="labels"),
    StepInput(option="weighted_objective", bit=L.OBJ_WEIGHTS, region="obj_weights", replay="obj_weights", dtype=torch.float32,
              stride=lambda B, D: 4, shape=lambda B, D: (4,),
              held="_objw_dev", arg=None, check=None, absent=None, noun="weight row", tag="weights"),
    StepInput(option="temperature_on_device", bit=L.Y_TEMP_DEV, region="y_temperature", replay="y_temperature",
              dtype=torch.float32, stride=lambda B, D: 1, shape=lambda B, D: (),
              held="_tau_dev", arg=None, check=None, absent=None, noun="temperature", tag="temp"),
    StepInput(option="pixel_mask", bit=L.OBJ_PIXEL_MASK, region="pixel_mask", replay="pixel_mask", dtype=torch.uint8,
              stride=lambda B, D: (B * D + 255) // 256 * 256, shape=lambda B, D: (B, D),
              held=None, arg="mask", check=_check_mask, absent=1, noun="mask", tag="mask"),
)
# The part of the library's kIwMasked (csrc/gmvae_hip.hip) that names per-step inputs: gmvae_iw_bound* and gmvae_posterior_*
# clear these bits on entry, so their workspaces hold no such region and _chunked_eval clears them before it binds slot 0.
_EVAL_MASKED = L.OBJ_LABELS | L.OBJ_WEIGHTS | L.Y_TEMP_DEV


class Engine:
    def __init__(self, model: str, data_size: int, latent_size: int, mixture_components: int,
                 hidden: Sequence[int], n_samples: int = 1, sigma_min: float = 0.0, raw_sigma_bias: float = 0.5,
                 temperature: float = 1.0, gen_bias_init=0.0, random_seed: Optional[int] = None, hidden_act: str = "relu",
                 y_inference: str = "gumbel", grad_estimator: str = "standard", semi_supervised: bool = False,
                 sup_weight: float = 1.0, weighted_objective: bool = False, kl_weight: float = 1.0, y_weight: float = 1.0,
                 y_free_nats: float = 0.0, temperature_on_device: bool = False, y_estimator: str = "relaxed",
                 pixel_mask: bool = False, clip_norm: Optional[float] = None, likelihood: str = "bernoulli",
                 likelihood_sigma: float = 1.0, real_valued: Optional[bool] = None, likelihood_scale: str = "fixed"):
        """gen_bias_init: a scalar or a vector of data_size values (scripts/base.py:102-103: "a scalar or vector Tensor
        that is added to the output of the fully connected network", e.g. the logit of the training-set mean).
        y_inference (GMVAE): "gumbel" -- one Gumbel-softmax draw of y per sample (scripts/gmvae.py:238-240, the default) -- or
        "marginal": y summed out exactly over its K values (include/gmvae_hip.h GMVAE_OBJ_MARGINAL_Y).  Marginal steps have
        B*K rows: eps is [B*K, L], u is not used, forward() returns rows / z / y of B*K rows; n_samples must be 1.
        "marginal_iw": y summed out and z importance-weighted over n_samples = S samples per component (GMVAE_OBJ_MARGINAL_Y_IW;
        at S = 1 the "marginal" objective).  Its steps have B*S*K rows, row (b*S + s)*K + k: eps is [B*S*K, L], u is not used,
        forward(n_samples=S') returns rows / z / y of B*S'*K rows.
        grad_estimator: "standard" -- the reparameterised gradient -- or "dreg": the doubly reparameterised gradient for the
        inference network (include/gmvae_hip.h GMVAE_GRAD_DREG): the same bound and generative gradients, an encoder gradient
        whose signal-to-noise ratio grows with n_samples.  Every step takes the general schedule.  Not for the GMVAE with
        y_inference="gumbel".  Parameters and checkpoints are the same under both.
        semi_supervised (GMVAE with y_inference "marginal" or "marginal_iw"; include/gmvae_hip.h GMVAE_OBJ_LABELS): step / loss /
        forward / train_step / dp_step take y_observed, an int tensor [B] of observed components (-1 or any value outside
        [0, K): unlabelled).  A labelled example's loss is its own component's term plus sup_weight * (-ln q(y|x)); an
        unlabelled one's is the marginal objective's.  Parameters and checkpoints are the same with and without it.
        weighted_objective (n_samples = 1; include/gmvae_hip.h GMVAE_OBJ_WEIGHTS): the KL terms carry weights every step reads
        from device memory -- loss = nll + kl_weight * kl_z + y_weight * max(nent, y_free_nats - ln K) (the y term: GMVAE only;
        y_free_nats nats of free bits on KL(q(y|x) || uniform), 0 = off).  set_objective_weights changes them between steps
        without a host sync; a captured train graph reads one row of replay.obj_weights per step (a KL warm-up).  Every step
        takes the general schedule.  Parameters and checkpoints are the same with and without it.
        temperature_on_device (GMVAE, y_inference "gumbel"; include/gmvae_hip.h GMVAE_Y_TEMP_DEV): every step reads the
        Gumbel-softmax temperature from device memory.  set_temperature changes it between steps without a host sync; a
        captured train graph reads one value of replay.y_temperature per step (annealing).  General schedule.
        y_estimator (same domain; GMVAE_Y_STRAIGHT_THROUGH): "relaxed" -- y = softmax((logits + g) / T), the default -- or
        "straight_through": the step consumes the one-hot argmax of logits + g and differentiates through the relaxed
        sample, so that training feeds prior_gmm and encoder_gmm the one-hot y that generation and the enumerating
        evaluators (iw_bound_enum_y, posterior_y) feed them.  General schedule.  Parameters and checkpoints are the same.
        pixel_mask (all three models, the GMVAE with y_inference "gumbel"; include/gmvae_hip.h GMVAE_OBJ_PIXEL_MASK): step /
        loss / forward / train_step / dp_step / iw_bound take mask=, a uint8 / bool tensor [B, D] (non-zero: observed; None:
        all observed).  The networks that read x see mask * x, the likelihood and every gradient count the observed pixels
        alone, and tail [5..7] report the held-out pixels' -log-likelihood and the missing / observed counts.  General
        schedule.  Parameters and checkpoints are the same with and without it.
        clip_norm (every model and objective; include/gmvae_hip.h GMVAE_OPT_CLIP_NORM): None -- off, nothing changes -- or a
        threshold C > 0: every optimizer step clips the batch-mean gradient by its global norm (tf.clip_by_global_norm in front
        of apply_gradients; behind the all-reduce under data parallelism) and skips the update when the gradient or the loss is
        not finite; float("inf") only reports.  grad_clip [4] = (norm before clipping, divisor, clipped 0 / 1, guard: the loss
        sum or NaN where the step was skipped) of the last eager step; a captured graph hands out replay.grad_clip [n_steps, 4].
        set_clip_norm changes C between steps and between replays without a host sync or a recapture.  General schedule.
        likelihood (all three models, the GMVAE with y_inference "gumbel"; include/gmvae_hip.h GMVAE_LIK_*): "bernoulli" -- x in
        {0, 1}, the default, nothing changes -- or, on GREY LEVELS t = x / 255, "grey_bernoulli" (Bernoulli cross-entropy on soft
        targets: no normalised density), "continuous_bernoulli" (Loaiza-Ganem & Cunningham 2019) or "gaussian" (mean = the
        decoder's output, fixed scale likelihood_sigma; set_likelihood_sigma changes it between steps and replays, a device-side
        write).  x is then taken as uint8 grey levels as given; a float tensor must lie in [0, 1] and is rounded to the nearest
        k / 255.  Every network that reads x reads t; tail[5] / tail[6] is the per-pixel squared reconstruction error.  General
        schedule; combines with clip_norm alone.  Parameters and checkpoints have the same layout under every likelihood.
        real_valued (likelihood "gaussian"; include/gmvae_hip.h GMVAE_X_F32): x is a float feature matrix [B, D] -- embeddings,
        sensor vectors, tabular data -- taken as given (float32, any finite values; no uint8): the networks and the likelihood
        read x itself.  likelihood_scale (likelihood "gaussian"; GMVAE_LIK_SCALE_LEARNED): "fixed" -- one sigma, the default --
        or "learned": a scale per dimension, sigma_d = exp(rho_d), rho = the parameter "decoder/log_sigma" [1, D] initialised to
        ln(likelihood_sigma) and trained like every other parameter (it is the layout's last entry; a checkpoint carries it,
        and restoring one without it into such an engine, or the reverse, raises).  set_likelihood_sigma then raises.
        likelihood "poisson" / "negative_binomial" (GMVAE_LIK_POISSON / GMVAE_LIK_NEG_BINOMIAL): x is a float matrix [B, D] of
        counts (finite, >= 0; real_valued is implied, an explicit False raises), the decoder's output is the LOG-mean, every
        network that reads x reads log1p(x), and tail[5] / tail[6] is the squared error of log1p(mean) against log1p(x).  The
        negative binomial's inverse dispersion r_d = exp(rho_d) is the parameter "decoder/log_dispersion" [1, D], initialised to
        0 (r = 1) and trained like every other parameter (the layout's last entry, carried by checkpoints)."""
        clip_norm = check_clip_norm(clip_norm)
        check_real_valued(likelihood, real_valued, likelihood_scale)
        if likelihood in L.COUNT_LIKELIHOODS:
            check_count_likelihood(model, y_inference, grad_estimator, semi_supervised, weighted_objective, temperature_on_device,
                                   y_estimator, pixel_mask, likelihood)
            likelihood_sigma = 1.0
        else:
            likelihood_sigma = check_likelihood(model, y_inference, grad_estimator, semi_supervised, weighted_objective,
                                                temperature_on_device, y_estimator, pixel_mask, likelihood, likelihood_sigma)
        check_pixel_mask(model, y_inference, grad_estimator, semi_supervised, weighted_objective, temperature_on_device,
                         y_estimator, pixel_mask)
        check_y_head(model, y_inference, temperature, temperature_on_device, y_estimator)
        check_semi_supervised(model, y_inference, semi_supervised, sup_weight)
        check_weighted_objective(model, y_inference, n_samples, grad_estimator, semi_supervised, weighted_objective,
                                 kl_weight, y_weight, y_free_nats)
        if y_inference not in L.Y_INFERENCE:
            raise ValueError(f"y_inference must be one of {L.Y_INFERENCE}, got {y_inference!r}")
        if y_inference == "marginal" and (L.MODEL_IDS.get(model) != L.MODEL_GMVAE or int(n_samples) != 1):
            raise ValueError("y_inference='marginal' needs the GMVAE model and n_samples=1 (y is enumerated over the K "
                             "components instead of sampled)")
        if y_inference == "marginal_iw" and L.MODEL_IDS.get(model) != L.MODEL_GMVAE:
            raise ValueError("y_inference='marginal_iw' sums y out over the GMVAE's mixture components: it needs the GMVAE model")
        if grad_estimator not in L.GRAD_ESTIMATORS:
            raise ValueError(f"grad_estimator must be one of {L.GRAD_ESTIMATORS}, got {grad_estimator!r}")
        if grad_estimator == "dreg" and L.MODEL_IDS.get(model) == L.MODEL_GMVAE and y_inference == "gumbel":
            raise ValueError("grad_estimator='dreg' is not available for the GMVAE with y_inference='gumbel' (its relaxed y is "
                             "reparameterised too): use y_inference='marginal' or 'marginal_iw'")
        self.device = L.require_gpu()
        # data parallel: this process's shard index.  Row b of a local batch of B rows is global row rank*B + b for the
        # Philox counters (GmvaeDims.row0), so G ranks draw the noise of ONE step on the global batch of G*B rows.
        import torch.distributed as dist
        self.rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        self.model_name = model
        self.model = L.MODEL_IDS[model]
        self.D, self.Lz, self.K, self.S = int(data_size), int(latent_size), int(mixture_components), int(n_samples)
        self.hidden = [int(h) for h in hidden]
        self.gen_bias_vec = None
        if not isinstance(gen_bias_init, (int, float)):
            gb = torch.as_tensor(gen_bias_init, dtype=torch.float32).reshape(-1)
            if gb.numel() == 1:
                gen_bias_init = float(gb.item())
            elif gb.numel() == self.D:
                self.gen_bias_vec = gb.to(self.device).contiguous()
                gen_bias_init = 0.0
            else:
                raise ValueError(f"gen_bias_init must be a scalar or a vector of data_size = {self.D} values, got {gb.numel()}")
        if hidden_act not in L.ACTS:
            raise ValueError(f"hidden_act must be one of {sorted(L.ACTS)} (hidden_activation_fn, scripts/base.py:19), got {hidden_act!r}")
        self.hidden_act = hidden_act
        self.y_inference = y_inference
        self.marginal = y_inference in ("marginal", "marginal_iw")      # y enumerated over the K components
        self.marginal_iw = y_inference == "marginal_iw"
        self.grad_estimator = grad_estimator
        self.semi_supervised = bool(semi_supervised)
        self.sup_weight = float(sup_weight)
        self.weighted_objective = bool(weighted_objective)
        self.obj_weights = (float(kl_weight), float(y_weight), float(y_free_nats))
        self.temperature_on_device = bool(temperature_on_device)
        self.y_estimator = y_estimator
        self.pixel_mask = bool(pixel_mask)
        self.clip_norm = clip_norm
        self.likelihood = likelihood
        self.likelihood_sigma = likelihood_sigma
        self.count_likelihood = likelihood in L.COUNT_LIKELIHOODS
        self.real_valued = bool(real_valued) or self.count_likelihood
        self.likelihood_scale = likelihood_scale
        self.rows_per_x = self._rows_per_x(self.S)      # sample-dependent rows per batch row
        self.hp = dict(sigma_min=sigma_min, raw_sigma_bias=raw_sigma_bias, temperature=float(temperature),
                       gen_bias_init=float(gen_bias_init), hidden_act=hidden_act)
        self.safe_schedule = False              # use_safe_schedule(): the schedules without mutual waits (per engine)
        d0 = self.dims(1)
        self.P, self.P_real = L.param_count(d0, self.model)
        self.layout = L.param_layout(d0, self.model)
        self.random_seed = random_seed
        self.noise_seed = int(random_seed) if random_seed is not None else int(torch.seed() & 0x7FFFFFFFFFFFFFFF)
        self.params = torch.zeros(self.P, dtype=torch.float32, device=self.device, requires_grad=True)
        self.grads = torch.zeros(self.P + L.TAIL, dtype=torch.float32, device=self.device)
        self.m = torch.zeros(self.P, dtype=torch.float32, device=self.device)
        self.v = torch.zeros(self.P, dtype=torch.float32, device=self.device)
        self.step_dev = torch.zeros(2, dtype=torch.int64, device=self.device)   # global_step (device resident) + scratch copy
        self.global_step = 0
        self._ws: Dict[tuple, torch.Tensor] = {}
        self._graphs: Dict[tuple, tuple] = {}
        self._graph_gen = 0                     # bumped by drop_graphs: replay closures of dropped graphs raise
        self._param_epoch = 0                   # bumped by every Engine call that enqueues a writer of the parameter buffer
        self._eval_imgs: Dict[tuple, tuple] = {}   # (B, S) -> the state of the parameters a forward-only pass left images for
        self._chunked_ws: Dict[tuple, torch.Tensor] = {}  # (kind, B, chunk) -> the workspace of a chunked evaluator (_CHUNKED)
        # weighted objective: the current (kl_weight, y_weight, y_free_nats, 0) on the device; every eager entry copies it into
        # slot 0 of its workspace's weight rows (device to device: a captured graph may have left its own row there)
        self._objw_dev = None
        if self.weighted_objective:
            self._objw_dev = torch.zeros(4, dtype=torch.float32, device=self.device)
            self.set_objective_weights(*self.obj_weights)
        # temperature on the device: the current T; every eager entry copies it into slot 0 of its workspace's temperatures
        self._tau_dev = None
        if self.temperature_on_device:
            self._tau_dev = torch.full((1,), float(temperature), dtype=torch.float32, device=self.device)
        # gradient clipping: the current threshold on the device (every workspace's "clip_norm" cell is a copy of it), the record
        # of the last eager step and the partials' scratch of gmvae_grad_clip
        self._clip_dev = self.grad_clip = self._clip_scratch = None
        self._clip_cells: Dict[tuple, torch.Tensor] = {}
        if self.clip_norm is not None:
            self._clip_dev = torch.full((1,), self.clip_norm, dtype=torch.float32, device=self.device)
            self.grad_clip = torch.zeros(4, dtype=torch.float32, device=self.device)
            self._clip_scratch = torch.zeros(L.grad_clip_scratch_bytes(self.P) // 8, dtype=torch.float64, device=self.device)
        # the Gaussian likelihood's sigma on the device: every workspace's "lik_sigma" cell is a copy of it
        self._sigma_dev = None
        self._sigma_cells: Dict[tuple, torch.Tensor] = {}
        if self.likelihood == "gaussian" and self.likelihood_scale == "fixed":
            self._sigma_dev = torch.full((1,), self.likelihood_sigma, dtype=torch.float32, device=self.device)
        self.init_parameters(random_seed)

    @property
    def temperature(self) -> float:
        """The Gumbel-softmax temperature the next eager calls use (set_temperature)."""
        return self.hp["temperature"]

    # ------------------------------------------------------------ parameters
    def dims(self, B: int, S: Optional[int] = None, row0: Optional[int] = None, extra_flags: int = 0):
        """GmvaeDims for a local batch of B rows; row0 = global index of its first row (default rank * B)."""
        S = self.S if S is None else S
        # (the weighted objective is the one-sample bound's: a forward at another number of samples reports the plain bound)
        wobj = L.OBJ_WEIGHTS if self.weighted_objective and int(S) == 1 else 0
        yh = (L.Y_TEMP_DEV if self.temperature_on_device else 0) | (L.Y_STRAIGHT_THROUGH if self.y_estimator == "straight_through" else 0)
        pmask = (L.OBJ_PIXEL_MASK if self.pixel_mask else 0) | (L.OPT_CLIP_NORM if self.clip_norm is not None else 0)
        pmask |= L.COUNT_LIKELIHOODS[self.likelihood] if self.count_likelihood else L.LIKELIHOODS[self.likelihood]
        pmask |= (L.X_F32 if self.real_valued else 0) | (L.LIK_SCALE_LEARNED if self.likelihood_scale == "learned" else 0)
        return L.make_dims(B, self.D, self.Lz, self.K, self.hidden, S=S,
                           row0=self.rank * B if row0 is None else int(row0), gen_bias_vec=self.gen_bias_vec,
                           sched_flags=(L.SCHED_SAFE if self.safe_schedule else 0) | self._obj_flags() | wobj | yh | pmask | extra_flags, **self.hp)

    def _obj_flags(self):
        obj = L.OBJ_MARGINAL_Y_IW if self.marginal_iw else L.OBJ_MARGINAL_Y if self.marginal else 0
        return obj | (L.GRAD_DREG if self.grad_estimator == "dreg" else 0) | (L.OBJ_LABELS if self.semi_supervised else 0)

    def _rows_per_x(self, S):
        """Sample-dependent rows per batch row at S samples: S K with y summed out over the K components, else S."""
        return S * self.K if self.marginal_iw else self.K if self.marginal else S

    def _params_state(self):
        """What identifies the parameter VALUES: torch's version counter of the buffer (in-place writes through torch) and the
        Engine's own count of the HIP writers it enqueued (the optimizer kernels, train graphs: invisible to torch)."""
        return (self._param_epoch, self.params._version, self.params.data_ptr())

    def sync_replicas(self, src: int = 0):
        """Data parallel: every rank takes rank `src`'s parameters, Adam moments, step counter and noise seed (the
        reference's default random_seed=None seeds each process from entropy, scripts/run_gmvae.py:30).  Afterwards
        replicas stay bit-identical: every rank applies the same all-reduced gradient."""
        import torch.distributed as dist
        from . import parallel
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return
        self._param_epoch += 1
        self.noise_seed, self.global_step = parallel.broadcast_state((self.params, self.m, self.v),
                                                                     (self.noise_seed, self.global_step), src)
        self.step_dev.fill_(self.global_step)
        self.drop_graphs()                       # captured graphs baked the old seed

    def init_parameters(self, seed: Optional[int] = None):
        """Xavier-uniform weights, zero biases (scripts/base.py:12); Glorot-uniform
        prior variables (tf.get_variable default, scripts/vae.py:233-238)."""
        gen = torch.Generator(device="cpu")
        if seed is not None:
            gen.manual_seed(int(seed))
        else:
            gen.seed()
        flat = torch.zeros(self.P, dtype=torch.float32)
        for name, (rows, cols), off in self.layout:
            if name.endswith("/b"):
                continue
            if name == L.LOG_SIGMA:             # rho = ln sigma for every dimension
                flat[off:off + rows * cols] = math.log(self.likelihood_sigma)
                continue
            if name == L.LOG_DISPERSION:        # rho = 0: inverse dispersion r = 1 for every dimension
                flat[off:off + rows * cols] = 0.0
                continue
            fan_in, fan_out = (cols, cols) if name == "mixture_logits" else (rows, cols)
            lim = math.sqrt(6.0 / (fan_in + fan_out))
            flat[off:off + rows * cols] = (torch.rand(rows * cols, generator=gen) * 2 - 1) * lim
        self._param_epoch += 1
        with torch.no_grad():
            self.params.copy_(flat.to(self.device))
            self.m.zero_()
            self.v.zero_()
            self.step_dev.zero_()
        self.global_step = 0

    def views(self) -> Dict[str, torch.Tensor]:
        """Named views of the flat buffer, keyed by the reference's TF variable names."""
        out = {}
        for name, (rows, cols), off in self.layout:
            v = self.params.detach()[off:off + rows * cols]
            if name.endswith("/b") or name in ("mixture_logits", L.LOG_SIGMA, L.LOG_DISPERSION):
                out[name] = v
            else:
                out[name] = v.view(rows, cols)
        return out

    def _slot_views(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        out = {}
        for name, (rows, cols), off in self.layout:
            v = flat[off:off + rows * cols]
            out[name] = v if (name.endswith("/b") or name in ("mixture_logits", L.LOG_SIGMA, L.LOG_DISPERSION)) else v.view(rows, cols)
        return out

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """Keys = the reference's TF checkpoint variable names: every model variable, its two Adam
        slots `<var>/Adam` (m) and `<var>/Adam_1` (v) as tf.train.AdamOptimizer names them (scripts/runners.py:181),
        the optimizer's `beta1_power` / `beta2_power` accumulators (= beta^(global_step+1) in TF 1.13: the value the
        NEXT apply uses) and `global_step`.  `noise_seed` (not a TF variable) keeps the Philox stream across a restart."""
        sd = {k: v.clone() for k, v in self.views().items()}
        for k, v in self._slot_views(self.m).items():
            sd[k + "/Adam"] = v.clone()
        for k, v in self._slot_views(self.v).items():
            sd[k + "/Adam_1"] = v.clone()
        sd["global_step"] = torch.tensor(self.global_step)
        sd["beta1_power"] = torch.tensor(0.9 ** (self.global_step + 1), dtype=torch.float32)
        sd["beta2_power"] = torch.tensor(0.999 ** (self.global_step + 1), dtype=torch.float32)
        sd["noise_seed"] = torch.tensor(self.noise_seed, dtype=torch.int64)
        return sd

    def load_state_dict(self, sd: Dict[str, torch.Tensor]):
        if (L.LOG_DISPERSION in sd) != (self.likelihood == "negative_binomial"):
            raise ValueError(f"this checkpoint {'carries' if L.LOG_DISPERSION in sd else 'has no'} {L.LOG_DISPERSION!r}: it cannot "
                             f"be restored into an engine with likelihood={self.likelihood!r}")
        if (L.LOG_SIGMA in sd) != (self.likelihood_scale == "learned"):
            raise ValueError(f"this checkpoint {'carries' if L.LOG_SIGMA in sd else 'has no'} {L.LOG_SIGMA!r}: it cannot be restored "
                             f"into an engine with likelihood_scale={self.likelihood_scale!r}")
        self._param_epoch += 1
        views = self.views()
        with torch.no_grad():
            for k, v in views.items():
                v.copy_(sd[k].to(self.device).reshape(v.shape))
            if "adam/m" in sd:                    # round-1 checkpoints: two flat blobs
                self.m.copy_(sd["adam/m"].to(self.device))
                self.v.copy_(sd["adam/v"].to(self.device))
            else:
                for slot, flat in (("/Adam", self.m), ("/Adam_1", self.v)):
                    for k, v in self._slot_views(flat).items():
                        if k + slot in sd:
                            v.copy_(sd[k + slot].to(self.device).reshape(v.shape))
            self.global_step = int(sd.get("global_step", 0))
            if "noise_seed" in sd:
                self.noise_seed = int(sd["noise_seed"])
            self.step_dev.fill_(self.global_step)
        self.drop_graphs()                        # graphs bake the noise seed

    # ------------------------------------------------------------- workspace
    def _workspace(self, B: int, S: Optional[int] = None, row0: Optional[int] = None):
        key = (B, self.S if S is None else S)
        d = self.dims(B, S, row0)
        # the size is re-queried on every call: the library sizes the layout from the dims alone, but its few remaining
        # test / tuning switches (GMVAE_NSPLIT_SMALL) enter the slab count -- a cached allocation must never be too small
        n = L.workspace_bytes(d, self.model) // 4 + 64
        if key in self._ws and self._ws[key].numel() < n:
            self.drop_graphs(clear_handoff_errors=False)      # captured graphs hold pointers into the old allocation
            del self._ws[key]
            self._clip_cells.pop(key, None)
            self._sigma_cells.pop(key, None)
        if key not in self._ws:
            self._ws[key] = torch.zeros(n, dtype=torch.float32, device=self.device)
            # the library only reads the per-step inputs' regions (and the classification weight), and zeros would mean
            # "component 0 observed, weights 0, T = 0, nothing observed"
            for inp in STEP_INPUTS:
                if d.sched_flags & inp.bit:
                    self._fill(inp, self._slots(inp, d, self._ws[key]))
            if self.semi_supervised:
                off = L.workspace_offset(d, self.model, "sup_weight") // 4
                self._ws[key][off:off + 1].fill_(self.sup_weight)
            if d.sched_flags & L.OPT_CLIP_NORM:     # (a zeroed cell means C = 0: every step skipped)
                off = L.workspace_offset(d, self.model, "clip_norm") // 4
                self._clip_cells[key] = self._ws[key][off:off + 1]
                self._clip_cells[key].copy_(self._clip_dev, non_blocking=True)
            self._bind_sigma(key, d, self._ws[key])
        return d, self._ws[key]

    # ------------------------------------------------------- the Gaussian likelihood's sigma (likelihood_sigma)
    def _bind_sigma(self, key, d, ws):
        """The workspace's "lik_sigma" cell <- the engine's sigma (a zeroed cell means sigma = 0: a non-finite step)."""
        if (d.sched_flags & L.LIK_MASK) == L.LIK_GAUSSIAN and not d.sched_flags & L.LIK_SCALE_LEARNED:
            off = L.workspace_offset(d, self.model, "lik_sigma") // 4
            self._sigma_cells[key] = ws[off:off + 1]
            self._sigma_cells[key].copy_(self._sigma_dev, non_blocking=True)

    def set_likelihood_sigma(self, sigma: float):
        """The Gaussian likelihood's scale the next steps read, eager or replayed: device-side writes, no host sync, no recapture."""
        if self.likelihood != "gaussian":
            raise ValueError("set_likelihood_sigma needs an engine created with likelihood='gaussian'")
        if self.likelihood_scale == "learned":
            raise ValueError("set_likelihood_sigma: with likelihood_scale='learned' the scale is the parameter "
                             f"{L.LOG_SIGMA!r}, not a setting")
        self.likelihood_sigma = check_likelihood(self.model_name, "gumbel", "standard", False, False, False, "relaxed", False,
                                                 "gaussian", sigma)
        self._sigma_dev.fill_(self.likelihood_sigma)
        for cell in self._sigma_cells.values():
            cell.copy_(self._sigma_dev, non_blocking=True)

    # ------------------------------------------------------- gradient clipping (clip_norm)
    def _push_clip_norm(self):
        """Every workspace's "clip_norm" cell <- the engine's threshold (device to device: a caller may have written a cell)."""
        for cell in self._clip_cells.values():
            cell.copy_(self._clip_dev, non_blocking=True)

    def _clip_records(self, d, ws) -> torch.Tensor:
        """View [LABEL_SLOTS, 4] of the workspace's "grad_clip" region: step i of a train graph writes row i."""
        off = L.workspace_offset(d, self.model, "grad_clip") // 4
        return ws[off:off + 4 * L.LABEL_SLOTS].view(L.LABEL_SLOTS, 4)

    def set_clip_norm(self, clip_norm: float):
        """The threshold the next optimizer steps read, eager or replayed: device-side writes, no host sync, no recapture."""
        if self.clip_norm is None:
            raise ValueError("set_clip_norm needs an engine created with clip_norm=")
        c = check_clip_norm(clip_norm)
        if c is None:
            raise ValueError("set_clip_norm takes a number > 0: clipping cannot be switched off on an engine created with it "
                             "(float('inf') never clips)")
        self.clip_norm = c
        self._clip_dev.fill_(c)
        self._push_clip_norm()

    # ------------------------------------------------------- per-step inputs (STEP_INPUTS)
    @property
    def step_inputs(self) -> Tuple[str, ...]:
        """The options of this engine's per-step inputs, in the order of STEP_INPUTS."""
        return tuple(inp.option for inp in STEP_INPUTS if getattr(self, inp.option))

    def _slots(self, inp: StepInput, d, ws) -> torch.Tensor:
        """View [LABEL_SLOTS, *inp.shape] of the input's region of the workspace (slot i starts i * inp.stride elements in)."""
        shape, stride = inp.shape(d.B, d.D), inp.stride(d.B, d.D)
        off = L.workspace_offset(d, self.model, inp.region) // inp.dtype.itemsize
        slots = ws.view(inp.dtype)[off:off + L.LABEL_SLOTS * stride].view(L.LABEL_SLOTS, stride)
        return slots[:, :math.prod(shape)].view(L.LABEL_SLOTS, *shape)

    def _fill(self, inp: StepInput, slots: torch.Tensor, value=None):
        """Every slot of the view <- value (a device-side write, no host sync); None: the engine-held tensor, or inp.absent."""
        if value is None:
            value = getattr(self, inp.held) if inp.held else inp.absent
        if isinstance(value, torch.Tensor):
            slots.copy_(value.reshape(slots.shape[1:]).expand_as(slots), non_blocking=True)
        else:
            slots.fill_(value)

    def _bind_step_inputs(self, d, ws, y_observed: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None):
        """Slot 0 of every per-step input these dims carry <- what this eager call reads: the engine's current weights and
        temperature, the call's y_observed (None: all unlabelled) and mask (None: all observed)."""
        args = dict(y_observed=y_observed, mask=mask)
        for inp in STEP_INPUTS:
            value = args[inp.arg] if inp.arg else None
            if not getattr(self, inp.option):
                if value is not None:
                    raise ValueError(f"{inp.arg} needs an engine created with {inp.option}=True")
            elif d.sched_flags & inp.bit:       # (not the weights of a forward at S != 1: dims() leaves their bit out)
                if value is not None:
                    value = inp.check(self, value, d.B)
                self._fill(inp, self._slots(inp, d, ws)[:1], value)

    def set_objective_weights(self, kl_weight: float, y_weight: float, y_free_nats: float):
        """The weights the next eager steps (step / loss / forward / train_step / dp_step) read: device-side writes, no host
        sync.  A captured train graph reads its own rows (replay.obj_weights), pre-filled at capture with these."""
        if not self.weighted_objective:
            raise ValueError("set_objective_weights needs an engine created with weighted_objective=True")
        check_weighted_objective(self.model_name, self.y_inference, self.S, self.grad_estimator, self.semi_supervised, True,
                                 kl_weight, y_weight, y_free_nats)
        self.obj_weights = (float(kl_weight), float(y_weight), float(y_free_nats))
        for i, v in enumerate(self.obj_weights):
            self._objw_dev[i:i + 1].fill_(v)

    def set_temperature(self, t: float):
        """The Gumbel-softmax temperature of the next eager calls (step / loss / forward / train_step / dp_step, the
        evaluators, ConditionalCategorical.sample).  With temperature_on_device: a device-side write, no host sync, and a
        captured train graph keeps reading its own values (replay.y_temperature).  Without: the value travels in the dims,
        and the captured graphs, which baked the old one, are dropped."""
        check_y_head(self.model_name, self.y_inference, t, self.temperature_on_device, self.y_estimator)
        changed = float(t) != self.hp["temperature"]
        self.hp["temperature"] = float(t)
        if self.temperature_on_device:
            self._tau_dev.fill_(float(t))
        elif changed:
            self.drop_graphs(clear_handoff_errors=False)

    @staticmethod
    def _as_u8(x: torch.Tensor) -> torch.Tensor:
        if x.dtype == torch.bool:
            x = x.view(torch.uint8) if x.is_contiguous() else x.to(torch.uint8)
        elif x.dtype != torch.uint8:
            x = x.to(torch.uint8)
        return x.contiguous()

    def _prep_x(self, x: torch.Tensor) -> torch.Tensor:
        x = x.to(self.device)
        if self.real_valued:
            # a float feature matrix, as given: float32, contiguous, [B, D], its base 16-byte aligned (GMVAE_X_F32)
            if not x.dtype.is_floating_point:
                raise ValueError(f"real_valued=True takes a float tensor [B, {self.D}], got {x.dtype}")
            x = x.to(torch.float32).reshape(x.shape[0], -1).contiguous()
            if x.shape[1] != self.D:
                raise ValueError(f"expected [B,{self.D}] inputs, got {tuple(x.shape)}")
            if x.numel() and not bool(torch.isfinite(x).all()):
                raise ValueError("real_valued=True takes finite values: x holds NaN or inf")
            if self.count_likelihood and x.numel() and bool((x < 0).any()):
                raise ValueError(f"likelihood={self.likelihood!r} takes counts: x holds negative values")
            return x.clone() if x.data_ptr() % 16 else x
        if self.likelihood != "bernoulli" and x.dtype.is_floating_point:
            # grey levels: a float image in [0, 1] -> the nearest k / 255 (uint8 tensors are taken as grey levels as given)
            if x.numel() and not bool(((x >= 0) & (x <= 1)).all()):
                raise ValueError(f"likelihood={self.likelihood!r} takes uint8 grey levels or floats in [0, 1]")
            x = torch.round(x.to(torch.float32) * 255.0).to(torch.uint8)
        x = self._as_u8(x)
        x = x.reshape(x.shape[0], -1)           # utils.flatten_tensor (scripts/utils.py:140-141)
        if x.shape[1] != self.D:
            raise ValueError(f"expected [B,{self.D}] inputs, got {tuple(x.shape)}")
        return x

    def _prep_u(self, u, rows):
        if self.marginal:
            if u is not None:
                raise ValueError(f"y_inference={self.y_inference!r} enumerates y: it takes no Gumbel noise u")
            return None
        return self._prep_noise(u, rows, self.K) if self.model == L.MODEL_GMVAE else None

    def _prep_noise(self, t, rows, cols):
        if t is None:
            return None
        t = t.to(self.device, torch.float32).contiguous()
        if t.numel() != rows * cols:
            raise ValueError(f"noise must have {rows}x{cols} elements")
        return t

    # ------------------------------------------------------------------ ops
    def step(self, x, eps=None, u=None, use_step_dev: bool = False, row0: Optional[int] = None,
             y_observed: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Fused forward + backward.  Returns the [P + TAIL] buffer of gradient
        SUMS and loss sums (see include/gmvae_hip.h).  eps/u None -> Philox, keyed by
        (noise_seed, global_step, global row = row0 + b; row0 defaults to rank * B)."""
        x = self._prep_x(x)
        B = x.shape[0]
        d, ws = self._workspace(B, row0=row0)
        self._bind_step_inputs(d, ws, y_observed, mask)
        eps = self._prep_noise(eps, B * self.rows_per_x, self.Lz)
        u = self._prep_u(u, B * self.S)
        rc = L.lib.gmvae_step(C.byref(d), self.model, L.ptr(x), L.ptr(eps), L.ptr(u), L.ptr(self.params),
                              L.ptr(self.grads), L.ptr(ws), self.noise_seed, self.global_step,
                              L.ptr(self.step_dev) if use_step_dev else None, L.current_stream())
        L.check(rc, "gmvae_step")
        self._keep = (x, eps, u)
        return self.grads

    def loss(self, x, eps=None, u=None, y_observed: Optional[torch.Tensor] = None,
             mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Differentiable scalar: loss.backward() fills params.grad."""
        return _ElboFn.apply(self.params, self, x, eps, u, y_observed, mask)

    def forward(self, x, eps=None, u=None, n_samples: Optional[int] = None, y_observed: Optional[torch.Tensor] = None,
                mask: Optional[torch.Tensor] = None):
        """Forward only.  dict(tail[8], rows[R,4]=(logpx,logq,logp,logw), z, y, logits)."""
        x = self._prep_x(x)
        B = x.shape[0]
        S = self.S if n_samples is None else int(n_samples)
        if self.marginal and not self.marginal_iw and S != 1:
            raise ValueError("y_inference='marginal' enumerates y over the K components: n_samples must be 1")
        d, ws = self._workspace(B, S)
        self._bind_step_inputs(d, ws, y_observed, mask)
        # an evaluation walks a split batch by batch on fixed parameters (scripts/runners.py:320-333): the operand images the
        # previous pass left in this workspace are reused while nothing has written the parameters since
        state = self._params_state() + (ws.data_ptr(),)
        if self._eval_imgs.get((B, S)) == state:
            d = self.dims(B, S, extra_flags=L.SCHED_EVAL_IMAGES_VALID)
        R = B * self._rows_per_x(S)
        eps = self._prep_noise(eps, R, self.Lz)
        gm = self.model == L.MODEL_GMVAE
        u = self._prep_u(u, R)
        f32 = dict(dtype=torch.float32, device=self.device)
        o = dict(tail=torch.empty(L.TAIL, **f32), rows=torch.empty(R, 4, **f32), z=torch.empty(R, self.Lz, **f32),
                 y=torch.empty(R, self.K, **f32) if gm else None,
                 logits=torch.empty(B, self.K, **f32) if gm else None)
        rc = L.lib.gmvae_forward(C.byref(d), self.model, L.ptr(x), L.ptr(eps), L.ptr(u), L.ptr(self.params),
                                 L.ptr(o["tail"]), L.ptr(o["rows"]), L.ptr(o["z"]), L.ptr(o["y"]), L.ptr(o["logits"]),
                                 L.ptr(ws), self.noise_seed, self.global_step, L.current_stream())
        L.check(rc, "gmvae_forward")
        self._eval_imgs[(B, S)] = state
        return o

    IW_CHUNK_ROWS = 51200          # default B * chunk of iw_bound: the rows of bench.py's eval_iwae pass (B = 1024, S = 50)

    def _cached_ws(self, key, n_words: int):
        """(an evaluator's workspace of at least n_words zeroed floats, kept under `key`; whether this call allocated it)."""
        ws = self._chunked_ws.get(key)
        if ws is not None and ws.numel() >= n_words:
            return ws, False
        self._chunked_ws[key] = torch.zeros(n_words, dtype=torch.float32, device=self.device)
        return self._chunked_ws[key], True

    def _require_plain_bernoulli(self, what: str):
        if self.pixel_mask or self.likelihood != "bernoulli":
            raise ValueError(f"{what} scores the Bernoulli likelihood on every pixel: not available with pixel_mask=True or "
                             f"likelihood={self.likelihood!r}")

    # the chunked importance-sampling evaluators, gmvae_<kind> and gmvae_<kind>_workspace_bytes of include/gmvae_hip.h:
    # kind -> (y enumerated: K rows per sample in the default chunk; outputs per component: log_joint [B, K], log_post [B, K]
    # and stats [B, 4] in place of bound [B] and mean_logw [B])
    _CHUNKED = {"iw_bound": (False, False), "iw_bound_enum_y": (True, False), "posterior_y": (True, True),
                "posterior_component": (False, True), "impute": (False, False)}

    def _chunked_eval(self, kind: str, x, n_samples: int, chunk: Optional[int], row0: Optional[int], mask=None,
                      n_draws: int = 0, return_logw: bool = False):
        """One call of a chunked evaluator: (its output tensors in the order of the C signature, tail [8]).  kind "impute"
        (gmvae_impute) takes n_draws and return_logw too; an output it was not asked for is None."""
        enum_y, per_component = self._CHUNKED[kind]
        if self.pixel_mask and kind not in ("iw_bound", "impute"):
            raise ValueError(f"{kind} is not available with pixel_mask=True (it would score the unobserved pixels): use iw_bound")
        if self.likelihood != "bernoulli" and kind != "iw_bound":
            raise ValueError(f"{kind} is not available with likelihood={self.likelihood!r} (it would score Bernoulli): use iw_bound")
        x = self._prep_x(x)
        if x.data_ptr() % 16:
            x = x.clone()
        B, n = x.shape[0], int(n_samples)
        if n < 1:
            raise ValueError(f"n_samples must be >= 1, got {n}")
        chunk = max(1, min(n, self.IW_CHUNK_ROWS // (B * self.K if enum_y else B))) if chunk is None else int(chunk)
        if chunk < 1:
            raise ValueError(f"chunk must be >= 1, got {chunk}")
        d = self.dims(B, chunk, row0)
        d.sched_flags &= ~_EVAL_MASKED      # (as the library's iw_dims does: the same size query, the same run)
        if kind == "impute":
            key, nbytes = (kind, B, chunk, n_draws), L.impute_workspace_bytes(d, self.model, n_draws)
        else:
            key, nbytes = (kind, B, chunk), getattr(L, f"{kind}_workspace_bytes")(d, self.model)
        ws, fresh = self._cached_ws(key, nbytes // 4 + 64)
        if fresh:
            self._bind_sigma(key, d, ws)      # (the forward's workspace opens the evaluator's: the same offsets)
        self._bind_step_inputs(d, ws, mask=mask)      # (the forward's workspace opens the evaluator's: the same offsets)
        f32 = dict(dtype=torch.float32, device=self.device)
        shapes = ((B, self.K), (B, self.K), (B, 4)) if per_component else ((B,), (B,))
        outs = [torch.empty(*shape, **f32) for shape in shapes]
        tail = torch.empty(L.TAIL, **f32)
        if kind == "impute":
            outs = [torch.empty(B, self.D, **f32), torch.empty(B, 4, **f32), torch.empty(B, n, **f32) if return_logw else None,
                    torch.empty(B, n_draws, dtype=torch.int64, device=self.device) if n_draws else None,
                    torch.empty(B, n_draws, self.Lz, **f32) if n_draws else None]
            rc = L.lib.gmvae_impute(C.byref(d), self.model, L.ptr(x), L.ptr(self.params), n, n_draws, *map(L.ptr, outs),
                                    L.ptr(tail), L.ptr(ws), self.noise_seed, self.global_step, L.current_stream())
            L.check(rc, "gmvae_impute")
            self._keep_iw = x
            return outs, tail
        rc = getattr(L.lib, f"gmvae_{kind}")(C.byref(d), self.model, L.ptr(x), L.ptr(self.params), n, *map(L.ptr, outs),
                                             L.ptr(tail), L.ptr(ws), self.noise_seed, self.global_step, L.current_stream())
        L.check(rc, f"gmvae_{kind}")
        self._keep_iw = x
        return outs, tail

    def iw_bound(self, x, n_samples: int, chunk: Optional[int] = None, row0: Optional[int] = None,
                 mask: Optional[torch.Tensor] = None):
        """The importance-weighted bound at any number of samples, streamed in chunks (include/gmvae_hip.h gmvae_iw_bound):
        dict(bound [B] = logsumexp_s log w - log n, mean_logw [B], tail [8] as forward's at S = n).  chunk: samples per pass
        (default: B * chunk near IW_CHUNK_ROWS, at most n_samples); the memory depends on B * chunk, not on n_samples.
        Sample s of row b draws Philox row (row0 + b) * n_samples + s keyed by (noise_seed, global_step), row0 defaulting to
        rank * B: the result does not depend on the chunk, the batch size or the sharding.
        mask (pixel_mask=True): the bound on log p(x_observed)."""
        if self.marginal:
            raise ValueError(f"iw_bound: the importance-weighted bound is not available with y_inference={self.y_inference!r} "
                             "(it is the Gumbel objective's bound)")
        (bound, mean_logw), tail = self._chunked_eval("iw_bound", x, n_samples, chunk, row0, mask)
        return dict(bound=bound, mean_logw=mean_logw, tail=tail)

    def impute_posterior(self, x, n_samples: int, mask: Optional[torch.Tensor] = None, n_draws: int = 0,
                         chunk: Optional[int] = None, row0: Optional[int] = None, return_logw: bool = False):
        """The missing pixels imputed by self-normalised importance sampling on iw_bound's weights (Mattei & Frellsen, MIWAE,
        2019; include/gmvae_hip.h gmvae_impute): dict(mean [B, D] = sum_s w~_s sigmoid(lambda_s) ~ E[x | x_observed] at every
        pixel, imputed = where(mask, x, mean), bound [B] -- iw_bound's --, ess [B], cond_loglik [B] ~ log p(x_missing |
        x_observed) at the x given (0 for a row with nothing missing), max_weight [B], draw_index [B, n_draws] (int64) and
        draw_z [B, n_draws, L] -- sampling-importance-resampling draws of z, None at n_draws = 0 --, logw [B, n_samples] with
        return_logw (else None), tail [8] = the batch sums of (-bound, ess, cond_loglik, missing pixels), B).  mask
        (pixel_mask=True): non-zero = observed; None: every pixel observed, the posterior-mean reconstruction.  chunk, row0 and
        the noise keying as iw_bound: the result does not depend on the chunk, the batch size or the sharding."""
        n, m = check_impute_args(self.model_name, self.y_inference, self.likelihood, self.pixel_mask, n_samples, n_draws,
                                 mask is not None)
        (mean, stats, logw, di, dz), tail = self._chunked_eval("impute", x, n, chunk, row0, mask, n_draws=m,
                                                               return_logw=return_logw)
        xs = self._keep_iw.reshape(mean.shape)
        imputed = mean if mask is None else torch.where(_check_mask(self, mask, mean.shape[0]).reshape(mean.shape),
                                                        xs.to(mean.dtype), mean)
        return dict(mean=mean, imputed=imputed, bound=stats[:, 0], ess=stats[:, 1], cond_loglik=stats[:, 2],
                    max_weight=stats[:, 3], draw_index=di, draw_z=dz, logw=logw, tail=tail)

    def iw_bound_enum_y(self, x, n_samples: int, chunk: Optional[int] = None, row0: Optional[int] = None):
        """The GMVAE's importance-weighted bound with y summed out exactly over its K components, streamed in chunks
        (include/gmvae_hip.h gmvae_iw_bound_enum_y): dict(bound [B] = logsumexp_{s,k} log w'_sk - log n -- log p(x) + ln K for
        a uniform p(y) --, mean_logw [B] = sum_k q_k mean_s log w'_sk - sum_k q_k ln q_k, tail [8]).  Any GMVAE engine,
        y_inference 'gumbel' or 'marginal': the bound depends only on the generative model and q(z|x,y).  chunk: samples per
        component per pass (default: B * K * chunk near IW_CHUNK_ROWS, at most n_samples).  Sample s of component k of row b
        draws Philox row ((row0 + b) * n_samples + s) * K + k keyed by (noise_seed, global_step), row0 defaulting to rank * B:
        the result does not depend on the chunk, the batch size or the sharding."""
        if self.model != L.MODEL_GMVAE:
            raise ValueError("iw_bound_enum_y sums y out over the GMVAE's mixture components: not available for the VAE family")
        (bound, mean_logw), tail = self._chunked_eval("iw_bound_enum_y", x, n_samples, chunk, row0)
        return dict(bound=bound, mean_logw=mean_logw, tail=tail)

    def posterior_y(self, x, n_samples: int, chunk: Optional[int] = None, row0: Optional[int] = None):
        """The GMVAE's own posterior over its component, p(y = k | x) = softmax_k l_k with l_k = logsumexp_s log w'_sk - log n
        an importance-sampling estimate of log p(x | y = k) (include/gmvae_hip.h gmvae_posterior_y): dict(log_joint [B, K] = l,
        log_post [B, K] = ln p(y | x), bound [B] = logsumexp_k l_k -- iw_bound_enum_y's bound --, entropy [B] of the posterior,
        kl_q_post [B] = KL(q(y|x) || p(y|x)), ess [B] = the effective sample size of the n * K weights, tail [8] = the batch
        sums of (-bound, entropy, kl_q_post, ess), B).  Any GMVAE engine, whatever its y_inference.  chunk, row0 and the noise
        keying as iw_bound_enum_y: the result does not depend on the chunk, the batch size or the sharding."""
        if self.model != L.MODEL_GMVAE:
            raise ValueError("posterior_y is the posterior over the GMVAE's mixture components: not available for the VAE family")
        (lj, lp, stats), tail = self._chunked_eval("posterior_y", x, n_samples, chunk, row0)
        return dict(log_joint=lj, log_post=lp, bound=stats[:, 0], entropy=stats[:, 1], kl_q_post=stats[:, 2], ess=stats[:, 3],
                    tail=tail)

    def posterior_component(self, x, n_samples: int, chunk: Optional[int] = None, row0: Optional[int] = None):
        """The VAE_GMP's own posterior over the component of its mixture prior, p(k | x) = softmax_k l_k with l_k =
        logsumexp_s log w_sk - log n an importance-sampling estimate of log p(x, k) (include/gmvae_hip.h
        gmvae_posterior_component; one sample z ~ q(z|x) serves all K components): dict(log_joint [B, K] = l, log_post [B, K] =
        ln p(k | x), bound [B] = logsumexp_k l_k -- iw_bound's bound --, entropy [B] of the posterior, kl_post_prior [B] =
        KL(p(k|x) || pi), ess [B] = the effective sample size of iw_bound's n weights, tail [8] = the batch sums of (-bound,
        entropy, kl_post_prior, ess), B).  chunk, row0 and the noise keying as iw_bound: the result does not depend on the chunk,
        the batch size or the sharding."""
        if self.model != L.MODEL_VAE_GMP:
            raise ValueError("posterior_component is the posterior over the components of the VAE's learned mixture prior: "
                             "it needs model 'vae_gmp' (the GMVAE has posterior_y)")
        (lj, lp, stats), tail = self._chunked_eval("posterior_component", x, n_samples, chunk, row0)
        return dict(log_joint=lj, log_post=lp, bound=stats[:, 0], entropy=stats[:, 1], kl_post_prior=stats[:, 2],
                    ess=stats[:, 3], tail=tail)

    def ais_bound(self, x, n_chains: int = 16, n_temps: int = 1000, schedule="sigmoid", n_leapfrog: int = 10,
                  step_size: float = 0.05, init: str = "prior", adapt: bool = True, row0: Optional[int] = None,
                  eps: Optional[torch.Tensor] = None, u: Optional[torch.Tensor] = None, step_up: float = 1.02,
                  step_down: float = 0.96):
        """log p(x) by annealed importance sampling with HMC transitions (include/gmvae_hip.h gmvae_ais; Neal 2001; Wu et al.
        2017): n_chains chains per example anneal from the base to p(z) p(x|z) over n_temps temperatures, n_leapfrog leapfrog
        steps of step_size per transition.  It uses the generative model alone, so -- unlike iw_bound, iw_bound_enum_y and the
        posteriors, which are importance sampling from the inference network -- its gap says nothing about q, and it tightens
        towards log p(x) as n_temps grows: iw_bound far below ais_bound is a weak encoder, both low a weak decoder.
        init: "prior" -- the chains start from p(z) -- or "encoder": from the example's inference mixture (_latent_components:
        q(z|x), for the GMVAE sum_k q(k|x) q(z|x, e_k)), a shorter path for the same target.
        schedule: "sigmoid" -- beta_t = (s(4 (2 t / T - 1)) - s(-4)) / (s(4) - s(-4)) --, "linear", or a tensor of n_temps + 1
        increasing values from 0 to 1.
        adapt: every chain multiplies its step size by step_up after an accepted transition and step_down after a rejected one
        (1.02 and 0.96: their fixed point is an acceptance rate of ln(1 / 0.96) / (ln 1.02 + ln(1 / 0.96)) = 0.67), clipped to
        [1e-4, 1].  adapt=False keeps step_size: that is the strictly valid AIS -- an adapted step depends on the chain's past,
        so the adapted estimate is not exactly unbiased in the weights; in practice the difference is far below the chains'
        standard error.
        Returns dict(bound [B] = logsumexp_c log w - ln n_chains, logw [B, n_chains], stats [B, 4] = (bound, effective sample
        size of the chains' weights, mean acceptance rate, mean final step size), z [B n_chains, L] = the chains' final states
        (approximate posterior samples), tail [8] = the batch sums of (-bound, ESS, acceptance rate, step size), B).  For the
        GMVAE the bound estimates log p(x) itself, the uniform p(y) inside: it is comparable to iw_bound_enum_y's bound MINUS ln K
        (that one leaves the + ln K out).
        Chain c of row b draws Philox row (row0 + b) * n_chains + c keyed by (noise_seed, global_step * (n_temps + 1) + t), row0
        defaulting to rank * B: the result does not depend on the batch size or the sharding.  eps [n_temps + 1, B n_chains, L] and
        u [n_temps + 1, B n_chains] replace the draw (tests).  Bernoulli likelihood only; not with pixel_mask."""
        return self._ais_chains("ais_bound", x, None, n_chains, n_temps, schedule, n_leapfrog, step_size, init, adapt, row0, eps, u,
                                step_up, step_down, self.noise_seed)

    def _ais_chains(self, what, x, z_start, n_chains, n_temps, schedule, n_leapfrog, step_size, init, adapt, row0, eps, u, step_up,
                    step_down, seed):
        """One gmvae_ais call (z_start None) or one gmvae_ais_reverse call from z_start [B, L]: the common host side."""
        self._require_plain_bernoulli(what)
        if init not in ("prior", "encoder"):
            raise ValueError(f"init must be 'prior' or 'encoder', got {init!r}")
        C_, T, nl = int(n_chains), int(n_temps), int(n_leapfrog)
        if C_ < 1 or T < 1 or nl < 1:
            raise ValueError(f"n_chains, n_temps and n_leapfrog must be >= 1, got {C_}, {T}, {nl}")
        if not (0.0 < float(step_size) < float("inf")):
            raise ValueError(f"step_size must be positive and finite, got {step_size}")
        betas = ais_schedule(schedule, T).to(self.device, torch.float32).contiguous()
        x = self._prep_x(x)
        B = x.shape[0]
        d = self.dims(B, 1, row0)
        base, base_K = None, 0
        if init == "encoder":
            logpi, mu, sigma = self._latent_components(x)
            base_K = logpi.shape[1]
            base = torch.cat([logpi.reshape(B, base_K), mu.reshape(B, -1), sigma.reshape(B, -1)], dim=1).contiguous()
        n = B * C_
        eps = self._prep_noise(eps, (T + 1) * n, self.Lz)
        u = self._prep_noise(u, (T + 1) * n, 1)
        up, down = (float(step_up), float(step_down)) if adapt else (1.0, 1.0)
        ws, _ = self._cached_ws(("ais", B, C_, base_K), L.ais_workspace_bytes(d, self.model, base_K, C_) // 4 + 64)
        f32 = dict(dtype=torch.float32, device=self.device)
        o = dict(logw=torch.empty(B, C_, **f32), bound=torch.empty(B, **f32), stats=torch.empty(B, 4, **f32),
                 z=torch.empty(n, self.Lz, **f32), tail=torch.empty(L.TAIL, **f32))
        out = (L.ptr(eps), L.ptr(u), L.ptr(o["logw"]), L.ptr(o["bound"]), L.ptr(o["stats"]), L.ptr(o["z"]), L.ptr(o["tail"]), L.ptr(ws),
               int(seed), self.global_step, L.current_stream())
        if z_start is None:
            rc = L.lib.gmvae_ais(C.byref(d), self.model, L.ptr(x), L.ptr(self.params), L.ptr(base), base_K, L.ptr(betas), T, C_, nl,
                                 float(step_size), up, down, *out)
        else:
            z_start = z_start.to(self.device, torch.float32).contiguous()
            if tuple(z_start.shape) != (B, self.Lz):
                raise ValueError(f"z_start must be [B, L] = [{B}, {self.Lz}], got {tuple(z_start.shape)}")
            rc = L.lib.gmvae_ais_reverse(C.byref(d), self.model, L.ptr(x), L.ptr(self.params), L.ptr(base), base_K, L.ptr(z_start),
                                         L.ptr(betas), T, C_, nl, float(step_size), up, down, *out)
        L.check(rc, "gmvae_ais" if z_start is None else "gmvae_ais_reverse")
        self._keep_ais = (x, base, betas, eps, u, z_start)
        return o

    # Philox keys of the bidirectional pair: the forward chains keep ais_bound's key (noise_seed), the simulation and the reverse
    # chains each take the seed with a fixed pattern folded in -- another Philox key is another stream, so the three are disjoint
    _SIM_SALT, _REV_SALT = 0x53494D5F42444D43, 0x5245565F42444D43

    def simulate(self, n: int, row0: Optional[int] = None, eps: Optional[torch.Tensor] = None, u: Optional[torch.Tensor] = None,
                 ux: Optional[torch.Tensor] = None):
        """n ancestral samples (z*, x) ~ p(z) p(x|z) from the generative model (include/gmvae_hip.h gmvae_simulate): a component k
        of the prior by inverse CDF (for the GMVAE k is y, uniform), z* = mu_k + sigma_k eps, x_d = [u_d < sigmoid(lambda_d(z*))].
        z* is an EXACT posterior sample for x -- what ais_bound_reverse starts from.  Returns dict(z [n, L], k [n] int32,
        x [n, D] uint8, prob [n, D] = sigmoid(lambda)).  Example b draws Philox row row0 + b (default rank * n) keyed by
        (noise_seed with a fixed pattern folded in, 2 global_step and 2 global_step + 1): disjoint from every other draw of this
        engine, independent of the batch and the sharding.  eps [n, L], u [n] and ux [n, D] replace the draws (tests).
        Bernoulli likelihood only; not with pixel_mask."""
        self._require_plain_bernoulli("simulate")
        n = int(n)
        if n < 1:
            raise ValueError(f"n must be >= 1, got {n}")
        d = self.dims(n, 1, row0)
        eps, u, ux = self._prep_noise(eps, n, self.Lz), self._prep_noise(u, n, 1), self._prep_noise(ux, n, self.D)
        ws, _ = self._cached_ws(("simulate",), L.simulate_workspace_bytes(d, self.model) // 4 + 64)
        o = dict(z=torch.empty(n, self.Lz, dtype=torch.float32, device=self.device),
                 k=torch.empty(n, dtype=torch.int32, device=self.device),
                 x=torch.empty(n, self.D, dtype=torch.uint8, device=self.device),
                 prob=torch.empty(n, self.D, dtype=torch.float32, device=self.device))
        rc = L.lib.gmvae_simulate(C.byref(d), self.model, L.ptr(self.params), L.ptr(eps), L.ptr(u), L.ptr(ux), L.ptr(o["z"]),
                                  L.ptr(o["k"]), L.ptr(o["x"]), L.ptr(o["prob"]), L.ptr(ws), self.noise_seed ^ self._SIM_SALT,
                                  self.global_step, L.current_stream())
        L.check(rc, "gmvae_simulate")
        self._keep_sim = (eps, u, ux)
        return o

    def ais_bound_reverse(self, x, z_start, n_chains: int = 16, n_temps: int = 1000, schedule="sigmoid", n_leapfrog: int = 10,
                          step_size: float = 0.05, init: str = "prior", adapt: bool = True, row0: Optional[int] = None,
                          eps: Optional[torch.Tensor] = None, u: Optional[torch.Tensor] = None, step_up: float = 1.02,
                          step_down: float = 0.96):
        """An UPPER bound on log p(x) from ais_bound's chains run backwards (include/gmvae_hip.h gmvae_ais_reverse; Grosse,
        Ghahramani & Adams 2015): every chain of example b starts at z_start[b], which must be an exact posterior sample for x[b],
        and anneals from beta = 1 down to 0 -- at each temperature first the HMC transition, then the weight update at the new
        point.  Such a sample exists ONLY for simulated data (simulate's z for simulate's x): there is no exact posterior sample
        for a real x, and so no upper bound for it.
        Keywords and the returned dict are ais_bound's, with bound [B] = -(logsumexp_c log w_rev - ln n_chains) the upper bound,
        logw = log w_rev, stats = (that bound, the ESS of the reverse weights, acceptance rate, final step size), z = the chains'
        ends z_0, tail[0] the batch sum of -bound.  adapt=False is the strictly valid form, as for ais_bound: an adapted step size
        depends on the chain's past, so the adapted weights are not exactly unbiased; in practice the difference is far below the
        chains' standard error.  The chains draw ais_bound's Philox rows and steps under another key (noise_seed with a fixed
        pattern folded in), so the two directions never share a draw.  eps and u have ais_bound's layout, slot 0 unused."""
        return self._ais_chains("ais_bound_reverse", x, z_start, n_chains, n_temps, schedule, n_leapfrog, step_size, init, adapt,
                                row0, eps, u, step_up, step_down, self.noise_seed ^ self._REV_SALT)

    def bdmc_gap(self, n_examples: int, n_chains: int = 16, n_temps: int = 1000, row0: Optional[int] = None, **kw):
        """Bidirectional Monte Carlo (Grosse, Ghahramani & Adams 2015; the validation of Wu et al. 2017): how far below log p(x)
        ais_bound sits at these settings.  n_examples are simulated from the model (simulate); ais_bound on the simulated x gives
        the lower bound -- the very call ais_bound(x_sim, n_chains, n_temps, row0=row0, **kw), bit for bit --, ais_bound_reverse
        from the simulation's own z the upper one, on Philox keys disjoint from both.  In expectation lower <= log p(x) <= upper,
        so gap = upper - lower bounds the bias of ais_log_px at n_chains, n_temps and kw (ais_bound's keywords: schedule,
        n_leapfrog, step_size, init, adapt, step_up, step_down).  The upper bound exists only for simulated data, because there is
        no exact posterior sample for a real x: the gap is a statement about data distributed as the model's own samples, and
        carries over to real data as far as the model fits them.  adapt=False is the strictly valid form in both directions
        (ais_bound's caveat).
        Returns dict(lower [n], upper [n], gap [n], lower_ess, upper_ess, lower_accept, upper_accept [n], x [n, D], z [n, L],
        k [n], forward, reverse = the two calls' dicts, and the means lower_mean, upper_mean, gap_mean, upper_ess_mean,
        upper_accept_mean)."""
        sim = self.simulate(n_examples, row0=row0)
        fwd = self.ais_bound(sim["x"], n_chains, n_temps, row0=row0, **kw)
        rev = self.ais_bound_reverse(sim["x"], sim["z"], n_chains, n_temps, row0=row0, **kw)
        lower, upper = fwd["bound"], rev["bound"]
        gap = upper.double() - lower.double()
        return dict(lower=lower, upper=upper, gap=gap, lower_ess=fwd["stats"][:, 1], upper_ess=rev["stats"][:, 1],
                    lower_accept=fwd["stats"][:, 2], upper_accept=rev["stats"][:, 2], x=sim["x"], z=sim["z"], k=sim["k"],
                    forward=fwd, reverse=rev, lower_mean=lower.double().mean().item(), upper_mean=upper.double().mean().item(),
                    gap_mean=gap.mean().item(), upper_ess_mean=rev["stats"][:, 1].double().mean().item(),
                    upper_accept_mean=rev["stats"][:, 2].double().mean().item())

    REFINE_STATS = ("elbo_start", "elbo_refined", "iw_start", "iw_refined", "ess_refined", "updates", "mean_shift",
                    "log_sigma_ratio")

    def refine_posterior(self, x, n_steps: int = 500, n_samples: int = 4, n_eval: int = 256, lr: float = 0.05,
                         betas=(0.9, 0.999), adam_eps: float = 1e-8, row0: Optional[int] = None,
                         eps: Optional[torch.Tensor] = None, start: Optional[torch.Tensor] = None):
        """Per-example refinement of q(z|x) (include/gmvae_hip.h gmvae_refine; Cremer, Li & Duvenaud 2018): for every example a
        local Gaussian q_phi(z) = N(m, diag sigma^2) starts at the encoder's output and climbs the example's own ELBO, log p(x, z)
        with y summed out, by n_steps steps of TF-Adam ascent (lr, betas, adam_eps) on n_samples reparameterised draws each; the
        ELBO and the importance-weighted bound of the start and of the refined phi* are then evaluated on the same n_eval draws
        (rounded up to a multiple of n_samples).  elbo_refined - elbo_start is what the encoder loses against the best member of
        its own family on that example (the amortisation gap); what remains up to log p(x) only a richer family closes.
        The start comes from _latent_components: q(z|x) for the VAE family; for the GMVAE the component at argmax_k q(k|x),
        lowest index on ties.  start [B, 2 L] = (mu_0, sigma_0) replaces it.
        Returns dict(phi [B, 2 L] = (m*, sigma*), trace [n_steps, B] = the ELBO estimate before each step, stats [B, 8] and its
        columns by name -- elbo_start, elbo_refined, iw_start, iw_refined, ess_refined (of the n_eval weights at phi*), updates
        (steps applied: a step whose gradient is not finite is skipped), mean_shift = mean_l |m* - mu_0| / sigma_0,
        log_sigma_ratio = mean_l ln(sigma* / sigma_0) --, tail [8] = the batch sums of the first four, B).
        Sample s of row b draws Philox row (row0 + b) * n_samples + s keyed by (noise_seed, global_step * (n_steps + rounds + 1)
        + t), row0 defaulting to rank * B: the result does not depend on the batch size or the sharding.  eps [n_steps + rounds,
        B n_samples, L] replaces the draw (tests).  Bernoulli likelihood only; not with pixel_mask."""
        self._require_plain_bernoulli("refine_posterior")
        T, S, N = int(n_steps), int(n_samples), int(n_eval)
        if S not in (1, 2, 4, 8, 16):
            raise ValueError(f"n_samples must be one of 1, 2, 4, 8, 16, got {n_samples}")
        if T < 0 or N < 1:
            raise ValueError(f"n_steps must be >= 0 and n_eval >= 1, got {T}, {N}")
        if not (0.0 < float(lr) < float("inf")):
            raise ValueError(f"lr must be positive and finite, got {lr}")
        R = (N + S - 1) // S
        x = self._prep_x(x)
        B = x.shape[0]
        d = self.dims(B, 1, row0)
        if start is None:
            logpi, mu, sigma = self._latent_components(x)
            Kc = logpi.shape[1]
            k = torch.argmax(logpi, dim=1) + Kc * torch.arange(B, device=self.device)      # (argmax: the first of equal values)
            start = torch.cat([mu[k], sigma[k]], dim=1)
        start = start.to(self.device, torch.float32).contiguous()
        if tuple(start.shape) != (B, 2 * self.Lz):
            raise ValueError(f"start must be [B, 2 L] = [{B}, {2 * self.Lz}] (mu_0, sigma_0), got {tuple(start.shape)}")
        eps = self._prep_noise(eps, (T + R) * B * S, self.Lz)
        ws, _ = self._cached_ws(("refine", B, S), L.refine_workspace_bytes(d, self.model, S) // 4 + 64)
        f32 = dict(dtype=torch.float32, device=self.device)
        o = dict(phi=torch.empty(B, 2 * self.Lz, **f32), trace=torch.empty(T, B, **f32), stats=torch.empty(B, 8, **f32),
                 tail=torch.empty(L.TAIL, **f32))
        rc = L.lib.gmvae_refine(C.byref(d), self.model, L.ptr(x), L.ptr(self.params), L.ptr(start), T, S, R, float(lr),
                                float(betas[0]), float(betas[1]), float(adam_eps), L.ptr(eps), L.ptr(o["phi"]),
                                L.ptr(o["trace"]) if T else None, L.ptr(o["stats"]), L.ptr(o["tail"]), L.ptr(ws), self.noise_seed,
                                self.global_step, L.current_stream())
        L.check(rc, "gmvae_refine")
        self._keep_refine = (x, start, eps)
        for i, name in enumerate(self.REFINE_STATS):
            o[name] = o["stats"][:, i]
        o["start"] = start
        return o

    def inference_gaps(self, x, n_steps: int = 500, n_samples: int = 4, n_eval: int = 256, lr: float = 0.05, betas=(0.9, 0.999),
                       adam_eps: float = 1e-8, ais: Optional[dict] = None, row0: Optional[int] = None):
        """The inference gap log p(x) - L[q(z|x)] of a batch split in two (Cremer, Li & Duvenaud 2018), batch means as floats:
          amortisation_gap = elbo_refined - elbo_amortised: what the encoder loses against q*, the best single Gaussian for each
            example (refine_posterior) -- more encoder capacity or training closes it;
          approximation_gap = log_px - elbo_refined: what the family loses -- only a richer family or another model closes it.
        elbo_amortised is refine_posterior's elbo_start for the VAE family.  For the GMVAE it is the z-marginal ELBO of the
        inference MIXTURE sum_k q(k|x) q(z|x, e_k), E_q[log p(x, z) - log q(z|x)] on n_eval draws (ais_bound at n_temps=1,
        init="encoder": the mean of its log w), and elbo_start, the ELBO of the one component refine_posterior starts from, is
        reported beside it.  The GMVAE's amortised family is thus a K-mixture and the local one a single Gaussian: where q(y|x) is
        genuinely spread the mixture can beat every single Gaussian and the amortisation gap is NEGATIVE; it is reported as it is.
        log_px is the larger of the batch means of iw_refined and, with ais = a dict of ais_bound's arguments (n_chains, n_temps,
        ...), of the AIS bound (ais_log_px, else None): both are lower bounds in expectation, so the larger is the better
        estimate -- Cremer et al.'s convention.  Also returned: iw_bound_refined, the per-example tensors elbo_amortised_rows,
        ais_rows (or None) and refine = refine_posterior's dict.  row0 as refine_posterior's."""
        r = self.refine_posterior(x, n_steps, n_samples, n_eval, lr, betas, adam_eps, row0=row0)
        am = r["elbo_start"].double()
        if self.model == L.MODEL_GMVAE:
            am = self.ais_bound(x, n_chains=int(n_eval), n_temps=1, init="encoder", n_leapfrog=1, row0=row0)["logw"].double().mean(dim=1)
        ab = None if ais is None else self.ais_bound(x, row0=row0, **ais)["bound"].double()
        o = dict(refine=r, elbo_amortised_rows=am, ais_rows=ab, elbo_amortised=am.mean().item(),
                 elbo_start=r["elbo_start"].double().mean().item(), elbo_refined=r["elbo_refined"].double().mean().item(),
                 iw_bound_refined=r["iw_refined"].double().mean().item(), ais_log_px=None if ab is None else ab.mean().item())
        o["log_px"] = o["iw_bound_refined"] if ab is None else max(o["iw_bound_refined"], o["ais_log_px"])
        o["amortisation_gap"] = o["elbo_refined"] - o["elbo_amortised"]
        o["approximation_gap"] = o["log_px"] - o["elbo_refined"]
        return o

    AGG_CHUNK = 2048               # default examples per pass of aggregate_posterior (K rows each for the GMVAE)

    def _normal_head(self, out: torch.Tensor):
        """(mu, sigma) of a conditional normal's MLP output [rows, 2 L]: sigma = max(softplus(raw + raw_sigma_bias), sigma_min)
        (scripts/base.py:66-72)."""
        mu, raw = out[:, :self.Lz], out[:, self.Lz:]
        sigma = torch.nn.functional.softplus(raw + self.hp["raw_sigma_bias"]).clamp_min(self.hp["sigma_min"])
        return mu.contiguous(), sigma.contiguous()

    def _latent_components(self, xb: torch.Tensor):
        """q(z | x) of a batch as mixture components, example-major: (log pi [n, Kc], mu [n Kc, L], sigma [n Kc, L]) with Kc = K
        for the GMVAE -- pi = softmax(encoder_y(x)), (mu, sigma) = encoder_gmm(x, one-hot k), the convention of iw_bound_enum_y
        and posterior_y whatever the engine's y_inference -- and Kc = 1, log pi = 0 for the VAE family."""
        n = xb.shape[0]
        if self.model != L.MODEL_GMVAE:
            mu, sigma = self._normal_head(self.mlp(L.NET_ENCODER, xb))
            return torch.zeros(n, 1, dtype=torch.float32, device=self.device), mu, sigma
        logpi = torch.log_softmax(self.mlp(L.NET_ENCODER_Y, xb), dim=1)
        onehot = torch.eye(self.K, dtype=torch.float32, device=self.device).repeat(n, 1)
        mu, sigma = self._normal_head(self.mlp(L.NET_ENCODER_GMM, xb.repeat_interleave(self.K, dim=0), onehot))
        return logpi.contiguous(), mu, sigma

    def _mixture_logpdf(self, ws, z, mu, sigma, logw, c_first=0, comps_per_owner=1, owner=None, per_dim=True):
        """One chunk of components folded into the workspace's running state (include/gmvae_hip.h
        gmvae_mixture_logpdf_accumulate)."""
        rc = L.lib.gmvae_mixture_logpdf_accumulate(L.ptr(z), z.shape[0], self.Lz, L.ptr(mu), L.ptr(sigma), L.ptr(logw),
                                                   mu.shape[0], int(c_first), int(comps_per_owner), L.ptr(owner), int(per_dim),
                                                   L.ptr(ws), L.current_stream())
        L.check(rc, "gmvae_mixture_logpdf_accumulate")

    def _mixture_finish(self, ws, M, per_dim, log_norm, own):
        f32 = dict(dtype=torch.float32, device=self.device)
        joint = torch.empty(M, **f32)
        dim = torch.empty(M, self.Lz, **f32) if per_dim else None
        lown = torch.empty(M, **f32) if own else None
        rc = L.lib.gmvae_mixture_logpdf_finish(M, self.Lz, int(per_dim), float(log_norm), L.ptr(joint), L.ptr(dim), L.ptr(lown),
                                               L.ptr(ws), L.current_stream())
        L.check(rc, "gmvae_mixture_logpdf_finish")
        return joint, dim, lown

    @torch.no_grad()
    def aggregate_posterior(self, x, queries: Optional[torch.Tensor] = None, per_dim: bool = True, chunk: Optional[int] = None,
                            row0: Optional[int] = None):
        """Diagnostics of the aggregate posterior q(z) = 1/N sum_n q(z | x_n) over the examples x [N, D] (Hoffman & Johnson 2016;
        Chen et al. 2018): E_x KL(q(z|x) || p(z)) = I_q(x; z) + KL(q(z) || p(z)), and KL(q(z) || p(z)) = TC(q(z)) + sum_d
        KL(q(z_d) || p(z_d)) (+ a rest for a mixture prior).  All three models; for the GMVAE q(z | x) = sum_k pi_k(x) N(mu_k(x),
        sigma_k(x)) with the one-hot y of iw_bound_enum_y and posterior_y, whatever the engine's y_inference.
        queries: None -- every example -- or an int tensor [M] of indices into x; one sample z_m ~ q(z | x_queries[m]) each (GMVAE:
        k by Gumbel-max on log pi + g, then z = mu_k + sigma_k eps), the noise being gmvae_noise_fill's rows row0 + m keyed by
        (noise_seed, global_step), row0 defaulting to rank * M.  Every log-density is a logsumexp over all N (N K) components in
        the HIP evaluator gmvae_mixture_logpdf_* (include/gmvae_hip.h), streamed `chunk` examples at a time (default AGG_CHUNK):
        the memory depends on chunk and M, not on N, and the result does not depend on chunk beyond fp64 fold order.
        Returns a dict.  Per query: z [M, L], log_q_zx [M] = log q(z | x_own), log_q_z [M] = log q(z) (log N subtracted), log_q_zd
        [M, L] = log q(z_d), log_p_z [M], log_p_zd [M, L] (the prior and its marginals: closed form for the VAE, the same kernel
        over the K components of the VAE_GMP's mixture and of the GMVAE's 1/K sum_k prior_gmm(e_k)).  Means over the queries, 0-d
        fp64 device tensors: kl_avg = mean(log_q_zx - log_p_z), mi = mean(log_q_zx - log_q_z) (<= ln N), kl_marginal =
        mean(log_q_z - log_p_z), tc = mean(log_q_z - sum_d log_q_zd), dim_kl [L] = mean(log_q_zd - log_p_zd).  From the encoder
        alone: au_variance [L] = the variance over the N examples of E[z_d | x] = sum_k pi_k mu_kd and active_units = the count
        above 0.01 (Burda et al. 2016); GMVAE: q_y [K] = mean_n pi_n, q_y_entropy = H(q_y), mi_xy = H(q_y) - mean_n H(pi_n) (None
        for the VAE family).  per_dim=False skips the per-dimension terms (L times the exponentials): log_q_zd, log_p_zd, tc and
        dim_kl are None.  Not with pixel_mask=True (the encoders here take no mask).  One device: across ranks each rank
        reports its own shard's aggregate posterior."""
        if self.pixel_mask:
            raise ValueError("aggregate_posterior is not available with pixel_mask=True (Engine.mlp encodes x without a mask)")
        x = self._prep_x(x)
        N, Lz, gm = x.shape[0], self.Lz, self.model == L.MODEL_GMVAE
        Kc = self.K if gm else 1
        if N < 1:
            raise ValueError("aggregate_posterior needs at least one example")
        chunk = self.AGG_CHUNK if chunk is None else int(chunk)
        if chunk < 1:
            raise ValueError(f"chunk must be >= 1, got {chunk}")
        if queries is None:
            qidx = torch.arange(N, dtype=torch.int64, device=self.device)
        else:
            qidx = torch.as_tensor(queries).to(self.device, torch.int64).reshape(-1).contiguous()
            if qidx.numel() < 1 or int(qidx.min()) < 0 or int(qidx.max()) >= N:
                raise ValueError(f"queries must be a non-empty tensor of indices into the {N} examples")
        M = qidx.numel()
        row0 = self.rank * M if row0 is None else int(row0)
        f32 = dict(dtype=torch.float32, device=self.device)
        f64 = dict(dtype=torch.float64, device=self.device)
        # one sample per query
        eps = torch.empty(M, Lz, **f32)
        u = torch.empty(M, self.K, **f32) if gm else None
        L.check(L.lib.gmvae_noise_fill(L.ptr(eps), L.ptr(u), M, Lz, self.K, row0, self.noise_seed, self.global_step, None,
                                       L.current_stream()), "gmvae_noise_fill")
        z = torch.empty(M, Lz, **f32)
        for m0 in range(0, M, chunk):
            sl = slice(m0, min(M, m0 + chunk))
            logpi, mu, sigma = self._latent_components(x[qidx[sl]])
            rows = torch.arange(logpi.shape[0], device=self.device) * Kc
            if gm:
                rows = rows + (logpi.double() - torch.log(-torch.log(u[sl].double()))).argmax(dim=1)
            z[sl] = mu[rows] + sigma[rows] * eps[sl]
        # the aggregate posterior: every example's components through the evaluator, and the encoder-only statistics
        nb = C.c_uint64()
        L.check(L.lib.gmvae_mixture_logpdf_workspace_bytes(M, Lz, int(per_dim), C.byref(nb)), "gmvae_mixture_logpdf_workspace_bytes")
        ws = torch.zeros(nb.value // 8, **f64)
        ez_sum, ez_sq = torch.zeros(Lz, **f64), torch.zeros(Lz, **f64)
        pi_sum, hy_sum = torch.zeros(Kc, **f64), torch.zeros((), **f64)
        for n0 in range(0, N, chunk):
            logpi, mu, sigma = self._latent_components(x[n0:n0 + chunk])
            self._mixture_logpdf(ws, z, mu, sigma, logpi.reshape(-1), n0 * Kc, Kc, qidx, per_dim)
            pi = logpi.double().exp()
            ez = (pi.unsqueeze(2) * mu.double().view(-1, Kc, Lz)).sum(dim=1)
            ez_sum += ez.sum(dim=0)
            ez_sq += (ez * ez).sum(dim=0)
            pi_sum += pi.sum(dim=0)
            hy_sum -= (pi * logpi.double().clamp_min(-745.0)).sum()
        log_q_z, log_q_zd, log_q_zx = self._mixture_finish(ws, M, per_dim, math.log(N), True)
        # the prior
        if self.model == L.MODEL_VAE:
            t = -0.5 * z * z - 0.5 * math.log(2.0 * math.pi)
            log_p_z, log_p_zd = t.double().sum(dim=1).float(), (t if per_dim else None)
        else:
            if gm:
                eye = torch.eye(self.K, **f32)
                pmu, psig = self._normal_head(self.mlp(L.NET_PRIOR_GMM, eye))
                plogw = torch.full((self.K,), -math.log(self.K), **f32)
            else:
                v = self.views()
                pmu = v["loc"].contiguous()
                psig = torch.nn.functional.softplus(v["raw_scale_diag"]).contiguous()
                plogw = torch.log_softmax(v["mixture_logits"], dim=0).contiguous()
            ws.zero_()
            self._mixture_logpdf(ws, z, pmu, psig, plogw, per_dim=per_dim)
            log_p_z, log_p_zd, _ = self._mixture_finish(ws, M, per_dim, 0.0, False)
        own, agg, pri = log_q_zx.double(), log_q_z.double(), log_p_z.double()
        ez_mean = ez_sum / N
        au_var = (ez_sq / N - ez_mean * ez_mean).clamp_min(0.0)
        out = dict(z=z, log_q_zx=log_q_zx, log_q_z=log_q_z, log_q_zd=log_q_zd, log_p_z=log_p_z, log_p_zd=log_p_zd,
                   kl_avg=(own - pri).mean(), mi=(own - agg).mean(), kl_marginal=(agg - pri).mean(),
                   tc=(agg - log_q_zd.double().sum(dim=1)).mean() if per_dim else None,
                   dim_kl=(log_q_zd.double() - log_p_zd.double()).mean(dim=0) if per_dim else None,
                   au_variance=au_var, active_units=(au_var > 0.01).sum(), q_y=None, q_y_entropy=None, mi_xy=None)
        if gm:
            q_y = pi_sum / N
            h_qy = -(q_y * q_y.clamp_min(1e-300).log()).sum()
            out.update(q_y=q_y, q_y_entropy=h_qy, mi_xy=h_qy - hy_sum / N)
        return out

    def mlp(self, net: int, inp: torch.Tensor, in2: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One conditional network's MLP on the device (snt.nets.MLP, scripts/base.py:47-60)."""
        if self.real_valued and net in (L.NET_ENCODER_Y, L.NET_ENCODER_GMM, L.NET_ENCODER):
            inp = self._prep_x(inp)                                 # (the networks that read x read the floats themselves)
            if self.count_likelihood:
                inp = torch.log1p(inp)                              # (... counts: t = log1p(x))
        elif self.likelihood != "bernoulli" and net in (L.NET_ENCODER_Y, L.NET_ENCODER_GMM, L.NET_ENCODER):
            inp = self._prep_x(inp).to(torch.float32) / 255.0       # (the networks that read x read t = x / 255 as fp32)
        is_u8 = inp.dtype in (torch.uint8, torch.bool)
        inp = self._as_u8(inp.to(self.device)) if is_u8 else inp.to(self.device, torch.float32).contiguous()
        inp = inp.reshape(inp.shape[0], -1)
        rows = inp.shape[0]
        if in2 is not None:
            in2 = in2.to(self.device, torch.float32).contiguous()
        d, ws = self._workspace(rows, 1)
        out_dim = {L.NET_ENCODER_Y: self.K, L.NET_PRIOR_GMM: 2 * self.Lz, L.NET_ENCODER_GMM: 2 * self.Lz,
                   L.NET_DECODER: self.D, L.NET_ENCODER: 2 * self.Lz}[net]
        out = torch.empty(rows, out_dim, dtype=torch.float32, device=self.device)
        rc = L.lib.gmvae_mlp_forward(C.byref(d), self.model, net, L.ptr(inp), int(is_u8), L.ptr(in2), rows,
                                     L.ptr(self.params), L.ptr(out), L.ptr(ws), L.current_stream())
        L.check(rc, "gmvae_mlp_forward")
        return out

    def adam(self, lr: float = 1e-3, beta1=0.9, beta2=0.999, epsilon=1e-8, grads: Optional[torch.Tensor] = None,
             use_step_dev: bool = False):
        """TF-formula Adam over the flat buffer; gradient sums are scaled by
        1/count read from the (possibly all-reduced) tail on the device."""
        g = self.grads if grads is None else grads
        self._param_epoch += 1
        if not use_step_dev:
            self.global_step += 1
        count = g[self.P + 4:self.P + 5]
        loss_sum = g[self.P:self.P + 1]          # non-finite (poisoned step, on any rank) -> the update is skipped
        if self.clip_norm is not None:
            # the record of THIS buffer (behind train_step's all-reduce: the global gradient): its divisor stands where the count
            # stood, its guard where the loss sum stood
            self._push_clip_norm()
            rc = L.lib.gmvae_grad_clip(L.ptr(g), self.P, L.ptr(self._clip_dev), L.ptr(self.grad_clip),
                                       L.ptr(self._clip_scratch), L.current_stream())
            L.check(rc, "gmvae_grad_clip")
            count, loss_sum = self.grad_clip[1:2], self.grad_clip[3:4]
        rc = L.lib.adam_tf_step(L.ptr(self.params), L.ptr(self.m), L.ptr(self.v), L.ptr(g), self.P, lr, beta1, beta2,
                                epsilon, self.global_step, L.ptr(self.step_dev) if use_step_dev else None, 1.0,
                                L.ptr(count), L.ptr(loss_sum), L.current_stream())
        L.check(rc, "adam_tf_step")
        if not use_step_dev:
            self.step_dev.fill_(self.global_step)   # one source of truth: graphs replayed later start from here

    def train_step(self, x, eps=None, u=None, lr: float = 1e-3, all_reduce: bool = True,
                   row0: Optional[int] = None, y_observed: Optional[torch.Tensor] = None,
                   beta1: float = 0.9, beta2: float = 0.999, epsilon: float = 1e-8,
                   mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One full reference step: fwd + bwd (+ RCCL all-reduce) + Adam (beta1, beta2, epsilon: tf.train.AdamOptimizer's).
        Returns the [TAIL] loss sums (device tensor; no host sync)."""
        import torch.distributed as dist
        self.step(x, eps, u, row0=row0, y_observed=y_observed, mask=mask)
        if all_reduce and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            from . import parallel
            parallel.all_reduce_flat(self.grads)     # ONE collective: grads + loss sums + count
        self.adam(lr, beta1, beta2, epsilon)
        return self.grads[self.P:]

    # -------------------------------------------------- data parallel over RCCL inside the C library
    def _agree(self, ok: bool) -> bool:
        """True only if `ok` on EVERY rank (one all-reduce(MIN)): ranks must never split over a fallback decision,
        or they would issue mismatched collectives and hang."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return bool(ok)
        t = torch.tensor([1 if ok else 0], dtype=torch.int32)
        t = t.to(self.device) if dist.get_backend() == "nccl" else t
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        return bool(t.item())

    def enable_rccl(self):
        """Creates this rank's RCCL communicator inside libgmvae_hip.so (the 128-byte unique id travels over
        torch.distributed).  Afterwards train_step / capture_train_step(all_reduce=True) enqueue
        gradients -> ONE all-reduce -> Adam from a single C call (or one hipGraph).  Every rank takes every
        collective of this function whatever happens locally; a failure on any rank raises on ALL ranks."""
        import torch.distributed as dist
        if getattr(self, "_comm", None):
            return self._comm
        world = dist.get_world_size() if dist.is_initialized() else 1
        rank = dist.get_rank() if dist.is_initialized() else 0
        buf = C.create_string_buffer(128)
        ok, why = True, ""
        if rank == 0:
            rc = L.lib.gmvae_comm_unique_id(L.rccl_path(), buf)
            ok, why = rc == 0, f"gmvae_comm_unique_id rc={rc}"
        if world > 1:
            t = torch.frombuffer(bytearray(buf.raw), dtype=torch.uint8).clone()
            t = t.to(self.device) if dist.get_backend() == "nccl" else t
            dist.broadcast(t, src=0)
            buf = C.create_string_buffer(bytes(t.cpu().numpy().tobytes()), 128)
        if not self._agree(ok):
            raise L.GmvaeError(f"in-library RCCL unavailable on some rank ({why or 'another rank failed'})")
        comm = C.c_void_p()
        torch.cuda.synchronize()
        rc = L.lib.gmvae_comm_init(L.rccl_path(), buf, rank, world, C.byref(comm))
        if not self._agree(rc == 0):
            raise L.GmvaeError(f"gmvae_comm_init failed on some rank (this rank rc={rc}"
                               f"{': a rank did not join within GMVAE_COMM_INIT_TIMEOUT seconds' if rc == -7 else ''})")
        n = C.c_int(0)
        rc = L.lib.gmvae_comm_count(comm, C.byref(n))
        if not self._agree(rc == 0 and n.value == world):
            raise L.GmvaeError(f"the RCCL communicator spans {n.value} ranks (rc={rc}), torch.distributed's world is {world}")
        self._comm = comm
        self.rccl_nranks = n.value
        return comm

    def dp_step(self, x, lr: float = 1e-3, y_observed: Optional[torch.Tensor] = None,
                beta1: float = 0.9, beta2: float = 0.999, epsilon: float = 1e-8, mask: Optional[torch.Tensor] = None):
        """gmvae_dp_step: one C call enqueues step + RCCL all-reduce + Adam on the current stream."""
        x = self._prep_x(x)
        d, ws = self._workspace(x.shape[0])
        self._bind_step_inputs(d, ws, y_observed, mask)
        if self.clip_norm is not None:
            self._push_clip_norm()
        self._keep = (x, None, None)
        self._param_epoch += 1
        rc = L.lib.gmvae_dp_step(C.byref(d), self.model, L.ptr(x), L.ptr(self.params), L.ptr(self.m), L.ptr(self.v),
                                 L.ptr(self.grads), L.ptr(ws), self.noise_seed, L.ptr(self.step_dev), lr, beta1, beta2,
                                 epsilon, self._comm, L.current_stream())
        L.check(rc, "gmvae_dp_step")
        if self.clip_norm is not None:
            self.grad_clip.copy_(self._clip_records(d, ws)[0], non_blocking=True)      # (gmvae_dp_step writes record 0)
        self.global_step += 1
        return self.grads[self.P:]

    # -------------------------------------------------- hipGraph fast path
    def capture_train_step(self, B: int, lr: float = 1e-3, all_reduce: bool = False, n_steps: int = 1,
                           beta1: float = 0.9, beta2: float = 0.999, epsilon: float = 1e-8):
        """One hipGraph for noise + fwd + bwd + Adam at batch size B, captured and owned by the HIP
        library (gmvae_train_graph_*).  Returns (static_x, replay).  With n_steps > 1 the graph holds
        that many consecutive steps and static_x is [n_steps, B, D] (the next n_steps batches): one
        launch per n_steps steps hides the idle time between graph launches.  With all_reduce (data
        parallel) the RCCL all-reduce is captured too when the library owns the communicator
        (enable_rccl); otherwise the step is two eager halves around torch.distributed.all_reduce.
        beta1, beta2, epsilon: tf.train.AdamOptimizer's, baked into the graph like lr (and part of the key it is cached under).
        replay.tail_log [n_steps, TAIL]: the per-step tails of the last launch.  Per-step inputs (STEP_INPUTS; None where the
        engine has none): replay.y_observed [n_steps, B] (int32; pre-filled -1 = unlabelled), replay.obj_weights [n_steps, 4]
        (kl_weight, y_weight, y_free_nats, 0; pre-filled with the engine's current weights), replay.y_temperature [n_steps]
        (pre-filled with the engine's current temperature) and replay.pixel_mask [n_steps, B, D] (uint8; pre-filled 1 = all
        observed) are VIEWS of the workspace's regions; replay.grad_clip [n_steps, 4] (clip_norm; None without it) is the view of
        the records the launch WRITES (norm, divisor, clipped, guard per step): step i of the graph reads row i, the caller fills them before replay().
        Row 0 is also what every eager entry (step / loss / forward / train_step / dp_step) on the same batch size writes
        before it runs -- the engine's current weights and temperature, its y_observed and mask -- so after any eager call
        row 0 holds that call's values until the caller refills it: fill the rows before EVERY replay (run_train does)."""
        import torch.distributed as dist
        do_ar = all_reduce and ((dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1)
                                or getattr(self, "_comm", None) is not None)
        n_steps = int(n_steps)
        active = [inp for inp in STEP_INPUTS if getattr(self, inp.option)]
        if active and n_steps > L.LABEL_SLOTS:
            raise ValueError(f"a train graph of an engine with {active[0].option}=True holds at most {L.LABEL_SLOTS} steps (one "
                             f"{active[0].noun} per step), got {n_steps}")
        clip = self.clip_norm is not None
        if clip and n_steps > L.LABEL_SLOTS:
            raise ValueError(f"a train graph of an engine with clip_norm holds at most {L.LABEL_SLOTS} steps (one clip record "
                             f"per step), got {n_steps}")
        adam_hp = (float(beta1), float(beta2), float(epsilon))
        key = (B, lr, do_ar, n_steps) + adam_hp + (clip,)
        if key in self._graphs:
            self.step_dev.fill_(self.global_step)   # eager steps may have run since the capture
            return self._graphs[key][:2]
        xdt = torch.float32 if self.real_valued else torch.uint8      # (GMVAE_X_F32: step i reads the floats at x + i B D)
        if n_steps == 1:
            static_x = torch.zeros(B, self.D, dtype=xdt, device=self.device)
        else:
            static_x = torch.zeros(n_steps, B, self.D, dtype=xdt, device=self.device)
        d, ws = self._workspace(B)
        rows = {inp: self._slots(inp, d, ws)[:n_steps] for inp in active}      # step i reads row i; the caller fills them
        for inp, view in rows.items():
            self._fill(inp, view)
        self.step_dev.fill_(self.global_step)
        # per-step tails of one launch (loss sums + count; all-reduced under data parallelism): replay.tail_log
        tail_log = torch.zeros(n_steps, L.TAIL, dtype=torch.float32, device=self.device)
        records = self._clip_records(d, ws)[:n_steps] if clip else None      # step i writes row i

        def hand_out(replay, handle):
            replay.tail_log = tail_log
            replay.grad_clip = records
            for inp in STEP_INPUTS:
                setattr(replay, inp.replay, rows.get(inp))
            self._graphs[key] = (static_x, replay, handle)
            return static_x, replay

        def graph_replay(handle):
            launch = L.lib.gmvae_train_graph_launch
            gen = self._graph_gen

            def replay():
                self._check_alive(gen)
                rc2 = launch(handle, L.current_stream())
                if rc2:
                    L.check(rc2, "gmvae_train_graph_launch")
                self.global_step += n_steps
            return hand_out(replay, handle)

        def eager_replay(step):
            """The graph's steps one by one (no graph could be captured): an eager step reads slot 0, so row i of every input
            passes through it -- as step(i, y_observed=, mask=)'s arguments, or through the engine-held tensor that every eager
            entry copies there.  Afterwards row 0 and the engine's own current values are what they were."""
            batches = [static_x] if n_steps == 1 else list(static_x.unbind(0))

            def replay():
                saved = {inp: view.clone() for inp, view in rows.items()}
                own = {inp: getattr(self, inp.held).clone() for inp in rows if inp.held}
                recs = []
                for i in range(n_steps):
                    args = {}
                    for inp, r in saved.items():
                        if inp.held:
                            getattr(self, inp.held).copy_(r[i].reshape(own[inp].shape))
                        else:
                            args[inp.arg] = r[i]
                    step(batches[i], **args)
                    tail_log[i].copy_(self.grads[self.P:])
                    if clip:
                        recs.append(self.grad_clip.clone())      # (an eager C-side step writes row 0 itself: rows go in last)
                if recs:
                    records.copy_(torch.stack(recs))
                for inp, r in saved.items():
                    rows[inp][0].copy_(r[0])
                    if inp.held:
                        getattr(self, inp.held).copy_(own[inp])
            return hand_out(replay, None)

        if do_ar and getattr(self, "_comm", None):
            torch.cuda.synchronize()
            handle = C.c_void_p()
            rc = L.lib.gmvae_dp_graph_create(C.byref(d), self.model, L.ptr(static_x), n_steps, L.ptr(self.params), L.ptr(self.m),
                                             L.ptr(self.v), L.ptr(self.grads), L.ptr(ws), self.noise_seed,
                                             L.ptr(self.step_dev), lr, *adam_hp, self._comm, L.ptr(tail_log),
                                             C.byref(handle))
            if self._agree(rc == 0):                # all ranks jointly: the graph, or (below) the eager C-side step
                self.dp_mode = "rccl-in-hipgraph"
                return graph_replay(handle)
            if rc == 0:
                L.lib.gmvae_train_graph_destroy(handle)
            self.step_dev.fill_(self.global_step)   # capture refused somewhere: eager C-side step instead
            self.dp_mode = "rccl-eager-c"
            return eager_replay(lambda x, y_observed=None, mask=None: self.dp_step(x, lr, y_observed, *adam_hp, mask=mask))
        if do_ar:
            from . import parallel
            self.dp_mode = "torch.distributed"

            def step(x, **args):
                self.step(x, use_step_dev=True, **args)
                parallel.all_reduce_flat(self.grads)
                self.adam(lr, *adam_hp, use_step_dev=True)
                self.global_step += 1
            return eager_replay(step)
        torch.cuda.synchronize()
        handle = C.c_void_p()
        rc = L.lib.gmvae_train_graph_create(C.byref(d), self.model, L.ptr(static_x), n_steps, L.ptr(self.params), L.ptr(self.m),
                                            L.ptr(self.v), L.ptr(self.grads), L.ptr(ws), self.noise_seed,
                                            L.ptr(self.step_dev), lr, *adam_hp, L.ptr(tail_log), C.byref(handle))
        L.check(rc, "gmvae_train_graph_create")
        return graph_replay(handle)

    BINARIZE_SEED_XOR = 0x62696E6172697A65      # the pipeline graph keys its binarisation uniforms by noise_seed ^ this

    def capture_train_pipeline(self, dataset, B: int, lr: float = 1e-3, n_steps: int = 16,
                               beta1: float = 0.9, beta2: float = 0.999, epsilon: float = 1e-8):
        """A train graph that starts from the RAW pixels (gmvae_train_graph_create_pipeline): each of its n_steps
        steps first binarises its own batch on the device (scripts/runners.py:44-47), rows taken from `dataset`
        (gmvae_amd.data.DeviceDataset: resident uint8 pixels + an epoch permutation on the device).  Returns
        replay(): refills the row indices (device-to-device) and launches the graph; nothing crosses PCIe."""
        for inp in STEP_INPUTS:
            if getattr(self, inp.option):
                raise ValueError("capture_train_pipeline gathers its batches by index inside the graph and has no label gather, "
                                 f"nor one for weight rows, temperatures or masks: an engine with {inp.option}=True trains "
                                 f"through capture_train_step (replay.{inp.replay})")
        if self.likelihood != "bernoulli":
            raise ValueError(f"capture_train_pipeline binarises its batches inside the graph: an engine with "
                             f"likelihood={self.likelihood!r} trains through capture_train_step on grey batches")
        n_steps = int(n_steps)
        clip = self.clip_norm is not None
        if clip and n_steps > L.LABEL_SLOTS:
            raise ValueError(f"a train graph of an engine with clip_norm holds at most {L.LABEL_SLOTS} steps (one clip record "
                             f"per step), got {n_steps}")
        key = ("pipeline", id(dataset), B, lr, n_steps, float(beta1), float(beta2), float(epsilon), clip)
        if key in self._graphs:
            self.step_dev.fill_(self.global_step)
            return self._graphs[key][1]
        if dataset.D != self.D:
            raise ValueError("dataset rows must have D pixels")
        d, ws = self._workspace(B)
        idx = torch.zeros(n_steps, B, dtype=torch.int32, device=self.device)
        xs = torch.zeros(n_steps, B, self.D, dtype=torch.uint8, device=self.device)
        tail_log = torch.zeros(n_steps, L.TAIL, dtype=torch.float32, device=self.device)
        self.step_dev.fill_(self.global_step)
        torch.cuda.synchronize()
        handle = C.c_void_p()
        rc = L.lib.gmvae_train_graph_create_pipeline(C.byref(d), self.model, L.ptr(dataset.pixels), dataset.N, L.ptr(idx),
                                                     L.ptr(xs), n_steps, L.ptr(self.params), L.ptr(self.m), L.ptr(self.v),
                                                     L.ptr(self.grads), L.ptr(ws), self.noise_seed, L.ptr(self.step_dev), lr,
                                                     beta1, beta2, epsilon, L.ptr(tail_log), C.byref(handle))
        L.check(rc, "gmvae_train_graph_create_pipeline")
        launch = L.lib.gmvae_train_graph_launch
        gen = self._graph_gen

        def replay():
            self._check_alive(gen)
            idx.copy_(dataset.next_rows(n_steps * B).view(n_steps, B))
            rc2 = launch(handle, L.current_stream())
            if rc2:
                L.check(rc2, "gmvae_train_graph_launch")
            self.global_step += n_steps

        replay.rows, replay.batches, replay.tail_log = idx, xs, tail_log   # the buffers of the last launch (tests, summaries)
        replay.grad_clip = self._clip_records(d, ws)[:n_steps] if clip else None
        self._graphs[key] = (xs, replay, handle)
        return replay

    def _check_alive(self, gen: int):
        self._param_epoch += 1                  # (every train-graph replay passes here: its kernels write the parameters)
        if gen != self._graph_gen:
            raise L.GmvaeError("this replay closure belongs to a train graph that drop_graphs() destroyed; capture again")

    def _sync_word(self, key, ws):
        off = C.c_uint64()
        d = self.dims(key[0], key[1])
        if L.lib.gmvae_workspace_offset(C.byref(d), self.model, b"sync", C.byref(off)) != 0:
            return None
        return ws.view(torch.int32)[off.value // 4 + 1:off.value // 4 + 2]

    def handoff_timeouts(self) -> int:
        """Number of workspaces whose in-launch hand-off (mega_fwd_bwd's tagged-granule exchange between the
        workgroups of a panel) ever gave up waiting.  Such a step poisons its loss and gradients with NaN and the
        optimizer skips it (params, m, v untouched); this is the explicit flag.  0 on a healthy device."""
        bad = 0
        for key, ws in self._ws.items():
            w = self._sync_word(key, ws)
            if w is not None:
                bad += int(w.item() != 0)
        return bad

    def inject_handoff_fault(self):
        """Test / diagnostics hook: set the hand-off error word of every workspace, exactly what a timed-out wait of the
        fused schedule leaves behind (a co-tenant or a partitioned device kept part of a panel's workgroups off the chip)."""
        for key, ws in self._ws.items():
            w = self._sync_word(key, ws)
            if w is not None:
                w.fill_(1)

    def use_safe_schedule(self):
        """Switch THIS ENGINE to the schedules WITHOUT mutual waits between workgroups (first layer as its own launch, one
        workgroup per panel: GmvaeDims.sched_flags = GMVAE_SCHED_SAFE on every call from now on -- no process-wide state),
        destroy the captured graphs and clear the error words.  Slower (4 launches per step instead of 2), never stalling:
        what run_train and bench.py degrade to when a hand-off of the fused schedule timed out."""
        self.safe_schedule = True
        self.drop_graphs(clear_handoff_errors=True)

    def drop_graphs(self, clear_handoff_errors: bool = True):
        """Destroy every captured train graph (they are re-captured on the next capture_* call, under whatever
        GMVAE_* schedule switches are set by then; replay closures handed out before raise from now on) and,
        optionally, clear the workspaces' hand-off error words."""
        for _, _, handle in self._graphs.values():
            if handle:
                L.lib.gmvae_train_graph_destroy(handle)
        self._graphs.clear()
        self._graph_gen += 1
        if clear_handoff_errors:
            for key, ws in self._ws.items():
                w = self._sync_word(key, ws)
                if w is not None:
                    w.zero_()

    def __del__(self):
        try:
            for _, _, handle in self._graphs.values():
                if handle:
                    L.lib.gmvae_train_graph_destroy(handle)
            self._graphs.clear()
            self._graph_gen += 1
        except Exception:
            pass

    def profile_train_levels(self, x, lr: float = 1e-3, iters: int = 20):
        """Per-launch timing of the steady-state training step of a train graph (gmvae_train_profile): a list of
        (name, in-kernel span us, algorithmic FLOPs, timeline share us).  The timeline share runs from the launch's first
        workgroup start to the next launch's (dispatch + end-of-kernel write-back included: what rocprofv3 reports); the
        shares add up to the step.  Advances the optimizer by 3 * iters steps."""
        x = self._prep_x(x)
        d, ws = self._workspace(x.shape[0])
        self._param_epoch += 1
        self.step_dev.fill_(self.global_step)
        n = C.c_int()
        names = C.create_string_buffer(96 * 48)
        usec = (C.c_float * 96)()
        usec_tl = (C.c_float * 96)()
        flops = (C.c_double * 96)()
        rc = L.lib.gmvae_train_profile(C.byref(d), self.model, L.ptr(x), L.ptr(self.params), L.ptr(self.m), L.ptr(self.v),
                                       L.ptr(self.grads), L.ptr(ws), self.noise_seed, L.ptr(self.step_dev), lr, iters, 96,
                                       C.byref(n), names, usec, usec_tl, flops, L.current_stream())
        L.check(rc, "gmvae_train_profile")
        self.global_step += 3 * iters
        out = []
        for i in range(n.value):
            nm = names.raw[i * 48:(i + 1) * 48].split(b"\0")[0].decode()
            out.append((nm, float(usec[i]), float(flops[i]), float(usec_tl[i])))
        return out

    def profile_forward(self, x, n_samples: Optional[int] = None, iters: int = 20):
        """gmvae_forward_profile: the forward-only evaluation (in-kernel Philox noise) at n_samples importance samples.
        Returns ([(launch, usec, flops)], usec per forward of a replayed hipGraph, the pass's [TAIL] loss sums)."""
        x = self._prep_x(x)
        S = self.S if n_samples is None else int(n_samples)
        d, ws = self._workspace(x.shape[0], S)
        tail = torch.empty(L.TAIL, dtype=torch.float32, device=self.device)
        n = C.c_int(0)
        names = C.create_string_buffer(96 * 48)
        usec = (C.c_float * 96)()
        flops = (C.c_double * 96)()
        total = C.c_float(0)
        rc = L.lib.gmvae_forward_profile(C.byref(d), self.model, L.ptr(x), L.ptr(self.params), L.ptr(tail), L.ptr(ws),
                                         self.noise_seed, iters, 96, C.byref(n), names, usec, flops, C.byref(total),
                                         L.current_stream())
        L.check(rc, "gmvae_forward_profile")
        lev = [(names.raw[i * 48:(i + 1) * 48].split(b"\0")[0].decode(), usec[i], flops[i]) for i in range(n.value)]
        return lev, total.value, tail

    def profile_dp_step(self, x, lr: float = 1e-3, iters: int = 10):
        """gmvae_dp_profile: the data-parallel step's timeline with this engine's RCCL communicator (enable_rccl first; a
        one-rank communicator is allowed).  COLLECTIVE: every rank calls it with the same `iters`.  Returns a dict of
        microseconds: grad_span, allreduce_window, adam_span, gap_to_next_step, step; and the gradient launches' names."""
        if not getattr(self, "_comm", None):
            raise L.GmvaeError("profile_dp_step needs enable_rccl()")
        x = self._prep_x(x)
        d, ws = self._workspace(x.shape[0])
        self._param_epoch += 1
        out = (C.c_float * 8)()
        n = C.c_int(0)
        names = C.create_string_buffer(16 * 48)
        rc = L.lib.gmvae_dp_profile(C.byref(d), self.model, L.ptr(x), L.ptr(self.params), L.ptr(self.m), L.ptr(self.v),
                                    L.ptr(self.grads), L.ptr(ws), self.noise_seed, L.ptr(self.step_dev), lr, self._comm, iters,
                                    out, 16, C.byref(n), names, L.current_stream())
        L.check(rc, "gmvae_dp_profile")
        self.global_step = int(self.step_dev[0].item())
        return {"grad_span": out[0], "allreduce_window": out[1], "adam_span": out[2], "gap_to_next_step": out[3], "step": out[4],
                "grad_launches": [names.raw[i * 48:(i + 1) * 48].split(b"\0")[0].decode() for i in range(n.value)]}

    def profile_levels(self, x, iters: int = 20):
        """Per-launch timing of the step with hipEvents (gmvae_step_profile)."""
        x = self._prep_x(x)
        d, ws = self._workspace(x.shape[0])
        n = C.c_int()
        names = C.create_string_buffer(96 * 48)
        usec = (C.c_float * 96)()
        flops = (C.c_double * 96)()
        rc = L.lib.gmvae_step_profile(C.byref(d), self.model, L.ptr(x), None, None, L.ptr(self.params),
                                      L.ptr(self.grads), L.ptr(ws), self.noise_seed, iters, 96, C.byref(n), names,
                                      usec, flops, L.current_stream())
        L.check(rc, "gmvae_step_profile")
        out = []
        for i in range(n.value):
            nm = names.raw[i * 48:(i + 1) * 48].split(b"\0")[0].decode()
            out.append((nm, float(usec[i]), float(flops[i])))
        return out

    def profile_skinny_levels(self, x, lr: float = 1e-3, n_steps: int = 8, launches: int = 60):
        """Per-launch durations of the skinny schedule (csrc/skinny.hpp) inside a replayed train graph, from the device
        wall-clock stamps its kernels leave (gmvae_debug_sk_stamps): [(name, in-kernel span us, None, timeline share us)],
        the share running from the launch's first workgroup start to the next launch's (the last launch: to the next step's
        first).  Returns None when the configuration does not take that schedule.  Advances training by the replayed steps."""
        import numpy as np
        if L.lib.gmvae_debug_sk_stamps(None) != 0:
            return None
        x = self._prep_x(x)
        B = x.shape[0]
        self.drop_graphs(clear_handoff_errors=False)              # graphs captured before the buffer existed do not stamp
        sx, replay = self.capture_train_step(B, lr=lr, n_steps=n_steps)
        sx.copy_(x.unsqueeze(0).expand(n_steps, -1, -1) if n_steps > 1 else x)
        for _ in range(launches):
            replay()
        torch.cuda.synchronize()
        buf = np.zeros(10 * 1024 * 8, np.uint64)
        L.check(L.lib.gmvae_debug_sk_stamps(buf.ctypes.data_as(C.c_void_p)), "gmvae_debug_sk_stamps")
        st = buf.reshape(10, 1024, 8).astype(np.float64)
        names = ["sk_first_layers", "sk_y_path", "sk_q_head_z", "sk_dec_hidden", "sk_dec_bernoulli", "sk_bwd_dhd", "sk_bwd_dz_heads",
                 "sk_bwd_dhg", "sk_y_path_bwd", "sk_dw_adam"]
        order = list(range(10))
        if self.model == L.MODEL_IDS["vae_gmp"]:                   # the mixture prior's launch stamps the (free) slot of the y
            names[8] = "sk_gmp_bwd"                                #  path's reverse and runs behind B2
            order = [0, 1, 2, 3, 4, 5, 6, 8, 7, 9]
        starts, ends, present = [], [], []
        for i in order:
            r = st[i][st[i][:, 0] > 0]
            if not len(r):
                continue                                           # (the VAE has no y path: slots 1 and 8 stay empty)
            present.append(names[i])
            starts.append(r[:, 0].min())
            ends.append(r[:, 3].max())
        n = len(present)
        self.drop_graphs(clear_handoff_errors=False)              # the stamped graphs hold the buffer's address: destroy them,
        L.check(L.lib.gmvae_debug_sk_stamps_free(), "gmvae_debug_sk_stamps_free")      # then disarm (later steps do not stamp)
        if n < 8 or not all(starts[i + 1] > starts[i] for i in range(n - 1)):
            return None                                            # (stamps of different steps: a launch was mid-flight)
        out = []
        for i in range(n):
            share = (starts[i + 1] - starts[i]) * 0.01 if i < n - 1 else None
            out.append([present[i], (ends[i] - starts[i]) * 0.01, None, share])
        return out
