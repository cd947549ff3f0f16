"""Training / evaluation loops (mirror of scripts/runners.py, plumbing only).

`create_dataset`, `create_model`, `run_train`, `run_eval` keep the reference's names
(scripts/runners.py:21,65,106,235).  What is NOT reproduced: TensorBoard summaries,
image tiles and matplotlib plots (visualisation, out of scope -- DESIGN.md 6); the t-SNE embedding those plots show is
computed (run_eval --embed_latent, tsne.py).
"""
from __future__ import annotations

import glob
import gzip
import math
import os
import time
from typing import Iterator, Tuple

import numpy as np
import torch

from . import gmvae, linprobe, mixfit, neighbours, parallel, pca, tsne, twosample, utils, vae


# ------------------------------------------------------------------ data
def _load_mnist(root: str, split: str):
    """Local MNIST only (no network here): <root>/mnist.npz (keys x_train,y_train,x_test,y_test) or IDX files."""
    npz = os.path.join(root, "mnist.npz")
    if os.path.exists(npz):
        z = np.load(npz)
        return z[f"x_{split}"].reshape(-1, 784), z[f"y_{split}"].astype(np.int64)
    pre = "train" if split == "train" else "t10k"
    imgs = glob.glob(os.path.join(root, f"{pre}-images*"))
    labs = glob.glob(os.path.join(root, f"{pre}-labels*"))
    if imgs and labs:
        op = gzip.open if imgs[0].endswith(".gz") else open
        with op(imgs[0], "rb") as f:
            x = np.frombuffer(f.read(), np.uint8, offset=16).reshape(-1, 784)
        with op(labs[0], "rb") as f:
            y = np.frombuffer(f.read(), np.uint8, offset=8).astype(np.int64)
        return x, y
    return None


def create_dataset(config, split="train", shuffle=True, repeat=True, device="cuda", with_index=False, standardize=None):
    """Yields (images bool/uint8 [B,784] on device, labels int64 [B]) -- the output contract of
    scripts/runners.py:21-62.  Dynamic binarisation keeps the reference's INVERTED rule
    `image < U(0,1)` (runners.py:44-47: P(pixel=1) = 1 - intensity) and is redrawn every epoch;
    examples are shuffled per epoch (the reference's batch-level shuffle order is not copied).
    The last partial batch is kept (no drop_remainder, runners.py:51).  Without local MNIST files
    (--data_dir) a synthetic Bernoulli(0.87) set with random labels stands in.  with_index: yields a third item, the index in
    the split of the batch's first example (its rows follow in order when shuffle=False).  --real_valued: float32 rows as
    they are (real_rows; standardize = the checkpoint's (mean, std))."""
    if real_valued(config):
        return _real_batches(config, shuffle, repeat, device, with_index, standardize)
    data = _load_mnist(getattr(config, "data_dir", "") or "", split) if getattr(config, "data_dir", None) else None
    rank, world = (parallel.dist.get_rank(), parallel.dist.get_world_size()) if parallel.dist.is_initialized() else (0, 1)
    gen = torch.Generator(device=device)
    gen.manual_seed((config.random_seed or 0) * 7919 + 17 + rank)
    grey = None                                                    # --likelihood on grey levels: the uint8 rows as they are
    if data is None:
        n = int(getattr(config, "synthetic_size", 8192))
        D = int(getattr(config, "data_dim", 784))
        inten = torch.full((n, D), 0.13, device=device)            # 1 - 0.87: P(1) = 0.87 after inversion
        labels = torch.randint(0, 10, (n,), generator=torch.Generator().manual_seed(3)).to(device)
        if grey_levels(config):
            grey = torch.from_numpy(synthetic_grey(n, D)).to(device)
    else:
        inten = torch.from_numpy(np.ascontiguousarray(data[0])).to(device).float() / 255.0
        labels = torch.from_numpy(data[1]).to(device)
        if grey_levels(config):
            grey = torch.from_numpy(np.ascontiguousarray(data[0])).to(device).reshape(inten.shape[0], -1)
    a, b = parallel.shard_rows(inten.shape[0], rank, world)
    inten, labels = inten[a:b], labels[a:b]
    grey = None if grey is None else grey[a:b]
    n = inten.shape[0]
    B = int(config.batch_size)

    def it() -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        while True:
            order = torch.randperm(n, device=device, generator=gen) if shuffle else torch.arange(n, device=device)
            binar = grey if grey is not None else (inten < torch.rand(inten.shape, device=device, generator=gen)).to(torch.uint8)
            for s in range(0, n, B):
                idx = order[s:s + B]
                yield (binar[idx], labels[idx], a + s) if with_index else (binar[idx], labels[idx])
            if not repeat:
                return
    return it()


def real_valued(config) -> bool:
    """--real_valued: the rows are float feature vectors fed as they are (Engine(real_valued=True))."""
    return bool(getattr(config, "real_valued", False)) or count_data(config)


def npy_shape(path: str):
    """The shape of the array in a .npy file, from its header."""
    return tuple(np.load(path, mmap_mode="r").shape)


def synthetic_real(n: int, D: int):
    """The synthetic stand-in of a real-valued run: (float32 [n, D], int64 labels [n]) -- a fixed-seed mixture of 10
    well-separated Gaussian blobs (centres drawn at scale 3, noise of 0.2 .. 0.6 per feature), so that clustering accuracy
    means something; train and eval see the same rows."""
    rng = np.random.default_rng(6)
    k = 10
    centres = rng.normal(0.0, 3.0, (k, D))
    noise = rng.uniform(0.2, 0.6, D)
    lab = rng.integers(0, k, n)
    x = centres[lab] + rng.normal(0.0, 1.0, (n, D)) * noise[None, :]
    return x.astype(np.float32), lab.astype(np.int64)


def count_data(config) -> bool:
    """--likelihood=poisson | negative_binomial: the rows are counts (Engine(likelihood=...); float rows are implied)."""
    return getattr(config, "likelihood", "bernoulli") in ("poisson", "negative_binomial")


def synthetic_counts(n: int, D: int, k: int = 3, seed: int = 7):
    """The synthetic stand-in of a count run: (float32 [n, D] counts, int64 labels [n]) -- a fixed-seed K-cluster gamma-Poisson
    mixture.  Each cluster has its own log-normal mean profile over the features (a tenth of them raised tenfold, so that the
    clusters differ where it matters), each feature its own inverse dispersion r in [0.5, 4]; a row draws its rates from
    Gamma(r, r / mean) and its counts from Poisson(rate): over-dispersed and zero-heavy, like an expression matrix."""
    rng = np.random.default_rng(seed)
    base = np.exp(rng.normal(0.0, 1.0, (1, D)))
    prof = base * np.exp(rng.normal(0.0, 0.5, (k, D)))
    prof = prof * np.where(rng.random((k, D)) < 0.1, 10.0, 1.0)
    r = rng.uniform(0.5, 4.0, D)
    lab = rng.integers(0, k, n)
    mean = prof[lab]
    rate = rng.gamma(np.broadcast_to(r, mean.shape), mean / r)
    return rng.poisson(rate).astype(np.float32), lab.astype(np.int64)


def check_counts(x: np.ndarray) -> np.ndarray:
    """Count rows are finite and >= 0: checked once, on the host, where the rows are loaded."""
    if not np.isfinite(x).all():
        raise ValueError("count data must be finite: the rows hold NaN or inf")
    if (x < 0).any():
        raise ValueError("count data must be >= 0: the rows hold negative values")
    return x


def real_rows(config):
    """--real_valued: (float32 [N, D] rows, int64 [N] labels) from --data_npy / --labels_npy (labels 0 without the second
    file), or synthetic_real(--synthetic_size, --data_dim)."""
    path = getattr(config, "data_npy", None)
    if not path and count_data(config):
        return synthetic_counts(int(getattr(config, "synthetic_size", 8192)), int(getattr(config, "data_dim", 784)),
                                max(int(getattr(config, "mixture_components", 3) or 3), 1))
    if not path:
        return synthetic_real(int(getattr(config, "synthetic_size", 8192)), int(getattr(config, "data_dim", 784)))
    x = np.ascontiguousarray(np.load(path), dtype=np.float32)
    if x.ndim != 2:
        raise ValueError(f"--data_npy must hold a float32 [N, D] array, got shape {x.shape}")
    lp = getattr(config, "labels_npy", None)
    lab = np.asarray(np.load(lp)).astype(np.int64).reshape(-1) if lp else np.zeros(x.shape[0], np.int64)
    if lab.shape[0] != x.shape[0]:
        raise ValueError(f"--labels_npy holds {lab.shape[0]} labels for {x.shape[0]} rows")
    if count_data(config):
        check_counts(x)
    return x, lab


def standardize_stats(x: np.ndarray):
    """--standardize: the per-feature (mean, std) of the rows as float32 tensors [D]; a constant feature keeps std 1."""
    mean, std = x.mean(axis=0, dtype=np.float64), x.std(axis=0, dtype=np.float64)
    std[std == 0] = 1.0
    return torch.from_numpy(mean.astype(np.float32)), torch.from_numpy(std.astype(np.float32))


def _standardized(x: np.ndarray, stats) -> np.ndarray:
    return x if stats is None else ((x - stats[0].numpy()[None, :]) / stats[1].numpy()[None, :]).astype(np.float32)


def _real_batches(config, shuffle, repeat, device, with_index, stats):
    x, lab = real_rows(config)
    rank, world = (parallel.dist.get_rank(), parallel.dist.get_world_size()) if parallel.dist.is_initialized() else (0, 1)
    a, b = parallel.shard_rows(x.shape[0], rank, world)
    xt = torch.from_numpy(_standardized(x, stats)[a:b]).to(device)
    labels = torch.from_numpy(lab[a:b]).to(device)
    gen = torch.Generator(device=device)
    gen.manual_seed((config.random_seed or 0) * 7919 + 17 + rank)
    n, B = xt.shape[0], int(config.batch_size)

    def it():
        while True:
            order = torch.randperm(n, device=device, generator=gen) if shuffle else torch.arange(n, device=device)
            for s in range(0, n, B):
                idx = order[s:s + B]
                yield (xt[idx], labels[idx], a + s) if with_index else (xt[idx], labels[idx])
            if not repeat:
                return
    return it()


# ----------------------------------------------------------------- model
def kl_warmup(t: int, n: int) -> float:
    """--kl_warmup_steps N: the factor on both KL weights during the step with 0-based index t -- min(1, (t + 1) / N), 1 for
    N <= 0.  A pure function of the global step, so a restored checkpoint continues the schedule."""
    return 1.0 if n <= 0 else min(1.0, (int(t) + 1) / float(n))


def weighted_flags(config) -> bool:
    """Whether any of --kl_weight / --y_weight / --y_free_nats / --kl_warmup_steps leaves its default: the engine is then
    created with the weighted objective (Engine(weighted_objective=True))."""
    return (float(getattr(config, "kl_weight", 1.0)) != 1.0 or float(getattr(config, "y_weight", 1.0)) != 1.0 or
            float(getattr(config, "y_free_nats", 0.0)) != 0.0 or int(getattr(config, "kl_warmup_steps", 0) or 0) != 0)


def objective_weights_at(config, t: int):
    """(kl_weight, y_weight, y_free_nats) of the step with 0-based index t: the flags under the warm-up factor."""
    f = kl_warmup(t, int(getattr(config, "kl_warmup_steps", 0) or 0))
    return (float(getattr(config, "kl_weight", 1.0)) * f, float(getattr(config, "y_weight", 1.0)) * f,
            float(getattr(config, "y_free_nats", 0.0)))


def temperature_flags(config) -> bool:
    """Whether any of --temperature / --temperature_min / --temperature_anneal_rate / --temperature_anneal_every leaves its
    default: training then creates the engine with the temperature on the device (Engine(temperature_on_device=True))."""
    return (float(getattr(config, "temperature", 1.0)) != 1.0 or float(getattr(config, "temperature_min", 0.0)) != 0.0 or
            float(getattr(config, "temperature_anneal_rate", 0.0)) != 0.0 or
            int(getattr(config, "temperature_anneal_every", 0) or 0) != 0)


def temperature_at(config, t: int) -> float:
    """The Gumbel-softmax temperature of the step with 0-based index t: max(tau_min, tau_0 exp(-r N floor(t / N))) with
    tau_0 = --temperature, tau_min = --temperature_min, r = --temperature_anneal_rate, N = --temperature_anneal_every (Jang
    et al. 2017: the temperature is updated every N steps); N <= 0: no annealing, max(tau_min, tau_0).  A pure function of the
    global step, so a restored checkpoint continues the schedule."""
    t0, tmin = float(getattr(config, "temperature", 1.0)), float(getattr(config, "temperature_min", 0.0))
    r, n = float(getattr(config, "temperature_anneal_rate", 0.0)), int(getattr(config, "temperature_anneal_every", 0) or 0)
    if n <= 0:
        return max(tmin, t0)
    return max(tmin, t0 * math.exp(-r * n * (int(t) // n)))


def missing_mask(config, split: str, n_rows: int, data_dim: int):
    """--missing_rate p: the observation mask of a split, uint8 [n_rows, data_dim] (1 = observed), or None for p = 0.  ONE
    fixed mask per dataset row, each pixel missing independently with probability p, drawn once from --missing_seed and the
    split's name over the WHOLE split (before any rank's shard is cut): training and evaluation see the same mask for a row."""
    p = float(getattr(config, "missing_rate", 0.0) or 0.0)
    if p <= 0.0:
        return None
    rng = np.random.default_rng([int(getattr(config, "missing_seed", 0) or 0), 0 if split == "train" else 1])
    return (rng.random((int(n_rows), int(data_dim)), dtype=np.float32) >= p).astype(np.uint8)


def likelihood_of(config):
    """--likelihood / --likelihood_sigma: (Engine's likelihood, its sigma)."""
    return getattr(config, "likelihood", "bernoulli") or "bernoulli", float(getattr(config, "likelihood_sigma", 1.0) or 1.0)


def grey_levels(config) -> bool:
    """The model reads grey levels t = pixel / 255 (--likelihood other than bernoulli): no binarisation anywhere."""
    return likelihood_of(config)[0] != "bernoulli"


def synthetic_grey(n: int, D: int) -> np.ndarray:
    """The synthetic stand-in of a grey-level run: uint8 [n, D], a smooth ramp per row plus noise, about a third of the pixels
    exactly 0 (train and eval see the same rows)."""
    rng = np.random.default_rng(4)
    ramp = np.linspace(0.0, 1.0, D)[None, :] * rng.uniform(0.3, 1.0, (n, 1))
    pix = np.clip(ramp + rng.normal(0.0, 0.05, (n, D)), 0.0, 1.0)
    pix[rng.random((n, D)) < 0.3] = 0.0
    return np.round(pix * 255.0).astype(np.uint8)


def clip_norm_of(config):
    """--clip_norm C: Engine's clip_norm -- None for 0 (off), else the threshold (inf: report only)."""
    c = float(getattr(config, "clip_norm", 0.0) or 0.0)
    return c if c > 0.0 else None


def create_model(config, data_dim, weighted=None, temperature_on_device=None, clip=None):
    """scripts/runners.py:65-103: binds the flags and FIXES sigma_min=0.0, raw_sigma_bias=0.5 (and temperature=1.0 unless
    --temperature says otherwise).
    weighted: create the engine with the weighted objective (None: as the flags say; run_eval passes False, so that its
    numbers stay comparable).  temperature_on_device: likewise for the temperature flags (run_eval passes False: it sets one
    temperature, which travels in the dims).  clip: likewise for --clip_norm (run_eval passes False: it runs no optimizer)."""
    pclip = dict(clip_norm=clip_norm_of(config) if clip is None or clip else None)
    wobj = dict(weighted_objective=weighted_flags(config) if weighted is None else bool(weighted))
    yhead = dict(temperature_on_device=temperature_flags(config) if temperature_on_device is None else bool(temperature_on_device),
                 y_estimator=getattr(config, "y_estimator", "relaxed"))
    pmask = dict(pixel_mask=float(getattr(config, "missing_rate", 0.0) or 0.0) > 0.0)      # (--missing_rate: train AND eval)
    pmask.update(likelihood=likelihood_of(config)[0], likelihood_sigma=likelihood_of(config)[1])      # (--likelihood: likewise)
    pmask.update(real_valued=real_valued(config), likelihood_scale=getattr(config, "likelihood_scale", "fixed") or "fixed")
    hidden = [config.hidden_size] * config.num_layers
    ns = int(getattr(config, "n_samples", 1))
    ge = getattr(config, "grad_estimator", "standard")
    lpc = int(getattr(config, "labelled_per_class", 0) or 0)
    if lpc > 0 and config.model != "gmvae":
        raise ValueError("--labelled_per_class trains the GMVAE semi-supervised: it needs --model=gmvae")
    if config.model == "gmvae":
        return gmvae.create_gmvae(data_dim, config.latent_size, mixture_components=config.mixture_components,
                                  fcnet_hidden_sizes=hidden, sigma_min=0.0, raw_sigma_bias=0.5,
                                  temperature=temperature_at(config, 0), random_seed=config.random_seed, n_samples=ns,
                                  y_inference=getattr(config, "y_inference", "gumbel"), grad_estimator=ge,
                                  semi_supervised=lpc > 0, sup_weight=float(getattr(config, "sup_weight", 1.0)), **wobj, **yhead, **pmask, **pclip)
    if temperature_flags(config) or yhead["y_estimator"] != "relaxed":
        raise ValueError("--temperature* and --y_estimator belong to the GMVAE's Gumbel-softmax draw: they need --model=gmvae")
    if config.model == "vae_gmp":
        return vae.create_vae(data_dim, config.latent_size, mixture_components=config.mixture_components,
                              fcnet_hidden_sizes=hidden, sigma_min=0.0, raw_sigma_bias=0.5,
                              random_seed=config.random_seed, n_samples=ns, grad_estimator=ge, **wobj, **pmask, **pclip)
    if config.model == "vae":
        return vae.create_vae(data_dim, config.latent_size, fcnet_hidden_sizes=hidden, sigma_min=0.0,
                              raw_sigma_bias=0.5, random_seed=config.random_seed, n_samples=ns, grad_estimator=ge, **wobj, **pmask, **pclip)
    raise ValueError(f"unknown model {config.model!r}")


def select_device(config, local_rank: int) -> int:
    """The device of this process.  Under a launcher (LOCAL_RANK set: one process per GPU) it is the local rank.
    Otherwise the reference's flags decide (scripts/run_gmvae.py:45-48, scripts/runners.py:193,209): `--gpu_num` is the
    comma-separated list of visible physical devices (gpu_options.visible_device_list) and `--gpu_id` indexes INTO that
    list (tf.device('/gpu:<gpu_id>'))."""
    if "LOCAL_RANK" in os.environ:
        return int(local_rank)
    visible = [int(t) for t in str(getattr(config, "gpu_num", "0") or "0").split(",") if t.strip() != ""] or [0]
    idx = int(getattr(config, "gpu_id", "0") or 0)
    if not 0 <= idx < len(visible):
        raise ValueError(f"--gpu_id={idx} does not index the visible device list --gpu_num={visible}")
    dev = visible[idx]
    if not 0 <= dev < torch.cuda.device_count():
        raise ValueError(f"--gpu_num names device {dev}, but this host has {torch.cuda.device_count()} GPU(s)")
    return dev


def _logdir(config):
    """<logdir>/<model>/h<hidden>_n<layers>_z<latent> (scripts/runners.py:212-217)."""
    return os.path.join(config.logdir, config.model,
                        f"h{config.hidden_size}_n{config.num_layers}_z{config.latent_size}")


def _ckpt(config):
    return os.path.join(_logdir(config), "model.pt")


def _save_checkpoint(model, path: str):
    """Atomic: a reader (run_eval's wait_for_checkpoint, a restart) never sees a half-written file.  The metadata records the
    likelihood the parameters were trained under (the tensors have the same names and shapes under every one)."""
    tmp = path + ".tmp"
    sd = model.state_dict()
    sd["likelihood"] = model._engine.likelihood
    sd["likelihood_sigma"] = torch.tensor(model._engine.likelihood_sigma, dtype=torch.float64)
    sd["real_valued"], sd["likelihood_scale"] = model._engine.real_valued, model._engine.likelihood_scale
    if getattr(model, "standardize", None) is not None:      # (--standardize: the train rows' per-feature mean and std)
        sd["standardize_mean"], sd["standardize_std"] = model.standardize
    torch.save(sd, tmp)
    os.replace(tmp, path)


def _restore_checkpoint(model, path: str):
    """load_state_dict from the file -- an error if it was written under another likelihood (or another sigma of the
    Gaussian): the parameters would load, and mean something else.  A file without the metadata is a Bernoulli one."""
    sd = torch.load(path, map_location="cpu")
    eng = model._engine
    lik, sigma = sd.pop("likelihood", "bernoulli"), float(sd.pop("likelihood_sigma", eng.likelihood_sigma))
    if lik != eng.likelihood or (lik == "gaussian" and sigma != eng.likelihood_sigma):
        raise ValueError(f"{path} was trained with --likelihood={lik}" + (f" --likelihood_sigma={sigma:g}" if lik == "gaussian" else "")
                         + f": it cannot be restored under --likelihood={eng.likelihood}"
                         + (f" --likelihood_sigma={eng.likelihood_sigma:g}" if eng.likelihood == "gaussian" else ""))
    real, scale = bool(sd.pop("real_valued", False)), sd.pop("likelihood_scale", "fixed")
    if real != eng.real_valued or scale != eng.likelihood_scale:
        raise ValueError(f"{path} was trained with{'' if real else 'out'} --real_valued and --likelihood_scale={scale}: it cannot "
                         f"be restored with{'' if eng.real_valued else 'out'} --real_valued and --likelihood_scale={eng.likelihood_scale}")
    mean, std = sd.pop("standardize_mean", None), sd.pop("standardize_std", None)
    model.standardize = None if mean is None else (mean, std)
    model.load_state_dict(sd)


def wait_for_checkpoint(path: str, poll_seconds: float = 60.0, max_wait: float | None = None) -> str:
    """scripts/utils.py:100-111: loop until a checkpoint exists, sleeping `poll_seconds` (60 s in the reference)
    between looks.  max_wait (build-side addition, None = forever like the reference) bounds the wait."""
    t0 = time.time()
    while not os.path.exists(path):
        if max_wait is not None and time.time() - t0 >= max_wait:
            raise FileNotFoundError(f"no checkpoint at {path} after waiting {max_wait:.0f} s")
        print(f"Checkpoint not found in {os.path.dirname(path)}, sleeping for {poll_seconds:g} seconds.", flush=True)
        time.sleep(poll_seconds)
    return path


def select_labelled(labels, per_class: int, seed: int) -> np.ndarray:
    """--labelled_per_class N: which rows of a split show their label to the semi-supervised objective.  int32 [n]: the label
    where it is observed, -1 elsewhere.  For each class the first N of its rows in ONE permutation of the whole split seeded by
    `seed` (a class with fewer rows shows them all).  The choice looks at the whole split, before any rank's shard is cut, so
    every world size labels the same rows."""
    labels = np.asarray(labels).astype(np.int64).reshape(-1)
    out = np.full(labels.shape[0], -1, dtype=np.int32)
    if per_class <= 0:
        return out
    perm = np.random.default_rng(int(seed)).permutation(labels.shape[0])
    pl = labels[perm]
    for c in np.unique(labels):
        rows = perm[pl == c][:per_class]
        out[rows] = c
    return out


def create_device_dataset(config, split="train", shuffle=True, standardize=None):
    """The input pipeline of scripts/runners.py:21-62 with the raw uint8 pixels resident in HBM (data.DeviceDataset):
    this rank's contiguous shard of the split's rows (+ labels), shuffled per epoch on the device; binarisation happens
    per step on the device (gmvae_binarize: inside the train graph, or as a launch in the eager loop).  Without local
    MNIST files a synthetic set of intensity 33/255 (P[x = 1] = 0.87 after the reference's inverted rule) stands in.
    --real_valued: the float32 rows of real_rows (standardize = the (mean, std) to apply), resident as they are."""
    from .data import DeviceDataset
    if real_valued(config):
        x, lab = real_rows(config)
        rank, world = (parallel.dist.get_rank(), parallel.dist.get_world_size()) if parallel.dist.is_initialized() else (0, 1)
        a, b = parallel.shard_rows(x.shape[0], rank, world)
        return DeviceDataset(_standardized(x, standardize)[a:b], lab[a:b], shuffle=shuffle,
                             seed=(config.random_seed or 0) * 7919 + 17 + rank, binarize=False, counts=count_data(config))
    data = _load_mnist(getattr(config, "data_dir", "") or "", split) if getattr(config, "data_dir", None) else None
    rank, world = (parallel.dist.get_rank(), parallel.dist.get_world_size()) if parallel.dist.is_initialized() else (0, 1)
    if data is None:
        n = int(getattr(config, "synthetic_size", 8192))
        D = int(getattr(config, "data_dim", 784))
        pix = synthetic_grey(n, D) if grey_levels(config) else np.full((n, D), 33, dtype=np.uint8)
        lab = np.random.default_rng(3).integers(0, 10, n)
    else:
        pix, lab = np.ascontiguousarray(data[0]), data[1]
    a, b = parallel.shard_rows(pix.shape[0], rank, world)
    lpc = int(getattr(config, "labelled_per_class", 0) or 0)
    yobs = select_labelled(lab, lpc, config.random_seed or 0)[a:b] if lpc > 0 else None
    pm = missing_mask(config, split, pix.shape[0], pix.shape[1] if pix.ndim == 2 else int(np.prod(pix.shape[1:])))
    return DeviceDataset(pix[a:b], lab[a:b], shuffle=shuffle, seed=(config.random_seed or 0) * 7919 + 17 + rank, y_observed=yobs,
                         pixel_mask=None if pm is None else pm[a:b], binarize=not grey_levels(config))


def _graph_steps(every: int, cap: int = 32) -> int:
    """Steps per graph launch: the largest divisor of summarise_every up to `cap`, so that summaries fall on launch
    boundaries (one host sync per summary, none in between)."""
    return max(g for g in range(1, max(1, min(cap, every)) + 1) if every % g == 0)


def _verify_launch(eng, snap, batches, g, lr):
    """GMVAE_VERIFY_EVERY=n (debug): the g steps a train-graph launch just took, replayed from a snapshot of (params, m, v,
    step) on a SHADOW engine through the two-launch form (GMVAE_NO_FUSE=1: mega2_fwd_bwd -> dw_adam, no plain loads behind flags
    inside a launch) on the same binarised batches and the same noise keys, and compared BIT FOR BIT.  The one-launch steps
    (csrc/mega3.hpp) are correct under the cache behaviour they were verified on (gfx950, ROCm 7.2: INTEGRATION.md); a stale
    line would give silently wrong gradients, not a timeout -- this is the canary for other firmware / partitions."""
    from .engine import Engine
    p0, m0, v0, step0 = snap
    hp = dict(eng.hp)
    gb = eng.gen_bias_vec if eng.gen_bias_vec is not None else hp.pop("gen_bias_init")
    hp.pop("gen_bias_init", None)
    sh = Engine(eng.model_name, eng.D, eng.Lz, eng.K, eng.hidden, n_samples=eng.S, gen_bias_init=gb, random_seed=0,
                y_inference=eng.y_inference, grad_estimator=eng.grad_estimator, semi_supervised=eng.semi_supervised,
                sup_weight=eng.sup_weight, y_estimator=eng.y_estimator, clip_norm=eng.clip_norm, **hp)
    sh.rank, sh.noise_seed = eng.rank, eng.noise_seed
    with torch.no_grad():
        sh.params.copy_(p0); sh.m.copy_(m0); sh.v.copy_(v0)
    sh.global_step = step0
    sh.step_dev.fill_(step0)
    old = os.environ.get("GMVAE_NO_FUSE")
    os.environ["GMVAE_NO_FUSE"] = "1"
    try:
        sx, rp = sh.capture_train_step(batches.shape[-2], lr=lr, n_steps=g)
        sx.copy_(batches if g > 1 else batches.reshape(sx.shape))
        rp()
        torch.cuda.synchronize()
    finally:
        if old is None:
            del os.environ["GMVAE_NO_FUSE"]
        else:
            os.environ["GMVAE_NO_FUSE"] = old
        sh.drop_graphs()
    bad = [nm for nm, a_, b_ in (("params", sh.params, eng.params), ("Adam m", sh.m, eng.m), ("Adam v", sh.v, eng.v))
           if not torch.equal(a_.detach(), b_.detach())]
    if bad:
        d = (sh.params.detach() - eng.params.detach()).abs()
        raise RuntimeError(f"GMVAE_VERIFY_EVERY: steps {step0 + 1}..{step0 + g} of the train graph differ from the two-launch form in "
                           f"{bad} (max |d params| {d.max().item():.3e}, {int((d > 0).sum().item())} elements): the one-launch "
                           f"step's plain loads saw stale data on this device -- run with GMVAE_NO_FUSE=1")


def run_train(config):
    """scripts/runners.py:106-232.  One iteration = the reference's sess.run([train_op, global_step]); here
    `summarise_every`-aligned hipGraph launches of several steps each: binarisation from the resident pixels, Philox
    noise, forward, backward, (RCCL all-reduce,) TF-Adam and the per-step loss log all run on the device, and the host
    looks only at summary steps: the logging hook's line, the early-stopping hook fed with EVERY step's (all-reduced)
    loss from the log (scripts/utils.py:13-57), the checkpoint timer (save_checkpoint_secs=120, runners.py:226).
    `config.eager = True` (or GMVAE_EAGER_TRAIN=1) runs the same batches through eager launches instead."""
    from .data import binarize
    from .engine import STEP_INPUTS, Engine
    rank, world, local = parallel.init_from_env()
    torch.cuda.set_device(select_device(config, local))
    data_dim = int(getattr(config, "data_dim", 784))
    model = create_model(config, data_dim)
    eng = model._engine
    os.makedirs(_logdir(config), exist_ok=True)
    if os.path.exists(_ckpt(config)):                      # MonitoredTrainingSession auto-restore
        _restore_checkpoint(model, _ckpt(config))
        if rank == 0:
            print(f"restored {_ckpt(config)} at step {eng.global_step}")
    eng.sync_replicas()            # default --random_seed=None: every process drew its own init; rank 0's wins
    if real_valued(config) and getattr(config, "standardize", False) and getattr(model, "standardize", None) is None:
        model.standardize = standardize_stats(real_rows(config)[0])      # (a restored checkpoint keeps its own)
    ds = create_device_dataset(config, "train", shuffle=True, standardize=getattr(model, "standardize", None))
    B, lr, every = int(config.batch_size), float(config.learning_rate), int(config.summarise_every)
    eager = bool(getattr(config, "eager", False)) or os.environ.get("GMVAE_EAGER_TRAIN") == "1"
    bseed = eng.noise_seed ^ Engine.BINARIZE_SEED_XOR
    G = _graph_steps(every)
    dp_graph = False
    if world > 1 and not eager and parallel.dist.get_backend() == "nccl":     # (in-library RCCL: one device per rank)
        try:
            eng.enable_rccl()                               # raises on EVERY rank if it fails on any
            dp_graph = True
        except Exception as e:
            if rank == 0:
                print(f"[run_train] in-library RCCL unavailable ({e}); torch.distributed all-reduce", flush=True)
    # per-step inputs (engine.STEP_INPUTS): the pipeline graph has no gather for them, so one device takes the branch that
    # world > 1 takes -- binarise, fill the graph's rows, replay.  Per launch: the label sets (--labelled_per_class) and the masks
    # (--missing_rate) are gathered by the batch's rows; the weight rows (--kl_weight / --y_weight / --y_free_nats /
    # --kl_warmup_steps) and the temperatures (--temperature / --temperature_min / --temperature_anneal_rate /
    # --temperature_anneal_every) are pure functions of the global step
    inputs = eng.step_inputs
    tags = [inp.tag for inp in STEP_INPUTS if inp.option in inputs]
    grey = eng.likelihood != "bernoulli"                    # grey batches are gathered, never binarised: capture_train_step's branch
    if grey:
        tags = tags + ["real" if eng.real_valued else "grey"]
    run_train.last_path = ("eager" if eager else "dp-graph" if world > 1 else f"graph+{tags[0]}" if tags else "pipeline-graph")
    run_train.temperature_log = []                          # temperature on the device: (0-based step index, temperature) of the
                                                            # LAST launch's steps, as placed in replay.y_temperature
    run_train.weight_log = []                               # weighted objective: (step, tail[5] / tail[4], tail[6] / tail[4]) of the
                                                            # LAST summary block's steps (replaced per block: it does not grow)
    verify_every = int(os.environ.get("GMVAE_VERIFY_EVERY", "0") or 0)      # debug canary: see _verify_launch
    run_train.launches = run_train.verified_launches = 0
    run_train.degraded = False
    hook = utils.EarlyStoppingHook(config.early_stop_rounds, config.early_stop_threshold)
    last_save, t0, s0 = time.time(), time.time(), eng.global_step
    logs = []                                               # device tensors [n, TAIL]: no host sync until a summary
    clips = []                                              # --clip_norm: device tensors [n, 4], the steps' clip records
    clip = eng.clip_norm is not None
    run_train.clip_log = []                                 # per summary window: dict(mean, max, clipped_share, skipped_share, steps)
    last_x = last_rows = None

    def run(n):
        """n training steps on the next n batches of the pipeline."""
        nonlocal last_x, last_rows
        while n > 0:
            g = G if n >= G else 1
            if eager:
                rows = ds.next_rows(B)
                x = (ds.pixels[rows.long()] if grey else
                     binarize(ds.pixels, rows=rows, seed=bseed, step=eng.global_step, out_row0=rank * B))
                yo = ds.y_observed[rows.long()] if "semi_supervised" in inputs else None
                if "weighted_objective" in inputs:
                    eng.set_objective_weights(*objective_weights_at(config, eng.global_step))
                if "temperature_on_device" in inputs:
                    run_train.temperature_log = [(eng.global_step, temperature_at(config, eng.global_step))]
                    eng.set_temperature(run_train.temperature_log[0][1])
                mk = ds.pixel_mask[rows.long()] if "pixel_mask" in inputs else None
                logs.append(eng.train_step(x, lr=lr, y_observed=yo, mask=mk).clone().view(1, -1))
                if clip:
                    clips.append(eng.grad_clip.clone().view(1, 4))
                last_x, last_rows, g = x, rows, 1
            elif world == 1 and not inputs and not grey:
                replay = eng.capture_train_pipeline(ds, B, lr=lr, n_steps=g)
                run_train.launches += 1
                snap = None
                if verify_every and run_train.launches % verify_every == 0:
                    snap = (eng.params.detach().clone(), eng.m.clone(), eng.v.clone(), eng.global_step)
                replay()
                if snap is not None:
                    _verify_launch(eng, snap, replay.batches.clone(), g, lr)
                    run_train.verified_launches += 1
                logs.append(replay.tail_log.clone())
                if clip:
                    clips.append(replay.grad_clip.clone())
                last_x, last_rows = replay.batches[g - 1], replay.rows[g - 1]
            else:
                sx, replay = eng.capture_train_step(B, lr=lr, all_reduce=world > 1, n_steps=g)
                xs = sx if g > 1 else sx.unsqueeze(0)
                for i in range(g):                          # this launch's batches, binarised on the device
                    last_rows = ds.next_rows(B)
                    if grey:
                        xs[i].copy_(ds.pixels[last_rows.long()])
                    else:
                        binarize(ds.pixels, rows=last_rows, seed=bseed, step=eng.global_step + i, out=xs[i], out_row0=rank * B)
                    if replay.y_observed is not None:
                        replay.y_observed[i].copy_(ds.y_observed[last_rows.long()])
                    if replay.pixel_mask is not None:
                        replay.pixel_mask[i].copy_(ds.pixel_mask[last_rows.long()])
                if replay.obj_weights is not None:
                    rows_w = torch.tensor([objective_weights_at(config, eng.global_step + i) + (0.0,) for i in range(g)],
                                          dtype=torch.float32)
                    replay.obj_weights.copy_(rows_w, non_blocking=True)
                if replay.y_temperature is not None:
                    run_train.temperature_log = [(eng.global_step + i, temperature_at(config, eng.global_step + i)) for i in range(g)]
                    replay.y_temperature.copy_(torch.tensor([v for _, v in run_train.temperature_log], dtype=torch.float32),
                                               non_blocking=True)
                replay()
                logs.append(replay.tail_log.clone())
                if clip:
                    clips.append(replay.grad_clip.clone())      # (read once per launch, next to tail_log)
                last_x = xs[g - 1]
            n -= g

    stop = False
    while eng.global_step <= config.max_steps and not stop:  # `<=`: the reference runs one extra step (runners.py:231)
        n = min(every - eng.global_step % every, config.max_steps + 1 - eng.global_step)
        run(n)
        tails = torch.cat(logs).cpu()                       # the summary's host sync
        logs = []
        clip_msg = ""
        if clip:
            # the window's clip records: the norm's mean and maximum over the applied steps, the clipped share of those, and the
            # share the optimizer skipped (guard NaN: a gradient or a loss that is not finite, or a threshold that is not > 0)
            recs = torch.cat(clips).cpu().double()
            clips = []
            applied = recs[torch.isfinite(recs[:, 3])]
            win = dict(steps=int(recs.shape[0]), skipped_share=1.0 - applied.shape[0] / max(recs.shape[0], 1),
                       mean=applied[:, 0].mean().item() if len(applied) else float("nan"),
                       max=applied[:, 0].max().item() if len(applied) else float("nan"),
                       clipped_share=applied[:, 2].mean().item() if len(applied) else 0.0)
            run_train.clip_log.append(win)
            clip_msg = (f"  grad_norm mean {win['mean']:.4g} max {win['max']:.4g}  clipped {win['clipped_share']:.3f}"
                        f"  skipped {win['skipped_share']:.3f}")
        vals = (tails[:, 0] / tails[:, 4]).tolist()
        base = eng.global_step - len(vals)
        if "weighted_objective" in inputs:
            run_train.weight_log = [(base + i + 1, (tails[i, 5] / tails[i, 4]).item(), (tails[i, 6] / tails[i, 4]).item())
                                     for i in range(len(vals))]
        fault = getattr(config, "fault_hook", None)         # (tests: called with the engine after every summary block)
        timed_out = bool(eng.handoff_timeouts())            # the explicit flag of a hand-off that gave up waiting
        nonfinite = not all(np.isfinite(vals))
        if world > 1:                                       # every rank takes the same branch (the tails are all-reduced,
            flag = torch.tensor([int(timed_out)], device=eng.device)     # the error word is per device)
            parallel.all_reduce_flat(flag, op=parallel.dist.ReduceOp.MAX)
            timed_out = bool(flag.item())
        if nonfinite and not timed_out:
            # no hand-off gave up: the loss itself left the finite range (divergence, bad input).  Changing the schedule
            # would re-run the same arithmetic; stop here with the last good checkpoint, like a failed sess.run.
            # (A deliberate deviation, INTEGRATION.md "Non-finite losses": the reference's MonitoredTrainingSession has no
            #  NanTensorHook and would keep stepping on NaN parameters.  No checkpoint is written here -- the parameters
            #  already went through the non-finite update -- the one on disk is from a finite step.)
            bad = [base + i + 1 for i, v in enumerate(vals) if not np.isfinite(v)]
            last_good = bad[0] - 1
            raise RuntimeError(f"non-finite training loss at step(s) {bad[:8]} with no hand-off timeout on any rank: "
                               f"training diverged (or the inputs are not finite); last step with a finite loss: {last_good}; "
                               f"the last good checkpoint ({_ckpt(config)}) was kept")
        good = [(base + i + 1, v) for i, v in enumerate(vals) if np.isfinite(v)]      # (true step index, loss)
        if timed_out:
            # A hand-off of the fused schedule timed out: something else holds part of the chip (a co-tenant, a
            # partitioned device).  The poisoned steps carry NaN losses and the optimizer SKIPPED them (params, m, v
            # untouched), so the model is intact.  Like MonitoredTrainingSession recovering from a failed step
            # (scripts/runners.py:222-232) the loop goes on -- once: re-captured on the schedule without mutual waits.
            if eng.safe_schedule:
                raise RuntimeError(f"training step poisoned between steps {base + 1} and {eng.global_step} although the "
                                   f"schedule without mutual waits is in use (hand-off timeouts: {eng.handoff_timeouts()}; "
                                   f"losses finite: {not nonfinite}); the last good checkpoint was kept")
            bad = [i for i, v in enumerate(vals) if not np.isfinite(v)]
            rewind = bool(bad) and bad == list(range(bad[0], len(vals)))      # the poisoned steps are the block's tail:
            if rewind:                                                        # run them again (new batches, same noise keys)
                eng.global_step = base + bad[0]
                eng.step_dev.fill_(eng.global_step)
            if rank == 0:
                print(f"[run_train] hand-off timeout: {len(bad)} step(s) of {base + 1}..{base + len(vals)} skipped by the "
                      f"optimizer; continuing from step {eng.global_step} on the schedule without mutual waits", flush=True)
            eng.use_safe_schedule()                         # (a field of THIS engine's dims: no process-wide state)
            run_train.degraded = True
        for step_i, v in good:                              # EarlyStoppingHook sees every applied step's (all-reduced) loss
            stop = hook.after_run(step_i, v) or stop        # under its TRUE step index (skipped steps leave gaps)
        vals = [v for _, v in good]
        if fault is not None:
            fault(eng)
        if not vals:
            continue
        if rank == 0 and (eng.global_step % every == 0 or eng.global_step > config.max_steps):
            rate = (eng.global_step - s0) / max(time.time() - t0, 1e-9)
            msg = f"Step {eng.global_step}, loss: {vals[-1]:f}  ({rate:.1f} global_step/sec)" + clip_msg
            if "weighted_objective" in inputs:
                msg += (f"  kl_weight {run_train.weight_log[-1][1]:.4f}  y_weight {run_train.weight_log[-1][2]:.4f}"
                        f"  y_floor_share {(tails[-1, 7] / tails[-1, 4]).item():.4f}")
            if "temperature_on_device" in inputs:           # (of the last step taken)
                msg += f"  temperature {temperature_at(config, eng.global_step - 1):.4f}"
            if "pixel_mask" in inputs:                      # (of the last step taken)
                if tails[-1, 6].item() > 0:
                    msg += f"  imputation_nll {(tails[-1, 5] / tails[-1, 6]).item():.4f}"
                msg += f"  observed_share {(tails[-1, 7] / (tails[-1, 6] + tails[-1, 7])).item():.4f}"
            if grey:                                        # (of the last step taken)
                msg += f"  recon_mse {(tails[-1, 5] / tails[-1, 6]).item():.6f}"
            if "semi_supervised" in inputs:                 # over the summary block's labelled examples (all ranks')
                blk = tails[torch.isfinite(tails[:, 0])][:, 5:8].double().sum(0)
                if blk[1].item() > 0:
                    msg += f"  sup_acc {blk[2].item() / blk[1].item():.4f}  sup_ce {blk[0].item() / blk[1].item():.4f}"
            if config.model == "gmvae" and ds.labels is not None:
                # (--missing_rate: q(y|x) of what the step saw, m x)
                q = model.encoder_y(last_x * ds.pixel_mask[last_rows.long()] if "pixel_mask" in inputs else last_x).distribution.logits
                acc = utils.cluster_acc(q, ds.labels[last_rows.long()], config.mixture_components)
                msg += f"  cluster_acc {acc.item():.4f}"
            print(msg, flush=True)
        if stop and rank == 0:
            print("[Early Stopping Criterion Satisfied]")
        if rank == 0 and time.time() - last_save > 120:     # save_checkpoint_secs=120 (runners.py:226)
            _save_checkpoint(model, _ckpt(config))
            last_save = time.time()
    if rank == 0:
        _save_checkpoint(model, _ckpt(config))
    return model


def _check_embed_size(config, em_n, n, perp):
    """--embed_latent N on a split of fewer than N examples: the perplexity must still fit the codes there are."""
    if n < 4 or not perp < n - 1:
        raise ValueError(f"--embed_latent {em_n}: the {config.split} split holds {n} examples, too few for --tsne_perplexity "
                         f"{perp:g}, which must lie in (1, examples - 1): lower --tsne_perplexity or evaluate a larger split")


@torch.no_grad()
def run_eval(config):
    """scripts/runners.py:235-459 without the plots.  Reports the true per-example loss and, under a
    different name, the reference's figure (sum of per-batch MEANS / number of examples,
    runners.py:298,330-335 -- i.e. roughly loss / batch_size).  Like the reference it WAITS for a checkpoint
    (scripts/utils.py:100-111, 60 s polls; config.checkpoint_poll_seconds / checkpoint_max_wait adjust that)."""
    rank, world, local = parallel.init_from_env()
    torch.cuda.set_device(select_device(config, local))
    data_dim = int(getattr(config, "data_dim", 784))
    model = create_model(config, data_dim, clip=False, weighted=False,     # (the weighting flags are training's: the reported terms stay unweighted)
                         temperature_on_device=False)
    wait_for_checkpoint(_ckpt(config), float(getattr(config, "checkpoint_poll_seconds", 60.0)),
                        getattr(config, "checkpoint_max_wait", None))
    _restore_checkpoint(model, _ckpt(config))
    eng = model._engine
    if config.model == "gmvae" and temperature_flags(config):
        eng.set_temperature(temperature_at(config, eng.global_step))      # the schedule's value where training stopped
    tot = torch.zeros(5, device=eng.device)
    # --missing_rate: the split's fixed masks (missing_mask), resident; a batch's rows are first .. first + B of the split
    pmask_all, pm_tot = None, torch.zeros(3, dtype=torch.float64, device=eng.device)
    if eng.pixel_mask:
        data = _load_mnist(config.data_dir, config.split) if getattr(config, "data_dir", None) else None
        n_split = data[0].shape[0] if data is not None else int(getattr(config, "synthetic_size", 8192))
        pmask_all = torch.from_numpy(missing_mask(config, config.split, n_split, data_dim)).to(eng.device)
    ref_sum, n_batches, codes, labs = 0.0, 0, [], []
    class_hits = torch.zeros(2, dtype=torch.float64, device=eng.device)      # GMVAE: (argmax q(y|x) == label, examples)
    # --iw_samples N: the importance-weighted bound at N samples per example, streamed in chunks; row0 = the example's index in
    # the split, so every example draws its own noise whatever --batch_size or the number of ranks
    iw_n, iw_chunk, iw_rows = int(getattr(config, "iw_samples", 0) or 0), getattr(config, "iw_chunk", None), []
    # --iw_enum_samples N: the same with y summed out over the mixture components (GMVAE, either --y_inference), keyed alike
    ie_n, ie_rows = int(getattr(config, "iw_enum_samples", 0) or 0), []
    # --ais_chains C --ais_temps T: log p(x) by annealed importance sampling from the generative model alone, keyed alike
    ais_c, ais_t, ais_rows = int(getattr(config, "ais_chains", 0) or 0), int(getattr(config, "ais_temps", 0) or 0), []
    # --refine_steps N: the inference gap split by per-example refinement of q(z|x) (Engine.inference_gaps), keyed alike
    rf_t, rf_rows, rf_stats = int(getattr(config, "refine_steps", 0) or 0), [], []
    # --posterior_samples N: the model's own posterior p(y|x) by importance sampling per component (GMVAE), keyed alike
    py_n, py_rows, py_stats, py_logits = int(getattr(config, "posterior_samples", 0) or 0), [], [], []
    # --component_posterior_samples N: the VAE_GMP's posterior p(k|x) over the components of its mixture prior, keyed alike
    pc_n, pc_rows, pc_stats = int(getattr(config, "component_posterior_samples", 0) or 0), [], []
    # --impute_samples N [--impute_draws M] (with --missing_rate): the missing pixels imputed by importance sampling
    # (Engine.impute_posterior), keyed alike; the sums over this rank's examples of (cross-entropy and wrong roundings at the
    # missing pixels, missing pixels, cond_loglik, ESS, distinct draws per example, examples)
    im_n, im_m = int(getattr(config, "impute_samples", 0) or 0), int(getattr(config, "impute_draws", 0) or 0)
    im_tot = torch.zeros(7, dtype=torch.float64, device=eng.device)
    q_logits = []                                           # --real_valued, gmvae: q(y|x)'s logits over the split, for cluster_acc_q
    # --latent_diagnostics N: the first N examples of the split, as the aggregate posterior's components and as its queries
    ld_n, ld_imgs = int(getattr(config, "latent_diagnostics", 0) or 0), []
    # --embed_latent N: the code of the first N examples of the split, embedded in two dimensions by exact t-SNE (tsne.embed)
    em_n = int(getattr(config, "embed_latent", 0) or 0)
    if em_n and world > 1:
        raise ValueError("--embed_latent embeds one rank's codes: it is not available with more than one rank")
    if em_n and not getattr(config, "data_dir", None) and not getattr(config, "data_npy", None):
        # a synthetic split's size is known before the pass (a file's is checked when its codes are in hand)
        _check_embed_size(config, em_n, min(em_n, int(getattr(config, "synthetic_size", 8192))), float(getattr(config, "tsne_perplexity", 40.0)))
    # --fit_latent_mixture N: a mixture fitted to the code of the first N examples of the split, the whole split assigned (mixfit.fit)
    mf_n = int(getattr(config, "fit_latent_mixture", 0) or 0)
    if mf_n and world > 1:
        raise ValueError("--fit_latent_mixture fits one rank's codes: it is not available with more than one rank")
    # --neighbour_scores N: the code of the first N examples of the split scored by its neighbourhoods (neighbours.scores)
    ns_n, ns_k, ns_logits = int(getattr(config, "neighbour_scores", 0) or 0), int(getattr(config, "knn_k", 10)), []
    if ns_n and world > 1:
        raise ValueError("--neighbour_scores scores one rank's codes: it is not available with more than one rank")
    # --linear_probe N: a linear classifier fitted to the code of the first N examples of the split, scored on the next M (linprobe.fit)
    lp_n = int(getattr(config, "linear_probe", 0) or 0)
    if lp_n and world > 1:
        raise ValueError("--linear_probe fits one rank's codes: it is not available with more than one rank")
    # --sample_test N: the kernel two-sample test of N samples of the model against the first N examples of the split (twosample)
    st_n, st_imgs = int(getattr(config, "sample_test", 0) or 0), []
    if st_n and world > 1:
        raise ValueError("--sample_test tests one rank's examples: it is not available with more than one rank")
    # --sample_distance N: the Sinkhorn divergence between N samples of the model and the first N examples of the split (sinkhorn)
    sd_n, sd_imgs = int(getattr(config, "sample_distance", 0) or 0), []
    if sd_n and world > 1:
        raise ValueError("--sample_distance compares one rank's examples: it is not available with more than one rank")
    # --latent_pca N: the spectrum of the code of the first N examples of the split (pca.fit)
    lpca_n = int(getattr(config, "latent_pca", 0) or 0)
    if lpca_n and world > 1:
        raise ValueError("--latent_pca fits one rank's codes: it is not available with more than one rank")
    # --pca_baseline k: PCA + GMM on the examples --fit_latent_mixture fits, as the encoder reads them
    pb_k, pb_imgs = int(getattr(config, "pca_baseline", 0) or 0), []
    if pb_k and not mf_n:
        raise ValueError("--pca_baseline needs --fit_latent_mixture")
    # --sample_frechet N: the Frechet distance between the two code samples --sample_test compares (pca.frechet_distance)
    sf_n, sf_imgs = int(getattr(config, "sample_frechet", 0) or 0), []
    if sf_n and world > 1:
        raise ValueError("--sample_frechet compares one rank's examples: it is not available with more than one rank")
    for images, labels, first in create_dataset(config, config.split, shuffle=False, repeat=False, with_index=True,
                                                standardize=getattr(model, "standardize", None)):
        if pb_k and first < mf_n:
            pb_imgs.append(images[:mf_n - first])
        if first < sf_n:
            sf_imgs.append(images[:sf_n - first])
        if pc_n > 0:
            po = eng.posterior_component(images, pc_n, chunk=iw_chunk, row0=first)
            pc_rows.append(po["log_post"])
            pc_stats.append(torch.stack([po["bound"], po["entropy"], po["kl_post_prior"], po["ess"]], dim=1))
        if py_n > 0:
            po = eng.posterior_y(images, py_n, chunk=iw_chunk, row0=first)
            py_rows.append(po["log_post"])
            py_stats.append(torch.stack([po["bound"], po["entropy"], po["kl_q_post"], po["ess"]], dim=1))
        if first < ld_n:
            ld_imgs.append(images[:ld_n - first])
        if first < st_n:
            st_imgs.append(images[:st_n - first])
        if first < sd_n:
            sd_imgs.append(images[:sd_n - first])
        mk = None if pmask_all is None else pmask_all[first:first + images.shape[0]]
        if iw_n > 0:
            iw_rows.append(eng.iw_bound(images, iw_n, chunk=iw_chunk, row0=first, mask=mk)["bound"])
        if ie_n > 0:
            ie_rows.append(eng.iw_bound_enum_y(images, ie_n, chunk=iw_chunk, row0=first)["bound"])
        if im_n > 0 and mk is not None:
            io = eng.impute_posterior(images, im_n, mask=mk, n_draws=im_m, chunk=iw_chunk, row0=first)
            t = (images.reshape(io["mean"].shape).to(eng.device) != 0).double()
            ph = io["mean"].double().clamp(1e-12, 1.0 - 1e-12)
            miss = (mk.to(eng.device) == 0).double()
            distinct = torch.zeros((), dtype=torch.float64, device=eng.device)
            if im_m > 0:
                srt = io["draw_index"].sort(dim=1).values
                distinct = (1 + (srt[:, 1:] != srt[:, :-1]).sum(dim=1)).double().sum()
            im_tot += torch.stack([-(miss * (t * ph.log() + (1.0 - t) * (-ph).log1p())).sum(),
                                   (miss * ((ph >= 0.5).double() != t).double()).sum(), miss.sum(),
                                   io["cond_loglik"].double().sum(), io["ess"].double().sum(), distinct,
                                   torch.tensor(float(t.shape[0]), dtype=torch.float64, device=eng.device)])
        if ais_c > 0:
            ais_rows.append(eng.ais_bound(images, ais_c, ais_t, schedule=getattr(config, "ais_schedule", "sigmoid"),
                                          n_leapfrog=int(getattr(config, "ais_leapfrog", 10)),
                                          step_size=float(getattr(config, "ais_step_size", 0.05)),
                                          init=getattr(config, "ais_init", "prior"), row0=first)["stats"])
        if rf_t > 0:
            g = eng.inference_gaps(images, rf_t, int(getattr(config, "refine_samples", 4)), int(getattr(config, "refine_eval_samples", 256)),
                                   float(getattr(config, "refine_lr", 0.05)), row0=first)
            rf_rows.append(g["elbo_amortised_rows"])
            rf_stats.append(g["refine"]["stats"])
        o = eng.forward(images, mask=mk)
        tot += o["tail"][:5]
        pm_tot += o["tail"][5:8].double()
        ref_sum += (o["tail"][0] / o["tail"][4]).item()
        n_batches += 1
        # z = model.transform(flat_inputs) (runners.py:274): the VAE's MEAN code (vae.py:108-114), the GMVAE's SAMPLED
        # code (gmvae.py:140-149) -- the forward pass's z is exactly that sample
        # (y enumerated: the code of the example's most probable component, at its sample 0 with --y_inference=marginal_iw)
        if config.model == "gmvae" and eng.marginal:
            B = o["logits"].shape[0]
            z = o["z"].view(B, eng.rows_per_x // eng.K, eng.K, eng.Lz)[:, 0]
            codes.append(z[torch.arange(B, device=eng.device), o["logits"].argmax(dim=1)])
        else:
            codes.append(o["z"] if config.model == "gmvae" else model.transform(images if mk is None else images * mk))
        labs.append(labels)
        if config.model == "gmvae":
            class_hits[0] += (o["logits"].argmax(dim=1) == labels.to(eng.device)).sum()
            class_hits[1] += labels.numel()
        if py_n > 0:
            py_logits.append(o["logits"])
        if eng.real_valued and config.model == "gmvae":
            q_logits.append(o["logits"])
        if ns_n and config.model == "gmvae" and first < ns_n:
            ns_logits.append(o["logits"][:ns_n - first])
    # --bdmc_examples N: bidirectional Monte Carlo on N examples SIMULATED from the model (Engine.bdmc_gap) at the --ais_* settings:
    # example i is Philox row i whatever --batch_size or the number of ranks; each rank takes a contiguous share
    bd_n, bd_rows = int(getattr(config, "bdmc_examples", 0) or 0), []
    if bd_n > 0:
        share = (bd_n + world - 1) // world
        lo, hi = min(rank * share, bd_n), min((rank + 1) * share, bd_n)
        for first in range(lo, hi, int(config.batch_size)):
            g = eng.bdmc_gap(min(int(config.batch_size), hi - first), ais_c, ais_t, row0=first,
                             schedule=getattr(config, "ais_schedule", "sigmoid"), n_leapfrog=int(getattr(config, "ais_leapfrog", 10)),
                             step_size=float(getattr(config, "ais_step_size", 0.05)), init=getattr(config, "ais_init", "prior"))
            bd_rows.append(torch.stack([g["lower"], g["upper"], g["upper_ess"], g["upper_accept"]], dim=1))
    # the sums over this rank's simulated examples of (lower, upper, reverse ESS, reverse acceptance rate), and their number
    bd_tot = torch.zeros(5, dtype=torch.float64, device=eng.device)
    if bd_rows:
        bd_tot[:4] = torch.cat(bd_rows).double().sum(0)
        bd_tot[4] = sum(r.shape[0] for r in bd_rows)
    iw_sum = torch.cat(iw_rows).double().sum().reshape(1) if iw_rows else torch.zeros(1, dtype=torch.float64, device=eng.device)
    ie_sum = torch.cat(ie_rows).double().sum().reshape(1) if ie_rows else torch.zeros(1, dtype=torch.float64, device=eng.device)
    py_tot = torch.cat(py_stats).double().sum(0) if py_stats else torch.zeros(4, dtype=torch.float64, device=eng.device)
    pc_tot = torch.cat(pc_stats).double().sum(0) if pc_stats else torch.zeros(4, dtype=torch.float64, device=eng.device)
    ais_tot = torch.cat(ais_rows).double().sum(0) if ais_rows else torch.zeros(4, dtype=torch.float64, device=eng.device)
    # the sums over this rank's examples of (elbo_amortised, elbo_refined, iw_refined)
    rf_tot = torch.zeros(3, dtype=torch.float64, device=eng.device)
    if rf_rows:
        rf_tot = torch.stack([torch.cat(rf_rows).sum(), *torch.cat(rf_stats)[:, [1, 3]].double().sum(0)])
    if world > 1:
        parallel.all_reduce_flat(tot)
        if rf_t > 0:
            parallel.all_reduce_flat(rf_tot)
        if ais_c > 0:
            parallel.all_reduce_flat(ais_tot)
        if bd_n > 0:
            parallel.all_reduce_flat(bd_tot)
        parallel.all_reduce_flat(iw_sum)
        parallel.all_reduce_flat(class_hits)
        parallel.all_reduce_flat(pm_tot)
        if im_n > 0:
            parallel.all_reduce_flat(im_tot)
        if ie_n > 0:
            parallel.all_reduce_flat(ie_sum)
        if py_n > 0:
            parallel.all_reduce_flat(py_tot)
        if pc_n > 0:
            parallel.all_reduce_flat(pc_tot)
    n = tot[4].item()
    res = {f"{config.split}/loss_per_example": tot[0].item() / n, f"{config.split}/nll": tot[1].item() / n,
           f"{config.split}/kl_div_z": tot[2].item() / n, f"{config.split}/nent": tot[3].item() / n,
           f"{config.split}/reference_misnormalised_loss_per_example": ref_sum / n, "examples": int(n)}
    if config.model == "gmvae":
        # the share of examples whose most probable component under q(y|x) IS their label -- no mode matching: meaningful
        # where training saw labels (--labelled_per_class), chance level otherwise
        res[f"{config.split}/class_acc_q"] = class_hits[0].item() / max(class_hits[1].item(), 1.0)
    if eng.pixel_mask:
        # loss_per_example and nll above count the observed pixels alone; the held-out ones are scored per missing pixel
        if pm_tot[1].item() > 0:
            res[f"{config.split}/imputation_nll"] = pm_tot[0].item() / pm_tot[1].item()
        res[f"{config.split}/observed_share"] = pm_tot[2].item() / (pm_tot[1].item() + pm_tot[2].item())
        if im_n > 0:
            # the same held-out pixels scored under the importance-sampling imputation p^ at im_n samples; cond_loglik per
            # example is the proper score log p^(x_missing | x_observed), ESS the effective number of the im_n samples
            it = im_tot.tolist()
            res[f"{config.split}/imputation_nll_is"] = it[0] / max(it[2], 1.0)
            res[f"{config.split}/imputation_error_rate_is"] = it[1] / max(it[2], 1.0)
            res[f"{config.split}/imputation_cond_loglik"] = it[3] / max(it[6], 1.0)
            res[f"{config.split}/imputation_ess"] = it[4] / max(it[6], 1.0)
            if im_m > 0:
                res[f"{config.split}/imputation_distinct_draws"] = it[5] / max(it[6], 1.0) / im_m
    if eng.likelihood != "bernoulli":
        # the per-pixel squared error of the mean image A'(lambda) against t = pixel / 255 (tail[5] / tail[6] over the split)
        res[f"{config.split}/recon_mse"] = pm_tot[0].item() / max(pm_tot[1].item(), 1.0)
    if eng.likelihood_scale == "learned":
        res[f"{config.split}/sigma_mean"] = torch.exp(eng.views()["decoder/log_sigma"]).mean().item()
    if eng.likelihood == "negative_binomial":
        res[f"{config.split}/dispersion_mean"] = torch.exp(eng.views()["decoder/log_dispersion"]).mean().item()
    if q_logits:
        # clustering accuracy of q(y|x) over the WHOLE split, components matched to labels by majority (utils.cluster_acc)
        res[f"{config.split}/cluster_acc_q"] = utils.cluster_acc(torch.cat(q_logits), torch.cat(labs), int(config.mixture_components),
                                                                 all_reduce=True).item()
    if iw_n > 0:
        res[f"{config.split}/iw_bound_{iw_n}_per_example"] = iw_sum.item() / n
    if ie_n > 0:
        res[f"{config.split}/iw_bound_enum_y_{ie_n}_per_example"] = ie_sum.item() / n
    if ais_c > 0:
        # log p(x) itself (the GMVAE's uniform p(y) inside): the gap to an importance-weighted bound is what the inference
        # network loses; iw_bound_enum_y leaves a + ln K out, which the gap puts back
        res[f"{config.split}/ais_log_px"] = ais_tot[0].item() / n
        res[f"{config.split}/ais_ess"] = ais_tot[1].item() / n
        res[f"{config.split}/ais_accept_rate"] = ais_tot[2].item() / n
        res[f"{config.split}/ais_step_size"] = ais_tot[3].item() / n
        if ie_n > 0:
            res[f"{config.split}/ais_gap_to_iw_bound_enum_y"] = ((ais_tot[0].item() - ie_sum.item()) / n
                                                                 + math.log(int(config.mixture_components)))
        elif iw_n > 0 and config.model != "gmvae":
            res[f"{config.split}/ais_gap_to_iw_bound"] = (ais_tot[0].item() - iw_sum.item()) / n
    if bd_n > 0:
        # lower <= log p(x) <= upper in expectation ON SIMULATED DATA (a real x has no exact posterior sample, so no upper bound):
        # the gap bounds the bias of ais_log_px at these settings on data distributed as the model's own samples
        m = bd_tot[4].item()
        res[f"{config.split}/bdmc_lower"] = bd_tot[0].item() / m
        res[f"{config.split}/bdmc_upper"] = bd_tot[1].item() / m
        res[f"{config.split}/bdmc_gap"] = (bd_tot[1].item() - bd_tot[0].item()) / m
        res[f"{config.split}/bdmc_reverse_ess"] = bd_tot[2].item() / m
        res[f"{config.split}/bdmc_reverse_accept_rate"] = bd_tot[3].item() / m
    if rf_t > 0:
        # the inference gap in its two parts (Cremer et al. 2018); log p(x) is the larger of the two lower bounds in hand
        am, er, ir = (rf_tot / n).tolist()
        log_px = max(ir, ais_tot[0].item() / n) if ais_c > 0 else ir
        res[f"{config.split}/elbo_amortised"], res[f"{config.split}/elbo_refined"] = am, er
        res[f"{config.split}/iw_bound_refined"] = ir
        res[f"{config.split}/amortisation_gap"] = er - am
        res[f"{config.split}/approximation_gap"] = log_px - er
    if py_n > 0:
        # clustering accuracy over the WHOLE split (the ranks' histograms add), by the model's posterior and by q(y|x)
        K, all_labs = int(config.mixture_components), torch.cat(labs)
        res[f"{config.split}/cluster_acc_posterior_{py_n}"] = utils.cluster_acc(torch.cat(py_rows), all_labs, K,
                                                                                 all_reduce=True).item()
        res[f"{config.split}/cluster_acc_q"] = utils.cluster_acc(torch.cat(py_logits), all_labs, K, all_reduce=True).item()
        res[f"{config.split}/posterior_entropy_{py_n}_per_example"] = py_tot[1].item() / n
        res[f"{config.split}/kl_q_posterior_{py_n}_per_example"] = py_tot[2].item() / n
        res[f"{config.split}/ess_{py_n}_per_example"] = py_tot[3].item() / n
    if pc_n > 0:
        # clustering accuracy over the WHOLE split (the ranks' histograms add), by the model's posterior over its prior's components
        res[f"{config.split}/cluster_acc_posterior_{pc_n}"] = utils.cluster_acc(torch.cat(pc_rows), torch.cat(labs),
                                                                                 int(config.mixture_components), all_reduce=True).item()
        res[f"{config.split}/posterior_entropy_{pc_n}_per_example"] = pc_tot[1].item() / n
        res[f"{config.split}/kl_posterior_prior_{pc_n}_per_example"] = pc_tot[2].item() / n
        res[f"{config.split}/ess_{pc_n}_per_example"] = pc_tot[3].item() / n
    if ld_imgs:
        # the decomposition of kl_div_z over this rank's first N examples (Engine.aggregate_posterior): E_x KL(q(z|x) || p(z)) =
        # kl_avg = mi_xz + kl_marginal, the total correlation of q(z), the dimensions in use; GMVAE: what q(y|x) says about x
        ld = eng.aggregate_posterior(torch.cat(ld_imgs))
        for key, name in (("mi", "mi_xz"), ("kl_marginal", "kl_marginal"), ("tc", "total_correlation"), ("kl_avg", "kl_avg"),
                          ("active_units", "active_units"), ("mi_xy", "mi_xy"), ("q_y_entropy", "q_y_entropy")):
            if ld[key] is not None:
                res[f"{config.split}/{name}"] = ld[key].item()
    if rank == 0:
        for k, v in res.items():
            print(f"{k}: {v}")
    # The tensors the reference's evaluation graph also produces (scripts/runners.py:274-292) and hands to its plots
    # (which are out of scope): the latent state and labels over the split, `num_samples` draws from the prior and
    # `num_generations` decoded prior draws; for the GMVAE additionally the decoded draws of ONE random component k,
    # stacked on the unconditional ones (runners.py:285-292).
    img_shape = (28, 28, 1) if data_dim == 784 else (data_dim, 1, 1)
    res["latent_state"] = torch.cat(codes) if codes else None
    res["labels"] = torch.cat(labs) if labs else None
    res["iw_bounds"] = torch.cat(iw_rows) if iw_rows else None      # this rank's examples, in split order
    res["iw_bounds_enum_y"] = torch.cat(ie_rows) if ie_rows else None
    res["refine_stats"] = torch.cat(rf_stats) if rf_stats else None   # [..., 8]: Engine.REFINE_STATS
    res["bdmc_stats"] = torch.cat(bd_rows) if bd_rows else None     # [..., 4]: lower, upper, reverse ESS, reverse acceptance rate
    res["ais_stats"] = torch.cat(ais_rows) if ais_rows else None     # [..., 4]: log p(x) estimate, ESS, acceptance rate, step size
    if py_n > 0:
        res["log_posterior_y"] = torch.cat(py_rows)                  # [this rank's examples, K], in split order
        res["posterior_y_stats"] = torch.cat(py_stats)               # [..., 4]: bound, entropy, KL(q || p(y|x)), ESS
    if pc_n > 0:
        res["log_posterior_component"] = torch.cat(pc_rows)          # [this rank's examples, K], in split order
        res["posterior_component_stats"] = torch.cat(pc_stats)       # [..., 4]: bound, entropy, KL(p(k|x) || pi), ESS
    res["samples"] = model.generate_samples(num_samples=int(config.num_samples))
    sample_images = utils.unflatten_tensor(model.generate_sample_images(num_samples=int(config.num_generations)), img_shape)
    if config.model == "gmvae":
        k = int(np.random.randint(0, high=config.mixture_components))
        samples_k = model.generate_samples(num_samples=int(config.num_generations) * int(config.mixture_components), clusters=[k])
        sample_images_k = utils.unflatten_tensor(model.generate_sample_images(samples_k, name="sample_images_k"), img_shape)
        sample_images = torch.stack((sample_images, sample_images_k), dim=0)
        res["sampled_cluster"] = k
    res["sample_images"] = sample_images
    if em_n:
        # utils.reduce_dimensionality on the code and on the prior draws (scripts/runners.py:446-450), without the plots
        perp, iters = float(getattr(config, "tsne_perplexity", 40.0)), int(getattr(config, "tsne_iters", 300))
        seed = int(config.random_seed) if getattr(config, "random_seed", None) is not None else 0
        em_codes = res["latent_state"][:em_n]
        _check_embed_size(config, em_n, em_codes.shape[0], perp)
        emb = tsne.embed(em_codes, perplexity=perp, n_iter=iters, seed=seed,
                         init="pca" if getattr(config, "tsne_init", "random") == "pca" else None)
        res["latent_embedding"] = emb["embedding"]
        res[f"{config.split}/embedding_kl"] = emb["kl"].item()
        smp = res["samples"]
        res["samples_embedding"] = (tsne.embed(smp, perplexity=perp, n_iter=iters, seed=seed)["embedding"]
                                    if smp.shape[0] >= 4 and perp < smp.shape[0] - 1 else None)
        if rank == 0:
            print(f"{config.split}/embedding_kl: {res[f'{config.split}/embedding_kl']}")
        if getattr(config, "embedding_out", None):
            np.save(config.embedding_out, res["latent_embedding"].cpu().numpy())
    if mf_n:
        # the "VAE + GMM" baseline: EM on the first N codes, then every code of the split assigned to its component
        K = int(config.mixture_components)
        seed = int(config.random_seed) if getattr(config, "random_seed", None) is not None else 0
        mf_codes = res["latent_state"]
        if mf_codes[:mf_n].shape[0] < K:
            raise ValueError(f"--fit_latent_mixture {mf_n}: the {config.split} split holds {mf_codes.shape[0]} examples, fewer than "
                             f"--mixture_components {K}")
        fitted = mixfit.fit(mf_codes[:mf_n], K, n_iter=int(getattr(config, "mixture_fit_iters", 100)),
                            n_init=int(getattr(config, "mixture_fit_inits", 1)), seed=seed,
                            covariance=getattr(config, "mixture_covariance", "diag"))
        whole = mixfit.assign(mf_codes, fitted)
        res[f"{config.split}/latent_mixture_loglik"] = whole["lse"].double().mean().item()
        res[f"{config.split}/cluster_acc_latent_mixture"] = utils.cluster_acc(whole["log_resp"], res["labels"], K).item()
        res["latent_mixture"] = fitted
        if getattr(config, "mixture_bic", False):
            res[f"{config.split}/latent_mixture_bic"] = mixfit.bic(fitted, mf_codes[:mf_n].shape[0]).item()
        if rank == 0:
            for k in ("latent_mixture_loglik", "cluster_acc_latent_mixture") + (("latent_mixture_bic",) if getattr(config, "mixture_bic", False) else ()):
                print(f"{config.split}/{k}: {res[f'{config.split}/{k}']}")
    if pb_k:
        # the "PCA + GMM" baseline: the same examples as the encoder reads them (binary under the Bernoulli likelihood, else the
        # values themselves), projected on their first k principal components, fitted with the latent fit's settings
        pb_x = torch.cat(pb_imgs).to(eng.device)
        pb_x = pb_x.reshape(pb_x.shape[0], -1)
        pb_x = (pb_x != 0).float() if eng.likelihood == "bernoulli" else pb_x.float()
        n, D = pb_x.shape
        if n < max(2, K) or D > pca.MAX_D or pb_k > min(D, pca.MAX_M):
            raise ValueError(f"--pca_baseline {pb_k}: needs at least max(2, --mixture_components) examples (the split gave {n}), a data "
                             f"dimension of at most {pca.MAX_D} (it is {D}) and k <= min(data dimension, {pca.MAX_M})")
        pb_fit = pca.fit(pb_x, n_components=pb_k, seed=seed)
        if int(pb_fit["info"].item()) != 0:
            raise ValueError(f"--pca_baseline {pb_k}: the {n} examples span fewer dimensions than the subspace iteration's "
                             f"{min(pb_k + pca.OVERSAMPLE, pca.MAX_M, D)} vectors: lower k or fit more examples")
        pb_z = pca.transform(pb_x, pb_fit)
        pb_mix = mixfit.fit(pb_z, K, n_iter=int(getattr(config, "mixture_fit_iters", 100)),
                            n_init=int(getattr(config, "mixture_fit_inits", 1)), seed=seed,
                            covariance=getattr(config, "mixture_covariance", "diag"))
        pb_as = mixfit.assign(pb_z, pb_mix)
        res[f"{config.split}/pca_mixture_loglik"] = pb_as["lse"].double().mean().item()
        res[f"{config.split}/cluster_acc_pca_mixture"] = utils.cluster_acc(pb_as["log_resp"], res["labels"][:n], K).item()
        res[f"{config.split}/pca_residual_max"] = pb_fit["residual"].max().item()
        res["pca_baseline"] = {"pca": pb_fit, "mixture": pb_mix}
        if rank == 0:
            for k in ("pca_mixture_loglik", "cluster_acc_pca_mixture", "pca_residual_max"):
                print(f"{config.split}/{k}: {res[f'{config.split}/{k}']}")
    if lpca_n:
        # the rotation-invariant counterpart of the active units: the spectrum of the code's covariance
        lp_fit = pca.fit(res["latent_state"][:lpca_n])
        res["latent_pca"] = lp_fit
        for k, v in {**pca.spectrum_summary(lp_fit), "offdiag": lp_fit["offdiag"]}.items():
            res[f"{config.split}/latent_pca_{k}"] = v.item()
            if rank == 0:
                print(f"{config.split}/latent_pca_{k}: {res[f'{config.split}/latent_pca_{k}']}")
    if sf_n:
        sf_x = torch.cat(sf_imgs)
        if sf_x.shape[0] < 2:
            raise ValueError(f"--sample_frechet {sf_n}: the {config.split} split holds {sf_x.shape[0]} examples; it needs two")
        prior, code = twosample.model_samples(model, sf_x, None, "code", what="--sample_frechet")["code"]
        res["sample_frechet"] = pca.frechet_distance(prior, code)
        res[f"{config.split}/frechet_code"] = res["sample_frechet"]["distance"].item()
        if rank == 0:
            print(f"{config.split}/frechet_code: {res[f'{config.split}/frechet_code']}")
    if ns_n:
        # the model's own clustering, where it has one: the GMVAE's argmax q(y|x), the VAE_GMP's posterior over its prior's
        # components (--component_posterior_samples); then the fitted mixture's assignment, then the embedding's neighbourhoods
        K = int(config.mixture_components)
        ns_codes, ns_labs = res["latent_state"][:ns_n], res["labels"][:ns_n].to(eng.device)
        n = ns_codes.shape[0]
        if not n > 2 * ns_k:
            raise ValueError(f"--neighbour_scores {ns_n}: the {config.split} split holds {n} examples, too few for --knn_k {ns_k}, "
                             f"which must be below examples / 2: lower --knn_k or evaluate a larger split")
        n_labels = max(10, int(ns_labs.max().item()) + 1)                  # (as utils.cluster_acc widens its histogram)
        if n_labels > neighbours.MAX_C:
            raise ValueError(f"--neighbour_scores: the labels reach {n_labels - 1}, past the {neighbours.MAX_C} classes it takes")
        clusters = (torch.cat(ns_logits).argmax(dim=1) if ns_logits else torch.cat(pc_rows)[:ns_n].argmax(dim=1) if pc_rows else None)
        sc = neighbours.scores(ns_codes, ns_labs, clusters, k=ns_k, n_labels=n_labels, n_clusters=K if clusters is not None else None)
        new = {f"knn_acc_loo_{ns_k}": sc["knn_acc_loo"], "silhouette_labels": sc["silhouette_labels"]}
        if clusters is not None:
            new.update(silhouette_clusters=sc["silhouette_clusters"], nmi_clusters=sc["nmi"], ari_clusters=sc["ari"])
            res["neighbour_clusters"] = clusters                               # the clustering that was scored, [examples scored]
        if mf_n:
            assigned = whole["log_resp"][:ns_n].argmax(dim=1)
            new.update(silhouette_latent_mixture=neighbours.silhouette(ns_codes, assigned, K)["score"],
                       nmi_latent_mixture=neighbours.nmi(ns_labs, assigned, n_labels, K),
                       ari_latent_mixture=neighbours.ari(ns_labs, assigned, n_labels, K))
        if em_n:
            m = min(n, res["latent_embedding"].shape[0])
            if not m > 2 * ns_k:
                raise ValueError(f"--neighbour_scores with --embed_latent {em_n}: {m} embedded examples are too few for --knn_k {ns_k}")
            new[f"embedding_trustworthiness_{ns_k}"] = neighbours.trustworthiness(ns_codes[:m], res["latent_embedding"][:m], ns_k)
            new[f"embedding_continuity_{ns_k}"] = neighbours.continuity(ns_codes[:m], res["latent_embedding"][:m], ns_k)
        for k, v in new.items():
            res[f"{config.split}/{k}"] = v.item()
            if rank == 0:
                print(f"{config.split}/{k}: {res[f'{config.split}/{k}']}")
    if lp_n:
        # the linear probe: fitted on the first N codes (with --probe_labelled_per_class on the labels select_labelled shows: the M1
        # baseline of a semi-supervised run with the same seed), scored on the next M
        lp_codes, lp_labs = res["latent_state"], res["labels"]
        total = lp_codes.shape[0]
        lp_m = int(getattr(config, "probe_test", 0) or 0) or min(lp_n, total - lp_n)
        if lp_n >= total or lp_m < 1 or lp_n + lp_m > total:
            raise ValueError(f"--linear_probe {lp_n} with --probe_test {lp_m}: the {config.split} split holds {total} examples; it "
                             f"must hold the N fitted and at least one more to score")
        n_labels = max(10, int(lp_labs.max().item()) + 1)                  # (as utils.cluster_acc widens its histogram)
        linprobe.check_sizes(lp_n, lp_codes.shape[1], n_labels)
        seed = int(config.random_seed) if getattr(config, "random_seed", None) is not None else 0
        lpc = int(getattr(config, "probe_labelled_per_class", 0) or 0)
        train_labs = lp_labs[:lp_n]
        shown = torch.from_numpy(select_labelled(train_labs.cpu().numpy(), lpc, seed)) if lpc > 0 else train_labs
        fitted = linprobe.fit(lp_codes[:lp_n], shown, n_labels, l2=float(getattr(config, "probe_l2", 1e-3)),
                              n_iter=int(getattr(config, "probe_iters", 300)), standardize=bool(getattr(config, "probe_standardize", False)))
        tr = linprobe.score(lp_codes[:lp_n], train_labs, fitted)
        te = linprobe.score(lp_codes[lp_n:lp_n + lp_m], lp_labs[lp_n:lp_n + lp_m], fitted)
        res["linear_probe"] = fitted
        for k, v in (("linear_probe_acc", te["accuracy"]), ("linear_probe_nll", te["nll"]), ("linear_probe_train_acc", tr["accuracy"]),
                     ("linear_probe_grad_max", fitted["grad_max"])):
            res[f"{config.split}/{k}"] = v.item()
            if rank == 0:
                print(f"{config.split}/{k}: {res[f'{config.split}/{k}']}")
    if st_n:
        # the two-sample test: as many samples of the model as examples, per space the statistic and its permutation p-value
        st_x = torch.cat(st_imgs)
        if st_x.shape[0] < 2:
            raise ValueError(f"--sample_test {st_n}: the {config.split} split holds {st_x.shape[0]} examples; the test needs two")
        seed = int(config.random_seed) if getattr(config, "random_seed", None) is not None else 0
        tested = model.sample_test(st_x, space=getattr(config, "sample_test_space", "data"),
                                   n_perms=int(getattr(config, "sample_test_perms", 1000)),
                                   kernel=getattr(config, "sample_test_kernel", "rbf"), seed=seed)
        res["sample_test"] = tested
        for space, t in tested.items():
            for k, v in ((f"mmd2_{space}", t["mmd2"]), (f"mmd_p_{space}", t["p_value"])):
                res[f"{config.split}/{k}"] = v.item()
                if rank == 0:
                    print(f"{config.split}/{k}: {res[f'{config.split}/{k}']}")
    if sd_n:
        # the transport distance: as many samples of the model as examples, per space the divergence and its convergence readout
        sd_x = torch.cat(sd_imgs)
        if sd_x.shape[0] < 2:
            raise ValueError(f"--sample_distance {sd_n}: the {config.split} split holds {sd_x.shape[0]} examples; it needs two")
        seed = int(config.random_seed) if getattr(config, "random_seed", None) is not None else 0
        sd_p = int(getattr(config, "sample_distance_perms", 0) or 0)
        measured = model.sample_distance(sd_x, space=getattr(config, "sample_distance_space", "data"), n_perms=sd_p,
                                         blur_rel=float(getattr(config, "sinkhorn_blur_rel", 0.1)),
                                         n_iter=int(getattr(config, "sinkhorn_iters", 200)), **({"seed": seed} if sd_p else {}))
        res["sample_distance"] = measured
        for space, t in measured.items():
            for k, v in ((f"sinkhorn_{space}", t["sinkhorn"]), (f"sinkhorn_marginal_err_{space}", t["marginal_err"])) + \
                    (((f"sinkhorn_p_{space}", t["p_value"]),) if sd_p else ()):
                res[f"{config.split}/{k}"] = v.item()
                if rank == 0:
                    print(f"{config.split}/{k}: {res[f'{config.split}/{k}']}")
    return res
