"""-m gpu: every fused TF-Adam site of the library held to the update statement, element by element.

adam_update (csrc/adam.hpp) is one statement applied from about thirty call sites, each with its own plumbing of alpha_t,
1 - b1, 1 - b2, eps and 1 / count and its own map from threads to the elements of the flat buffer.  The update is elementwise,
and every schedule leaves the gradient SUMS it applied in the gradient buffer and the count in tail[4]: from the device's own
(p, m, v) before a step and its own g after it, tests/adam_ref.py predicts (p', m', v') in fp64 to a few fp32 roundings -- the
error of the gradient kernels cancels, no forward oracle is needed.  A case is one graph launch plus NumPy over P elements.

Per site (one per optimizer tail, at the smallest batch its gate admits; the schedule string -- and GMVAE_TRACE's line for the
data-parallel tails -- is asserted so that a case cannot land elsewhere), hyperparameter set (adam_ref.HP: the second differs
from TF's defaults in every value, with eps comparable to sqrt(v)) and step counter t0 (adam_ref.T0), check_site:
  m', v', p' inside adam_ref.bounds over every real element; every element with g != 0 updated, every one with g = m = 0 left
  alone (each element updated once, by somebody); the padding finite; the counter advanced by one; no hand-off timeout.
  "Updated" is read on the optimizer STATE, not on p alone: an update below half an ulp of p leaves p's bits as they are in any
  fp32 implementation, so an element counts as updated when any of p, m, v changed, and it is required of every element with
  |gj| > 1e-18 (below, gj^2 is no normal fp32 number and v' may keep its bits; b1 = 0 with gj = m keeps m).  What this leaves
  open the m' bound closes: an element nobody updated keeps m, which is (1 - b1) |gj - m| away from m' -- outside 4u (|gj| + |m|)
  unless gj and m agree to 4u / (1 - b1).
alpha_t: "fp64" sites get d_alpha = 2u, "fp32" sites (-expm1f form: dw_adam without mega2's lr_t_out, the skinny schedule) the
CPU-measured, doubled error of that form (adam_ref.d_alpha_fp32; tests/test_optimizer_sites_cpu.py bounds it).
Measured margins per site: profiles/optimizer_sites_notes.md."""
import dataclasses

import numpy as np
import pytest
import torch

import adam_ref as A
import oracle as O

pytestmark = pytest.mark.gpu

@dataclasses.dataclass(frozen=True)
class Site:
    id: str
    model: str
    D: int
    L: int
    K: int
    hidden: tuple
    B: int
    sched: str                  # gmvae_step_schedule
    alpha: str                  # "fp64" | "fp32": the form of alpha_t the site computes
    hps: tuple = (1, 2)
    mode: str = "graph"         # graph: single-device train graph | dp: DP graph behind a one-rank communicator | eager: Engine.train_step
    S: int = 1
    y_inference: str = "gumbel"
    env: tuple = ()
    trace: tuple = None         # dp: GMVAE_TRACE's (first_layer_inside, workgroups_per_panel, specialised) of the captured step
    n3: tuple = ()              # step counters at which a 3-step graph is checked too (steps 2..3: the in-graph forms, a cached alpha_t)
    w_form: str = None          # skinny: the W stage's kernel at these sizes (_skinny_w_form; the schedule string does not name it)


G784 = dict(D=784, K=10, hidden=(64,))
SITES = [
    # ---- the one-launch steps: alpha_t (fp64) from the previous step's tail slot (lr_next) in steps 2..n of a graph
    Site("mega3_step", "gmvae", L=64, B=1024, sched="mega2", alpha="fp64", n3=(999, A.T0_WRAP), **G784),   # the only batch with fuse_pending
    Site("mega3v_step-vae", "vae", 784, 2, 1, (64,), 100, "mega2v", "fp64", n3=(999,)),
    Site("mega3v_step-vae_gmp", "vae_gmp", L=64, B=256, sched="mega2v", alpha="fp64", n3=(999,), **G784),  # + the prior's tensors
    # ---- mega2_fwd_bwd + dw_adam, alpha_t (fp64) from mega2_fwd_bwd's lr_t_out
    Site("mega2+dw_adam", "gmvae", L=64, B=17, sched="mega2", alpha="fp64", hps=(1, 2, 3, 4), n3=(999,), **G784),
    # ---- the generic mega instance + dw_adam with its own fp32 alpha_t (D = 896: the last D with the first layer inside the launch);
    #      D = 912, the first one past it: no dw_adam -- split-K weight gradients and finalize_adam (fp64 alpha_t)
    Site("mega+dw_adam", "gmvae", L=16, B=24, sched="mega", alpha="fp32", hps=(1, 2, 3, 4), n3=(999,), **G784),
    Site("mega+dw_adam-gmvae-D896", "gmvae", 896, 36, 10, (64,), 24, "mega", "fp32", n3=(999,)),
    Site("mega+finalize_adam-gmvae-D912", "gmvae", 912, 36, 10, (64,), 24, "mega", "fp64", n3=(999,)),
    Site("mega+dw_adam-vae-D896", "vae", 896, 8, 1, (64,), 24, "mega", "fp32", n3=(999,)),
    Site("mega+finalize_adam-vae-D912", "vae", 912, 8, 1, (64,), 24, "mega", "fp64", n3=(999,)),
    Site("mega+dw_adam-vae_gmp-D896", "vae_gmp", 896, 8, 10, (64,), 24, "mega", "fp32", n3=(999,)),
    Site("mega+finalize_adam-vae_gmp-D912", "vae_gmp", 912, 8, 10, (64,), 24, "mega", "fp64", n3=(999,)),
    # ---- the skinny schedule (fp32 alpha_t everywhere).  Its W stage has four forms (csrc/gmvae_hip.hip run_skinny, launch_dw): up to
    #      128 rows sk_dw; above, [64 x 64] tiles -- at most 256 of them: sk_dwb<1>; more: sk_dwb<0>, or from 512 rows sk_dwc, whose
    #      last-arriving batch share runs the optimizer.  The GMVAE has more than 256 tiles from H = 512 on (three D x H tensors), so at
    #      H = 512, B = 768 sk_dwb<1> is the VAE family's and the GMVAE takes sk_dwc; only the GMVAE has tensors whose N is no
    #      multiple of 4 (encoder_y/linear_1: N = K = 10), the scalar branch of every form's optimizer epilogue
    Site("skinny-W-gmvae", "gmvae", 784, 128, 10, (512,), 64, "skinny", "fp32", hps=(1, 2, 3, 4), w_form="sk_dw"),
    Site("skinny-W-vae", "vae", 784, 128, 1, (512,), 64, "skinny", "fp32", w_form="sk_dw"),
    Site("skinny-W-vae_gmp", "vae_gmp", 784, 64, 10, (512,), 64, "skinny", "fp32", w_form="sk_dw"),
    Site("skinny-B129", "gmvae", 784, 8, 10, (256,), 129, "skinny", "fp32", w_form="sk_dwb<1>"),          # 173 tiles
    Site("skinny-dwb0-gmvae", "gmvae", 784, 64, 10, (512,), 129, "skinny", "fp32", w_form="sk_dwb<0>"),   # 354 tiles, B < 512
    Site("skinny-dwb1-vae", "vae", 784, 64, 1, (512,), 768, "skinny", "fp32", w_form="sk_dwb<1>"),        # 232 tiles
    Site("skinny-dwb1-vae_gmp", "vae_gmp", 784, 64, 10, (512,), 768, "skinny", "fp32", w_form="sk_dwb<1>"),
    Site("skinny-dwc-gmvae-H512", "gmvae", 784, 64, 10, (512,), 768, "skinny", "fp32", w_form="sk_dwc"),  # the same sizes: 354 tiles
    Site("skinny-dwc-gmvae", "gmvae", 784, 64, 10, (1024,), 512, "skinny", "fp32", w_form="sk_dwc"),      # 706 tiles
    Site("skinny-dwc-vae", "vae", 784, 64, 1, (1024,), 512, "skinny", "fp32", w_form="sk_dwc"),
    Site("skinny-dwc-vae_gmp", "vae_gmp", 784, 64, 10, (1024,), 512, "skinny", "fp32", w_form="sk_dwc"),
    # ---- the general schedule's finalize_adam; marginal: count = B while the rows are B K
    Site("general-2hidden", "vae", 784, 8, 1, (96, 96), 48, "general", "fp64", hps=(1, 2, 3, 4), n3=(999,)),
    Site("general-S3", "gmvae", 300, 6, 7, (40,), 24, "general", "fp64", S=3),
    Site("general-marginal", "gmvae", 64, 6, 7, (40,), 24, "general+marginal", "fp64", y_inference="marginal"),
    # ---- the data-parallel tails behind a one-rank communicator (tests/test_timed_path.py DP_CASES' shapes)
    Site("dp-adam_tiles", "gmvae", L=64, B=1024, sched="mega2", alpha="fp64", mode="dp", trace=(1, 4, 1), n3=(999,), **G784),
    Site("dp-adam_tf_img-mega", "gmvae", L=16, B=96, sched="mega", alpha="fp64", mode="dp", trace=(1, 4, 0), n3=(999, A.T0_WRAP), **G784),
    Site("dp-adam_tf_img-mega2v", "vae", 784, 2, 1, (64,), 100, "mega2v", "fp64", mode="dp", trace=(1, 7, 1), n3=(999, A.T0_WRAP)),
    Site("dp-adam_tf_step-nofl", "gmvae", L=64, B=1024, sched="mega2", alpha="fp64", mode="dp", trace=(0, 4, 1),
         env=(("GMVAE_NO_FL", "1"),), **G784),
    # ---- eager: Engine.train_step = gmvae_step + adam_tf_step
    Site("eager-train_step", "gmvae", 784, 8, 10, (64,), 16, "mega", "fp64", mode="eager"),
]
CASES = [(s, h) for s in SITES for h in s.hps]


def _real_mask(site, P):
    """(real [P] bool, [(name, begin, end)]) of oracle.param_layout."""
    d = O.Dims(D=site.D, L=site.L, K=site.K, hidden=site.hidden, S=site.S)
    lay, P_pad, P_real = O.param_layout(O.MODEL_NAMES[site.model], d)
    assert P_pad == P
    real = np.zeros(P, bool)
    spans = []
    for name, shape, off in lay:
        n = int(np.prod(shape))
        real[off:off + n] = True
        spans.append((name, off, off + n))
    assert int(real.sum()) == P_real
    return real, spans


def _skinny_w_form(site):
    """The kernel of the skinny schedule's W stage at the site's sizes: run_skinny's launch_dw (csrc/gmvae_hip.hip) restated."""
    (H,), D, Lz, K, B = site.hidden, site.D, site.L, site.K, site.B
    if B <= 128:
        return "sk_dw"
    t = [(H, D), (Lz, H), (H, 2 * Lz)] + ([(D, H)] if site.model != "gmvae" else [(D, H), (D, H), (K, H), (H, K), (K, 2 * Lz)])
    tiles = sum(-(-M // 64) * -(-N // 64) for M, N in t)
    return "sk_dwb<1>" if tiles <= 256 else "sk_dwc" if B >= 512 else "sk_dwb<0>"


def _tensor_of(spans, i):
    return next((name for name, b, e in spans if b <= i < e), "padding")


def prepare(e, t0, real, seed):
    """Steps 1-2: the step counter (host and device) <- t0, the warm state of t0 into m and v (padding: zero)."""
    e.global_step = int(t0)
    e.step_dev.fill_(int(t0))
    m, v = A.warm_state(e.P, t0, seed)
    m[~real] = 0
    v[~real] = 0
    e.m.copy_(torch.from_numpy(m))
    e.v.copy_(torch.from_numpy(v))


def run_and_check(e, replay_one_step, hp, tag, alpha, real, spans, sched):
    """Steps 2 (snapshot) to 8 of check_site on whatever state the engine holds: replays ONE step and holds it to the statement."""
    t0 = e.global_step
    assert int(e.step_dev[0].item()) == t0, tag
    p, m, v = (a.detach().cpu().numpy().copy() for a in (e.params, e.m, e.v))
    replay_one_step()
    torch.cuda.synchronize()
    assert e.handoff_timeouts() == 0, tag
    assert e.global_step == t0 + 1 and int(e.step_dev[0].item()) == t0 + 1, (tag, e.global_step, int(e.step_dev[0].item()))
    buf = e.grads.cpu().numpy()
    g, count = buf[:e.P], float(buf[e.P + 4])
    assert count >= 1 and np.isfinite(buf[e.P]), (tag, count, buf[e.P])
    p2, m2, v2 = (a.detach().cpu().numpy() for a in (e.params, e.m, e.v))
    t = t0 + 1
    d_alpha = A.D_ALPHA_FP64 if alpha == "fp64" else A.d_alpha_fp32(t, hp[1], hp[2])
    rp, rm, rv, _ = A.predict(p, m, v, g, count, t, *hp)
    dm, dv, dp = A.bounds(p, m, v, g, count, t, *hp, d_alpha=d_alpha)
    w = []
    for got, ref, bound in ((m2, rm, dm), (v2, rv, dv), (p2, rp, dp)):
        r, i = A.worst(got[real], ref[real], bound[real])
        w.append((r, _tensor_of(spans, int(np.flatnonzero(real)[i]))))
    print(f"[adam-site] {tag} ({sched}, t = {t}, count = {count:g}): dm {w[0][0]:.3f} of its bound in {w[0][1]}, "
          f"dv {w[1][0]:.3f} in {w[1][1]}, dp {w[2][0]:.3f} in {w[2][1]}")
    for (r, name), what in zip(w, ("m'", "v'", "p'")):
        assert r <= 1.0, f"{tag}: {what} is {r:.3g} of its bound away from the fp64 statement, in {name}"
    # each element updated once, by somebody: a gradient that is not numerically nothing changed the state; no gradient and no
    # momentum: the parameter stays, bit for bit
    gj = np.abs(g.astype(np.float64)) / count
    moved = (p2 != p) | (m2 != m) | (v2 != v)
    lost = real & (gj > 1e-18) & ~moved          # (below 1e-18 gj^2 is no normal fp32 number: v' may keep its bits)
    assert not lost.any(), f"{tag}: {int(lost.sum())} elements with a gradient were not updated, the first in {_tensor_of(spans, int(np.argmax(lost)))}"
    still = real & (g == 0) & (m == 0)
    assert (p2[still] == p[still]).all(), f"{tag}: an element without gradient or momentum moved"
    assert np.isfinite(p2[~real]).all() and np.isfinite(m2[~real]).all() and np.isfinite(v2[~real]).all(), f"{tag}: padding"


def check_site(e, replay_one_step, hp, t0, tag, alpha, real, spans, sched, seed=7):
    prepare(e, t0, real, seed)
    run_and_check(e, replay_one_step, hp, tag, alpha, real, spans, sched)


def _engine(site, seed=11):
    from gmvae_amd.engine import Engine
    e = Engine(site.model, site.D, site.L, site.K, list(site.hidden), n_samples=site.S, random_seed=seed,
               y_inference=site.y_inference)
    if site.mode == "dp":
        e.rank = 3                      # as on rank 3 of a larger world: row0 = 3 B enters the Philox counters only
        e.enable_rccl()
    return e


def _batches(site, n, seed=0):
    x = (np.random.default_rng(site.B + seed).random((n, site.B, site.D)) < 0.87).astype(np.uint8)
    return torch.from_numpy(x).cuda()


def _stepper(e, site, hp, n, xs, capfd=None):
    """A callable that advances the engine by n steps on xs [n, B, D] under hp = (lr, b1, b2, eps)."""
    lr, b1, b2, eps = hp
    if site.mode == "eager":
        def run():
            for i in range(n):
                e.train_step(xs[i], lr=lr, beta1=b1, beta2=b2, epsilon=eps)
        return run
    if capfd is not None:
        capfd.readouterr()
    sx, replay = e.capture_train_step(site.B, lr=lr, all_reduce=site.mode == "dp", n_steps=n, beta1=b1, beta2=b2, epsilon=eps)
    if site.mode == "dp":
        assert e.dp_mode == "rccl-in-hipgraph", site.id
        if capfd is not None:
            import test_timed_path as T
            assert T._trace_lines(capfd) == [site.trace] * n, site.id
    sx.copy_(xs if n > 1 else xs[0])
    return replay


def _setup(site, monkeypatch):
    from gmvae_amd import _lib as L
    for k, v in site.env:
        monkeypatch.setenv(k, v)
    if site.mode == "dp":
        monkeypatch.setenv("GMVAE_TRACE", "1")
    e = _engine(site)
    sched = L.step_schedule(e.dims(site.B), e.model)
    assert sched == site.sched, (site.id, sched)
    assert (site.w_form is None) == (sched != "skinny") and (site.w_form is None or _skinny_w_form(site) == site.w_form), site.id
    real, spans = _real_mask(site, e.P)
    return e, sched, real, spans


def _release(engines):
    import test_timed_path as T
    T._release(engines)


@pytest.mark.parametrize("site,hp_id", CASES, ids=[f"{s.id}-hp{h}" for s, h in CASES])
def test_site_applies_the_update_statement(site, hp_id, capfd, monkeypatch):
    """One step of the site at every step counter of adam_ref.T0, on one engine and one captured graph."""
    hp = A.HP[hp_id]
    engines = []
    try:
        e, sched, real, spans = _setup(site, monkeypatch)
        engines.append(e)
        step = _stepper(e, site, hp, 1, _batches(site, 1), capfd)
        for t0 in A.T0:
            check_site(e, step, hp, t0, f"{site.id}-hp{hp_id}-t{t0}", site.alpha, real, spans, sched)
    finally:
        _release(engines)


N3 = [(s, h, t0) for s in SITES for h in s.hps[:2] for t0 in s.n3]


@pytest.mark.parametrize("site,hp_id,t0", N3, ids=[f"{s.id}-hp{h}-t{t0}" for s, h, t0 in N3])
def test_three_step_graph_is_the_statement_iterated(site, hp_id, t0, capfd, monkeypatch):
    """A 3-step graph from counter t0: a twin engine launches a ONE-step graph three times, each step held to the statement on
    the gradient it left; the 3-step graph -- steps 2..3 in their in-graph forms: alpha_t from the previous step's tail slot,
    the first layer from the images the optimizer scattered -- must leave the same parameters and moments bit for bit.
    t0 = 2^32 - 2: the cache tag's (unsigned)t passes through 0."""
    hp = A.HP[hp_id]
    engines = []
    try:
        e1, sched, real, spans = _setup(site, monkeypatch)
        engines.append(e1)
        xs = _batches(site, 3, seed=1)
        lr, b1, b2, eps = hp
        sx1, replay1 = e1.capture_train_step(site.B, lr=lr, all_reduce=site.mode == "dp", n_steps=1, beta1=b1, beta2=b2, epsilon=eps)
        prepare(e1, t0, real, 7)
        for i in range(3):
            sx1.copy_(xs[i])
            run_and_check(e1, replay1, hp, f"{site.id}-hp{hp_id}-t{t0}+{i}", site.alpha, real, spans, sched)
        e3 = _engine(site)
        engines.append(e3)
        step3 = _stepper(e3, site, hp, 3, xs, capfd)
        prepare(e3, t0, real, 7)
        step3()
        torch.cuda.synchronize()
        assert e3.handoff_timeouts() == 0 and int(e3.step_dev[0].item()) == t0 + 3
        for a, b, what in ((e3.params, e1.params, "parameters"), (e3.m, e1.m, "m"), (e3.v, e1.v, "v")):
            assert torch.equal(a.detach(), b.detach()), f"{site.id} hp{hp_id} t0 = {t0}: {what} of the 3-step graph and of three 1-step launches differ"
    finally:
        _release(engines)


INVALIDATION = [s for s in SITES if s.id in ("mega3_step", "mega3v_step-vae_gmp", "dp-adam_tiles", "dp-adam_tf_img-mega2v")]


@pytest.mark.parametrize("site", INVALIDATION, ids=[s.id for s in INVALIDATION])
def test_cached_alpha_is_invalidated(site, monkeypatch):
    """The cached alpha_t (mega3_step's tail slot -> lr_next / lr_dev, tagged with (unsigned)t, the bits of lr and
    alpha_key(b1, b2)) on ONE engine and ONE workspace, every step held to the statement of the graph that ran it:
      1. a graph at TF's defaults, two launches (the second may take the first's cached value);
      2. a graph at lr = 3e-4: the tag's step matches, the lr bits must not;
      3. a graph at the second hyperparameter set (lr = 3e-4 again): step and lr match, alpha_key must not;
      4. the counter rewound by 3 through load_state_dict, then a graph at TF's defaults again."""
    engines = []
    try:
        e, sched, real, spans = _setup(site, monkeypatch)
        engines.append(e)
        xs = _batches(site, 1, seed=2)
        hp1, hp2 = A.HP[1], A.HP[2]
        hp_lr = (3e-4,) + hp1[1:]
        assert hp2[0] == hp_lr[0]
        args = (site.alpha, real, spans, sched)
        step = _stepper(e, site, hp1, 1, xs)
        prepare(e, 999, real, 7)
        run_and_check(e, step, hp1, f"{site.id}-inval-1a", *args)
        run_and_check(e, step, hp1, f"{site.id}-inval-1b", *args)
        run_and_check(e, _stepper(e, site, hp_lr, 1, xs), hp_lr, f"{site.id}-inval-2-lr", *args)
        run_and_check(e, _stepper(e, site, hp2, 1, xs), hp2, f"{site.id}-inval-3-betas", *args)
        ws = {k: w.data_ptr() for k, w in e._ws.items()}
        sd = e.state_dict()
        sd["global_step"] = torch.tensor(e.global_step - 3)
        e.load_state_dict(sd)                      # (destroys the graphs; the workspace and its cached tag stay)
        assert e.global_step == 1000 and {k: w.data_ptr() for k, w in e._ws.items()} == ws
        run_and_check(e, _stepper(e, site, hp1, 1, xs), hp1, f"{site.id}-inval-4-rewound", *args)
    finally:
        _release(engines)
