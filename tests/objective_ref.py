"""The one fp64 statement of the three models' forward pass and of every per-example objective built on it, in torch with
autograd -- test infrastructure: tests/ymarg_ref.py, ymarg_iw_ref.py, dreg_ref.py, semisup_ref.py, wobj_ref.py, ytemp_ref.py and
pmask_ref.py are adapters onto loss_and_grads() here and only pick the keys their tests read.  oracle/gmvae_oracle.py (numpy, the
hand-derived backward) stays a separate implementation: tests/test_*_cpu.py hold the two against each other.

forward(): straight from the reference's call sites (scripts/gmvae.py:238-262, scripts/base.py:47-72), with these switches:
    S                    rows per example: r = b S + s; with y summed out r = (b S + s) K + k
    y                    "gumbel": y = softmax((logits + g) / tau), g = -ln(-ln u)      (gmvae.py:238-240)
                         "summed": y_r = e_k, every component of every sample
                         "leaf":   y = the LEAF e_argmax(logits + g) (no path back to the logits; o["y"].grad = d loss / d y)
    tau                  the temperature (default d.temperature);  straight_through: y = y_soft + (y_hard - y_soft).detach()
    mask                 m [B, D], observed iff non-zero: the encoders read m x (encoder_sees_mask=False: x, the WRONG variant
                         tests/test_pmask_cpu.py tells apart) and the likelihood sums the observed pixels; hid = the rest, detached
    detach_q             log q at stopped (mu, sigma), z attached: the DReG surrogate's pass
    relu_masks           per-net ReLU subgradients, as oracle.loss_and_grads takes them
The objectives are small functions of forward()'s dict o: iwae, summed_out, labelled, weighted.  Each returns dict(Lb [B], ...)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import oracle as O

LOG_2PI = math.log(2.0 * math.pi)
INFERENCE_NET = {O.MODEL_VAE: "encoder", O.MODEL_VAE_GMP: "encoder", O.MODEL_GMVAE: "encoder_gmm"}


def _act(h, act):
    if act == "relu":
        return torch.relu(h)
    if act == "tanh":
        return torch.tanh(h)
    if act == "sigmoid":
        return torch.sigmoid(h)
    if act == "elu":
        return F.elu(h)
    raise ValueError(act)


def _mlp(p, name, n_layers, x, act, masks, pres):
    """snt.nets.MLP (scripts/base.py:47-60).  masks[i] (bool, optional): the ReLU subgradient of hidden layer i to take --
    the unit passes its pre-activation where the mask is set, 0 elsewhere (differs from relu only at a pre-activation that
    is zero to within rounding).  pres receives (pre-activation, sum_k |a_k| |w_kj| + |b_j|) of every hidden layer."""
    h = x
    for i in range(n_layers):
        w, b = p[f"{name}_fcnet/linear_{i}/w"], p[f"{name}_fcnet/linear_{i}/b"]
        a = h
        h = a @ w + b
        if i < n_layers - 1:
            pres.append((h.detach().numpy(), (a.abs() @ w.abs() + b.abs()).detach().numpy()))
            m = masks[i + 1] if masks is not None and i + 1 < len(masks) and masks[i + 1] is not None else None
            if m is not None:
                assert act == "relu", "subgradient masks are a ReLU matter"
                h = torch.where(torch.as_tensor(m), h, torch.zeros_like(h))
            else:
                h = _act(h, act)
    return h


def _mvn_logprob(z, mu, sigma):
    e = (z - mu) / sigma
    return (-0.5 * e * e - 0.5 * LOG_2PI).sum(dim=1) - torch.log(sigma).sum(dim=1)


def is_inference(model, name):
    return name.startswith(INFERENCE_NET[model] + "_fcnet/")


def leaves(p):
    return {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in p.items()}


def grads_of(t):
    return {k: v.grad.numpy().copy() if v.grad is not None else np.zeros_like(v.detach().numpy()) for k, v in t.items()}


def forward(model, d, t, x, eps, S=1, y="gumbel", u=None, tau=None, straight_through=False, mask=None, encoder_sees_mask=True,
            detach_q=False, relu_masks=None):
    """One forward pass on the torch leaves t: dict of the per-row terms (logits, q, nent [B]; y, y_soft, pert = logits + g;
    mu_q, sig_q, z, logq, logp, logpx, hid, lam; lw = log w' = logpx + logp - logq, without the entropy term), qp0 (the VAE
    family's encoder output, one row per example), pre = per-net pre-activations, and B, S, K."""
    rm = relu_masks or {}
    gm = model == O.MODEL_GMVAE
    B, K, L = x.shape[0], d.K, d.L
    rpx = S * K if gm and y == "summed" else S
    nl = len(d.hidden) + 1
    c, smin = float(d.raw_sigma_bias), float(d.sigma_min)
    xf = torch.tensor(np.asarray(x), dtype=torch.float64)
    mf = None if mask is None else torch.tensor((np.asarray(mask) != 0).astype(np.float64))
    xe = mf * xf if mf is not None and encoder_sees_mask else xf
    eps = torch.tensor(np.asarray(eps, np.float64).reshape(B * rpx, L))
    pre = {n: [] for n in (("encoder_y", "encoder_gmm", "decoder") if gm else ("encoder", "decoder"))}
    o = dict(B=B, S=S, K=K, pre=pre)
    if gm:
        logits = _mlp(t, "encoder_y", nl, xe, d.act, rm.get("encoder_y"), pre["encoder_y"])            # gmvae.py:238
        logits.retain_grad()
        lnq = torch.log_softmax(logits, dim=1)
        q = lnq.exp()
        nent = (q * lnq).sum(dim=1)                                                                      # gmvae.py:262
        if y == "summed":
            yy = torch.eye(K, dtype=torch.float64).repeat(B * S, 1)                                      # row (b S + s) K + k: e_k
        else:
            ut = torch.tensor(np.asarray(u, np.float64).reshape(B * S, K))
            pert = logits.repeat_interleave(S, dim=0) - torch.log(-torch.log(ut))
            y_soft = torch.softmax(pert / float(d.temperature if tau is None else tau), dim=1)
            y_hard = F.one_hot(pert.detach().argmax(dim=1), K).to(torch.float64)                         # (the first maximal index on ties)
            if y == "leaf":
                yy = y_hard.clone().requires_grad_(True)
            elif straight_through:
                yy = y_soft + (y_hard - y_soft).detach()
            else:
                yy = y_soft
            o.update(y_soft=y_soft, pert=pert.detach())
        pp = yy @ t["prior_gmm_fcnet/linear_0/w"] + t["prior_gmm_fcnet/linear_0/b"]                      # gmvae.py:243
        qp = _mlp(t, "encoder_gmm", nl, torch.cat([xe.repeat_interleave(rpx, dim=0), yy], dim=1), d.act, rm.get("encoder_gmm"),
                  pre["encoder_gmm"])                                                                    # gmvae.py:246
        o.update(logits=logits, q=q, nent=nent, y=yy)
    else:
        qp0 = _mlp(t, "encoder", nl, xe, d.act, rm.get("encoder"), pre["encoder"])                       # [B, 2L]: one row per example
        qp0.retain_grad()
        qp = qp0.repeat_interleave(S, dim=0)
        o.update(qp0=qp0, nent=torch.zeros(B, dtype=torch.float64))
    mu_q, sig_q = qp[:, :L], torch.clamp(F.softplus(qp[:, L:] + c), min=smin)                            # base.py:66-72
    z = mu_q + sig_q * eps                                                                               # gmvae.py:248
    logq = _mvn_logprob(z, mu_q.detach(), sig_q.detach()) if detach_q else _mvn_logprob(z, mu_q, sig_q)
    if gm:
        mu_p, sig_p = pp[:, :L], torch.clamp(F.softplus(pp[:, L:] + c), min=smin)
        logp = _mvn_logprob(z, mu_p, sig_p)                                                              # gmvae.py:258
    elif model == O.MODEL_VAE:
        logp = (-0.5 * z * z - 0.5 * LOG_2PI).sum(dim=1)
    else:
        loc, s = t["loc"], F.softplus(t["raw_scale_diag"])
        lnw = torch.log_softmax(t["mixture_logits"], dim=0)
        tt = (z[:, None, :] - loc[None]) / s[None]
        lnN = (-0.5 * tt * tt - 0.5 * LOG_2PI).sum(dim=2) - torch.log(s).sum(dim=1)[None]
        logp = torch.logsumexp(lnw[None] + lnN, dim=1)
    lam = _mlp(t, "decoder", nl, z, d.act, rm.get("decoder"), pre["decoder"])                            # gmvae.py:251
    lam = lam + torch.as_tensor(np.asarray(d.gen_bias_init, np.float64))
    el = xf.repeat_interleave(rpx, dim=0) * lam - F.softplus(lam)                                        # gmvae.py:254
    if mf is None:
        logpx = el.sum(dim=1)
    else:
        mr = mf.repeat_interleave(rpx, dim=0)
        logpx = (mr * el).sum(dim=1)
        o.update(hid=((1.0 - mr) * el).sum(dim=1).detach(), n_missing=float((1.0 - mf).sum().item()),
                 n_observed=float(mf.sum().item()))
    o.update(mu_q=mu_q, sig_q=sig_q, z=z, logq=logq, logp=logp, logpx=logpx, lam=lam, lw=logpx + logp - logq)
    return o


# ---- the per-example objectives: o -> dict(Lb [B], and what the estimators and the tests read)
def iwae(o):
    """L_b = -(logsumexp_s log w_bs - ln S), log w_r = log w'_r - nent_b (rows b S + s; S = 1: the ELBO).  v = w = softmax_s."""
    B, S = o["B"], o["S"]
    logw = o["lw"] - o["nent"].repeat_interleave(S)
    v = torch.softmax(o["lw"].view(B, S), dim=1).reshape(-1)
    return dict(Lb=-(torch.logsumexp(logw.view(B, S), dim=1) - math.log(S)), logw=logw, v=v, w=v)


def summed_out(o):
    """y summed out: l_bk = -(logsumexp_s log w'_bsk - ln S), L_b = sum_k q_bk l_bk + nent_b; v = softmax_s(log w') of the row's
    own group, w = q_bk v the step's row weight."""
    B, S, K = o["B"], o["S"], o["K"]
    lw = o["lw"].view(B, S, K)
    ell = -(torch.logsumexp(lw, dim=1) - math.log(S))
    v = torch.softmax(lw, dim=1)
    return dict(Lb=(o["q"] * ell).sum(dim=1) + o["nent"], ell=ell, v=v.reshape(-1), w=(o["q"][:, None, :] * v).reshape(-1),
                wk=o["q"].detach())


def labelled(o, y_observed, alpha):
    """summed_out for the unlabelled examples; c_b in [0, K): L_b = l_bc + alpha (-ln q_bc), row weights [k == c] v."""
    B, S, K = o["B"], o["S"], o["K"]
    c = torch.as_tensor(np.asarray(y_observed).astype(np.int64).reshape(B))
    lab = (c >= 0) & (c < K)
    cc = torch.where(lab, c, torch.zeros_like(c))
    onehot = F.one_hot(cc, K).double() * lab[:, None].double()                                # zero rows where unlabelled
    lnq = torch.log_softmax(o["logits"], dim=1)
    lw = o["lw"].view(B, S, K)
    ell = -(torch.logsumexp(lw, dim=1) - math.log(S))
    ce_b = -(onehot * lnq).sum(dim=1)                                                         # 0 where unlabelled
    L_unl = (o["q"] * ell).sum(dim=1) + o["nent"]
    L_lab = (onehot * ell).sum(dim=1) + alpha * ce_b
    wk = torch.where(lab[:, None], onehot, o["q"].detach())                                   # the component weights [B, K]
    v = torch.softmax(lw.detach(), dim=1)
    return dict(Lb=torch.where(lab, L_lab, L_unl), ell=ell, v=v.reshape(-1), w=(wk[:, None, :] * v).reshape(-1), wk=wk, lab=lab,
                c=c, ce_b=ce_b)


def weighted(o, weights, marginal=False):
    """S = 1: L_b = nll_b + beta_z kl_b + beta_y max(nent_b, lambda - ln K) (GMVAE; lambda == 0: no floor, whatever the
    rounding); marginal: nll_b, kl_b = sum_k q_bk (.)_bk."""
    B, K = o["B"], o["K"]
    assert o["S"] == 1
    bz, by, lam = (float(w) for w in weights)
    nent = o["nent"]
    nll_b, kl_b = -o["logpx"], o["logq"] - o["logp"]
    if marginal:
        nll_b, kl_b = (o["q"] * nll_b.view(B, K)).sum(dim=1), (o["q"] * kl_b.view(B, K)).sum(dim=1)
    Lb = nll_b + bz * kl_b
    floor = np.zeros(B)
    if "q" in o:
        thr = lam - math.log(K)
        if lam == 0.0:
            nef = nent
        else:
            nef = torch.clamp(nent, min=thr)                       # (autograd through the max: no gradient below the floor)
            floor = (nent.detach().numpy() <= thr).astype(np.float64)
        Lb = Lb + by * nef
    return dict(Lb=Lb, nll_b=nll_b, kl_b=kl_b, floor=floor)


def loss_and_grads(model, d, p, x, eps, objective=iwae, S=1, estimator="standard", **switches):
    """loss = mean_b objective(forward(...))["Lb"].  Returns (C, g): g = {name: d loss / d param} (float64 numpy); C = the
    forward's dict and the objective's, tensors detached, plus loss, dlogits [B, K] = d loss / d logits (GMVAE), dqp [B, 2L]
    (VAE family), dmu, dsig [rows, L] = d (B loss) / d (mu_q, sigma_q), dy = d loss / d y (y="leaf").
    estimator="dreg" (Tucker et al. 2018), stated by stop-gradients: the inference net's gradients (and dmu, dsig, dqp) are those
    of  sum_rows (w v).detach() (-log w'_row) / B  on a second forward with detach_q=True; everything else is the true loss's."""
    assert estimator in ("standard", "dreg")
    B = x.shape[0]
    gm = model == O.MODEL_GMVAE

    def run(detach_q):
        t = leaves(p)
        o = forward(model, d, t, x, eps, S=S, detach_q=detach_q, **switches)
        o["mu_q"].retain_grad()
        o["sig_q"].retain_grad()
        return t, o

    t, o = run(False)
    ob = objective(o)
    loss = ob["Lb"].mean()
    loss.backward()
    g = grads_of(t)
    C = {k: v.detach() if isinstance(v, torch.Tensor) else v for k, v in {**o, **ob}.items()}
    C.update(loss=loss.item(), dlogits=o["logits"].grad.numpy().copy() if gm else None,
             dy=o["y"].grad.numpy().copy() if switches.get("y") == "leaf" else None)
    if estimator == "dreg":
        t2, o2 = run(True)
        sur = ((ob["w"] * ob["v"]).detach() * (-o2["lw"])).sum() / B
        sur.backward()
        for k in g:
            if is_inference(model, k):
                g[k] = t2[k].grad.numpy().copy()
        o = o2
    C.update(dmu=o["mu_q"].grad.numpy() * B, dsig=o["sig_q"].grad.numpy() * B, dqp=None if gm else o["qp0"].grad.numpy() * B)
    return C, g


def row_terms(C):
    """rows [R, 4] = logpx, logq, logp, log w' (numpy)."""
    return torch.stack([C["logpx"], C["logq"], C["logp"], C["lw"]], dim=1).numpy()


def summed_means(C, wk):
    """(nll, kl) batch means with y summed out: component weights wk [B, K], the mean over s."""
    B, S, K = C["B"], C["S"], C["K"]
    return ((wk * (-C["logpx"]).view(B, S, K).mean(dim=1)).sum().item() / B,
            (wk * (C["logq"] - C["logp"]).view(B, S, K).mean(dim=1)).sum().item() / B)
