"""fp64 statement of the objective under a per-example observation mask (include/gmvae_hip.h GMVAE_OBJ_PIXEL_MASK), in torch
with autograd -- test infrastructure, the checker of tests/test_pmask*.py.

m_bd in {0, 1} (observed iff non-zero), rows r = b S + s:
    the networks that read x (encoder_y, encoder_gmm, encoder) read x~ = m x               (zero imputation)
    logpx_r = sum_d m_bd (x_bd lambda_rd - softplus lambda_rd)                              (observed pixels)
    hid_r   = sum_d (1 - m_bd)(x_bd lambda_rd - softplus lambda_rd)                         (held out: detached, not in the loss)
    log w_r = logpx_r + logp_r - logq_r - nent_b,   L_b = -(logsumexp_s log w_bs - ln S)    (oracle.forward's, on the masked logpx)
Parameters as oracle.unpack gives them; per-net ReLU masks as oracle.loss_and_grads takes them.  The module also holds the
mask recipe and the shapes of the device tests."""
import dataclasses

import numpy as np

import objective_ref as OR
import oracle as O


def loss_and_grads(model, d: O.Dims, p, x, eps, u=None, mask=None, relu_masks=None, encoder_sees_mask=True):
    """model: oracle.MODEL_*; x uint8 [B, D]; eps [B S, L]; u [B S, K] (GMVAE only); mask uint8 / bool [B, D] (None: all observed).
    encoder_sees_mask=False is the WRONG variant "likelihood masked, encoder fed the unmasked x" (tests/test_pmask_cpu.py shows
    that the gates tell it apart).  Returns (C, g): C = dict(loss, nll, kl, nent -- batch means, nll / kl averaged over s --,
    hid = sum_b mean_s(-hid_bs), n_missing, n_observed, rows [R, 4] = logpx, logq, logp, log w, bound [B], pre = per-net
    pre-activations) and g = {name: d loss / d param} (loss = mean_b L_b), all float64 numpy."""
    B, S = x.shape[0], d.S
    kw = dict(u=u) if model == O.MODEL_GMVAE else {}
    c, g = OR.loss_and_grads(model, d, p, x, eps, OR.iwae, S=S, mask=np.ones(x.shape) if mask is None else mask,
                             encoder_sees_mask=encoder_sees_mask, relu_masks=relu_masks, **kw)
    C = {"loss": c["loss"], "nll": -c["logpx"].mean().item(), "kl": (c["logq"] - c["logp"]).mean().item(),
         "nent": c["nent"].mean().item(), "hid": -c["hid"].view(B, S).mean(dim=1).sum().item(), "n_missing": c["n_missing"],
         "n_observed": c["n_observed"], "bound": -c["Lb"].numpy(), "pre": c["pre"],
         "rows": OR.row_terms({**c, "lw": c["logw"]})}
    return C, g


# ---- the mask recipe of every case
RATE = 0.3                       # each pixel missing independently at this rate, then the four conditions are forced


def dead_columns(D):
    """The two columns missing in EVERY row: the last one and one inside the first column quad."""
    return (2 % D, D - 1) if D > 2 else (D - 1,)


def live_column(D):
    """The column observed from row 2 on."""
    return 1 if D > 3 else 0


def make_mask(B, D, seed=77, single_pixel_row=None):
    """uint8 [B, D], 1 = observed.  Drawn at RATE from `seed`, then: row 0 observes nothing; row 1 everything but the dead
    columns; the dead columns are missing in every row; live_column(D) is observed from row 2 on.  single_pixel_row (>= 2): that
    row observes live_column(D) alone."""
    assert B >= 3
    m = (np.random.default_rng(seed).random((B, D)) >= RATE).astype(np.uint8)
    m[1, :] = 1
    m[2:, live_column(D)] = 1
    if single_pixel_row is not None:
        assert single_pixel_row >= 2
        m[single_pixel_row, :] = 0
        m[single_pixel_row, live_column(D)] = 1
    m[:, list(dead_columns(D))] = 0
    m[0, :] = 0
    return m


def check_mask(m):
    """The recipe's four conditions (tests/test_pmask_cpu.py asserts them for every case)."""
    B, D = m.shape
    dead = list(dead_columns(D))
    assert m[0].sum() == 0
    assert (m[:, dead] == 0).all() and len(dead) >= 2 and D - 1 in dead
    assert m[1].sum() == D - len(dead)
    assert (m[2:, live_column(D)] == 1).all()
    assert live_column(D) not in dead


def flip_missing(x, m):
    """x with every missing pixel flipped: what the device tests feed, so that any use of x there shows."""
    return np.where(m != 0, x, 1 - x).astype(np.uint8)


# ---- the shapes of tests/test_pmask.py: (model name, Dims, B) and the options of setup()
@dataclasses.dataclass(frozen=True)
class Case:
    mname: str
    d: object
    B: int
    bias_vec: bool = False       # gen_bias_init as a [D] vector (GmvaeDims::gen_bias_vec)
    lam_scale: float = None      # the decoder's last layer scaled so that max |lambda| is about this
    single_pixel_row: int = None


CASES = {
    "vae": Case("vae", O.Dims(D=100, L=5, K=1, hidden=(24,)), 9),
    "vae_gmp": Case("vae_gmp", O.Dims(D=100, L=5, K=3, hidden=(24,), sigma_min=0.5), 9),
    "gumbel": Case("gmvae", O.Dims(D=100, L=5, K=7, hidden=(24, 24), temperature=0.7), 8),
    "gmvae-s3": Case("gmvae", O.Dims(D=96, L=4, K=6, hidden=(16,), S=3), 4),
    "vae-s3": Case("vae", O.Dims(D=96, L=4, K=1, hidden=(16,), S=3), 4),
    "gumbel-d99": Case("gmvae", O.Dims(D=99, L=5, K=7, hidden=(24,)), 5),                  # unaligned rows: the element path
    # B = 16: no 32-row tile is whole, so every tile of the logits launch goes element by element (24 full column tiles + the
    # 16-column last one); the masked interior block and its predicated last column tile run in tests/test_epilogue_forms.py
    "gumbel-784": Case("gmvae", O.Dims(D=784, L=64, K=10, hidden=(64,)), 16),
    "vae_gmp-tanh": Case("vae_gmp", O.Dims(D=100, L=5, K=3, hidden=(24,), act="tanh"), 9),
    "gumbel-bias-vec": Case("gmvae", O.Dims(D=100, L=5, K=7, hidden=(24,)), 8, bias_vec=True),
    "vae-saturated": Case("vae", O.Dims(D=100, L=5, K=1, hidden=(24,)), 9, lam_scale=60.0, single_pixel_row=3),
}


def setup(name, seed=0):
    """(model id, Dims, p as the device sees it, flat fp32, x with the missing pixels flipped, eps, u, mask, the unflipped x)."""
    c = CASES[name]
    model = O.MODEL_NAMES[c.mname]
    d = c.d
    rng = np.random.default_rng(seed)
    if c.bias_vec:
        d = dataclasses.replace(d, gen_bias_init=np.linspace(-1.5, 1.5, d.D).astype(np.float32))
    p = O.init_params(model, d, rng)
    x, eps, u = O.make_inputs(d, c.B, model)
    m = make_mask(c.B, d.D, single_pixel_row=c.single_pixel_row)
    if c.lam_scale:
        nl = len(d.hidden)
        wn, bn = f"decoder_fcnet/linear_{nl}/w", f"decoder_fcnet/linear_{nl}/b"
        z = _decoder_logits(model, d, p, x, eps, u, m)
        f = c.lam_scale / np.abs(z).max()
        p = dict(p)
        p[wn], p[bn] = p[wn] * f, p[bn] * f
    flat = O.pack(model, d, p, np.float32)
    p32 = O.unpack(model, d, flat.astype(np.float64))
    return model, d, p32, flat, flip_missing(x, m), eps, (u if model == O.MODEL_GMVAE else None), m, x


def _decoder_logits(model, d, p, x, eps, u, m):
    """The decoder's logits of the masked forward (the networks that read x see m x)."""
    kw = dict(u=u) if model == O.MODEL_GMVAE else {}
    return OR.forward(model, d, OR.leaves(p), x, eps, S=d.S, mask=m, **kw)["lam"].detach().numpy()
