"""The parity cases of gmvae_simulate and gmvae_ais_reverse (tests/test_bdmc.py), their models and their Philox keys -- apart from
the tests so that tests/test_bdmc_cpu.py can hold the CONDITIONS of every case (undecided chains, pixels at their threshold,
component picks at a CDF edge, acceptance rate) to the fp64 statement alone, on the CPU restatement of the device's noise."""
import numpy as np

import oracle as O

MODELS = {"vae": O.MODEL_VAE, "vae_gmp": O.MODEL_VAE_GMP, "gmvae": O.MODEL_GMVAE}
SEED, STEP, STEP_REV = 7, 3, 5         # the simulation's key (SEED, STEP) and the reverse chains' (SEED, STEP_REV)
SMALL = dict(T=8, leap=3)
STEP0 = 0.5

# (model, init, act, D, L, K, hidden, B, C[, T, n_leapfrog]): tests/test_ais.py's shapes -- D = 23 carries gen_bias_vec; B C = 3 x 5 is
# one ragged panel that spans examples, 4 x 16 four panels
CASES = [
    ("gmvae", "prior", "relu", 24, 3, 4, (16,), 4, 16),
    ("gmvae", "encoder", "tanh", 23, 5, 3, (12, 20), 3, 5),
    ("gmvae", "encoder", "relu", 23, 3, 4, (), 3, 5),
    ("gmvae", "prior", "tanh", 24, 5, 4, (), 4, 16),
    ("vae", "prior", "relu", 23, 5, 1, (12, 20), 4, 16),
    ("vae", "encoder", "tanh", 24, 3, 1, (16,), 3, 5),
    ("vae_gmp", "prior", "tanh", 23, 3, 4, (16,), 3, 5),
    ("vae_gmp", "encoder", "relu", 24, 5, 3, (12, 20), 4, 16),
    ("gmvae", "encoder", "elu", 23, 5, 3, (16,), 3, 5),
    ("vae_gmp", "prior", "sigmoid", 24, 3, 4, (12, 20), 3, 5),
    # every size gate's last admitted corner at once (and the largest LDS layout): 3 x 512, L = 128, K = base_K = 64
    ("gmvae", "encoder", "tanh", 23, 128, 64, (512, 512, 512), 2, 3, 2, 2),
    # D off a multiple of 4 and of the 128-column pass, hidden 512, L = 128
    ("vae_gmp", "prior", "relu", 787, 128, 10, (512,), 1, 5, 2, 2),
    # the reference's defaults, from both bases
    ("gmvae", "prior", "relu", 784, 64, 10, (64,), 2, 16, 2, 2),
    ("gmvae", "encoder", "relu", 784, 64, 10, (64,), 2, 16, 2, 2),
    # the gates' lower corners: one pixel; one pixel, one latent dimension, one component, one hidden unit
    ("vae", "prior", "tanh", 1, 3, 1, (16,), 3, 5),
    ("vae_gmp", "encoder", "tanh", 1, 1, 1, (1,), 3, 5),
]
cid = lambda c: "-".join(str(v).replace(" ", "") for v in c)


def unpack_case(case):
    """(model id, Dims, init, B, C, T, n_leapfrog, explicit T?)"""
    name, init, act, D, Lz, K, hidden, B, C_ = case[:9]
    T, leap = case[9:] if len(case) > 9 else (SMALL["T"], SMALL["leap"])
    d = O.Dims(D=D, L=Lz, K=K, hidden=hidden, act=act, gen_bias_init=np.linspace(-0.5, 0.5, D).astype(np.float32) if D == 23 else 0.1)
    return MODELS[name], d, init, B, C_, T, leap, len(case) > 9


def make(model, d, seed, scale=2.0):
    """Xavier weights times `scale`, small random biases: (params fp32-exact as float64, flat fp32)."""
    rng = np.random.default_rng(seed)
    p = {k: scale * v for k, v in O.init_params(model, d, rng).items()}
    for k in p:
        if k.endswith("/b"):
            p[k] = 0.1 * rng.standard_normal(p[k].shape)
    flat = O.pack(model, d, p)
    return {k: v.astype(np.float64) for k, v in O.unpack(model, d, flat).items()}, flat


def case_model(case):
    model, d = unpack_case(case)[:2]
    return make(model, d, 2000 + CASES.index(case))


def cpu_sim_noise(B, d, row0=0, seed=SEED, step=STEP):
    """gmvae_simulate's draws restated on the CPU (oracle.noise): eps [B, L], u [B], ux [B, D]."""
    eps, u = O.noise(B, d.L, 1, row0, seed, 2 * step)
    _, ux = O.noise(B, 1, d.D, row0, seed, 2 * step + 1)
    return eps, u.reshape(B), ux


def cpu_chain_noise(T, n, Lz, row_base=0, seed=SEED, step=STEP_REV):
    """gmvae_ais_reverse's draws restated on the CPU: eps [T + 1, n, L], u [T + 1, n] (slot 0 unused)."""
    es, us = zip(*(O.noise(n, Lz, 1, row_base, seed, step * (T + 1) + t) for t in range(T + 1)))
    return np.stack(es), np.stack(us).reshape(T + 1, n)
