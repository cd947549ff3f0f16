"""-m gpu: the one-launch step with its first-layer addresses handed over as leading scalar kernel parameters (csrc/mega2.hpp
M2_HEAD_PARAMS: w0a, w0b, x, img2f, the control block, the step counter, B and the diagnostic bits arrive in SGPRs at wave start; the
start state -- hand-off tag, error word, step counter, alpha_t's tag -- is read through them by the kernel's first instructions).

mega2_fwd_bwd and mega3_step share one body and take the same head, so the head is checked where a wrong value shows:
  1. GMVAE_FUSE=1 against GMVAE_NO_FUSE=1 -- parameters, both moments and the gradient sums bit for bit after 6 steps, at B = 1024,
     1000 (a ragged last wave), 48 (an odd panel count: a phantom panel's workgroups leave behind the first layer; workgroups run
     more than one slot) and 32;
  2. the same for the VAE family (the build flag is translation-unit wide; their kernels take no head);
  3. two graphs on one workspace with different lr, beta1, beta2 and a rewound step counter, 3 steps each: every step of the second
     graph is held to tests/adam_ref.py -- what a head that carried a per-step value (the counter, alpha_t's tag) over from an
     earlier capture would fail;
  4. the data-parallel one-rank graph (mega3_step's gradient-only form, the all-reduce, adam_tiles) against the single-device graph,
     bit for bit after 4 steps."""
import numpy as np
import pytest
import torch

import adam_ref as A
import hip_util as HU

pytestmark = pytest.mark.gpu

LR = 1e-3


def _batches(B, n, seed=0):
    return torch.from_numpy((np.random.default_rng(B + seed).random((n, B, 784)) < 0.87).astype(np.uint8)).cuda()


def _fused_and_two_launch(model, Lz, K, B, monkeypatch, force):
    """[(params, m, v, grads, level names)] of 6 steps (two launches of a 3-step graph) in the one-launch and the two-launch form."""
    from gmvae_amd.engine import Engine
    import test_timed_path as T
    xs = _batches(B, 3)
    res, engines = [], []
    try:
        for fused in (True, False):
            if fused:
                monkeypatch.delenv("GMVAE_NO_FUSE", raising=False)
                if force:
                    monkeypatch.setenv("GMVAE_FUSE", "1")
            else:
                monkeypatch.setenv("GMVAE_NO_FUSE", "1"); monkeypatch.delenv("GMVAE_FUSE", raising=False)
            e = Engine(model, 784, Lz, K, [64], random_seed=5)
            engines.append(e)
            sx, replay = e.capture_train_step(B, LR, n_steps=3)
            sx.copy_(xs)
            replay(); replay()
            torch.cuda.synchronize()
            assert e.handoff_timeouts() == 0 and int(e.step_dev[0].item()) == 6
            st = T._state(e)
            names = [nm for nm, *_ in e.profile_train_levels(xs[0], lr=LR, iters=1)]
            res.append(st + (names,))
    finally:
        T._release(engines)
    return res


def _same(res, what):
    assert torch.isfinite(res[0][0]).all(), what
    for a, b, nm in zip(res[0][:4], res[1][:4], ("parameters", "m", "v", "gradient sums")):
        assert torch.equal(a, b), f"{what}: {nm} of the one-launch and the two-launch form differ"


@pytest.mark.parametrize("B", [1024, 1000, 48, 32])
def test_one_launch_gmvae_step_equals_two_launch_step(B, monkeypatch):
    res = _fused_and_two_launch("gmvae", 64, 10, B, monkeypatch, force=True)
    assert res[0][4] == ["mega3_step"] and res[1][4] == ["mega2_fwd_bwd", "dw_adam"], (res[0][4], res[1][4])
    _same(res, f"gmvae B = {B}")


@pytest.mark.parametrize("model,Lz,K,B", [("vae", 2, 1, 100), ("vae_gmp", 64, 10, 256)])
def test_one_launch_vae_family_step_equals_two_launch_step(model, Lz, K, B, monkeypatch):
    res = _fused_and_two_launch(model, Lz, K, B, monkeypatch, force=False)
    assert res[0][4] == ["mega3v_step"] and res[1][4] == ["mega2v_fwd_bwd", "dw_adam"], (res[0][4], res[1][4])
    _same(res, f"{model} B = {B}")


def test_second_graph_on_one_workspace_takes_its_own_rates_and_counter(monkeypatch):
    import test_optimizer_sites as S
    site = next(s for s in S.SITES if s.id == "mega3_step")
    engines = []
    try:
        e, sched, real, spans = S._setup(site, monkeypatch)
        engines.append(e)
        xs = S._batches(site, 1, seed=3)
        hp1, hp2 = A.HP[1], A.HP[2]
        assert hp1[0] != hp2[0] and hp1[1] != hp2[1] and hp1[2] != hp2[2]
        args = (site.alpha, real, spans, sched)
        step1 = S._stepper(e, site, hp1, 1, xs)
        S.prepare(e, 999, real, 7)
        for i in range(3):
            S.run_and_check(e, step1, hp1, f"cold-start-graph1+{i}", *args)
        ws = {k: w.data_ptr() for k, w in e._ws.items()}
        sd = e.state_dict()
        sd["global_step"] = torch.tensor(e.global_step - 2)      # rewound: the cached alpha_t's tag names a later step
        e.load_state_dict(sd)
        assert e.global_step == 1000 and {k: w.data_ptr() for k, w in e._ws.items()} == ws
        step2 = S._stepper(e, site, hp2, 1, xs)
        for i in range(3):
            S.run_and_check(e, step2, hp2, f"cold-start-graph2+{i}", *args)
    finally:
        S._release(engines)


def test_data_parallel_one_rank_graph_equals_single_device_graph():
    import test_timed_path as T
    HU.need_rccl()
    B, n = 1024, 4
    xs = _batches(B, n, seed=1)
    engines, st = [], []
    try:
        for rccl in (True, False):
            e = T._dp_engine("gmvae", 784, 64, 10, (64,), 1, 8, 3, False, rccl=rccl)
            engines.append(e)
            sx, replay = e.capture_train_step(B, lr=LR, all_reduce=rccl, n_steps=n)
            if rccl:
                assert e.dp_mode == "rccl-in-hipgraph", e.dp_mode
            sx.copy_(xs)
            replay()
            torch.cuda.synchronize()
            assert e.handoff_timeouts() == 0 and int(e.step_dev[0].item()) == n
            st.append(T._state(e))
        assert T._bit_equal(st[0], st[1]), "the one-rank data-parallel graph and the single-device graph differ"
    finally:
        T._release(engines)
