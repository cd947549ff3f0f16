"""Regenerates tests/golden/launch_names_parent.json on a device (from the repo root: ``python tests/golden/make_launch_names.py``):
the ordered launch names the measurement hooks report (iters = 1), and the device's compute-unit count, over

  step    Engine.profile_levels (one eager step) at every `step` corner of tests/gate_corners.py under its switches, one
          general-schedule case per objective / estimator / optimizer bit (BITS), the forced plane case;
  train   Engine.profile_train_levels (the steady-state step of a train graph) at every `train` corner, and under
          GMVAE_NO_FUSE=1, GMVAE_NO_FL=1 and GMVAE_SCHED_SAFE;
  skinny  Engine.profile_skinny_levels at two skinny corners;
  fwd     Engine.profile_forward at the `evalf` corners and on either side of the forward pairs' 8192-row gate;
  dp      Engine.profile_dp_step with a one-rank communicator (the gradient launches), also under GMVAE_NO_ADAM_TILES=1.

The committed file was written by the library as it stood BEFORE the schedule decision was folded into plan_step
(profiles/schedule_plan_notes.md); tests/test_schedule_plan.py holds every later build to it.  Cases whose batch follows the
compute-unit count (`edge`) are comparable only on a device with the recorded count.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "launch_names_parent.json")
SWITCHES = ("GMVAE_NO_MEGA", "GMVAE_NO_FUSED", "GMVAE_NO_MEGA2", "GMVAE_NO_SKINNY", "GMVAE_NO_EVALF", "GMVAE_NO_PLANES",
            "GMVAE_PLANES_MINROWS", "GMVAE_PLANES_EXACT", "GMVAE_MEGA_Q", "GMVAE_SKINNY_MAXB", "GMVAE_NO_FL", "GMVAE_NO_FUSE",
            "GMVAE_FUSE", "GMVAE_NO_ADAM_TILES", "GMVAE_NO_RWS")
# one general-schedule case per bit, at the smallest shape of its feature test: (id, model, D, L, K, hidden, S, B, Engine options)
BITS = [("bit-marginal", "gmvae", 64, 8, 5, (32,), 1, 24, dict(y_inference="marginal")),
        ("bit-marginal_iw", "gmvae", 64, 8, 5, (32,), 2, 24, dict(y_inference="marginal_iw")),
        ("bit-labels", "gmvae", 64, 8, 5, (32,), 1, 24, dict(y_inference="marginal", semi_supervised=True)),
        ("bit-dreg", "vae", 64, 8, 1, (32,), 2, 24, dict(grad_estimator="dreg")),
        ("bit-weights", "gmvae", 64, 8, 5, (32,), 1, 24, dict(weighted_objective=True)),
        ("bit-temp", "gmvae", 64, 8, 5, (32,), 1, 24, dict(temperature_on_device=True)),
        ("bit-st", "gmvae", 64, 8, 5, (32,), 1, 24, dict(y_estimator="straight_through")),
        ("bit-mask", "gmvae", 64, 8, 5, (32,), 1, 24, dict(pixel_mask=True)),
        ("bit-clip", "gmvae", 64, 8, 5, (32,), 1, 24, dict(clip_norm=1.0))]


def cases():
    """[dict(id, hook, model, D, L, K, hidden, S, B, env, edge, opts, safe)] -- B = None: gate_corners.batch_on on the device."""
    sys.path.insert(0, os.path.dirname(HERE))
    import gate_corners as G
    out = []

    def add(id, hook, model, D, Lz, K, hidden, S, B, env=(), edge=None, opts=None, safe=False, corner=None):
        out.append(dict(id=id, hook=hook, model=model, D=D, L=Lz, K=K, hidden=list(hidden), S=S, B=B, env=dict(env), edge=edge,
                        opts=opts or {}, safe=safe, corner=corner))

    def corner(c, hook, id=None, env=(), **kw):
        add(id or f"{hook}:{c.id}", hook, c.model, c.d.D, c.d.L, c.d.K, c.d.hidden, c.d.S, None if c.edge else c.B,
            tuple(c.env) + tuple(env), c.edge, corner=c.id, **kw)

    for c in G.CORNERS:
        corner(c, {"step": "step", "train": "train", "evalf": "fwd"}[c.kind])
    for id, model, D, Lz, K, hidden, S, B, opts in BITS:
        add(id, "step", model, D, Lz, K, hidden, S, B, opts=opts)
    add("planes-S4", "step", "gmvae", 256, 64, 10, (128,), 4, 64, env=(("GMVAE_PLANES_MINROWS", "128"),))
    for cid in ("skinny-H64", "skinny-B129"):
        corner(G.BY_ID[cid], "skinny")
    for B in (8064, 8192):                                    # fwd_pairs_ok: R >= 8192 rows of 128-row tiles
        add(f"fwd-pairs-B{B}", "fwd", "vae", 64, 8, 1, (64,), 1, B)
    t1024, mega = G.BY_ID["train-gmvae-B1024"], G.BY_ID["train-gmvae-D896"]
    corner(t1024, "train", "train-NO_FUSE", env=(("GMVAE_NO_FUSE", "1"),))
    corner(t1024, "train", "train-NO_FL", env=(("GMVAE_NO_FL", "1"),))
    corner(t1024, "train", "train-SCHED_SAFE", safe=True)
    corner(t1024, "dp")
    corner(mega, "dp")
    corner(t1024, "dp", "dp-NO_ADAM_TILES", env=(("GMVAE_NO_ADAM_TILES", "1"),))
    assert len({c["id"] for c in out}) == len(out)
    return out


def compute_units():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def run_case(c, cus):
    """The launch names of one case on the current device, under exactly its switches."""
    import numpy as np
    import torch
    sys.path.insert(0, os.path.dirname(HERE))
    import gate_corners as G
    from gmvae_amd.engine import Engine
    from gmvae_amd._lib import GmvaeError
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(c["env"])
    e = None
    try:
        B = c["B"] if c["B"] is not None else G.batch_on(G.BY_ID[c["corner"]], cus)
        e = Engine(c["model"], c["D"], c["L"], c["K"], c["hidden"], n_samples=c["S"], random_seed=3, **c["opts"])
        if c["safe"]:
            e.use_safe_schedule()
        x = torch.from_numpy((np.random.default_rng(1).random((B, c["D"])) < 0.87).astype(np.uint8)).cuda()
        if c["hook"] == "step":
            names = [lv[0] for lv in e.profile_levels(x, iters=1)]
        elif c["hook"] == "train":
            names = [lv[0] for lv in e.profile_train_levels(x, iters=1)]
        elif c["hook"] == "skinny":
            lv = e.profile_skinny_levels(x, n_steps=2, launches=1)
            names = None if lv is None else [r[0] for r in lv]
        elif c["hook"] == "fwd":
            names = [lv[0] for lv in e.profile_forward(x, iters=1)[0]]
        else:
            e.enable_rccl()
            names = e.profile_dp_step(x, iters=1)["grad_launches"]
        torch.cuda.synchronize()
        return names
    except GmvaeError as ex:                                  # a return code of the library: part of the record
        return f"ERROR {ex}"
    finally:
        if e is not None:
            e.drop_graphs(clear_handoff_errors=False)
        for k in SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    cus = compute_units()
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    names = {}
    for c in cases():
        names[c["id"]] = run_case(c, cus)                      # (a device error ends the run)
        print(c["id"], names[c["id"]], flush=True)
    with open(path, "w") as f:
        f.write("{\n" + f' "compute_units": {cus},\n "names": {{\n')
        f.write(",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in names.items()))
        f.write("\n }\n}\n")
    print(f"{path}: {len(names)} cases on {cus} compute units")
