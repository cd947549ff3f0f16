"""Regenerates tests/golden/schedule_table.json (run from the repo root: ``python tests/golden/make_schedule_table.py``): what
gmvae_step_schedule answers -- the schedule string, or its negative return code -- and gmvae_workspace_bytes, over

  every corner of tests/gate_corners.py whose batch does not follow the compute-unit count, under its own switches, and the
    EXTRA shapes below (mega2v at batches any device admits, one plane-eligible shape);
  x no bit, every objective / estimator / optimizer bit alone, and the pairs the feature tests use (FLAG_SETS);
  x no further switch, each switch of gate_corners.SWITCHES alone, GMVAE_NO_PLANES, GMVAE_SCHED_SAFE (VARIANTS), and
    GMVAE_PLANES_MINROWS=128 at the plane-eligible shape.

The committed file was written by the library as it stood BEFORE the schedule decision was folded into plan_step
(profiles/schedule_plan_notes.md); tests/test_schedule_plan_cpu.py holds every later build to it.  Neither entry point needs a
device.  Run this again only when a change is MEANT to move a gate or the workspace layout.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "schedule_table.json")

ALL_SWITCHES = ("GMVAE_NO_MEGA", "GMVAE_NO_FUSED", "GMVAE_NO_MEGA2", "GMVAE_NO_SKINNY", "GMVAE_NO_EVALF", "GMVAE_NO_PLANES",
                "GMVAE_PLANES_MINROWS", "GMVAE_PLANES_EXACT", "GMVAE_MEGA_Q", "GMVAE_SKINNY_MAXB", "GMVAE_NO_FL", "GMVAE_NO_FUSE",
                "GMVAE_FUSE")
# (name, environment on top of the corner's own, sched_flags on top of the case's)
VARIANTS = [("-", {}, 0), ("NO_MEGA", {"GMVAE_NO_MEGA": "1"}, 0), ("NO_FUSED", {"GMVAE_NO_FUSED": "1"}, 0),
            ("NO_MEGA2", {"GMVAE_NO_MEGA2": "1"}, 0), ("NO_SKINNY", {"GMVAE_NO_SKINNY": "1"}, 0),
            ("NO_EVALF", {"GMVAE_NO_EVALF": "1"}, 0), ("NO_PLANES", {"GMVAE_NO_PLANES": "1"}, 0), ("SCHED_SAFE", {}, 1)]
PLANE_VARIANTS = [("MINROWS128", {"GMVAE_PLANES_MINROWS": "128"}, 0),
                  ("MINROWS128+NO_PLANES", {"GMVAE_PLANES_MINROWS": "128", "GMVAE_NO_PLANES": "1"}, 0),
                  ("MINROWS128+NO_SKINNY", {"GMVAE_PLANES_MINROWS": "128", "GMVAE_NO_SKINNY": "1"}, 0)]
# (id, model, B, D, L, K, hidden, S, own environment): tests/test_abi.py's mega2v sizes (16 x 7 and 7 x 7 workgroups: below the
# compute-unit count of any device the suite runs on) and the plane shapes tests/test_hip_parity.py forces from 128 rows
EXTRA = [("extra-mega2v-vae_gmp-B256", "vae_gmp", 256, 784, 64, 10, (64,), 1, ()),
         ("extra-mega2v-vae-B100", "vae", 100, 784, 2, 1, (64,), 1, ()),
         ("extra-planes-S4", "gmvae", 64, 256, 64, 10, (128,), 4, ()),
         ("extra-planes-S1", "gmvae", 128, 256, 64, 10, (128,), 1, ())]
PLANE_IDS = ("extra-planes-S4", "extra-planes-S1")


def flag_sets(L, model):
    """No bit, each bit alone, the pairs of the feature tests, the clip bit with each -- refused ones included (their return
    code is recorded), except the GMVAE's own bits on the VAE family (GMVAE_E_MODEL whatever the shape)."""
    W, T, ST, M, LB = L.OBJ_WEIGHTS, L.Y_TEMP_DEV, L.Y_STRAIGHT_THROUGH, L.OBJ_PIXEL_MASK, L.OBJ_LABELS
    MY, IW, DR, CL = L.OBJ_MARGINAL_Y, L.OBJ_MARGINAL_Y_IW, L.GRAD_DREG, L.OPT_CLIP_NORM
    out = [0, W, M, DR, CL]
    if model == "gmvae":
        out += [T, ST, LB, MY, IW, W | T | ST, MY | LB, IW | LB, MY | DR, IW | DR, MY | W]
    out += [CL | f for f in out[1:] if f != CL]
    return out


def shapes():
    sys.path.insert(0, os.path.dirname(HERE))
    import gate_corners as G
    for c in G.CORNERS:
        if c.edge is None:
            yield (c.id, c.model, c.B, c.d.D, c.d.L, c.d.K, tuple(c.d.hidden), c.d.S, tuple(c.env))
    yield from EXTRA


def probe(L, model, B, D, Lz, K, hidden, S, flags, env):
    """(schedule string or return code, workspace bytes or return code) under exactly `env`."""
    import ctypes as C
    saved = {k: os.environ.pop(k, None) for k in ALL_SWITCHES}
    os.environ.update(env)
    try:
        d = L.make_dims(B, D, Lz, K, list(hidden), S=S, sched_flags=flags)
        buf, nb = C.create_string_buffer(48), C.c_uint64()
        rc = L.lib.gmvae_step_schedule(C.byref(d), L.MODEL_IDS[model], buf)
        rb = L.lib.gmvae_workspace_bytes(C.byref(d), L.MODEL_IDS[model], C.byref(nb))
        return (buf.value.decode() if rc == 0 else rc), (nb.value if rb == 0 else rb)
    finally:
        for k in ALL_SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def _fold(v):
    return v[0] if all(x == v[0] for x in v) else v


def table(L):
    cases = []
    for sid, model, B, D, Lz, K, hidden, S, own in shapes():
        variants = VARIANTS + (PLANE_VARIANTS if sid in PLANE_IDS else [])
        for flags in flag_sets(L, model):
            got = [probe(L, model, B, D, Lz, K, hidden, S, flags | vf, dict(own, **venv)) for _, venv, vf in variants]
            # (one value where every variant answers the same, else one per variant, in VARIANTS' order)
            cases.append(dict(id=sid, flags=flags, sched=_fold([g[0] for g in got]), bytes=_fold([g[1] for g in got])))
    return dict(variants=[v[0] for v in VARIANTS], plane_variants=[v[0] for v in PLANE_VARIANTS], cases=cases)


def write(doc, path):
    with open(path, "w") as f:
        f.write("{\n" + f' "variants": {json.dumps(doc["variants"])},\n "plane_variants": {json.dumps(doc["plane_variants"])},\n "cases": [\n')
        f.write(",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in doc["cases"]))
        f.write("\n ]\n}\n")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import build_hip
    build_hip.build(verbose=False)
    from gmvae_amd import _lib
    doc = table(_lib)
    write(doc, sys.argv[1] if len(sys.argv) > 1 else OUT)
    print(f"{len(doc['cases'])} cases")
