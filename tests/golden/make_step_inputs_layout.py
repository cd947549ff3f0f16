"""Regenerates tests/golden/step_inputs_layout.json (run from the repo root: ``python tests/golden/make_step_inputs_layout.py``):
gmvae_workspace_bytes and gmvae_workspace_offset of every region name, over a grid of dims that covers every legal
combination of the four per-step-input bits (GMVAE_OBJ_LABELS, GMVAE_OBJ_WEIGHTS, GMVAE_Y_TEMP_DEV, GMVAE_OBJ_PIXEL_MASK).

The committed file was written by the library as it stood BEFORE the per-step inputs were folded onto one table
(profiles/step_inputs_refactor_notes.md); tests/test_step_inputs_cpu.py holds every later build to it, byte for byte.  Run this
again only when a change is MEANT to move the workspace layout.
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "step_inputs_layout.json")

# every name gmvae_workspace_offset answers for (tests/test_abi.py's seven among them), the side inputs' last
NAMES = ["hy1", "hg1", "hd1", "gx", "logits", "y", "nent", "pp", "qp", "z", "logq", "logp", "logpx", "logw", "g", "dz", "dqp",
         "dpp", "dy", "dlogits", "dbuf0", "dbuf1", "dbuf2", "slabs", "s1", "s4", "eps", "u", "stamps", "gstamps", "sync",
         "ev_dbg", "vs", "sup_weight", "rwk", "y_floor", "y_soft", "labels", "obj_weights", "y_temperature", "pixel_mask"]

BATCHES = {1: (1, 16, 100, 1024), 3: (16,)}          # S -> batch sizes at the default sizes (the file stays small)
# (D, L, K, hidden): the factories' defaults (create_gmvae / create_vae: one hidden layer of latent_size units) and one H = 512
SIZES = {"gmvae": ((784, 64, 10, (64,)), (784, 64, 10, (512,))),
         "vae": ((784, 64, 1, (64,)), (784, 64, 1, (512,))),
         "vae_gmp": ((784, 64, 10, (64,)), (784, 64, 10, (512,)))}
H512_BATCH = 100          # (the H = 512 sizes at one batch size)


def flag_sets(L, mname, S):
    """Every legal combination of the four bits at S samples, with the objective / estimator bits it needs or admits."""
    W, T, M, LB = L.OBJ_WEIGHTS, L.Y_TEMP_DEV, L.OBJ_PIXEL_MASK, L.OBJ_LABELS
    MY, IW, DR, ST = L.OBJ_MARGINAL_Y, L.OBJ_MARGINAL_Y_IW, L.GRAD_DREG, L.Y_STRAIGHT_THROUGH
    out = [0, M]
    if S == 1:
        out.append(W)
    if mname == "gmvae":
        out += [T, T | ST, IW | LB, IW | LB | DR]
        if S == 1:
            out += [W | T, W | T | ST, MY | W, MY | LB, MY | LB | DR]
    return out


def grid(L):
    for mname in ("vae", "vae_gmp", "gmvae"):
        for si, (D, Lz, K, hidden) in enumerate(SIZES[mname]):
            for S in (1, 3):
                for B in (BATCHES[S] if si == 0 else (H512_BATCH,)):
                    for flags in flag_sets(L, mname, S):
                        yield dict(model=mname, B=B, D=D, L=Lz, K=K, hidden=list(hidden), S=S, flags=flags)


def probe(L, case):
    """(gmvae_workspace_bytes, [offset of NAMES[i], or its negative return code]) of one case."""
    model = L.MODEL_IDS[case["model"]]
    d = L.make_dims(case["B"], case["D"], case["L"], case["K"], case["hidden"], S=case["S"], sched_flags=case["flags"])
    offs = []
    for name in NAMES:
        o = C.c_uint64()
        rc = L.lib.gmvae_workspace_offset(C.byref(d), model, name.encode(), C.byref(o))
        offs.append(o.value if rc == 0 else rc)
    return L.workspace_bytes(d, model), offs


def layout(L):
    cases = []
    for case in grid(L):
        nbytes, offs = probe(L, case)
        cases.append(dict(case, bytes=nbytes, offsets=offs))
    return dict(names=NAMES, label_slots=L.LABEL_SLOTS, cases=cases)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import build_hip
    build_hip.build(verbose=False)
    from gmvae_amd import _lib
    doc = layout(_lib)
    with open(OUT, "w") as f:
        f.write("{\n" + f' "names": {json.dumps(doc["names"])},\n "label_slots": {doc["label_slots"]},\n "cases": [\n')
        f.write(",\n".join("  " + json.dumps(c) for c in doc["cases"]))
        f.write("\n ]\n}\n")
    print(f"{OUT}: {len(doc['cases'])} cases")
