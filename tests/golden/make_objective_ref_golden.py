"""Regenerates tests/golden/objective_ref_parent.json (run from the repo root: ``python tests/golden/make_objective_ref_golden.py``):
what the seven fp64 statements (tests/ymarg_ref.py, ymarg_iw_ref.py, dreg_ref.py, semisup_ref.py, wobj_ref.py, ytemp_ref.py,
pmask_ref.py) return on every entry of every case table they and their device tests use, and on each optional switch at least
once (both estimators, relu_masks= from the statement's own pre-activations -- once per module --, encoder_sees_mask=False,
mask=None, y_leaf=True).

The committed file was written by the seven modules as they stood BEFORE they became adapters onto tests/objective_ref.py
(profiles/objective_ref_refactor_notes.md); tests/test_objective_ref_cpu.py holds the adapters to it.  Per record: every scalar
of C as it is, and (sum, largest magnitude, dot product with a fixed-seed normal vector) of every array of C and of every tensor
of g; the relu_masks= records add the same of every pre-activation.  The file holds each distinct list of keys once ("keys") and
per record the index of its list and the values in that order.  Run this again only when a change is MEANT to move the statement.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "objective_ref_parent.json")
PROBE_SEED = 20261019


def three(a):
    """(sum, largest magnitude, dot product with the probe vector) of an array, in fp64."""
    a = np.asarray(a).astype(np.float64).reshape(-1)
    if a.size == 0:
        return [0.0, 0.0, 0.0]
    v = np.random.default_rng(PROBE_SEED).standard_normal(a.size)
    return [float(a.sum()), float(np.abs(a).max()), float(a @ v)]


def digest(C, g, with_pre):
    """{key: scalar | None | [sum, max, dot]} of one statement's (C, g)."""
    out = {}
    for k, v in C.items():
        if k == "pre":
            for net, layers in v.items() if with_pre else ():
                for i, (pre, mag) in enumerate(layers):
                    out[f"C/pre/{net}/{i}/pre"] = three(pre)
                    out[f"C/pre/{net}/{i}/mag"] = three(mag)
        elif v is None:
            out[f"C/{k}"] = None
        elif np.ndim(v) == 0:
            out[f"C/{k}"] = float(v)
        else:
            out[f"C/{k}"] = three(v)
    for k, v in g.items():
        out[f"g/{k}"] = three(v)
    return out


def digest_of(rid, thunk):
    return digest(*thunk(), with_pre=rid.endswith("own-masks"))


def pack(doc):
    """{id: digest} -> the file's form: dict(keys = the distinct key lists, records = {id: [index into keys, values]})."""
    keys, records = [], {}
    for rid, dg in doc.items():
        if list(dg) not in keys:
            keys.append(list(dg))
        records[rid] = [keys.index(list(dg)), list(dg.values())]
    return dict(keys=keys, records=records)


def unpack(packed):
    return {rid: dict(zip(packed["keys"][i], values)) for rid, (i, values) in packed["records"].items()}


def own_masks(C):
    """relu_masks= in the form the statements take them, from a statement's own pre-activations."""
    return {net: [None] + [pre > 0 for pre, _ in layers] for net, layers in C["pre"].items()}


def records():
    """{id: thunk -> (C, g)} in a fixed order.  The inputs are the device tests' own (their _setup / the modules' setup())."""
    import dreg_ref as DR
    import oracle as O
    import pmask_ref as PR
    import semisup_ref as SR
    import test_dreg
    import test_semisup
    import test_ymarg
    import test_ymarg_iw
    import wobj_ref as WR
    import ymarg_iw_ref as YI
    import ymarg_ref as YM
    import ytemp_ref as TR
    GM = O.MODEL_GMVAE
    r = {}

    def p32_of(model, d, flat):
        return O.unpack(model, d, flat.astype(np.float64))

    def with_own_masks(f):
        return lambda: f(relu_masks=own_masks(f()[0]))

    for name, (d, B) in test_ymarg.SIZES.items():
        def f(name=name, d=d, B=B, **kw):
            flat, x, eps = test_ymarg._setup(d, B, seed=len(name))
            return YM.loss_and_grads(d, p32_of(GM, d, flat), x, eps, **kw)
        r[f"ymarg/{name}"] = f
        if name == "h24x2_relu":
            r[f"ymarg/{name}/own-masks"] = with_own_masks(f)

    for name, (d, B, S) in test_ymarg_iw.SIZES.items():
        def f(name=name, d=d, B=B, S=S, **kw):
            flat, x, eps = test_ymarg_iw._setup(d, B, S, seed=len(name))
            return YI.loss_and_grads(d, p32_of(GM, d, flat), x, eps, S, **kw)
        r[f"ymarg_iw/{name}"] = f
        if name == "run_gmvae_defaults_s5":
            r[f"ymarg_iw/{name}/own-masks"] = with_own_masks(f)

    for name, (mname, d, B, S, _) in test_dreg.CASES.items():
        def f(name=name, mname=mname, d=d, B=B, S=S, **kw):
            model = test_dreg.MODELS[mname]
            flat, x, eps = test_dreg._setup(model, d, B, S, seed=len(name))
            return DR.loss_and_grads(model, d, p32_of(model, d, flat), x, eps, S, **kw)
        r[f"dreg/{name}"] = f
        if name in ("vae_gmp_s3", "gmvae_marginal_iw_s3"):
            r[f"dreg/{name}/standard"] = lambda f=f: f(estimator="standard")
        if name == "vae_gmp_s3":
            r[f"dreg/{name}/own-masks"] = with_own_masks(f)

    for name, (d, B, S) in test_semisup.CASES.items():
        def f(name=name, d=d, B=B, S=S, **kw):
            seed = test_semisup.SEEDS[name]
            flat, x, eps = test_semisup._setup(d, B, S, seed=seed)
            y = test_semisup._labels(d.K, B, seed)
            if name == "c":
                y[3] = 71
            return SR.loss_and_grads(d, p32_of(GM, d, flat), x, eps, S, y, test_semisup.ALPHA, **kw)
        r[f"semisup/{name}"] = f
        if name == "b":
            r[f"semisup/{name}/dreg"] = lambda f=f: f(estimator="dreg")
            r[f"semisup/{name}/dreg/own-masks"] = with_own_masks(lambda f=f, **kw: f(estimator="dreg", **kw))

    for name in WR.CASES:
        def f(weights, name=name, **kw):
            model, marginal, d, p32, flat, x, eps, u = WR.setup(name)
            return WR.loss_and_grads(model, d, p32, x, eps, u, weights, marginal, **kw)
        r[f"wobj/{name}/case-weights"] = lambda f=f, name=name: f(WR.WEIGHTS + (WR.case_lambda(name),))
        r[f"wobj/{name}/unit-weights"] = lambda f=f: f((1.0, 1.0, 0.0))
        if name == "marginal":
            r[f"wobj/{name}/own-masks"] = with_own_masks(lambda f=f, name=name, **kw: f(WR.WEIGHTS + (WR.case_lambda(name),), **kw))

    for name in TR.CASES:
        def f(tau, st, name=name, **kw):
            d, p32, flat, x, eps, u = TR.setup(name)
            return TR.loss_and_grads(d, p32, x, eps, u, tau, straight_through=st, weights=TR.case_weights(name), **kw)
        for tau in TR.TAUS:
            for st in (False, True):
                r[f"ytemp/{name}/tau{tau}/{'straight-through' if st else 'relaxed'}"] = lambda f=f, tau=tau, st=st: f(tau, st)
        if name == "K7-S3":
            r[f"ytemp/{name}/y-leaf"] = lambda f=f: f(0.5, True, y_leaf=True)
            r[f"ytemp/{name}/own-masks"] = with_own_masks(lambda f=f, **kw: f(0.5, True, **kw))

    for name in PR.CASES:
        def f(name=name, **kw):
            model, d, p32, flat, xf, eps, u, m, x = PR.setup(name)
            return PR.loss_and_grads(model, d, p32, xf, eps, u, m, **kw)
        r[f"pmask/{name}"] = f
        if name == "gmvae-s3":
            r[f"pmask/{name}/encoder-unmasked"] = lambda f=f: f(encoder_sees_mask=False)
            r[f"pmask/{name}/own-masks"] = with_own_masks(f)

    def no_mask():
        model, d, p32, flat, xf, eps, u, m, x = PR.setup("gumbel")
        return PR.loss_and_grads(model, d, p32, x, eps, u, None)
    r["pmask/gumbel/mask-none"] = no_mask
    return r


if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
    doc = pack({k: digest_of(k, f) for k, f in records().items()})
    with open(OUT, "w") as f:
        f.write('{\n "keys": [\n' + ",\n".join("  " + json.dumps(k) for k in doc["keys"]) + '\n ],\n "records": {\n')
        f.write(",\n".join(f"  {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in doc["records"].items()) + "\n }\n}\n")
    print(f"{OUT}: {len(doc['records'])} records, {len(doc['keys'])} key lists, {os.path.getsize(OUT)} bytes")
