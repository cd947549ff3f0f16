"""Builds gmvae_amd/lib/libgmvae_hip.so in-tree with hipcc for gfx950 (no hipify, no JIT cache).

Standalone on purpose (`python build_hip.py [--force]`): importing the gmvae_amd package loads the
shared library, so the builder must not live inside it."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
HERE = os.path.join(ROOT, "gmvae_amd")
SRC = os.path.join(HERE, "csrc", "gmvae_hip.hip")
# a translation unit -- and a device code object -- of its own: code added there leaves the training step's code object, and so the
# placement of the one-launch step's code, untouched (csrc/tsne.hip)
SRC_EVAL = os.path.join(HERE, "csrc", "tsne.hip")
SRC_MIXFIT = os.path.join(HERE, "csrc", "mixfit.hip")      # a third one, for the same reason
SRC_NEIGH = os.path.join(HERE, "csrc", "neigh.hip")        # and a fourth
SRC_AIS = os.path.join(HERE, "csrc", "ais.hip")            # and a fifth: gmvae_ais, gmvae_refine, gmvae_simulate, gmvae_ais_reverse (ais.hpp's kernels, defined once)
SRC_IMPUTE = os.path.join(HERE, "csrc", "impute.hip")      # and a sixth: gmvae_impute's kernels (its host path is iw_run in gmvae_hip.hip)
SRC_LINPROBE = os.path.join(HERE, "csrc", "linprobe.hip")  # and a seventh: gmvae_linprobe_*
SRC_TWOSAMPLE = os.path.join(HERE, "csrc", "twosample.hip")  # and an eighth: gmvae_mmd, gmvae_sinkhorn (cgram.hpp's kernels, defined once)
SRC_PCA = os.path.join(HERE, "csrc", "pca.hip")              # and a ninth: gmvae_pca_*, gmvae_sym_eigh
import glob
DEPS = sorted(glob.glob(os.path.join(HERE, "csrc", "*"))) + [os.path.join(ROOT, "include", "gmvae_hip.h")]
OUT = os.path.join(HERE, "lib", "libgmvae_hip.so")


def needs_build() -> bool:
    if not os.path.exists(OUT):
        return True
    t = os.path.getmtime(OUT)
    return any(os.path.getmtime(d) > t for d in DEPS)


def build(force: bool = False, verbose: bool = True) -> str:
    if not force and not needs_build():
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # -amdgpu-kernarg-preload-count: leading scalar kernel parameters arrive in SGPRs at wave start (mega2.hpp M2_HEAD_PARAMS: the
    # first layer's addresses need no round trip into the cold argument block); translation-unit wide, and a kernel keeps a
    # prologue of ordinary loads for firmware that does not preload
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-value",
           "-mllvm", "-amdgpu-kernarg-preload-count=14", "-o", OUT, SRC, SRC_EVAL, SRC_MIXFIT, SRC_NEIGH, SRC_AIS, SRC_IMPUTE, SRC_LINPROBE, SRC_TWOSAMPLE, SRC_PCA]
    # PyTorch-ROCm ships its own libamdhip64.so (soname without the .7).  Link against THAT
    # copy so that the process holds one HIP runtime: streams and device pointers handed over
    # by torch are then valid inside this library whatever the import order.
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is not None and spec.submodule_search_locations:
        tl = os.path.join(list(spec.submodule_search_locations)[0], "lib")
        if os.path.exists(os.path.join(tl, "libamdhip64.so")):
            cmd += [f"-L{tl}", f"-Wl,-rpath,{tl}"]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return OUT


if __name__ == "__main__":
    build(force="--force" in sys.argv)
