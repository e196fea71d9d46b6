"""Build libgnnmanip_hip.so (gfx950) in-tree with hipcc.  No CPU fallback exists: if the
library is missing the package fails loudly at first use."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libgnnmanip_hip.so")
SOURCES = ["graph.hip", "features.hip", "mlp.hip", "hedge.hip", "hmlp.hip", "model.hip", "train.hip", "train_model.hip", "train_step.hip", "sinkhorn.hip", "rollout_grad.hip", "train_batch.hip", "dataset_stats.hip"]
# hedge.hip: packed fp32 VALU (SLP-vectorised v_pk_fma_f32) returned wrong low lanes next to its LDS / MFMA traffic on gfx950
EXTRA_FLAGS = {"hedge.hip": ["-fno-slp-vectorize"] + os.environ.get("GM_HEDGE_FLAGS", "").split(), "hmlp.hip": ["-fno-slp-vectorize"] + os.environ.get("GM_HM_FLAGS", "").split(),
               "train.hip": os.environ.get("GM_TRAIN_FLAGS", "").split(), "graph.hip": os.environ.get("GM_GRAPH_FLAGS", "").split()}
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Wno-unused-value"]


def source_digest():
    """sha256 (first 16 hex digits) over the sources of the kernels whose HBM traffic is recorded: profiles/<tag>_traffic.json records the digest of the build its PMC
    passes ran, and bench.py reports the measured traffic only while it still matches the tree."""
    import hashlib
    h = hashlib.sha256()
    # the processor edge kernels whose traffic is recorded, and what they include (host-side files do not change a kernel)
    for f in ("common.h", "hedge.h", "hedge.hip", "hmlp.h", "hmlp.hip", "hmma_dev.h", "mlp.h", "blocks_dev.h"):
        h.update(f.encode())
        h.update(open(os.path.join(CSRC, f), "rb").read())
    return h.hexdigest()[:16]


def _newer(a, b):
    return (not os.path.exists(b)) or os.path.getmtime(a) > os.path.getmtime(b)


def build(force=False, verbose=False, tag=None):
    """tag: development A/B builds -- objects in build_<tag>/, library in <repo>/variants/lib_<tag>.so (GM_LIB_PATH selects it)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = os.path.join(HERE, "build" if not tag else "build_" + tag)
    lib = LIB
    if tag:
        os.makedirs(os.path.join(os.path.dirname(HERE), "variants"), exist_ok=True)
        lib = os.path.join(os.path.dirname(HERE), "variants", f"lib_{tag}.so")
    os.makedirs(objdir, exist_ok=True)
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    headers.append(os.path.join(os.path.dirname(HERE), "include", "gnn_manip_hip.h"))
    objs, jobs = [], []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(objdir, src.replace(".hip", ".o"))
        objs.append(o)
        if force or _newer(s, o) or any(_newer(h, o) for h in headers):
            jobs.append([hipcc] + FLAGS + EXTRA_FLAGS.get(src, []) + ["-c", s, "-o", o])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stdout + r.stderr)

    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(run, jobs))
    if jobs or force or not os.path.exists(lib):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs)
    return lib


if __name__ == "__main__":
    tag = next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--tag=")), None)
    print(build(force="--force" in sys.argv, verbose=True, tag=tag))
