"""Build libposecnn_hip.so in-tree for gfx950 (hipcc, no JIT cache).

Each source compiles to its own object under build/ (in parallel), then the
objects link into the shared library."""
import glob
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "build")
OUT = os.path.join(HERE, "libposecnn_hip.so")
SOURCES = ["capi.hip", "hough_compact.hip", "hough_vote.hip", "hough_peak.hip", "hough_emit.hip", "roi_pooling.hip",
           "average_distance.hip", "backprojecting.hip", "pose_head.hip", "gemm.hip", "gemm_f32.hip", "gemm_x3.hip",
           "gemm_x6.hip", "box_nms.hip", "label_producer.hip", "icp.hip", "pose_search.hip", "dropout.hip", "pose2d.hip", "pose3d.hip", "gemm_tp.hip",
           "render.hip", "render_scene.hip", "render_lit.hip", "seg_loss.hip", "vertex_pred_bwd.hip", "fc8_fused.hip", "upscore.hip",
           "momentum.hip", "pose_eval.hip", "neck.hip", "backbone.hip"]
HEADERS = sorted(glob.glob(os.path.join(CSRC, "*.h"))) + [os.path.join(HERE, "..", "include", h) for h in ("posecnn_hip.h", "posecnn_image.h", "posecnn_train.h", "posecnn_eval.h", "posecnn_neck.h", "posecnn_backbone.h")]
# -ffp-contract=off: the parity arithmetic rounds every float op separately
# (reference semantics restated by oracle/); MFMA kernels are unaffected.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wno-unused-result"]
# The GEMM files: the SLP vectorizer pairs the hi/lo split of two staged floats from
# different load tuples into v_pk_add_f32, which forces register copies of the
# freshly loaded tuples at the loop edge -- each behind a vmcnt wait that
# exposes the full load latency every K step.  (pose_head.hip: built with the
# flag since its kernels shared a file with the GEMMs.)
NO_SLP = ["pose_head.hip", "gemm.hip", "gemm_f32.hip", "gemm_x3.hip", "gemm_x6.hip", "gemm_tp.hip",
          "fc8_fused.hip", "backbone.hip"]
FILE_FLAGS = {src: ["-fno-slp-vectorize"] for src in NO_SLP}


def _obj(src):
    return os.path.join(OBJ, src.replace(".hip", ".o"))


def needs_build():
    if not os.path.exists(OUT):
        return True
    t = os.path.getmtime(OUT)
    deps = [os.path.join(CSRC, s) for s in SOURCES] + HEADERS + [os.path.abspath(__file__)]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True):
    if not force and not needs_build():
        return OUT
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(OBJ, exist_ok=True)
    newest_header = max(os.path.getmtime(h) for h in HEADERS + [os.path.abspath(__file__)])

    def compile_one(src):
        o = _obj(src)
        path = os.path.join(CSRC, src)
        if not force and os.path.exists(o) and os.path.getmtime(o) > max(os.path.getmtime(path), newest_header):
            return
        cmd = [hipcc] + FLAGS + FILE_FLAGS.get(src, []) + ["-c", path, "-o", o + ".tmp"]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)
        os.replace(o + ".tmp", o)

    jobs = min(len(SOURCES), max(1, min(8, os.cpu_count() or 1)))
    with ThreadPoolExecutor(jobs) as ex:
        list(ex.map(compile_one, SOURCES))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT + ".tmp"] + [_obj(s) for s in SOURCES]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    os.replace(OUT + ".tmp", OUT)
    return OUT


if __name__ == "__main__":
    build(force="--force" in sys.argv)
