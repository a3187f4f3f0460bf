"""Builds libirbfn_hip.so (HIP kernels + C ABI) for gfx950 with hipcc, in-tree.

``python -m irbfn_amd.build`` or ``irbfn_amd.build.build_lib()``.  hipcc cross-compiles without a
GPU.  Objects are cached under ``irbfn_amd/csrc/_obj`` and rebuilt when a source or header is newer.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(os.path.dirname(HERE), "include")
OBJ = os.path.join(CSRC, "_obj")
LIB = os.path.join(HERE, "libirbfn_hip.so")
ARCH = "gfx950"

_SLP = ["-fno-slp-vectorize"] if os.environ.get("IRBFN_NO_SLP") == "1" else []

# (source, object name, extra flags)
UNITS = [
    ("abi.hip", "abi.o", []),
    ("pack_all.hip", "pack_all.o", []),          # K0: every image of a net in two launches
    ("rbf_forward.hip", "rbf_forward.o", []),
    # NOTE on -fno-slp-vectorize (IRBFN_NO_SLP=1): hipcc's SLP vectoriser fuses the weight-row FMAs
    # into v_pk_fma_f32 with an SGPR-pair operand; measured on MI355X (cfg-2) the packed form is
    # FASTER than ten v_fmac_f32 with SGPR operands (152 vs 173 us), so SLP stays on by default.
    ("rbf_forward_kernels.hip", "rbf_fwd_d3.o", ["-DIRBFN_INST_D=3"] + _SLP),
    ("rbf_forward_kernels.hip", "rbf_fwd_d4.o", ["-DIRBFN_INST_D=4"] + _SLP),
    ("rbf_forward_kernels.hip", "rbf_fwd_d7.o", ["-DIRBFN_INST_D=7"] + _SLP),
    ("rbf_forward_kernels.hip", "rbf_fwd_d8.o", ["-DIRBFN_INST_D=8"] + _SLP),
    ("rbf_forward_mfma.hip", "rbf_fwd_mfma.o", []),
    ("rbf_forward_f16.hip", "rbf_fwd_f16.o", []),
    ("rbf_forward_small.hip", "rbf_fwd_small.o", []),
    # region-sparse kernels of the multi-region nets (per-lane lists of active regions)
    ("rbf_sparse.hip", "rbf_sparse.o", ["-fno-slp-vectorize"]),
    # float64 mode (--use_float64 of the reference): plain f64 VALU kernels
    ("rbf_f64.hip", "rbf_f64.o", []),
    ("rbf_forward_gram.hip", "rbf_forward_gram.o", []),
    ("rbf_forward_gram_wide.hip", "rbf_forward_gram_wide.o", []),
    ("rbf_forward_gram_gamma.hip", "rbf_forward_gram_gamma.o", []),    # K1g over padded regions, caller-provided region weights
    ("rbf_vjp.hip", "rbf_vjp.o", [] + _SLP),
    ("rbf_vjp_f16.hip", "rbf_vjp_f16.o", ["-fno-slp-vectorize"]),
    ("rbf_vjp_gram.hip", "rbf_vjp_gram.o", ["-fno-slp-vectorize"]),   # K2g, and the same loop over padded regions with caller-provided region weights
    ("rbf_vjp_mfma.hip", "rbf_vjp_mfma.o", []),        # K2m: hbar and dW on the f32 matrix cores   # VGPR operands: plain FMAs (2.4 cyc) beat packed (4.7) + pairing moves
    # x-VJP: plan + launchers, K5 per compiled D (as K1), K5m
    ("rbf_vjpx.hip", "rbf_vjpx.o", []),
    ("rbf_vjpx_kernels.hip", "rbf_vjpx_d3.o", ["-DIRBFN_INST_D=3"] + _SLP),
    ("rbf_vjpx_kernels.hip", "rbf_vjpx_d4.o", ["-DIRBFN_INST_D=4"] + _SLP),
    ("rbf_vjpx_kernels.hip", "rbf_vjpx_d7.o", ["-DIRBFN_INST_D=7"] + _SLP),
    ("rbf_vjpx_kernels.hip", "rbf_vjpx_d8.o", ["-DIRBFN_INST_D=8"] + _SLP),
    ("rbf_vjpx_mfma.hip", "rbf_vjpx_mfma.o", []),
    # 12-step unrolled groups of the roll-out; no SLP: v_pk_* cost more than the two plain VALU instructions they replace
    ("rollout.hip", "rollout.o", ["-mllvm", "-pragma-unroll-threshold=100000", "-fno-slp-vectorize"]),
    # the fused planning tick: wide K1h forward + K3p roll-out core in one kernel (the roll-out's flags: 50-knot register arrays)
    ("plan_tick_wide.hip", "plan_tick_wide.o", ["-mllvm", "-pragma-unroll-threshold=100000", "-fno-slp-vectorize"]),
    ("rollout_vjp.hip", "rollout_vjp.o", ["-mllvm", "-pragma-unroll-threshold=100000", "-fno-slp-vectorize"]),
    ("train_step.hip", "train_step.o", []),
    ("eval_errors.hip", "eval_errors.o", []),          # K6: roll-out error statistics of a table (rolled step loop)
    ("kmeans.hip", "kmeans.o", []),                    # K7: one Lloyd iteration of k-means on a table
    ("rbf_hidden.hip", "rbf_hidden.o", []),            # the hidden layer h[B][K] of a net: the design matrix of the closed-form fit
    ("syrk_f64.hip", "syrk_f64.o", []),                # K8: float64 Gram matrix of float32 rows on the f64 matrix instruction
    ("knn.hip", "knn.o", []),                          # K9: the p nearest centres of every row (the width rules)
    ("ols.hip", "ols.o", []),                          # K10: OLS forward selection of centres on the Gram matrix (f64 VALU)
    ("rows_quad_f64.hip", "rows_quad_f64.o", []),      # K11: per-row leverages and predictions of the closed-form fit (f64 MFMA)
    ("mlp_head.hip", "mlp_head.o", []),
    ("planner_front.hip", "planner_front.o", []),
    # the closed-loop tick around the net: plant step, windowed way-point search, goal, statistics, next query (no SLP: the plant
    # step is the roll-out's)
    ("sim_advance.hip", "sim_advance.o", ["-fno-slp-vectorize"]),
    # K13 / K15: batched NMPC solver (single-track and Frenet models), one problem per lane; every array statically indexed, so
    # the T and 2T loops must unroll fully (the roll-out's flags: the step inside is the roll-out's)
    ("nmpc_solve.hip", "nmpc_solve.o", ["-mllvm", "-pragma-unroll-threshold=100000", "-fno-slp-vectorize"]),
]


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC or install ROCm)")


def _newest_header() -> float:
    hs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    hs.append(os.path.join(INCLUDE, "irbfn_hip.h"))
    return max(os.path.getmtime(h) for h in hs)


def compile_cmd(src, extra, emit, out, root=os.path.dirname(HERE), hipcc=None):
    """The hipcc line of one unit of the tree at `root`: `emit` says what to write to `out` (["-c"] for the object).
    tools/isa_diff.py compiles two checkouts with it, so that it compares what ships."""
    csrc = os.path.join(root, "irbfn_amd", "csrc")
    return [hipcc or _hipcc(), "-O3", "-std=c++17", f"--offload-arch={ARCH}", "-fPIC", "-I", os.path.join(root, "include"),
            "-I", csrc, *extra, *emit, os.path.join(csrc, src), "-o", out]


def _compile(unit, hipcc, hdr_mtime, force):
    src, obj, extra = unit
    srcp, objp = os.path.join(CSRC, src), os.path.join(OBJ, obj)
    if (not force and os.path.exists(objp)
            and os.path.getmtime(objp) >= max(os.path.getmtime(srcp), hdr_mtime)):
        return objp, False
    cmd = compile_cmd(src, extra, ["-c"], objp, hipcc=hipcc)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src} {extra}:\n{r.stderr[-4000:]}")
    return objp, True


def build_lib(force: bool = False, verbose: bool = False, jobs: int | None = None) -> str:
    hipcc = _hipcc()
    os.makedirs(OBJ, exist_ok=True)
    hdr = _newest_header()
    jobs = jobs or min(len(UNITS), os.cpu_count() or 4)
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        res = list(ex.map(lambda u: _compile(u, hipcc, hdr, force), UNITS))
    objs = [r[0] for r in res]
    rebuilt = any(r[1] for r in res)
    if rebuilt or not os.path.exists(LIB):
        cmd = [hipcc, "-shared", "-fPIC", f"--offload-arch={ARCH}", *objs, "-o", LIB]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stderr[-4000:]}")
    if verbose:
        print(f"[irbfn_amd.build] {'rebuilt' if rebuilt else 'up to date'}: {LIB}")
    return LIB


if __name__ == "__main__":
    build_lib(force="--force" in sys.argv, verbose=True)
