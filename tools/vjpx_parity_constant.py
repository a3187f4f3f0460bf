"""The constant c of the query-VJP tests' bound |gx - ref| <= 1e-5 |ref| + c S (tests/_vjpx_util.py), measured without a GPU:
max |hand_gx(float32) - ref| / S per case of tests/test_gpu_vjpx.py's shape grids -- the formula in NumPy float32, i.e. the
reference arithmetic at the kernels' precision, against torch.autograd of the float64 restatement.  The tests use 4 x the
largest ratio, for the kernels' other summation order over up to 4096 terms.  Output: profiles/vjp_x_parity.txt (stdout)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _vjpx_util as vx  # noqa: E402


def main():
    worst = 0.0
    print("# max |hand_gx(float32) - ref_gx| / S per case (NumPy float32 against float64 autograd of the restatement; CPU)")
    print(f"# {'case':58s} {'B':>5s} {'centres':>7s} {'ratio':>9s} {'max|ref|':>10s} {'gate/all':>8s}")
    for family, cases in (("K5", vx.k5_cases()), ("K5m", vx.k5m_cases())):
        for name, build in cases.items():
            cfg, params, x, g = build()
            ref = vx.ref_gx(cfg, params, x, g)
            gx32, _ = vx.hand_gx(cfg, params, x, g, np.float32)
            gx64, S = vx.hand_gx(cfg, params, x, g, np.float64)
            assert np.abs(gx64 - ref).max() <= 1e-11 * np.abs(ref).max(), name
            # share of the gate term in the gradient (RBF term alone = the formula at the gate's own gamma, held fixed)
            rbf, _, _ = vx.hand_gx(cfg, params, x, g, np.float64, gamma=vx._gate(cfg, np.asarray(x, np.float64), np.float64)[0])
            share = np.abs(gx64 - rbf).max() / np.abs(ref).max()
            ratio = float((np.abs(gx32.astype(np.float64) - ref) / S).max())
            worst = max(worst, ratio)
            n = cfg["num_regions"] * cfg["num_kernels"]
            print(f"{family + ':' + name:60s} {x.shape[0]:5d} {n:7d} {ratio:9.2e} {np.abs(ref).max():10.3e} {share:8.1e}", flush=True)
    print(f"# largest ratio {worst:.2e}; tests use C_S = 4 x {worst:.1e} = {4 * float(f'{worst:.1e}'):.2e}")


if __name__ == "__main__":
    main()
