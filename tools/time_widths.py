"""Times irbfn_knn_d2 and the width stage (irbfn_amd/widths.py) on one GPU, next to two baselines that are not the code under
test: chunked ``torch.cdist`` -> ``topk`` (its distances come from a Gram expansion, so it is the speed yardstick only) and, for
p = 1, ``irbfn_kmeans_step`` in its assign-only form at the same shape, this project's pair-rate yardstick.

Shapes: centres against themselves at (K, D, p) = (4096, 7, 2), (16384, 8, 2), (65536, 16, 8), with the library's own split and with
fixed ones; rows against centres at N = 2^22, K = 500, D = 8, p = 1 and 4; then the wall time of ``nearest_neighbour`` and of one
``select_scale`` over five scales at N = 2^20, K = 1000, O = 10.  One warm-up pass over every variant, then ROUNDS interleaved
rounds (every variant once per round, between two device events as many calls as fill about 20 ms, at least 5); medians with
min / max.  Gpairs/s = N K / time.

Without arguments every step runs as a child process of its own under its own time limit, the first failure ends the run, and
profiles/widths.txt (or the file after ``--out``) is written afresh: PREAMBLE, then the steps' output.  What the lines say is in
DESIGN.md (K9).  ``--step NAME`` runs one step in this process."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS, INNER, INNER_MAX, SPAN_US = 7, 5, 400, 20000.0      # a timed span is at least 5 calls and about 20 ms
SELF_SHAPES = ((4096, 7, 2), (16384, 8, 2), (65536, 16, 8))
SELF_SPLITS = (0, 1, 4, 16, 64)
ROWS_N, ROWS_K, ROWS_D = 1 << 22, 500, 8
FIT_N, FIT_K, FIT_D, FIT_O = 1 << 20, 1000, 8, 10
STEPS = (("clocks", 60), ("self", 300), ("rows", 300), ("rules", 300))      # (name, seconds)
PREAMBLE = """\
RBF widths from the data (irbfn_amd/widths.py, irbfn_knn_d2 = kernel K9): times on one GPU, written by tools/time_widths.py.
Every step is a process of its own under its own time limit.  Device events around xN calls (as many as fill about 20 ms, at
least 5), every variant once per round, median over 7 interleaved rounds after one warm-up pass [min .. max]; a time per call as
the host module issues it (one launch with one segment, the list pass + the merge with more), launch gaps included.
Gpairs/s = N K / time / 1e9.  Clocks: the idle state rocm-smi reports before the first launch; the clocks under load are not read.
Baselines, neither of which is the code under test: (a) chunked torch.cdist -> topk (blocks of at most 256 MiB; for centres
against themselves the row's own centre is masked with +Inf first); its distances come from a Gram expansion (the lines "largest
|sqrt(d2) - torch distance|"), so it is the speed yardstick only.  (b) for p = 1, irbfn_kmeans_step with new_centers = counts =
NULL (assign only) on the same rows and centres: this project's pair-rate yardstick.  No ratio was fixed in advance.
Not measured: PMC counters of the list pass; one row per lane; a 256-centre tile; clocks under load.

"""


def span(torch, fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def measure(torch, variants):
    """variants: [(label, fn)] -> {label: (median, min, max, calls per span)} in us.  After the warm-up every variant gets the number
    of calls that fills a span of SPAN_US (between INNER and INNER_MAX), from one trial span."""
    for _, fn in variants:
        fn()
    torch.cuda.synchronize()
    calls = {}
    for label, fn in variants:
        calls[label] = int(min(INNER_MAX, max(INNER, np.ceil(SPAN_US / max(span(torch, fn, INNER), 1e-3)))))
    t = {label: [] for label, _ in variants}
    for _ in range(ROUNDS):
        for label, fn in variants:
            t[label].append(span(torch, fn, calls[label]))
    return {k: (float(np.median(v)), min(v), max(v), calls[k]) for k, v in t.items()}


def report(res, pairs):
    for label, (med, lo, hi, n) in res.items():
        print(f"   {label:44s} {med:10.1f} us  [{lo:.1f} .. {hi:.1f}]  x{n:<4d} {pairs / med * 1e-3:9.1f} Gpairs/s")


def knn_call(lib, torch, q, c, p, self0, split):
    from irbfn_amd.model import _ptr, _stream_ptr
    N, D = q.shape
    K = c.shape[0]
    d2 = torch.empty((N, p), dtype=torch.float32, device="cuda")
    idx = torch.empty((N, p), dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.irbfn_knn_workspace_bytes(N, K, D, p, split), dtype=torch.uint8, device="cuda")
    stream = _stream_ptr(torch)

    def call():
        st = lib.irbfn_knn_d2(_ptr(q), _ptr(c), N, K, D, p, self0, split, _ptr(d2), _ptr(idx), _ptr(ws), ws.numel(), stream)
        assert st == 0, st
    return call, d2, idx


def torch_topk(torch, q, c, p, drop_self):
    """cdist -> topk in chunks of rows whose [chunk, K] float32 block stays at 256 MiB; drop_self: the row's own centre is masked."""
    chunk = max(1, min(q.shape[0], (1 << 26) // c.shape[0]))
    out = torch.empty((q.shape[0], p), dtype=torch.float32, device="cuda")

    def call():
        for r0 in range(0, q.shape[0], chunk):
            d = torch.cdist(q[r0:r0 + chunk], c)
            if drop_self:
                n = d.shape[0]
                d[torch.arange(n, device="cuda"), torch.arange(r0, r0 + n, device="cuda")] = float("inf")
            out[r0:r0 + chunk] = torch.topk(d, p, dim=1, largest=False).values
    return call, out


def step_clocks():
    import torch
    print(f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30)
        lines = [ln.strip() for ln in r.stdout.splitlines() if "sclk" in ln or "mclk" in ln]
        print("clock state (rocm-smi --showclocks, idle, before the first launch): " + ("; ".join(lines[:4]) if lines else "not reported"))
    except (OSError, subprocess.SubprocessError) as e:
        print(f"clock state: not read ({type(e).__name__})")


def step_self():
    import torch
    from irbfn_amd import _lib
    lib = _lib.load()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    print(f"centres against themselves (self0 = 0): {ROUNDS} rounds, median us [min .. max], xN = calls per timed span")
    for K, D, p in SELF_SHAPES:
        c = torch.rand((K, D), device="cuda", generator=gen) * 6 - 3
        variants, outs = [], []
        for split in SELF_SPLITS:
            call, d2, idx = knn_call(lib, torch, c, c, p, 0, split)
            variants.append((f"irbfn_knn_d2 split = {split}" + (" (the library's)" if split == 0 else ""), call))
            outs.append((d2, idx))
        tcall, tout = torch_topk(torch, c, c, p, True)
        variants.append(("torch cdist -> topk", tcall))
        res = measure(torch, variants)
        print(f"-- K = {K}, D = {D}, p = {p}")
        report(res, K * K)
        same = all(torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1], o[1]) for o in outs[1:])
        dev = (outs[0][0].sqrt() - tout).abs().max().item()
        print(f"   splits bit-identical: {same}; largest |sqrt(d2) - torch distance| = {dev:.3e}; "
              f"torch / irbfn_knn_d2 = {res['torch cdist -> topk'][0] / res[variants[0][0]][0]:.2f}")


def step_rows():
    import torch
    from irbfn_amd import _lib
    from irbfn_amd.model import _ptr, _stream_ptr
    lib = _lib.load()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    N, K, D = ROWS_N, ROWS_K, ROWS_D
    x = torch.rand((N, D), device="cuda", generator=gen) * 6 - 3
    c = x[torch.randperm(N, device="cuda", generator=gen)[:K]].clone()
    labels = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    ad2 = torch.empty(N, dtype=torch.float32, device="cuda")
    stats = torch.zeros(4, dtype=torch.float64, device="cuda")
    kws = torch.empty(lib.irbfn_kmeans_workspace_bytes(N, K, D), dtype=torch.uint8, device="cuda")
    stream = _stream_ptr(torch)

    def assign():
        st = lib.irbfn_kmeans_step(_ptr(x), _ptr(c), _ptr(labels), _ptr(ad2), None, None, _ptr(stats), N, K, D, _ptr(kws), kws.numel(), stream)
        assert st == 0, st
    print(f"rows against centres: N = {N}, K = {K}, D = {D}, {ROUNDS} rounds, median us [min .. max], xN = calls per timed span")
    for p in (1, 4):
        call, d2, idx = knn_call(lib, torch, x, c, p, -1, 0)
        tcall, tout = torch_topk(torch, x, c, p, False)
        variants = [(f"irbfn_knn_d2 p = {p}", call), ("torch cdist -> topk", tcall)]
        if p == 1:
            variants.append(("irbfn_kmeans_step, assign only", assign))
        res = measure(torch, variants)
        print(f"-- p = {p}")
        report(res, N * K)
        line = f"   torch / irbfn_knn_d2 = {res['torch cdist -> topk'][0] / res[variants[0][0]][0]:.2f}"
        if p == 1:
            line += (f"; irbfn_knn_d2 / assign only = {res[variants[0][0]][0] / res['irbfn_kmeans_step, assign only'][0]:.3f}; equal to its labels "
                     f"and d2 bit for bit: {torch.equal(idx[:, 0], labels) and torch.equal(d2[:, 0], ad2)}")
        print(line + f"; largest |sqrt(d2) - torch distance| = {(d2.sqrt() - tout).abs().max().item():.3e}")


def wall(torch, fn, n=3):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return r, float(np.median(t)), min(t), max(t)


def step_rules():
    import torch
    from irbfn_amd import kmeans, widths
    from irbfn_amd.model import WCRBFNet
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    print("host entry points: wall ms around a device synchronise, median of 3 after one warm-up [min .. max]")
    for K, D, p in SELF_SHAPES + ((FIT_K, FIT_D, 2),):
        c = torch.rand((K, D), device="cuda", generator=gen) * 6 - 3
        _, med, lo, hi = wall(torch, lambda: widths.nearest_neighbour(c, p=p))
        print(f"-- nearest_neighbour(K = {K}, D = {D}, p = {p}): {med:.2f} ms  [{lo:.2f} .. {hi:.2f}]")
    N, K, D, O = FIT_N, FIT_K, FIT_D, FIT_O
    x = torch.rand((N, D), device="cuda", generator=gen)
    y = torch.stack([torch.sin((3 + o) * x[:, o % D]) + x[:, (o + 1) % D] * x[:, (o + 2) % D] for o in range(O)], 1).contiguous()
    res = kmeans.fit(x, K, max_iter=5, init="random")
    cfg = dict(in_features=D, out_features=O, num_kernels=K, basis_func="gaussian", num_regions=1, lower_bounds=[], upper_bounds=[],
               dimension_ranges=[[]], activation_idx=[], delta=[], fixed_centers=True, fixed_width=True)
    net = WCRBFNet.from_config(cfg, centers=res.centers.cpu().numpy())
    w = widths.nearest_neighbour(res.centers, p=2)
    _, med, lo, hi = wall(torch, lambda: widths.cluster_spread(x, res.centers))
    print(f"-- cluster_spread(N = {N}, K = {K}, D = {D}): {med:.2f} ms  [{lo:.2f} .. {hi:.2f}]")
    s, med, lo, hi = wall(torch, lambda: widths.select_scale(net, w, x, y), n=3)
    print(f"-- select_scale(N = {N}, K = {K}, D = {D}, O = {O}, five scales): {med:.1f} ms  [{lo:.1f} .. {hi:.1f}]; held-out MSE "
          f"{['%.3e' % h for h in s.holdout_mse]}, best scale {s.best_scale}")


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--step":
        import torch
        assert torch.cuda.is_available(), "time_widths.py measures on the GPU"
        {"clocks": step_clocks, "self": step_self, "rows": step_rows, "rules": step_rules}[sys.argv[2]]()
        return 0
    out = sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--out" else os.path.join(ROOT, "profiles", "widths.txt")
    text = []
    for name, limit in STEPS:          # a fresh process per step, each under its own limit; the first failure ends the run
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"step {name}: no result within {limit} s; stopping", file=sys.stderr)
            return 124
        sys.stdout.write(r.stdout)
        text.append(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print(f"step {name}: exit status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode
    with open(out, "w") as f:
        f.write(PREAMBLE + "".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
