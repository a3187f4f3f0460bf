"""Times OLS forward selection (irbfn_ols_begin / irbfn_ols_steps = kernel K10, irbfn_amd/ols.py) on one GPU, next to a baseline
that is not the code under test: the same algorithm written in torch float64 ops (``index_select``, ``mv``, ``argmax``; no host
read), which is what a user would write without the kernel.

Shapes (M, K, O) = (512, 64, 2), (4096, 1000, 10), (8000, 1000, 10): G = Z^T Z of M + 200 random rows, so that no pool runs out.
Per shape: the whole selection (begin + K + 1 steps) between two device events, ROUNDS interleaved rounds of kernel and baseline
after one warm-up of each, medians with min / max; then, inside one selection, the time per step over the first and the last
WINDOW steps (launch-bound against read-bound), and the bytes of the factor L those last steps read per second.

Without arguments every shape runs as a child process of its own under its own time limit, the first failure ends the run, and
profiles/ols.txt (or the file after ``--out``) is written afresh: PREAMBLE, then the steps' output.  What the lines say is in
DESIGN.md (K10).  ``--step NAME`` runs one step in this process; from a shell every step under its own limit:

    timeout -k 10 120 python tools/profile_ols.py --step small && timeout -k 10 300 python tools/profile_ols.py --step mid && \\
    timeout -k 10 420 python tools/profile_ols.py --step large
"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS, WINDOW = 5, 16
SHAPES = {"small": (512, 64, 2), "mid": (4096, 1000, 10), "large": (8000, 1000, 10)}
STEPS = (("small", 120), ("mid", 300), ("large", 420))          # (name, seconds)
HBM_TBS, LLC_MIB = 6.29, 256                                    # the measured float4-copy rate and the last-level cache of an MI355X
PREAMBLE = """\
OLS forward selection of centres (irbfn_amd/ols.py, irbfn_ols_begin / irbfn_ols_steps = kernel K10): times on one GPU, written by
tools/profile_ols.py.  Every shape is a process of its own under its own time limit.  G = Z^T Z of M + 200 rows of U(0,1) hidden
values, a ones column and O mixed targets; ridge 1e-8, fit_bias.  "selection" = irbfn_ols_begin + K + 1 steps (two launches each)
between two device events, launch gaps included, median of 5 interleaved rounds after one warm-up [min .. max].  Baseline, not the
code under test: the same algorithm in torch float64 ops on the same GPU (index_select, mv, argmax, where; no host read).  No ratio
was fixed in advance.  "first / last 16 steps" = events inside one selection around steps 1 .. 16 and K - 15 .. K.  L bytes/s =
t npad 8 bytes per step (the factor rows a step reads) over the step time of the last 16 steps, against 6.29 TB/s (the measured
float4-copy rate of HBM); whether the factor fits the 256 MiB last-level cache is printed with its size.
Not measured: PMC counters, the clocks under load.  Other block geometries of the step kernel: profiles/ols_ab.txt.

"""


def make_g(torch, M, O, gen):
    N = M + 200
    H = torch.rand((N, M), dtype=torch.float64, device="cuda", generator=gen)
    W = torch.randn((M, O), dtype=torch.float64, device="cuda", generator=gen) / M ** 0.5
    Y = H @ W + 0.1 * torch.randn((N, O), dtype=torch.float64, device="cuda", generator=gen)
    Z = torch.cat([H, torch.ones((N, 1), dtype=torch.float64, device="cuda"), Y], 1)
    return (Z.T @ Z).contiguous()


def torch_ols(torch, G, M, O, K, lam, tol):
    """The baseline: forward selection with the ones column first, in torch ops, nothing read by the host -> sel [K + 1]."""
    n = M + 1
    A = G[:n, :n].clone()
    torch.diagonal(A)[:M] += lam
    d = torch.diagonal(A).clone()
    d0 = d.clone()
    c = G[:n, M + 1:].clone()
    avail = torch.ones(n, dtype=torch.bool, device=G.device)
    L = torch.zeros((K + 1, n), dtype=torch.float64, device=G.device)
    sel = torch.empty(K + 1, dtype=torch.long, device=G.device)
    zero = torch.zeros((), dtype=torch.float64, device=G.device)
    j = torch.full((1,), M, dtype=torch.long, device=G.device)
    for t in range(K + 1):
        if t > 0:
            ok = avail[:M] & (d[:M] > tol * d0[:M])
            score = torch.where(ok, (c[:M] * c[:M]).sum(1) / d[:M], zero)
            j = torch.argmax(score).reshape(1)
        sq = d.index_select(0, j).sqrt()
        a = A.index_select(0, j).squeeze(0)                       # the row: A is symmetric
        col = a
        if t > 0:
            lj = L[:t].index_select(1, j).squeeze(1)
            col = a - torch.mv(L[:t].T, lj)
        col = torch.where(avail, col / sq, zero)
        col.index_copy_(0, j, sq)
        ly = c.index_select(0, j) / sq
        L[t] = col
        d -= torch.where(avail, col * col, zero)
        c -= col[:, None] * ly
        avail.index_fill_(0, j, False)
        sel[t] = j[0]
    return sel


def run_shape(name):
    import torch
    from irbfn_amd import _lib, ols
    lib = _lib.load()
    M, K, O = SHAPES[name]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    G = make_g(torch, M, O, gen)
    lam = 1e-8 * float(torch.diagonal(G)[:M].sum().item()) / M
    tol = ols.default_tol(M, True)
    npad = ols.npad(M)
    lbytes = (K + 1) * npad * 8
    print(f"-- {name}: M = {M}, K = {K}, O = {O} on {torch.cuda.get_device_name(0)}; factor L = {lbytes / 2 ** 20:.1f} MiB "
          f"({'fits' if lbytes <= LLC_MIB * 2 ** 20 else 'exceeds'} the {LLC_MIB} MiB last-level cache)")
    state = {}

    def kernel():
        state["st"] = ols._State(G, M, O, True, lam, tol, K, torch, lib)
        state["st"].steps(K + 1)

    def baseline():
        state["sel"] = torch_ols(torch, G, M, O, K, lam, tol)

    def span(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    kernel()
    baseline()
    torch.cuda.synchronize()
    st = state["st"]
    same = int((st.sel.to(torch.long) == state["sel"]).sum().item())
    print(f"   pivots taken {int(st.count.item())} of {K + 1}; the baseline names the same column at {same} of {K + 1} steps")
    t = {"kernel": [], "torch": []}
    for _ in range(ROUNDS):
        t["kernel"].append(span(kernel))
        t["torch"].append(span(baseline))
    for label, v in t.items():
        med = float(np.median(v))
        print(f"   selection, {label:7s} {med:10.2f} ms  [{min(v):.2f} .. {max(v):.2f}]  {med / (K + 1) * 1e3:8.1f} us per step")
    print(f"   torch / kernel = {np.median(t['torch']) / np.median(t['kernel']):.2f}")
    # inside one selection: the first and the last WINDOW steps
    w = min(WINDOW, K // 2)
    first, last = [], []
    for _ in range(ROUNDS):
        s = ols._State(G, M, O, True, lam, tol, K, torch, lib)
        s.steps(1)                                                 # the ones column
        first.append(span(lambda: s.steps(w)) / w * 1e3)
        s.steps(K - 2 * w)
        last.append(span(lambda: s.steps(w)) / w * 1e3)
    la = float(np.median(last))
    tl = K - (w - 1) / 2                                           # the mean t of the last steps
    print(f"   per step, steps 1 .. {w}: {float(np.median(first)):.1f} us [{min(first):.1f} .. {max(first):.1f}]; steps {K - w + 1} .. {K}: {la:.1f} us "
          f"[{min(last):.1f} .. {max(last):.1f}]")
    rate = tl * npad * 8 / (la * 1e-6) / 1e12
    print(f"   L read by a step at t = {tl:.0f}: {tl * npad * 8 / 2 ** 20:.1f} MiB -> {rate:.2f} TB/s over the whole step time "
          f"({rate / HBM_TBS * 100:.0f} % of {HBM_TBS} TB/s), of which {min(first):.1f} us are what a step costs with nothing to read")


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--step":
        import torch
        assert torch.cuda.is_available(), "profile_ols.py measures on the GPU"
        run_shape(sys.argv[2])
        return 0
    out = sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--out" else os.path.join(ROOT, "profiles", "ols.txt")
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
