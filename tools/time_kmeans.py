"""Times one Lloyd iteration (irbfn_kmeans_step) next to what a user can write without it on the same GPU: chunked
``torch.cdist`` -> ``argmin`` -> ``index_add_`` (float32 sums and counts; its labels come from a Gram expansion, so it does not
meet the library's label condition -- it is the speed yardstick only).

Shapes: N = 2^22 rows, D = 8 with K = 500 and K = 4096, D = 3 with K = 1000 (uniform rows, centres drawn from the rows).
One warm-up pass over every variant, then ROUNDS interleaved rounds (every variant once per round, INNER calls between two
device events); medians with min / max.  Tpairs/s = N K / time.  Also: the assignment alone (new_centers = NULL), the
k-means++ start and the wall time of ``fit(k=500, max_iter=20, init="kmeans++")`` on the D = 8 table.  GPU box; output kept
as profiles/kmeans.txt."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from irbfn_amd import _lib, kmeans  # noqa: E402
from irbfn_amd.model import _ptr, _stream_ptr  # noqa: E402

ROUNDS, INNER = 7, 3
N = 1 << 22
SHAPES = ((8, 500), (8, 4096), (3, 1000))
CHUNK = 1 << 16               # rows per cdist call: a [65536, K] float32 distance block (1 GiB at K = 4096)


def span(fn, n):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def measure(variants):
    """variants: [(label, fn)] -> {label: (median, min, max)} in us."""
    for _, fn in variants:
        fn()
    torch.cuda.synchronize()
    t = {label: [] for label, _ in variants}
    for _ in range(ROUNDS):
        for label, fn in variants:
            t[label].append(span(fn, INNER))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in t.items()}


def torch_step(x, c, labels, sums, counts):
    """The torch formulation of one iteration: labels, float32 sums and counts -> new centres (empty clusters keep theirs)."""
    sums.zero_()
    counts.zero_()
    for r0 in range(0, x.shape[0], CHUNK):
        xb = x[r0:r0 + CHUNK]
        lab = torch.cdist(xb, c).argmin(dim=1)
        labels[r0:r0 + CHUNK] = lab
        sums.index_add_(0, lab, xb)
        counts.index_add_(0, lab, torch.ones_like(lab, dtype=torch.float32))
    return torch.where(counts[:, None] > 0, sums / counts[:, None].clamp(min=1), c)


def main():
    assert torch.cuda.is_available(), "time_kmeans.py measures on the GPU"
    lib = _lib.load()
    stream = _stream_ptr(torch)
    print(f"k-means step (irbfn_kmeans_step) on {torch.cuda.get_device_name(0)}: N = {N}, {ROUNDS} rounds x {INNER} calls, "
          f"median us [min .. max]")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    tables = {}
    for D, K in SHAPES:
        if D not in tables:
            tables[D] = torch.rand((N, D), device="cuda", generator=gen) * 6 - 3
        x = tables[D]
        c = x[torch.randperm(N, device="cuda", generator=gen)[:K]].clone()
        labels = torch.full((N,), -1, dtype=torch.int32, device="cuda")
        new = torch.empty_like(c)
        counts = torch.zeros(K, dtype=torch.int64, device="cuda")
        stats = torch.zeros(4, dtype=torch.float64, device="cuda")
        ws = torch.empty(lib.irbfn_kmeans_workspace_bytes(N, K, D), dtype=torch.uint8, device="cuda")
        t_labels = torch.empty(N, dtype=torch.int64, device="cuda")
        t_sums, t_counts = torch.zeros_like(c), torch.zeros(K, device="cuda")

        def step(new_ptr=_ptr(new), cnt_ptr=_ptr(counts)):
            st = lib.irbfn_kmeans_step(_ptr(x), _ptr(c), _ptr(labels), None, new_ptr, cnt_ptr, _ptr(stats), N, K, D, _ptr(ws),
                                       ws.numel(), stream)
            assert st == 0, st
        res = measure([("irbfn_kmeans_step", step), ("torch cdist -> argmin -> index_add_", lambda: torch_step(x, c, t_labels, t_sums, t_counts)),
                       ("irbfn_kmeans_step, assign only", lambda: step(None, None))])
        print(f"-- D = {D}, K = {K}")
        for label, (med, lo, hi) in res.items():
            print(f"   {label:40s} {med:10.1f} us  [{lo:.1f} .. {hi:.1f}]   {N * K / med * 1e-6:6.3f} Tpairs/s")
        a, b = res["irbfn_kmeans_step"][0], res["torch cdist -> argmin -> index_add_"][0]
        print(f"   torch / step = {b / a:.2f}")
        # the two formulations on the same centres: how many labels differ, how far the centres are apart
        step()
        t_new = torch_step(x, c, t_labels, t_sums, t_counts)
        torch.cuda.synchronize()
        print(f"   labels that differ from torch's: {(t_labels != labels.long()).sum().item()} of {N}; "
              f"largest |centre - torch centre| = {(t_new - new).abs().max().item():.3e}; stats = {stats.tolist()}")
    x = tables[8]
    for label, fn in (("k-means++ start, k = 500", lambda: kmeans.fit(x, 500, max_iter=0, init="kmeans++")),
                      ('fit(k = 500, max_iter = 20, init = "kmeans++")', lambda: kmeans.fit(x, 500, max_iter=20, init="kmeans++")),
                      ('fit(k = 500, max_iter = 20, init = "random")', lambda: kmeans.fit(x, 500, max_iter=20, init="random"))):
        fn()
        torch.cuda.synchronize()
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        print(f"-- {label}: wall {np.median(walls) * 1e3:.1f} ms  [{min(walls) * 1e3:.1f} .. {max(walls) * 1e3:.1f}]"
              + (f", inertia {r.inertia:.6e}" if r.n_iter else ""))


if __name__ == "__main__":
    main()
