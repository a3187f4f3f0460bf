"""out.npy of `bench.py --dump-outputs DIR` (config 2) from two trees: equality, max |delta| over sum_k |phi_k W_k|, and both
against the float64 oracle on 1024 rows.  python tools/compare_dumps.py PARENT_DIR RESULT_DIR (CPU only; run from the repository root)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
from irbfn_amd import configs  # noqa: E402
from oracle import irbfn_oracle as orc  # noqa: E402

a = np.load(os.path.join(sys.argv[1], "out.npy"))
b = np.load(os.path.join(sys.argv[2], "out.npy"))
cfg, P = configs.model_card(2), configs.synth_params(2)
x = configs.synth_queries(2)
assert a.shape == b.shape == (x.shape[0], cfg["out_features"]), (a.shape, b.shape, x.shape)
rows = np.random.default_rng(0).choice(x.shape[0], size=1024, replace=False)
p64 = orc.cast_params(P, np.float64)
pa = {"params": {"rbf_list": p64["params"]["rbf_list"],
                 "linear": {"kernel": np.abs(p64["params"]["linear"]["kernel"]), "bias": np.abs(p64["params"]["linear"]["bias"])}}}
x64 = x.astype(np.float64)
scale_rows = orc.wcrbfnet_apply(cfg, pa, x64[rows])
ref = orc.wcrbfnet_apply(cfg, p64, x64[rows])
print(f"full size [B={a.shape[0]}, O={a.shape[1]}]: array_equal(parent, result) = {np.array_equal(a, b)}; rows that differ {int((a != b).any(axis=1).sum())}; "
      f"max |delta| {np.abs(a - b).max():.3e}")
print(f"on 1024 rows: max |delta| / sum|phi W| {(np.abs(a[rows] - b[rows]) / scale_rows).max():.3e}")
for tag, o in (("parent", a), ("result", b)):
    e = np.abs(o[rows] - ref) / scale_rows
    print(f"{tag}: against the float64 oracle on 1024 rows: max {e.max():.3e} mean {e.mean():.3e}")
