"""CPU side of the region-weighted K1g forward: the option and its enum in the header and in ``_lib``, and the float64
statement the GPU tests run against (tests/_cluster_gram_util.py)."""
import os
import re

import numpy as np

from _cluster_gram_util import gamma_forward64, softmax_gamma
from _cluster_util import cluster_case
from conftest import ROOT
from irbfn_amd import _lib
from oracle import irbfn_oracle as orc

HEADER = open(os.path.join(ROOT, "include", "irbfn_hip.h")).read()


def _enum(name):
    m = re.search(r"\b" + name + r"\s*=\s*(\d+)", HEADER)
    assert m, name
    return int(m.group(1))


def test_option_and_enum_agree_with_header():
    assert _lib.OPTIONS["fwd_gamma_kernel"] == _enum("IRBFN_OPT_FWD_GAMMA_KERNEL") == 17
    assert _enum("IRBFN_OPT_COUNT") == 18 == max(_lib.OPTIONS.values()) + 1
    assert (_lib.FWDG_AUTO, _lib.FWDG_K1, _lib.FWDG_K1G) == (_enum("IRBFN_FWDG_AUTO"), _enum("IRBFN_FWDG_K1"), _enum("IRBFN_FWDG_K1G")) == (0, 1, 2)
    assert "typedef enum irbfn_fwd_gamma_kernel" in HEADER
    assert re.search(r"#define IRBFN_ABI_VERSION 1\b", HEADER)


def test_new_unit_is_built():
    from irbfn_amd import build
    assert any(u[0] == "rbf_forward_gram_gamma.hip" for u in build.UNITS)


def test_statement_equals_cluster_oracle():
    for basis in ("gaussian", "inverse_quadratic", "inverse_multiquadric"):
        _, cfg, params, x = cluster_case(3, R=5, K=7, O=4, B=37, D=8, basis=basis)
        ref, _ = orc.cluster_wcrbfnet_apply(cfg, params, x.astype(np.float64))
        out, scale = gamma_forward64(cfg, params, x, softmax_gamma(params, x))
        assert np.abs(out - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
        assert (scale >= np.abs(out - np.asarray(params["params"]["linear"]["bias"], np.float64)) - 1e-12).all()


def test_statement_takes_arbitrary_gamma():
    rng, cfg, params, x = cluster_case(4, R=3, K=5, O=2, B=9, D=8)
    p = params["params"]
    bias = np.asarray(p["linear"]["bias"], np.float64)
    out0, scale0 = gamma_forward64(cfg, params, x, np.zeros((9, 3)))
    assert np.array_equal(out0, np.broadcast_to(bias, out0.shape)) and not scale0.any()
    g = rng.uniform(-1, 1, size=(9, 3))
    out, scale = gamma_forward64(cfg, params, x, g)
    phi = orc.rbf_layer(x.astype(np.float64), p["rbf_list"]["centers"].astype(np.float64), p["rbf_list"]["log_sigs"].astype(np.float64), "gaussian")
    W = p["linear"]["kernel"].astype(np.float64)
    brute = np.einsum("br,brk,ko->bo", g, phi, W) + bias
    assert np.abs(out - brute).max() <= 1e-12
    assert np.abs(scale - np.einsum("br,brk,ko->bo", np.abs(g), phi, np.abs(W))).max() <= 1e-12
    onehot = np.zeros((9, 3)); onehot[:, 1] = 1.0
    out1, _ = gamma_forward64(cfg, params, x, onehot)
    assert np.abs(out1 - (phi[:, 1] @ W + bias)).max() <= 1e-12
    g[4, 2] = np.nan
    outn, _ = gamma_forward64(cfg, params, x, g)
    assert np.isnan(outn[4]).all() and np.isfinite(np.delete(outn, 4, 0)).all()
