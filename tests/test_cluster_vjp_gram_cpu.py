"""CPU side of the region-weighted matrix-core VJP (rbf_vjp_f16gram_gamma): the new value of the VJP option in the header and
in ``_lib``, and the float64 statement the GPU tests run against (tests/_cluster_vjp_gram_util.py)."""
import os
import re

import numpy as np

from _cluster_gram_util import softmax_gamma
from _cluster_util import CLEAVES, LEAVES, cluster_case, oracle_vjp
from _cluster_vjp_gram_util import STAGE, cluster_leaves_from_dgamma, gamma_vjp64
from conftest import ROOT
from irbfn_amd import _lib

HEADER = open(os.path.join(ROOT, "include", "irbfn_hip.h")).read()
FAST = ("gaussian", "inverse_quadratic", "inverse_multiquadric")


def _enum(name):
    m = re.search(r"\b" + name + r"\s*=\s*(\d+)", HEADER)
    assert m, name
    return int(m.group(1))


def test_enum_agrees_with_header():
    assert _lib.VJP_K2G_GAMMA == _enum("IRBFN_VJP_K2G_GAMMA") == 6
    assert (_lib.VJP_AUTO, _lib.VJP_K2, _lib.VJP_K2G, _lib.VJP_K2M) == (_enum("IRBFN_VJP_AUTO"), _enum("IRBFN_VJP_K2"), _enum("IRBFN_VJP_K2G"),
                                                                       _enum("IRBFN_VJP_K2M")) == (0, 1, 4, 5)
    assert _enum("IRBFN_OPT_COUNT") == 18 == max(_lib.OPTIONS.values()) + 1
    assert re.search(r"#define IRBFN_ABI_VERSION 1\b", HEADER)


def _case(basis):
    rng, cfg, params, x = cluster_case(5, R=5, K=7, O=4, B=37, D=8, basis=basis)
    g = rng.normal(size=(37, 4))
    gl = rng.normal(size=(37, 5))
    return cfg, params, x, g, gl


def test_statement_equals_cluster_oracle_on_the_stage_leaves():
    for basis in FAST:
        cfg, params, x, g, _ = _case(basis)
        ref, _ = oracle_vjp(cfg, params, x, g)
        leaves, _, _ = gamma_vjp64(cfg, params, x, softmax_gamma(params, x), g)
        for key, name in zip(LEAVES, STAGE):
            assert np.abs(leaves[name] - ref[key]).max() <= 1e-12 * np.abs(ref[key]).max(), (basis, name)


def test_dgamma_through_the_softmax_gives_the_cluster_leaves():
    for basis in FAST:
        cfg, params, x, g, gl = _case(basis)
        ref, ref_gl = oracle_vjp(cfg, params, x, g, gl)
        gamma = softmax_gamma(params, x)
        _, dgamma, scale = gamma_vjp64(cfg, params, x, gamma, g)
        assert (scale >= np.abs(dgamma) - 1e-12).all()
        for r, glv in ((ref, None), (ref_gl, gl)):
            wc, bc = cluster_leaves_from_dgamma(params, x, gamma, dgamma, glv)
            for got, key in ((wc, CLEAVES[4]), (bc, CLEAVES[5])):
                assert np.abs(got - r[key]).max() <= 1e-12 * np.abs(r[key]).max(), (basis, key)


def test_statement_takes_arbitrary_gamma():
    """d gamma does not depend on gamma; a region at gamma = 0 for every row has zero centre and width gradients."""
    cfg, params, x, g, _ = _case("gaussian")
    rng = np.random.default_rng(1)
    gam = rng.uniform(-1, 1, size=(37, 5))
    gam[:, 2] = 0.0
    leaves, dgamma, _ = gamma_vjp64(cfg, params, x, gam, g)
    _, dgamma2, _ = gamma_vjp64(cfg, params, x, softmax_gamma(params, x), g)
    assert np.abs(dgamma - dgamma2).max() <= 1e-12 * np.abs(dgamma).max()
    assert not leaves["centers"][2].any() and not leaves["log_sigs"][2].any()
    assert leaves["centers"][1].any()
    assert np.abs(leaves["bias"] - g.sum(0)).max() <= 1e-12
