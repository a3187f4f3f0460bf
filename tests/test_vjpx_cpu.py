"""CPU checks of the query VJP: the three entry points exist in header, library and ctypes binding and reject bad arguments
without a GPU; the NumPy statement of the formula (tests/_vjpx_util.py::hand_gx), on which the GPU tests lean for queries that
sit on a centre and for the error model, equals torch.autograd of the float64 restatement; ``_WCRBFApply.backward`` asks for
the query gradient only when x requires one."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _vjpx_util as vx
from irbfn_amd import _lib, autograd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("irbfn_net_vjp_x", "irbfn_net_vjp_x_gamma", "irbfn_f64_vjp_x")


def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "irbfn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} not declared in include/irbfn_hip.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.SIGNATURES
    assert "are never taken by the reference and are\n * not produced" not in hdr
    assert _lib.OPTIONS["vjpx_kernel"] == 16 and (_lib.VJPX_AUTO, _lib.VJPX_K5, _lib.VJPX_K5M) == (0, 1, 2)
    assert lib.irbfn_abi_version() == 1


def test_arg_validation_without_gpu():
    lib = _lib.load()
    one = C.c_void_p(8)                          # a non-null pointer that is never dereferenced: every call below stops earlier
    # no descriptor / negative batch
    assert lib.irbfn_net_vjp_x(None, one, one, one, 4, None) == -1
    assert lib.irbfn_net_vjp_x(None, one, one, one, -1, None) == -1
    assert lib.irbfn_net_vjp_x_gamma(None, one, one, one, one, one, 4, None) == -1
    assert lib.irbfn_net_vjp_x_gamma(None, one, one, one, one, None, 0, None) == -1
    # float64: no card, an invalid card, negative B, B = 0 no-op, null arrays
    assert lib.irbfn_f64_vjp_x(None, one, one, one, one, one, one, 4, None, 0, None) == -1
    card = _lib.F64Card(7, 1, 10, 2, 0, 0, 0, 0, None, None, None, None)
    bad = _lib.F64Card(9, 1, 10, 2, 0, 0, 0, 0, None, None, None, None)        # D > 8
    assert lib.irbfn_f64_vjp_x(C.byref(bad), one, one, one, one, one, one, 4, None, 0, None) == -1
    assert lib.irbfn_f64_vjp_x(C.byref(card), one, one, one, one, one, one, -1, None, 0, None) == -1
    assert lib.irbfn_f64_vjp_x(C.byref(card), None, None, None, None, None, None, 0, None, 0, None) == 0
    assert lib.irbfn_f64_vjp_x(C.byref(card), one, one, one, None, one, one, 4, None, 0, None) == -1
    assert lib.irbfn_f64_vjp_x(C.byref(card), one, one, one, one, one, None, 4, None, 0, None) == -1


@pytest.mark.parametrize("basis", vx.BASES)
def test_hand_formula_equals_autograd_of_the_restatement(basis):
    cfg, params = vx.synth_net(11, D=7, O=10, K=50, grid=(2, 2), basis=basis, extra_regions=1)
    x = vx.queries(11, cfg, 256)
    g = vx.cotangent(11, 256, 10)
    # off the centres: the restatement's sqrt has no derivative at 0, and linear / poisson_* diverge there
    assert vx.min_scaled_distance(params, x) >= 1e-3
    ref = vx.ref_gx(cfg, params, x, g)
    gx, S = vx.hand_gx(cfg, params, x, g, np.float64)
    assert np.isfinite(ref).all() and np.abs(ref).max() > 0
    assert np.abs(gx - ref).max() <= 1e-12 * np.abs(ref).max()
    assert (S >= np.abs(gx) * (1 - 1e-12)).all()
    # the gate term is part of it: without it the formula misses the reference
    gx_rbf, _, _ = vx.hand_gx(cfg, params, x, g, np.float64, gamma=vx._gate(cfg, np.asarray(x, np.float64), np.float64)[0])
    assert np.abs(gx_rbf - ref).max() > 1e-6 * np.abs(ref).max()


def test_hand_formula_on_a_centre_is_finite():
    for basis in vx.BASES:
        cfg, params = vx.synth_net(5, D=3, O=2, K=8, grid=(2,), basis=basis)
        x = np.asarray(vx.inner(params)["rbf_list"]["centers"][1, :4], np.float32).copy()
        gx, S = vx.hand_gx(cfg, params, x, vx.cotangent(5, 4, 2), np.float64)
        assert np.isfinite(gx).all() and np.isfinite(S).all()


class _StubNet:
    """Stands in for WCRBFNet behind _WCRBFApply: records which VJPs backward asks for."""

    def __init__(self):
        self.calls = []

    def apply(self, params, x):
        return x @ params["linear"]["kernel"][: x.shape[1]] + params["linear"]["bias"]

    def vjp(self, params, x, gout):
        self.calls.append("vjp")
        z = {k: {n: torch.zeros_like(v) for n, v in d.items()} for k, d in params.items()}
        return {"params": z}

    def vjp_x(self, params, x, gout):
        self.calls.append("vjp_x")
        return gout @ params["linear"]["kernel"][: x.shape[1]].t()


def _stub_params():
    t = lambda *s: torch.ones(s, requires_grad=True)
    return {"rbf_list": {"centers": t(1, 4, 3), "log_sigs": t(1, 4)}, "linear": {"kernel": t(4, 2), "bias": t(2)}}


def test_backward_takes_the_query_gradient_only_when_x_requires_it():
    net, p = _StubNet(), _stub_params()
    x = torch.arange(6.0).reshape(2, 3)
    autograd.wcrbf_apply(net, p, x).sum().backward()
    assert net.calls == ["vjp"] and x.grad is None
    net, p = _StubNet(), _stub_params()
    x = torch.arange(6.0).reshape(2, 3).requires_grad_()
    autograd.wcrbf_apply(net, p, x).sum().backward()
    assert net.calls == ["vjp", "vjp_x"]
    assert torch.equal(x.grad, torch.full((2, 3), 2.0))
    assert p["linear"]["kernel"].grad is not None
