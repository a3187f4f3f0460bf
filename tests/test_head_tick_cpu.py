"""CPU checks of the planning tick of DeeperWCRBFNet / ClusterWCRBFNet: the three entry points exist in header, library and
ctypes binding; their status table holds without a GPU (every status below is decided before any HIP call);
``irbfn_mlp_head_tick_needs_controls`` over modes and widths; ``plan_tick`` / ``plan_batch`` refuse a foreign type."""
import ctypes as C
import os
import re

import pytest

from irbfn_amd import _lib, planner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("irbfn_mlp_head_tick", "irbfn_mlp_head_tick_needs_controls", "irbfn_plan_tick_gamma")
OK, BAD_ARG, UNSUPPORTED = 0, -1, -2
ROLL_MODES = (_lib.ROLLOUT_ST_SELECT, _lib.ROLLOUT_ST_KS, _lib.ROLLOUT_FULLINT, _lib.ROLLOUT_FRENET_LS)


def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "irbfn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} not declared in include/irbfn_hip.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.SIGNATURES
    assert lib.irbfn_abi_version() == 1


def _head_tick(lib, h1, w2, b2, w3, b3, mode, mirror, state0, dyn, ctrl, states, B, H1, H2, O, T):
    return lib.irbfn_mlp_head_tick(h1, w2, b2, w3, b3, mode, mirror, state0, dyn, ctrl, states, B, H1, H2, O, T, None)


def test_head_tick_status_table_without_gpu():
    lib = _lib.load()
    one = C.c_void_p(8)                          # a non-null pointer that is never dereferenced: every call below stops earlier
    dyn = (C.c_float * 16)()
    FR = _lib.ROLLOUT_FRENET_LS
    good = dict(h1=one, w2=one, b2=one, w3=one, b3=one, mode=FR, mirror=one, state0=one, dyn=dyn, ctrl=one, states=one,
                B=4, H1=64, H2=64, O=10, T=5)
    call = lambda **kw: _head_tick(lib, **dict(good, **kw))
    # no roll-out mode, negative batch, no horizon, O != 2T
    assert call(mode=5) == BAD_ARG and call(mode=-1) == BAD_ARG
    assert call(B=-1) == BAD_ARG
    assert call(T=0) == BAD_ARG
    assert call(O=9) == BAD_ARG and call(O=10, T=4) == BAD_ARG
    # an empty batch is a no-op, whatever the pointers
    assert call(B=0, h1=None, w2=None, b2=None, w3=None, b3=None, state0=None, ctrl=None, states=None) == OK
    # required pointers
    for k in ("h1", "w2", "b2", "w3", "b3"):
        assert call(**{k: None}) == BAD_ARG, k
    assert call(state0=None) == BAD_ARG                       # states without initial states
    assert call(ctrl=None, states=None) == BAD_ARG            # both outputs null
    assert call(dyn=None) == BAD_ARG                          # a model with parameters and none given
    # outside the compiled set
    assert call(H1=32) == UNSUPPORTED and call(H2=128) == UNSUPPORTED
    assert call(mode=_lib.ROLLOUT_SPIRAL) == UNSUPPORTED
    # O > 16 goes through the controls buffer: required there
    assert call(O=20, T=10, ctrl=None) == BAD_ARG
    # a bad argument wins over an unsupported shape (the order of irbfn_plan_tick)
    assert call(H1=32, O=9) == BAD_ARG and call(H1=32, h1=None) == BAD_ARG


def test_head_entry_points_refuse_a_misaligned_h1_without_gpu():
    """h1_dev is read with 16-byte vector loads: the three head entry points return BAD_ARG for an address that is not a
    multiple of 16, before any HIP call (every other argument below is acceptable, so alignment alone decides; the aligned
    counterpart runs in tests/test_gpu_mlp_head.py::test_refusals).  No call reaches a launch: the fake pointers are never
    dereferenced.  The tick checks the address behind its shape checks: an unsupported shape keeps its status."""
    lib = _lib.load()
    ok = C.c_void_p(64)
    dyn = (C.c_float * 16)()
    FR = _lib.ROLLOUT_FRENET_LS
    nb = lib.irbfn_mlp_head_vjp_workspace_bytes(64, 64, 10)
    assert nb > 0
    for addr in (4, 8, 12, 20, 60, 68):
        bad = C.c_void_p(addr)
        tick = lambda h1, H1=64: _head_tick(lib, h1, ok, ok, ok, ok, FR, ok, ok, dyn, ok, ok, 4, H1, 64, 10, 5)
        assert tick(bad) == BAD_ARG, addr
        assert tick(bad, H1=32) == UNSUPPORTED and tick(ok, H1=32) == UNSUPPORTED
        fwd = lambda h1, H1=64, O=10: lib.irbfn_mlp_head_forward(h1, ok, ok, ok, ok, ok, 4, H1, 64, O, None)
        assert fwd(bad) == BAD_ARG and fwd(bad, O=20) == BAD_ARG, addr               # both forward kernels
        assert fwd(bad, H1=32) == BAD_ARG and fwd(ok, H1=32) == UNSUPPORTED          # here the bad argument wins
        for B in (1, 4, 80000):
            assert lib.irbfn_mlp_head_vjp(bad, ok, ok, ok, ok, ok, ok, ok, ok, ok, B, 64, 64, 10, ok, nb, None) == BAD_ARG, (addr, B)
    # an empty batch reads no h1: a no-op whatever the pointer (the VJP's, which still zeroes its leaves: on the GPU)
    assert lib.irbfn_mlp_head_forward(C.c_void_p(4), ok, ok, ok, ok, ok, 0, 64, 64, 10, None) == OK
    assert _head_tick(lib, C.c_void_p(4), ok, ok, ok, ok, FR, ok, ok, dyn, ok, ok, 0, 64, 64, 10, 5) == OK


def test_plan_tick_gamma_status_table_without_gpu():
    lib = _lib.load()
    one = C.c_void_p(8)
    dyn = (C.c_float * 16)()
    FR = _lib.ROLLOUT_FRENET_LS
    # no descriptor (a descriptor needs a device): every combination is a bad argument, B = 0 included
    assert lib.irbfn_plan_tick_gamma(None, FR, one, one, one, one, dyn, one, one, 4, 5, None) == BAD_ARG
    assert lib.irbfn_plan_tick_gamma(None, FR, one, one, one, one, dyn, one, one, 0, 5, None) == BAD_ARG
    assert lib.irbfn_plan_tick_gamma(None, 7, one, one, one, one, dyn, one, one, 4, 5, None) == BAD_ARG
    assert lib.irbfn_plan_tick_gamma(None, FR, one, one, one, one, dyn, one, one, -1, 5, None) == BAD_ARG
    assert lib.irbfn_plan_tick_gamma(None, FR, one, one, one, one, dyn, one, one, 4, 0, None) == BAD_ARG


@pytest.mark.parametrize("mode", ROLL_MODES + (_lib.ROLLOUT_SPIRAL,))
def test_head_tick_needs_controls(mode):
    lib = _lib.load()
    for O in (2, 10, 16, 18, 20):
        assert lib.irbfn_mlp_head_tick_needs_controls(mode, O, O // 2) == (1 if O > 16 else 0), (mode, O)
        assert lib.irbfn_mlp_head_tick_needs_controls(mode, O, O // 2 + 1) == BAD_ARG
    assert lib.irbfn_mlp_head_tick_needs_controls(mode, 0, 0) == BAD_ARG
    assert lib.irbfn_mlp_head_tick_needs_controls(9, 10, 5) == BAD_ARG


def test_planner_refuses_a_foreign_net_type():
    class NotANet:
        in_features, out_features = 8, 10

    with pytest.raises(TypeError):
        planner.plan_tick(NotANet(), {}, [[0.0] * 8], None, rollout=False)
    with pytest.raises(TypeError):
        planner.plan_batch(NotANet(), {}, [[0.0] * 8], [[0.0] * 8], None)
