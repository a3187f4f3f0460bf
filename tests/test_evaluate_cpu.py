"""CPU checks of the table evaluation (irbfn_amd/evaluate.py, irbfn_eval_rollout_errors): the symbols exist in header,
library and ctypes binding; the number of metrics per mode; every argument refusal is decided before any HIP call; the
histogram's bin function on its worked cases and at the edges of one octave; the metric-name tables; ``evaluate_table``
refuses a foreign net type."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from _evaluate_util import FRENET, FULLINT, KS, MODES, NUM_BINS, NUM_METRICS, SELECT, SPIRAL, bin_of, edge
from irbfn_amd import _lib, build, evaluate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("irbfn_eval_num_metrics", "irbfn_eval_workspace_bytes", "irbfn_eval_rollout_errors")
OK, BAD_ARG, UNSUPPORTED = 0, -1, -2


def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "irbfn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} not declared in include/irbfn_hip.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.SIGNATURES
    assert lib.irbfn_abi_version() == 1
    assert any(u[0] == "eval_errors.hip" for u in build.UNITS)
    assert "eval_irbfn_dnmpc.py:92-167" in hdr and "unpinned" in hdr


def test_num_metrics_and_workspace_per_mode():
    lib = _lib.load()
    assert [lib.irbfn_eval_num_metrics(m) for m in (SELECT, KS, FULLINT, FRENET)] == [9, 9, 7, 10]
    assert lib.irbfn_eval_num_metrics(SPIRAL) < 0                 # no controls
    assert lib.irbfn_eval_num_metrics(5) < 0 and lib.irbfn_eval_num_metrics(-1) < 0
    for m in MODES:
        assert lib.irbfn_eval_workspace_bytes(m) > 0 and lib.irbfn_eval_workspace_bytes(m) % 8 == 0
    assert lib.irbfn_eval_workspace_bytes(SPIRAL) < 0


def test_status_table_without_gpu():
    lib = _lib.load()
    one = C.c_void_p(8)                          # a non-null pointer that is never dereferenced: every call below stops earlier
    dyn = (C.c_float * 16)()
    big = 1 << 30
    good = dict(mode=FRENET, state0=one, yp=one, y=one, dyn=dyn, B=4, T=5, row0=0, acc=1, err=one, stats=one, argmax=one,
                hist=one, ws=one, nbytes=big)

    def call(**kw):
        a = dict(good, **kw)
        return lib.irbfn_eval_rollout_errors(a["mode"], a["state0"], a["yp"], a["y"], a["dyn"], a["B"], a["T"], a["row0"],
                                             a["acc"], a["err"], a["stats"], a["argmax"], a["hist"], a["ws"], a["nbytes"], None)
    assert call(mode=5) == BAD_ARG and call(mode=-1) == BAD_ARG
    assert call(B=-1) == BAD_ARG
    assert call(T=0) == BAD_ARG and call(T=-3) == BAD_ARG
    for k in ("state0", "yp", "y", "stats", "argmax", "hist", "ws"):
        assert call(**{k: None}) == BAD_ARG, k
    assert call(dyn=None) == BAD_ARG                              # a model with parameters and none given
    assert call(mode=SELECT, dyn=None) == BAD_ARG and call(mode=KS, dyn=None) == BAD_ARG
    assert call(T=65) == UNSUPPORTED and call(mode=FULLINT, dyn=None, T=65) == UNSUPPORTED
    assert call(mode=SPIRAL) == UNSUPPORTED and call(mode=SPIRAL, dyn=None, T=1) == UNSUPPORTED
    assert call(nbytes=lib.irbfn_eval_workspace_bytes(FRENET) - 1) == BAD_ARG
    # a bad argument wins over an unsupported shape
    assert call(T=65, stats=None) == BAD_ARG and call(mode=SPIRAL, B=-1) == BAD_ARG
    # an empty batch that accumulates touches nothing: no row pointer is needed, no launch is made
    assert call(B=0, state0=None, yp=None, y=None, err=None) == OK
    assert call(B=0, mode=FULLINT, dyn=None, state0=None, yp=None, y=None, err=None) == OK
    assert call(B=0, stats=None) == BAD_ARG


def test_bin_function_worked_cases_and_one_octave():
    f = lambda v: int(bin_of(np.float32(v)).reshape(-1)[0])
    assert f(1.0) == 320 and f(1.125) == 321
    assert f(2.0 ** -40) == 0 and f(2.0 ** -41) == 0 and f(2.0 ** -60) == 0
    assert f(0.0) == 0
    assert f(1e-45) == 0 and f(np.float32(2.0 ** -149)) == 0 and f(1.1e-38) == 0        # subnormals
    assert f(2.0 ** 24) == 511 and f(2.0 ** 30) == 511 and f(np.finfo(np.float32).max) == 511
    assert f(edge(511)) == 511 and f(np.nextafter(np.float32(edge(511)), np.float32(0))) == 510
    assert edge(320) == 1.0 and edge(321) == 1.125 and edge(328) == 2.0 and edge(0) == 2.0 ** -40
    # both sides of every edge of the octave [1, 2): the edge itself opens bin k, the float32 below it closes bin k - 1
    for k in range(320, 329):
        e = np.float32(edge(k))
        assert float(e) == edge(k)                                # edges are float32 numbers
        assert f(e) == k and f(np.nextafter(e, np.float32(0))) == k - 1 and f(np.nextafter(e, np.float32(4))) == k
        assert edge(k + 1) / edge(k) <= 9.0 / 8.0
    # the product's own statement of bin and edge is the same
    v = (np.abs(np.random.default_rng(0).normal(size=4096)) * 2.0 ** np.arange(-48, 16).repeat(64)).astype(np.float32)
    assert np.array_equal(evaluate.bin_of(v), bin_of(v))
    assert all(evaluate.bin_edge(k) == edge(k) for k in range(NUM_BINS + 1))
    inside = (bin_of(v) > 0) & (bin_of(v) < NUM_BINS - 1)
    lo = np.array([edge(k) for k in bin_of(v)])
    hi = np.array([edge(k + 1) for k in bin_of(v)])
    assert ((lo <= v) & (v < hi))[inside].all() and (v[bin_of(v) == 0] < edge(1)).all()


def test_metric_name_tables():
    assert set(evaluate.METRIC_NAMES) == set(MODES)
    for m in MODES:
        names = evaluate.METRIC_NAMES[m]
        assert len(names) == NUM_METRICS[m] == _lib.load().irbfn_eval_num_metrics(m)
        assert names[-2:] == ("position", "controls") and len(set(names)) == len(names)
    assert evaluate.METRIC_NAMES[FULLINT] == ("x", "y", "delta", "v", "yaw", "position", "controls")
    assert evaluate.METRIC_NAMES[FRENET][:8] == ("s", "ey", "delta", "vx", "vy", "wz", "epsi", "cur")
    assert evaluate.METRIC_NAMES[SELECT] == evaluate.METRIC_NAMES[KS]
    assert {k: v[0] for k, v in evaluate.KINDS.items()} == {"cartesian": FULLINT, "cartesian_st": SELECT, "frenet": FRENET}


def test_evaluate_table_refuses_a_foreign_net_type_and_kind():
    class NotANet:
        in_features, out_features = 8, 10

    with pytest.raises(TypeError):
        evaluate.evaluate_table(NotANet(), {}, np.zeros((4, 8), np.float32), np.zeros((4, 10), np.float32), "frenet")
    from irbfn_amd import configs
    from irbfn_amd.model import WCRBFNet
    net = WCRBFNet.from_config(dict(configs.model_card(2)))
    with pytest.raises(ValueError):
        evaluate.evaluate_table(net, {}, np.zeros((4, 7), np.float32), np.zeros((4, 10), np.float32), "polar")
    with pytest.raises(ValueError):
        evaluate.evaluate_table(net, {}, np.zeros((4, 7), np.float32), np.zeros((4, 10), np.float32), "cartesian", mode=FRENET)
