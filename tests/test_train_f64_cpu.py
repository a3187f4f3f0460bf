"""CPU checks of float64 training: the ``*_f64`` entry points validate their arguments as their float32 twins do (before
any HIP call), ``config()`` carries ``use_float64`` only for a float64 net, and the models without a float64 mode say so."""
import ctypes as C

import numpy as np
import pytest

from irbfn_amd import _lib, configs
from irbfn_amd.model import _CFG_FIELDS, ClusterWCRBFNet, DeeperWCRBFNet, WCRBFNet

BAD = -1
P = C.c_void_p(1)           # a non-NULL pointer that no call below dereferences: each is rejected first
N = None


def test_f64_entry_points_reject_bad_arguments_like_their_twins():
    lib = _lib.load()
    dyn32 = np.zeros(13, np.float32)
    dyn64 = np.zeros(13, np.float64)
    d32, d64 = dyn32.ctypes.data_as(C.c_void_p), dyn64.ctypes.data_as(C.c_void_p)
    # (x, y_pred, y, gy, loss, partials, B, D, O)
    oneint = [(P, P, P, P, P, P, -1, 7, 2), (P, P, P, P, P, P, 4, 6, 2), (P, P, P, P, P, P, 4, 7, 1),
              (N, P, P, P, P, P, 4, 7, 2), (P, P, P, N, P, P, 4, 7, 2), (P, P, P, P, N, P, 4, 7, 2), (P, P, P, P, P, N, 0, 7, 2)]
    for x, yp, y, gy, lo, pa, B, D, O in oneint:
        got = lib.irbfn_train_seeds_oneint_f64(x, yp, y, d64, 0.5, gy, lo, pa, B, D, O, None)
        assert got == BAD and got == lib.irbfn_train_seeds_oneint(x, yp, y, d32, 0.5, gy, lo, pa, B, D, O, None)
    assert lib.irbfn_train_seeds_oneint_f64(P, P, P, None, 0.5, P, P, P, 4, 7, 2, None) == BAD
    # (x, y_pred, y, gy, loss, partials, B, D, T): bad arguments, and T > 64 unsupported
    fullint = [(P, P, P, P, P, P, -1, 7, 5), (P, P, P, P, P, P, 4, 0, 5), (P, P, P, P, P, P, 4, 7, 0), (P, P, P, P, P, P, 4, 7, 65),
               (N, P, P, P, P, P, 4, 7, 5), (P, P, P, P, N, P, 4, 7, 5), (P, P, P, P, P, N, 0, 7, 5)]
    for x, yp, y, gy, lo, pa, B, D, T in fullint:
        got = lib.irbfn_train_seeds_fullint_f64(x, yp, y, 0.5, gy, lo, pa, B, D, T, None)
        assert got < 0 and got == lib.irbfn_train_seeds_fullint(x, yp, y, 0.5, gy, lo, pa, B, D, T, None)
    assert lib.irbfn_train_seeds_fullint_f64(P, P, P, 0.5, P, P, P, 4, 7, 65, None) == -2
    frenet = [(P, P, P, P, P, P, -1, 8, 5), (P, P, P, P, P, P, 4, 7, 5), (P, P, P, P, P, P, 4, 8, 0), (P, P, P, P, P, P, 4, 8, 17),
              (P, N, P, P, P, P, 4, 8, 5), (P, P, P, P, N, P, 4, 8, 5)]
    for x, yp, y, gy, lo, pa, B, D, T in frenet:
        got = lib.irbfn_train_seeds_frenet_fullint_f64(x, yp, y, d64, 0.5, gy, lo, pa, B, D, T, None)
        assert got == BAD and got == lib.irbfn_train_seeds_frenet_fullint(x, yp, y, d32, 0.5, gy, lo, pa, B, D, T, None)
    assert lib.irbfn_train_seeds_frenet_fullint_f64(P, P, P, None, 0.5, P, P, P, 4, 8, 5, None) == BAD
    # (params, grads, m, v, n, step, partials)
    adam = [(P, P, P, P, -1, P, P), (P, P, P, P, 4, N, P), (P, P, P, P, 4, P, N), (N, P, P, P, 4, P, P), (P, P, P, N, 4, P, P)]
    for p, g, m, v, n, st, pa in adam:
        got = lib.irbfn_adam_clip_step_f64(p, g, m, v, n, st, 1e-3, 0.9, 0.999, 1e-8, 1.0, pa, None)
        assert got == BAD and got == lib.irbfn_adam_clip_step(p, g, m, v, n, st, 1e-3, 0.9, 0.999, 1e-8, 1.0, pa, None)


def test_config_round_trips_use_float64():
    card = configs.model_card(2)
    net = WCRBFNet.from_config(card, use_float64=True)
    cfg = net.config()
    assert cfg["use_float64"] is True
    back = WCRBFNet.from_config(cfg)
    assert back.use_float64 and back.config() == cfg


def test_float32_card_has_no_new_key():
    card = configs.model_card(2)
    cfg = WCRBFNet.from_config(card).config()
    assert "use_float64" not in cfg
    assert set(cfg) == set(_CFG_FIELDS)
    assert WCRBFNet.from_config(cfg).use_float64 is False


def test_models_without_a_float64_mode_refuse_it():
    card = configs.model_card(2)
    with pytest.raises(ValueError, match="float64"):
        DeeperWCRBFNet.from_config(dict(card, use_float64=True))
    with pytest.raises(ValueError, match="float64"):
        ClusterWCRBFNet(in_features=8, out_features=10, num_kernels=8, basis_func="gaussian", num_regions=2, use_float64=True)
    DeeperWCRBFNet.from_config(card)          # float32: as before
