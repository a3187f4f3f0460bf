"""Fixed-centre and fixed-width RBF nets (the reference's layer classes, src/irbfn_mpc/model.py:131-140) without a GPU:
constructor, reduced trees, model card, checkpoints shaped like the two upstream ones, flat buffers, ABI validation."""
import ctypes as C
import os
import warnings

import msgpack
import numpy as np
import pytest
import torch

from irbfn_amd import checkpoint, distributed
from irbfn_amd.model import ClusterWCRBFNet, DeeperWCRBFNet, WCRBFNet

D, O = 8, 10


def card(K, R=1):
    return dict(in_features=D, out_features=O, num_kernels=K, basis_func="gaussian", num_regions=R,
                lower_bounds=[[-1.0]], upper_bounds=[[1.0]], dimension_ranges=[[0]] * R, activation_idx=[0], delta=[0.1])


def test_constructor_centre_shapes():
    rng = np.random.default_rng(0)
    c3 = rng.normal(size=(2, 16, D)).astype(np.float32)
    net = WCRBFNet(**card(16, R=2), centers=c3, fixed_centers=True)
    assert net.frozen == ("centers",)
    np.testing.assert_array_equal(net.centers, c3)
    c2 = rng.normal(size=(16, D)).astype(np.float32)
    net = WCRBFNet(**card(16, R=2), centers=c2, fixed_width=True)
    assert net.frozen == ("centers", "log_sigs")
    assert net.centers.shape == (2, 16, D)
    np.testing.assert_array_equal(net.centers[1], c2)
    np.testing.assert_array_equal(net.log_sigs, np.zeros((2, 16)))
    for bad in (np.zeros((3, 16, D)), np.zeros((16, D + 1)), np.zeros((16,))):
        with pytest.raises(ValueError):
            WCRBFNet(**card(16, R=2), centers=bad)


def test_flags_without_centres_warn_and_freeze_nothing():
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        net = WCRBFNet(**card(16), fixed_centers=True)
    assert any("freeze nothing" in str(x.message) for x in w)
    assert net.frozen == ()
    p = net.init()["params"]
    assert set(p["rbf_list"]) == {"centers", "log_sigs"}
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        WCRBFNet(**card(16), fixed_width=True)
    assert len(w) >= 1


def test_init_trees_per_mode():
    c = np.random.default_rng(1).normal(size=(1, 32, D)).astype(np.float32)
    warm = WCRBFNet(**card(32), centers=c).init()["params"]
    assert set(warm) == {"rbf_list", "linear"} and set(warm["rbf_list"]) == {"centers", "log_sigs"}
    np.testing.assert_array_equal(warm["rbf_list"]["centers"], c)
    fc = WCRBFNet(**card(32), centers=c, fixed_centers=True).init()["params"]
    assert set(fc) == {"rbf_list", "linear"} and set(fc["rbf_list"]) == {"log_sigs"}
    assert fc["rbf_list"]["log_sigs"].shape == (1, 32)
    fw = WCRBFNet(**card(32), centers=c, fixed_width=True).init()["params"]
    assert set(fw) == {"linear"}
    assert fw["linear"]["kernel"].shape == (32, O) and fw["linear"]["bias"].shape == (O,)


def test_tree_with_a_frozen_leaf_raises():
    c = np.zeros((1, 32, D), np.float32)
    net = WCRBFNet(**card(32), centers=c, fixed_centers=True)
    full = WCRBFNet(**card(32)).init()["params"]
    with pytest.raises(ValueError, match="centers"):
        net._check_shapes(full)
    net._check_shapes(net.init()["params"])
    fw = WCRBFNet(**card(32), centers=c, fixed_width=True)
    with pytest.raises(ValueError, match="log_sigs"):
        fw._check_shapes({"rbf_list": {"log_sigs": np.zeros((1, 32))}, "linear": full["linear"]})


def test_config_round_trip():
    c = np.random.default_rng(2).normal(size=(32, D)).astype(np.float32)
    for kw in (dict(fixed_centers=True), dict(fixed_width=True, log_sigs=0.5), dict(fixed_width=True)):
        net = WCRBFNet(**card(32), centers=c, **kw)
        cfg = net.config()
        assert cfg.get("fixed_centers", False) == kw.get("fixed_centers", False)
        assert cfg.get("fixed_width", False) == kw.get("fixed_width", False)
        back = WCRBFNet.from_config(cfg, centers=c)
        assert back.frozen == net.frozen
        np.testing.assert_array_equal(back.centers, net.centers)
        if net.log_sigs is not None:
            np.testing.assert_array_equal(back.log_sigs, net.log_sigs)
    plain = WCRBFNet(**card(32)).config()
    assert "fixed_centers" not in plain and "fixed_width" not in plain and "log_sigs" not in plain


def test_deeper_and_cluster_refuse_frozen_centres():
    c = np.zeros((1, 32, D), np.float32)
    with pytest.raises(NotImplementedError):
        DeeperWCRBFNet(**card(32), centers=c, fixed_centers=True)
    with pytest.raises(NotImplementedError):
        ClusterWCRBFNet(in_features=D, out_features=O, num_kernels=32, basis_func="gaussian", num_regions=1, centers=c,
                        fixed_width=True)


def _arr(a):
    a = np.asarray(a)
    return msgpack.ExtType(1, msgpack.packb((list(a.shape), a.dtype.name, a.tobytes()), use_bin_type=True))


def _write(path, params, step=7):
    """A flax checkpoint as the reference writes it (ext type 1 arrays; chain(clip, adam) optimiser state)."""
    def conv(t):
        return {k: conv(v) for k, v in t.items()} if isinstance(t, dict) else _arr(t)
    zeros = {g: {n: np.zeros_like(a) for n, a in d.items()} for g, d in params.items()}
    adam = {"count": _arr(np.asarray(3, np.int32)), "mu": {"params": conv(zeros)}, "nu": {"params": conv(zeros)}}
    tree = {"step": _arr(np.asarray(step, np.int64)), "params": {"params": conv(params)},
            "opt_state": {"0": {}, "1": {"0": adam, "1": {}}}}
    with open(path, "wb") as f:
        f.write(msgpack.packb(tree, use_bin_type=True))


UPSTREAM = {
    # dnmpc_fixed_constraint_centers_mode: fixed centres, 500 kernels
    "fixed_centers": {"rbf_list": {"log_sigs": np.random.default_rng(3).normal(size=(1, 500)).astype(np.float32)},
                      "linear": {"kernel": np.random.default_rng(4).normal(size=(500, O)).astype(np.float32),
                                 "bias": np.arange(O, dtype=np.float32)}},
    # dnmpc_fixed_width_mode_1000: fixed width, 1000 kernels
    "fixed_width": {"linear": {"kernel": np.random.default_rng(5).normal(size=(1000, O)).astype(np.float32),
                               "bias": np.arange(O, dtype=np.float32)}},
}


@pytest.mark.parametrize("mode", sorted(UPSTREAM))
def test_checkpoint_round_trip_of_upstream_shapes(tmp_path, mode):
    src = UPSTREAM[mode]
    _write(str(tmp_path / "checkpoint_7"), src)
    params, step = checkpoint.restore_checkpoint(str(tmp_path))
    assert step == 7
    p = params["params"]
    assert set(p) == set(src)
    for g in src:
        for n in src[g]:
            np.testing.assert_array_equal(p[g][n], src[g][n])
    mu, nu, count = checkpoint.restore_opt_state(str(tmp_path))
    assert count == 3 and set(mu["params"]) == set(src)
    # write it back with moments and read it again
    mu2 = {"params": {g: {n: a + 1 for n, a in d.items()} for g, d in p.items()}}
    out = checkpoint.save_checkpoint(str(tmp_path / "again"), params, 8, opt_state=(mu2, nu, 4))
    params2, step2 = checkpoint.restore_checkpoint(out)
    assert step2 == 8
    for g in src:
        for n in src[g]:
            np.testing.assert_array_equal(params2["params"][g][n], src[g][n])
    mu3, _, count3 = checkpoint.restore_opt_state(out)
    assert count3 == 4
    for g in src:
        for n in src[g]:
            np.testing.assert_array_equal(mu3["params"][g][n], src[g][n] + 1)
    # the net of the checkpoint takes the tree
    K = src["linear"]["kernel"].shape[0]
    net = WCRBFNet(**card(K), centers=np.zeros((K, D), np.float32), **{mode: True})
    net._check_shapes(params2["params"])


def test_mlp_baseline_still_rejected(tmp_path):
    _write(str(tmp_path / "checkpoint_1"), {"Dense_0": {"kernel": np.zeros((8, 4), np.float32), "bias": np.zeros(4, np.float32)}})
    with pytest.raises(ValueError, match="MLP baseline"):
        checkpoint.restore_checkpoint(str(tmp_path))
    _write(str(tmp_path / "checkpoint_2"), {"Dense_0": {"kernel": np.zeros((8, 4), np.float32), "bias": np.zeros(4, np.float32)},
                                            "linear": {"kernel": np.zeros((4, 2), np.float32), "bias": np.zeros(2, np.float32)}})
    with pytest.raises(ValueError):
        checkpoint.restore_checkpoint(str(tmp_path))


@pytest.mark.parametrize("kw,count", [({}, 32 * D + 32 + 32 * O + O), ({"fixed_centers": True}, 32 + 32 * O + O),
                                      ({"fixed_width": True}, 32 * O + O)])
def test_flat_buffers_per_mode(kw, count):
    c = np.random.default_rng(6).normal(size=(32, D)).astype(np.float32)
    net = WCRBFNet(**card(32), centers=c, **kw)
    p = net.init(seed=3)
    assert distributed.flat_param_count(net) == count
    flat = distributed.flatten_params(distributed.params_to_device(p, torch.device("cpu")))
    assert flat.numel() == count
    back = distributed.unflatten_params(net, flat)["params"]
    assert {g: set(d) for g, d in back.items()} == {g: set(d) for g, d in p["params"].items()}
    for g, d in p["params"].items():
        for n, a in d.items():
            np.testing.assert_array_equal(back[g][n].numpy(), a)
    with pytest.raises(ValueError):
        distributed.unflatten_params(net, flat[:-1])


def _lib_or_skip():
    from irbfn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libirbfn_hip.so not built")
    return _lib.load()


def test_vjp_frozen_argument_validation_without_gpu():
    lib = _lib_or_skip()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    # NULL net
    assert lib.irbfn_net_vjp_frozen(None, p, p, None, None, p, p, 1, p, 1 << 20, None) == -1
    # NULL g_kernel / g_bias: refused before the descriptor is touched (a stand-in handle is never dereferenced)
    assert lib.irbfn_net_vjp_frozen(p, p, p, None, None, None, p, 1, p, 1 << 20, None) == -1
    assert lib.irbfn_net_vjp_frozen(p, p, p, None, None, p, None, 1, p, 1 << 20, None) == -1
    assert lib.irbfn_net_vjp_frozen(None, p, p, p, p, p, p, -1, p, 1 << 20, None) == -1
