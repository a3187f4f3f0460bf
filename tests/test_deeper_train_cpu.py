"""DeeperWCRBFNet training without a GPU: the flat layout of its eight leaves, the unchanged layouts of the other models,
a checkpoint round trip with eight leaves, and the K2m entries of the ABI."""
import os
import re

import numpy as np
import torch

from conftest import ROOT, load_ckpt_fixture, load_deeper_fixture
from irbfn_amd import _lib, checkpoint, distributed
from irbfn_amd.model import ClusterWCRBFNet, DeeperWCRBFNet, WCRBFNet

ORDER = (("rbf_list", "centers"), ("rbf_list", "log_sigs"), ("linear_pre1", "kernel"), ("linear_pre1", "bias"),
         ("linear_pre2", "kernel"), ("linear_pre2", "bias"), ("linear", "kernel"), ("linear", "bias"))


def _torch_tree(P):
    return {"params": {g: {n: torch.from_numpy(np.asarray(v, np.float32)) for n, v in d.items()} for g, d in P["params"].items()}}


def test_deeper_tree_flattens_in_order_and_back():
    cfg, P, _, _ = load_deeper_fixture()
    net = DeeperWCRBFNet.from_config(cfg)
    assert net.live_leaves() == ORDER
    tp = _torch_tree(P)
    flat = distributed.flatten_params(distributed.params_to_device(tp, torch.device("cpu")))
    want = np.concatenate([np.asarray(P["params"][g][n], np.float32).reshape(-1) for g, n in ORDER])
    assert flat.numel() == distributed.flat_param_count(net) == want.size
    assert np.array_equal(flat.numpy(), want)
    back = distributed.unflatten_params(net, flat)["params"]
    for g, n in ORDER:
        assert np.array_equal(back[g][n].numpy(), np.asarray(P["params"][g][n], np.float32)), (g, n)
    again = distributed.broadcast_params(net, tp, device=torch.device("cpu"))["params"]
    for g, n in ORDER:
        assert np.array_equal(again[g][n].numpy(), np.asarray(P["params"][g][n], np.float32)), (g, n)


def test_other_flat_layouts_unchanged():
    cfg, P, *_ = load_ckpt_fixture("dnmpc_1regions_newdata_oldintloss_nomirror_highk")
    net = WCRBFNet.from_config(cfg)
    four = (("rbf_list", "centers"), ("rbf_list", "log_sigs"), ("linear", "kernel"), ("linear", "bias"))
    flat = distributed.flatten_params(distributed.params_to_device(_torch_tree(P), torch.device("cpu")))
    assert np.array_equal(flat.numpy(), np.concatenate([np.asarray(P["params"][g][n], np.float32).reshape(-1) for g, n in four]))
    assert distributed.flat_param_count(net) == flat.numel()
    # fixed-centre net: the live leaves only, in the same order
    c = np.asarray(P["params"]["rbf_list"]["centers"])
    frozen = WCRBFNet.from_config(dict(cfg, fixed_centers=True), centers=c)
    red = {"params": {"rbf_list": {"log_sigs": P["params"]["rbf_list"]["log_sigs"]}, "linear": P["params"]["linear"]}}
    f2 = distributed.flatten_params(distributed.params_to_device(_torch_tree(red), torch.device("cpu")))
    assert np.array_equal(f2.numpy(), np.concatenate([np.asarray(red["params"][g][n], np.float32).reshape(-1) for g, n in four[1:]]))
    assert distributed.flat_param_count(frozen) == f2.numel()
    # ClusterWCRBFNet: its stage's four leaves first (ClusterTrainState appends cluster.kernel and cluster.bias)
    cl = ClusterWCRBFNet(in_features=8, out_features=10, num_kernels=20, basis_func="gaussian", num_regions=3)
    rng = np.random.default_rng(0)
    cp = {"params": {"rbf_list": {"centers": rng.normal(size=(3, 20, 8)), "log_sigs": rng.normal(size=(3, 20))},
                     "linear": {"kernel": rng.normal(size=(20, 10)), "bias": rng.normal(size=10)},
                     "cluster": {"kernel": rng.normal(size=(8, 3)), "bias": rng.normal(size=3)}}}
    f3 = distributed.flatten_params(distributed.params_to_device(cp, torch.device("cpu")))
    assert np.array_equal(f3.numpy(), np.concatenate([np.asarray(cp["params"][g][n], np.float32).reshape(-1) for g, n in four]))
    assert distributed.flat_param_count(cl.stage) == f3.numel()


def test_checkpoint_round_trip_with_eight_leaves(tmp_path):
    cfg, P, _, _ = load_deeper_fixture()
    rng = np.random.default_rng(1)
    P = {"params": {g: {n: np.asarray(v, np.float32) for n, v in d.items()} for g, d in P["params"].items()}}
    mu = {"params": {g: {n: rng.normal(size=v.shape).astype(np.float32) for n, v in d.items()} for g, d in P["params"].items()}}
    nu = {"params": {g: {n: rng.uniform(size=v.shape).astype(np.float32) for n, v in d.items()} for g, d in P["params"].items()}}
    path = checkpoint.save_checkpoint(str(tmp_path), P, 7, opt_state=(mu, nu, 7))
    params, step = checkpoint.restore_checkpoint(path)
    m2, v2, count = checkpoint.restore_opt_state(path)
    assert step == 7 and count == 7
    for g, n in ORDER:
        assert np.array_equal(np.asarray(params["params"][g][n]), P["params"][g][n]), (g, n)
        assert np.array_equal(np.asarray(m2["params"][g][n]), mu["params"][g][n]), (g, n)
        assert np.array_equal(np.asarray(v2["params"][g][n]), nu["params"][g][n]), (g, n)


def test_k2m_in_the_abi():
    hdr = open(os.path.join(ROOT, "include", "irbfn_hip.h")).read()
    assert re.search(r"IRBFN_VJP_K2M\s*=\s*5", hdr) and _lib.VJP_K2M == 5
    assert "int irbfn_net_vjp_kernel_supported(irbfn_net* net, int kernel, int64_t B);" in hdr
    assert "irbfn_net_vjp_kernel_supported" in _lib.SIGNATURES
    lib = _lib.load()
    assert hasattr(lib, "irbfn_net_vjp_kernel_supported")
