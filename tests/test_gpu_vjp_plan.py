"""The parameter VJP's plan (plan_vjp, rbf_vjp.hip) at its boundaries: which kernel AUTO takes on either side of each threshold,
what a forced kernel answers where it cannot run, and that the workspace does not depend on the option.

Where the kernel has a name the name is asserted.  K2h and K2r record none (irbfn_net_last_launch keeps the previous name), so
there every leaf of the AUTO result must be bit-identical to the leaf from the kernel forced by option -- after checking, as a
precondition on the inputs, that the kernels on the two sides of the boundary do NOT give identical bits at that batch."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_ckpt_fixture
from irbfn_amd import _lib
from irbfn_amd.model import ClusterWCRBFNet, WCRBFNet
from oracle import irbfn_oracle as orc

pytestmark = pytest.mark.gpu

LEAVES = (("rbf_list", "centers"), ("rbf_list", "log_sigs"), ("linear", "kernel"), ("linear", "bias"))
CLUSTER_LEAVES = LEAVES + (("cluster", "kernel"), ("cluster", "bias"))
OPTS = {"AUTO": _lib.VJP_AUTO, "K2": _lib.VJP_K2, "K2H": _lib.VJP_K2H, "K2R": _lib.VJP_K2R, "K2G": _lib.VJP_K2G, "K2M": _lib.VJP_K2M}


def card(D, K, O, basis="gaussian"):
    return {"in_features": D, "out_features": O, "num_kernels": K, "basis_func": basis, "num_regions": 1,
            "lower_bounds": [[-1.0]] * D, "upper_bounds": [[2.0]] * D, "dimension_ranges": [[0] * D],
            "activation_idx": list(range(D)), "delta": [20.0] * D}


def one_region(K, D=7, O=10, basis="gaussian"):
    """Net and parameters drawn as in test_gpu_gram's every-instance test, so that K1g's expansion (and with it K2g) fits."""
    rng = np.random.default_rng(100 * D + O)
    P = {"params": {"rbf_list": {"centers": rng.uniform(-1.4, 2.4, size=(1, K, D)).astype(np.float32),
                                 "log_sigs": rng.uniform(-0.2, 0.9, size=(1, K)).astype(np.float32)},
                    "linear": {"kernel": rng.normal(size=(K, O)).astype(np.float32), "bias": rng.normal(size=(O,)).astype(np.float32)}}}
    return WCRBFNet.from_config(card(D, K, O, basis)), P


def batch(torch, B, D=7, O=10, seed=5):
    rng = np.random.default_rng(seed)
    return (torch.from_numpy(rng.uniform(-1.05, 2.05, size=(B, D)).astype(np.float32)).cuda(),
            torch.from_numpy(rng.normal(size=(B, O)).astype(np.float32)).cuda())


def cluster(R, K, D=8, O=10):
    rng = np.random.default_rng(7 * R + K)
    P = {"params": {"rbf_list": {"centers": rng.uniform(-1.4, 2.4, size=(R, K, D)).astype(np.float32),
                                 "log_sigs": rng.uniform(-0.2, 0.9, size=(R, K)).astype(np.float32)},
                    "linear": {"kernel": rng.normal(size=(K, O)).astype(np.float32), "bias": rng.normal(size=(O,)).astype(np.float32)},
                    "cluster": {"kernel": rng.normal(size=(D, R)).astype(np.float32), "bias": rng.normal(size=(R,)).astype(np.float32)}}}
    return ClusterWCRBFNet(in_features=D, out_features=O, num_kernels=K, basis_func="gaussian", num_regions=R), P


def run(net, P, x, g, option, leaves=LEAVES):
    """(leaves, kernel name) of one VJP under `option`.  A one-row forward goes first: a VJP kernel without a name of its own
    leaves that forward's name standing, whatever VJP ran before."""
    net.apply(P, x[:1].contiguous())
    net.set_options(vjp_kernel=OPTS[option])
    try:
        got = net.vjp(P, x, g)["params"]
    finally:
        net.set_options(vjp_kernel=_lib.VJP_AUTO)
    return [got[a][b] for a, b in leaves], getattr(net, "stage", net).last_launch()["kernel"]


def same(torch, a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b))


def supported(torch, net, option, B):
    return _lib.load().irbfn_net_vjp_kernel_supported(getattr(net, "stage", net)._handle(torch), OPTS[option], B)


def distinct(torch, net, P, x, g, one, other, leaves=LEAVES):
    """Precondition on the inputs: the two forced kernels differ in some bit at this batch; returns their results."""
    a, b = run(net, P, x, g, one, leaves), run(net, P, x, g, other, leaves)
    if same(torch, a[0], b[0]):
        pytest.fail(f"test inputs, not the code under test: {one} and {other} give bit-identical leaves at B = {x.shape[0]}, "
                    f"the case distinguishes nothing")
    return a, b


def need_k2g(torch, net, P, B):
    net.bind(P)                                  # the verdict on the expansion belongs to the parameters bound
    if supported(torch, net, "K2G", B) != 1:
        pytest.fail(f"test inputs, not the code under test: the parameters fall outside K2g's expansion at B = {B}")


def test_auto_takes_k2h_from_2048_queries(gpu):
    torch = gpu
    net, P = one_region(200)
    x, g = batch(torch, 2048)
    (k2, name2), (k2h, nameh) = distinct(torch, net, P, x, g, "K2", "K2H")
    assert name2.startswith("rbf_vjp_kernel<") and nameh.startswith("rbf_fwd_"), (name2, nameh)     # K2h records no name
    auto, name = run(net, P, x, g, "AUTO")
    assert same(torch, auto, k2h) and name == nameh, name
    x, g = x[:2047].contiguous(), g[:2047].contiguous()
    auto, name = run(net, P, x, g, "AUTO")
    assert name.startswith("rbf_vjp_kernel<") and "GATED=0" in name, name
    assert same(torch, auto, run(net, P, x, g, "K2")[0])


@pytest.mark.parametrize("K,below,at", [(3000, 8333, 8334),     # 8333 * 3000 < 2.5e7 <= 8334 * 3000 (query, centre) pairs
                                        (4096, 8191, 8192)])    # the batch floor, well above 2.5e7 pairs
def test_auto_puts_k2g_in_front_of_k2h_from_8192_queries_and_25e6_pairs(gpu, K, below, at):
    torch = gpu
    net, P = one_region(K)
    xa, ga = batch(torch, at)
    need_k2g(torch, net, P, below)
    need_k2g(torch, net, P, at)
    (k2g, nameg), _ = distinct(torch, net, P, xa, ga, "K2G", "K2H")
    assert nameg.startswith("rbf_vjp_f16gram<"), nameg
    auto, name = run(net, P, xa, ga, "AUTO")
    assert name == nameg and same(torch, auto, k2g), (name, nameg)
    xb, gb = xa[:below].contiguous(), ga[:below].contiguous()
    _, (k2h, nameh) = distinct(torch, net, P, xb, gb, "K2G", "K2H")
    auto, name = run(net, P, xb, gb, "AUTO")
    assert name.startswith("rbf_fwd_") and name == nameh and same(torch, auto, k2h), (name, nameh)


def test_auto_takes_k2r_on_the_128_region_net(gpu):
    torch = gpu
    cfg, P, *_ = load_ckpt_fixture("dnmpc_128regions")
    P = orc.cast_params(P, np.float32)
    B, rng = 20000, np.random.default_rng(8)
    ns, D = len(cfg["activation_idx"]), cfg["in_features"]
    lo = np.array([min(cfg["lower_bounds"][d]) for d in range(ns)])
    hi = np.array([max(cfg["upper_bounds"][d]) for d in range(ns)])
    x = torch.from_numpy(np.hstack([rng.uniform(lo, hi, size=(B, ns)), rng.normal(size=(B, D - ns)) * 0.1]).astype(np.float32)).cuda()
    g = torch.from_numpy(rng.normal(size=(B, cfg["out_features"])).astype(np.float32)).cuda()
    net = WCRBFNet.from_config(cfg)
    (k2r, namer), (_, name2) = distinct(torch, net, P, x, g, "K2R", "K2")
    assert namer.startswith("rbf_fwd_") and "GATED=1" in name2, (namer, name2)                       # K2r records no name
    auto, name = run(net, P, x, g, "AUTO")
    assert name == namer and same(torch, auto, k2r), name
    with pytest.raises(ValueError, match="UNSUPPORTED"):
        run(net, P, x, g, "K2G")


@pytest.mark.parametrize("R,K,B", [(8, 16, 300), (8, 16, 2100), (1, 16, 300), (1, 16, 2100),
                                   (1, 1000, 20000)])    # one region, where K2h's shorter slab count would apply: K2 keeps its own
def test_cluster_nets_run_the_gated_k2(gpu, R, K, B):
    """Caller-provided region weights: the gated K2 whatever the option prefers, with K2's own slab count.  At R = 1, K = 1000,
    B = 20000 K2h's rule gives 48 slabs where 79 are allocated; a K2 launched with 48 slabs and the queries per wave of 79 left
    7712 of the 20000 queries out of the centre, width and kernel gradients."""
    torch = gpu
    net, P = cluster(R, K)
    x, g = batch(torch, B, D=8)
    k2, name2 = run(net, P, x, g, "K2", CLUSTER_LEAVES)
    auto, name = run(net, P, x, g, "AUTO", CLUSTER_LEAVES)
    assert name == name2 and name.startswith("rbf_vjp_kernel<") and "GATED=1" in name, (name, name2)
    assert same(torch, auto, k2)
    for option in ("K2G", "K2M"):
        with pytest.raises(ValueError, match="UNSUPPORTED"):
            run(net, P, x, g, option, CLUSTER_LEAVES)


def test_forced_kernels_refuse_and_k2h_is_a_preference(gpu):
    torch = gpu
    lib = _lib.load()
    net, P = one_region(200)
    h = net._handle(torch)
    x, g = batch(torch, 300)
    sizes = []
    for option in OPTS:
        net.set_options(vjp_kernel=OPTS[option])
        sizes.append([int(lib.irbfn_net_vjp_workspace_bytes(h, B)) for B in (300, 2100, 20000)])
    net.set_options(vjp_kernel=_lib.VJP_AUTO)
    assert all(s == sizes[0] for s in sizes) and min(sizes[0]) > 0, sizes          # one size per batch, whatever the option
    for option in ("K2G", "K2R", "K2M"):                            # below 2048 queries / one region / O <= 16
        assert supported(torch, net, option, 300) == 0, option
        now = C.c_int(-1)
        assert lib.irbfn_net_get_option(h, _lib.OPTIONS["vjp_kernel"], C.byref(now)) == 0 and now.value == _lib.VJP_AUTO
        with pytest.raises(ValueError, match="UNSUPPORTED"):
            run(net, P, x, g, option)
    assert supported(torch, net, "K2H", 300) == 1
    k2h, name = run(net, P, x, g, "K2H")                            # a preference: K2 runs, status OK
    assert name.startswith("rbf_vjp_kernel<"), name
    assert same(torch, k2h, run(net, P, x, g, "K2")[0])
    wide, Pw = one_region(200, O=64)                                # K2m's shapes: forced only
    xw, gw = batch(torch, 300, O=64)
    assert supported(torch, wide, "K2M", 300) == 1 and supported(torch, wide, "K2G", 300) == 0
    assert run(wide, Pw, xw, gw, "K2M")[1].startswith("rbf_vjp_mfma<")
    assert run(wide, Pw, xw, gw, "AUTO")[1].startswith("rbf_vjp_kernel<")
