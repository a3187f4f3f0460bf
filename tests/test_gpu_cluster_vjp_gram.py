"""The region-weighted parameter VJP on the matrix cores: ``rbf_vjp_f16gram_gamma``, selected by ``vjp_kernel = VJP_K2G_GAMMA``
for ``irbfn_net_vjp_gamma``.

Every parity case runs against the float64 statement of tests/_cluster_vjp_gram_util.py (arbitrary gamma) with two bounds of
the project: every leaf within 5e-5 of the leaf's max (tests/test_gpu_train.py::test_cluster_wcrbfnet_vjp) and d gamma per
element within 1e-5 |ref| + 3e-6 sum_k |hbar phi| (tests/test_gpu_fullsize.py).  Each has a K2 leg on the same inputs that must
meet the same bounds: a K2 leg that fails faults the inputs, not the new kernel.  Inputs follow
tests/test_gpu_cluster_gram.py::_case: centres and queries in [-2, 2]^d, log sigma in [0, 1] -- by gram_header (pack_all.hip)
ex = 2, ec = 3, so the pack's verdict is "ok" and every query is inside the expansion's box; a call that answers UNSUPPORTED
there fails as "test inputs, not the code under test".
"""
import functools

import numpy as np
import pytest
import torch

from _cluster_gram_util import softmax_gamma
from _cluster_util import CLEAVES, cluster_case, oracle_train_loss, oracle_vjp
from _cluster_vjp_gram_util import STAGE, gamma_vjp64
from irbfn_amd import _lib, configs, train
from irbfn_amd.model import ClusterWCRBFNet, _ptr, _stream_ptr
from oracle import irbfn_oracle as orc

pytestmark = pytest.mark.gpu
FAST = ("gaussian", "inverse_quadratic", "inverse_multiquadric")
KERNELS = {"k2": _lib.VJP_K2, "k2g": _lib.VJP_K2G_GAMMA}
NAME = {"k2": "rbf_vjp_kernel<", "k2g": "rbf_vjp_f16gram_gamma<"}
OK, UNSUPPORTED, NO_PARAMS = 0, -2, -4
DP = np.array(configs.DYN_PARAMS)
LEAF_TOL = 5e-5


def _case(seed, R, K, basis, B, D=8, O=10, wide_w=False, dense_g=False):
    """``_case`` of tests/test_gpu_cluster_gram.py, with a cotangent g[B, O]; wide_w: Dense rows of 1e4 next to rows of 1e-2.

    The cotangent and the place of the wide factor are chosen for d gamma's bound.  Its scale sum_k |hbar phi| sees hbar[b, k] =
    sum_o g[b, o] W[k, o] only after the sum: where the terms cancel (a normal g over 16 outputs: to 1 / 3000 for some (b, k) of
    2049 x 10), float32 evaluates hbar to eps sum_o |g W| and NO float32 d gamma meets the bound -- the float32 kernel of the K2
    leg misses it by 9.7 x at gaussian, d = 8, K = 10, R = 3, O = 16, B = 2049 with a normal g, a plain NumPy float32 evaluation by
    8.5 x, and both are at 0.3 x a scale that takes |g W| per term.  A K2 leg that fails faults the inputs, so: each row of g has
    ONE output of normal size (drawn per row, so that every output leads in 1 / O of the rows) and the others at 1e-3 of it,
    and the wide factor is drawn per ROW of W (centre), not per element -- then hbar is one product plus a small remainder and
    cannot cancel.  A padding row that picked up its neighbour's weights shows just the same.  dense_g: a normal g (the
    model-level cases, whose bounds are per leaf)."""
    rng, cfg, params, x = cluster_case(seed, R=R, K=K, O=O, B=B, D=D, basis=basis)
    p = params["params"]
    p["rbf_list"]["log_sigs"] = rng.uniform(0.0, 1.0, size=(R, K)).astype(np.float32)
    w = rng.normal(size=(K, O))
    if wide_w:
        w = w * np.where(rng.uniform(size=(K, 1)) < 0.5, 1e4, 1e-2)
    p["linear"]["kernel"] = w.astype(np.float32)
    p["linear"]["bias"] = rng.normal(size=(O,)).astype(np.float32)
    p["cluster"]["kernel"] = rng.normal(size=(D, R)).astype(np.float32) * 2.0
    g = rng.normal(size=(B, O))
    if not dense_g:
        lead = np.full((B, O), 1e-3)
        lead[np.arange(B), rng.integers(0, O, size=B)] = 1.0
        g = g * lead
    return rng, cfg, params, x, g.astype(np.float32)


def _rbf(params):
    p = params["params"]
    return {"rbf_list": p["rbf_list"], "linear": p["linear"]}


def _stage(cfg, params, kern):
    stage = ClusterWCRBFNet(**cfg).stage.set_options(vjp_kernel=KERNELS[kern])
    stage.bind(_rbf(params))
    return stage


def _vjp(stage, xt, gt, gd, expect=OK, entry="gamma", dgamma=True):
    """irbfn_net_vjp_gamma (or irbfn_net_vjp) on device tensors -> {four leaves, dgamma} (None where another status is expected);
    dgamma=False passes a null d gamma (its float32 kernel stops at O = 16)."""
    lib = _lib.load()
    R, K, D, O = stage.num_regions, stage.num_kernels, stage.in_features, stage.out_features
    B = xt.shape[0]
    dev = xt.device
    out = {"centers": torch.full((R, K, D), 7.0, device=dev), "log_sigs": torch.full((R, K), 7.0, device=dev),
           "kernel": torch.full((K, O), 7.0, device=dev), "bias": torch.full((O,), 7.0, device=dev),
           "dgamma": torch.full((B, R), 7.0, device=dev)}
    h = stage._handle(torch)
    nbytes = int(lib.irbfn_net_vjp_workspace_bytes(h, B))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    if entry == "gamma":
        st = lib.irbfn_net_vjp_gamma(h, _ptr(xt), _ptr(gt), _ptr(gd), _ptr(out["centers"]), _ptr(out["log_sigs"]), _ptr(out["kernel"]),
                                     _ptr(out["bias"]), _ptr(out["dgamma"]) if dgamma else None, B, _ptr(ws), nbytes, _stream_ptr(torch))
    else:
        st = lib.irbfn_net_vjp(h, _ptr(xt), _ptr(gd), _ptr(out["centers"]), _ptr(out["log_sigs"]), _ptr(out["kernel"]), _ptr(out["bias"]),
                               B, _ptr(ws), nbytes, _stream_ptr(torch))
    torch.cuda.synchronize()
    if expect == OK and st == UNSUPPORTED:
        pytest.fail("UNSUPPORTED for inputs inside the expansion's budget: test inputs, not the code under test")
    assert st == expect, (st, expect)
    return out if st == OK else None


def _check(got, leaves, dgamma, scale, what):
    """The two bounds; prints the measured ratios (err / bound) before it asserts."""
    ratios = {}
    for n in STAGE:
        a = got[n].cpu().numpy().astype(np.float64)
        assert np.isfinite(a).all(), (what, n)
        ratios[n] = np.abs(a - leaves[n]).max() / (LEAF_TOL * np.abs(leaves[n]).max() + 1e-300)
    d = got["dgamma"].cpu().numpy().astype(np.float64)
    assert np.isfinite(d).all(), what
    bound = 1e-5 * np.abs(dgamma) + 3e-6 * scale
    ratios["dgamma"] = float((np.abs(d - dgamma) / np.maximum(bound, 1e-300)).max())
    print(f"cluster_vjp_gram {what}: err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1.0, (what, k, v)


def _equal(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


def _prefix_refs(cfg, params, x, gamma, g, Bs):
    """The float64 statement for every prefix x[:B], B in Bs (ascending), from one pass over the longest: the leaves are sums
    over rows, so the segments between the batch sizes are differentiated once and accumulated."""
    refs, acc, prev = {}, None, 0
    dgs, scs = [], []
    for B in Bs:
        leaves, dg, sc = gamma_vjp64(cfg, params, x[prev:B], gamma[prev:B], g[prev:B])
        acc = leaves if acc is None else {n: acc[n] + leaves[n] for n in STAGE}
        dgs.append(dg); scs.append(sc)
        refs[B] = (dict(acc), np.concatenate(dgs), np.concatenate(scs))
        prev = B
    return refs


# ---- 1. chunk map and padding ---------------------------------------------------------------------------------------------
BATCHES = (1, 31, 32, 33, 257, 2049)
# (K, R, O): K -- a part chunk, a whole chunk, one centre into the second chunk, two part-filled chunks; R -- regions straddling the
# four-chunk block, a last block with idle waves; O -- hbar as one MFMA (<= 10) and as two
SHAPES = ((10, 1, 10), (32, 2, 2), (33, 3, 16), (50, 5, 10), (50, 11, 16), (10, 11, 2), (33, 5, 10), (32, 11, 16), (10, 3, 16), (50, 1, 2),
          (33, 2, 10), (32, 5, 2))


@functools.lru_cache(maxsize=None)
def _padding_case(basis, D, K, R, O):
    _, cfg, params, x, g = _case(1000 * K + 10 * R + D + O, R, K, basis, BATCHES[-1], D=D, O=O, wide_w=True)
    gamma = softmax_gamma(params, x).astype(np.float32)
    return cfg, params, x, gamma, g, _prefix_refs(cfg, params, x, gamma, g, BATCHES)


@pytest.mark.parametrize("basis,D", [(b, D) for b in FAST for D in (7, 8)] + [("gaussian", 3), ("gaussian", 4)])
def test_chunk_map_and_padding(gpu, basis, D):
    for K, R, O in SHAPES:
        cfg, params, x, gamma, g, refs = _padding_case(basis, D, K, R, O)
        xt, gt, gd = (torch.from_numpy(a).cuda() for a in (x, gamma, g))
        for kern in KERNELS:
            stage = _stage(cfg, params, kern)
            for B in BATCHES:
                got = _vjp(stage, xt[:B].contiguous(), gt[:B].contiguous(), gd[:B].contiguous())
                assert stage.last_launch()["kernel"].startswith(NAME[kern]), stage.last_launch()
                _check(got, *refs[B], (basis, D, K, R, O, B, kern))


# ---- 2. gamma values ------------------------------------------------------------------------------------------------------
def test_gamma_values(gpu):
    """Hand-made region weights: one-hot rows, negative entries with |gamma| <= 1, whole regions at 0 (their centre and width
    gradients are exactly 0); gamma = 1 at R = 1."""
    R, K, B = 11, 33, 300
    rng, cfg, params, x, g = _case(33, R, K, "gaussian", B)
    xt, gd = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    soft = softmax_gamma(params, x).astype(np.float32)
    dead = [0, 4, 5, 10]
    zeros = soft.copy(); zeros[:, dead] = 0.0
    onehot = np.zeros((B, R), np.float32); onehot[np.arange(B), rng.integers(0, R, size=B)] = 1.0
    signed = rng.uniform(-1, 1, size=(B, R)).astype(np.float32)
    signed_zeros = signed.copy(); signed_zeros[:, dead] = 0.0
    for what, gam in (("zero regions", zeros), ("one-hot", onehot), ("uniform [-1, 1]", signed), ("signed, zero regions", signed_zeros)):
        ref = gamma_vjp64(cfg, params, x, gam, g)
        for kern in KERNELS:
            got = _vjp(_stage(cfg, params, kern), xt, torch.from_numpy(gam).cuda(), gd)
            _check(got, *ref, (what, kern))
            if "zero" in what:
                assert not got["centers"][dead].any() and not got["log_sigs"][dead].any(), (what, kern)
    _, cfg1, params1, x1, g1 = _case(34, 1, 50, "inverse_quadratic", B)
    ones = np.ones((B, 1), np.float32)
    ref = gamma_vjp64(cfg1, params1, x1, ones, g1)
    for kern in KERNELS:
        stage = _stage(cfg1, params1, kern)
        got = _vjp(stage, torch.from_numpy(x1).cuda(), torch.from_numpy(ones).cuda(), torch.from_numpy(g1).cuda())
        assert stage.last_launch()["kernel"].startswith(NAME[kern])
        _check(got, *ref, ("gamma = 1, R = 1", kern))


# ---- 3. slices and determinism --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [4097, 20000])
def test_slices_and_determinism(gpu, B):
    """Several query slices: parity, bitwise repeat, vjp(4 g) = 4 vjp(g) exactly, batch additivity at a split that is no multiple
    of 32 within 2e-5 of the leaf's max (tests/test_gpu_cluster_scale.py::test_cluster_vjp_batch_additivity)."""
    R, K = 3, 50
    _, cfg, params, x, g = _case(B, R, K, "gaussian", B)
    gamma = softmax_gamma(params, x).astype(np.float32)
    ref = gamma_vjp64(cfg, params, x, gamma, g)
    xt, gt, gd = (torch.from_numpy(a).cuda() for a in (x, gamma, g))
    _check(_vjp(_stage(cfg, params, "k2"), xt, gt, gd), *ref, ("slices", B, "k2"))
    stage = _stage(cfg, params, "k2g")
    a = _vjp(stage, xt, gt, gd)
    ll = stage.last_launch()
    assert ll["kernel"].startswith(NAME["k2g"]) and int(ll["kernel"].split("QSB=")[1].rstrip(">")) > 1, ll
    _check(a, *ref, ("slices", B, "k2g"))
    assert _equal(a, _vjp(stage, xt, gt, gd))
    a4 = _vjp(stage, xt, gt, 4.0 * gd)
    assert all(torch.equal(a4[k], 4.0 * a[k]) for k in a)
    split = B // 2 + 5
    assert split % 32 != 0
    a1 = _vjp(stage, xt[:split].contiguous(), gt[:split].contiguous(), gd[:split].contiguous())
    a2 = _vjp(stage, xt[split:].contiguous(), gt[split:].contiguous(), gd[split:].contiguous())
    for n in STAGE:
        e = float((a[n] - (a1[n] + a2[n])).abs().max() / a[n].abs().max())
        assert e <= 2e-5, (n, e)
    assert torch.equal(a["dgamma"], torch.cat([a1["dgamma"], a2["dgamma"]]))


# ---- 4. hand-over ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,K", [(5, 33), (1, 50)])
def test_query_outside_the_box_hands_over_to_k2(gpu, R, K):
    """One query at 50 in one coordinate: status OK, every leaf and d gamma bit-equal to a forced K2 call."""
    B = 700
    _, cfg, params, x, g = _case(44 + R, R, K, "gaussian", B)
    x[123, 4] = 50.0
    gamma = softmax_gamma(params, x).astype(np.float32)
    xt, gt, gd = (torch.from_numpy(a).cuda() for a in (x, gamma, g))
    k2 = _vjp(_stage(cfg, params, "k2"), xt, gt, gd)
    stage = _stage(cfg, params, "k2g")
    got = _vjp(stage, xt, gt, gd)
    assert stage.last_launch()["kernel"].startswith(NAME["k2g"])
    assert _equal(got, k2)
    # the next call, all inside the box, is the matrix-core kernel's again
    x[123, 4] = 1.0
    ref = gamma_vjp64(cfg, params, x, gamma, g)
    _check(_vjp(stage, torch.from_numpy(x).cuda(), gt, gd), *ref, ("after the hand-over", R, K))


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["generic basis", "O = 32", "outside the budget"])
def test_refusals(gpu, what):
    """IRBFN_ERR_UNSUPPORTED, nothing launched in its place (the outputs keep their fill); back on VJP_AUTO the gated K2 returns
    the bits it returned before the option was ever set."""
    basis = "matern52" if what == "generic basis" else "gaussian"
    O = 32 if what == "O = 32" else 10
    R, K, B = 3, 40, 200
    rng, cfg, params, x, g = _case(6, R, K, basis, B, O=O)
    if what == "outside the budget":
        params["params"]["rbf_list"]["centers"] = (params["params"]["rbf_list"]["centers"] * 500.0).astype(np.float32)   # spread over 1e3
        params["params"]["rbf_list"]["log_sigs"][:] = -3.0
    gamma = softmax_gamma(params, x).astype(np.float32)
    xt, gt, gd = (torch.from_numpy(a).cuda() for a in (x, gamma, g))
    stage = ClusterWCRBFNet(**cfg).stage
    stage.bind(_rbf(params))
    base = _vjp(stage, xt, gt, gd, dgamma=O <= 16)
    assert stage.last_launch()["kernel"].startswith(NAME["k2"])
    stage.set_options(vjp_kernel=_lib.VJP_K2G_GAMMA)
    stage.bind(_rbf(params))
    lib = _lib.load()
    R_, K_, D_ = stage.num_regions, stage.num_kernels, stage.in_features
    h = stage._handle(torch)
    nbytes = int(lib.irbfn_net_vjp_workspace_bytes(h, B))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    outs = [torch.full(s, 7.0, device="cuda") for s in ((R_, K_, D_), (R_, K_), (K_, O), (O,), (B, R_))]
    st = lib.irbfn_net_vjp_gamma(h, _ptr(xt), _ptr(gt), _ptr(gd), *[_ptr(t) for t in outs], B, _ptr(ws), nbytes, _stream_ptr(torch))
    torch.cuda.synchronize()
    assert st == UNSUPPORTED, st
    assert all(bool((t == 7.0).all()) for t in outs)
    stage.set_options(vjp_kernel=_lib.VJP_AUTO)
    stage.bind(_rbf(params))
    again = _vjp(stage, xt, gt, gd, dgamma=O <= 16)
    assert stage.last_launch()["kernel"].startswith(NAME["k2"]) and "GATED=1" in stage.last_launch()["kernel"]
    assert _equal(again, base)


def test_only_vjp_gamma_takes_the_value(gpu):
    """irbfn_net_vjp and irbfn_net_vjp_kernel_supported under the value; the workspace size does not depend on the option's value;
    7 is a bad argument."""
    lib = _lib.load()
    R, K, B = 3, 40, 200
    _, cfg, params, x, g = _case(9, R, K, "gaussian", B)
    gamma = softmax_gamma(params, x).astype(np.float32)
    xt, gt, gd = (torch.from_numpy(a).cuda() for a in (x, gamma, g))
    stage = _stage(cfg, params, "k2g")
    h = stage._handle(torch)
    assert _vjp(stage, xt, gt, gd, expect=UNSUPPORTED, entry="plain") is None
    # irbfn_net_vjp_kernel_supported speaks of irbfn_net_vjp: the value stays a bad argument there, as
    # tests/test_gpu_deeper_train.py::test_k2m_refusals_and_auto_unchanged pins for 6
    assert lib.irbfn_net_vjp_kernel_supported(h, _lib.VJP_K2G_GAMMA, B) < 0
    assert lib.irbfn_net_set_option(h, _lib.OPTIONS["vjp_kernel"], _lib.VJP_K2G_GAMMA + 1) == -1
    sizes = [int(lib.irbfn_net_vjp_workspace_bytes(h, n)) for n in (1, B, 20000)]
    stage.set_options(vjp_kernel=_lib.VJP_AUTO)
    assert sizes == [int(lib.irbfn_net_vjp_workspace_bytes(h, n)) for n in (1, B, 20000)] and min(sizes) > 0
    assert _vjp(stage, xt, gt, gd, entry="plain") is not None                     # the tanh gate of a net without gate tables


def test_option_needs_a_bind(gpu):
    """The option selected after a bind, behind Python's back: IRBFN_ERR_NO_PARAMS until the next irbfn_net_set_params."""
    lib = _lib.load()
    R, K, B = 5, 40, 300
    _, cfg, params, x, g = _case(7, R, K, "gaussian", B)
    gamma = softmax_gamma(params, x).astype(np.float32)
    xt, gt, gd = (torch.from_numpy(a).cuda() for a in (x, gamma, g))
    stage = ClusterWCRBFNet(**cfg).stage
    stage.bind(_rbf(params))
    h = stage._handle(torch)
    assert lib.irbfn_net_set_option(h, _lib.OPTIONS["vjp_kernel"], _lib.VJP_K2G_GAMMA) == OK
    assert _vjp(stage, xt, gt, gd, expect=NO_PARAMS) is None
    stage.set_options(vjp_kernel=_lib.VJP_K2G_GAMMA)                 # forgets the bind: the next one packs the images
    stage.bind(_rbf(params))
    _check(_vjp(stage, xt, gt, gd), *gamma_vjp64(cfg, params, x, gamma, g), "after the bind")
    assert stage.last_launch()["kernel"].startswith(NAME["k2g"])


# ---- 6. model level -------------------------------------------------------------------------------------------------------
def _assert_six(a, ref, what):
    for grp, name in CLEAVES:
        got = a[grp][name].cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all(), (what, grp, name)
        e = np.abs(got - ref[(grp, name)]).max() / (np.abs(ref[(grp, name)]).max() + 1e-300)
        print(f"cluster_vjp_gram {what} {grp}.{name}: err / max = {e:.2e}")
        assert e <= LEAF_TOL, (what, grp, name, e)


@pytest.mark.parametrize("B", [129, 2049])
@pytest.mark.parametrize("K,basis", [(50, "gaussian"), (10, "inverse_quadratic")])
def test_model_reference_shapes(gpu, K, basis, B):
    """ClusterWCRBFNet.vjp at R = 500: six leaves against ``oracle_vjp``, with and without a cotangent of the logits."""
    R = 500
    rng, cfg, params, x, g = _case(K + B, R, K, basis, B, dense_g=True)
    gl = rng.normal(size=(B, R)).astype(np.float32)
    ref, ref_gl = oracle_vjp(cfg, params, x, g, gl)
    xt, gd, gld = (torch.from_numpy(a).cuda() for a in (x, g, gl))
    for kern in KERNELS:
        net = ClusterWCRBFNet(**cfg).set_options(vjp_kernel=KERNELS[kern])
        _assert_six(net.vjp(params, xt, gd)["params"], ref, (K, basis, B, kern, "no glogits"))
        assert net.stage.last_launch()["kernel"].startswith(NAME[kern]), net.stage.last_launch()
        _assert_six(net.vjp(params, xt, gd, glogits=gld)["params"], ref_gl, (K, basis, B, kern, "glogits"))
    out = net.vjp(params, xt, gd, glogits=gld)                        # out=: the same bits into the caller's leaves
    out2 = {"params": {grp: {n: torch.zeros_like(t) for n, t in d.items()} for grp, d in out["params"].items()}}
    net.vjp(params, xt, gd, glogits=gld, out=out2)
    assert all(torch.equal(out["params"][grp][n], out2["params"][grp][n]) for grp, n in CLEAVES)


def test_train_step_reference_shape(gpu):
    """One train_step_fullint_withcluster step at R = 500, K = 10, B = 2048 under the option, with the bounds of
    tests/test_gpu_cluster_scale.py::test_cluster_train_step_reference_shapes.  Its Frenet queries have a speed in [1, 6]; the
    centres' third coordinate is drawn there too, so that the queries stay inside the expansion's box and the step runs the
    matrix-core kernel (not the gated K2 behind it)."""
    R, K, B, T = 500, 10, 2048, 5
    rng, cfg, params, x = cluster_case(77, R=R, K=K, O=10, B=B, D=8)
    params["params"]["rbf_list"]["centers"][:, :, 2] = rng.uniform(1.0, 6.0, size=(R, K)).astype(np.float32)
    x[:, 7] = rng.normal(size=B).astype(np.float32) * 0.05
    x[:, 0] = rng.normal(size=B).astype(np.float32) * 0.2
    x[:, 2] = rng.uniform(1.0, 6.0, size=B).astype(np.float32)
    y = np.hstack([rng.normal(size=(B, T)) * 2, rng.normal(size=(B, T)) * 0.5]).astype(np.float32)
    ids = np.eye(R, dtype=np.float32)[rng.integers(0, R, size=B)]
    net = ClusterWCRBFNet(**cfg).set_options(vjp_kernel=_lib.VJP_K2G_GAMMA)
    state = train.ClusterTrainState.create(net, params, lr=1e-3, max_grad_norm=1.0)
    p_ref = np.concatenate([np.asarray(params["params"][g_][n_], np.float64).reshape(-1) for g_, n_ in CLEAVES])
    n = p_ref.size
    loss, g_ref = oracle_train_loss(cfg, params, x, y, ids, DP)
    p_ref, _, _ = orc.adam_update(p_ref, orc.clip_by_global_norm(g_ref, 1.0), np.zeros(n), np.zeros(n), 1, lr=1e-3)
    state, l_gpu = train.train_step_fullint_withcluster(state, torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(),
                                                        torch.from_numpy(ids).cuda(), DP)
    assert net.stage.last_launch()["kernel"].startswith(NAME["k2g"]), net.stage.last_launch()
    assert abs(float(l_gpu) - loss) <= 3e-5 * abs(loss), (float(l_gpu), loss)
    g_gpu = state.g.cpu().numpy()
    assert np.abs(g_gpu - g_ref).max() <= 5e-4 * np.abs(g_ref).max(), np.abs(g_gpu - g_ref).max() / np.abs(g_ref).max()
    assert np.abs(state.flat.cpu().numpy() - p_ref).max() <= 5e-5 + 1e-6 * np.abs(p_ref).max()


def test_training_batch_against_k2(gpu):
    """R = 500, K = 50 at the reference's batch 80 000: six leaves within 5e-5 of the leaf's max of the K2 leg; bitwise repeat."""
    R, K, B = 500, 50, 80000
    rng, cfg, params, x, g = _case(80, R, K, "gaussian", B, dense_g=True)
    gl = rng.normal(size=(B, R)).astype(np.float32)
    xt, gd, gld = (torch.from_numpy(a).cuda() for a in (x, g, gl))
    k2 = ClusterWCRBFNet(**cfg).set_options(vjp_kernel=_lib.VJP_K2).vjp(params, xt, gd, glogits=gld)["params"]
    net = ClusterWCRBFNet(**cfg).set_options(vjp_kernel=_lib.VJP_K2G_GAMMA)
    a = net.vjp(params, xt, gd, glogits=gld)["params"]
    assert net.stage.last_launch()["kernel"].startswith(NAME["k2g"]), net.stage.last_launch()
    b = net.vjp(params, xt, gd, glogits=gld)["params"]
    for grp, name in CLEAVES:
        assert torch.equal(a[grp][name], b[grp][name]), (grp, name)
        e = float((a[grp][name] - k2[grp][name]).abs().max() / k2[grp][name].abs().max())
        print(f"cluster_vjp_gram training batch {grp}.{name}: |k2g - k2| / max = {e:.2e}")
        assert e <= LEAF_TOL, (grp, name, e)
