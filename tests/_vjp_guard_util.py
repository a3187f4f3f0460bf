"""The guarded-buffer runner of tests/test_gpu_k2.py, tests/test_gpu_k2h.py and tests/test_gpu_k2m.py: one parameter VJP whose
leaves are views of one NaN-filled buffer with GUARD words around each, run twice, or refused with the buffer untouched.  The case
is a tests/_k2_util.py::Case (or a subclass)."""
import numpy as np
import pytest

from irbfn_amd import _lib
from irbfn_amd.model import ClusterWCRBFNet, WCRBFNet

GUARD = 64


def make_net(case):
    if case.cluster:
        return ClusterWCRBFNet(in_features=case.D, out_features=case.O, num_kernels=case.K, basis_func=case.basis, num_regions=case.R)
    return WCRBFNet.from_config(case.cfg)


def guarded_out(torch, case):
    """The leaves as views of one flat NaN buffer with GUARD words around each -> (buffer, shapes, spans, the `out` tree)."""
    R, K, D, O = case.R, case.K, case.D, case.O
    shapes = {"centers": (R, K, D), "log_sigs": (R, K), "kernel": (K, O), "bias": (O,)}
    if case.cluster:
        shapes.update(ckernel=(D, R), cbias=(R,))
    total = GUARD + sum(int(np.prod(s)) + GUARD for s in shapes.values())
    buf = torch.full((total,), float("nan"), dtype=torch.float32, device="cuda")
    views, spans, off = {}, {}, GUARD
    for n, s in shapes.items():
        size = int(np.prod(s))
        views[n], spans[n] = buf[off:off + size].view(s), (off, off + size)
        off += size + GUARD
    out = {"params": {"rbf_list": {"centers": views["centers"], "log_sigs": views["log_sigs"]},
                      "linear": {"kernel": views["kernel"], "bias": views["bias"]}}}
    if case.cluster:
        out["params"]["cluster"] = {"kernel": views["ckernel"], "bias": views["cbias"]}
    return buf, shapes, spans, out


def vjp_guarded(torch, net, case, x=None, g=None, option=_lib.VJP_K2):
    """One VJP into views of a flat NaN buffer -> ({leaf: float32 array}, what the launch reports, the buffer's bits)."""
    buf, shapes, spans, out = guarded_out(torch, case)
    total = buf.numel()
    xd = torch.from_numpy(case.x if x is None else x).cuda()
    gd = torch.from_numpy(case.g if g is None else g).cuda()
    net.set_options(vjp_kernel=option)
    try:
        net.vjp(case.params, xd, gd, out=out)
    finally:
        net.set_options(vjp_kernel=_lib.VJP_AUTO)
    torch.cuda.synchronize()
    launch = getattr(net, "stage", net).last_launch()
    host = buf.cpu().numpy()
    guard = np.ones(total, bool)
    for a, b in spans.values():
        guard[a:b] = False
    assert np.isnan(host[guard]).all(), f"{case.tag}: {launch['kernel']} wrote outside its leaves"
    return {n: host[a:b].reshape(shapes[n]) for n, (a, b) in spans.items()}, launch, host.view(np.uint32)


def run_twice(torch, net, case, expect, x=None, g=None, option=_lib.VJP_K2):
    """Two runs, bit-identical, the guards untouched; expect(launch) asserts what the launch must report."""
    got, launch, bits = vjp_guarded(torch, net, case, x, g, option)
    expect(launch)
    _, launch2, bits2 = vjp_guarded(torch, net, case, x, g, option)
    assert launch2 == launch and np.array_equal(bits, bits2), f"{case.tag}: two runs differ in some bit"
    return got, bits


def vjp_refused(torch, case, option, match="IRBFN_ERR_UNSUPPORTED"):
    """A forced kernel that cannot take the case: creating the net's descriptor, setting the option or the call raises ValueError
    with `match`, and the NaN-filled buffer of guarded_out is still all NaN afterwards."""
    buf, _, _, out = guarded_out(torch, case)
    xd, gd = torch.from_numpy(case.x).cuda(), torch.from_numpy(case.g).cuda()
    net = make_net(case)
    with pytest.raises(ValueError, match=match):
        net.set_options(vjp_kernel=option)
        try:
            net.vjp(case.params, xd, gd, out=out)
        finally:
            net.set_options(vjp_kernel=_lib.VJP_AUTO)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all()), f"{case.tag}: a refused call wrote into its output"
