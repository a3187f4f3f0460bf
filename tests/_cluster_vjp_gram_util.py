"""The float64 statement the region-weighted matrix-core VJP (rbf_vjp_f16gram_gamma) is tested against: the four stage
leaves and d gamma of  sum(g * (sum_r gamma[b, r] sum_k phi[b, r, k] W[k, o] + bias[o]))  for ARBITRARY region weights
gamma[B, R] (not only a softmax), by torch.autograd in float64 over ``orc.rbf_layer``, and the magnitude of d gamma's terms
sum_k |hbar[b, k] phi[b, r, k]| -- the scale of the per-element bound of tests/test_gpu_fullsize.py.  Row chunks keep the
[rows, R, K, D] intermediate small.  A plain module (no fixtures, no hooks)."""
import numpy as np
import torch

from oracle import irbfn_oracle as orc

CHUNK_ELEMS = 1 << 23          # float64 elements of one chunk's [rows, R, K, D] difference tensor
STAGE = ("centers", "log_sigs", "kernel", "bias")


def gamma_vjp64(cfg, params, x, gamma, g):
    """(leaves, dgamma, dgamma_scale): leaves = {centers [R,K,D], log_sigs [R,K], kernel [K,O], bias [O]}, dgamma and its
    scale [B, R]; float64 NumPy arrays."""
    p = params["params"] if "params" in params else params
    t = lambda a, rg=False: torch.tensor(np.asarray(a, np.float64), requires_grad=rg)
    c, ls = t(p["rbf_list"]["centers"], True), t(p["rbf_list"]["log_sigs"], True)
    W, bias = t(p["linear"]["kernel"], True), t(p["linear"]["bias"], True)
    xs, gs = t(x), t(g)
    R, K, D = c.shape
    assert tuple(np.shape(gamma)) == (xs.shape[0], R), np.shape(gamma)
    rows = max(1, CHUNK_ELEMS // (R * K * D))
    acc = [torch.zeros_like(v) for v in (c, ls, W, bias)]
    dgam, scale = [], []
    for i in range(0, xs.shape[0], rows):
        gm = t(gamma[i:i + rows], True)
        phi = orc.rbf_layer(xs[i:i + rows], c, ls, cfg["basis_func"])                  # [rows, R, K]
        out = (gm[:, :, None] * phi).sum(1) @ W + bias
        grads = torch.autograd.grad((out * gs[i:i + rows]).sum(), [c, ls, W, bias, gm])
        acc = [a + b for a, b in zip(acc, grads[:4])]
        dgam.append(grads[4].numpy())
        with torch.no_grad():
            hbar = gs[i:i + rows] @ W.t()                                             # [rows, K]
            scale.append((hbar.abs()[:, None, :] * phi.abs()).sum(-1).numpy())
    return {n: a.numpy() for n, a in zip(STAGE, acc)}, np.concatenate(dgam), np.concatenate(scale)


def cluster_leaves_from_dgamma(params, x, gamma, dgamma, gl=None):
    """d gamma through the softmax backward (model.py:402-404) and logits = x Wc + bc: (d cluster.kernel [D,R], d cluster.bias [R]);
    gl: the direct cotangent of the logits."""
    x, gamma, dgamma = (np.asarray(a, np.float64) for a in (x, gamma, dgamma))
    dlogits = gamma * (dgamma - (gamma * dgamma).sum(1, keepdims=True))
    if gl is not None:
        dlogits = dlogits + np.asarray(gl, np.float64)
    return x.T @ dlogits, dlogits.sum(0)
