"""The float64 statement the region-weighted matrix-core forward (rbf_fwd_f16gram_gamma) is tested against:
out[b, o] = sum_r gamma[b, r] sum_k phi[b, r, k] W[k, o] + bias[o] for ARBITRARY region weights gamma[B, R], and the
magnitude of its terms sum_r sum_k |gamma phi W| -- the scale of the per-element bound of tests/test_gpu_fullsize.py.
Plain NumPy in row chunks; a plain module (no fixtures, no hooks)."""
import numpy as np

from oracle import irbfn_oracle as orc

CHUNK_ELEMS = 1 << 23          # float64 elements of one chunk's [rows, R, K, D] difference tensor


def softmax_gamma(params, x):
    """The cluster gate (model.py:402-404) in float64: gamma[B, R]."""
    p = params["params"]["cluster"]
    logits = np.asarray(x, np.float64) @ np.asarray(p["kernel"], np.float64) + np.asarray(p["bias"], np.float64)
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def gamma_forward64(cfg, params, x, gamma):
    """(out, scale), float64 [B, O] each.  A NaN in gamma gives NaN in that row of both."""
    p = params["params"] if "params" in params else params
    c = np.asarray(p["rbf_list"]["centers"], np.float64)
    ls = np.asarray(p["rbf_list"]["log_sigs"], np.float64)
    W = np.asarray(p["linear"]["kernel"], np.float64)
    bias = np.asarray(p["linear"]["bias"], np.float64)
    x = np.asarray(x, np.float64)
    gamma = np.asarray(gamma, np.float64)
    R, K, D = c.shape
    assert gamma.shape == (x.shape[0], R), gamma.shape
    rows = max(1, CHUNK_ELEMS // (R * K * D))
    outs, scales = [], []
    with np.errstate(invalid="ignore"):
        for i in range(0, x.shape[0], rows):
            phi = orc.rbf_layer(x[i:i + rows], c, ls, cfg["basis_func"])             # [rows, R, K]
            g = gamma[i:i + rows, :, None]
            outs.append((g * phi).sum(1) @ W + bias)
            scales.append((np.abs(g) * np.abs(phi)).sum(1) @ np.abs(W))
    return np.concatenate(outs), np.concatenate(scales)


def assert_elementwise(got, ref, scale, what):
    """|err| <= 1e-5 |ref| + 3e-6 sum |gamma phi W| per element (tests/test_gpu_fullsize.py); returns max err / bound."""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), what
    err = np.abs(got - ref)
    bound = 1e-5 * np.abs(ref) + 3e-6 * scale
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"cluster_gram {what}: max err / bound = {ratio:.3f}, max err / sum|terms| = {float((err / np.maximum(scale, 1e-300)).max()):.2e}")
    assert (err <= bound).all(), (what, ratio, float(err.max()))
    return ratio
