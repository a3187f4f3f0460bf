"""tests/_train_step_util.py -- the float64 statements test_gpu_train_step.py holds the training-step kernels to -- against
torch.autograd (float64) of the oracle's own loss compositions (orc.train_*_loss with y_pred put in place of the net's output),
torch.nn.functional.cross_entropy and torch.optim.Adam.  No GPU."""
from unittest import mock

import numpy as np
import pytest
import torch

import _train_step_util as tu
from irbfn_amd import configs
from oracle import irbfn_oracle as orc

DP = np.array(configs.DYN_PARAMS, np.float64)
B = 301
ROWS = (0, B - 1, 7)


def _autograd(kind, x, yp, y):
    """(loss, d loss / d y_pred) of orc.train_<kind>_loss with y_pred as the leaf: the net's apply returns the leaf"""
    leaf = torch.tensor(yp, dtype=torch.float64, requires_grad=True)
    xt, yt = torch.tensor(x, dtype=torch.float64), torch.tensor(y, dtype=torch.float64)
    with mock.patch.object(orc, "wcrbfnet_apply", lambda cfg, params, x_, **kw: leaf):
        if kind == "oneint":
            loss = orc.train_oneint_loss(None, None, xt, yt, DP)
        elif kind == "fullint":
            loss = orc.train_fullint_loss(None, None, xt, yt)
        else:
            loss = orc.train_frenet_fullint_loss(None, None, xt, yt, DP)
    (g,) = torch.autograd.grad(loss, leaf)
    return float(loss.detach()), g.numpy()


def _case(kind, n, seed):
    if kind == "oneint":
        x, yp, y = tu.oneint_case(B, n, 7, seed)
    elif kind == "fullint":
        x, yp, y = tu.fullint_case(B, n, 3, seed)
    else:
        x, yp, y = tu.frenet_case(B, n, 8, seed)
    used = tu.splice_rows(kind, x, yp, y, ROWS, DP)
    return x, yp, y, used


def _statement(kind, x, yp, y, tie):
    if kind == "fullint":
        return tu.seeds_fullint(x, yp, y, tie)
    return (tu.seeds_oneint if kind == "oneint" else tu.seeds_frenet_fullint)(x, yp, y, DP, tie)


def _typed(kind, x, yp, y, tie, ft):
    if kind == "fullint":
        return tu.seeds_fullint_typed(x, yp, y, tie, ft)
    return (tu.seeds_oneint_typed if kind == "oneint" else tu.seeds_frenet_fullint_typed)(x, yp, y, DP, tie, ft)


CASES = [("oneint", n) for n in (2, 3, 10)] + [("fullint", n) for n in (1, 4, 5, 9, 64)] + [("frenet", n) for n in (1, 5, 6, 16)]


@pytest.mark.parametrize("kind,n", CASES)
def test_seed_statement_is_autograd_of_the_loss(kind, n):
    """Off the kinks gy is torch.autograd's to 1e-12 of max |gy|.  On a clip bound torch.clip passes the whole cotangent
    (its mask is lo <= v <= hi), so the tie rows agree with autograd at tie = 1.  sgn(0) = 0 on both sides (the zero row)."""
    x, yp, y, used = _case(kind, n, seed=100 + n)
    loss_ref, g_ref = _autograd(kind, x, yp, y)
    loss, gy, amb = _statement(kind, x, yp, y, 0.5)
    assert amb.mean() <= tu.AMBIGUOUS_CAP
    ties = [used[k] for k in ("tie_lo", "tie_hi")]
    plain = ~amb
    plain[ties] = False
    assert plain[used["zero"]]
    scale = np.abs(g_ref).max()
    assert abs(loss - loss_ref) <= 1e-12 * abs(loss_ref)
    assert np.abs(gy[plain] - g_ref[plain]).max() <= 1e-12 * scale
    gy1 = _statement(kind, x, yp, y, 1.0)[1]
    assert np.abs(gy1[ties] - g_ref[ties]).max() <= 1e-12 * scale
    assert np.abs(gy[ties] - g_ref[ties]).max() > 1e-3 * scale          # ... and tie = 0.5 does not: the rows are on a bound


@pytest.mark.parametrize("kind,n", CASES)
def test_tie_scales_the_tie_rows_and_nothing_else(kind, n):
    x, yp, y, used = _case(kind, n, seed=200 + n)
    g0, gh, g1 = (_statement(kind, x, yp, y, tie)[1] for tie in (0.0, 0.5, 1.0))
    ties = [used[k] for k in ("tie_lo", "tie_hi")]
    others = np.setdiff1d(np.arange(B), ties)
    assert np.array_equal(g0[others], gh[others]) and np.array_equal(g0[others], g1[others])
    full = g1[ties] - g0[ties]
    assert (np.abs(full).max(axis=1) > 0).all()
    assert np.abs((gh[ties] - g0[ties]) - 0.5 * full).max() <= 1e-15 * np.abs(g1).max()
    # the loss does not depend on tie
    assert len({_statement(kind, x, yp, y, tie)[0] for tie in (0.0, 0.5, 1.0)}) == 1


@pytest.mark.parametrize("kind,n", CASES)
def test_typed_twin_in_float64_is_the_statement(kind, n):
    """The lines the float32 twins evaluate, run in float64, are the statement (they restate oracle/hand_vjp.py dtype-clean);
    run in float32 they stay float32 and land within float32 rounding of it."""
    x, yp, y, used = _case(kind, n, seed=300 + n)
    for tie in (0.0, 0.5, 1.0):
        loss, gy, amb = _statement(kind, x, yp, y, tie)
        loss64, gy64 = _typed(kind, x, yp, y, tie, np.float64)
        assert abs(loss64 - loss) <= 1e-14 * abs(loss) and np.abs(gy64 - gy).max() <= 1e-14 * np.abs(gy).max()
    loss32, gy32 = _typed(kind, x, yp, y, 0.5, np.float32)
    assert gy32.dtype == np.float32
    loss, gy, amb = _statement(kind, x, yp, y, 0.5)
    assert abs(float(loss32) - loss) <= 1e-5 * abs(loss)
    assert np.abs(gy32[~amb] - gy[~amb]).max() <= 1e-3 * np.abs(gy).max()


def test_ambiguity_flags_what_it_says():
    x, yp, y = tu.fullint_case(50, 5, 1, seed=1)
    base = tu.seeds_fullint(x, yp, y, 0.5)[2]
    rows = np.flatnonzero(~base)[:4]
    yp[rows[0], 0] = y[rows[0], 0] + 3e-6                    # an L1 difference within the margin
    yp[rows[1], 0] = y[rows[1], 0]                           # exactly 0: a tie, not ambiguous
    x[rows[2], 0], yp[rows[2], 0] = 0.0, 5e-5                # the first pre-clip speed 5e-6 above VMIN
    x[rows[3], 0], yp[rows[3], 0] = 0.0, 0.0                 # exactly on VMIN
    amb = tu.seeds_fullint(x, yp, y, 0.5)[2]
    assert list(amb[rows]) == [True, False, True, False]
    xf, ypf, yf = tu.frenet_case(50, 5, 8, seed=2)
    clear = np.flatnonzero(~tu.seeds_frenet_fullint(xf, ypf, yf, DP, 0.5)[2])[:2]
    ypf[clear[0], 0] = DP[10] + 2e-6
    ypf[clear[1], 0] = DP[10]
    amb = tu.seeds_frenet_fullint(xf, ypf, yf, DP, 0.5)[2]
    assert list(amb[clear]) == [True, False]


def test_ratio32_is_the_projects_float32_rule():
    """tu.ratio32 <= 1 exactly where tests/_rollout_util.assert_states_close passes the case taken as one trajectory"""
    import _rollout_util as ru
    rng = np.random.default_rng(0)
    ref = rng.normal(size=500) * 1e-3
    ref32 = ref + rng.normal(size=500) * 1e-10
    e32 = np.abs(ref32 - ref).max()
    for k, ok in ((0.5, True), (0.99, True), (1.01, False), (3.0, False)):
        got = ref.copy()
        got[17] += k * max(ru.RTOL * (abs(ref[17]) + np.abs(ref).max()), 4 * e32 + 1e-7 * np.abs(ref).max())
        assert (tu.ratio32(got, ref, ref32) <= 1.0) == ok
        try:
            ru.assert_states_close(got[None, :], ref[None, :], ref32[None, :], floor=0.0)
            passed = True
        except AssertionError:
            passed = False
        assert passed == ok
    bad = ref.copy()
    bad[3] = np.inf
    with pytest.raises(AssertionError):
        tu.ratio32(bad, ref, ref32)


@pytest.mark.parametrize("T", [1, 5, 9, 64])
def test_input_recipe_keeps_the_ambiguous_share_under_the_cap(T):
    x, yp, y = tu.fullint_case(20000, T, 1, seed=T)
    assert tu.seeds_fullint(x, yp, y, 0.5)[2].mean() <= tu.AMBIGUOUS_CAP
    if T <= 16:
        x, yp, y = tu.frenet_case(20000, T, 8, seed=T)
        assert tu.seeds_frenet_fullint(x, yp, y, DP, 0.5)[2].mean() <= tu.AMBIGUOUS_CAP


@pytest.mark.parametrize("R", [1, 2, 12])
@pytest.mark.parametrize("labels", ["onehot", "soft", "unnormalised"])
def test_softmax_xent_is_torch_cross_entropy(R, labels):
    rng = np.random.default_rng(R)
    Bx = 97
    logits = rng.normal(size=(Bx, R)) + rng.choice([-80.0, 0.0, 80.0], size=(Bx, 1))
    logits[5] = 1.25
    lab = make_labels(labels, Bx, R, rng)
    loss, g = tu.softmax_xent(logits, lab)
    lt = torch.tensor(logits, requires_grad=True)
    ref = torch.nn.functional.cross_entropy(lt, torch.tensor(lab))
    ref.backward()
    ref = float(ref.detach())
    assert abs(loss - ref) <= 1e-13 * abs(ref) or (R == 1 and loss == 0 == ref)
    assert np.abs(g - lt.grad.numpy()).max() <= 1e-14 / Bx * max(1.0, np.abs(lab).sum(1).max())


def make_labels(kind, Bx, R, rng):
    if kind == "onehot":
        return np.eye(R)[rng.integers(0, R, Bx)]
    lab = rng.uniform(0.0, 1.0, size=(Bx, R))
    if kind == "soft":
        lab /= lab.sum(axis=1, keepdims=True)
    return lab


def test_adam_clip_is_torch_adam_where_the_definitions_coincide():
    """No clipping happens (||g|| < max_norm), where clip_grad_norm_ (coefficient max_norm / (norm + 1e-6), capped at 1) and
    optax.clip_by_global_norm are both the identity: three steps of torch.optim.Adam from a zero state."""
    rng = np.random.default_rng(3)
    n = 1000
    p0 = rng.normal(size=n)
    p = torch.tensor(p0.copy(), requires_grad=True)
    opt = torch.optim.Adam([p], lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    pn, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    for t in range(1, 4):
        g = rng.normal(size=n) * 0.01
        p.grad = torch.tensor(g.copy())
        assert float(torch.nn.utils.clip_grad_norm_([p], 1.0)) < 1.0
        opt.step()
        pn, m, v = tu.adam_clip(pn, g, m, v, t, 1e-3, 0.9, 0.999, 1e-8, 1.0)
        assert np.abs(pn - p.detach().numpy()).max() <= 1e-13 * np.abs(p0).max()


@pytest.mark.parametrize("max_norm", [1.0, 1e-3, 0.0, -1.0])
def test_adam_clip_is_the_optax_formula(max_norm):
    rng = np.random.default_rng(4)
    n = 777
    p, g, m, v = rng.normal(size=n), rng.normal(size=n), rng.normal(size=n) * 0.1, rng.uniform(0.5, 1.5, n) * 0.01
    for t in (1, 2, 1000):
        gc = orc.clip_by_global_norm(g, max_norm) if max_norm > 0 else g
        ref = orc.adam_update(p, gc, m, v, t, lr=1e-3)
        got = tu.adam_clip(p, g, m, v, t, 1e-3, 0.9, 0.999, 1e-8, max_norm)
        for a, b in zip(got, ref):
            assert np.array_equal(a, b)
    # the boundary: ||g|| == max_norm is "not less", scale max_norm / ||g|| = 1 exactly
    g34 = np.zeros(n)
    g34[:2] = [3.0, 4.0]
    for a, b in zip(tu.adam_clip(p, g34, m, v, 5, 1e-3, 0.9, 0.999, 1e-8, 5.0), tu.adam_clip(p, g34, m, v, 5, 1e-3, 0.9, 0.999, 1e-8, 0.0)):
        assert np.array_equal(a, b)
    clipped = tu.adam_clip(p, g34, m, v, 5, 1e-3, 0.9, 0.999, 1e-8, 4.999)
    assert np.allclose(clipped[1][:2], 0.9 * m[:2] + 0.1 * np.array([3.0, 4.0]) * 4.999 / 5.0, rtol=1e-15, atol=0)
    # a zero gradient: no NaN; a NaN gradient under a positive max_norm: every parameter NaN
    assert np.isfinite(tu.adam_clip(p, np.zeros(n), m, v, 1, 1e-3, 0.9, 0.999, 1e-8, 1.0)[0]).all()
    gn = g.copy()
    gn[13] = np.nan
    assert np.isnan(tu.adam_clip(p, gn, m, v, 1, 1e-3, 0.9, 0.999, 1e-8, 1.0)[0]).all()
    assert np.isnan(tu.adam_clip(p, gn, m, v, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0)[0]).sum() == 1
