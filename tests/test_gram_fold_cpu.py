"""The folded slot tables of K1g's forward (`gram_fold_slot`, irbfn_amd/csrc/rbf_forward_gram.h) restated in NumPy: two k = 32
operands per 16 x 16 tile, the eleven fixed-point heads in k 0..15 of operand 0 (lane groups 0 and 1, which the matrix core
sums and accumulates exactly) and the 47 tails behind them.  Every product of the expansion appears once, no head lies at
k >= 16 or in operand 1, and the float64 sum over all slots is u = alpha |x - c|^2 + beta up to what the parts rule drops."""
import numpy as np
import pytest

DIMS = 8
COMB = [(0, 1), (1, 0), (0, 2), (2, 0), (1, 1)]          # (part of the query-side factor, part of the centre-side factor)
EMPTY = (0, 0, 0, 0)


def fold_slot(o, k):
    """(kind, dim, p, q): kind 0 empty, 1 x'_dim part p x C_dim part q, 2 Q part p x alpha part q, 3 1 x c2 part p."""
    g, j = k >> 3, k & 7
    if o == 0 and g < 2:
        if j < 2:
            return (1, 2 * g + j, 0, 0)
        if j < 4:
            return (1, 4 + 2 * g + (j - 2), 0, 0)
        if g == 0:
            return (2, 0, 0, 0) if j == 4 else EMPTY
        return (3, 0, 0, 0) if j == 4 else ((3, 0, 1, 0) if j == 5 else EMPTY)
    if o == 0:
        if j < 5:
            return (1, 2 * g, *COMB[j])
        if j < 7:
            return (1, 2 * (g - 2) + (j - 5), 1, 1)
        return (3, 0, 3, 0) if g == 2 else EMPTY
    if g < 2:
        return (1, 2 * g + (j >> 2), *COMB[j & 3])
    if j < 5:
        return (1, 2 * g + 1, *COMB[j])
    m = (g - 2) * 3 + (j - 5)
    return (2, 0, *COMB[m]) if m < 5 else (3, 0, 2, 0)


SLOTS = [(o, k, fold_slot(o, k)) for o in range(2) for k in range(32)]


def is_head(sl):
    return sl[2] < 2 if sl[0] == 3 else sl[2] + sl[3] == 0


def test_every_product_of_the_expansion_sits_in_exactly_one_slot():
    want = [(1, d, p, q) for d in range(DIMS) for p in range(3) for q in range(3 - p)]
    want += [(2, 0, p, q) for p in range(3) for q in range(3 - p)]
    want += [(3, 0, p, 0) for p in range(4)]
    used = [sl for _, _, sl in SLOTS if sl[0] != 0]
    assert len(want) == 58 and sorted(used) == sorted(want)                 # once each, and nothing else
    assert len(SLOTS) - len(used) == 6


def test_heads_sit_in_k_0_to_15_of_operand_0_and_nowhere_else():
    heads = [(o, k) for o, k, sl in SLOTS if sl[0] != 0 and is_head(sl)]
    assert len(heads) == 11 and all(o == 0 and k < 16 for o, k in heads)
    assert all(is_head(sl) for o, k, sl in SLOTS if o == 0 and k < 16 and sl[0] != 0)     # no tail among them
    assert all(not is_head(sl) for o, k, sl in SLOTS if (o == 1 or k >= 16) and sl[0] != 0)


def test_a_lane_group_converts_only_its_own_coordinates_but_for_one_exchange():
    """Group g splits coordinates 2 g and 2 g + 1.  What its slots hold of other coordinates is the partner group's (g ^ 2: lane
    ^ 32) two heads (groups 0, 1) or two (1, 1) tails (groups 2, 3), in coordinate order: one dword per query tile."""
    for g in range(4):
        foreign = [(o, k, sl) for o, k, sl in SLOTS if k >> 3 == g and sl[0] == 1 and sl[1] >> 1 != g]
        assert len(foreign) == 2 and all(o == 0 for o, _, _ in foreign)
        assert [sl[1] for _, _, sl in foreign] == [2 * (g ^ 2), 2 * (g ^ 2) + 1]
        assert all((sl[2], sl[3]) == ((0, 0) if g < 2 else (1, 1)) for _, _, sl in foreign)


def f16(v):
    return np.asarray(v, np.float64).astype(np.float16).astype(np.float64)


def parts(v, E):
    """gram_parts_d: v = 2^E (n0 + 2^-11 n1 + 2^-22 n2), n0 on the grid 2^-10, n1 and n2 f16 values."""
    a = v * 2.0 ** -E
    n0 = np.rint(a * 1024.0) / 1024.0
    r1 = (a - n0) * 2048.0
    n1 = f16(r1)
    n2 = f16((r1 - n1) * 2048.0)
    return [n0, n1, n2]


def parts_c2(v, E):
    """gram_parts_c2: two fixed-point heads, two f16 tails."""
    a = v * 2.0 ** -E
    n0 = np.rint(a * 1024.0) / 1024.0
    r1 = (a - n0) * 2048.0
    n1 = np.rint(r1 * 1024.0) / 1024.0
    r2 = (r1 - n1) * 2048.0
    n2 = f16(r2)
    n3 = f16((r2 - n2) * 2048.0)
    return [n0, n1, n2, n3]


def exp_above(v):
    return int(np.frexp(float(v))[1])                     # smallest e with |v| < 2^e for v > 0


@pytest.mark.parametrize("D", [3, 4, 7, 8])
def test_the_float64_sum_over_all_slots_is_u(D):
    """Random (x, c, alpha) inside the box.  What the sum may miss, from the parts rule: a factor is represented up to
    2^(E - 33) (the f16 rounding of its last part, |n2| <= 1/2), and of the nine part products the table keeps the six with
    p + q <= 2 -- the dropped (1, 2), (2, 1) weigh 2^-33 |n1 n2| <= 2^-34 each, (2, 2) 2^-46.  Per coordinate that is below
    (2 + 1 + 1) 2^-33 = 2^-31 of 2^(ex + ec), the same for Q x alpha, and c2 (four parts, no product) is good to 2^(e2 - 43)."""
    rng = np.random.default_rng(D)
    n = 4000
    half = rng.uniform(0.5, 6.0)
    cp = rng.uniform(-half, half, size=(n, D))                               # c' = c - r
    xp = rng.uniform(-1.2 * half, 1.2 * half, size=(n, D))                    # x' inside the box |x'| < 2^ex
    xp[: n // 4] = cp[: n // 4] + rng.normal(0, 0.01, size=(n // 4, D))       # near a centre: the expansion cancels
    xp[: n // 16] = cp[: n // 16]
    alpha = -rng.uniform(0.05, 3.0, size=n)                                  # gaussian: u = -|x - c|^2 / (2 sigma^2) ... + beta
    beta = 14.0
    ex = exp_above(1.25 * half)
    ea = exp_above(np.abs(alpha).max())
    ec = exp_above(2.0 * np.abs(alpha).max() * half)
    eq = max(2 * ex + int(np.ceil(np.log2(D))), ex + ec - ea)
    e2 = max(exp_above(np.abs(alpha).max() * D * half * half + beta), ex + ec + 1)
    Q = (xp * xp).sum(axis=1)
    Cm = -2.0 * alpha[:, None] * cp
    c2 = alpha * (cp * cp).sum(axis=1) + beta
    assert np.abs(xp).max() < 2.0 ** ex and Q.max() < 2.0 ** eq and np.abs(Cm).max() < 2.0 ** ec and np.abs(c2).max() < 2.0 ** e2
    nx = [parts(xp[:, d], ex) if d < D else [np.zeros(n)] * 3 for d in range(DIMS)]
    nC = [parts(Cm[:, d], ec) if d < D else [np.zeros(n)] * 3 for d in range(DIMS)]
    nq, na, n2 = parts(Q, eq), parts(alpha, ea), parts_c2(c2, e2)
    total = np.zeros(n)
    head = np.zeros(n)
    for o, k, (kind, dim, p, q) in SLOTS:
        if kind == 0:
            continue
        if kind == 1:
            v = nx[dim][p] * nC[dim][q] * 2.0 ** (ex + ec - 11 * (p + q))
        elif kind == 2:
            v = nq[p] * na[q] * 2.0 ** (eq + ea - 11 * (p + q))
        else:
            v = n2[p] * 2.0 ** (e2 - 11 * p)
        total += v
        if o == 0 and k < 16:
            head += v
            assert np.array_equal(v, np.rint(v * 2.0 ** (20 - ex - ec)) * 2.0 ** (ex + ec - 20))     # on the head grid
    u = alpha * ((xp - cp) ** 2).sum(axis=1) + beta
    tol = D * 2.0 ** (ex + ec - 31) + 2.0 ** (eq + ea - 31) + 2.0 ** (e2 - 43)
    tol += 64 * np.finfo(np.float64).eps * 2.0 ** max(e2, eq + ea, ex + ec + 3)                          # float64 rounding of the 58 terms and of u itself
    assert np.abs(total - u).max() <= tol, (np.abs(total - u).max(), tol)
    # the heads alone are u up to the tails: 2^-10 of the terms, not of u -- the cancellation the first two lane groups carry exactly
    assert np.abs(head - u).max() <= D * 2.0 ** (ex + ec - 9) + 2.0 ** (eq + ea - 9) + 2.0 ** (e2 - 21)
