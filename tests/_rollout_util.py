"""Roll-out test helpers shared by test_gpu_parity.py and test_gpu_rollout_horizons.py: seeded input rows and the
state comparison against the float64 oracle.  A plain module (no fixtures, no hooks)."""
import numpy as np

RTOL = 1e-5          # north_star tolerance


def assert_states_close(got, ref, ref32=None, rtol=RTOL, floor=1e-3, k32=4.0):
    """Trajectory states against the float64 oracle.  Pass if |err| <= rtol * (|ref| + scale), scale =
    max |ref| of that state component along the trajectory -- or, where float32 integration itself is
    worse conditioned than that (T = 50 steps; the dynamic single-track RHS has a prefactor
    mu*m/(I*L) = 67 and 1/V terms), if the error is within k32 = 4x the error the float32 NumPy restatement
    of the reference makes on the same trajectory component (the reference itself runs in float32).
    ``floor``: the least scale, a number or one per row ([B, 1, 1])."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape
    scale = np.maximum(np.abs(ref).max(axis=1, keepdims=True), floor)
    err = np.abs(got - ref)
    bound = rtol * (np.abs(ref) + scale)
    if ref32 is not None:
        e32 = np.abs(np.asarray(ref32, np.float64) - ref).max(axis=1, keepdims=True)
        bound = np.maximum(bound, k32 * e32 + 1e-7 * scale)
    bad = err > bound
    assert not bad.any(), (int(bad.sum()), float(err.max()), float((err / (np.abs(ref) + scale)).max()))


def st_inputs(B, T, seed, fast=True):
    rng = np.random.default_rng(seed)
    st = rng.normal(size=(B, 7)) * [2, 2, .3, 1, 1, .4, .1]
    st[:, 3] = rng.uniform(0.2, 7.5, B) if fast else rng.uniform(0.0, 2.9, B)
    u = np.hstack([rng.normal(size=(B, T)) * 5.0, rng.normal(size=(B, T)) * 2.0])
    return np.hstack([st, u])


def frenet_inputs(B, T, rng):
    """[s, ey, delta, vx, vy, wz, epsi, cur] + controls; curvature / offsets kept in the range of a
    race track (|ey*cur| << 1) so that 1/(1 - ey*cur) (dynamics.py:268) stays away from its pole over T steps."""
    st = rng.normal(size=(B, 8)) * [1, .2, .2, 1, .1, .1, .15, .08] + [0, 0, 0, 4, 0, 0, 0, 0]
    amp = 1.0 if T <= 10 else 0.25
    return np.hstack([st, rng.normal(size=(B, T)) * 5 * amp, rng.normal(size=(B, T)) * 2 * amp])


def frenet_inputs_long(B, T, seed, dp, margin=0.5):
    """Frenet rows for long horizons: B rows whose float64 trajectory keeps max |ey*cur| < margin over all T steps, i.e.
    stays off the pole of 1/(1 - ey*cur).  Calmer than frenet_inputs (slower, straighter, smaller controls); random rows
    that still wander towards the pole are dropped."""
    from oracle import irbfn_oracle as orc
    rng = np.random.default_rng(seed)
    n = 2 * B + 16
    st = rng.normal(size=(n, 8)) * [1, .3, .05, .5, .1, .1, .05, .03] + [0, 0, 0, 3, 0, 0, 0, 0]
    xf = np.hstack([st, rng.normal(size=(n, T)), rng.normal(size=(n, T)) * 0.3]).astype(np.float32).astype(np.float64)
    if T == 0:
        return xf[:B]
    ref = orc.integrate_frenet_mult(xf, dp)
    keep = np.abs(ref[:, :, 1] * ref[:, :, 7]).max(axis=1) < margin
    assert keep.sum() >= B, (int(keep.sum()), B)
    return xf[keep][:B]


def spiral_inputs(B, seed):
    rng = np.random.default_rng(seed)
    return np.hstack([rng.normal(size=(B, 4)) * .3, rng.uniform(1, 10, size=(B, 1))])
