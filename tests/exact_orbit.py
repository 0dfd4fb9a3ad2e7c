"""The oracle's chain of one-second J2 RK4 steps and its 6x6 sensitivity (oracle/ba_oracle.py: _accel, _accel_jac, rk4_step_stm,
propagate_orbit), restated in np.longdouble -- the EXACT chain that the fp64 walks (the oracle's, the GPU's) round away from.

Same formulas, same fp64 constants (MU, J2C, J2_MAT, widened without change); only the arithmetic is 64-bit-mantissa extended
precision (x86 long double: eps 1.1e-19, four thousand times below fp64's).  The oracle's own propagate_orbit cannot simply be
fed long doubles: it allocates Phi in float64.

``coarse_chain`` restates the first stage of vba_long.hip's long_states (the coarse chain of one RK4 step per chunk and the
linearised sweep) in fp64, for the question whether a FINITE start state can make that chain non-finite while the serial walk
stays finite (see its docstring)."""
import numpy as np

from oracle import ba_oracle as O

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "needs an extended-precision long double"

MU = LD(O.MU)
J2C = LD(O.J2C)
J2_MAT = O.J2_MAT.astype(LD)
EYE3 = np.eye(3, dtype=LD)


def _accel(p):
    r2 = (p * p).sum(-1, keepdims=True)
    r = np.sqrt(r2)
    u = (p * p) @ J2_MAT.T
    return -(MU / r ** 3) * p + (J2C / r ** 7) * u * p


def _accel_jac(p):
    r2 = (p * p).sum(-1)
    r = np.sqrt(r2)
    u = (p * p) @ J2_MAT.T
    pp = p[..., :, None] * p[..., None, :]
    G = -MU * (EYE3 / (r ** 3)[..., None, None] - 3 * pp / (r ** 5)[..., None, None])
    up = u * p
    return G + J2C * (-7 * up[..., :, None] * p[..., None, :] / (r ** 9)[..., None, None]
                      + (2 * J2_MAT * pp + u[..., :, None] * EYE3) / (r ** 7)[..., None, None])


def _deriv(x):
    return np.concatenate([x[..., 3:], _accel(x[..., :3])], -1)


def _deriv_jvp(x, T):
    G = _accel_jac(x[..., :3])
    return np.concatenate([T[..., 3:, :], G @ T[..., :3, :]], -2)


def rk4_step(x, h=1):
    h = LD(h)
    f1 = _deriv(x)
    f2 = _deriv(x + h / 2 * f1)
    f3 = _deriv(x + h / 2 * f2)
    f4 = _deriv(x + h * f3)
    return x + (h / 6) * (f1 + 2 * f2 + 2 * f3 + f4)


def rk4_step_stm(x, Phi, h=1):
    h = LD(h)
    f1 = _deriv(x)
    d1 = _deriv_jvp(x, Phi)
    x2 = x + h / 2 * f1
    f2 = _deriv(x2)
    d2 = _deriv_jvp(x2, Phi + h / 2 * d1)
    x3 = x + h / 2 * f2
    f3 = _deriv(x3)
    d3 = _deriv_jvp(x3, Phi + h / 2 * d2)
    x4 = x + h * f3
    f4 = _deriv(x4)
    d4 = _deriv_jvp(x4, Phi + h * d3)
    return x + (h / 6) * (f1 + 2 * f2 + 2 * f3 + f4), Phi + (h / 6) * (d1 + 2 * d2 + 2 * d3 + d4)


def propagate(x, steps, stm=True):
    """x [n,6] (any float type) over steps[i] one-second steps, in long double: x_hat [n,6] (, Phi [n,6,6]), long double."""
    x = np.array(x, dtype=LD).reshape(-1, 6)
    steps = np.asarray(steps, dtype=np.int64).reshape(-1)
    n = x.shape[0]
    Phi = np.broadcast_to(np.eye(6, dtype=LD), (n, 6, 6)).copy()
    for s in range(int(steps.max()) if n else 0):
        act = steps > s
        if stm:
            x[act], Phi[act] = rk4_step_stm(x[act], Phi[act])
        else:
            x[act] = rk4_step(x[act])
    return (x, Phi) if stm else x


def edge_errors(xh, Phi, xh_ex, Phi_ex):
    """Per edge, against the exact chain: (position max-rel, velocity max-rel, Phi position columns, Phi velocity columns),
    each [n]; the two column blocks (both row blocks) are normalised by their own max, so a wrong velocity column cannot hide
    behind the larger position columns."""
    xh, Phi = np.asarray(xh, dtype=LD), np.asarray(Phi, dtype=LD)
    d = np.abs(xh - xh_ex)
    pos = d[:, :3].max(1) / np.abs(xh_ex[:, :3]).max(1)
    vel = d[:, 3:].max(1) / np.abs(xh_ex[:, 3:]).max(1)
    D = np.abs(Phi - Phi_ex)
    cp = D[:, :, :3].max((1, 2)) / np.abs(Phi_ex[:, :, :3]).max((1, 2))
    cv = D[:, :, 3:].max((1, 2)) / np.abs(Phi_ex[:, :, 3:]).max((1, 2))
    return tuple(np.asarray(v, dtype=np.float64) for v in (pos, vel, cp, cv))


# ------------------------------------------------------------------------------------------------ coarse chain of long_states
def coarse_chain(x0, s):
    """vba_long.hip long_states up to its first defect check, in fp64, for a batch of start states x0 [N,6] over s steps each:
    the plan of s steps (long_plan), the coarse chain (one RK4 step of L s per chunk, the tail chunk shorter), the fine pass of
    every chunk from its coarse start state, one linearised sweep c_{j+1} = (F_j - N_j) + A_j c_j (A_j the coarse step's
    Jacobian) and the serial walk of s one-second steps.  Returns per start state (coarse chain and sweep finite,
    serial walk finite, max |c| / max |x0|).

    The question it answers (vba_long.hip breaks out of the iteration on a non-finite defect): is there a FINITE start state
    whose coarse chain or sweep goes non-finite while its serial walk stays finite?  An RK4 stage is non-finite only where
    |p|^2 underflows to 0 or |p|^7 / |p|^9 leave the fp64 range; a coarse step of L <= 94 s (16 384 s at the gap limit) that
    passes close to the Earth's centre throws the chain far off (|c| / |x| of 3e2 at seed 315's diverged states, 7e3 at seed
    318's, whose pose starts 1 735 km from the centre; up to 1e16 on exactly radial states), but MU / r^2 then falls off, and
    the chain and the sweep stay hundreds of binades below overflow.  Searched: seed 315's and 318's diverged states, exactly
    and nearly radial states from 100 .. 1e5 km at 0.5 .. 12 km/s, gaps of 65 .. 6000 s (2 800 states; a share of them in
    tests/test_exact_orbit.py): none was found, so the kernel keeps its single non-finite exit and no edge needs a serial
    fallback."""
    x0 = np.asarray(x0, dtype=np.float64).reshape(-1, 6)
    s = int(s)
    L, P = _plan(s)
    lens = [L] * (P - 1) + [s - (P - 1) * L]
    n = x0.shape[0]
    with np.errstate(all="ignore"):
        U = np.zeros((P, n, 6))
        N = np.zeros((P, n, 6))
        u = x0.copy()
        for j in range(P):
            U[j] = u
            u = O.rk4_step(u, float(lens[j]))
            N[j] = u
        F = U.copy()
        for q in range(L):
            act = np.array([q < ln for ln in lens])
            F[act] = O.rk4_step(F[act])
        c = np.zeros((n, 6))
        cmax = np.zeros(n)
        ok = np.isfinite(N).all((0, 2)) & np.isfinite(F).all((0, 2))
        for j in range(P):
            _, A = O.rk4_step_stm(U[j], np.broadcast_to(np.eye(6), (n, 6, 6)).copy(), float(lens[j]))
            c = (F[j] - N[j]) + np.einsum("nab,nb->na", A, c)
            ok &= np.isfinite(c).all(1)
            cmax = np.maximum(cmax, np.abs(c).max(1))
        serial = O.propagate_orbit(x0, np.full(n, s), stm=False)
    return ok, np.isfinite(serial).all(1), cmax / np.abs(x0).max(1)


def _plan(s):
    """(L, P) of vba_math.h long_plan."""
    L = 1
    while 45 * L * L < 34 * s:
        L += 1
    if 64 * L < s:
        L = (s + 63) // 64
    return L, (s + L - 1) // L
