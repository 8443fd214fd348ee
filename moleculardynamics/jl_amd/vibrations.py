"""Vibrational analysis of a configuration: the Hessian of the pair energy as an operator on the device (md_hess_*),
its diagonal blocks, and the lowest modes by Lanczos with the basis resident on the device.

With U(r) the pair energy, t = U'/r, k = U'' and n = (x_i - x_j)/r,
    (H X)_i = sum_j [(k - t) n (n . (X_i - X_j)) + t (X_i - X_j)]
over the pairs the force kernels take.  H is the Hessian of the smooth part of the energy: the jump of U or U' at a sharp
cutoff (plain Lennard-Jones) contributes nothing.  New relative to the reference, which has no second derivatives."""
import numpy as np

from .simulation import _configure_device

DENSE_MAX_DOF = 4096      # HessianOperator.dense(): N d above this is refused (a 4096 x 4096 fp64 matrix is 128 MiB)


class HessianOperator:
    """H of `state` under params.potential, frozen on the state's frame on its device handle.

    matvec(X): H X for X of shape (N, d) or (m, N, d), any m (blocks of 8 on the device).  blocks(): the diagonal blocks
    H_ii (N, d, d): the local stiffness; trace / d is the squared Einstein frequency.  dense(): the N d x N d matrix, by
    applying H to identity columns (refused above DENSE_MAX_DOF degrees of freedom).  Every call raises (MdhipError) once
    the handle's frame has been changed by an upload, a run, a minimisation or swap rounds: build a new operator then."""

    def __init__(self, state, params):
        spec = params.potential.device_spec()
        if spec[0] != "builtin":
            raise ValueError("HessianOperator needs a built-in potential (user potentials have no second derivative here)")
        dev = _configure_device(state, params)
        dev.upload(x=state.system.positions, v=state.velocities, images=state.images, diameters=state.diameters)
        dev.hess_setup()
        self.device = dev
        self.n, self.dim = dev.n, dev.dim
        self.shape = (self.n * self.dim, self.n * self.dim)

    def matvec(self, X):
        X = np.asarray(X, dtype=np.float64)
        single = X.ndim == 2
        if single:
            X = X[None]
        if X.ndim != 3 or X.shape[1:] != (self.n, self.dim):
            raise ValueError(f"expected vectors of shape ({self.n}, {self.dim}) or (m, {self.n}, {self.dim}), got {X.shape}")
        B = self.device.HESS_MAX_BLOCK
        Y = np.empty(X.shape)
        for a in range(0, X.shape[0], B):
            Y[a:a + B] = self.device.hess_apply(X[a:a + B])
        return Y[0] if single else Y

    def blocks(self):
        return self.device.hess_blocks()

    def dense(self):
        nd = self.n * self.dim
        if nd > DENSE_MAX_DOF:
            raise ValueError(f"dense(): N d = {nd} exceeds {DENSE_MAX_DOF}; use matvec or lowest_modes")
        B = self.device.HESS_MAX_BLOCK
        H = np.empty((nd, nd))
        for a in range(0, nd, B):
            m = min(B, nd - a)
            E = np.zeros((m, nd))
            E[np.arange(m), a + np.arange(m)] = 1.0
            H[:, a:a + m] = self.device.hess_apply(E.reshape(m, self.n, self.dim)).reshape(m, nd).T
        return H


def participation_ratio(modes):
    """P = (sum_i |e_i|^2)^2 / (N sum_i |e_i|^4) of modes (nvec, N, d): 1 for a plane wave's uniform amplitude, 1/N for
    one moving particle."""
    e2 = (np.asarray(modes, dtype=np.float64) ** 2).sum(axis=-1)
    return e2.sum(axis=-1) ** 2 / (e2.shape[-1] * (e2 ** 2).sum(axis=-1))


def _tridiagonal(alpha, beta):
    k = len(alpha)
    T = np.diag(alpha)
    if k > 1:
        T += np.diag(beta[:k - 1], 1) + np.diag(beta[:k - 1], -1)
    return T


def lowest_modes(state, params, nmodes, tol=1e-8, k0=None, kmax=None, seed=0):
    """The nmodes lowest vibrational modes of `state` (the D uniform translations deflated).

    k Lanczos steps with full reorthogonalisation run on the device; the k x k tridiagonal matrix is diagonalised here;
    the nmodes lowest Ritz pairs go back to the device for their residuals |H y - theta y|.  k doubles (restarting from
    the same seed) until every residual is <= tol * |H|, |H| estimated by the largest Ritz value, or kmax is reached.
    Defaults: k0 = max(4 nmodes, 32), kmax = N d - d (the whole deflated space, where Lanczos is exact).

    Returns dict(eigenvalues, frequencies (sqrt(lambda); nan for a negative one), modes (nmodes, N, d), residuals,
    participation (the participation ratios), stable, converged, ksteps (the last k), norm (the |H| estimate), operator
    (the HessianOperator, still valid)).  A negative eigenvalue beyond max(its residual, tol |H|) marks a saddle:
    stable = False; nothing is raised.  kmax reached before convergence: converged = False, nothing is raised.

    Unrestarted Lanczos needs many steps for modes inside a dense band: at large N the basis (k vectors of N d doubles on
    the device) and the k^2 N d reorthogonalisation grow quickly.  Thick restart, a stochastic density of states and
    elastic moduli are not provided."""
    nmodes = int(nmodes)
    op = HessianOperator(state, params)
    nd, d = op.n * op.dim, op.dim
    kfull = nd - d
    if not 1 <= nmodes <= kfull:
        raise ValueError(f"nmodes must be in 1..{kfull}")
    if not tol > 0.0:
        raise ValueError("tol must be > 0")
    kmax = kfull if kmax is None else int(kmax)
    if not nmodes <= kmax <= kfull:
        raise ValueError(f"kmax must be in nmodes..{kfull}")
    k = max(4 * nmodes, 32) if k0 is None else int(k0)
    if k < nmodes:
        raise ValueError("k0 must be >= nmodes")
    k = min(k, kmax)
    dev = op.device
    while True:
        alpha, beta = dev.hess_lanczos(k, seed)
        theta, S = np.linalg.eigh(_tridiagonal(alpha, beta))
        norm = float(np.abs(theta).max())
        modes, resid = dev.hess_ritz(S[:, :nmodes], theta[:nmodes])
        converged = bool((resid <= tol * norm).all())
        if converged or k >= kmax:
            break
        k = min(2 * k, kmax)
    lam = theta[:nmodes].copy()
    with np.errstate(invalid="ignore"):
        freq = np.sqrt(lam)
    return dict(eigenvalues=lam, frequencies=freq, modes=modes, residuals=resid, participation=participation_ratio(modes),
                stable=bool((lam > -np.maximum(resid, tol * norm)).all()), converged=converged, ksteps=k, norm=norm,
                operator=op)
