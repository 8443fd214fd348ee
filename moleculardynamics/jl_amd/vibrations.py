"""Vibrational analysis of a configuration: the Hessian of the pair energy as an operator on the device (md_hess_*),
its diagonal blocks, and the lowest modes by Lanczos with the basis resident on the device.

With U(r) the pair energy, t = U'/r, k = U'' and n = (x_i - x_j)/r,
    (H X)_i = sum_j [(k - t) n (n . (X_i - X_j)) + t (X_i - X_j)]
over the pairs the force kernels take.  H is the Hessian of the smooth part of the energy: the jump of U or U' at a sharp
cutoff (plain Lennard-Jones) contributes nothing.  New relative to the reference, which has no second derivatives.

elastic_moduli adds the stiffness of the same minimum: the Born term, the affine force field and the non-affine term by
conjugate gradients around the same operator (md_elas_*)."""
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
    the device) and the k^2 N d reorthogonalisation grow quickly.  Thick restart and a stochastic density of states are
    not provided; the elastic moduli of the same minimum are elastic_moduli's (pass it operator=result["operator"])."""
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


def _contract(C, comps, d):
    """(shear, bulk) of a component matrix: the mean over a < b of C_abab, and (1/d^2) sum_ab C_aabb."""
    ix = {c: i for i, c in enumerate(comps)}
    shear = [C[ix[(a, b)], ix[(a, b)]] for a in range(d) for b in range(a + 1, d)]
    bulk = sum(C[ix[(a, a)], ix[(b, b)]] for a in range(d) for b in range(d)) / d ** 2
    return float(np.mean(shear)), float(bulk)


def elastic_moduli(state, params, tol=1e-10, max_iter=None, operator=None):
    """The elastic moduli of the minimum `state` sits in (run fire_minimize first), zero temperature.

    Strain is the Green-Lagrange tensor eta (a separation goes to r'^2 = r^2 + 2 del^T eta del); eta_ab and eta_ba are one
    tensor component and no Voigt or engineering factor appears: the energy change along the relaxed path is
    (V / 2) sum_abcd C_abcd eta_ab eta_cd over all tensor indices.  C = born + nonaffine, with the Born tensor
    (1/V) sum_pairs (U'' - U'/r) / r^2 del_a del_b del_c del_d and the non-affine term -(1/V) Xi_ab H^+ Xi_cd, Xi the affine
    force field d2U / dx d eta; u_ab = -H^+ Xi_ab is the non-affine displacement per unit strain.  The device solves
    H u = -Xi for all components at once by conjugate gradients to |H u + Xi| <= tol |Xi| (max_iter iterations at most,
    default N d).  operator: a valid HessianOperator of this state (e.g. lowest_modes(...)["operator"]) to reuse instead
    of a second upload.

    Returns dict(components (tuples of axes, the order of every array: xx, yy, zz, xy, xz, yz or xx, yy, xy), volume,
    stress (d x d; configurational, tension positive), born, nonaffine, moduli (nc x nc; moduli = born + the symmetric part
    of nonaffine), asymmetry (max |N - N^T|: the solve's error), shear_modulus (the mean over a < b of C_abab),
    bulk_modulus ((1/d^2) sum_ab C_aabb), born_shear_modulus, born_bulk_modulus, displacements (nc, N, d),
    affine_forces (nc, N, d), residuals (the true |H u + Xi| per component), iterations, converged, indefinite, stable
    (converged and not indefinite), operator).

    shear_modulus and bulk_modulus are contractions of this Green-strain tensor, the second derivative of the energy.  The
    moduli that relate the Cauchy stress to a small deformation of a stressed state differ from them by terms linear in
    `stress` (zero at zero pressure), which the caller adds for the convention it needs.  A saddle (indefinite) or
    non-convergence is reported in the flags; nothing is raised for either."""
    if params.potential.device_spec()[0] != "builtin":
        raise ValueError("elastic_moduli needs a built-in potential (user potentials have no second derivative here)")
    if not tol > 0.0:
        raise ValueError("tol must be > 0")
    op = HessianOperator(state, params) if operator is None else operator
    if not isinstance(op, HessianOperator):
        raise ValueError("operator must be a HessianOperator")
    dev, n, d = op.device, op.n, op.dim
    max_iter = n * d if max_iter is None else int(max_iter)
    if max_iter < 1:
        raise ValueError("max_iter must be >= 1")
    comps = tuple(tuple(c) for c in dev.elas_components)
    aff = dev.elas_affine(fields=True)
    sol = dev.elas_solve(tol, max_iter, fields=True)
    stress = np.zeros((d, d))
    for s, (a, b) in enumerate(comps):
        stress[a, b] = stress[b, a] = aff["stress"][s]
    born, N = np.array(aff["born"]), np.array(sol["nonaffine"])
    moduli = born + 0.5 * (N + N.T)
    shear, bulk = _contract(moduli, comps, d)
    bshear, bbulk = _contract(born, comps, d)
    converged, indefinite = bool(sol["converged"]), bool(sol["indefinite"])
    cell = np.asarray(state.unitcell, dtype=np.float64)
    volume = float(np.prod(cell[:d])) if cell.ndim == 1 else float(abs(np.linalg.det(cell[:d, :d])))
    return dict(components=comps, volume=volume, stress=stress, born=born, nonaffine=N, moduli=moduli, asymmetry=float(np.abs(N - N.T).max()),
                shear_modulus=shear, bulk_modulus=bulk, born_shear_modulus=bshear, born_bulk_modulus=bbulk,
                displacements=sol["u"], affine_forces=aff["xi"], residuals=sol["residuals"], iterations=sol["iterations"],
                converged=converged, indefinite=indefinite, stable=converged and not indefinite, operator=op)
