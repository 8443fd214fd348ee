"""Deformation of a live sample: cell changes in place (md_set_cell), lattice reduction of a sheared cell, the non-affine
displacement since a mark (md_nonaffine_*), the athermal quasi-static (AQS) strain loop on top of the device's FIRE, and
shear flow at a finite rate and temperature (ShearFlow: SLLOD on md_deform_cell).
New relative to the reference, which fixes the unit cell at initialisation.

Conventions.  The unit cell U is d x d with the lattice vectors in its COLUMNS (src/initialization.jl:7-18); a deformation
gradient F acts from the left, U' = F U, and an affine change keeps every particle's fractional coordinates.  Like the
reference, nothing here touches `params`: after a change of volume params.ρ is the caller's to keep consistent.
"""
import os

import numpy as np

from . import _lib
from .analysis import _next_multiple
from .simulation import _configure_device

_REDUCE_MAX_SWEEPS = 64


def _plane(d, plane):
    a, b = int(plane[0]), int(plane[1])
    if not (0 <= a < d and 0 <= b < d and a != b):
        raise ValueError(f"plane must name two different axes below {d}, got {plane}")
    return a, b


def simple_shear(d, gamma, plane=(0, 1)):
    """F = 1 + gamma e_a e_b^T for plane = (a, b): x_a grows by gamma x_b; volume preserving."""
    a, b = _plane(d, plane)
    F = np.eye(d)
    F[a, b] = float(gamma)
    return F


def pure_shear(d, eps, plane=(0, 1)):
    """F = diag(..., 1 + eps, ..., 1 / (1 + eps), ...) on the axes of plane = (a, b); volume preserving."""
    a, b = _plane(d, plane)
    if not 1.0 + eps > 0.0:
        raise ValueError("eps must be > -1")
    F = np.eye(d)
    F[a, a] = 1.0 + float(eps)
    F[b, b] = 1.0 / (1.0 + float(eps))
    return F


def volumetric(d, eps):
    """F = (1 + eps) 1: every length grows by 1 + eps, the volume by (1 + eps)^d."""
    if not 1.0 + eps > 0.0:
        raise ValueError("eps must be > -1")
    return np.eye(d) * (1.0 + float(eps))


def _cell_of(state):
    d = state.dimension
    U = np.asarray(state.unitcell, dtype=np.float64)
    return np.diag(U[:d]) if U.ndim == 1 else np.array(U[:d, :d])


def _face_distances(U):
    inv = np.linalg.inv(U)
    return 1.0 / np.sqrt((inv * inv).sum(axis=1))


def _device_set_cell(state, U, mode):
    """The device call alone: the handle's cell and frame change, the host copies of the frame do not."""
    state.system.device.set_cell(U, mode)
    state.unitcell = np.array(U)
    state.system.unitcell = state.unitcell


def _download_frame(state):
    x, _, f, img = state.system.device.download()
    state.system.positions[:] = x
    state.system.energy_and_forces.forces[:] = f
    state.images[:] = img


def set_unitcell(state, params, unitcell, remap="affine", upload=True):
    """Give the live sample the cell `unitcell` (d x d, columns = lattice vectors; or d lengths).

    remap="affine": fractional coordinates are kept -- every particle moves with the cell; remap="lattice": Cartesian
    positions are kept and `unitcell` must generate the same lattice (U_old^-1 U_new integer with determinant +-1).
    upload=True sends the host frame (positions, images, diameters) first, as fire_minimize does: the host state is the
    truth at entry (this discards a mark of nonaffine_mark); upload=False works on the frame the device holds.  Updates
    state.unitcell and the host copies of positions and images; the device handle stays the same object; forces are
    those of the old cell until the next evaluation.  `params` is not touched: params.ρ is the caller's to keep
    consistent after a change of volume, the reference's own convention.  A refusal (MdhipError) changes nothing."""
    if remap not in ("affine", "lattice"):
        raise ValueError("remap must be 'affine' or 'lattice'")
    d = state.dimension
    U = np.asarray(unitcell, dtype=np.float64)
    U = np.diag(U[:d]) if U.ndim == 1 else np.array(U[:d, :d])
    dev = _configure_device(state, params)
    if upload:
        dev.upload(x=state.system.positions, images=state.images, diameters=state.diameters)
    _device_set_cell(state, U, _lib.MD_CELL_AFFINE if remap == "affine" else _lib.MD_CELL_LATTICE)
    x, _, _, img = dev.download()
    state.system.positions[:] = x
    state.images[:] = img


def deform(state, params, F, upload=True):
    """Apply the deformation gradient F affinely: the cell becomes F @ unitcell, fractional coordinates are kept."""
    F = np.asarray(F, dtype=np.float64)
    d = state.dimension
    if F.shape != (d, d):
        raise ValueError(f"F must have shape ({d}, {d})")
    set_unitcell(state, params, F @ _cell_of(state), remap="affine", upload=upload)


def gauss_reduce(U):
    """Pairwise Gauss reduction of the lattice vectors (columns of U): u_b <- u_b - round(u_b.u_a / u_a.u_a) u_a over the
    ordered pairs (a, b) until nothing changes.  A step that would make any face distance smaller is not taken (in 2-D
    none does; in 3-D shortening u_b can lengthen u_b x u_c).  Returns (U @ M, M) with M integer and det M = +-1."""
    U = np.array(U, dtype=np.float64)
    d = U.shape[0]
    M = np.eye(d, dtype=np.int64)
    W = U.copy()
    for _ in range(_REDUCE_MAX_SWEEPS):
        changed = False
        for a in range(d):
            for b in range(d):
                if a == b:
                    continue
                k = int(np.rint(np.dot(W[:, b], W[:, a]) / np.dot(W[:, a], W[:, a])))
                if k == 0:
                    continue
                M2 = M.copy()
                M2[:, b] -= k * M2[:, a]
                W2 = U @ M2.astype(np.float64)
                if np.any(_face_distances(W2) < _face_distances(W) * (1.0 - 1e-12)):
                    continue
                M, W, changed = M2, W2, True
        if not changed:
            break
    return W, M


def reduce_cell(state, params, upload=True):
    """Replace a sheared cell by the reduced cell of the same lattice (gauss_reduce), particles where they are
    (set_unitcell(..., remap="lattice")).  For a simply sheared orthorhombic box this is the usual flip by one lattice
    vector once the tilt passes half a box length, so strains beyond 1/2 never meet the face-distance refusal.  Returns
    the integer matrix M (new cell = old cell @ M), or None when the cell is reduced already."""
    W, M = gauss_reduce(_cell_of(state))
    if np.array_equal(M, np.eye(state.dimension, dtype=np.int64)):
        return None
    set_unitcell(state, params, W, remap="lattice", upload=upload)
    return M


AQS_MODES = ("simple", "pure", "volumetric")


def _gradient(mode, d, step, plane):
    if mode == "simple":
        return simple_shear(d, step, plane)
    if mode == "pure":
        return pure_shear(d, step, plane)
    if mode == "volumetric":
        return volumetric(d, step)
    raise ValueError(f"mode must be one of {AQS_MODES}")


def aqs_columns(d):
    """The column names of aqs.txt, in order."""
    names = "xyz"
    comps = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)) if d == 3 else ((0, 0), (1, 1), (0, 1))
    return (["step", "strain", "energy"] + ["stress_" + names[a] + names[b] for a, b in comps] +
            ["pressure", "fire_steps", "converged", "d2_nonaffine", "participation", "max_u", "flips"])


def athermal_quasistatic_shear(state, params, pathname, strain_step, nsteps, mode="simple", plane=(0, 1), tol=1e-9,
                               reduce=True, mark="previous", on_step=None, **fire_kwargs):
    """Athermal quasi-static deformation: nsteps increments of (strain, minimise) on one device handle.

    Per increment: the cell becomes F(strain_step) @ cell affinely (mode "simple": simple_shear, "pure": pure_shear,
    "volumetric": volumetric; the increments compose, so simple shear adds up and the stretches of the other two
    compound); with reduce=True the cell is reduced (reduce_cell) when it can be; the frame is marked (mark="previous":
    at every increment after the strain, so u is the non-affine displacement of this increment; mark="start": once,
    before the first one, so u accumulates); the device's FIRE relaxes to `tol` (fire_kwargs: max_steps, dt_initial,
    dt_max, alpha0, f_inc, f_dec, nmin of MDDevice.fire_minimize); then the stress, the energy and the non-affine sums are
    read.  The frame never goes to the host inside the loop; at the end it is downloaded once into `state`.  The host frame
    is uploaded once at entry.  The loop reads the stress through the handle's pressure-tensor sampler and sets it up
    afresh (md_stress_setup with no lags): a StressTensor setup the handle carried, its lag ring and its running sums, is
    discarded -- read it out before calling this.

    Writes pathname/aqs.txt with the columns aqs_columns(d): step (1-based), strain (step x strain_step), energy per
    particle, the configurational stress in elastic_moduli's components, order, sign and normalisation (tension positive,
    per unit volume), pressure (-trace(stress) / d), fire_steps, converged (1 / 0), d2_nonaffine (sum |u|^2 / N),
    participation ((sum |u|^2)^2 / (N sum |u|^4); 0 when nothing moved), max_u (the largest |u|), flips (cell reductions
    at this increment).  An increment whose FIRE does not converge is recorded with converged = 0 and the run goes on;
    nothing is raised, like elastic_moduli's flags.  on_step(row: dict), if given, is called after every increment.
    Returns dict(column name -> array)."""
    if mark not in ("previous", "start"):
        raise ValueError("mark must be 'previous' or 'start'")
    if mode not in AQS_MODES:
        raise ValueError(f"mode must be one of {AQS_MODES}")
    nsteps = int(nsteps)
    if nsteps < 1:
        raise ValueError("nsteps must be >= 1")
    if not tol > 0.0:
        raise ValueError("tol must be > 0")
    d = state.dimension
    n = state.system.positions.shape[0]
    F = _gradient(mode, d, float(strain_step), plane)
    dev = _configure_device(state, params)
    dev.upload(x=state.system.positions, f=state.system.energy_and_forces.forces, images=state.images,
               diameters=state.diameters)
    dev.stress_setup(0)
    comps = dev.elas_components
    names = aqs_columns(d)
    rows = []
    if mark == "start":
        dev.nonaffine_mark()
    for k in range(1, nsteps + 1):
        _device_set_cell(state, F @ _cell_of(state), _lib.MD_CELL_AFFINE)
        flips = 0
        if reduce:
            W, M = gauss_reduce(_cell_of(state))
            if not np.array_equal(M, np.eye(d, dtype=np.int64)):
                _device_set_cell(state, W, _lib.MD_CELL_LATTICE)
                flips = 1
        if mark == "previous":
            dev.nonaffine_mark()
        r = dev.fire_minimize(tol=tol, **fire_kwargs)
        dev.stress_sample()
        _, vir = dev.stress_tensor()
        volume = abs(float(np.linalg.det(_cell_of(state))))
        stress = -vir / volume
        na = dev.nonaffine()
        s2, s4 = na["sum_u2"], na["sum_u4"]
        row = [k, k * float(strain_step), r["energy"] / n] + list(stress) + [
            -sum(stress[i] for i, (a, b) in enumerate(comps) if a == b) / d, r["steps"], 1 if r["converged"] else 0,
            s2 / n, (s2 * s2 / (n * s4)) if s4 > 0.0 else 0.0, float(np.sqrt(na["max_u2"])), flips]
        rows.append(row)
        if on_step is not None:
            on_step(dict(zip(names, row)))
    _download_frame(state)
    state.system.energy_and_forces.energy = rows[-1][2] * n
    table = np.array(rows, dtype=np.float64)
    os.makedirs(pathname, exist_ok=True)
    with open(os.path.join(pathname, "aqs.txt"), "w") as fh:
        fh.write("# " + " ".join(names) + "\n")
        for row in rows:
            fh.write(" ".join(("%d" % v) if isinstance(v, (int, np.integer)) else ("%.17g" % v) for v in row) + "\n")
    out = {name: table[:, i] for i, name in enumerate(names)}
    for name in ("step", "fire_steps", "converged", "flips"):
        out[name] = out[name].astype(np.int64)
    return out


def shear_columns():
    """The column names of shear.txt, in order."""
    return ["step", "strain", "tilt", "sigma_ab", "pressure", "K_ab", "rows_kept", "flips"]


def shear_flow_update(cell, rate, dt_flow, plane):
    """The pure part of one application of the flow operator: (F, G, F U) for the elapsed time dt_flow.
    F = simple_shear(d, rate dt_flow, plane); G = F^-1 = 1 - rate dt_flow e_a e_b^T, exact for simple shear; F U in the
    device's arithmetic (row times column, left to right, every product and sum rounded)."""
    U = np.asarray(cell, dtype=np.float64)
    d = U.shape[0]
    dgamma = float(rate) * float(dt_flow)
    F = simple_shear(d, dgamma, plane)
    G = simple_shear(d, -dgamma, plane)
    new = F[:, 0:1] * U[0:1, :] + F[:, 1:2] * U[1:2, :]
    if d == 3:
        new = new + F[:, 2:3] * U[2:3, :]
    return F, G, new


class ShearFlow:
    """Homogeneous simple shear at the rate `rate` (strain per unit time) in plane = (a, b) -- the streaming velocity is
    u_a = rate x_b -- by the SLLOD equations of motion in a deforming cell, on the device's md_deform_cell (DESIGN.md
    section 27).  New relative to the reference, which fixes its cell at initialisation.

    After every `every`-th MD step the flow operator is applied for the elapsed time Dt = every dt: with
    F = simple_shear(d, rate Dt, plane) the cell becomes F U, every position F x and every velocity F^-1 v, in one device
    pass that keeps the neighbour rows; then the forces are evaluated in the new cell.  The velocities the handle stores
    are therefore PECULIAR velocities (relative to the streaming motion); the thermostat of the MD step acts on them, which
    is what SLLOD asks for; the ordinary drift x += v dt plus the flow operator is the streaming motion.  With flip=True
    the sheared cell is replaced by the reduced cell of the same lattice when reduce_cell's rule says so (once per half
    box length of strain; particles stay where they are, velocities need no change, the neighbour lists are rebuilt).

    This is the Lie splitting exp(L_md Dt) exp(L_flow Dt) of the SLLOD propagator: its error is FIRST ORDER in
    rate * every * dt.  every=1 is the plain one-step splitting; a larger `every` trades accuracy in the rate for fewer
    force evaluations.

    Stress: at every stress_every-th coupling, BEFORE the flow is applied, the stress tensor of the moment is read through
    the handle's md_stress_ sums (set up afresh at the start of the run, as athermal_quasistatic_shear does):
    sigma = -(sum v v + sum (f/r) del del) / V, aqs.txt's sign and normalisation (tension positive, per unit volume) plus
    the kinetic part.  Couplings without a reading record nan.

    Fields, accumulated over the runs until reset(): records (one dict per coupling, the columns of shear.txt: step,
    strain -- the accumulated rate * time, monotone across flips --, tilt -- the entry U[a, b] of the cell after the
    coupling --, sigma_ab, pressure = -trace(sigma) / d, K_ab -- the kinetic part -sum v_a v_b / V of sigma_ab --,
    rows_kept, flips), strain, n_stress, sum_sigma; mean_stress(), viscosity() = <sigma_ab> / rate."""

    def __init__(self, rate, every=10, plane=(0, 1), stress_every=1, flip=True):
        rate, every, stress_every = float(rate), int(every), int(stress_every)
        if not np.isfinite(rate):
            raise ValueError("rate must be finite")
        if every < 1:
            raise ValueError("every must be >= 1")
        if stress_every < 1:
            raise ValueError("stress_every must be >= 1")
        a, b = int(plane[0]), int(plane[1])
        if a == b or a < 0 or b < 0:
            raise ValueError(f"plane must name two different axes, got {plane}")
        self.rate, self.every, self.plane, self.stress_every, self.flip = rate, every, (a, b), stress_every, bool(flip)
        self.reset()

    def reset(self):
        self.records = []
        self.strain = 0.0
        self.n_couplings = 0
        self.n_stress = 0
        self.sum_sigma = 0.0

    def mean_stress(self):
        return self.sum_sigma / self.n_stress if self.n_stress else float("nan")

    def viscosity(self):
        return self.mean_stress() / self.rate if self.rate != 0.0 else float("nan")

    def write(self, path):
        with open(path, "w") as io:
            io.write("# " + " ".join(shear_columns()) + "\n")
            for c in self.records[self._first:]:
                io.write("%d %.17g %.17g %.17g %.17g %.17g %d %d\n" % (c["step"], c["strain"], c["tilt"], c["sigma_ab"],
                                                                      c["pressure"], c["K_ab"], c["rows_kept"], c["flips"]))

    # -- run_simulation's protocol: one application of the flow operator after every `every`-th step -----------------------
    def _begin(self, dev, run):
        if run.brownian:
            raise ValueError("shear= is not available with Brownian dynamics (no velocities: SLLOD maps peculiar velocities)")
        self._dim = run.dim
        _plane(self._dim, self.plane)
        self._total_steps = run.total_steps
        self._dt_flow = self.every * run.dt
        self._first = len(self.records)
        dev.stress_setup(0)
        a, b = min(self.plane), max(self.plane)
        self._comp = list(dev.elas_components).index((a, b))
        self._diag = [i for i, (p, q) in enumerate(dev.elas_components) if p == q]

    def _next(self, step):
        s = _next_multiple(step + 1, self.every, self._total_steps + 1)
        return None if s is None else s - 1

    def _act(self, dev, step, U, W, K, volume):
        """One application on the frame the segment (or the swap block) left: returns dict(step, cell, U, W, K, rows_kept,
        flips, ...) with the cell after the flow (and the flip), U, W of that cell and K of the mapped velocities."""
        d = self._dim
        a, b = self.plane
        sigma = pressure = k_ab = float("nan")
        if self.n_couplings % self.stress_every == 0:
            dev.stress_sample()
            kin, vir = dev.stress_tensor()
            st = -(kin + vir) / volume
            sigma, k_ab = float(st[self._comp]), float(-kin[self._comp] / volume)
            pressure = -float(sum(st[i] for i in self._diag)) / d
            self.n_stress += 1
            self.sum_sigma += sigma
        F, G, _ = shear_flow_update(dev.unitcell, self.rate, self._dt_flow, self.plane)
        kept = dev.deform_cell(F, G)
        flips = 0
        if self.flip:
            Wc, M = gauss_reduce(dev.unitcell)
            if not np.array_equal(M, np.eye(d, dtype=np.int64)):
                dev.set_cell(Wc, _lib.MD_CELL_LATTICE)
                flips = 1
        U, W = dev.compute_forces()                         # the next half-kick needs the new cell's forces
        K = dev.kinetic()
        self.n_couplings += 1
        self.strain += self.rate * self._dt_flow
        cell = np.array(dev.unitcell)
        rec = dict(step=step, strain=self.strain, tilt=float(cell[a, b]), sigma_ab=sigma, pressure=pressure, K_ab=k_ab,
                   rows_kept=int(kept), flips=flips)
        self.records.append(rec)
        return dict(rec, cell=cell, U=U, W=W, K=K)

    def _finish(self, dev, run, pathname):
        self.write(os.path.join(pathname, "shear.txt"))
