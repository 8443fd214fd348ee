"""run_simulation! -- src/simulation.jl:40-178 (the NVE/NVT method).

The step loop itself runs device-resident inside libmdhip (md_run); this driver only cuts the
run into segments that end on the reference's output steps (step % frequency == 0, 0-based,
so step 0 is always an output step), draws the thermostat's random numbers on the host in the
reference's order, and writes the thermo / trajectory files.
"""
import os
import types

import numpy as np

from . import _lib
from . import analysis as _analysis
from . import io as _io
from .thermostat import draw_bussi
from .types import NVE, NVT, Brownian


def compute_box_volume(unitcell):
    """src/simulation.jl:7-9"""
    return abs(float(np.linalg.det(np.asarray(unitcell))))


def _configure_device(state, params):
    dev = state.system.device
    spec = params.potential.device_spec()
    if spec[0] == "builtin":
        dev.set_potential(spec[1], spec[2])
    elif spec[0] == "source":
        dev.set_potential_source(spec[1], spec[2], spec[3] if len(spec) > 3 else ())
    else:
        raise ValueError("device_spec() must return ('builtin', kind, params) or ('source', src, entry, params)")
    return dev


def run_simulation(state, params, ensemble, total_steps, frequency, pathname, traj_name="trajectory.xyz",
                   thermo_name="thermo.txt", compress=False, log_times=False, write_trajectory=True, rdf=None,
                   dynamics=None, orientational=None, swap=None, barostat=None, shear=None, sq=None, currents=None,
                   stress=None, four_point=None, clusters=None, cage=None, bond_order=None):
    """Python spelling of run_simulation! (mutates `state`, returns None).

    rdf: a RadialDistribution (analysis.py) to sample g(r) into, on the device, at every rdf.every-th output step
    (step % frequency == 0); the counts are added to it at the end and written to pathname/rdf.txt.  Sampling happens
    only where the loop stops anyway and changes nothing else the run produces.

    dynamics: a SelfDynamics (analysis.py) to sample MSD, alpha2, F_s(q, t) and the van Hove function into, on the device,
    at the steps of its schedule (by default the log-time steps `log_times=True` writes snapshots at); the schedule
    restarts at step 0 in every call and the samples accumulate in the object.  At the end it is written to
    pathname/dynamics.txt (and pathname/vanhove.txt when it has bins).  Its stops are added to the loop's output steps;
    nothing else the run produces changes.

    sq: a StructureFactor (analysis.py) to sample S(q) into, on the device, at every sq.every-th output step and, with
    dynamic=True, the coherent F(q, t) at the steps of its schedule (SelfDynamics' rules: the stops are added to the
    loop's output steps, the schedule restarts at step 0 in every call).  Written to pathname/sq.txt and, if dynamic,
    pathname/fqt.txt.  Nothing else the run produces changes.

    currents: a CurrentCorrelations (analysis.py) to sample the longitudinal and transverse current correlations
    C_L(q, t), C_T(q, t) and, with vacf=True, the velocity autocorrelation into, on the device, at the steps of its
    schedule (SelfDynamics' rules: the stops are added to the loop's output steps, the schedule restarts at step 0 in
    every call, the samples accumulate in the object); the equal-time sample is taken at the stops that store an origin.
    Written to pathname/currents.txt (with wave vectors) and pathname/vacf.txt (with vacf).  Not available with Brownian
    dynamics (no velocities).  Nothing else the run produces changes.

    stress: a StressTensor (analysis.py) to sample the pressure tensor and, with nlags > 0, its lag correlations into, on
    the device, at every step that is a multiple of stress.every (the stops are added to the loop's output steps; the step
    counter and the ring of past samples restart in every call, the sums accumulate in the object).  Written to
    pathname/stress.txt and, with nlags > 0, pathname/stress_acf.txt.  Not available with Brownian dynamics (no velocities)
    or a user potential.  Nothing else the run produces changes.

    bond_order: a BondOrder (analysis.py) to sample the local bond-orientational order into (Steinhardt q_l and qbar_l in
    3-D, psi_k in 2-D, the solid-particle count), on the device, at every bond_order.every-th output step, as rdf does.
    Written to pathname/bond_order.txt (the means and the q / qbar histograms) and pathname/bond_order_series.txt (one row
    per sample).  It never evaluates the potential: it works with Brownian dynamics and with user potentials.  Nothing else
    the run produces changes.

    clusters: a ClusterAnalysis (analysis.py) to sample the connected components of the bond graph into (cluster sizes, the
    size distribution, the largest cluster), on the device, at every clusters.every-th output step.  Written to
    pathname/clusters.txt (the means and n(s)) and pathname/clusters_series.txt (one row per sample).  With
    members="solid" the members are the solid particles of bond_order's sample of the same step: bond_order= is required
    and clusters.every must be a multiple of bond_order.every.  It never evaluates the potential.  Nothing else the run
    produces changes.

    cage: a CageDynamics (analysis.py) to sample the cage-relative MSD, alpha2 and F_s(q, t) -- displacements relative to
    the mean displacement of the neighbours a particle had at the time origin -- and the bond-breaking correlation C_B(t)
    into, on the device, at the steps of its schedule (SelfDynamics' rules: the stops are added to the loop's output
    steps, the schedule restarts at step 0 in every call, the samples accumulate in the object).  Written to
    pathname/cage.txt.  It never evaluates the potential: it works with Brownian dynamics and with user potentials.  More
    neighbours than cage.max_neighbours at an origin is an error at the end of the run.  Nothing else the run produces
    changes.

    four_point: a FourPoint (analysis.py) to sample the self overlap Q(t), the four-point susceptibility chi4(t) and, if it
    has wave vectors, the structure factor S4(q, t) of the slow particles into, on the device, at the steps of its
    schedule (SelfDynamics' rules: the stops are added to the loop's output steps, the schedule restarts at step 0 in
    every call, the samples accumulate in the object).  Written to pathname/chi4.txt and, with vectors, pathname/s4.txt.
    It never evaluates the potential.  Nothing else the run produces changes.

    orientational: an OrientationalCorrelation (analysis.py) to sample the orientational correlation function into --
    G_l(r) of q_lm in 3-D, g6(r) of psi_6 in 2-D -- on the device, at every orientational.every-th output step.  Its
    marks are bond_order's sample of the same step: bond_order= is required and orientational.every must be a multiple of
    bond_order.every.  Written to pathname/orient_corr.txt.  It never evaluates the potential.  Nothing else the run
    produces changes.

    swap: a SwapMonteCarlo (montecarlo.py): after every swap.every-th step, swap.rounds rounds of diameter exchanges on
    the device at the ensemble's target temperature of that step (or swap.ktemp), then the MD goes on from the new
    diameters and forces.  Unlike the samplers it CHANGES the run.  Its stops are added to the loop's output steps; at a
    step it shares with samplers it acts after all of them, so they see the frame the MD produced; a trajectory frame or
    snapshot of that step carries the diameters after the block.  The round counter continues across blocks (and calls
    with the same object).  After each block state.diameters is refreshed, so frames and final.xyz carry the diameters of
    their moment.  Written to pathname/swap.txt.  Not available with a user potential.  With swap=None nothing the run
    produces changes.

    barostat: a StochasticCellRescaling (barostat.py): after every barostat.every-th step one coupling to its pressure --
    the cell and the positions are scaled by mu, the velocities by 1 / mu, on the device (md_scale_cell, which keeps the
    neighbour rows), at the ensemble's target temperature of that step (or barostat.ktemp), and the forces are evaluated
    in the new cell.  Like swap it CHANGES the run.  Its stops are added to the loop's output steps; at a step it shares it
    acts after every sampler and after swap, before the thermo line and the frame export of that step, which therefore
    show the scaled frame.  state.unitcell and state.system.unitcell follow every coupling; the thermo line's density is
    n / V of the moment; every frame, snapshot and final.xyz carries the cell of its moment.  `params` is not touched
    (params.rho is the caller's to keep consistent, as with set_unitcell).  Written to pathname/barostat.txt.  Not
    available with Brownian dynamics.  Refused up front, before any file is opened, together with the samplers that
    belong to one cell: dynamics=, sq=, currents=, four_point= and cage= store time origins or wave vectors of the cell
    they were set up in (md_scale_cell refuses them on the device), and rdf=, stress= and orientational= normalise their
    sums with one volume, which a run whose volume moves does not have.  bond_order=, clusters= and swap= go with it.
    With barostat=None nothing the run produces changes.

    shear: a ShearFlow (deformation.py): after every shear.every-th step the flow operator of SLLOD for the elapsed time --
    the cell becomes F U, positions F x, velocities F^-1 v with F the simple shear of rate * every * dt, on the device
    (md_deform_cell, which keeps the neighbour rows) -- a lattice flip of the cell when it is due, and the forces of the
    new cell.  The velocities the run holds, exports and thermostats are peculiar velocities.  The splitting is first
    order in rate * every * dt (every=1: the plain one-step splitting).  Like swap and barostat it CHANGES the run; its
    stops are added to the loop's output steps and it acts where the barostat acts: after every sampler and after swap,
    before the thermo line and the frame export of that step.  state.unitcell and state.system.unitcell follow; every
    frame, snapshot and final.xyz carries the cell of its moment.  Written to pathname/shear.txt.  Refused up front,
    before any file is opened: Brownian dynamics; barostat=; stress= (one handle has one set of md_stress_ sums and the
    shear reads its stress through them; sharing them is left for later); dynamics=, sq=, currents=, four_point= and
    cage=, which are bound to the cell they were set up in.  rdf=, bond_order=, clusters=, orientational= and swap= go
    with it: the volume is constant.  With shear=None nothing the run produces changes."""
    if shear is not None:
        if isinstance(ensemble, Brownian):
            raise ValueError("shear= is not available with Brownian dynamics (no velocities: SLLOD maps peculiar velocities)")
        if barostat is not None:
            raise ValueError("shear= cannot be combined with barostat=: both own the cell of the run")
        if stress is not None:
            raise ValueError("shear= cannot be combined with stress=: one handle has one set of md_stress_ sums and the "
                             "shear reads its stress through them; sharing them is left for later")
        for name, smp in dict(dynamics=dynamics, sq=sq, currents=currents, four_point=four_point, cage=cage).items():
            if smp is not None:
                raise ValueError("shear= cannot be combined with %s=: its stored time origins or wave vectors belong to "
                                 "the cell it is set up in, and the shear changes the cell" % name)
    if barostat is not None:
        one_cell = dict(dynamics=dynamics, sq=sq, currents=currents, four_point=four_point, cage=cage)
        one_volume = dict(rdf=rdf, stress=stress, orientational=orientational)
        for name, smp in one_cell.items():
            if smp is not None:
                raise ValueError("barostat= cannot be combined with %s=: its stored time origins or wave vectors belong to "
                                 "the cell it is set up in, and the barostat changes the cell" % name)
        for name, smp in one_volume.items():
            if smp is not None:
                raise ValueError("barostat= cannot be combined with %s=: it normalises its sums with one volume, and the "
                                 "barostat changes the volume during the run" % name)
    if clusters is not None and clusters.members == "solid":
        if bond_order is None:
            raise ValueError('clusters with members="solid" needs bond_order= in the same run')
        if clusters.every % bond_order.every != 0:
            raise ValueError("clusters.every must be a multiple of bond_order.every: every cluster sample needs the "
                             "bond-order sample of its step")
    brownian = isinstance(ensemble, Brownian)
    os.makedirs(pathname, exist_ok=True)
    trajectory_file, thermo_file = _io.open_files(pathname, traj_name, thermo_name)
    with open(thermo_file, "a") as io:
        io.write("# Step Energy Temperature Pressure\n")

    dev = _configure_device(state, params)
    dim = state.dimension
    n = params.n_particles
    pot = params.potential
    volume = compute_box_volume(state.unitcell)
    if not brownian and (state.velocities is None or len(state.velocities) != n):
        raise ValueError("state.velocities must be set before run_simulation (README.md:39-41)")
    # the host-side state is the truth at entry, exactly as in the reference
    dev.upload(x=state.system.positions, v=None if brownian else state.velocities,
               f=state.system.energy_and_forces.forces, images=state.images, diameters=state.diameters)
    # Brownian method (src/simulation.jl:181-308): the device's noise stream is keyed by one draw of state.rng;
    # the virial is sampled every 10th step and averaged at the output steps (:253-266)
    brown_seed = int(state.rng.integers(1 << 63)) if brownian else 0
    # the samplers (analysis.py's protocol), in the order their device calls are made at a step they share
    # (clusters after bond_order: with members="solid" it reads the bond-order frame of the same step; then cage;
    # four_point; currents right after sq; orientational last: it reads the bond-order frame of the same step)
    samplers = [s for s in (rdf, dynamics, sq, stress, bond_order) + (clusters, cage, four_point) if s is not None]
    if currents is not None:
        samplers.insert(sum(s is not None for s in (rdf, dynamics, sq)), currents)
    if orientational is not None:
        samplers.append(orientational)
    run = types.SimpleNamespace(total_steps=total_steps, frequency=frequency, n=n, dim=dim, dt=params.dt,
                                unitcell=state.unitcell, brownian=brownian, bond_order=bond_order, ensemble=ensemble,
                                rng=state.rng, potential=pot)
    for s in samplers:
        s._begin(dev, run)
    if swap is not None:
        swap._begin(dev, run)
    if barostat is not None:
        barostat._begin(dev, run)
    if shear is not None:
        shear._begin(dev, run)
    vir_acc = [0.0, 0.0]

    nvt = isinstance(ensemble, NVT)
    ens_kind = _lib.MD_NVT if nvt else _lib.MD_NVE
    tau = ensemble.tau if nvt else 0.0

    def segment(first_step, nsteps):
        if brownian:
            r = dev.run_brownian(nsteps, params.dt, ensemble.ktemp, brown_seed, first_step=first_step, virial_every=10)
            vir_acc[0] += r["virial_sum"]
            vir_acc[1] += r["virial_count"]
            return r["U"], r["W"], 0.0
        kt = r1 = r2 = None
        if nvt:
            # ensemble_step! receives step+1 (src/simulation.jl:108)
            kt = np.array([ensemble.ktemp(s + 1) for s in range(first_step, first_step + nsteps)], dtype=np.float64)
            r1, r2 = draw_bussi(state.nf, state.rng, nsteps)
        return dev.run(nsteps, params.dt, ens_kind, tau, state.nf, kt, r1, r2, thermo=True)

    # log-spaced snapshots (src/simulation.jl:80-87,153-171): step 0 plus generate_log_times()
    snapshot_times = [0] + _io.generate_log_times() if log_times else []
    writer = _io.AsyncWriter()      # frames are formatted and written while the next segment runs
    # A frame is exported asynchronously (md_snapshot_begin: gather + copy to pinned memory on a copy stream) and collected
    # AFTER the next segment has been run: the device-to-host copy overlaps that segment, the formatting and the file
    # write overlap the one after (writer thread).  `pending` = where the frame in flight goes.
    pending = []

    def collect():
        if pending:
            x, img = dev.snapshot_end()
            for path, at, mode, diam, cell in pending:      # (the cell of the frame's own moment: a barostat moves it)
                writer.submit(_io.write_to_file_lammps, path, at, cell, n, x, img, diam, dim, mode=mode)
            pending.clear()

    step = 0
    while step < total_steps:
        # run up to and including the next output step (thermo / trajectory cadence, a snapshot time or a sampler's stop)
        stops = [-(-step // frequency) * frequency, _analysis._next_stop(snapshot_times, step)]
        stops += [s._next(step) for s in samplers]
        if swap is not None:
            stops.append(swap._next(step))
        if barostat is not None:
            stops.append(barostat._next(step))
        if shear is not None:
            stops.append(shear._next(step))
        last = min(min(t for t in stops if t is not None), total_steps - 1)
        U, W, K = segment(step, last - step + 1)
        collect()                       # the frame exported before this segment: its copy had the whole segment to finish
        step = last + 1
        for s in samplers:
            if s._next(last) == last:
                s._act(dev, last)
        if swap is not None and swap._next(last) == last:
            # after every sampler: they saw the frame the MD produced.  A block replaces state.diameters by a new array
            # (never in place: a frame in flight keeps the diameters of its own moment)
            r = swap._act(dev, last)
            state.diameters = dev.diameters()
            U, W = r["U"], r["W"]
        if barostat is not None and barostat._next(last) == last:
            # after every sampler and after swap; no frame is in flight (collect() above).  The cell is replaced by a new
            # array (never in place: a frame queued earlier keeps the cell of its own moment)
            r = barostat._act(dev, last, U, W, K, volume)
            state.unitcell = r["mu"] * np.asarray(state.unitcell, dtype=np.float64)
            state.system.unitcell = state.unitcell
            volume = compute_box_volume(state.unitcell)
            barostat._record(r, volume)
            U, W, K = r["U"], r["W"], r["K"]
        if shear is not None and shear._next(last) == last:
            # where the barostat acts (the two exclude each other); the cell is replaced by a new array, never in place
            r = shear._act(dev, last, U, W, K, volume)
            state.unitcell = r["cell"]
            state.system.unitcell = state.unitcell
            volume = compute_box_volume(state.unitcell)
            U, W, K = r["U"], r["W"], r["K"]
        want_frame = False
        if last % frequency == 0:
            if brownian:
                temperature = ensemble.ktemp                            # src/simulation.jl:259-266
                total_energy = U / n
                pressure = vir_acc[0] / (dim * max(vir_acc[1], 1.0) * volume) + params.rho * ensemble.ktemp
                vir_acc[0] = vir_acc[1] = 0.0
            else:
                temperature = 2.0 * K / state.nf
                total_energy = (U + pot.energy_lrc(n, volume)) / n      # src/simulation.jl:120-124
                rho = params.rho if barostat is None else n / volume
                pressure = W / (dim * volume) + rho * temperature       # :128-129
                pressure += pot.pressure_lrc(n, volume)                 # :131
            with open(thermo_file, "a") as io:
                io.write("%d %.6f %.6f %.6f\n" % (last, total_energy, temperature, pressure))
            state.system.energy_and_forces.energy = U
            state.system.energy_and_forces.virial = W
            if write_trajectory:
                pending.append((trajectory_file, last, "a", state.diameters, state.unitcell))
                want_frame = True
        if _analysis._next_stop(snapshot_times, last) == last:
            pending.append((os.path.join(pathname, f"snapshot.{last}"), last, "w", state.diameters, state.unitcell))
            want_frame = True
        if want_frame:
            dev.snapshot_begin()

    collect()
    writer.close()
    x, v, f, img = dev.download()
    state.system.positions = x
    state.system.xpositions = x
    if not brownian:
        state.velocities = v
    state.images = img
    state.system.energy_and_forces.forces = f
    # finalize_simulation!: src/simulation.jl:11-36
    _io.write_to_file(os.path.join(pathname, "final.xyz"), total_steps, state.unitcell, n, x, state.diameters, dim,
                      mode="w")
    for s in samplers:
        s._finish(dev, run, pathname)
    if swap is not None:
        swap._finish(dev, run, pathname)
    if barostat is not None:
        barostat._finish(dev, run, pathname)
    if shear is not None:
        shear._finish(dev, run, pathname)
    if compress and os.path.isfile(trajectory_file):
        _io.compress_zstd(trajectory_file)
    return None
