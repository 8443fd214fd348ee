"""Structure and dynamics of a simulated configuration, sampled on the device: the radial distribution function g(r),
the self dynamics (MSD, F_s(q, t), van Hove), the collective side (density modes, S(q), coherent F(q, t)), the stress
(pressure tensor, stress autocorrelations, Green-Kubo viscosity), the bond-orientational order (Steinhardt q_l, the
neighbour-averaged qbar_l, psi_k in 2-D, the solid-particle count) and the clusters (connected components of the bond
graph: sizes, the size distribution, the largest -- solid -- cluster), the cage-relative dynamics (displacements
relative to the origin neighbours' mean, the bond-breaking correlation C_B), the four-point functions of the self
overlap (chi4(t), S4(q, t)), the currents (C_L(q, t), C_T(q, t), the velocity autocorrelation) and the marked pair
correlations (the orientational correlation g6(r) / G_l(r), the spatial correlation of any per-particle field).

The pair histogram itself is accumulated by libmdhip (md_rdf_*: integer counts, exact and independent of the order the
pairs are visited in); this module keeps the samples, normalises them and writes them out.
"""
import bisect
import math
import os

import numpy as np


# ---------------------------------------------------------------------------------------------------------------------
# The sampler protocol.  run_simulation drives every sampler class of this module through four private methods:
#   _begin(dev, run)            set the sampler up on the device and derive what it needs for this run; `run` carries
#                               total_steps, frequency, n, dim, dt, unitcell, brownian, bond_order (the run's
#                               BondOrder or None), ensemble and rng (the state's generator; montecarlo.py uses both)
#   _next(step)                 the first step >= `step` at which the sampler acts in this run, or None
#   _act(dev, step)             the device calls of that step
#   _finish(dev, run, pathname) read back, accumulate into the object, write the files

def _next_multiple(step, period, total_steps):
    """The first multiple of `period` that is >= step, or None when the run ends before it."""
    s = -(-step // period) * period
    return s if s < total_steps else None


def _next_stop(stops, step):
    """The first entry >= step of the sorted list `stops`, or None."""
    i = bisect.bisect_left(stops, step)
    return stops[i] if i < len(stops) else None


def shell_volumes(edges, dimension):
    """Volumes (3-D) or areas (2-D) of the shells between consecutive radii of `edges`."""
    e = edges
    if dimension == 3:
        return 4.0 * math.pi / 3.0 * (e[1:] ** 3 - e[:-1] ** 3)
    return math.pi * (e[1:] ** 2 - e[:-1] ** 2)


class RadialDistribution:
    """g(r) on `nbins` bins of width r_max / nbins, accumulated over samples until reset().

    Fields: edges (nbins + 1 radii), r (bin centres), counts (unordered pair counts summed over the samples), nsamples.
    Passed to run_simulation(..., rdf=...), it takes a sample at every `every`-th output step."""

    def __init__(self, r_max, nbins, every=1):
        r_max, nbins, every = float(r_max), int(nbins), int(every)
        if not (r_max > 0.0 and math.isfinite(r_max)):
            raise ValueError("r_max must be finite and > 0")
        if not 1 <= nbins <= 8192:
            raise ValueError("nbins must be in 1..8192")
        if every < 1:
            raise ValueError("every must be >= 1")
        self.r_max, self.nbins, self.every = r_max, nbins, every
        delta = r_max / nbins
        # the same edges the device bins on: e2[k] = (k delta)^2
        self.edges = np.arange(nbins + 1, dtype=np.float64) * delta
        self.r = 0.5 * (self.edges[:-1] + self.edges[1:])
        self.counts = np.zeros(nbins, dtype=np.int64)
        self.nsamples = 0
        self.n_particles = 0
        self.volume = 0.0
        self.dimension = 3

    def reset(self):
        self.counts[:] = 0
        self.nsamples = 0

    def _accumulate(self, counts, nsamples, n_particles, unitcell):
        self.counts += np.asarray(counts, dtype=np.int64)
        self.nsamples += int(nsamples)
        u = np.asarray(unitcell, dtype=np.float64)
        self.n_particles = int(n_particles)
        self.volume = abs(float(np.linalg.det(u)))
        self.dimension = u.shape[0]

    def shell_volumes(self, dimension=None):
        return shell_volumes(self.edges, self.dimension if dimension is None else dimension)

    def g(self):
        """g_k = counts_k / (nsamples * N (N - 1) / (2 V) * V_k): 1 for an ideal gas."""
        if self.nsamples == 0 or self.n_particles < 2:
            return np.zeros(self.nbins)
        n = self.n_particles
        ideal = self.nsamples * n * (n - 1.0) / (2.0 * self.volume) * self.shell_volumes()
        return self.counts / ideal

    def write(self, path):
        gr = self.g()
        with open(path, "w") as io:
            io.write("# r g(r) count\n")
            for k in range(self.nbins):
                io.write("%.6f %.6f %d\n" % (self.r[k], gr[k], self.counts[k]))


    # -- run_simulation's sampler protocol: a sample at every `every`-th output step ---------------------------------
    def _begin(self, dev, run):
        self._period, self._total_steps = run.frequency * self.every, run.total_steps
        dev.rdf_setup(self.r_max, self.nbins)

    def _next(self, step):
        return _next_multiple(step, self._period, self._total_steps)

    def _act(self, dev, step):
        dev.rdf_sample()

    def _finish(self, dev, run, pathname):
        counts, ns = dev.rdf_read()
        self._accumulate(counts, ns, run.n, run.unitcell)
        self.write(os.path.join(pathname, "rdf.txt"))


def compute_rdf(state, params, r_max, nbins):
    """One sample of g(r) of `state`'s positions, taken on its device handle; returns a RadialDistribution."""
    rdf = RadialDistribution(r_max, nbins)
    dev = state.system.device
    dev.upload(x=state.system.positions, images=state.images)
    dev.rdf_setup(rdf.r_max, rdf.nbins)
    dev.rdf_sample()
    counts, ns = dev.rdf_read()
    rdf._accumulate(counts, ns, dev.n, state.unitcell)
    return rdf


# ---------------------------------------------------------------------------------------------------------------------
# Self dynamics: MSD, the non-Gaussian parameter, F_s(q, t) and the self part of the van Hove function, sampled on the
# device (md_dyn_*) from the wrapped positions and image counters the handle already holds.

LOG_N, LOG_BASE = 40, 1.35                 # io.generate_log_times' defaults: the reference's log-time schedule


def _log_schedule():
    """(maxlog, lags, stops): the reference's log-time steps -- `log_times=True` writes snapshot.<step> at step 0 and at
    every io.generate_log_times() step -- and their distinct lags floor(1.35^i), i <= 40 (the steps of the first block)."""
    from . import io as _io
    maxlog = int(np.floor(LOG_BASE ** LOG_N))
    stops = _io.generate_log_times(logn=LOG_N, logbase=LOG_BASE, filename=None)
    lags = [s for s in stops if s <= maxlog]
    return maxlog, lags, stops


def _parse_schedule(lags, origin_every):
    """(maxlog, lag_list, origin_every, nslots) of a sampling schedule: lags=None is the log-time schedule (one slot),
    explicit positive distinct `lags` need `origin_every` and use ceil(max lag / origin_every) <= 64 slots."""
    if lags is None:
        if origin_every is not None:
            raise ValueError("origin_every needs explicit lags (the default is the log-time schedule)")
        maxlog, lag_list, _ = _log_schedule()
        return maxlog, lag_list, None, 1
    lag_list = [int(v) for v in np.atleast_1d(lags)]
    if not lag_list or any(v < 1 for v in lag_list) or any(int(v) != v for v in np.atleast_1d(lags)):
        raise ValueError("lags must be positive integers")
    if len(set(lag_list)) != len(lag_list):
        raise ValueError("lags must be distinct")
    if origin_every is None or int(origin_every) != origin_every or int(origin_every) < 1:
        raise ValueError("explicit lags need origin_every, a positive integer")
    nslots = -(-max(lag_list) // int(origin_every))
    if nslots > 64:
        raise ValueError(f"ceil(max lag / origin_every) = {nslots} origin slots; at most 64")
    return None, lag_list, int(origin_every), nslots


def _schedule(maxlog, lags, origin_every, nslots, total_steps):
    """(stops, events) of one run of `total_steps` steps (SelfDynamics.schedule, shared with StructureFactor)."""
    T = int(total_steps)
    events = {}

    def ev(s):
        return events.setdefault(s, ([], None))

    if maxlog is not None:
        maxlog, _, stops = _log_schedule()
        row = {int(l): k for k, l in enumerate(lags)}
        for s in [0] + [s for s in stops if s < T]:
            smp, org = ev(s)
            if s > 0:
                j = (s - 1) // maxlog
                k = row.get(s - j * maxlog)
                if k is not None:
                    smp.append((0, k))
            if s % maxlog == 0:
                org = 0
            events[s] = (smp, org)
    else:
        E, ns = origin_every, nslots
        for m in range(0, (T + E - 1) // E):
            o = m * E
            smp, _ = ev(o)
            events[o] = (smp, m % ns)
        for m in range(0, (T + E - 1) // E):
            for k, l in enumerate(lags):
                s = m * E + int(l)
                if s < T:
                    ev(s)[0].append((m % ns, k, m))
        for s, (smp, org) in events.items():
            smp.sort(key=lambda t: (t[2], t[1]))
            events[s] = ([(a, b) for a, b, _ in smp], org)
    stops = sorted(events)
    return stops, events


def _check_q(q):
    """The wavenumbers of SelfDynamics / CageDynamics as a float64 array: at most 16, all finite."""
    q = np.array([float(v) for v in np.atleast_1d(np.asarray(q, dtype=np.float64))], dtype=np.float64)
    if q.size > 16:
        raise ValueError("at most 16 wavenumbers q")
    if not np.all(np.isfinite(q)):
        raise ValueError("every q must be finite")
    return q


def _write_blocks(path, header, lags, nsamples, lines):
    """`header`, then one block per lag that has a sample -- the lines that lines(k, lag) yields -- with a blank line
    between blocks."""
    with open(path, "w") as io:
        io.write(header)
        first = True
        for k, l in enumerate(lags):
            if nsamples[k] == 0:
                continue
            if not first:
                io.write("\n")
            first = False
            io.writelines(lines(k, l))


class _Scheduled:
    """What the samplers that correlate a frame with stored origins share: the schedule (lags, origin_every) and, for
    run_simulation's sampler protocol, the stops of schedule() and the device calls dev.<_prefix>_sample / _origin."""
    _prefix = None

    def _set_schedule(self, lags, origin_every):
        """maxlog, origin_every, nslots, lags and an all-zero nsamples; returns the number of lags."""
        self.maxlog, lag_list, self.origin_every, self.nslots = _parse_schedule(lags, origin_every)
        self.lags = np.array(lag_list, dtype=np.int64)
        self.nsamples = np.zeros(len(lag_list), dtype=np.int64)
        return len(lag_list)

    def schedule(self, total_steps):
        """(stops, events) for one run of `total_steps` steps: the sorted steps where the sampler acts, and per stop a
        pair (samples, origin): samples = [(slot, row), ...] in origin order, origin = the slot the frame is stored in
        after them, or None."""
        return _schedule(self.maxlog, self.lags, self.origin_every, self.nslots, total_steps)

    def _next(self, step):
        return _next_stop(self._stops, step)

    def _act(self, dev, step):
        """The work at one stop: the samples, then the origin (the frame is exported once for all samples)."""
        smp, org = self._events[step]
        if smp:
            getattr(dev, self._prefix + "_sample")([a for a, _ in smp], [b for _, b in smp])
        if org is not None:
            getattr(dev, self._prefix + "_origin")(org)


class SelfDynamics(_Scheduled):
    """Self dynamics of the particles, accumulated on the device over the samples of a schedule until reset().

    q: up to 16 wavenumbers for F_s(q, t).  r_max, nbins: the van Hove histogram (nbins = 0: none).  The schedule:
    lags=None is the reference's log-time schedule (origins at every multiple of maxlog = floor(1.35^40), samples at
    j maxlog + l for the 39 distinct lags l = floor(1.35^i)); explicit positive `lags` need `origin_every` = E (origins at
    m E, samples at m E + l, ceil(max l / E) origin slots used round-robin, at most 64).  At a step that has both, the
    samples are taken before the new origin is stored.  Each run_simulation call restarts the schedule at step 0; the
    samples accumulate here across calls.

    Fields: lags, nsamples (per lag), sums (per lag: sum d2, sum d4, sum s(q) per q), hist (per lag and bin), edges, r."""
    _prefix = "dyn"

    def __init__(self, q=(2.0 * math.pi,), r_max=None, nbins=0, lags=None, origin_every=None):
        q = _check_q(q)
        nbins = int(nbins)
        if not 0 <= nbins <= 8192:
            raise ValueError("nbins must be in 0..8192")
        if nbins > 0:
            if r_max is None or not (float(r_max) > 0.0 and math.isfinite(float(r_max))):
                raise ValueError("r_max must be finite and > 0 when nbins > 0")
            r_max = float(r_max)
        else:
            r_max = None if r_max is None else float(r_max)
        nl = self._set_schedule(lags, origin_every)
        self.q, self.r_max, self.nbins = q, r_max, nbins
        self.sums = np.zeros((nl, 2 + q.size))
        self.hist = np.zeros((nl, nbins), dtype=np.int64)
        self.edges = np.arange(nbins + 1, dtype=np.float64) * (r_max / nbins) if nbins else np.zeros(1)
        self.r = 0.5 * (self.edges[:-1] + self.edges[1:])
        self.n_particles = 0
        self.dimension = 3
        self.dt = 1.0

    def reset(self):
        self.nsamples[:] = 0
        self.sums[:] = 0.0
        self.hist[:] = 0

    # -- results ----------------------------------------------------------------------------------------------------
    def _accumulate(self, nsamples, sums, hist, n_particles, dimension, dt):
        self.nsamples += np.asarray(nsamples, dtype=np.int64)
        self.sums += np.asarray(sums, dtype=np.float64)
        if self.nbins:
            self.hist += np.asarray(hist, dtype=np.int64)
        self.n_particles, self.dimension, self.dt = int(n_particles), int(dimension), float(dt)

    def _per(self, col):
        ns = self.nsamples.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(ns > 0, self.sums[:, col] / (self.n_particles * ns), np.nan)

    def msd(self):
        """<d^2> per lag: sum d2 / (N ns); nan where a lag has no sample."""
        return self._per(0)

    def alpha2(self):
        """Non-Gaussian parameter d <d^4> / ((d + 2) <d^2>^2) - 1 per lag."""
        d = self.dimension
        with np.errstate(invalid="ignore", divide="ignore"):
            return d * self._per(1) / ((d + 2) * self.msd() ** 2) - 1.0

    def fs(self):
        """F_s(q, t), (nlags, nq): the axis-averaged self-intermediate scattering function sum s / (d N ns)."""
        ns = self.nsamples.astype(np.float64)[:, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(ns > 0, self.sums[:, 2:] / (self.dimension * self.n_particles * ns), np.nan)

    def shell_volumes(self, dimension=None):
        return shell_volumes(self.edges, self.dimension if dimension is None else dimension)

    def van_hove(self):
        """G_s(r_k, t), (nlags, nbins): count_k / (ns N V_k)."""
        ns = self.nsamples.astype(np.float64)[:, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(ns > 0, self.hist / (ns * self.n_particles * self.shell_volumes()[None, :]), np.nan)

    def write(self, path, dt=None):
        """# lag time msd alpha2 Fs(q=..)... nsamples, one row per lag that has a sample, time = lag dt."""
        dt = self.dt if dt is None else float(dt)
        msd, a2, fs = self.msd(), self.alpha2(), self.fs()
        fmt = "%d %.6e %.6e %.6e" + " %.6e" * self.q.size + " %d\n"
        with open(path, "w") as io:
            io.write("# lag time msd alpha2" + "".join(" Fs(q=%.6g)" % v for v in self.q) + " nsamples\n")
            for k, l in enumerate(self.lags):
                if self.nsamples[k] > 0:
                    io.write(fmt % ((int(l), l * dt, msd[k], a2[k]) + tuple(fs[k]) + (int(self.nsamples[k]),)))

    def write_van_hove(self, path):
        """One block per lag that has a sample, lines `lag r G_s count`, a blank line between blocks."""
        g = self.van_hove()
        _write_blocks(path, "# lag r G_s count\n", self.lags, self.nsamples, lambda k, l: (
            "%d %.6f %.6e %d\n" % (int(l), self.r[b], g[k, b], self.hist[k, b]) for b in range(self.nbins)))

    # -- run_simulation's sampler protocol: the stops of schedule() (_next and _act are _Scheduled's) -------------------
    def _begin(self, dev, run):
        self._stops, self._events = self.schedule(run.total_steps)
        dev.dyn_setup(self.nslots, len(self.lags), self.q, self.r_max or 0.0, self.nbins)

    def _finish(self, dev, run, pathname):
        ns, sums, hist = dev.dyn_read()
        self._accumulate(ns, sums, hist, run.n, run.dim, run.dt)
        self.write(os.path.join(pathname, "dynamics.txt"))
        if self.nbins > 0:
            self.write_van_hove(os.path.join(pathname, "vanhove.txt"))


# ---------------------------------------------------------------------------------------------------------------------
# Collective structure: the density modes rho(q) = sum_j exp(i q.x_j), the static structure factor S(q) = <|rho|^2> / N
# and the coherent intermediate scattering function F(q, t) = <rho(q, t0 + t) rho*(q, t0)> / N, sampled on the device
# (md_sq_*) on wave vectors commensurate with the cell.

MAX_WAVE_VECTORS = 16384


def select_wave_vectors(unitcell, q_max, dq=None, max_per_bin=16, seed=0):
    """Wave vectors commensurate with `unitcell` (d x d, columns = lattice vectors): returns (n, q, bin).

    n: int32 (nvec, d), every integer vector of the half space (first non-zero component positive, so -q never duplicates
    q) with |q_n| <= q_max, q_n = 2 pi U^-T n, thinned to at most `max_per_bin` per |q| bin of width dq (default 2 pi / the
    smallest face distance) by a permutation seeded with `seed`; q: |q_n|; bin: floor(|q_n| / dq).  Sorted by bin, then by
    n.  The same arguments give the same selection."""
    u = np.asarray(unitcell, dtype=np.float64)
    if u.ndim == 1:
        u = np.diag(u)
    d = u.shape[0]
    if u.shape != (d, d) or d not in (2, 3):
        raise ValueError("unitcell must be a 2 x 2 or 3 x 3 matrix (or its diagonal)")
    q_max, max_per_bin = float(q_max), int(max_per_bin)
    if not (q_max > 0.0 and math.isfinite(q_max)):
        raise ValueError("q_max must be finite and > 0")
    if max_per_bin < 1:
        raise ValueError("max_per_bin must be >= 1")
    uinv = np.linalg.inv(u)
    if dq is None:
        dq = 2.0 * math.pi * float(np.max(np.linalg.norm(uinv, axis=1)))   # face distance c = 1 / |row c of U^-1|
    dq = float(dq)
    if not (dq > 0.0 and math.isfinite(dq)):
        raise ValueError("dq must be finite and > 0")
    # n_c = (column c of U) . q / 2 pi, so |n_c| <= |column c| q_max / 2 pi
    m = [int(math.floor(np.linalg.norm(u[:, c]) * q_max / (2.0 * math.pi) * (1.0 + 1e-12))) for c in range(d)]
    if max(m) > 32767:
        raise ValueError("q_max needs integer components beyond 32767")
    rng = np.random.default_rng(seed)
    g2 = 4.0 * math.pi * math.pi * (uinv @ uinv.T)      # |q_n|^2 = n^T g2 n
    rest = np.meshgrid(*[np.arange(-m[c], m[c] + 1, dtype=np.int64) for c in range(1, d)], indexing="ij")
    rest = [r.reshape(-1) for r in rest]
    if d == 3:
        positive0 = (rest[0] > 0) | ((rest[0] == 0) & (rest[1] > 0))
    else:
        positive0 = rest[0] > 0
    restf = [r.astype(np.float64) for r in rest]
    # the part of n^T g2 n that does not involve n_0
    base = sum(g2[a + 1, b + 1] * restf[a] * restf[b] for a in range(d - 1) for b in range(d - 1))
    cross = 2.0 * sum(g2[0, a + 1] * restf[a] for a in range(d - 1))
    q2max = q_max * q_max
    nbins_max = int(q_max / dq) + 2
    thr = np.full(nbins_max, np.inf)                    # per bin: the largest key still in the selection once it is full
    pool_n = np.zeros((0, d), dtype=np.int64)
    pool_q = np.zeros(0)
    pool_b = np.zeros(0, dtype=np.int64)
    pool_k = np.zeros(0)
    for n0 in range(0, m[0] + 1):
        q2 = (g2[0, 0] * n0 * n0 + n0 * cross) + base
        ok = q2 <= q2max
        if n0 == 0:
            ok &= positive0
        idx = np.nonzero(ok)[0]
        if idx.size == 0:
            continue
        key = rng.random(idx.size)                      # a random key per candidate: the smallest keys of a bin are kept
        qn = np.sqrt(q2[idx])
        b = np.floor(qn / dq).astype(np.int64)
        keep = key <= thr[b]
        idx, key, qn, b = idx[keep], key[keep], qn[keep], b[keep]
        nn = np.empty((idx.size, d), dtype=np.int64)
        nn[:, 0] = n0
        for c in range(1, d):
            nn[:, c] = rest[c - 1][idx]
        pool_n = np.concatenate([pool_n, nn])
        pool_q = np.concatenate([pool_q, qn])
        pool_b = np.concatenate([pool_b, b])
        pool_k = np.concatenate([pool_k, key])
        order = np.lexsort((pool_k, pool_b))
        sb = pool_b[order]
        first = np.searchsorted(sb, sb, side="left")    # rank of an entry within its bin = position - first of the bin
        rank = np.arange(sb.size) - first
        sel = order[rank < max_per_bin]
        pool_n, pool_q, pool_b, pool_k = pool_n[sel], pool_q[sel], pool_b[sel], pool_k[sel]
        full = np.nonzero(np.bincount(pool_b, minlength=nbins_max) >= max_per_bin)[0]
        if full.size:
            worst = np.zeros(nbins_max)
            np.maximum.at(worst, pool_b, pool_k)
            thr[full] = worst[full]
    if pool_n.shape[0] == 0:
        raise ValueError("no wave vector with |q| <= q_max: the smallest one of this cell is longer")
    if pool_n.shape[0] > MAX_WAVE_VECTORS:
        raise ValueError(f"{pool_n.shape[0]} wave vectors selected; at most {MAX_WAVE_VECTORS} (lower q_max or max_per_bin, "
                         "or widen dq)")
    order = np.lexsort(tuple(pool_n[:, c] for c in range(d - 1, -1, -1)) + (pool_b,))
    return pool_n[order].astype(np.int32), pool_q[order], pool_b[order]


def wave_vector_lengths(unitcell, n):
    """|q_n| = 2 pi |U^-T n| of integer vectors n (nvec, d)."""
    u = np.asarray(unitcell, dtype=np.float64)
    if u.ndim == 1:
        u = np.diag(u)
    return 2.0 * math.pi * np.linalg.norm(np.asarray(n, dtype=np.float64) @ np.linalg.inv(u), axis=1)


class _WaveVectors:
    """What the samplers on select_wave_vectors' vectors share: the selection for the cell of the first use (q_max=None:
    none; at most _max_vectors, refused with the class's _too_many message), the |q| bins, the bin average."""
    _max_vectors = _too_many = None

    def _select(self, unitcell):
        if self.q_max is None:
            return
        u = np.array(unitcell, dtype=np.float64)
        if self.unitcell is not None:
            if u.shape != self.unitcell.shape or not np.array_equal(u, self.unitcell):
                raise ValueError("the unit cell differs from the one the wave vectors were selected for; reset() first")
            return
        n, q, b = select_wave_vectors(u, self.q_max, self.dq, self.max_per_bin, self.seed)
        if self._max_vectors is not None and n.shape[0] > self._max_vectors:
            raise ValueError(self._too_many.format(n.shape[0]))
        self._set_vectors(u, n, q, b)

    def _set_vectors(self, unitcell, n, q, b):
        self.unitcell = unitcell
        self.n, self.qvec = np.ascontiguousarray(n, dtype=np.int32), np.asarray(q, dtype=np.float64)
        bins, self.bin = np.unique(np.asarray(b), return_inverse=True)
        self.bin = self.bin.reshape(-1)
        self.nvectors = np.bincount(self.bin, minlength=bins.size).astype(np.int64)
        self.q = np.bincount(self.bin, weights=self.qvec, minlength=bins.size) / self.nvectors
        self._zero_vector_sums(self.n.shape[0])

    def _binned(self, per_vector):
        return np.bincount(self.bin, weights=per_vector, minlength=self.q.size) / self.nvectors


class StructureFactor(_Scheduled, _WaveVectors):
    """S(q) and, with dynamic=True, the coherent F(q, t), accumulated on the device until reset().

    The wave vectors are select_wave_vectors(unitcell, q_max, dq, max_per_bin, seed) of the cell the sampler is first used
    on.  Static samples are taken at every `every`-th output step of run_simulation(..., sq=...).  dynamic=True adds the
    correlations on SelfDynamics' schedule: lags=None is the reference's log-time schedule, explicit positive `lags` need
    `origin_every` (at most 64 origin slots); at a step that has both, the samples are taken before the new origin is
    stored.  An origin costs 2 nvec doubles.

    Fields: n (nvec, d), qvec (|q| per vector), bin (per vector: index into q), q (mean |q| of a bin), nvectors (per bin),
    nstatic, s2 (per vector: sum |rho|^2), lags, nsamples (per lag), corr (nlags, nvec: sum Re rho(t0 + t) rho*(t0))."""

    def __init__(self, q_max, dq=None, max_per_bin=16, seed=0, every=1, lags=None, origin_every=None, dynamic=False):
        q_max, max_per_bin, every = float(q_max), int(max_per_bin), int(every)
        if not (q_max > 0.0 and math.isfinite(q_max)):
            raise ValueError("q_max must be finite and > 0")
        if dq is not None and not (float(dq) > 0.0 and math.isfinite(float(dq))):
            raise ValueError("dq must be finite and > 0")
        if max_per_bin < 1:
            raise ValueError("max_per_bin must be >= 1")
        if every < 1:
            raise ValueError("every must be >= 1")
        self.q_max, self.dq, self.max_per_bin, self.seed, self.every = q_max, dq, max_per_bin, seed, every
        self.dynamic = bool(dynamic)
        if self.dynamic:
            self._set_schedule(lags, origin_every)
        else:
            if lags is not None or origin_every is not None:
                raise ValueError("lags and origin_every need dynamic=True")
            self.maxlog, self.origin_every, self.nslots = None, None, 0
            self.lags, self.nsamples = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
        self.nstatic = 0
        self.unitcell = None
        self.n = self.qvec = self.bin = self.q = self.nvectors = self.s2 = self.corr = None
        self.n_particles = 0
        self.dt = 1.0

    def _zero_vector_sums(self, nvec):
        self.s2 = np.zeros(nvec)
        self.corr = np.zeros((len(self.lags), nvec))

    def reset(self):
        """Forget the samples and the wave vectors (the next use selects them again, for the cell it meets)."""
        self.nsamples[:] = 0
        self.nstatic = 0
        self.unitcell = None
        self.n = self.qvec = self.bin = self.q = self.nvectors = self.s2 = self.corr = None

    def schedule(self, total_steps):
        """(stops, events) of the dynamic part, as SelfDynamics.schedule; empty without dynamic=True."""
        return super().schedule(total_steps) if self.dynamic else ([], {})

    def _accumulate(self, nstatic, s2, nsamples, corr, n_particles, dt):
        self.nstatic += int(nstatic)
        self.s2 += np.asarray(s2, dtype=np.float64)
        if self.dynamic:
            self.nsamples += np.asarray(nsamples, dtype=np.int64)
            self.corr += np.asarray(corr, dtype=np.float64)
        self.n_particles, self.dt = int(n_particles), float(dt)

    # -- results ----------------------------------------------------------------------------------------------------
    def s_vectors(self):
        """S(q_v) per wave vector: s2_v / (nstatic N); nan before the first static sample."""
        if self.nstatic == 0:
            return np.full(self.s2.shape, np.nan)
        return self.s2 / (self.nstatic * self.n_particles)

    def s(self):
        """S(q) per |q| bin: sum over the bin's vectors of s2_v / (nstatic N M_bin)."""
        return self._binned(self.s_vectors())

    def f_vectors(self):
        """F(q_v, t), (nlags, nvec): corr_kv / (ns_k N); nan where a lag has no sample."""
        ns = self.nsamples.astype(np.float64)[:, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(ns > 0, self.corr / (ns * self.n_particles), np.nan)

    def f(self):
        """F(q, t), (nlags, nbins): sum over the bin's vectors of corr_kv / (ns_k N M_bin)."""
        fv = self.f_vectors()
        return np.array([self._binned(fv[k]) for k in range(fv.shape[0])]).reshape(fv.shape[0], self.q.size)

    def f_normalised(self):
        """F(q, t) / S(q), (nlags, nbins)."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.f() / self.s()[None, :]

    def write(self, path):
        """# q S(q) nvectors nsamples, one row per |q| bin."""
        sq = self.s()
        with open(path, "w") as io:
            io.write("# q S(q) nvectors nsamples\n")
            for b in range(self.q.size):
                io.write("%.6f %.6e %d %d\n" % (self.q[b], sq[b], self.nvectors[b], self.nstatic))

    def write_fqt(self, path, dt=None):
        """One block per lag that has a sample, lines `lag time q F F/S nsamples`, a blank line between blocks."""
        dt = self.dt if dt is None else float(dt)
        f, fn = self.f(), self.f_normalised()
        _write_blocks(path, "# lag time q F F/S nsamples\n", self.lags, self.nsamples, lambda k, l: (
            "%d %.6e %.6f %.6e %.6e %d\n" % (int(l), l * dt, self.q[b], f[k, b], fn[k, b], int(self.nsamples[k]))
            for b in range(self.q.size)))

    # -- run_simulation's sampler protocol: static at every `every`-th output step, dynamic at the stops of schedule() -
    def _begin(self, dev, run):
        self._period, self._total_steps = run.frequency * self.every, run.total_steps
        self._stops, self._events = self.schedule(run.total_steps)
        self._select(run.unitcell)
        dev.sq_setup(self.n, self.nslots, len(self.lags))

    def _next(self, step):
        static = _next_multiple(step, self._period, self._total_steps)
        dynamic = _next_stop(self._stops, step)
        if static is None or dynamic is None:
            return dynamic if static is None else static
        return min(static, dynamic)

    def _act(self, dev, step):
        """The work at one stop: rho of the frame once, then the static sample, the correlations, the origin."""
        smp, org = self._events.get(step, ([], None))
        dev.sq_sample(step % self._period == 0, [a for a, _ in smp], [b for _, b in smp], org)

    def _finish(self, dev, run, pathname):
        nst, s2, ns, corr = dev.sq_read()
        self._accumulate(nst, s2, ns, corr, run.n, run.dt)
        self.write(os.path.join(pathname, "sq.txt"))
        if self.dynamic:
            self.write_fqt(os.path.join(pathname, "fqt.txt"))


def compute_sq(state, params, q_max, dq=None, max_per_bin=16, seed=0):
    """One static sample of S(q) of `state`'s positions, taken on its device handle; returns a StructureFactor."""
    sq = StructureFactor(q_max, dq=dq, max_per_bin=max_per_bin, seed=seed)
    dev = state.system.device
    dev.upload(x=state.system.positions, images=state.images)
    sq._select(state.unitcell)
    dev.sq_setup(sq.n, sq.nslots, len(sq.lags))
    dev.sq_sample(True)
    nst, s2, ns, corr = dev.sq_read()
    sq._accumulate(nst, s2, ns, corr, dev.n, params.dt)
    return sq


# ---------------------------------------------------------------------------------------------------------------------
# Currents: j_a(q) = sum_i v_i,a exp(i q.x_i), its longitudinal part e.j (e = q / |q|) and the rest, the transverse part;
# C_L(q, t) = <e.j(t0 + t) (e.j)*(t0)> / N, C_T(q, t) = <j_T(t0 + t) . j_T*(t0)> / ((d - 1) N), and the velocity
# autocorrelation Z(t) = <v_i(t0 + t) . v_i(t0)>, sampled on the device (md_cur_*) on wave vectors commensurate with the cell.

class CurrentCorrelations(_Scheduled, _WaveVectors):
    """Longitudinal and transverse current correlations C_L(q, t), C_T(q, t) and, with vacf=True, the velocity
    autocorrelation Z(t), accumulated on the device over the samples of a schedule until reset().

    The wave vectors are select_wave_vectors(unitcell, q_max, dq, max_per_bin, seed) of the cell the sampler is first used
    on, their directions e = q_n / |q_n| from the same Cartesian q_n that wave_vector_lengths forms; q_max=None samples
    the VACF only.  The schedule (lags, origin_every) is SelfDynamics': log-time by default, explicit lags need
    origin_every (at most 64 origin slots), samples before the new origin at a shared step.  The equal-time (static)
    sample -- C_L(q, 0), C_T(q, 0), Z(0) -- is taken exactly at the stops that store an origin.  An origin costs
    2 d nvec doubles on the device and, with vacf, the frame's N d velocities.  Unit mass throughout: C_L(q, 0) =
    C_T(q, 0) = Z(0) / d = kT in equilibrium; -d^2 F(q, t) / dt^2 = q^2 C_L(q, t).

    Fields: n (nvec, d), e (nvec, d), qvec (|q| per vector), bin (per vector: index into q), q (mean |q| of a bin),
    nvectors (per bin), nstatic, s_tot, s_long (per vector: sum |j|^2, sum |e.j|^2), lags, nsamples (per lag), c_tot,
    c_long (nlags, nvec), z (per lag: sum Z), z0 (sum of the equal-time Z)."""
    _prefix = "cur"

    def __init__(self, q_max, dq=None, max_per_bin=16, seed=0, lags=None, origin_every=None, vacf=True):
        if q_max is not None:
            q_max = float(q_max)
            if not (q_max > 0.0 and math.isfinite(q_max)):
                raise ValueError("q_max must be finite and > 0 (or None for the VACF only)")
        elif dq is not None:
            raise ValueError("dq needs q_max")
        elif not vacf:
            raise ValueError("q_max=None with vacf=False leaves nothing to sample")
        if dq is not None and not (float(dq) > 0.0 and math.isfinite(float(dq))):
            raise ValueError("dq must be finite and > 0")
        if int(max_per_bin) < 1:
            raise ValueError("max_per_bin must be >= 1")
        nl = self._set_schedule(lags, origin_every)
        self.q_max, self.dq, self.max_per_bin, self.seed = q_max, dq, int(max_per_bin), seed
        self.with_vacf = bool(vacf)
        self.nstatic = 0
        self.z, self.z0 = np.zeros(nl), 0.0
        self.unitcell = None
        self.n = self.e = self.qvec = self.bin = self.q = self.nvectors = None
        self.s_tot = self.s_long = self.c_tot = self.c_long = None
        self.n_particles = 0
        self.dimension = 3
        self.dt = 1.0

    def _zero_vector_sums(self, nvec):
        u = self.unitcell if self.unitcell.ndim == 2 else np.diag(self.unitcell)
        qc = 2.0 * math.pi * (np.asarray(self.n, dtype=np.float64) @ np.linalg.inv(u))
        self.e = np.ascontiguousarray(qc / np.linalg.norm(qc, axis=1)[:, None])
        self.s_tot, self.s_long = np.zeros(nvec), np.zeros(nvec)
        self.c_tot, self.c_long = np.zeros((len(self.lags), nvec)), np.zeros((len(self.lags), nvec))

    def reset(self):
        """Forget the samples and the wave vectors (the next use selects them again, for the cell it meets)."""
        self.nsamples[:] = 0
        self.nstatic = 0
        self.z[:] = 0.0
        self.z0 = 0.0
        self.unitcell = None
        self.n = self.e = self.qvec = self.bin = self.q = self.nvectors = None
        self.s_tot = self.s_long = self.c_tot = self.c_long = None

    # -- results ----------------------------------------------------------------------------------------------------
    def _accumulate(self, nstatic, s_tot, s_long, nsamples, c_tot, c_long, z, n_particles, dimension, dt):
        self.nstatic += int(nstatic)
        self.nsamples += np.asarray(nsamples, dtype=np.int64)
        if self.s_tot is not None:
            self.s_tot += np.asarray(s_tot, dtype=np.float64)
            self.s_long += np.asarray(s_long, dtype=np.float64)
            self.c_tot += np.asarray(c_tot, dtype=np.float64)
            self.c_long += np.asarray(c_long, dtype=np.float64)
        if self.with_vacf:
            z = np.asarray(z, dtype=np.float64)
            self.z += z[:-1]
            self.z0 += float(z[-1])
        self.n_particles, self.dimension, self.dt = int(n_particles), int(dimension), float(dt)

    def _need_vectors(self):
        if self.s_tot is None:
            raise ValueError("no wave vectors: give q_max (and use the sampler once) for C_L and C_T")

    def _lag_norm(self):
        ns = self.nsamples.astype(np.float64)[:, None]
        return ns, ns * self.n_particles

    def cl_vectors(self):
        """C_L(q_v, t), (nlags, nvec): c_long / (ns N); nan where a lag has no sample."""
        self._need_vectors()
        ns, norm = self._lag_norm()
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(ns > 0, self.c_long / norm, np.nan)

    def ct_vectors(self):
        """C_T(q_v, t), (nlags, nvec): (c_tot - c_long) / ((d - 1) ns N); nan where a lag has no sample."""
        self._need_vectors()
        ns, norm = self._lag_norm()
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(ns > 0, (self.c_tot - self.c_long) / ((self.dimension - 1) * norm), np.nan)

    def _binned_rows(self, per_vector):
        return np.array([self._binned(row) for row in per_vector]).reshape(per_vector.shape[0], self.q.size)

    def cl(self):
        """C_L(q, t), (nlags, nbins): the mean of cl_vectors() over a |q| bin's vectors."""
        return self._binned_rows(self.cl_vectors())

    def ct(self):
        """C_T(q, t), (nlags, nbins): the mean of ct_vectors() over a |q| bin's vectors."""
        return self._binned_rows(self.ct_vectors())

    def cl0(self):
        """C_L(q, 0) per |q| bin from the static sums: s_long / (nstatic N); nan before the first static sample."""
        self._need_vectors()
        if self.nstatic == 0:
            return np.full(self.q.size, np.nan)
        return self._binned(self.s_long / (self.nstatic * self.n_particles))

    def ct0(self):
        """C_T(q, 0) per |q| bin from the static sums: (s_tot - s_long) / ((d - 1) nstatic N)."""
        self._need_vectors()
        if self.nstatic == 0:
            return np.full(self.q.size, np.nan)
        return self._binned((self.s_tot - self.s_long) / ((self.dimension - 1) * self.nstatic * self.n_particles))

    def _need_vacf(self):
        if not self.with_vacf:
            raise ValueError("the VACF was not sampled: construct with vacf=True")

    def vacf(self):
        """Z(t) = <v_i(t0 + t) . v_i(t0)> per lag: z / (ns N); nan where a lag has no sample."""
        self._need_vacf()
        ns = self.nsamples.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(ns > 0, self.z / (ns * self.n_particles), np.nan)

    def vacf0(self):
        """Z(0) = <v_i . v_i> from the static samples: z0 / (nstatic N); nan before the first."""
        self._need_vacf()
        return self.z0 / (self.nstatic * self.n_particles) if self.nstatic > 0 else float("nan")

    def write(self, path, dt=None):
        """One block per lag, lines `lag time q C_L C_T nsamples`, a blank line between blocks: first lag 0 from the
        static sums (nsamples = nstatic), then every lag that has a sample."""
        dt = self.dt if dt is None else float(dt)
        cl, ct, cl0, ct0 = self.cl(), self.ct(), self.cl0(), self.ct0()
        lags = [0] + [int(l) for l in self.lags]
        ns = [self.nstatic] + [int(v) for v in self.nsamples]

        def lines(k, l):
            a, b = (cl0, ct0) if k == 0 else (cl[k - 1], ct[k - 1])
            return ("%d %.6e %.6f %.6e %.6e %d\n" % (l, l * dt, self.q[i], a[i], b[i], ns[k]) for i in range(self.q.size))

        _write_blocks(path, "# lag time q C_L C_T nsamples\n", lags, ns, lines)

    def write_vacf(self, path, dt=None):
        """# lag time Z Z/Z(0) nsamples: lag 0 from the static samples, then one row per lag that has a sample."""
        dt = self.dt if dt is None else float(dt)
        z, z0 = self.vacf(), self.vacf0()
        with open(path, "w") as io:
            io.write("# lag time Z Z/Z(0) nsamples\n")
            if self.nstatic > 0:
                io.write("%d %.6e %.6e %.6e %d\n" % (0, 0.0, z0, 1.0, self.nstatic))
            for k, l in enumerate(self.lags):
                if self.nsamples[k] > 0:
                    with np.errstate(invalid="ignore", divide="ignore"):
                        io.write("%d %.6e %.6e %.6e %d\n" % (int(l), l * dt, z[k], z[k] / z0, int(self.nsamples[k])))

    # -- run_simulation's sampler protocol: the stops of schedule(); the static sample where an origin is stored ---------
    def _begin(self, dev, run):
        if run.brownian:
            raise ValueError("currents= is not available with Brownian dynamics (no velocities)")
        self._stops, self._events = self.schedule(run.total_steps)
        self._select(run.unitcell)
        dev.cur_setup(self.n, self.e, self.nslots, len(self.lags), vacf=self.with_vacf)

    def _act(self, dev, step):
        """The work at one stop: j of the frame once, then the static sample (at an origin stop), the correlations, the
        origin."""
        smp, org = self._events[step]
        dev.cur_sample(org is not None, [a for a, _ in smp], [b for _, b in smp], org)

    def _finish(self, dev, run, pathname):
        nst, s_tot, s_long, ns, c_tot, c_long, z = dev.cur_read()
        self._accumulate(nst, s_tot, s_long, ns, c_tot, c_long, z, run.n, run.dim, run.dt)
        if self.s_tot is not None:
            self.write(os.path.join(pathname, "currents.txt"))
        if self.with_vacf:
            self.write_vacf(os.path.join(pathname, "vacf.txt"))


# ---------------------------------------------------------------------------------------------------------------------
# Stress: the pressure tensor P_ab = (K_ab + W_ab) / V, K_ab = sum v_a v_b (unit mass), W_ab = sum over pairs of
# (f/r) del_a del_b, and the Green-Kubo correlations of its shear components, sampled on the device (md_stress_*) from the
# positions, velocities and neighbour rows the handle already holds.

def _tensor(comp, d):
    """d x d symmetric matrix of a component vector (xx, yy, zz, xy, xz, yz in 3-D; xx, yy, xy in 2-D)."""
    c = np.asarray(comp, dtype=np.float64)
    t = np.zeros((d, d))
    if d == 3:
        t[0, 0], t[1, 1], t[2, 2] = c[0], c[1], c[2]
        t[0, 1] = t[1, 0] = c[3]
        t[0, 2] = t[2, 0] = c[4]
        t[1, 2] = t[2, 1] = c[5]
    else:
        t[0, 0], t[1, 1] = c[0], c[1]
        t[0, 1] = t[1, 0] = c[2]
    return t


class StressTensor:
    """The pressure tensor and, with nlags > 0, the stress autocorrelation functions and the running Green-Kubo viscosity,
    accumulated on the device until reset().

    Passed to run_simulation(..., stress=...), it takes a sample at every step that is a multiple of `every` (0 included);
    lag k of the correlations is the time k * every * dt.  Each run_simulation call restarts the step counter and the
    ring of past samples; the sums accumulate here across calls.

    Channels: 3-D  sig_xy, sig_xz, sig_yz, (sig_xx - sig_yy)/2, (sig_yy - sig_zz)/2, tr sig / 3;
    2-D  sig_xy, (sig_xx - sig_yy)/2, tr sig / 2, with sig = K + W (extensive: the pressure tensor times V).

    Fields: nsamples, sum_kin, sum_vir (component vectors summed over the samples), corr (nlags, nc: sum of ch(m) ch(m - k)),
    ncorr (products per lag)."""

    def __init__(self, every, nlags=0):
        if int(every) != every or int(every) < 1:
            raise ValueError("every must be a positive integer")
        if int(nlags) != nlags or not 0 <= int(nlags) <= 65536:
            raise ValueError("nlags must be in 0..65536")
        self.every, self.nlags = int(every), int(nlags)
        self.dimension = 3
        self.n_particles = 0
        self.volume = 0.0
        self.dt = 1.0
        self.nsamples = 0
        self.sum_kin = self.sum_vir = self.corr = None
        self.ncorr = np.zeros(self.nlags, dtype=np.int64)

    def reset(self):
        self.nsamples = 0
        self.sum_kin = self.sum_vir = self.corr = None
        self.ncorr = np.zeros(self.nlags, dtype=np.int64)

    def schedule(self, total_steps):
        """The steps of one run of `total_steps` steps at which a sample is taken: 0, every, 2 every, ... < total_steps."""
        return list(range(0, int(total_steps), self.every))

    def _accumulate(self, nsamples, sum_kin, sum_vir, ncorr, corr, n_particles, unitcell, dt):
        u = np.asarray(unitcell, dtype=np.float64)
        d = u.shape[0]
        nc = 6 if d == 3 else 3
        sum_kin, sum_vir = np.asarray(sum_kin, dtype=np.float64), np.asarray(sum_vir, dtype=np.float64)
        corr = np.asarray(corr, dtype=np.float64).reshape(self.nlags, nc)
        if sum_kin.shape != (nc,) or sum_vir.shape != (nc,):
            raise ValueError(f"expected {nc} tensor components")
        if self.sum_kin is None:
            self.sum_kin, self.sum_vir, self.corr = np.zeros(nc), np.zeros(nc), np.zeros((self.nlags, nc))
        elif self.sum_kin.shape != (nc,):
            raise ValueError("the dimension differs from the one already accumulated; reset() first")
        self.nsamples += int(nsamples)
        self.sum_kin += sum_kin
        self.sum_vir += sum_vir
        self.corr += corr
        self.ncorr += np.asarray(ncorr, dtype=np.int64).reshape(self.nlags)
        self.dimension, self.n_particles = d, int(n_particles)
        self.volume = abs(float(np.linalg.det(u)))
        self.dt = float(dt)

    # -- results ----------------------------------------------------------------------------------------------------
    def _need(self):
        if self.nsamples == 0 or self.sum_kin is None:
            raise ValueError("no sample yet")

    def kinetic(self):
        """Mean kinetic tensor <sum v_a v_b>, d x d."""
        self._need()
        return _tensor(self.sum_kin / self.nsamples, self.dimension)

    def virial(self):
        """Mean virial tensor <sum (f/r) del_a del_b>, d x d."""
        self._need()
        return _tensor(self.sum_vir / self.nsamples, self.dimension)

    def pressure_tensor(self):
        """(K + W) / V, d x d."""
        return (self.kinetic() + self.virial()) / self.volume

    def pressure(self):
        """tr P / d.  The isotropic tail correction of a truncated potential (pot.pressure_lrc(N, V)) is NOT included: it
        is the caller's to add, as the thermo line of run_simulation does."""
        return float(np.trace(self.pressure_tensor())) / self.dimension

    def temperature(self):
        """tr K / nf with nf = d (N - 1), the thermo line's temperature."""
        return float(np.trace(self.kinetic())) / (self.dimension * (self.n_particles - 1.0))

    def shear_channels(self):
        """Indices of the channels averaged into C_shear: the off-diagonal components and the normal-stress differences."""
        return [0, 1, 2, 3, 4] if self.dimension == 3 else [0, 1]

    def acf(self):
        """(t, C, C_shear): lag times k every dt, the per-channel correlations corr / ncorr (nlags, nc) with <p-channel>^2
        subtracted from the last (pressure) channel, and the average of the shear channels.  nan where a lag has no
        product.  Units of sig = P V."""
        self._need()
        if self.nlags == 0:
            raise ValueError("no correlations were requested (nlags = 0)")
        t = np.arange(self.nlags, dtype=np.float64) * (self.every * self.dt)
        nn = self.ncorr.astype(np.float64)[:, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            c = np.where(nn > 0, self.corr / nn, np.nan)
        d = self.dimension
        pbar = (np.sum(self.sum_kin[:d]) + np.sum(self.sum_vir[:d])) / (d * self.nsamples)
        c[:, -1] = c[:, -1] - pbar * pbar
        return t, c, c[:, self.shear_channels()].mean(axis=1)

    def viscosity(self, kT=None):
        """(t, eta): the running Green-Kubo integral eta(t) = 1 / (V kT) int_0^t C_shear, trapezoid rule on the lag grid;
        kT defaults to temperature()."""
        t, _, cs = self.acf()
        kT = self.temperature() if kT is None else float(kT)
        eta = np.zeros(self.nlags)
        if self.nlags > 1:
            eta[1:] = np.cumsum(0.5 * (cs[1:] + cs[:-1]) * np.diff(t))
        return t, eta / (self.volume * kT)

    def write(self, path):
        """# component kinetic virial pressure, one row per tensor component (means over the samples), then nsamples."""
        d = self.dimension
        names = ["xx", "yy", "zz", "xy", "xz", "yz"] if d == 3 else ["xx", "yy", "xy"]
        k, w = self.sum_kin / self.nsamples, self.sum_vir / self.nsamples
        with open(path, "w") as io:
            io.write("# component kinetic virial pressure\n")
            for c, name in enumerate(names):
                io.write("%s %.10e %.10e %.10e\n" % (name, k[c], w[c], (k[c] + w[c]) / self.volume))
            io.write("# nsamples %d\n" % self.nsamples)

    def write_acf(self, path, kT=None):
        """# lag time C_shear C_ch... C_pp eta_running ncorr, one row per lag that has a product."""
        t, c, cs = self.acf()
        _, eta = self.viscosity(kT)
        nch = c.shape[1]
        with open(path, "w") as io:
            io.write("# lag time C_shear" + "".join(" C_ch%d" % i for i in range(nch - 1)) + " C_pp eta_running ncorr\n")
            for k in range(self.nlags):
                if self.ncorr[k] > 0:
                    io.write(("%d %.6e %.6e" + " %.6e" * nch + " %.6e %d\n")
                             % ((k, t[k], cs[k]) + tuple(c[k]) + (eta[k], int(self.ncorr[k]))))


    # -- run_simulation's sampler protocol: a sample at every multiple of `every` --------------------------------------
    def _begin(self, dev, run):
        if run.brownian:
            raise ValueError("stress= needs velocities: not available with the Brownian ensemble")
        self._total_steps = run.total_steps
        dev.stress_setup(self.nlags)

    def _next(self, step):
        return _next_multiple(step, self.every, self._total_steps)

    def _act(self, dev, step):
        dev.stress_sample()

    def _finish(self, dev, run, pathname):
        ns, sk, sv, ncorr, corr = dev.stress_read()
        self._accumulate(ns, sk, sv, ncorr, corr, run.n, run.unitcell, run.dt)
        if self.nsamples > 0:
            self.write(os.path.join(pathname, "stress.txt"))
        if self.nsamples > 0 and self.nlags > 0:
            self.write_acf(os.path.join(pathname, "stress_acf.txt"))


def compute_stress(state, params):
    """One sample of the stress of `state` (positions and velocities), taken on its device handle with params.potential;
    returns (K, W) as d x d arrays: K_ab = sum v_a v_b, W_ab = sum over pairs of (f/r) del_a del_b.  The pressure tensor is
    (K + W) / V."""
    dev = state.system.device
    spec = params.potential.device_spec()
    if spec[0] != "builtin":
        raise ValueError("compute_stress needs a built-in potential (user potentials are not supported by the sampler)")
    dev.set_potential(spec[1], spec[2])
    dev.upload(x=state.system.positions, v=state.velocities, images=state.images, diameters=state.diameters)
    dev.stress_setup(0)
    dev.stress_sample()
    kin, vir = dev.stress_tensor()
    return _tensor(kin, dev.dim), _tensor(vir, dev.dim)


# ---------------------------------------------------------------------------------------------------------------------
# Bond-orientational order: Steinhardt q_l(i) (l = 4, 6) and its neighbour-averaged form qbar_l(i) in 3-D, |psi_k(i)| in
# 2-D, and ten Wolde's solid particles (at least min_connections neighbours with bond coherence s_ij > threshold), sampled
# on the device (md_boo_*) from the positions and the neighbour rows the handle already holds.  The potential is never
# evaluated: it works with every potential and every ensemble.

_BOO_FR = ("sum_q", "sum_q2", "sum_qbar", "sum_qbar2", "sum_n", "sum_c", "n_solid", "global_order")


class BondOrder:
    """Local bond-orientational order, accumulated on the device until reset().

    r_neigh: the neighbour radius (<= the list cutoff of the handle).  order: l (4 or 6) in 3-D, k (1..12) in 2-D.
    Passed to run_simulation(..., bond_order=...), it takes a sample at every `every`-th output step; `nseries` rows of
    the per-sample series are kept (default: one per sample of the run).

    Fields: nsamples, sum_fr (the 8 frame sums added over the samples: sum q, q^2, qbar, qbar^2, n, c, solid particles,
    global order), hist_q, hist_qbar (nbins bins over [0, 1]), hist_nnb, hist_conn (33 bins, clamped to 32), steps and
    frames (the series: the step and the frame vector of each recorded sample)."""

    def __init__(self, r_neigh, order=6, every=1, nbins=100, threshold=0.7, min_connections=7, nseries=None):
        r_neigh, threshold = float(r_neigh), float(threshold)
        if not (r_neigh > 0.0 and math.isfinite(r_neigh)):
            raise ValueError("r_neigh must be finite and > 0")
        if int(order) != order or not 1 <= int(order) <= 12:
            raise ValueError("order must be 4 or 6 (3-D) or in 1..12 (2-D)")
        if int(every) != every or int(every) < 1:
            raise ValueError("every must be a positive integer")
        if int(nbins) != nbins or not 1 <= int(nbins) <= 8192:
            raise ValueError("nbins must be in 1..8192")
        if not math.isfinite(threshold):
            raise ValueError("threshold must be finite")
        if int(min_connections) != min_connections or not 0 <= int(min_connections) <= 32:
            raise ValueError("min_connections must be in 0..32")
        if nseries is not None and (int(nseries) != nseries or not 0 <= int(nseries) <= 1 << 20):
            raise ValueError("nseries must be in 0..1048576")
        self.r_neigh, self.order, self.every, self.nbins = r_neigh, int(order), int(every), int(nbins)
        self.threshold, self.min_connections = threshold, int(min_connections)
        self.nseries = None if nseries is None else int(nseries)
        self.edges = np.arange(self.nbins + 1, dtype=np.float64) / self.nbins
        self.centres = 0.5 * (self.edges[:-1] + self.edges[1:])
        self.n_particles = 0
        self.reset()

    def reset(self):
        self.nsamples = 0
        self.sum_fr = np.zeros(8)
        self.hist_q = np.zeros(self.nbins, dtype=np.int64)
        self.hist_qbar = np.zeros(self.nbins, dtype=np.int64)
        self.hist_nnb = np.zeros(33, dtype=np.int64)
        self.hist_conn = np.zeros(33, dtype=np.int64)
        self.steps = np.zeros(0, dtype=np.int64)
        self.frames = np.zeros((0, 8))

    def schedule(self, total_steps, frequency):
        """The steps of one run at which a sample is taken: the multiples of frequency * every below total_steps."""
        return list(range(0, int(total_steps), int(frequency) * self.every))

    def _accumulate(self, nsamples, sum_fr, hist_q, hist_qbar, hist_nnb, hist_conn, series, steps, n_particles):
        if self.nsamples > 0 and int(n_particles) != self.n_particles:
            raise ValueError("the number of particles differs from the one already accumulated; reset() first")
        self.nsamples += int(nsamples)
        self.sum_fr += np.asarray(sum_fr, dtype=np.float64).reshape(8)
        self.hist_q += np.asarray(hist_q, dtype=np.int64).reshape(self.nbins)
        self.hist_qbar += np.asarray(hist_qbar, dtype=np.int64).reshape(self.nbins)
        self.hist_nnb += np.asarray(hist_nnb, dtype=np.int64).reshape(33)
        self.hist_conn += np.asarray(hist_conn, dtype=np.int64).reshape(33)
        series = np.asarray(series, dtype=np.float64).reshape(-1, 8)
        steps = np.asarray(steps, dtype=np.int64)[: len(series)]
        self.frames = np.concatenate([self.frames, series[: len(steps)]])
        self.steps = np.concatenate([self.steps, steps])
        self.n_particles = int(n_particles)

    # -- results ----------------------------------------------------------------------------------------------------
    def _per_particle(self, k):
        if self.nsamples == 0 or self.n_particles == 0:
            raise ValueError("no sample yet")
        return float(self.sum_fr[k]) / (self.nsamples * self.n_particles)

    def mean_q(self):
        """<q_l(i)> (2-D: <|psi_k(i)|>) over particles and samples."""
        return self._per_particle(0)

    def mean_qbar(self):
        """<qbar_l(i)>, the neighbour-averaged invariant, over particles and samples."""
        return self._per_particle(2)

    def mean_neighbours(self):
        return self._per_particle(4)

    def solid_fraction(self):
        """Fraction of particles with at least min_connections solid bonds, over the samples."""
        return self._per_particle(6)

    def global_order(self):
        """The global order parameter (the invariant of the n_i-weighted mean of q_lm), averaged over the samples."""
        if self.nsamples == 0:
            raise ValueError("no sample yet")
        return float(self.sum_fr[7]) / self.nsamples

    def histogram(self, which="q"):
        """(bin centres, density normalised to integral 1 over [0, 1], counts) of `which`: "q" or "qbar"; for "neighbours"
        or "connections" the centres are 0..32 (the last bin holds everything above) and the density sums to 1."""
        if which in ("q", "qbar"):
            counts = self.hist_q if which == "q" else self.hist_qbar
            tot = counts.sum()
            dens = counts * (self.nbins / tot) if tot > 0 else np.zeros(self.nbins)
            return self.centres.copy(), dens, counts.copy()
        if which in ("neighbours", "connections"):
            counts = self.hist_nnb if which == "neighbours" else self.hist_conn
            tot = counts.sum()
            return np.arange(33, dtype=np.float64), (counts / tot if tot > 0 else np.zeros(33)), counts.copy()
        raise ValueError('which must be "q", "qbar", "neighbours" or "connections"')

    def series(self):
        """(steps, columns): per recorded sample, the step and <q>, <qbar>, <n>, solid fraction, global order."""
        n = max(self.n_particles, 1)
        f = self.frames
        cols = np.stack([f[:, 0] / n, f[:, 2] / n, f[:, 4] / n, f[:, 6] / n, f[:, 7]], axis=1) if len(f) else np.zeros((0, 5))
        return self.steps.copy(), cols

    def write(self, path):
        """A header with the means, then # bin q_density qbar_density count_q count_qbar, one row per bin."""
        _, dq, cq = self.histogram("q")
        _, db, cb = self.histogram("qbar")
        with open(path, "w") as io:
            io.write("# order %d r_neigh %.6f threshold %.6f min_connections %d nsamples %d\n"
                     % (self.order, self.r_neigh, self.threshold, self.min_connections, self.nsamples))
            io.write("# mean_q %.8f mean_qbar %.8f mean_neighbours %.6f solid_fraction %.8f global_order %.8f\n"
                     % (self.mean_q(), self.mean_qbar(), self.mean_neighbours(), self.solid_fraction(),
                        self.global_order()))
            io.write("# bin q_density qbar_density count_q count_qbar\n")
            for k in range(self.nbins):
                io.write("%.6f %.6e %.6e %d %d\n" % (self.centres[k], dq[k], db[k], cq[k], cb[k]))

    def write_series(self, path):
        """# step <q> <qbar> <n> solid_fraction global_order, one row per recorded sample."""
        steps, cols = self.series()
        with open(path, "w") as io:
            io.write("# step <q> <qbar> <n> solid_fraction global_order\n")
            for s, c in zip(steps, cols):
                io.write("%d %.8f %.8f %.6f %.8f %.8f\n" % ((int(s),) + tuple(c)))

    # -- run_simulation's sampler protocol: a sample at every `every`-th output step ---------------------------------
    def _begin(self, dev, run):
        self._period, self._total_steps = run.frequency * self.every, run.total_steps
        self._run_steps = self.schedule(run.total_steps, run.frequency)
        ns = len(self._run_steps) if self.nseries is None else self.nseries
        dev.boo_setup(self.r_neigh, self.order, self.nbins, self.threshold, self.min_connections, min(ns, 1 << 20))

    def _next(self, step):
        return _next_multiple(step, self._period, self._total_steps)

    def _act(self, dev, step):
        dev.boo_sample()

    def _finish(self, dev, run, pathname):
        ns, fr, hq, hb, hn, hc, series = dev.boo_read()
        self._accumulate(ns, fr, hq, hb, hn, hc, series, self._run_steps[:ns], run.n)
        if self.nsamples > 0:
            self.write(os.path.join(pathname, "bond_order.txt"))
            self.write_series(os.path.join(pathname, "bond_order_series.txt"))


def compute_bond_order(state, params, r_neigh, order=6, threshold=0.7, min_connections=7):
    """One sample of the bond-orientational order of `state`'s positions, taken on its device handle (any potential);
    returns a dict of the per-particle arrays in particle order -- neighbours, q, qbar, connections, solid (bool), qlm
    (complex, N x (l + 1) for m = 0..l; N x 1 in 2-D) -- and the scalar global_order."""
    from .simulation import _configure_device
    BondOrder(r_neigh, order=order, threshold=threshold, min_connections=min_connections)    # the argument checks
    dev = _configure_device(state, params)
    dev.upload(x=state.system.positions, images=state.images, diameters=state.diameters)
    dev.boo_setup(r_neigh, order, 1, threshold, min_connections, 1)
    dev.boo_sample()
    nnb, q, qbar, nconn = dev.boo_particles()
    _, fr, _, _, _, _, _ = dev.boo_read()
    return dict(neighbours=nnb, q=q, qbar=qbar, connections=nconn, solid=nconn >= int(min_connections),
                qlm=dev.boo_qlm(), global_order=float(fr[7]))


# ---------------------------------------------------------------------------------------------------------------------
# Clusters: the connected components of the bond graph (two members closer than r_bond are bonded), sampled on the
# device (md_cluster_*) from the positions and the neighbour rows the handle already holds.  members="all": every
# particle (droplets, gels: the size distribution n(s), the weight-average size).  members="solid": the solid particles of
# the bond-order sampler's frame of the same step -- the largest one is ten Wolde, Ruiz-Montero and Frenkel's n_max.
# Everything is an integer and a function of the frame alone.

_CLUSTER_FR = ("members", "clusters", "largest", "second_largest", "directed_bonds", "sum_size2", "largest_label",
               "singletons")
_CLUSTER_MEMBERS = {"all": 0, "solid": 1}


class ClusterAnalysis:
    """Cluster statistics, accumulated on the device until reset().

    r_bond: the bond length (<= the list cutoff of the handle).  members: "all" or "solid" (then run_simulation needs a
    bond_order= as well, sampled at the same steps).  Passed to run_simulation(..., clusters=...), it takes a sample at
    every `every`-th output step; clusters larger than max_size are counted in the histogram's last entry; `nseries` rows
    of the per-sample series are kept (default: one per sample of the run).

    Fields: nsamples, sum_fr (the 8 frame entries added over the samples: members, clusters, largest, second largest,
    directed bonds, sum of size^2, the label of the largest -- whose sum means nothing -- and size-1 clusters), hist_size
    (max_size + 1 counts of clusters by size), steps and frames (the series: the step and the frame vector of each
    recorded sample)."""

    def __init__(self, r_bond, members="all", every=1, max_size=1024, nseries=None):
        r_bond = float(r_bond)
        if not (r_bond > 0.0 and math.isfinite(r_bond)):
            raise ValueError("r_bond must be finite and > 0")
        if members not in _CLUSTER_MEMBERS:
            raise ValueError('members must be "all" or "solid"')
        if int(every) != every or int(every) < 1:
            raise ValueError("every must be a positive integer")
        if int(max_size) != max_size or not 1 <= int(max_size) <= 65536:
            raise ValueError("max_size must be in 1..65536")
        if nseries is not None and (int(nseries) != nseries or not 0 <= int(nseries) <= 1 << 20):
            raise ValueError("nseries must be in 0..1048576")
        self.r_bond, self.members, self.every, self.max_size = r_bond, members, int(every), int(max_size)
        self.nseries = None if nseries is None else int(nseries)
        self.reset()

    def reset(self):
        self.nsamples = 0
        self.sum_fr = np.zeros(8, dtype=np.int64)
        self.hist_size = np.zeros(self.max_size + 1, dtype=np.int64)
        self.steps = np.zeros(0, dtype=np.int64)
        self.frames = np.zeros((0, 8), dtype=np.int64)

    def schedule(self, total_steps, frequency):
        """The steps of one run at which a sample is taken: the multiples of frequency * every below total_steps."""
        return list(range(0, int(total_steps), int(frequency) * self.every))

    def _accumulate(self, nsamples, sum_fr, hist_size, series, steps):
        self.nsamples += int(nsamples)
        self.sum_fr += np.asarray(sum_fr, dtype=np.int64).reshape(8)
        self.hist_size += np.asarray(hist_size, dtype=np.int64).reshape(self.max_size + 1)
        series = np.asarray(series, dtype=np.int64).reshape(-1, 8)
        steps = np.asarray(steps, dtype=np.int64)[: len(series)]
        self.frames = np.concatenate([self.frames, series[: len(steps)]])
        self.steps = np.concatenate([self.steps, steps])

    # -- results ----------------------------------------------------------------------------------------------------
    def _mean(self, k):
        if self.nsamples == 0:
            raise ValueError("no sample yet")
        return float(self.sum_fr[k]) / self.nsamples

    def mean_largest(self):
        """<n_max>: the size of the largest cluster, averaged over the samples."""
        return self._mean(2)

    def mean_clusters(self):
        """The number of clusters, averaged over the samples."""
        return self._mean(1)

    def mean_members(self):
        return self._mean(0)

    def weight_average_size(self):
        """sum_s s^2 n(s) / sum_s s n(s) over all samples (0 when there was no member)."""
        if self.nsamples == 0:
            raise ValueError("no sample yet")
        return float(self.sum_fr[5]) / float(self.sum_fr[0]) if self.sum_fr[0] > 0 else 0.0

    def size_distribution(self):
        """(s, n(s)): the sizes 0..max_size and the number of clusters of that size per sample; the last entry also holds
        every larger cluster, entry 0 is 0."""
        if self.nsamples == 0:
            raise ValueError("no sample yet")
        return np.arange(self.max_size + 1, dtype=np.int64), self.hist_size / float(self.nsamples)

    def series(self):
        """(steps, frames): per recorded sample, the step and the eight frame entries (int64)."""
        return self.steps.copy(), self.frames.copy()

    def write(self, path):
        """A header with the means, then # s n(s), one row per size 1..max_size (the last row holds everything larger)."""
        s, ns = self.size_distribution()
        with open(path, "w") as io:
            io.write("# members %s r_bond %.6f max_size %d nsamples %d\n"
                     % (self.members, self.r_bond, self.max_size, self.nsamples))
            io.write("# mean_members %.6f mean_clusters %.6f mean_largest %.6f weight_average_size %.6f\n"
                     % (self.mean_members(), self.mean_clusters(), self.mean_largest(), self.weight_average_size()))
            io.write("# s n(s)\n")
            for k in range(1, self.max_size + 1):
                io.write("%d %.6e\n" % (s[k], ns[k]))

    def write_series(self, path):
        """# step and the eight frame entries, one row per recorded sample."""
        with open(path, "w") as io:
            io.write("# step " + " ".join(_CLUSTER_FR) + "\n")
            for s, f in zip(self.steps, self.frames):
                io.write("%d %s\n" % (int(s), " ".join("%d" % int(v) for v in f)))

    # -- run_simulation's sampler protocol: a sample at every `every`-th output step ---------------------------------
    def _begin(self, dev, run):
        self._period, self._total_steps = run.frequency * self.every, run.total_steps
        self._run_steps = self.schedule(run.total_steps, run.frequency)
        ns = len(self._run_steps) if self.nseries is None else self.nseries
        dev.cluster_setup(self.r_bond, _CLUSTER_MEMBERS[self.members], self.max_size, min(ns, 1 << 20))

    def _next(self, step):
        return _next_multiple(step, self._period, self._total_steps)

    def _act(self, dev, step):
        dev.cluster_sample()

    def _finish(self, dev, run, pathname):
        ns, fr, hist, series = dev.cluster_read()
        self._accumulate(ns, fr, hist, series, self._run_steps[:ns])
        if self.nsamples > 0:
            self.write(os.path.join(pathname, "clusters.txt"))
            self.write_series(os.path.join(pathname, "clusters_series.txt"))


def compute_clusters(state, params, r_bond, members="all", bond_order=None):
    """One sample of the clusters of `state`'s positions, taken on its device handle (any potential); returns (labels,
    sizes, fr): per particle the smallest particle id of its cluster and the cluster's size (-1 and 0 for a non-member), and
    the frame vector (int64[8]: members, clusters, largest, second largest, directed bonds, sum of size^2, the label of the
    largest, size-1 clusters).  members="solid" needs a BondOrder (bond_order=): it is sampled first, on the same frame."""
    from .simulation import _configure_device
    ClusterAnalysis(r_bond, members=members)                # the argument checks
    if members == "solid" and not isinstance(bond_order, BondOrder):
        raise ValueError('members="solid" needs bond_order=BondOrder(...)')
    dev = _configure_device(state, params)
    dev.upload(x=state.system.positions, images=state.images, diameters=state.diameters)
    if members == "solid":
        dev.boo_setup(bond_order.r_neigh, bond_order.order, 1, bond_order.threshold, bond_order.min_connections, 0)
        dev.boo_sample()
    dev.cluster_setup(r_bond, _CLUSTER_MEMBERS[members], 1, 1)
    dev.cluster_sample()
    labels, sizes = dev.cluster_particles()
    _, fr, _, _ = dev.cluster_read()
    return labels, sizes, fr


# ---------------------------------------------------------------------------------------------------------------------
# Cage-relative dynamics and bond breaking, sampled on the device (md_cage_*): displacements measured relative to the
# mean displacement of the neighbours a particle had at the time origin, and the fraction of origin bonds that survive.

class CageDynamics(_Scheduled):
    """Cage-relative self dynamics and the bond-breaking correlation, accumulated on the device over the samples of a
    schedule until reset().

    r_neigh: particles closer than r_neigh at an origin are neighbours (bonded); r_break >= r_neigh (default r_neigh): a
    bond counts as broken at a sample when it is at least r_break long.  scaled=True multiplies both radii by
    sigma_ij = (sigma_i + sigma_j) / 2 per pair.  r_neigh (times the largest diameter if scaled) must not exceed the list
    cutoff of the handle.  max_neighbours <= 32 entries are kept per particle: more neighbours than that is an error at the
    end of the run (a truncated cage would bias every column).  q: up to 16 wavenumbers for the cage-relative F_s(q, t).
    The schedule (lags, origin_every) is SelfDynamics': log-time by default, samples before the new origin at a shared step.

    Fields: lags, nsamples (per lag), sums (per lag: sum d2, sum d4, sum s(q) per q, of Del^CR), counts (per lag: particles
    with neighbours, sum n_i, surviving bonds), hist_broken (per lag: particles by their number of broken bonds, 0..32)."""
    _prefix = "cage"

    def __init__(self, r_neigh, r_break=None, scaled=False, max_neighbours=16, q=(2.0 * math.pi,), lags=None,
                 origin_every=None):
        r_neigh = float(r_neigh)
        if not (r_neigh > 0.0 and math.isfinite(r_neigh)):
            raise ValueError("r_neigh must be finite and > 0")
        r_break = r_neigh if r_break is None else float(r_break)
        if not (math.isfinite(r_break) and r_break >= r_neigh):
            raise ValueError("r_break must be finite and >= r_neigh")
        if int(max_neighbours) != max_neighbours or not 1 <= int(max_neighbours) <= 32:
            raise ValueError("max_neighbours must be in 1..32")
        q = _check_q(q)
        nl = self._set_schedule(lags, origin_every)
        self.r_neigh, self.r_break, self.scaled, self.max_neighbours = r_neigh, r_break, bool(scaled), int(max_neighbours)
        self.q = q
        self.sums = np.zeros((nl, 2 + q.size))
        self.counts = np.zeros((nl, 3), dtype=np.int64)
        self.hist_broken = np.zeros((nl, 33), dtype=np.int64)
        self.dimension = 3
        self.dt = 1.0

    def reset(self):
        self.nsamples[:] = 0
        self.sums[:] = 0.0
        self.counts[:] = 0
        self.hist_broken[:] = 0

    # -- results ----------------------------------------------------------------------------------------------------
    def _accumulate(self, nsamples, sums, counts, hist_broken, dimension, dt):
        self.nsamples += np.asarray(nsamples, dtype=np.int64)
        self.sums += np.asarray(sums, dtype=np.float64)
        self.counts += np.asarray(counts, dtype=np.int64)
        self.hist_broken += np.asarray(hist_broken, dtype=np.int64)
        self.dimension, self.dt = int(dimension), float(dt)

    def _per(self, col):
        cnt = self.counts[:, 0].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(cnt > 0, self.sums[:, col] / cnt, np.nan)

    def msd(self):
        """<|Del^CR|^2> per lag over the particles that had neighbours; nan where a lag has none."""
        return self._per(0)

    def alpha2(self):
        """Non-Gaussian parameter d <d^4> / ((d + 2) <d^2>^2) - 1 of the cage-relative displacement, per lag."""
        d = self.dimension
        with np.errstate(invalid="ignore", divide="ignore"):
            return d * self._per(1) / ((d + 2) * self.msd() ** 2) - 1.0

    def fs(self):
        """Cage-relative F_s(q, t), (nlags, nq): sum s / (d count)."""
        cnt = self.counts[:, 0].astype(np.float64)[:, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(cnt > 0, self.sums[:, 2:] / (self.dimension * cnt), np.nan)

    def bond_correlation(self):
        """C_B(t) per lag: surviving bonds / origin bonds (directed); nan where a lag has no bond."""
        nb = self.counts[:, 1].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(nb > 0, self.counts[:, 2] / nb, np.nan)

    def broken_distribution(self):
        """(nlags, 33): the fraction of particles (with neighbours) that lost b = 0..32 bonds, per lag."""
        cnt = self.counts[:, 0].astype(np.float64)[:, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(cnt > 0, self.hist_broken / cnt, np.nan)

    def write(self, path, dt=None):
        """# lag time msd_cr alpha2_cr Fs_cr(q=..)... C_B nsamples, one row per lag that has a sample, time = lag dt."""
        dt = self.dt if dt is None else float(dt)
        msd, a2, fs, cb = self.msd(), self.alpha2(), self.fs(), self.bond_correlation()
        fmt = "%d %.6e %.6e %.6e" + " %.6e" * self.q.size + " %.6e %d\n"
        with open(path, "w") as io:
            io.write("# lag time msd_cr alpha2_cr" + "".join(" Fs_cr(q=%.6g)" % v for v in self.q) + " C_B nsamples\n")
            for k, l in enumerate(self.lags):
                if self.nsamples[k] > 0:
                    io.write(fmt % ((int(l), l * dt, msd[k], a2[k]) + tuple(fs[k]) + (cb[k], int(self.nsamples[k]))))

    # -- run_simulation's sampler protocol: the stops of schedule() (_next and _act are _Scheduled's) -------------------
    def _begin(self, dev, run):
        self._stops, self._events = self.schedule(run.total_steps)
        dev.cage_setup(self.nslots, len(self.lags), self.r_neigh, self.r_break, self.scaled, self.max_neighbours, self.q)

    def _finish(self, dev, run, pathname):
        ns, sums, counts, hist, overflow = dev.cage_read()
        if overflow != 0:
            raise ValueError(f"CageDynamics: {int(overflow)} neighbours did not fit max_neighbours = {self.max_neighbours} "
                             "entries per particle at the origins of this run: raise max_neighbours (at most 32) or lower "
                             "r_neigh; nothing was accumulated")
        self._accumulate(ns, sums, counts, hist, run.dim, run.dt)
        self.write(os.path.join(pathname, "cage.txt"))


# ---------------------------------------------------------------------------------------------------------------------
# Four-point dynamics, sampled on the device (md_chi4_*): the self overlap Q(t0, t) = sum_i w_i of the particles that
# moved less than a, its variance chi4(t) and the structure factor S4(q, t) of the slow particles.

class FourPoint(_Scheduled, _WaveVectors):
    """Dynamic heterogeneity from the four-point functions of the self overlap, accumulated on the device over the samples
    of a schedule until reset().

    a: particle i is slow at lag t, w_i = 1, iff |x_i(t0 + t) - x_i(t0)| < a (unwrapped displacement, strict).
    Q = sum_i w_i; overlap() = <Q> / N; chi4() = (<Q^2> - <Q>^2) / N; S4(q, t) = <|W(q)|^2> / N with
    W(q) = sum_i w_i exp(+i q.x_i(t0)) on the wave vectors select_wave_vectors(unitcell, q_max, dq, max_per_bin, seed) of
    the cell the sampler is first used on (at most 4096); q_max=None samples chi4 only.  The schedule (lags, origin_every)
    is SelfDynamics': log-time by default, explicit lags need origin_every (at most 64 origin slots), samples before the
    new origin at a shared step.  An origin costs N d 20 bytes on the device with vectors, N d 12 without.

    What chi4 means here: it is the variance of Q at fixed N in the ensemble the run samples, so NVE, NVT and Brownian
    runs each miss the contributions of the quantities they hold fixed (density, and energy or temperature); S4(q -> 0, t)
    of the same run is the estimate without that loss.  The overlap is the SELF overlap (a particle against its own
    origin position, not against any particle's).  A cage-relative variant for 2-D is not provided.

    Fields: lags, nsamples (per lag), sum_q, sum_q2 (per lag, Python integers), n (nvec, d), qvec, bin, q (mean |q| of a
    bin), nvectors (per bin), sum_s4 (nlags, nvec: sum |W|^2)."""
    _prefix = "chi4"
    _max_vectors = 4096
    _too_many = "{} wave vectors selected; FourPoint takes at most 4096 (lower q_max or max_per_bin, or widen dq)"

    def __init__(self, a, q_max=None, dq=None, max_per_bin=16, seed=0, lags=None, origin_every=None):
        a = float(a)
        if not (a > 0.0 and math.isfinite(a)):
            raise ValueError("a must be finite and > 0")
        if q_max is not None:
            q_max = float(q_max)
            if not (q_max > 0.0 and math.isfinite(q_max)):
                raise ValueError("q_max must be finite and > 0 (or None for chi4 only)")
        elif dq is not None:
            raise ValueError("dq needs q_max")
        if dq is not None and not (float(dq) > 0.0 and math.isfinite(float(dq))):
            raise ValueError("dq must be finite and > 0")
        if int(max_per_bin) < 1:
            raise ValueError("max_per_bin must be >= 1")
        nl = self._set_schedule(lags, origin_every)
        self.a, self.q_max, self.dq, self.max_per_bin, self.seed = a, q_max, dq, int(max_per_bin), seed
        self.sum_q = np.array([0] * nl, dtype=object)
        self.sum_q2 = np.array([0] * nl, dtype=object)
        self.unitcell = None
        self.n = self.qvec = self.bin = self.q = self.nvectors = self.sum_s4 = None
        self.n_particles = 0
        self.dt = 1.0

    def _zero_vector_sums(self, nvec):
        self.sum_s4 = np.zeros((len(self.lags), nvec))

    def reset(self):
        """Forget the samples and the wave vectors (the next use selects them again, for the cell it meets)."""
        self.nsamples[:] = 0
        self.sum_q[:] = 0
        self.sum_q2[:] = 0
        self.unitcell = None
        self.n = self.qvec = self.bin = self.q = self.nvectors = self.sum_s4 = None

    # -- results ----------------------------------------------------------------------------------------------------
    def _accumulate(self, nsamples, sum_q, sum_q2, s4, n_particles, dt):
        self.nsamples += np.asarray(nsamples, dtype=np.int64)
        for k in range(len(self.lags)):
            self.sum_q[k] += int(sum_q[k])
            self.sum_q2[k] += int(sum_q2[k])
        if self.sum_s4 is not None:
            self.sum_s4 += np.asarray(s4, dtype=np.float64)
        self.n_particles, self.dt = int(n_particles), float(dt)

    def overlap(self):
        """<Q> / N per lag: sum Q / (ns N); nan where a lag has no sample."""
        return np.array([int(sq) / (int(ns) * self.n_particles) if ns > 0 else np.nan
                         for ns, sq in zip(self.nsamples, self.sum_q)], dtype=np.float64)

    def chi4(self):
        """chi4 per lag: (ns sum Q^2 - (sum Q)^2) / (ns^2 N), the numerator formed in integers (nothing cancels in floating
        point); nan where a lag has no sample."""
        out = np.full(len(self.lags), np.nan)
        for k, ns in enumerate(self.nsamples):
            ns = int(ns)
            if ns > 0:
                out[k] = (ns * int(self.sum_q2[k]) - int(self.sum_q[k]) ** 2) / (ns * ns * self.n_particles)
        return out

    def s4_vectors(self):
        """S4(q_v, t), (nlags, nvec): sum |W|^2 / (ns N); nan where a lag has no sample."""
        if self.sum_s4 is None:
            raise ValueError("no wave vectors: give q_max (and use the sampler once) for S4")
        ns = self.nsamples.astype(np.float64)[:, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(ns > 0, self.sum_s4 / (ns * self.n_particles), np.nan)

    def s4(self):
        """S4(q, t), (nlags, nbins): sum over the bin's vectors of sum |W|^2 / (ns N M_bin)."""
        sv = self.s4_vectors()
        return np.array([self._binned(sv[k]) for k in range(sv.shape[0])]).reshape(sv.shape[0], self.q.size)

    def write(self, path, dt=None):
        """# lag time Q/N chi4 nsamples, one row per lag that has a sample, time = lag dt."""
        dt = self.dt if dt is None else float(dt)
        ov, c4 = self.overlap(), self.chi4()
        with open(path, "w") as io:
            io.write("# lag time Q/N chi4 nsamples\n")
            for k, l in enumerate(self.lags):
                if self.nsamples[k] > 0:
                    io.write("%d %.6e %.6e %.6e %d\n" % (int(l), l * dt, ov[k], c4[k], int(self.nsamples[k])))

    def write_s4(self, path, dt=None):
        """One block per lag that has a sample, lines `lag time q S4 nvectors nsamples`, a blank line between blocks."""
        dt = self.dt if dt is None else float(dt)
        s4 = self.s4()
        _write_blocks(path, "# lag time q S4 nvectors nsamples\n", self.lags, self.nsamples, lambda k, l: (
            "%d %.6e %.6f %.6e %d %d\n" % (int(l), l * dt, self.q[b], s4[k, b], self.nvectors[b], int(self.nsamples[k]))
            for b in range(self.q.size)))

    # -- run_simulation's sampler protocol: the stops of schedule() (_next and _act are _Scheduled's) -------------------
    def _begin(self, dev, run):
        self._stops, self._events = self.schedule(run.total_steps)
        self._select(run.unitcell)
        dev.chi4_setup(self.a, self.n, self.nslots, len(self.lags))

    def _finish(self, dev, run, pathname):
        ns, sq, sq2, s4 = dev.chi4_read()
        self._accumulate(ns, sq, sq2, s4, run.n, run.dt)
        self.write(os.path.join(pathname, "chi4.txt"))
        if self.sum_s4 is not None:
            self.write_s4(os.path.join(pathname, "s4.txt"))


# ---------------------------------------------------------------------------------------------------------------------
# Marked pair correlations, sampled on the device (md_mpc_*): the orientational correlation function -- g6(r) of psi_6
# in 2-D, whose decay (exponential, algebraic, constant) tells the liquid, the hexatic and the solid apart, G_l(r) of
# q_lm in 3-D -- and the spatial correlation of any per-particle field.  The device accumulates integers (pair counts
# and sums of terms quantised to tmax 2^-31), so a sample is a function of the frame and the marks alone.

def _pair_density(counts, nsamples, n_particles, volume, edges, dimension):
    """RadialDistribution.g's normalisation: counts / (nsamples N (N - 1) / (2 V) V_k)."""
    if nsamples == 0 or n_particles < 2:
        return np.zeros(len(counts))
    ideal = nsamples * n_particles * (n_particles - 1.0) / (2.0 * volume) * shell_volumes(edges, dimension)
    return counts / ideal


def _per_pair(sums, counts, quantum):
    """sums * quantum / counts, nan where a bin is empty."""
    out = np.full(len(counts), np.nan)
    np.divide(np.asarray(sums, dtype=np.float64) * quantum, counts, out=out, where=np.asarray(counts) > 0)
    return out


class OrientationalCorrelation:
    """The orientational correlation function of the bond-order sampler's marks on `nbins` bins of width r_max / nbins,
    accumulated on the device until reset(): G(r) = <t_ij>_r with t_ij = 4 pi / (2l + 1) sum_m q_lm(i) q_lm*(j) in 3-D and
    Re psi_k(i) psi_k*(j) in 2-D, averaged over the pairs at distance r; g(r); and g_l(r) = G(r) g(r).

    Passed to run_simulation(..., bond_order=..., orientational=...), it takes a sample at every `every`-th output step,
    after the bond-order sample of the same step: `every` must be a multiple of bond_order.every.

    Fields: edges, r (bin centres), counts (pairs per bin, summed over the samples), sums (the device's acc_sum: the
    integer terms, one double add per sample), self_sum (sum over samples of sum_i I_ii), tmax, nsamples, order, r_neigh."""

    def __init__(self, r_max, nbins, every=1):
        r_max = float(r_max)
        if not (r_max > 0.0 and math.isfinite(r_max)):
            raise ValueError("r_max must be finite and > 0")
        if int(nbins) != nbins or not 1 <= int(nbins) <= 4096:
            raise ValueError("nbins must be in 1..4096")
        if int(every) != every or int(every) < 1:
            raise ValueError("every must be a positive integer")
        self.r_max, self.nbins, self.every = r_max, int(nbins), int(every)
        self.edges = np.arange(self.nbins + 1, dtype=np.float64) * (r_max / self.nbins)
        self.r = 0.5 * (self.edges[:-1] + self.edges[1:])
        self.order, self.r_neigh, self.tmax = 0, 0.0, 1.0
        self.n_particles, self.volume, self.dimension = 0, 0.0, 3
        self.reset()

    def reset(self):
        self.counts = np.zeros(self.nbins, dtype=np.int64)
        self.sums = np.zeros(self.nbins)
        self.self_sum = 0.0
        self.nsamples = 0

    def _accumulate(self, nsamples, counts, sums, self_sum, tmax, n_particles, unitcell, order, r_neigh):
        if self.nsamples > 0 and float(tmax) != self.tmax:
            raise ValueError("tmax differs from the one already accumulated; reset() first")
        self.nsamples += int(nsamples)
        self.counts += np.asarray(counts, dtype=np.int64).reshape(self.nbins)
        self.sums += np.asarray(sums, dtype=np.float64).reshape(self.nbins)
        self.self_sum += float(self_sum)
        u = np.asarray(unitcell, dtype=np.float64)
        self.tmax, self.n_particles, self.volume, self.dimension = float(tmax), int(n_particles), abs(float(np.linalg.det(u))), u.shape[0]
        self.order, self.r_neigh = int(order), float(r_neigh)

    # -- results ----------------------------------------------------------------------------------------------------
    @property
    def quantum(self):
        """The value of one unit of `sums`: tmax 2^-31."""
        return self.tmax * 2.0 ** -31

    def g(self):
        """The radial distribution function of the same pairs."""
        return _pair_density(self.counts, self.nsamples, self.n_particles, self.volume, self.edges, self.dimension)

    def G(self):
        """G(r): the mean of t_ij over the pairs of a bin (nan for an empty bin); 1 in a perfect crystal."""
        return _per_pair(self.sums, self.counts, self.quantum)

    def g_l(self):
        """g_l(r) = G(r) g(r) (g6(r) for k = 6 in 2-D); 0 for an empty bin."""
        return np.where(self.counts > 0, np.nan_to_num(self.G()) * self.g(), 0.0)

    def mean_self(self):
        """<t_ii>: <q_l(i)^2> in 3-D, <|psi_k(i)|^2> in 2-D, over particles and samples."""
        if self.nsamples == 0 or self.n_particles == 0:
            raise ValueError("no sample yet")
        return self.self_sum * self.quantum / (self.nsamples * self.n_particles)

    def write(self, path):
        """A header naming the order, then # r_mid count g(r) G(r) g_l(r), one row per bin; the last line is <t_ii>."""
        g, G, gl = self.g(), self.G(), self.g_l()
        with open(path, "w") as io:
            io.write("# %s %d r_neigh %.6f tmax %.6g nsamples %d\n"
                     % ("l" if self.dimension == 3 else "k", self.order, self.r_neigh, self.tmax, self.nsamples))
            io.write("# r_mid count g(r) G(r) g_l(r)\n")
            for k in range(self.nbins):
                io.write("%.6f %d %.6f %.8f %.8f\n" % (self.r[k], self.counts[k], g[k], G[k], gl[k]))
            io.write("# <t_ii> %.8f\n" % self.mean_self())

    # -- run_simulation's sampler protocol: a sample at every `every`-th output step, after bond_order's ----------------
    def _begin(self, dev, run):
        bo = getattr(run, "bond_order", None)
        if bo is None:
            raise ValueError("orientational= needs bond_order= in the same run: its marks are the bond-order frame's")
        if self.every % bo.every != 0:
            raise ValueError("orientational.every must be a multiple of bond_order.every: every sample needs the "
                             "bond-order sample of its step")
        self._period, self._total_steps = run.frequency * self.every, run.total_steps
        self._order, self._r_neigh = bo.order, bo.r_neigh
        dev.mpc_setup(self.r_max, self.nbins)

    def _next(self, step):
        return _next_multiple(step, self._period, self._total_steps)

    def _act(self, dev, step):
        dev.mpc_sample()

    def _finish(self, dev, run, pathname):
        ns, cnt, sums, own, tmax, err = dev.mpc_read()
        if err:
            raise RuntimeError("the orientational correlation sampler reports range_error = %d (1: a term beyond tmax, "
                               "2: a bin with 2^31 pairs in one sample)" % err)
        self._accumulate(ns, cnt, sums, own, tmax, run.n, run.unitcell, self._order, self._r_neigh)
        if self.nsamples > 0:
            self.write(os.path.join(pathname, "orient_corr.txt"))


def compute_orientational_correlation(state, params, r_neigh, order, r_max, nbins):
    """One sample of the orientational correlation of `state`'s positions, taken on its device handle (any potential):
    the bond order within r_neigh (l in 3-D, k in 2-D) first, then the pair walk out to r_max on the same frame; returns
    an OrientationalCorrelation."""
    from .simulation import _configure_device
    BondOrder(r_neigh, order=order)                         # the argument checks
    oc = OrientationalCorrelation(r_max, nbins)
    dev = _configure_device(state, params)
    dev.upload(x=state.system.positions, images=state.images, diameters=state.diameters)
    dev.boo_setup(r_neigh, order, 1, 0.7, 7, 0)
    dev.boo_sample()
    dev.mpc_setup(oc.r_max, oc.nbins)
    dev.mpc_sample()
    ns, cnt, sums, own, tmax, err = dev.mpc_read()
    if err:
        raise RuntimeError("range_error = %d" % err)
    oc._accumulate(ns, cnt, sums, own, tmax, dev.n, state.unitcell, order, r_neigh)
    return oc


def default_tmax(marks, weights):
    """The next power of two >= sum_c |w_c| max_i |a_c(i)|^2 (1 when every mark is zero): no term can exceed it."""
    m = np.abs(np.asarray(marks, dtype=np.float64))
    bound = float(np.dot(np.abs(np.asarray(weights, dtype=np.float64)), m.max(axis=0) ** 2)) if m.size else 0.0
    if not math.isfinite(bound):
        raise ValueError("marks and weights must be finite")
    return 2.0 ** math.ceil(math.log2(bound)) if bound > 0.0 else 1.0


def compute_marked_correlation(state, params, marks, r_max, nbins, weights=None, tmax=None):
    """One sample of the spatial correlation of the per-particle field `marks` (N, or N x NC with NC <= 3, in particle
    order) over `state`'s positions, taken on its device handle: the pair {i, j} contributes t_ij = sum_c weights[c]
    a_c(i) a_c(j) (weights default to 1) to its distance bin.  tmax bounds |t_ij| (default: default_tmax).  Returns a dict:
    r, edges, count (pairs per bin), sum (the integer terms per bin), self (sum_i I_ii), tmax, quantum (tmax 2^-31), C
    (sum quantum / count, nan for an empty bin: C_vv(r) for velocities), g (the radial distribution of the same pairs)."""
    m = np.ascontiguousarray(marks, dtype=np.float64)
    m = m.reshape(len(m), -1)
    w = np.ones(m.shape[1]) if weights is None else np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    if w.size != m.shape[1]:
        raise ValueError("one weight per mark component")
    tmax = default_tmax(m, w) if tmax is None else float(tmax)
    dev = state.system.device
    dev.upload(x=state.system.positions, images=state.images)
    dev.mpc_setup(r_max, nbins, weights=w, tmax=tmax)
    dev.mpc_marks(m)
    dev.mpc_sample()
    cnt, tot, own = dev.mpc_last()
    _, _, _, _, tmax, err = dev.mpc_read()
    if err:
        raise RuntimeError("range_error = %d: a term exceeds tmax = %g" % (err, tmax))
    edges = np.arange(int(nbins) + 1, dtype=np.float64) * (float(r_max) / int(nbins))
    u = np.asarray(state.unitcell, dtype=np.float64)
    quantum = tmax * 2.0 ** -31
    return dict(r=0.5 * (edges[:-1] + edges[1:]), edges=edges, count=cnt, sum=tot, self=own, tmax=tmax, quantum=quantum,
                C=_per_pair(tot, cnt, quantum),
                g=_pair_density(cnt, 1, dev.n, abs(float(np.linalg.det(u))), edges, u.shape[0]))
