"""Structure of a simulated configuration: the radial distribution function g(r), sampled on the device.

The pair histogram itself is accumulated by libmdhip (md_rdf_*: integer counts, exact and independent of the order the
pairs are visited in); this module keeps the samples, normalises them and writes them out.
"""
import math

import numpy as np


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
        d = self.dimension if dimension is None else dimension
        e = self.edges
        if d == 3:
            return 4.0 * math.pi / 3.0 * (e[1:] ** 3 - e[:-1] ** 3)
        return math.pi * (e[1:] ** 2 - e[:-1] ** 2)

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


def _start(dev, rdf):
    dev.rdf_setup(rdf.r_max, rdf.nbins)


def _collect(dev, rdf, n_particles, unitcell):
    counts, ns = dev.rdf_read()
    rdf._accumulate(counts, ns, n_particles, unitcell)


def compute_rdf(state, params, r_max, nbins):
    """One sample of g(r) of `state`'s positions, taken on its device handle; returns a RadialDistribution."""
    rdf = RadialDistribution(r_max, nbins)
    dev = state.system.device
    dev.upload(x=state.system.positions, images=state.images)
    _start(dev, rdf)
    dev.rdf_sample()
    _collect(dev, rdf, dev.n, state.unitcell)
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


class SelfDynamics:
    """Self dynamics of the particles, accumulated on the device over the samples of a schedule until reset().

    q: up to 16 wavenumbers for F_s(q, t).  r_max, nbins: the van Hove histogram (nbins = 0: none).  The schedule:
    lags=None is the reference's log-time schedule (origins at every multiple of maxlog = floor(1.35^40), samples at
    j maxlog + l for the 39 distinct lags l = floor(1.35^i)); explicit positive `lags` need `origin_every` = E (origins at
    m E, samples at m E + l, ceil(max l / E) origin slots used round-robin, at most 64).  At a step that has both, the
    samples are taken before the new origin is stored.  Each run_simulation call restarts the schedule at step 0; the
    samples accumulate here across calls.

    Fields: lags, nsamples (per lag), sums (per lag: sum d2, sum d4, sum s(q) per q), hist (per lag and bin), edges, r."""

    def __init__(self, q=(2.0 * math.pi,), r_max=None, nbins=0, lags=None, origin_every=None):
        q = np.array([float(v) for v in np.atleast_1d(np.asarray(q, dtype=np.float64))], dtype=np.float64)
        if q.size > 16:
            raise ValueError("at most 16 wavenumbers q")
        if not np.all(np.isfinite(q)):
            raise ValueError("every q must be finite")
        nbins = int(nbins)
        if not 0 <= nbins <= 8192:
            raise ValueError("nbins must be in 0..8192")
        if nbins > 0:
            if r_max is None or not (float(r_max) > 0.0 and math.isfinite(float(r_max))):
                raise ValueError("r_max must be finite and > 0 when nbins > 0")
            r_max = float(r_max)
        else:
            r_max = None if r_max is None else float(r_max)
        if lags is None:
            if origin_every is not None:
                raise ValueError("origin_every needs explicit lags (the default is the log-time schedule)")
            self.maxlog, lag_list, _ = _log_schedule()
            self.origin_every = None
            self.nslots = 1
        else:
            lag_list = [int(v) for v in np.atleast_1d(lags)]
            if not lag_list or any(v < 1 for v in lag_list) or any(int(v) != v for v in np.atleast_1d(lags)):
                raise ValueError("lags must be positive integers")
            if len(set(lag_list)) != len(lag_list):
                raise ValueError("lags must be distinct")
            if origin_every is None or int(origin_every) != origin_every or int(origin_every) < 1:
                raise ValueError("explicit lags need origin_every, a positive integer")
            self.maxlog = None
            self.origin_every = int(origin_every)
            self.nslots = -(-max(lag_list) // self.origin_every)
            if self.nslots > 64:
                raise ValueError(f"ceil(max lag / origin_every) = {self.nslots} origin slots; at most 64")
        self.q, self.r_max, self.nbins = q, r_max, nbins
        self.lags = np.array(lag_list, dtype=np.int64)
        nl = len(lag_list)
        self.nsamples = np.zeros(nl, dtype=np.int64)
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

    # -- schedule ---------------------------------------------------------------------------------------------------
    def schedule(self, total_steps):
        """(stops, events) for one run of `total_steps` steps: the sorted steps where the sampler acts, and per stop a
        pair (samples, origin): samples = [(slot, row), ...] in origin order, origin = the slot the frame is stored in
        after them, or None."""
        T = int(total_steps)
        events = {}

        def ev(s):
            return events.setdefault(s, ([], None))

        if self.maxlog is not None:
            maxlog, _, stops = _log_schedule()
            row = {int(l): k for k, l in enumerate(self.lags)}
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
            E, ns = self.origin_every, self.nslots
            for m in range(0, (T + E - 1) // E):
                o = m * E
                smp, _ = ev(o)
                events[o] = (smp, m % ns)
            for m in range(0, (T + E - 1) // E):
                for k, l in enumerate(self.lags):
                    s = m * E + int(l)
                    if s < T:
                        ev(s)[0].append((m % ns, k, m))
            for s, (smp, org) in events.items():
                smp.sort(key=lambda t: (t[2], t[1]))
                events[s] = ([(a, b) for a, b, _ in smp], org)
        stops = sorted(events)
        return stops, events

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
        d = self.dimension if dimension is None else dimension
        e = self.edges
        if d == 3:
            return 4.0 * math.pi / 3.0 * (e[1:] ** 3 - e[:-1] ** 3)
        return math.pi * (e[1:] ** 2 - e[:-1] ** 2)

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
        with open(path, "w") as io:
            io.write("# lag r G_s count\n")
            first = True
            for k, l in enumerate(self.lags):
                if self.nsamples[k] == 0:
                    continue
                if not first:
                    io.write("\n")
                first = False
                for b in range(self.nbins):
                    io.write("%d %.6f %.6e %d\n" % (int(l), self.r[b], g[k, b], self.hist[k, b]))


def _dyn_start(dev, dyn):
    dev.dyn_setup(dyn.nslots, len(dyn.lags), dyn.q, dyn.r_max or 0.0, dyn.nbins)


def _dyn_act(dev, event):
    """The sampler's work at one stop: the samples, then the origin (the frame is exported once for all samples)."""
    smp, org = event
    if smp:
        dev.dyn_sample([a for a, _ in smp], [b for _, b in smp])
    if org is not None:
        dev.dyn_origin(org)


def _dyn_collect(dev, dyn, n_particles, dimension, dt):
    ns, sums, hist = dev.dyn_read()
    dyn._accumulate(ns, sums, hist, n_particles, dimension, dt)
