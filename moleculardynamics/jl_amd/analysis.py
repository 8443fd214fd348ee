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
