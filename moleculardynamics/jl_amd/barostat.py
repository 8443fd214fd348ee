"""Constant pressure: stochastic cell rescaling (Bernetti and Bussi, J. Chem. Phys. 153, 114107, 2020), the partner of the
stochastic velocity rescaling thermostat (thermostat.py), on the device's md_scale_cell.  New
relative to the reference, which has no barostat.

The barostat is first order: no extra dynamical variable, one Gaussian number per coupling.  With eps = ln V, beta_T the
isothermal compressibility that sets the time scale, tau_p the relaxation time and dt_p the time between two couplings,

    d eps = -(beta_T / tau_p) (P0 - P_int) dt_p + sqrt(2 kT beta_T dt_p / (V tau_p)) xi,     mu = exp(d eps / d)

scales every length by mu and every velocity by 1 / mu.  This is the Ito form IN eps: it has no kT / V term.  (The same
process written for V, dV = -(beta_T V / tau_p)(P0 - P_int - kT / V) dt + sqrt(2 kT beta_T V / tau_p) dW, has one; Ito's
lemma for eps = ln V, d eps = dV / V - (dV)^2 / (2 V^2), cancels it against the noise's second-order term.  Either form has
the stationary density exp(-(F + P0 V) / kT) in V.)

The pressure that enters is the instantaneous one, P_int = (2 K + W) / (d V) + the potential's long-range correction, with
K, W and V of the moment, as in the paper.  (run_simulation's thermo line uses rho T with T = 2 K / nf, nf = d (N - 1):
the two differ by a factor (N - 1) / N in the kinetic part.)

StochasticCellRescaling speaks the protocol run_simulation drives its samplers and SwapMonteCarlo through (_begin / _next /
_act / _finish), but like swap it CHANGES the state: the cell, the positions, the velocities and the forces."""
import math
import os

import numpy as np

from .analysis import _next_multiple
from .types import NVT, Brownian


def crescale_factor(p_int, volume, ktemp, pressure, compressibility, tau_p, dt_p, xi, dim):
    """The length scale factor mu of one coupling (module docstring): exp(d eps / dim).  Pure; xi is the Gaussian draw
    (0 for the deterministic relaxation).  xi = 0 and p_int == pressure give exactly 1."""
    drift = -(compressibility / tau_p) * (pressure - p_int) * dt_p
    noise = math.sqrt(2.0 * ktemp * compressibility * dt_p / (volume * tau_p)) * xi
    return math.exp((drift + noise) / dim)


class StochasticCellRescaling:
    """Isotropic stochastic cell rescaling to the pressure `pressure`, after every `every`-th MD step.

    tau_p: the relaxation time of the volume; compressibility: the isothermal compressibility beta_T the coupling assumes
    (only tau_p / beta_T matters for the dynamics; a wrong guess changes the relaxation time, not the ensemble).  ktemp:
    the temperature of the noise; None takes the NVT ensemble's target temperature of that step -- NVE has none and needs
    ktemp.  stochastic=False draws no random number: the deterministic relaxation towards `pressure` (Berendsen's).

    Fields, accumulated over the runs until reset(): couplings (one dict per coupling: step, volume, density, p_int, mu,
    rows_kept -- volume and density AFTER the scale, p_int the pressure that drove it), n_couplings, sum_v, sum_v2,
    sum_p (of the volume before each coupling and of p_int); mean_volume(), var_volume(), mean_pressure()."""

    def __init__(self, pressure, tau_p, compressibility, every=10, ktemp=None, stochastic=True):
        pressure, tau_p, compressibility, every = float(pressure), float(tau_p), float(compressibility), int(every)
        if not math.isfinite(pressure):
            raise ValueError("pressure must be finite")
        if not (tau_p > 0.0 and math.isfinite(tau_p)):
            raise ValueError("tau_p must be finite and > 0")
        if not (compressibility > 0.0 and math.isfinite(compressibility)):
            raise ValueError("compressibility must be finite and > 0")
        if every < 1:
            raise ValueError("every must be >= 1")
        if ktemp is not None and not (float(ktemp) > 0.0 and math.isfinite(float(ktemp))):
            raise ValueError("ktemp must be finite and > 0 (or None)")
        self.pressure, self.tau_p, self.compressibility, self.every = pressure, tau_p, compressibility, every
        self.ktemp = None if ktemp is None else float(ktemp)
        self.stochastic = bool(stochastic)
        self.reset()

    def reset(self):
        self.couplings = []
        self.n_couplings = 0
        self.sum_v = self.sum_v2 = self.sum_p = 0.0

    def mean_volume(self):
        return self.sum_v / self.n_couplings if self.n_couplings else float("nan")

    def var_volume(self):
        if not self.n_couplings:
            return float("nan")
        m = self.sum_v / self.n_couplings
        return self.sum_v2 / self.n_couplings - m * m

    def mean_pressure(self):
        return self.sum_p / self.n_couplings if self.n_couplings else float("nan")

    def _ktemp_at(self, step):
        if self.ktemp is not None:
            return self.ktemp
        return float(self._ensemble.ktemp(step + 1))       # the target the thermostat used for this step

    def write(self, path):
        with open(path, "w") as io:
            io.write("# step volume density p_int mu rows_kept\n")
            for c in self.couplings[self._first:]:
                io.write("%d %.17g %.17g %.17g %.17g %d\n" % (c["step"], c["volume"], c["density"], c["p_int"], c["mu"],
                                                              c["rows_kept"]))

    # -- run_simulation's protocol: one coupling after every `every`-th step ---------------------------------------------
    def _begin(self, dev, run):
        ens = run.ensemble
        if isinstance(ens, Brownian):
            raise ValueError("barostat= is not available with Brownian dynamics (no velocities, no kinetic pressure)")
        if self.ktemp is None and not isinstance(ens, NVT):
            raise ValueError("barostat= with the NVE ensemble needs StochasticCellRescaling(ktemp=...): NVE has no target "
                             "temperature")
        self._ensemble = ens
        self._total_steps = run.total_steps
        self._rng = run.rng
        self._n, self._dim, self._pot = run.n, run.dim, run.potential
        self._dt_p = self.every * run.dt
        self._first = len(self.couplings)

    def _next(self, step):
        # after step s (0-based) s + 1 steps are done: the stops are the steps every - 1, 2 every - 1, ...
        s = _next_multiple(step + 1, self.every, self._total_steps + 1)
        return None if s is None else s - 1

    def _act(self, dev, step, U, W, K, volume):
        """One coupling on the frame the segment (or the swap block) left: returns dict(mu, U, W, K, rows_kept, p_int) with
        U, W of the new cell and K scaled by 1 / mu^2."""
        n, d = self._n, self._dim
        p_int = (2.0 * K + W) / (d * volume) + self._pot.pressure_lrc(n, volume)
        xi = float(self._rng.standard_normal()) if self.stochastic else 0.0
        mu = crescale_factor(p_int, volume, self._ktemp_at(step), self.pressure, self.compressibility, self.tau_p,
                             self._dt_p, xi, d)
        kept = dev.scale_cell(mu, 1.0 / mu)
        U, W = dev.compute_forces()                         # the next half-kick needs the new cell's forces
        self.n_couplings += 1
        self.sum_v += volume
        self.sum_v2 += volume * volume
        self.sum_p += p_int
        return dict(step=step, mu=mu, U=U, W=W, K=K / (mu * mu), rows_kept=int(kept), p_int=p_int)

    def _record(self, r, volume):
        """The loop's report of the volume after the coupling `r` (it owns the cell)."""
        self.couplings.append(dict(step=r["step"], volume=volume, density=self._n / volume, p_int=r["p_int"], mu=r["mu"],
                                   rows_kept=r["rows_kept"]))

    def _finish(self, dev, run, pathname):
        self.write(os.path.join(pathname, "barostat.txt"))
