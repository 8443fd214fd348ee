"""Swap Monte Carlo: diameter exchanges interleaved with blocks of molecular dynamics (Berthier, Flenner, Fullerton,
Scalliet, Singh, J. Stat. Mech. 2019), on the device (md_swap_*).

SwapMonteCarlo speaks the protocol run_simulation drives its samplers through (_begin / _next / _act / _finish, see
analysis.py), but it is no analysis object: it CHANGES the state -- the diameters, and with them the forces the next MD
step starts from."""
import math
import os

import numpy as np

from .analysis import _next_multiple
from .types import NVT, Brownian

DEFAULT_FRACTION = 0.005     # the largest measured fraction at which half the proposals are decided


class SwapMonteCarlo:
    """`rounds` rounds of swap attempts after every `every`-th MD step.

    fraction: the probability with which a particle proposes a swap in a round (its partner is drawn uniformly from the
    whole box).  max_diameter_difference: swaps between diameters further apart are not attempted (None: no limit).
    ktemp: the temperature of the Metropolis test; None takes the ensemble's target temperature at that step (NVT,
    Brownian) -- NVE has none and needs ktemp.  seed: keys the device's Philox stream; None draws it from state.rng.

    Fields, accumulated over the runs until reset(): blocks (one dict per block: step, proposed, void, lost, blocked,
    filtered, accepted, decided, du_accepted, U, W), rounds_done (the round counter: it continues across blocks and
    runs, so no round of the stream is used twice)."""

    def __init__(self, every, rounds, fraction=DEFAULT_FRACTION, max_diameter_difference=None, ktemp=None, seed=None):
        every, rounds, fraction = int(every), int(rounds), float(fraction)
        if every < 1:
            raise ValueError("every must be >= 1")
        if rounds < 1:
            raise ValueError("rounds must be >= 1")
        if not (0.0 < fraction <= 1.0):
            raise ValueError("fraction must be in (0, 1]")
        if max_diameter_difference is not None and not (float(max_diameter_difference) > 0.0):
            raise ValueError("max_diameter_difference must be > 0 (or None)")
        if ktemp is not None and not (float(ktemp) > 0.0 and math.isfinite(float(ktemp))):
            raise ValueError("ktemp must be finite and > 0 (or None)")
        self.every, self.rounds, self.fraction = every, rounds, fraction
        self.max_diameter_difference = None if max_diameter_difference is None else float(max_diameter_difference)
        self.ktemp = None if ktemp is None else float(ktemp)
        self.seed = None if seed is None else int(seed)
        self.reset()

    def reset(self):
        self.blocks = []
        self.rounds_done = 0

    def acceptance(self):
        """Accepted over decided swaps, over all blocks (0 when nothing was decided)."""
        dec = sum(b["decided"] for b in self.blocks)
        return sum(b["accepted"] for b in self.blocks) / dec if dec else 0.0

    def _ktemp_at(self, step):
        if self.ktemp is not None:
            return self.ktemp
        ens = self._ensemble
        if isinstance(ens, NVT):
            return float(ens.ktemp(step + 1))          # the target the thermostat used for this step
        return float(ens.ktemp)

    def write(self, path):
        with open(path, "w") as io:
            io.write("# step proposed blocked decided accepted acceptance dU_accepted U\n")
            for b in self.blocks[self._first_block:]:
                acc = b["accepted"] / b["decided"] if b["decided"] else 0.0
                io.write("%d %d %d %d %d %.6f %.10e %.10e\n" % (b["step"], b["proposed"], b["blocked"], b["decided"],
                                                                b["accepted"], acc, b["du_accepted"], b["U"]))

    # -- run_simulation's protocol: a block of rounds after every `every`-th step -------------------------------------
    def _begin(self, dev, run):
        ens = run.ensemble
        if self.ktemp is None and not isinstance(ens, (NVT, Brownian)):
            raise ValueError("swap= with the NVE ensemble needs SwapMonteCarlo(ktemp=...): NVE has no target temperature")
        self._ensemble = ens
        self._total_steps = run.total_steps
        self._first_block = len(self.blocks)
        if self.seed is None:
            self.seed = int(run.rng.integers(1 << 63))
        dev.swap_setup(self.fraction, self.max_diameter_difference, self.seed)

    def _next(self, step):
        # after step s (0-based) s + 1 steps are done: the stops are the steps every - 1, 2 every - 1, ...
        s = _next_multiple(step + 1, self.every, self._total_steps + 1)
        return None if s is None else s - 1

    def _act(self, dev, step):
        r = dev.swap_rounds(self.rounds, self._ktemp_at(step), first_round=self.rounds_done)
        self.rounds_done += self.rounds
        r["step"] = step
        self.blocks.append(r)
        return r

    def _finish(self, dev, run, pathname):
        self.write(os.path.join(pathname, "swap.txt"))


def swap_rounds(state, params, ktemp, rounds, fraction=DEFAULT_FRACTION, max_diameter_difference=None, seed=0,
                first_round=0):
    """`rounds` rounds of swap attempts on `state` at temperature ktemp, on its device handle with params.potential: uploads
    the positions and diameters, runs the rounds, writes the new diameters to state.diameters and returns the device's
    result dict (MDDevice.swap_rounds)."""
    dev = state.system.device
    spec = params.potential.device_spec()
    if spec[0] != "builtin":
        raise ValueError("swap_rounds needs a built-in potential (the pair energy of a user potential is not reachable "
                         "from the swap kernel)")
    dev.set_potential(spec[1], spec[2])
    dev.upload(x=state.system.positions, images=state.images, diameters=state.diameters)
    dev.swap_setup(fraction, max_diameter_difference, seed)
    r = dev.swap_rounds(int(rounds), float(ktemp), first_round=int(first_round))
    state.diameters = dev.diameters()
    state.system.energy_and_forces.energy = r["U"]
    state.system.energy_and_forces.virial = r["W"]
    return r
