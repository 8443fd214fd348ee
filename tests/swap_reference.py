"""The swap Monte Carlo round (include/mdhip.h md_swap_*) restated in numpy on the CPU oracle.  Takes
nothing from the code under test: the pair set is oracle.forces_brute(..., want_pairs=True) (tests/test_gpu_parity.py
test_polydisperse_2d shows it equals the device's exactly), pair energies are oracle.evaluate, the random words are
oracle.philox.

Status codes (the device's): 0 none, 1 void, 2 lost the claim, 3 blocked, 4 filtered, 5 rejected, 6 accepted."""
import numpy as np

from oracle import oracle as orc
from tests.util import lj_system, poly_system, sheared, with_diameters

NONE, VOID, LOST, BLOCKED, FILTERED, REJECTED, ACCEPTED = range(7)
NOKEY = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------------------------------
# The systems of the tests, and the seeds at which the reference meets the fairness conditions (conditions() below;
# tests/test_swap.py checks them on the CPU, tests/test_gpu_swap.py again before it compares).
# ---------------------------------------------------------------------------------------------------------------------
def case(name):
    """dict(system, cutoff, kind, params, pot, ktemp, fraction, seed) of 'poly', 'lj' or 'lj_sheared'."""
    if name == "poly":
        s = poly_system()
        return dict(name=name, system=s, cutoff=1.5, kind=orc.POT_POLYDISPERSE, params=[1.25, 0.2],
                    pot=orc.make_pot(orc.POT_POLYDISPERSE, [1.25, 0.2]), ktemp=0.11, fraction=0.02, seed=SEEDS[name])
    s = with_diameters(lj_system(1000), 0.9, 1.1)
    if name == "lj_sheared":
        # ten lattice sites per edge: a tilt of three spacings keeps the periodic images on the grid
        s = sheared(s, 3.0 * s["box"][0] / 10.0)
    elif name != "lj":
        raise KeyError(name)
    return dict(name=name, system=s, cutoff=2.5, kind=orc.POT_LJ, params=[1.0, 1.0, 2.5],
                pot=orc.make_pot(orc.POT_LJ, [1.0, 1.0, 2.5]), ktemp=1.0, fraction=0.01, seed=SEEDS[name])


SEEDS = {"poly": 2024, "lj": 11, "lj_sheared": 11}
ROUNDS = 8


class _cell_of:
    """with _cell_of(system): the oracle uses the system's general cell, if it has one."""

    def __init__(self, system):
        self.ctx = orc.set_cell(system["cell"]) if "cell" in system else None

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)


def total_energy(system, cutoff, pot, diam, x=None):
    with _cell_of(system):
        return orc.forces_brute(system["x"] if x is None else x, system["box"], cutoff, pot, diam)[1]


def forces(system, cutoff, pot, diam, x=None):
    with _cell_of(system):
        return orc.forces_brute(system["x"] if x is None else x, system["box"], cutoff, pot, diam)[:3]


class Frame:
    """The positions' part of a round, which no diameter enters: the pair set and the pair distances."""

    def __init__(self, system, cutoff, pot, x=None):
        x = np.ascontiguousarray(system["x"] if x is None else x, dtype=np.float64)
        n = x.shape[0]
        with _cell_of(system):
            pairs = orc.forces_brute(x, system["box"], cutoff, pot, np.ones(n), want_pairs=True)[3]
        U = np.asarray(system["cell"], dtype=np.float64) if "cell" in system else np.diag(system["box"])
        d = x[pairs[:, 1]] - x[pairs[:, 0]]
        fr = np.linalg.solve(U, d.T).T
        d = (fr - np.round(fr)) @ U.T                       # the minimum image (cutoff < half of every face distance)
        r = np.sqrt((d * d).sum(axis=1))
        assert r.max() <= cutoff * (1.0 + 1e-12)
        self.n, self.pot = n, pot
        self.nbr = [[] for _ in range(n)]
        for (a, b), rr in zip(pairs, r):
            self.nbr[a].append((int(b), float(rr)))
            self.nbr[b].append((int(a), float(rr)))

    def half(self, a, b, diam):
        """Particle a takes b's diameter: (sum over a's neighbours k != b of u_new - u_old, sum of |u_new| + |u_old|)."""
        du = s = 0.0
        for k, r in self.nbr[a]:
            if k == b:
                continue
            un = orc.evaluate(self.pot, r, diam[b], diam[k])[0]
            uo = orc.evaluate(self.pot, r, diam[a], diam[k])[0]
            du += un - uo
            s += abs(un) + abs(uo)
        return du, s


def threshold(fraction):
    return min(2 ** 32 - 1, int(np.floor(fraction * 2.0 ** 32)))


def selection(frame, seed, rnd, fraction):
    """What a round decides before any diameter is read: partner, status in {NONE, VOID, LOST, BLOCKED, -1 = survives},
    the fourth Philox word, by particle id."""
    n, thr = frame.n, threshold(fraction)
    key = [seed & 0xffffffff, (seed >> 32) & 0xffffffff]
    partner = np.full(n, -1, dtype=np.int64)
    status = np.zeros(n, dtype=np.int64)
    w3 = np.zeros(n, dtype=np.int64)
    keys = {}
    claim = [NOKEY] * n
    for i in range(n):
        w = orc.philox([i, rnd & 0xffffffff, (rnd >> 32) & 0xffffffff, 1], key)
        w3[i] = w[3]
        if not w[0] < thr:
            continue
        j = (w[1] * n) >> 32
        partner[i] = j
        if j == i:
            status[i] = VOID
            continue
        keys[i] = (w[2] << 32) | i
        claim[i] = min(claim[i], keys[i])
        claim[j] = min(claim[j], keys[i])
    livekey = [NOKEY] * n
    live = []
    for i, k in keys.items():
        j = int(partner[i])
        if claim[i] == k and claim[j] == k:
            live.append(i)
            livekey[i] = livekey[j] = k
        else:
            status[i] = LOST
    for i in live:
        j = int(partner[i])
        blocked = False
        for a, b in ((i, j), (j, i)):
            for k, _ in frame.nbr[a]:
                if k != b and livekey[k] < keys[i]:
                    blocked = True
        status[i] = BLOCKED if blocked else -1
    return partner, status, w3


def swap_round(frame, diam, seed, rnd, fraction, ktemp, max_diff=None):
    """One round: dict(partner, status, du, S, u3, diam) -- by proposer id; du, S of the decided swaps; the new diameters."""
    partner, status, w3 = selection(frame, seed, rnd, fraction)
    n = frame.n
    du, S, u3 = np.zeros(n), np.zeros(n), np.zeros(n)
    new = np.array(diam, dtype=np.float64, copy=True)
    for i in np.flatnonzero(status == -1):
        i = int(i)
        j = int(partner[i])
        if max_diff is not None and abs(diam[i] - diam[j]) > max_diff:
            status[i] = FILTERED
            continue
        (da, sa), (db, sb) = frame.half(i, j, diam), frame.half(j, i, diam)
        du[i], S[i] = da + db, sa + sb
        u3[i] = (float(w3[i]) + 0.5) / 2.0 ** 32
        with np.errstate(over="ignore"):
            accept = u3[i] < np.exp(-du[i] / ktemp)
        status[i] = ACCEPTED if accept else REJECTED
        if accept:
            new[i], new[j] = diam[j], diam[i]
    return dict(partner=partner, status=status, du=du, S=S, u3=u3, diam=new)


def run_rounds(frame, diam, seed, first_round, nrounds, fraction, ktemp, max_diff=None):
    out = []
    for r in range(first_round, first_round + nrounds):
        out.append(swap_round(frame, diam, seed, r, fraction, ktemp, max_diff))
        diam = out[-1]["diam"]
    return out


def conditions(rounds, ktemp):
    """The two conditions under which equal statuses are a fair demand of another implementation: no decided swap within
    1e-9 (1 + S / kT) of the acceptance threshold in ln; at least 10 decided and one each accepted, rejected, blocked,
    lost.  Returns (ok, text)."""
    margin, counts = np.inf, np.zeros(7, dtype=np.int64)
    for r in rounds:
        st = r["status"]
        counts += np.bincount(st, minlength=7)
        for i in np.flatnonzero(st >= REJECTED):
            margin = min(margin, abs(np.log(r["u3"][i]) + r["du"][i] / ktemp) / (1e-9 * (1.0 + r["S"][i] / ktemp)))
    decided = counts[REJECTED] + counts[ACCEPTED]
    ok = margin > 1.0 and decided >= 10 and all(counts[c] >= 1 for c in (ACCEPTED, REJECTED, BLOCKED, LOST))
    text = "decided %d accepted %d rejected %d blocked %d lost %d void %d filtered %d, smallest margin %.3g x the cushion" % (
        decided, counts[ACCEPTED], counts[REJECTED], counts[BLOCKED], counts[LOST], counts[VOID], counts[FILTERED], margin)
    return ok, text
