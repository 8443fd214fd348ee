"""The sampler audit: a run of run_simulation with every sampler attached at once, checked against its own frames.

No GPU in this module.  Its parts:

Recorder(dev)       a proxy around anything with MDDevice's method surface, installed as state.system.device.  It forwards
                    every call, keeps the ordered trace (last completed step, method, args) in the form of
                    tests/test_sampler_protocol.py, stores the frame (download() and diameters()) once per stop before the
                    first sampler call of that stop, stats()["rebuilds"] before and after every sampler call, what the
                    sampler's *_read returns after every sampler call, and the diameters after every swap block.
Restatement         the ten samplers restated on the CPU behind the device's own method names, by particle id, from a
                    frame (x, v, images, diameters) alone.  Pairs come from tests/pair_reference.brute_pairs on the frame
                    (every pair a < b is looked at; general cells included), never from the device's rows; per frame it
                    uses the references the repository already has (boo_reference, cluster_reference, cage_reference,
                    chi4_reference, cur_reference, mpc_reference, dyn_reference, sq_reference).
expected(...)       the accumulators at the end of the run, restated from the frames and the documented walk.
audit(...)          walks the run by each sampler's documented rule (schedule(), every, the origin ring; expected_trace),
                    demands that the recorded trace is that walk -- the documented order at every shared stop, every
                    sampler call before swap_rounds of its stop, a snapshot_begin of that stop after the swap block --
                    that the frame of every stop carries the diameters the previous swap block left, and that after EVERY
                    sampler call the device's accumulators are the restatement's.  Because the accumulators are compared
                    after every call and not only at the end, a failure names the sampler, the step, the quantity and the
                    first differing index.

Integers are compared exactly.  fp64 sums are held to the bound the sampler's own device test uses for one sample, applied
per accumulated sample and added up (nothing here is a new tolerance):

  dynamics      sum d2, sum d4: TOL |ref| of the sample; sum s(q): TOL d N        (tests/test_gpu_dynamics.py, TOL = 1e-12)
  cage          TOL N s1, TOL N s1^2, TOL N d, s1 = max(1, max d2)                 (tests/test_gpu_cage.py)
  bond order    frame sums 0..3: TOL N; global order: TOL; n, c, solid exact       (tests/test_gpu_bond_order.py)
  stress        virial 1e-12 A, A = sum |f/r| d2; kinetic 1e-12 sum v^2            (tests/test_gpu_stress.py)
  orientational counts exact; the quantised sums 2 quanta per pair, the self sum 2 N: the marks are the reference's q_lm, not
                the device's bits, and a term may round to the neighbouring integer (tests/test_gpu_pair_correlation.py)
  Z (VACF)      64 A 2^-53, A = sum |v o|                                          (tests/test_gpu_currents.py)

The wave-vector accumulators have no bound of their own in the tests (given the device's rho they are exact; here rho is
the extended-precision one), so theirs is derived from the bound B on a mode (sq_reference.bound for rho and W,
cur_reference.j_bound for j) by counting operations.  A term p = a b + c d of two modes with errors <= B (the frame's)
and <= Bo (the origin's) is off by at most B (|b| + |d|) + Bo (|a| + |c|) + 2 B Bo, plus 3 u (|a b| + |c d|) for the two
products and the add in fp64, u = 2^-53; adding it to the accumulator costs u |accumulator| more.  The longitudinal
projection pL = sum_a e_a j_a has error BL = sum_a |e_a| B_a + d u sum_a |e_a j_a|, and the same rule applies with BL.  The
stress lag products ch(m) ch(m - k) follow the rule too with the channel error e = (bound of K) + (bound of W) of the
component, and u-terms for the product and the add.

A pair within 1e-9 (relative, in d2) of a neighbour, bond or break radius, or a bond coherence within 1e-9 of the solid
threshold, is a guard (AuditGuard), not a failure: the two sides round differently there, as the device tests say."""
import math
import types

import numpy as np

from tests import boo_reference, cage_reference, chi4_reference, cluster_reference, cur_reference, dyn_reference
from tests import mpc_reference, pair_reference, sq_reference
from tests.test_gpu_bond_order import TOL

U53 = cur_reference.U53

# method -> prefix of the ten samplers' acting calls
SAMPLER_CALLS = {"rdf_sample": "rdf", "dyn_sample": "dyn", "dyn_origin": "dyn", "sq_sample": "sq", "cur_sample": "cur",
                 "stress_sample": "stress", "boo_sample": "boo", "cluster_sample": "cluster", "cage_sample": "cage",
                 "cage_origin": "cage", "chi4_sample": "chi4", "chi4_origin": "chi4", "mpc_sample": "mpc"}
# prefix -> the keyword run_simulation takes the sampler by
KEYWORD = {"rdf": "rdf", "dyn": "dynamics", "sq": "sq", "cur": "currents", "stress": "stress", "boo": "bond_order",
           "cluster": "clusters", "cage": "cage", "chi4": "four_point", "mpc": "orientational", "swap": "swap"}
READ_NAMES = {
    "rdf": ("counts", "nsamples"),
    "dyn": ("nsamples", "sums", "hist"),
    "sq": ("nstatic", "s2", "nsamples", "corr"),
    "cur": ("nstatic", "s_tot", "s_long", "nsamples", "c_tot", "c_long", "z"),
    "stress": ("nsamples", "sum_kin", "sum_vir", "ncorr", "corr"),
    "boo": ("nsamples", "sum_fr", "hist_q", "hist_qbar", "hist_nnb", "hist_conn", "series"),
    "cluster": ("nsamples", "sum_fr", "hist_size", "series"),
    "cage": ("nsamples", "sums", "counts", "hist_broken", "overflow"),
    "chi4": ("nsamples", "sum_q", "sum_q2", "s4"),
    "mpc": ("nsamples", "counts", "sums", "self_sum", "tmax", "range_error"),
}


class SamplerAuditFailure(AssertionError):
    """sampler (run_simulation's keyword), step, quantity, index (the first differing flat index, or None)."""

    def __init__(self, sampler, step, quantity, index=None, detail=""):
        self.sampler, self.step, self.quantity, self.index = sampler, step, quantity, index
        super().__init__("sampler %s, step %s, %s%s%s" % (sampler, step, quantity,
                                                          "" if index is None else ", first differing index %d" % index,
                                                          ": " + detail if detail else ""))


class AuditGuard(AssertionError):
    """A frame sits on a knife edge where two correct implementations may disagree: change the inputs of the case."""


def _ints(v):
    return tuple(int(a) for a in v)


# ---------------------------------------------------------------------------------------------------------------------
# Recorder

class Recorder:
    def __init__(self, dev):
        self._dev = dev
        self.step = 0                   # steps completed on the handle since the upload
        self.trace, self.calls, self.setups = [], {}, []
        self.frames, self.post_swap, self.blocks = {}, {}, {}
        self.initial_diameters = None

    def __getattr__(self, name):        # everything that is not recorded is forwarded as it is
        return getattr(self._dev, name)

    # -- the loop --------------------------------------------------------------------------------------------------
    def upload(self, *a, **kw):
        r = self._dev.upload(*a, **kw)
        self.step = 0
        self.initial_diameters = np.array(self._dev.diameters(), copy=True)
        return r

    def run(self, nsteps, *a, **kw):
        r = self._dev.run(nsteps, *a, **kw)
        self.step += int(nsteps)
        return r

    def run_brownian(self, nsteps, *a, **kw):
        r = self._dev.run_brownian(nsteps, *a, **kw)
        self.step += int(nsteps)
        return r

    def snapshot_begin(self):
        self.trace.append((self.step - 1, "snapshot_begin", ()))
        return self._dev.snapshot_begin()

    def _frame(self):
        s = self.step - 1
        if s not in self.frames:
            x, v, f, img = self._dev.download()
            self.frames[s] = types.SimpleNamespace(step=s, x=x, v=v, f=f, img=img,
                                                   diam=np.array(self._dev.diameters(), copy=True))

    def _sampler_call(self, method, args, call):
        self._frame()
        r0 = self._dev.stats()["rebuilds"]
        out = call()
        r1 = self._dev.stats()["rebuilds"]
        read = getattr(self._dev, SAMPLER_CALLS[method] + "_read")()
        self.calls[len(self.trace)] = dict(step=self.step - 1, method=method, rebuilds=(r0, r1), read=read)
        self.trace.append((self.step - 1, method, args))
        return out

    # -- the samplers: the trace's argument forms are tests/test_sampler_protocol.py's -----------------------------------
    def rdf_sample(self):
        return self._sampler_call("rdf_sample", (), self._dev.rdf_sample)

    def dyn_sample(self, slots, rows):
        return self._sampler_call("dyn_sample", (_ints(slots), _ints(rows)), lambda: self._dev.dyn_sample(slots, rows))

    def dyn_origin(self, slot):
        return self._sampler_call("dyn_origin", (int(slot),), lambda: self._dev.dyn_origin(slot))

    def _wave(self, method, static, slots, rows, origin):
        args = (bool(static), _ints(slots), _ints(rows), None if origin is None else int(origin))
        return self._sampler_call(method, args, lambda: getattr(self._dev, method)(static, slots, rows, origin))

    def sq_sample(self, static=True, slots=(), rows=(), origin=None):
        return self._wave("sq_sample", static, slots, rows, origin)

    def cur_sample(self, static=True, slots=(), rows=(), origin=None):
        return self._wave("cur_sample", static, slots, rows, origin)

    def stress_sample(self):
        return self._sampler_call("stress_sample", (), self._dev.stress_sample)

    def boo_sample(self):
        return self._sampler_call("boo_sample", (), self._dev.boo_sample)

    def cluster_sample(self):
        return self._sampler_call("cluster_sample", (), self._dev.cluster_sample)

    def cage_sample(self, slots, rows):
        return self._sampler_call("cage_sample", (_ints(slots), _ints(rows)), lambda: self._dev.cage_sample(slots, rows))

    def cage_origin(self, slot):
        return self._sampler_call("cage_origin", (int(slot),), lambda: self._dev.cage_origin(slot))

    def chi4_sample(self, slots, rows):
        return self._sampler_call("chi4_sample", (_ints(slots), _ints(rows)), lambda: self._dev.chi4_sample(slots, rows))

    def chi4_origin(self, slot):
        return self._sampler_call("chi4_origin", (int(slot),), lambda: self._dev.chi4_origin(slot))

    def mpc_sample(self):
        return self._sampler_call("mpc_sample", (), self._dev.mpc_sample)

    def swap_rounds(self, nrounds, ktemp, first_round=0):
        self._frame()
        self.trace.append((self.step - 1, "swap_rounds", (int(nrounds), float(ktemp), int(first_round))))
        r = self._dev.swap_rounds(nrounds, ktemp, first_round=first_round)
        self.post_swap[self.step - 1] = np.array(self._dev.diameters(), copy=True)
        self.blocks[self.step - 1] = dict(r)
        return r

    def pairs_per_call(self):
        """The largest number of (slot, row) pairs one sampler call carried."""
        return max([len(a[0]) for _, m, a in self.trace if m in ("dyn_sample", "cage_sample", "chi4_sample")]
                   + [len(a[1]) for _, m, a in self.trace if m in ("sq_sample", "cur_sample")] + [0])

    def rebuilding_calls(self):
        """[(step, method)] of the sampler calls during which the handle rebuilt its list."""
        return [(c["step"], c["method"]) for c in self.calls.values() if c["rebuilds"][1] > c["rebuilds"][0]]


for _name in ("rdf", "dyn", "sq", "cur", "stress", "boo", "cluster", "cage", "chi4", "mpc", "swap"):
    def _setup(self, *a, _n=_name + "_setup", **kw):
        self.setups.append((_n, a, kw))
        return getattr(self._dev, _n)(*a, **kw)
    setattr(Recorder, _name + "_setup", _setup)


# ---------------------------------------------------------------------------------------------------------------------
# The documented walk

def expected_trace(samplers, total_steps, frequency, log_times=False, write_trajectory=True, ensemble=None,
                   first_round=0):
    """(trace, stops): the device calls of one run_simulation call in order, as (step, method, args), and the sorted steps
    at which a segment ends.  `samplers` maps run_simulation's keywords (rdf, dynamics, sq, currents, stress, bond_order,
    clusters, cage, four_point, orientational, swap) to the objects; only public names of theirs are used: every,
    schedule(), lags, rounds, ktemp."""
    from moleculardynamics.jl_amd.analysis import LOG_BASE, LOG_N
    T, f = int(total_steps), int(frequency)
    g = samplers.get
    snapshots = ({0} | {int(math.floor(LOG_BASE ** i)) for i in range(LOG_N + 1)}) if log_times else set()
    events = {k: g(k).schedule(T)[1] for k in ("dynamics", "sq", "currents", "cage", "four_point") if g(k) is not None}
    stress_steps = set(g("stress").schedule(T)) if g("stress") is not None else set()
    swap, rounds_done = g("swap"), int(first_round)

    def split(smp):
        return tuple(int(a) for a, _ in smp), tuple(int(b) for _, b in smp)

    def scheduled(name, prefix, step, want):
        ev = events[name].get(step) if name in events else None
        if ev is not None:
            if ev[0]:
                want.append((step, prefix + "_sample", split(ev[0])))
            if ev[1] is not None:
                want.append((step, prefix + "_origin", (int(ev[1]),)))

    def every(name, step):
        s = g(name)
        return s is not None and step % f == 0 and (step // f) % s.every == 0

    want, stops = [], {T - 1}
    for step in range(T):
        before = len(want)
        output = step % f == 0
        if every("rdf", step):
            want.append((step, "rdf_sample", ()))
        scheduled("dynamics", "dyn", step, want)
        if g("sq") is not None:
            static = every("sq", step)
            ev = events["sq"].get(step)
            if static or ev is not None:
                smp, org = ev if ev is not None else ([], None)
                want.append((step, "sq_sample", (static,) + split(smp) + (None if org is None else int(org),)))
        if g("currents") is not None:
            ev = events["currents"].get(step)
            if ev is not None:          # the equal-time sample exactly at the stops that store an origin
                want.append((step, "cur_sample", (ev[1] is not None,) + split(ev[0]) + (None if ev[1] is None else int(ev[1]),)))
        if step in stress_steps:
            want.append((step, "stress_sample", ()))
        if every("bond_order", step):
            want.append((step, "boo_sample", ()))
        if every("clusters", step):
            want.append((step, "cluster_sample", ()))
        scheduled("cage", "cage", step, want)
        scheduled("four_point", "chi4", step, want)
        if every("orientational", step):
            want.append((step, "mpc_sample", ()))
        if swap is not None and (step + 1) % swap.every == 0:
            kt = swap.ktemp
            if kt is None:
                kt = ensemble.ktemp(step + 1) if callable(ensemble.ktemp) else ensemble.ktemp
            want.append((step, "swap_rounds", (swap.rounds, float(kt), rounds_done)))
            rounds_done += swap.rounds
        if (output and write_trajectory) or step in snapshots:
            want.append((step, "snapshot_begin", ()))
        if len(want) > before or output:
            stops.add(step)
    return want, sorted(stops)


# ---------------------------------------------------------------------------------------------------------------------
# Restatement

def _term(a, b, c, d, B, Bo):
    """(a b + c d, its error bound) for mode parts a, c (error <= B) against b, d (error <= Bo); see the module docstring."""
    val = a * b + c * d
    err = B * (np.abs(b) + np.abs(d)) + Bo * (np.abs(a) + np.abs(c)) + 2.0 * B * Bo + 3.0 * U53 * (np.abs(a * b) + np.abs(c * d))
    return val, err


def _add(acc, bnd, val, err):
    acc = acc + val
    return acc, bnd + err + U53 * np.abs(acc)


def _channels(sig, d):
    """tests/test_gpu_stress.py's _channels: the shear components, the normal-stress differences, the pressure channel."""
    if d == 3:
        return np.array([sig[3], sig[4], sig[5], (sig[0] - sig[1]) * 0.5, (sig[1] - sig[2]) * 0.5,
                         ((sig[0] + sig[1]) + sig[2]) / 3.0])
    return np.array([sig[2], (sig[0] - sig[1]) * 0.5, (sig[0] + sig[1]) / 2.0])


def _comp(d):
    return [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)] if d == 3 else [(0, 0), (1, 1), (0, 1)]


class Restatement:
    """The ten samplers by particle id from self.fr = a frame with x, v, img, diam.  pair_force(r, s_i, s_j) -> f (arrays),
    zero beyond the potential's range, and force_range (the largest pair distance with a force) are needed by stress only.
    *_read() returns what MDDevice's returns; read(prefix) adds the names and the bounds (None: exact)."""

    def __init__(self, n, dim, unitcell, pair_force=None, force_range=0.0):
        U = np.asarray(unitcell, dtype=np.float64)
        self.n, self.dim, self.U = int(n), int(dim), (U if U.ndim == 2 else np.diag(U))
        self.pair_force, self.force_range = pair_force, float(force_range)
        self.r_search = self.force_range
        self.fr, self._cache = None, {}
        self.boo_last = None
        self.boo_history = []

    def set_frame(self, fr):
        if fr is not self.fr:
            self.fr, self._cache = fr, {}

    def frame_for(self, prefix):
        return self.fr

    def _pairs(self, fr, r):
        ent = self._cache.get(id(fr))
        if ent is None or ent[0] < r:
            rs = max(r, self.r_search)
            ent = (rs, fr) + pair_reference.brute_pairs(fr.x, self.U, rs)
            self._cache[id(fr)] = ent
        return ent[2], ent[3], ent[4]

    def _within(self, fr, thr2_of, wide, what):
        """The pairs with d2 < thr2 (a number or a function of the pair ids), the guard asserted."""
        pairs, de, d2 = self._pairs(fr, wide)
        thr2 = thr2_of(pairs) if callable(thr2_of) else np.full(len(pairs), thr2_of)
        if np.any(np.abs(d2 - thr2) <= 1e-9 * thr2):
            raise AuditGuard("step %s: a pair sits on the %s" % (getattr(fr, "step", "?"), what))
        keep = d2 < thr2
        return pairs[keep], de[keep], d2[keep]

    def _want(self, r):
        self.r_search = max(self.r_search, float(r))

    # -- g(r) ------------------------------------------------------------------------------------------------------
    def rdf_setup(self, r_max, nbins):
        self.rdf = types.SimpleNamespace(r_max=float(r_max), nbins=int(nbins), counts=np.zeros(int(nbins), np.int64), ns=0)
        self._want(r_max)

    def rdf_sample(self):
        s, fr = self.rdf, self.frame_for("rdf")
        _, _, d2 = self._pairs(fr, s.r_max)
        s.counts = s.counts + dyn_reference.bin_counts(d2, s.r_max, s.nbins)
        s.ns += 1

    def rdf_read(self):
        return self.rdf.counts.copy(), self.rdf.ns

    # -- self dynamics ---------------------------------------------------------------------------------------------
    def dyn_setup(self, nslots, nrows, q=(), r_max=0.0, nbins=0):
        q = np.asarray(q, dtype=np.float64).reshape(-1)
        self.dyn = types.SimpleNamespace(nslots=int(nslots), q=q, r_max=float(r_max), nbins=int(nbins), org={},
                                         ns=np.zeros(nrows, np.int64), sums=np.zeros((nrows, 2 + q.size)),
                                         bnd=np.zeros((nrows, 2 + q.size)), hist=np.zeros((nrows, int(nbins)), np.int64))

    def dyn_origin(self, slot):
        fr = self.frame_for("dyn")
        self.dyn.org[int(slot)] = (fr.x.copy(), fr.img.copy())

    def dyn_sample(self, slots, rows):
        s, fr = self.dyn, self.frame_for("dyn")
        for slot, row in zip(slots, rows):
            x0, n0 = s.org[int(slot)]
            de, d2 = dyn_reference.restate(x0, n0, fr.x, fr.img, self.U)
            vals = [math.fsum(d2), math.fsum(d2 * d2)]
            errs = [dyn_reference.TOL * vals[0], dyn_reference.TOL * vals[1]]
            for q in s.q:
                c = np.cos(q * de[:, 0])
                for a in range(1, self.dim):
                    c = c + np.cos(q * de[:, a])
                vals.append(math.fsum(c))
                errs.append(dyn_reference.TOL * self.dim * self.n)
            s.sums[row] += vals
            s.bnd[row] += errs
            self._count_sample("dyn", slot, row)
            if s.nbins:
                s.hist[row] += dyn_reference.bin_counts(d2, s.r_max, s.nbins)

    def _count_sample(self, prefix, slot, row):
        getattr(self, prefix).ns[row] += 1

    def dyn_read(self):
        return self.dyn.ns.copy(), self.dyn.sums.copy(), self.dyn.hist.copy()

    # -- density modes ---------------------------------------------------------------------------------------------
    def sq_setup(self, n, nslots=0, nrows=0):
        n = np.ascontiguousarray(n, dtype=np.int32)
        nv = n.shape[0]
        self.sq = types.SimpleNamespace(n=n, B=sq_reference.bound(self.n, self.U, n), org={}, nst=0, s2=np.zeros(nv),
                                        s2b=np.zeros(nv), ns=np.zeros(nrows, np.int64), corr=np.zeros((nrows, nv)),
                                        corrb=np.zeros((nrows, nv)))

    def sq_sample(self, static=True, slots=(), rows=(), origin=None):
        s, fr = self.sq, self.frame_for("sq")
        re, im = sq_reference.rho_true(fr.x, self.U, s.n)
        if static:
            val, err = _term(re, re, im, im, s.B, s.B)
            s.s2, s.s2b = _add(s.s2, s.s2b, val, err)
            s.nst += 1
        for slot, row in zip(slots, rows):
            ore, oim = s.org[int(slot)]
            val, err = _term(re, ore, im, oim, s.B, s.B)
            s.corr[row], s.corrb[row] = _add(s.corr[row], s.corrb[row], val, err)
            s.ns[row] += 1
        if origin is not None:
            s.org[int(origin)] = (re.copy(), im.copy())

    def sq_read(self):
        return self.sq.nst, self.sq.s2.copy(), self.sq.ns.copy(), self.sq.corr.copy()

    # -- currents --------------------------------------------------------------------------------------------------
    def cur_setup(self, n, e, nslots=0, nrows=0, vacf=False):
        n = np.ascontiguousarray(n, dtype=np.int32)
        nv = n.shape[0]
        z = lambda *shape: np.zeros(shape)          # noqa: E731
        self.cur = types.SimpleNamespace(n=n, e=np.asarray(e, dtype=np.float64), vacf=bool(vacf), org={}, nst=0,
                                         ns=np.zeros(nrows, np.int64), s_tot=z(nv), s_long=z(nv), c_tot=z(nrows, nv),
                                         c_long=z(nrows, nv), b_st=z(nv), b_sl=z(nv), b_ct=z(nrows, nv), b_cl=z(nrows, nv),
                                         z=z(nrows + 1), zb=z(nrows + 1))

    def _cur_terms(self, j, B, o, Bo):
        s = self.cur
        tot, tb = 0.0, 0.0
        for a in range(self.dim):
            v, e = _term(j.real[:, a], o.real[:, a], j.imag[:, a], o.imag[:, a], B[:, a], Bo[:, a])
            tot, tb = tot + v, tb + e + U53 * np.abs(tot + v)
        ea = np.abs(s.e)

        def proj(m, Bm):
            return (cur_reference.p_long(s.e, m.real), cur_reference.p_long(s.e, m.imag),
                    (ea * Bm).sum(axis=1) + self.dim * U53 * (ea * (np.abs(m.real) + np.abs(m.imag))).sum(axis=1))

        pr, pi, BL = proj(j, B)
        qr, qi, BLo = proj(o, Bo)
        lon, lb = _term(pr, qr, pi, qi, BL, BLo)
        return tot, tb, lon, lb

    def cur_sample(self, static=True, slots=(), rows=(), origin=None):
        s, fr = self.cur, self.frame_for("cur")
        j = cur_reference.j_true(fr.x, fr.v, self.U, s.n)
        B = cur_reference.j_bound(fr.v, self.U, s.n)
        if static:
            tot, tb, lon, lb = self._cur_terms(j, B, j, B)
            s.s_tot, s.b_st = _add(s.s_tot, s.b_st, tot, tb)
            s.s_long, s.b_sl = _add(s.s_long, s.b_sl, lon, lb)
            s.nst += 1
            if s.vacf:
                zt, A = cur_reference.z_true(fr.v, fr.v)
                s.z[-1] += zt
                s.zb[-1] += A * 64 * U53
        for slot, row in zip(slots, rows):
            o, Bo, vo = s.org[int(slot)]
            tot, tb, lon, lb = self._cur_terms(j, B, o, Bo)
            s.c_tot[row], s.b_ct[row] = _add(s.c_tot[row], s.b_ct[row], tot, tb)
            s.c_long[row], s.b_cl[row] = _add(s.c_long[row], s.b_cl[row], lon, lb)
            s.ns[row] += 1
            if s.vacf:
                zt, A = cur_reference.z_true(fr.v, vo)
                s.z[row] += zt
                s.zb[row] += A * 64 * U53
        if origin is not None:
            s.org[int(origin)] = (j.copy(), B.copy(), fr.v.copy())

    def cur_read(self):
        s = self.cur
        return (s.nst, s.s_tot.copy(), s.s_long.copy(), s.ns.copy(), s.c_tot.copy(), s.c_long.copy(),
                s.z.copy() if s.vacf else None)

    # -- stress ----------------------------------------------------------------------------------------------------
    def stress_setup(self, nlags=0):
        nc = 6 if self.dim == 3 else 3
        self.stress = types.SimpleNamespace(nlags=int(nlags), ns=0, kin=np.zeros(nc), vir=np.zeros(nc), kb=np.zeros(nc),
                                            vb=np.zeros(nc), ncorr=np.zeros(int(nlags), np.int64),
                                            corr=np.zeros((int(nlags), nc)), cb=np.zeros((int(nlags), nc)), ring=[])

    def stress_tensors(self, fr):
        """(K, bound of K, W, bound of W) of one frame, tests/test_gpu_stress.py's reference and bounds."""
        d = self.dim
        pairs, de, d2 = self._pairs(fr, self.force_range)
        r = np.sqrt(d2)
        f = np.asarray(self.pair_force(r, fr.diam[pairs[:, 0]], fr.diam[pairs[:, 1]]), dtype=np.float64)
        live = f != 0.0
        fpr, de, d2 = f[live] / r[live], de[live], d2[live]
        W = np.array([math.fsum(fpr * de[:, a] * de[:, b]) for a, b in _comp(d)])
        A = math.fsum(np.abs(fpr) * d2)
        K = np.array([math.fsum(fr.v[:, a] * fr.v[:, b]) for a, b in _comp(d)])
        v2 = math.fsum((fr.v * fr.v).sum(axis=1))
        return K, np.full(len(K), 1e-12 * v2), W, np.full(len(W), 1e-12 * A)

    def stress_sample(self):
        s, fr = self.stress, self.frame_for("stress")
        K, kb, W, wb = self.stress_tensors(fr)
        s.kin, s.kb = _add(s.kin, s.kb, K, kb)
        s.vir, s.vb = _add(s.vir, s.vb, W, wb)
        s.ns += 1
        if s.nlags:
            ch = _channels(K + W, self.dim)
            e = np.full(len(ch), float((kb + wb).max()) + 4.0 * U53 * float(np.abs(K).max() + np.abs(W).max()))
            s.ring.insert(0, (ch, e))
            del s.ring[s.nlags:]
            for k, (old, eo) in enumerate(s.ring):
                val = ch * old
                err = e * np.abs(old) + eo * np.abs(ch) + e * eo + 2.0 * U53 * np.abs(val)
                s.corr[k], s.cb[k] = _add(s.corr[k], s.cb[k], val, err)
                s.ncorr[k] += 1

    def stress_read(self):
        s = self.stress
        return s.ns, s.kin.copy(), s.vir.copy(), s.ncorr.copy(), s.corr.copy()

    # -- bond order ------------------------------------------------------------------------------------------------
    def boo_setup(self, r_neigh, order=6, nbins=100, threshold=0.7, min_conn=7, nseries=0):
        nb = int(nbins)
        self.boo = types.SimpleNamespace(r=float(r_neigh), order=int(order), nbins=nb, thr=float(threshold),
                                         minc=int(min_conn), nseries=int(nseries), ns=0, fr=np.zeros(8), frb=np.zeros(8),
                                         hq=np.zeros(nb, np.int64), hb=np.zeros(nb, np.int64), hn=np.zeros(33, np.int64),
                                         hc=np.zeros(33, np.int64), series=[], edge=0)
        self._want(r_neigh)

    def boo_frame(self, fr):
        s = self.boo
        pairs, de, _ = self._within(fr, s.r * s.r, s.r, "bond-order neighbour radius")
        r = boo_reference.bond_order(self.n, pairs, de, s.order, s.thr, s.minc)
        if np.any(np.abs(r["sij"] - s.thr) <= 1e-9):
            raise AuditGuard("step %s: a bond coherence sits on the solid threshold" % getattr(fr, "step", "?"))
        return r

    def boo_sample(self):
        s, fr = self.boo, self.frame_for("boo")
        r = self.boo_frame(fr)
        self.boo_last = r
        self.boo_history.append(r)
        one = np.array([TOL * self.n] * 4 + [0.0, 0.0, 0.0, TOL])
        s.fr, s.frb = s.fr + r["fr"], s.frb + one + U53 * np.abs(s.fr + r["fr"])
        s.frb[4:7] = 0.0
        s.hq += boo_reference.bins(r["q"], s.nbins)
        s.hb += boo_reference.bins(r["qbar"], s.nbins)
        for v in (r["q"], r["qbar"]):          # values the bound allows to fall on either side of a bin edge
            t = v * s.nbins
            s.edge += int(np.count_nonzero(np.abs(t - np.rint(t)) <= TOL * s.nbins))
        s.hn += boo_reference.clamped_counts(r["nnb"])
        s.hc += boo_reference.clamped_counts(r["conn"])
        if len(s.series) < s.nseries:
            s.series.append(r["fr"].copy())
        s.ns += 1

    def boo_read(self):
        s = self.boo
        return (s.ns, s.fr.copy(), s.hq.copy(), s.hb.copy(), s.hn.copy(), s.hc.copy(),
                np.array(s.series).reshape(-1, 8))

    # -- clusters --------------------------------------------------------------------------------------------------
    def cluster_setup(self, r_bond, members=0, max_size=1024, nseries=0):
        self.cluster = types.SimpleNamespace(r=float(r_bond), members=int(members), max_size=int(max_size),
                                             nseries=int(nseries), ns=0, fr=np.zeros(8, np.int64),
                                             hist=np.zeros(int(max_size) + 1, np.int64), series=[])
        self._want(r_bond)

    def solid_members(self):
        """The solid particles of the bond-order frame of the same step, by particle id."""
        return self.boo_last["solid"]

    def cluster_sample(self):
        s, fr = self.cluster, self.frame_for("cluster")
        pairs, _, _ = self._within(fr, s.r * s.r, s.r, "cluster bond length")
        c = cluster_reference.clusters(self.n, pairs, self.solid_members() if s.members == 1 else None, s.max_size)
        s.fr = s.fr + c["fr"]
        s.hist = s.hist + c["hist"]
        if len(s.series) < s.nseries:
            s.series.append(c["fr"].copy())
        s.ns += 1

    def cluster_read(self):
        s = self.cluster
        return s.ns, s.fr.copy(), s.hist.copy(), np.array(s.series, dtype=np.int64).reshape(-1, 8)

    # -- cage ------------------------------------------------------------------------------------------------------
    def cage_setup(self, nslots, nrows, r_neigh, r_break=None, scaled=False, max_neigh=16, q=()):
        q = np.asarray(q, dtype=np.float64).reshape(-1)
        self.cage = types.SimpleNamespace(r=float(r_neigh), rb=float(r_neigh if r_break is None else r_break),
                                          scaled=bool(scaled), maxn=int(max_neigh), q=q, org={},
                                          ns=np.zeros(nrows, np.int64), sums=np.zeros((nrows, 2 + q.size)),
                                          bnd=np.zeros((nrows, 2 + q.size)), counts=np.zeros((nrows, 3), np.int64),
                                          hist=np.zeros((nrows, 33), np.int64), overflow=0)
        self._want(r_neigh)

    def cage_store(self, slot, fr):
        s = self.cage
        wide = s.r * (float(fr.diam.max()) if s.scaled else 1.0)
        diam = fr.diam
        pairs, de, _ = self._within(
            fr, lambda p: cage_reference.threshold2(s.r, diam, p[:, 0], p[:, 1], s.scaled), wide, "cage neighbour radius")
        nnb = np.bincount(pairs.reshape(-1), minlength=self.n)
        s.overflow += int(np.maximum(nnb - s.maxn, 0).sum())
        s.org[int(slot)] = (fr.x.copy(), fr.img.copy(), pairs, de, diam.copy())

    def cage_origin(self, slot):
        self.cage_store(slot, self.frame_for("cage"))

    def cage_sample(self, slots, rows):
        s, fr = self.cage, self.frame_for("cage")
        for slot, row in zip(slots, rows):
            x0, n0, pairs, de, diam = s.org[int(slot)]
            r = cage_reference.cage(x0, n0, fr.x, fr.img, self.U, pairs, de, diam, s.rb, s.scaled, s.q)
            if np.any(np.abs(r["b2"] - r["thr2"]) <= 1e-9 * r["thr2"]):
                raise AuditGuard("step %s: a bond sits on the break radius" % getattr(fr, "step", "?"))
            s1 = max(1.0, float(r["d2"].max()))
            s.sums[row] += r["sums"]
            s.bnd[row] += np.array([TOL * self.n * s1, TOL * self.n * s1 * s1] + [TOL * self.n * self.dim] * s.q.size)
            s.counts[row] += r["counts"]
            s.hist[row] += r["hist"]
            s.ns[row] += 1

    def cage_read(self):
        s = self.cage
        return s.ns.copy(), s.sums.copy(), s.counts.copy(), s.hist.copy(), s.overflow

    # -- four-point ------------------------------------------------------------------------------------------------
    def chi4_setup(self, a, n=None, nslots=1, nrows=1):
        n = np.zeros((0, self.dim), np.int32) if n is None else np.ascontiguousarray(n, dtype=np.int32)
        nv = n.shape[0]
        self.chi4 = types.SimpleNamespace(a=float(a), n=n, B=sq_reference.bound(self.n, self.U, n) if nv else np.zeros(0),
                                          org={}, ns=np.zeros(nrows, np.int64), sq=np.zeros(nrows, np.int64),
                                          sq2=np.zeros(nrows, np.int64), s4=np.zeros((nrows, nv)), s4b=np.zeros((nrows, nv)))

    def chi4_origin(self, slot):
        fr = self.frame_for("chi4")
        self.chi4.org[int(slot)] = (fr.x.copy(), fr.img.copy())

    def chi4_sample(self, slots, rows):
        s, fr = self.chi4, self.frame_for("chi4")
        for slot, row in zip(slots, rows):
            x0, n0 = s.org[int(slot)]
            slow, Q = chi4_reference.overlap(x0, n0, fr.x, fr.img, self.U, s.a)
            s.sq[row] += Q
            s.sq2[row] += Q * Q
            s.ns[row] += 1
            if s.n.shape[0]:
                re, im = sq_reference.rho_true(x0[slow.astype(bool)], self.U, s.n)
                val, err = _term(re, re, im, im, s.B, s.B)
                s.s4[row], s.s4b[row] = _add(s.s4[row], s.s4b[row], val, err)

    def chi4_read(self):
        s = self.chi4
        return s.ns.copy(), s.sq.copy(), s.sq2.copy(), s.s4.copy()

    # -- orientational correlation ---------------------------------------------------------------------------------
    def mpc_setup(self, r_max, nbins, weights=None, tmax=None):
        nb = int(nbins)
        self.mpc = types.SimpleNamespace(r_max=float(r_max), nbins=nb, ns=0, cnt=np.zeros(nb, np.int64), tot=np.zeros(nb),
                                         totb=np.zeros(nb), own=0.0, ownb=0.0, err=0)
        self._want(r_max)

    def mpc_marks_qlm(self):
        """q_lm of the bond-order frame of the same step, by particle id."""
        return self.boo_last["qlm"]

    def mpc_sample(self):
        s, fr = self.mpc, self.frame_for("mpc")
        pairs, _, d2 = self._pairs(fr, s.r_max)
        marks = mpc_reference.boo_marks(self.mpc_marks_qlm())
        cnt, tot, own, ok = mpc_reference.correlate(pairs, d2, marks, mpc_reference.boo_weights(self.dim, self.boo.order),
                                                    1.0, s.r_max, s.nbins)
        s.cnt = s.cnt + cnt
        s.tot, s.totb = s.tot + tot, s.totb + 2.0 * cnt
        s.own, s.ownb = s.own + own, s.ownb + 2.0 * self.n
        s.err |= 0 if ok else 1
        s.ns += 1

    def mpc_read(self):
        s = self.mpc
        return s.ns, s.cnt.copy(), s.tot.copy(), s.own, 1.0, s.err

    # -- the named quantities and their bounds -----------------------------------------------------------------------
    def read(self, prefix):
        vals = getattr(self, prefix + "_read")()
        b = [None] * len(vals)
        if prefix == "dyn":
            b[1] = self.dyn.bnd
        elif prefix == "sq":
            b[1], b[3] = self.sq.s2b, self.sq.corrb
        elif prefix == "cur":
            s = self.cur
            b[1], b[2], b[4], b[5], b[6] = s.b_st, s.b_sl, s.b_ct, s.b_cl, s.zb
        elif prefix == "stress":
            s = self.stress
            b[1], b[2], b[4] = s.kb, s.vb, s.cb
        elif prefix == "boo":
            b[1] = self.boo.frb
            b[6] = np.tile(np.array([TOL * self.n] * 4 + [0.0, 0.0, 0.0, TOL]), (len(vals[6]), 1))
        elif prefix == "cage":
            b[1] = self.cage.bnd
        elif prefix == "chi4":
            b[3] = self.chi4.s4b
        elif prefix == "mpc":
            b[2], b[3] = self.mpc.totb, self.mpc.ownb
        return list(zip(READ_NAMES[prefix], vals, b))


# ---------------------------------------------------------------------------------------------------------------------
# audit

def _compare(name, step, quantity, got, want, bound, margins, slack=0):
    if want is None or got is None:
        if not (want is None and got is None):
            raise SamplerAuditFailure(name, step, quantity, None, "one side has no value")
        return
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        raise SamplerAuditFailure(name, step, quantity, None, "shape %s, expected %s" % (got.shape, want.shape))
    if bound is None:
        bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
        if slack and np.abs(got.astype(np.int64) - want.astype(np.int64)).sum() <= 2 * slack:
            return
        if bad.size:
            k = int(bad[0])
            raise SamplerAuditFailure(name, step, quantity, k, "got %r, expected %r" % (got.reshape(-1)[k], want.reshape(-1)[k]))
        return
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)).reshape(-1)
    bnd = np.broadcast_to(np.asarray(bound, dtype=np.float64), got.shape).reshape(-1)
    bad = np.flatnonzero(~(err <= bnd))
    if bad.size:
        k = int(bad[0])
        raise SamplerAuditFailure(name, step, quantity, k, "got %r, expected %r, |difference| %.3e > bound %.3e"
                                  % (got.reshape(-1)[k], want.reshape(-1)[k], err[k], bnd[k]))
    pos = bnd > 0.0
    if np.any(pos):
        key = (name, quantity)
        margins[key] = max(margins.get(key, 0.0), float((err[pos] / bnd[pos]).max()))


def _object_fields(name, s):
    """The public accumulators of a sampler object in the order of the device's read."""
    if name == "rdf":
        return s.counts, s.nsamples
    if name == "dynamics":
        return s.nsamples, s.sums, s.hist
    if name == "sq":
        return s.nstatic, s.s2, s.nsamples, s.corr
    if name == "currents":
        return (s.nstatic, s.s_tot, s.s_long, s.nsamples, s.c_tot, s.c_long,
                np.concatenate([s.z, [s.z0]]) if s.with_vacf else None)
    if name == "stress":
        return s.nsamples, s.sum_kin, s.sum_vir, s.ncorr, s.corr
    if name == "bond_order":
        return s.nsamples, s.sum_fr, s.hist_q, s.hist_qbar, s.hist_nnb, s.hist_conn, s.frames
    if name == "clusters":
        return s.nsamples, s.sum_fr, s.hist_size, s.frames
    if name == "cage":
        return s.nsamples, s.sums, s.counts, s.hist_broken
    if name == "four_point":
        return (s.nsamples, np.array([int(v) for v in s.sum_q], np.int64), np.array([int(v) for v in s.sum_q2], np.int64),
                s.sum_s4)
    return s.nsamples, s.counts, s.sums, s.self_sum


def audit(rec, samplers, restatement, total_steps, frequency, log_times=False, write_trajectory=True, ensemble=None,
          first_round=0, swap_truth=None):
    """Audit one recorded run (see the module docstring); `samplers` as for expected_trace, the objects as the run left
    them (reset before it).  swap_truth(frame, diameters_before, step, first_round) -> (diameters_after, counts dict), if
    given, restates every swap block.  Returns {(sampler, quantity): worst |difference| / bound} of the fp64 quantities."""
    want, _ = expected_trace(samplers, total_steps, frequency, log_times, write_trajectory, ensemble, first_round)
    for i in range(max(len(want), len(rec.trace))):
        w = want[i] if i < len(want) else None
        g = rec.trace[i] if i < len(rec.trace) else None
        if w != g:
            m = (w or g)[1]
            name = KEYWORD.get(SAMPLER_CALLS.get(m, "swap" if m == "swap_rounds" else m), m)
            raise SamplerAuditFailure(name, (w or g)[0], "trace", i, "device call %r, documented %r" % (g, w))

    # the frame of every stop carries the diameters the previous swap block left; a block only permutes them
    swap = samplers.get("swap")
    diam, rounds_done = rec.initial_diameters, int(first_round)
    for step in sorted(rec.frames):
        fr = rec.frames[step]
        if diam is not None and not np.array_equal(fr.diam, diam):
            k = int(np.flatnonzero(fr.diam != diam)[0])
            raise SamplerAuditFailure("swap", step, "diameters of the frame the samplers saw (pre-swap)", k)
        if step in rec.post_swap:
            after, blk = rec.post_swap[step], rec.blocks[step]
            if not np.array_equal(np.sort(after), np.sort(fr.diam)):
                raise SamplerAuditFailure("swap", step, "diameters after the block are no permutation")
            if swap_truth is not None:
                ref_after, counts = swap_truth(fr, fr.diam, step, rounds_done)
                for key, val in counts.items():
                    if int(blk[key]) != int(val):
                        raise SamplerAuditFailure("swap", step, key, None, "got %d, expected %d" % (blk[key], val))
                if not np.array_equal(after, ref_after):
                    raise SamplerAuditFailure("swap", step, "diameters", int(np.flatnonzero(after != ref_after)[0]))
            rounds_done += swap.rounds if swap is not None else 0
            diam = after

    # replay: after every sampler call the device's accumulators are the restatement's
    R, margins = restatement, {}
    for name, args, kw in rec.setups:
        if name != "swap_setup":
            getattr(R, name)(*args, **kw)
    last = {}
    for i, (step, method, args) in enumerate(want):
        prefix = SAMPLER_CALLS.get(method)
        if prefix is None:
            continue
        R.set_frame(rec.frames[step])
        getattr(R, method)(*args)
        got = rec.calls[i]["read"]
        last[prefix] = got
        for (q, val, bnd), g in zip(R.read(prefix), got):
            slack = R.boo.edge if prefix == "boo" and q in ("hist_q", "hist_qbar") else 0
            _compare(KEYWORD[prefix], step, q, g, val, bnd, margins, slack)
    # the objects hold what the last read returned
    for prefix, got in last.items():
        name = KEYWORD[prefix]
        for q, g, o in zip(READ_NAMES[prefix], got, _object_fields(name, samplers[name])):
            _compare(name, total_steps - 1, "object." + q, o, g, None, margins)
    return margins


def expected(frames, setups, samplers, restatement, total_steps, frequency, **walk):
    """What every attached sampler's accumulators must hold after the run: {keyword: [(quantity, value, bound or None)]},
    restated from the recorded `frames` (by step) alone, walking the run by the samplers' documented rules (`walk`: the
    further arguments of expected_trace).  `setups` are the recorded *_setup calls (the configuration the run was given)."""
    want, _ = expected_trace(samplers, total_steps, frequency, **walk)
    for name, args, kw in setups:
        if name != "swap_setup":
            getattr(restatement, name)(*args, **kw)
    used = []
    for step, method, args in want:
        prefix = SAMPLER_CALLS.get(method)
        if prefix is not None:
            restatement.set_frame(frames[step])
            getattr(restatement, method)(*args)
            if prefix not in used:
                used.append(prefix)
    return {KEYWORD[p]: restatement.read(p) for p in used}


def margins_lines(case, margins):
    return ["%s %s %s %.3e" % (case, s, q, m) for (s, q), m in sorted(margins.items())]
