"""A chaos-free audit of a step loop against the CPU oracle, one short segment at a time.

Long trajectory comparisons are limited by chaos to 1e-9 .. 1e-8: a single neighbour dropped near r_c (|F(r_c)| = 0.039 on
one particle) or a drift applied twice in a redo branch can hide in them.  audit_run() never lets an error age: the step
loop under test (a "stepper": upload / run / download / stats, the shape of MDDevice) runs a schedule of short segments,
and after every segment two things are checked against the oracle, RESTARTED FROM THE STEPPER'S OWN STATE:

  (A) force completeness.  The forces the stepper holds must be oracle.forces_brute at the positions the stepper holds, to
      the suite's single-evaluation tolerance (tests/test_gpu_parity.py: 1e-11 * max(1, |F|inf); pseudo hard spheres
      1e-10), and -- when the segment's last step was an energy step -- U and W at those positions to 1e-12 (pseudo hard
      spheres 1e-10) and K = oracle.kinetic(v) to 1e-12.  No trajectory enters: whatever row the last step walked (outer,
      inner, freshly pruned, freshly built) has to hold every neighbour within the cutoff.
  (B) shadow step.  oracle.run from the state at the segment's START for the segment's k steps (brute force, the same
      thermostat draws) must land on the stepper's end state, compared on unwrapped coordinates x + U * image:
        k == 1, diagonal cell   the derived one-step bound: |dx| <= 8 * spacing(max L) (two download-wrap roundings at each
                                end, at most four differing roundings of x + (v + f dt/2) dt; the new force does not enter
                                x) and |dv| <= 0.5 dt tol_F + 4 spacing(|v|inf), plus 1e-12 |v|inf under NVT (the K
                                tolerance through Bussi's scale)
        k <= 10 otherwise       1e-10 absolute on x and v (tests/test_gpu_parity.py::test_nve_trajectory_10_steps)
        k > 10                  (A) only
      Image counters must be equal, except for a particle whose oracle coordinate lies within the x bound of a face: at
      most one over the whole run.

The `thermo` flag alternates -- separately among the one-step segments and among the longer ones, so that each class sees
both values -- which makes the audited last steps come from the energy kernels and from the no-energy kernels alike.

Knife edges.  The state a stepper hands out can differ from the one it computed on by an ulp of L (the wrap at download),
which may move a pair across an acceptance threshold d2 <= cutoff^2 (or the potential's own cutoff).  For every audited
state the pairs whose reference-form d2 lies within 1e-9 (relative) of such a threshold are found with numpy and their
particles left out of (A) for that state (U and W too).  This is a cap, not a tolerance: more than two particles over a
whole run is a failure.

Every segment is also classified from the stats() delta: a one-step segment's step followed a list build ("after_rebuild"),
was a prune step ("prune") or walked the rows it found ("ordinary"); a longer segment's last step is known to be "ordinary"
only if the whole segment saw neither a prune nor a build ("unknown" otherwise).

The Brownian loop and the FIRE minimiser have modes of their own, audit_brownian and audit_fire (with
audit_fire_convergence), on the same ledger, knife edges and image exceptions: see the comment block above BD_MIXED.
The slab-decomposed loops (DomainDevice.run / run_async / run_native) are audited by audit_run through a multi-process
stepper, tests/domain_audit_worker.py.
"""
import contextlib

import numpy as np

NVE, NVT = 0, 1
POT_LJ, POT_PSEUDOHS, POT_POLYDISPERSE, POT_LJ_MODIFIED = 0, 1, 2, 3
PSEUDOHS_B = 1.0204081632653061      # the pseudo-hard-sphere potential's own cutoff (oracle/md_oracle.c b_param)
KNIFE_REL = 1e-9
MAX_EXCLUDED = 2
MAX_IMAGE_EXCEPTIONS = 1
SHORT_TOL = 1e-10                    # x and v after <= 10 steps
SHORT_STEPS = 10

# The two schedules of segment lengths.  MIXED: one-step segments (whose step kind the stats() delta tells exactly) between
# windows of every length up to 14, which see scheduled list builds.  ONES: one-step calls only -- with nsteps == 1 the
# planner's scheduled build (s < nsteps) can never fire, so every list build goes through the violation-redo branch of md_run.
MIXED = (1, 1, 2, 1, 5, 1, 9, 1, 3, 1, 14, 1, 7, 1, 10, 1, 6, 1, 12, 1)
ONES = (1,) * 60


class AuditFailure(AssertionError):
    """check: 'A' (force completeness), 'B' (shadow step) or 'precondition'; what: the quantity that missed its bound."""

    def __init__(self, check, what, msg):
        super().__init__("(%s) %s: %s" % (check, what, msg))
        self.check = check
        self.what = what


def force_tolerance(pot):
    return 1e-10 if pot.kind == POT_PSEUDOHS else 1e-11


def energy_tolerance(pot):
    return 1e-10 if pot.kind == POT_PSEUDOHS else 1e-12


def thermo_flags(schedule, first=True):
    """The thermo flag of every segment: alternating among the one-step segments and, separately, among the longer ones."""
    one, many, out = first, first, []
    for k in schedule:
        if k == 1:
            out.append(one)
            one = not one
        else:
            out.append(many)
            many = not many
    return out


def cell_matrix(box, cell):
    return np.diag(np.asarray(box, dtype=np.float64)) if cell is None else np.asarray(cell, dtype=np.float64)


def pair_d2(x, box, cell=None):
    """(n, n) squared minimum-image separations.  Diagonal cell: the reference form (oracle/md_oracle.c canon_d2: b's
    translated image rounded once, products and sums rounded left to right), oriented a = row < b = column.  General cell:
    the image chosen in fractional coordinates (unique below half the face distance); its last bits are not the
    reference's, which a relative window of 1e-9 does not see."""
    x = np.asarray(x, dtype=np.float64)
    d = x.shape[1]
    if cell is None:
        L = np.asarray(box, dtype=np.float64)
        d2 = None
        for c in range(d):
            xa, xb = x[:, None, c], x[None, :, c]
            d0 = xb - xa
            s = np.where(d0 > 0.5 * L[c], -1.0, np.where(d0 < -0.5 * L[c], 1.0, 0.0))
            dl = (xb + s * L[c]) - xa
            d2 = dl * dl if d2 is None else d2 + dl * dl
        return d2
    U = np.asarray(cell, dtype=np.float64)
    dl = x[None, :, :] - x[:, None, :]
    fr = dl @ np.linalg.inv(U).T
    dl = dl - np.rint(fr) @ U.T
    return (dl * dl).sum(axis=2)


def pair_thresholds(pot, cutoff, diam):
    """The squared acceptance thresholds of a pair: the list cutoff and the potential's own cutoff (a scalar, or an (n, n)
    array where it depends on the pair)."""
    thr = [float(cutoff) ** 2]
    p = pot.p
    if pot.kind in (POT_LJ, POT_LJ_MODIFIED):
        thr.append(float(p[2]) ** 2)
    elif pot.kind == POT_PSEUDOHS:
        thr.append(PSEUDOHS_B ** 2)
    elif pot.kind == POT_POLYDISPERSE:
        s1, s2 = diam[:, None], diam[None, :]
        se = 0.5 * (s1 + s2) * (1.0 - p[1] * np.abs(s1 - s2))
        thr.append((p[0] * se) ** 2)
    return thr


def knife_edge_particles(x, box, cell, thresholds, rel=KNIFE_REL):
    """Indices of the particles of every pair whose d2 lies within `rel` (relative) of one of the thresholds."""
    d2 = pair_d2(x, box, cell)
    n = d2.shape[0]
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    hit = np.zeros((n, n), dtype=bool)
    for t in thresholds:
        hit |= np.abs(d2 - t) <= rel * t
    i, j = np.nonzero(hit & upper)
    return np.union1d(i, j)


def face_distance(x, box, cell=None):
    """Distance of every particle to the nearest face of the cell, per particle."""
    if cell is None:
        L = np.asarray(box, dtype=np.float64)
        return np.minimum(np.abs(x), np.abs(L - x)).min(axis=1)
    Uinv = np.linalg.inv(np.asarray(cell, dtype=np.float64))
    perp = 1.0 / np.linalg.norm(Uinv, axis=1)
    fr = x @ Uinv.T
    return (np.minimum(np.abs(fr), np.abs(1.0 - fr)) * perp).min(axis=1)


class Ledger:
    """What every mode of the audit keeps: the worst error of each quantity as a fraction of its bound, the misses, the
    particles the knife-edge precondition left out and the image exceptions, with their caps."""

    def __init__(self, keys, box, cell, thresholds):
        self.worst = {k: 0.0 for k in keys}
        self.failures, self.excluded, self.image_exc = [], set(), set()
        self.box, self.cell, self.thresholds = box, cell, thresholds

    def miss(self, check, what, msg):
        self.failures.append(AuditFailure(check, what, msg))

    def note(self, key, err, bound):
        """Records err / bound; True if the bound is missed."""
        with np.errstate(over="ignore"):
            self.worst[key] = max(self.worst[key], float(err) / bound if np.isfinite(err) else np.inf)
        return not (err <= bound)

    def knife(self, x):
        """(knife-edge particles at x, mask of the others); the particles join the excluded set."""
        knife = knife_edge_particles(x, self.box, self.cell, self.thresholds)
        self.excluded.update(int(i) for i in knife)
        keep = np.ones(len(x), dtype=bool)
        keep[knife] = False
        return knife, keep

    def images(self, where, img, ref_x, ref_img, xb, check="B"):
        """Image counters must be equal, except for a particle whose oracle coordinate lies within xb of a face."""
        differ = np.flatnonzero((img != ref_img).any(axis=1))
        if differ.size:
            near = face_distance(ref_x, self.box, self.cell)[differ] <= xb
            self.image_exc.update(int(i) for i in differ[near])
            if not near.all() or len(self.image_exc) > MAX_IMAGE_EXCEPTIONS:
                self.miss(check, "img", "%s: image counters differ for particles %s" % (where, differ[:8].tolist()))

    def close_segment(self, where, raise_on_failure):
        if len(self.excluded) > MAX_EXCLUDED:
            self.miss("precondition", "knife", "%s: %d particles on a knife edge so far" % (where, len(self.excluded)))
        if self.failures and raise_on_failure:
            raise self.failures[0]

    def result(self, segments, stats):
        return dict(worst=self.worst, segments=segments, excluded=sorted(self.excluded),
                    image_exceptions=sorted(self.image_exc), failures=self.failures, stats=stats)


def audit_run(stepper, oracle, system, pot, cutoff, dt, schedule, ensemble=NVE, tau=0.1, ktemp=None, r1=None, r2=None,
              cell=None, raise_on_failure=True):
    """Runs `schedule` (segment lengths) on `stepper` from `system` and audits every segment as the module docstring says.
    `pot` is the oracle's potential (the stepper is already configured with the same one); `cell`: a general unit cell
    (columns = lattice vectors), audited under oracle.set_cell.  NVT takes per-step ktemp / r1 / r2 for the whole schedule.

    Returns dict(worst, segments, excluded, image_exceptions, failures, stats): worst[q] is the largest observed error of
    q as a fraction of its bound (F, U, W, K: check (A); x1, v1: the derived one-step bounds; x, v: the 1e-10 of longer
    segments and of general cells), segments a list of dict(k, thermo, kind, prunes, rebuilds, violations), excluded the
    particles the precondition left out.  With raise_on_failure the first miss raises AuditFailure at the end of its
    segment; without, the misses are collected in failures and the run goes on."""
    n, dim = system["x"].shape
    box = np.asarray(system["box"], dtype=np.float64)
    diam = np.asarray(system["diam"], dtype=np.float64)
    U = cell_matrix(box, cell)
    Lmax = float(np.abs(U).sum(axis=1).max()) if cell is not None else float(box.max())
    ftol, etol = force_tolerance(pot), energy_tolerance(pot)
    thresholds = pair_thresholds(pot, cutoff, diam)
    nf = dim * (n - 1.0)
    nvt = ensemble == NVT
    total = int(sum(schedule))
    if nvt:
        ktemp, r1, r2 = (np.ascontiguousarray(a, dtype=np.float64) for a in (ktemp, r1, r2))
        assert min(ktemp.size, r1.size, r2.size) >= total
    led = Ledger(("F", "U", "W", "K", "x1", "v1", "x", "v"), box, cell, thresholds)
    segments = []
    note, miss = led.note, led.miss

    with (oracle.set_cell(cell) if cell is not None else contextlib.nullcontext()):
        f0 = oracle.forces_brute(system["x"], box, cutoff, pot, diam)[0]
        stepper.upload(system["x"], system["v"], f0, system["img"], diam)
        start = stepper.download()
        a = 0
        for seg, (k, thermo) in enumerate(zip(schedule, thermo_flags(schedule))):
            where = "segment %d (steps %d..%d, thermo=%s)" % (seg, a, a + k - 1, thermo)
            before = stepper.stats()
            kw = dict(ensemble=NVT, tau=tau, nf=nf, ktemp=ktemp[a:a + k], r1=r1[a:a + k], r2=r2[a:a + k]) if nvt else {}
            uwk = stepper.run(k, dt, thermo=thermo, **kw)
            x, v, f, img = end = stepper.download()
            after = stepper.stats()
            delta = {key: int(after[key] - before[key]) for key in ("prunes", "rebuilds", "violations")}
            if k == 1:
                kind = "after_rebuild" if delta["rebuilds"] else ("prune" if delta["prunes"] else "ordinary")
            else:
                kind = "unknown" if (delta["prunes"] or delta["rebuilds"]) else "ordinary"
            segments.append(dict(k=k, thermo=thermo, kind=kind, **delta))

            # ---- (A) force completeness at the stepper's own positions
            f_ref, u_ref, w_ref, _ = oracle.forces_brute(x, box, cutoff, pot, diam)
            knife, keep = led.knife(x)
            tol_f = ftol * max(1.0, float(np.abs(f_ref).max()))
            err = np.abs(f - f_ref)[keep].max() if keep.any() else 0.0
            if note("F", err, tol_f):
                i = int(np.argmax(np.abs(f - f_ref).max(axis=1) * keep))
                miss("A", "F", "%s, %s step: |dF|inf = %.3e > %.3e (particle %d)" % (where, kind, err, tol_f, i))
            if thermo:
                if uwk is None:
                    miss("A", "U", "%s: no U, W, K returned" % where)
                else:
                    if len(knife) == 0:
                        for key, got, ref in (("U", uwk[0], u_ref), ("W", uwk[1], w_ref)):
                            bound = etol * max(1.0, abs(ref))
                            if note(key, abs(got - ref), bound):
                                miss("A", key, "%s, %s step: %s = %.17g, oracle %.17g, |d| = %.3e > %.3e"
                                     % (where, kind, key, got, ref, abs(got - ref), bound))
                    k_ref = oracle.kinetic(v)
                    bound = 1e-12 * max(abs(k_ref), np.finfo(float).tiny)
                    if note("K", abs(uwk[2] - k_ref), bound):
                        miss("A", "K", "%s: K = %.17g, oracle %.17g" % (where, uwk[2], k_ref))

            # ---- (B) shadow step from the state at the segment's start
            if k <= SHORT_STEPS:
                x0, v0, f_start, img0 = start
                kw = dict(ensemble=1, tau=tau, ktemp=ktemp[a:a + k], r1=r1[a:a + k], r2=r2[a:a + k]) if nvt else {}
                ref = oracle.run(x0, img0, v0, f_start, diam, box, cutoff, pot, dt, k, use_cells=False, **kw)
                vinf = float(np.abs(ref["v"]).max())
                if k == 1 and cell is None:
                    xb = 8.0 * float(np.spacing(Lmax))
                    vb = 0.5 * dt * tol_f + 4.0 * float(np.spacing(vinf)) + (1e-12 * vinf if nvt else 0.0)
                    xkey, vkey = "x1", "v1"
                else:
                    xb = vb = SHORT_TOL
                    xkey, vkey = "x", "v"
                dx = np.abs((x - ref["x"]) + (img - ref["img"]) @ U.T)
                dv = np.abs(v - ref["v"])
                if note(xkey, dx.max(), xb):
                    miss("B", "x", "%s: |dx|inf = %.3e > %.3e (particle %d)" % (where, dx.max(), xb, int(dx.max(axis=1).argmax())))
                if note(vkey, dv.max(), vb):
                    miss("B", "v", "%s: |dv|inf = %.3e > %.3e (particle %d)" % (where, dv.max(), vb, int(dv.max(axis=1).argmax())))
                led.images(where, img, ref["x"], ref["img"], xb)
            led.close_segment(where, raise_on_failure)
            start = end
            a += k
        stats = stepper.stats()
    return led.result(segments, stats)


def coverage(result):
    """{(kind, thermo): number of audited last steps}"""
    out = {}
    for s in result["segments"]:
        out[(s["kind"], s["thermo"])] = out.get((s["kind"], s["thermo"]), 0) + 1
    return out


def margins_line(name, result):
    """One line per case for the records: the worst force, x and v error as a fraction of its bound."""
    w = result["worst"]
    return ("%-28s F %.3f  U %.3f  W %.3f  K %.3f | one step: x %.3f  v %.3f | <= 10 steps: x %.2e  v %.2e | excluded %d"
            % (name, w["F"], w["U"], w["W"], w["K"], w["x1"], w["v1"], w["x"], w["v"], len(result["excluded"])))


class OracleStepper:
    """The stepper interface on top of the oracle's own step functions (velocity Verlet, brute-force forces): what
    audit_run must pass on, and the base of the sabotaged steppers of tests/test_step_audit.py."""

    def __init__(self, oracle, box, cutoff, pot):
        self.o, self.box, self.cutoff, self.pot = oracle, np.asarray(box, dtype=np.float64), cutoff, pot
        self.step = 0           # steps taken since upload

    def upload(self, x, v, f, images, diameters):
        self.x, self.v, self.f = (np.array(a, dtype=np.float64) for a in (x, v, f))
        self.img = np.array(images, dtype=np.int32)
        self.diam = np.array(diameters, dtype=np.float64)
        self.step = 0

    def download(self):
        return self.x.copy(), self.v.copy(), self.f.copy(), self.img.copy()

    def stats(self):
        return dict(steps=self.step, prunes=0, rebuilds=0, violations=0, fused=0)

    # the three places a sabotaged stepper reaches into
    def forces(self, x):
        f, u, w, _ = self.o.forces_brute(x, self.box, self.cutoff, self.pot, self.diam)
        return f, u, w

    def drift(self, dt):
        self.o.integrate_half(self.x, self.img, self.v, self.f, dt, self.box)

    def run(self, nsteps, dt, ensemble=NVE, tau=0.0, nf=None, ktemp=None, r1=None, r2=None, thermo=True):
        u = w = 0.0
        for t in range(nsteps):
            self.drift(dt)
            self.f, u, w = self.forces(self.x)
            self.o.integrate_second_half(self.v, self.f, dt)
            if ensemble == NVT:
                self.o.bussi(self.v, float(ktemp[t]), nf, dt, tau, float(r1[t]), float(r2[t]))
            self.step += 1
        return (u, w, self.o.kinetic(self.v)) if thermo else None


# =================================================================================================================
# The other two device loops: Brownian dynamics (md_run_brownian) and the FIRE minimiser (md_fire_minimize).
#
# Both are audited the same way, with two differences in what a segment leaves behind.
#
# Brownian.  A step evaluates the forces at x and then moves, so the forces a run of k steps leaves are those of its LAST
# evaluation, at the positions BEFORE the last move.  (A) for k == 1 is therefore forces_brute at the segment's start (no
# trajectory enters), and for k > 1 the shadow's last evaluation, whose positions carry the segment's trajectory error:
# bound tol_F + 1e-10 |F|inf for k <= 10 (the x bound through a force gradient of order |F|inf per unit length), and the
# project's long-run bound 1e-8 max(1, |F|inf) beyond.  U and W of that evaluation: the energy tolerance plus the x bound
# through sum_i |f_i| (dU = -sum f_i dx_i), for W with the factor 64 >= 1 + the steepest exponent of the suite's potentials
# (r dF/dr = -(m + 1) F for a power law r^-m; pseudo hard spheres m = 50).  The knife-edge precondition is evaluated where
# that evaluation took place (k > 1: the shadow's positions after k - 1 steps).
# (B) one step, diagonal cell: |dx| <= 8 spacing(Lmax) + (dt / kT) tol_F -- the eight roundings of the MD bound, and the
# force now enters x, with weight dt / kT.  1 < k <= 10 and every segment in a general cell: 1e-10.  k > 10: 1e-9
# (tests/test_brownian.py).  Segments chain through first_step, so the noise counter is the global step throughout.
# The virial: virial_count is the number of global steps g of the segment with g % virial_every == 0, virial_sum the
# shadow's to 1e-12 relative (pseudo hard spheres: the energy tolerance, relative).
#
# FIRE.  Every call restarts the minimiser's own state (v = 0, dt = dt_initial, alpha = alpha0), so a segment is a run
# of max_steps = k that cannot converge (tol = 1e-300).  Its closing evaluation is at the positions it leaves: (A) is
# exact at the held positions, f_rms included.  (B): a numpy restatement of the algorithm (FireRestated) from the
# segment's start; one step in a diagonal cell |dx| <= 8 spacing(Lmax) + dt_initial^2 tol_F (x += dt (dt f)), <= 10
# steps 1e-10, beyond 1e-9.  Convergence is audited apart (audit_fire_convergence).
# =================================================================================================================
BD_MIXED = (1, 1, 2, 1, 5, 1, 9, 1, 3, 1, 10, 1, 7, 1, 10, 1, 6, 1, 8, 1)
BD_CHUNKS = (31, 32, 33, 64, 65)      # across the 32-step host chunk, with and without a remainder
FIRE_MIXED = (0, 1, 1, 2, 5, 9, 14, 10, 3, 33, 7)
LONG_X_TOL = 1e-9                     # x after > 10 steps (tests/test_brownian.py, tests/test_fire.py)
LONG_F_TOL = 1e-8                     # f after > 10 steps, times max(1, |F|inf)
W_SLOPE = 64.0                        # |dW| <= W_SLOPE sum_i |f_i| |dx|: see above
NEVER = 1e-300                        # a FIRE tolerance no force meets


def wrap_np(x, img, box, cell=None, cell_inv=None):
    """oracle/md_oracle.c wrap1 / wrap_tric restated, operation for operation: (wrapped x, images) as new arrays."""
    img = img.copy()
    if cell is None:
        L = np.asarray(box, dtype=np.float64)
        frac = (1.0 / L) * x
        nn = np.floor(frac)
        img += nn.astype(np.int32)
        return L * (frac - nn), img
    d = x.shape[1]
    U, Ui = np.asarray(cell, dtype=np.float64), np.asarray(cell_inv, dtype=np.float64)

    def rows(M, y):
        out = np.empty_like(y)
        for r in range(d):
            a = M[r, 0] * y[:, 0] + M[r, 1] * y[:, 1]
            out[:, r] = a + M[r, 2] * y[:, 2] if d == 3 else a
        return out
    frac = rows(Ui, x)
    nn = np.floor(frac)
    img += nn.astype(np.int32)
    return rows(U, frac - nn), img


def philox_np(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays (or scalars) of counter and key words; returns the four output words as uint64 arrays."""
    m = np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    c0, c1, c2, c3, k0, k1 = (np.asarray(a, dtype=np.uint64) & m for a in np.broadcast_arrays(c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m, (p0 >> s32) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m, (k1 + np.uint64(0xBB67AE85)) & m
    return c0, c1, c2, c3


def _unwrapped_diff(x, img, ref_x, ref_img, U):
    return np.abs((x - ref_x) + (img - ref_img) @ U.T)


def _x_bound(k, cell, one_step):
    """(bound, key of `worst`) of the unwrapped positions after k moves."""
    if k == 1 and cell is None:
        return one_step, "x1"
    if k <= SHORT_STEPS or cell is not None:
        return SHORT_TOL, "x"
    return LONG_X_TOL, "xl"


class _Setup:
    """The quantities all modes derive from (system, pot, cutoff, cell)."""

    def __init__(self, system, pot, cutoff, cell):
        self.n, self.dim = system["x"].shape
        self.box = np.asarray(system["box"], dtype=np.float64)
        self.diam = np.asarray(system["diam"], dtype=np.float64)
        self.cell = cell
        self.U = cell_matrix(self.box, cell)
        self.Lmax = float(np.abs(self.U).sum(axis=1).max()) if cell is not None else float(self.box.max())
        self.ftol, self.etol = force_tolerance(pot), energy_tolerance(pot)
        self.thresholds = pair_thresholds(pot, cutoff, self.diam)

    def ledger(self, keys):
        return Ledger(keys, self.box, self.cell, self.thresholds)


def audit_brownian(stepper, oracle, system, pot, cutoff, dt, ktemp, seed, schedule, first_step=0, virial_every=10,
                   cell=None, raise_on_failure=True):
    """The Brownian mode: `stepper` has upload / download / stats and run_brownian(nsteps, dt, ktemp, seed, first_step,
    virial_every) -> dict(U, W, virial_sum, virial_count), the shape of MDDevice.  Checks as the comment block above says.
    worst: F U W (k <= 10), Fl (k > 10), V (virial sum), x1 (one step), x (<= 10 steps, general cell), xl (> 10 steps);
    segments: dict(k, g0, rebuilds, violations)."""
    su = _Setup(system, pot, cutoff, cell)
    box, diam, n = su.box, su.diam, su.n
    led = su.ledger(("F", "U", "W", "Fl", "V", "x1", "x", "xl"))
    note, miss = led.note, led.miss
    segments = []
    kw = dict(use_cells=False, nthreads=1, virial_every=virial_every)
    with (oracle.set_cell(cell) if cell is not None else contextlib.nullcontext()):
        f0 = oracle.forces_brute(system["x"], box, cutoff, pot, diam)[0]
        stepper.upload(system["x"], system["v"], f0, system["img"], diam)
        start = stepper.download()
        g0 = int(first_step)
        for seg, k in enumerate(schedule):
            where = "segment %d (global steps %d..%d)" % (seg, g0, g0 + k - 1)
            before = stepper.stats()
            got = stepper.run_brownian(k, dt, ktemp, seed, first_step=g0, virial_every=virial_every)
            x, v, f, img = end = stepper.download()
            after = stepper.stats()
            segments.append(dict(k=k, g0=g0, **{key: int(after[key] - before[key]) for key in ("rebuilds", "violations")}))

            # ---- the shadow: k - 1 steps, then the last one (the same arithmetic as k steps in one call)
            x0, _, _, img0 = start
            head = oracle.run_brownian(x0, img0, diam, box, cutoff, pot, dt, ktemp, seed, k - 1, first_step=g0, **kw)
            ref = oracle.run_brownian(head["x"], head["img"], diam, box, cutoff, pot, dt, ktemp, seed, 1,
                                      first_step=g0 + k - 1, **kw)
            finf = float(np.abs(ref["f"]).max())
            tol_f = su.ftol * max(1.0, finf)
            xb, xkey = _x_bound(k, cell, 8.0 * float(np.spacing(su.Lmax)) + (dt / ktemp) * tol_f)

            # ---- (A) the forces of the last evaluation, at the positions before the last move
            knife, keep = led.knife(head["x"])
            if k == 1:
                fb, fkey, slope = tol_f, "F", 0.0
            elif k <= SHORT_STEPS:
                fb, fkey, slope = tol_f + SHORT_TOL * finf, "F", SHORT_TOL
            else:
                fb, fkey, slope = LONG_F_TOL * max(1.0, finf), "Fl", LONG_X_TOL
            err = np.abs(f - ref["f"])[keep].max() if keep.any() else 0.0
            if note(fkey, err, fb):
                i = int(np.argmax(np.abs(f - ref["f"]).max(axis=1) * keep))
                miss("A", "F", "%s: |dF|inf = %.3e > %.3e (particle %d)" % (where, err, fb, i))
            if len(knife) == 0:
                f1 = float(np.abs(ref["f"]).sum())
                for key, mult in (("U", 1.0), ("W", W_SLOPE)):
                    bound = su.etol * max(1.0, abs(ref[key])) + mult * slope * f1
                    if note(key, abs(got[key] - ref[key]), bound):
                        miss("A", key, "%s: %s = %.17g, oracle %.17g, |d| = %.3e > %.3e"
                             % (where, key, got[key], ref[key], abs(got[key] - ref[key]), bound))

            # ---- (B) the end state
            dx = _unwrapped_diff(x, img, ref["x"], ref["img"], su.U)
            if note(xkey, dx.max(), xb):
                miss("B", "x", "%s: |dx|inf = %.3e > %.3e (particle %d)" % (where, dx.max(), xb, int(dx.max(axis=1).argmax())))
            led.images(where, img, ref["x"], ref["img"], xb)
            if not np.array_equal(v, system["v"]):
                miss("B", "v", "%s: the velocities are not the uploaded ones" % where)

            # ---- the virial bookkeeping, on the global step
            count = sum(1 for g in range(g0, g0 + k) if g % virial_every == 0)
            vsum = head["virial_sum"] + ref["virial_sum"]
            assert count == head["virial_count"] + ref["virial_count"]
            if got["virial_count"] != count:
                miss("V", "count", "%s: virial_count = %g, %d steps sampled" % (where, got["virial_count"], count))
            bound = su.etol * max(abs(vsum), np.finfo(float).tiny)
            if note("V", abs(got["virial_sum"] - vsum), bound):
                miss("V", "sum", "%s: virial_sum = %.17g, oracle %.17g" % (where, got["virial_sum"], vsum))

            led.close_segment(where, raise_on_failure)
            start = end
            g0 += k
        stats = stepper.stats()
    return led.result(segments, stats)


class FireRestated:
    """fire_minimize! restated in numpy over oracle.forces_brute (oracle/md_oracle.c oracle_fire_minimize, statement for
    statement; the sums are numpy's, so P, |v| and |f| differ from the C loop's in the last bits).  run() also returns
    `trace`, one dict(P, branch, f_rms, energy, dt, finf) per executed step -- branch 'accelerate' (P > 0 past nmin: dt
    and alpha change), 'hold' (P > 0), 'reset' (P <= 0) or 'converged' -- and `hist`, the (x, img) every evaluation,
    the closing one included, took place at.  The three pieces a sabotaged copy overrides are methods."""

    def __init__(self, oracle, box, cutoff, pot, diam, cell=None):
        self.o, self.box, self.cutoff, self.pot, self.diam, self.cell = oracle, box, cutoff, pot, diam, cell
        self.cell_inv = oracle.set_cell.inverse() if cell is not None else None

    mix_first = True      # the mix comes before the sign test of P, with the alpha of this step

    def mix(self, v, f, alpha, vn, fn):
        return (1.0 - alpha) * v + (alpha * (vn / fn)) * f

    def update(self, P, dt, alpha, since_neg, kw):
        """-> (dt, alpha, since_neg, branch)"""
        if P > 0.0:
            since_neg += 1
            if since_neg > kw["nmin"]:
                return min(dt * kw["f_inc"], kw["dt_max"]), alpha * 0.99, since_neg, "accelerate"
            return dt, alpha, since_neg, "hold"
        return max(dt * kw["f_dec"], kw["dt_initial"]), kw["alpha0"], 0, "reset"

    def drift(self, x, img, v, dt_new, dt_old):
        return wrap_np(x + dt_new * v, img, self.box, self.cell, self.cell_inv)

    def converging_step(self, x, img, v, f, dt):
        return x, img

    def run(self, x, img, max_steps, tol, dt_initial=0.01, dt_max=0.1, alpha0=0.1, f_inc=1.2, f_dec=0.2, nmin=5):
        kw = dict(dt_initial=dt_initial, dt_max=dt_max, alpha0=alpha0, f_inc=f_inc, f_dec=f_dec, nmin=nmin)
        x, img = np.array(x, dtype=np.float64), np.array(img, dtype=np.int32)
        n, dim = x.shape
        v = np.zeros_like(x)
        alpha, dt, ndof, since_neg, steps, converged = alpha0, dt_initial, dim * (n - 1.0), 0, 0, False
        trace, hist = [], []
        for step in range(1, max_steps + 2):
            f, u, _, _ = self.o.forces_brute(x, self.box, self.cutoff, self.pot, self.diam)
            hist.append((x.copy(), img.copy()))
            fn = float(np.sqrt((f * f).sum(axis=1).sum()))
            f_rms = fn / np.sqrt(ndof)
            if step == max_steps + 1:
                break
            steps += 1
            rec = dict(f_rms=f_rms, energy=u, dt=dt, finf=float(np.abs(f).max()), P=0.0, branch="converged")
            trace.append(rec)
            if f_rms < tol:
                converged = True
                x, img = self.converging_step(x, img, v, f, dt)
                break
            v = v + dt * f
            P = float((v * f).sum(axis=1).sum())
            vn = float(np.sqrt((v * v).sum(axis=1).sum()))
            dt_old, alpha_old = dt, alpha
            if self.mix_first and vn > 0.0 and fn > 0.0:
                v = self.mix(v, f, alpha_old, vn, fn)
            dt, alpha, since_neg, branch = self.update(P, dt, alpha, since_neg, kw)
            if not self.mix_first and vn > 0.0 and fn > 0.0:
                v = self.mix(v, f, alpha, vn, fn)
            if branch == "reset":
                v = np.zeros_like(x)
            rec.update(P=P, branch=branch)
            x, img = self.drift(x, img, v, dt, dt_old)
        return dict(x=x, img=img, f=f, steps=steps, converged=converged, energy=u, f_rms=f_rms, trace=trace, hist=hist)


def audit_fire(stepper, oracle, system, pot, cutoff, fire_kw, schedule, cell=None, raise_on_failure=True):
    """The FIRE mode: `stepper` has upload / download / stats and fire_minimize(max_steps, tol, **fire_kw) ->
    dict(steps, converged, energy, f_rms).  worst: F U R (f_rms) of check (A); x1, x, xl as in the Brownian mode.
    segments: dict(k, rebuilds, violations, branches) with the shadow's branches of that segment."""
    su = _Setup(system, pot, cutoff, cell)
    box, diam, n = su.box, su.diam, su.n
    led = su.ledger(("F", "U", "R", "x1", "x", "xl"))
    note, miss = led.note, led.miss
    segments = []
    dt0 = float(fire_kw.get("dt_initial", 0.01))
    with (oracle.set_cell(cell) if cell is not None else contextlib.nullcontext()):
        shadow = FireRestated(oracle, box, cutoff, pot, diam, cell)
        f0 = oracle.forces_brute(system["x"], box, cutoff, pot, diam)[0]
        stepper.upload(system["x"], system["v"], f0, system["img"], diam)
        start = stepper.download()
        a = 0
        for seg, k in enumerate(schedule):
            where = "segment %d (steps %d..%d)" % (seg, a, a + k - 1)
            before = stepper.stats()
            got = stepper.fire_minimize(max_steps=k, tol=NEVER, **fire_kw)
            x, v, f, img = end = stepper.download()
            after = stepper.stats()
            x0, _, _, img0 = start
            ref = shadow.run(x0, img0, k, NEVER, **fire_kw)
            segments.append(dict(k=k, branches=[t["branch"] for t in ref["trace"]],
                                 **{key: int(after[key] - before[key]) for key in ("rebuilds", "violations")}))
            if got["steps"] != k or got["converged"]:
                miss("B", "steps", "%s: steps = %d, converged = %s" % (where, got["steps"], got["converged"]))

            # ---- (A) the closing evaluation, at the positions the stepper holds
            f_ref, u_ref, _, _ = oracle.forces_brute(x, box, cutoff, pot, diam)
            knife, keep = led.knife(x)
            tol_f = su.ftol * max(1.0, float(np.abs(f_ref).max()))
            err = np.abs(f - f_ref)[keep].max() if keep.any() else 0.0
            if note("F", err, tol_f):
                i = int(np.argmax(np.abs(f - f_ref).max(axis=1) * keep))
                miss("A", "F", "%s: |dF|inf = %.3e > %.3e (particle %d)" % (where, err, tol_f, i))
            if len(knife) == 0:
                bound = su.etol * max(1.0, abs(u_ref))
                if note("U", abs(got["energy"] - u_ref), bound):
                    miss("A", "U", "%s: energy = %.17g, oracle %.17g" % (where, got["energy"], u_ref))
                r_ref = float(np.sqrt((f_ref * f_ref).sum())) / np.sqrt(su.dim * (n - 1.0))
                if note("R", abs(got["f_rms"] - r_ref), 1e-12 * max(r_ref, np.finfo(float).tiny)):
                    miss("A", "f_rms", "%s: f_rms = %.17g, oracle %.17g" % (where, got["f_rms"], r_ref))

            # ---- (B) the restated algorithm from the segment's start
            finf0 = ref["trace"][0]["finf"] if ref["trace"] else 0.0
            xb, xkey = _x_bound(k, cell, 8.0 * float(np.spacing(su.Lmax)) + dt0 * dt0 * su.ftol * max(1.0, finf0))
            dx = _unwrapped_diff(x, img, ref["x"], ref["img"], su.U)
            if note(xkey, dx.max(), xb):
                miss("B", "x", "%s: |dx|inf = %.3e > %.3e (particle %d)" % (where, dx.max(), xb, int(dx.max(axis=1).argmax())))
            led.images(where, img, ref["x"], ref["img"], xb)
            if not np.array_equal(v, system["v"]):
                miss("B", "v", "%s: the MD velocities are not the uploaded ones" % where)
            led.close_segment(where, raise_on_failure)
            start = end
            a += k
        stats = stepper.stats()
    return led.result(segments, stats)


def pick_tolerance(f_rms, j):
    """A tolerance at which evaluation j (1-based) is the first to converge: the midpoint between its f_rms and the
    smallest earlier one (j == 1: twice its f_rms -- nothing precedes it), or None if the two are closer than 1e-6
    relative or evaluation j is not the smallest so far."""
    r = float(f_rms[j - 1])
    if j == 1:
        return 2.0 * r
    prev = float(min(f_rms[:j - 1]))
    if not (prev - r >= 1e-6 * prev):
        return None
    return 0.5 * (prev + r)


def audit_fire_convergence(stepper, oracle, system, pot, cutoff, fire_kw, cell=None, wanted=(1, 16, 32), horizon=40,
                           raise_on_failure=True):
    """Convergence inside the host loop's 32-step chunk.  From the uploaded start the restated algorithm gives the f_rms of
    every evaluation; for each j in `wanted` (or the nearest j with a usable gap, see pick_tolerance) the stepper runs
    from the same start with that tolerance and must report converged, steps == j, the energy of evaluation j, and
    hold the positions of evaluation j -- the shadow's after j - 1 moves, within the bound of a (j - 1)-step segment;
    for j == 1 exactly the uploaded state as a download with no run in between returns it.  check 'C'."""
    su = _Setup(system, pot, cutoff, cell)
    box, diam = su.box, su.diam
    led = su.ledger(("U", "x1", "x", "xl"))
    note, miss = led.note, led.miss
    segments = []
    dt0 = float(fire_kw.get("dt_initial", 0.01))
    with (oracle.set_cell(cell) if cell is not None else contextlib.nullcontext()):
        shadow = FireRestated(oracle, box, cutoff, pot, diam, cell)
        f0 = oracle.forces_brute(system["x"], box, cutoff, pot, diam)[0]
        stepper.upload(system["x"], system["v"], f0, system["img"], diam)
        x_up, v_up, _, img_up = stepper.download()
        ref = shadow.run(x_up, img_up, horizon, NEVER, **fire_kw)
        f_rms = [t["f_rms"] for t in ref["trace"]]
        for want in wanted:
            j, tol = None, None
            for cand in sorted(range(1 if want == 1 else 2, horizon), key=lambda c: (abs(c - want), c)):
                tol = pick_tolerance(f_rms, cand)
                if tol is not None:
                    j = cand
                    break
            assert j is not None, "no evaluation with a usable f_rms gap"
            where = "convergence at evaluation %d (tol %.6e)" % (j, tol)
            stepper.upload(system["x"], system["v"], f0, system["img"], diam)
            before = stepper.stats()
            got = stepper.fire_minimize(max_steps=horizon, tol=tol, **fire_kw)
            x, v, f, img = stepper.download()
            after = stepper.stats()
            segments.append(dict(k=j - 1, j=j, tol=tol, steps=got["steps"], converged=bool(got["converged"]),
                                 **{key: int(after[key] - before[key]) for key in ("rebuilds", "violations")}))
            rec, (xr, imr) = ref["trace"][j - 1], ref["hist"][j - 1]
            if not got["converged"]:
                miss("C", "converged", "%s: not converged after %d steps" % (where, got["steps"]))
            if got["steps"] != j:
                miss("C", "steps", "%s: steps = %d" % (where, got["steps"]))
            finf0 = ref["trace"][0]["finf"]
            xb, xkey = _x_bound(j - 1, cell, 8.0 * float(np.spacing(su.Lmax)) + dt0 * dt0 * su.ftol * max(1.0, finf0))
            if j == 1:
                if not (np.array_equal(x, x_up) and np.array_equal(img, img_up)):
                    miss("C", "x", "%s: the positions moved on the converging step" % where)
            else:
                dx = _unwrapped_diff(x, img, xr, imr, su.U)
                if note(xkey, dx.max(), xb):
                    miss("C", "x", "%s: |dx|inf = %.3e > %.3e" % (where, dx.max(), xb))
                led.images(where, img, xr, imr, xb, check="C")
            fr = oracle.forces_brute(xr, box, cutoff, pot, diam)[0]
            bound = su.etol * max(1.0, abs(rec["energy"])) + (xb if j > 1 else 0.0) * float(np.abs(fr).sum())
            if note("U", abs(got["energy"] - rec["energy"]), bound):
                miss("C", "energy", "%s: energy = %.17g, evaluation %d has %.17g" % (where, got["energy"], j, rec["energy"]))
            if not np.array_equal(v, v_up):
                miss("C", "v", "%s: the MD velocities are not the uploaded ones" % where)
            if led.failures and raise_on_failure:
                raise led.failures[0]
        stats = stepper.stats()
    return led.result(segments, stats)


def loop_margins_line(name, result):
    """One line per case for the records of the Brownian and FIRE modes: every entry of `worst` as a fraction of its bound."""
    w = result["worst"]
    return "%-30s %s | excl %d  img %d" % (
        name, "  ".join("%s %.1e" % (k, w[k]) for k in w), len(result["excluded"]), len(result["image_exceptions"]))


class OracleBrownianStepper:
    """The Brownian stepper interface on the oracle's own functions: forces_brute, the Philox block (philox_np, held to
    oracle.philox by tests/test_loop_audit.py) and the oracle's move and wrap restated operation for operation, so that
    audit_brownian sees exactly zero error.  The pieces a sabotaged stepper overrides are methods."""

    def __init__(self, oracle, box, cutoff, pot, cell=None):
        self.o, self.box, self.cutoff, self.pot, self.cell = oracle, np.asarray(box, dtype=np.float64), cutoff, pot, cell
        self.steps = 0

    def upload(self, x, v, f, images, diameters):
        self.x, self.v, self.f = (np.array(a, dtype=np.float64) for a in (x, v, f))
        self.img = np.array(images, dtype=np.int32)
        self.diam = np.array(diameters, dtype=np.float64)
        self.cell_inv = self.o.set_cell.inverse() if self.cell is not None else None

    def download(self):
        return self.x.copy(), self.v.copy(), self.f.copy(), self.img.copy()

    def stats(self):
        return dict(steps=self.steps, prunes=0, rebuilds=0, violations=0, fused=0)

    def forces(self, x, t):
        """(f, U, W) at x for local step t"""
        f, u, w, _ = self.o.forces_brute(x, self.box, self.cutoff, self.pot, self.diam)
        return f, u, w

    def counter(self, g, first_step, t):
        """the two counter words of the global step g = first_step + t"""
        return g & 0xFFFFFFFF, (g >> 32) & 0xFFFFFFFF

    def key(self, seed):
        return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF

    def noise_ids(self):
        return np.arange(len(self.x))

    def mobility(self, dt, ktemp, f):
        return f * dt / ktemp

    def wrap(self, x, img):
        return wrap_np(x, img, self.box, self.cell, self.cell_inv)

    def samples(self, g, t, virial_every):
        return g % virial_every == 0

    def run_brownian(self, nsteps, dt, ktemp, seed, first_step=0, virial_every=10):
        sigma = np.sqrt(2.0 * dt)
        u = w = vsum = vcnt = 0.0
        for t in range(nsteps):
            g = int(first_step) + t
            self.f, u, w = self.forces(self.x, t)
            if self.samples(g, t, virial_every):
                vsum += w
                vcnt += 1.0
            words = philox_np(self.noise_ids(), *self.counter(g, int(first_step), t), 0, *self.key(int(seed)))
            un = (np.stack(words[:self.x.shape[1]], axis=1).astype(np.float64) + 0.5) * 2.3283064365386963e-10
            noise = (2.0 * un - 1.0) * 1.7320508075688772
            self.x, self.img = self.wrap(self.x + self.mobility(dt, ktemp, self.f) + noise * sigma, self.img)
            self.steps += 1
        return dict(U=u, W=w, virial_sum=vsum, virial_count=vcnt)


class OracleFireStepper:
    """The FIRE stepper interface on oracle.fire_minimize (brute force).  `restated`: a FireRestated (sub)class to run
    instead -- what the sabotaged steppers of tests/test_loop_audit.py are made of."""

    def __init__(self, oracle, box, cutoff, pot, cell=None, restated=None):
        self.o, self.box, self.cutoff, self.pot, self.cell = oracle, np.asarray(box, dtype=np.float64), cutoff, pot, cell
        self.restated = restated
        self.steps = 0

    upload = OracleBrownianStepper.upload
    download = OracleBrownianStepper.download
    stats = OracleBrownianStepper.stats

    def restore_velocities(self, v):
        self.v = v

    def fire_minimize(self, max_steps=10000, tol=1e-6, **kw):
        v = self.v.copy()
        self.v = np.zeros_like(v)               # FIRE's own velocities live where the MD ones do
        if self.restated is None:
            r = self.o.fire_minimize(self.x, self.img, self.diam, self.box, self.cutoff, self.pot, max_steps=max_steps,
                                     tol=tol, use_cells=False, nthreads=1, **kw)
        else:
            r = self.restated(self.o, self.box, self.cutoff, self.pot, self.diam, self.cell).run(
                self.x, self.img, max_steps, tol, **kw)
        self.x, self.img, self.f = r["x"], r["img"], r["f"]
        self.steps += r["steps"]
        self.restore_velocities(v)
        return dict(steps=r["steps"], converged=r["converged"], energy=r["energy"], f_rms=r["f_rms"])
