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
    worst = dict(F=0.0, U=0.0, W=0.0, K=0.0, x1=0.0, v1=0.0, x=0.0, v=0.0)
    segments, failures = [], []
    excluded, image_exc = set(), set()

    def miss(check, what, msg):
        failures.append(AuditFailure(check, what, msg))

    def note(key, err, bound):
        worst[key] = max(worst[key], float(err) / bound if np.isfinite(err) else np.inf)
        return not (err <= bound)

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
            knife = knife_edge_particles(x, box, cell, thresholds)
            excluded.update(int(i) for i in knife)
            keep = np.ones(n, dtype=bool)
            keep[knife] = False
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
                differ = np.flatnonzero((img != ref["img"]).any(axis=1))
                if differ.size:
                    near = face_distance(ref["x"], box, cell)[differ] <= xb
                    image_exc.update(int(i) for i in differ[near])
                    if not near.all() or len(image_exc) > MAX_IMAGE_EXCEPTIONS:
                        miss("B", "img", "%s: image counters differ for particles %s" % (where, differ[:8].tolist()))
            if len(excluded) > MAX_EXCLUDED:
                miss("precondition", "knife", "%s: %d particles on a knife edge so far" % (where, len(excluded)))
            if failures and raise_on_failure:
                raise failures[0]
            start = end
            a += k
        stats = stepper.stats()
    return dict(worst=worst, segments=segments, excluded=sorted(excluded), image_exceptions=sorted(image_exc),
                failures=failures, stats=stats)


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
