"""MDDevice: a thin object wrapper over one libmdhip handle (one GPU).

Arrays cross this boundary as (N, d) C-contiguous numpy arrays, which is byte-for-byte the
column-major d x N matrix the C ABI (and the Julia wrapper) uses.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import MdhipError, MdStats


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def _pairs(slots, rows):
    """The (slot, row) pairs of a *_sample call as two flat int32 arrays of one length."""
    s = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
    r = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
    if s.shape != r.shape:
        raise ValueError("slots and rows must have the same length")
    return s, r


def _f64(a, shape=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != shape:
        raise ValueError(f"expected array of shape {shape}, got {a.shape}")
    return a


class MDDevice:
    def __init__(self, dim, n_particles, box, list_cutoff, device_id=-1):
        self._L = _lib.load()
        self.dim = int(dim)
        self.n = int(n_particles)
        box = np.asarray(box, dtype=np.float64)
        if box.ndim == 0:
            box = np.eye(self.dim) * float(box)
        elif box.ndim == 1:
            box = np.diag(box)
        self.unitcell = np.ascontiguousarray(box[: self.dim, : self.dim])
        # column-major d x d: for a numpy (d,d) array that is the transpose's C order
        cm = np.ascontiguousarray(self.unitcell.T)
        h = C.c_void_p()
        rc = self._L.md_create(self.dim, self.n, _dp(cm), float(list_cutoff), int(device_id), C.byref(h))
        if rc != 0:
            raise MdhipError(self._L.md_last_error(None).decode())
        self._h = h
        self.list_cutoff = float(list_cutoff)

    # -- plumbing -------------------------------------------------------------------------
    def _chk(self, rc):
        if rc != 0:
            raise MdhipError(self._L.md_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._L.md_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- configuration --------------------------------------------------------------------
    def set_potential(self, kind, params):
        p = np.ascontiguousarray(params, dtype=np.float64)
        self._chk(self._L.md_set_potential(self._h, int(kind), _dp(p), int(p.size)))

    def set_potential_source(self, src, entry, params=()):
        p = np.ascontiguousarray(params, dtype=np.float64)
        self._chk(self._L.md_set_potential_source(self._h, src.encode(), entry.encode(), _dp(p), int(p.size)))

    def set_skin(self, skin):
        self._chk(self._L.md_set_skin(self._h, float(skin)))

    def set_inner_skin(self, inner_skin):
        self._chk(self._L.md_set_inner_skin(self._h, float(inner_skin)))

    # -- the cell of a live handle -----------------------------------------------------------
    CELL_AFFINE, CELL_LATTICE = _lib.MD_CELL_AFFINE, _lib.MD_CELL_LATTICE

    def set_cell(self, unitcell, mode=_lib.MD_CELL_AFFINE):
        """Change the unit cell of the handle (md_set_cell) and carry the particles along: CELL_AFFINE keeps fractional
        coordinates (forces stay those of the old cell until the next evaluation), CELL_LATTICE keeps Cartesian positions
        in a cell that generates the same lattice.  unitcell: a box length, d lengths or a d x d matrix (columns = lattice
        vectors), as the constructor takes.  A refusal (MdhipError) leaves the handle as it was."""
        box = np.asarray(unitcell, dtype=np.float64)
        if box.ndim == 0:
            box = np.eye(self.dim) * float(box)
        elif box.ndim == 1:
            box = np.diag(box)
        cell = np.ascontiguousarray(box[: self.dim, : self.dim])
        cm = np.ascontiguousarray(cell.T)
        self._chk(self._L.md_set_cell(self._h, _dp(cm), int(mode)))
        self.unitcell = cell

    def scale_cell(self, mu, vscale=1.0):
        """Scale the whole frame isotropically (md_scale_cell): cell and positions times mu, velocities times vscale, one
        rounding per component, nothing wrapped -- and the Verlet rows are kept with the skins they still leave (forces stay
        those of the old cell until the next evaluation).  Returns rows_kept: 1 when the outer rows stayed, 0 when the next
        evaluation builds the list again.  A refusal (MdhipError) leaves the handle as it was; waits."""
        kept = C.c_int(0)
        self._chk(self._L.md_scale_cell(self._h, float(mu), float(vscale), C.byref(kept)))
        self.unitcell = np.float64(mu) * self.unitcell
        return int(kept.value)

    def deform_cell(self, F, G=None):
        """Map the whole frame by the deformation gradient F (md_deform_cell): the cell becomes F U, x <- F x and, with G,
        v <- G v (G = inv(F): the stored velocities become peculiar ones, SLLOD), row times vector with every product and
        sum rounded, nothing wrapped -- and the Verlet rows are kept with the skins they still leave (forces stay those of
        the old cell until the next evaluation).  F, G: d x d.  Returns rows_kept: 1 when the outer rows stayed, 0 when the
        next evaluation builds the list again.  A refusal (MdhipError) leaves the handle as it was; waits."""
        d = self.dim
        Fm = np.ascontiguousarray(np.asarray(F, dtype=np.float64))
        if Fm.shape != (d, d):
            raise ValueError(f"F must have shape ({d}, {d})")
        Gm = None
        if G is not None:
            Gm = np.ascontiguousarray(np.asarray(G, dtype=np.float64))
            if Gm.shape != (d, d):
                raise ValueError(f"G must have shape ({d}, {d})")
        kept = C.c_int(0)
        self._chk(self._L.md_deform_cell(self._h, _dp(Fm), None if Gm is None else _dp(Gm), C.byref(kept)))
        # F U in the library's arithmetic: row times column, left to right, every product and sum rounded
        U = np.asarray(self.unitcell, dtype=np.float64)
        new = Fm[:, 0:1] * U[0:1, :] + Fm[:, 1:2] * U[1:2, :]
        if d == 3:
            new = new + Fm[:, 2:3] * U[2:3, :]
        self.unitcell = np.ascontiguousarray(new)
        return int(kept.value)

    def deform_state(self):
        """(M0, M1, sig) of md_deform_state: the products of the maps since the list build and since the last prune (d x d;
        identity when nothing was mapped) and sig = (s0, S0, s1, S1), the bounds on their singular values the skins left
        to the rows are formed from."""
        m0, m1, sig = np.zeros(9), np.zeros(9), np.zeros(4)
        self._chk(self._L.md_deform_state(self._h, _dp(m0), _dp(m1), _dp(sig)))
        d = self.dim
        return m0.reshape(3, 3)[:d, :d].copy(), m1.reshape(3, 3)[:d, :d].copy(), sig

    def nonaffine_mark(self):
        """Mark the current frame (md_nonaffine_mark): fractional coordinates and image counts by particle id."""
        self._chk(self._L.md_nonaffine_mark(self._h))

    def nonaffine(self, fields=False):
        """The displacement since the mark with the affine part taken out (md_nonaffine): dict(sum_u float64[d], sum_u2,
        sum_u4, max_u2, argmax (particle id), n) and with fields=True u float64[N, d] by particle id; waits."""
        sums = np.zeros(8)
        u = np.empty((self.n, self.dim)) if fields else None
        self._chk(self._L.md_nonaffine(self._h, _dp(sums), _dp(u)))
        out = dict(sum_u=sums[: self.dim].copy(), sum_u2=sums[3], sum_u4=sums[4], max_u2=sums[5], argmax=int(sums[6]),
                   n=int(sums[7]), sums=sums)
        if fields:
            out["u"] = u
        return out

    # -- state ----------------------------------------------------------------------------
    def upload(self, x=None, v=None, f=None, images=None, diameters=None):
        shp = (self.n, self.dim)
        x, v, f = _f64(x, shp), _f64(v, shp), _f64(f, shp)
        im = None if images is None else np.ascontiguousarray(images, dtype=np.int32)
        if im is not None and im.shape != shp:
            raise ValueError("images must have shape (N, d)")
        d = _f64(diameters, (self.n,))
        self._chk(self._L.md_upload(self._h, _dp(x), _dp(v), _dp(f), _ip(im), _dp(d)))

    def download(self):
        shp = (self.n, self.dim)
        x, v, f = np.empty(shp), np.empty(shp), np.empty(shp)
        im = np.empty(shp, dtype=np.int32)
        self._chk(self._L.md_download(self._h, _dp(x), _dp(v), _dp(f), _ip(im)))
        return x, v, f, im

    def snapshot_begin(self):
        """Start the export of one frame (positions + images, what the trajectory dump holds: src/simulation.jl:139-171):
        gather on the device, copy to pinned host memory on a copy stream.  Does not wait -- run the next segment and
        collect the frame with snapshot_end()."""
        self._chk(self._L.md_snapshot_begin(self._h))

    def snapshot_end(self):
        shp = (self.n, self.dim)
        x = np.empty(shp)
        im = np.empty(shp, dtype=np.int32)
        self._chk(self._L.md_snapshot_end(self._h, _dp(x), _ip(im)))
        return x, im

    # -- compute --------------------------------------------------------------------------
    def compute_forces(self):
        u, w = C.c_double(), C.c_double()
        self._chk(self._L.md_compute_forces(self._h, C.byref(u), C.byref(w)))
        return u.value, w.value

    def neighbor_pairs(self):
        cnt = C.c_int64()
        self._chk(self._L.md_neighbor_pairs(self._h, None, 0, C.byref(cnt)))
        out = np.empty((max(cnt.value, 1), 2), dtype=np.int32)
        cnt2 = C.c_int64()
        self._chk(self._L.md_neighbor_pairs(self._h, _ip(out), cnt.value, C.byref(cnt2)))
        if cnt2.value != cnt.value:
            raise MdhipError("pair count changed between calls")
        out = out[: cnt.value]
        order = np.lexsort((out[:, 1], out[:, 0]))
        return out[order]

    def run(self, nsteps, dt, ensemble=_lib.MD_NVE, tau=0.0, nf=None, ktemp=None, r1=None, r2=None, thermo=True):
        nf = float(self.dim * (self.n - 1.0)) if nf is None else float(nf)
        kt, a1, a2 = _f64(ktemp), _f64(r1), _f64(r2)
        for a in (kt, a1, a2):
            if a is not None and a.size < nsteps:
                raise ValueError("per-step thermostat arrays are shorter than nsteps")
        uwk = np.zeros(3)
        self._chk(self._L.md_run(self._h, int(nsteps), float(dt), int(ensemble), float(tau), nf, _dp(kt), _dp(a1),
                                 _dp(a2), _dp(uwk) if thermo else None))
        return (uwk[0], uwk[1], uwk[2]) if thermo else None

    def fire_minimize(self, max_steps=10000, tol=1e-6, dt_initial=0.01, dt_max=0.1, alpha0=0.1, f_inc=1.2, f_dec=0.2,
                      nmin=5):
        """fire_minimize! (src/minimize.jl:31-135) on the device state; returns dict(steps, converged, energy, f_rms)."""
        st, cv = C.c_int64(), C.c_int()
        en, fr = C.c_double(), C.c_double()
        self._chk(self._L.md_fire_minimize(self._h, int(max_steps), float(tol), float(dt_initial), float(dt_max),
                                           float(alpha0), float(f_inc), float(f_dec), int(nmin), C.byref(st), C.byref(cv),
                                           C.byref(en), C.byref(fr)))
        return dict(steps=st.value, converged=bool(cv.value), energy=en.value, f_rms=fr.value)

    def run_brownian(self, nsteps, dt, ktemp, seed, first_step=0, virial_every=10):
        """The Brownian step loop (src/simulation.jl:181-308); returns dict(U, W, virial_sum, virial_count)."""
        out = np.zeros(4)
        self._chk(self._L.md_run_brownian(self._h, int(nsteps), float(dt), float(ktemp), int(seed), int(first_step),
                                          int(virial_every), _dp(out)))
        return dict(U=out[0], W=out[1], virial_sum=out[2], virial_count=out[3])

    def kinetic(self):
        k = C.c_double()
        self._chk(self._L.md_kinetic(self._h, C.byref(k)))
        return k.value

    def scale_velocities(self, s):
        self._chk(self._L.md_scale_velocities(self._h, float(s)))

    # -- radial distribution function -----------------------------------------------------
    def rdf_setup(self, r_max, nbins):
        """Allocate the device g(r) sampler (md_rdf_setup): nbins bins of width r_max / nbins, histogram zeroed."""
        self._chk(self._L.md_rdf_setup(self._h, float(r_max), int(nbins)))
        self._rdf_nbins = int(nbins)

    def rdf_sample(self):
        """Add one sample of the current positions to the device histogram (does not wait, changes no state)."""
        self._chk(self._L.md_rdf_sample(self._h))

    def rdf_read(self):
        """(counts int64[nbins], nsamples): unordered pair counts summed over the samples since setup / reset."""
        counts = np.zeros(max(getattr(self, "_rdf_nbins", 0), 1), dtype=np.int64)
        ns = C.c_int64()
        self._chk(self._L.md_rdf_read(self._h, counts.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(ns)))
        return counts[: getattr(self, "_rdf_nbins", 0)], ns.value

    def rdf_reset(self):
        self._chk(self._L.md_rdf_reset(self._h))

    # -- self dynamics (MSD, F_s(q, t), van Hove) -----------------------------------------
    def dyn_setup(self, nslots, nrows, q=(), r_max=0.0, nbins=0):
        """Allocate the device self-dynamics sampler (md_dyn_setup): nslots origin slots, nrows zeroed rows of
        {sum d2, sum d4, sum s(q) per q} and, when nbins > 0, a van Hove histogram of nbins bins of width r_max / nbins."""
        qa = np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
        self._chk(self._L.md_dyn_setup(self._h, int(nslots), int(nrows), _dp(qa) if qa.size else None, int(qa.size),
                                       float(r_max), int(nbins)))
        self._dyn_shape = (int(nrows), int(qa.size), int(nbins))

    def dyn_origin(self, slot):
        """Store the current frame (what download() returns: wrapped x and images) in `slot` (does not wait)."""
        self._chk(self._L.md_dyn_origin(self._h, int(slot)))

    def dyn_sample(self, slots, rows):
        """Export the current frame once and add one sample per (slots[i], rows[i]): this frame against the origin in
        slots[i], accumulated into rows[i] (does not wait, changes no state)."""
        s, r = _pairs(slots, rows)
        self._chk(self._L.md_dyn_sample(self._h, _ip(s), _ip(r), int(s.size)))

    def dyn_read(self):
        """(nsamples int64[nrows], sums float64[nrows, 2 + nq], hist int64[nrows, nbins]), summed since setup / reset."""
        nrows, nq, nbins = getattr(self, "_dyn_shape", (0, 0, 0))
        ns = np.zeros(max(nrows, 1), dtype=np.int64)
        sums = np.zeros((max(nrows, 1), 2 + nq))
        hist = np.zeros((max(nrows, 1), max(nbins, 1)), dtype=np.int64)
        i64 = C.POINTER(C.c_int64)
        self._chk(self._L.md_dyn_read(self._h, ns.ctypes.data_as(i64), _dp(sums), hist.ctypes.data_as(i64)))
        return ns[:nrows], sums[:nrows], hist[:nrows, :nbins]

    def dyn_reset(self):
        self._chk(self._L.md_dyn_reset(self._h))

    # -- density modes, S(q), coherent F(q, t) --------------------------------------------
    def sq_setup(self, n, nslots=0, nrows=0):
        """Allocate the device density-mode sampler (md_sq_setup): the integer wave vectors n (nvec, d), q_n = 2 pi U^-T n,
        nslots origin slots and nrows correlation rows, all zeroed."""
        na = np.ascontiguousarray(n, dtype=np.int32)
        if na.ndim != 2 or na.shape[1] != self.dim:
            raise ValueError(f"n must have shape (nvec, {self.dim})")
        self._chk(self._L.md_sq_setup(self._h, _ip(na) if na.size else None, int(na.shape[0]), int(nslots), int(nrows)))
        self._sq_shape = (int(na.shape[0]), int(nrows))

    def sq_sample(self, static=True, slots=(), rows=(), origin=None):
        """Evaluate rho(q) of the current frame once; then add |rho|^2 to the static accumulator if `static`, one
        correlation per (slots[i], rows[i]) -- this frame against the origin in slots[i], into rows[i] -- and store rho in
        slot `origin` unless it is None, in that order (does not wait, changes no state)."""
        s, r = _pairs(slots, rows)
        self._chk(self._L.md_sq_sample(self._h, 1 if static else 0, _ip(s) if s.size else None, _ip(r) if r.size else None,
                                       int(s.size), -1 if origin is None else int(origin)))

    def sq_rho(self):
        """rho(q) of the last sampled frame, complex128[nvec] (rho = sum exp(+i q.x)); waits."""
        nvec, _ = getattr(self, "_sq_shape", (0, 0))
        out = np.zeros((max(nvec, 1), 2))
        self._chk(self._L.md_sq_rho(self._h, _dp(out)))
        return out[:nvec].copy().view(np.complex128).reshape(nvec)

    def sq_read(self):
        """(nstatic, s2 float64[nvec], nsamples int64[nrows], corr float64[nrows, nvec]), summed since setup / reset."""
        nvec, nrows = getattr(self, "_sq_shape", (0, 0))
        nst = C.c_int64()
        s2 = np.zeros(max(nvec, 1))
        ns = np.zeros(max(nrows, 1), dtype=np.int64)
        corr = np.zeros((max(nrows, 1), max(nvec, 1)))
        self._chk(self._L.md_sq_read(self._h, C.byref(nst), _dp(s2), ns.ctypes.data_as(C.POINTER(C.c_int64)), _dp(corr)))
        return nst.value, s2[:nvec], ns[:nrows], corr[:nrows, :nvec]

    def sq_reset(self):
        self._chk(self._L.md_sq_reset(self._h))

    # -- currents, C_L / C_T(q, t), the VACF ----------------------------------------------
    def cur_setup(self, n, e, nslots=0, nrows=0, vacf=False):
        """Allocate the device current sampler (md_cur_setup): the integer wave vectors n (nvec, d), q_n = 2 pi U^-T n,
        their unit directions e (nvec, d) for the longitudinal / transverse split, nslots origin slots and nrows
        correlation rows, all zeroed; vacf=True adds Z = sum v(t).v(t0) per (slot, row) and an origin's velocity frame.
        n = None (with vacf) samples Z only."""
        na = np.zeros((0, self.dim), dtype=np.int32) if n is None else np.ascontiguousarray(n, dtype=np.int32)
        ea = np.zeros((0, self.dim)) if e is None else np.ascontiguousarray(e, dtype=np.float64)
        if na.ndim != 2 or na.shape[1] != self.dim:
            raise ValueError(f"n must have shape (nvec, {self.dim})")
        if ea.shape != na.shape:
            raise ValueError(f"e must have n's shape {na.shape}")
        self._chk(self._L.md_cur_setup(self._h, _ip(na) if na.size else None, _dp(ea) if ea.size else None,
                                       int(na.shape[0]), int(nslots), int(nrows), 1 if vacf else 0))
        self._cur_shape = (int(na.shape[0]), int(nrows), bool(vacf))

    def cur_sample(self, static=True, slots=(), rows=(), origin=None):
        """Evaluate j(q) of the current frame once; then add the static sample if `static`, one correlation per
        (slots[i], rows[i]) -- this frame against the origin in slots[i], into rows[i] -- and store the origin (j and,
        with vacf, the velocities) in slot `origin` unless it is None, in that order (does not wait, changes no state)."""
        s, r = _pairs(slots, rows)
        self._chk(self._L.md_cur_sample(self._h, 1 if static else 0, _ip(s) if s.size else None, _ip(r) if r.size else None,
                                        int(s.size), -1 if origin is None else int(origin)))

    def cur_last(self):
        """j(q) of the last sampled frame, complex128[nvec, d] (j_a = sum v_a exp(+i q.x)); waits."""
        nvec, _, _ = getattr(self, "_cur_shape", (0, 0, False))
        out = np.zeros((max(nvec, 1), self.dim, 2))
        self._chk(self._L.md_cur_last(self._h, _dp(out)))
        return out[:nvec].copy().view(np.complex128).reshape(nvec, self.dim)

    def cur_read(self):
        """(nstatic, s_tot float64[nvec], s_long float64[nvec], nsamples int64[nrows], c_tot float64[nrows, nvec],
        c_long float64[nrows, nvec], z), summed since setup / reset; z is float64[nrows + 1] -- the lag rows, then the
        equal-time sum of the static samples -- with vacf and None without."""
        nvec, nrows, vacf = getattr(self, "_cur_shape", (0, 0, False))
        nst = C.c_int64()
        s_tot, s_long = np.zeros(max(nvec, 1)), np.zeros(max(nvec, 1))
        ns = np.zeros(max(nrows, 1), dtype=np.int64)
        c_tot, c_long = np.zeros((max(nrows, 1), max(nvec, 1))), np.zeros((max(nrows, 1), max(nvec, 1)))
        z = np.zeros(nrows + 1) if vacf else None
        self._chk(self._L.md_cur_read(self._h, C.byref(nst), _dp(s_tot), _dp(s_long),
                                      ns.ctypes.data_as(C.POINTER(C.c_int64)), _dp(c_tot), _dp(c_long), _dp(z)))
        if nvec == 0:
            c_tot, c_long = np.zeros((nrows, 0)), np.zeros((nrows, 0))
        else:
            c_tot, c_long = c_tot.reshape(-1)[:nrows * nvec].reshape(nrows, nvec), c_long.reshape(-1)[:nrows * nvec].reshape(nrows, nvec)
        return nst.value, s_tot[:nvec], s_long[:nvec], ns[:nrows], c_tot, c_long, z

    def cur_reset(self):
        self._chk(self._L.md_cur_reset(self._h))

    # -- pressure tensor and its lag correlations -----------------------------------------
    def stress_setup(self, nlags=0):
        """Allocate the device pressure-tensor sampler (md_stress_setup): running sums of the kinetic and virial tensors
        and, with nlags > 0, a ring of nlags channel vectors and the lag products corr[k][ch], all zeroed."""
        self._chk(self._L.md_stress_setup(self._h, int(nlags)))
        self._stress_nlags = int(nlags)

    def stress_sample(self):
        """Add one sample of the current state (does not wait, changes nothing the handle computes afterwards)."""
        self._chk(self._L.md_stress_sample(self._h))

    def stress_tensor(self):
        """(kin, vir) of the last sampled frame, float64[nc] each: K_ab = sum v_a v_b and W_ab = sum (f/r) del_a del_b, in the
        order xx, yy, zz, xy, xz, yz (3-D) or xx, yy, xy (2-D); waits."""
        nc = 6 if self.dim == 3 else 3
        kin, vir = np.zeros(nc), np.zeros(nc)
        self._chk(self._L.md_stress_tensor(self._h, _dp(kin), _dp(vir)))
        return kin, vir

    def stress_read(self):
        """(nsamples, sum_kin float64[nc], sum_vir float64[nc], ncorr int64[nlags], corr float64[nlags, nc]), summed since
        setup / reset; waits."""
        nc = 6 if self.dim == 3 else 3
        nl = getattr(self, "_stress_nlags", 0)
        ns = C.c_int64()
        sk, sv = np.zeros(nc), np.zeros(nc)
        ncorr = np.zeros(max(nl, 1), dtype=np.int64)
        corr = np.zeros((max(nl, 1), nc))
        self._chk(self._L.md_stress_read(self._h, C.byref(ns), _dp(sk), _dp(sv),
                                         ncorr.ctypes.data_as(C.POINTER(C.c_int64)), _dp(corr)))
        return ns.value, sk, sv, ncorr[:nl], corr[:nl]

    def stress_reset(self):
        self._chk(self._L.md_stress_reset(self._h))

    # -- bond-orientational order ---------------------------------------------------------
    def boo_setup(self, r_neigh, order=6, nbins=100, threshold=0.7, min_conn=7, nseries=0):
        """Allocate the device bond-order sampler (md_boo_setup): neighbours within r_neigh <= list cutoff, order = l (4 or
        6) in 3-D or k (1..12) in 2-D, nbins histogram bins over [0, 1], the solid-bond threshold on s_ij, the number of
        solid bonds that makes a particle solid, and nseries rows of the per-sample series; all zeroed."""
        self._chk(self._L.md_boo_setup(self._h, float(r_neigh), int(order), int(nbins), float(threshold), int(min_conn),
                                       int(nseries)))
        self._boo_shape = (int(order) + 1 if self.dim == 3 else 1, int(nbins), int(nseries))

    def boo_sample(self):
        """Add one sample of the current positions (does not wait, changes nothing the handle computes afterwards)."""
        self._chk(self._L.md_boo_sample(self._h))

    def boo_particles(self):
        """(nnb int32[N], q float64[N], qbar float64[N], nconn int32[N]) of the last sampled frame, in particle-id order;
        waits."""
        nnb, nconn = np.zeros(self.n, dtype=np.int32), np.zeros(self.n, dtype=np.int32)
        q, qbar = np.zeros(self.n), np.zeros(self.n)
        self._chk(self._L.md_boo_particles(self._h, _ip(nnb), _dp(q), _dp(qbar), _ip(nconn)))
        return nnb, q, qbar, nconn

    def boo_qlm(self):
        """q_lm of the last sampled frame, complex128[N, NM] for m = 0..NM-1 (3-D: NM = l + 1; 2-D: NM = 1, psi_k); waits."""
        nm = getattr(self, "_boo_shape", (1, 0, 0))[0]
        out = np.zeros((self.n, nm, 2))
        self._chk(self._L.md_boo_qlm(self._h, _dp(out)))
        return out.view(np.complex128).reshape(self.n, nm)

    def boo_read(self):
        """(nsamples, sum_fr float64[8], hist_q int64[nbins], hist_qbar int64[nbins], hist_nnb int64[33], hist_conn int64[33],
        series float64[min(nsamples, nseries), 8]), accumulated since setup / reset; waits."""
        _, nbins, nseries = getattr(self, "_boo_shape", (1, 0, 0))
        ns = C.c_int64()
        fr = np.zeros(8)
        hq, hb = np.zeros(max(nbins, 1), dtype=np.int64), np.zeros(max(nbins, 1), dtype=np.int64)
        hn, hc = np.zeros(33, dtype=np.int64), np.zeros(33, dtype=np.int64)
        series = np.zeros((max(nseries, 1), 8))
        i64 = C.POINTER(C.c_int64)
        self._chk(self._L.md_boo_read(self._h, C.byref(ns), _dp(fr), hq.ctypes.data_as(i64), hb.ctypes.data_as(i64),
                                      hn.ctypes.data_as(i64), hc.ctypes.data_as(i64), _dp(series)))
        return ns.value, fr, hq[:nbins], hb[:nbins], hn, hc, series[: min(ns.value, nseries)]

    def boo_reset(self):
        self._chk(self._L.md_boo_reset(self._h))

    # -- clusters ---------------------------------------------------------------------------
    def cluster_setup(self, r_bond, members=0, max_size=1024, nseries=0):
        """Allocate the device cluster sampler (md_cluster_setup): members bonded within r_bond <= list cutoff, members =
        MD_CLUSTER_ALL (0) or MD_CLUSTER_SOLID (1: the solid particles of the last bond-order frame), a size histogram of
        max_size + 1 entries and nseries rows of the per-sample series; all zeroed."""
        self._chk(self._L.md_cluster_setup(self._h, float(r_bond), int(members), int(max_size), int(nseries)))
        self._cluster_shape = (int(max_size), int(nseries))

    def cluster_sample(self):
        """Add one sample of the current positions (does not wait, changes nothing the handle computes afterwards)."""
        self._chk(self._L.md_cluster_sample(self._h))

    def cluster_particles(self):
        """(label int32[N], size int32[N]) of the last sampled frame, in particle-id order: the smallest particle id of the
        particle's cluster and the cluster's size; -1 and 0 for a non-member; waits."""
        label, size = np.zeros(self.n, dtype=np.int32), np.zeros(self.n, dtype=np.int32)
        self._chk(self._L.md_cluster_particles(self._h, _ip(label), _ip(size)))
        return label, size

    def cluster_read(self):
        """(nsamples, sum_fr int64[8], hist_size int64[max_size + 1], series int64[min(nsamples, nseries), 8]), accumulated
        since setup / reset; waits."""
        max_size, nseries = getattr(self, "_cluster_shape", (0, 0))
        ns = C.c_int64()
        fr = np.zeros(8, dtype=np.int64)
        hist = np.zeros(max_size + 1, dtype=np.int64)
        series = np.zeros((max(nseries, 1), 8), dtype=np.int64)
        i64 = C.POINTER(C.c_int64)
        self._chk(self._L.md_cluster_read(self._h, C.byref(ns), fr.ctypes.data_as(i64), hist.ctypes.data_as(i64),
                                          series.ctypes.data_as(i64)))
        return ns.value, fr, hist, series[: min(ns.value, nseries)]

    def cluster_reset(self):
        self._chk(self._L.md_cluster_reset(self._h))

    # -- cage-relative dynamics and bond breaking ------------------------------------------
    def cage_setup(self, nslots, nrows, r_neigh, r_break=None, scaled=False, max_neigh=16, q=()):
        """Allocate the device cage sampler (md_cage_setup): nslots origin slots with a neighbour table of max_neigh <= 32
        entries per particle (bonds d2 < (r_neigh s)^2 at the origin, s = sigma_ij if scaled else 1; broken when
        d2 >= (r_break s)^2 at the sample), nrows zeroed rows of {sum d2, sum d4, sum s(q) per q} of the cage-relative
        displacement, the three counts and the broken-bond histogram."""
        qa = np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
        r_break = r_neigh if r_break is None else r_break
        self._chk(self._L.md_cage_setup(self._h, int(nslots), int(nrows), float(r_neigh), float(r_break), int(bool(scaled)),
                                        int(max_neigh), _dp(qa) if qa.size else None, int(qa.size)))
        self._cage_shape = (int(nrows), int(qa.size))

    def cage_origin(self, slot):
        """Store the current frame and its neighbour table in `slot` (does not wait; builds the list if it is not valid)."""
        self._chk(self._L.md_cage_origin(self._h, int(slot)))

    def cage_sample(self, slots, rows):
        """Export the current frame once and add one sample per (slots[i], rows[i]): this frame against the origin and the
        neighbours stored in slots[i], accumulated into rows[i] (does not wait, changes no state)."""
        s, r = _pairs(slots, rows)
        self._chk(self._L.md_cage_sample(self._h, _ip(s), _ip(r), int(s.size)))

    def cage_particles(self):
        """(nnb int32[N], d2cr float64[N], broken int32[N]) of the last (slot, row) of the last cage_sample call, in
        particle-id order: the neighbours kept at the origin, |Del^CR|^2 and the broken bonds; waits."""
        nnb, broken = np.zeros(self.n, dtype=np.int32), np.zeros(self.n, dtype=np.int32)
        d2 = np.zeros(self.n)
        self._chk(self._L.md_cage_particles(self._h, _ip(nnb), _dp(d2), _ip(broken)))
        return nnb, d2, broken

    def cage_read(self):
        """(nsamples int64[nrows], sums float64[nrows, 2 + nq], counts int64[nrows, 3], hist_broken int64[nrows, 33],
        overflow), summed since setup / reset (overflow: since setup); waits."""
        nrows, nq = getattr(self, "_cage_shape", (0, 0))
        ns = np.zeros(max(nrows, 1), dtype=np.int64)
        sums = np.zeros((max(nrows, 1), 2 + nq))
        counts = np.zeros((max(nrows, 1), 3), dtype=np.int64)
        hist = np.zeros((max(nrows, 1), 33), dtype=np.int64)
        ov = C.c_int64()
        i64 = C.POINTER(C.c_int64)
        self._chk(self._L.md_cage_read(self._h, ns.ctypes.data_as(i64), _dp(sums), counts.ctypes.data_as(i64),
                                       hist.ctypes.data_as(i64), C.byref(ov)))
        return ns[:nrows], sums[:nrows], counts[:nrows], hist[:nrows], ov.value

    def cage_reset(self):
        self._chk(self._L.md_cage_reset(self._h))

    # -- four-point dynamics: the overlap Q, chi4, S4(q, t) --------------------------------
    def chi4_setup(self, a, n=None, nslots=1, nrows=1):
        """Allocate the device four-point sampler (md_chi4_setup): a particle is slow while it has moved less than `a`
        since the origin; the integer wave vectors n (nvec <= 4096, d) of W(q), or None / empty for chi4 only; nslots
        origin slots; nrows zeroed rows of {sum Q, sum Q^2, samples, sum |W|^2 per vector}."""
        na = np.zeros((0, self.dim), dtype=np.int32) if n is None else np.ascontiguousarray(n, dtype=np.int32)
        if na.ndim != 2 or na.shape[1] != self.dim:
            raise ValueError(f"n must have shape (nvec, {self.dim})")
        self._chk(self._L.md_chi4_setup(self._h, float(a), _ip(na) if na.size else None, int(na.shape[0]), int(nslots),
                                        int(nrows)))
        self._chi4_shape = (int(nrows), int(na.shape[0]))

    def chi4_origin(self, slot):
        """Store the current frame (and, with vectors, its fractional coordinates) in `slot` (does not wait)."""
        self._chk(self._L.md_chi4_origin(self._h, int(slot)))

    def chi4_sample(self, slots, rows):
        """Export the current frame once and add one sample per (slots[i], rows[i]), in order: the overlap of this frame
        with the origin in slots[i] and W on the slow particles, accumulated into rows[i] (does not wait, changes no
        state)."""
        s, r = _pairs(slots, rows)
        self._chk(self._L.md_chi4_sample(self._h, _ip(s), _ip(r), int(s.size)))

    def chi4_last(self):
        """(Q int, W complex128[nvec], slow uint8[N] by particle id) of the last (slot, row) of the last chi4_sample call;
        waits."""
        _, nvec = getattr(self, "_chi4_shape", (0, 0))
        q = C.c_int64()
        w = np.zeros((max(nvec, 1), 2))
        slow = np.zeros(self.n, dtype=np.uint8)
        self._chk(self._L.md_chi4_last(self._h, C.byref(q), _dp(w), slow.ctypes.data_as(C.c_void_p)))
        return q.value, w[:nvec].copy().view(np.complex128).reshape(nvec), slow

    def chi4_read(self):
        """(nsamples int64[nrows], sum_q int64[nrows], sum_q2 int64[nrows], s4 float64[nrows, nvec]), summed since setup /
        reset; waits."""
        nrows, nvec = getattr(self, "_chi4_shape", (0, 0))
        ns, sq, sq2 = (np.zeros(max(nrows, 1), dtype=np.int64) for _ in range(3))
        s4 = np.zeros(max(nrows * nvec, 1))
        i64 = C.POINTER(C.c_int64)
        self._chk(self._L.md_chi4_read(self._h, ns.ctypes.data_as(i64), sq.ctypes.data_as(i64), sq2.ctypes.data_as(i64),
                                       _dp(s4)))
        return ns[:nrows], sq[:nrows], sq2[:nrows], s4[: nrows * nvec].reshape(nrows, nvec)

    def chi4_reset(self):
        self._chk(self._L.md_chi4_reset(self._h))

    # -- marked pair correlations: G_l(r), g6(r), C_aa(r) of an uploaded field -------------
    def mpc_setup(self, r_max, nbins, weights=None, tmax=None):
        """Allocate the device marked-pair-correlation sampler (md_mpc_setup) out to r_max on nbins <= 4096 bins.
        weights=None: the marks are q_lm / psi_k of the bond-order sampler's last frame (MD_MPC_BOO; boo_setup first),
        tmax = 1.  weights = NC in 1..3 numbers: the marks are the caller's (MD_MPC_USER; mpc_marks), a pair contributes
        t = sum_c weights[c] a_c(i) a_c(j), and tmax bounds |t| (rounded up to a power of two).  All zeroed."""
        if weights is None:
            self._chk(self._L.md_mpc_setup(self._h, _lib.MD_MPC_BOO, float(r_max), int(nbins), 0, None, 0.0))
            nc = 0
        else:
            w = _f64(weights).reshape(-1)
            if tmax is None:
                raise ValueError("user marks need tmax")
            self._chk(self._L.md_mpc_setup(self._h, _lib.MD_MPC_USER, float(r_max), int(nbins), int(w.size), _dp(w),
                                           float(tmax)))
            nc = int(w.size)
        self._mpc_shape = (int(nbins), nc)

    def mpc_marks(self, marks):
        """Upload the marks float64[N, NC] (or [N] when NC = 1), in particle-id order; they stay until replaced; waits."""
        _, nc = getattr(self, "_mpc_shape", (0, 0))
        m = _f64(marks)
        if nc > 0:
            m = _f64(m.reshape(self.n, nc) if m.size == self.n * nc else m, (self.n, nc))
        self._chk(self._L.md_mpc_marks(self._h, _dp(m)))

    def mpc_sample(self):
        """Add one sample of the current positions (does not wait, changes nothing the handle computes afterwards)."""
        self._chk(self._L.md_mpc_sample(self._h))

    def mpc_last(self):
        """(cnt int64[nbins], sum int64[nbins], self int) of the last sample: pairs per bin, sum of the integer terms
        I_ij = llrint(t_ij 2^31 / tmax) per bin, sum_i I_ii; waits."""
        nbins, _ = getattr(self, "_mpc_shape", (0, 0))
        cnt, tot = np.zeros(max(nbins, 1), dtype=np.int64), np.zeros(max(nbins, 1), dtype=np.int64)
        own = C.c_int64()
        i64 = C.POINTER(C.c_int64)
        self._chk(self._L.md_mpc_last(self._h, cnt.ctypes.data_as(i64), tot.ctypes.data_as(i64), C.byref(own)))
        return cnt[:nbins], tot[:nbins], own.value

    def mpc_read(self):
        """(nsamples, acc_cnt int64[nbins], acc_sum float64[nbins], acc_self float, tmax, range_error), accumulated since
        setup / reset; acc_sum * tmax * 2^-31 / acc_cnt is the correlation.  range_error: bit 0 a term beyond tmax, bit 1
        a bin with 2^31 pairs in one sample; waits."""
        nbins, _ = getattr(self, "_mpc_shape", (0, 0))
        ns, err = C.c_int64(), C.c_int32()
        cnt = np.zeros(max(nbins, 1), dtype=np.int64)
        tot = np.zeros(max(nbins, 1))
        own, tmax = C.c_double(), C.c_double()
        self._chk(self._L.md_mpc_read(self._h, C.byref(ns), cnt.ctypes.data_as(C.POINTER(C.c_int64)), _dp(tot),
                                      C.byref(own), C.byref(tmax), C.byref(err)))
        return ns.value, cnt[:nbins], tot[:nbins], own.value, tmax.value, err.value

    def mpc_reset(self):
        self._chk(self._L.md_mpc_reset(self._h))

    # -- swap Monte Carlo ------------------------------------------------------------------
    SWAP_COUNTS = ("proposed", "void", "lost", "blocked", "filtered", "accepted")
    SWAP_STATUS = ("none", "void", "lost", "blocked", "filtered", "rejected", "accepted")

    def swap_setup(self, fraction, max_diameter_difference=None, seed=0):
        """Allocate the device swap sampler (md_swap_setup): every round a particle proposes with probability `fraction`
        in (0, 1]; max_diameter_difference=None: no filter; `seed` keys the Philox stream."""
        mdd = 0.0 if max_diameter_difference is None else float(max_diameter_difference)
        self._chk(self._L.md_swap_setup(self._h, float(fraction), mdd, C.c_uint64(int(seed) & (2 ** 64 - 1))))

    def swap_rounds(self, nrounds, ktemp, first_round=0):
        """Run rounds first_round .. first_round + nrounds - 1 of diameter exchanges at the current positions
        (md_swap_rounds), then refresh the forces.  Returns dict(proposed, void, lost, blocked, filtered, accepted, decided,
        du_accepted, U, W): the counts over the call's rounds, the sum of dU over the accepted swaps, and U, W of the new
        diameters; waits."""
        counts = np.zeros(6, dtype=np.int64)
        dec = C.c_int64()
        du, u, w = C.c_double(), C.c_double(), C.c_double()
        self._chk(self._L.md_swap_rounds(self._h, int(nrounds), float(ktemp), int(first_round),
                                         counts.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(dec), C.byref(du),
                                         C.byref(u), C.byref(w)))
        out = {k: int(v) for k, v in zip(self.SWAP_COUNTS, counts)}
        out.update(decided=dec.value, du_accepted=du.value, U=u.value, W=w.value)
        return out

    def swap_last(self):
        """(partner int32[N], status int32[N], du float64[N]) of the last round, by particle id: the proposer's partner
        (-1: did not propose), its status (index into SWAP_STATUS) and dU of a decided swap; waits."""
        partner, status = np.zeros(self.n, dtype=np.int32), np.zeros(self.n, dtype=np.int32)
        du = np.zeros(self.n)
        self._chk(self._L.md_swap_last(self._h, _ip(partner), _ip(status), _dp(du)))
        return partner, status, du

    def diameters(self):
        """The current diameters float64[N], in particle-id order (md_diameters); waits."""
        d = np.zeros(self.n)
        self._chk(self._L.md_diameters(self._h, _dp(d)))
        return d

    # -- Hessian of the pair energy --------------------------------------------------------
    HESS_MAX_BLOCK = 8

    def hess_setup(self):
        """Freeze the Hessian operator on the frame the handle holds (md_hess_setup): built-in potentials only; builds the
        list when it is not valid.  Any upload, run, minimisation, swap round or list rebuild invalidates it."""
        self._chk(self._L.md_hess_setup(self._h))

    def hess_apply(self, X):
        """Y = H X for a block X float64[m, N, d] (by particle id), 1 <= m <= 8 (md_hess_apply); waits."""
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.ndim != 3 or X.shape[1:] != (self.n, self.dim) or not 1 <= X.shape[0] <= self.HESS_MAX_BLOCK:
            raise ValueError(f"expected a block of shape (m, {self.n}, {self.dim}) with 1 <= m <= {self.HESS_MAX_BLOCK}, "
                             f"got {X.shape}")
        Y = np.empty_like(X)
        self._chk(self._L.md_hess_apply(self._h, int(X.shape[0]), _dp(X), _dp(Y)))
        return Y

    def hess_blocks(self):
        """The diagonal blocks H_ii, float64[N, d, d] by particle id (md_hess_blocks); waits."""
        out = np.empty((self.n, self.dim, self.dim))
        self._chk(self._L.md_hess_blocks(self._h, _dp(out)))
        return out

    def hess_lanczos(self, ksteps, seed=0):
        """ksteps Lanczos steps with full reorthogonalisation, the basis resident on the device (md_hess_lanczos).  Returns
        (alpha[ksteps], beta[ksteps]): the tridiagonal matrix has diagonal alpha and off-diagonal beta[:-1]; waits."""
        ksteps = int(ksteps)
        if ksteps < 1:
            raise ValueError("ksteps must be >= 1")
        a, b = np.empty(ksteps), np.empty(ksteps)
        self._chk(self._L.md_hess_lanczos(self._h, ksteps, C.c_uint64(int(seed) & (2 ** 64 - 1)), _dp(a), _dp(b)))
        return a, b

    def hess_ritz(self, S, theta):
        """Ritz vectors Y = V S of the last hess_lanczos basis for S float64[ksteps, nvec] and the values theta[nvec]
        (md_hess_ritz).  Returns (modes float64[nvec, N, d] by particle id, resid[nvec] = |H y - theta y|); waits."""
        S = np.ascontiguousarray(S, dtype=np.float64)
        if S.ndim != 2 or S.shape[1] < 1:
            raise ValueError("S must have shape (ksteps, nvec) with nvec >= 1")
        theta = _f64(theta, (S.shape[1],))
        modes = np.empty((S.shape[1], self.n, self.dim))
        resid = np.empty(S.shape[1])
        self._chk(self._L.md_hess_ritz(self._h, int(S.shape[0]), int(S.shape[1]), _dp(S), _dp(theta), _dp(modes), _dp(resid)))
        return modes, resid

    # -- elastic moduli of the frozen frame ------------------------------------------------
    ELAS_CONVERGED, ELAS_MAX_ITER, ELAS_INDEFINITE = _lib.MD_ELAS_CONVERGED, _lib.MD_ELAS_MAX_ITER, _lib.MD_ELAS_INDEFINITE

    @property
    def elas_components(self):
        """The strain components in the order of every elas_* array: tuples of axis indices."""
        return ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)) if self.dim == 3 else ((0, 0), (1, 1), (0, 1))

    def elas_affine(self, fields=False):
        """The affine pass on the operator hess_setup froze (md_elas_affine).  Returns dict(stress[nc], born[nc, nc]) --
        configurational stress and Born tensor per unit volume, tensor components in elas_components order -- and with
        fields=True also xi float64[nc, N, d], the affine force field by particle id; waits."""
        nc = len(self.elas_components)
        stress, born = np.empty(nc), np.empty((nc, nc))
        xi = np.empty((nc, self.n, self.dim)) if fields else None
        self._chk(self._L.md_elas_affine(self._h, _dp(stress), _dp(born), _dp(xi) if fields else None))
        out = dict(stress=stress, born=born)
        if fields:
            out["xi"] = xi
        return out

    def elas_solve(self, tol, max_iter, fields=True):
        """H u_c = -Xi_c for the nc strain components at once by conjugate gradients on the device (md_elas_solve); needs
        elas_affine of the same hess_setup.  Returns dict(nonaffine[nc, nc] = Xi_s . u_t / V (not symmetrised), iterations[nc],
        residuals[nc] = the true |H u_c + Xi_c|, xi_norm[nc], status (bits ELAS_CONVERGED | ELAS_MAX_ITER | ELAS_INDEFINITE),
        converged, indefinite) and with fields=True u float64[nc, N, d] by particle id; waits."""
        tol, max_iter = float(tol), int(max_iter)
        if not tol > 0.0:
            raise ValueError("tol must be > 0")
        if max_iter < 1:
            raise ValueError("max_iter must be >= 1")
        nc = len(self.elas_components)
        iters = np.zeros(nc, dtype=np.int64)
        resid, xin, nonaff = np.empty(nc), np.empty(nc), np.empty((nc, nc))
        u = np.empty((nc, self.n, self.dim)) if fields else None
        status = C.c_int(0)
        self._chk(self._L.md_elas_solve(self._h, tol, max_iter, iters.ctypes.data_as(C.POINTER(C.c_int64)), _dp(resid), _dp(xin),
                                        C.byref(status), _dp(nonaff), _dp(u) if fields else None))
        out = dict(nonaffine=nonaff, iterations=iters, residuals=resid, xi_norm=xin, status=status.value,
                   converged=bool(status.value & self.ELAS_CONVERGED), indefinite=bool(status.value & self.ELAS_INDEFINITE))
        if fields:
            out["u"] = u
        return out

    # -- instrumentation ------------------------------------------------------------------
    def profile(self, enable=True):
        """True/1: time every force and kick-drift launch; k > 1: every k-th; False/0: off."""
        self._chk(self._L.md_profile(self._h, int(enable)))

    def stats(self):
        s = MdStats()
        self._chk(self._L.md_get_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in MdStats._fields_}

    LIST_ROWS_INFO = ("rc", "skin", "rl", "inner_skin", "d1", "list_valid", "inner_valid", "tiled", "fused_build",
                      "own_first", "inner_halo_live", "n", "rows32", "n_ghost", "virtual_ghosts", "prune_on")

    def list_rows(self, which=0):
        """The Verlet rows as they are (md_list_rows; builds and changes nothing).  which = 0: outer rows, 1: inner rows
        (an error without valid inner rows).  Returns dict(which, info, entries, x0, x1, pos): info = the named fields of
        LIST_ROWS_INFO (flags and n as int), entries int32[m, 5] = (id_i, id_j, n_0, n_1, n_2) in row order, both
        directions of every pair, x0 / x1 / pos float64[n, d] by particle id in the device's own unwrapped frame.  A handle
        whose rows are not valid gives info["list_valid"] == 0 and no entries."""
        info = np.zeros(_lib.MD_LIST_ROWS_INFO)
        shp = (self.n, self.dim)
        x0, x1, pos = np.empty(shp), np.empty(shp), np.empty(shp)
        cnt = C.c_int64()
        self._chk(self._L.md_list_rows(self._h, int(which), _dp(info), None, 0, C.byref(cnt), _dp(x0), _dp(x1), _dp(pos)))
        ent = np.empty((max(cnt.value, 1), 5), dtype=np.int32)
        cnt2 = C.c_int64()
        self._chk(self._L.md_list_rows(self._h, int(which), None, _ip(ent), cnt.value, C.byref(cnt2), None, None, None))
        if cnt2.value != cnt.value:
            raise MdhipError("row entry count changed between calls")
        named = {k: (float(v) if i < 5 else int(v)) for i, (k, v) in enumerate(zip(self.LIST_ROWS_INFO, info))}
        return dict(which=int(which), info=named, entries=ent[: cnt.value], x0=x0, x1=x1, pos=pos)
