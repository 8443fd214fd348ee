"""A plain numpy restatement of what md_cur_* computes (include/mdhip.h), for the tests of the
current-correlation sampler: the currents in extended precision, the accumulator expressions as the no-fma fp64
expressions the contract states, and the velocity autocorrelation sum."""
import numpy as np

LD = np.longdouble
PI_LD = LD(3.141592653589793) + LD(1.2246467991473532e-16)
U53 = 2.0 ** -53


def inv_ld(U):
    """U^-1 in extended precision (adjugate / determinant)."""
    d = U.shape[0]
    A = U.astype(LD)
    if d == 2:
        det = A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]
        return np.array([[A[1, 1], -A[0, 1]], [-A[1, 0], A[0, 0]]], dtype=LD) / det
    C = np.empty((3, 3), dtype=LD)
    for r in range(3):
        for c in range(3):
            r1, r2 = (r + 1) % 3, (r + 2) % 3
            c1, c2 = (c + 1) % 3, (c + 2) % 3
            C[r, c] = A[r1, c1] * A[r2, c2] - A[r1, c2] * A[r2, c1]
    det = A[0, 0] * C[0, 0] + A[0, 1] * C[0, 1] + A[0, 2] * C[0, 2]
    return C.T / det


def j_true(x, v, U, n):
    """j_a(n) = sum_i v_i,a exp(+2 pi i n.f_i), f = U^-1 x, summed in extended precision from the fp64 frame (x, v);
    complex128 (nvec, d)."""
    assert np.finfo(LD).eps < 2e-19, "np.longdouble is not an extended type here"
    x, v, U, n = np.asarray(x), np.asarray(v), np.asarray(U, dtype=np.float64), np.asarray(n)
    if U.ndim == 1:
        U = np.diag(U)
    f = x.astype(LD) @ inv_ld(U).T
    vl = v.astype(LD)
    out = np.empty((n.shape[0], x.shape[1]), dtype=np.complex128)
    step = max(1, min(128, (1 << 21) // max(x.shape[0], 1)))   # (the extended-precision temporaries stay small)
    for v0 in range(0, n.shape[0], step):
        t = f @ n[v0:v0 + step].astype(LD).T                   # (N, chunk)
        ph = (2 * PI_LD) * (t - np.rint(t))
        c, s = np.cos(ph), np.sin(ph)
        out[v0:v0 + step] = (c.T @ vl).astype(np.float64) + 1j * (s.T @ vl).astype(np.float64)
    return out


def kappa(U):
    U = np.asarray(U, dtype=np.float64)
    if U.ndim == 1 or np.count_nonzero(U - np.diag(np.diagonal(U))) == 0:
        return 1.0
    return float(np.max(np.sum(np.abs(np.linalg.inv(U)) @ np.abs(U), axis=1)))


def j_bound(v, U, n):
    """(nvec, d): V_a (32 kappa |n|_1 + 128) 2^-53, V_a = sum_i |v_i,a|."""
    V = np.sum(np.abs(np.asarray(v, dtype=np.float64)), axis=0)
    return (32.0 * kappa(U) * np.sum(np.abs(n), axis=1) + 128.0)[:, None] * V[None, :] * U53


def directions(U, n):
    """e = q_n / |q_n| from the Cartesian q_n = 2 pi U^-T n that wave_vector_lengths forms; (nvec, d)."""
    U = np.asarray(U, dtype=np.float64)
    if U.ndim == 1:
        U = np.diag(U)
    q = 2.0 * np.pi * (np.asarray(n, dtype=np.float64) @ np.linalg.inv(U))
    return q / np.linalg.norm(q, axis=1)[:, None]


def p_long(e, part):
    """pL = (e_0 j_0 + e_1 j_1) + e_2 j_2 of one part (Re or Im) of j; every operation rounded on its own."""
    p = e[:, 0] * part[:, 0] + e[:, 1] * part[:, 1]
    if e.shape[1] == 3:
        p = p + e[:, 2] * part[:, 2]
    return p


def tot_term(j, o):
    """sum over a, in order, of (Re_a oRe_a + Im_a oIm_a); o = j gives the static term."""
    t = j.real[:, 0] * o.real[:, 0] + j.imag[:, 0] * o.imag[:, 0]
    for a in range(1, j.shape[1]):
        t = t + (j.real[:, a] * o.real[:, a] + j.imag[:, a] * o.imag[:, a])
    return t


def long_term(j, o, e):
    """pL_re oL_re + pL_im oL_im; o = j gives the static term."""
    return p_long(e, j.real) * p_long(e, o.real) + p_long(e, j.imag) * p_long(e, o.imag)


class Accumulators:
    """The sums md_cur_read returns, kept by the contract's expressions from the j values md_cur_last returns."""

    def __init__(self, e, nrows):
        self.e = np.asarray(e, dtype=np.float64)
        nvec = self.e.shape[0]
        self.nstatic, self.nsamples = 0, np.zeros(nrows, np.int64)
        self.s_tot, self.s_long = np.zeros(nvec), np.zeros(nvec)
        self.c_tot, self.c_long = np.zeros((nrows, nvec)), np.zeros((nrows, nvec))
        self.org = {}

    def sample(self, j, static, pairs, origin):
        if static:
            self.s_tot = self.s_tot + tot_term(j, j)
            self.s_long = self.s_long + long_term(j, j, self.e)
            self.nstatic += 1
        for slot, row in pairs:
            o = self.org[slot]
            self.c_tot[row] = self.c_tot[row] + tot_term(j, o)
            self.c_long[row] = self.c_long[row] + long_term(j, o, self.e)
            self.nsamples[row] += 1
        if origin is not None:
            self.org[origin] = j.copy()


def z_true(v, o):
    """(Z, A): sum_i v_i.o_i in extended precision, and A = sum_i sum_a |v_i,a o_i,a|."""
    p = np.asarray(v).astype(LD) * np.asarray(o).astype(LD)
    return float(np.sum(p)), float(np.sum(np.abs(p)))
