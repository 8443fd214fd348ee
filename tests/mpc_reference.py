"""The numpy reference of the marked-pair-correlation sampler (md_mpc_*), shared by tests/test_pair_correlation.py (CPU)
and tests/test_gpu_pair_correlation.py (the device against it).  Nothing here comes from the code under test: the pair
set is the oracle's (or a brute-force one on a small lattice), d2 is the oracle's canonical form restated in numpy (as
tests/test_gpu_rdf.py does), the bin is the edge table's, and every accumulated quantity is an int64.

numpy has no fused multiply-add: the chain acc = fma(w_c, p_c, acc) is evaluated as acc + w_c * p_c.  Where every product
and partial sum is exactly representable (the dyadic marks of the exact tests) the two agree bit for bit; elsewhere a
term may round to the neighbouring integer, which the callers allow for per pair."""
import numpy as np


def edges2(r_max, nbins):
    """The host's table e2[k] = (k delta)^2, delta = r_max / nbins."""
    delta = r_max / nbins
    rk = np.arange(nbins + 1, dtype=np.float64) * delta
    return rk * rk


def canon_d2(x, box, pairs):
    """oracle/md_oracle.c canon_d2 for the (a < b) pairs: b translated, every operation rounded on its own."""
    a, b = x[pairs[:, 0]], x[pairs[:, 1]]
    L = np.asarray(box, dtype=np.float64)
    d0 = b - a
    half = 0.5 * L
    s = np.where(d0 > half, -1.0, np.where(d0 < -half, 1.0, 0.0))
    de = (b + s * L) - a
    d2 = de[:, 0] * de[:, 0] + de[:, 1] * de[:, 1]
    if x.shape[1] == 3:
        d2 = d2 + de[:, 2] * de[:, 2]
    return d2


def tric_d2(x, U, pairs):
    """oracle/md_oracle.c tric_d2: 3^d translations t_r = (s0 U_r0 + s1 U_r1) + s2 U_r2, strict < in its loop order."""
    d = x.shape[1]
    a, b = x[pairs[:, 0]], x[pairs[:, 1]]
    best = np.full(len(pairs), 1e300)
    for s2 in ((-1, 0, 1) if d == 3 else (0,)):
        for s1 in (-1, 0, 1):
            for s0 in (-1, 0, 1):
                de = np.empty_like(a)
                for r in range(d):
                    t = float(s0) * U[r, 0] + float(s1) * U[r, 1]
                    if d == 3:
                        t = t + float(s2) * U[r, 2]
                    de[:, r] = (b[:, r] + t) - a[:, r]
                d2 = de[:, 0] * de[:, 0] + de[:, 1] * de[:, 1]
                if d == 3:
                    d2 = d2 + de[:, 2] * de[:, 2]
                best = np.where(d2 < best, d2, best)
    return best


def round_up_pow2(tmax):
    """The tmax md_mpc_setup uses: the next power of two >= tmax."""
    m, e = np.frexp(float(tmax))
    return float(tmax) if m == 0.5 else float(np.ldexp(1.0, e))


def terms(a, b, weights, tmax):
    """I = rint(t 2^31 / tmax), t = sum_c w_c a_c b_c in chain order, for rows of marks a and b; a term with
    |t| > tmax (1 + 2^-10) contributes 0 (the device raises range_error for it)."""
    a = np.asarray(a, dtype=np.float64).reshape(len(a), -1)
    b = np.asarray(b, dtype=np.float64).reshape(len(b), -1)
    acc = np.zeros(len(a))
    for c, w in enumerate(np.asarray(weights, dtype=np.float64).reshape(-1)):
        acc = acc + w * (a[:, c] * b[:, c])
    ok = np.abs(acc) <= tmax * (1.0 + 2.0 ** -10)
    return np.where(ok, np.rint(np.where(ok, acc, 0.0) * (2.0 ** 31 / tmax)), 0.0).astype(np.int64), ok


def correlate(pairs, d2, marks, weights, tmax, r_max, nbins):
    """(cnt int64[nbins], sum int64[nbins], self int, in_range bool) for the unordered pairs `pairs` with squared
    distances d2: the pair goes into bin k iff e2[k] <= d2 < e2[k+1], with one count and its integer term."""
    tmax = round_up_pow2(tmax)
    marks = np.asarray(marks, dtype=np.float64).reshape(len(marks), -1)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    e2 = edges2(r_max, nbins)
    keep = d2 < e2[-1]
    pairs, d2 = pairs[keep], d2[keep]
    k = np.searchsorted(e2, d2, "right") - 1
    I, ok = terms(marks[pairs[:, 0]], marks[pairs[:, 1]], weights, tmax)
    cnt = np.bincount(k, minlength=nbins).astype(np.int64)
    tot = np.zeros(nbins, dtype=np.int64)
    np.add.at(tot, k, I)
    Iself, oks = terms(marks, marks, weights, tmax)
    return cnt, tot, int(Iself.sum()), bool(ok.all() and oks.all())


def boo_marks(qlm):
    """The marks of MD_MPC_BOO from complex q_lm (N, NM): Re, Im of m = 0..NM-1 interleaved, (N, 2 NM)."""
    q = np.asarray(qlm, dtype=np.complex128)
    return np.ascontiguousarray(q.view(np.float64).reshape(len(q), -1))


def boo_weights(dim, order):
    """pref {1, 1, 2, 2, ...} with pref = 4 pi / (2l + 1) in 3-D; {1, 1} in 2-D."""
    if dim == 2:
        return np.ones(2)
    w = np.full(2 * (order + 1), 2.0)
    w[:2] = 1.0
    return 4.0 * np.pi / (2 * order + 1) * w
