"""-m gpu: the row audit (tests/row_audit.py) on an MDDevice -- the Verlet rows themselves, read back with md_list_rows,
against brute force in fp64: every build path right after a build, the list radius with a pair put next to it, the rows in
use through md_run segment by segment, and the rows the Brownian and FIRE loops leave behind.

Findings: none.  Every invariant of tests/row_audit.py held on every snapshot of every case and path below; no knife-edge
band held a pair (the cap is step_audit.MAX_EXCLUDED per case).  What follows are records (MI355X), not tolerances.

Which build path a case takes is asserted from the info block and stats().  The fused build (k_build_tile) takes lj_diam,
lj_2d, poly_3d, the tiny systems and the two_words inputs; the two-kernel fallback takes cell_above_64 and the dilute case
-- and, with no switch set, also blob, blob_sheared, phs and poly_2d, whose tiles hold more than the 36 non-empty cells
the fused build stages (so for the blobs MDHIP_NO_FUSED_BUILD and MDHIP_NO_OWN_FIRST select the path they are on
already, and the fused_build setting of (b) runs the fallback too), and lj_2d at skin 0.

O4, the largest d2(x0) / rl^2 among entries.  Fused build: at most 1.000099893 (two_words_3d_full), under the path's bound
rl^2 (1 + 1e-4) plus the fp32 slack of row_audit.fused_bound (1.0001034 there) -- the rows are as wide as the margin and no
wider.  Fallback and no-tiles build: never above 1 (0.999999998 with rl put 1e-9 beyond a pair): k_build_list tests
d2 <= rl * rl in fp64.

What the paths do just outside rl (rl = d / (1 + 1e-9) for a pair at distance d; printed by (b), not asserted): the fused
build keeps the pair, in both rows, every time (8 of 8 pairs: it lies inside the 1e-4 margin); the two-kernel fallback drops
it, from both rows, every time (20 of 20), and so does the build without tiles (14 of 14), which is the same k_build_list.  With
rl = d / (1 - 1e-9) every pair was in both rows on every path (42 of 42): inside a tile, between tiles, across a face,
across an edge or corner (the liquids; the blobs' gas has no pair of that kind at a usable distance).

(a), (d) fresh builds: entries of the outer rows (both directions), the largest d2 / rl^2 among them, band counts rl / rc
  blob                       46546  0.999959985  0 / 0
  blob_sheared               46550  0.999959985  0 / 0
  cell_above_64             336296  0.999999269  0 / 0
  dilute                       476  0.997079432  0 / 0
  lj_2d                      18298  1.000073347  0 / 0
  lj_diam                   104148  1.000099725  0 / 0
  phs                         2960  0.999244968  0 / 0
  poly_2d                    14198  0.998764956  0 / 0
  poly_3d                    22346  1.000058172  0 / 0
  tiny2                          2  0.120040010  0 / 0
  tiny257                    13086  0.999622065  0 / 0
  tiny3                          2  0.120040010  0 / 0
  tiny65                      1926  0.913835918  0 / 0
  two_words_2d              178456  1.000099126  0 / 0
  two_words_3d_full         310798  1.000099893  0 / 0
  blob/no_fused_build        46546  0.999959985  0 / 0
  blob/no_own_first          46546  0.999959985  0 / 0
  blob/no_tiles              46546  0.999959985  0 / 0
  blob/skin_0                30448  0.991474741  0 / 0
  lj_diam/no_fused_build    104090  0.999998948  0 / 0
  lj_diam/no_own_first      104148  1.000099725  0 / 0
  lj_diam/no_tiles          104090  0.999998948  0 / 0
  lj_diam/skin_0             60182  1.000090645  0 / 0
  lj_2d/no_fused_build       18294  0.999987108  0 / 0
  lj_2d/no_own_first         18298  1.000073347  0 / 0
  lj_2d/no_tiles             18294  0.999987108  0 / 0
  lj_2d/skin_0               14366  0.999999653  0 / 0
  lj_diam/user_lj           104148  1.000099725  0 / 0
  blob/after brownian        40630  0.999967343  0 / 0
  blob/after fire            41260  0.988831477  0 / 0

(b) rl next to a pair: the largest d2 / rl^2 per case and path over its pairs, and what happened to the pairs
  blob           fused_build     pairs 3  d2/rl^2 <= 0.999999998  inside: 3 of 3 in both rows   just outside: 0 of 3   bands 0
  blob           no_fused_build  pairs 3  d2/rl^2 <= 0.999999998  inside: 3 of 3 in both rows   just outside: 0 of 3   bands 0
  lj_diam        fused_build     pairs 4  d2/rl^2 <= 1.000092707  inside: 4 of 4 in both rows   just outside: 4 of 4   bands 0
  lj_diam        no_fused_build  pairs 4  d2/rl^2 <= 0.999999998  inside: 4 of 4 in both rows   just outside: 0 of 4   bands 0
  lj_2d          fused_build     pairs 4  d2/rl^2 <= 1.000099265  inside: 4 of 4 in both rows   just outside: 4 of 4   bands 0
  lj_2d          no_fused_build  pairs 4  d2/rl^2 <= 0.999999998  inside: 4 of 4 in both rows   just outside: 0 of 4   bands 0
  blob_sheared   fused_build     pairs 3  d2/rl^2 <= 0.999999998  inside: 3 of 3 in both rows   just outside: 0 of 3   bands 0
  blob_sheared   no_fused_build  pairs 3  d2/rl^2 <= 0.999999998  inside: 3 of 3 in both rows   just outside: 0 of 3   bands 0
  blob           no_tiles        pairs 3  d2/rl^2 <= 0.999999998  inside: 3 of 3 in both rows   just outside: 0 of 3   bands 0
  lj_diam        no_tiles        pairs 4  d2/rl^2 <= 0.999999998  inside: 4 of 4 in both rows   just outside: 0 of 4   bands 0
  lj_2d          no_tiles        pairs 4  d2/rl^2 <= 0.999999998  inside: 4 of 4 in both rows   just outside: 0 of 4   bands 0
  blob_sheared   no_tiles        pairs 3  d2/rl^2 <= 0.999999998  inside: 3 of 3 in both rows   just outside: 0 of 3   bands 0

(c) rows in use, 21 snapshots per case (after the first build, then after each of MIXED's 20 segments): list builds and
    prunes, the largest d2(x0) / rl^2 and d2(x1) / rin^2 among entries, bands, and the largest displacement as a fraction
    of its limit (V1: skin / 2; V2: min(inner / 2, skin / 2 - d1)).  Row entries per snapshot: blob 46 k outer / 36-38 k
    inner, lj_diam 104-108 k / 71-79 k, lj_2d 18-20 k / 16-18 k (each snapshot's line is printed by the test).
  blob                              builds 10 prunes 35  d2/rl^2 <= 0.999999717  d2(x1)/rin^2 <= 0.999998411239  bands 0  V1 0.597  V2 0.746
  tiny3                             builds 11 prunes 43  d2/rl^2 <= 0.965688334  d2(x1)/rin^2 <= 0.961108245833  bands 0  V1 0.774  V2 0.690
  tiny65                            builds  5 prunes 36  d2/rl^2 <= 0.999344480  d2(x1)/rin^2 <= 0.999945037928  bands 0  V1 0.631  V2 0.667
  lj_diam                           builds  7 prunes 27  d2/rl^2 <= 1.000099725  d2(x1)/rin^2 <= 0.999999391017  bands 0  V1 0.915  V2 0.889
  lj_2d                             builds  6 prunes 22  d2/rl^2 <= 1.000081594  d2(x1)/rin^2 <= 0.999997719353  bands 0  V1 0.801  V2 0.864
  poly_2d                           builds  7 prunes 42  d2/rl^2 <= 0.999980750  d2(x1)/rin^2 <= 0.999999306014  bands 0  V1 0.866  V2 0.943
  phs_diam                          builds  8 prunes 39  d2/rl^2 <= 0.999851669  d2(x1)/rin^2 <= 0.999992816640  bands 0  V1 0.987  V2 0.928
  blob_sheared                      builds 10 prunes 35  d2/rl^2 <= 0.999999717  d2(x1)/rin^2 <= 0.999998411239  bands 0  V1 0.597  V2 0.746
  blob/nvt                          builds 10 prunes 40  d2/rl^2 <= 0.999998632  d2(x1)/rin^2 <= 0.999999635048  bands 0  V1 0.817  V2 0.768
  blob/no_fused_step                builds  9 prunes 29  d2/rl^2 <= 0.999994261  d2(x1)/rin^2 <= 0.999999417808  bands 0  V1 0.696  V2 0.746
  blob/no_fused_step_inner_halo     builds  9 prunes 29  d2/rl^2 <= 0.999994261  d2(x1)/rin^2 <= 0.999999417808  bands 0  V1 0.696  V2 0.746
  blob/no_tiles                     builds  9 prunes  0  d2/rl^2 <= 0.999997664  d2(x1)/rin^2 <= -               bands 0  V1 0.994  V2 -
  blob/no_fused_build               builds 10 prunes 35  d2/rl^2 <= 0.999999717  d2(x1)/rin^2 <= 0.999998411239  bands 0  V1 0.597  V2 0.746
  blob/inner_skin_0                 builds  9 prunes  0  d2/rl^2 <= 0.999999717  d2(x1)/rin^2 <= -               bands 0  V1 0.796  V2 -
  blob/skin_0                       builds 80 prunes  0  d2/rl^2 <= 0.999999920  d2(x1)/rin^2 <= -               bands 0  V1 0.000  V2 -
  lj_diam/no_fused_step             builds  7 prunes 25  d2/rl^2 <= 1.000099725  d2(x1)/rin^2 <= 0.999996894704  bands 0  V1 0.915  V2 0.889
  lj_diam/no_fused_step_inner_halo  builds  8 prunes 27  d2/rl^2 <= 1.000099725  d2(x1)/rin^2 <= 0.999998583466  bands 0  V1 0.915  V2 0.889
  lj_diam/no_tiles                  builds  8 prunes  0  d2/rl^2 <= 0.999999491  d2(x1)/rin^2 <= -               bands 0  V1 0.744  V2 -
  lj_diam/no_fused_build            builds  7 prunes 27  d2/rl^2 <= 0.999999443  d2(x1)/rin^2 <= 0.999999391017  bands 0  V1 0.915  V2 0.889
  lj_diam/inner_skin_0              builds  8 prunes  0  d2/rl^2 <= 1.000099725  d2(x1)/rin^2 <= -               bands 0  V1 0.744  V2 -
  lj_diam/skin_0                    builds 80 prunes  0  d2/rl^2 <= 1.000099512  d2(x1)/rin^2 <= -               bands 0  V1 0.000  V2 -
  Coverage of the default path (asserted, under NVT too): between 6 and 10 of the 21 snapshots hold inner rows right after a
  prune (x1 == pos), 10 to 14 hold aged inner rows, one has no inner rows (right after the first build: after any step of
  md_run a handle that prunes has them, since the step after every build is a prune step).  I4's largest d2(x1) / rin^2
  stays below 1: the prune's own d2 (an fma chain on the LJ fast path) never disagreed with the reference form.

Run time of the module on one MI355X: 63 tests in 16.0 s (the slowest, lj_diam through md_run, 1.0 s each).
"""
import numpy as np
import pytest

from tests import row_audit as ra
from tests import step_audit as sa
from tests import test_gpu_build_masks as bm
from tests.test_gpu_step_audit import SWITCHES, build_case
from tests.util import lj_system

pytestmark = pytest.mark.gpu

LJ = [1.0, 1.0, 2.5]
MIXED = sa.MIXED
DEFAULT_SKIN = 0.6                           # md_create's skin (mdhip.hip: skin_req)


# ---------------------------------------------------------------------------------------------------------------------
# inputs (no device here: tests/test_row_audit.py asserts their empty knife-edge bands without one)
# ---------------------------------------------------------------------------------------------------------------------
def dilute_system(n=512, rho=0.008, seed=31):
    """Random positions, no two closer than 0.9, in a box of 40^3: about one neighbour within 3.1 per particle, nearly
    every particle alone in its cell -- a tile's 256 particles occupy far more than the 36 non-empty cells the fused build
    holds, so the two-kernel fallback builds the rows, on a sparse grid."""
    rng = np.random.default_rng(seed)
    L = (n / rho) ** (1.0 / 3.0)
    x = np.zeros((0, 3))
    while len(x) < n:
        p = rng.uniform(0.0, L, 3)
        d = x - p
        d -= L * np.rint(d / L)
        if len(x) == 0 or (d * d).sum(axis=1).min() > 0.81:
            x = np.vstack([x, p])
    s = lj_system(n, rho=rho)
    s["x"] = np.ascontiguousarray(x)
    return s


BUILD_CASES = {name: "step" for name in ("tiny2", "tiny3", "tiny65", "tiny257", "blob", "blob_sheared", "lj_diam", "lj_2d",
                                          "poly_2d", "poly_3d", "phs")}
BUILD_CASES.update({name: "masks" for name in ("two_words_3d_full", "two_words_2d", "cell_above_64")})
BUILD_CASES["dilute"] = "dilute"
# What the fused build (k_build_tile) cannot take goes through the two-kernel fallback: a cell of more than 64 particles
# (cell_above_64), or a tile whose 256 particles lie in more than 36 non-empty cells -- the dilute case, and the ragged or
# thin ones (the blob's gas, pseudo hard spheres at rho = 0.5 with rl = 1.62, the 2-D polydisperse system with rl = 2.1).
FALLBACK_CASES = ("cell_above_64", "dilute", "blob", "blob_sheared", "phs", "poly_2d")
_INPUTS = {}


def build_input(case):
    """dict(system, kind, params, cutoff, skin[, inner_skin, dt]) of a named case, built once."""
    if case not in _INPUTS:
        src = BUILD_CASES[case]
        if src == "step":
            c = dict(build_case(case))
            c.setdefault("skin", DEFAULT_SKIN)
        elif src == "masks":
            s, m = bm._system(case)
            c = dict(system=s, kind=sa.POT_LJ, params=LJ, cutoff=2.5, skin=m["skin"])
        else:
            c = dict(system=dilute_system(), kind=sa.POT_LJ, params=LJ, cutoff=2.5, skin=DEFAULT_SKIN)
        _INPUTS[case] = c
    return _INPUTS[case]


def cell_of(s):
    return s["box"] if s.get("cell") is None else s["cell"]


def effective_skin(U, rc, skin):
    """md_set_skin's box clip (mdhip.hip configure_grid): three cells of the list radius per axis must fit between the faces."""
    perp = 1.0 / np.linalg.norm(np.linalg.inv(U), axis=1)
    smax = perp.min() / 3.0 - rc
    return max(0.0, smax * 0.999) if skin > smax else skin


def slot_order(x, U, rl):
    """slot -> particle id of the first list build after an upload, as the device sorts (md_kernels.hpp cell_coords,
    ext_linear; mdhip.hip configure_grid): cells cut per axis, numbered brick-major in boustrophedon order, particles of a
    cell in id order (the sort is stable).  Tile of a particle = slot // 256.  The device tests check it against the order
    of the rows md_list_rows returns."""
    n, dim = x.shape
    Uinv = np.linalg.inv(U)
    perp = 1.0 / np.linalg.norm(Uinv, axis=1)
    nc = np.ones(3, dtype=np.int64)
    for d in range(dim):
        k = int(np.floor(perp[d] / rl))
        while k > 3 and perp[d] / k < rl:
            k -= 1
        nc[d] = max(k, 3)
    cc = np.zeros((n, 3), dtype=np.int64)
    if np.count_nonzero(U - np.diag(np.diagonal(U))) == 0:
        cc[:, :dim] = (x * (nc[:dim] / perp)).astype(np.int64)
    else:
        cc[:, :dim] = ((x @ Uinv.T) * nc[:dim]).astype(np.int64)
    cc = np.clip(cc, 0, nc - 1)
    target = np.array([2, 2, 3] if dim == 3 else [4, 3, 1])
    nb = np.maximum(1, nc // target)
    bd = -(-nc // nb)
    b = ((cc + 1) * nb - 1) // nc
    w = cc - (b * nc) // nb
    byp = np.where(b[:, 2] & 1, nb[1] - 1 - b[:, 1], b[:, 1])
    r = b[:, 2] * nb[1] + byp
    bxp = np.where(r & 1, nb[0] - 1 - b[:, 0], b[:, 0])
    lin = (r * nb[0] + bxp) * (bd[0] * bd[1] * bd[2]) + (w[:, 2] * bd[1] + w[:, 1]) * bd[0] + w[:, 0]
    return np.argsort(lin, kind="stable")


KNIFE = 1e-9
KNIFE_CASES = ("blob", "lj_diam", "lj_2d", "blob_sheared")
KNIFE_KINDS = ("inside_a_tile", "between_tiles", "across_a_face", "across_an_edge_or_corner")


def knife_pairs(case, seed=23):
    """{kind: (i, j, n, d)}: for each kind the first pair, in a seeded random order, whose distance d makes
    skin = d / (1 - 1e-9) - rc fall in [0.3, 0.9] below the box clip, and that is of that kind in the list built with that
    skin (tiles from slot_order).  A kind the input has no pair of is left out (tests/test_row_audit.py asserts which)."""
    c = build_input(case)
    s = c["system"]
    n, dim = s["x"].shape
    U = ra.lattice(cell_of(s), dim)
    rc = c["cutoff"]
    perp = 1.0 / np.linalg.norm(np.linalg.inv(U), axis=1)
    hi = min(0.9, 0.999 * (perp.min() / 3.0 - rc))
    keys, d2 = ra.pairs_within(s["x"], U, ((rc + hi) * (1.0 - KNIFE)) ** 2)
    ent = ra.keys_to_entries(keys, n)
    d = np.sqrt(d2)
    ok = (ent[:, 0] < ent[:, 1]) & (d / (1.0 - KNIFE) - rc >= 0.3)
    ent, d = ent[ok], d[ok]
    out = {}
    for k in np.random.default_rng(seed).permutation(len(ent)):
        crossings = int(np.count_nonzero(ent[k, 2:]))
        if crossings >= 2:
            kind = KNIFE_KINDS[3]
        elif crossings == 1:
            kind = KNIFE_KINDS[2]
        elif KNIFE_KINDS[0] in out and KNIFE_KINDS[1] in out:
            continue
        else:
            order = slot_order(s["x"], U, d[k] / (1.0 - KNIFE))
            slot = np.empty(n, dtype=np.int64)
            slot[order] = np.arange(n)
            kind = KNIFE_KINDS[0] if slot[ent[k, 0]] // 256 == slot[ent[k, 1]] // 256 else KNIFE_KINDS[1]
        if kind not in out:
            out[kind] = (int(ent[k, 0]), int(ent[k, 1]), ent[k, 2:].copy(), float(d[k]))
        if len(out) == len(KNIFE_KINDS):
            break
    return out


# ---------------------------------------------------------------------------------------------------------------------
# device plumbing
# ---------------------------------------------------------------------------------------------------------------------
def _device(c, skin=None, inner_skin=None, user=False):
    from moleculardynamics.jl_amd import MDDevice
    s = c["system"]
    dev = MDDevice(s["dim"], s["n"], cell_of(s), c["cutoff"])
    if user:
        from tests.test_gpu_parity import USER_LJ_SRC
        dev.set_potential_source(USER_LJ_SRC, "user_lj", [1.0, 2.5])
    else:
        dev.set_potential(c["kind"], c["params"])
    if skin is not None:
        dev.set_skin(skin)
    if inner_skin is not None:
        dev.set_inner_skin(inner_skin)
    return dev


def _upload(dev, s):
    dev.upload(s["x"], s["v"], np.zeros_like(s["x"]), s["img"], s["diam"])


def _audit(name, snap, c, cache=None):
    s = c["system"]
    res = ra.check_rows(snap, cell_of(s), s["dim"], cache)
    print(ra.counts_line(name, res["counts"]))
    assert res["violations"] == [], (name, [str(v) for v in res["violations"]])
    return res["counts"]


def _bands(counts):
    return counts["band_rl"] + counts["band_rin"] + counts["band_rc"]


# ---------------------------------------------------------------------------------------------------------------------
# (a) fresh build, every path
# ---------------------------------------------------------------------------------------------------------------------
FUSED_PATH = dict(tiled=1, fused_build=1, own_first=1, rows32=0)
FALLBACK_PATH = dict(tiled=1, fused_build=0, own_first=0, rows32=0)
BUILD_SWITCHES = {
    "no_fused_build": dict(env={"MDHIP_NO_FUSED_BUILD": "1"}, path=lambda base: FALLBACK_PATH),
    "no_own_first": dict(env={"MDHIP_NO_OWN_FIRST": "1"}, path=lambda base: dict(base, own_first=0)),
    "no_tiles": dict(env={"MDHIP_NO_TILES": "1"}, path=lambda base: dict(tiled=0, fused_build=0, own_first=0, rows32=1)),
    # (lj_2d with rl = 2.5: five particles per cell, a tile spans more than 36 cells)
    "skin_0": dict(skin=0.0, path=lambda base: base, fallback=("lj_2d",)),
}


def default_path(case):
    """The build path a case is meant to take with no switch set."""
    return FALLBACK_PATH if case in FALLBACK_CASES else FUSED_PATH


def _fresh_build(name, case, path, skin=None, user=False):
    c = build_input(case)
    s = c["system"]
    skin = c["skin"] if skin is None else skin
    U = ra.lattice(cell_of(s), s["dim"])
    with _device(c, skin=skin, user=user) as dev:
        _upload(dev, s)
        assert dev.list_rows(0)["info"]["list_valid"] == 0 and len(dev.list_rows(0)["entries"]) == 0   # never builds
        dev.compute_forces()
        snap = ra.snapshot_of(dev)
        st = dev.stats()
    info = snap["info"]
    assert info["list_valid"] == 1 and info["inner_valid"] == 0 and info["n"] == s["n"]
    assert info["skin"] == effective_skin(U, c["cutoff"], skin) and info["rl"] == c["cutoff"] + info["skin"], info
    got = {k: info[k] for k in path}
    assert got == path and st["tiled"] == path["tiled"] and st["fused_build"] == path["fused_build"], (name, got, path)
    counts = _audit(name, snap, c)
    assert counts["disp0"] == 0.0 and np.array_equal(snap["x1"], snap["x0"])             # V1 at pos == x0
    assert _bands(counts) <= sa.MAX_EXCLUDED
    return snap, counts


@pytest.mark.parametrize("case", sorted(BUILD_CASES))
def test_fresh_build_default_path(case):
    _fresh_build(case, case, default_path(case))


@pytest.mark.parametrize("switch", sorted(BUILD_SWITCHES))
@pytest.mark.parametrize("case", ["blob", "lj_diam", "lj_2d"])
def test_fresh_build_path_switches(monkeypatch, case, switch):
    sw = BUILD_SWITCHES[switch]
    for k, v in sw.get("env", {}).items():
        monkeypatch.setenv(k, v)
    base = FALLBACK_PATH if case in sw.get("fallback", ()) else default_path(case)
    snap, _ = _fresh_build(case + "/" + switch, case, sw["path"](base), skin=sw.get("skin"))
    if switch == "skin_0":
        assert snap["info"]["skin"] == 0.0 and snap["info"]["rl"] == snap["info"]["rc"]


def test_fresh_build_user_potential():
    """Rows of a handle with a run-time compiled potential come from the same build (32-byte records)."""
    _fresh_build("lj_diam/user_lj", "lj_diam", FUSED_PATH, user=True)


# ---------------------------------------------------------------------------------------------------------------------
# (b) the list radius at the knife edge
# ---------------------------------------------------------------------------------------------------------------------
def _has(snap, i, j, nv):
    n = snap["info"]["n"]
    e = np.array([[i, j, *nv], [j, i, *(-np.asarray(nv))]], dtype=np.int32)
    return np.isin(ra.entry_keys(e, n), ra.entry_keys(snap["outer"], n))


@pytest.mark.parametrize("path", ["fused_build", "no_fused_build", "no_tiles"])
@pytest.mark.parametrize("case", KNIFE_CASES)
def test_list_radius_next_to_a_pair(monkeypatch, case, path):
    """rl = d / (1 - 1e-9) for a pair at distance d: the pair is 2e-9 (relative, in d2) inside rl^2 -- far outside the
    1e-12 band, far inside what fp32 resolves (6e-8) -- and must be in both rows; the fused build has only its 1e-4 margin
    for that.  With rl = d / (1 + 1e-9) the pair is just outside: what each path does then is printed, not asserted.
    (no_tiles: the same k_build_list as the fallback, its 32-bit rows read back through the ghost tables.)"""
    if path != "fused_build":
        monkeypatch.setenv("MDHIP_NO_FUSED_BUILD" if path == "no_fused_build" else "MDHIP_NO_TILES", "1")
    c = build_input(case)
    s = c["system"]
    n, dim = s["x"].shape
    U = ra.lattice(cell_of(s), dim)
    pairs = knife_pairs(case)
    assert pairs, "no knife-edge pair in this input"
    for kind, (i, j, nv, d) in sorted(pairs.items()):
        for side, rl in (("inside", d / (1.0 - KNIFE)), ("outside", d / (1.0 + KNIFE))):
            skin = rl - c["cutoff"]
            with _device(c, skin=skin) as dev:
                _upload(dev, s)
                dev.compute_forces()
                snap = ra.snapshot_of(dev)
            info = snap["info"]
            assert info["skin"] == skin and 0.3 - 1e-8 <= skin <= 0.9, (info["skin"], skin)      # (below the box clip)
            # (the blobs take the fallback on either setting: FALLBACK_CASES)
            fused = path == "fused_build" and case not in FALLBACK_CASES
            assert info["fused_build"] == (1 if fused else 0) and info["tiled"] == (0 if path == "no_tiles" else 1), info
            assert info["rows32"] == (1 if path == "no_tiles" else 0)
            # the tiles the pair was classified with are the device's: rows come back in slot order
            rows = snap["outer"][:, 0]
            rows = rows[np.concatenate([[True], rows[1:] != rows[:-1]])]
            order = slot_order(s["x"], U, info["rl"])
            assert np.array_equal(order[np.isin(order, rows)], rows), "the CPU slot order is not the device's"
            present = _has(snap, i, j, nv)
            name = "%s/%s/%s/%s" % (case, path, kind, side)
            counts = _audit(name, snap, c)
            assert _bands(counts) <= sa.MAX_EXCLUDED
            print("    pair (%d, %d, %s) d = %.12f, rl = d / (1 %s 1e-9): in row i %s, in row j %s"
                  % (i, j, nv[:dim].tolist(), d, "-" if side == "inside" else "+", bool(present[0]), bool(present[1])))
            if side == "inside":
                assert present.all(), "%s: a pair 2e-9 inside rl^2 is missing from the rows (%s)" % (name, present)


# ---------------------------------------------------------------------------------------------------------------------
# (c) rows in use
# ---------------------------------------------------------------------------------------------------------------------
def run_rows_in_use(oracle, name, schedule=MIXED, skin=None, inner_skin=None, nvt=False, label=None):
    """md_run over `schedule` on a fresh handle; the rows are audited after the first build (compute_forces: no inner rows
    yet) and after every segment.  Returns dict(snaps: the counts of every audited snapshot, stats, infos)."""
    from moleculardynamics.jl_amd.thermostat import draw_bussi
    c = build_input(name) if name in BUILD_CASES else dict(build_case(name))
    s = c["system"]
    skin = c.get("skin") if skin is None else skin
    inner_skin = c.get("inner_skin") if inner_skin is None else inner_skin
    total = int(sum(schedule))
    kw = {}
    if nvt:
        nf = s["dim"] * (s["n"] - 1.0)
        r1, r2 = draw_bussi(nf, np.random.default_rng(17), total)
        kT = 2.0 * float(oracle.kinetic(s["v"])) / nf
        kw = dict(ensemble=sa.NVT, tau=0.1, nf=nf, ktemp=np.full(total, kT), r1=r1, r2=r2)
    cache, snaps, infos = {}, [], []
    name = label or name
    with _device(c, skin=skin, inner_skin=inner_skin) as dev:
        _upload(dev, s)
        dev.compute_forces()
        snap = ra.snapshot_of(dev)
        snaps.append(_audit("%s/after the first build" % name, snap, c, cache))
        infos.append(snap["info"])
        a = 0
        for seg, (k, thermo) in enumerate(zip(schedule, sa.thermo_flags(schedule))):
            seg_kw = {key: (v[a:a + k] if key in ("ktemp", "r1", "r2") else v) for key, v in kw.items()}
            dev.run(k, c["dt"], thermo=thermo, **seg_kw)
            snap = ra.snapshot_of(dev)
            new_build = cache.get("tag") is None or cache["tag"][2] != snap["x0"].tobytes()
            counts = _audit("%s/segment %d (%d steps)" % (name, seg, k), snap, c, cache)
            counts["new_build"] = new_build
            snaps.append(counts)
            infos.append(snap["info"])
            a += k
        stats = dev.stats()
    bands = sum(x["band_rin"] + x["band_rc"] + (x["band_rl"] if x.get("new_build", True) else 0) for x in snaps)
    print("%-34s snapshots %d  rebuilds %d prunes %d | d2/rl^2 <= %.9f  d2(x1)/rin^2 <= %.12f | bands %d | V1 %.3f  V2 %.3f"
          % (name + " (all)", len(snaps), stats["rebuilds"], stats["prunes"], max(x["max_d2_over_rl2"] for x in snaps),
             max(x["max_d2x1_over_rin2"] for x in snaps), bands,
             max(x["disp0"] / x["limit0"] for x in snaps if x.get("limit0")) if skin != 0.0 else 0.0,
             max([x["disp1"] / x["limit1"] for x in snaps if x.get("limit1")] or [0.0])))
    assert bands <= sa.MAX_EXCLUDED
    return dict(snaps=snaps, stats=stats, infos=infos)


def _check_rows_coverage(res):
    """Without these a pass means little: freshly pruned inner rows, aged inner rows and rows without inner rows right after a
    build were all audited, and the lists turned over."""
    snaps, st = res["snaps"], res["stats"]
    fresh = sum(1 for x in snaps if x["inner_valid"] and x["disp1"] == 0.0)
    aged = sum(1 for x in snaps if x["inner_valid"] and x["disp1"] > 0.0)
    bare = sum(1 for x in snaps if x["list_valid"] and not x["inner_valid"] and x["disp0"] == 0.0)
    assert fresh >= 3 and aged >= 3 and bare >= 1, dict(fresh=fresh, aged=aged, bare=bare)
    assert st["rebuilds"] >= 2 and st["prunes"] >= 3, st
    assert all(x["list_valid"] for x in snaps)


ROWS_CASES = ["blob", "tiny3", "tiny65", "lj_diam", "lj_2d", "poly_2d", "phs_diam", "blob_sheared"]


@pytest.mark.parametrize("name", ROWS_CASES)
def test_rows_in_use_default_path(oracle, name):
    res = run_rows_in_use(oracle, name)
    assert res["stats"]["fused"] == 1
    _check_rows_coverage(res)


def test_rows_in_use_nvt(oracle):
    res = run_rows_in_use(oracle, "blob", nvt=True, label="blob/nvt")
    assert res["stats"]["fused"] == 1
    _check_rows_coverage(res)


@pytest.mark.parametrize("switch", list(SWITCHES))
@pytest.mark.parametrize("name", ["blob", "lj_diam"])
def test_rows_in_use_path_switches(oracle, monkeypatch, name, switch):
    sw = SWITCHES[switch]
    for k, v in sw.get("env", {}).items():
        monkeypatch.setenv(k, v)
    res = run_rows_in_use(oracle, name, skin=sw.get("skin"), inner_skin=sw.get("inner_skin"), label=name + "/" + switch)
    st, infos = res["stats"], res["infos"]
    assert st["steps"] == sum(MIXED) and st["rebuilds"] >= 2, st
    if "NO_FUSED_STEP" in "".join(sw.get("env", {})) or switch in ("no_tiles", "skin_0"):
        assert st["fused"] == 0, st
    if switch == "no_fused_build":
        assert st["fused_build"] == 0 and all(i["fused_build"] == 0 and i["tiled"] == 1 for i in infos), st
    if switch == "no_tiles":
        assert all(i["tiled"] == 0 and i["rows32"] == 1 for i in infos)
    if switch == "skin_0":
        assert st["rebuilds"] >= sum(MIXED) and all(x["disp0"] == 0.0 for x in res["snaps"]), st
    if switch in ("inner_skin_0", "skin_0", "no_tiles"):
        # no inner rows on these paths: every step walks the outer rows
        assert st["prunes"] == 0 and all(not x["inner_valid"] for x in res["snaps"]), st
        assert sum(1 for x in res["snaps"] if x["disp0"] > 0.0) >= (0 if switch == "skin_0" else 3)
    else:
        _check_rows_coverage(res)
        live = [i["inner_halo_live"] for i in infos if i["inner_valid"]]
        if switch == "no_fused_step_inner_halo":
            assert any(live), "no audited inner rows index the inner halo image"
        else:
            assert not any(live)


# ---------------------------------------------------------------------------------------------------------------------
# (d) Brownian and FIRE
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loop", ["brownian", "fire"])
def test_loops_that_end_without_a_valid_list(loop):
    """md_run_brownian and md_fire_minimize end on moved positions with list_valid = false; the next force evaluation builds."""
    c = build_input("blob")
    s = c["system"]
    with _device(c, skin=0.3) as dev:
        _upload(dev, s)
        dev.compute_forces()
        if loop == "brownian":
            dev.run_brownian(7, 4e-4, 1.5, 0xC0FFEE1234ABCDEF)
        else:
            dev.fire_minimize(max_steps=9, tol=1e-300, dt_initial=0.005, dt_max=0.03, nmin=0)
        o = dev.list_rows(0)
        assert o["info"]["list_valid"] == 0 and o["info"]["inner_valid"] == 0 and len(o["entries"]) == 0, o["info"]
        with pytest.raises(Exception, match="inner"):
            dev.list_rows(1)
        dev.compute_forces()
        snap = ra.snapshot_of(dev)
    assert snap["info"]["list_valid"] == 1 and {k: snap["info"][k] for k in FALLBACK_PATH} == default_path("blob")
    counts = _audit("blob/after %s" % loop, snap, c)
    assert counts["disp0"] == 0.0 and _bands(counts) <= sa.MAX_EXCLUDED
    assert np.abs(snap["pos"] - s["x"]).max() > 0.0                                   # (the loop did move the particles)
