"""The row audit (tests/row_audit.py) proved on the CPU: check_rows passes a numpy model of the two-level list scheme and
reports every sabotage of it; and the knife-edge bands of the device module's build-only inputs are empty.

The model (3-D blob, 2-D liquid, sheared blob -- systems of tests/test_gpu_step_audit.build_case): a brute-force outer
build at x0 that keeps d2 <= rl^2 (1 + 1e-4), as the fused device build does in exact arithmetic, with one pair moved into
that margin so that it is never empty; a prune at x1 = x0 + random displacements of at most 0.3 skin / 2 that keeps the
outer entries with d2(x1) <= rin^2 in the outer order; and pos = x1 + displacements of at most 0.9 of the limit
min(inner / 2, skin / 2 - d1).  A second snapshot of each system has no inner rows (the state right after a list build).

Sabotages.  Each is reported under its own invariant, and under no other -- except where the defect is by its nature also
a defect of another invariant, which the expected set then names:
   1  a shell pair (rc, rl] removed from the rows (both directions)         O1      (from one row only: O1 and O2 -- a
                                                                                    one-sided removal is an asymmetry)
   2  the reverse direction of the margin pair removed                       O2
   3  an entry duplicated                                                    O3
   4  a wrong image vector on an entry beyond rc (both directions of the
      margin pair, consistently)                                             O4      (on one entry of a shell pair: the
                                                                                    right entry is also missing, and its
                                                                                    mirror alone: O1, O2, O4)
   5  a self entry                                                           O3
   6  rows built at 1.2 rl                                                   O4
   7  an inner entry that is not in the outer row                            I1, I4  (what is not in the outer row is
                                                                                    farther than rin at x1)
   8  two inner entries swapped                                              I2
   9  an inner row missing a pair inside rin (and outside rc at pos)         I3
  10  x1 shifted so that d1 is under-reported                                V2
  11  a particle moved by 0.6 skin with list_valid set (no inner rows)       V1
  12  a pair inside rc absent from the rows to be walked                     I3, V3  (V3 follows from the other ten: a row
                                                                                    that breaks it breaks I3 or O1 too)
"""
import numpy as np
import pytest

from tests import row_audit as ra
from tests import test_gpu_row_audit as gra
from tests.test_gpu_step_audit import build_case

MODEL_SYSTEMS = ["blob", "lj_2d", "blob_sheared"]


def _cell_of(s):
    return s["box"] if s.get("cell") is None else s["cell"]


def _rows_from_keys(keys, n):
    return ra.keys_to_entries(np.sort(keys), n)          # ascending keys: rows contiguous, by (i, j, image)


def _unit(rng, m, dim):
    v = rng.standard_normal((m, dim))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def model_snapshot(name, with_inner=True, build_factor=1.0, seed=5):
    c = build_case(name)
    s = c["system"]
    n, dim = s["x"].shape
    U = ra.lattice(_cell_of(s), dim)
    rc, skin, inner_skin = c["cutoff"], c.get("skin", 0.6), c.get("inner_skin", 0.16)
    rl, rin = rc + skin, rc + inner_skin
    rng = np.random.default_rng(seed)
    x0 = s["x"].copy()
    # the margin pair: the shell pair closest to rl, its first particle moved along the bond to rl sqrt(1 + 0.5e-4)
    keys, d2 = ra.pairs_within(x0, U, rl * rl)
    k = int(np.argmax(d2))
    e = ra.keys_to_entries(keys[k:k + 1], n)[0]
    bond = x0[e[1]] + ra.image_shift(e[None, 2:2 + dim], U)[0] - x0[e[0]]
    r = np.linalg.norm(bond)
    x0[e[0]] -= bond / r * (rl * np.sqrt(1.0 + 0.5 * ra.FUSED_MARGIN) - r)
    okeys, od2 = ra.pairs_within(x0, U, (build_factor * rl) ** 2 * (1.0 + ra.FUSED_MARGIN))
    outer = _rows_from_keys(okeys, n)
    info = dict(rc=rc, skin=skin, rl=rl, inner_skin=0.0, d1=0.0, list_valid=1, inner_valid=0, tiled=1, fused_build=1,
                own_first=1, inner_halo_live=0, n=n, rows32=0, n_ghost=0, virtual_ghosts=1, prune_on=1)
    if not with_inner:
        pos = x0 + _unit(rng, n, dim) * rng.uniform(0.0, 0.1 * 0.5 * skin, (n, 1))
        snap = dict(info=info, x0=x0, x1=x0.copy(), pos=pos, outer=outer, inner=None)
    else:
        x1 = x0 + _unit(rng, n, dim) * rng.uniform(0.0, 0.3 * 0.5 * skin, (n, 1))
        d1 = float(np.sqrt(((x1 - x0) ** 2).sum(axis=1)).max())
        inner = outer[ra.entry_d2(x1, outer, U) <= rin * rin]
        limit = min(0.5 * inner_skin, 0.5 * skin - d1)
        pos = x1 + _unit(rng, n, dim) * rng.uniform(0.0, 0.9 * limit, (n, 1))
        info.update(inner_skin=inner_skin, d1=d1, inner_valid=1)
        snap = dict(info=info, x0=x0, x1=x1, pos=pos, outer=outer, inner=inner)
    margin = np.array([e, [e[1], e[0], -e[2], -e[3], -e[4]]], dtype=np.int32)
    return snap, U, dim, _cell_of(s), margin


_MODELS = {}


def _model(name, with_inner=True):
    """The model snapshots, built once per system (the tests copy what they change)."""
    key = (name, with_inner)
    if key not in _MODELS:
        _MODELS[key] = model_snapshot(name, with_inner)
    snap, U, dim, cell, margin = _MODELS[key]
    return dict(snap, info=dict(snap["info"]), **{k: snap[k].copy() for k in ("x0", "x1", "pos", "outer")},
                inner=None if snap["inner"] is None else snap["inner"].copy()), U, dim, cell, margin


def _checks(res):
    return sorted({v.check for v in res["violations"]})


def _find(ent, e):
    return int(np.flatnonzero((ent == np.asarray(e, dtype=np.int32)).all(axis=1))[0])


def _mirror(e):
    return [e[1], e[0], -e[2], -e[3], -e[4]]


def _drop(ent, *entries):
    keep = np.ones(len(ent), dtype=bool)
    for e in entries:
        keep[_find(ent, e)] = False
    return ent[keep]


def _shell_entry(snap, U, lo, hi, at="x0", rows="outer", also=None):
    """The first entry of `rows` with lo < d(at) <= hi (and, with also=(at2, lo2, hi2), lo2 < d(at2) <= hi2 too)."""
    ent = snap[rows]
    d = np.sqrt(ra.entry_d2(snap[at], ent, U))
    ok = (d > lo) & (d <= hi)
    if also is not None:
        d2 = np.sqrt(ra.entry_d2(snap[also[0]], ent, U))
        ok &= (d2 > also[1]) & (d2 <= also[2])
    assert ok.any(), "the model has no such entry"
    return ent[int(np.flatnonzero(ok)[0])].copy()


@pytest.mark.parametrize("with_inner", [True, False])
@pytest.mark.parametrize("name", MODEL_SYSTEMS)
def test_the_checker_passes_the_model(name, with_inner):
    snap, U, dim, cell, margin = _model(name, with_inner)
    res = ra.check_rows(snap, cell, dim)
    print(ra.counts_line("%s/model%s" % (name, "" if with_inner else "/no_inner"), res["counts"]))
    assert res["violations"] == [], res["violations"]
    c = res["counts"]
    assert c["band_rl"] == c["band_rin"] == c["band_rc"] == 0
    assert c["required_rl"] > 0 and c["required_rc"] > 0 and c["outer_entries"] > c["required_rl"]     # (the margin pair)
    assert 1.0 < c["max_d2_over_rl2"] <= 1.0 + ra.FUSED_MARGIN
    if with_inner:
        assert 0 < c["inner_entries"] < c["outer_entries"] and c["disp1"] > 0.0 and c["d1_true"] > 0.0
        assert c["max_d2x1_over_rin2"] <= 1.0


def _sabotage(kind, name):
    """(sabotaged snapshot, cell, dim, expected invariants)"""
    with_inner = kind not in ("moved_0p6_skin",)
    snap, U, dim, cell, margin = _model(name, with_inner)
    info = snap["info"]
    rc, rl, skin = info["rc"], info["rl"], info["skin"]
    rin = rc + info["inner_skin"]
    n = info["n"]
    if kind == "shell_pair_removed":
        e = _shell_entry(snap, U, rin + 2 * info["d1"] + 1e-3, rl)       # (not in the inner rows either)
        snap["outer"] = _drop(snap["outer"], e, _mirror(e))
        return snap, cell, dim, ["O1"]
    if kind == "shell_entry_removed_from_one_row":
        e = _shell_entry(snap, U, rin + 2 * info["d1"] + 1e-3, rl)
        snap["outer"] = _drop(snap["outer"], e)
        return snap, cell, dim, ["O1", "O2"]
    if kind == "reverse_direction_removed":
        snap["outer"] = _drop(snap["outer"], margin[1])
        return snap, cell, dim, ["O2"]
    if kind == "entry_duplicated":
        k = len(snap["outer"]) // 2
        snap["outer"] = np.insert(snap["outer"], k, snap["outer"][k], axis=0)
        return snap, cell, dim, ["O3"]
    if kind == "wrong_image_both_directions":
        v = 1 if margin[0][2] <= 0 else -1
        k0, k1 = _find(snap["outer"], margin[0]), _find(snap["outer"], margin[1])
        snap["outer"][k0, 2], snap["outer"][k1, 2] = v, -v
        return snap, cell, dim, ["O4"]
    if kind == "wrong_image_one_entry":
        e = _shell_entry(snap, U, rin + 2 * info["d1"] + 1e-3, rl)
        k = _find(snap["outer"], e)
        snap["outer"][k, 2] = 1 if e[2] <= 0 else -1
        return snap, cell, dim, ["O1", "O2", "O4"]
    if kind == "self_entry":
        # (at the head of a row, and -- as a prune step would keep an entry at distance 0 -- of its inner row too)
        i = int(snap["inner"][len(snap["inner"]) // 3, 0])
        row = np.array([i, i, 0, 0, 0], dtype=np.int32)
        for rows in ("outer", "inner"):
            snap[rows] = np.insert(snap[rows], int(np.flatnonzero(snap[rows][:, 0] == i)[0]), row, axis=0)
        return snap, cell, dim, ["O3"]
    if kind == "built_at_1p2_rl":
        wide = model_snapshot(name, True, build_factor=1.2)[0]
        return wide, cell, dim, ["O4"]
    if kind == "inner_entry_not_in_outer":
        i = int(snap["inner"][len(snap["inner"]) // 2, 0])
        d2 = ra.entry_d2(snap["x0"], np.array([[i, j, 0, 0, 0] for j in range(n)], dtype=np.int32), U)
        j = int(np.argmax(d2 > (1.5 * rl) ** 2))
        k = _find_row_end(snap["inner"], i)
        snap["inner"] = np.insert(snap["inner"], k, np.array([i, j, 0, 0, 0], dtype=np.int32), axis=0)
        return snap, cell, dim, ["I1", "I4"]
    if kind == "inner_entries_swapped":
        ent = snap["inner"]
        k = int(np.flatnonzero(ent[1:, 0] == ent[:-1, 0])[len(ent) // 4])
        ent[[k, k + 1]] = ent[[k + 1, k]]
        return snap, cell, dim, ["I2"]
    if kind == "inner_row_misses_a_pair":
        e = _shell_entry(snap, U, rc + 1e-3, rin - 1e-3, at="x1", rows="inner", also=("pos", rc + 1e-3, 1e9))
        snap["inner"] = _drop(snap["inner"], e)
        return snap, cell, dim, ["I3"]
    if kind == "d1_under_reported":
        p = int(np.argmax(((snap["x1"] - snap["x0"]) ** 2).sum(axis=1)))
        d = snap["x1"][p] - snap["x0"][p]
        snap["x1"][p] += d / np.linalg.norm(d) * 1e-9
        return snap, cell, dim, ["V2"]
    if kind == "moved_0p6_skin":
        p = n // 2
        snap["pos"][p] = snap["x0"][p] + _unit(np.random.default_rng(1), 1, dim)[0] * 0.6 * skin
        return snap, cell, dim, ["V1"]
    if kind == "pair_inside_rc_absent":
        e = _shell_entry(snap, U, 0.0, rc - 1e-3, at="pos", rows="inner")
        snap["inner"] = _drop(snap["inner"], e, _mirror(e))
        return snap, cell, dim, ["I3", "V3"]
    raise KeyError(kind)


def _find_row_end(ent, i):
    return int(np.flatnonzero(ent[:, 0] == i)[-1]) + 1


SABOTAGES = ["shell_pair_removed", "shell_entry_removed_from_one_row", "reverse_direction_removed", "entry_duplicated",
             "wrong_image_both_directions", "wrong_image_one_entry", "self_entry", "built_at_1p2_rl",
             "inner_entry_not_in_outer", "inner_entries_swapped", "inner_row_misses_a_pair", "d1_under_reported",
             "moved_0p6_skin", "pair_inside_rc_absent"]


@pytest.mark.parametrize("kind", SABOTAGES)
@pytest.mark.parametrize("name", MODEL_SYSTEMS)
def test_every_sabotage_is_reported_under_its_own_invariant(name, kind):
    snap, cell, dim, expected = _sabotage(kind, name)
    res = ra.check_rows(snap, cell, dim)
    assert _checks(res) == sorted(expected), (kind, [str(v) for v in res["violations"]])


def test_undecodable_entries_and_invalid_lists():
    """What md_list_rows reports for an entry it cannot decode (id_j = -1, image component 2) is a hygiene violation; a
    handle without valid rows has nothing to audit."""
    snap, U, dim, cell, margin = _model("lj_2d")
    snap["outer"][7, 1] = -1
    snap["outer"][11, 3] = 2
    assert "O3" in _checks(ra.check_rows(snap, cell, dim))
    snap, U, dim, cell, margin = _model("lj_2d")
    snap["info"]["list_valid"] = 0
    res = ra.check_rows(dict(snap, outer=snap["outer"][:0], inner=None), cell, dim)
    assert res["violations"] == [] and res["counts"]["list_valid"] == 0


@pytest.mark.parametrize("case", sorted(gra.BUILD_CASES))
def test_build_only_inputs_have_empty_knife_edge_bands(case):
    """The bands of the fresh-build tests depend on the uploaded positions alone: no pair within 1e-12 (relative, in d2)
    of rl^2 -- with the case's skin after the box clip, and with skin 0 -- or of rc^2, and no pair with two images inside
    rl.  So the cap of the device tests hides nothing."""
    c = gra.build_input(case)
    s = c["system"]
    dim = s["dim"]
    U = ra.lattice(_cell_of(s), dim)
    for skin in sorted({gra.effective_skin(U, c["cutoff"], c["skin"]), 0.0}):
        viol = []
        req, band = ra.required_pairs(s["x"], U, c["cutoff"] + skin, "x", viol)
        print("%-22s skin %.4f: %d ordered pairs within rl, band %d" % (case, skin, len(req), band))
        assert viol == [] and band == 0


def test_knife_edge_pairs_cover_every_kind():
    """The pairs the device module puts rl next to, picked here without a device: the two liquids offer all four kinds;
    the blob's gas (120 particles on a grid of spacing 2 in a 24^3 box) has no pair of the right distance across an edge
    or corner, sheared or not, so the blobs run the other three."""
    for case in gra.KNIFE_CASES:
        pairs = gra.knife_pairs(case)
        kinds = set(gra.KNIFE_KINDS) if case in ("lj_diam", "lj_2d") else set(gra.KNIFE_KINDS[:3])
        assert set(pairs) == kinds, (case, sorted(pairs))
        c = gra.build_input(case)
        for i, j, nv, d in pairs.values():
            assert 0.3 <= d / (1.0 - gra.KNIFE) - c["cutoff"] <= 0.9
