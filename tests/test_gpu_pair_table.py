"""-m gpu: the pair-table audit (tests/pair_table.py) on an MDDevice -- every built-in potential and
the plugin, pair by pair over isolated dimers, against the same formulas in numpy.longdouble, on every kernel that
evaluates a pair: md_compute_forces (tiled and MDHIP_NO_TILES=1), the step loop's prune-step and inner-row kernels
(fused and MDHIP_NO_FUSED_STEP=1, with and without energies), md_stress_tensor, md_hess_blocks, md_swap_rounds, and the
branch thresholds one ulp either side.  Bounds: pair_table.bounds (10 x the reference's own rounding floor, plus the one-step
reciprocal's documented error for the r^-2 Lennard-Jones forms).  Every test prints its largest error / S in units of
2^-53; DESIGN.md section 24 holds the table."""
import numpy as np
import pytest

from tests import pair_table as pt
from tests.test_gpu_parity import USER_LJ_SRC

pytestmark = pytest.mark.gpu

ENVS = {"default": {}, "no_tiles": {"MDHIP_NO_TILES": "1"}, "no_fused_step": {"MDHIP_NO_FUSED_STEP": "1"}}
SWAP_SEED, SWAP_KT = 7, 2.0          # tests/test_pair_table.py: the reference alone meets swap_conditions with these

DEFAULT = ([(c, "mixed", 3) for c in pt.CASES] +
           [(c, v, 3) for c in ("lj", "lj_eps", "lj_wca", "lj_sigma", "lj_list") for v in ("ones", "uniform", "ulp")] +
           [(c, v, 3) for c in ("phs50", "poly", "ljmod1") for v in ("uniform", "ulp")] +
           [("lj", "uniform", 2), ("poly", "mixed", 2)])
SWITCHED = [("lj_eps", "uniform", 3), ("lj_eps", "mixed", 3), ("phs24", "mixed", 3), ("poly_14", "mixed", 3),
            ("ljmod2", "mixed", 3)]


def _open(t, plugin=False):
    from moleculardynamics.jl_amd import MDDevice
    d = MDDevice(t["dim"], t["n"], t["box"], t["cutoff"])
    if plugin:
        d.set_potential_source(USER_LJ_SRC, "user_lj", pt.PLUGIN_PARAMS)
    else:
        d.set_potential(t["kind"], t["params"])
    d.upload(t["x"], t["v"], t["f"], t["img"], t["diam"])
    return d


def _note(worst, key, value):
    if isinstance(value, dict):
        for k, v in value.items():
            _note(worst, key + " " + k, v)
    else:
        worst[key] = max(worst.get(key, 0.0), value)


def _steps(d, t, x, B, band, worst, expect_prune, thermo):
    """md_run(1, 1e-30) twice at positions x (nothing moves): with inner rows the first call is a prune step, the second
    walks the inner rows -- asserted from stats() and list_rows(), not assumed."""
    for call in range(2):
        p0 = d.stats()["prunes"]
        uwk = d.run(1, 1e-30, thermo=thermo)
        st = d.stats()
        xd, _, f, _ = d.download()
        assert np.array_equal(xd, x)
        if expect_prune:
            assert st["prunes"] - p0 == (1 if call == 0 else 0), (call, st)
            assert d.list_rows(1)["info"]["inner_valid"] == 1
            name = "prune step" if call == 0 else "inner rows"
        else:
            assert st["prunes"] == 0, st
            name = "outer rows step"
        name += " thermo" if thermo else ""
        _note(worst, name + " f", pt.check_pair_forces(t, f, B, x=x, what=name))
        if thermo and band is not None:
            _note(worst, name, pt.check_band_sums(t, band, B, uwk[0], uwk[1], x=x, what=name))
    return f


def _audit(oracle, t, path, plugin=False):
    builtin = not plugin
    r2 = t["kind"] == pt.POT_LJ and builtin
    B = pt.bounds(t, r2)
    worst = {}
    with _open(t, plugin) as d:
        u, w = d.compute_forces()
        st = d.stats()
        assert st["tiled"] == (0 if path == "no_tiles" else 1), st
        _, _, f, _ = d.download()
        _note(worst, "compute f", pt.check_pair_forces(t, f, B, what="md_compute_forces"))
        pt.check_decisions(t, oracle, f, d.neighbor_pairs())
        if builtin and path == "default":
            d.hess_setup()
            _note(worst, "hess blk", pt.check_blocks(t, d.hess_blocks(), pt.bounds(t, False)))
            d.stress_setup(0)
        fused = builtin and path == "default"
        inner = path != "no_tiles" and builtin
        for band in list(range(len(t["band_names"]))) + [None]:
            x = t["x"] if band is None else pt.pulled(t, band)
            d.upload(x=x)
            if band is not None:
                u, w = d.compute_forces()
                _note(worst, "compute", pt.check_band_sums(t, band, B, u, w, x=x, what="md_compute_forces"))
                if builtin and path == "default":
                    d.stress_sample()
                    _, vir = d.stress_tensor()
                    _note(worst, "stress", pt.check_band_sums(t, band, B, vir=vir, x=x, what="md_stress_tensor"))
            last = {}
            for thermo in (True, False):
                d.upload(x, t["v"], t["f"], t["img"], t["diam"])
                last[thermo] = _steps(d, t, x, B, band, worst, inner, thermo)
                st = d.stats()
                assert st["fused"] == (1 if fused else 0), st
            if r2 and inner and t["dim"] == 3 and band is None and t["variant"] in ("ones", "uniform"):
                # one diameter, 3-D, no energies: the inner-row kernel takes the sigma-folded ljA z^7 - ljB z^4 form on a shared
                # reciprocal.  No counter names it; that it ran shows in forces that are within bound and NOT the bits of
                # the energy-computing instantiation (every other table prints equal figures for the two)
                assert not np.array_equal(last[True], last[False])
    print("%s/%s/%dd %s%s: %s" % (t["case"], t["variant"], t["dim"], path, " plugin" if plugin else "",
                                  "  ".join("%s %.1f" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("case,variant,dim", DEFAULT, ids=["%s-%s-%dd" % c for c in DEFAULT])
def test_default_path(oracle, case, variant, dim):
    _audit(oracle, pt.make_table(case, variant, dim), "default")


@pytest.mark.parametrize("path", ["no_tiles", "no_fused_step"])
@pytest.mark.parametrize("case,variant,dim", SWITCHED, ids=["%s-%s-%dd" % c for c in SWITCHED])
def test_path_switches(oracle, monkeypatch, case, variant, dim, path):
    for k, v in ENVS[path].items():
        monkeypatch.setenv(k, v)
    _audit(oracle, pt.make_table(case, variant, dim), path)


@pytest.mark.parametrize("variant", ["mixed", "uniform"])
def test_plugin(oracle, variant):
    """USER_LJ_SRC at (0.37, 2.2) against the LJ table of the same parameters: the plugin has no fused and no inner-row path
    (asserted in _audit: fused == 0, prunes == 0), and goes through sqrt and a division: no reciprocal term in its bound."""
    _audit(oracle, pt.make_table("lj_eps", variant), "default", plugin=True)


@pytest.mark.parametrize("case", ["lj", "poly", "phs50", "ljmod1"])
def test_swap(oracle, case):
    t = pt.make_table(case, "mixed")
    key = [SWAP_SEED & 0xffffffff, SWAP_SEED >> 32]
    w3 = np.array([oracle.philox([i, 0, 0, 1], key)[3] for i in range(t["n"])])
    with _open(t) as d:
        d.swap_setup(1.0, None, SWAP_SEED)
        d.swap_rounds(1, SWAP_KT)
        partner, status, du = d.swap_last()
    res = pt.check_swap(t, partner, status, du, t["diam"], w3, SWAP_KT, pt.bounds(t, t["kind"] == pt.POT_LJ)["u"])
    print("%s swap: %s" % (case, res))
    pt.swap_conditions(res)


@pytest.mark.parametrize("name", list(pt.THRESHOLDS))
def test_threshold_dimers(oracle, name):
    """Squared separations on the branch's d2 threshold, one ulp either side, and between the reference-form and the fma-chain
    value: pair set and zero / non-zero force pattern the oracle's bit for bit on md_compute_forces and both md_run kernels
    (across r_on, where the value is continuous: the values only), values within bound."""
    t = pt.threshold_table(name)
    B = pt.bounds(t, t["kind"] == pt.POT_LJ, quantities=("u", "f"))
    worst = {}
    with _open(t) as d:
        d.compute_forces()
        _, _, f, _ = d.download()
        pt.check_decisions(t, oracle, f, d.neighbor_pairs(), what="md_compute_forces")
        _note(worst, "compute f", pt.check_pair_forces(t, f, B))
        for thermo in (False, True):
            d.upload(t["x"], t["v"], t["f"], t["img"], t["diam"])
            for call in range(2):
                p0 = d.stats()["prunes"]
                d.run(1, 1e-30, thermo=thermo)
                st = d.stats()
                assert st["fused"] == 1 and st["prunes"] - p0 == (1 if call == 0 else 0), st
                xd, _, f, _ = d.download()
                assert np.array_equal(xd, t["x"])
                what = ("prune step" if call == 0 else "inner rows") + (" thermo" if thermo else "")
                pt.check_decisions(t, oracle, f, what=what)
                _note(worst, what + " f", pt.check_pair_forces(t, f, B, what=what))
    print("%s: %s" % (name, "  ".join("%s %.1f" % kv for kv in sorted(worst.items()))))
