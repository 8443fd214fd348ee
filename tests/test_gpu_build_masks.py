"""The fused per-tile list build (k_build_tile) keeps a cell's hits as two 32-bit words: staged candidates 0-31 and
32-63 of the cell.  The benchmark's state point (about 27 particles per cell) reaches the second word only by chance;
the systems here are made so that it is always in use:

  * "mixed": cells of 27 to 48 particles (3-D) -- cells whose second word is empty next to cells whose second word
    holds a few candidates;
  * "full": the same with the fullest cell topped up to exactly 64 particles (interstitial sites) -- a second word of
    all 32 candidates, the particle's own bit in either word.  (A uniform system of 64 per cell does not fit the fused
    build at all: a tile's staged set and its 16-bit halo offsets end near 2700 particles.)
  * cells of 36 to 49 particles in 2-D (the kernel's other instantiation);
  * a cell of more than 64 particles, which no mask holds: the two-kernel fallback has to take over.

Pair set, forces, energy and virial against the oracle, with the tolerances of test_gpu_parity.py.  The cell
populations are computed here with the device's own binning rule (floor(L / (cutoff + skin)) cells per axis, at least
three) and asserted, without a GPU, by test_inputs_fill_the_cells_as_intended."""
import numpy as np
import pytest

from tests.util import lj_system

LJ = [1.0, 1.0, 2.5]

# dimension, particles, density, skin; need_max: the range in which the largest cell population has to fall
# (the lattice start of lj_system puts 13 sites per axis over 4 cells (3-D): 3 or 4 per cell and axis, so at most
# 4^3 = 64 per cell; 13 over 3 cells -> up to 5^3)
CASES = {
    "two_words_3d_mixed": dict(dim=3, n=13 ** 3, rho=1.2, skin=0.5, need_max=(33, 64)),
    "two_words_3d_full": dict(dim=3, n=13 ** 3, rho=1.2, skin=0.5, need_max=(64, 64), top_up=64),
    "two_words_2d": dict(dim=2, n=40 ** 2, rho=1.2, skin=3.0, need_max=(33, 64)),
    "cell_above_64": dict(dim=3, n=13 ** 3, rho=1.2, skin=0.6, need_max=(65, 10 ** 9)),
}


def _cells(x, box, rl):
    """Cells per axis and every particle's cell coordinates, as the device bins them (mdhip.hip, configure_grid)."""
    k = np.maximum(3, np.floor(box / rl).astype(int))
    while np.any((box / k < rl) & (k > 3)):
        k = np.where((box / k < rl) & (k > 3), k - 1, k)
    return k, np.minimum((x * (k / box)).astype(int), k - 1)


def _cell_populations(x, box, rl):
    k, idx = _cells(x, box, rl)
    flat = np.ravel_multi_index(tuple(idx.T), tuple(k))
    return np.bincount(flat, minlength=int(np.prod(k)))


def _top_up(s, rl, target):
    """Adds particles to the fullest cell until it holds `target`: body-centred interstitial sites of the lattice (0.81
    from the nearest particle at this density), at least a tenth of a lattice spacing inside the cell."""
    x, box = s["x"], s["box"]
    k, idx = _cells(x, box, rl)
    pop = _cell_populations(x, box, rl)
    cell = np.array(np.unravel_index(int(np.argmax(pop)), tuple(k)))
    m = round(len(x) ** (1.0 / 3.0))
    h = box / m
    sites = np.stack(np.meshgrid(*[np.arange(1, m)] * 3, indexing="ij"), -1).reshape(-1, 3) * h
    lo, hi = cell * box / k, (cell + 1) * box / k
    sites = sites[np.all((sites > lo + 0.1 * h) & (sites < hi - 0.1 * h), axis=1)]
    extra = sites[: target - pop.max()]
    assert len(extra) == target - pop.max(), "not enough interstitial sites in the cell"
    n = len(x) + len(extra)
    return dict(n=n, dim=3, box=box, x=np.ascontiguousarray(np.concatenate([x, extra])), v=np.zeros((n, 3)),
                f=np.zeros((n, 3)), img=np.zeros((n, 3), dtype=np.int32), diam=np.ones(n))


def _system(case):
    c = CASES[case]
    s = lj_system(c["n"], rho=c["rho"], dim=c["dim"])
    if "top_up" in c:
        s = _top_up(s, 2.5 + c["skin"], c["top_up"])
    return s, c


@pytest.mark.parametrize("case", sorted(CASES))
def test_inputs_fill_the_cells_as_intended(case):
    s, c = _system(case)
    pop = _cell_populations(s["x"], s["box"], 2.5 + c["skin"])
    lo, hi = c["need_max"]
    assert lo <= pop.max() <= hi, f"largest cell holds {pop.max()} particles"
    if case == "two_words_3d_mixed":
        assert pop.min() <= 32                            # second words without a candidate
    if case == "two_words_3d_full":
        assert np.sum(pop == 64) == 1 and np.any((pop > 32) & (pop < 64))   # one full second word, others partly filled


def _forces_and_pairs(oracle, s, skin):
    from moleculardynamics.jl_amd import MDDevice
    pot = oracle.make_pot(oracle.POT_LJ, LJ)
    f_ref, u_ref, w_ref, pairs_ref = oracle.forces_brute(s["x"], s["box"], 2.5, pot, s["diam"], want_pairs=True)
    with MDDevice(s["dim"], s["n"], s["box"], 2.5) as d:
        d.set_potential(0, LJ)
        d.set_skin(skin)
        d.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        u, w = d.compute_forces()
        _, _, f, _ = d.download()
        pairs = d.neighbor_pairs()
        st = d.stats()
    pr = pairs_ref[np.lexsort((pairs_ref[:, 1], pairs_ref[:, 0]))]
    assert pairs.shape == pr.shape and np.array_equal(pairs, pr), "neighbour pair set differs"
    scale = max(1.0, np.abs(f_ref).max())
    err = np.abs(f - f_ref).max()
    assert err <= 1e-11 * scale, f"force error {err:.3e} > {1e-11 * scale:.3e}"
    assert abs(u - u_ref) <= 1e-12 * abs(u_ref)
    assert abs(w - w_ref) <= 1e-12 * abs(w_ref)
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["two_words_3d_mixed", "two_words_3d_full", "two_words_2d"])
def test_cells_beyond_32_particles(oracle, case):
    s, c = _system(case)
    st = _forces_and_pairs(oracle, s, c["skin"])
    assert st["tiled"] == 1 and st["fused_build"] == 1, "the fused tiled build was not used"


@pytest.mark.gpu
def test_cell_beyond_64_particles_falls_back(oracle):
    s, c = _system("cell_above_64")
    st = _forces_and_pairs(oracle, s, c["skin"])
    assert st["fused_build"] == 0, "a cell of more than 64 particles cannot have gone through the fused build"


@pytest.mark.gpu
def test_rebuilds_during_a_run_with_two_word_cells(oracle):
    """The same dense system through md_run: list builds, prune steps and the fused step loop on rows that came out of
    second mask words, against the oracle's trajectory (tolerances of test_gpu_parity.py's 10-step run)."""
    from moleculardynamics.jl_amd import MDDevice
    s, c = _system("two_words_3d_mixed")
    pot = oracle.make_pot(oracle.POT_LJ, LJ)
    ref = oracle.run(s["x"], s["img"], s["v"], s["f"], s["diam"], s["box"], 2.5, pot, 0.001, 10, use_cells=True,
                     nthreads=1)
    with MDDevice(3, s["n"], s["box"], 2.5) as d:
        d.set_potential(0, LJ)
        d.set_skin(c["skin"])
        d.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        U, W, K = d.run(10, 0.001)
        x, v, f, img = d.download()
        st = d.stats()
    assert st["fused_build"] == 1
    assert np.abs(x - ref["x"]).max() <= 1e-10
    assert np.abs(v - ref["v"]).max() <= 1e-10
    assert np.abs(f - ref["f"]).max() <= 1e-10 * max(1.0, np.abs(ref["f"]).max())
    assert np.array_equal(img, ref["img"])
    assert abs(U - ref["U"]) <= 1e-11 * abs(ref["U"])
