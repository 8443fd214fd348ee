"""Own-first halo lists: k_build_tile gives halo slots 0..255 of every tile to the tile's own particles
and the fused step kernel writes those records to LDS from the registers that hold them instead of gathering them a
second time.  Only LDS slot numbers move: the candidates, their order in the rows, the coordinates and every sum stay
what they were, so a default handle and one created under MDHIP_NO_OWN_FIRST=1 (the numbering and the staging of before)
must agree in every bit, over list builds and prune steps, on ragged last tiles, periodic self-images inside a tile (a
box of three cells a side), 32-byte records and in two dimensions."""
import numpy as np
import pytest

from tests.util import lj_system, with_diameters

pytestmark = pytest.mark.gpu

LJ = [1.0, 1.0, 2.5]
KT = 1.4737
DT = 0.004
CHUNK, CAP = 40, 400


def _systems():
    return {
        "lj3d_n1000": lj_system(1000, kT=KT),                                   # 3 tiles + 232 lanes, 3 cells a side
        "lj3d_n2500": lj_system(2500, kT=KT),
        "lj3d_n1000_diam": with_diameters(lj_system(1000, kT=KT), 0.9, 1.1),    # 32-byte records
        "lj2d_n1500": lj_system(1500, rho=0.8, dim=2, kT=KT),
    }


def _noise(s):
    nf = s["dim"] * (s["n"] - 1.0)
    rng = np.random.default_rng(5)
    return nf, rng.standard_normal(CAP), 2.0 * rng.gamma((nf - 1) / 2, size=CAP), np.full(CAP, KT)


def _run(s, nvt, monkeypatch, env=None, nsteps=None):
    """One handle, run in chunks until two list builds and four prune steps have happened (or for `nsteps` steps, in the
    same chunks).  Returns (x, v, f, images), the (U, W, K) of every chunk, the stats and the steps taken."""
    from moleculardynamics.jl_amd import MDDevice, _lib
    for k in ("MDHIP_NO_OWN_FIRST", "MDHIP_NO_FUSED_BUILD", "MDHIP_NO_FUSED_STEP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    nf, r1, r2, kt = _noise(s)
    uwk, done = [], 0
    with MDDevice(s["dim"], s["n"], s["box"], 2.5) as d:
        d.set_potential(0, LJ)
        d.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        while done < (CAP if nsteps is None else nsteps):
            sl = slice(done, done + CHUNK)
            if nvt:
                uwk.append(tuple(d.run(CHUNK, DT, _lib.MD_NVT, 0.1, nf, kt[sl], r1[sl], r2[sl])))
            else:
                uwk.append(tuple(d.run(CHUNK, DT)))
            done += CHUNK
            st = d.stats()
            if nsteps is None and st["rebuilds"] >= 2 and st["prunes"] >= 4:
                break
        out = d.download()
        st = d.stats()
    return out, uwk, st, done


def _same(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a[0], b[0])) and a[1] == b[1]


@pytest.mark.parametrize("nvt", [True, False], ids=["nvt", "nve"])
@pytest.mark.parametrize("name", ["lj3d_n1000", "lj3d_n2500", "lj3d_n1000_diam", "lj2d_n1500"])
def test_own_first_changes_no_bit(name, nvt, monkeypatch):
    """Default handle against MDHIP_NO_OWN_FIRST=1 over at least two list builds and four prune steps: every bit of x, v,
    f, images and of the U, W, K of every chunk; then the flags.

    lj3d_n2500: a box of five cells a side, where the neighbour cells of a tile hold 3788-3920 staged entries (Smax of
    MDHIP_DEBUG=1 over the builds of this run) -- the system that needs k_build_tile's MD_SCAP = 4096; with 3584 it fell
    back to the two-kernel build and the flags below were 0."""
    s = _systems()[name]
    a = _run(s, nvt, monkeypatch)
    st, nsteps = a[2], a[3]
    print(name, "nvt" if nvt else "nve", "steps", nsteps, "rebuilds", st["rebuilds"], "prunes", st["prunes"],
          "max_halo", st["max_halo"])
    assert st["rebuilds"] >= 2 and st["prunes"] >= 4, "no list build / prune step inside the run"
    # the precondition: the default path repeats itself bit for bit
    a2 = _run(s, nvt, monkeypatch, nsteps=nsteps)
    assert _same(a, a2), "two default runs differ: the comparison below would mean nothing"
    b = _run(s, nvt, monkeypatch, env={"MDHIP_NO_OWN_FIRST": "1"}, nsteps=nsteps)
    assert b[2]["rebuilds"] == st["rebuilds"] and b[2]["prunes"] == st["prunes"]
    for what, p, q in zip("xvfi", a[0], b[0]):
        assert np.array_equal(p, q), f"{what} differs between own-first and cell-by-cell halo numbering"
    assert a[1] == b[1], "U, W, K differ"
    # (last, so that a system whose build takes the two-kernel fallback still has its trajectories compared above)
    assert b[2]["fused"] == 1 and b[2]["own_first"] == 0
    assert st["fused"] == 1 and st["fused_build"] == 1 and st["own_first"] == 1
    assert b[2]["fused_build"] == 1


def test_two_kernel_build_keeps_its_numbering(monkeypatch):
    """MDHIP_NO_FUSED_BUILD=1: rows and halo from k_build_list + k_tile_localize, which number the halo their own way, so
    the step kernel gathers every record.  Against the default handle, with the tolerance tests/test_gpu_parity.py
    (test_full_size_properties) uses for this pair of builds on one cell grid: forces bit-identical, U and W to 1e-13."""
    from moleculardynamics.jl_amd import MDDevice
    s = _systems()["lj3d_n1000"]
    res = []
    for env in ({}, {"MDHIP_NO_FUSED_BUILD": "1"}):
        monkeypatch.delenv("MDHIP_NO_FUSED_BUILD", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with MDDevice(3, s["n"], s["box"], 2.5) as d:
            d.set_potential(0, LJ)
            d.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
            u, w = d.compute_forces()
            f = d.download()[2]
            res.append((f, u, w))
    (f0, u0, w0), (f1, u1, w1) = res
    assert np.array_equal(f0, f1)
    assert abs(u1 - u0) <= 1e-13 * abs(u0) and abs(w1 - w0) <= 1e-13 * abs(w0)
    # the flag belongs to a step launch: a run over builds and prune steps.  (The trajectories of the two builds agree to
    # rounding only, before this change as after it: rows rebuilt from drifted positions need not list their entries in
    # one order.  Bounds: those tests/test_gpu_edge.py sets for two list strategies over prunes and rebuilds.)
    a = _run(s, True, monkeypatch)
    b = _run(s, True, monkeypatch, env={"MDHIP_NO_FUSED_BUILD": "1"}, nsteps=a[3])
    assert a[2]["own_first"] == 1
    assert b[2]["fused"] == 1 and b[2]["fused_build"] == 0 and b[2]["own_first"] == 0
    assert b[2]["rebuilds"] >= 2 and b[2]["prunes"] >= 4
    (xa, va, fa, ia), (xb, vb, fb, ib) = a[0], b[0]
    print("two-kernel build against default: max |dx| %.3e |dv| %.3e |df| %.3e" %
          (np.abs(xa - xb).max(), np.abs(va - vb).max(), np.abs(fa - fb).max()))
    assert np.array_equal(ia, ib) and np.abs(xa - xb).max() <= 1e-9 and np.abs(va - vb).max() <= 1e-9
    assert np.abs(fa - fb).max() <= 1e-7 * max(1.0, np.abs(fa).max())
    assert all(abs(p - q) <= 1e-9 * max(1.0, abs(p)) for ca, cb in zip(a[1], b[1]) for p, q in zip(ca, cb))


def test_classic_kernels_over_an_own_first_list(oracle, monkeypatch):
    """MDHIP_NO_FUSED_STEP=1: k_kickdrift + k_force_tile stage the whole own-first list, own slots included, through the
    index -> record gather.  Against the oracle, with the bounds of the classic trajectory tests
    (tests/test_gpu_edge.py::test_inner_halo_switch_changes_nothing_but_the_staging)."""
    s = _systems()["lj3d_n1000"]
    nf, r1, r2, kt = _noise(s)
    (x, v, f, img), uwk, st, nsteps = _run(s, True, monkeypatch, env={"MDHIP_NO_FUSED_STEP": "1"})
    assert st["fused"] == 0 and st["fused_build"] == 1 and st["own_first"] == 0
    assert st["rebuilds"] >= 2 and st["prunes"] >= 4
    ref = oracle.run(s["x"], s["img"], s["v"], s["f"], s["diam"], s["box"], 2.5, oracle.make_pot(0, LJ), DT, nsteps,
                     ensemble=1, tau=0.1, ktemp=kt, r1=r1, r2=r2, nthreads=8)
    assert np.array_equal(img, ref["img"]) and np.abs(x - ref["x"]).max() <= 1e-8
