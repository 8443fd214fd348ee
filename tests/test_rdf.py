"""CPU tests of the g(r) layer (analysis.py, the Julia twin's binding): edges, normalisation, file format.  The device
histogram itself is tested in tests/test_gpu_rdf.py."""
import math
import os
import re

import numpy as np
import pytest

import moleculardynamics.jl_amd as md
from moleculardynamics.jl_amd import RadialDistribution, compute_rdf
from moleculardynamics.jl_amd.analysis import RadialDistribution as RD2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exported_from_the_package():
    assert RadialDistribution is RD2
    assert "RadialDistribution" in md.__all__ and "compute_rdf" in md.__all__
    assert callable(compute_rdf)


def test_edges_and_centres():
    rdf = RadialDistribution(4.0, 400)
    assert rdf.edges.shape == (401,) and rdf.r.shape == (400,)
    assert rdf.edges[0] == 0.0 and rdf.edges[-1] == pytest.approx(4.0, rel=1e-15)
    delta = 4.0 / 400
    # the device's table: e2[k] = (k delta)^2 with k as a double
    assert np.array_equal(rdf.edges, np.arange(401, dtype=np.float64) * delta)
    assert np.allclose(rdf.r, (np.arange(400) + 0.5) * delta, rtol=1e-15)
    assert rdf.counts.dtype == np.int64 and rdf.nsamples == 0
    assert np.all(rdf.g() == 0.0)


@pytest.mark.parametrize("dim", [2, 3])
def test_uniform_density_gives_one(dim):
    """Synthetic counts of an ideal gas (the expected number of pairs in every shell) normalise to exactly 1."""
    n, nbins, r_max, nsamples = 5000, 50, 3.0, 7
    U = np.diag([20.0, 25.0, 30.0][:dim])
    V = abs(np.linalg.det(U))
    rdf = RadialDistribution(r_max, nbins)
    e = rdf.edges
    Vk = 4.0 * math.pi / 3.0 * (e[1:] ** 3 - e[:-1] ** 3) if dim == 3 else math.pi * (e[1:] ** 2 - e[:-1] ** 2)
    expect = nsamples * n * (n - 1) / (2.0 * V) * Vk
    rdf._accumulate(np.zeros(nbins, np.int64), 0, n, U)          # (the unit cell is what sets V and the dimension)
    rdf.counts = expect.copy()                                   # float counts: exact expectation
    rdf.nsamples = nsamples
    assert np.allclose(rdf.g(), 1.0, rtol=1e-13, atol=0)
    # integer counts accumulate, and reset() empties them
    rdf2 = RadialDistribution(r_max, nbins)
    c = np.rint(expect / nsamples).astype(np.int64)
    for _ in range(nsamples):
        rdf2._accumulate(c, 1, n, U)
    assert rdf2.nsamples == nsamples and np.array_equal(rdf2.counts, nsamples * c)
    assert np.allclose(rdf2.g()[5:], 1.0, rtol=2e-2)
    rdf2.reset()
    assert rdf2.nsamples == 0 and not rdf2.counts.any()


def test_argument_checks():
    for bad in [(0.0, 10), (-1.0, 10), (float("inf"), 10), (1.0, 0), (1.0, 8193)]:
        with pytest.raises(ValueError):
            RadialDistribution(*bad)
    with pytest.raises(ValueError):
        RadialDistribution(1.0, 10, every=0)
    assert RadialDistribution(1.0, 8192).nbins == 8192


def test_write_format(tmp_path):
    rdf = RadialDistribution(2.0, 4)
    rdf._accumulate(np.array([0, 3, 10, 25]), 2, 100, np.diag([10.0, 10.0, 10.0]))
    p = tmp_path / "rdf.txt"
    rdf.write(str(p))
    lines = p.read_text().splitlines()
    assert lines[0] == "# r g(r) count"
    assert len(lines) == 5
    g = rdf.g()
    for k, line in enumerate(lines[1:]):
        assert re.fullmatch(r"\d+\.\d{6} -?\d+\.\d{6} \d+", line), line
        assert line == "%.6f %.6f %d" % (rdf.r[k], g[k], rdf.counts[k])
    assert lines[2].split()[0] == "0.750000" and lines[4].endswith(" 25")


def test_julia_binds_the_rdf_entries():
    src = open(os.path.join(ROOT, "julia", "MDHip.jl")).read()
    for name in ("md_rdf_setup", "md_rdf_sample", "md_rdf_read", "md_rdf_reset"):
        assert re.search(r"ccall\(\(:" + name + r",\s*LIB\)", src), f"MDHip.jl does not bind {name}"
    assert "struct RadialDistribution" in src and "function compute_rdf(" in src
    assert re.search(r"rdf::Union\{Nothing,\s*RadialDistribution\}\s*=\s*nothing", src)
    assert '"# r g(r) count"' in src and '"%.6f %.6f %d\\n"' in src
