"""Time one device sample of g(r) (md_rdf_sample) on the bench system: N = 2^20 LJ, rho = 0.897, r_max = 4.0, 400 bins,
after a short equilibration; then the cost of sampling inside run_simulation (rdf at every output step, frequency 100)
against the same run without it.  Prints one JSON line.
python scripts/probe/rdf_rate.py [N] [nsamples] [steps]"""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

import moleculardynamics.jl_amd as md
from moleculardynamics.jl_amd import MDDevice, _lib, lattice_positions, initialize_velocities

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
nsamp = int(sys.argv[2]) if len(sys.argv) > 2 else 40
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
rho, r_max, nbins = 0.897, 4.0, 400
L = (n / rho) ** (1.0 / 3.0)
box = np.full(3, L)
x = lattice_positions(n, box, 3, np.random.default_rng(12345))
v = initialize_velocities(1.4737, np.random.default_rng(67890), n, 3)
out = dict(n=n, rho=rho, r_max=r_max, nbins=nbins)

with MDDevice(3, n, box, 2.5) as dev:
    dev.set_potential(_lib.MD_POT_LJ, [1.0, 1.0, 2.5])
    dev.upload(x, v, np.zeros_like(x), np.zeros((n, 3), np.int32), np.ones(n))
    dev.run(200, 0.001)
    dev.rdf_setup(r_max, nbins)
    for _ in range(5):
        dev.rdf_sample()
    dev.rdf_read()                                   # waits for the stream
    t0 = time.perf_counter()
    for _ in range(nsamp):
        dev.rdf_sample()
    counts, ns = dev.rdf_read()
    t1 = time.perf_counter()
    out["ms_per_sample"] = (t1 - t0) * 1e3 / nsamp
    out["samples_timed"] = nsamp
    out["pairs_per_sample"] = int(counts.sum() // ns)
    xs = dev.download()[0]

# run_simulation with and without rdf (NVE, thermo at every 100th step, no trajectory file), same start
params = md.Parameters(rho, n, 0.001, md.LennardJones())
walls = {}
with tempfile.TemporaryDirectory() as tmp:
    for label in ("warmup", "plain", "rdf", "plain2", "rdf2"):
        st = md.initialize_state(params, None, cutoff=2.5, positions=xs, diameters=np.ones(n), unitcell=L)
        st.velocities = v.copy()
        rdf = md.RadialDistribution(r_max, nbins) if label.startswith("rdf") else None
        t0 = time.perf_counter()
        md.run_simulation(st, params, md.NVE(), steps, 100, os.path.join(tmp, label), write_trajectory=False, rdf=rdf)
        walls[label] = time.perf_counter() - t0
        st.system.device.close()
plain = min(walls["plain"], walls["plain2"])
with_rdf = min(walls["rdf"], walls["rdf2"])
out["run_simulation"] = dict(steps=steps, frequency=100, samples=steps // 100, wall_s_plain=plain, wall_s_rdf=with_rdf,
                             overhead_frac=(with_rdf - plain) / plain, walls=walls)
print(json.dumps(out), flush=True)
