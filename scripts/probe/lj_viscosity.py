"""Green-Kubo shear viscosity of the Lennard-Jones liquid near its triple point (T* = 0.722, rho* = 0.8442, r_c = 2.5,
truncated) from the device stress sampler: NVT equilibration, then an NVE run_simulation with stress=StressTensor(every,
nlags).  The literature's eta* for this state point is about 3.2-3.3 (full potential; a 2.5 sigma truncation lowers it a little).
Prints one JSON line: the plateau estimate (mean of eta(t) over the last fifth of the lag window), eta at a few lags, the
mean temperature and pressure, and the wall time.  A probe, not a test.
python scripts/probe/lj_viscosity.py [N] [steps] [every] [nlags] [dt]"""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

import moleculardynamics.jl_amd as md

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 1000000
every = int(sys.argv[3]) if len(sys.argv) > 3 else 5
nlags = int(sys.argv[4]) if len(sys.argv) > 4 else 300
dt = float(sys.argv[5]) if len(sys.argv) > 5 else 0.004
kT, rho = 0.722, 0.8442

params = md.Parameters(rho, n, dt, md.LennardJones())
with tempfile.TemporaryDirectory() as tmp:
    st = md.initialize_state(params, tmp, random_init=True, cutoff=2.5, rng=np.random.default_rng(2024))
    st.velocities = md.initialize_velocities(kT, np.random.default_rng(2025), n, 3)
    t0 = time.perf_counter()
    md.run_simulation(st, params, md.NVT(kT, 0.5), 30000, 10000, os.path.join(tmp, "eq"), write_trajectory=False)
    t_eq = time.perf_counter() - t0
    stress = md.StressTensor(every, nlags=nlags)
    t0 = time.perf_counter()
    md.run_simulation(st, params, md.NVE(), steps, 100000, os.path.join(tmp, "run"), write_trajectory=False, stress=stress)
    t_run = time.perf_counter() - t0
    st.system.device.close()
t, eta = stress.viscosity()
_, c, cs = stress.acf()
tail = eta[-max(nlags // 5, 1):]
out = dict(n=n, steps=steps, every=every, nlags=nlags, dt=dt, nsamples=int(stress.nsamples),
           temperature=stress.temperature(), pressure=stress.pressure(), eta_plateau=float(tail.mean()),
           eta_plateau_spread=float(tail.max() - tail.min()),
           eta_at={"%.2f" % t[k]: float(eta[k]) for k in range(0, nlags, max(nlags // 10, 1))},
           c_shear0=float(cs[0]), c_channels0=[float(v) for v in c[0]], wall_eq_s=t_eq, wall_run_s=t_run)
print(json.dumps(out), flush=True)
