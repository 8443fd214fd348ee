"""Time the elastic-moduli passes (md_elas_affine, md_elas_solve) on the bench system: N = 2^20 LJ, rho = 0.897, d = 3, taken
to a minimum by the device's FIRE first (the solve needs a positive semi-definite H).  Synchronised wall clock, fields left on
the device: the affine pass over `ncalls` calls, `rounds` times; one conjugate-gradient iteration (one block apply of 8
vectors, two dot-product kernels with their finishes, two update kernels) from the difference of two solves capped at 32 and
96 iterations; then the solve to tol (default 1e-10) for the iteration counts.  The split of an iteration into the apply and
the vector kernels is read from a kernel trace of this script (rocprofv3 --kernel-trace --stats -- python
scripts/probe/elas_rate.py N 2 1 out 64: the last argument caps the final solve).  Prints one JSON line and writes it to `out`
(default profiles/elas_rate.txt).
python scripts/probe/elas_rate.py [N] [ncalls] [rounds] [out] [max_iter] [tol]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np

from moleculardynamics.jl_amd import MDDevice, _lib, lattice_positions, initialize_velocities

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
ncalls = int(sys.argv[2]) if len(sys.argv) > 2 else 5
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "elas_rate.txt")
max_iter = int(sys.argv[5]) if len(sys.argv) > 5 else 3 * n
tol = float(sys.argv[6]) if len(sys.argv) > 6 else 1e-10
rho = 0.897
L = (n / rho) ** (1.0 / 3.0)
box = np.full(3, L)
x = lattice_positions(n, box, 3, np.random.default_rng(12345))
v = initialize_velocities(1.4737, np.random.default_rng(67890), n, 3)
out = dict(n=n, rho=rho, ncalls=ncalls, tol=tol, max_iter=max_iter)


def timed(call, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        r = call()
    return (time.perf_counter() - t0) * 1e3 / reps, r


with MDDevice(3, n, box, 2.5) as dev:
    dev.set_potential(_lib.MD_POT_LJ, [1.0, 1.0, 2.5])
    dev.upload(x, v, np.zeros_like(x), np.zeros((n, 3), np.int32), np.ones(n))
    dev.run(200, 0.001)
    t0 = time.perf_counter()
    fire = dev.fire_minimize(max_steps=40000, tol=1e-8, dt_initial=0.002, dt_max=0.02)
    out["fire"] = dict(fire, seconds=time.perf_counter() - t0)
    dev.hess_setup()
    dev.elas_affine()
    dev.elas_solve(tol, 8, fields=False)                                      # (allocations, first launches)
    res = dict(affine_ms=[], solve_32_ms=[], solve_96_ms=[], compute_forces_ms=[])
    for _ in range(rounds):
        res["affine_ms"].append(timed(dev.elas_affine, ncalls)[0])
        res["compute_forces_ms"].append(timed(dev.compute_forces, ncalls)[0])
        res["solve_32_ms"].append(timed(lambda: dev.elas_solve(tol, 32, fields=False), 1)[0])
        res["solve_96_ms"].append(timed(lambda: dev.elas_solve(tol, 96, fields=False), 1)[0])
    out.update(res)
    out["best"] = {k: min(val) for k, val in res.items()}
    out["iteration_ms"] = (out["best"]["solve_96_ms"] - out["best"]["solve_32_ms"]) / 64.0
    aff = dev.elas_affine()
    ms, sol = timed(lambda: dev.elas_solve(tol, max_iter, fields=False), 1)
    out["solve_ms"] = ms
    out["iterations"] = [int(i) for i in sol["iterations"]]
    out["status"] = sol["status"]
    out["residual_over_xi"] = [float(r / x) for r, x in zip(sol["residuals"], sol["xi_norm"])]
    N = sol["nonaffine"]
    C = aff["born"] + 0.5 * (N + N.T)
    out["asymmetry"] = float(np.abs(N - N.T).max())
    out["born_shear"] = float(np.mean([aff["born"][i, i] for i in (3, 4, 5)]))
    out["shear"] = float(np.mean([C[i, i] for i in (3, 4, 5)]))
    out["bulk"] = float(C[:3, :3].sum() / 9.0)
    out["pressure"] = float(-aff["stress"][:3].mean())
    st = dev.stats()
    out["tiled"] = st["tiled"]
line = json.dumps(out)
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
with open(path, "w") as fh:
    fh.write("scripts/probe/elas_rate.py %d %d %d (synchronised wall clock, fields left on the device; ms)\n%s\n" % (n, ncalls, rounds, line))
