"""Time a swap Monte Carlo round (md_swap_*) on the bench-sized system: N = 2^20, 3-D LJ with diameters U[0.9, 1.1],
rho = 0.897, list cutoff 2.5, after a short run -- for each fraction the time of one round (device events on the handle's
stream around md_swap_rounds(1 + R) and md_swap_rounds(1): the difference over R leaves out the call's preamble, its force
refresh and its wait), the counts proposed -> live -> decided -> accepted, and in the same process one ordinary md_run step
and one md_boo_sample (l = 6), an N-wide walk of the same outer rows.  Prints one JSON line per stage.
python scripts/probe/swap_rate.py [--profile]
--profile: a few calls only -- the run to put under `rocprofv3 --kernel-trace --stats` (a run of its own)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
profile = "--profile" in sys.argv
import torch                                            # noqa: E402  (torch first, as bench.py does)
torch.cuda.set_device(0)
torch.zeros(1, device="cuda")
from moleculardynamics.jl_amd import MDDevice, lattice_positions, initialize_velocities  # noqa: E402

N, rho = 1 << 20, 0.897
box = np.full(3, (N / rho) ** (1.0 / 3.0))
x0 = lattice_positions(N, box, 3, np.random.default_rng(12345))
v0 = initialize_velocities(1.0, np.random.default_rng(67890), N, 3)
diam = np.random.default_rng(11).uniform(0.9, 1.1, N)
dev = MDDevice(3, N, box, 2.5)
stream = torch.cuda.Stream()
assert dev._L.md_set_stream(dev._h, C.c_void_p(stream.cuda_stream)) == 0


def timed(fn):
    """(result, milliseconds between two events on the handle's stream around fn(), host milliseconds)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record(stream)
    r = fn()
    e1.record(stream)
    e1.synchronize()
    return r, e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


dev.set_potential(0, [1.0, 1.0, 2.5])
dev.upload(x0, v0, np.zeros_like(x0), np.zeros((N, 3), np.int32), diam)
dev.run(300, 0.002)                                     # melt the jittered lattice a little, settle the list schedule
_, ms, host = timed(lambda: dev.run(200, 0.002))
kT = 2.0 * dev.kinetic() / (3.0 * (N - 1.0))
st = dev.stats()
out = {"N": N, "step_ms": ms / 200, "step_ms_host": host / 200, "kT": kT, "tiled": st["tiled"], "max_halo": st.get("max_halo"),
       "avg_neighbors": st.get("avg_neighbors")}
dev.boo_setup(1.5, 6, 100, 0.7, 7, 0)
dev.boo_sample()
dev.boo_read()
K = 3 if profile else 20
_, ms, host = timed(lambda: [dev.boo_sample() for _ in range(K)] and dev.boo_read())
out["boo_sample_ms"] = ms / K
out["boo_sample_ms_host"] = host / K
print(json.dumps(out), flush=True)

R = 4 if profile else 64
first = 0
for fraction in (0.002, 0.005, 0.01, 0.02):
    dev.swap_setup(fraction, None, 2024)
    dev.swap_rounds(1, kT, first_round=first)           # warm every kernel of the round
    first += 1
    per_round, one_call, res = [], [], None
    for rep in range(1 if profile else 5):              # alternate the two lengths: the spread is in the output
        res, ms_long, _ = timed(lambda: dev.swap_rounds(1 + R, kT, first_round=first))
        first += 1 + R
        _, ms_one, _ = timed(lambda: dev.swap_rounds(1, kT, first_round=first))
        first += 1
        per_round.append((ms_long - ms_one) / R)
        one_call.append(ms_one)
    live = res["proposed"] - res["void"] - res["lost"]
    rounds = 1 + R
    med = float(np.median(per_round))
    print(json.dumps({"fraction": fraction, "round_ms": med, "round_ms_min": min(per_round), "round_ms_max": max(per_round),
                      "call_of_one_round_ms": float(np.median(one_call)),
                      "proposed_per_round": res["proposed"] / rounds, "live_per_round": live / rounds,
                      "blocked_per_round": res["blocked"] / rounds, "decided_per_round": res["decided"] / rounds,
                      "accepted_per_round": res["accepted"] / rounds,
                      "decided_over_proposed": res["decided"] / max(res["proposed"], 1),
                      "us_per_decided_swap": 1e3 * med / max(res["decided"] / rounds, 1e-9),
                      "round_over_boo_sample": med / out["boo_sample_ms"], "round_over_step": med / out["step_ms"]}),
          flush=True)
d = dev.diameters()
assert np.array_equal(np.sort(d), np.sort(diam))
dev.close()
