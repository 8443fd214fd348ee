"""-m gpu: the step audit (tests/step_audit.py) on the slab-decomposed step loops -- DomainDevice.run, run_async and
run_native with 1 to 4 ranks on one GPU -- through a multi-process stepper (tests/domain_audit_worker.py; the harness is
proved on a CPU model in tests/test_slab_audit.py).  One launch is one combination of rank count, path and switch and runs
its cases in sequence; at most 4 processes have the GPU open at a time, every launch under its own time limit.

Measured margins (MI355X; records, not tolerances), step_audit.margins_line of every case of every launch: the worst error
of each quantity as a fraction of audit_run's own, unchanged bound -- F, U, W, K: check (A); one step: the derived bounds
8 spacing(L) and 0.5 dt tol_F + 4 spacing(|v|inf); <= 10 steps: 1e-10; excluded: particles the knife-edge precondition left
out.  No slab case missed a one-step bound (the worst is a quarter of it), so no slab-specific bound was derived and
audit_run has no new parameter.  No image exception anywhere.

  sync-2 blob                  F 0.001  U 0.008  W 0.011  K 0.002 | one step: x 0.125  v 0.006 | <= 10 steps: x 3.20e-04  v 1.00e-03 | excluded 0
  sync-2 lj_diam_long          F 0.002  U 0.010  W 0.011  K 0.002 | one step: x 0.125  v 0.004 | <= 10 steps: x 1.78e-04  v 2.86e-03 | excluded 0
  sync-2 ljmod0                F 0.002  U 0.017  W 0.011  K 0.002 | one step: x 0.125  v 0.005 | <= 10 steps: x 1.42e-04  v 3.41e-03 | excluded 0
  sync-2 ljmod1                F 0.002  U 0.014  W 0.008  K 0.002 | one step: x 0.125  v 0.005 | <= 10 steps: x 1.42e-04  v 4.65e-03 | excluded 0
  sync-2 ljmod2                F 0.002  U 0.011  W 0.014  K 0.002 | one step: x 0.250  v 0.005 | <= 10 steps: x 1.78e-04  v 3.52e-03 | excluded 0
  sync-2 lj_2d                 F 0.005  U 0.004  W 0.016  K 0.002 | one step: x 0.062  v 0.007 | <= 10 steps: x 2.49e-04  v 4.41e-03 | excluded 0
  sync-2 poly_2d               F 0.003  U 0.003  W 0.005  K 0.002 | one step: x 0.125  v 0.009 | <= 10 steps: x 3.20e-04  v 2.28e-03 | excluded 0
  sync-2 phs                   F 0.000  U 0.000  W 0.000  K 0.001 | one step: x 0.062  v 0.001 | <= 10 steps: x 8.88e-05  v 2.08e-03 | excluded 0
  sync-2 phs_diam              F 0.000  U 0.000  W 0.000  K 0.001 | one step: x 0.062  v 0.001 | <= 10 steps: x 8.88e-05  v 2.65e-03 | excluded 0
  sync-2 poly_3d               F 0.001  U 0.003  W 0.003  K 0.001 | one step: x 0.125  v 0.002 | <= 10 steps: x 1.07e-04  v 5.51e-04 | excluded 0
  sync-3 blob                  F 0.001  U 0.008  W 0.012  K 0.002 | one step: x 0.125  v 0.006 | <= 10 steps: x 3.55e-04  v 1.10e-03 | excluded 0
  sync-3 lj_diam_long          F 0.002  U 0.010  W 0.012  K 0.002 | one step: x 0.125  v 0.006 | <= 10 steps: x 2.13e-04  v 3.96e-03 | excluded 0
  sync-3 ljmod0                F 0.002  U 0.016  W 0.014  K 0.002 | one step: x 0.125  v 0.005 | <= 10 steps: x 2.13e-04  v 3.69e-03 | excluded 0
  sync-3 ljmod1                F 0.002  U 0.012  W 0.016  K 0.003 | one step: x 0.125  v 0.006 | <= 10 steps: x 1.78e-04  v 4.82e-03 | excluded 0
  sync-3 ljmod2                F 0.002  U 0.015  W 0.008  K 0.003 | one step: x 0.125  v 0.008 | <= 10 steps: x 2.13e-04  v 4.64e-03 | excluded 0
  sync-3 lj_2d                 F 0.004  U 0.004  W 0.022  K 0.001 | one step: x 0.062  v 0.007 | <= 10 steps: x 2.49e-04  v 4.08e-03 | excluded 0
  sync-3 poly_2d               F 0.003  U 0.003  W 0.004  K 0.002 | one step: x 0.125  v 0.010 | <= 10 steps: x 3.20e-04  v 3.70e-03 | excluded 0
  sync-3 phs                   F 0.001  U 0.000  W 0.000  K 0.001 | one step: x 0.062  v 0.001 | <= 10 steps: x 8.88e-05  v 4.41e-03 | excluded 0
  sync-3 phs_diam              F 0.000  U 0.000  W 0.000  K 0.001 | one step: x 0.062  v 0.001 | <= 10 steps: x 8.88e-05  v 7.18e-03 | excluded 0
  sync-3 poly_3d               F 0.001  U 0.003  W 0.002  K 0.001 | one step: x 0.125  v 0.003 | <= 10 steps: x 1.07e-04  v 5.58e-04 | excluded 0
  sync-nvt-3 blob              F 0.001  U 0.009  W 0.012  K 0.002 | one step: x 0.125  v 0.000 | <= 10 steps: x 2.13e-04  v 1.55e-03 | excluded 0
  sync-nvt-3 poly_2d           F 0.004  U 0.002  W 0.002  K 0.003 | one step: x 0.125  v 0.003 | <= 10 steps: x 3.20e-04  v 2.24e-03 | excluded 0
  async-prune-nvt-2 blob       F 0.001  U 0.009  W 0.014  K 0.002 | one step: x 0.125  v 0.000 | <= 10 steps: x 2.13e-04  v 1.52e-03 | excluded 0
  async-prune-nvt-2 lj_diam_long F 0.002  U 0.014  W 0.010  K 0.002 | one step: x 0.125  v 0.002 | <= 10 steps: x 1.42e-04  v 4.31e-03 | excluded 0
  async-prune-nvt-2 lj_2d      F 0.005  U 0.003  W 0.016  K 0.002 | one step: x 0.125  v 0.002 | <= 10 steps: x 2.49e-04  v 4.10e-03 | excluded 0
  async-prune-nvt-2 phs_diam   F 0.000  U 0.000  W 0.000  K 0.001 | one step: x 0.125  v 0.000 | <= 10 steps: x 5.33e-05  v 6.09e-03 | excluded 0
  async-prune-nvt-3 blob       F 0.001  U 0.009  W 0.012  K 0.002 | one step: x 0.125  v 0.000 | <= 10 steps: x 2.13e-04  v 1.54e-03 | excluded 0
  async-prune-nvt-3 lj_diam_long F 0.002  U 0.010  W 0.013  K 0.003 | one step: x 0.125  v 0.003 | <= 10 steps: x 1.78e-04  v 4.83e-03 | excluded 0
  async-prune-nvt-3 lj_2d      F 0.004  U 0.004  W 0.022  K 0.002 | one step: x 0.125  v 0.002 | <= 10 steps: x 2.13e-04  v 3.13e-03 | excluded 0
  async-prune-nvt-3 phs_diam   F 0.000  U 0.000  W 0.000  K 0.001 | one step: x 0.125  v 0.000 | <= 10 steps: x 5.33e-05  v 6.34e-03 | excluded 0
  native-prune-2 blob          F 0.001  U 0.009  W 0.009  K 0.002 | one step: x 0.250  v 0.010 | <= 10 steps: x 3.20e-04  v 1.73e-03 | excluded 0
  native-prune-2 lj_diam_long  F 0.005  U 0.011  W 0.009  K 0.003 | one step: x 0.250  v 0.010 | <= 10 steps: x 1.78e-04  v 5.97e-03 | excluded 0
  native-prune-2 ljmod0        F 0.005  U 0.018  W 0.008  K 0.003 | one step: x 0.250  v 0.008 | <= 10 steps: x 2.13e-04  v 5.63e-03 | excluded 0
  native-prune-2 ljmod1        F 0.003  U 0.011  W 0.008  K 0.003 | one step: x 0.250  v 0.010 | <= 10 steps: x 1.78e-04  v 4.77e-03 | excluded 0
  native-prune-2 ljmod2        F 0.003  U 0.012  W 0.015  K 0.003 | one step: x 0.250  v 0.009 | <= 10 steps: x 2.13e-04  v 4.40e-03 | excluded 0
  native-prune-2 lj_2d         F 0.006  U 0.003  W 0.023  K 0.002 | one step: x 0.125  v 0.014 | <= 10 steps: x 2.84e-04  v 5.93e-03 | excluded 0
  native-prune-2 poly_2d       F 0.006  U 0.003  W 0.003  K 0.003 | one step: x 0.250  v 0.013 | <= 10 steps: x 4.26e-04  v 5.27e-03 | excluded 0
  native-prune-2 phs           F 0.001  U 0.000  W 0.000  K 0.001 | one step: x 0.125  v 0.001 | <= 10 steps: x 8.88e-05  v 4.97e-03 | excluded 0
  native-prune-2 phs_diam      F 0.000  U 0.000  W 0.000  K 0.001 | one step: x 0.125  v 0.001 | <= 10 steps: x 8.88e-05  v 6.84e-03 | excluded 0
  native-prune-2 poly_3d       F 0.002  U 0.003  W 0.002  K 0.002 | one step: x 0.250  v 0.006 | <= 10 steps: x 1.24e-04  v 1.23e-03 | excluded 0
  native-prune-nvt-3 blob      F 0.001  U 0.007  W 0.011  K 0.001 | one step: x 0.250  v 0.001 | <= 10 steps: x 2.49e-04  v 2.37e-03 | excluded 0
  native-prune-nvt-3 lj_diam_long F 0.003  U 0.008  W 0.015  K 0.002 | one step: x 0.250  v 0.004 | <= 10 steps: x 2.13e-04  v 8.11e-03 | excluded 0
  native-prune-nvt-3 ljmod0    F 0.004  U 0.017  W 0.013  K 0.002 | one step: x 0.250  v 0.006 | <= 10 steps: x 2.49e-04  v 7.51e-03 | excluded 0
  native-prune-nvt-3 ljmod1    F 0.003  U 0.014  W 0.011  K 0.002 | one step: x 0.250  v 0.004 | <= 10 steps: x 2.84e-04  v 8.22e-03 | excluded 0
  native-prune-nvt-3 ljmod2    F 0.003  U 0.013  W 0.017  K 0.002 | one step: x 0.250  v 0.004 | <= 10 steps: x 2.49e-04  v 6.77e-03 | excluded 0
  native-prune-nvt-3 lj_2d     F 0.005  U 0.003  W 0.014  K 0.001 | one step: x 0.125  v 0.004 | <= 10 steps: x 3.20e-04  v 5.62e-03 | excluded 0
  native-prune-nvt-3 poly_2d   F 0.007  U 0.002  W 0.002  K 0.001 | one step: x 0.250  v 0.006 | <= 10 steps: x 4.26e-04  v 3.04e-03 | excluded 0
  native-prune-nvt-3 phs       F 0.000  U 0.000  W 0.000  K 0.001 | one step: x 0.125  v 0.001 | <= 10 steps: x 7.11e-05  v 7.66e-03 | excluded 0
  native-prune-nvt-3 phs_diam  F 0.001  U 0.000  W 0.000  K 0.001 | one step: x 0.125  v 0.001 | <= 10 steps: x 7.99e-05  v 7.03e-03 | excluded 0
  native-prune-nvt-3 poly_3d   F 0.002  U 0.002  W 0.003  K 0.001 | one step: x 0.250  v 0.001 | <= 10 steps: x 1.42e-04  v 1.27e-03 | excluded 0
  native-prune-4 blob          F 0.001  U 0.008  W 0.009  K 0.002 | one step: x 0.250  v 0.010 | <= 10 steps: x 3.55e-04  v 2.10e-03 | excluded 0
  native-prune-4 lj_2d         F 0.006  U 0.004  W 0.023  K 0.002 | one step: x 0.125  v 0.014 | <= 10 steps: x 2.84e-04  v 5.94e-03 | excluded 0
  native-prune-ones-2 blob     F 0.001  U 0.006  W 0.201  K 0.001 | one step: x 0.250  v 0.014 | <= 10 steps: x 0.00e+00  v 0.00e+00 | excluded 0
  native-prune-ones-2 lj_diam_long F 0.005  U 0.019  W 0.019  K 0.003 | one step: x 0.250  v 0.014 | <= 10 steps: x 0.00e+00  v 0.00e+00 | excluded 0
  native-prune-2/p2p_0 blob    F 0.001  U 0.009  W 0.009  K 0.002 | one step: x 0.250  v 0.010 | <= 10 steps: x 3.20e-04  v 1.73e-03 | excluded 0
  native-prune-2/p2p_0 lj_diam_long F 0.005  U 0.011  W 0.009  K 0.003 | one step: x 0.250  v 0.010 | <= 10 steps: x 1.78e-04  v 5.97e-03 | excluded 0
  native-prune-2/p2p_split blob F 0.001  U 0.009  W 0.009  K 0.002 | one step: x 0.250  v 0.010 | <= 10 steps: x 3.20e-04  v 1.73e-03 | excluded 0
  native-prune-2/p2p_split lj_diam_long F 0.005  U 0.011  W 0.010  K 0.003 | one step: x 0.250  v 0.010 | <= 10 steps: x 1.78e-04  v 5.97e-03 | excluded 0
  native-prune-2/no_fused_step blob F 0.001  U 0.008  W 0.014  K 0.001 | one step: x 0.125  v 0.006 | <= 10 steps: x 3.20e-04  v 1.00e-03 | excluded 0
  native-prune-2/no_fused_step lj_diam_long F 0.002  U 0.010  W 0.012  K 0.002 | one step: x 0.125  v 0.004 | <= 10 steps: x 1.78e-04  v 2.86e-03 | excluded 0
  native-prune-2/no_tiles blob F 0.001  U 0.008  W 0.012  K 0.002 | one step: x 0.125  v 0.006 | <= 10 steps: x 3.20e-04  v 1.14e-03 | excluded 0
  native-prune-2/no_tiles lj_diam_long F 0.002  U 0.010  W 0.011  K 0.002 | one step: x 0.125  v 0.004 | <= 10 steps: x 1.78e-04  v 2.84e-03 | excluded 0
  native-prune-2/no_fused_build blob F 0.001  U 0.009  W 0.009  K 0.002 | one step: x 0.250  v 0.010 | <= 10 steps: x 3.20e-04  v 1.73e-03 | excluded 0
  native-prune-2/no_fused_build lj_diam_long F 0.005  U 0.011  W 0.010  K 0.003 | one step: x 0.250  v 0.010 | <= 10 steps: x 1.78e-04  v 5.97e-03 | excluded 0
  rccl-native-prune-1 blob     F 0.001  U 0.007  W 0.009  K 0.001 | one step: x 0.250  v 0.001 | <= 10 steps: x 2.49e-04  v 2.17e-03 | excluded 0
  rccl-native-prune-1 lj_diam  F 0.002  U 0.006  W 0.008  K 0.002 | one step: x 0.250  v 0.003 | <= 10 steps: x 1.07e-04  v 2.52e-03 | excluded 0
  void-sync-4 void             F 0.001  U 0.008  W 0.009  K 0.001 | one step: x 0.125  v 0.006 | <= 10 steps: x 2.13e-04  v 1.13e-03 | excluded 0
  void-sync-nvt-4 void         F 0.001  U 0.008  W 0.008  K 0.002 | one step: x 0.125  v 0.001 | <= 10 steps: x 1.78e-04  v 1.21e-03 | excluded 0
  void-native-prune-4 void     F 0.001  U 0.008  W 0.011  K 0.001 | one step: x 0.250  v 0.010 | <= 10 steps: x 3.20e-04  v 1.37e-03 | excluded 0

Fused-window exception (a rank's tiles stop fitting and all ranks fall back to the classic window, which
tests/domain_gpu_worker.py tolerates for DOM_POLY): used by no case, so the module has none -- every native launch without
MDHIP_NO_FUSED_STEP / MDHIP_NO_TILES had fused_windows == windows == direct_windows (22 to 65 windows a case; with
MDHIP_DOM_P2P=0 direct_windows == 0), the 2-D, per-particle-diameter and empty-slab cases included.

void: ranks 0 and 3 owned no particle from upload to the end (owner_of on every gathered state and md_dom_counts agree);
68 owner changes across the face between ranks 1 and 2 (52 to 67 of them followed by the handles at list builds), none
across the seam, which nothing can reach in 79 steps.  The prune count of a launch is the largest over the ranks' handles,
so the prune assertions hold for void too, whose leader owns nothing (40 prunes; inner rows in use on all four ranks); the
NVT launch runs the end-of-run rescale on the empty slabs.

Migration: face / seam crossings are counted from owner_of on the gathered positions AND from which handle holds the
particle (md_dom_download's ids per rank), which changes only at a list build; every multi-rank case must show at least
one of the latter, so migrate pack and unpack ran on a particle that the audit then followed.

What the audit found.  (1) A slab that owns no particle could not build its list: void failed in both launches at the first
build, "invalid configuration argument" -- rebuild_t launched the tile kernels with an empty grid.  The list build now skips
them (and md_scale_velocities its kernel) on such a slab.  (2) async-prune-nvt-3 lj_diam_long, segment 17 (one step,
thermo=False) missed (B): |dx|inf = 1.9e-4 against 2.8e-14 and |dv|inf = 4.5e-2 against 1.4e-11 with (A) clean -- the whole
velocity field rescaled once too often.  The segment before it had ended on a step redone through the classic violation
branch under NVT; that branch applies the step's Bussi scale with md_scale_velocities and left the window's scale word
holding the scale the violating drift had already consumed, which the next run's first kick-drift applied again.
DomainDevice._run_planned now clears it.  A single run() never sees this; a driver that calls run_async (or the classic
run_native) repeatedly under NVT did, whenever a call's last step violated.

Coverage is tuned, not assumed: tests/domain_audit_worker.py translates some systems along x so that their lattice
planes meet the seam and a face (XSHIFT), runs phs / phs_diam at kT = 6 with three ranks, and sets the inner skin to three
steps of the fastest particle (a prune every second step); INNER_STEPS and SKINS below list the cases that needed another
value -- among them blob under the ONES schedule, where a period of two locks onto the alternating thermo flag.

Run time, one session on one MI355X: this module 207 s (18 launches, the largest -- ten systems -- 25 s);
tests/test_domain_gpu.py at the parent commit 252 s.

Out of scope: the overlapped window (MDHIP_DOM_OVERLAP=1) needs slabs wide enough for interior tiles -- 110 592 particles in
tests/test_domain_gpu.py -- which is beyond a brute-force oracle; the fault-injection modes (MDHIP_DOM_FAIL) are not used.  Nothing was removed
after a fault or hang: none occurred.
"""
import json
import os
import re
import subprocess

import pytest

from tests import step_audit as sa
from tests.domain_audit_worker import launch
from tests.test_domain_gpu import _build_shim

pytestmark = pytest.mark.gpu

FIT2 = ["blob", "lj_diam_long", "ljmod0", "ljmod1", "ljmod2", "lj_2d", "poly_2d", "phs", "phs_diam", "poly_3d"]
FIT3 = FIT2                      # (phs: slabs of 3.33 >= 2 * 1.5; poly_3d: the skin is clipped to 0.23)
PAIR = ["blob", "lj_diam_long"]

# id -> (ranks, path, nvt, schedule, cases, extra environment)
LAUNCHES = {
    "sync-2": (2, "sync", 0, "MIXED", FIT2, {}),
    "sync-3": (3, "sync", 0, "MIXED", FIT3, {}),
    "sync-nvt-3": (3, "sync", 1, "MIXED", ["blob", "poly_2d"], {}),
    "async-prune-nvt-2": (2, "async-prune", 1, "MIXED", ["blob", "lj_diam_long", "lj_2d", "phs_diam"], {}),
    "async-prune-nvt-3": (3, "async-prune", 1, "MIXED", ["blob", "lj_diam_long", "lj_2d", "phs_diam"], {}),
    "native-prune-2": (2, "native-prune", 0, "MIXED", FIT2, {}),
    "native-prune-nvt-3": (3, "native-prune", 1, "MIXED", FIT3, {}),
    "native-prune-4": (4, "native-prune", 0, "MIXED", ["blob", "lj_2d"], {}),
    "native-prune-ones-2": (2, "native-prune", 0, "ONES", PAIR, {}),
    "native-prune-2/p2p_0": (2, "native-prune", 0, "MIXED", PAIR, {"MDHIP_DOM_P2P": "0"}),
    "native-prune-2/p2p_split": (2, "native-prune", 0, "MIXED", PAIR, {"MDHIP_DOM_P2P_SPLIT": "1"}),
    "native-prune-2/no_fused_step": (2, "native-prune", 0, "MIXED", PAIR, {"MDHIP_NO_FUSED_STEP": "1"}),
    "native-prune-2/no_tiles": (2, "native-prune", 0, "MIXED", PAIR, {"MDHIP_NO_TILES": "1"}),
    "native-prune-2/no_fused_build": (2, "native-prune", 0, "MIXED", PAIR, {"MDHIP_NO_FUSED_BUILD": "1"}),
    # one rank on the real RCCL: its own left and right neighbour
    "rccl-native-prune-1": (1, "native-prune", 1, "MIXED", ["blob", "lj_diam"], {}),
    # slabs that own no particle, in launches of their own
    "void-sync-4": (4, "sync", 0, "MIXED", ["void"], {}),
    "void-sync-nvt-4": (4, "sync", 1, "MIXED", ["void"], {}),      # the end-of-run rescale on a slab with nothing to rescale
    "void-native-prune-4": (4, "native-prune", 0, "MIXED", ["void"], {}),
}

# (launch, case) -> inner skin in steps of the fastest particle, where the default of three left a kind of step off the
# audited one-step segments (build_slab_case; which steps are prune steps is the planner's decision)
# ... and (launch, case) -> list skin: blob under the thermostat puts no prune step on a thermo=False one-step segment with
# 0.6 whatever the inner skin; 0.7 gives another rebuild interval and with it another phase
SKINS = {("native-prune-nvt-3", "blob"): 0.7, ("rccl-native-prune-1", "blob"): 0.7}
INNER_STEPS = {("native-prune-ones-2", "blob"): 5.0,      # (a period of 2 would lock onto the alternating thermo flag)
               ("async-prune-nvt-3", "phs_diam"): 5.0, ("native-prune-2", "poly_2d"): 12.0,
               ("native-prune-nvt-3", "poly_2d"): 5.0, ("native-prune-2/no_fused_step", "blob"): 6.0}


def _run_launch(tmp_path, lid):
    ranks, path, nvt, schedule, cases, extra = LAUNCHES[lid]
    rccl = lid.startswith("rccl")
    limit = 40 + 6 * len(cases)          # (measured: 5 s for one case, 20 to 26 s for ten)
    env = {"SLAB_CASES": ",".join(cases), "SLAB_PATH": path, "SLAB_NVT": str(nvt), "SLAB_SCHEDULE": schedule,
           "SLAB_OUT": str(tmp_path), "SLAB_WATCHDOG": str(limit - 10), "DOM_BACKEND": "nccl" if rccl else "gloo",
           "MDHIP_DOM_STAGE": "" if rccl else "device",
           "MDHIP_RCCL_PATH": _build_shim() if path.startswith("native") and not rccl else ""}
    env["SLAB_SKIN"] = ",".join("%s=%g" % (c, v) for (l, c), v in SKINS.items() if l == lid)
    env["SLAB_INNER_STEPS"] = ",".join("%s=%g" % (c, v) for (l, c), v in INNER_STEPS.items() if l == lid)
    if path.startswith("native"):
        env["MDHIP_DOM_P2P"] = "1"
    env.update(extra)
    try:
        rc, out, err = launch(ranks, env, 29800 + list(LAUNCHES).index(lid), limit)
    except subprocess.TimeoutExpired:
        pytest.exit("slab audit launch %s ran into its time limit of %d s: a hang -- nothing more is started" % (lid, limit), 3)
    if rc != 0 and re.search(r"exitcode\s*:\s*(-6|-11|134|139)\b|illegal memory access|Timeout \(\d", err):
        pytest.exit("slab audit launch %s faulted, aborted or hung -- nothing more is started:\n%s" % (lid, err[-3000:]), 3)
    assert rc == 0, "the worker failed:\n" + err[-3000:]
    res = {}
    for c in cases:
        with open(os.path.join(str(tmp_path), c + ".json")) as fh:
            res[c] = json.load(fh)
    return res


def _check(lid, name, r):
    """The assertions of one case of one launch; returns the list of what failed (so that a launch reports all its cases)."""
    ranks, path, nvt, schedule, cases, extra = LAUNCHES[lid]
    st, cov = r["stats"], sa.coverage(r)
    bad = []

    def need(ok, what):
        if not ok:
            bad.append("%s %s: %s" % (lid, name, what))

    need(r["failures"] == [], "audit failures: %s" % r["failures"][:4])
    need(len(r["excluded"]) <= sa.MAX_EXCLUDED and len(r["image_exceptions"]) <= sa.MAX_IMAGE_EXCEPTIONS, "caps")
    need(st["rebuilds"] >= 2, "rebuilds %d" % st["rebuilds"])
    void = name == "void"
    if void:
        # the crystallite lives on ranks 1 and 2 and vibrates across the face between them; nothing can reach the seam
        # within the schedule (the nearest particle is 7.6 away), and the outer slabs own no particle from start to end
        need(r["face_moves"] >= 1 and r["seam_moves"] == 0, "moves %d %d" % (r["face_moves"], r["seam_moves"]))
        need(r["face_migrations"] >= 1 and r["seam_migrations"] == 0, "migrations %d %d"
             % (r["face_migrations"], r["seam_migrations"]))
        need(r["owned_max"][0] == 0 and r["owned_max"][3] == 0 and r["n_own"][0] == 0 and r["n_own"][3] == 0,
             "the outer slabs did not stay empty: %s %s" % (r["owned_max"], r["n_own"]))
        need(sum(r["n_own"]) == r["n"], "n_own %s" % r["n_own"])
    else:
        need(r["seam_moves"] >= 1, "no particle crossed the seam")
        need(ranks == 1 or r["face_moves"] >= 1, "no particle changed owner across an interior face")
        # ... and the device followed: some particle changed HANDLE at a list build (migrate pack and unpack ran)
        need(ranks == 1 or r["face_migrations"] + r["seam_migrations"] >= 1, "no particle migrated between handles")
    pruning = path.endswith("prune") and "MDHIP_NO_TILES" not in extra
    if pruning:                       # (the prune count is the largest over the ranks: the leader's slab may be empty)
        need(st["prunes"] >= 3, "prunes %d" % st["prunes"])
        need(any(st["pruning"]), "inner rows in use on no rank: %s" % st["pruning"])
        for thermo in (True, False):
            need(cov.get(("prune", thermo), 0) >= 1, "no audited prune step with thermo=%s: %s" % (thermo, cov))
    else:
        need(st["prunes"] == 0 and not any(st["pruning"]), "prunes %d, inner rows %s" % (st["prunes"], st["pruning"]))
    for thermo in (True, False):
        need(cov.get(("ordinary", thermo), 0) >= 1, "no audited ordinary step with thermo=%s: %s" % (thermo, cov))
    need(sum(v for (kind, _), v in cov.items() if kind == "after_rebuild") >= 1, "no audited step after a rebuild: %s" % cov)
    if path.startswith("native"):
        classic = "MDHIP_NO_FUSED_STEP" in extra or "MDHIP_NO_TILES" in extra
        if classic:
            need(st["fused_windows"] == 0 and st["windows"] >= 1, "windows %s" % st)
        else:
            need(st["fused_windows"] == st["windows"] >= 1, "fused %d of %d windows" % (st["fused_windows"], st["windows"]))
        if classic or extra.get("MDHIP_DOM_P2P") == "0":
            need(st["direct_windows"] == 0, "direct windows %d" % st["direct_windows"])
        else:
            need(st["direct_windows"] == st["fused_windows"], "direct %d of %d fused windows"
                 % (st["direct_windows"], st["fused_windows"]))
    if schedule == "ONES":
        # one-step calls: a scheduled build (s < nsteps) cannot fire; every build after the first is a violation's
        need(st["violations"] >= 2, "violations %d" % st["violations"])
        need(all(s["rebuilds"] <= s["violations"] + (1 if i == 0 else 0) for i, s in enumerate(r["segments"])),
             "a build without a violation")
    return bad


@pytest.mark.parametrize("lid", list(LAUNCHES))
def test_slab_audit(tmp_path, lid):
    res = _run_launch(tmp_path, lid)
    bad = []
    for name, r in res.items():
        print(sa.margins_line("%s %s" % (lid, name), r))
        st = r["stats"]
        print("    kinds %s  stats %s  moves face %d seam %d  owned %s..%s  img exc %d" % (
            sorted(sa.coverage(r).items()), {k: st[k] for k in ("prunes", "pruning", "rebuilds", "violations", "windows",
                                                                "fused_windows", "direct_windows")},
            r["face_moves"], r["seam_moves"], r["owned_min"], r["owned_max"], len(r["image_exceptions"])))
        print("    migrations between handles: face %d seam %d" % (r["face_migrations"], r["seam_migrations"]))
        bad += _check(lid, name, r)
    assert not bad, "\n".join(bad)
