"""CPU tests of the cluster layer (analysis.ClusterAnalysis / compute_clusters, the binding, run_simulation's clusters=
keyword): the exports, the argument checks, the stop schedule, the file formats and the order of the device calls on a
recording fake handle, and the scipy reference of tests/cluster_reference.py -- which the GPU tests compare the device
against -- on hand-made graphs.  The device is tested in tests/test_gpu_clusters.py."""
import inspect
import os
import re
import types

import numpy as np
import pytest

import moleculardynamics.jl_amd as md
from moleculardynamics.jl_amd import BondOrder, ClusterAnalysis, _lib, analysis
from tests import cluster_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("md_cluster_setup", "md_cluster_sample", "md_cluster_particles", "md_cluster_read", "md_cluster_reset")
N, DIM = 8, 3


def test_exports():
    for name in ("ClusterAnalysis", "compute_clusters"):
        assert name in md.__all__ and getattr(md, name) is getattr(analysis, name)
    header = open(os.path.join(ROOT, "include", "mdhip.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert hasattr(_lib.load(), name)
        assert re.search(r"\bint\s+" + name + r"\s*\(", header)
    assert re.search(r"#define\s+MD_CLUSTER_ALL\s+0\b", header) and re.search(r"#define\s+MD_CLUSTER_SOLID\s+1\b", header)
    assert (_lib.MD_CLUSTER_ALL, _lib.MD_CLUSTER_SOLID) == (0, 1)
    assert "same step" in header and "has no meaning" in header        # the two sentences the contract asks for
    for name in ("cluster_setup", "cluster_sample", "cluster_particles", "cluster_read", "cluster_reset"):
        assert callable(getattr(md.MDDevice, name))
    mk = open(os.path.join(ROOT, "moleculardynamics", "jl_amd", "csrc", "Makefile")).read()
    assert re.search(r"^libmdhip\.so:.*\bmd_cluster\.hpp\b", mk, re.M)
    sig = inspect.signature(md.run_simulation)
    assert "clusters" in sig.parameters and sig.parameters["clusters"].default is None
    assert list(inspect.signature(md.compute_clusters).parameters) == ["state", "params", "r_bond", "members", "bond_order"]
    p = inspect.signature(ClusterAnalysis).parameters
    assert [(k, v.default) for k, v in p.items()] == [("r_bond", inspect.Parameter.empty), ("members", "all"), ("every", 1),
                                                      ("max_size", 1024), ("nseries", None)]


def test_the_union_uses_agent_scope_atomics_only():
    """The hooks have no plain access to parent[]: every one goes through the three helpers, and those are
    agent-scope relaxed atomics."""
    src = open(os.path.join(ROOT, "moleculardynamics", "jl_amd", "csrc", "md_cluster.hpp")).read()
    src = re.sub(r"//[^\n]*", "", src)                      # the code, not what the comments say about it
    body = src[src.index("__device__ __forceinline__ uint32_t cl_load"):src.index("cl_block_sum")]
    assert "parent[" not in body                            # only parent + x, handed to an atomic builtin
    assert body.count("__HIP_MEMORY_SCOPE_AGENT") == 3 and body.count("__ATOMIC_RELAXED") == 4
    hooks = src[src.index("struct ClLane"):src.index("k_cl_flatten")]
    assert "parent[" not in hooks and "cl_union(A.parent" in hooks and "visit(" in hooks and "end(" in hooks
    # the hooks run as a lane of the shared row walk, whose kernels know nothing of parent[]
    walk = open(os.path.join(ROOT, "moleculardynamics", "jl_amd", "csrc", "md_rowwalk.hpp")).read()
    assert "k_rows_tile" in walk and "k_rows(" in walk and "parent" not in re.sub(r"//[^\n]*", "", walk)


def test_argument_checks():
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="r_bond"):
            ClusterAnalysis(bad)
    for bad in ("liquid", 0, None):
        with pytest.raises(ValueError, match="members"):
            ClusterAnalysis(1.5, members=bad)
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError, match="every"):
            ClusterAnalysis(1.5, every=bad)
    for bad in (0, 65537, 2.5):
        with pytest.raises(ValueError, match="max_size"):
            ClusterAnalysis(1.5, max_size=bad)
    for bad in (-1, (1 << 20) + 1, 0.5):
        with pytest.raises(ValueError, match="nseries"):
            ClusterAnalysis(1.5, nseries=bad)
    ClusterAnalysis(1.5, members="solid", max_size=65536, nseries=1 << 20)
    ClusterAnalysis(1.5, max_size=1, nseries=0)
    cl = ClusterAnalysis(1.5)
    for call in (cl.mean_largest, cl.mean_clusters, cl.size_distribution, cl.weight_average_size):
        with pytest.raises(ValueError, match="no sample"):
            call()


def test_schedule():
    assert ClusterAnalysis(1.5).schedule(21, 5) == [0, 5, 10, 15, 20]
    assert ClusterAnalysis(1.5, every=2).schedule(21, 5) == [0, 10, 20]
    assert ClusterAnalysis(1.5, every=2).schedule(20, 5) == [0, 10]
    assert ClusterAnalysis(1.5, every=3).schedule(0, 5) == []


def test_means_and_distribution():
    cl = ClusterAnalysis(1.5, max_size=4)
    fr = np.array([20, 6, 8, 4, 40, 100, 3, 2])
    cl._accumulate(2, 2 * fr, [0, 4, 2, 0, 6], np.stack([fr, fr]), [0, 10])
    assert cl.nsamples == 2 and cl.sum_fr.dtype == np.int64
    assert cl.mean_largest() == 8.0 and cl.mean_clusters() == 6.0 and cl.weight_average_size() == 5.0
    s, ns = cl.size_distribution()
    assert list(s) == [0, 1, 2, 3, 4] and list(ns) == [0.0, 2.0, 1.0, 0.0, 3.0]
    steps, frames = cl.series()
    assert list(steps) == [0, 10] and frames.dtype == np.int64 and np.array_equal(frames[1], fr)
    cl.reset()
    assert cl.nsamples == 0 and not cl.hist_size.any() and cl.series()[1].shape == (0, 8)


class _FakeDevice:
    """Records the segment lengths and an ordered trace of (last completed step, method); reads back a fixed answer."""

    FR = np.array([8, 3, 5, 2, 10, 30, 0, 1], dtype=np.int64)

    def __init__(self):
        self.n, self.dim = N, DIM
        self.step = 0
        self.segments, self.trace, self.setups = [], [], []
        self.cluster_args = None

    def set_potential(self, kind, params):
        pass

    def upload(self, **kw):
        pass

    def run(self, nsteps, dt, *a, **kw):
        self.segments.append(nsteps)
        self.step += nsteps
        return 0.0, 0.0, 1.0

    def download(self):
        z = np.zeros((N, DIM))
        return z, z, z, np.zeros((N, DIM), dtype=np.int32)

    def snapshot_begin(self):
        pass

    def snapshot_end(self):
        return np.zeros((N, DIM)), np.zeros((N, DIM), dtype=np.int32)

    def boo_setup(self, r_neigh, order=6, nbins=100, threshold=0.7, min_conn=7, nseries=0):
        self.setups.append("boo_setup")
        self.boo_args = (nbins, nseries)

    def boo_sample(self):
        self.trace.append((self.step - 1, "boo_sample"))

    def boo_read(self):
        nbins, nseries = self.boo_args
        ns = sum(1 for _, m in self.trace if m == "boo_sample")
        z = np.zeros(nbins, dtype=np.int64)
        return ns, np.zeros(8), z, z, np.zeros(33, dtype=np.int64), np.zeros(33, dtype=np.int64), np.zeros((min(ns, nseries), 8))

    def cluster_setup(self, r_bond, members=0, max_size=1024, nseries=0):
        self.setups.append("cluster_setup")
        self.cluster_args = (r_bond, members, max_size, nseries)

    def cluster_sample(self):
        self.trace.append((self.step - 1, "cluster_sample"))

    def cluster_read(self):
        _, _, max_size, nseries = self.cluster_args
        ns = sum(1 for _, m in self.trace if m == "cluster_sample")
        hist = np.zeros(max_size + 1, dtype=np.int64)
        hist[1], hist[2], hist[max_size] = ns, ns, ns
        return ns, self.FR * ns, hist, np.tile(self.FR, (min(ns, nseries), 1))


def _fake_state():
    dev = _FakeDevice()
    system = types.SimpleNamespace(device=dev, positions=np.zeros((N, DIM)), xpositions=None,
                                   energy_and_forces=types.SimpleNamespace(forces=np.zeros((N, DIM)), energy=0.0,
                                                                           virial=0.0))
    state = md.SimulationState(system, np.ones(N), np.random.default_rng(1), np.diag([2.0, 2.0, 2.0]),
                               np.zeros((N, DIM)), np.zeros((N, DIM), dtype=np.int32), DIM, DIM * (N - 1.0))
    return state, dev


PARAMS = md.Parameters(1.0, N, 0.002, md.LennardJones())


@pytest.mark.parametrize("every,freq,total", [(1, 5, 21), (2, 5, 21), (3, 4, 9), (1, 7, 1)])
def test_samples_at_every_nth_output_step(tmp_path, every, freq, total):
    state, dev = _fake_state()
    cl = ClusterAnalysis(1.2, every=every, max_size=4)
    md.run_simulation(state, PARAMS, md.NVE(), total, freq, str(tmp_path), write_trajectory=False, clusters=cl)
    want = [s for s in range(0, total, freq) if (s // freq) % every == 0]
    assert [s for s, _ in dev.trace] == want == cl.schedule(total, freq)
    # the sampler adds no stop of its own: the loop stops at the output steps and at the last step
    assert list(np.cumsum(dev.segments) - 1) == sorted(set(range(0, total, freq)) | {total - 1})
    assert dev.cluster_args == (1.2, 0, 4, len(want))       # by default one series row per sample of the run
    assert cl.nsamples == len(want) and list(cl.steps) == want


def test_file_formats(tmp_path):
    state, dev = _fake_state()
    cl = ClusterAnalysis(1.35, max_size=3)
    out = str(tmp_path)
    md.run_simulation(state, PARAMS, md.NVE(), 11, 5, out, write_trajectory=False, clusters=cl)
    assert set(os.listdir(out)) == {"thermo.txt", "final.xyz", "clusters.txt", "clusters_series.txt"}
    lines = open(os.path.join(out, "clusters.txt")).read().splitlines()
    assert lines[0] == "# members all r_bond 1.350000 max_size 3 nsamples 3"
    assert lines[1] == "# mean_members 8.000000 mean_clusters 3.000000 mean_largest 5.000000 weight_average_size 3.750000"
    assert lines[2] == "# s n(s)"
    assert lines[3:] == ["1 1.000000e+00", "2 1.000000e+00", "3 1.000000e+00"]
    lines = open(os.path.join(out, "clusters_series.txt")).read().splitlines()
    assert lines[0] == ("# step members clusters largest second_largest directed_bonds sum_size2 largest_label "
                        "singletons")
    assert lines[1:] == ["%d 8 3 5 2 10 30 0 1" % s for s in (0, 5, 10)]
    # a second run accumulates in the object; nseries caps the recorded rows, not the sums
    cl2 = ClusterAnalysis(1.35, max_size=3, nseries=2)
    state, dev = _fake_state()
    md.run_simulation(state, PARAMS, md.NVE(), 11, 5, out, write_trajectory=False, clusters=cl2)
    assert dev.cluster_args[-1] == 2 and cl2.nsamples == 3 and list(cl2.steps) == [0, 5]
    state, dev = _fake_state()
    md.run_simulation(state, PARAMS, md.NVE(), 6, 5, out, write_trajectory=False, clusters=cl2)
    assert cl2.nsamples == 5 and list(cl2.steps) == [0, 5, 0, 5] and cl2.mean_largest() == 5.0


def test_solid_mode_needs_the_bond_order_sampler(tmp_path):
    state, dev = _fake_state()
    out = str(tmp_path / "refused")
    with pytest.raises(ValueError, match="bond_order"):
        md.run_simulation(state, PARAMS, md.NVE(), 11, 5, out, clusters=ClusterAnalysis(1.2, members="solid"))
    with pytest.raises(ValueError, match="multiple of bond_order.every"):
        md.run_simulation(state, PARAMS, md.NVE(), 11, 5, out, clusters=ClusterAnalysis(1.2, members="solid", every=3),
                          bond_order=BondOrder(1.5, every=2))
    assert dev.setups == [] and dev.segments == [] and not os.path.exists(out)      # refused before anything was done
    with pytest.raises(ValueError, match="bond_order"):
        md.compute_clusters(state, PARAMS, 1.2, members="solid")


def test_bond_order_acts_before_clusters_at_a_shared_step(tmp_path):
    state, dev = _fake_state()
    cl = ClusterAnalysis(1.2, members="solid", every=2, max_size=4)
    bo = BondOrder(1.5, nbins=4)
    md.run_simulation(state, PARAMS, md.NVE(), 21, 5, str(tmp_path), write_trajectory=False, clusters=cl, bond_order=bo)
    assert dev.setups == ["boo_setup", "cluster_setup"] and dev.cluster_args[1] == 1
    want = []
    for s in range(0, 21, 5):
        want.append((s, "boo_sample"))
        if (s // 5) % 2 == 0:
            want.append((s, "cluster_sample"))
    assert dev.trace == want


# ---------------------------------------------------------------------------------------------------------------------
# The reference on hand-made graphs

def test_reference_path_and_isolated_points():
    # ids 5-2-7-0 form a path, 1, 3, 4, 6 are isolated
    r = ref.clusters(8, [[5, 2], [7, 2], [0, 7]], max_size=3)
    assert r["label"].tolist() == [0, 1, 0, 3, 4, 0, 6, 0]
    assert r["size"].tolist() == [4, 1, 4, 1, 1, 4, 1, 4]
    assert r["fr"].tolist() == [8, 5, 4, 1, 6, 4 * 4 + 4, 0, 4]
    assert r["hist"].tolist() == [0, 4, 0, 1]               # the path of 4 lands in the overflow entry 3


def test_reference_two_triangles_tie_for_the_largest():
    pairs = [[1, 4], [4, 6], [6, 1], [2, 3], [3, 5], [5, 2]]
    r = ref.clusters(8, pairs)
    assert r["label"].tolist() == [0, 1, 2, 2, 1, 2, 1, 7]
    assert r["fr"].tolist() == [8, 4, 3, 3, 12, 9 + 9 + 1 + 1, 1, 2]    # second = largest on a tie, the smaller label wins
    assert r["hist"][:4].tolist() == [0, 2, 0, 2] and r["hist"].sum() == 4 and len(r["hist"]) == 1025


def test_reference_members_restrict_the_graph():
    # the path 0-1-2-3 with 2 not a member falls into {0, 1} and {3}; the pair (1, 2) is no bond
    member = np.array([True, True, False, True, False])
    r = ref.clusters(5, [[0, 1], [1, 2], [2, 3]], member=member)
    assert r["label"].tolist() == [0, 0, -1, 3, -1] and r["size"].tolist() == [2, 2, 0, 1, 0]
    assert r["fr"].tolist() == [3, 2, 2, 1, 2, 5, 0, 1]
    none = ref.clusters(3, [[0, 1]], member=np.zeros(3, dtype=bool))
    assert none["fr"].tolist() == [0, 0, 0, 0, 0, 0, -1, 0] and not none["hist"].any()
    one = ref.clusters(3, [[0, 1], [1, 2]])
    assert one["fr"].tolist() == [3, 1, 3, 0, 4, 9, 0, 0]   # one cluster: the second-largest is 0
