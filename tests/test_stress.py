"""CPU tests of the stress layer (analysis.StressTensor / compute_stress, the binding, run_simulation's stress= keyword):
the tensor assembly, the channel averaging, the <p>^2 subtraction, the trapezoid viscosity, the stop schedule merged into
the loop's output steps, the file formats and the argument checks.  The device sums are tested in
tests/test_gpu_stress.py."""
import inspect
import math
import os
import re
import types

import numpy as np
import pytest

import moleculardynamics.jl_amd as md
from moleculardynamics.jl_amd import StressTensor, _lib, analysis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("md_stress_setup", "md_stress_sample", "md_stress_tensor", "md_stress_read", "md_stress_reset")


def test_exports():
    for name in ("StressTensor", "compute_stress"):
        assert name in md.__all__ and getattr(md, name) is getattr(analysis, name)
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert hasattr(_lib.load(), name)
    header = open(os.path.join(ROOT, "include", "mdhip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header)
    assert "xx, yy, zz, xy, xz, yz" in header and "ring[m % nlags]" in header      # the orders are stated
    for name in ("stress_setup", "stress_sample", "stress_tensor", "stress_read", "stress_reset"):
        assert callable(getattr(md.MDDevice, name))
    mk = open(os.path.join(ROOT, "moleculardynamics", "jl_amd", "csrc", "Makefile")).read()
    assert re.search(r"^libmdhip\.so:.*\bmd_stress\.hpp\b", mk, re.M)
    sig = inspect.signature(md.run_simulation)
    assert "stress" in sig.parameters and sig.parameters["stress"].default is None
    assert list(inspect.signature(md.compute_stress).parameters) == ["state", "params"]


def test_argument_checks():
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="every"):
            StressTensor(bad)
    for bad in (-1, 65537, 2.5):
        with pytest.raises(ValueError, match="nlags"):
            StressTensor(1, nlags=bad)
    StressTensor(1, nlags=0)
    StressTensor(7, nlags=65536)
    st = StressTensor(2, nlags=3)
    for call in (st.kinetic, st.virial, st.pressure_tensor, st.pressure, st.temperature, st.acf, st.viscosity):
        with pytest.raises(ValueError, match="no sample"):
            call()
    st0 = StressTensor(2)
    st0._accumulate(1, np.ones(6), np.ones(6), np.zeros(0), np.zeros((0, 6)), 10, np.eye(3), 0.1)
    with pytest.raises(ValueError, match="nlags = 0"):
        st0.acf()
    with pytest.raises(ValueError, match="dimension"):
        st0._accumulate(1, np.ones(3), np.ones(3), np.zeros(0), np.zeros((0, 3)), 10, np.eye(2), 0.1)
    with pytest.raises(ValueError, match="components"):
        StressTensor(1)._accumulate(1, np.ones(3), np.ones(3), np.zeros(0), np.zeros((0, 3)), 10, np.eye(3), 0.1)


def test_schedule():
    assert StressTensor(5).schedule(21) == [0, 5, 10, 15, 20]
    assert StressTensor(5).schedule(20) == [0, 5, 10, 15]
    assert StressTensor(1).schedule(3) == [0, 1, 2]
    assert StressTensor(9).schedule(0) == []


def test_tensor_assembly_3d():
    st = StressTensor(1)
    U = np.diag([2.0, 3.0, 4.0])
    kin = np.array([1.0, 2.0, 3.0, 0.1, 0.2, 0.3])
    vir = np.array([10.0, 20.0, 30.0, 1.0, 2.0, 3.0])
    st._accumulate(2, 2 * kin, 2 * vir, np.zeros(0), np.zeros((0, 6)), 11, U, 0.01)
    st._accumulate(1, kin, vir, np.zeros(0), np.zeros((0, 6)), 11, U, 0.01)          # accumulates across calls
    assert st.nsamples == 3
    K = np.array([[1.0, 0.1, 0.2], [0.1, 2.0, 0.3], [0.2, 0.3, 3.0]])
    W = np.array([[10.0, 1.0, 2.0], [1.0, 20.0, 3.0], [2.0, 3.0, 30.0]])
    assert np.allclose(st.kinetic(), K, rtol=1e-15) and np.allclose(st.virial(), W, rtol=1e-15)
    assert np.allclose(st.pressure_tensor(), (K + W) / 24.0, rtol=1e-15)
    assert st.pressure() == pytest.approx((6.0 + 60.0) / 24.0 / 3.0, rel=1e-15)
    assert st.temperature() == pytest.approx(6.0 / (3 * 10.0), rel=1e-15)
    assert "pressure_lrc" in StressTensor.pressure.__doc__
    st.reset()
    assert st.nsamples == 0 and st.sum_kin is None


def test_tensor_assembly_2d():
    st = StressTensor(1)
    st._accumulate(1, [1.0, 2.0, 0.5], [3.0, 4.0, -0.5], np.zeros(0), np.zeros((0, 3)), 5, np.diag([2.0, 5.0]), 0.01)
    assert np.array_equal(st.kinetic(), [[1.0, 0.5], [0.5, 2.0]])
    assert np.array_equal(st.virial(), [[3.0, -0.5], [-0.5, 4.0]])
    assert st.pressure() == pytest.approx(10.0 / 10.0 / 2.0)
    assert st.temperature() == pytest.approx(3.0 / (2 * 4.0))
    assert st.shear_channels() == [0, 1]


def _synthetic(nlags=50, every=4, dt=0.005, tau=0.1, amp=(3.0, 5.0, 7.0, 9.0, 11.0), pbar=2.5, ppvar=0.75):
    """Sums of a made-up process: shear channel c has C_c(t) = amp_c exp(-t / tau), the pressure channel has mean pbar
    and C_pp(t) = ppvar exp(-t / tau); lag k has (M - k) products."""
    st = StressTensor(every, nlags=nlags)
    M = 1000
    n, U = 101, np.diag([3.0, 4.0, 5.0])
    t = np.arange(nlags) * every * dt
    ncorr = M - np.arange(nlags)
    c = np.empty((nlags, 6))
    for ch in range(5):
        c[:, ch] = amp[ch] * np.exp(-t / tau)
    c[:, 5] = ppvar * np.exp(-t / tau) + pbar * pbar
    # <p-channel> = tr(sum_kin + sum_vir) / (d M) = pbar
    sk = np.array([0.5, 0.25, 0.25, 0.0, 0.0, 0.0]) * M * 3 * pbar * 0.4
    sv = np.array([0.25, 0.5, 0.25, 0.0, 0.0, 0.0]) * M * 3 * pbar * 0.6
    st._accumulate(M, sk, sv, ncorr, c * ncorr[:, None], n, U, dt)
    return st, t, amp, tau, pbar, ppvar


def test_acf_channel_average_and_pressure_subtraction():
    st, t, amp, tau, pbar, ppvar = _synthetic()
    tt, c, cs = st.acf()
    assert np.array_equal(tt, t) and c.shape == (50, 6)
    for ch in range(5):
        assert np.allclose(c[:, ch], amp[ch] * np.exp(-t / tau), rtol=1e-13)
    assert np.allclose(cs, np.mean(amp) * np.exp(-t / tau), rtol=1e-13)
    assert np.allclose(c[:, 5], ppvar * np.exp(-t / tau), rtol=0, atol=1e-13 * pbar * pbar)
    # a lag without a product is nan, not a division error
    st2 = StressTensor(1, nlags=3)
    st2._accumulate(2, np.ones(6), np.ones(6), [2, 1, 0], np.ones((3, 6)), 10, np.eye(3), 0.1)
    assert np.isnan(st2.acf()[1][2]).all() and np.isfinite(st2.acf()[1][:2]).all()


def test_trapezoid_viscosity_of_an_exponential():
    st, t, amp, tau, _, _ = _synthetic()
    kT = 0.8
    tt, eta = st.viscosity(kT=kT)
    a, V = np.mean(amp), 60.0
    h = t[1] - t[0]
    # the trapezoid rule on a geometric sequence, in closed form
    q = math.exp(-h / tau)
    expect = a * h * 0.5 * (1.0 + q) * (1.0 - q ** np.arange(50)) / (1.0 - q) / (V * kT)
    assert eta[0] == 0.0 and np.allclose(eta, expect, rtol=1e-12)
    # and close to the analytic integral a tau (1 - exp(-t / tau)) / (V kT): trapezoid error h^2 / (12 tau^2)
    exact = a * tau * (1.0 - np.exp(-t / tau)) / (V * kT)
    assert np.allclose(eta[1:], exact[1:], rtol=1.01 * h * h / (12.0 * tau * tau))
    # kT defaults to temperature()
    _, eta_t = st.viscosity()
    assert np.allclose(eta_t * st.temperature(), eta * kT, rtol=1e-14)


def test_file_formats(tmp_path):
    st, t, *_ = _synthetic(nlags=6)
    p = str(tmp_path / "stress.txt")
    st.write(p)
    lines = open(p).read().splitlines()
    assert lines[0] == "# component kinetic virial pressure" and lines[-1] == "# nsamples 1000" and len(lines) == 8
    assert [ln.split()[0] for ln in lines[1:7]] == ["xx", "yy", "zz", "xy", "xz", "yz"]
    k, w = st.sum_kin / 1000, st.sum_vir / 1000
    assert lines[1] == "xx %.10e %.10e %.10e" % (k[0], w[0], (k[0] + w[0]) / 60.0)
    st.ncorr[5] = 0                                    # a lag that has no product is left out
    p = str(tmp_path / "stress_acf.txt")
    st.write_acf(p)
    lines = open(p).read().splitlines()
    assert lines[0] == "# lag time C_shear C_ch0 C_ch1 C_ch2 C_ch3 C_ch4 C_pp eta_running ncorr"
    assert len(lines) == 6
    _, c, cs = st.acf()
    _, eta = st.viscosity()
    row = lines[3].split()
    assert len(row) == 11 and row[0] == "2" and row[1] == "%.6e" % t[2] and row[2] == "%.6e" % cs[2]
    assert row[3:9] == ["%.6e" % v for v in c[2]] and row[9] == "%.6e" % eta[2] and row[10] == "998"


class _FakeDevice:
    """Records what run_simulation asks of the handle: the segment lengths and the steps a sample is taken after."""

    def __init__(self, n, dim):
        self.n, self.dim = n, dim
        self.step = 0
        self.segments, self.samples, self.setup = [], [], None

    def set_potential(self, kind, params):
        pass

    def upload(self, **kw):
        pass

    def run(self, nsteps, dt, *a, **kw):
        self.segments.append(nsteps)
        self.step += nsteps
        return 0.0, 0.0, 1.0

    def download(self):
        z = np.zeros((self.n, self.dim))
        return z, z, z, np.zeros((self.n, self.dim), dtype=np.int32)

    def stress_setup(self, nlags):
        self.setup = nlags

    def stress_sample(self):
        self.samples.append(self.step - 1)              # the last completed step

    def stress_read(self):
        ns = len(self.samples)
        nl = self.setup
        return ns, np.full(6, 3.0 * ns), np.full(6, 6.0 * ns), np.maximum(ns - np.arange(nl), 0), np.ones((nl, 6))


def _fake_state(n=8):
    dev = _FakeDevice(n, 3)
    system = types.SimpleNamespace(device=dev, positions=np.zeros((n, 3)), xpositions=None,
                                   energy_and_forces=types.SimpleNamespace(forces=np.zeros((n, 3)), energy=0.0, virial=0.0))
    state = md.SimulationState(system, np.ones(n), np.random.default_rng(1), np.diag([2.0, 2.0, 2.0]),
                               np.zeros((n, 3)), np.zeros((n, 3), dtype=np.int32), 3, 3 * (n - 1.0))
    return state, dev


@pytest.mark.parametrize("every,freq,total", [(4, 10, 23), (10, 10, 31), (3, 7, 7), (25, 10, 20)])
def test_stops_are_merged_into_the_output_steps(tmp_path, every, freq, total):
    state, dev = _fake_state()
    params = md.Parameters(1.0, 8, 0.002, md.LennardJones())
    st = StressTensor(every, nlags=2)
    md.run_simulation(state, params, md.NVE(), total, freq, str(tmp_path), write_trajectory=False, stress=st)
    stops = sorted(set(range(0, total, freq)) | set(range(0, total, every)) | {total - 1})
    ends = list(np.cumsum(dev.segments) - 1)
    assert ends == stops                                # every output step and every stress stop ends a segment
    assert dev.samples == list(range(0, total, every)) and dev.setup == 2
    assert st.nsamples == len(dev.samples)
    thermo = open(os.path.join(str(tmp_path), "thermo.txt")).read().splitlines()
    assert [int(ln.split()[0]) for ln in thermo[1:]] == list(range(0, total, freq))
    assert os.path.exists(os.path.join(str(tmp_path), "stress.txt"))
    assert os.path.exists(os.path.join(str(tmp_path), "stress_acf.txt"))
    # without the keyword the loop stops at the output steps only
    state2, dev2 = _fake_state()
    md.run_simulation(state2, params, md.NVE(), total, freq, str(tmp_path / "b"), write_trajectory=False)
    assert list(np.cumsum(dev2.segments) - 1) == sorted(set(range(0, total, freq)) | {total - 1})
    assert not os.path.exists(os.path.join(str(tmp_path / "b"), "stress.txt"))


def test_brownian_is_refused(tmp_path):
    state, _ = _fake_state()
    params = md.Parameters(1.0, 8, 0.002, md.LennardJones())
    with pytest.raises(ValueError, match="Brownian"):
        md.run_simulation(state, params, md.Brownian(1.0), 5, 1, str(tmp_path), write_trajectory=False,
                          stress=StressTensor(1))
