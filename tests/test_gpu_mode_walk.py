"""-m gpu: the three wave-vector samplers (md_sq_*, md_chi4_*, md_cur_*) share one particle walk and one partial tree
(mode_walk and sq_row_sum in md_sq.hpp), as their headers say.

One handle carries sq, chi4 and cur on the same integer vectors.  With velocities that are exactly (1, 0, -2) for every
particle the three sums have known relations that hold bit for bit only if phase, term and tree are the same operation for
operation: fma(1, c, acc) is acc + c, so the first axis of j is rho; fma(0, c, 0) is 0; a scaling by -2, a power of two,
commutes with every rounding of the tree, so the last axis of j is -2 rho.  With a threshold larger than the cell every
particle is slow against its own frame, so the masked walk over an all-ones mask must return rho as well.  Sizes: N = 63 (less
than a wave) and 4161 (two particle blocks, a tail that is no multiple of 64); nvec = 1 (one padded tile), 5 (a second cur
tile holding one real vector) and 9 (a second sq tile holding one real vector).  No tolerance anywhere."""
import numpy as np
import pytest

from tests import cur_reference as ref
from tests.test_gpu_currents import CELLS, _handle, _points

pytestmark = pytest.mark.gpu
VECTORS = np.array([[3, -1, 2], [0, 5, 0], [-7, 1, 1], [1, 1, 1], [2, 0, -9], [4, 4, -3], [-1, 6, 0], [5, -2, 7], [1, 0, 0]],
                   dtype=np.int32)                              # (the first two components are never both zero: 2-D)
VELOCITY = {3: (1.0, 0.0, -2.0), 2: (1.0, -2.0)}


def _floats(z):
    return np.ascontiguousarray(z).view(np.float64)


@pytest.mark.parametrize("N", [63, 4161])
@pytest.mark.parametrize("cell", ["sheared", "2d"])
def test_sq_chi4_and_cur_share_one_walk_and_tree(cell, N):
    U = CELLS[cell]
    d = U.shape[0]
    x = _points(U, N, 31 + N)
    v = np.tile(np.array(VELOCITY[d]), (N, 1))
    with _handle(U, x, v) as dev:
        assert np.array_equal(dev.download()[1], v)
        for nvec in (1, 5, 9):
            n = np.ascontiguousarray(VECTORS[:nvec, :d])
            dev.sq_setup(n)
            dev.cur_setup(n, ref.directions(U, n))
            dev.chi4_setup(4.0 * np.abs(U).sum(), n, 1, 1)      # a larger than the cell: every particle is slow
            dev.sq_sample()
            dev.cur_sample()
            dev.chi4_origin(0)
            dev.chi4_sample([0], [0])
            rho, j = dev.sq_rho(), dev.cur_last()
            Q, W, slow = dev.chi4_last()
            tag = f"{cell} N {N} nvec {nvec}"
            assert rho.shape == (nvec,) and j.shape == (nvec, d) and W.shape == (nvec,), tag
            assert np.abs(rho).max() > 0.0, tag                 # (not all zeros)
            assert np.array_equal(_floats(j[:, 0]), _floats(rho)), tag
            assert np.array_equal(_floats(j[:, d - 1]), -2.0 * _floats(rho)), tag
            if d == 3:
                assert np.array_equal(_floats(j[:, 1]), np.zeros(2 * nvec)), tag
            assert Q == N and np.array_equal(slow, np.ones(N, np.uint8)), tag
            assert np.array_equal(_floats(W), _floats(rho)), tag
