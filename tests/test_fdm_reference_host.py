"""`tests/fdm_reference.py` against second formulations, so that the GPU
tests of the Schwarz kernels (`tests/test_gpu_schwarz_kernels.py`) can trust
it: the dense Kronecker product per element, the production code's own torch
route on CPU tensors, and plain loops for the small helpers.  No GPU."""
import numpy as np
import pytest
import torch

from swirl_fem_amd.navier_stokes import pressure_preconditioner as pc
from tests import fdm_reference as R


def _inputs(ndim, Pp, E=5, C=4, seed=0, permuted=True):
  rng = np.random.default_rng(seed + 100 * ndim + Pp)
  n = Pp ** ndim
  S = np.eye(Pp) + rng.standard_normal((C, Pp, Pp)) / np.sqrt(Pp)
  cases = rng.integers(0, C, (ndim, E))
  w = rng.uniform(0.5, 1.5, (E,) + (Pp,) * ndim)
  pel = (rng.permutation(E * n) if permuted else np.arange(E * n)).reshape(E, n)
  r = rng.standard_normal(E * n)
  return r, pel, S, cases, w


@pytest.mark.parametrize('ndim', [1, 2, 3])
@pytest.mark.parametrize('Pp', [1, 2, 3, 4])
def test_reference_is_the_kronecker_product(ndim, Pp):
  """z_e = K diag(w_e) K^T r_e with K = S_0 (x) .. (x) S_{d-1}: `np.kron` puts
  its LAST factor on the fastest index, the convention of the header."""
  r, pel, S, cases, w = _inputs(ndim, Pp)
  z = R.fdm_solve(r, pel, S, cases, w, ndim, Pp)
  E = cases.shape[1]
  for e in range(E):
    K = np.ones((1, 1))
    for a in range(ndim):
      K = np.kron(K, S[cases[a, e]])
    want = K @ (w[e].reshape(-1) * (K.T @ r[pel[e]]))
    assert np.abs(z[pel[e]] - want).max() <= 1e-13 * np.abs(want).max()
  # pel=None is arange
  z0 = R.fdm_solve(r, None, S, cases, w, ndim, Pp)
  ident = np.arange(r.size).reshape(pel.shape)
  assert np.array_equal(z0, R.fdm_solve(r, ident, S, cases, w, ndim, Pp))


@pytest.mark.parametrize('ndim,Pp', [(1, 3), (2, 2), (2, 5), (3, 3), (3, 4)])
def test_reference_is_local_solve_torch(ndim, Pp):
  """The production convention: `SchwarzPressurePreconditioner.
  local_solve_torch` on hand-made S, case and inv_ev (CPU tensors, a bare
  object: no StokesSEM)."""
  r, pel, S, cases, w = _inputs(ndim, Pp, seed=1)
  M = object.__new__(pc.SchwarzPressurePreconditioner)
  M.d, M.Pp = ndim, Pp
  M.pel = torch.as_tensor(pel)
  M.S = torch.as_tensor(S)
  M.case = [torch.as_tensor(c) for c in cases]
  M.inv_ev = torch.as_tensor(w)
  got = M.local_solve_torch(torch.as_tensor(r)).numpy()
  want = R.fdm_solve(r, pel, S, cases, w, ndim, Pp)
  assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()


def test_reference_float32_is_float32():
  """`dtype=np.float32` keeps every intermediate in single precision (the
  result is float32 and differs from the float64 one at the 1e-7 level, not
  at 1e-16)."""
  r, pel, S, cases, w = _inputs(3, 4, seed=2)
  f = lambda x: np.asarray(x, np.float32).astype(np.float64)
  r, S, w = f(r), f(S), f(w)
  z64 = R.fdm_solve(r, pel, S, cases, w, 3, 4)
  z32 = R.fdm_solve(r, pel, S, cases, w, 3, 4, dtype=np.float32)
  assert z32.dtype == np.float32
  err = np.abs(z32 - z64).max() / np.abs(z64).max()
  assert 1e-9 < err < 2e-6, err


def test_sums_and_constants_against_loops():
  r, pel, S, cases, w = _inputs(2, 3, E=6, seed=3)
  rng = np.random.default_rng(4)
  z = rng.standard_normal(r.size)
  weights = rng.uniform(0.5, 1.5, r.size)
  es, ws = R.fdm_sums(r, z, pel, weights)
  for e in range(6):
    assert abs(es[e] - sum(r[i] for i in pel[e])) < 1e-13
    assert abs(ws[e] - sum(weights[i] * z[i] for i in pel[e])) < 1e-13
  yc, shift = rng.standard_normal(6), rng.standard_normal(3)
  out = R.add_element_constants(z, yc, shift, 9, 2)
  for e in range(6):
    for i in range(9):
      assert out[e * 9 + i] == z[e * 9 + i] + (yc[e] - shift[e // 2])


def test_ell_storage_and_chebyshev_precisions():
  """`ell_from_csr` holds the matrix (padding: column 0, value 0), and the
  float32 evaluation of the polynomial is a float32 one."""
  import scipy.sparse as sp
  from tests import pmg_reference
  rng = np.random.default_rng(5)
  n = 23
  A = sp.random(n, n, density=0.2, random_state=1, format='csr')
  A = (A + A.T + sp.diags(np.full(n, 4.0))).tocsr()
  cols, vals = R.ell_from_csr(A)
  assert cols.dtype == np.int32 and cols.shape == vals.shape
  assert cols.shape == (int(np.diff(A.indptr).max()), n)
  x = rng.standard_normal(n)
  assert np.abs((vals * x[cols]).sum(0) - A @ x).max() < 1e-13
  pad = vals == 0
  assert pad.any() and not cols[pad].any()
  dinv = 1.0 / A.diagonal()
  b = rng.standard_normal(n)
  x64 = R.ell_chebyshev(A, dinv, b, 5, 0.3, 1.7)
  assert np.array_equal(x64, pmg_reference.coarse_chebyshev(A, dinv, b, 5,
                                                            0.3, 1.7))
  x32 = R.ell_chebyshev(A, dinv, b, 5, 0.3, 1.7, dtype=np.float32)
  assert x32.dtype == np.float32
  err = np.abs(x32 - x64).max() / np.abs(x64).max()
  assert 1e-9 < err < 1e-5, err
