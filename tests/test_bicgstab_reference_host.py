"""Host checks of the piecewise BiCGStab restatement
(`tests/bicgstab_reference.py`: `update_p`, `update_s`, `update_xr`,
`scalar_phase`) that `tests/test_gpu_bicgstab_kernels.py` compares the device
kernels with: an iteration loop composed of the pieces is `bicgstab` itself,
iterate for iterate."""
import numpy as np
import pytest

from tests import bicgstab_reference as BS


def _dense_system(n=200, seed=7):
  """The system of `test_gpu_advection._dense_system`."""
  rng = np.random.default_rng(seed)
  A = 0.5 * rng.standard_normal((n, n)) / np.sqrt(n)
  A += np.diag(1.0 + rng.random(n))
  return A, rng.standard_normal(n)


def _same(A, b, dinv=None, **kw):
  M = None if dinv is None else (lambda v: dinv * v)
  x, its, status = BS.bicgstab(A, b, M=M, **kw)
  y, jts, jstatus, count = BS.bicgstab_by_pieces(A, b, dinv=dinv, **kw)
  assert jstatus == status
  assert len(jts) == len(its) and count == len(its)
  for a, c in zip(its, jts):
    assert np.array_equal(a, c)
  assert np.array_equal(x, y)
  return its, status


@pytest.mark.parametrize('precond', [False, True])
def test_pieces_reproduce_bicgstab_on_the_dense_system(precond):
  A, b = _dense_system()
  dinv = 1.0 / np.diag(A) if precond else None
  op = lambda v: A @ v
  its, status = _same(op, b, dinv, tol=1e-13)
  assert status == 'converged' and len(its) > 5
  its, status = _same(op, b, dinv, tol=1e-30, maxiter=10)
  assert status == 'maxiter' and len(its) == 10
  x0 = np.random.default_rng(1).standard_normal(len(b))
  its, status = _same(op, b, dinv, x0=x0, tol=1e-13)
  assert status == 'converged'
  # atol wins over tol
  its, status = _same(op, b, dinv, tol=1e-30, atol=1e-3)
  assert status == 'converged' and 0 < len(its) < 30
  # b = 0: converged before the first iteration
  its, status = _same(op, np.zeros(len(b)), dinv)
  assert status == 'converged' and not its


def test_pieces_reproduce_the_skew_breakdown():
  K = np.array([[0.0, 1.0], [-1.0, 0.0]])
  its, status = _same(lambda v: K @ v, np.array([1.0, 2.0]))
  assert status == 'breakdown_alpha' and not its


def test_pieces_reproduce_the_half_step_stop():
  """The identity: p = b, v = b, alpha = 1, s = 0.  The iteration ends after
  its first half, counted as one, and t is never formed."""
  b = np.random.default_rng(3).standard_normal(50)
  calls = []

  def A(v):
    calls.append(1)
    return v.copy()
  x, its, status, count = BS.bicgstab_by_pieces(A, b, tol=1e-12)
  assert status == 'converged' and count == 1 and len(calls) == 1
  assert np.array_equal(x, b)
  its, status = _same(lambda v: v.copy(), b, tol=1e-12)
  assert status == 'converged' and len(its) == 1
  # a diagonal operator stops in the half-step with the Jacobi preconditioner
  d = 1.0 + np.arange(50.0)
  its, status = _same(lambda v: d * v, b, 1.0 / d, tol=1e-12)
  assert status == 'converged' and len(its) == 1


def test_update_xr_half_step_reads_neither_t_nor_shat():
  rng = np.random.default_rng(0)
  x, phat, sv, r0 = rng.standard_normal((4, 9))
  nan = np.full(9, np.nan)
  for half, tt in ((1.0, 2.0), (0.0, 0.0)):
    s = np.zeros(BS.NSLOTS)
    s[BS.ALPHA], s[BS.HALF], s[BS.TS], s[BS.TT] = 0.75, half, 1.0, tt
    xn, rn, rr, rho = BS.update_xr(x, phat, nan, sv, nan, r0, s)
    assert np.array_equal(xn, x + 0.75 * phat) and np.array_equal(rn, sv)
    assert rr == sv @ sv and rho == r0 @ sv


def test_scalar_phase_leaves_a_finished_solve_alone():
  s = np.arange(1.0, BS.NSLOTS + 1)
  s[BS.DONE] = 1.0
  for phase in (1, 2, 3):
    assert np.array_equal(BS.scalar_phase(s, phase, 10, 1e-5, 0.0), s)
  t = BS.scalar_phase(s, 0, 10, 1e-5, 0.0)
  assert t[BS.DONE] == 0.0 and t[BS.STATUS] == 0.0 and t[BS.ITERS] == 0.0
  assert t[BS.RHO] == s[BS.RHO_NEW] and t[BS.RESIDUAL] == s[BS.RR]
  with pytest.raises(ValueError):
    BS.scalar_phase(np.zeros(BS.NSLOTS), 4, 10, 1e-5, 0.0)
