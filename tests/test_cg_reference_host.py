"""The NumPy restatement of the device CG (`tests/cg_reference.py`) against
the oracle's CG on a small SPD system: pinned on the host before any kernel is
compared with it."""
import numpy as np
import pytest

from oracle import sfem_oracle as O
from tests import cg_reference as CG

N = 37


def _system(seed=0, n=N):
  rng = np.random.default_rng(seed)
  q = rng.standard_normal((n, n))
  a = q @ q.T / n + np.diag(1.0 + rng.random(n))
  return (lambda v: a @ v), a, rng.standard_normal(n)


def _oracle_iterates(A, b, count, **kw):
  return [O.cg(A, b, tol=0.0, maxiter=k, **kw)[0] for k in range(1, count + 1)]


@pytest.mark.parametrize('schedule', CG.SCHEDULES)
def test_schedules_give_the_oracle_iterates(schedule):
  A, _, b = _system()
  want = _oracle_iterates(A, b, 12)
  x, iterates, status, iters = CG.cg_by_pieces(A, b, tol=0.0, maxiter=12,
                                               schedule=schedule)
  assert status == 'maxiter' and iters == 12 and len(iterates) == 12
  for k, (g, w) in enumerate(zip(iterates, want)):
    assert np.array_equal(g, w), (schedule, k)
  assert np.array_equal(x, want[-1])


@pytest.mark.parametrize('schedule', CG.SCHEDULES)
@pytest.mark.parametrize('tol', [1e-3, 1e-8, 1e-13])
def test_schedules_stop_where_the_oracle_stops(schedule, tol):
  A, _, b = _system(1)
  want, info = O.cg(A, b, tol=tol)
  x, iterates, status, iters = CG.cg_by_pieces(A, b, tol=tol,
                                               schedule=schedule)
  assert status == 'converged'
  assert iters == info['num_iterations'] == len(iterates)
  assert np.array_equal(x, want)


def test_nine_pass_with_a_preconditioner():
  A, a, b = _system(2)
  d = 1.0 / np.diag(a)
  M = lambda r: d * r
  want, info = O.cg(A, b, tol=1e-10, M=M)
  x, _, status, iters = CG.cg_by_pieces(A, b, tol=1e-10, M=M)
  assert status == 'converged' and iters == info['num_iterations']
  assert np.array_equal(x, want)


def test_start_and_breakdown_statuses():
  A, _, b = _system(3)
  assert CG.cg_by_pieces(A, 0.0 * b)[2:] == ('converged', 0)
  assert CG.cg_by_pieces(A, b, maxiter=0)[2:] == ('maxiter', 0)
  zero = lambda v: 0.0 * v
  for schedule in CG.SCHEDULES:
    x, its, status, iters = CG.cg_by_pieces(zero, b, schedule=schedule)
    assert (status, iters, its) == ('breakdown_pAp', 0, [])
    assert np.array_equal(x, 0.0 * b)
  # a negative definite operator converges like its negative
  neg = lambda v: -A(v)
  for schedule in CG.SCHEDULES:
    xn, _, status, iters = CG.cg_by_pieces(neg, b, tol=1e-10,
                                           schedule=schedule)
    xp, _, _, ip = CG.cg_by_pieces(A, b, tol=1e-10, schedule=schedule)
    assert status == 'converged' and iters == ip
    assert np.array_equal(xn, -xp)


@pytest.mark.parametrize('schedule', ['eight', 'deferred'])
@pytest.mark.parametrize('m', [2, 3, 4])
def test_lazy_update_is_bitwise_the_plain_one(m, schedule):
  """After any number of steps: the flush after k iterations for every k up
  to two and a half turns of the largest ring."""
  A, _, b = _system(4)
  for k in range(1, 11):
    want, plain, _, _ = CG.cg_by_pieces(A, b, tol=0.0, maxiter=k,
                                        schedule=schedule)
    x, iterates, status, iters = CG.cg_by_pieces(
        A, b, tol=0.0, maxiter=k, schedule=schedule, lazy_m=m)
    assert (status, iters) == ('maxiter', k)
    assert np.array_equal(x, want), (m, k)
    assert all(np.array_equal(g, w) for g, w in zip(iterates, plain))
  want, _, _, iw = CG.cg_by_pieces(A, b, tol=1e-9, schedule=schedule)
  x, _, status, iters = CG.cg_by_pieces(A, b, tol=1e-9, schedule=schedule,
                                        lazy_m=m)
  assert status == 'converged' and iters == iw and np.array_equal(x, want)


@pytest.mark.parametrize('schedule', ['eight', 'deferred'])
def test_mean_pair_is_the_oracle_with_the_projection(schedule):
  """M r = r - (w.r / total) 1 folded into the two updates.  The fused form
  takes r.z as r.r - c 1.r where the oracle sums r (r - c): the same number
  up to the rounding of two sums of n terms, so the iterates agree to a few
  n eps times the growth over the iterations, not bitwise."""
  rng = np.random.default_rng(5)
  n = N
  # a singular Neumann-like operator: the weighted graph Laplacian of a ring
  c = 1.0 + rng.random(n)
  A = lambda v: c * (v - np.roll(v, 1)) - np.roll(c * (v - np.roll(v, 1)), -1)
  w = np.ones(n) * 0.75
  total_w = w.sum()
  b = rng.standard_normal(n)
  b -= b.mean()
  M = lambda r: r - np.vdot(w, r) / total_w
  count = 8
  want = _oracle_iterates(A, b, count, M=M)
  x, iterates, status, iters = CG.cg_by_pieces(
      A, b, tol=0.0, maxiter=count, schedule=schedule, mean=(w, total_w))
  assert (status, iters, len(iterates)) == ('maxiter', count, count)
  for k, (g, wnt) in enumerate(zip(iterates, want)):
    assert np.abs(g - wnt).max() <= 1e-12 * np.abs(wnt).max(), (k,)
  xo, info = O.cg(A, b, tol=1e-6, M=M)
  x, _, status, iters = CG.cg_by_pieces(A, b, tol=1e-6, schedule=schedule,
                                        mean=(w, total_w))
  assert status == 'converged' and iters == info['num_iterations']
  assert np.abs(x - xo).max() <= 1e-10 * np.abs(xo).max()


def test_scalar_phase_refusals_and_copies():
  s = np.arange(1.0, CG.NSLOTS + 1)
  s[[CG.DONE, CG.OPEN]] = 0.0
  for phase in (-1, 9):
    with pytest.raises(ValueError):
      CG.scalar_phase(s, phase, 10, 1e-5, 0.0)
  for phase in (3, 4, 5):
    with pytest.raises(ValueError):
      CG.scalar_phase(s, phase, 10, 1e-5, 0.0)
  for phase in (0, 1, 2, 6, 7):
    with pytest.raises(ValueError):
      CG.scalar_phase(s, phase, 10, 1e-5, 0.0, np.ones(4), stored=True)
  before = s.copy()
  parts = np.ones(CG.DOT_SLOTS)
  out, pout = CG.scalar_phase(s, 5, 10, 1e-5, 0.0, parts)
  assert np.array_equal(s, before) and parts.sum() == CG.DOT_SLOTS
  assert out[CG.PAP] == CG.DOT_SLOTS and not pout.any()
  # done: scalars kept, accumulated partials still cleared (1, 2, 5)
  s[CG.DONE] = 1.0
  for phase in (0, 1, 3, 4, 5, 6, 7):
    out, pout = CG.scalar_phase(s, phase, 10, 1e-5, 0.0, parts)
    assert np.array_equal(out, s)
    assert pout.any() == (phase not in (1, 5))
  out, pout = CG.scalar_phase(s, 2, 10, 1e-5, 0.0, parts)
  assert out[CG.DONE] == 0.0 and not pout.any()
