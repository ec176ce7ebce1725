"""`linalg.newton.newton_cg`, the Newton-CG driver of one load entry of
`solve_hyperelasticity` and `solve_plasticity`, on a synthetic problem: no
mesh and no element kernel.  The unknown is a device vector of 8 entries,

    r(v) = v^3 + v - b,   T(v) w = (3 v^2 + 1) w,

in plain torch; `cg` and its kernels are the real ones.  Convergence and every
failure branch of the forward iteration: the status left in the record and the
caller's texts in the message.  NaN and negative curvature are arithmetic
here; nothing faults."""
import math

import pytest
import torch

from swirl_fem_amd.examples import hyperelasticity
from swirl_fem_amd.linalg import newton
from swirl_fem_amd.linalg.newton import LINE_SEARCH_HALVINGS, newton_cg

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N = 8


def _problem(b=None):
  """(evaluate, tangent, u0, calls): `calls` counts the evaluations."""
  if b is None:
    b = torch.linspace(1.0, 30.0, N, dtype=torch.float64, device=DEV)
  calls = []

  def evaluate(v):
    calls.append(1)
    r = v ** 3 + v - b
    return v, r, float(torch.linalg.vector_norm(r))
  tangent = lambda v: lambda w: (3.0 * v ** 2 + 1.0) * w
  return evaluate, tangent, torch.zeros_like(b), calls


def _where(it, note=None):
  return f'entry A ({note})' if it is None else f'entry A, iteration {it}'


def _run(evaluate, tangent, u0, rec=None, M=None, **kw):
  opts = dict(newton_rtol=1e-10, newton_atol=0.0, max_newton=40,
              linear_rtol=1e-12, who='synthetic', where=_where,
              breakdown_hint='the hint of the caller')
  opts.update(kw)
  return newton_cg(evaluate, tangent, u0, M, rec=rec, **opts)


def _record():
  return dict(tag='mine', residual_norms=[], step_lengths=[],
              cg_iterations=[], status='running')


def test_constants_are_shared():
  assert hyperelasticity.LINE_SEARCH_HALVINGS is newton.LINE_SEARCH_HALVINGS
  assert hyperelasticity.ARMIJO is newton.ARMIJO


def test_converges():
  evaluate, tangent, u0, calls = _problem()
  rec = _record()
  u, lin, out = _run(evaluate, tangent, u0, rec)
  assert out is rec and list(rec)[0] == 'tag'   # the caller's record, kept
  assert rec['status'] == 'converged'
  norms = rec['residual_norms']
  assert len(norms) >= 3          # from zero the full step overshoots
  assert all(b < a for a, b in zip(norms, norms[1:]))
  assert len(rec['step_lengths']) == len(rec['cg_iterations']) == len(norms) - 1
  assert rec['step_lengths'][0] < 1.0 and rec['step_lengths'][-1] == 1.0
  assert norms[-1] <= 1e-10 * norms[0]
  # `lin` is the linearisation at the returned u, and u solves the cubic
  assert torch.equal(lin, u)
  _, r, n = evaluate(u)
  assert n == norms[-1]
  # one evaluation at the start, one per trial state
  trials = sum(1 + round(-math.log2(t)) for t in rec['step_lengths'])
  assert len(calls) - 1 == 1 + trials
  assert u0.abs().max() == 0.0    # the start vector is not written


def test_default_record():
  evaluate, tangent, u0, _ = _problem()
  _, _, rec = _run(evaluate, tangent, u0)
  assert list(rec) == ['residual_norms', 'step_lengths', 'cg_iterations',
                       'status']
  assert rec['status'] == 'converged'


def test_nonfinite_start():
  b = torch.ones(N, dtype=torch.float64, device=DEV)
  b[3] = float('nan')
  evaluate, tangent, u0, calls = _problem(b)
  rec = _record()
  with pytest.raises(RuntimeError) as err:
    _run(evaluate, tangent, u0, rec, nonfinite_hint=' (a hint)')
  assert str(err.value) == ('synthetic: the residual is not finite at the '
                            'start of entry A, iteration 0 (a hint)')
  assert rec['status'] == 'running' and rec['residual_norms'] == []
  assert len(calls) == 1


def test_max_newton():
  evaluate, tangent, u0, _ = _problem()
  rec = _record()
  with pytest.raises(RuntimeError) as err:
    _run(evaluate, tangent, u0, rec, max_newton=1)
  assert rec['status'] == 'max_newton'
  text = str(err.value)
  assert text.startswith('synthetic: no convergence within max_newton = 1 '
                         'iterations in entry A (|r| = ')
  assert f'|r| = {rec["residual_norms"][-1]:.3e}, target ' in text
  assert len(rec['step_lengths']) == len(rec['cg_iterations']) == 1
  assert len(rec['residual_norms']) == 2


def test_line_search_exhausted():
  inner, tangent, u0, calls = _problem()
  first = []

  def evaluate(v):
    lin, r, n = inner(v)
    first.append(n)
    return lin, r, first[0]       # the norm never decreases
  rec = _record()
  with pytest.raises(RuntimeError) as err:
    _run(evaluate, tangent, u0, rec)
  assert rec['status'] == 'line_search'
  assert len(calls) - 1 == LINE_SEARCH_HALVINGS + 1    # trial evaluations
  text = str(err.value)
  assert text.startswith(
      f'synthetic: line search exhausted (t down to 2^-{LINE_SEARCH_HALVINGS})'
      ' in entry A, iteration 1, |r| = ')
  assert len(rec['cg_iterations']) == 1 and rec['step_lengths'] == []
  assert len(rec['residual_norms']) == 1


def test_cg_breakdown():
  """A negative definite tangent under its own Jacobi preconditioner: r.Mr is
  negative and CG reports a breakdown.  (Without a preconditioner this CG
  divides by any finite non-zero p.Ap and solves a negative definite system
  like its negative; what breaks down is the sign of r.Mr, or p.Ap = 0.)"""
  evaluate, _, u0, calls = _problem()
  diag = lambda v: -(3.0 * v ** 2 + 1.0)
  tangent = lambda v: lambda w: diag(v) * w
  M = lambda r: r / diag(u0)
  rec = _record()
  with pytest.warns(RuntimeWarning, match='breakdown'):
    with pytest.raises(RuntimeError) as err:
      _run(evaluate, tangent, u0, rec, M=M)
  assert rec['status'] == 'cg_breakdown_gamma'
  text = str(err.value)
  assert text.startswith('synthetic: CG broke down (breakdown')
  assert text.endswith('; the hint of the caller) in entry A, iteration 1')
  assert len(rec['cg_iterations']) == 1 and rec['step_lengths'] == []
  assert len(calls) == 1          # no trial state was evaluated
