"""Host tests of what the Krylov solvers share around their iteration
(`swirl_fem_amd/linalg/_driver.py`): none of it needs a GPU."""

import inspect

import pytest

from swirl_fem_amd.linalg import _driver


def _solver(name, info):
  """Stands for `cg` / `cg_ensemble` / `bicgstab`: one frame between the
  helper and the caller the warning is meant for."""
  _driver.warn_on_breakdown(name, info)


def test_breakdown_warning_names_the_solvers_caller():
  info = {'status': 'breakdown_pAp', 'num_iterations': 7}
  with pytest.warns(RuntimeWarning) as caught:
    line = inspect.currentframe().f_lineno + 1
    _solver('cg', info)
  assert len(caught) == 1
  assert caught[0].filename == __file__ and caught[0].lineno == line
  assert str(caught[0].message) == (
      "cg stopped with status 'breakdown_pAp' after 7 iterations: x is the "
      'last iterate, not a solution to the requested tolerance')
  with pytest.warns(RuntimeWarning, match=r"^bicgstab stopped with status "
                    r"'breakdown_rho' after 3 iterations: x is the last"):
    _solver('bicgstab', {'status': 'breakdown_rho', 'num_iterations': 3})


def test_breakdown_warning_of_an_ensemble():
  info = {'status': 'breakdown_gamma', 'num_iterations': 4,
          'member_status': ['converged', 'breakdown_gamma']}
  with pytest.warns(RuntimeWarning) as caught:
    _solver('cg_ensemble', info)
  assert str(caught[0].message) == (
      "cg_ensemble: a member stopped with status 'breakdown_gamma': its x is "
      'the last iterate, not a solution to the requested tolerance')
  assert caught[0].filename == __file__


@pytest.mark.parametrize('status', ['converged', 'maxiter', 'running'])
def test_no_warning_without_a_breakdown(status, recwarn):
  _solver('cg', {'status': status, 'num_iterations': 1})
  assert not recwarn.list


class _Run:
  """Counts steps and polls; reports the end after `stop_at` steps."""

  def __init__(self, maxiter, stop_at):
    self.maxiter, self.stop_at = maxiter, stop_at
    self.issued = self.polls = 0

  def step(self):
    self.issued += 1

  def done(self):
    self.polls += 1
    return self.issued >= self.stop_at


@pytest.mark.parametrize('maxiter,stop_at,check_every,steps,polls', [
    (100, 20, 16, 32, 2),     # polled after 16 and 32 steps
    (10, 99, 4, 10, 3),       # the last batch is cut to maxiter
    (10, 0, 16, 10, 1),       # no poll before the first batch
    (0, 0, 16, 0, 0)])
def test_drive_steps_in_batches(maxiter, stop_at, check_every, steps, polls):
  run = _Run(maxiter, stop_at)
  _driver.drive(run, check_every)
  assert (run.issued, run.polls) == (steps, polls)


def test_kept_runner_reuses_orders_and_trims():
  ws, made = {}, []

  def make():
    made.append(object())
    return made[-1]

  a, kept = _driver.kept_runner(ws, 'a', 2, lambda run: True, make)
  assert not kept and ws == {'a': a}
  b, _ = _driver.kept_runner(ws, 'b', 2, lambda run: True, make)
  again, kept = _driver.kept_runner(ws, 'a', 2, lambda run: run is a, make)
  assert kept and again is a and list(ws) == ['b', 'a']   # most recent last
  c, _ = _driver.kept_runner(ws, 'c', 2, lambda run: True, make)
  assert list(ws) == ['a', 'c']                           # the oldest went
  # a state that does not fit is replaced under its key
  a2, kept = _driver.kept_runner(ws, 'a', 2, lambda run: False, make)
  assert not kept and a2 is not a and ws == {'c': c, 'a': a2}
  assert len(made) == 4
