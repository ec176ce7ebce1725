"""Newton's method with CG on the tangent and a backtracking line search: the
driver of one load entry of `solve_hyperelasticity` and `solve_plasticity`.

    r = evaluate(u),   T(u) dw = -r  (CG),   u <- u + t dw,

with t = 1, 1/2, .., 2^-LINE_SEARCH_HALVINGS until |r(u + t dw)| is finite and
<= (1 - ARMIJO t) |r|.  One `evaluate` per trial state, one tangent apply per
CG iteration; the driver itself touches the device only through them, `cg`
and the update of u.
"""

from __future__ import annotations

import math

from swirl_fem_amd.linalg.cg import cg

# pylint: disable=invalid-name

LINE_SEARCH_HALVINGS = 10     # t = 1, 1/2, ..., 2^-10
ARMIJO = 1e-4


def newton_cg(evaluate, tangent, u, M=None, *, newton_rtol, newton_atol,
              max_newton, linear_rtol, who, where, breakdown_hint,
              nonfinite_hint='', check_every=16, rec=None):
  """Iterates from `u` until |r| <= max(newton_rtol |r_0|, newton_atol);
  returns (u, lin, rec) with `lin` the linearisation at the returned u.

  `evaluate(v) -> (lin, r, |r|)`: whatever `tangent` needs at v, the residual
  in the shape of `u` and its norm as a float.  `tangent(lin) -> apply`, the
  tangent's product with a vector in the shape of `u`; CG runs on the flat
  vectors with the preconditioner `M`, to `linear_rtol`, polling its
  convergence flag every `check_every` iterations.

  `rec`: the record of this entry, a dict with the lists 'residual_norms' (one
  per iteration, the first is |r_0|), 'step_lengths' and 'cg_iterations' and
  with 'status'; the caller may pass one that has further keys.

  Raises RuntimeError with `rec['status']` set to 'max_newton', 'line_search'
  or 'cg_' + CG's status when the iteration fails (a non-finite residual at
  the start leaves 'running').  The texts begin with `who`; `where(it)` names
  Newton iteration `it` of the entry and `where(None, note)` the entry alone,
  with `note` inside its parenthesis; `breakdown_hint` says why CG may have
  broken down and `nonfinite_hint` is appended to the first refusal."""
  if rec is None:
    rec = dict(residual_norms=[], step_lengths=[], cg_iterations=[],
               status='running')
  lin, r, rnorm = evaluate(u)
  if not math.isfinite(rnorm):
    raise RuntimeError(f'{who}: the residual is not finite at the start of '
                       f'{where(0)}{nonfinite_hint}')
  rec['residual_norms'].append(rnorm)
  target = max(newton_rtol * rnorm, newton_atol)
  it = 0
  while rnorm > target:
    if it == max_newton:
      rec['status'] = 'max_newton'
      note = f'|r| = {rnorm:.3e}, target {target:.3e}'
      raise RuntimeError(
          f'{who}: no convergence within max_newton = {max_newton} '
          f'iterations in {where(None, note)}')
    it += 1
    apply = tangent(lin)
    A = lambda x: apply(x.view(u.shape)).reshape(-1)
    dw, cg_info = cg(A, (-r).reshape(-1).contiguous(), tol=linear_rtol, M=M,
                     check_every=check_every)
    rec['cg_iterations'].append(int(cg_info['num_iterations']))
    if str(cg_info['status']).startswith('breakdown'):
      rec['status'] = 'cg_' + cg_info['status']
      raise RuntimeError(
          f'{who}: CG broke down ({cg_info["status"]}; {breakdown_hint}) in '
          f'{where(it)}')
    dw = dw.view(u.shape)
    t, accepted = 1.0, False
    for _ in range(LINE_SEARCH_HALVINGS + 1):
      lin_t, r_t, n_t = evaluate(u + t * dw)
      if math.isfinite(n_t) and n_t <= (1.0 - ARMIJO * t) * rnorm:
        accepted = True
        break
      t *= 0.5
    if not accepted:
      rec['status'] = 'line_search'
      raise RuntimeError(
          f'{who}: line search exhausted (t down to '
          f'2^-{LINE_SEARCH_HALVINGS}) in {where(it)}, |r| = {rnorm:.3e}')
    u = u + t * dw
    lin, r, rnorm = lin_t, r_t, n_t
    rec['step_lengths'].append(t)
    rec['residual_norms'].append(rnorm)
  rec['status'] = 'converged'
  return u, lin, rec


__all__ = ['ARMIJO', 'LINE_SEARCH_HALVINGS', 'newton_cg']
