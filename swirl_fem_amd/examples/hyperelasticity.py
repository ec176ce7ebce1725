"""Finite-strain elasticity of a compressible neo-Hookean solid.

    lambda0 rho u - Div P(F) = f   in the reference mesh,   F = I + grad u,
    P(F) = mu (F - F^-T) + lambda ln J F^-T,   J = det F,
    u_c = g_c on the fixed components of Dirichlet groups,
    (P N)_c = t_c on Neumann groups (dead loads: traction per unit reference
    area in Cartesian components; zero on every free component of the
    boundary that no group names),

for displacements u (N, d), total Lagrangian; plane strain in 2D.  The stored
energy is psi = mu/2 (F:F - d) - mu ln J + lambda/2 (ln J)^2, whose
linearisation at u = 0 is the material of `examples/elasticity.py`.

Quadrature, boundary data and the load vector are those of
`solve_elasticity`.  The loads are applied in `load_steps` equal increments;
each increment is solved by Newton's method on the free components,

    r = keep (R(u) - f_ext),   T(u) dw = -r  (CG),   u <- u + t dw,

with a backtracking line search on |r| (`FiniteElementSpace.
hyperelastic_operator`): one residual launch per trial state,
which also stores what the tangent needs, one tangent launch per CG iteration.

With `differentiable=True` the solve is one autograd node: the
adjoint solve runs CG on the tangent at the converged state, the coefficient
gradients come from `sfem_hyperelastic_sens` on the state that launch stored.
"""

from __future__ import annotations

from typing import Mapping, Tuple

import torch

from swirl_fem_amd.core.mesh import Mesh
from swirl_fem_amd.examples.elasticity import _check_every
from swirl_fem_amd.examples.elasticity import _check_preconditioner
from swirl_fem_amd.examples.elasticity import _detached
from swirl_fem_amd.examples.elasticity import _requires_grad
from swirl_fem_amd.examples.elasticity import _setup
from swirl_fem_amd.examples.poisson import BCType
from swirl_fem_amd.linalg.cg import cg
# (the two constants stay importable from here)
from swirl_fem_amd.linalg.newton import ARMIJO, LINE_SEARCH_HALVINGS
from swirl_fem_amd.linalg.newton import newton_cg

# pylint: disable=invalid-name


class _HyperelasticSolve(torch.autograd.Function):
  """`_solve` as one autograd node: the adjoint solve on the tangent at the
  final accepted linearisation, the mass apply and the coefficient
  sensitivities in `backward`."""

  @staticmethod
  def forward(ctx, body_force, lame_lambda, lame_mu, density, mesh,
              boundary_conditions, kwargs, adjoint_rtol, holder):
    state = {}
    u, info = _solve(mesh, _detached(body_force), boundary_conditions,
                     lame_lambda=_detached(lame_lambda),
                     lame_mu=_detached(lame_mu), density=_detached(density),
                     return_info=True, _state=state, **kwargs)
    holder['info'] = info
    state.update(holder=holder, adjoint_rtol=adjoint_rtol)
    ctx.state = state
    ctx.save_for_backward(u)
    ctx.force_shape = (tuple(body_force.shape)
                       if isinstance(body_force, torch.Tensor) else None)
    ctx.like = [(v.dtype, v.device) if isinstance(v, torch.Tensor) else None
                for v in (body_force, lame_lambda, lame_mu, density)]
    return u

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, u_bar):
    st = ctx.state
    op, keep, l0, lin = st['op'], st['keep'], st['lambda0'], st['lin']
    N, d = keep.shape
    # keep T(u) keep v = keep u_bar: the tangent is symmetric (dead loads)
    # and the operator's mask is `keep`
    T = op.tangent(lin, l0)
    A = lambda x: T.apply(x.view(N, d)).reshape(-1)
    rhs = (u_bar.detach().to(keep.dtype) * keep).reshape(-1).contiguous()
    v, info = cg(A, rhs, tol=st['adjoint_rtol'], M=st['M'],
                 check_every=_check_every(st['M']))
    st['holder']['info']['adjoint'] = info
    if str(info['status']).startswith('breakdown'):
      raise RuntimeError(
          f'solve_hyperelasticity: CG broke down in the adjoint solve of '
          f'backward ({info["status"]}; the tangent at the converged state '
          f'may have lost definiteness)')
    v = v.view(N, d)
    need = ctx.needs_input_grad
    grads = [None, None, None, None]
    if need[0]:
      g = st['Bf'](v)
      grads[0] = g.sum(dim=0) if ctx.force_shape == (d,) else g
    if any(need[1:4]):
      sens = op.sensitivity(ctx.saved_tensors[0], v, l0,
                            want=tuple(need[1:4]), linearization=lin)
      for n, g in enumerate(sens):
        if need[1 + n] and g is not None:
          grads[1 + n] = -g
    for n, like in enumerate(ctx.like):
      if grads[n] is not None and like is not None:
        grads[n] = grads[n].to(dtype=like[0], device=like[1])
    return (*grads, None, None, None, None, None)


def solve_hyperelasticity(mesh: Mesh, body_force,
                          boundary_conditions: Mapping[str,
                                                       Tuple[BCType, object]],
                          *, lame_lambda, lame_mu, density=None,
                          lambda0: float = 0.0, load_steps: int = 1,
                          newton_rtol: float = 1e-8, newton_atol: float = 0.0,
                          max_newton: int = 25, linear_rtol: float = 1e-6,
                          preconditioner=None, u0=None,
                          return_info: bool = False,
                          differentiable: bool = False, adjoint_rtol=None):
  """Solves `lambda0 rho u - Div P(I + grad u) = body_force` for a
  compressible neo-Hookean material; returns u (N, d).

  `lame_lambda`, `lame_mu`, `density`, `body_force` and
  `boundary_conditions` take the forms of `solve_elasticity`: per-component
  Dirichlet values (None leaves a component free, so rollers and symmetry
  planes work) and Neumann values, here dead loads: the traction P N per unit
  reference area, in Cartesian components.

  For load step k = 1 .. `load_steps` the body force, the tractions and the
  Dirichlet values are scaled by k / load_steps, the fixed components of u are
  set to the scaled values and Newton iterates on the free ones from the
  previous step's solution (`u0` (N, d), default zero, before the first).  An
  iteration stops the step when |r| <= max(newton_rtol |r_0|, newton_atol)
  with r_0 the residual at the start of the step; otherwise it solves
  T(u) dw = -r by CG to `linear_rtol` and backtracks t = 1, 1/2, .., 2^-10
  until |r(u + t dw)| is finite and <= (1 - 1e-4 t) |r|.  A trial state with
  an inverted element (J <= 0, a non-finite residual) is rejected like any
  other.

  `preconditioner`: None, 'jacobi' or a callable `(op, lambda0) -> M`, built
  once per solve on the linear `ElasticityOperator` with the same mask and
  coefficients (the tangent at u = 0), so
  `linalg.pmg_elasticity.ElasticityPMultigrid` works unchanged.

  Raises RuntimeError, naming the load step and the iteration, when the line
  search is exhausted, when CG breaks down (the tangent can lose
  definiteness) and when `max_newton` iterations do not converge.  With
  `return_info` returns (u, info): info['load_steps'] is a list with, per load
  step, 'residual_norms' (one per Newton iteration, the first is |r_0|),
  'step_lengths', 'cg_iterations' and 'status'; info['status'] is
  'converged'.

  Autograd is opt-in: without `differentiable=True` inputs that
  require grad are refused.  With it the result is differentiable with respect
  to `body_force` and to `lame_lambda`, `lame_mu` and `density` given as
  tensors that require grad (scalar, (E,) or (E, Q^d); the gradient has the
  form passed in).  The gradient is that of the converged state: load stepping
  does not enter it, and its error scales with the Newton residual that is
  left, so tighten `newton_rtol` for an accurate gradient.  Backward is one CG
  solve on the tangent at the final accepted linearisation with the forward
  solve's preconditioner, to `adjoint_rtol` (None: `newton_rtol`; the forward
  `linear_rtol` is that of an inexact Newton step and would limit the
  gradient), one launch of the sensitivity kernel
  (`HyperelasticOperator.sensitivity`) and one mass apply; with `return_info`
  the info then also carries `adjoint`, the adjoint solve's CG info.  A
  breakdown of that CG raises RuntimeError and names the adjoint solve.
  Gradients with respect to Dirichlet values, tractions, through callables and
  with respect to the mesh are not propagated, nor are second derivatives.
  `u0` that requires grad is refused either way: the solution does not depend
  on it.  When nothing requires grad the solve runs exactly as without the
  keyword and builds no autograd node.

  Partitioned meshes, ensembles, periodic images and ROBIN conditions are
  refused."""
  _check_preconditioner(preconditioner)
  if int(load_steps) != load_steps or load_steps < 1:
    raise ValueError(f'load_steps must be a positive integer, got '
                     f'{load_steps!r}')
  if max_newton < 1:
    raise ValueError(f'max_newton must be at least 1, got {max_newton!r}')
  if _requires_grad(u0):
    raise NotImplementedError(
        'autograd through solve_hyperelasticity with respect to u0: the '
        'solution does not depend on the initial guess; pass it detached')
  grad = _requires_grad(body_force, lame_lambda, lame_mu, density)
  if grad and not differentiable:
    raise NotImplementedError(
        'autograd through solve_hyperelasticity: pass differentiable=True, '
        'or detached inputs')
  kwargs = dict(lambda0=lambda0, load_steps=load_steps,
                newton_rtol=newton_rtol, newton_atol=newton_atol,
                max_newton=max_newton, linear_rtol=linear_rtol,
                preconditioner=preconditioner, u0=u0)
  if not grad:
    return _solve(mesh, body_force, boundary_conditions,
                  lame_lambda=lame_lambda, lame_mu=lame_mu, density=density,
                  return_info=return_info, **kwargs)
  holder = {}
  rtol = newton_rtol if adjoint_rtol is None else adjoint_rtol
  u = _HyperelasticSolve.apply(body_force, lame_lambda, lame_mu, density, mesh,
                               boundary_conditions, kwargs, float(rtol),
                               holder)
  return (u, holder['info']) if return_info else u


def _solve(mesh: Mesh, body_force, boundary_conditions, *, lame_lambda,
           lame_mu, density, lambda0, load_steps, newton_rtol, newton_atol,
           max_newton, linear_rtol, preconditioner, u0, return_info=False,
           _state=None):
  """The body of `solve_hyperelasticity`, its arguments checked.  `_state`: a
  dict that receives what the adjoint solve needs (the operator, the mask,
  the preconditioner, the final linearisation, the mass apply)."""
  load_steps = int(load_steps)
  st = _setup(
      'solve_hyperelasticity', mesh, body_force, boundary_conditions, lambda0,
      preconditioner,
      lambda fespace, mask: fespace.hyperelastic_operator(
          mask, lame_lambda=lame_lambda, lame_mu=lame_mu, density=density),
      linear=lambda op: op.linear, u0=u0)
  op, fespace, keep, M, u = st.op, st.fespace, st.keep, st.M, st.u
  lambda0 = st.lambda0
  f_ext = st.load * keep

  steps = []
  for k in range(1, load_steps + 1):
    scale = k / load_steps
    u = torch.where(st.fixed, scale * st.u_D, u)
    rec = dict(residual_norms=[], step_lengths=[], cg_iterations=[],
               status='running')
    steps.append(rec)

    def where(it, note=None):
      step = f'load step {k} of {load_steps}'
      return (f'{step} ({note})' if it is None
              else f'{step}, Newton iteration {it}')

    def evaluate(v):
      """(linearisation at v, r = keep (R(v) - scale f_ext), |r|)."""
      lin = op.linearize(v, lambda0)       # the mask is applied: keep R(v)
      r = lin.residual - scale * f_ext
      return lin, r, float(torch.linalg.vector_norm(r))

    u, lin, _ = newton_cg(
        evaluate, lambda lin: op.tangent(lin, lambda0).apply, u, M,
        newton_rtol=newton_rtol, newton_atol=newton_atol,
        max_newton=max_newton, linear_rtol=linear_rtol,
        who='solve_hyperelasticity', where=where,
        breakdown_hint='the tangent may have lost definiteness',
        nonfinite_hint=' (an inverted element: more load steps may help)',
        check_every=_check_every(M), rec=rec)
  if _state is not None:
    _state.update(op=op, keep=keep, M=M, lambda0=lambda0, lin=lin,
                  Bf=lambda x: fespace.helmholtz_operator(None).apply(
                      x.contiguous(), 1.0, 0.0))
  if return_info:
    return u, {'load_steps': steps, 'status': 'converged',
               'num_newton': sum(len(s['step_lengths']) for s in steps),
               'num_cg': sum(sum(s['cg_iterations']) for s in steps)}
  return u


__all__ = ['BCType', 'solve_hyperelasticity']
