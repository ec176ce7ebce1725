"""Small-strain von Mises (J2) elastoplasticity with linear isotropic hardening.

    lambda0 rho u - div sigma = f,
    sigma = lambda tr(eps) I + 2 mu (eps - eps_p),   eps = sym grad u,
    |dev sigma| sqrt(3/2) <= sigma_y + Hh alpha   (the yield condition),
    u_c = g_c on the fixed components of Dirichlet groups,
    (sigma n)_c = t_c on Neumann groups,

for displacements u (N, d) and a history (eps_p, alpha) at every quadrature
point: the plastic strain (symmetric, trace-free) and the accumulated plastic
strain.  Plane strain in 2D; there is no plane-stress variant.  The material
is rate independent and the answer depends on the load path, so the loads are
given as a path of factors; each entry is one backward-Euler step of the flow
rule (the radial return of `sfem_plasticity_local`) from the
history committed by the entry before.

Quadrature, boundary data and the load vector are those of `solve_elasticity`.
Each entry of the path is solved by Newton's method on the free components,

    r = keep (R(u; history) - s f_ext),   T dw = -r  (CG),   u <- u + t dw,

with the algorithmic tangent T and the backtracking line search of
`solve_hyperelasticity`: one residual launch per trial state, which also
stores what the tangent needs and the trial history, one tangent launch per CG
iteration.  When an entry converges the accepted trial history becomes the
committed one: a buffer swap, no launch.

With `differentiable=True` the whole load path is one autograd node (DESIGN
§3.23): backward walks the entries from the last to the first, each with one
CG solve on the algorithmic tangent of that entry and two launches of
`sfem_plasticity_vjp`, the vector-Jacobian product of the radial return.

With `hardening_modulus = 0` (perfect plasticity) the tangent is only positive
semi-definite once a mechanism has formed: at a limit load CG may break down
or Newton may stall.  Either is reported as a RuntimeError that names the entry
and the iteration; nothing is retried.
"""

from __future__ import annotations

import math
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
from swirl_fem_amd.linalg.newton import newton_cg

# pylint: disable=invalid-name


def _load_path(load_factors):
  """The load path as a tuple of floats: an integer n means k / n, k = 1..n."""
  if isinstance(load_factors, int) and not isinstance(load_factors, bool):
    if load_factors < 1:
      raise ValueError(f'load_factors: a positive integer or a sequence, got '
                       f'{load_factors!r}')
    return tuple(k / load_factors for k in range(1, load_factors + 1))
  try:
    path = tuple(float(s) for s in load_factors)
  except (TypeError, ValueError):
    raise ValueError(f'load_factors: a positive integer or a sequence of '
                     f'factors, got {load_factors!r}') from None
  if not path:
    raise ValueError('load_factors is empty: the load path needs an entry')
  if not all(math.isfinite(s) for s in path):
    raise ValueError(f'load_factors must be finite, got {path!r}')
  return path


class _PlasticitySolve(torch.autograd.Function):
  """`_solve` as one autograd node returning (u, history).  `backward` is the
  path adjoint: over the entries k = K .. 1, each with solution u_k, committed
  history h_{k-1} and factor s_k,

      rhs_k = keep (ubar_k + d(hbar_k . Phi)/du),   T_k v_k = rhs_k   (CG),
      (hbar_{k-1}, g) = d(w . R + hbar_k . Phi)/d(h_{k-1}, theta) at w = -v_k,

  with Phi the history update, ubar_k = 0 for k < K, theta_bar the sum of the
  g, the body-force gradient one mass apply of sum_k s_k v_k and the gradient
  with respect to the input history hbar_0."""

  @staticmethod
  def forward(ctx, body_force, lame_lambda, lame_mu, yield_stress,
              hardening_modulus, density, history, mesh, boundary_conditions,
              kwargs, adjoint_rtol, holder):
    state = {}
    u, committed, info = _solve(
        mesh, _detached(body_force), boundary_conditions,
        lame_lambda=_detached(lame_lambda), lame_mu=_detached(lame_mu),
        yield_stress=_detached(yield_stress),
        hardening_modulus=_detached(hardening_modulus),
        density=_detached(density), history=_detached(history),
        return_info=True, _state=state, **kwargs)
    holder['info'] = info
    state.update(holder=holder, adjoint_rtol=adjoint_rtol)
    ctx.state = state
    ctx.force_shape = (tuple(body_force.shape)
                       if isinstance(body_force, torch.Tensor) else None)
    ctx.like = [(v.dtype, v.device) if isinstance(v, torch.Tensor) else None
                for v in (body_force, lame_lambda, lame_mu, yield_stress,
                          hardening_modulus, density, history)]
    return u, committed

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, u_bar, h_bar):
    st = ctx.state
    op, keep, l0, M = st['op'], st['keep'], st['lambda0'], st['M']
    entries = st['entries']
    N, d = keep.shape
    need = ctx.needs_input_grad
    want = tuple(need[1:6])
    ubar = (u_bar.detach().to(keep.dtype) * keep).contiguous()
    hbar = h_bar.detach().to(keep.dtype).contiguous()
    theta = [None] * 5
    vsum = None
    infos = [None] * len(entries)
    for k in range(len(entries), 0, -1):
      u_k, h_prev, scale = entries[k - 1]
      live = bool((hbar != 0).any())
      rhs = ubar
      if live:   # the operator's mask is `keep`
        rhs = rhs + op.history_vjp(u_k, h_prev, hbar)
      ubar = torch.zeros_like(ubar)      # only the last entry's u is returned
      if not bool((rhs != 0).any()):
        # v_k = 0: no solve, and with hbar_k = 0 nothing flows further back
        infos[k - 1] = {'status': 'skipped', 'num_iterations': 0}
        if not live:
          continue
        v = torch.zeros_like(rhs)
      else:
        lin = op.linearize(u_k, h_prev, l0)
        T = op.tangent(lin, l0)
        A = lambda x, T=T: T.apply(x.view(N, d)).reshape(-1)
        v, info = cg(A, rhs.reshape(-1).contiguous(), tol=st['adjoint_rtol'],
                     M=M, check_every=_check_every(M))
        infos[k - 1] = info
        if str(info['status']).startswith('breakdown'):
          st['holder']['info']['adjoint'] = infos
          raise RuntimeError(
              f'solve_plasticity: CG broke down in the adjoint solve of entry '
              f'{k} of {len(entries)} of the load path in backward '
              f'({info["status"]}; without hardening the tangent is only '
              f'semi-definite at a limit load)')
        v = v.view(N, d)
        if need[0]:
          vsum = scale * v if vsum is None else vsum + scale * v
      grads, hbar = op.sensitivity(u_k, -v, h_prev, hbar if live else None, l0,
                                   want=want, want_history=True)
      for n, g in enumerate(grads):
        if g is not None:
          theta[n] = g if theta[n] is None else theta[n] + g
    st['holder']['info']['adjoint'] = infos
    out = [None] * 7
    if need[0]:
      g = st['Bf'](vsum if vsum is not None else torch.zeros_like(keep))
      out[0] = g.sum(dim=0) if ctx.force_shape == (d,) else g
    for n in range(5):
      if need[1 + n] and theta[n] is not None:
        out[1 + n] = theta[n]
    if need[6]:
      out[6] = hbar
    for n, like in enumerate(ctx.like):
      if out[n] is not None and like is not None:
        out[n] = out[n].to(dtype=like[0], device=like[1])
    return (*out, None, None, None, None, None)


def solve_plasticity(mesh: Mesh, body_force,
                     boundary_conditions: Mapping[str, Tuple[BCType, object]],
                     *, lame_lambda, lame_mu, yield_stress,
                     hardening_modulus=0.0, density=None,
                     lambda0: float = 0.0, load_factors=(1.0,), history=None,
                     newton_rtol: float = 1e-8, newton_atol: float = 0.0,
                     max_newton: int = 25, linear_rtol: float = 1e-6,
                     preconditioner=None, u0=None, return_info: bool = False,
                     differentiable: bool = False, adjoint_rtol=None):
  """Follows the load path `load_factors` for a J2 elastoplastic material;
  returns (u (N, d), history (E, Q^d, NH)) after its last entry.

  `lame_lambda`, `lame_mu`, `density`, `body_force` and `boundary_conditions`
  take the forms of `solve_elasticity`; `yield_stress` > 0 and
  `hardening_modulus` >= 0 those of the Lame parameters.

  `load_factors` is the load path: each entry s scales the body force, the
  tractions and the Dirichlet values, so (0.5, 1.0, 0.0) loads in two steps
  and unloads; an integer n means k / n for k = 1 .. n.  For each entry the
  fixed components of u are set to the scaled values and Newton iterates on
  the free ones from the previous entry's solution (`u0`, default zero, before
  the first) and from the committed history (`history`, default virgin,
  before the first).  An iteration stops the entry when |r| <=
  max(newton_rtol |r_0|, newton_atol) with r_0 the residual at its start;
  otherwise it solves T dw = -r by CG to `linear_rtol` and backtracks t = 1,
  1/2, .., 2^-10 until |r(u + t dw)| is finite and <= (1 - 1e-4 t) |r|.  Trial
  states never touch the committed history; the accepted state's trial
  history is committed when the entry has converged.

  `history` continues a previous call: following (a, b) in one call equals
  following (a,) and then (b,) with the returned history and `u0` = the
  returned u.  The returned history holds per quadrature point eps_p (3D: xx,
  yy, zz, xy, xz, yz; 2D: xx, yy, xy) and, in its last slot, alpha, the
  equivalent plastic strain.

  `preconditioner`: None, 'jacobi' or a callable `(op, lambda0) -> M`, built
  once per call on the linear `ElasticityOperator` with the same mask and
  coefficients (the tangent before first yield), so
  `linalg.pmg_elasticity.ElasticityPMultigrid` works unchanged.

  Raises RuntimeError, naming the entry of the load path and the iteration,
  when the line search is exhausted, when CG breaks down (with
  `hardening_modulus = 0` the tangent is only semi-definite at a limit load)
  and when `max_newton` iterations do not converge; none of these is retried.
  With `return_info` returns (u, history, info): info['load_path'] is a list
  with, per entry, 'factor', 'residual_norms' (one per Newton iteration, the
  first is |r_0|), 'step_lengths', 'cg_iterations', 'plastic_points' (points
  that yielded in the entry's accepted state) and 'status'; info['status'] is
  'converged'.

  Autograd is opt-in: without `differentiable=True` inputs
  that require grad are refused.  With it (u, history) are both
  differentiable with respect to `body_force` ((N, d) or (d,)), to
  `lame_lambda`, `lame_mu`, `yield_stress`, `hardening_modulus` and `density`
  given as tensors that require grad (scalar, (E,) or (E, Q^d); the gradient
  has the form passed in) and to an input `history`.  The gradient is that of
  the whole path: every entry's converged state and committed history enter
  it, so its error scales with the Newton residuals left along the path;
  tighten `newton_rtol` for an accurate gradient.  Forward keeps, per entry,
  u_k and a reference to the history h_{k-1} it started from, so K + 1
  histories (E, Q^d, NH) and K displacement fields stay alive until backward
  has run.  Backward walks the entries from the last to the first: one
  `linearize(u_k, h_{k-1})` launch re-forms the tangent, one CG solve on it
  with the forward solve's preconditioner runs to `adjoint_rtol` (None:
  `newton_rtol`), and two launches of `sfem_plasticity_vjp` carry the
  cotangent of the history through the radial return
  (`PlasticityOperator.history_vjp`, `.sensitivity`); an entry whose
  right-hand side is exactly zero solves nothing.  With `return_info` the
  info then also carries `adjoint`, the list of the per-entry CG infos.  A
  breakdown of such a CG raises RuntimeError and names the entry and the
  adjoint solve.  The return mapping is only piecewise smooth: where a point
  sits on the yield surface (f = 0) the gradient is one-sided, that of the
  elastic branch.  In 3D the cotangent of a history along the trace of eps_p
  is that of sigma = lambda tr(eps) I + 2 mu (eps - eps_p'), which is the
  kernel's stress on trace-free plastic strains, the only admissible ones.
  Gradients with respect to Dirichlet values, tractions, `load_factors`,
  through callables and with respect to the mesh are not propagated, nor are
  second derivatives.  `u0` that requires grad is refused either way: pass it
  detached.  When nothing requires grad the solve runs exactly as without the
  keyword and builds no autograd node.

  Partitioned meshes, ensembles, periodic images and ROBIN conditions are
  refused; 2D is plane strain."""
  who = 'solve_plasticity'
  _check_preconditioner(preconditioner)
  _load_path(load_factors)
  if max_newton < 1:
    raise ValueError(f'max_newton must be at least 1, got {max_newton!r}')
  inputs = (body_force, lame_lambda, lame_mu, yield_stress, hardening_modulus,
            density, history)
  if not differentiable and _requires_grad(*inputs, u0):
    raise NotImplementedError(
        f'autograd through {who}: the solve depends on the load path and is '
        'not differentiated; pass detached inputs')
  if _requires_grad(u0):
    raise NotImplementedError(
        f'autograd through {who} with respect to u0: pass the initial guess '
        'detached')
  kwargs = dict(lambda0=lambda0, load_factors=load_factors,
                newton_rtol=newton_rtol, newton_atol=newton_atol,
                max_newton=max_newton, linear_rtol=linear_rtol,
                preconditioner=preconditioner, u0=u0)
  if not (differentiable and _requires_grad(*inputs)):
    return _solve(mesh, body_force, boundary_conditions,
                  lame_lambda=lame_lambda, lame_mu=lame_mu,
                  yield_stress=yield_stress,
                  hardening_modulus=hardening_modulus, density=density,
                  history=history, return_info=return_info, **kwargs)
  holder = {}
  rtol = newton_rtol if adjoint_rtol is None else adjoint_rtol
  u, committed = _PlasticitySolve.apply(*inputs, mesh, boundary_conditions,
                                        kwargs, float(rtol), holder)
  return (u, committed, holder['info']) if return_info else (u, committed)


def _solve(mesh, body_force, boundary_conditions, *, lame_lambda, lame_mu,
           yield_stress, hardening_modulus, density, lambda0, load_factors,
           history, newton_rtol, newton_atol, max_newton, linear_rtol,
           preconditioner, u0, return_info=False, _state=None):
  """The body of `solve_plasticity`, its arguments checked.  `_state`: a dict
  that receives what the path adjoint needs (the operator, the mask, the
  preconditioner, the mass apply and per entry (u_k, h_{k-1}, s_k))."""
  who = 'solve_plasticity'
  path = _load_path(load_factors)
  st = _setup(
      who, mesh, body_force, boundary_conditions, lambda0, preconditioner,
      lambda fespace, mask: fespace.plasticity_operator(
          mask, lame_lambda=lame_lambda, lame_mu=lame_mu,
          yield_stress=yield_stress, hardening_modulus=hardening_modulus,
          density=density),
      linear=lambda op: op.linear, u0=u0)
  op, M, u, lambda0 = st.op, st.M, st.u, st.lambda0
  f_ext = st.load * st.keep
  if history is None:
    committed = op.virgin_history()
  else:
    committed = torch.as_tensor(history, dtype=mesh.dtype,
                                device=mesh.device)
    if tuple(committed.shape) != op.history_shape():
      raise ValueError(f'history: shape {tuple(committed.shape)}; expected '
                       f'{op.history_shape()}')
    committed = committed.contiguous()   # read only: never written here

  entries = []
  for k, scale in enumerate(path, start=1):
    u = torch.where(st.fixed, scale * st.u_D, u)
    rec = dict(factor=scale, residual_norms=[], step_lengths=[],
               cg_iterations=[], plastic_points=0, status='running')
    entries.append(rec)

    def where(it, note=None):
      entry = f'entry {k} of {len(path)} of the load path'
      return (f'{entry} (factor {scale:g}, {note})' if it is None
              else f'{entry} (factor {scale:g}), Newton iteration {it}')

    def evaluate(v):
      """(linearisation at v from the committed history, r = keep (R(v) -
      scale f_ext), |r|)."""
      lin = op.linearize(v, committed, lambda0)   # the mask is applied
      r = lin.residual - scale * f_ext
      return lin, r, float(torch.linalg.vector_norm(r))

    u, lin, _ = newton_cg(
        evaluate, lambda lin: op.tangent(lin, lambda0).apply, u, M,
        newton_rtol=newton_rtol, newton_atol=newton_atol,
        max_newton=max_newton, linear_rtol=linear_rtol, who=who, where=where,
        breakdown_hint=('without hardening the tangent is only semi-definite '
                        'at a limit load'),
        check_every=_check_every(M), rec=rec)
    # the accepted state's launch already formed its history: commit it
    if _state is not None:
      _state.setdefault('entries', []).append((u, committed, scale))
    committed = lin.history
    rec['plastic_points'] = lin.num_plastic()
  if _state is not None:
    fespace = st.fespace
    _state.update(op=op, keep=st.keep, M=M, lambda0=lambda0,
                  Bf=lambda x: fespace.helmholtz_operator(None).apply(
                      x.contiguous(), 1.0, 0.0))
  if return_info:
    return u, committed, {
        'load_path': entries, 'status': 'converged',
        'num_newton': sum(len(s['step_lengths']) for s in entries),
        'num_cg': sum(sum(s['cg_iterations']) for s in entries)}
  return u, committed


__all__ = ['BCType', 'solve_plasticity']
