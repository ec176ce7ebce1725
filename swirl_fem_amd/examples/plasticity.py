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

With `hardening_modulus = 0` (perfect plasticity) the tangent is only positive
semi-definite once a mechanism has formed: at a limit load CG may break down
or Newton may stall.  Either is reported as a RuntimeError that names the entry
and the iteration; nothing is retried.
"""

from __future__ import annotations

import math
from typing import Mapping, Tuple

import torch

from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import NodeType
from swirl_fem_amd.core.interpolation import Quadrature1D
from swirl_fem_amd.core.mesh import Mesh
from swirl_fem_amd.examples.elasticity import _boundary_data
from swirl_fem_amd.examples.elasticity import _check_every
from swirl_fem_amd.examples.elasticity import _check_mesh
from swirl_fem_amd.examples.elasticity import _load_vector
from swirl_fem_amd.examples.elasticity import _requires_grad
from swirl_fem_amd.examples.hyperelasticity import ARMIJO
from swirl_fem_amd.examples.hyperelasticity import LINE_SEARCH_HALVINGS
from swirl_fem_amd.examples.poisson import BCType
from swirl_fem_amd.linalg.cg import cg

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


def solve_plasticity(mesh: Mesh, body_force,
                     boundary_conditions: Mapping[str, Tuple[BCType, object]],
                     *, lame_lambda, lame_mu, yield_stress,
                     hardening_modulus=0.0, density=None,
                     lambda0: float = 0.0, load_factors=(1.0,), history=None,
                     newton_rtol: float = 1e-8, newton_atol: float = 0.0,
                     max_newton: int = 25, linear_rtol: float = 1e-6,
                     preconditioner=None, u0=None, return_info: bool = False):
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

  Partitioned meshes, ensembles, periodic images, ROBIN conditions and inputs
  that require grad are refused; 2D is plane strain."""
  who = 'solve_plasticity'
  if isinstance(preconditioner, str) and preconditioner == 'pmg':
    raise NotImplementedError(
        "preconditioner='pmg' for elasticity: the V-cycle of that name is "
        'built for the scalar operator; pass preconditioner='
        'linalg.pmg_elasticity.ElasticityPMultigrid (or any callable '
        '(op, lambda0) -> M)')
  if not callable(preconditioner) and preconditioner not in (None, 'jacobi'):
    raise ValueError(f'unknown preconditioner {preconditioner!r}')
  path = _load_path(load_factors)
  if max_newton < 1:
    raise ValueError(f'max_newton must be at least 1, got {max_newton!r}')
  if _requires_grad(body_force, lame_lambda, lame_mu, density, yield_stress,
                    hardening_modulus, history, u0):
    raise NotImplementedError(
        f'autograd through {who}: the solve depends on the load path and is '
        'not differentiated; pass detached inputs')
  _check_mesh(mesh, who)
  d, N = mesh.ndim, mesh.num_nodes
  dtype = mesh.dtype
  lambda0 = float(lambda0)

  fixed, u_D, tractions = _boundary_data(mesh, boundary_conditions)
  has_fixed = bool(fixed.any())
  singular = ValueError(
      'lambda0 rho = 0 everywhere and no component of any node is fixed: the '
      'rigid-body modes are not removed (the problem is singular)')
  if lambda0 == 0.0 and not has_fixed:
    raise singular

  quadrature = Quadrature1D.create(
      num_points=mesh.order + (d + 1) // 2,
      quadrature_type=NodeType.GAUSS_LEGENDRE)
  fespace = FiniteElementSpace.create(mesh, quadrature)
  op = fespace.plasticity_operator(
      fixed if has_fixed else None, lame_lambda=lame_lambda, lame_mu=lame_mu,
      yield_stress=yield_stress, hardening_modulus=hardening_modulus,
      density=density)
  if not has_fixed and bool((torch.as_tensor(op.rho) == 0).all()):
    raise singular
  f_ext = _load_vector(fespace, body_force, tractions)
  keep = (~fixed).to(dtype)
  f_ext = f_ext * keep

  M = None
  if preconditioner == 'jacobi':
    from swirl_fem_amd.linalg.jacobi import JacobiPreconditioner
    M = JacobiPreconditioner(op.linear.diagonal(lambda0).reshape(-1))
  elif callable(preconditioner):
    M = preconditioner(op.linear, lambda0)

  if u0 is None:
    u = torch.zeros((N, d), dtype=dtype, device=mesh.device)
  else:
    u = torch.as_tensor(u0, dtype=dtype, device=mesh.device)
    if tuple(u.shape) != (N, d):
      raise ValueError(f'u0: shape {tuple(u.shape)}; expected ({N}, {d})')
    u = u.clone()
  if history is None:
    committed = op.virgin_history()
  else:
    committed = torch.as_tensor(history, dtype=dtype, device=mesh.device)
    if tuple(committed.shape) != op.history_shape():
      raise ValueError(f'history: shape {tuple(committed.shape)}; expected '
                       f'{op.history_shape()}')
    committed = committed.contiguous()   # read only: never written here

  entries = []
  for k, scale in enumerate(path, start=1):
    u = torch.where(fixed, scale * u_D, u)
    rec = dict(factor=scale, residual_norms=[], step_lengths=[],
               cg_iterations=[], plastic_points=0, status='running')
    entries.append(rec)
    where = lambda it: (f'entry {k} of {len(path)} of the load path (factor '
                        f'{scale:g}), Newton iteration {it}')

    def evaluate(v):
      """(linearisation at v from the committed history, r = keep (R(v) -
      scale f_ext), |r|)."""
      lin = op.linearize(v, committed, lambda0)   # the mask is applied
      r = lin.residual - scale * f_ext
      return lin, r, float(torch.linalg.vector_norm(r))

    lin, r, rnorm = evaluate(u)
    if not math.isfinite(rnorm):
      raise RuntimeError(f'{who}: the residual is not finite at the start of '
                         f'{where(0)}')
    rec['residual_norms'].append(rnorm)
    target = max(newton_rtol * rnorm, newton_atol)
    it = 0
    while rnorm > target:
      if it == max_newton:
        rec['status'] = 'max_newton'
        raise RuntimeError(
            f'{who}: no convergence within max_newton = {max_newton} '
            f'iterations in entry {k} of {len(path)} of the load path '
            f'(factor {scale:g}, |r| = {rnorm:.3e}, target {target:.3e})')
      it += 1
      T = op.tangent(lin, lambda0)
      A = lambda x: T.apply(x.view(N, d)).reshape(-1)
      dw, cg_info = cg(A, (-r).reshape(-1).contiguous(), tol=linear_rtol,
                       M=M, check_every=_check_every(M))
      rec['cg_iterations'].append(int(cg_info['num_iterations']))
      if str(cg_info['status']).startswith('breakdown'):
        rec['status'] = 'cg_' + cg_info['status']
        raise RuntimeError(
            f'{who}: CG broke down ({cg_info["status"]}; without hardening '
            f'the tangent is only semi-definite at a limit load) in '
            f'{where(it)}')
      dw = dw.view(N, d)
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
    # the accepted state's launch already formed its history: commit it
    committed = lin.history
    rec['plastic_points'] = lin.num_plastic()
    rec['status'] = 'converged'
  if return_info:
    return u, committed, {
        'load_path': entries, 'status': 'converged',
        'num_newton': sum(len(s['step_lengths']) for s in entries),
        'num_cg': sum(sum(s['cg_iterations']) for s in entries)}
  return u, committed


__all__ = ['BCType', 'solve_plasticity']
