"""Helmholtz / Poisson solves with inhomogeneous Dirichlet, Neumann and Robin
data, variable coefficients and an optional advective term.

    lambda0 c u + b . grad u - lambda1 div(k grad u) = f   in the mesh,
    u = g_D on Dirichlet groups,   k du/dn = g_N on Neumann groups,
    k du/dn + alpha u = g_R on Robin groups (alpha >= 0),
    k du/dn = 0 on the rest of the boundary,

with the diffusivity k > 0 and the reaction coefficient c >= 0 (both 1 by
default: then the equation is lambda0 u - lambda1 lap u = f) and the
advecting velocity b (default: none).  Only the diffusive term is integrated
by parts, so Neumann and Robin data stay the flux k du/dn with or without b.
The advective term is the plain Galerkin convective form
C_b[i,j] = sum_q W_q phi_i(q) b_q . grad phi_j(q) without stabilisation: the
mesh has to resolve the boundary layers of an advection-dominated problem.
With a velocity the system is not symmetric and is solved by right-
preconditioned BiCGStab (`linalg/bicgstab.py`) instead of CG.

The boundary data the reference's `solve_poisson` docstring promises and
leaves as a TODO (swirl_fem/examples/poisson.py:79-90); `solve_poisson`
itself keeps the reference's homogeneous-only contract.  Quadrature, forms,
operators and preconditioners are those of `examples/poisson.py`.

Method: lift and solve for the homogeneous remainder.  u_D holds the Dirichlet
values on the Dirichlet nodes and 0 elsewhere; w solves the masked system

    K w = mask (B f + lambda1 b_N - (lambda0 B_c + lambda1 A_k) u_D),

with K the operator of `solve_poisson` (Dirichlet rows and columns removed)
and b_N the sum of `FiniteElementSpace.boundary_covector(group, g_N)` over the
Neumann groups; u = w + u_D.  (lambda0 B_c + lambda1 A_k) u_D is applied by an
operator without a mask, so that it reads the Dirichlet values.  B f keeps the
plain mass matrix: the coefficients act on u only.

A Robin group adds lambda1 <alpha u, v> to the operator
(`FiniteElementSpace.boundary_mass`, masked like K: where it shares nodes with
a Dirichlet group, Dirichlet wins), lambda1 <g_R, v> to the right-hand side
and -lambda1 M_R u_D (unmasked) to the lift.  The Jacobi diagonal and every
p-multigrid level carry the term.

On a mesh with periodic images the unknowns are the lowest-numbered node of
each class: K = R QQ^T A QQ^T R^T with R the restriction to those nodes
(QQ^T copies a class's only nonzero value to all its images), which keeps K
symmetric for CG; the result is copied back to the images.

Differentiation.  `solve_helmholtz` is differentiable with
respect to `forcing` and to tensor-valued `diffusivity`, `reaction` and
`velocity` that require grad.  With u_bar the cotangent of u, backward solves
the transposed masked system K^T lam = mask u_bar with the forward solve's
solver, tolerances and preconditioner (CG without a velocity, BiCGStab on the
transposed operator with one), then forcing_bar = B lam and theta_bar =
-d(lam . A(theta) u)/d theta with the full u = w + u_D (`op.sensitivity`),
which covers the lift.  Neumann and Robin data are the flux k du/dn, so the
right-hand side carries no further dependence on k.
"""

from __future__ import annotations

from typing import Mapping, Tuple

import torch

from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.fespace import grad
from swirl_fem_amd.core.interpolation import NodeType
from swirl_fem_amd.core.interpolation import Quadrature1D
from swirl_fem_amd.core.mesh import Mesh
from swirl_fem_amd.examples.poisson import BCType
from swirl_fem_amd.examples.poisson import BCValue
from swirl_fem_amd.linalg.bicgstab import bicgstab
from swirl_fem_amd.linalg.cg import cg

# pylint: disable=invalid-name


def _nodal_values(mesh: Mesh, value, dtype, device) -> torch.Tensor:
  """A `BCValue` as `(N,)` nodal values: a scalar, an `(N,)` array, or a
  callable on the `(N, d)` node coordinates."""
  if callable(value):
    value = value(mesh.node_coords)
  v = torch.as_tensor(value, dtype=dtype, device=device)
  if v.dim() == 0:
    return v.expand(mesh.num_nodes)
  if tuple(v.shape) != (mesh.num_nodes,):
    raise ValueError(f'a Dirichlet value must be a scalar, ({mesh.num_nodes},) '
                     f'nodal values or a callable; got {tuple(v.shape)}')
  return v


def _requires_grad(*values) -> bool:
  return torch.is_grad_enabled() and any(
      isinstance(v, torch.Tensor) and v.requires_grad for v in values)


def _detached(v):
  return v.detach() if isinstance(v, torch.Tensor) else v


def _point_covector(mesh, point_sources, dtype, device):
  """`sum_m s_m phi_i(x_m)` as an `(N,)` vector, periodic images summed."""
  from swirl_fem_amd.core.points import PointEvaluator
  if not (isinstance(point_sources, (tuple, list)) and
          len(point_sources) == 2):
    raise ValueError('point_sources is a pair (points, strengths)')
  points, strengths = point_sources
  points = torch.as_tensor(points, dtype=dtype, device=device)
  strengths = torch.as_tensor(strengths, dtype=dtype, device=device)
  if strengths.dim() != 1 or points.dim() != 2 or (
      points.shape[0] != strengths.shape[0]):
    raise ValueError('point_sources: expected points (M, d) and strengths '
                     f'(M,), got {tuple(points.shape)} and '
                     f'{tuple(strengths.shape)}')
  ev = PointEvaluator.create(mesh, points)
  return mesh.exchange(ev.transpose(strengths.detach()))


class _HelmholtzSolve(torch.autograd.Function):
  """`_solve` as one autograd node: the adjoint solve and the coefficient
  sensitivities in `backward`."""

  @staticmethod
  def forward(ctx, forcing, diffusivity, reaction, velocity, mesh,
              boundary_conditions, kwargs, holder):
    state = {}
    u, info = _solve(mesh, _detached(forcing), boundary_conditions,
                     diffusivity=_detached(diffusivity),
                     reaction=_detached(reaction),
                     velocity=_detached(velocity), return_info=True,
                     _state=state, **kwargs)
    holder['info'] = info
    ctx.state = state
    ctx.save_for_backward(u)
    ctx.like = [(v.dtype, v.device) if isinstance(v, torch.Tensor) else None
                for v in (forcing, diffusivity, reaction, velocity)]
    return u

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, u_bar):
    st = ctx.state
    l0, l1 = st['lambda0'], st['lambda1']
    op, keep = st['op'], st['keep']
    rhs = (u_bar.detach().to(keep.dtype) * keep).contiguous()
    if st['advection']:
      if st['rmass']:
        At = lambda x: st['add_robin'](x, op.apply_transpose(x, l0, l1))
      else:
        At = op.linear_operator(l0, l1, transpose=True)
      lam, info = bicgstab(At, rhs, tol=st['rtol'], atol=st['atol'],
                           M=st['M'])
    else:
      lam, info = cg(st['K'], rhs, tol=st['rtol'], atol=st['atol'],
                     M=st['M'])
    st['adjoint_info'] = info
    need = ctx.needs_input_grad
    grads = [None, None, None, None]
    if need[0]:
      grads[0] = st['Bf'](lam)
    if any(need[1:4]):
      sens = op.sensitivity(ctx.saved_tensors[0], lam, l0, l1,
                            want=tuple(need[1:4]))
      for n, g in enumerate(sens):
        if need[1 + n] and g is not None:
          grads[1 + n] = -g
    for n, like in enumerate(ctx.like):
      if grads[n] is not None and like is not None:
        grads[n] = grads[n].to(dtype=like[0], device=like[1])
    return (*grads, None, None, None, None)


def solve_helmholtz(mesh: Mesh, forcing,
                    boundary_conditions: Mapping[str, Tuple[BCType, BCValue]],
                    *, lambda0: float = 0.0, lambda1: float = 1.0,
                    rtol: float = 1e-5, atol: float = 0.,
                    return_info: bool = False, preconditioner=None,
                    diffusivity=None, reaction=None, velocity=None,
                    point_sources=None):
  """Solves `lambda0 c u + b . grad u - lambda1 div(k grad u) = forcing` with
  boundary data.

  `point_sources`: None, or `(points (M, d), strengths (M,))`: the Dirac loads
  `sum_m strengths[m] delta(x - points[m])` added to the forcing.  The points
  are located once (`core.points.PointEvaluator`) and the covector
  `ev.transpose(strengths)` joins the right-hand side with the Neumann
  covectors (before lift and mask, summed over periodic images); a point
  outside the mesh contributes nothing.  `strengths` that require grad raise
  NotImplementedError.

  `velocity` b: None (no advective term: the symmetric solve by CG), a `(d,)`
  constant, an `(E, d)` tensor, an `(E, Q^d, d)` tensor at the quadrature
  points of the solve's rule (`FiniteElementSpace.to_quadrature` makes one
  from nodal values) or a callable from `(M, d)` coordinates to `(M, d)`
  values.  The solve then runs BiCGStab (`info` is its), `preconditioner` is
  None or 'jacobi', and it needs the fused operator and a mesh without
  partitions.  A velocity does not remove the constant nullspace.

  `diffusivity` k (> 0) and `reaction` c (>= 0): None (= 1), a scalar, an
  `(E,)` tensor of per-element values, an `(E, Q^d)` tensor at the quadrature
  points of the solve's rule (`FiniteElementSpace.quad_coords` order) or a
  callable from `(M, d)` coordinates to `(M,)` values, evaluated once there
  (`FiniteElementSpace.helmholtz_operator`).  They need the fused operator
  and a mesh without partitions.

  `boundary_conditions` maps physical group names to `(BCType, BCValue)`:
  DIRICHLET sets u = value on the group's nodes, NEUMANN sets the flux
  k du/dn = value (outward normal) on its facets, ROBIN with the value
  `(alpha, g)` sets k du/dn + alpha u = g there (alpha >= 0).  A value is a scalar, an `(N,)` nodal
  array (only the group's nodes are read) or a callable on coordinates:
  `(N, d)` node coordinates for Dirichlet data, `(M, d)` facet quadrature
  points for Neumann and Robin data (alpha and g alike; alpha may also be
  given at the `(F, Q^(d-1))` points of `boundary_points`).  Where Dirichlet
  groups share a node, the later group in the mapping sets its value.
  `forcing` is nodal.

  `preconditioner`: None, 'jacobi' or 'pmg', as in `solve_poisson` (on a
  mesh without periodic images).  `rtol` is relative to the norm of the
  lifted right-hand side; `info` is CG's (BiCGStab's with a velocity).

  Autograd: the result is differentiable with respect to `forcing` and to
  `diffusivity`, `reaction` and `velocity` given as tensors that require grad
  (any of their tensor forms; the gradient has the form passed in).  Backward
  is one adjoint solve with the forward solve's solver, `rtol`, `atol` and
  `preconditioner` plus the sensitivity kernel (`op.sensitivity`).  Gradients
  with respect to boundary data (Dirichlet, Neumann, Robin values) and
  through callables are not propagated, nor are second derivatives.  It
  needs the fused operator and a mesh without periodic images
  (NotImplementedError otherwise).  When nothing requires grad the solve
  runs exactly as without this feature and builds no autograd node.
  """
  kwargs = dict(lambda0=lambda0, lambda1=lambda1, rtol=rtol, atol=atol,
                preconditioner=preconditioner)
  if point_sources is not None:
    if _requires_grad(point_sources[1]):
      raise NotImplementedError('gradients of solve_helmholtz with respect to '
                                'point source strengths')
    kwargs['point_sources'] = point_sources
  if not _requires_grad(forcing, diffusivity, reaction, velocity):
    return _solve(mesh, forcing, boundary_conditions, diffusivity=diffusivity,
                  reaction=reaction, velocity=velocity,
                  return_info=return_info, **kwargs)
  gi = mesh.exchange_gather_indices
  if gi is not None and gi.numel() > 0:
    raise NotImplementedError('gradients of solve_helmholtz on a mesh with '
                              'periodic images')
  holder = {}
  u = _HelmholtzSolve.apply(forcing, diffusivity, reaction, velocity, mesh,
                            boundary_conditions, kwargs, holder)
  return (u, holder['info']) if return_info else u


def _solve(mesh: Mesh, forcing,
           boundary_conditions: Mapping[str, Tuple[BCType, BCValue]],
           *, lambda0: float = 0.0, lambda1: float = 1.0,
           rtol: float = 1e-5, atol: float = 0.,
           return_info: bool = False, preconditioner=None,
           diffusivity=None, reaction=None, velocity=None, _state=None,
           point_sources=None):
  """The body of `solve_helmholtz`.  `_state`: a dict that receives what the
  adjoint solve needs (the operators, the mask, the preconditioner)."""
  if preconditioner not in (None, 'jacobi', 'pmg'):
    raise ValueError(f'unknown preconditioner {preconditioner!r}')
  if mesh.axis_name is not None or mesh.neighbor_plan is not None:
    raise NotImplementedError('solve_helmholtz on a partitioned mesh')
  if mesh._cache.get('replicas', 1) > 1:
    raise NotImplementedError('solve_helmholtz on an ensemble '
                              '(Mesh.replicate)')
  advection = velocity is not None
  if advection and preconditioner == 'pmg':
    raise NotImplementedError("preconditioner='pmg' with a velocity: the "
                              'V-cycle is built for the symmetric operator')
  lambda0, lambda1 = float(lambda0), float(lambda1)
  quadrature = Quadrature1D.create(
      num_points=mesh.order + (mesh.ndim + 1) // 2,
      quadrature_type=NodeType.GAUSS_LEGENDRE)
  fespace = FiniteElementSpace.create(mesh, quadrature)
  dtype, device = fespace.dtype, fespace.device

  dirichlet = torch.zeros(mesh.num_nodes, dtype=torch.bool, device=device)
  u_D = torch.zeros(mesh.num_nodes, dtype=dtype, device=device)
  neumann = []
  robin = []
  for group, (bctype, value) in boundary_conditions.items():
    if bctype == BCType.DIRICHLET:
      if group not in mesh.physical_masks:
        raise KeyError(f'unknown physical group {group!r}')
      m = mesh.physical_masks[group]
      u_D = torch.where(m, _nodal_values(mesh, value, dtype, device), u_D)
      dirichlet = dirichlet | m
    elif bctype == BCType.NEUMANN:
      neumann.append((group, value))
    elif bctype is BCType.ROBIN:
      if not (isinstance(value, (tuple, list)) and len(value) == 2):
        raise ValueError(f'a ROBIN value is a pair (alpha, g); got {value!r} '
                         f'on {group!r}')
      alpha = value[0]
      if not callable(alpha) and torch.as_tensor(alpha).dim() == 0 and not (
          float(alpha) >= 0.0):
        raise ValueError(f'Robin alpha must be >= 0, got {alpha!r} on '
                         f'{group!r}')
      robin.append((group, alpha, value[1]))
    else:
      raise ValueError(f'unsupported boundary condition type {bctype!r} on '
                       f'{group!r}: DIRICHLET, NEUMANN or ROBIN')
  has_dirichlet = bool(dirichlet.any())
  singular = ValueError('lambda0 = 0 (or a reaction that is 0 everywhere) '
                        'with no Dirichlet node and no Robin alpha > 0: the '
                        'problem is singular (u is determined up to a '
                        'constant)')
  coefficients = diffusivity is not None or reaction is not None
  # a reaction that is 0 everywhere removes the mass term as lambda0 = 0 does
  # (a callable is decided once the operator has evaluated it)
  no_mass = lambda0 == 0.0 or (
      reaction is not None and not callable(reaction) and
      bool((torch.as_tensor(reaction) == 0).all()))
  if no_mass and not has_dirichlet and all(
      not callable(a) and torch.as_tensor(a).dim() == 0 and float(a) == 0.0
      for _, a, _ in robin):
    raise singular

  gi = mesh.exchange_gather_indices
  periodic = gi is not None and gi.numel() > 0
  keep = (~dirichlet).to(dtype)
  if periodic:
    if preconditioner is not None:
      raise NotImplementedError(f'preconditioner={preconditioner!r} on a mesh '
                                'with periodic images')
    ids = torch.arange(mesh.num_nodes, device=device)
    master = (mesh.node_indices.to(ids.dtype) == ids).to(dtype)
    u_D = mesh.exchange(u_D * master)        # one value per periodic class
    keep = keep * master

  # (lambda0 B + lambda1 A) with and without the Dirichlet rows
  from swirl_fem_amd.core import operators
  M = None
  mask = dirichlet if has_dirichlet else None
  # the Robin terms <alpha u, v>: masked (in K) and whole (for the lift)
  rmass = [fespace.boundary_mass(g, a, mask) for g, a, _ in robin]
  rfull = ([fespace.boundary_mass(g, a) for g, a, _ in robin]
           if has_dirichlet else rmass)
  robin_weight = sum(r.total_weight() for r in rmass)
  if no_mass and not has_dirichlet and not robin_weight > 0.0:
    raise singular

  def add_robin(u, out):
    for r in rmass:
      r.apply(u, lambda1, out=out)
    return out
  if (fespace.is_collocated and operators.supports_fused(fespace) is None) or (
      not fespace.is_collocated and
      operators.supports_two_grid(fespace) is None):
    if advection:
      # the masked operator with the advective term goes to BiCGStab, the
      # unmasked one lifts the Dirichlet data; B f takes the plain mass matrix
      op = fespace.helmholtz_operator(mask, diffusivity=diffusivity,
                                      reaction=reaction, velocity=velocity)
      full = (fespace.helmholtz_operator(None, diffusivity=diffusivity,
                                         reaction=reaction, velocity=velocity)
              if has_dirichlet else op)
      plain = fespace.helmholtz_operator(None)
    else:
      op = fespace.helmholtz_operator(mask, diffusivity=diffusivity,
                                      reaction=reaction)
      full = (fespace.helmholtz_operator(None, diffusivity=diffusivity,
                                         reaction=reaction)
              if has_dirichlet or not coefficients else op)
      # the right-hand side B f takes the plain mass matrix
      plain = fespace.helmholtz_operator(None) if coefficients else full
    if callable(reaction) and not no_mass:
      c = op.coefs[1][1]
      if bool((c == 0).all()) and not has_dirichlet and not robin_weight > 0:
        raise singular
    if rmass:
      K = lambda u: add_robin(u, op.apply(u, lambda0, lambda1))
    else:
      K = lambda u: op.apply(u, lambda0, lambda1)
    H = lambda u, l0, l1: full.apply(u, l0, l1)
    Bf = lambda u: plain.apply(u, 1.0, 0.0)
    if preconditioner == 'jacobi':
      from swirl_fem_amd.linalg.jacobi import JacobiPreconditioner
      if rmass:
        diag = op.diagonal(lambda0, lambda1)
        for r in rmass:
          diag = diag + lambda1 * r.diagonal()
        M = JacobiPreconditioner(diag)
      else:
        M = JacobiPreconditioner(op, lambda0, lambda1)
    elif preconditioner == 'pmg':
      from swirl_fem_amd.linalg.pmg import PMultigridPreconditioner
      M = PMultigridPreconditioner(
          op, lambda0, lambda1,
          boundary_terms=[(r, lambda1) for r in rmass] or None)
  elif preconditioner is not None:
    raise NotImplementedError(
        f"preconditioner={preconditioner!r} needs the fused operator: "
        f"{operators.supports_two_grid(fespace)}")
  elif advection:
    raise NotImplementedError(
        'a velocity needs the fused operator: '
        f'{operators.supports_two_grid(fespace)}')
  elif coefficients:
    raise NotImplementedError(
        'diffusivity / reaction need the fused operator: '
        f'{operators.supports_two_grid(fespace)}')
  elif _state is not None:
    raise NotImplementedError(
        'gradients of solve_helmholtz need the fused operator: '
        f'{operators.supports_two_grid(fespace)}')
  else:
    def l(u, v):
      return lambda x: u(x) * v(x)

    def a(u, v):
      return lambda x: torch.vdot(grad(u)(x), grad(v)(x))

    def H(u, l0, l1):
      uf = fespace.scalar_function(mesh.gather(u))
      v = fespace.scalar_function(None)
      out = torch.zeros_like(u)
      if l0 != 0.0:
        out = out + l0 * mesh.scatter(fespace.local_covector(l, (uf, v)))
      if l1 != 0.0:
        out = out + l1 * mesh.scatter(fespace.local_covector(a, (uf, v)))
      return out

    K = lambda u: add_robin(u, H(u, lambda0, lambda1)) * keep
    Bf = lambda u: H(u, 1.0, 0.0)

  forcing = torch.as_tensor(forcing, dtype=dtype, device=device)
  rhs = Bf(forcing)
  if has_dirichlet:
    rhs = rhs - H(u_D, lambda0, lambda1)
    for r in rfull:
      r.apply(u_D, -lambda1, out=rhs)
  rhs = mesh.exchange(rhs)
  for group, value in neumann:
    rhs = rhs + lambda1 * fespace.boundary_covector(group, value)
  for group, _, g in robin:
    rhs = rhs + lambda1 * fespace.boundary_covector(group, g)
  if point_sources is not None:
    rhs = rhs + _point_covector(mesh, point_sources, dtype, device)
  b = rhs * keep

  A = K
  if periodic:
    A = lambda x: mesh.exchange(K(mesh.exchange(x))) * keep
  if advection:
    w, info = bicgstab(A, b, tol=rtol, atol=atol, M=M)
  else:
    w, info = cg(A, b, tol=rtol, atol=atol, M=M)
  if periodic:
    w = mesh.exchange(w)
  u = w + u_D
  if _state is not None:
    _state.update(op=op, K=K, Bf=Bf, M=M, keep=keep, rmass=rmass,
                  add_robin=add_robin, advection=advection, lambda0=lambda0,
                  lambda1=lambda1, rtol=rtol, atol=atol)
  if return_info:
    return u, info
  return u


__all__ = ['BCType', 'solve_helmholtz']
