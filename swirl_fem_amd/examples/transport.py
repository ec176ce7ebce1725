"""Time-dependent scalar transport by BDFk/EXTk.

    dT/dt + u . grad T - div(k grad T) = s   in the mesh,

with the boundary conditions, the discretisation and the diffusivity forms of
`solve_helmholtz` (examples/helmholtz.py): Gauss rule with
`order + (ndim+1)//2` points, the two-grid operator, the plain Galerkin
convective form C(u)[i,j] = sum_q W_q phi_i(q) u_q . grad phi_j(q) without
stabilisation.  Boundary data are fixed in time; the velocity u is given per
time level (for example the velocities `StokesSEM.stokes_one_step` returns).

One step of order k (`time_order`), the splitting `stokes_one_step` uses for
the velocity: the convective term is extrapolated from the last k levels, the
time derivative is the BDF of order k and diffusion is implicit,

    ((bdf[-1] / dt) B + A_k + Robin) T_new
        = B s - (1 / dt) B sum_j bdf[j] T_j - sum_j ext[j] C(u_j) T_j
          + Neumann / Robin covectors,

with bdf = bdfk_coeffs(k) and ext = extk_coeffs(k - 1) over the levels oldest
first.  The right-hand side is formed in one `operators.TransportRhs.apply`
(one fused kernel over all levels); the system is the symmetric
Helmholtz solve with lambda0 = bdf[-1] / dt: CG with Jacobi or p-multigrid,
the Dirichlet lift and the periodic wrapping exactly as in `solve_helmholtz`.

`ScalarTransport.create(..., differentiable=True)` makes a stepper whose
steps take part in autograd: gradients reach the scalar levels,
the velocities, the source and the diffusivity.  The right-hand side goes
through the differentiable `TransportRhs.apply`; the implicit half is one
autograd node whose backward is one more CG solve on the same (symmetric)
system and, for the diffusivity, one sensitivity launch.

Because sum(bdf) = 0 and sum(ext) = 1, a fixed point of the stepper with
constant u and s is the discrete solution of
`solve_helmholtz(mesh, s, bcs, lambda0=0, velocity=u, diffusivity=k)`.
"""

from __future__ import annotations

import dataclasses
from typing import Mapping, Tuple

import torch

from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import NodeType
from swirl_fem_amd.core.interpolation import Quadrature1D
from swirl_fem_amd.core.mesh import Mesh
from swirl_fem_amd.examples.helmholtz import _nodal_values
from swirl_fem_amd.examples.poisson import BCType
from swirl_fem_amd.examples.poisson import BCValue
from swirl_fem_amd.linalg.cg import cg
from swirl_fem_amd.navier_stokes.navier_stokes import bdfk_coeffs
from swirl_fem_amd.navier_stokes.navier_stokes import extk_coeffs

# pylint: disable=invalid-name


def _no_grad_inputs(*values):
  for v in values:
    if isinstance(v, (list, tuple)):
      _no_grad_inputs(*v)
    elif isinstance(v, torch.Tensor) and v.requires_grad:
      raise NotImplementedError('autograd through ScalarTransport steps: '
                                'detach the inputs')


class _ImplicitHalf(torch.autograd.Function):
  """T_new = u_D + K^-1 keep (rhs - lift(k) + covector) of one step, with K =
  keep (lambda0 B + A_k + Robin) keep symmetric.  Backward: K lam = keep
  T_new_bar by the same CG, rhs_bar = lam (through the symmetric exchange on a
  periodic mesh) and k_bar = -d(lam . A_k T_new)/dk with the full T_new, which
  covers the lift."""

  @staticmethod
  def forward(ctx, st, lambda0, solve, info_out, rhs, diffusivity):
    T_new, info = st._implicit(rhs.detach(), lambda0, **solve)
    info_out.update(info)
    ctx.st, ctx.lambda0, ctx.solve = st, lambda0, solve
    ctx.info_out = info_out
    ctx.save_for_backward(T_new)
    return T_new

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, g):
    st, lambda0, solve = ctx.st, ctx.lambda0, ctx.solve
    T_new, = ctx.saved_tensors
    A, M, _ = st._system(lambda0, solve['preconditioner'])
    g = g.contiguous()
    if st.periodic:
      g = st.mesh.exchange(g)
    lam, info = cg(A, g * st.keep, tol=solve['rtol'], atol=solve['atol'], M=M)
    ctx.info_out.setdefault('adjoint', []).append(info)
    rhs_bar = st.mesh.exchange(lam) if ctx.needs_input_grad[4] else None
    k_bar = None
    if ctx.needs_input_grad[5]:
      k_bar = -st.full.sensitivity(T_new, lam, lambda0, 1.0,
                                   want=(True, False, False))[0]
    return None, None, None, None, rhs_bar, k_bar


@dataclasses.dataclass(eq=False)
class ScalarTransport:
  """The operators of a transport problem, built once; see the module."""
  mesh: Mesh
  fespace: FiniteElementSpace
  op: object                  # masked (lambda0 B + A_k)
  full: object                # the same without the mask (the lift)
  rhs_op: object              # operators.TransportRhs
  rmass: list                 # Robin terms, masked
  rfull: list                 # Robin terms, whole
  u_D: torch.Tensor           # Dirichlet values, 0 elsewhere
  keep: torch.Tensor          # 1 on the unknowns
  covector: torch.Tensor | None   # Neumann + Robin data
  has_dirichlet: bool
  periodic: bool
  differentiable: bool = False
  diffusivity: object = None  # the caller's tensor (differentiable only)
  _cache: dict = dataclasses.field(default_factory=dict, repr=False)

  @classmethod
  def create(cls, mesh: Mesh,
             boundary_conditions: Mapping[str, Tuple[BCType, BCValue]], *,
             diffusivity=None, differentiable=False) -> 'ScalarTransport':
    """`boundary_conditions` and `diffusivity`: as in `solve_helmholtz`.
    `differentiable`: steps propagate gradients to `Ts`, `us`, `source` and
    to a `diffusivity` tensor that requires grad (a scalar, (E,) or per
    point); without it such inputs are refused."""
    if mesh.axis_name is not None or mesh.neighbor_plan is not None:
      raise NotImplementedError('ScalarTransport on a partitioned mesh')
    if mesh._cache.get('replicas', 1) > 1:
      raise NotImplementedError('ScalarTransport on an ensemble '
                                '(Mesh.replicate)')
    kept = None
    if differentiable:
      if isinstance(diffusivity, torch.Tensor) and diffusivity.requires_grad:
        gi = mesh.exchange_gather_indices
        if gi is not None and gi.numel() > 0:
          raise NotImplementedError('a diffusivity that requires grad on a '
                                    'mesh with periodic images')
        # the operators hold its value; steps return its gradient
        kept, diffusivity = diffusivity, diffusivity.detach()
    else:
      _no_grad_inputs(diffusivity)
    from swirl_fem_amd.core import operators
    quadrature = Quadrature1D.create(
        num_points=mesh.order + (mesh.ndim + 1) // 2,
        quadrature_type=NodeType.GAUSS_LEGENDRE)
    fespace = FiniteElementSpace.create(mesh, quadrature)
    dtype, device = fespace.dtype, fespace.device
    rhs_op = operators.TransportRhs.create(fespace)

    dirichlet = torch.zeros(mesh.num_nodes, dtype=torch.bool, device=device)
    u_D = torch.zeros(mesh.num_nodes, dtype=dtype, device=device)
    neumann, robin = [], []
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
          raise ValueError(f'a ROBIN value is a pair (alpha, g); got '
                           f'{value!r} on {group!r}')
        robin.append((group, value[0], value[1]))
      else:
        raise ValueError(f'unsupported boundary condition type {bctype!r} on '
                         f'{group!r}: DIRICHLET, NEUMANN or ROBIN')
    has_dirichlet = bool(dirichlet.any())
    gi = mesh.exchange_gather_indices
    periodic = gi is not None and gi.numel() > 0
    keep = (~dirichlet).to(dtype)
    if periodic:
      ids = torch.arange(mesh.num_nodes, device=device)
      master = (mesh.node_indices.to(ids.dtype) == ids).to(dtype)
      u_D = mesh.exchange(u_D * master)        # one value per periodic class
      keep = keep * master
    mask = dirichlet if has_dirichlet else None
    rmass = [fespace.boundary_mass(g, a, mask) for g, a, _ in robin]
    rfull = ([fespace.boundary_mass(g, a) for g, a, _ in robin]
             if has_dirichlet else rmass)
    op = fespace.helmholtz_operator(mask, diffusivity=diffusivity)
    full = (fespace.helmholtz_operator(None, diffusivity=diffusivity)
            if has_dirichlet else op)
    covector = None
    for group, g in neumann + [(grp, g) for grp, _, g in robin]:
      c = fespace.boundary_covector(group, g)
      covector = c if covector is None else covector + c
    return cls(mesh=mesh, fespace=fespace, op=op, full=full, rhs_op=rhs_op,
               rmass=rmass, rfull=rfull, u_D=u_D, keep=keep,
               covector=covector, has_dirichlet=has_dirichlet,
               periodic=periodic, differentiable=bool(differentiable),
               diffusivity=kept)

  # what depends on lambda0 = bdf[-1] / dt only: kept per value
  def _system(self, lambda0, preconditioner):
    key = ('system', lambda0, preconditioner)
    if key in self._cache:
      return self._cache[key]
    op, rmass, mesh, keep = self.op, self.rmass, self.mesh, self.keep

    def K(u):
      out = op.apply(u, lambda0, 1.0)
      for r in rmass:
        r.apply(u, 1.0, out=out)
      return out
    A = K
    if self.periodic:
      A = lambda x: mesh.exchange(K(mesh.exchange(x))) * keep
    M = None
    if preconditioner == 'jacobi':
      from swirl_fem_amd.linalg.jacobi import JacobiPreconditioner
      if rmass:
        diag = op.diagonal(lambda0, 1.0)
        for r in rmass:
          diag = diag + r.diagonal()
        M = JacobiPreconditioner(diag)
      else:
        M = JacobiPreconditioner(op, lambda0, 1.0)
    elif preconditioner == 'pmg':
      from swirl_fem_amd.linalg.pmg import PMultigridPreconditioner
      M = PMultigridPreconditioner(
          op, lambda0, 1.0,
          boundary_terms=[(r, 1.0) for r in rmass] or None)
    lift = None
    if self.has_dirichlet:
      lift = self.full.apply(self.u_D, lambda0, 1.0)
      for r in self.rfull:
        r.apply(self.u_D, 1.0, out=lift)
    self._cache[key] = (A, M, lift)
    return self._cache[key]

  def _source(self, source):
    if source is None:
      return None
    fes, mesh = self.fespace, self.mesh
    s = torch.as_tensor(source, dtype=fes.dtype, device=fes.device)
    if s.dim() == 0:
      nq = fes.quadrature.num_points ** mesh.ndim
      return s.expand(mesh.num_elements, nq).contiguous()
    return s

  def step(self, Ts, us, dt, time_order, source=None, *, rtol=1e-8, atol=0.0,
           preconditioner=None, return_info=False):
    """One BDF/EXT step of order `time_order` (1..3).

    `Ts`: the last `time_order` (or more) scalar levels (N,), oldest first;
    `us`: the velocities of those levels, each nodal (N, d) in any strides, a
    (d,) constant, (E, Q^d, d) values at the quadrature points or None (no
    convection at that level).  `source`: None, a scalar, nodal (N,) or
    (E, Q^d).  `preconditioner`: None, 'jacobi' or 'pmg' (None on a mesh with
    periodic images).  Returns T at the new level (and CG's info)."""
    if time_order not in (1, 2, 3):
      raise ValueError(f'time_order={time_order!r} outside 1..3')
    if preconditioner not in (None, 'jacobi', 'pmg'):
      raise ValueError(f'unknown preconditioner {preconditioner!r}')
    if len(Ts) < time_order or len(us) < time_order:
      raise ValueError(f'time_order={time_order} needs {time_order} levels: '
                       f'got {len(Ts)} scalars and {len(us)} velocities')
    if not float(dt) > 0.0:
      raise ValueError(f'dt={dt!r} must be positive')
    if not self.differentiable:
      _no_grad_inputs(list(Ts), list(us), source)
    if self.periodic and preconditioner is not None:
      raise NotImplementedError(f'preconditioner={preconditioner!r} on a '
                                'mesh with periodic images')
    k, dt = int(time_order), float(dt)
    Ts, us = list(Ts)[-k:], list(us)[-k:]
    bdf = bdfk_coeffs(k)
    ext = extk_coeffs(k - 1)
    lambda0 = float(bdf[-1]) / dt
    levels = [(T, u, -float(bdf[j]) / dt, -float(ext[j]))
              for j, (T, u) in enumerate(zip(Ts, us))]
    rhs = self.rhs_op.apply(levels, self._source(source))
    solve = dict(rtol=rtol, atol=atol, preconditioner=preconditioner)
    from swirl_fem_amd.core import autodiff
    if self.differentiable and autodiff.needs_grad(rhs, self.diffusivity):
      info = {}
      T_new = _ImplicitHalf.apply(self, lambda0, solve, info, rhs,
                                  self.diffusivity)
    else:
      T_new, info = self._implicit(rhs, lambda0, **solve)
    return (T_new, info) if return_info else T_new

  def _implicit(self, rhs, lambda0, rtol, atol, preconditioner):
    """The implicit half of a step from the assembled right-hand side."""
    A, M, lift = self._system(lambda0, preconditioner)
    if lift is not None:
      rhs = rhs - lift
    rhs = self.mesh.exchange(rhs)
    if self.covector is not None:
      rhs = rhs + self.covector
    w, info = cg(A, rhs * self.keep, tol=rtol, atol=atol, M=M)
    if self.periodic:
      w = self.mesh.exchange(w)
    return w + self.u_D, info

  def run(self, T0, velocity, dt, steps, time_order, source=None, **kwargs):
    """`steps` steps from `T0` (N,), the order ramping 1, 2, ...,
    `time_order` over the first steps.  `velocity`: one value in a form
    `step` takes, or a callable step_index -> velocity of that time level
    (index 0 is the level of `T0`).  Returns the last level."""
    if time_order not in (1, 2, 3):
      raise ValueError(f'time_order={time_order!r} outside 1..3')
    kwargs.pop('return_info', None)
    at = velocity if callable(velocity) and not isinstance(
        velocity, torch.Tensor) else (lambda n: velocity)
    Ts = [torch.as_tensor(T0, dtype=self.fespace.dtype,
                          device=self.fespace.device)]
    us = [at(0)]
    for n in range(int(steps)):
      k = min(n + 1, time_order)
      Ts.append(self.step(Ts, us, dt, k, source, **kwargs))
      us.append(at(n + 1))
      Ts, us = Ts[-time_order:], us[-time_order:]
    return Ts[-1]


__all__ = ['BCType', 'ScalarTransport']
