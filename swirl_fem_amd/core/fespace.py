"""Finite element space on a `Mesh`: q-functions, integration, operator action.

API of the reference `swirl_fem/core/fespace.py`: `NodalQFunction` family
:76-225, `grad` :233-241, `div` :244-248, `FiniteElementSpace.create` :306-348,
`scalar_function` :364-370, `vector_function` :372-379, `integrate` :381-403,
`local_covector` :405-471.

How it runs here
  * `create` gathers element coordinates and computes `invjacs (E,Q,d,d)`,
    `jacdets (E,Q)` (signed) and `quad_coords (E,Q,d)` with
    `sfem_geom_factors` (sum-factorised, closed-form d x d inverse).
  * Nodal q-functions evaluate with `sfem_basis_eval` (values / physical
    gradients at all quadrature points of all elements).
  * `local_covector` does not trace: the form is evaluated once on `QExpr`
    values (core/qexpr.py); the placeholder's slot yields the coefficient
    fields `(c0, c1)` and `sfem_basis_eval_t` applies the exact transpose
    `sum_q w detJ (I^T c0 + G^T J^-T c1)` -- what `jax.linear_transpose`
    produces in the reference (:466-471).
  * The collocated mass / stiffness / Helmholtz operators have a fused
    gather->apply->scatter kernel, reached through `helmholtz_operator`.
  * Boundary integrals over the facets of a physical group
    (`Mesh.boundary_facets`): `boundary_points` / `boundary_covector` run
    `sfem_boundary_geom` / `sfem_boundary_covector` with the space's 1D rule
    in each facet direction, and `sfem_scatter_csr` sums the facet values per
    node in a fixed order.
  * `boundary_mass` is the facet mass operator of a Robin term,
    `<alpha u, v>` over a group: `sfem_boundary_mass_apply` on each facet,
    then `sfem_boundary_add_rows` adds the facet values into the operator's
    output on the group's nodes only, in a fixed order.
"""

from __future__ import annotations

import dataclasses
from typing import Protocol

import numpy as np
import torch

from swirl_fem_amd import _ops
from swirl_fem_amd.core import autodiff
from swirl_fem_amd.core import interpolation
from swirl_fem_amd.core.interpolation import BarycentricInterpolator
from swirl_fem_amd.core.interpolation import Quadrature1D
from swirl_fem_amd.core.mesh import Mesh
from swirl_fem_amd.core.qexpr import QExpr
from swirl_fem_amd.core import qexpr


# ---------------------------------------------------------------- q-functions
class QFunction(Protocol):
  """A function from the mesh to R^k, called on the point variable `x`
  (reference core/fespace.py:35-56).  Here `x` is a `QExpr` carrying all
  quadrature points of all elements at once, and so is the result."""

  def __call__(self, x):
    ...


class Form(Protocol):
  """Maps q-functions to the scalar q-function that gets integrated
  (reference core/fespace.py:59-72), e.g.
  `lambda u, v: lambda x: torch.vdot(grad(u)(x), grad(v)(x))`."""

  def __call__(self, *args: QFunction) -> QFunction:
    ...


@dataclasses.dataclass(eq=False)
class NodalQFunction:
  """A nodal function of a `FiniteElementSpace` (u_local None = placeholder)."""
  fespace: 'FiniteElementSpace'
  value_shape: tuple
  u_local: torch.Tensor | None = None

  def __post_init__(self):
    expected = (self.fespace.num_elements,
                self.fespace.mesh.num_nodes_per_element) + self.value_shape
    if self.u_local is not None and tuple(self.u_local.shape) != expected:
      raise ValueError('shape:', tuple(self.u_local.shape))

  def _evaluate(self) -> torch.Tensor:
    raise NotImplementedError

  def _placeholder(self) -> QExpr:
    raise NotImplementedError

  def __call__(self, x=None) -> QExpr:
    del x   # nodal values suffice (reference fespace.py:162-165)
    if self.u_local is None:
      return self._placeholder()
    return QExpr(self._evaluate())

  def _u3(self):
    E, n = self.u_local.shape[:2]
    return self.u_local.reshape(E, n, -1)


class ScalarNodalQFunction(NodalQFunction):
  """Scalar function interpolated from nodal values (fespace.py:171-179)."""

  def __init__(self, fespace, u_local=None):
    super().__init__(fespace, (), u_local)

  def _evaluate(self):
    val, _ = self.fespace._basis(self._u3(), want_val=True, want_grad=False)
    return val[..., 0]

  def _placeholder(self):
    return QExpr(shape=(), pullback=lambda ct: (ct, None))


class ScalarNodalQFunctionGrad(NodalQFunction):
  """Gradient of a scalar nodal function (fespace.py:183-195)."""

  def __init__(self, fespace, u_local=None):
    super().__init__(fespace, (), u_local)

  def _evaluate(self):
    _, g = self.fespace._basis(self._u3(), want_val=False, want_grad=True)
    return g[..., 0]                                    # (E, Q, d)

  def _placeholder(self):
    d = self.fespace.mesh.ndim
    return QExpr(shape=(d,), pullback=lambda ct: (None, ct))


class VectorNodalQFunction(NodalQFunction):
  """Vector function interpolated from nodal values (fespace.py:199-209)."""

  def __init__(self, fespace, u_local=None):
    super().__init__(fespace, (fespace.mesh.ndim,), u_local)

  def _evaluate(self):
    val, _ = self.fespace._basis(self._u3(), want_val=True, want_grad=False)
    return val

  def _placeholder(self):
    d = self.fespace.mesh.ndim
    return QExpr(shape=(d,), pullback=lambda ct: (ct, None))


class VectorNodalQFunctionGrad(NodalQFunction):
  """Gradient [j, k] = d u_k / d x_j of a vector function (:213-225)."""

  def __init__(self, fespace, u_local=None):
    super().__init__(fespace, (fespace.mesh.ndim,), u_local)

  def _evaluate(self):
    _, g = self.fespace._basis(self._u3(), want_val=False, want_grad=True)
    return g                                            # (E, Q, d, d)

  def _placeholder(self):
    d = self.fespace.mesh.ndim
    return QExpr(shape=(d, d), pullback=lambda ct: (None, ct))


def grad(f):
  """Gradient of a q-function (fespace.py:233-241)."""
  if isinstance(f, ScalarNodalQFunction):
    return ScalarNodalQFunctionGrad(fespace=f.fespace, u_local=f.u_local)
  if isinstance(f, VectorNodalQFunction):
    return VectorNodalQFunctionGrad(fespace=f.fespace, u_local=f.u_local)

  # A plain function of the coordinate x: differentiate pointwise with
  # autograd (the reference falls back to jax.grad here).
  def _grad_f(x: QExpr) -> QExpr:
    with torch.enable_grad():
      xv = x.val.detach().clone().requires_grad_(True)
      out = f(QExpr(xv))
      out = out.val if isinstance(out, QExpr) else out
      (g,) = torch.autograd.grad(out.sum(), xv)
    return QExpr(g.detach())

  return _grad_f


def div(f):
  """Divergence of a vector-valued q-function (fespace.py:244-248)."""
  def _divf(x):
    return qexpr.trace(grad(f)(x))
  return _divf


# ------------------------------------------------------------ the FE space
@dataclasses.dataclass(frozen=True, eq=False)
class FiniteElementSpace:
  """Nodal finite element space on a mesh with a tensor quadrature."""
  mesh: Mesh
  quadrature: Quadrature1D
  interpolator: BarycentricInterpolator
  _cache: dict = dataclasses.field(default_factory=dict, repr=False,
                                   compare=False)

  @classmethod
  def create(cls, mesh: Mesh, quadrature: Quadrature1D) -> 'FiniteElementSpace':
    interpolator = BarycentricInterpolator(
        ndim=mesh.ndim, gridpoints_1d=mesh.gridpoints_1d,
        evalpoints_1d=quadrature.nodes)
    return cls(mesh=mesh, quadrature=quadrature, interpolator=interpolator,
               _cache={})

  # The reference computes and stores `invjacs (E,Q,d,d)`, `jacdets (E,Q)` and
  # `quad_coords (E,Q,d)` in `create` (core/fespace.py:330-348): 13 reals per
  # quadrature point, 14 GB at 64^3 elements / p = 7.  Here they are built on
  # first use (one `sfem_geom_factors` launch): the fused operators evaluate
  # the geometry of multilinear elements in registers and never ask for them.
  def _geometry(self):
    if 'geometry' not in self._cache:
      i1, g1 = self._matrices()
      self._cache['geometry'] = _ops.geom_factors(
          self.mesh.element_coords(), i1, g1, self.mesh.ndim,
          self.mesh.gridpoints_1d.num_points, self.quadrature.num_points,
          want_quad_coords=True)
    return self._cache['geometry']

  @property
  def invjacs(self) -> torch.Tensor:
    return self._geometry()[0]

  @property
  def jacdets(self) -> torch.Tensor:
    return self._geometry()[1]

  @property
  def quad_coords(self) -> torch.Tensor:
    return self._geometry()[2]

  def replace(self, **kw):
    kw.setdefault('_cache', {})
    return dataclasses.replace(self, **kw)

  # ------------------------------------------------------------- properties
  @property
  def num_elements(self) -> int:
    return self.mesh.num_elements

  @property
  def num_quadrature_points_per_element(self) -> int:
    return int(self.quadrature.num_points ** self.mesh.ndim)

  @property
  def dtype(self):
    return self.mesh.dtype

  @property
  def device(self):
    return self.mesh.device

  @property
  def is_collocated(self) -> bool:
    return self.interpolator.is_collocated

  def _matrices(self):
    return _device_matrices(self.interpolator, self.dtype, self.device,
                            self._cache)

  def wdet(self) -> torch.Tensor:
    """`jacdets * quadrature weights`, shape (E, Q)."""
    if 'wdet' not in self._cache:
      w = torch.as_tensor(self.quadrature.weights_nd(self.mesh.ndim),
                          dtype=self.dtype, device=self.device)
      self._cache['wdet'] = (self.jacdets * w[None, :]).contiguous()
    return self._cache['wdet']

  def _basis(self, u3, want_val, want_grad):
    """u3 (E, n, nc) -> values (E,Q,nc), physical gradients (E,Q,d,nc)."""
    i1, g1 = self._matrices()
    u3 = u3.to(self.dtype)
    ev = autodiff.basis_eval if autodiff.needs_grad(u3) else _ops.basis_eval
    return ev(
        u3, i1, g1, self.invjacs if want_grad else None, self.mesh.ndim,
        self.mesh.gridpoints_1d.num_points, self.quadrature.num_points,
        self.is_collocated, want_val, want_grad)

  def _interpolate(self, u3):
    """Element-local values (E, n, nc) at the quadrature points (E, Q^d, nc):
    the values of `_basis`; `u3` itself when collocated."""
    return u3 if self.is_collocated else self._basis(u3, True, False)[0]

  def _interpolate_t(self, rq, grad=False):
    """The bare transpose of `_interpolate`, (E, Q^d, nc) -> (E, n, nc): no
    weights (`sfem_basis_eval_t` with ones for w detJ); `rq` itself when
    collocated.  `grad`: the route that carries its own transpose."""
    if self.is_collocated:
      return rq
    mesh, q = self.mesh, self.quadrature.num_points
    i1, g1 = self._matrices()
    key = 'ones_eq'
    if key not in self._cache:
      self._cache[key] = torch.ones((mesh.num_elements, q ** mesh.ndim),
                                    dtype=self.dtype, device=self.device)
    ev = autodiff.basis_eval_t if grad else _ops.basis_eval_t
    return ev(rq, None, i1, g1, None, self._cache[key], mesh.ndim,
              mesh.gridpoints_1d.num_points, q, rq.shape[-1], False)

  # ------------------------------------------------------------ q-functions
  def _evaluate(self, f) -> torch.Tensor:
    """Evaluates a q-function at every element's quadrature points."""
    out = f(QExpr(self.quad_coords))
    if isinstance(out, QExpr):
      if out.is_linear:
        raise ValueError('cannot evaluate a placeholder q-function')
      return out.val
    out = torch.as_tensor(out, dtype=self.dtype, device=self.device)
    if out.dim() == 0:
      return out.expand(self.num_elements,
                        self.num_quadrature_points_per_element)
    return out

  def scalar_function(self, u_local):
    expected = (self.num_elements, self.mesh.num_nodes_per_element)
    if u_local is not None and tuple(u_local.shape) != expected:
      raise ValueError(
          f'Expecting shape {expected} but got {tuple(u_local.shape)=}')
    return ScalarNodalQFunction(fespace=self, u_local=u_local)

  def vector_function(self, u_local):
    expected = (self.num_elements, self.mesh.num_nodes_per_element,
                self.mesh.ndim)
    if u_local is not None and tuple(u_local.shape) != expected:
      raise ValueError(
          f'Expecting shape {expected} but got {tuple(u_local.shape)=}')
    return VectorNodalQFunction(fespace=self, u_local=u_local)

  def integrate(self, f) -> torch.Tensor:
    """Quadrature of a scalar q-function over the mesh (0-dim tensor)."""
    w = self._evaluate(f)
    expected = (self.num_elements, self.num_quadrature_points_per_element)
    if tuple(w.shape) != expected:
      raise ValueError(
          'Expecting an array of shape (num elements, num quadrature points), '
          f'that is ({expected}) but got: {tuple(w.shape)}')
    res = torch.zeros(1, dtype=torch.float64, device=self.device)
    _ops.dot(w.to(self.dtype).contiguous().reshape(-1),
             self.wdet().reshape(-1), res, 0)
    return res[0].to(self.dtype)

  def local_covector(self, form, funs) -> torch.Tensor:
    """Local covector `(E, n) + value_shape` of the functional obtained by
    fixing every argument of the multilinear `form` except the placeholder."""
    def _is_input(f):
      return isinstance(f, NodalQFunction) and f.u_local is None

    if sum(_is_input(f) for f in funs) != 1:
      raise ValueError('Exactly one `QFunction` must be a nodal function and '
                       'have `None` as nodal values')
    placeholder = [f for f in funs if _is_input(f)][0]
    if placeholder.fespace is not self:
      # mixed forms (e.g. div(v) q): the covector lives in the space that
      # `local_covector` is called on, like the reference (:465-470).
      pass
    expr = form(*funs)(QExpr(self.quad_coords))
    if not isinstance(expr, QExpr) or not expr.is_linear:
      raise ValueError('the form does not depend on the placeholder function')
    if expr.shape != ():
      raise ValueError(f'the form must be scalar valued, got {expr.shape}')
    E, Q = self.num_elements, self.num_quadrature_points_per_element
    ones = torch.ones((E, Q), dtype=self.dtype, device=self.device)
    c0, c1 = expr.pullback(ones)
    value_shape = placeholder.value_shape
    nc = int(np.prod(value_shape)) if value_shape else 1
    d = self.mesh.ndim
    if c0 is not None:
      c0 = c0.to(self.dtype).reshape(E, Q, nc)
    if c1 is not None:
      c1 = c1.to(self.dtype).reshape(E, Q, d, nc)
    i1, g1 = self._matrices()
    ev_t = (autodiff.basis_eval_t if autodiff.needs_grad(c0, c1)
            else _ops.basis_eval_t)
    out = ev_t(
        c0, c1, i1, g1, self.invjacs, self.wdet(), d,
        self.mesh.gridpoints_1d.num_points, self.quadrature.num_points, nc,
        self.is_collocated)
    return out.reshape((E, self.mesh.num_nodes_per_element) + value_shape)

  # ------------------------------------------------------ boundary facets
  def _boundary_plan(self, group: str) -> dict:
    """Per group: facet rows, facet points and weights, the CSR of the facet
    slots per node (built once, on the host)."""
    key = ('boundary', group)
    if key in self._cache:
      return self._cache[key]
    mesh = self.mesh
    if mesh.axis_name is not None or mesh.neighbor_plan is not None:
      raise NotImplementedError('boundary integrals on a partitioned mesh')
    if mesh._cache.get('replicas', 1) > 1:
      raise NotImplementedError('boundary integrals on an ensemble '
                                '(Mesh.replicate)')
    if group not in mesh.boundary_facets:
      if group in mesh.physical_masks:
        raise ValueError(f'physical group {group!r} has no facets: its node '
                         'array is not (F, (P+1)^(d-1)) facet rows')
      raise KeyError(f'unknown physical group {group!r}; the mesh has '
                     f'{sorted(mesh.physical_masks)}')
    facets = mesh.boundary_facets[group].to(torch.int32).contiguous()
    host = facets.cpu().numpy().astype(np.int64)
    n = mesh.num_nodes
    if host.size and (host.min() < 0 or host.max() >= n):
      raise ValueError(f'physical group {group!r}: node ids outside [0, {n})')
    d = mesh.ndim
    plan = {'facets': facets}
    if d == 1:
      plan['xq'] = mesh.node_coords[facets[:, 0].long()].reshape(-1, 1, 1)
      plan['wj'] = torch.ones((facets.shape[0], 1), dtype=self.dtype,
                              device=self.device)
    else:
      i1, g1 = self._matrices()
      w = torch.as_tensor(self.quadrature.weights, dtype=self.dtype,
                          device=self.device)
      plan['xq'], plan['wj'] = _ops.boundary_geom(
          mesh.node_coords.contiguous(), facets, i1, g1, w)
      offsets, slots = boundary_csr(host, n)
      plan['offsets'] = torch.as_tensor(offsets, device=self.device)
      plan['slots'] = torch.as_tensor(slots, device=self.device)
    self._cache[key] = plan
    return plan

  def boundary_points(self, group: str):
    """`(x_q (F, Q^(d-1), d), wJ (F, Q^(d-1)))`: the quadrature points on the
    facets of `group` and their weights times the facet Jacobian
    (w_s w_t |x_s x x_t| on faces, w_s |x_s| on edges; 1 at 1D points)."""
    plan = self._boundary_plan(group)
    return plan['xq'], plan['wj']

  def boundary_covector(self, group: str, g) -> torch.Tensor:
    """The assembled `(N,)` vector `int_group g phi_i dGamma`.

    `g`: a scalar; an `(N,)` nodal tensor (interpolated on each facet); the
    values `(F, Q^(d-1))` at the facet points of `boundary_points`; or a
    callable that takes the `(M, d)` point coordinates and returns `(M,)`.
    Periodic images are summed by the mesh's exchange.
    """
    plan = self._boundary_plan(group)
    mesh, facets = self.mesh, plan['facets']
    xq, wj = plan['xq'], plan['wj']
    nodal = False
    if callable(g):
      g = torch.as_tensor(g(xq.reshape(-1, mesh.ndim)), dtype=self.dtype,
                          device=self.device)
      if g.numel() != wj.numel():
        raise ValueError(f'the callable returned {tuple(g.shape)} values for '
                         f'{wj.numel()} points')
      g = g.reshape(wj.shape)
    else:
      g = torch.as_tensor(g, dtype=self.dtype, device=self.device)
      if g.dim() == 0:
        g = g.expand(wj.shape)
      elif tuple(g.shape) == (mesh.num_nodes,):
        nodal = True
      elif tuple(g.shape) != tuple(wj.shape):
        raise ValueError(f'g must be a scalar, ({mesh.num_nodes},) nodal '
                         f'values or {tuple(wj.shape)} point values; got '
                         f'{tuple(g.shape)}')
    g = g.contiguous()
    if mesh.ndim == 1:
      ids = facets[:, 0].long()
      out = torch.zeros(mesh.num_nodes, dtype=self.dtype, device=self.device)
      out[ids] = g[ids] if nodal else g[:, 0]
    else:
      i1, _ = self._matrices()
      local = _ops.boundary_covector(g, nodal, facets, wj.contiguous(), i1,
                                     mesh.ndim)
      out = _ops.scatter_csr(local.reshape(-1), plan['offsets'],
                             plan['slots'], mesh.num_nodes)
    return mesh.exchange(out)

  def boundary_mass(self, group: str, alpha,
                    dirichlet_mask=None) -> 'BoundaryMassOperator':
    """The facet mass operator `<alpha u, v>` over the facets of `group`
    (the operator term of a Robin condition du/dn + alpha u = g).

    `alpha` >= 0 takes the forms of `boundary_covector`'s `g`: a scalar, `(N,)`
    nodal values (interpolated to the points once), `(F, Q^(d-1))` point
    values or a callable on the `(M, d)` points.  `dirichlet_mask` (N,) bool:
    those rows and columns are removed, as in the masked volume operator.
    """
    mesh = self.mesh
    if not callable(alpha):
      a = torch.as_tensor(alpha, dtype=self.dtype)
      if a.dim() == 0 and not bool(a >= 0):
        raise ValueError(f'alpha must be >= 0, got {float(a)}')
      if a.dim() != 0 and bool((a < 0).any()):
        raise ValueError('alpha has negative values')
    plan = self._boundary_plan(group)
    facets, xq, wj = plan['facets'], plan['xq'], plan['wj']
    if callable(alpha):
      a = torch.as_tensor(alpha(xq.reshape(-1, mesh.ndim)), dtype=self.dtype,
                          device=self.device)
      if a.numel() != wj.numel():
        raise ValueError(f'the callable returned {tuple(a.shape)} values for '
                         f'{wj.numel()} points')
      a = a.reshape(wj.shape)
    else:
      a = torch.as_tensor(alpha, dtype=self.dtype, device=self.device)
      if a.dim() == 0:
        a = a.expand(wj.shape)
      elif tuple(a.shape) == (mesh.num_nodes,):
        a = a[facets.long()]                              # (F, (P+1)^(d-1))
        if mesh.ndim == 3:
          p1 = mesh.gridpoints_1d.num_points
          a = a.reshape(-1, p1, p1)
        if mesh.ndim > 1:
          i1, _ = self._matrices()
          a = (torch.einsum('qi,rj,fij->fqr', i1, i1, a) if mesh.ndim == 3
               else torch.einsum('qi,fi->fq', i1, a))
        a = a.reshape(wj.shape)
      elif tuple(a.shape) != tuple(wj.shape):
        raise ValueError(f'alpha must be a scalar, ({mesh.num_nodes},) nodal '
                         f'values or {tuple(wj.shape)} point values; got '
                         f'{tuple(a.shape)}')
    if bool((a < 0).any()):
      raise ValueError('alpha has negative values')
    return BoundaryMassOperator(self, facets, wj, (a * wj).contiguous(),
                                dirichlet_mask)

  # -------------------------------------------------------- fused operators
  def to_quadrature(self, nodal) -> torch.Tensor:
    """Nodal values (N,) or (N, d) at the quadrature points: (E, Q^d) or
    (E, Q^d, d), in the point order of `quad_coords` (gather + the
    values-only basis kernel).  E.g. a nodal velocity of `StokesSEM` as the
    `velocity` of `helmholtz_operator`."""
    u = torch.as_tensor(nodal, dtype=self.dtype, device=self.device)
    if u.dim() not in (1, 2) or u.shape[0] != self.mesh.num_nodes:
      raise ValueError(f'expected ({self.mesh.num_nodes},) or '
                       f'({self.mesh.num_nodes}, d) nodal values, got '
                       f'{tuple(u.shape)}')
    scalar = u.dim() == 1
    loc = (self.mesh.gather(u)[..., None] if scalar
           else _ops.gather_rows(u.contiguous(), self.mesh.elements))
    vals = self._interpolate(loc.contiguous())
    return (vals[..., 0] if scalar else vals).contiguous()

  def helmholtz_operator(self, dirichlet_mask=None, geometry='auto',
                         assembly='auto', *, diffusivity=None, reaction=None,
                         velocity=None):
    """Fused `out = mask * scatter((l0 B + l1 A)_local(gather(u)))`.

    `geometry`: 'auto' evaluates the geometric factors of affine / multilinear
    elements in registers and stores 6 factors per point only for curved
    elements; 'stored' stores them for every element (same results to
    rounding).  `assembly`: how shared nodes are summed, see
    `operators.HelmholtzOperator.create`.

    `diffusivity` k, `reaction` c: the operator becomes l0 B_c + l1 A_k with
    B_c[i,j] = sum_q c_q W_q phi_i phi_j, A_k[i,j] = sum_q k_q grad phi_i .
    G_q grad phi_j.  Each is a scalar, an (E,) tensor, an (E, Q^d) tensor at
    the quadrature points (`quad_coords` order) or a callable (M, d) ->
    (M,) evaluated there once (`operators.coefficient`); None means 1.  Such
    operators are not cached.

    `velocity` b adds the advective term C_b[i,j] = sum_q W_q phi_i(q) b_q .
    grad phi_j(q) (plain Galerkin convective form, scaled by neither
    lambda): a (d,) constant, an (E, d) tensor, an (E, Q^d, d) tensor at the
    quadrature points (`to_quadrature` makes one from nodal values) or a
    callable (M, d) -> (M, d) on coordinates (`operators.velocity_field`).
    The operator is then not symmetric: solve with `linalg.bicgstab`.  There
    is no stabilisation, so boundary layers have to be resolved.  Not cached.
    """
    from swirl_fem_amd.core import operators
    if velocity is not None:
      if (not self.is_collocated and assembly in ('auto', 'atomic') and
          operators.supports_two_grid(self) is None):
        return operators.TwoGridHelmholtzOperator.create(
            self, dirichlet_mask, 'stored' if geometry == 'stored' else 'auto',
            diffusivity=diffusivity, reaction=reaction, velocity=velocity)
      return operators.HelmholtzOperator.create(
          self, dirichlet_mask, geometry, assembly, diffusivity=diffusivity,
          reaction=reaction, velocity=velocity)
    if diffusivity is not None or reaction is not None:
      if (not self.is_collocated and assembly in ('auto', 'atomic') and
          operators.supports_two_grid(self) is None):
        return operators.TwoGridHelmholtzOperator.create(
            self, dirichlet_mask, 'stored' if geometry == 'stored' else 'auto',
            diffusivity=diffusivity, reaction=reaction)
      return operators.HelmholtzOperator.create(
          self, dirichlet_mask, geometry, assembly, diffusivity=diffusivity,
          reaction=reaction)
    # cached per (mask object, options); the entry keeps the mask alive so that
    # its id cannot be recycled by another tensor
    key = ('helmholtz', None if dirichlet_mask is None else id(dirichlet_mask),
           geometry, assembly)
    hit = self._cache.get(key)
    if hit is not None and hit[0] is dirichlet_mask:
      return hit[1]
    if not self.is_collocated and assembly in ('auto', 'atomic') and (
        operators.supports_two_grid(self) is None):
      # quadrature != nodes: interpolate, fused element kernel on the
      # quadrature grid, transposed interpolation
      op = operators.TwoGridHelmholtzOperator.create(
          self, dirichlet_mask, 'stored' if geometry == 'stored' else 'auto')
    else:
      op = operators.HelmholtzOperator.create(self, dirichlet_mask, geometry,
                                              assembly)
    self._cache[key] = (dirichlet_mask, op)
    return op

  def elasticity_operator(self, dirichlet_mask=None, *, lame_lambda, lame_mu,
                          density=None, geometry='auto'):
    """Fused linear elasticity, `out = mask * scatter((K + lambda0 M_rho)_local
    (gather(u)))` for displacements u (N, d): `v^T K u = int sigma(u) : grad
    v` with sigma = lambda tr(eps) I + 2 mu eps (plane strain in 2D).

    `lame_lambda` >= 0, `lame_mu` > 0 and `density` >= 0 (None: 1) are each a
    scalar, an (E,) tensor, an (E, Q^d) tensor at the quadrature points or a
    callable (M, d) -> (M,) on their coordinates (`operators.coefficient`;
    `operators.lame_parameters` makes the first two from E and nu).
    `dirichlet_mask`: (N, d) bool per component, or (N,) for all components
    of a node."""
    from swirl_fem_amd.core import operators
    return operators.ElasticityOperator.create(
        self, dirichlet_mask, lame_lambda=lame_lambda, lame_mu=lame_mu,
        density=density, geometry=geometry)

  def hyperelastic_operator(self, dirichlet_mask=None, *, lame_lambda,
                            lame_mu, density=None, geometry='auto'):
    """Finite-strain elasticity of a compressible neo-Hookean material, total
    Lagrangian: residual, energy and tangent for displacements u (N, d)
    (`operators.HyperelasticOperator`).  Arguments as for
    `elasticity_operator`, which is its tangent at u = 0."""
    from swirl_fem_amd.core import operators
    return operators.HyperelasticOperator.create(
        self, dirichlet_mask, lame_lambda=lame_lambda, lame_mu=lame_mu,
        density=density, geometry=geometry)

  def plasticity_operator(self, dirichlet_mask=None, *, lame_lambda, lame_mu,
                          yield_stress, hardening_modulus=0.0, density=None,
                          geometry='auto'):
    """Small-strain von Mises (J2) plasticity with linear isotropic hardening:
    residual, algorithmic tangent and stress for displacements u (N, d) and a
    history at the quadrature points (`operators.PlasticityOperator`, DESIGN
    §3.22).  `yield_stress` > 0 and `hardening_modulus` >= 0 take the forms of
    the Lame parameters; the other arguments are those of
    `elasticity_operator`, which is its tangent before first yield."""
    from swirl_fem_amd.core import operators
    return operators.PlasticityOperator.create(
        self, dirichlet_mask, lame_lambda=lame_lambda, lame_mu=lame_mu,
        yield_stress=yield_stress, hardening_modulus=hardening_modulus,
        density=density, geometry=geometry)


class BoundaryMassOperator:
  """`scale * M u` with M the facet mass matrix `(B (x) B)^T diag(aw) (B (x) B)`
  of every facet, summed over the facets' nodes.

  `facets` (F, (P+1)^(d-1)) int32 node ids, `wj` (F, Q^(d-1)) the facet
  weights at the points of the space's rule, `aw` alpha times them;
  `dirichlet_mask`: the rows and columns removed (a facet slot of a
  Dirichlet node is stored as ~id, `pmg.encode_rows`).  `apply` costs
  O(boundary): one wave per facet,
  then one thread per non-Dirichlet node of the group adds that node's facet
  values in a fixed order into the output.  No exchange: a caller on a mesh
  with periodic images sums them with its own.  In 1D a facet is a point and
  the term is alpha u there.
  """

  def __init__(self, fespace, facets, wj, aw, dirichlet_mask=None):
    mesh = fespace.mesh
    self.fespace, self.ndim = fespace, mesh.ndim
    self.facets = facets.to(torch.int32).contiguous()
    self.wj = wj
    self.aw = aw.to(fespace.dtype).contiguous()
    self.dirichlet = dirichlet_mask
    host = self.facets.cpu().numpy()
    dmask = (None if dirichlet_mask is None else
             dirichlet_mask.cpu().numpy().astype(bool))
    rows, offsets, slots = boundary_rows(host, mesh.num_nodes, dmask)
    dev = fespace.device
    self.rows = torch.as_tensor(rows, device=dev)
    self.offsets = torch.as_tensor(offsets, device=dev)
    self.slots = torch.as_tensor(slots, device=dev)
    if dirichlet_mask is None:
      self.encoded = self.facets
    else:
      self.encoded = torch.where(dirichlet_mask.to(dev)[self.facets.long()],
                                 ~self.facets, self.facets).contiguous()
    if self.ndim == 1:
      # the alpha of every row (the sum over the point facets at its node)
      aw1 = self.aw[:, 0].double().cpu().numpy()
      ra = np.array([aw1[slots[offsets[r]:offsets[r + 1]]].sum()
                     for r in range(rows.size)])
      self._row_alpha = torch.as_tensor(ra, dtype=fespace.dtype, device=dev)
      self._rows_long = self.rows.long()
    else:
      self.bmat = fespace._matrices()[0]
      self._local = torch.empty(self.facets.shape, dtype=fespace.dtype,
                                device=dev)

  @property
  def num_nodes(self) -> int:
    return self.fespace.mesh.num_nodes

  def total_weight(self) -> float:
    """sum(alpha wJ) over the group: > 0 iff alpha > 0 on a set of positive
    measure."""
    return float(self.aw.double().sum())

  def apply(self, u, scale=1.0, out=None):
    """out += scale M u on the group's nodes (every other entry untouched);
    a fresh vector when `out` is None."""
    if out is None:
      out = torch.zeros(self.num_nodes, dtype=u.dtype, device=u.device)
    if self.ndim == 1:
      r = self._rows_long
      out[r] += scale * self._row_alpha * u[r]
      return out
    _ops.boundary_mass(u.contiguous(), self.encoded, self.aw, self.bmat,
                       self.ndim, scale, out=self._local)
    return _ops.boundary_add_rows(self._local, self.rows, self.offsets,
                                  self.slots, out)

  def diagonal(self) -> torch.Tensor:
    """The assembled (N,) diagonal of M (0 off the group and on Dirichlet
    rows)."""
    out = torch.zeros(self.num_nodes, dtype=self.aw.dtype,
                      device=self.aw.device)
    if self.ndim == 1:
      out[self._rows_long] = self._row_alpha
      return out
    loc = _ops.boundary_mass(None, self.encoded, self.aw, self.bmat,
                             self.ndim, 1.0, diag=True)
    return _ops.boundary_add_rows(loc, self.rows, self.offsets, self.slots,
                                  out)

  def local_matrices(self) -> torch.Tensor:
    """(F, n, n) facet matrices (Dirichlet rows and columns zero) for host
    assembly with the rows of `facets`: unit vectors through the kernel."""
    F, n = self.facets.shape
    dev, dt = self.aw.device, self.aw.dtype
    if self.ndim == 1:
      keep = self.encoded[:, 0] >= 0
      return (self.aw[:, 0] * keep).reshape(F, 1, 1)
    ids = torch.arange(F * n, dtype=torch.int32, device=dev).reshape(F, n)
    ids = torch.where(self.encoded >= 0, ids, ~ids).contiguous()
    cols = []
    for j in range(n):
      u = torch.zeros(F * n, dtype=dt, device=dev)
      u[j::n] = 1.0
      cols.append(_ops.boundary_mass(u, ids, self.aw, self.bmat, self.ndim))
    return torch.stack(cols, dim=-1)


def boundary_rows(facets: np.ndarray, num_nodes: int,
                  dirichlet: np.ndarray | None = None):
  """The compact CSR of `sfem_boundary_add_rows`: `(rows (R,) int32,
  offsets (R+1,) int64, slots int32)` over the distinct nodes of `facets`
  that are not `dirichlet`, ascending, with each row's facet slots ascending
  (a fixed summation order)."""
  flat = np.asarray(facets, np.int64).reshape(-1)
  if flat.size and (flat.min() < 0 or flat.max() >= num_nodes):
    raise ValueError(f'facet node ids outside [0, {num_nodes})')
  order = np.argsort(flat, kind='stable')
  rows, counts = np.unique(flat[order], return_counts=True)
  keep = (np.ones(rows.size, dtype=bool) if dirichlet is None else
          ~np.asarray(dirichlet, bool)[rows])
  slots = order[np.repeat(keep, counts)]
  offsets = np.zeros(int(keep.sum()) + 1, dtype=np.int64)
  offsets[1:] = np.cumsum(counts[keep])
  return (rows[keep].astype(np.int32), offsets, slots.astype(np.int32))


def boundary_csr(facets: np.ndarray, num_nodes: int):
  """CSR of the facet slots per node: `(offsets (N+1,) int64, slots int32)`,
  slots ascending per node, so `sfem_scatter_csr` sums in a fixed order."""
  flat = np.asarray(facets, np.int64).reshape(-1)
  slots = np.argsort(flat, kind='stable').astype(np.int32)
  offsets = np.zeros(num_nodes + 1, dtype=np.int64)
  offsets[1:] = np.cumsum(np.bincount(flat, minlength=num_nodes))
  return offsets, slots


def _device_matrices(interpolator, dtype, device, cache):
  key = ('mats', dtype, str(device))
  if key not in cache:
    i1, _ = interpolation.matrices_1d(interpolator.gridpoints_1d,
                                      interpolator.evalpoints_1d)
    g1 = interpolator._interp_grad_matrix_1d()
    cache[key] = tuple(
        torch.as_tensor(np.array(m), dtype=dtype, device=device)
        for m in (i1, g1))
  return cache[key]
