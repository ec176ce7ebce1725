"""NumPy reference of time-dependent scalar transport by BDFk/EXTk
(`swirl_fem_amd/examples/transport.py`):

    dT/dt + u . grad T - div(k grad T) = s.

* `integrand`: what the kernel `sfem_transport_rhs` computes on the Q^d
  quadrature grid,
      out[e,q] = W[e,q] (s[e,q] + sum_j m_j T_j[e,q])
               + sum_j c_j W[e,q] u_j[e,q] . grad T_j[e,q],
  sum-factorised with the 1D derivative matrix of the Q points (as
  `tests/sumfact_reference.py` does for its nodes), the geometry (`invjacs`,
  `jacdets`) from the oracle space.
* `Dense`: the assembled problem from the dense element matrices of
  `tests/advection_reference.py` (B, A_k, C(u)), the facet terms of
  `tests/bvp_reference.py` / `tests/robin_reference.py` and the Dirichlet
  lift: the right-hand side, one step by `numpy.linalg.solve`, the steady
  state, and the exact solution of the semi-discrete system by an eigen-
  decomposition of B^-1 (A + C) on the free nodes.

Time levels are lists oldest first; the coefficient conventions are those of
the stepper: bdf = bdfk_coeffs(k), ext = extk_coeffs(k - 1).
"""

import numpy as np

from oracle import sfem_oracle as O
from tests import advection_reference as AR
from tests import bvp_reference as BR
from tests import robin_reference as RR
from tests.sumfact_reference import _along


def coefficients(order):
  """(bdf, ext) of a step of order k over k levels, oldest first; bdf has one
  more entry, the new level's."""
  return O.bdfk_coeffs(order), (np.ones(1) if order == 1
                                else O.extk_coeffs(order - 1))


def quadrature_dmat(Q):
  """Differentiation matrix of the Lagrange basis on the Q Gauss points."""
  return O.differentiation_matrix_1d(O.nodes_1d(Q, 'gl'), 'gl')


def wdet(fes):
  return fes.jacdets * fes.weights[None, :]


def integrand(fes, levels, source_q=None):
  """`levels`: (T_q (E, Q^d), u_q (E, Q^d, d) or None, mass_coef, conv_coef)
  on the quadrature grid of the oracle space `fes` -> (E, Q^d)."""
  d = fes.ndim
  W = wdet(fes)
  E, nq = W.shape
  Q = round(nq ** (1.0 / d))
  assert Q ** d == nq
  D = quadrature_dmat(Q)
  out = np.zeros((E, nq))
  if source_q is not None:
    out += W * source_q
  for Tq, uq, mc, cc in levels:
    Tq = np.asarray(Tq, np.float64)
    out += mc * W * Tq
    if uq is None or cc == 0.0:
      continue
    grid = Tq.reshape((E,) + (Q,) * d)
    ref = np.stack([_along(D, grid, 1 + a).reshape(E, nq) for a in range(d)],
                   axis=-1)                                   # d T / d xi_a
    # invjacs[e,q,j,a] = d xi_a / d x_j
    phys = np.einsum('eqja,eqa->eqj', fes.invjacs, ref)
    out += cc * W * np.einsum('eqj,eqj->eq', np.asarray(uq, np.float64), phys)
  return out


def to_points(fes, nodal):
  """Nodal (N,) or (N, d) values at the quadrature points."""
  return np.einsum('qi,ei...->eq...', fes.M, fes.gather(np.asarray(nodal)))


def point_velocity(fes, u):
  """A velocity in any form the stepper takes as (E, Q^d, d), or None."""
  if u is None:
    return None
  u = np.asarray(u, np.float64)
  E, nq, d = fes.num_elements, fes.Q, fes.ndim
  if u.shape == (d,):
    return np.broadcast_to(u, (E, nq, d))
  if u.shape == (E, nq, d):
    return u
  assert u.shape == (fes.num_nodes, d), u.shape
  return to_points(fes, u)


class Dense:
  """The assembled transport problem on a refined premesh `rp` with P nodes
  per direction and the Gauss rule of the solves.  `kf`: NumPy callable on
  (..., d) points or None; `dvals` (N,) with NaN off the Dirichlet nodes (or
  None); robin [(group, alpha, g)], neumann [(group, g)] as in
  `test_gpu_advection.dense_solve`; `node_indices`: periodic classes (the
  unknowns are then one value per class)."""

  def __init__(self, rp, P, kf=None, dvals=None, facets=None, robin=(),
               neumann=(), node_indices=None):
    from swirl_fem_amd.core.interpolation import Nodes1D, NodeType
    from swirl_fem_amd.core.interpolation import Quadrature1D
    x = np.asarray(rp.node_coords, np.float64)
    d = x.shape[1]
    q = (P - 1) + (d + 1) // 2
    self.fes = fes = AR.space(x, rp.elements, P, (q, 'gl'))
    xq = AR.quad_points(fes)
    N = fes.num_nodes
    kq = None if kf is None else kf(xq)
    self.B = AR.assemble(fes, AR.element_matrices(fes, 1.0, 0.0))
    self.A = AR.assemble(fes, AR.element_matrices(fes, 0.0, 1.0, kq))
    self.b = np.zeros(N)
    grid = Nodes1D.create(P, NodeType.GAUSS_LOBATTO_LEGENDRE)
    quad = Quadrature1D.create(q, NodeType.GAUSS_LEGENDRE)

    def points(fr, g):
      pq, wj = BR.facet_quadrature(x, fr, grid, quad)
      return (np.asarray(g(pq.reshape(-1, d))).reshape(wj.shape)
              if callable(g) else np.full(wj.shape, float(g)))
    for group, alpha, g in robin:
      fr = facets[group]
      self.A = self.A + RR.robin_matrix(x, fr, grid, quad, alpha)
      self.b = self.b + BR.covector(x, fr, grid, quad, points(fr, g))
    for group, g in neumann:
      fr = facets[group]
      self.b = self.b + BR.covector(x, fr, grid, quad, points(fr, g))
    # periodic classes: R (N, classes) copies a class value to its images
    self.R = None
    if node_indices is not None:
      ni = np.asarray(node_indices, np.int64)
      masters, cls = np.unique(ni, return_inverse=True)
      self.R = np.zeros((N, len(masters)))
      self.R[np.arange(N), cls] = 1.0
      self.masters = masters
    dv = np.full(N, np.nan) if dvals is None else np.asarray(dvals, float)
    self.isd = ~np.isnan(dv)
    self.uD = np.where(self.isd, dv, 0.0)

  # ------------------------------------------------------------ operators
  def convection(self, u):
    """Dense C(u) for a velocity in any form of the stepper; None -> 0."""
    uq = point_velocity(self.fes, u)
    if uq is None:
      return np.zeros_like(self.B)
    return AR.assemble(self.fes, AR.advection_matrices(self.fes, uq))

  def source_vector(self, source):
    """B s for None, a scalar, nodal (N,) or point values (E, Q^d)."""
    fes = self.fes
    if source is None:
      return np.zeros(fes.num_nodes)
    s = np.asarray(source, np.float64)
    if s.shape == (fes.num_nodes,):
      return self.B @ s
    sq = np.broadcast_to(s, (fes.num_elements, fes.Q))
    return fes.scatter(np.einsum('qi,eq->ei', fes.M, wdet(fes) * sq))

  def rhs(self, levels, source=None):
    """The assembled vector of `TransportRhs.apply`: `levels` (T (N,), u,
    mass_coef, conv_coef)."""
    out = self.source_vector(source)
    mass = 0.0      # summed before B: the BDF terms of a steady state cancel
    for T, u, mc, cc in levels:
      mass = mass + mc * np.asarray(T, np.float64)
      if u is not None and cc != 0.0:
        out = out + cc * (self.convection(u) @ T)
    return out + self.B @ mass

  def _reduce(self, K, f):
    """Free-node system of K T = f with T = uD on the Dirichlet nodes, one
    unknown per periodic class: (K_ff, f_f, expand)."""
    f = f - K @ self.uD
    free = ~self.isd
    if self.R is None:
      def expand(w):
        T = self.uD.copy()
        T[free] = w
        return T
      return K[np.ix_(free, free)], f[free], expand
    R = self.R[:, free[self.masters]]

    def expand(w):
      return R @ w + self.uD
    return R.T @ K @ R, R.T @ f, expand

  def step_matrix(self, lambda0):
    return self._reduce(lambda0 * self.B + self.A, self.b)[0]

  def step(self, Ts, us, dt, order, source=None):
    """One BDF/EXT step of order `order` from the last `order` levels."""
    bdf, ext = coefficients(order)
    Ts, us = list(Ts)[-order:], list(us)[-order:]
    f = self.rhs([(T, u, -bdf[j] / dt, -ext[j])
                  for j, (T, u) in enumerate(zip(Ts, us))], source) + self.b
    K, g, expand = self._reduce((bdf[-1] / dt) * self.B + self.A, f)
    return expand(np.linalg.solve(K, g))

  def steady(self, u, source=None):
    """(A + C(u)) T = B s + b: the fixed point of the stepper."""
    K, g, expand = self._reduce(self.A + self.convection(u),
                                self.source_vector(source) + self.b)
    return expand(np.linalg.solve(K, g))

  def exact(self, T0, u, times, source=None):
    """The semi-discrete solution B dT/dt + (A + C(u)) T = B s + b at each of
    `times` from T(0) = T0, by the eigen-decomposition of B^-1 (A + C)."""
    Kfull = self.A + self.convection(u)
    K, g, expand = self._reduce(Kfull, self.source_vector(source) + self.b)
    Bff, _, _ = self._reduce(self.B, np.zeros_like(self.b))
    L = np.linalg.solve(Bff, K)
    lam, V = np.linalg.eig(L)
    Tstar = np.linalg.solve(K, g)
    free = ~self.isd
    if self.R is None:
      w0 = np.asarray(T0, np.float64)[free]
    else:
      w0 = np.asarray(T0, np.float64)[self.masters][free[self.masters]]
    c = np.linalg.solve(V, (w0 - Tstar).astype(complex))
    return [expand(Tstar + (V @ (np.exp(-lam * t) * c)).real) for t in times]


# ------------------------------------------------------------------ meshes
def _sides(ndim, periodic=()):
  names = ['x', 'y', 'z']

  def classify(c):
    for a in range(ndim):
      if a in periodic:
        continue
      if abs(c[a]) < 1e-9:
        return names[a] + '0'
      if abs(c[a] - 1) < 1e-9:
        return names[a] + '1'
    return None
  return classify


def box_with_sides(n, ndim, P, periodic=(), three_kinds=False):
  """The unit box of n^d elements with one physical group per side ('x0',
  'x1', 'y0', ...), refined to P GLL nodes per direction; `three_kinds`: the
  deformations of `geometry_cases.three_kinds` (they leave the box boundary
  in place)."""
  from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
  from swirl_fem_amd.core.interpolation import Nodes1D, NodeType
  from swirl_fem_amd.core.mesh_refiner import refine_premesh
  from tests import geometry_cases as G
  pm = unit_cube_mesh(n, ndim=ndim, periodic_dims=periodic)
  pm = pm.replace(physical_groups=BR.boundary_groups(pm,
                                                     _sides(ndim, periodic)))
  if three_kinds:
    pm = pm.replace(node_coords=G._move_centre_vertex(pm.node_coords, n))
  rp = refine_premesh(pm, Nodes1D.create(P, NodeType.GAUSS_LOBATTO_LEGENDRE))
  return G._bend_first_layer(rp, n) if three_kinds else rp
