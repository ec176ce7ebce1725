"""NumPy reference of linear elasticity,

    K + lambda0 M_rho,   v^T K u = int sigma(u) : grad v,
    sigma = lambda tr(eps) I + 2 mu eps,   eps = (grad u + grad u^T) / 2,

on the oracle space of `tests/coefficient_reference.py` (same geometry, same
index convention: phys = einsum('qid,eqjd->eqij', G, invjacs) are the physical
gradients of the basis).  Displacements are (N, d) nodal or (E, n, d) element
values; an element matrix is (n d, n d) with the unknown (node i, component c)
at i d + c.  `lam`, `mu`, `rho`: a scalar or (E, Q) values at the quadrature
points (`rho` None = 1).

* `element_matrices`, `local_apply`, `apply`, `diagonal`, `assemble`: dense,
  from the physical gradients;
* `grid_apply`: what the kernel `sfem_elasticity_local` computes on the Q^d
  quadrature grid, sum-factorised with the 1D derivative matrix of the Q
  points (as `transport_reference.integrand`), optionally in float32;
* `pcg`: dense preconditioned conjugate gradients with an optional Jacobi
  preconditioner, for iteration counts.
"""

import numpy as np

from tests import advection_reference as AR
from tests import coefficient_reference as R
from tests.sumfact_reference import _along
from tests.transport_reference import quadrature_dmat

space = R.space
quad_points = R.quad_points
_phys, _wdet = AR._phys, AR._wdet


def _points(fes, c, default=None):
  """A coefficient as (E, Q)."""
  if c is None:
    c = default
  return np.broadcast_to(np.asarray(c, np.float64),
                         (fes.num_elements, fes.Q))


def stress(H, lam, mu):
  """sigma (..., d, d) of displacement gradients H[..., c, j] = d u_c / d x_j
  with lam, mu broadcast over the leading axes."""
  d = H.shape[-1]
  tr = np.trace(H, axis1=-2, axis2=-1)
  return (np.asarray(lam)[..., None, None] * tr[..., None, None] * np.eye(d) +
          np.asarray(mu)[..., None, None] * (H + np.swapaxes(H, -1, -2)))


def element_matrices(fes, lam, mu, rho=None, lambda0=0.0):
  """(E, n d, n d) dense element matrices of K + lambda0 M_rho."""
  W = _wdet(fes)
  E, Q = W.shape
  n, d = fes.M.shape[1], fes.ndim
  lam, mu, rho = _points(fes, lam), _points(fes, mu), _points(fes, rho, 1.0)
  out = np.zeros((E, n, d, n, d))
  for e in range(E):
    ph = np.einsum('qid,qjd->qij', fes.G, fes.invjacs[e])         # (Q, n, d)
    lap = np.einsum('q,qij,qkj->ik', W[e] * mu[e], ph, ph)
    for c in range(d):
      out[e, :, c, :, c] += lap
      if lambda0:
        out[e, :, c, :, c] += lambda0 * (fes.M.T * (W[e] * rho[e])) @ fes.M
    out[e] += np.einsum('q,qic,qkb->ickb', W[e] * lam[e], ph, ph)
    out[e] += np.einsum('q,qib,qkc->ickb', W[e] * mu[e], ph, ph)
  return out.reshape(E, n * d, n * d)


def local_apply(fes, u_local, lam, mu, rho=None, lambda0=0.0):
  """(E, n, d) -> (E, n, d): the element action of K + lambda0 M_rho."""
  W, ph = _wdet(fes), _phys(fes)
  lam, mu, rho = _points(fes, lam), _points(fes, mu), _points(fes, rho, 1.0)
  H = np.einsum('eqij,eic->eqcj', ph, u_local, optimize=True)
  S = stress(H, lam, mu)
  out = np.einsum('eq,eqcj,eqij->eic', W, S, ph, optimize=True)
  if lambda0:
    v = np.einsum('qi,eic->eqc', fes.M, u_local)
    out = out + lambda0 * np.einsum('qi,eqc->eic', fes.M,
                                    (W * rho)[..., None] * v)
  return out


def apply(fes, u, lam, mu, rho=None, lambda0=0.0, keep=None):
  """Assembled (N, d) action; `keep` (N, d): 0 on the fixed components."""
  out = fes.scatter(local_apply(fes, fes.gather(u), lam, mu, rho, lambda0))
  return out if keep is None else out * keep


def diagonal(fes, lam, mu, rho=None, lambda0=0.0, keep=None):
  """Assembled (N, d) diagonal of K + lambda0 M_rho."""
  W, ph = _wdet(fes), _phys(fes)
  lam, mu, rho = _points(fes, lam), _points(fes, mu), _points(fes, rho, 1.0)
  lap = np.einsum('eq,eqij,eqij->ei', W * mu, ph, ph, optimize=True)
  d = lap[..., None] + np.einsum('eq,eqic,eqic->eic', W * (lam + mu), ph, ph,
                                 optimize=True)
  if lambda0:
    d = d + lambda0 * np.einsum('eq,qi->ei', W * rho, fes.M ** 2)[..., None]
  out = fes.scatter(d)
  return out if keep is None else out * keep


def assemble(fes, mats):
  """(N d, N d) dense matrix from (E, n d, n d) element matrices; the unknown
  (node i, component c) at i d + c; padding slots skipped."""
  d = fes.ndim
  N = fes.num_nodes
  A = np.zeros((N * d, N * d))
  for row, m in zip(np.asarray(fes.elements, np.int64), mats):
    ok = np.repeat(row >= 0, d)
    dofs = (row[:, None] * d + np.arange(d)[None, :]).reshape(-1)
    A[np.ix_(dofs[ok], dofs[ok])] += m[np.ix_(ok, ok)]
  return A


def grid_apply(fes, u_q, lam, mu, rho=None, lambda0=0.0, dtype=np.float64):
  """`u_q` (E, Q^d, d) on the quadrature grid of the oracle space `fes` ->
  (E, Q^d, d), the steps of the kernel evaluated in `dtype`:
  G[c][a] = D_a u_c, H = J^-T G, S = stress(H), F[c][a] = W sum_j
  (d xi_a / d x_j) S[c][j], out_c = sum_a D_a^T F[c][a] + lambda0 rho W u_c."""
  d = fes.ndim
  W = _wdet(fes).astype(dtype)
  E, nq = W.shape
  Q = round(nq ** (1.0 / d))
  assert Q ** d == nq
  D = quadrature_dmat(Q).astype(dtype)
  ij = fes.invjacs.astype(dtype)                     # [e,q,j,a] = d xi_a / d x_j
  lam = _points(fes, lam).astype(dtype)
  mu = _points(fes, mu).astype(dtype)
  rho = _points(fes, rho, 1.0).astype(dtype)
  u_q = np.asarray(u_q, dtype)
  grid = np.moveaxis(u_q, -1, 1).reshape((E, d) + (Q,) * d)
  G = np.stack([_along(D, grid, 2 + a).reshape(E, d, nq) for a in range(d)],
               axis=-1)                               # (E, c, q, a)
  H = np.einsum('eqja,ecqa->eqcj', ij, G)
  S = stress(H, lam, mu).astype(dtype)
  F = np.einsum('eq,eqja,eqcj->ecaq', W, ij, S).astype(dtype)
  out = np.zeros((E, d, nq), dtype)
  Dt = np.ascontiguousarray(D.T)
  for a in range(d):
    fa = F[:, :, a].reshape((E, d) + (Q,) * d)
    out += _along(Dt, fa, 2 + a).reshape(E, d, nq)
  out = np.moveaxis(out, 1, -1)
  if lambda0:
    out = out + dtype(lambda0) * (rho * W)[..., None] * u_q
  return out


def pcg(A, b, rtol=1e-8, jacobi=False, maxiter=None):
  """Dense (preconditioned) conjugate gradients from x = 0 with the stopping
  rule of `linalg.cg`: r . M r <= rtol^2 b . b (M = 1 / diag A scaled by its
  largest diagonal entry, as `JacobiPreconditioner(strict=True)`, or the
  identity).  Returns (x, iterations)."""
  A = np.asarray(A, np.float64)
  b = np.asarray(b, np.float64)
  dg = np.diag(A)
  dinv = dg.max() / dg if jacobi else np.ones_like(b)
  x = np.zeros_like(b)
  r = b.copy()
  z = dinv * r
  p = z.copy()
  gamma = r @ z
  stop = rtol ** 2 * (b @ b)
  k = 0
  maxiter = 10 * len(b) if maxiter is None else maxiter
  while gamma > stop and k < maxiter:
    Ap = A @ p
    alpha = gamma / (p @ Ap)
    x += alpha * p
    r -= alpha * Ap
    z = dinv * r
    new = r @ z
    p = z + (new / gamma) * p
    gamma = new
    k += 1
  return x, k


# ------------------------------------------------------------------ meshes
def jittered_box(n, ndim, P):
  """The unit box of n^d elements with one physical group per side ('x0',
  'x1', 'y0', ...) and one interior vertex moved (its 2^d elements become
  multilinear; the box boundary stays in place), refined to P GLL nodes."""
  from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
  from swirl_fem_amd.core.interpolation import Nodes1D, NodeType
  from swirl_fem_amd.core.mesh_refiner import refine_premesh
  from tests import bvp_reference as BR
  from tests import geometry_cases as G
  from tests.transport_reference import _sides
  pm = unit_cube_mesh(n, ndim=ndim)
  pm = pm.replace(physical_groups=BR.boundary_groups(pm, _sides(ndim)))
  pm = pm.replace(node_coords=G._move_centre_vertex(pm.node_coords, n))
  return refine_premesh(pm, Nodes1D.create(P, NodeType.GAUSS_LOBATTO_LEGENDRE))


class Dense:
  """The assembled elasticity problem on a refined premesh `rp` with P nodes
  per direction and the Gauss rule of `solve_elasticity`: K + lambda0 M_rho,
  the plain mass matrix B, tractions by `bvp_reference.covector`, the
  Dirichlet lift and `numpy.linalg.solve`."""

  def __init__(self, rp, P, lam, mu, rho=None, lambda0=0.0):
    from swirl_fem_amd.core.interpolation import Nodes1D, NodeType
    from swirl_fem_amd.core.interpolation import Quadrature1D
    self.x = x = np.asarray(rp.node_coords, np.float64)
    self.d = d = x.shape[1]
    q = (P - 1) + (d + 1) // 2
    self.fes = fes = space(x, rp.elements, P, (q, 'gl'))
    co = lambda c: c(quad_points(fes)) if callable(c) else c
    self.coefs = (co(lam), co(mu), co(rho))
    self.A = assemble(fes, element_matrices(fes, *self.coefs, lambda0))
    self.B = assemble(fes, element_matrices(fes, 0.0, 0.0, 1.0, 1.0))
    self.grid = Nodes1D.create(P, NodeType.GAUSS_LOBATTO_LEGENDRE)
    self.quad = Quadrature1D.create(q, NodeType.GAUSS_LEGENDRE)

  def traction(self, facets, t):
    """(N, d) covector of a traction: entries None, a scalar or a NumPy
    callable on the (M, d) facet points."""
    from tests import bvp_reference as BR
    out = np.zeros_like(self.x)
    pq, wj = BR.facet_quadrature(self.x, facets, self.grid, self.quad)
    for c, g in enumerate(t):
      if g is None:
        continue
      vals = (np.asarray(g(pq.reshape(-1, self.d))).reshape(wj.shape)
              if callable(g) else np.full(wj.shape, float(g)))
      out[:, c] = BR.covector(self.x, facets, self.grid, self.quad, vals)
    return out

  def system(self, force, fixed, values, tractions=()):
    """(free-dof matrix, right-hand side, expand) for nodal `force` (N, d),
    `fixed` (N, d) bool, `values` (N, d) and [(facets, t)] tractions."""
    rhs = (self.B @ np.asarray(force, np.float64).reshape(-1)).reshape(
        self.x.shape)
    for facets, t in tractions:
      rhs = rhs + self.traction(facets, t)
    fx = np.asarray(fixed, bool).reshape(-1)
    uD = np.where(fx, np.asarray(values, np.float64).reshape(-1), 0.0)
    b = rhs.reshape(-1) - self.A @ uD
    free = ~fx

    def expand(w):
      u = uD.copy()
      u[free] = w
      return u.reshape(self.x.shape)
    return self.A[np.ix_(free, free)], b[free], expand

  def solve(self, force, fixed, values, tractions=()):
    K, b, expand = self.system(force, fixed, values, tractions)
    return expand(np.linalg.solve(K, b))


def jacobi_case():
  """The case of the Jacobi test: 2 x 2 deformed elements of order 3 in 2D,
  mu = 1 and 1e3 on alternating elements, lambda = 2 mu, clamped on x0 under
  its own weight.  Returns (rp, P, mu per element (E,), body force (d,))."""
  from tests.transport_reference import box_with_sides
  P = 4
  rp = box_with_sides(2, 2, P, three_kinds=True)
  E = rp.elements.shape[0]
  mu = np.where(np.arange(E) % 2 == 0, 1.0, 1e3)
  return rp, P, mu, np.array([0.0, -1.0])
