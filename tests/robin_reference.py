"""NumPy restatement of the Robin facet mass term (tests only).

M_f = (B (x) B)^T diag(alpha wJ) (B (x) B) on every facet, from
`tests/bvp_reference.py`'s dense facet matrices and quadrature, assembled
into an (N, N) matrix.  In 1D a facet is a point and M_f = alpha there.
"""
import numpy as np

from tests import bvp_reference as R


def alpha_points(alpha, coords, facets, gridpoints_1d, quadrature):
  """alpha at the facet points (F, Q^k): a scalar, (N,) nodal values, point
  values or a NumPy callable on the (M, d) points."""
  coords = np.asarray(coords, np.float64)
  facets = np.asarray(facets)
  d = coords.shape[1]
  if d == 1:
    if callable(alpha):
      return np.asarray(alpha(coords[facets[:, 0]]), np.float64).reshape(-1, 1)
    a = np.asarray(alpha, np.float64)
    if a.ndim == 0:
      return np.full((len(facets), 1), float(a))
    return a[facets[:, 0]].reshape(-1, 1) if a.shape == (len(coords),) else a
  xq, wj = R.facet_quadrature(coords, facets, gridpoints_1d, quadrature)
  if callable(alpha):
    return np.asarray(alpha(xq.reshape(-1, d)), np.float64).reshape(wj.shape)
  a = np.asarray(alpha, np.float64)
  if a.ndim == 0:
    return np.full(wj.shape, float(a))
  if a.shape == (len(coords),):
    B, _, _ = R.facet_matrices(gridpoints_1d, quadrature, d - 1)
    return np.einsum('qi,fi->fq', B, a[facets])
  return a


def facet_mass(coords, facets, gridpoints_1d, quadrature, alpha):
  """(F, n, n) dense facet matrices."""
  coords = np.asarray(coords, np.float64)
  facets = np.asarray(facets)
  a = alpha_points(alpha, coords, facets, gridpoints_1d, quadrature)
  if coords.shape[1] == 1:
    return a.reshape(-1, 1, 1)
  B, _, _ = R.facet_matrices(gridpoints_1d, quadrature, coords.shape[1] - 1)
  _, wj = R.facet_quadrature(coords, facets, gridpoints_1d, quadrature)
  return np.einsum('qi,fq,qj->fij', B, a * wj, B)


def assemble(mats, facets, num_nodes, dirichlet=None):
  """(N, N) sum of the facet matrices; `dirichlet` (N,) bool rows and
  columns zero."""
  facets = np.asarray(facets, np.int64)
  A = np.zeros((num_nodes, num_nodes))
  for f, m in zip(facets, mats):
    A[np.ix_(f, f)] += m
  if dirichlet is not None:
    keep = ~np.asarray(dirichlet, bool)
    A = A * keep[:, None] * keep[None, :]
  return A


def robin_matrix(coords, facets, gridpoints_1d, quadrature, alpha,
                 dirichlet=None):
  """The assembled (N, N) Robin term <alpha u, v> of one group."""
  mats = facet_mass(coords, facets, gridpoints_1d, quadrature, alpha)
  return assemble(mats, facets, len(coords), dirichlet)
