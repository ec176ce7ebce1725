"""Host checks of the advective term's references: the NumPy operator
(`tests/advection_reference.py`) and the NumPy BiCGStab
(`tests/bicgstab_reference.py`) that the GPU tests compare against."""
import numpy as np

from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType
from swirl_fem_amd.core.mesh_refiner import refine_premesh
from tests import advection_reference as AR
from tests import bicgstab_reference as BS
from tests import coefficient_reference as R
from tests import geometry_cases as G

GLL = NodeType.GAUSS_LOBATTO_LEGENDRE


def _velocity(fes, rng):
  xq = AR.quad_points(fes)
  return np.stack([1.0 + xq[..., 0] * xq[..., -1], np.sin(2.0 * xq[..., 0])] +
                  ([0.5 - xq[..., 1] ** 2] if fes.ndim == 3 else []), axis=-1)


def test_constant_field_is_annihilated():
  for ndim, P, quad in ((2, 4, (4, 'gll')), (3, 3, (4, 'gl'))):
    rp = G.three_kinds(3, ndim, P).rp
    fes = AR.space(rp.node_coords, rp.elements, P, quad)
    b = _velocity(fes, None)
    out = AR.apply(fes, np.ones(fes.num_nodes), 0.0, 0.0, b_q=b)
    scale = np.abs(AR.apply(fes, rp.node_coords[:, 0], 0.0, 0.0, b_q=b)).max()
    assert np.abs(out).max() <= 1e-12 * scale


def test_local_apply_equals_dense_matrices():
  rng = np.random.default_rng(0)
  for ndim, P, quad in ((2, 5, (5, 'gll')), (3, 3, (4, 'gl'))):
    rp = G.three_kinds(3, ndim, P).rp
    fes = AR.space(rp.node_coords, rp.elements, P, quad)
    b = _velocity(fes, rng)
    xq = AR.quad_points(fes)
    k, c = 1.0 + xq[..., 0] ** 2, 0.5 + xq[..., -1]
    ul = rng.standard_normal((fes.num_elements, fes.n))
    want = np.einsum('eij,ej->ei',
                     AR.element_matrices(fes, 0.7, 1.3, k, c, b), ul)
    got = AR.local_apply(fes, ul, 0.7, 1.3, k, c, b)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # without a velocity: the matrices of the coefficient reference
    m0 = R.element_matrices(fes, 0.7, 1.3, k, c)
    assert np.abs(AR.element_matrices(fes, 0.7, 1.3, k, c) - m0).max() <= \
        1e-12 * np.abs(m0).max()
    # ... and the diagonal is the diagonal of the assembled matrices
    A = AR.assemble(fes, AR.element_matrices(fes, 0.7, 1.3, k, c, b))
    d = AR.diagonal(fes, 0.7, 1.3, k, c, b)
    assert np.abs(d - np.diag(A)).max() <= 1e-12 * np.abs(d).max()
    u = rng.standard_normal(fes.num_nodes)
    assert np.abs(A @ u - AR.apply(fes, u, 0.7, 1.3, k, c, b)).max() <= \
        1e-12 * np.abs(A @ u).max()


def test_collocated_diagonal_equals_diagonal():
  """The closed form the order sweep uses where `diagonal`'s (E, Q, n, d)
  array is too large, pinned to `diagonal`: every term alone and together,
  with and without coefficients and a mask."""
  rng = np.random.default_rng(2)
  for ndim, P in ((2, 5), (3, 3)):
    rp = G.three_kinds(3, ndim, P).rp
    fes = AR.space(rp.node_coords, rp.elements, P, (P, 'gll'))
    b = _velocity(fes, rng)
    xq = AR.quad_points(fes)
    k, c = 1.0 + xq[..., 0] ** 2, 0.5 + xq[..., -1]
    keep = (rng.random(fes.num_nodes) > 0.2).astype(np.float64)
    for l0, l1, kq, cq, bq, kp in ((0.7, 1.3, k, c, b, keep),
                                   (0.7, 1.3, None, None, b, None),
                                   (0.0, 0.0, None, None, b, None),
                                   (1.0, 0.0, None, c, None, None),
                                   (0.0, 1.0, k, None, None, keep)):
      want = AR.diagonal(fes, l0, l1, kq, cq, bq, kp)
      got = AR.collocated_diagonal(fes, l0, l1, kq, cq, bq, kp)
      assert np.abs(want).max() > 0
      assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max(), (ndim, l0)


def test_divergence_free_velocity_is_skew_on_the_interior():
  """int (b . grad u) v + (b . grad v) u = int b . grad(uv) = -int div(b) uv
  + boundary terms: for div b = 0 the interior block of C_b + C_b^T is 0,
  exactly so with a quadrature that integrates the polynomial integrand."""
  P = 4
  pm = unit_cube_mesh(3, ndim=2)
  rp = refine_premesh(pm, Nodes1D.create(P, GLL))
  fes = AR.space(rp.node_coords, rp.elements, P, (P + 2, 'gl'))
  xq = AR.quad_points(fes)
  x, y = xq[..., 0], xq[..., 1]
  # b = curl of the stream function x^2 y^2 / 2 + x y: (psi_y, -psi_x)
  b = np.stack([x * x * y + x, -(x * y * y + y)], axis=-1)
  C = AR.assemble(fes, AR.advection_matrices(fes, b))
  X = np.asarray(rp.node_coords)
  inner = np.all((X > 1e-9) & (X < 1 - 1e-9), axis=1)
  S = (C + C.T)[np.ix_(inner, inner)]
  assert inner.sum() > 0
  assert np.abs(S).max() <= 1e-13 * np.abs(C).max()


def test_numpy_bicgstab_solves_nonsymmetric_system():
  rng = np.random.default_rng(4)
  n = 40
  A = rng.standard_normal((n, n))
  A += np.diag(np.abs(A).sum(axis=1) + 1.0)
  assert np.abs(A - A.T).max() > 0.1
  b = rng.standard_normal(n)
  want = np.linalg.solve(A, b)
  for M in (None, lambda v: v / np.diag(A)):
    x, its, status = BS.bicgstab(lambda v: A @ v, b, tol=1e-14, M=M)
    assert status == 'converged'
    assert 0 < len(its) < 10 * n
    assert np.abs(x - want).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(its[-1], x)
  x, its, status = BS.bicgstab(lambda v: A @ v, np.zeros(n))
  assert status == 'converged' and not its and not x.any()


def test_numpy_bicgstab_names_a_breakdown():
  # a skew-symmetric A: r0 . v = b . A b = 0 in the first iteration
  A = np.array([[0.0, 1.0], [-1.0, 0.0]])
  x, its, status = BS.bicgstab(lambda v: A @ v, np.array([1.0, 2.0]))
  assert status == 'breakdown_alpha'
  assert np.isfinite(x).all()
