"""Host-side checks of linear elasticity: the NumPy reference
(`tests/elasticity_reference.py`) against properties that need no second
implementation -- symmetry, rigid-body modes, the patch test, the scalar
operators it contains -- so that the GPU tests rest on something verified;
`lame_parameters`; the refusals of `solve_elasticity` that need no device;
the header, the ctypes mirror and the ABI number."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from swirl_fem_amd import _lib
from swirl_fem_amd.core import operators
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType, Quadrature1D
from swirl_fem_amd.examples.elasticity import BCType, solve_elasticity
from tests import advection_reference as AR
from tests import bvp_reference as BR
from tests import coefficient_reference as R
from tests import elasticity_reference as ER
from tests import geometry_cases as G
from tests import transport_reference as TR

P = 3
CASES = [('multilinear', 2), ('multilinear', 3), ('three_kinds', 2),
         ('three_kinds', 3), ('affine', 3)]


def _space(kind, ndim):
  case = getattr(G, kind)(2, ndim, P)
  q = P - 1 + (ndim + 1) // 2
  return case.rp, ER.space(case.rp.node_coords, case.rp.elements, P, (q, 'gl'))


def _coefficients(fes, rng):
  xq = ER.quad_points(fes)
  lam = 1.0 + 0.5 * np.sin(2.0 * xq[..., 0]) + rng.uniform(
      0, 0.2, xq.shape[:2])
  mu = 0.7 + 0.3 * xq[..., 1] ** 2
  rho = 1.5 + np.cos(xq[..., 0])
  return lam, mu, rho


def _rigid_modes(x):
  """Translations and infinitesimal rotations at the nodes, (modes, N, d)."""
  N, d = x.shape
  modes = [np.tile(np.eye(d)[c], (N, 1)) for c in range(d)]
  for a in range(d):
    for b in range(a + 1, d):
      r = np.zeros((N, d))
      r[:, a], r[:, b] = -x[:, b], x[:, a]
      modes.append(r)
  return np.stack(modes)


@pytest.mark.parametrize('kind,ndim', CASES)
def test_element_matrices(kind, ndim):
  """K_e is symmetric to 1e-13, agrees with `local_apply`, and its diagonal
  is `diagonal`; variable coefficients and a mass term."""
  rp, fes = _space(kind, ndim)
  rng = np.random.default_rng(ndim)
  lam, mu, rho = _coefficients(fes, rng)
  for l0 in (0.0, 2.5):
    Ke = ER.element_matrices(fes, lam, mu, rho, l0)
    scale = np.abs(Ke).max()
    assert np.abs(Ke - Ke.transpose(0, 2, 1)).max() <= 1e-13 * scale
    u = rng.standard_normal((fes.num_elements, fes.n, ndim))
    want = np.einsum('eij,ej->ei', Ke, u.reshape(fes.num_elements, -1))
    got = ER.local_apply(fes, u, lam, mu, rho, l0)
    assert np.abs(got.reshape(want.shape) - want).max() <= 1e-12 * np.abs(
        want).max()
    A = ER.assemble(fes, Ke)
    dg = ER.diagonal(fes, lam, mu, rho, l0)
    assert np.abs(dg.reshape(-1) - np.diag(A)).max() <= 1e-13 * np.abs(
        dg).max()
    v = rng.standard_normal((fes.num_nodes, ndim))
    keep = (rng.uniform(size=v.shape) > 0.3).astype(float)
    got = ER.apply(fes, v, lam, mu, rho, l0, keep)
    want = (A @ v.reshape(-1)).reshape(v.shape) * keep
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize('kind,ndim', CASES)
def test_rigid_body_modes(kind, ndim):
  """Translations and infinitesimal rotations lie in the null space of the
  assembled K: relative residual <= 1e-12.  The elements are isoparametric,
  so a rigid motion is in the space and its strain vanishes at every
  quadrature point whatever the rule: the bound of the multilinear elements
  holds on the curved ones too (nothing is left to the quadrature)."""
  rp, fes = _space(kind, ndim)
  lam, mu, _ = _coefficients(fes, np.random.default_rng(1))
  A = ER.assemble(fes, ER.element_matrices(fes, lam, mu))
  x = np.asarray(rp.node_coords, np.float64)
  modes = _rigid_modes(x)
  assert len(modes) == ndim * (ndim + 1) // 2
  for m in modes:
    res = A @ m.reshape(-1)
    rel = np.abs(res).max() / (np.abs(A).sum(axis=1).max() * np.abs(m).max())
    assert rel <= 1e-12, (kind, ndim, rel)
  # and nothing else: the null space has exactly those dimensions
  w = np.linalg.eigvalsh(A)
  assert (np.abs(w) <= 1e-10 * w.max()).sum() == len(modes)
  assert w.min() >= -1e-10 * w.max()


@pytest.mark.parametrize('ndim', [2, 3])
def test_patch_test(ndim):
  """A linear displacement has a constant stress S: `apply` is int (S n) . v
  over the boundary (`bvp_reference.covector` with the facet normals) and
  zero at interior nodes.  With P = 3 the integrands on the bent elements
  have degree <= 6 per direction and the Gauss rules (4 points in 3D: degree
  7; 3 in 2D, degree <= 4 there) integrate them exactly."""
  rp = TR.box_with_sides(2, ndim, P, three_kinds=True)
  x = np.asarray(rp.node_coords, np.float64)
  q = P - 1 + (ndim + 1) // 2
  fes = ER.space(x, rp.elements, P, (q, 'gl'))
  rng = np.random.default_rng(ndim)
  Amat = rng.standard_normal((ndim, ndim))
  u = x @ Amat.T + rng.standard_normal(ndim)          # H[c][j] = Amat[c, j]
  lam, mu = 1.3, 0.6
  S = ER.stress(Amat, lam, mu)
  got = ER.apply(fes, u, lam, mu)
  mesh = rp.finalize(device='cpu')
  grid = Nodes1D.create(P, NodeType.GAUSS_LOBATTO_LEGENDRE)
  quad = Quadrature1D.create(q, NodeType.GAUSS_LEGENDRE)
  want = np.zeros_like(got)
  on_boundary = np.zeros(len(x), bool)
  sides = [s for s in mesh.boundary_facets if len(s) == 2]
  assert len(sides) == 2 * ndim
  for side in sides:
    fr = mesh.boundary_facets[side].numpy().astype(np.int64)
    on_boundary[fr.reshape(-1)] = True
    nrm = BR.facet_normals(x, fr, rp.elements, grid, quad)
    t = np.einsum('cj,fqj->fqc', S, nrm)
    for c in range(ndim):
      want[:, c] += BR.covector(x, fr, grid, quad, t[..., c])
  scale = np.abs(want).max()
  assert scale > 1e-2
  assert np.abs(got - want).max() <= 1e-12 * scale
  assert np.abs(got[~on_boundary]).max() <= 1e-12 * scale
  assert (~on_boundary).sum() > 0


@pytest.mark.parametrize('kind,ndim', [('three_kinds', 2), ('three_kinds', 3)])
def test_reduces_to_scalar_operators(kind, ndim):
  """The diagonal block of component i is the scalar operator with the
  tensor mu I + (lambda + mu) e_i e_i^T: K_ii = A_mu + A_ii(lambda + mu),
  A_ii[k,l] = int (lambda + mu) d_i phi_k d_i phi_l; with lambda = 0 that is
  mu (A + A_ii).  Summed over i: (d + 1) A_mu + A_lambda, the Laplacian of
  `coefficient_reference` with k = (d + 1) mu + lambda; the mass term is
  lambda0 B_rho in every block."""
  rp, fes = _space(kind, ndim)
  lam, mu, rho = _coefficients(fes, np.random.default_rng(5))
  E, n, d = fes.num_elements, fes.n, ndim
  ph, W = AR._phys(fes), AR._wdet(fes)
  for lm, l0 in ((0.0 * lam, 0.0), (lam, 1.7)):
    Ke = ER.element_matrices(fes, lm, mu, rho, l0).reshape(E, n, d, n, d)
    A_mu = R.element_matrices(fes, 0.0, 1.0, k_q=mu)
    B = R.element_matrices(fes, l0, 0.0, c_q=rho) if l0 else 0.0
    total = 0.0
    for i in range(d):
      Aii = np.einsum('eq,eqk,eql->ekl', W * (lm + mu), ph[..., i],
                      ph[..., i])
      want = A_mu + Aii + B
      got = Ke[:, :, i, :, i]
      assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
      total = total + got
    want = AR.element_matrices(fes, l0 * d, 1.0, k_q=(d + 1) * mu + lm,
                               c_q=rho)
    assert np.abs(total - want).max() <= 1e-13 * np.abs(want).max()


@pytest.mark.parametrize('ndim,Q', [(2, 3), (2, 5), (3, 4)])
def test_grid_apply_is_the_two_grid_form(ndim, Q):
  """M^T grid_apply(M u) = local_apply(u): the sum-factorised steps of the
  kernel on the quadrature grid are the dense element action (Q >= P: the
  derivative of the interpolant on the q-grid is exact)."""
  case = G.three_kinds(2, ndim, P)
  fes = ER.space(case.rp.node_coords, case.rp.elements, P, (Q, 'gl'))
  rng = np.random.default_rng(Q)
  lam, mu, rho = _coefficients(fes, rng)
  u = rng.standard_normal((fes.num_elements, fes.n, ndim))
  uq = np.einsum('qi,eic->eqc', fes.M, u)
  for l0 in (0.0, 0.8):
    got = np.einsum('qi,eqc->eic', fes.M,
                    ER.grid_apply(fes, uq, lam, mu, rho, l0))
    want = ER.local_apply(fes, u, lam, mu, rho, l0)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_pcg_solves():
  """The dense PCG of the reference reaches the direct solution, with and
  without the Jacobi preconditioner."""
  rp, fes = _space('multilinear', 2)
  A = ER.assemble(fes, ER.element_matrices(fes, 1.0, 0.5, 1.0, 3.0))
  b = np.random.default_rng(0).standard_normal(len(A))
  want = np.linalg.solve(A, b)
  for jac in (False, True):
    x, k = ER.pcg(A, b, rtol=1e-12, jacobi=jac)
    assert 0 < k < 10 * len(b)
    assert np.abs(x - want).max() <= 1e-8 * np.abs(want).max()


def test_lame_parameters():
  lam, mu = operators.lame_parameters(1.0, 0.25)
  assert abs(mu - 0.4) <= 1e-15 and abs(lam - 0.4) <= 1e-15
  lam, mu = operators.lame_parameters(210.0, 0.3)
  assert abs(mu - 210.0 / 2.6) <= 1e-12
  assert abs(lam - 210.0 * 0.3 / (1.3 * 0.4)) <= 1e-12
  # E and nu back from (lambda, mu)
  assert abs(mu * (3 * lam + 2 * mu) / (lam + mu) - 210.0) <= 1e-11
  assert abs(lam / (2 * (lam + mu)) - 0.3) <= 1e-14
  ls, ms = operators.lame_parameters(210.0, 0.3, plane_stress=True)
  assert ms == mu
  assert abs(ls - 2 * lam * mu / (lam + 2 * mu)) <= 1e-12
  assert abs(ls - 210.0 * 0.3 / (1 - 0.09)) <= 1e-11
  lam0, mu0 = operators.lame_parameters(2.0, 0.0, plane_stress=True)
  assert lam0 == 0.0 and mu0 == 1.0


# ------------------------------------------------------------- refusals
@pytest.fixture(scope='module')
def cpu_mesh():
  return TR.box_with_sides(2, 2, P).finalize(device='cpu')


def test_solve_refusals(cpu_mesh):
  """What `solve_elasticity` refuses before it touches a device."""
  D, N = BCType.DIRICHLET, BCType.NEUMANN
  kw = dict(lame_lambda=1.0, lame_mu=1.0)
  clamp = {'x0': (D, (0.0, 0.0))}
  f = (0.0, -1.0)
  with pytest.raises(ValueError, match='rigid-body'):
    solve_elasticity(cpu_mesh, f, {}, **kw)
  with pytest.raises(ValueError, match='rigid-body'):
    solve_elasticity(cpu_mesh, f, {'x1': (N, (1.0, None))}, **kw)
  with pytest.raises(ValueError, match='rigid-body'):      # every entry free
    solve_elasticity(cpu_mesh, f, {'x0': (D, (None, None))}, **kw)
  with pytest.raises(ValueError, match='DIRICHLET or NEUMANN'):
    solve_elasticity(cpu_mesh, f, {'x0': (BCType.ROBIN, (0.0, 0.0))}, **kw)
  with pytest.raises(ValueError, match='one entry per component'):
    solve_elasticity(cpu_mesh, f, {'x0': (D, (0.0, 0.0, 0.0))}, **kw)
  with pytest.raises(ValueError, match='one entry per component'):
    solve_elasticity(cpu_mesh, f, {'x0': (D, 0.0)}, **kw)
  with pytest.raises(ValueError, match='one entry per component'):
    solve_elasticity(cpu_mesh, f, {'x1': (N, (1.0,))}, **kw)
  with pytest.raises(KeyError):
    solve_elasticity(cpu_mesh, f, {'nowhere': (D, (0.0, 0.0))}, **kw)
  with pytest.raises(NotImplementedError, match='pmg'):
    solve_elasticity(cpu_mesh, f, clamp, preconditioner='pmg', **kw)
  with pytest.raises(ValueError, match='unknown preconditioner'):
    solve_elasticity(cpu_mesh, f, clamp, preconditioner='ilu', **kw)
  with pytest.raises(NotImplementedError, match='ensemble'):
    solve_elasticity(cpu_mesh.replicate(2), f, clamp, **kw)


def test_solve_refuses_partitions_and_periodic_images():
  from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
  from swirl_fem_amd.core.mesh_refiner import refine_premesh
  from swirl_fem_amd.distributed import blocks
  kw = dict(lame_lambda=1.0, lame_mu=1.0)
  part = blocks.build_block_partition(2, 3, (2, 1, 1), 0, device='cpu')
  with pytest.raises(NotImplementedError, match='partitioned'):
    solve_elasticity(part.mesh, (0.0, 0.0, 1.0), {}, lambda0=1.0, **kw)
  pm = unit_cube_mesh(2, ndim=2, periodic_dims=(0,))
  mesh = refine_premesh(pm, Nodes1D.create(
      P, NodeType.GAUSS_LOBATTO_LEGENDRE)).finalize(device='cpu')
  with pytest.raises(NotImplementedError, match='periodic'):
    solve_elasticity(mesh, (0.0, 1.0), {}, lambda0=1.0, **kw)


# ------------------------------------------------------- header and ABI
def test_struct_layout():
  """`sfem_elasticity_args` in the header and its ctypes mirror: the same
  fields in the same order; the ABI number is unchanged (a pure addition)."""
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  text = open(os.path.join(root, 'include', 'sfem.h')).read()
  assert '#define SFEM_ABI_VERSION 10' in text and _lib.ABI_VERSION == 10
  body = re.search(r'typedef struct sfem_elasticity_args \{(.*?)\} '
                   r'sfem_elasticity_args;', text, flags=re.S).group(1)
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  names = []
  for decl in body.split(';'):
    decl = decl.strip()
    if not decl:
      continue
    first, *rest = decl.split(',')
    names.append(re.findall(r'\w+', first)[-1])
    names += [r.strip() for r in rest]
  fields = _lib.ElasticityArgs._fields_
  assert names == [f[0] for f in fields], (names, fields)
  kinds = dict(fields)
  for name in ('lam_const', 'mu_const', 'rho_const', 'lambda0'):
    assert kinds[name] is ctypes.c_double
  assert kinds['num_elements'] is _lib.c_i64 and kinds['P'] is _lib.c_i32
  # 13 pointers, 4 doubles, 2 int64, 4 int32
  assert ctypes.sizeof(_lib.ElasticityArgs) == 13 * 8 + 4 * 8 + 16 + 16
  sig = _lib.SIGNATURES['sfem_elasticity_local']
  assert sig[0]._type_ is _lib.ElasticityArgs and sig[1] is _lib.c_ptr
  assert re.search(r'int sfem_elasticity_local\(const sfem_elasticity_args\* '
                   r'args,\s*sfem_stream_t stream\);', text)


def test_jacobi_case_separates_in_the_reference():
  """The case of the GPU Jacobi test, chosen here: dense PCG of the reference
  needs at least twice the iterations without the preconditioner (375
  against 78 at rtol = 1e-8), so 'strictly fewer' on the GPU is a safe claim."""
  rp, Pj, mu_e, force = ER.jacobi_case()
  x = np.asarray(rp.node_coords, np.float64)
  mu = lambda xq: np.broadcast_to(mu_e[:, None], xq.shape[:2])
  dense = ER.Dense(rp, Pj, lambda xq: 2.0 * mu(xq), mu)
  fixed = np.zeros(x.shape, bool)
  fixed[np.abs(x[:, 0]) < 1e-9] = True
  K, b, _ = dense.system(np.tile(force, (len(x), 1)), fixed, 0.0 * x)
  plain = ER.pcg(K, b, 1e-8, jacobi=False)[1]
  jac = ER.pcg(K, b, 1e-8, jacobi=True)[1]
  print(f'reference PCG: {plain} iterations, {jac} with Jacobi')
  assert plain >= 2 * jac and jac > 0
