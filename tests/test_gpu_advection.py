"""The advective term b . grad u of the Helmholtz solves on the GPU: the fused
operator (collocated and two-grid, every velocity form, every geometry kind)
against the NumPy reference (`tests/advection_reference.py`), its consistency
across apply_local / diagonal, BiCGStab against its NumPy restatement
(`tests/bicgstab_reference.py`), discrete solves against dense solves,
manufactured solutions, a periodic box and the refusals.

Per-order coverage of the forward kernels (every P = 2..12 in 2D and 3D, both
precisions, every geometry path and coefficient form, `apply_local`, the
diagonal) is in `tests/test_gpu_advection_sweep.py`; the BiCGStab kernels and
scalar phases are called directly in `tests/test_gpu_bicgstab_kernels.py`."""
import warnings

import numpy as np
import pytest
import torch

from swirl_fem_amd.common.premesh_commons import box_mesh, unit_cube_mesh
from swirl_fem_amd.core import operators
from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType, Quadrature1D
from swirl_fem_amd.core.mesh_refiner import refine_premesh
from swirl_fem_amd.examples.helmholtz import BCType, solve_helmholtz
from tests import advection_reference as AR
from tests import bicgstab_reference as BS
from tests import bvp_reference as BR
from tests import coefficient_reference as R
from tests import geometry_cases as G
from tests import robin_reference as RR
from tests.fp32util import F32Rng, f32r, tolerance

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GLL, GL = NodeType.GAUSS_LOBATTO_LEGENDRE, NodeType.GAUSS_LEGENDRE
D, N, RB = BCType.DIRICHLET, BCType.NEUMANN, BCType.ROBIN


def _dev(a, dtype=torch.float64):
  return torch.as_tensor(np.asarray(a), dtype=dtype, device=DEV)


def _np(t):
  return t.detach().double().cpu().numpy()


def _arg(v, dtype=torch.float64):
  return _dev(v, dtype) if isinstance(v, np.ndarray) else v


def _rel(a, b):
  return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _coef_forms(fes_ref, E, axis, rng):
  """[(name, operator argument, reference values (E, Q))]: the coefficient
  forms of `test_gpu_coefficients._forms`."""
  xq = R.quad_points(fes_ref)
  elem = 0.5 + rng.random(E)
  point = 1.0 + xq[..., axis] ** 2 + 0.5 * np.sin(3.0 * xq[..., axis])
  fn = lambda x: 1.0 + x[:, axis] ** 2 + 0.5 * torch.sin(3.0 * x[:, axis])
  Q = xq.shape[1]
  return [('scalar', 2.5, np.full((E, Q), 2.5)),
          ('elem', elem, np.repeat(elem[:, None], Q, 1)),
          ('point', point, point),
          ('callable', fn, point)]


def _field_np(x):
  d = x.shape[-1]
  comps = [1.0 + x[..., 0] * x[..., d - 1], np.sin(2.0 * x[..., 0]) - 0.5]
  if d == 3:
    comps.append(0.5 - x[..., 1] ** 2 + x[..., 2])
  return np.stack(comps, axis=-1)


def _field_torch(x):
  d = x.shape[-1]
  comps = [1.0 + x[:, 0] * x[:, d - 1], torch.sin(2.0 * x[:, 0]) - 0.5]
  if d == 3:
    comps.append(0.5 - x[:, 1] ** 2 + x[:, 2])
  return torch.stack(comps, dim=-1)


def _velocity_forms(fes_ref, E, rng):
  """[(name, operator argument, reference values (E, Q, d))] for every form
  of `velocity`."""
  xq = R.quad_points(fes_ref)                                   # (E, Q, d)
  Q, d = xq.shape[1:]
  const = np.array([0.7, -1.1, 0.4][:d])
  elem = rng.standard_normal((E, d))
  point = _field_np(xq)
  return [('constant', const, np.broadcast_to(const, (E, Q, d))),
          ('elem', elem, np.repeat(elem[:, None, :], Q, 1)),
          ('point', point, point),
          ('callable', _field_torch, point)]


def _space(mesh, P, quad):
  q = (Quadrature1D.create(P, GLL) if quad is None
       else Quadrature1D.create(quad, GL))
  return FiniteElementSpace.create(mesh, q)


def _ref_space(rp, P, quad):
  return AR.space(rp.node_coords, rp.elements, P,
                  (P, 'gll') if quad is None else (quad, 'gl'))


# ------------------------------------------------ 1. operator vs reference
OPERATOR_CASES = [
    # (builder, ndim, P points, quad points or None = collocated)
    ('three_kinds', 2, 2, None), ('three_kinds', 2, 4, None),
    ('three_kinds', 2, 7, None), ('three_kinds', 2, 12, None),
    ('three_kinds', 3, 2, None), ('three_kinds', 3, 4, None),
    ('three_kinds', 3, 7, None), ('affine_curved', 2, 7, None),
    ('multilinear', 3, 4, None),
    ('three_kinds', 2, 4, 5), ('three_kinds', 3, 3, 4),
    ('multilinear', 2, 11, 12), ('affine', 3, 5, 6),
]


@pytest.mark.parametrize('name,ndim,P,quad', OPERATOR_CASES)
def test_operator_matches_reference(name, ndim, P, quad):
  """Every velocity form, paired with the coefficient forms as
  `test_gpu_coefficients` pairs them (and once without coefficients), with
  and without a Dirichlet mask, both lambda pairs; fp64, 1e-11."""
  n = 3 if name == 'three_kinds' else 2
  case = getattr(G, name)(n, ndim, P)
  mesh, bm, rp = case.finalize(DEV, torch.float64)
  fes = _space(mesh, P, quad)
  ref = _ref_space(rp, P, quad)
  E = mesh.num_elements
  rng = np.random.default_rng(P + 10 * ndim)
  u = rng.standard_normal(mesh.num_nodes)
  forms_b = _velocity_forms(ref, E, rng)
  forms_k = _coef_forms(ref, E, 0, rng)
  forms_c = _coef_forms(ref, E, ndim - 1, rng)
  forms_c = forms_c[1:] + forms_c[:1]
  combos = list(zip(forms_b, forms_k, forms_c))
  none = ('none', None, None)
  combos.append((forms_b[2], none, none))
  for (bn, b, bq), (kn, k, kq), (cn, c, cq) in combos:
    for mask in (bm, None):
      keep = None if mask is None else 1.0 - _np(mask)
      op = fes.helmholtz_operator(mask, diffusivity=_arg(k), reaction=_arg(c),
                                  velocity=_arg(b))
      if quad is None:
        assert isinstance(op, operators.HelmholtzOperator)
        assert op.facet_parts is None and op.layer_plan() is None
      else:
        assert isinstance(op, operators.TwoGridHelmholtzOperator)
      for l0, l1 in ((0.0, 1.0), (0.7, 1.3)):
        got = _np(op.apply(_dev(u), l0, l1))
        want = AR.apply(ref, u, l0, l1, kq, cq, bq, keep)
        err = _rel(got, want)
        assert err <= 1e-11, (name, bn, kn, cn, mask is None, l0, err)


@pytest.mark.parametrize('j', [0, 1, 2])
def test_one_component_one_axis(j):
  """A velocity with the single non-zero component j that varies along
  another axis only: a transposed point or component order fails."""
  case = G.three_kinds(3, 3, 4)
  mesh, bm, rp = case.finalize(DEV, torch.float64)
  fes = _space(mesh, 4, None)
  ref = _ref_space(rp, 4, None)
  xq = R.quad_points(ref)
  bq = np.zeros(xq.shape)
  bq[..., j] = 1.0 + 4.0 * xq[..., (j + 1) % 3] ** 2
  u = np.random.default_rng(j).standard_normal(mesh.num_nodes)
  op = fes.helmholtz_operator(None, velocity=_dev(bq))
  got = _np(op.apply(_dev(u), 0.5, 1.0))
  assert _rel(got, AR.apply(ref, u, 0.5, 1.0, b_q=bq)) <= 1e-11
  # the term alone (both lambdas 0): nothing else hides a wrong order
  got = _np(op.apply(_dev(u), 0.0, 0.0))
  assert _rel(got, AR.apply(ref, u, 0.0, 0.0, b_q=bq)) <= 1e-11


@pytest.mark.parametrize('ndim,P', [(2, 4), (3, 4), (2, 12), (3, 7)])
def test_fp32_within_policy(ndim, P):
  case = G.three_kinds(3, ndim, P)
  mesh, bm, rp = case.finalize(DEV, torch.float32)
  fes = _space(mesh, P, None)
  ref = _ref_space(rp, P, None)
  rng = F32Rng(P)
  E = mesh.num_elements
  _, k, kq = _coef_forms(ref, E, 0, rng)[2]
  _, c, cq = _coef_forms(ref, E, ndim - 1, rng)[1]
  kq, cq = f32r(kq), f32r(cq)
  bq = f32r(_velocity_forms(ref, E, rng)[2][2])
  f32 = torch.float32
  op = fes.helmholtz_operator(None, diffusivity=_dev(kq, f32),
                              reaction=_dev(cq[:, 0], f32),
                              velocity=_dev(bq, f32))
  u = rng.standard_normal(mesh.num_nodes)
  got = _np(op.apply(_dev(u, f32), 0.7, 1.3))
  err = _rel(got, AR.apply(ref, u, 0.7, 1.3, kq, cq, bq))
  print(f'fp32 ndim={ndim} P={P}: rel err {err:.3e}')
  assert err <= tolerance(torch.float32, P)


# ------------------------------------------------------- 4. consistency
@pytest.mark.parametrize('ndim,P,quad', [(3, 4, None), (2, 7, None),
                                         (3, 3, 4)])
def test_local_assembly_diagonal_consistent(ndim, P, quad):
  case = G.three_kinds(3, ndim, P)
  mesh, bm, rp = case.finalize(DEV, torch.float64)
  fes = _space(mesh, P, quad)
  ref = _ref_space(rp, P, quad)
  rng = np.random.default_rng(3)
  E = mesh.num_elements
  _, k, kq = _coef_forms(ref, E, 1, rng)[2]
  _, c, cq = _coef_forms(ref, E, 0, rng)[1]
  _, b, bq = _velocity_forms(ref, E, rng)[2]
  keep = 1.0 - _np(bm)
  op = fes.helmholtz_operator(bm, diffusivity=_dev(k), reaction=_dev(c),
                              velocity=_dev(b))
  u = rng.standard_normal(mesh.num_nodes)
  full = _np(op.apply(_dev(u), 0.7, 1.3))
  loc = op.apply_local(mesh.gather(_dev(u)), 0.7, 1.3)
  assert _rel(_np(loc), AR.local_apply(ref, ref.gather(u), 0.7, 1.3, kq, cq,
                                       bq)) <= 1e-11
  assert _rel(_np(mesh.scatter(loc)) * keep, full) <= 1e-13
  dg = _np(op.diagonal(0.7, 1.3))
  assert _rel(dg, AR.diagonal(ref, 0.7, 1.3, kq, cq, bq, keep)) <= 1e-11
  # linear_operator is a plain callable: BiCGStab needs no p . Ap
  lin = op.linear_operator(0.7, 1.3)
  assert not hasattr(lin, 'apply_with_dot')
  assert _rel(_np(lin(_dev(u))), full) <= 1e-13
  if quad is None:
    assert 'helmholtz_adv_kernel<double, %d, %d, true' % (P, ndim) in \
        op.kernel_name(0.7, 1.3)
    col = fes.helmholtz_operator(bm, assembly='colored', diffusivity=_dev(k),
                                 reaction=_dev(c), velocity=_dev(b))
    assert _rel(_np(col.apply(_dev(u), 0.7, 1.3)), full) <= 1e-13
    # split carries the term (no coefficients: those refuse to split)
    plain = fes.helmholtz_operator(bm, velocity=_dev(b))
    sel = torch.arange(E, device=DEV) % 2 == 0
    a, bb = plain.split(sel)
    whole = _np(plain.apply(_dev(u), 0.7, 1.3))
    # the halves write one output, the second without clearing it (a half
    # stores nothing at the nodes only the other half's elements own)
    out = a.apply(_dev(u), 0.7, 1.3)
    bb.apply(_dev(u), 0.7, 1.3, out=out, zero=False)
    assert _rel(_np(out), whole) <= 1e-13
    assert _rel(_np(a.diagonal(0.7, 1.3)) + _np(bb.diagonal(0.7, 1.3)),
                _np(plain.diagonal(0.7, 1.3))) <= 1e-13
  # a velocity of zeros is the operator without the argument
  zero = torch.zeros((E, fes.num_quadrature_points_per_element, ndim),
                     dtype=torch.float64, device=DEV)
  with_zero = fes.helmholtz_operator(bm, diffusivity=_dev(k),
                                     reaction=_dev(c), velocity=zero)
  without = fes.helmholtz_operator(bm, diffusivity=_dev(k), reaction=_dev(c))
  assert _rel(_np(with_zero.apply(_dev(u), 0.7, 1.3)),
              _np(without.apply(_dev(u), 0.7, 1.3))) <= 1e-14


def test_to_quadrature():
  """Nodal values at the quadrature points: a nodal velocity as `velocity`."""
  case = G.three_kinds(3, 2, 4)
  mesh, bm, rp = case.finalize(DEV, torch.float64)
  for quad in (None, 5):
    fes = _space(mesh, 4, quad)
    ref = _ref_space(rp, 4, quad)
    rng = np.random.default_rng(0)
    v = rng.standard_normal((mesh.num_nodes, 2))
    want = np.einsum('qi,eic->eqc', ref.M, v[np.asarray(rp.elements)])
    got = fes.to_quadrature(_dev(v))
    assert tuple(got.shape) == want.shape
    assert _rel(_np(got), want) <= 1e-13
    assert _rel(_np(fes.to_quadrature(_dev(v[:, 0]))), want[..., 0]) <= 1e-13
    u = rng.standard_normal(mesh.num_nodes)
    op = fes.helmholtz_operator(bm, velocity=got)
    assert _rel(_np(op.apply(_dev(u), 0.3, 1.0)),
                AR.apply(ref, u, 0.3, 1.0, b_q=want, keep=1.0 - _np(bm))) \
        <= 1e-11


# ------------------------------------------------------- 5. solver alone
class _Diag:
  """A preconditioner the solver folds into its kernels."""

  def __init__(self, dinv):
    self.dinv = dinv

  def jacobi_diagonal(self):
    return self.dinv

  def __call__(self, r):
    return self.dinv * r


def _dense_system(n=200, seed=7):
  rng = np.random.default_rng(seed)
  A = 0.5 * rng.standard_normal((n, n)) / np.sqrt(n)
  A += np.diag(1.0 + rng.random(n))
  return A, rng.standard_normal(n)


@pytest.mark.parametrize('precond', [None, 'fused', 'callable'])
def test_bicgstab_iterates_match_numpy(precond):
  from swirl_fem_amd.linalg.bicgstab import BiCGStabRunner, bicgstab
  A, b = _dense_system()
  assert np.abs(A - A.T).max() > 1e-2
  Ad = _dev(A)
  op = lambda v: Ad @ v
  dinv = 1.0 / np.diag(A)
  M = {None: None, 'fused': _Diag(_dev(dinv)),
       'callable': (lambda r, d=_dev(dinv): d * r)}[precond]
  Mh = None if precond is None else (lambda v: dinv * v)
  _, iterates, _ = BS.bicgstab(lambda v: A @ v, b, tol=1e-30, maxiter=10,
                               M=Mh)
  assert len(iterates) == 10
  run = BiCGStabRunner(op, _dev(b), tol=1e-30, M=M)
  assert (run.dinv is not None) == (precond == 'fused')
  for want in iterates:
    run.step()
    assert _rel(_np(run.x), want) <= 1e-10
  assert run.info()['num_iterations'] == 10
  x, info = bicgstab(op, _dev(b), tol=1e-13, M=M)
  assert info['status'] == 'converged'
  want = np.linalg.solve(A, b)
  # cond(A) < 10 by construction (eigenvalues in a disc of radius ~ 0.5
  # around [1, 2]): residual 1e-13 -> error well under 1e-10
  assert _rel(_np(x), want) <= 1e-10
  assert float(info['residual']) <= 1e-26 * float(b @ b)
  # the count is that of the NumPy loop (device stop test, host polling)
  _, its, _ = BS.bicgstab(lambda v: A @ v, b, tol=1e-13, M=Mh)
  assert abs(info['num_iterations'] - len(its)) <= 1
  # a start away from zero, a maxiter stop
  x0 = np.random.default_rng(1).standard_normal(len(b))
  x, info = bicgstab(op, _dev(b), _dev(x0), tol=1e-13, M=M)
  assert info['status'] == 'converged' and _rel(_np(x), want) <= 1e-10
  x, info = bicgstab(op, _dev(b), tol=1e-13, M=M, maxiter=3, check_every=2)
  assert info['status'] == 'maxiter' and info['num_iterations'] == 3


def test_bicgstab_edge_cases():
  from swirl_fem_amd.linalg.bicgstab import bicgstab
  A, b = _dense_system(50, 3)
  Ad = _dev(A)
  x, info = bicgstab(lambda v: Ad @ v, torch.zeros(50, dtype=torch.float64,
                                                   device=DEV))
  assert info['status'] == 'converged' and info['num_iterations'] == 0
  assert not bool(x.any())
  # SPD operator
  S = A @ A.T + np.eye(50)
  Sd = _dev(S)
  x, info = bicgstab(lambda v: Sd @ v, _dev(b), tol=1e-12)
  assert info['status'] == 'converged'
  assert _rel(_np(x), np.linalg.solve(S, b)) <= 1e-9
  # the identity converges in the first half-step, counted as one iteration
  x, info = bicgstab(lambda v: v.clone(), _dev(b), tol=1e-12)
  assert info['status'] == 'converged' and info['num_iterations'] == 1
  assert _rel(_np(x), b) <= 1e-14
  # fp32 vectors
  x, info = bicgstab(lambda v: Ad.float() @ v, _dev(b, torch.float32),
                     tol=1e-5)
  assert info['status'] == 'converged' and x.dtype == torch.float32
  assert _rel(_np(x), np.linalg.solve(A, b)) <= 1e-4
  # a skew-symmetric operator: r0 . v = 0, named, warned about, no NaN
  K = _dev(np.array([[0.0, 1.0], [-1.0, 0.0]]))
  with warnings.catch_warnings(record=True) as seen:
    warnings.simplefilter('always')
    x, info = bicgstab(lambda v: K @ v, _dev(np.array([1.0, 2.0])))
  assert info['status'] == 'breakdown_alpha'
  assert any(issubclass(w.category, RuntimeWarning) for w in seen)
  assert bool(torch.isfinite(x).all())
  _, _, status = BS.bicgstab(lambda v: _np(K) @ v, np.array([1.0, 2.0]))
  assert status == 'breakdown_alpha'


# --------------------------------------- 6. discrete solve vs dense solve
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


def _three_kinds_with_sides(n, ndim, P):
  """`geometry_cases.three_kinds` with one physical group per side (its
  deformations leave the box boundary in place)."""
  pm = unit_cube_mesh(n, ndim=ndim)
  pm = pm.replace(physical_groups=BR.boundary_groups(pm, _sides(ndim)),
                  node_coords=G._move_centre_vertex(pm.node_coords, n))
  rp = refine_premesh(pm, Nodes1D.create(P, GLL))
  return G._bend_first_layer(rp, n)


def _box(ndim, n, P, periodic=()):
  pm = unit_cube_mesh(n, ndim=ndim, periodic_dims=periodic)
  pm = pm.replace(physical_groups=BR.boundary_groups(pm,
                                                     _sides(ndim, periodic)))
  return refine_premesh(pm, Nodes1D.create(P, GLL))


def solve_quadrature(ndim, P):
  """Gauss points per direction of `solve_helmholtz` for P nodes."""
  return (P - 1) + (ndim + 1) // 2


def dense_solve(rp, facets, P, l0, l1, kf, cf, bf, f, dvals, robin=(),
                neumann=(), want_cond=True):
  """`numpy.linalg.solve` on the assembled reference matrices with the lift
  of `solve_helmholtz`.  kf, cf, bf: NumPy callables on (..., d) points or
  None; `dvals` (N,) with NaN off the Dirichlet nodes; robin [(group, alpha,
  g)], neumann [(group, g)] with NumPy callables / scalars on the facet
  points.  Returns (u, condition number of the reduced matrix or None)."""
  x = np.asarray(rp.node_coords, np.float64)
  ndim = x.shape[1]
  q = solve_quadrature(ndim, P)
  ref = AR.space(x, rp.elements, P, (q, 'gl'))
  xq = AR.quad_points(ref)
  val = lambda fn: None if fn is None else fn(xq)
  K = AR.assemble(ref, AR.element_matrices(ref, l0, l1, val(kf), val(cf),
                                           val(bf)))
  Bm = AR.assemble(ref, AR.element_matrices(ref, 1.0, 0.0))
  grid, quad = Nodes1D.create(P, GLL), Quadrature1D.create(q, GL)
  b = Bm @ f

  def points(fr, g):
    pq, wj = BR.facet_quadrature(x, fr, grid, quad)
    return (np.asarray(g(pq.reshape(-1, ndim))).reshape(wj.shape)
            if callable(g) else np.full(wj.shape, float(g)))
  for group, alpha, g in robin:
    fr = facets[group]
    K = K + l1 * RR.robin_matrix(x, fr, grid, quad, alpha)
    b = b + l1 * BR.covector(x, fr, grid, quad, points(fr, g))
  for group, g in neumann:
    fr = facets[group]
    b = b + l1 * BR.covector(x, fr, grid, quad, points(fr, g))
  isd = ~np.isnan(dvals)
  u = np.where(isd, dvals, 0.0)
  free = ~isd
  Kff = K[np.ix_(free, free)]
  u[free] = np.linalg.solve(Kff, b[free] - K[np.ix_(free, isd)] @ u[isd])
  return u, (np.linalg.cond(Kff) if want_cond else None)


DENSE_K = lambda x: 1.0 + 0.5 * x[..., 0] ** 2
DENSE_C = lambda x: 40.0 + 10.0 * x[..., -1]


def _dense_b(x):
  d = x.shape[-1]
  comps = [1.0 + x[..., 1], 0.5 - x[..., 0]]
  if d == 3:
    comps.append(0.3 + 0.0 * x[..., 0])
  return np.stack(comps, axis=-1)


def _t(fn):
  """A NumPy callable on points as a torch callable."""
  return lambda x: _dev(fn(_np(x)))


@pytest.mark.parametrize('ndim,P', [(2, 5), (3, 3)])
def test_solve_matches_dense_solve(ndim, P):
  """`solve_helmholtz(velocity=, diffusivity=, reaction=, rtol=1e-12)` on the
  three-kinds mesh with Dirichlet (x0, with values), Neumann (y1) and Robin
  (x1) groups against the dense reference solve.  The agreement bound is
  100 cond 1e-12 with cond the condition number of the reference matrix,
  computed in the test; with lambda0 = 1, c = 40 + 10 x_last, k = 1 + x^2 / 2
  it is 2D, P = 5: cond = 60.2 (bound 6.0e-9); 3D, P = 3: cond = 41.6 (bound
  4.2e-9), both under the 1e-7 the bound may reach."""
  rp = _three_kinds_with_sides(3, ndim, P)
  mesh = rp.finalize(device=DEV)
  x = np.asarray(rp.node_coords)
  facets = {g: f.cpu().numpy().astype(np.int64)
            for g, f in mesh.boundary_facets.items()}
  rng = np.random.default_rng(ndim)
  f = rng.standard_normal(mesh.num_nodes)
  dmask = mesh.physical_masks['x0'].cpu().numpy()
  dvals = np.where(dmask, 1.0 + x[:, 1] ** 2, np.nan)
  alpha, gr = 2.0, (lambda y: 1.0 + y[:, 1])
  gn = lambda y: np.cos(2.0 * y[:, 0])
  want, cond = dense_solve(rp, facets, P, 1.0, 1.3, DENSE_K, DENSE_C,
                           _dense_b, f, dvals, [('x1', alpha, gr)],
                           [('y1', gn)])
  bound = 100.0 * cond * 1e-12
  print(f'ndim={ndim} P={P}: cond {cond:.3e}, bound {bound:.2e}')
  assert bound <= 1e-7
  bcs = {'x0': (D, _dev(np.nan_to_num(dvals))),
         'x1': (RB, (alpha, _t(gr))), 'y1': (N, _t(gn))}
  kw = dict(lambda0=1.0, lambda1=1.3, rtol=1e-12, return_info=True,
            diffusivity=_t(DENSE_K), reaction=_t(DENSE_C))
  for pc in (None, 'jacobi'):
    got, info = solve_helmholtz(mesh, _dev(f), bcs, preconditioner=pc,
                                velocity=_t(_dense_b), **kw)
    err = _rel(_np(got), want)
    print(f'  {pc}: {info["num_iterations"]} iterations, rel err {err:.2e}')
    assert info['status'] == 'converged'
    assert err <= bound
  # the advection-free problem: Jacobi needs no more iterations than none
  its = {}
  for pc in (None, 'jacobi'):
    _, info = solve_helmholtz(mesh, _dev(f), bcs, preconditioner=pc, **kw)
    its[pc] = int(info['num_iterations'])
  assert its['jacobi'] <= its[None], its


# ------------------------------------------- 7. manufactured solutions
def _manufactured(ndim):
  """u = sin(pi x) cos(pi y) [cos(pi z)], b = (1, 2[, -1]), k = 1 + x^2 / 2,
  lambda0 = 1: (exact, forcing, k, b) as NumPy callables."""
  pi = np.pi
  b = np.array([1.0, 2.0, -1.0][:ndim])
  k = lambda x: 1.0 + 0.5 * x[..., 0] ** 2

  def parts(x):
    s, c = np.sin(pi * x[..., 0]), np.cos(pi * x[..., 0])
    rest = np.prod(np.cos(pi * x[..., 1:]), axis=-1)
    u = s * rest
    grad = [pi * c * rest]
    for a in range(1, ndim):
      grad.append(-pi * s * np.sin(pi * x[..., a]) *
                  np.prod(np.cos(pi * np.delete(x[..., 1:], a - 1, axis=-1)),
                          axis=-1))
    return u, grad
  exact = lambda x: parts(x)[0]

  def forcing(x):
    u, grad = parts(x)
    # -div(k grad u) = -k lap u - k_x u_x, lap u = -ndim pi^2 u, k_x = x
    diff = k(x) * ndim * pi ** 2 * u - x[..., 0] * grad[0]
    return u + sum(b[a] * grad[a] for a in range(ndim)) + diff
  return exact, forcing, k, (lambda x: np.broadcast_to(b, x.shape).copy())


@pytest.mark.parametrize('ndim', [2, 3])
def test_manufactured_converges(ndim):
  """The error to the exact solution falls strictly from order 4 to 6 to 8 on
  2^d elements (P = 5, 7, 9 nodes per direction, as `_box(ndim, 2, P)` of
  `test_gpu_coefficients.test_manufactured_converges` counts), and at order 8
  it is within 10x the error of the reference dense solve of the same
  discrete problem."""
  exact, forcing, k, b = _manufactured(ndim)
  errs = []
  for order in (4, 6, 8):
    P = order + 1
    rp = _box(ndim, 2, P)
    mesh = rp.finalize(device=DEV)
    x = np.asarray(rp.node_coords)
    bcs = {g: (D, _dev(exact(x))) for g in mesh.physical_masks
           if g in ('x0', 'x1', 'y0')}
    got = solve_helmholtz(mesh, _dev(forcing(x)), bcs, lambda0=1.0,
                          rtol=1e-13, diffusivity=_t(k), velocity=_t(b),
                          preconditioner='jacobi')
    errs.append(np.abs(_np(got) - exact(x)).max())
  print(f'ndim={ndim}: errors {errs}')
  assert errs[1] < errs[0] and errs[2] < errs[1], errs
  dmask = np.zeros(len(x), bool)
  for g in bcs:
    dmask |= mesh.physical_masks[g].cpu().numpy()
  want, _ = dense_solve(rp, {}, P, 1.0, 1.0, k, None, b, forcing(x),
                        np.where(dmask, exact(x), np.nan), want_cond=False)
  ref_err = np.abs(want - exact(x)).max()
  print(f'  dense solve error {ref_err:.3e}')
  assert errs[2] <= 10.0 * ref_err


def test_boundary_layer():
  """-eps u'' + u' = 0, u(0) = 0, u(1) = 1 on a 4 x 1 strip, eps = 0.1,
  P = 10: u = (e^(x/eps) - 1) / (e^(1/eps) - 1), a layer of width eps at
  x = 1 that the 0.25-wide last element resolves.  Within 10x the dense
  solve's error to the exact u."""
  eps, P = 0.1, 10
  pm = box_mesh((4, 1), (0.0, 0.0), (1.0, 1.0))
  pm = pm.replace(physical_groups=BR.boundary_groups(pm, _sides(2)))
  rp = refine_premesh(pm, Nodes1D.create(P, GLL))
  mesh = rp.finalize(device=DEV)
  x = np.asarray(rp.node_coords)
  exact = np.expm1(x[:, 0] / eps) / np.expm1(1.0 / eps)
  b = lambda y: np.stack([np.ones(y.shape[:-1]), np.zeros(y.shape[:-1])], -1)
  f = np.zeros(len(x))
  got, info = solve_helmholtz(mesh, _dev(f), {'x0': (D, 0.0), 'x1': (D, 1.0)},
                              lambda0=0.0, lambda1=eps, rtol=1e-13,
                              velocity=_t(b), return_info=True)
  assert info['status'] == 'converged'
  dmask = (mesh.physical_masks['x0'] | mesh.physical_masks['x1']).cpu().numpy()
  want, _ = dense_solve(rp, {}, P, 0.0, eps, None, None, b, f,
                        np.where(dmask, exact, np.nan), want_cond=False)
  err, ref_err = np.abs(_np(got) - exact).max(), np.abs(want - exact).max()
  print(f'boundary layer: error {err:.3e}, dense solve {ref_err:.3e}')
  assert err <= 10.0 * ref_err


# ---------------------------------------------------------- 8. periodic
def test_periodic_box():
  """u = sin(2 pi x) cos(2 pi y) on a box periodic in x (du/dn = 0 on y = 0,
  1, the natural condition), constant b, lambda0 = 1.  On 3 x 3 elements of
  order 8 the interpolation error of a mode of wavenumber 2 pi is about
  (pi / 3)^9 / 9! = 4e-6; the bound leaves the Galerkin constant a factor
  25."""
  P = 9
  rp = _box(2, 3, P, periodic=(0,))
  mesh = rp.finalize(device=DEV)
  x = np.asarray(rp.node_coords)
  two_pi = 2.0 * np.pi
  s, c = np.sin(two_pi * x[:, 0]), np.cos(two_pi * x[:, 0])
  cy, sy = np.cos(two_pi * x[:, 1]), np.sin(two_pi * x[:, 1])
  b = np.array([1.0, 0.5])
  u = s * cy
  f = u + b[0] * two_pi * c * cy - b[1] * two_pi * s * sy + 2 * two_pi ** 2 * u
  got, info = solve_helmholtz(mesh, _dev(f), {}, lambda0=1.0, rtol=1e-12,
                              velocity=_dev(b), return_info=True)
  assert info['status'] == 'converged'
  got = _np(got)
  assert np.abs(got - u).max() <= 1e-4
  ni = mesh.node_indices.cpu().numpy().astype(np.int64)
  assert (ni != np.arange(len(ni))).any()
  assert np.array_equal(got, got[ni])
  with pytest.raises(NotImplementedError):
    solve_helmholtz(mesh, _dev(f), {}, lambda0=1.0, velocity=_dev(b),
                    preconditioner='jacobi')


# ---------------------------------------------------------- 9. refusals
def test_refusals():
  case = G.affine(2, 3, 4)
  mesh, bm, rp = case.finalize(DEV, torch.float64)
  fes = _space(mesh, 4, None)
  b = torch.ones(3, dtype=torch.float64, device=DEV)
  E, n = mesh.num_elements, mesh.num_nodes_per_element
  op = fes.helmholtz_operator(None, velocity=b)
  f = torch.zeros(mesh.num_nodes, dtype=torch.float64, device=DEV)
  # a vector field
  with pytest.raises(NotImplementedError):
    op.apply(torch.zeros((mesh.num_nodes, 3), dtype=torch.float64,
                         device=DEV))
  with pytest.raises(NotImplementedError):
    op.apply_local(torch.zeros((E, n, 3), dtype=torch.float64, device=DEV))
  # p-multigrid with a velocity
  with pytest.raises(NotImplementedError):
    solve_helmholtz(mesh, f, {'boundary': (D, 0.0)}, velocity=b,
                    preconditioner='pmg')
  # assemblies that do not run on index rows
  for assembly in ('cluster', 'layered', 'facet'):
    with pytest.raises(NotImplementedError):
      fes.helmholtz_operator(None, assembly=assembly, velocity=b)
  # a velocity of the wrong shape / kind
  for bad in (torch.ones(2, dtype=torch.float64, device=DEV),
              torch.ones((E, n), dtype=torch.float64, device=DEV),
              torch.ones((E + 1, 3), dtype=torch.float64, device=DEV),
              torch.ones((E, n, 2), dtype=torch.float64, device=DEV),
              lambda x: x[:, 0],
              torch.full((3,), float('nan'), dtype=torch.float64,
                         device=DEV)):
    with pytest.raises(ValueError):
      fes.helmholtz_operator(None, velocity=bad)
  # an ensemble and a partitioned mesh
  with pytest.raises(NotImplementedError):
    solve_helmholtz(mesh.replicate(2), torch.zeros(
        2 * mesh.num_nodes, dtype=torch.float64, device=DEV),
                    {'boundary': (D, 0.0)}, velocity=b)
  with pytest.raises(NotImplementedError):
    FiniteElementSpace.create(mesh.replicate(2), fes.quadrature) \
        .helmholtz_operator(None, velocity=b)
  pm = unit_cube_mesh(2, ndim=3, partitions=np.arange(2).reshape(2, 1, 1))
  part = refine_premesh(pm, Nodes1D.create(4, GLL)).finalize(
      'x', rank=0, device=DEV)
  with pytest.raises(NotImplementedError):
    solve_helmholtz(part, torch.zeros(part.num_nodes, dtype=torch.float64,
                                      device=DEV), {}, lambda0=1.0,
                    velocity=b)
  with pytest.raises(NotImplementedError):
    FiniteElementSpace.create(part, fes.quadrature).helmholtz_operator(
        None, velocity=b)
  # the C entry point: out-of-scope combinations are SFEM_EUNSUPPORTED
  from swirl_fem_amd import _lib, _ops
  u = torch.zeros(mesh.num_nodes, dtype=torch.float64, device=DEV)
  parts = [dict(p, kappa=torch.ones(E, dtype=torch.float64, device=DEV),
                coef_mode=_lib.COEF_ELEM) for p in op.parts]
  with pytest.raises(_lib.SfemError, match='status -3'):
    _ops.helmholtz_apply(u, torch.empty_like(u), op.enc, parts, op.host, 3, 4,
                         0.0, 1.0, op.zero_range)
