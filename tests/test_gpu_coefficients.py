"""Variable diffusivity and reaction coefficients on the GPU: the fused
operator (collocated and two-grid, every coefficient form, every geometry
kind) against the NumPy reference (`tests/coefficient_reference.py`), its
consistency across apply_local / assembly modes / diagonal, an exactly
solvable two-material problem, a manufactured solution and the
preconditioners."""
import numpy as np
import pytest
import torch

from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
from swirl_fem_amd.core import operators
from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType, Quadrature1D
from swirl_fem_amd.core.mesh_refiner import refine_premesh
from swirl_fem_amd.examples.helmholtz import BCType, solve_helmholtz
from tests import bvp_reference as BR
from tests import coefficient_reference as R
from tests import geometry_cases as G
from tests.fp32util import tolerance

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GLL, GL = NodeType.GAUSS_LOBATTO_LEGENDRE, NodeType.GAUSS_LEGENDRE
D, N, RB = BCType.DIRICHLET, BCType.NEUMANN, BCType.ROBIN


def _dev(a, dtype=torch.float64):
  return torch.as_tensor(np.asarray(a), dtype=dtype, device=DEV)


def _np(t):
  return t.detach().double().cpu().numpy()


def _forms(fes_ref, E, axis, rng):
  """[(name, operator argument, reference values (E, Q))] for every form; the
  per-point and callable ones vary along `axis` only."""
  xq = R.quad_points(fes_ref)                                   # (E, Q, d)
  elem = 0.5 + rng.random(E)
  point = 1.0 + xq[..., axis] ** 2 + 0.5 * np.sin(3.0 * xq[..., axis])
  fn = lambda x: 1.0 + x[:, axis] ** 2 + 0.5 * torch.sin(3.0 * x[:, axis])
  Q = xq.shape[1]
  return [('scalar', 2.5, np.full((E, Q), 2.5)),
          ('elem', elem, np.repeat(elem[:, None], Q, 1)),
          ('point', point, point),
          ('callable', fn, point)]


def _rel(a, b):
  return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


# ------------------------------------------------ 1. operator vs reference
OPERATOR_CASES = [
    # (builder, ndim, P points, quad points or None = collocated)
    ('three_kinds', 2, 2, None), ('three_kinds', 2, 4, None),
    ('three_kinds', 2, 7, None), ('three_kinds', 2, 12, None),
    ('three_kinds', 3, 2, None), ('three_kinds', 3, 4, None),
    ('three_kinds', 3, 7, None), ('affine', 3, 4, None),
    ('multilinear', 3, 4, None), ('affine_curved', 2, 7, None),
    ('three_kinds', 2, 4, 5), ('three_kinds', 3, 3, 4),
    ('multilinear', 2, 11, 12), ('affine', 3, 5, 6),
]


@pytest.mark.parametrize('name,ndim,P,quad', OPERATOR_CASES)
def test_operator_matches_reference(name, ndim, P, quad):
  n = 3 if name == 'three_kinds' else 2
  case = getattr(G, name)(n, ndim, P)
  mesh, bm, rp = case.finalize(DEV, torch.float64)
  q = (Quadrature1D.create(P, GLL) if quad is None
       else Quadrature1D.create(quad, GL))
  fes = FiniteElementSpace.create(mesh, q)
  ref = R.space(rp.node_coords, rp.elements, P,
                (P, 'gll') if quad is None else (quad, 'gl'))
  E = mesh.num_elements
  rng = np.random.default_rng(P + 10 * ndim)
  keep = 1.0 - _np(bm)
  u = rng.standard_normal(mesh.num_nodes)
  forms_k = _forms(ref, E, 0, rng)
  forms_c = _forms(ref, E, ndim - 1, rng)
  for (kn, k, kq), (cn, c, cq) in zip(forms_k, forms_c[1:] + forms_c[:1]):
    op = fes.helmholtz_operator(bm, diffusivity=_arg(k), reaction=_arg(c))
    if quad is None:
      assert isinstance(op, operators.HelmholtzOperator)
      assert op.facet_parts is None and op.layer_plan() is None
    else:
      assert isinstance(op, operators.TwoGridHelmholtzOperator)
    for l0, l1 in ((0.0, 1.0), (0.7, 1.3)):
      got = _np(op.apply(_dev(u), l0, l1))
      want = R.apply(ref, u, l0, l1, kq, cq, keep)
      err = _rel(got, want)
      assert err <= 1e-11, (name, kn, cn, l0, err)


def _arg(v):
  return _dev(v) if isinstance(v, np.ndarray) else v


@pytest.mark.parametrize('axis', [0, 1, 2])
def test_point_order_per_axis(axis):
  """A per-point coefficient that varies along one axis only, one case per
  axis: a transposed point order fails."""
  case = G.three_kinds(3, 3, 4)
  mesh, bm, rp = case.finalize(DEV, torch.float64)
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(4, GLL))
  ref = R.space(rp.node_coords, rp.elements, 4, (4, 'gll'))
  xq = R.quad_points(ref)
  kq = 1.0 + 4.0 * xq[..., axis] ** 2
  u = np.random.default_rng(axis).standard_normal(mesh.num_nodes)
  op = fes.helmholtz_operator(None, diffusivity=_dev(kq), reaction=_dev(kq))
  got = _np(op.apply(_dev(u), 0.5, 1.0))
  assert _rel(got, R.apply(ref, u, 0.5, 1.0, kq, kq)) <= 1e-11


@pytest.mark.parametrize('ndim,P', [(2, 4), (3, 4), (2, 12), (3, 7)])
def test_fp32_within_policy(ndim, P):
  case = G.three_kinds(3, ndim, P)
  mesh, bm, rp = case.finalize(DEV, torch.float32)
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(P, GLL))
  ref = R.space(rp.node_coords, rp.elements, P, (P, 'gll'))
  rng = np.random.default_rng(P)
  _, k, kq = _forms(ref, mesh.num_elements, 0, rng)[2]
  _, c, cq = _forms(ref, mesh.num_elements, ndim - 1, rng)[1]
  op = fes.helmholtz_operator(None, diffusivity=_dev(k, torch.float32),
                              reaction=_dev(c, torch.float32))
  u = rng.standard_normal(mesh.num_nodes)
  got = _np(op.apply(_dev(u, torch.float32), 0.7, 1.3))
  tol = tolerance(torch.float32, P)
  assert _rel(got, R.apply(ref, u, 0.7, 1.3, kq, cq)) <= tol


# ------------------------------------------------------- 2. consistency
@pytest.mark.parametrize('ndim,P,quad', [(3, 4, None), (2, 7, None),
                                         (3, 3, 4)])
def test_local_assembly_diagonal_consistent(ndim, P, quad):
  case = G.three_kinds(3, ndim, P)
  mesh, bm, rp = case.finalize(DEV, torch.float64)
  q = (Quadrature1D.create(P, GLL) if quad is None
       else Quadrature1D.create(quad, GL))
  fes = FiniteElementSpace.create(mesh, q)
  ref = R.space(rp.node_coords, rp.elements, P,
                (P, 'gll') if quad is None else (quad, 'gl'))
  rng = np.random.default_rng(3)
  _, k, kq = _forms(ref, mesh.num_elements, 1, rng)[2]
  _, c, cq = _forms(ref, mesh.num_elements, 0, rng)[1]
  keep = 1.0 - _np(bm)
  op = fes.helmholtz_operator(bm, diffusivity=_dev(k), reaction=_dev(c))
  ul = rng.standard_normal((mesh.num_elements, mesh.num_nodes_per_element))
  got = _np(op.apply_local(_dev(ul), 0.7, 1.3))
  assert _rel(got, R.local_apply(ref, ul, 0.7, 1.3, kq, cq)) <= 1e-11
  dg = _np(op.diagonal(0.7, 1.3))
  assert _rel(dg, R.diagonal(ref, 0.7, 1.3, kq, cq, keep)) <= 1e-11
  if quad is None:
    u = rng.standard_normal(mesh.num_nodes)
    col = fes.helmholtz_operator(bm, assembly='colored', diffusivity=_dev(k),
                                 reaction=_dev(c))
    a = _np(op.apply(_dev(u), 0.7, 1.3))
    b = _np(col.apply(_dev(u), 0.7, 1.3))
    assert _rel(a, b) <= 1e-13
    assert 'helmholtz_kernel<double, %d, %d, true, true' % (P, ndim) in \
        op.kernel_name(0.7, 1.3)
    with pytest.raises(NotImplementedError):
      fes.helmholtz_operator(bm, assembly='cluster', diffusivity=_dev(k))


@pytest.mark.parametrize('quad', [None, 5])
def test_all_ones_is_constant_operator(quad):
  case = G.three_kinds(3, 3, 4)
  mesh, bm, rp = case.finalize(DEV, torch.float64)
  q = (Quadrature1D.create(4, GLL) if quad is None
       else Quadrature1D.create(quad, GL))
  fes = FiniteElementSpace.create(mesh, q)
  npts = q.num_points ** 3
  E = mesh.num_elements
  u = _dev(np.random.default_rng(1).standard_normal(mesh.num_nodes))
  want = _np(fes.helmholtz_operator(bm).apply(u, 0.7, 1.3))
  for k, c in ((torch.ones(E, dtype=torch.float64, device=DEV), None),
               (torch.ones((E, npts), dtype=torch.float64, device=DEV),
                torch.ones((E, npts), dtype=torch.float64, device=DEV))):
    op = fes.helmholtz_operator(bm, diffusivity=k, reaction=c)
    assert _rel(_np(op.apply(u, 0.7, 1.3)), want) <= 1e-14


def test_refusals():
  case = G.affine(2, 2, 3)
  mesh, bm, rp = case.finalize(DEV, torch.float64)
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(3, GLL))
  op = fes.helmholtz_operator(None, diffusivity=2.0)
  with pytest.raises(NotImplementedError):
    op.apply(torch.zeros((mesh.num_nodes, 2), dtype=torch.float64,
                         device=DEV))
  with pytest.raises(NotImplementedError):
    op.split(torch.zeros(mesh.num_elements, dtype=torch.bool, device=DEV))
  with pytest.raises(ValueError):
    fes.helmholtz_operator(None, diffusivity=-1.0)
  with pytest.raises(ValueError):
    fes.helmholtz_operator(None, reaction=torch.full(
        (mesh.num_elements,), float('nan'), dtype=torch.float64, device=DEV))
  # a new coefficient is never served from the cache
  a = fes.helmholtz_operator(None, diffusivity=2.0)
  b = fes.helmholtz_operator(None, diffusivity=3.0)
  u = torch.ones(mesh.num_nodes, dtype=torch.float64, device=DEV)
  assert torch.allclose(a.apply(u, 1.0, 0.0), b.apply(u, 1.0, 0.0))
  assert _rel(_np(b.diagonal(0.0, 1.0)), 1.5 * _np(a.diagonal(0.0, 1.0))) \
      <= 1e-14


# ---------------------------------------------- 3. two-material problems
def _box(ndim, n, P, deform=False):
  pm = unit_cube_mesh(n, ndim=ndim)
  pm = pm.replace(physical_groups=BR.boundary_groups(pm, _sides(ndim)))
  if deform:
    # moves only y / z of the interior vertices: the interface x = 1/2
    # stays on element faces
    rng = np.random.default_rng(5)
    x = pm.node_coords.copy()
    inner = np.all((x[:, 1:] > 1e-9) & (x[:, 1:] < 1 - 1e-9), axis=1)
    x[inner, 1:] += 0.2 / n * rng.uniform(-1, 1, x[inner, 1:].shape)
    pm = pm.replace(node_coords=x)
  return refine_premesh(pm, Nodes1D.create(P + 1, GLL))


def _sides(ndim):
  names = ['x', 'y', 'z']

  def classify(c):
    for a in range(ndim):
      if abs(c[a]) < 1e-9:
        return names[a] + '0'
      if abs(c[a] - 1) < 1e-9:
        return names[a] + '1'
    return None
  return classify


def _two_material(mesh, k1, k2):
  centre = mesh.element_coords()[..., 0].mean(dim=1)
  k = torch.where(centre < 0.5, torch.full_like(centre, k1),
                  torch.full_like(centre, k2))
  return k


def _exact(x, k1, k2):
  s1, s2 = 2 * k2 / (k1 + k2), 2 * k1 / (k1 + k2)
  return np.where(x < 0.5, s1 * x, s1 * 0.5 + s2 * (x - 0.5))


@pytest.mark.parametrize('ndim,deform', [(2, False), (3, False), (3, True)])
def test_two_material_exact(ndim, deform):
  k1, k2 = 1.0, 100.0
  rp = _box(ndim, 4, 3, deform)
  mesh = rp.finalize(device=DEV)
  k = _two_material(mesh, k1, k2)
  bcs = {'x0': (D, 0.0), 'x1': (D, 1.0)}
  u = solve_helmholtz(mesh, torch.zeros(mesh.num_nodes, dtype=torch.float64,
                                        device=DEV), bcs, rtol=1e-12,
                      diffusivity=k)
  want = _exact(rp.node_coords[:, 0], k1, k2)
  assert np.abs(_np(u) - want).max() <= 1e-8


@pytest.mark.parametrize('preconditioner', ['jacobi', 'pmg'])
def test_preconditioners_at_contrast(preconditioner):
  k1, k2 = 1.0, 1e4
  rp = _box(3, 4, 4, deform=True)
  mesh = rp.finalize(device=DEV)
  k = _two_material(mesh, k1, k2)
  rng = np.random.default_rng(2)
  f = _dev(rng.standard_normal(mesh.num_nodes))
  bcs = {'x0': (D, 0.0), 'x1': (D, 1.0), 'y0': (RB, (2.0, 1.0))}
  ref, info0 = solve_helmholtz(mesh, f, bcs, rtol=1e-13, diffusivity=k,
                               reaction=0.5, lambda0=1.0, return_info=True)
  u, info = solve_helmholtz(mesh, f, bcs, rtol=1e-13, diffusivity=k,
                            reaction=0.5, lambda0=1.0, return_info=True,
                            preconditioner=preconditioner)
  err = np.abs(_np(u) - _np(ref)).max() / np.abs(_np(ref)).max()
  assert err <= 1e-8, err
  its, its0 = int(info['num_iterations']), int(info0['num_iterations'])
  print(f'{preconditioner}: {its} iterations (plain CG {its0})')
  assert its < its0
  if preconditioner == 'pmg':
    assert its <= PMG_ITERATION_BOUND, its


PMG_ITERATION_BOUND = 20   # measured: 13 (plain CG: 4283)


# --------------------------------------------- 4. manufactured solution
def test_manufactured_converges():
  """u = sin(x) cos(y) e^z style solution with callable k and c, a Neumann
  face (the flux k du/dn) and a Robin face; the error falls with the order."""
  errs = []
  for P in (2, 4, 6):
    rp = _box(2, 2, P)
    mesh = rp.finalize(device=DEV)
    ex = lambda x: torch.sin(x[:, 0] + 0.3) * torch.cos(x[:, 1])
    kf = lambda x: 1.0 + x[:, 0] ** 2
    cf = lambda x: 2.0 + x[:, 1]
    # -div(k grad u) + c u with u = sin(x+.3) cos(y), k = 1 + x^2:
    # u_x = cos(x+.3)cos y, u_xx = -u, u_yy = -u
    def forcing(x):
      ux = torch.cos(x[:, 0] + 0.3) * torch.cos(x[:, 1])
      u = ex(x)
      return -(2 * x[:, 0] * ux - kf(x) * u - kf(x) * u) + cf(x) * u
    fl = lambda x: -kf(x) * torch.sin(x[:, 0] + 0.3) * -torch.sin(x[:, 1]) * 0
    x = mesh.node_coords
    # flux on y0 (outward normal -y): -k u_y = k sin(x+.3) sin(y) = 0 at y=0
    # Robin on x1 (normal +x): k u_x + alpha u = g
    g = lambda y: (kf(y) * torch.cos(y[:, 0] + 0.3) * torch.cos(y[:, 1]) +
                   2.0 * ex(y))
    bcs = {'x0': (D, ex), 'y1': (D, ex), 'y0': (N, fl), 'x1': (RB, (2.0, g))}
    u = solve_helmholtz(mesh, forcing(x), bcs, lambda0=1.0, rtol=1e-13,
                        diffusivity=kf, reaction=cf, preconditioner='jacobi')
    errs.append(float((u - ex(x)).abs().max()))
  assert errs[1] < 0.1 * errs[0] and errs[2] < 0.1 * errs[1], errs
