"""Host-side checks of neo-Hookean elasticity: the NumPy
reference (`tests/hyperelastic_reference.py`) against properties that need no
second implementation -- the residual is the derivative of the energy, the
tangent the derivative of the residual, symmetry, the linear operator at
u = 0, objectivity -- so that the GPU tests rest on something verified; the
state layout; the header and its ctypes mirror; the refusals of
`solve_hyperelasticity` that need no device; the dense Newton on a
homogeneous stretch."""
import ctypes
import os
import re

import numpy as np
import pytest

from swirl_fem_amd import _lib
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType
from swirl_fem_amd.examples.hyperelasticity import BCType
from swirl_fem_amd.examples.hyperelasticity import solve_hyperelasticity
from tests import elasticity_reference as ER
from tests import geometry_cases as G
from tests import hyperelastic_reference as HR
from tests import transport_reference as TR

P = 3
CASES = [('multilinear', 2), ('three_kinds', 2), ('three_kinds', 3),
         ('affine', 3)]
SCALE = 0.3     # the largest Frobenius norm of H of a random field


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


def _field(fes, rng):
  """A random nodal field whose largest |H| over the quadrature points is
  SCALE, so J >= (1 - SCALE)^d everywhere."""
  u = rng.standard_normal((fes.num_nodes, fes.ndim))
  H = HR.gradients(fes, fes.gather(u))
  u *= SCALE / np.sqrt((H * H).sum((-2, -1))).max()
  H = HR.gradients(fes, fes.gather(u))
  assert np.linalg.det(H + np.eye(fes.ndim)).min() >= 0.3
  return u


# ------------------------------------------------------------ pointwise
@pytest.mark.parametrize('d', [2, 3])
def test_pointwise_derivatives(d):
  """P : dH is the central difference of psi, dP[dH] that of P, and the
  fourth-order moduli contract to dP (h = 1e-5: truncation h^2 times an O(10)
  constant, rounding 1e-16 / h; 1e-8 bounds both with room)."""
  rng = np.random.default_rng(d)
  lam, mu, h = 1.3, 0.7, 1e-5
  for _ in range(5):
    H = rng.standard_normal((d, d))
    H *= SCALE / np.linalg.norm(H)
    dH = rng.standard_normal((d, d))
    dH /= np.linalg.norm(dH)
    fd = (HR.psi(H + h * dH, lam, mu) - HR.psi(H - h * dH, lam, mu)) / (2 * h)
    assert abs(fd - (HR.piola(H, lam, mu) * dH).sum()) <= 1e-8
    fd = (HR.piola(H + h * dH, lam, mu) - HR.piola(H - h * dH, lam, mu)) / (
        2 * h)
    dP = HR.dpiola(H, dH, lam, mu)
    assert np.abs(fd - dP).max() <= 1e-8
    C = HR.tangent_moduli(H, lam, mu)
    assert np.abs(np.einsum('cjbl,bl->cj', C, dH) - dP).max() <= 1e-13
    # major symmetry: the tangent comes from an energy
    assert np.abs(C - C.transpose(2, 3, 0, 1)).max() <= 1e-13
  # small strains: P(eps H) / eps is the linear stress up to O(eps)
  H = rng.standard_normal((d, d))
  H /= np.linalg.norm(H)
  eps = 1e-6
  lin = ER.stress(H, lam, mu)
  assert np.abs(HR.piola(eps * H, lam, mu) / eps - lin).max() <= 10 * eps


# ------------------------------------------------- residual, tangent, energy
@pytest.mark.parametrize('kind,ndim', CASES)
def test_residual_is_derivative_of_energy(kind, ndim):
  """R(u) . v equals the central difference of Psi along v (h = 1e-5,
  relative 1e-6), with variable coefficients and a mass term."""
  rp, fes = _space(kind, ndim)
  rng = np.random.default_rng(ndim)
  lam, mu, rho = _coefficients(fes, rng)
  u = _field(fes, rng)
  h = 1e-5
  for l0 in (0.0, 1.7):
    R = HR.residual(fes, u, lam, mu, rho, l0)
    for _ in range(3):
      v = rng.standard_normal(u.shape)
      v /= np.abs(v).max()
      fd = (HR.energy(fes, u + h * v, lam, mu, rho, l0) -
            HR.energy(fes, u - h * v, lam, mu, rho, l0)) / (2 * h)
      assert abs(fd - (R * v).sum()) <= 1e-6 * np.linalg.norm(R) * \
          np.linalg.norm(v)


@pytest.mark.parametrize('kind,ndim', CASES)
def test_tangent_is_derivative_of_residual(kind, ndim):
  """T(u) w equals the central difference of R along w (h = 1e-5, 1e-6
  relative: truncation is h^2 times an O(10) constant and rounding 1e-16 /
  h), by `local_tangent` (from dP) and by the assembled matrix (from the
  moduli); the matrix is symmetric to 1e-13."""
  rp, fes = _space(kind, ndim)
  rng = np.random.default_rng(10 + ndim)
  lam, mu, rho = _coefficients(fes, rng)
  u = _field(fes, rng)
  h = 1e-5
  for l0 in (0.0, 1.7):
    A = HR.assemble_tangent(fes, u, lam, mu, rho, l0)
    assert np.abs(A - A.T).max() <= 1e-13 * np.abs(A).max()
    Ke = HR.local_tangent_matrix(fes, fes.gather(u), lam, mu, rho, l0)
    assert np.abs(Ke - Ke.transpose(0, 2, 1)).max() <= 1e-13 * np.abs(Ke).max()
    w = rng.standard_normal(u.shape)
    fd = (HR.residual(fes, u + h * w, lam, mu, rho, l0) -
          HR.residual(fes, u - h * w, lam, mu, rho, l0)) / (2 * h)
    Tw = HR.tangent(fes, u, w, lam, mu, rho, l0)
    scale = np.abs(Tw).max()
    assert np.abs(fd - Tw).max() <= 1e-6 * scale
    assert np.abs((A @ w.reshape(-1)).reshape(w.shape) - Tw).max() <= \
        1e-12 * scale


@pytest.mark.parametrize('kind,ndim', CASES)
def test_grid_agrees_with_local(kind, ndim):
  """`grid_*` (the kernel's steps, sum-factorised) between interpolation and
  its transpose equals `local_*` (physical basis gradients) to 1e-12; so do
  the energy and the state."""
  rp, fes = _space(kind, ndim)
  rng = np.random.default_rng(20 + ndim)
  lam, mu, rho = _coefficients(fes, rng)
  u = _field(fes, rng)
  ul = fes.gather(u)
  wl = fes.gather(rng.standard_normal(u.shape))
  to_grid = lambda v: np.einsum('qi,eic->eqc', fes.M, v)
  back = lambda r: np.einsum('qi,eqc->eic', fes.M, r)
  for l0 in (0.0, 1.7):
    rq, st, pq = HR.grid_residual(fes, to_grid(ul), lam, mu, rho, l0)
    want = HR.local_residual(fes, ul, lam, mu, rho, l0)
    assert np.abs(back(rq) - want).max() <= 1e-12 * np.abs(want).max()
    e = HR.local_energy(fes, ul, lam, mu, rho, l0)
    assert np.abs(pq - e).max() <= 1e-12 * np.abs(e).max()
    assert abs(pq.sum() - HR.energy(fes, u, lam, mu, rho, l0)) <= \
        1e-12 * abs(pq.sum())
    assert np.abs(st - HR.state(HR.gradients(fes, ul))).max() <= 1e-12
    tq = HR.grid_tangent(fes, to_grid(wl), st, lam, mu, rho, l0)
    want = HR.local_tangent(fes, ul, wl, lam, mu, rho, l0)
    assert np.abs(back(tq) - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize('kind,ndim', CASES)
def test_tangent_at_zero_is_linear_operator(kind, ndim):
  """At u = 0 the tangent matrix is the linear element matrix of
  `elasticity_reference`, and the state is (I, 0)."""
  rp, fes = _space(kind, ndim)
  lam, mu, rho = _coefficients(fes, np.random.default_rng(5))
  zero = np.zeros((fes.num_elements, fes.n, ndim))
  for l0 in (0.0, 2.5):
    got = HR.local_tangent_matrix(fes, zero, lam, mu, rho, l0)
    want = ER.element_matrices(fes, lam, mu, rho, l0)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
  st = HR.state(HR.gradients(fes, zero))
  d = ndim
  assert np.array_equal(st[0, 0, :d * d].reshape(d, d), np.eye(d))
  assert np.all(st[..., d * d] == 0.0)


@pytest.mark.parametrize('ndim', [2, 3])
def test_objectivity(ndim):
  """u = (Rot - I) x with a rotation by 30 degrees: F is a rotation, so the
  residual and the energy vanish to 1e-12, while the linear K u does not."""
  rp, fes = _space('three_kinds', ndim)
  x = np.asarray(rp.node_coords, np.float64)
  c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
  Rot = np.eye(ndim)
  Rot[:2, :2] = [[c, -s], [s, c]]
  u = x @ (Rot - np.eye(ndim)).T
  lam, mu = 1.3, 0.7
  R = HR.residual(fes, u, lam, mu)
  Ku = ER.apply(fes, u, lam, mu)
  print(f'{ndim}D rotation: |R| {np.abs(R).max():.2e}, energy '
        f'{HR.energy(fes, u, lam, mu):.2e}, |K u| {np.abs(Ku).max():.2e}')
  assert np.abs(R).max() <= 1e-12
  assert abs(HR.energy(fes, u, lam, mu)) <= 1e-12
  assert np.abs(Ku).max() >= 1e-2


def test_state_layout():
  """Slots 0 .. d*d - 1 are F^-1 row-major, slot d*d is ln J."""
  for d in (2, 3):
    rng = np.random.default_rng(d)
    H = 0.1 * rng.standard_normal((4, 5, d, d))
    st = HR.state(H)
    assert st.shape == (4, 5, d * d + 1)
    F = H + np.eye(d)
    for c in range(d):
      for j in range(d):
        assert np.allclose(st[..., c * d + j], np.linalg.inv(F)[..., c, j],
                           rtol=0, atol=1e-15)
    assert np.allclose(st[..., d * d], np.log(np.linalg.det(F)), rtol=0,
                       atol=1e-15)
  # an inverted state is non-finite, not an exception
  st = HR.state(np.array([[-1.5, 0.0], [0.0, 0.0]]))
  assert not np.isfinite(st[-1])


# ------------------------------------------------------- header and ABI
def _declared(text, name):
  body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), text,
                   flags=re.S).group(1)
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  names = []
  for decl in body.split(';'):
    decl = decl.strip()
    if not decl:
      continue
    first, *rest = decl.split(',')
    names.append(re.findall(r'\w+', first)[-1])
    names += [r.strip() for r in rest]
  return names


def test_struct_layout():
  """`sfem_hyperelastic_args` in the header and its ctypes mirror: the fields
  of `sfem_elasticity_args` in the same order, then `state`, `psi`, `mode`;
  the mode values; the ABI number is unchanged (a pure addition)."""
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  text = open(os.path.join(root, 'include', 'sfem.h')).read()
  assert '#define SFEM_ABI_VERSION 10' in text and _lib.ABI_VERSION == 10
  names = _declared(text, 'sfem_hyperelastic_args')
  parent = _declared(text, 'sfem_elasticity_args')
  assert names == parent + ['state', 'psi', 'mode']
  fields = _lib.HyperelasticArgs._fields_
  assert names == [f[0] for f in fields], (names, fields)
  kinds = dict(fields)
  assert kinds['state'] is _lib.c_ptr and kinds['psi'] is _lib.c_ptr
  assert kinds['mode'] is _lib.c_i32
  # the parent (13 pointers, 4 doubles, 2 int64, 4 int32), 2 pointers, one
  # int32 padded to the alignment of the struct
  assert ctypes.sizeof(_lib.HyperelasticArgs) == \
      ctypes.sizeof(_lib.ElasticityArgs) + 2 * 8 + 8
  assert _lib.HyperelasticArgs.state.offset == ctypes.sizeof(
      _lib.ElasticityArgs)
  assert re.search(r'#define SFEM_HYPER_RESIDUAL 0\b', text)
  assert re.search(r'#define SFEM_HYPER_TANGENT 1\b', text)
  assert (_lib.SFEM_HYPER_RESIDUAL, _lib.SFEM_HYPER_TANGENT) == (0, 1)
  sig = _lib.SIGNATURES['sfem_hyperelastic_local']
  assert sig[0]._type_ is _lib.HyperelasticArgs and sig[1] is _lib.c_ptr
  assert re.search(r'int sfem_hyperelastic_local\(const '
                   r'sfem_hyperelastic_args\* args,\s*sfem_stream_t stream\);',
                   text)


# ------------------------------------------------------------- refusals
@pytest.fixture(scope='module')
def cpu_mesh():
  return TR.box_with_sides(2, 2, P).finalize(device='cpu')


def test_solve_refusals(cpu_mesh):
  """What `solve_hyperelasticity` refuses before it touches a device."""
  import torch
  D, N = BCType.DIRICHLET, BCType.NEUMANN
  kw = dict(lame_lambda=1.0, lame_mu=1.0)
  clamp = {'x0': (D, (0.0, 0.0))}
  f = (0.0, -1.0)
  solve = solve_hyperelasticity
  with pytest.raises(ValueError, match='rigid-body'):
    solve(cpu_mesh, f, {}, **kw)
  with pytest.raises(ValueError, match='rigid-body'):
    solve(cpu_mesh, f, {'x1': (N, (1.0, None))}, **kw)
  with pytest.raises(ValueError, match='DIRICHLET or NEUMANN'):
    solve(cpu_mesh, f, {'x0': (BCType.ROBIN, (0.0, 0.0))}, **kw)
  with pytest.raises(ValueError, match='one entry per component'):
    solve(cpu_mesh, f, {'x0': (D, (0.0, 0.0, 0.0))}, **kw)
  with pytest.raises(KeyError):
    solve(cpu_mesh, f, {'nowhere': (D, (0.0, 0.0))}, **kw)
  with pytest.raises(NotImplementedError, match='pmg'):
    solve(cpu_mesh, f, clamp, preconditioner='pmg', **kw)
  with pytest.raises(ValueError, match='unknown preconditioner'):
    solve(cpu_mesh, f, clamp, preconditioner='ilu', **kw)
  for bad in (0, -1, 1.5):
    with pytest.raises(ValueError, match='load_steps'):
      solve(cpu_mesh, f, clamp, load_steps=bad, **kw)
  with pytest.raises(NotImplementedError, match='ensemble'):
    solve(cpu_mesh.replicate(2), f, clamp, **kw)
  with pytest.raises(NotImplementedError, match='autograd'):
    solve(cpu_mesh, torch.tensor(f, requires_grad=True), clamp, **kw)
  with pytest.raises(NotImplementedError, match='autograd'):
    solve(cpu_mesh, f, clamp, lame_lambda=1.0,
          lame_mu=torch.tensor(1.0, requires_grad=True))


def test_solve_refuses_partitions_and_periodic_images():
  from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
  from swirl_fem_amd.core.mesh_refiner import refine_premesh
  from swirl_fem_amd.distributed import blocks
  kw = dict(lame_lambda=1.0, lame_mu=1.0)
  part = blocks.build_block_partition(2, 3, (2, 1, 1), 0, device='cpu')
  with pytest.raises(NotImplementedError, match='partitioned'):
    solve_hyperelasticity(part.mesh, (0.0, 0.0, 1.0), {}, lambda0=1.0, **kw)
  pm = unit_cube_mesh(2, ndim=2, periodic_dims=(0,))
  mesh = refine_premesh(pm, Nodes1D.create(
      P, NodeType.GAUSS_LOBATTO_LEGENDRE)).finalize(device='cpu')
  with pytest.raises(NotImplementedError, match='periodic'):
    solve_hyperelasticity(mesh, (0.0, 1.0), {}, lambda0=1.0, **kw)


# ----------------------------------------------------------- dense Newton
def _on(x, axis, value):
  return np.abs(x[:, axis] - value) < 1e-9


@pytest.mark.parametrize('ndim', [2, 3])
def test_uniaxial_lateral_stretch(ndim):
  a, lam, mu = 1.5, 1.3, 0.7
  b = HR.uniaxial_lateral_stretch(a, lam, mu, ndim)
  assert 0.5 < b < 1.0
  J = a * b ** (ndim - 1)
  assert abs(mu * (b - 1 / b) + lam * np.log(J) / b) <= 1e-14
  H = np.diag([a - 1.0] + [b - 1.0] * (ndim - 1))
  Pk = HR.piola(H, lam, mu)
  assert np.abs(Pk - np.diag(np.diag(Pk))).max() == 0.0
  assert np.abs(np.diag(Pk)[1:]).max() <= 1e-14
  assert abs(Pk[0, 0] - HR.uniaxial_traction(a, lam, mu, ndim)) <= 1e-14


@pytest.mark.parametrize('drive', ['dirichlet', 'dead_load'])
def test_dense_newton_reaches_uniaxial_solution(drive):
  """Homogeneous stretch a = 1.5 in 2D with rollers on x0 and y0, driven by
  the end displacement or by the dead load P_11 on x1, on a mesh with a moved
  interior vertex: the solution ((a - 1) x, (b - 1) y) is linear, so in the
  space; load_steps = 4, rtol 1e-10; nodal error at most 1e-8."""
  a, lam, mu, ndim = 1.5, 1.3, 0.7, 2
  b = HR.uniaxial_lateral_stretch(a, lam, mu, ndim)
  rp = ER.jittered_box(2, ndim, P)
  x = np.asarray(rp.node_coords, np.float64)
  dense = HR.DenseNewton(rp, P, lam, mu)
  fixed = np.zeros(x.shape, bool)
  values = np.zeros(x.shape)
  fixed[_on(x, 0, 0.0), 0] = True
  fixed[_on(x, 1, 0.0), 1] = True
  tractions = []
  if drive == 'dirichlet':
    end = _on(x, 0, 1.0)
    fixed[end, 0], values[end, 0] = True, a - 1.0
  else:
    mesh = rp.finalize(device='cpu')
    facets = mesh.boundary_facets['x1'].cpu().numpy().astype(np.int64)
    tractions = [(facets, [HR.uniaxial_traction(a, lam, mu, ndim), None])]
  u, counts = dense.solve(np.zeros(x.shape), fixed, values, tractions,
                          load_steps=4, rtol=1e-10)
  want = np.stack([(a - 1.0) * x[:, 0], (b - 1.0) * x[:, 1]], axis=-1)
  err = np.abs(u - want).max()
  print(f'{drive}: Newton iterations per load step {counts}, error {err:.2e}')
  assert len(counts) == 4 and max(counts) <= 10
  assert err <= 1e-8
