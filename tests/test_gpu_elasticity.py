"""Linear elasticity on the GPU: the kernel
`sfem_elasticity_local` at every Q = 2..12 against the NumPy reference
(`tests/elasticity_reference.py`), the assembled operator (masks, layouts,
symmetry, rigid motions, the generic-form path), its diagonal, solves against
dense solves, exact and manufactured solutions, Jacobi and the refusals."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from swirl_fem_amd import _lib, _ops
from swirl_fem_amd.core import layout, operators
from swirl_fem_amd.core.fespace import FiniteElementSpace, grad
from swirl_fem_amd.core.interpolation import NodeType, Quadrature1D
from swirl_fem_amd.examples.elasticity import BCType, solve_elasticity
from tests import elasticity_reference as ER
from tests import geometry_cases as G
from tests import transport_reference as TR
from tests.fp32util import F32Rng, f32r, tolerance

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GLL, GL = NodeType.GAUSS_LOBATTO_LEGENDRE, NodeType.GAUSS_LEGENDRE
D, N = BCType.DIRICHLET, BCType.NEUMANN
MESH_P = 3       # nodes per direction of the kernel tests' meshes


def _dev(a, dtype=torch.float64):
  return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _np(t):
  return t.detach().double().cpu().numpy()


def _rel(a, b):
  return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _t(fn):
  """A NumPy callable on points as a torch callable."""
  return lambda x: _dev(fn(_np(x)))


def _rigid_modes(x):
  n, d = x.shape
  modes = [np.tile(np.eye(d)[c], (n, 1)) for c in range(d)]
  for a in range(d):
    for b in range(a + 1, d):
      r = np.zeros((n, d))
      r[:, a], r[:, b] = -x[:, b], x[:, a]
      modes.append(r)
  return modes


# ------------------------------------------------ 1. kernel vs reference
def _kernel_setup(case, Q, dtype=torch.float64):
  mesh, _, rp = case.finalize(DEV, dtype)
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(Q, GL))
  ref = ER.space(rp.node_coords, rp.elements, MESH_P, (Q, 'gl'))
  op = fes.elasticity_operator(lame_lambda=1.0, lame_mu=1.0)
  return mesh, fes, ref, op


# (lambda, mu, rho: 'p' per point around the number, or the scalar; lambda0)
KERNEL_COMBOS = [
    (1.3, 0.7, None, 0.0),
    (('p', 1.0), ('p', 0.8), ('p', 1.5), 2.5),
    (('p', 0.9), 0.6, ('p', 2.0), 0.0),
    (0.0, ('p', 0.8), 1.5, 0.7),
    (50.0, 1.0, None, 0.0),
    (('p', 50.0), ('p', 1.0), None, 1.1),
]
FP32_COMBOS = [c for c in KERNEL_COMBOS if not (
    (c[0][1] if isinstance(c[0], tuple) else c[0]) > 2.0)]


def _run_combos(op, ref, ndim, Q, pad, rng, dtype, tol, combos, rnd=lambda a: a):
  """Each combination against `grid_apply`.  Above `tol` in fp32 the
  project's exception rule applies: the NumPy reference evaluated in
  float32, 4 times its error.  Returns [(combo index, error, allowed)]."""
  E, nq = ref.num_elements, ref.Q
  rows = []
  for n, (lam, mu, rho, l0) in enumerate(combos):
    def coef(c):
      if isinstance(c, tuple):
        return rnd(c[1] * (1.0 + 0.2 * rng.uniform(-1, 1, (E, nq))))
      return c
    lam, mu, rho = coef(lam), coef(mu), coef(rho)
    uq = rnd(rng.standard_normal((E, nq, ndim)))
    want = ER.grid_apply(ref, uq, lam, mu, rho, l0)

    def dev(c):
      if isinstance(c, np.ndarray):
        return _dev(np.concatenate([c, np.ones((pad, nq))]), dtype)
      return c
    got = _ops.elasticity_local(
        _dev(np.concatenate([uq, rng.standard_normal((pad, nq, ndim))]),
             dtype), op.parts, op.host, ndim, Q, op.point_weights(),
        dev(lam), dev(mu), dev(rho), l0)
    assert got.shape == (E + pad, nq, ndim) and got.dtype == dtype
    err = _rel(_np(got)[:E], want)
    allowed = tol
    if err > tol and dtype == torch.float32:
      ref32 = ER.grid_apply(ref, uq, lam, mu, rho, l0, dtype=np.float32)
      allowed = max(tol, 4.0 * _rel(ref32.astype(np.float64), want))
    print(f'{dtype} ndim={ndim} Q={Q} combo {n}: rel err {err:.3e} '
          f'(allowed {allowed:.3e})')
    rows.append((n, err, allowed))
    assert err <= allowed, (ndim, Q, n, err, allowed)
  return rows


@pytest.mark.parametrize('Q', range(2, 13))
@pytest.mark.parametrize('ndim', [2, 3])
def test_kernel_matches_reference(ndim, Q):
  """fp64, every Q: scalar and per-point coefficients, rho with and without
  a mass term, lambda = 0, lambda / mu = 50, on multilinear and curved
  elements with a padded row (list launches, a partial workgroup)."""
  case = G.three_kinds(2, ndim, MESH_P, pad=1)
  mesh, fes, ref, op = _kernel_setup(case, Q)
  assert len(op.parts) >= 2 and all('elem_list' in p for p in op.parts)
  assert {G.CURVED, G.MULTILINEAR} <= {p['geo_mode'] for p in op.parts}
  rng = np.random.default_rng(100 * ndim + Q)
  _run_combos(op, ref, ndim, Q, 1, rng, torch.float64,
              tolerance(torch.float64, Q), KERNEL_COMBOS)


@pytest.mark.parametrize('Q', range(2, 13))
@pytest.mark.parametrize('ndim', [2, 3])
def test_kernel_affine_elements(ndim, Q):
  """The affine instantiations at every Q (one launch over all elements, no
  list): the mesh of the test above has no affine element."""
  case = G.affine(2, ndim, MESH_P)
  mesh, fes, ref, op = _kernel_setup(case, Q)
  assert [p['geo_mode'] for p in op.parts] == [G.AFFINE]
  assert 'elem_list' not in op.parts[0]
  rng = np.random.default_rng(7 * ndim + Q)
  _run_combos(op, ref, ndim, Q, 0, rng, torch.float64,
              tolerance(torch.float64, Q), KERNEL_COMBOS[:3])


@pytest.mark.parametrize('Q', [2, 5, 8, 9, 12])
@pytest.mark.parametrize('ndim', [2, 3])
def test_kernel_fp32(ndim, Q):
  """fp32 with float32-representable meshes and inputs against the fp64
  reference at `tolerance(torch.float32, Q)`, lambda / mu <= 2 (cancellation
  in tr H is not what is tested).  A case above that is held to 4 times the
  error of the NumPy reference evaluated in float32 (DESIGN §3.16 lists
  them)."""
  case = G.three_kinds(2, ndim, MESH_P)
  mesh, fes, ref, op = _kernel_setup(case, Q, torch.float32)
  rng = F32Rng(Q)
  _run_combos(op, ref, ndim, Q, 0, rng, torch.float32,
              tolerance(torch.float32, Q), FP32_COMBOS, rnd=f32r)


# ------------------------------------------------ 2. assembled operator
def _coef_fns(ndim):
  lam = lambda x: 1.0 + 0.5 * np.sin(2.0 * x[..., 0]) * x[..., 1]
  mu = lambda x: 0.7 + 0.3 * x[..., ndim - 1] ** 2
  rho = lambda x: 1.5 + np.cos(x[..., 0])
  return lam, mu, rho


@functools.lru_cache(maxsize=None)
def _assembled(kind, ndim):
  P = 4 if ndim == 2 else 3
  case = getattr(G, kind)(2, ndim, P)
  mesh, _, rp = case.finalize(DEV, torch.float64)
  q = P - 1 + (ndim + 1) // 2
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(q, GL))
  ref = ER.space(rp.node_coords, rp.elements, P, (q, 'gl'))
  lam, mu, rho = _coef_fns(ndim)
  xq = ER.quad_points(ref)
  return mesh, fes, ref, (lam, mu, rho), (lam(xq), mu(xq), rho(xq))


ASSEMBLED = [('multilinear', 2), ('curved_multilinear', 2),
             ('multilinear', 3), ('curved_multilinear', 3)]


@pytest.mark.parametrize('kind,ndim', ASSEMBLED)
def test_apply_matches_reference(kind, ndim):
  """Per-component mask, dense and component-major layouts, with and without
  the mass term, against `reference.apply`."""
  mesh, fes, ref, fns, vals = _assembled(kind, ndim)
  rng = np.random.default_rng(ndim)
  fixed = rng.uniform(size=(mesh.num_nodes, ndim)) < 0.25
  op = fes.elasticity_operator(_dev(fixed, torch.bool), lame_lambda=_t(fns[0]),
                               lame_mu=_t(fns[1]), density=_t(fns[2]))
  u = rng.standard_normal((mesh.num_nodes, ndim))
  for l0 in (0.0, 1.7):
    want = ER.apply(ref, u, *vals, l0, keep=(~fixed).astype(float))
    dense = op.apply(_dev(u), l0)
    assert dense.is_contiguous()
    assert _rel(_np(dense), want) <= 1e-10
    cm = layout.component_major(_dev(u))
    assert not cm.is_contiguous()
    got = op.apply(cm, l0)
    assert layout.is_component_major(got) and got.stride() == cm.stride()
    assert _rel(_np(got), want) <= 1e-10
    assert _rel(_np(op.linear_operator(l0)(_dev(u))), want) <= 1e-10
  # (N,) mask: every component of the node
  nodes = rng.uniform(size=mesh.num_nodes) < 0.3
  op1 = fes.elasticity_operator(_dev(nodes, torch.bool), lame_lambda=2.0,
                                lame_mu=0.5)
  keep = np.repeat((~nodes)[:, None], ndim, axis=1).astype(float)
  want = ER.apply(ref, u, 2.0, 0.5, keep=keep)
  assert _rel(_np(op1.apply(_dev(u))), want) <= 1e-10


@pytest.mark.parametrize('kind,ndim', ASSEMBLED)
def test_symmetry_and_rigid_motions(kind, ndim):
  """v . K u = u . K v to 1e-12; translations and infinitesimal rotations
  are annihilated (1e-12 of the largest diagonal entry times |u|)."""
  mesh, fes, ref, fns, vals = _assembled(kind, ndim)
  op = fes.elasticity_operator(lame_lambda=_t(fns[0]), lame_mu=_t(fns[1]),
                               density=_t(fns[2]))
  rng = np.random.default_rng(3)
  u = _dev(rng.standard_normal((mesh.num_nodes, ndim)))
  v = _dev(rng.standard_normal((mesh.num_nodes, ndim)))
  for l0 in (0.0, 0.9):
    Ku, Kv = op.apply(u, l0), op.apply(v, l0)
    a, b = float((v * Ku).sum()), float((u * Kv).sum())
    scale = float(v.norm() * Ku.norm())
    print(f'{kind} {ndim}D lambda0={l0}: |vKu - uKv| / (|v||Ku|) = '
          f'{abs(a - b) / scale:.2e}')
    assert abs(a - b) <= 1e-12 * scale
  dmax = float(op.diagonal().max())
  x = _np(mesh.node_coords)
  for m in _rigid_modes(x):
    res = _np(op.apply(_dev(m)))
    assert np.abs(res).max() <= 1e-12 * dmax * np.abs(m).max()


@pytest.mark.parametrize('kind,ndim', [('curved_multilinear', 2),
                                       ('curved_multilinear', 3)])
def test_fused_equals_generic_form(kind, ndim):
  """The fused operator against what a user would write without it:
  `local_covector` of sigma(u) : grad v with `vector_function` and `grad`."""
  mesh, fes, ref, fns, vals = _assembled(kind, ndim)
  lam, mu = 1.3, 0.6
  op = fes.elasticity_operator(lame_lambda=lam, lame_mu=mu)
  rng = np.random.default_rng(11)
  u = _dev(rng.standard_normal((mesh.num_nodes, ndim)))

  def form(uf, vf):
    def at(x):
      gu, gv = grad(uf)(x), grad(vf)(x)
      sym = gu + torch.einsum('jk->kj', gu)
      return mu * torch.vdot(sym, gv) + lam * torch.trace(gu) * torch.trace(gv)
    return at
  u_local = _ops.gather_rows(u, mesh.elements)
  loc = fes.local_covector(form, (fes.vector_function(u_local),
                                  fes.vector_function(None)))
  want = _ops.scatter_add(loc.contiguous(), mesh.elements, mesh.num_nodes,
                          ncomp=ndim)
  got = op.apply(u)
  assert _rel(_np(got), _np(want)) <= 1e-10
  assert _rel(_np(got), ER.apply(ref, _np(u), lam, mu)) <= 1e-10


# ------------------------------------------------------------ 3. diagonal
@pytest.mark.parametrize('collocated', [False, True])
@pytest.mark.parametrize('ndim', [2, 3])
def test_diagonal_matches_reference(ndim, collocated):
  """Collocated (GLL rule on the nodes) and two-grid spaces on a mesh with
  all three geometry kinds, variable coefficients, a per-component mask."""
  P = 4 if ndim == 2 else 3
  case = G.three_kinds(3, ndim, P)
  mesh, _, rp = case.finalize(DEV, torch.float64)
  rule = (P, GLL, 'gll') if collocated else (P + 1, GL, 'gl')
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(rule[0], rule[1]))
  assert fes.is_collocated == collocated
  ref = ER.space(rp.node_coords, rp.elements, P, (rule[0], rule[2]))
  fns = _coef_fns(ndim)
  xq = ER.quad_points(ref)
  vals = [f(xq) for f in fns]
  rng = np.random.default_rng(ndim)
  fixed = rng.uniform(size=(mesh.num_nodes, ndim)) < 0.2
  op = fes.elasticity_operator(_dev(fixed, torch.bool), lame_lambda=_t(fns[0]),
                               lame_mu=_t(fns[1]), density=_t(fns[2]))
  assert {p['geo_mode'] for p in op.parts} == {G.CURVED, G.MULTILINEAR,
                                              G.AFFINE}
  keep = (~fixed).astype(float)
  for l0 in (0.0, 2.5):
    want = ER.diagonal(ref, *vals, l0, keep=keep)
    got = op.diagonal(l0)
    assert tuple(got.shape) == (mesh.num_nodes, ndim)
    assert _rel(_np(got), want) <= 1e-10
  # the diagonal is that of the operator the apply computes
  u = rng.standard_normal((mesh.num_nodes, ndim))
  assert _rel(_np(op.apply(_dev(u), 2.5)),
              ER.apply(ref, u, *vals, 2.5, keep=keep)) <= 1e-10
  # scalar coefficients, no mask
  op2 = fes.elasticity_operator(lame_lambda=0.0, lame_mu=2.0)
  assert _rel(_np(op2.diagonal()), ER.diagonal(ref, 0.0, 2.0)) <= 1e-10


# -------------------------------------------------------------- 4. solves
def _facets(mesh, group):
  return mesh.boundary_facets[group].cpu().numpy().astype(np.int64)


def _on(x, axis, value):
  return np.abs(x[:, axis] - value) < 1e-9


@pytest.mark.parametrize('ndim,order,pc', [(2, 5, None), (2, 4, 'jacobi'),
                                           (3, 3, 'jacobi')])
def test_solve_matches_dense_solve(ndim, order, pc):
  """Clamped face x0 with inhomogeneous values, a roller on y0 (normal
  component fixed, with a value), a traction on x1, a body force, variable
  coefficients; rtol = 1e-12, against `numpy.linalg.solve` to 1e-8."""
  P = order + 1
  rp = TR.box_with_sides(2, ndim, P, three_kinds=True)
  mesh = rp.finalize(device=DEV)
  x = np.asarray(rp.node_coords, np.float64)
  lam, mu, _ = _coef_fns(ndim)
  dense = ER.Dense(rp, P, lam, mu)
  gD = [lambda y: 0.01 * y[:, 1] ** 2, lambda y: 0.02 * np.sin(y[:, 1]),
        lambda y: 0.01 * y[:, 0] * y[:, 1]][:ndim]
  roll = lambda y: 0.005 * np.cos(2.0 * y[:, 0])
  trac = [lambda y: 1.0 + y[:, 1], None, 0.3][:ndim]
  force = lambda y: np.stack(
      [np.sin(2.0 * y[:, 0]), -1.0 + 0.0 * y[:, 0], y[:, 0] * y[:, 1]][:ndim],
      axis=-1)
  fixed = np.zeros(x.shape, bool)
  values = np.zeros(x.shape)
  on_y0, on_x0 = _on(x, 1, 0.0), _on(x, 0, 0.0)
  fixed[on_y0, 1], values[on_y0, 1] = True, roll(x)[on_y0]
  fixed[on_x0] = True                    # the later group wins where they meet
  values[on_x0] = np.stack([g(x) for g in gD], axis=-1)[on_x0]
  want = dense.solve(force(x), fixed, values,
                     [(_facets(mesh, 'x1'), trac)])
  free_y0 = [None] * ndim
  free_y0[1] = _t(roll)
  bcs = {'y0': (D, tuple(free_y0)),
         'x0': (D, tuple(_t(g) for g in gD)),
         'x1': (N, tuple(g if not callable(g) else _t(g) for g in trac))}
  u, info = solve_elasticity(mesh, _t(force), bcs, lame_lambda=_t(lam),
                             lame_mu=_t(mu), rtol=1e-12, preconditioner=pc,
                             return_info=True)
  assert info['status'] == 'converged'
  err = _rel(_np(u), want)
  print(f'{ndim}D order {order} {pc}: {info["num_iterations"]} iterations, '
        f'rel err {err:.2e}')
  assert err <= 1e-8
  # the data are met exactly
  assert np.abs(_np(u)[fixed] - values[fixed]).max() <= 1e-14


@pytest.mark.parametrize('ndim', [2, 3])
def test_uniaxial_tension(ndim):
  """Rollers on the coordinate planes through the origin, traction t on the
  opposite x face, on a mesh with a moved interior vertex: the exact solution
  is linear, u = (t x / E, -nu t y / E, -nu t z / E) in 3D and its
  plane-strain counterpart ((1 - nu^2) t x / E, -nu (1 + nu) t y / E) in 2D,
  to 1e-9."""
  E, nu, t = 3.0, 0.3, 0.7
  lam, mu = operators.lame_parameters(E, nu)
  rp = ER.jittered_box(2, ndim, 4)
  mesh = rp.finalize(device=DEV)
  x = np.asarray(rp.node_coords, np.float64)
  bcs = {}
  for a, name in enumerate(['x0', 'y0', 'z0'][:ndim]):
    entries = [None] * ndim
    entries[a] = 0.0
    bcs[name] = (D, tuple(entries))
  bcs['x1'] = (N, (t,) + (None,) * (ndim - 1))
  u = solve_elasticity(mesh, (0.0,) * ndim, bcs, lame_lambda=lam, lame_mu=mu,
                       rtol=1e-13, preconditioner='jacobi')
  if ndim == 3:
    want = np.stack([t * x[:, 0] / E, -nu * t * x[:, 1] / E,
                     -nu * t * x[:, 2] / E], axis=-1)
  else:
    want = np.stack([(1 - nu ** 2) * t * x[:, 0] / E,
                     -nu * (1 + nu) * t * x[:, 1] / E], axis=-1)
  err = _rel(_np(u), want)
  print(f'uniaxial {ndim}D: rel err {err:.2e}')
  assert err <= 1e-9


def test_plane_stress_tension():
  """The 2D operator with the modified lambda solves plane stress:
  u = (t x / E, -nu t y / E)."""
  E, nu, t = 3.0, 0.3, 0.7
  lam, mu = operators.lame_parameters(E, nu, plane_stress=True)
  rp = ER.jittered_box(2, 2, 4)
  mesh = rp.finalize(device=DEV)
  x = np.asarray(rp.node_coords, np.float64)
  bcs = {'x0': (D, (0.0, None)), 'y0': (D, (None, 0.0)), 'x1': (N, (t, None))}
  u = solve_elasticity(mesh, (0.0, 0.0), bcs, lame_lambda=lam, lame_mu=mu,
                       rtol=1e-13)
  want = np.stack([t * x[:, 0] / E, -nu * t * x[:, 1] / E], axis=-1)
  assert _rel(_np(u), want) <= 1e-9


def test_manufactured_solution_converges():
  """u = (sin 2x cos y, cos x sin 3y) with constant lambda, mu, Dirichlet data
  on the whole boundary and the nodal body force -div sigma(u), on 2 x 2
  elements with a moved interior vertex: the maximum nodal error decreases
  strictly over the orders 3, 5, 7 and ends below 1e-6 (the dense reference
  gives 4.5e-4, 2.5e-6, 7.0e-9)."""
  lam, mu = 1.5, 0.8

  def exact(y):
    return np.stack([np.sin(2 * y[:, 0]) * np.cos(y[:, 1]),
                     np.cos(y[:, 0]) * np.sin(3 * y[:, 1])], axis=-1)

  def force(y):
    X, Y = y[:, 0], y[:, 1]
    f1 = (lam + mu) * (4 * np.sin(2 * X) * np.cos(Y) +
                       3 * np.sin(X) * np.cos(3 * Y)) + \
        5 * mu * np.sin(2 * X) * np.cos(Y)
    f2 = (lam + mu) * (2 * np.cos(2 * X) * np.sin(Y) +
                       9 * np.cos(X) * np.sin(3 * Y)) + \
        10 * mu * np.cos(X) * np.sin(3 * Y)
    return np.stack([f1, f2], axis=-1)
  errs = []
  for order in (3, 5, 7):
    rp = ER.jittered_box(2, 2, order + 1)
    mesh = rp.finalize(device=DEV)
    x = np.asarray(rp.node_coords, np.float64)
    comp = lambda c: _t(lambda y: exact(y)[:, c])
    bcs = {g: (D, (comp(0), comp(1))) for g in ('x0', 'x1', 'y0', 'y1')}
    u = solve_elasticity(mesh, _t(force), bcs, lame_lambda=lam, lame_mu=mu,
                         rtol=1e-12, preconditioner='jacobi')
    errs.append(np.abs(_np(u) - exact(x)).max())
  print(f'manufactured solution, orders 3, 5, 7: {errs}')
  assert errs[0] > errs[1] > errs[2] and errs[2] < 1e-6


@pytest.mark.parametrize('ndim', [2, 3])
def test_shifted_problem_without_dirichlet_nodes(ndim):
  """lambda0 rho > 0 and no fixed component: the implicit-dynamics operator,
  tractions and a body force against the dense solve."""
  P = 4
  rp = TR.box_with_sides(2, ndim, P, three_kinds=True)
  mesh = rp.finalize(device=DEV)
  x = np.asarray(rp.node_coords, np.float64)
  lam, mu, rho = _coef_fns(ndim)
  l0 = 3.0
  dense = ER.Dense(rp, P, lam, mu, rho, l0)
  force = np.stack([np.cos(x[:, 0]), x[:, 1], 0.5 + 0.0 * x[:, 0]][:ndim],
                   axis=-1)
  trac = [None] * ndim
  trac[ndim - 1] = lambda y: 0.5 + y[:, 0]
  want = dense.solve(force, np.zeros(x.shape, bool), np.zeros(x.shape),
                     [(_facets(mesh, 'y1'), trac)])
  bcs = {'y1': (N, tuple(None if g is None else _t(g) for g in trac))}
  for pc in (None, 'jacobi'):
    u, info = solve_elasticity(
        mesh, _dev(force), bcs, lame_lambda=_t(lam), lame_mu=_t(mu),
        density=_t(rho), lambda0=l0, rtol=1e-12, preconditioner=pc,
        return_info=True)
    assert info['status'] == 'converged'
    assert _rel(_np(u), want) <= 1e-8


# -------------------------------------------------------------- 5. Jacobi
def test_jacobi_same_solution_fewer_iterations():
  """mu jumps by 1e3 between elements (`reference.jacobi_case`, where the
  dense PCG needs 375 iterations without and 78 with the preconditioner):
  the same solution as the unpreconditioned solve and as the dense solve to
  the solver tolerance 1e-8, strictly fewer iterations."""
  rp, P, mu_e, force = ER.jacobi_case()
  mesh = rp.finalize(device=DEV)
  bcs = {'x0': (D, (0.0, 0.0))}
  mu = _dev(mu_e)
  out = {}
  for pc in (None, 'jacobi'):
    out[pc] = solve_elasticity(mesh, tuple(force), bcs, lame_lambda=2.0 * mu,
                               lame_mu=mu, rtol=1e-8, preconditioner=pc,
                               return_info=True)
    assert out[pc][1]['status'] == 'converged'
  (u0, i0), (u1, i1) = out[None], out['jacobi']
  print(f'iterations: {i0["num_iterations"]} plain, '
        f'{i1["num_iterations"]} Jacobi')
  assert i1['num_iterations'] < i0['num_iterations']
  x = np.asarray(rp.node_coords, np.float64)
  mu_q = lambda xq: np.broadcast_to(mu_e[:, None], xq.shape[:2])
  dense = ER.Dense(rp, P, lambda xq: 2.0 * mu_q(xq), mu_q)
  fixed = np.zeros(x.shape, bool)
  fixed[_on(x, 0, 0.0)] = True
  K, b, expand = dense.system(np.tile(force, (len(x), 1)), fixed, 0.0 * x)
  want = expand(np.linalg.solve(K, b))
  # the dense PCG of the reference at this rtol is within 6.8e-11 (plain) and
  # 8.5e-12 (Jacobi) of the direct solve: the solver tolerance itself bounds
  # all three comparisons with two orders of margin
  errs = [_rel(_np(u0), want), _rel(_np(u1), want), _rel(_np(u1), _np(u0))]
  print(f'plain vs dense {errs[0]:.2e}, Jacobi vs dense {errs[1]:.2e}, '
        f'Jacobi vs plain {errs[2]:.2e}')
  assert max(errs) <= 1e-8


# ----------------------------------------------------------- 6. refusals
def test_operator_refusals():
  case = G.affine(2, 2, MESH_P)
  mesh, _, rp = case.finalize(DEV, torch.float64)
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(3, GL))
  ok = dict(lame_lambda=1.0, lame_mu=1.0)
  E, nq = mesh.num_elements, 9
  for bad in (dict(lame_mu=0.0), dict(lame_mu=-1.0), dict(lame_lambda=-0.5),
              dict(density=-1.0), dict(lame_mu=float('nan')),
              dict(lame_mu=torch.zeros(E)),
              dict(lame_lambda=-torch.ones(E, nq)),
              dict(lame_mu=torch.ones(E + 1)),
              dict(density=lambda x: -torch.ones(x.shape[0], device=DEV)),
              dict(lame_mu='steel')):
    with pytest.raises(ValueError):
      fes.elasticity_operator(**{**ok, **bad})
  with pytest.raises(ValueError, match='dirichlet_mask'):
    fes.elasticity_operator(torch.zeros(mesh.num_nodes, 3, dtype=torch.bool),
                            **ok)
  with pytest.raises(ValueError, match='geometry'):
    fes.elasticity_operator(geometry='multilinear', **ok)
  op = fes.elasticity_operator(**ok)
  u = torch.zeros((mesh.num_nodes, 2), dtype=torch.float64, device=DEV)
  with pytest.raises(ValueError):
    op.apply(u[:, 0])
  with pytest.raises(ValueError):
    op.apply_local(torch.zeros((E, 9), dtype=torch.float64, device=DEV))
  with pytest.raises(NotImplementedError, match='autograd'):
    op.apply(u.clone().requires_grad_(True))
  with pytest.raises(NotImplementedError, match='ensemble'):
    FiniteElementSpace.create(mesh.replicate(2), Quadrature1D.create(
        3, GL)).elasticity_operator(**ok)
  from swirl_fem_amd.distributed import blocks
  part = blocks.build_block_partition(2, 3, (2, 1, 1), 0, device='cpu')
  with pytest.raises(NotImplementedError, match='partitioned'):
    FiniteElementSpace.create(part.mesh, Quadrature1D.create(
        4, GL)).elasticity_operator(**ok)
  # a density that is zero everywhere leaves the shifted problem singular
  bm = TR.box_with_sides(2, 2, MESH_P).finalize(device=DEV)
  for zero in (0.0, torch.zeros(bm.num_elements),
               lambda x: torch.zeros(x.shape[0], device=DEV)):
    with pytest.raises(ValueError, match='rigid-body'):
      solve_elasticity(bm, (0.0, 1.0), {}, lambda0=1.0, density=zero, **ok)
  with pytest.raises(ValueError, match='body_force'):
    solve_elasticity(bm, (0.0, 1.0, 2.0), {'x0': (D, (0.0, 0.0))}, **ok)


def _raw_args(op, fes, **over):
  """A valid `ElasticityArgs` for the first launch of `op`, with overrides;
  returns (args, what must stay alive)."""
  mesh = fes.mesh
  d, Q = mesh.ndim, fes.quadrature.num_points
  E, nq = mesh.num_elements, Q ** d
  keep = dict(
      u=torch.zeros((E, nq, d), dtype=torch.float64, device=DEV),
      out=torch.zeros((E, nq, d), dtype=torch.float64, device=DEV),
      host={k: np.ascontiguousarray(v, np.float64)
            for k, v in op.host.items()})
  part = op.parts[0]
  args = _lib.ElasticityArgs(
      u=keep['u'].data_ptr(), out=keep['out'].data_ptr(),
      wdet=op.point_weights().data_ptr(), lam_const=1.0, mu_const=1.0,
      rho_const=1.0, geo_elem=part['geo_elem'].data_ptr(),
      dmat=keep['host']['dmat'].ctypes.data,
      weights=keep['host']['weights'].ctypes.data,
      nodes=keep['host']['nodes'].ctypes.data, num_elements=E, ndim=d, P=Q,
      dtype=_lib.SFEM_F64, geo_mode=part['geo_mode'])
  for k, v in over.items():
    setattr(args, k, v)
  return args, keep


def test_entry_point_refusals():
  """Status codes of the raw entry point; nothing that is refused launches."""
  case = G.affine(2, 3, MESH_P)
  mesh, _, rp = case.finalize(DEV, torch.float64)
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(4, GL))
  op = fes.elasticity_operator(lame_lambda=1.0, lame_mu=1.0)
  call = lambda a: _lib.load().sfem_elasticity_local(ctypes.byref(a), None)
  ok, keep = _raw_args(op, fes)
  assert call(ok) == 0
  torch.cuda.synchronize()
  # outside the compiled range: SFEM_EUNSUPPORTED
  for over in (dict(P=13), dict(P=1), dict(ndim=1), dict(ndim=4),
               dict(geo_mode=_lib.GEO_BOX), dict(geo_mode=7)):
    a, keep = _raw_args(op, fes, **over)
    assert call(a) == -3, over
  # a missing required pointer: SFEM_EINVAL
  for over in (dict(u=None), dict(out=None), dict(dmat=None), dict(wdet=None),
               dict(geo_elem=None), dict(weights=None), dict(nodes=None),
               dict(geo_mode=_lib.GEO_POINT), dict(dtype=5),
               dict(num_elements=-1),
               dict(elem_list=keep['u'].data_ptr(), num_listed=10 ** 6)):
    a, keep = _raw_args(op, fes, **over)
    assert call(a) == -1, over
  assert _lib.load().sfem_elasticity_local(None, None) == -1
  # nothing to do is not an error
  a, keep = _raw_args(op, fes, num_elements=0, u=None, out=None)
  assert call(a) == 0
