"""Neo-Hookean elasticity on the GPU: the kernel
`sfem_hyperelastic_local`, residual and tangent modes, at every Q = 2..12
against the NumPy reference (`tests/hyperelastic_reference.py`); the assembled
operator (masks, layouts, symmetry, the derivative relations, the linear
operator at u = 0 and for small strains, objectivity, an inverted state);
`solve_hyperelasticity` against exact homogeneous stretches and the dense
Newton of the reference, the preconditioners on a bent cantilever, and the
refusals.

Random fields are scaled so that the largest Frobenius norm of the
displacement gradient H over all points, computed by the reference, is 0.3:
then J >= 0.7^d > 0.3 everywhere, which each test asserts from the reference
before it looks at the kernel."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from swirl_fem_amd import _lib, _ops
from swirl_fem_amd.core import layout
from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import NodeType, Quadrature1D
from swirl_fem_amd.examples.elasticity import solve_elasticity
from swirl_fem_amd.examples.hyperelasticity import BCType
from swirl_fem_amd.examples.hyperelasticity import solve_hyperelasticity
from swirl_fem_amd.linalg.pmg_elasticity import ElasticityPMultigrid
from tests import elasticity_reference as ER
from tests import geometry_cases as G
from tests import hyperelastic_reference as HR
from tests import transport_reference as TR
from tests.fp32util import F32Rng, f32r, tolerance

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GL = NodeType.GAUSS_LEGENDRE
D, N = BCType.DIRICHLET, BCType.NEUMANN
MESH_P = 3       # nodes per direction of the kernel tests' meshes
SCALE = 0.3      # the largest |H| of a random field
MIN_J = 0.3

# (lambda, mu, rho: 'p' per point around the number, or the scalar; lambda0):
# the combinations of the linear kernel's test
KERNEL_COMBOS = [
    (1.3, 0.7, None, 0.0),
    (('p', 1.0), ('p', 0.8), ('p', 1.5), 2.5),
    (('p', 0.9), 0.6, ('p', 2.0), 0.0),
    (0.0, ('p', 0.8), 1.5, 0.7),
    (50.0, 1.0, None, 0.0),
    (('p', 50.0), ('p', 1.0), None, 1.1),
]


def _dev(a, dtype=torch.float64):
  return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _np(t):
  return t.detach().double().cpu().numpy()


def _rel(a, b):
  return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _t(fn):
  """A NumPy callable on points as a torch callable."""
  return lambda x: _dev(fn(_np(x)))


# ------------------------------------------------ 1. kernel vs reference
def _kernel_setup(case, Q, dtype=torch.float64):
  mesh, _, rp = case.finalize(DEV, dtype)
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(Q, GL))
  ref = HR.space(rp.node_coords, rp.elements, MESH_P, (Q, 'gl'))
  op = fes.hyperelastic_operator(lame_lambda=1.0, lame_mu=1.0)
  return mesh, fes, ref, op


def _scaled_grid_field(ref, rng, ndim, rnd):
  """A random field on the grid with max |H| = SCALE; min J asserted."""
  uq = rng.standard_normal((ref.num_elements, ref.Q, ndim))
  uq = rnd(uq * (SCALE / HR.max_gradient_norm(ref, uq)))
  assert HR.max_gradient_norm(ref, uq) <= SCALE * (1 + 1e-6)
  assert HR.min_jacobian(ref, uq) >= MIN_J
  return uq


def _check(name, got, want, tol, dtype, ref32, rows):
  """`got` against the fp64 reference `want` at `tol`; above it in fp32 the
  project's exception rule: 4 times the error of the NumPy reference
  evaluated in float32 (`ref32`, a thunk)."""
  err = _rel(got, want)
  allowed = tol
  if err > tol and dtype == torch.float32:
    allowed = max(tol, 4.0 * _rel(ref32().astype(np.float64), want))
  print(f'  {name}: rel err {err:.3e} (allowed {allowed:.3e})')
  rows.append((name, err, allowed))
  assert err <= allowed, (name, err, allowed)


def _run_combos(op, ref, ndim, Q, pad, rng, dtype, tol, combos, rnd=lambda a: a):
  """Each combination, both modes, against `grid_residual` / `grid_tangent`:
  residual, psi and state in residual mode; the tangent with the state of the
  reference (a wrong state cannot cancel a wrong tangent) and with the state
  of the kernel.  The `pad` trailing rows carry zero displacement."""
  E, nq = ref.num_elements, ref.Q
  d2 = ndim * ndim
  rows = []
  for n, (lam, mu, rho, l0) in enumerate(combos):
    def coef(c):
      if isinstance(c, tuple):
        return rnd(c[1] * (1.0 + 0.2 * rng.uniform(-1, 1, (E, nq))))
      return c
    lam, mu, rho = coef(lam), coef(mu), coef(rho)
    uq = _scaled_grid_field(ref, rng, ndim, rnd)
    wq = rnd(rng.standard_normal((E, nq, ndim)))
    want_r, want_s, want_p = HR.grid_residual(ref, uq, lam, mu, rho, l0)
    want_t = HR.grid_tangent(ref, wq, want_s, lam, mu, rho, l0)
    f32 = lambda: HR.grid_residual(ref, uq, lam, mu, rho, l0,
                                   dtype=np.float32)

    def dev(c):
      if isinstance(c, np.ndarray):
        return _dev(np.concatenate([c, np.ones((pad, nq))]), dtype)
      return c

    def padded(a):
      return _dev(np.concatenate([a, np.zeros((pad,) + a.shape[1:])]), dtype)
    args = (op.parts, op.host, ndim, Q, op.point_weights(), dev(lam), dev(mu),
            dev(rho), l0)
    print(f'{dtype} ndim={ndim} Q={Q} combo {n}:')
    got_r, got_s, got_p = _ops.hyperelastic_local(
        padded(uq), *args, mode='residual', want_state=True, want_psi=True)
    assert got_r.shape == (E + pad, nq, ndim) and got_r.dtype == dtype
    assert got_s.shape == (E + pad, nq, d2 + 1) and got_p.shape == (E + pad, nq)
    for t in (got_r, got_s, got_p):       # the padded row holds finite values
      assert bool(torch.isfinite(t).all())
    _check('residual', _np(got_r)[:E], want_r, tol, dtype,
           lambda: f32()[0], rows)
    _check('state', _np(got_s)[:E], want_s, tol, dtype, lambda: f32()[1], rows)
    _check('psi', _np(got_p)[:E], want_p, tol, dtype, lambda: f32()[2], rows)
    # without the optional outputs the residual is the same
    only_r, none_s, none_p = _ops.hyperelastic_local(
        padded(uq), *args, mode='residual')
    assert none_s is None and none_p is None
    assert torch.equal(only_r[:E], got_r[:E])
    t32 = lambda: HR.grid_tangent(ref, wq, want_s, lam, mu, rho, l0,
                                  dtype=np.float32)
    got_t = _ops.hyperelastic_local(padded(wq), *args, mode='tangent',
                                    state=padded(want_s))
    assert got_t.shape == (E + pad, nq, ndim) and got_t.dtype == dtype
    _check('tangent, reference state', _np(got_t)[:E], want_t, tol, dtype,
           t32, rows)
    got_t = _ops.hyperelastic_local(padded(wq), *args, mode='tangent',
                                    state=got_s)
    _check('tangent, kernel state', _np(got_t)[:E], want_t, tol, dtype, t32,
           rows)
  return rows


@pytest.mark.parametrize('Q', range(2, 13))
@pytest.mark.parametrize('ndim', [2, 3])
def test_kernel_matches_reference(ndim, Q):
  """fp64, every Q, both modes: scalar and per-point coefficients, rho with
  and without a mass term, lambda = 0, lambda / mu = 50, on multilinear and
  curved elements with a padded row (list launches, a partial workgroup)."""
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
  """The affine instantiations at every Q, both modes (one launch over all
  elements, no list)."""
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
  reference at `tolerance(torch.float32, Q)`, every combination, both modes.
  A case above that is held to 4 times the error of the NumPy reference
  evaluated in float32 (DESIGN §3.20 lists them)."""
  case = G.three_kinds(2, ndim, MESH_P)
  mesh, fes, ref, op = _kernel_setup(case, Q, torch.float32)
  rng = F32Rng(Q)
  rows = _run_combos(op, ref, ndim, Q, 0, rng, torch.float32,
                     tolerance(torch.float32, Q), KERNEL_COMBOS, rnd=f32r)
  for name, err, allowed in rows:
    if err > tolerance(torch.float32, Q):
      print(f'EXCEPTION ndim={ndim} Q={Q} {name}: {err:.3e} <= {allowed:.3e}')


# ------------------------------------------------ 2. assembled operator
def _coef_fns(ndim):
  lam = lambda x: 1.0 + 0.5 * np.sin(2.0 * x[..., 0]) * x[..., 1]
  mu = lambda x: 0.7 + 0.3 * x[..., ndim - 1] ** 2
  rho = lambda x: 1.5 + np.cos(x[..., 0])
  return lam, mu, rho


@functools.lru_cache(maxsize=None)
def _assembled(ndim):
  """A mesh with all three geometry kinds, the space of a solve on it, the
  reference space and variable coefficients (callables, values)."""
  P = 4 if ndim == 2 else 3
  case = G.three_kinds(3, ndim, P)
  mesh, _, rp = case.finalize(DEV, torch.float64)
  q = P - 1 + (ndim + 1) // 2
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(q, GL))
  ref = HR.space(rp.node_coords, rp.elements, P, (q, 'gl'))
  fns = _coef_fns(ndim)
  xq = HR.quad_points(ref)
  return mesh, fes, ref, rp, fns, tuple(f(xq) for f in fns)


def _operator(ndim, fixed=None):
  mesh, fes, ref, rp, fns, vals = _assembled(ndim)
  op = fes.hyperelastic_operator(
      None if fixed is None else _dev(fixed, torch.bool),
      lame_lambda=_t(fns[0]), lame_mu=_t(fns[1]), density=_t(fns[2]))
  assert {p['geo_mode'] for p in op.parts} == {G.CURVED, G.MULTILINEAR,
                                              G.AFFINE}
  return op


def _nodal_field(ref, rng):
  """A random nodal field with max |H| = SCALE at the quadrature points."""
  u = rng.standard_normal((ref.num_nodes, ref.ndim))
  H = HR.gradients(ref, ref.gather(u))
  u *= SCALE / np.sqrt((H * H).sum((-2, -1))).max()
  H = HR.gradients(ref, ref.gather(u))
  assert np.linalg.det(H + np.eye(ref.ndim)).min() >= MIN_J
  return u


@pytest.mark.parametrize('ndim', [2, 3])
def test_operator_matches_reference(ndim):
  """`residual`, `energy`, `linearize` and `tangent.apply` against the
  reference: a per-component mask, dense and component-major layouts,
  callable coefficients, with and without the mass term."""
  mesh, fes, ref, rp, fns, vals = _assembled(ndim)
  rng = np.random.default_rng(ndim)
  fixed = rng.uniform(size=(mesh.num_nodes, ndim)) < 0.25
  keep = (~fixed).astype(float)
  op = _operator(ndim, fixed)
  u = _nodal_field(ref, rng)
  w = rng.standard_normal(u.shape)
  for l0 in (0.0, 1.7):
    want = HR.residual(ref, u, *vals, l0, keep=keep)
    dense = op.residual(_dev(u), l0)
    assert dense.is_contiguous()
    assert _rel(_np(dense), want) <= 1e-10
    cm = layout.component_major(_dev(u))
    assert not cm.is_contiguous()
    got = op.residual(cm, l0)
    assert layout.is_component_major(got) and got.stride() == cm.stride()
    assert _rel(_np(got), want) <= 1e-10
    e = op.energy(_dev(u), l0)
    assert isinstance(e, float)
    assert abs(e - HR.energy(ref, u, *vals, l0)) <= 1e-10 * abs(e)
    lin = op.linearize(_dev(u), l0)
    assert _rel(_np(lin.residual), want) <= 1e-10
    d = ndim
    assert tuple(lin.state.shape) == (mesh.num_elements, ref.Q, d * d + 1)
    want_s = HR.state(HR.gradients(ref, ref.gather(u)))
    assert _rel(_np(lin.state), want_s) <= 1e-10
    T = op.tangent(lin, l0)
    want = HR.tangent(ref, u, w, *vals, l0, keep=keep)
    assert _rel(_np(T.apply(_dev(w))), want) <= 1e-10
    got = T.apply(layout.component_major(_dev(w)))
    assert layout.is_component_major(got)
    assert _rel(_np(got), want) <= 1e-10
    assert _rel(_np(T.linear_operator()(_dev(w))), want) <= 1e-10
    assert _rel(_np(op.tangent(lin.state, l0).apply(_dev(w))), want) <= 1e-10
  # (N,) mask: every component of the node; scalar coefficients
  nodes = rng.uniform(size=mesh.num_nodes) < 0.3
  op1 = fes.hyperelastic_operator(_dev(nodes, torch.bool), lame_lambda=2.0,
                                  lame_mu=0.5)
  keep = np.repeat((~nodes)[:, None], ndim, axis=1).astype(float)
  want = HR.residual(ref, u, 2.0, 0.5, keep=keep)
  assert _rel(_np(op1.residual(_dev(u))), want) <= 1e-10


@pytest.mark.parametrize('ndim', [2, 3])
def test_tangent_symmetry_and_derivative(ndim):
  """|v . T w - w . T v| <= 1e-12 |v| |T w|; T w against the central
  difference of the residual on the device (h = 1e-5, 1e-6 relative:
  truncation h^2 times an O(10) constant, rounding 1e-16 / h)."""
  mesh, fes, ref, rp, fns, vals = _assembled(ndim)
  op = _operator(ndim)
  rng = np.random.default_rng(3)
  u = _dev(_nodal_field(ref, rng))
  v = _dev(rng.standard_normal((mesh.num_nodes, ndim)))
  w = _dev(rng.standard_normal((mesh.num_nodes, ndim)))
  h = 1e-5
  for l0 in (0.0, 0.9):
    T = op.tangent(op.linearize(u, l0), l0)
    Tw, Tv = T.apply(w), T.apply(v)
    a, b = float((v * Tw).sum()), float((w * Tv).sum())
    scale = float(v.norm() * Tw.norm())
    print(f'{ndim}D lambda0={l0}: |vTw - wTv| / (|v||Tw|) = '
          f'{abs(a - b) / scale:.2e}')
    assert abs(a - b) <= 1e-12 * scale
    fd = (op.residual(u + h * w, l0) - op.residual(u - h * w, l0)) / (2 * h)
    err = _rel(_np(fd), _np(Tw))
    print(f'{ndim}D lambda0={l0}: central difference vs tangent {err:.2e}')
    assert err <= 1e-6


@pytest.mark.parametrize('ndim', [2, 3])
def test_small_strain_limit(ndim):
  """The tangent at u = 0 equals `ElasticityOperator.apply` to 1e-12, and
  R(eps u) / eps is within 100 eps (relative) of K u for eps = 1e-6: the
  difference is O(eps) with a coefficient of 3 to 8 times |H|."""
  mesh, fes, ref, rp, fns, vals = _assembled(ndim)
  rng = np.random.default_rng(5)
  fixed = rng.uniform(size=(mesh.num_nodes, ndim)) < 0.2
  op = _operator(ndim, fixed)
  zero = torch.zeros((mesh.num_nodes, ndim), dtype=torch.float64, device=DEV)
  w = _dev(rng.standard_normal((mesh.num_nodes, ndim)))
  u = _dev(_nodal_field(ref, rng))
  eps = 1e-6
  for l0 in (0.0, 1.3):
    lin = op.linearize(zero, l0)
    assert float(lin.residual.abs().max()) == 0.0
    got = op.tangent(lin, l0).apply(w)
    want = op.linear.apply(w, l0)
    assert _rel(_np(got), _np(want)) <= 1e-12
    Ku = op.linear.apply(u, l0)
    err = _rel(_np(op.residual(eps * u, l0)) / eps, _np(Ku))
    print(f'{ndim}D lambda0={l0}: |R(eps u)/eps - K u| / |K u| = {err:.2e}')
    assert err <= 100 * eps
  assert op.energy(zero) == 0.0


@pytest.mark.parametrize('ndim', [2, 3])
def test_objectivity(ndim):
  """u = (Rot - I) x, a rotation by 30 degrees: residual and energy vanish to
  1e-11, where the linear K u is of order one."""
  mesh, fes, ref, rp, fns, vals = _assembled(ndim)
  op = _operator(ndim)
  x = np.asarray(rp.node_coords, np.float64)
  c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
  Rot = np.eye(ndim)
  Rot[:2, :2] = [[c, -s], [s, c]]
  u = _dev(x @ (Rot - np.eye(ndim)).T)
  R = float(op.residual(u).abs().max())
  e = op.energy(u)
  Ku = float(op.linear.apply(u).abs().max())
  print(f'{ndim}D rotation: |R| {R:.2e}, energy {e:.2e}, |K u| {Ku:.2e}')
  assert R <= 1e-11 and abs(e) <= 1e-11
  assert Ku >= 1e-2


@pytest.mark.parametrize('ndim', [2, 3])
def test_inverted_state_is_not_sticky(ndim):
  """u_x = -1.5 x gives F_11 = -0.5, J < 0: the energy and the residual are
  non-finite (an arithmetic NaN, no exception), and a following call with a
  valid field is correct."""
  mesh, fes, ref, rp, fns, vals = _assembled(ndim)
  op = _operator(ndim)
  x = np.asarray(rp.node_coords, np.float64)
  bad = np.zeros_like(x)
  bad[:, 0] = -1.5 * x[:, 0]
  e = op.energy(_dev(bad))
  assert isinstance(e, float) and not np.isfinite(e)
  assert not bool(torch.isfinite(op.residual(_dev(bad))).all())
  lin = op.linearize(_dev(bad))
  assert not bool(torch.isfinite(lin.residual).all())
  torch.cuda.synchronize()
  u = _nodal_field(ref, np.random.default_rng(9))
  assert _rel(_np(op.residual(_dev(u))), HR.residual(ref, u, *vals)) <= 1e-10
  e = op.energy(_dev(u))
  assert abs(e - HR.energy(ref, u, *vals)) <= 1e-10 * abs(e)


# -------------------------------------------------------------- 3. solves
def _facets(mesh, group):
  return mesh.boundary_facets[group].cpu().numpy().astype(np.int64)


def _on(x, axis, value):
  return np.abs(x[:, axis] - value) < 1e-9


@pytest.mark.parametrize('drive', ['dirichlet', 'dead_load'])
@pytest.mark.parametrize('ndim', [2, 3])
def test_homogeneous_stretch(ndim, drive):
  """Stretch a = 1.5 with rollers on the coordinate planes through the
  origin, driven by the end displacement or by the dead load P_11 = mu (a -
  1/a) + lam ln J / a on x1, on a mesh with a moved interior vertex: the
  solution ((a - 1) x, (b - 1) y, ..) is linear, so exact at every order.
  load_steps = 4, newton_rtol = 1e-10; nodal error at most 1e-8."""
  a, lam, mu = 1.5, 1.3, 0.7
  b = HR.uniaxial_lateral_stretch(a, lam, mu, ndim)
  rp = ER.jittered_box(2, ndim, 3)
  mesh = rp.finalize(device=DEV)
  x = np.asarray(rp.node_coords, np.float64)
  bcs = {}
  for ax, name in enumerate(['x0', 'y0', 'z0'][:ndim]):
    entries = [None] * ndim
    entries[ax] = 0.0
    bcs[name] = (D, tuple(entries))
  if drive == 'dirichlet':
    bcs['x1'] = (D, (a - 1.0,) + (None,) * (ndim - 1))
  else:
    bcs['x1'] = (N, (HR.uniaxial_traction(a, lam, mu, ndim),) +
                 (None,) * (ndim - 1))
  u, info = solve_hyperelasticity(
      mesh, (0.0,) * ndim, bcs, lame_lambda=lam, lame_mu=mu, load_steps=4,
      newton_rtol=1e-10, linear_rtol=1e-8, preconditioner='jacobi',
      return_info=True)
  want = np.stack([(a - 1.0) * x[:, 0]] +
                  [(b - 1.0) * x[:, c] for c in range(1, ndim)], axis=-1)
  err = np.abs(_np(u) - want).max()
  its = [len(s['step_lengths']) for s in info['load_steps']]
  print(f'{ndim}D {drive}: Newton iterations {its}, error {err:.2e}')
  assert info['status'] == 'converged' and len(info['load_steps']) == 4
  assert err <= 1e-8


@pytest.mark.parametrize('ndim,order', [(2, 2), (2, 3), (3, 2), (3, 3)])
def test_solve_matches_dense_newton(ndim, order):
  """2 x 2 (x 2) elements of mixed geometry, variable coefficients, a body
  force, a clamp on x0 and a dead load on x1, two load steps: against the
  dense Newton of the reference to 1e-8, and with linear_rtol = 1e-12 at most
  one Newton iteration more per load step than the reference needs."""
  P = order + 1
  rp = TR.box_with_sides(2, ndim, P, three_kinds=True)
  mesh = rp.finalize(device=DEV)
  x = np.asarray(rp.node_coords, np.float64)
  lam, mu, _ = _coef_fns(ndim)
  dense = HR.DenseNewton(rp, P, lam, mu)
  force = lambda y: 0.5 * np.stack(
      [0.3 * np.sin(2.0 * y[:, 0]), -0.4 + 0.0 * y[:, 0],
       0.2 * y[:, 0] * y[:, 1]][:ndim], axis=-1)
  trac = [0.125, -0.075, 0.05][:ndim]
  fixed = np.zeros(x.shape, bool)
  fixed[_on(x, 0, 0.0)] = True
  want, counts = dense.solve(force(x), fixed, np.zeros(x.shape),
                             [(_facets(mesh, 'x1'), trac)], load_steps=2,
                             rtol=1e-10)
  bcs = {'x0': (D, (0.0,) * ndim), 'x1': (N, tuple(trac))}
  u, info = solve_hyperelasticity(
      mesh, _t(force), bcs, lame_lambda=_t(lam), lame_mu=_t(mu), load_steps=2,
      newton_rtol=1e-10, linear_rtol=1e-12, preconditioner='jacobi',
      return_info=True)
  its = [len(s['step_lengths']) for s in info['load_steps']]
  err = _rel(_np(u), want)
  print(f'{ndim}D order {order}: Newton iterations {its} (reference '
        f'{counts}), rel err {err:.2e}')
  assert err <= 1e-8
  assert all(i <= c + 1 for i, c in zip(its, counts))
  assert not _np(u)[fixed].any()


@functools.lru_cache(maxsize=None)
def _cantilever():
  """8 x 2 elements of order 4, length 1 and height 1/4, clamped on x0, with
  the dead load 0.016 per unit reference area in y on x1: the dense Newton of
  the reference gives a tip deflection of 0.33 and a tip shortening of 0.06."""
  rp = HR.beam(8, 2, 5)
  mesh = rp.finalize(device=DEV)
  x = np.asarray(rp.node_coords, np.float64)
  tip = int(np.where(_on(x, 0, 1.0) & _on(x, 1, 0.125))[0][0])
  bcs = {'x0': (D, (0.0, 0.0)), 'x1': (N, (None, 0.016))}
  return mesh, tip, bcs, dict(lame_lambda=1.5, lame_mu=1.0)


def test_cantilever_preconditioners():
  """The bent cantilever with load_steps = 3: None, 'jacobi' and
  `ElasticityPMultigrid` agree to 1e-7; p-multigrid needs fewer CG iterations
  in total than Jacobi; the tip deflects by about a third of the length and
  moves inward in x, which the linear solve does not show."""
  mesh, tip, bcs, kw = _cantilever()
  out = {}
  for pc in (None, 'jacobi', ElasticityPMultigrid):
    u, info = solve_hyperelasticity(
        mesh, (0.0, 0.0), bcs, load_steps=3, newton_rtol=1e-10,
        linear_rtol=1e-8, max_newton=40, preconditioner=pc, return_info=True,
        **kw)
    assert info['status'] == 'converged'
    assert [s['status'] for s in info['load_steps']] == ['converged'] * 3
    out[pc] = (_np(u), info)
    print(f'{getattr(pc, "__name__", pc)}: Newton '
          f'{[len(s["step_lengths"]) for s in info["load_steps"]]}, CG '
          f'iterations {info["num_cg"]}, tip {_np(u)[tip]}')
  u0 = out[None][0]
  scale = np.abs(u0).max()
  assert np.abs(out['jacobi'][0] - u0).max() <= 1e-7 * scale
  assert np.abs(out[ElasticityPMultigrid][0] - u0).max() <= 1e-7 * scale
  assert out[ElasticityPMultigrid][1]['num_cg'] < out['jacobi'][1]['num_cg']
  lin = _np(solve_elasticity(mesh, (0.0, 0.0), bcs, rtol=1e-10,
                             preconditioner='jacobi', **kw))
  print(f'tip: nonlinear {u0[tip]}, linear {lin[tip]}')
  assert 0.25 <= u0[tip, 1] <= 0.4
  assert u0[tip, 0] <= -0.03
  assert abs(lin[tip, 0]) <= 1e-6


def test_max_newton_names_the_load_step():
  mesh, tip, bcs, kw = _cantilever()
  with pytest.raises(RuntimeError, match='load step 1 of 3'):
    solve_hyperelasticity(mesh, (0.0, 0.0), bcs, load_steps=3, max_newton=1,
                          preconditioner='jacobi', **kw)


@pytest.mark.parametrize('ndim', [2, 3])
def test_shifted_problem_without_fixed_components(ndim):
  """lambda0 rho > 0 and no fixed component converges, to the dense Newton
  of the reference."""
  P = 3
  rp = TR.box_with_sides(2, ndim, P, three_kinds=True)
  mesh = rp.finalize(device=DEV)
  x = np.asarray(rp.node_coords, np.float64)
  lam, mu, rho = _coef_fns(ndim)
  l0 = 3.0
  dense = HR.DenseNewton(rp, P, lam, mu, rho, l0)
  force = 0.3 * np.stack([np.cos(x[:, 0]), x[:, 1], 0.5 + 0.0 * x[:, 0]][:ndim],
                         axis=-1)
  trac = [None] * ndim
  trac[ndim - 1] = 0.2
  want, counts = dense.solve(force, np.zeros(x.shape, bool), np.zeros(x.shape),
                             [(_facets(mesh, 'y1'), trac)], rtol=1e-10)
  u, info = solve_hyperelasticity(
      mesh, _dev(force), {'y1': (N, tuple(trac))}, lame_lambda=_t(lam),
      lame_mu=_t(mu), density=_t(rho), lambda0=l0, newton_rtol=1e-10,
      linear_rtol=1e-10, return_info=True)
  assert info['status'] == 'converged'
  assert _rel(_np(u), want) <= 1e-8


# ----------------------------------------------------------- 4. refusals
def test_operator_refusals():
  case = G.affine(2, 2, MESH_P)
  mesh, _, rp = case.finalize(DEV, torch.float64)
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(3, GL))
  ok = dict(lame_lambda=1.0, lame_mu=1.0)
  E = mesh.num_elements
  for bad in (dict(lame_mu=0.0), dict(lame_lambda=-0.5), dict(density=-1.0),
              dict(lame_mu=torch.ones(E + 1)), dict(lame_mu='rubber')):
    with pytest.raises(ValueError):
      fes.hyperelastic_operator(**{**ok, **bad})
  with pytest.raises(ValueError, match='dirichlet_mask'):
    fes.hyperelastic_operator(
        torch.zeros(mesh.num_nodes, 3, dtype=torch.bool), **ok)
  with pytest.raises(ValueError, match='geometry'):
    fes.hyperelastic_operator(geometry='multilinear', **ok)
  op = fes.hyperelastic_operator(**ok)
  u = torch.zeros((mesh.num_nodes, 2), dtype=torch.float64, device=DEV)
  with pytest.raises(ValueError):
    op.residual(u[:, 0])
  with pytest.raises(ValueError):
    op.residual_local(torch.zeros((E, 9), dtype=torch.float64, device=DEV))
  grad_u = u.clone().requires_grad_(True)
  for call in (op.residual, op.energy, op.linearize):
    with pytest.raises(NotImplementedError, match='autograd'):
      call(grad_u)
  with pytest.raises(NotImplementedError, match='autograd'):
    op.tangent(op.linearize(u)).apply(grad_u)
  with pytest.raises(NotImplementedError, match='ensemble'):
    FiniteElementSpace.create(mesh.replicate(2), Quadrature1D.create(
        3, GL)).hyperelastic_operator(**ok)
  from swirl_fem_amd.distributed import blocks
  part = blocks.build_block_partition(2, 3, (2, 1, 1), 0, device='cpu')
  with pytest.raises(NotImplementedError, match='partitioned'):
    FiniteElementSpace.create(part.mesh, Quadrature1D.create(
        4, GL)).hyperelastic_operator(**ok)
  # the launcher: a tangent without a state, outputs asked of the tangent
  uq = torch.zeros((E, 9, 2), dtype=torch.float64, device=DEV)
  args = (uq, op.parts, op.host, 2, 3, op.point_weights(), 1.0, 1.0)
  with pytest.raises(ValueError, match='state'):
    _ops.hyperelastic_local(*args, mode='tangent')
  with pytest.raises(ValueError, match='residual mode'):
    _ops.hyperelastic_local(*args, mode='tangent', want_psi=True,
                            state=torch.zeros((E, 9, 5), dtype=torch.float64,
                                              device=DEV))
  with pytest.raises(ValueError, match='mode'):
    _ops.hyperelastic_local(*args, mode='stress')
  bm = TR.box_with_sides(2, 2, MESH_P).finalize(device=DEV)
  with pytest.raises(ValueError, match='rigid-body'):
    solve_hyperelasticity(bm, (0.0, 1.0), {}, lambda0=1.0, density=0.0, **ok)
  with pytest.raises(ValueError, match='body_force'):
    solve_hyperelasticity(bm, (0.0, 1.0, 2.0), {'x0': (D, (0.0, 0.0))}, **ok)


def _raw_args(op, fes, **over):
  """A valid residual-mode `HyperelasticArgs` for the first launch of `op`,
  with overrides; returns (args, what must stay alive)."""
  mesh = fes.mesh
  d, Q = mesh.ndim, fes.quadrature.num_points
  E, nq = mesh.num_elements, Q ** d
  zeros = lambda *s: torch.zeros(s, dtype=torch.float64, device=DEV)
  keep = dict(
      u=zeros(E, nq, d), out=zeros(E, nq, d), state=zeros(E, nq, d * d + 1),
      psi=zeros(E, nq),
      host={k: np.ascontiguousarray(v, np.float64)
            for k, v in op.host.items()})
  part = op.parts[0]
  args = _lib.HyperelasticArgs(
      u=keep['u'].data_ptr(), out=keep['out'].data_ptr(),
      wdet=op.point_weights().data_ptr(), lam_const=1.0, mu_const=1.0,
      rho_const=1.0, geo_elem=part['geo_elem'].data_ptr(),
      dmat=keep['host']['dmat'].ctypes.data,
      weights=keep['host']['weights'].ctypes.data,
      nodes=keep['host']['nodes'].ctypes.data, num_elements=E, ndim=d, P=Q,
      dtype=_lib.SFEM_F64, geo_mode=part['geo_mode'],
      state=keep['state'].data_ptr(), psi=keep['psi'].data_ptr(),
      mode=_lib.SFEM_HYPER_RESIDUAL)
  for k, v in over.items():
    setattr(args, k, v)
  return args, keep


def test_entry_point_refusals():
  """Status codes of the raw entry point; nothing that is refused launches."""
  case = G.affine(2, 3, MESH_P)
  mesh, _, rp = case.finalize(DEV, torch.float64)
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(4, GL))
  op = fes.hyperelastic_operator(lame_lambda=1.0, lame_mu=1.0)
  call = lambda a: _lib.load().sfem_hyperelastic_local(ctypes.byref(a), None)
  TANGENT = _lib.SFEM_HYPER_TANGENT
  ok, keep = _raw_args(op, fes)
  assert call(ok) == 0
  torch.cuda.synchronize()
  # zero displacement: F = I, so the state is (I, 0) and psi is zero
  st = _np(keep['state'])
  assert np.array_equal(st[0, 0], np.append(np.eye(3).reshape(-1), 0.0))
  assert not _np(keep['psi']).any() and not _np(keep['out']).any()
  ok, keep = _raw_args(op, fes, state=None, psi=None)
  assert call(ok) == 0
  ok, keep = _raw_args(op, fes, mode=TANGENT, psi=None)
  assert call(ok) == 0
  torch.cuda.synchronize()
  # outside the compiled range: SFEM_EUNSUPPORTED
  for over in (dict(P=13), dict(P=1), dict(ndim=1), dict(ndim=4),
               dict(geo_mode=_lib.GEO_BOX), dict(geo_mode=7), dict(mode=2),
               dict(mode=-1), dict(P=13, mode=TANGENT, psi=None),
               dict(ndim=4, mode=TANGENT, psi=None)):
    a, keep = _raw_args(op, fes, **over)
    assert call(a) == -3, over
  # a missing required pointer, the tangent without a state or with psi:
  # SFEM_EINVAL
  for over in (dict(u=None), dict(out=None), dict(dmat=None), dict(wdet=None),
               dict(geo_elem=None), dict(weights=None), dict(nodes=None),
               dict(geo_mode=_lib.GEO_POINT), dict(dtype=5),
               dict(num_elements=-1),
               dict(mode=TANGENT, state=None, psi=None),
               dict(mode=TANGENT),
               dict(elem_list=keep['u'].data_ptr(), num_listed=10 ** 6)):
    a, keep = _raw_args(op, fes, **over)
    assert call(a) == -1, over
  assert _lib.load().sfem_hyperelastic_local(None, None) == -1
  # nothing to do is not an error
  a, keep = _raw_args(op, fes, num_elements=0, u=None, out=None)
  assert call(a) == 0
