"""Gradients of neo-Hookean solves on the GPU: the kernel
`sfem_hyperelastic_sens` at every Q = 2..12 against the NumPy reference
(`tests/hyperelastic_adjoint_reference.py`), against the residual kernel
(linearity in the coefficients), `HyperelasticOperator.sensitivity` in every
coefficient form, `.grad` through `solve_hyperelasticity(...,
differentiable=True)` against the dense adjoint solve and a central
difference, p-multigrid in the adjoint, a chain from Young's modulus to point
observations, the unchanged forward path and the refusals.

Random fields are scaled so that the largest Frobenius norm of the
displacement gradient H over all points, computed by the reference, is 0.3,
with min J >= 0.3 asserted from the reference before the kernel is looked
at."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from swirl_fem_amd import _lib, _ops
from swirl_fem_amd.core import layout, operators
from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import NodeType, Quadrature1D
from swirl_fem_amd.examples import hyperelasticity as hy
from swirl_fem_amd.examples.hyperelasticity import BCType
from swirl_fem_amd.examples.hyperelasticity import solve_hyperelasticity
from swirl_fem_amd.linalg.pmg_elasticity import ElasticityPMultigrid
from tests import geometry_cases as G
from tests import hyperelastic_adjoint_reference as HA
from tests import hyperelastic_reference as HR
from tests.fp32util import F32Rng, f32r, tolerance
from tests.test_gpu_hyperelastic import KERNEL_COMBOS, MESH_P, MIN_J, SCALE

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64 = torch.float64
GL = NodeType.GAUSS_LEGENDRE
D, N = BCType.DIRICHLET, BCType.NEUMANN
NAMES = ('dlam', 'dmu', 'drho')
SUBSETS = [(True, True, True), (True, False, False), (False, True, False),
           (False, False, True)]


def _dev(a, dtype=F64):
  return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _np(t):
  return t.detach().double().cpu().numpy()


def _rel(a, b):
  return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _t(fn):
  """A NumPy callable on points as a torch callable."""
  return lambda x: _dev(fn(_np(x)))


def _leaf(a):
  return _dev(a).requires_grad_(True)


# ------------------------------------------------ 1. kernel vs reference
def _kernel_setup(case, Q, dtype=F64):
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


def _run_sens(op, ref, ndim, Q, pad, rng, dtype, tol, combos,
              rnd=lambda a: a):
  """Per combination of `KERNEL_COMBOS` (its coefficients form the state's
  residual launch in the reference, its lambda0 is the kernel's): all three
  outputs together and each alone against `grid_sens` with the REFERENCE's
  state, in the max norm of each output.  A skipped output is None and the
  others are bitwise what the full launch gave.  The `pad` trailing rows (W =
  0) carry random fields and a zero state row and must give exactly zero.
  Above `tol` in fp32 the project's exception rule applies: the NumPy
  reference evaluated in float32, 4 times its error.  Returns [(combo, name,
  error, allowed)]."""
  E, nq = ref.num_elements, ref.Q
  rows = []
  for n, (lam, mu, rho, l0) in enumerate(combos):
    coef = lambda c: (rnd(c[1] * (1.0 + 0.2 * rng.uniform(-1, 1, (E, nq))))
                      if isinstance(c, tuple) else c)
    lam, mu, rho = coef(lam), coef(mu), coef(rho)
    uq = _scaled_grid_field(ref, rng, ndim, rnd)
    vq = rnd(rng.standard_normal((E, nq, ndim)))
    state = rnd(HR.grid_residual(ref, uq, lam, mu, rho, l0)[1])
    want = HA.grid_sens(ref, vq, state, uq, l0)
    padded = lambda a: _dev(np.concatenate(
        [a, rng.standard_normal((pad,) + a.shape[1:])]), dtype)
    ud, vd = padded(uq), padded(vq)
    sd = _dev(np.concatenate([state, np.zeros((pad,) + state.shape[1:])]),
              dtype)
    full = None
    for subset in SUBSETS:
      got = _ops.hyperelastic_sens(vd, sd, op.parts, op.host, ndim, Q,
                                   op.point_weights(), ud, l0, want=subset)
      for k, (g, w, on) in enumerate(zip(got, want, subset)):
        if not on:
          assert g is None
          continue
        assert g.shape == (E + pad, nq) and g.dtype == dtype
        if pad:     # W = 0: exactly zero, whatever the state row holds
          assert float(g[E:].abs().max()) == 0.0, (NAMES[k], subset)
        if full is not None:
          assert torch.equal(g, full[k]), (NAMES[k], subset)
          continue
        err = _rel(_np(g)[:E], w)
        if not l0 and k == 2:
          assert float(g.abs().max()) == 0.0
        allowed = tol
        if err > tol and dtype == torch.float32:
          ref32 = HA.grid_sens(ref, vq, state, uq, l0, dtype=np.float32)[k]
          allowed = max(tol, 4.0 * _rel(ref32.astype(np.float64), w))
        print(f'{dtype} ndim={ndim} Q={Q} combo {n} {NAMES[k]}: rel err '
              f'{err:.3e} (allowed {allowed:.3e})')
        rows.append((n, NAMES[k], err, allowed))
        assert err <= allowed, (ndim, Q, n, NAMES[k], err, allowed)
      if full is None:
        full = got
    # without u the Lame outputs are what they were
    got = _ops.hyperelastic_sens(vd, sd, op.parts, op.host, ndim, Q,
                                 op.point_weights(), None, l0,
                                 want=(True, True, False))
    assert got[2] is None
    assert torch.equal(got[0], full[0]) and torch.equal(got[1], full[1])
  return rows


@pytest.mark.parametrize('Q', range(2, 13))
@pytest.mark.parametrize('ndim', [2, 3])
def test_kernel_matches_reference(ndim, Q):
  """fp64, every Q, on multilinear and curved elements with a padded row
  (list launches, a partial workgroup), every combination of
  `KERNEL_COMBOS`."""
  case = G.three_kinds(2, ndim, MESH_P, pad=1)
  mesh, fes, ref, op = _kernel_setup(case, Q)
  assert len(op.parts) >= 2 and all('elem_list' in p for p in op.parts)
  assert {G.CURVED, G.MULTILINEAR} <= {p['geo_mode'] for p in op.parts}
  assert float(op.point_weights()[-1].abs().max()) == 0.0
  rng = np.random.default_rng(100 * ndim + Q)
  _run_sens(op, ref, ndim, Q, 1, rng, F64, tolerance(F64, Q), KERNEL_COMBOS)


@pytest.mark.parametrize('Q', range(2, 13))
@pytest.mark.parametrize('ndim', [2, 3])
def test_kernel_affine_elements(ndim, Q):
  """The affine instantiations at every Q (one launch over all elements, no
  list)."""
  case = G.affine(2, ndim, MESH_P)
  mesh, fes, ref, op = _kernel_setup(case, Q)
  assert [p['geo_mode'] for p in op.parts] == [G.AFFINE]
  assert 'elem_list' not in op.parts[0]
  rng = np.random.default_rng(7 * ndim + Q)
  _run_sens(op, ref, ndim, Q, 0, rng, F64, tolerance(F64, Q),
            KERNEL_COMBOS[:3])


@pytest.mark.parametrize('Q', [2, 5, 8, 9, 12])
@pytest.mark.parametrize('ndim', [2, 3])
def test_kernel_fp32(ndim, Q):
  """fp32 with float32-representable meshes and inputs (the state included)
  against the fp64 reference at `tolerance(torch.float32, Q)`.  A case above
  that is held to 4 times the error of the NumPy reference evaluated in
  float32 (DESIGN §3.21 lists them)."""
  case = G.three_kinds(2, ndim, MESH_P)
  mesh, fes, ref, op = _kernel_setup(case, Q, torch.float32)
  rng = F32Rng(Q)
  rows = _run_sens(op, ref, ndim, Q, 0, rng, torch.float32,
                   tolerance(torch.float32, Q), KERNEL_COMBOS, rnd=f32r)
  for n, name, err, allowed in rows:
    if err > tolerance(torch.float32, Q):
      print(f'EXCEPTION ndim={ndim} Q={Q} combo {n} {name}: {err:.3e} <= '
            f'{allowed:.3e}')


# ------------------------------------------------ 2. kernel vs kernel
@pytest.mark.parametrize('Q', [3, 6, 9, 12])
@pytest.mark.parametrize('ndim', [2, 3])
def test_linearity_against_residual_kernel(ndim, Q):
  """P is linear in (lam, mu, rho): sum_q (lam s_lam + mu s_mu + rho s_rho)
  from the new kernel, fed the state that `sfem_hyperelastic_local` itself
  stored, equals v_q . r_q of that residual launch, to `tolerance(float64,
  Q)` relative to |v| |r|; scalar and per-point coefficients."""
  case = G.three_kinds(2, ndim, MESH_P)
  mesh, fes, ref, op = _kernel_setup(case, Q)
  tol = tolerance(F64, Q)
  rng = np.random.default_rng(50 * ndim + Q)
  E, nq = ref.num_elements, ref.Q
  uq = _scaled_grid_field(ref, rng, ndim, lambda a: a)
  ud, vd = _dev(uq), _dev(rng.standard_normal((E, nq, ndim)))
  point = lambda c: _dev(c * (1.0 + 0.2 * rng.uniform(-1, 1, (E, nq))))
  for lam, mu, rho, l0 in ((1.3, 0.7, 1.5, 0.0), (1.3, 0.7, 1.5, 1.7),
                           (point(1.0), point(0.8), point(1.5), 2.5),
                           (point(50.0), point(1.0), 1.5, 0.0)):
    rq, state, _ = _ops.hyperelastic_local(
        ud, op.parts, op.host, ndim, Q, op.point_weights(), lam, mu, rho, l0,
        mode='residual', want_state=True)
    sl, sm, sr = _ops.hyperelastic_sens(vd, state, op.parts, op.host, ndim, Q,
                                        op.point_weights(), ud, l0)
    got = float((lam * sl + mu * sm + rho * sr).sum())
    want = float((vd * rq).sum())
    scale = float(vd.norm() * rq.norm())
    print(f'{ndim}D Q={Q} lambda0={l0}: |sum theta s - v.r| / (|v||r|) = '
          f'{abs(got - want) / scale:.2e}')
    assert abs(got - want) <= tol * scale


# ------------------------------------------------ 3. op.sensitivity forms
@functools.lru_cache(maxsize=None)
def _assembled(ndim):
  P = 4 if ndim == 2 else 3
  case = G.curved_multilinear(2, ndim, P)
  mesh, _, rp = case.finalize(DEV, F64)
  q = P - 1 + (ndim + 1) // 2
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(q, GL))
  ref = HR.space(rp.node_coords, rp.elements, P, (q, 'gl'))
  return mesh, fes, ref, q


@pytest.mark.parametrize('ndim', [2, 3])
def test_operator_sensitivity_forms(ndim):
  """Scalar, (E,), (E, Q^d) and callable sources, an absent density, dense
  and component-major fields, `want` subsets: each gradient in the form of
  its source against the reference's reduction, 1e-10; with `linearization=`
  (the object or its state tensor) bitwise what the method computes without;
  shape errors."""
  mesh, fes, ref, Q = _assembled(ndim)
  rng = np.random.default_rng(9 + ndim)
  E, nq = mesh.num_elements, Q ** ndim
  un = rng.standard_normal((mesh.num_nodes, ndim))
  H = HR.gradients(ref, ref.gather(un))
  un *= SCALE / np.sqrt((H * H).sum((-2, -1))).max()
  H = HR.gradients(ref, ref.gather(un))
  assert np.linalg.det(H + np.eye(ndim)).min() >= MIN_J
  vn = rng.standard_normal((mesh.num_nodes, ndim))
  l0 = 0.8
  want = HA.point_sensitivities(ref, un, vn, l0)
  u, v = _dev(un), _dev(vn)
  sources = {
      'scalar': lambda: 1.3,
      'tensor0': lambda: torch.tensor(1.3, dtype=F64, device=DEV),
      'elem': lambda: _dev(0.5 + rng.random(E)),
      'point': lambda: _dev(0.5 + rng.random((E, nq))),
      'callable': lambda: (lambda x: 1.0 + x[:, 0] ** 2),
  }
  form_of = {'scalar': 'scalar', 'tensor0': 'scalar', 'elem': 'elem',
             'point': 'point'}
  for forms in (('scalar', 'elem', 'point'), ('point', 'tensor0', 'elem'),
                ('elem', 'point', 'callable'), ('callable', 'scalar', None)):
    src = [None if f is None else sources[f]() for f in forms]
    op = fes.hyperelastic_operator(lame_lambda=src[0], lame_mu=src[1],
                                   density=src[2])
    lin = op.linearize(u, l0)
    for fields in ((u, v), (layout.component_major(u),
                            layout.component_major(v))):
      got = op.sensitivity(*fields, l0)
      for g, w, f in zip(got, want, forms):
        if f in (None, 'callable'):
          assert g is None
          continue
        w = HA.reduce_coefficient(w, form_of[f])
        assert tuple(g.shape) == np.shape(w), f
        assert _rel(_np(g), np.asarray(w)) <= 1e-10, f
      for given in (lin, lin.state):
        again = op.sensitivity(*fields, l0, linearization=given)
        for a, b in zip(got, again):
          assert (a is None and b is None) or torch.equal(a, b)
    for subset in SUBSETS[1:]:
      got = op.sensitivity(u, v, l0, want=subset, linearization=lin)
      for g, on, f in zip(got, subset, forms):
        assert (g is not None) == (on and f not in (None, 'callable'))
  assert op.sensitivity(u, v, want=(False, False, True)) == (None, None, None)
  with pytest.raises(ValueError):
    op.sensitivity(u[:, 0], v)
  with pytest.raises(ValueError):
    op.sensitivity(u, v[:-1])
  with pytest.raises(ValueError, match='state'):
    op.sensitivity(u, v, linearization=lin.state[:, :, :-1])
  with pytest.raises(ValueError, match='want'):
    op.sensitivity(u, v, want=(True, True))


# -------------------------------------------- 4. gradients through the solve
# Newton to 1e-11 of the residual at the start of the last load step (the
# dense Newton of the reference reaches 1e-14 of the load on the CPU, `tests/
# test_hyperelastic_adjoint_host.py`), inexact steps to 1e-8, the adjoint CG
# to 1e-12: the adjoint solve's accuracy is the gradient's.
SOLVE_KW = dict(load_steps=2, newton_rtol=1e-11, linear_rtol=1e-8,
                adjoint_rtol=1e-12, max_newton=40)


@functools.lru_cache(maxsize=None)
def _solve_setup(ndim, lambda0):
  """`HA.SolveProblem` on the GPU next to its dense reference, with the
  reference solution and gradient computed once; the finite-strain regime is
  asserted here."""
  rp, _, _ = HA.EA.AJ.solve_problem(ndim)
  mesh = rp.finalize(device=DEV)
  facets = mesh.boundary_facets['x1'].cpu().numpy().astype(np.int64)
  prob = HA.SolveProblem(ndim, lambda0, facets)
  u, gf, gl, gm, gr, cond = prob.gradients()
  hmax, jmin = prob.strain_measures()
  assert hmax >= 0.1 and jmin >= 0.3, (hmax, jmin)
  # a (d,) body force: the dense Newton solution and its force gradient
  fc = prob.LOAD[ndim] * np.array([0.3, -1.0, 0.5][:ndim])
  force = np.tile(fc, (len(prob.x), 1))
  u_fc = prob.solve(prob.dense(), force)
  gfc = HA.adjoint_gradients(prob.dense(), u_fc, prob.w, prob.fixed)[0]
  return dict(mesh=mesh, prob=prob, bcs=_bcs(prob), u=u, cond=cond,
              grads=dict(force=gf, lam=gl, mu=gm, rho=gr),
              constant=(fc, force, gfc.sum(axis=0)))


def _bcs(prob):
  roller = [None] * prob.ndim
  roller[1] = _t(prob.roll)
  return {'y0': (D, tuple(roller)),
          'x0': (D, tuple(_t(g) for g in prob.gD)),
          'x1': (N, tuple(g if not callable(g) else _t(g)
                          for g in prob.trac))}


def _gpu_solve(s, pc, lam, mu, rho, force=None, differentiable=True, **kw):
  prob = s['prob']
  force = _dev(prob.force) if force is None else force
  u, info = solve_hyperelasticity(
      s['mesh'], force, s['bcs'], lame_lambda=lam, lame_mu=mu, density=rho,
      lambda0=prob.lambda0, preconditioner=pc, return_info=True,
      differentiable=differentiable, **{**SOLVE_KW, **kw})
  assert info['status'] == 'converged'
  return u, info


def _bound(s, u, dense=None, force=None):
  """100 cond max(rho_res, 1e-12) with rho_res the relative residual that the
  NumPy reference finds at the GPU's solution, asserted <= 1e-9."""
  rho_res = s['prob'].relative_residual(_np(u), dense, force)
  assert rho_res <= 1e-9, rho_res
  return 100.0 * s['cond'] * max(rho_res, 1e-12), rho_res


@pytest.mark.parametrize('lambda0', [0.0, 1.7])
@pytest.mark.parametrize('pc', [None, 'jacobi'])
@pytest.mark.parametrize('ndim', [2, 3])
def test_solve_gradients_match_dense_adjoint(ndim, pc, lambda0):
  """`.grad` of a per-point lame_lambda, a per-element lame_mu, a scalar
  density and an (N, d) body force of the loss (w * u).sum() against the
  dense adjoint solve at the dense Newton solution, on the jittered mesh with
  a clamped face (x0, with values), a roller (y0), a traction (x1) and a body
  force in the finite-strain regime; then a (d,) body force.  `SOLVE_KW`:
  newton_rtol 1e-11, linear_rtol 1e-8, adjoint_rtol 1e-12, two load steps.
  Bound: 100 cond max(rho_res, 1e-12) relative, rho_res = |keep (R_ref(u_gpu)
  - f)| / |f| by the NumPy reference (asserted <= 1e-9), cond of the dense
  free tangent block (2D 1.2e3 / 8.3e2, 3D 1.8e3 / 6.6e2 for lambda0 = 0 /
  1.7).  Measured on an MI355X: 4 to 5 Newton iterations per load step,
  rho_res 1.2e-14 .. 3.3e-14, bounds 6.6e-8 .. 1.8e-7; u within 2.7e-15,
  force 7.8e-14 .. 1.5e-12, lam 2.3e-13 .. 7.2e-13, mu 1.2e-13 .. 2.8e-12, rho
  5.5e-16 .. 1.9e-12, the (d,) force 1.0e-14 .. 5.2e-13."""
  s = _solve_setup(ndim, lambda0)
  prob = s['prob']
  lam, mu, f = _leaf(prob.lam_q), _leaf(prob.mu_e), _leaf(prob.force)
  rho = torch.tensor(prob.rho, dtype=F64, device=DEV, requires_grad=True)
  u, info = _gpu_solve(s, pc, lam, mu, rho, f)
  assert u.grad_fn is not None and 'adjoint' not in info
  bound, rho_res = _bound(s, u)
  err_u = _rel(_np(u), s['u'])
  print(f'ndim={ndim} lambda0={lambda0} {pc}: cond {s["cond"]:.3e}, rho_res '
        f'{rho_res:.2e}, bound {bound:.2e}, u rel err {err_u:.2e}, Newton '
        f'{[len(t["step_lengths"]) for t in info["load_steps"]]}')
  assert err_u <= bound
  (u * _dev(prob.w)).sum().backward()
  assert info['adjoint']['status'] == 'converged'
  g = s['grads']
  checks = [('force', f.grad, g['force']), ('lam', lam.grad, g['lam']),
            ('mu', mu.grad, HA.reduce_coefficient(g['mu'], 'elem'))]
  for name, got, want in checks:
    assert got is not None and tuple(got.shape) == want.shape, name
    err = _rel(_np(got), want)
    print(f'  d/d{name}: rel err {err:.2e}')
    assert err <= bound, name
  assert rho.grad.shape == ()
  if lambda0:
    err = abs(float(rho.grad) - g['rho'].sum()) / np.abs(g['rho']).sum()
    print(f'  d/drho: rel err {err:.2e}')
    assert err <= bound
  else:
    assert float(rho.grad) == 0.0
  # a (d,) body force: its gradient is the nodal one summed over the nodes
  fc_np, force, gfc = s['constant']
  fc = _leaf(fc_np)
  u, _ = _gpu_solve(s, pc, _dev(prob.lam_q), _dev(prob.mu_e), prob.rho, fc)
  (u * _dev(prob.w)).sum().backward()
  bound, _ = _bound(s, u, prob.dense(), force)
  assert fc.grad.shape == (ndim,)
  err = _rel(_np(fc.grad), gfc)
  print(f'  d/d(constant force): rel err {err:.2e}')
  assert err <= bound


@pytest.mark.parametrize('ndim', [2, 3])
def test_central_difference_through_the_solve(ndim):
  """One central difference per coefficient (h = `HA.CD_H` = 1e-3, the
  directions of the host test) through the GPU solve against its own `.grad`,
  lambda0 = 1.7, Jacobi.  The dense reference on the same problem, directions
  and step sets the floor, the truncation of the quotient
  (`test_hyperelastic_adjoint_host`, which asserts it: 2D lam 2.5e-7, mu
  4.4e-7, rho 4.0e-8; 3D lam 2.5e-7, mu 2.3e-7, rho 5.1e-6); 10 x that is
  allowed.  Measured on an MI355X: 2D 2.50e-7, 4.44e-7, 4.01e-8; 3D 2.54e-7,
  2.35e-7, 5.13e-6, the reference's figures to three digits (both sides
  measure the truncation of the quotient)."""
  s = _solve_setup(ndim, 1.7)
  prob = s['prob']
  cds = HA.central_differences(prob)
  lam, mu = _leaf(prob.lam_q), _leaf(prob.mu_q())
  rho = torch.tensor(prob.rho, dtype=F64, device=DEV, requires_grad=True)
  w = _dev(prob.w)
  kw = dict(newton_rtol=1e-12, linear_rtol=1e-10, adjoint_rtol=1e-13)
  u, _ = _gpu_solve(s, 'jacobi', lam, mu, rho, **kw)
  (u * w).sum().backward()
  h = HA.CD_H
  base = dict(lam=prob.lam_q, mu=prob.mu_q(), rho=prob.rho)
  u0 = u.detach()

  def val(**over):
    c = {k: (_dev(v) if isinstance(v, np.ndarray) else v)
         for k, v in {**base, **over}.items()}
    # from the solution next to it, in one load step, to the same absolute
    # residual (newton_rtol is relative to the residual at the start)
    u, _ = _gpu_solve(s, 'jacobi', c['lam'], c['mu'], c['rho'],
                      differentiable=False, u0=u0, load_steps=1,
                      newton_rtol=0.0, newton_atol=atol, linear_rtol=1e-10)
    return float((u * w).sum())
  keep = (~prob.fixed).astype(np.float64)
  atol = 1e-12 * float(np.linalg.norm(keep * HA.load_vector(
      prob.dense(), prob.force, prob.tractions)))
  worst = []
  for name, leaf in (('lam', lam), ('mu', mu), ('rho', rho)):
    ref_rel, dirn, _ = cds[name]
    an = float((leaf.grad * _dev(dirn)).sum())
    cd = (val(**{name: base[name] + h * dirn}) -
          val(**{name: base[name] - h * dirn})) / (2 * h)
    rel = abs(cd - an) / abs(an)
    print(f'ndim={ndim} {name}: {rel:.2e} (reference {ref_rel:.2e})')
    worst.append((name, rel, ref_rel))
  for name, rel, ref_rel in worst:
    assert rel <= 10.0 * ref_rel, (name, rel, ref_rel)


def test_pmultigrid_in_forward_and_adjoint():
  """`ElasticityPMultigrid` (built once on the linear operator) preconditions
  the Newton steps and the adjoint solve of the 3D problem: gradients within
  the bound of `test_solve_gradients_match_dense_adjoint`, the adjoint's CG
  converged; its iteration count is printed next to Jacobi's."""
  s = _solve_setup(3, 0.0)
  prob = s['prob']
  its = {}
  for pc in ('jacobi', ElasticityPMultigrid):
    lam, mu = _leaf(prob.lam_q), _leaf(prob.mu_e)
    u, info = _gpu_solve(s, pc, lam, mu, prob.rho)
    bound, rho_res = _bound(s, u)
    (u * _dev(prob.w)).sum().backward()
    assert info['adjoint']['status'] == 'converged'
    its[pc] = int(info['adjoint']['num_iterations'])
    g = s['grads']
    errs = (_rel(_np(u), s['u']), _rel(_np(lam.grad), g['lam']),
            _rel(_np(mu.grad), HA.reduce_coefficient(g['mu'], 'elem')))
    print(f'{getattr(pc, "__name__", pc)}: adjoint CG iterations {its[pc]}, '
          f'forward CG {info["num_cg"]}, rho_res {rho_res:.2e}, bound '
          f'{bound:.2e}, rel err u {errs[0]:.2e}, lam {errs[1]:.2e}, mu '
          f'{errs[2]:.2e}')
    assert max(errs) <= bound
  print(f'adjoint CG iterations: p-multigrid {its[ElasticityPMultigrid]}, '
        f'Jacobi {its["jacobi"]}')


def test_chain_from_youngs_modulus_to_point_observations():
  """Per-element Young's modulus -> `lame_parameters` -> solve ->
  `mesh.point_evaluator` observations -> least-squares loss: dL/dE from
  `.backward()` against the dense adjoint at the dense Newton solution with
  the cotangent the evaluator's transpose gives, chained by hand through
  lam = E nu / ((1 + nu)(1 - 2 nu)), mu = E / (2 (1 + nu))."""
  s = _solve_setup(2, 0.0)
  prob = s['prob']
  nu = 0.3
  E, nq = prob.lam_q.shape
  rng = np.random.default_rng(21)
  young = 2.0 + rng.random(E)
  lam_e, mu_e = operators.lame_parameters(young, nu)
  expand = lambda c: HA.expand_coefficient(c, E, nq)
  dense = prob.dense(expand(lam_e), expand(mu_e), 1.0)
  u_ref = prob.solve(dense)
  H = HR.gradients(prob.fes, prob.fes.gather(u_ref))
  assert np.sqrt((H * H).sum((-2, -1))).max() >= 0.1
  assert np.linalg.det(H + np.eye(2)).min() >= 0.3
  pts = _dev([[0.21, 0.33], [0.5, 0.5], [0.77, 0.12], [0.9, 0.95],
              [0.34, 0.81]])
  ev = s['mesh'].point_evaluator(pts)
  obs = _dev(0.01 * np.arange(10.0).reshape(5, 2))
  Et = _leaf(young)
  lam_t, mu_t = operators.lame_parameters(Et, nu)
  u, info = _gpu_solve(s, 'jacobi', lam_t, mu_t, None)
  misfit = ev(u) - obs
  (0.5 * (misfit ** 2).sum()).backward()
  w = _np(ev.transpose(misfit.detach()))
  _, gl, gm, _, cond = HA.adjoint_gradients(dense, u_ref, w, prob.fixed)
  want = (gl.sum(1) * nu / ((1 + nu) * (1 - 2 * nu)) +
          gm.sum(1) / (2 * (1 + nu)))
  rho_res = prob.relative_residual(_np(u), dense)
  assert rho_res <= 1e-9
  bound = 100.0 * cond * max(rho_res, 1e-12)
  err = _rel(_np(Et.grad), want)
  print(f'chain: dL/dE rel err {err:.2e} (bound {bound:.2e}, rho_res '
        f'{rho_res:.2e}, cond {cond:.3e})')
  assert Et.grad.shape == (E,)
  assert err <= bound


# ------------------------------------------------------ 5. unchanged behaviour
def test_no_side_effects(monkeypatch):
  """With `differentiable=True` and nothing requiring grad (or under
  `torch.no_grad()`) the body runs exactly as by default: one call of
  `_solve` with the caller's own arguments and no `_state`, whose result is
  returned as it is, without a `grad_fn`.  With a leaf that requires grad the
  node hands the body the detached inputs and returns bitwise what the body
  computed.  `info['adjoint']` is absent before `backward` and present after.
  Two separate calls are compared to 2 cond newton_rtol, not bitwise: shared
  nodes and inner products are summed with float atomics in this project, so
  two identical calls already differ in the last bits (as `tests/
  test_gpu_elasticity_adjoint.py` notes); whether they were equal is
  printed."""
  body = hy._solve
  seen = []

  def recording(mesh, force, bcs, **kw):
    out = body(mesh, force, bcs, **kw)
    seen.append((force, kw, out, out[0].clone()))
    return out
  monkeypatch.setattr(hy, '_solve', recording)
  s = _solve_setup(2, 1.7)
  prob = s['prob']
  bound = 2.0 * s['cond'] * SOLVE_KW['newton_rtol']
  lam, mu = _dev(prob.lam_q), _dev(prob.mu_e)
  plain, _ = _gpu_solve(s, 'jacobi', lam, mu, prob.rho, differentiable=False)
  assert plain.grad_fn is None and not plain.requires_grad
  del seen[:]
  flagged, info = _gpu_solve(s, 'jacobi', lam, mu, prob.rho)
  assert flagged.grad_fn is None and not flagged.requires_grad
  assert len(seen) == 1 and seen[0][2][0] is flagged
  assert '_state' not in seen[0][1] and 'adjoint' not in info
  assert seen[0][1]['lame_lambda'] is lam and seen[0][1]['lame_mu'] is mu
  print(f'flagged vs default call: bitwise equal {torch.equal(flagged, plain)}'
        f', rel diff {_rel(_np(flagged), _np(plain)):.2e}')
  assert _rel(_np(flagged), _np(plain)) <= bound
  lg, fg = _leaf(prob.lam_q), _leaf(prob.force)
  del seen[:]
  tracked, info = _gpu_solve(s, 'jacobi', lg, mu, prob.rho, fg)
  assert tracked.grad_fn is not None and len(seen) == 1
  force, kw, _, u_body = seen[0]
  assert not force.requires_grad and torch.equal(force, fg.detach())
  assert not kw['lame_lambda'].requires_grad
  assert torch.equal(kw['lame_lambda'], lam)
  assert torch.equal(kw['lame_mu'], mu) and kw['density'] == prob.rho
  assert isinstance(kw['_state'], dict)
  assert torch.equal(tracked.detach(), u_body)
  print(f'tracked vs default call: bitwise equal '
        f'{torch.equal(tracked.detach(), plain)}, rel diff '
        f'{_rel(_np(tracked), _np(plain)):.2e}')
  assert _rel(_np(tracked), _np(plain)) <= bound
  assert 'adjoint' not in info
  tracked.sum().backward()
  assert info['adjoint']['status'] == 'converged'
  assert lg.grad is not None and fg.grad is not None
  del seen[:]
  with torch.no_grad():
    quiet, _ = _gpu_solve(s, 'jacobi', lg, mu, prob.rho, differentiable=False)
  assert quiet.grad_fn is None and '_state' not in seen[0][1]
  assert _rel(_np(quiet), _np(plain)) <= bound


# ----------------------------------------------------------------- 6. refusals
def test_refusals_and_failures():
  """`u0` that requires grad is refused with and without the keyword; without
  the keyword a leaf is refused as before; a second `backward` through the
  node raises; a callable coefficient receives no gradient and raises
  nothing; the wrapper's own checks."""
  s = _solve_setup(2, 0.0)
  prob = s['prob']
  lam, mu = _dev(prob.lam_q), _dev(prob.mu_e)
  u0 = torch.zeros((len(prob.x), 2), dtype=F64, device=DEV,
                   requires_grad=True)
  for flag in (False, True):
    with pytest.raises(NotImplementedError, match='u0'):
      _gpu_solve(s, 'jacobi', lam, mu, None, differentiable=flag, u0=u0)
  with pytest.raises(NotImplementedError, match='differentiable=True'):
    _gpu_solve(s, 'jacobi', _leaf(prob.lam_q), mu, None, differentiable=False)
  # a callable lame_lambda next to a leaf: the leaf alone receives a gradient
  mg = _leaf(prob.mu_e)
  lam_fn = lambda x: 1.0 + 0.5 * x[..., 0] ** 2
  u, info = _gpu_solve(s, 'jacobi', lam_fn, mg, None)
  loss = (u * _dev(prob.w)).sum()
  loss.backward()
  assert mg.grad is not None and bool(torch.isfinite(mg.grad).all())
  assert info['adjoint']['status'] == 'converged'
  with pytest.raises(RuntimeError):      # once_differentiable, buffers freed
    loss.backward()
  # a breakdown of the adjoint CG names the adjoint solve
  mg = _leaf(prob.mu_e)
  u, info = _gpu_solve(s, 'jacobi', lam, mg, None)
  node = u.grad_fn
  node.state['lin'].state.mul_(float('nan'))
  with pytest.raises(RuntimeError, match='adjoint solve'):
    with pytest.warns(RuntimeWarning, match='breakdown'):
      (u * _dev(prob.w)).sum().backward()
  assert str(info['adjoint']['status']).startswith('breakdown')
  # the wrapper
  mesh, fes, ref, Q = _assembled(3)
  op = fes.hyperelastic_operator(lame_lambda=1.0, lame_mu=1.0)
  E, nq = mesh.num_elements, Q ** 3
  z = torch.zeros((E, nq, 3), dtype=F64, device=DEV)
  st = torch.zeros((E, nq, 10), dtype=F64, device=DEV)
  args = (op.parts, op.host, 3, Q, op.point_weights())
  with pytest.raises(ValueError, match='want'):
    _ops.hyperelastic_sens(z, st, *args, z, want=(False, False, False))
  with pytest.raises(ValueError, match='displacement'):
    _ops.hyperelastic_sens(z, st, *args, None)
  with pytest.raises(ValueError, match='state'):
    _ops.hyperelastic_sens(z, st[:, :, :9], *args, z)
  with pytest.raises(ValueError, match='state'):
    _ops.hyperelastic_sens(z, None, *args, z)
  with pytest.raises(ValueError):
    _ops.hyperelastic_sens(z[:, :, :2], st, *args, z)


def _raw_args(op, fes, **over):
  """A valid `HyperelasticSensArgs` for the first launch of `op`, with
  overrides; returns (args, what must stay alive)."""
  mesh = fes.mesh
  d, Q = mesh.ndim, fes.quadrature.num_points
  E, nq = mesh.num_elements, Q ** d
  zeros = lambda *s: torch.zeros(s, dtype=F64, device=DEV)
  state = zeros(E, nq, d * d + 1)
  state[:, :, :d * d] = torch.eye(d, dtype=F64, device=DEV).reshape(-1)
  keep = dict(u=zeros(E, nq, d) + 1.0, v=zeros(E, nq, d) + 2.0, state=state,
              dlam=zeros(E, nq), dmu=zeros(E, nq), drho=zeros(E, nq),
              host={k: np.ascontiguousarray(v, np.float64)
                    for k, v in op.host.items()})
  part = op.parts[0]
  args = _lib.HyperelasticSensArgs(
      v=keep['v'].data_ptr(), state=state.data_ptr(), u=keep['u'].data_ptr(),
      wdet=op.point_weights().data_ptr(), dlam=keep['dlam'].data_ptr(),
      dmu=keep['dmu'].data_ptr(), drho=keep['drho'].data_ptr(), lambda0=1.0,
      geo_elem=part['geo_elem'].data_ptr(),
      dmat=keep['host']['dmat'].ctypes.data,
      weights=keep['host']['weights'].ctypes.data,
      nodes=keep['host']['nodes'].ctypes.data, num_elements=E, ndim=d, P=Q,
      dtype=_lib.SFEM_F64, geo_mode=part['geo_mode'])
  for k, v in over.items():
    setattr(args, k, v)
  return args, keep


def test_entry_point_refusals():
  """Status codes of the raw entry point: one valid call, then one field
  wrong at a time; nothing that is refused launches."""
  case = G.affine(2, 3, MESH_P)
  mesh, _, rp = case.finalize(DEV, F64)
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(4, GL))
  op = fes.hyperelastic_operator(lame_lambda=1.0, lame_mu=1.0)
  call = lambda a: _lib.load().sfem_hyperelastic_sens(ctypes.byref(a), None)
  ok, keep = _raw_args(op, fes)
  assert call(ok) == 0
  torch.cuda.synchronize()
  # constant fields at the state (I, 0): H_v = 0, so dlam = dmu = 0 and drho
  # = lambda0 W u . v = 6 W
  W = op.point_weights()
  assert not _np(keep['dlam']).any()
  assert float(keep['dmu'].abs().max()) <= 1e-12 * float(W.max())
  assert _rel(_np(keep['drho']), 6.0 * _np(W)) <= 1e-14
  ok, keep = _raw_args(op, fes, drho=None, u=None)
  assert call(ok) == 0
  ok, keep = _raw_args(op, fes, dlam=None, dmu=None)
  assert call(ok) == 0
  torch.cuda.synchronize()
  # outside the compiled range: SFEM_EUNSUPPORTED
  for over in (dict(P=13), dict(P=1), dict(ndim=1), dict(ndim=4),
               dict(geo_mode=_lib.GEO_BOX), dict(geo_mode=7)):
    a, keep = _raw_args(op, fes, **over)
    assert call(a) == -3, over
  # all three outputs null, a null state or v, drho without u, a missing
  # geometry array: SFEM_EINVAL
  for over in (dict(dlam=None, dmu=None, drho=None), dict(state=None),
               dict(v=None), dict(u=None), dict(dmat=None), dict(wdet=None),
               dict(geo_elem=None), dict(weights=None), dict(nodes=None),
               dict(geo_mode=_lib.GEO_POINT), dict(dtype=5),
               dict(num_elements=-1),
               dict(elem_list=keep['u'].data_ptr(), num_listed=10 ** 6)):
    a, keep = _raw_args(op, fes, **over)
    assert call(a) == -1, over
  assert _lib.load().sfem_hyperelastic_sens(None, None) == -1
  # nothing to do is not an error
  a, keep = _raw_args(op, fes, num_elements=0, v=None, state=None)
  assert call(a) == 0
