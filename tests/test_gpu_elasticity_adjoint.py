"""Gradients of elasticity solves on the GPU: the kernel
`sfem_elasticity_sens` at every Q = 2..12 against the NumPy reference
(`tests/elasticity_adjoint_reference.py`), against the forward kernel,
`ElasticityOperator.sensitivity` in every coefficient form, `.grad` through
`solve_elasticity` against the dense adjoint solve and a central difference,
compliance, point observations, the unchanged forward path and the
refusals."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from swirl_fem_amd import _lib, _ops
from swirl_fem_amd.core import layout, operators
from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import NodeType, Quadrature1D
from swirl_fem_amd.examples import elasticity as el
from swirl_fem_amd.examples.elasticity import BCType, solve_elasticity
from tests import elasticity_adjoint_reference as EA
from tests import elasticity_reference as ER
from tests import geometry_cases as G
from tests.fp32util import F32Rng, f32r, tolerance

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64 = torch.float64
GLL, GL = NodeType.GAUSS_LOBATTO_LEGENDRE, NodeType.GAUSS_LEGENDRE
D, N = BCType.DIRICHLET, BCType.NEUMANN
MESH_P = 3       # nodes per direction of the kernel tests' meshes
NAMES = ('dlam', 'dmu', 'drho')


def _dev(a, dtype=F64):
  return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _np(t):
  return t.detach().double().cpu().numpy()


def _rel(a, b):
  return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _t(fn):
  """A NumPy callable on points as a torch callable."""
  return lambda x: _dev(fn(_np(x)))


# ------------------------------------------------ 1. kernel vs reference
def _kernel_setup(case, Q, dtype=F64):
  mesh, _, rp = case.finalize(DEV, dtype)
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(Q, GL))
  ref = ER.space(rp.node_coords, rp.elements, MESH_P, (Q, 'gl'))
  op = fes.elasticity_operator(lame_lambda=1.0, lame_mu=1.0)
  return mesh, fes, ref, op


SUBSETS = [(True, True, True), (True, False, False), (False, True, False),
           (False, False, True)]


def _run_sens(op, ref, ndim, Q, pad, rng, dtype, tol, rnd=lambda a: a):
  """All three outputs together and each alone, lambda0 zero and non-zero,
  against `grid_sens` in the max norm of each output.  A skipped output is
  None and the others are bitwise what the full launch gave.  Above `tol` in
  fp32 the project's exception rule applies: the NumPy reference evaluated
  in float32, 4 times its error.  Returns [(lambda0, name, error, allowed)]."""
  E, nq = ref.num_elements, ref.Q
  rows = []
  for l0 in (0.0, 2.5):
    uq = rnd(rng.standard_normal((E, nq, ndim)))
    vq = rnd(rng.standard_normal((E, nq, ndim)))
    want = EA.grid_sens(ref, uq, vq, l0)
    padded = lambda a: _dev(np.concatenate(
        [a, rng.standard_normal((pad, nq, ndim))]), dtype)
    ud, vd = padded(uq), padded(vq)
    full = None
    for subset in SUBSETS:
      got = _ops.elasticity_sens(ud, vd, op.parts, op.host, ndim, Q,
                                 op.point_weights(), l0, want=subset)
      for n, (g, w, on) in enumerate(zip(got, want, subset)):
        if not on:
          assert g is None
          continue
        assert g.shape == (E + pad, nq) and g.dtype == dtype
        if full is not None:
          assert torch.equal(g[:E], full[n][:E]), (NAMES[n], subset)
          continue
        err = _rel(_np(g)[:E], w)
        if not l0 and n == 2:
          assert float(g[:E].abs().max()) == 0.0
        allowed = tol
        if err > tol and dtype == torch.float32:
          ref32 = EA.grid_sens(ref, uq, vq, l0, dtype=np.float32)[n]
          allowed = max(tol, 4.0 * _rel(ref32.astype(np.float64), w))
        print(f'{dtype} ndim={ndim} Q={Q} lambda0={l0} {NAMES[n]}: rel err '
              f'{err:.3e} (allowed {allowed:.3e})')
        rows.append((l0, NAMES[n], err, allowed))
        assert err <= allowed, (ndim, Q, l0, NAMES[n], err, allowed)
      if full is None:
        full = got
  return rows


@pytest.mark.parametrize('Q', range(2, 13))
@pytest.mark.parametrize('ndim', [2, 3])
def test_kernel_matches_reference(ndim, Q):
  """fp64, every Q, on multilinear and curved elements with a padded row
  (list launches, a partial workgroup)."""
  case = G.three_kinds(2, ndim, MESH_P, pad=1)
  mesh, fes, ref, op = _kernel_setup(case, Q)
  assert len(op.parts) >= 2 and all('elem_list' in p for p in op.parts)
  assert {G.CURVED, G.MULTILINEAR} <= {p['geo_mode'] for p in op.parts}
  rng = np.random.default_rng(100 * ndim + Q)
  _run_sens(op, ref, ndim, Q, 1, rng, F64, tolerance(F64, Q))


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
  _run_sens(op, ref, ndim, Q, 0, rng, F64, tolerance(F64, Q))


@pytest.mark.parametrize('Q', [2, 5, 8, 9, 12])
@pytest.mark.parametrize('ndim', [2, 3])
def test_kernel_fp32(ndim, Q):
  """fp32 with float32-representable meshes and inputs against the fp64
  reference at `tolerance(torch.float32, Q)`.  A case above that is held to
  4 times the error of the NumPy reference evaluated in float32 (DESIGN
  §3.17 lists them)."""
  case = G.three_kinds(2, ndim, MESH_P)
  mesh, fes, ref, op = _kernel_setup(case, Q, torch.float32)
  rng = F32Rng(Q)
  _run_sens(op, ref, ndim, Q, 0, rng, torch.float32,
            tolerance(torch.float32, Q), rnd=f32r)


# ------------------------------------------------ 2. kernel vs kernel
@functools.lru_cache(maxsize=None)
def _assembled(kind, ndim):
  P = 4 if ndim == 2 else 3
  case = getattr(G, kind)(2, ndim, P)
  mesh, _, rp = case.finalize(DEV, F64)
  q = P - 1 + (ndim + 1) // 2
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(q, GL))
  ref = ER.space(rp.node_coords, rp.elements, P, (q, 'gl'))
  return mesh, fes, ref, q


ASSEMBLED = [('multilinear', 2), ('curved_multilinear', 2),
             ('multilinear', 3), ('curved_multilinear', 3), ('affine', 3)]


@pytest.mark.parametrize('kind,ndim', ASSEMBLED)
def test_sensitivity_against_forward_kernel(kind, ndim):
  """The operator is linear in (lam, mu, rho): sum_q (lam dlam + mu dmu + rho
  drho) from the new kernel equals v . op.apply(u, lambda0) from the existing
  one, to `tolerance(float64, Q)` relative to |v| |A u|; sens(u, v) =
  sens(v, u); dlam = dmu = 0 for a rigid motion u (relative to the largest
  dmu of (v, v): the size of |grad v|^2 W)."""
  mesh, fes, ref, Q = _assembled(kind, ndim)
  tol = tolerance(F64, Q)
  rng = np.random.default_rng(5 + ndim)
  E, nq = mesh.num_elements, Q ** ndim
  lam, mu, rho = (_dev(0.5 + rng.random((E, nq))) for _ in range(3))
  op = fes.elasticity_operator(lame_lambda=lam, lame_mu=mu, density=rho)
  u = _dev(rng.standard_normal((mesh.num_nodes, ndim)))
  v = _dev(rng.standard_normal((mesh.num_nodes, ndim)))
  for l0 in (0.0, 1.3):
    dl, dm, dr = op.sensitivity(u, v, l0)
    assert dl.shape == dm.shape == dr.shape == (E, nq)
    Au = op.apply(u, l0)
    got = float((lam * dl + mu * dm + rho * dr).sum())
    want = float((v * Au).sum())
    scale = float(v.norm() * Au.norm())
    print(f'{kind} {ndim}D lambda0={l0}: |sum theta dtheta - v.Au| / '
          f'(|v||Au|) = {abs(got - want) / scale:.2e}')
    assert abs(got - want) <= tol * scale
    for a, b in zip((dl, dm, dr), op.sensitivity(v, u, l0)):
      assert float((a - b).abs().max()) <= tol * max(float(a.abs().max()),
                                                     1e-300)
  size = float(op.sensitivity(v, v)[1].abs().max())
  x = _np(mesh.node_coords)
  for m in EA.rigid_modes(x):
    dl, dm, _ = op.sensitivity(_dev(m), v)
    worst = max(float(dl.abs().max()), float(dm.abs().max()))
    assert worst <= tol * size * max(1.0, np.abs(m).max())


# ------------------------------------------------ 3. op.sensitivity forms
@pytest.mark.parametrize('ndim', [2, 3])
def test_operator_sensitivity_forms(ndim):
  """Scalar, (E,), (E, Q^d) and callable sources, an absent density, dense
  and component-major fields, `want` subsets: each gradient in the form of
  its source against the reference's reduction, 1e-10."""
  mesh, fes, ref, Q = _assembled('curved_multilinear', ndim)
  rng = np.random.default_rng(9 + ndim)
  E, nq = mesh.num_elements, Q ** ndim
  un = rng.standard_normal((mesh.num_nodes, ndim))
  vn = rng.standard_normal((mesh.num_nodes, ndim))
  l0 = 0.8
  want = EA.point_sensitivities(ref, un, vn, l0)
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
    op = fes.elasticity_operator(lame_lambda=src[0], lame_mu=src[1],
                                 density=src[2])
    assert op.coef_source == tuple(src)
    for fields in ((u, v), (layout.component_major(u),
                            layout.component_major(v))):
      got = op.sensitivity(*fields, l0)
      for g, w, f in zip(got, want, forms):
        if f in (None, 'callable'):
          assert g is None
          continue
        w = EA.reduce_coefficient(w, form_of[f])
        assert tuple(g.shape) == np.shape(w), f
        assert _rel(_np(g), np.asarray(w)) <= 1e-10, f
    for subset in SUBSETS[1:]:
      got = op.sensitivity(u, v, l0, want=subset)
      for g, on, f in zip(got, subset, forms):
        assert (g is not None) == (on and f not in (None, 'callable'))
  with pytest.raises(ValueError):
    op.sensitivity(u[:, 0], v)


# -------------------------------------------- 4. gradients through the solve
@functools.lru_cache(maxsize=None)
def _solve_setup(ndim, lambda0):
  """`EA.SolveProblem` on the GPU next to its dense reference, with the
  reference gradient computed once."""
  rp, _, _ = EA.AJ.solve_problem(ndim)
  mesh = rp.finalize(device=DEV)
  facets = mesh.boundary_facets['x1'].cpu().numpy().astype(np.int64)
  prob = EA.SolveProblem(ndim, lambda0, facets)
  u, gf, gl, gm, gr, cond = prob.gradients(want_cond=True)
  roller = [None] * ndim
  roller[1] = _t(prob.roll)
  bcs = {'y0': (D, tuple(roller)),
         'x0': (D, tuple(_t(g) for g in prob.gD)),
         'x1': (N, tuple(g if not callable(g) else _t(g) for g in prob.trac))}
  return dict(mesh=mesh, prob=prob, bcs=bcs, u=u, cond=cond,
              grads=dict(force=gf, lam=gl, mu=gm, rho=gr))


def _gpu_solve(s, pc, lam, mu, rho, force=None, rtol=1e-13, **kw):
  prob = s['prob']
  force = _dev(prob.force) if force is None else force
  u, info = solve_elasticity(s['mesh'], force, s['bcs'], lame_lambda=lam,
                             lame_mu=mu, density=rho, lambda0=prob.lambda0,
                             rtol=rtol, preconditioner=pc, return_info=True,
                             **kw)
  assert info['status'] == 'converged'
  return u, info


def _leaf(a):
  return _dev(a).requires_grad_(True)


@pytest.mark.parametrize('lambda0', [0.0, 1.7])
@pytest.mark.parametrize('pc', [None, 'jacobi'])
@pytest.mark.parametrize('ndim', [2, 3])
def test_solve_gradients_match_dense_adjoint(ndim, pc, lambda0):
  """`.grad` of a per-point lame_lambda, a per-element lame_mu, a scalar
  density and an (N, d) body force of the loss (w * u).sum() against the
  dense adjoint solve, on the jittered mesh with a clamped face (x0, with
  values), a roller (y0), a traction (x1) and a body force; then a (d,) body
  force.  Solves at rtol 1e-13; bound 100 cond 1e-12 relative, cond from the
  dense matrix."""
  s = _solve_setup(ndim, lambda0)
  prob = s['prob']
  bound = 100.0 * s['cond'] * 1e-12
  print(f'ndim={ndim} lambda0={lambda0}: cond {s["cond"]:.3e}, bound '
        f'{bound:.2e}')
  lam, mu, f = _leaf(prob.lam_q), _leaf(prob.mu_e), _leaf(prob.force)
  rho = torch.tensor(prob.rho, dtype=F64, device=DEV, requires_grad=True)
  u, info = _gpu_solve(s, pc, lam, mu, rho, f)
  assert u.grad_fn is not None and 'adjoint' not in info
  assert _rel(_np(u), s['u']) <= bound
  (u * _dev(prob.w)).sum().backward()
  assert info['adjoint']['status'] == 'converged'
  assert u.grad_fn.state['adjoint_info'] is info['adjoint']
  g = s['grads']
  checks = [('force', f.grad, g['force']), ('lam', lam.grad, g['lam']),
            ('mu', mu.grad, EA.reduce_coefficient(g['mu'], 'elem'))]
  for name, got, want in checks:
    assert got is not None and tuple(got.shape) == want.shape, name
    err = _rel(_np(got), want)
    print(f'  {pc} d/d{name}: rel err {err:.2e}')
    assert err <= bound, name
  assert rho.grad.shape == ()
  if lambda0:
    err = abs(float(rho.grad) - g['rho'].sum()) / np.abs(g['rho']).sum()
    print(f'  {pc} d/drho: rel err {err:.2e}')
    assert err <= bound
  else:
    assert float(rho.grad) == 0.0
  # a (d,) body force: its gradient is the nodal one summed over the nodes
  fc = _leaf(np.array([0.3, -1.0, 0.5][:ndim]))
  u, _ = _gpu_solve(s, pc, _dev(prob.lam_q), _dev(prob.mu_e), prob.rho, fc)
  (u * _dev(prob.w)).sum().backward()
  gfc = EA.solve_gradients(
      prob.dense(), prob.w, np.tile(_np(fc), (len(prob.x), 1)), prob.fixed,
      prob.values, [(prob.facets, prob.trac)], prob.lambda0)[1].sum(axis=0)
  assert fc.grad.shape == (ndim,)
  assert _rel(_np(fc.grad), gfc) <= bound


@pytest.mark.parametrize('ndim', [2, 3])
def test_central_difference_through_the_solve(ndim):
  """One central difference per coefficient (h = 1e-4, the directions of the
  host test) through the GPU solve against its own `.grad`, lambda0 = 1.7,
  Jacobi, rtol = 1e-15 (a loss known to rtol |loss| enters the quotient as
  rtol |loss| / (2 h |derivative|), `tests/test_gpu_adjoint.py`).  The dense
  reference on the same problem, directions and step sets the floor of
  truncation and rounding (`test_elasticity_adjoint_host`, which asserts it:
  2D lam 2.8e-9, mu 2.7e-9, rho 3.7e-10; 3D lam 3.0e-9, mu 6.3e-10, rho
  8.5e-9); 10 x that is allowed.  Measured on an MI355X over four runs: 2D lam
  2.6e-9, mu 2.8e-9, rho 2.7e-10 .. 3.3e-10; 3D lam 3.3e-9 .. 3.5e-9, mu
  5.8e-10 .. 7.1e-10, rho 8.2e-9 .. 8.5e-9: both sides measure the truncation
  of the quotient (`EA.CD_H`'s comment)."""
  s = _solve_setup(ndim, 1.7)
  prob = s['prob']
  cds = EA.central_differences(prob)
  lam, mu = _leaf(prob.lam_q), _leaf(prob.mu_q())
  rho = torch.tensor(prob.rho, dtype=F64, device=DEV, requires_grad=True)
  rtol = 1e-15
  w = _dev(prob.w)
  u, _ = _gpu_solve(s, 'jacobi', lam, mu, rho, rtol=rtol)
  (u * w).sum().backward()
  h = EA.CD_H
  base = dict(lam=prob.lam_q, mu=prob.mu_q(), rho=prob.rho)

  def val(**over):
    c = {k: (_dev(v) if isinstance(v, np.ndarray) else v)
         for k, v in {**base, **over}.items()}
    u, _ = _gpu_solve(s, 'jacobi', c['lam'], c['mu'], c['rho'], rtol=rtol)
    return float((u * w).sum())
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


def test_compliance_gradient():
  """Compliance C = f . u (f the load covector) with a per-element Young's
  modulus through `lame_parameters`, clamped on x0 with zero values: dC/dE
  from `.backward()` against -u^T (dK/dE) u of the reference, the
  self-adjoint case of topology optimisation."""
  ndim, nu = 2, 0.3
  rp, P, quad = EA.AJ.solve_problem(ndim)
  mesh = rp.finalize(device=DEV)
  x = np.asarray(rp.node_coords, np.float64)
  ref = ER.space(x, rp.elements, P, (quad, 'gl'))
  E, nq = ref.num_elements, ref.Q
  rng = np.random.default_rng(21)
  young = 1.0 + rng.random(E)
  lam_e, mu_e = operators.lame_parameters(young, nu)
  expand = lambda c: EA.expand_coefficient(c, E, nq)
  dense = ER.Dense(rp, P, expand(lam_e), expand(mu_e))
  force = np.tile([0.0, -1.0], (len(x), 1))
  fixed = np.zeros(x.shape, bool)
  fixed[np.abs(x[:, 0]) < 1e-9] = True
  load = (dense.B @ force.reshape(-1)).reshape(x.shape)
  u_ref, _, gl, gm, _, cond = EA.solve_gradients(
      dense, load, force, fixed, 0.0 * x, want_cond=True)
  # lam = u here, so the gradient is -u^T (dK/dE) u
  dl, dm, _ = EA.point_sensitivities(ref, u_ref, u_ref, 0.0)
  assert _rel(gl, -dl) <= 1e-9 and _rel(gm, -dm) <= 1e-9
  want = -(dl.sum(1) * nu / ((1 + nu) * (1 - 2 * nu)) +
           dm.sum(1) / (2 * (1 + nu)))
  bound = 100.0 * cond * 1e-12
  Et = _leaf(young)
  lam_t, mu_t = operators.lame_parameters(Et, nu)
  u = solve_elasticity(mesh, (0.0, -1.0), {'x0': (D, (0.0, 0.0))},
                       lame_lambda=lam_t, lame_mu=mu_t, rtol=1e-13,
                       preconditioner='jacobi')
  C = (u * _dev(load)).sum()
  C.backward()
  assert (want < 0).all()            # stiffer elements, less compliance
  err = _rel(_np(Et.grad), want)
  print(f'compliance: dC/dE rel err {err:.2e} (bound {bound:.2e})')
  assert err <= bound


def test_point_observations():
  """A least-squares loss on `mesh.point_evaluator(points)(u)` at a handful of
  sensors, differentiated to a per-element lame_mu: against the dense adjoint
  solve with the cotangent the evaluator's transpose gives."""
  s = _solve_setup(2, 0.0)
  prob = s['prob']
  bound = 100.0 * s['cond'] * 1e-12
  pts = _dev([[0.21, 0.33], [0.5, 0.5], [0.77, 0.12], [0.9, 0.95],
              [0.34, 0.81]])
  ev = s['mesh'].point_evaluator(pts)
  obs = _dev(0.01 * np.arange(10.0).reshape(5, 2))
  mu = _leaf(prob.mu_e)
  u, _ = _gpu_solve(s, 'jacobi', _dev(prob.lam_q), mu, prob.rho)
  misfit = ev(u) - obs
  (0.5 * (misfit ** 2).sum()).backward()
  w = _np(ev.transpose(misfit.detach()))
  gm = EA.solve_gradients(prob.dense(), w, prob.force, prob.fixed, prob.values,
                          [(prob.facets, prob.trac)], prob.lambda0)[3]
  err = _rel(_np(mu.grad), gm.sum(axis=1))
  print(f'point observations: d/dmu rel err {err:.2e} (bound {bound:.2e})')
  assert err <= bound


def test_lame_parameters_chain_through_the_solve():
  """Scalars E, nu that require grad reach `solve_elasticity` through
  `lame_parameters` and receive gradients."""
  s = _solve_setup(2, 0.0)
  prob = s['prob']
  young = torch.tensor(2.0, dtype=F64, device=DEV, requires_grad=True)
  nu = torch.tensor(0.3, dtype=F64, device=DEV, requires_grad=True)
  lam, mu = operators.lame_parameters(young, nu)
  u, _ = _gpu_solve(s, 'jacobi', lam, mu, None)
  (u * _dev(prob.w)).sum().backward()
  E, nq = prob.lam_q.shape
  lam0, mu0 = (float(t.detach()) for t in (lam, mu))
  _, _, gl, gm, _, cond = EA.solve_gradients(
      prob.dense(np.full((E, nq), lam0), np.full((E, nq), mu0), 1.0), prob.w,
      prob.force, prob.fixed, prob.values, [(prob.facets, prob.trac)],
      prob.lambda0, want_cond=True)
  n = 0.3
  want_E = gl.sum() * n / ((1 + n) * (1 - 2 * n)) + gm.sum() / (2 * (1 + n))
  scale = abs(gl.sum()) * n / ((1 + n) * (1 - 2 * n)) + \
      abs(gm.sum()) / (2 * (1 + n))
  assert abs(float(young.grad) - want_E) <= 100.0 * cond * 1e-12 * scale
  assert nu.grad is not None and nu.grad.shape == ()


# ------------------------------------------------------ 5. unchanged behaviour
def test_forward_result_unchanged_and_no_node_without_grad(monkeypatch):
  """With no input requiring grad, or under `torch.no_grad()`, the body runs
  as before and no autograd node is made.  With grad-requiring inputs the
  node hands the body the detached inputs and returns bitwise what it
  computed (within one call); two calls are compared to what their tolerance
  allows, 2 cond rtol (shared nodes and inner products are summed with
  atomics, so identical calls already differ in the last bits)."""
  body = el._solve
  seen = []

  def recording(mesh, force, bcs, **kw):
    out = body(mesh, force, bcs, **kw)
    seen.append((force, kw, out, out[0].clone() if isinstance(out, tuple)
                 else out.clone()))
    return out
  monkeypatch.setattr(el, '_solve', recording)
  for lambda0 in (0.0, 1.7):
    s = _solve_setup(2, lambda0)
    prob = s['prob']
    bound = 2.0 * s['cond'] * 1e-13
    lam, mu = _dev(prob.lam_q), _dev(prob.mu_e)
    del seen[:]
    plain, _ = _gpu_solve(s, 'jacobi', lam, mu, prob.rho)
    assert plain.grad_fn is None and not plain.requires_grad
    assert len(seen) == 1 and seen[0][2][0] is plain
    assert '_state' not in seen[0][1]
    lg, fg = _leaf(prob.lam_q), _leaf(prob.force)
    del seen[:]
    tracked, _ = _gpu_solve(s, 'jacobi', lg, mu, prob.rho, fg)
    assert tracked.grad_fn is not None and len(seen) == 1
    force, kw, _, u_body = seen[0]
    assert not force.requires_grad and torch.equal(force, fg.detach())
    assert not kw['lame_lambda'].requires_grad
    assert torch.equal(kw['lame_lambda'], lam)
    assert torch.equal(kw['lame_mu'], mu) and kw['density'] == prob.rho
    assert torch.equal(tracked.detach(), u_body)
    err = _rel(_np(tracked), _np(plain))
    print(f'lambda0={lambda0}: tracked vs plain call {err:.2e}, bound '
          f'{bound:.2e}')
    assert err <= bound
    del seen[:]
    with torch.no_grad():
      quiet, _ = _gpu_solve(s, 'jacobi', lg, mu, prob.rho)
    assert quiet.grad_fn is None and '_state' not in seen[0][1]
    assert _rel(_np(quiet), _np(plain)) <= bound


# ----------------------------------------------------------------- 6. refusals
def test_refusals():
  """`op.apply` on a field that requires grad still raises; periodic,
  partitioned and ensemble meshes and 'pmg' raise with grad as without."""
  from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
  from swirl_fem_amd.core.interpolation import Nodes1D
  from swirl_fem_amd.core.mesh_refiner import refine_premesh
  from swirl_fem_amd.distributed import blocks
  mesh, fes, ref, Q = _assembled('affine', 3)
  op = fes.elasticity_operator(lame_lambda=1.0, lame_mu=1.0)
  u = torch.zeros((mesh.num_nodes, 3), dtype=F64, device=DEV)
  with pytest.raises(NotImplementedError, match='autograd'):
    op.apply(u.clone().requires_grad_(True))
  with pytest.raises(NotImplementedError, match='autograd'):
    op.apply_local(_ops.gather_rows(u, mesh.elements).requires_grad_(True))
  ok = dict(lame_lambda=1.0)
  grad_mu = lambda: torch.tensor(1.0, dtype=F64, device=DEV,
                                 requires_grad=True)
  pm = unit_cube_mesh(3, ndim=2, periodic_dims=(0,))
  periodic = refine_premesh(pm, Nodes1D.create(4, GLL)).finalize(device=DEV)
  part = blocks.build_block_partition(2, 3, (2, 1, 1), 0, device='cpu')
  plain = refine_premesh(unit_cube_mesh(2, ndim=2),
                         Nodes1D.create(3, GLL)).finalize(device=DEV)
  for bad, d, what in ((periodic, 2, 'periodic'), (part.mesh, 3, 'partitioned'),
                       (plain.replicate(2), 2, 'ensemble')):
    for mu in (1.0, grad_mu()):
      with pytest.raises(NotImplementedError, match=what):
        solve_elasticity(bad, (0.0,) * d, {}, lambda0=1.0, lame_mu=mu, **ok)
  for mu in (1.0, grad_mu()):
    with pytest.raises(NotImplementedError, match='pmg'):
      solve_elasticity(plain, (0.0, 0.0), {}, lambda0=1.0, lame_mu=mu,
                       preconditioner='pmg', **ok)
  # the wrapper's own checks
  E, nq = mesh.num_elements, Q ** 3
  z = torch.zeros((E, nq, 3), dtype=F64, device=DEV)
  with pytest.raises(ValueError, match='want'):
    _ops.elasticity_sens(z, z, op.parts, op.host, 3, Q, op.point_weights(),
                         want=(False, False, False))
  with pytest.raises(ValueError):
    _ops.elasticity_sens(z, z[:, :, :2], op.parts, op.host, 3, Q,
                         op.point_weights())
  with pytest.raises(_lib.SfemError, match='status -3'):
    _ops.elasticity_sens(z[:, :1].expand(E, 13 ** 3, 3), z[:, :1].expand(
        E, 13 ** 3, 3), op.parts, op.host, 3, 13, op.point_weights()[
            :, :1].expand(E, 13 ** 3))


def test_entry_point_refusals():
  """Status codes of the raw entry point: one valid call, then one field
  wrong at a time; nothing that is refused launches."""
  case = G.affine(2, 3, MESH_P)
  mesh, _, rp = case.finalize(DEV, F64)
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(4, GL))
  op = fes.elasticity_operator(lame_lambda=1.0, lame_mu=1.0)
  part, = op.parts
  assert part['geo_mode'] == _lib.GEO_AFFINE
  E, nq = mesh.num_elements, 64
  z = lambda *s: torch.zeros(s, dtype=F64, device=DEV)
  keep = dict(u=z(E, nq, 3), v=z(E, nq, 3), dl=z(E, nq), dm=z(E, nq),
              dr=z(E, nq), lst=torch.zeros(E, dtype=torch.int32, device=DEV),
              host={k: _ops._host(v, F64) for k, v in op.host.items()})
  lst = keep['lst'].data_ptr()
  lib = _lib.load()

  def call(**over):
    a = _lib.ElasticitySensArgs(
        u=keep['u'].data_ptr(), v=keep['v'].data_ptr(),
        wdet=op.point_weights().data_ptr(), dlam=keep['dl'].data_ptr(),
        dmu=keep['dm'].data_ptr(), drho=keep['dr'].data_ptr(), lambda0=1.0,
        **_ops._launch_fields(part, keep['host'], 'kfac'), num_elements=E,
        ndim=3, P=4, dtype=_lib.SFEM_F64)
    for k, v in over.items():
      setattr(a, k, v)
    return lib.sfem_elasticity_sens(ctypes.byref(a), None)

  assert call() == 0
  torch.cuda.synchronize()
  assert call(dlam=None, drho=None) == 0 and call(dlam=None, dmu=None) == 0
  torch.cuda.synchronize()
  # outside the compiled range: SFEM_EUNSUPPORTED
  for over in (dict(P=13), dict(P=1), dict(ndim=1), dict(ndim=4),
               dict(geo_mode=_lib.GEO_BOX), dict(geo_mode=7)):
    assert call(**over) == -3, over
  # a missing required pointer or no output at all: SFEM_EINVAL
  for over in (dict(u=None), dict(v=None), dict(wdet=None), dict(dmat=None),
               dict(dlam=None, dmu=None, drho=None), dict(geo_elem=None),
               dict(weights=None), dict(nodes=None),
               dict(geo_mode=_lib.GEO_POINT), dict(dtype=5),
               dict(num_elements=-1),
               dict(elem_list=lst, num_listed=E + 1),
               dict(elem_list=lst, num_listed=-1)):
    assert call(**over) == -1, over
  assert lib.sfem_elasticity_sens(None, None) == -1
  assert call(dlam=None, dmu=None, drho=None) == -1
  msg = lib.sfem_last_error().decode(errors='replace')
  assert 'sfem_elasticity_sens' in msg and 'output' in msg
  # nothing to do is not an error
  assert call(num_elements=0, u=None, v=None) == 0
