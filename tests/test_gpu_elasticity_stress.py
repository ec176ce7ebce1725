"""Stress recovery of elasticity solves on the GPU: the kernels
`sfem_elasticity_stress` / `sfem_elasticity_stress_vjp` at every Q = 2..12
against the NumPy reference (`tests/elasticity_stress_reference.py`) and
against each other and the forward operator kernel, `ElasticityOperator.stress`
in every mode, `recover_stress` after `solve_elasticity` against analytic
stresses, `.grad` of stress functionals through solve and recovery against the
dense adjoint and a central difference, point values, the unchanged path
without grad and the refusals."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from swirl_fem_amd import _lib, _ops
from swirl_fem_amd.core import layout, operators
from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import NodeType, Quadrature1D
from swirl_fem_amd.examples.elasticity import (BCType, recover_stress,
                                               solve_elasticity)
from tests import elasticity_adjoint_reference as EA
from tests import elasticity_reference as ER
from tests import elasticity_stress_reference as SR
from tests import geometry_cases as G
from tests.fp32util import F32Rng, f32r, tolerance

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64 = torch.float64
GLL, GL = NodeType.GAUSS_LOBATTO_LEGENDRE, NodeType.GAUSS_LEGENDRE
D, N = BCType.DIRICHLET, BCType.NEUMANN
MESH_P = 3       # nodes per direction of the kernel tests' meshes
FWD_NAMES = ('sigma', 'vm')
VJP_NAMES = ('ubar', 'dlam', 'dmu')


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


# ------------------------------------------------ 1. kernels vs reference
def _kernel_setup(case, Q, dtype=F64):
  mesh, _, rp = case.finalize(DEV, dtype)
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(Q, GL))
  ref = ER.space(rp.node_coords, rp.elements, MESH_P, (Q, 'gl'))
  op = fes.elasticity_operator(lame_lambda=1.0, lame_mu=1.0)
  return mesh, fes, ref, op


FWD_SUBSETS = [(True, True), (True, False), (False, True)]
VJP_SUBSETS = [(True, True, True), (True, False, False), (False, True, False),
               (False, False, True)]


def _check_outputs(launch, subsets, names, want, ref32, E, tol, dtype, tag):
  """Every output together and each alone against `want` in the max norm of
  each output.  A skipped output is None, the others are bitwise what the full
  launch gave, and rows past E (padding) are exact zeros.  Above `tol` in fp32
  the project's exception rule applies: the NumPy reference evaluated in
  float32 (`ref32()`), 4 times its error."""
  full = None
  for subset in subsets:
    got = launch(subset)
    for n, (g, w, on) in enumerate(zip(got, want, subset)):
      if not on:
        assert g is None, (tag, names[n], subset)
        continue
      assert g.dtype == dtype and tuple(g.shape[1:]) == w.shape[1:]
      assert float(g[E:].abs().sum()) == 0.0, (tag, names[n], 'padding')
      if full is not None:
        assert torch.equal(g, full[n]), (tag, names[n], subset)
        continue
      err = _rel(_np(g)[:E], w)
      allowed = tol
      if err > tol and dtype == torch.float32:
        allowed = max(tol, 4.0 * _rel(ref32()[n].astype(np.float64), w))
      print(f'{tag} {names[n]}: rel err {err:.3e} (allowed {allowed:.3e})')
      assert err <= allowed, (tag, names[n], err, allowed)
    if full is None:
      full = got


def _run_kernels(op, ref, ndim, Q, pad, rng, dtype, tol, rnd=lambda a: a):
  """Both kernels with per-point and with scalar lam / mu, in 2D with
  `plane_stress` off and on."""
  E, nq, nv = ref.num_elements, ref.Q, SR.num_slots(ndim)
  W = op.point_weights()
  assert tuple(W.shape) == (E + pad, nq)
  if pad:
    assert float(W[E:].abs().max()) == 0.0
  np_dt = np.float64 if dtype == F64 else np.float32
  padded = lambda a: _dev(np.concatenate(
      [a, rnd(rng.standard_normal((pad,) + a.shape[1:]))]), dtype)
  for coefs in ('point', 'scalar'):
    if coefs == 'point':
      lam = rnd(0.5 + rng.random((E, nq)))
      mu = rnd(0.5 + rng.random((E, nq)))
      lam_d, mu_d = (_dev(np.concatenate([c, np.ones((pad, nq))]), dtype)
                     for c in (lam, mu))
    else:
      lam = lam_d = 1.25
      mu = mu_d = 0.75
    for ps in ((False, True) if ndim == 2 else (False,)):
      tag = f'{dtype} ndim={ndim} Q={Q} {coefs} plane_stress={ps}:'
      uq = rnd(rng.standard_normal((E, nq, ndim)))
      sbar = rnd(rng.standard_normal((E, nq, nv)))
      ud, sd = padded(uq), padded(sbar)
      sig = SR.grid_stress(ref, uq, lam, mu, ps)

      def fwd32():
        s = SR.grid_stress(ref, uq, lam, mu, ps, dtype=np_dt)
        return s, SR.von_mises(s)
      _check_outputs(
          lambda want: _ops.elasticity_stress(
              ud, op.parts, op.host, ndim, Q, W, lam_d, mu_d, want=want,
              plane_stress=ps),
          FWD_SUBSETS, FWD_NAMES, (sig, SR.von_mises(sig)), fwd32, E, tol,
          dtype, tag)
      _check_outputs(
          lambda want: _ops.elasticity_stress_vjp(
              sd, ud, op.parts, op.host, ndim, Q, W, lam_d, mu_d, want=want,
              plane_stress=ps),
          VJP_SUBSETS, VJP_NAMES,
          SR.grid_stress_vjp(ref, sbar, uq, lam, mu, ps),
          lambda: SR.grid_stress_vjp(ref, sbar, uq, lam, mu, ps, dtype=np_dt),
          E, tol, dtype, tag)
      # ubar alone needs no displacement
      alone = [_ops.elasticity_stress_vjp(
          sd, x, op.parts, op.host, ndim, Q, W, lam_d, mu_d,
          want=(True, False, False), plane_stress=ps)[0] for x in (ud, None)]
      assert torch.equal(*alone)


@pytest.mark.parametrize('Q', range(2, 13))
@pytest.mark.parametrize('ndim', [2, 3])
def test_kernels_match_reference(ndim, Q):
  """fp64, every Q, on multilinear and curved elements with a padded row
  (list launches, a partial workgroup)."""
  case = G.three_kinds(2, ndim, MESH_P, pad=1)
  mesh, fes, ref, op = _kernel_setup(case, Q)
  assert len(op.parts) >= 2 and all('elem_list' in p for p in op.parts)
  assert {G.CURVED, G.MULTILINEAR} <= {p['geo_mode'] for p in op.parts}
  rng = np.random.default_rng(100 * ndim + Q)
  _run_kernels(op, ref, ndim, Q, 1, rng, F64, tolerance(F64, Q))


@pytest.mark.parametrize('Q', range(2, 13))
@pytest.mark.parametrize('ndim', [2, 3])
def test_kernels_affine_elements(ndim, Q):
  """The affine instantiations at every Q (one launch over all elements, no
  list)."""
  case = G.affine(2, ndim, MESH_P)
  mesh, fes, ref, op = _kernel_setup(case, Q)
  assert [p['geo_mode'] for p in op.parts] == [G.AFFINE]
  assert 'elem_list' not in op.parts[0]
  rng = np.random.default_rng(7 * ndim + Q)
  _run_kernels(op, ref, ndim, Q, 0, rng, F64, tolerance(F64, Q))


@pytest.mark.parametrize('Q', [2, 5, 8, 9, 12])
@pytest.mark.parametrize('ndim', [2, 3])
def test_kernels_fp32(ndim, Q):
  """fp32 with float32-representable meshes and inputs against the fp64
  reference at `tolerance(torch.float32, Q)`.  A case above that is held to
  4 times the error of the NumPy reference evaluated in float32 (DESIGN
  §3.18 lists them)."""
  case = G.three_kinds(2, ndim, MESH_P)
  mesh, fes, ref, op = _kernel_setup(case, Q, torch.float32)
  rng = F32Rng(Q)
  _run_kernels(op, ref, ndim, Q, 0, rng, torch.float32,
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
def test_kernels_against_each_other(kind, ndim):
  """On the GPU alone, to `tolerance(float64, Q)`: B^T W sigma = K u, the vjp
  kernel at lam = 0, mu = 1/2 (the bare transposed symmetric gradient) on the
  work-conjugate cotangent of W sigma(u) (shear slots doubled, 2D zz slot
  zero: `SR.work_conjugate`) equals `_ops.elasticity_local(u, lambda0=0)`;
  the adjoint identity <sbar, sigma(u)> = <ubar, u>; the linearity identity
  sum_q (lam dlam + mu dmu) = <sbar, sigma(u)>."""
  mesh, fes, ref, Q = _assembled(kind, ndim)
  tol = tolerance(F64, Q)
  rng = np.random.default_rng(5 + ndim)
  E, nq, nv = mesh.num_elements, Q ** ndim, SR.num_slots(ndim)
  lam, mu = (_dev(0.5 + rng.random((E, nq))) for _ in range(2))
  op = fes.elasticity_operator(lame_lambda=lam, lame_mu=mu)
  W = op.point_weights()
  uq = _dev(rng.standard_normal((E, nq, ndim)))
  sbar = _dev(rng.standard_normal((E, nq, nv)))
  args = (op.parts, op.host, ndim, Q, W)
  for ps in ((False, True) if ndim == 2 else (False,)):
    sig = _ops.elasticity_stress(uq, *args, lam, mu, plane_stress=ps)[0]
    ws = sig * W[..., None]
    wc = _dev(SR.work_conjugate(_np(ws)))
    bt = _ops.elasticity_stress_vjp(wc, None, *args, 0.0, 0.5,
                                    want=(True, False, False))[0]
    Ku = _ops.elasticity_local(uq, *args, lam, mu)
    err = float((bt - Ku).abs().max() / Ku.abs().max())
    print(f'{kind} {ndim}D plane_stress={ps}: B^T W sigma vs K u {err:.2e}')
    assert err <= tol
    ub, dl, dm = _ops.elasticity_stress_vjp(sbar, uq, *args, lam, mu,
                                            plane_stress=ps)
    pair = float((sbar * sig).sum())
    scale = float(sbar.norm() * sig.norm())
    assert abs(pair - float((ub * uq).sum())) <= tol * scale
    assert abs(pair - float((lam * dl + mu * dm).sum())) <= tol * scale


# ------------------------------------------------ 3. operator
@pytest.mark.parametrize('kind,ndim', [('curved_multilinear', 2),
                                       ('curved_multilinear', 3),
                                       ('affine', 3)])
def test_operator_stress_modes(kind, ndim):
  """`op.stress` for dense and component-major displacements, at quadrature
  points and at nodes with both recoveries, against the dense reference
  (1e-10; 'l2' 1e-9: one CG solve per column at rtol 1e-12 on a mass matrix
  of condition < 1e3); the fused von Mises output against
  `operators.von_mises(sigma)` (a few roundings: 1e-13); nodal von Mises is
  `von_mises` of the nodal stress; `stress_local` is the quadrature route."""
  mesh, fes, ref, Q = _assembled(kind, ndim)
  rng = np.random.default_rng(9 + ndim)
  E, nq = mesh.num_elements, Q ** ndim
  lam, mu = 0.5 + rng.random((E, nq)), 0.5 + rng.random(E)
  mu_q = EA.expand_coefficient(mu, E, nq)
  op = fes.elasticity_operator(lame_lambda=_dev(lam), lame_mu=_dev(mu))
  un = rng.standard_normal((mesh.num_nodes, ndim))
  u = _dev(un)
  for ps in ((False, True) if ndim == 2 else (False,)):
    sq = SR.point_stress(ref, ref.gather(un), lam, mu_q, ps)
    for field in (u, layout.component_major(u)):
      got, vm = op.stress(field, at='quadrature', von_mises=True,
                          plane_stress=ps)
      assert got.grad_fn is None and tuple(got.shape) == sq.shape
      assert _rel(_np(got), sq) <= 1e-10
      assert _rel(_np(vm), _np(operators.von_mises(got, ndim))) <= 1e-13
      assert torch.equal(got, op.stress(field, at='quadrature',
                                        plane_stress=ps))
      for recovery, bound in (('lumped', 1e-10), ('l2', 1e-9)):
        want = (SR.lumped_recovery if recovery == 'lumped'
                else SR.l2_recovery)(ref, sq)
        sn, vn = op.stress(field, recovery=recovery, von_mises=True,
                           plane_stress=ps)
        assert tuple(sn.shape) == want.shape
        err = _rel(_np(sn), want)
        print(f'{kind} {ndim}D {recovery} plane_stress={ps}: {err:.2e}')
        assert err <= bound
        assert torch.equal(vn, operators.von_mises(sn, ndim))
    loc = op.stress_local(_ops.gather_rows(u, mesh.elements), plane_stress=ps)
    assert torch.equal(loc, op.stress(u, at='quadrature', plane_stress=ps))
  assert float(op._lumped_weights().min()) > 0
  assert _rel(_np(op._lumped_weights()), SR.lumped_weights(ref)) <= 1e-12


@pytest.mark.parametrize('ndim', [2, 3])
def test_composed_route_matches_kernel(ndim):
  """What a user had before: `fes._basis` with gradients (the stored
  (E, Q^d, d, d) tensor) and torch arithmetic, against the kernel."""
  mesh, fes, ref, Q = _assembled('curved_multilinear', ndim)
  rng = np.random.default_rng(13 + ndim)
  lam, mu = 1.3, 0.6
  op = fes.elasticity_operator(lame_lambda=lam, lame_mu=mu)
  u = _dev(rng.standard_normal((mesh.num_nodes, ndim)))
  _, grad = fes._basis(_ops.gather_rows(u, mesh.elements), False, True)
  H = grad.transpose(-1, -2)                  # [e, q, c, j] = d u_c / d x_j
  tr = H.diagonal(dim1=-2, dim2=-1).sum(-1)
  S = lam * tr[..., None, None] * torch.eye(ndim, dtype=F64, device=DEV) + \
      mu * (H + H.transpose(-1, -2))
  if ndim == 3:
    want = torch.stack([S[..., 0, 0], S[..., 1, 1], S[..., 2, 2],
                        S[..., 0, 1], S[..., 0, 2], S[..., 1, 2]], dim=-1)
  else:
    want = torch.stack([S[..., 0, 0], S[..., 1, 1], S[..., 0, 1], lam * tr],
                       dim=-1)
  got = op.stress(u, at='quadrature')
  assert _rel(_np(got), _np(want)) <= 1e-11


# ------------------------------------------------ 4. solves
def _tension_bcs(ndim, t):
  bcs = {}
  for a, name in enumerate(['x0', 'y0', 'z0'][:ndim]):
    entries = [None] * ndim
    entries[a] = 0.0
    bcs[name] = (D, tuple(entries))
  bcs['x1'] = (N, (t,) + (None,) * (ndim - 1))
  return bcs


@pytest.mark.parametrize('ndim,ps', [(2, False), (3, False), (2, True)])
def test_tension_stress(ndim, ps):
  """Uniaxial tension (and its plane-stress form) of
  `tests/test_gpu_elasticity.py` through `solve_elasticity` +
  `recover_stress`: sigma_xx = t, sigma_zz = nu t in plane strain, all else
  zero, at quadrature points and at nodes by both recoveries, with von Mises.
  Against the dense reference's stress under the solver bound 100 cond 1e-12
  (rtol 1e-13); against the analytic stress 10 times the dense reference's
  own error on the problem (`test_tension_reference_stress` on the host:
  below 3e-14), never below the solver bound."""
  rp, P, (lam, mu), t, u_ref, want, cond = SR.tension_problem(ndim, ps)
  mesh = rp.finalize(device=DEV)
  fes = ER.Dense(rp, P, lam, mu).fes
  sq_ref = SR.point_stress(fes, fes.gather(u_ref), lam, mu, ps)
  solver = 100.0 * cond * 1e-12
  ref_err = max(np.abs(sq_ref - want).max(),
                np.abs(SR.lumped_recovery(fes, sq_ref) - want).max()) / t
  bound = max(10.0 * ref_err, solver)
  u = solve_elasticity(mesh, (0.0,) * ndim, _tension_bcs(ndim, t),
                       lame_lambda=lam, lame_mu=mu, rtol=1e-13,
                       preconditioner='jacobi')
  kw = dict(lame_lambda=lam, lame_mu=mu, plane_stress=ps)
  sq, vq = recover_stress(mesh, u, at='quadrature', von_mises=True, **kw)
  err = _rel(_np(sq), sq_ref)
  print(f'tension {ndim}D plane_stress={ps}: vs dense {err:.2e} (bound '
        f'{solver:.2e}), reference vs analytic {ref_err:.2e}')
  assert err <= solver
  vm_want = float(SR.von_mises(want))
  assert np.abs(_np(sq) - want).max() <= bound * t
  assert np.abs(_np(vq) - vm_want).max() <= bound * t
  for recovery in ('lumped', 'l2'):
    sn, vn = recover_stress(mesh, u, recovery=recovery, von_mises=True, **kw)
    assert tuple(sn.shape) == (mesh.num_nodes, SR.num_slots(ndim))
    assert np.abs(_np(sn) - want).max() <= bound * t, recovery
    assert np.abs(_np(vn) - vm_want).max() <= bound * t, recovery


def test_manufactured_solution_stress_converges():
  """The manufactured solution of `tests/test_gpu_elasticity.py` at orders 3,
  5, 7: the maximum nodal stress error of both recoveries decreases strictly
  with the order."""
  lam, mu = 1.5, 0.8

  def exact(y):
    return np.stack([np.sin(2 * y[:, 0]) * np.cos(y[:, 1]),
                     np.cos(y[:, 0]) * np.sin(3 * y[:, 1])], axis=-1)

  def gradient(y):
    X, Y = y[:, 0], y[:, 1]
    H = np.zeros((len(y), 2, 2))
    H[:, 0, 0] = 2 * np.cos(2 * X) * np.cos(Y)
    H[:, 0, 1] = -np.sin(2 * X) * np.sin(Y)
    H[:, 1, 0] = -np.sin(X) * np.sin(3 * Y)
    H[:, 1, 1] = 3 * np.cos(X) * np.cos(3 * Y)
    return H

  def force(y):
    X, Y = y[:, 0], y[:, 1]
    f1 = (lam + mu) * (4 * np.sin(2 * X) * np.cos(Y) +
                       3 * np.sin(X) * np.cos(3 * Y)) + \
        5 * mu * np.sin(2 * X) * np.cos(Y)
    f2 = (lam + mu) * (2 * np.cos(2 * X) * np.sin(Y) +
                       9 * np.cos(X) * np.sin(3 * Y)) + \
        10 * mu * np.cos(X) * np.sin(3 * Y)
    return np.stack([f1, f2], axis=-1)
  errs = {'lumped': [], 'l2': []}
  for order in (3, 5, 7):
    rp = ER.jittered_box(2, 2, order + 1)
    mesh = rp.finalize(device=DEV)
    x = np.asarray(rp.node_coords, np.float64)
    comp = lambda c: _t(lambda y: exact(y)[:, c])
    bcs = {g: (D, (comp(0), comp(1))) for g in ('x0', 'x1', 'y0', 'y1')}
    u = solve_elasticity(mesh, _t(force), bcs, lame_lambda=lam, lame_mu=mu,
                         rtol=1e-12, preconditioner='jacobi')
    want = SR._stress_of(gradient(x), np.float64(lam), np.float64(mu), False)
    for recovery in errs:
      sn = recover_stress(mesh, u, lame_lambda=lam, lame_mu=mu,
                          recovery=recovery)
      errs[recovery].append(np.abs(_np(sn) - want).max())
  print(f'manufactured solution, nodal stress error at orders 3, 5, 7: {errs}')
  for e in errs.values():
    assert e[0] > e[1] > e[2]


# -------------------------------------------- 5. gradients through the solve
@functools.lru_cache(maxsize=None)
def _solve_setup(ndim):
  """`EA.SolveProblem` (lambda0 = 0) on the GPU next to its dense reference."""
  rp, _, _ = EA.AJ.solve_problem(ndim)
  mesh = rp.finalize(device=DEV)
  facets = mesh.boundary_facets['x1'].cpu().numpy().astype(np.int64)
  prob = EA.SolveProblem(ndim, 0.0, facets)
  roller = [None] * ndim
  roller[1] = _t(prob.roll)
  bcs = {'y0': (D, tuple(roller)),
         'x0': (D, tuple(_t(g) for g in prob.gD)),
         'x1': (N, tuple(g if not callable(g) else _t(g) for g in prob.trac))}
  return dict(mesh=mesh, prob=prob, bcs=bcs,
              W=_dev(ER._wdet(prob.fes)), m=_dev(SR.lumped_weights(prob.fes)))


@functools.lru_cache(maxsize=None)
def _reference_gradients(ndim, where, scalar=False):
  s = _solve_setup(ndim)
  prob = s['prob']
  dense = prob.dense()
  if scalar:
    E, nq = prob.lam_q.shape
    dense = prob.dense(np.full((E, nq), 1.4), np.full((E, nq), 0.9))
  return SR.functional_gradients(
      dense, where, prob.force, prob.fixed, prob.values,
      [(prob.facets, prob.trac)], 0.0, want_cond=True)


def _gpu_functional(s, where, pc, lam, mu, force=None, rtol=1e-13):
  """J of `SR._functional` through `solve_elasticity` + `recover_stress`."""
  prob, mesh = s['prob'], s['mesh']
  force = _dev(prob.force) if force is None else force
  u, info = solve_elasticity(mesh, force, s['bcs'], lame_lambda=lam,
                             lame_mu=mu, rtol=rtol, preconditioner=pc,
                             return_info=True)
  assert info['status'] == 'converged'
  kw = dict(lame_lambda=lam, lame_mu=mu, von_mises=True)
  if where == 'quadrature':
    _, vm = recover_stress(mesh, u, at='quadrature', **kw)
    return (s['W'] * vm ** 2).sum()
  _, vm = recover_stress(mesh, u, **kw)
  return (s['m'] * vm ** 2).sum()


@pytest.mark.parametrize('where', ['quadrature', 'nodes'])
@pytest.mark.parametrize('pc', [None, 'jacobi'])
@pytest.mark.parametrize('ndim', [2, 3])
def test_functional_gradients_match_dense_adjoint(ndim, pc, where):
  """`.grad` of J = sum_q W vm^2 and of J = sum_i m_i vm_i^2 through
  `solve_elasticity` + `recover_stress` on the problem of
  `test_gpu_elasticity_adjoint` (clamped face, roller, traction, body force)
  with respect to a per-point lame_lambda, a per-element lame_mu and the body
  force, then to scalar lame_lambda and lame_mu, against
  `SR.functional_gradients`.  Solves at rtol 1e-13; bound 100 cond 1e-12
  relative, cond from the dense matrix."""
  s = _solve_setup(ndim)
  prob = s['prob']
  J_ref, _, gf, gl, gm, cond = _reference_gradients(ndim, where)
  bound = 100.0 * cond * 1e-12
  lam, mu, f = _leaf(prob.lam_q), _leaf(prob.mu_e), _leaf(prob.force)
  J = _gpu_functional(s, where, pc, lam, mu, f)
  assert abs(float(J.detach()) - J_ref) <= bound * abs(J_ref)
  J.backward()
  for name, got, want in (('force', f.grad, gf), ('lam', lam.grad, gl),
                          ('mu', mu.grad, EA.reduce_coefficient(gm, 'elem'))):
    assert got is not None and tuple(got.shape) == want.shape, name
    err = _rel(_np(got), want)
    print(f'ndim={ndim} {where} {pc} d/d{name}: rel err {err:.2e} (bound '
          f'{bound:.2e})')
    assert err <= bound, name
  # scalar forms
  J_ref, _, _, gl, gm, cond = _reference_gradients(ndim, where, True)
  bound = 100.0 * cond * 1e-12
  lam0 = torch.tensor(1.4, dtype=F64, device=DEV, requires_grad=True)
  mu0 = torch.tensor(0.9, dtype=F64, device=DEV, requires_grad=True)
  J = _gpu_functional(s, where, pc, lam0, mu0)
  assert abs(float(J.detach()) - J_ref) <= bound * abs(J_ref)
  J.backward()
  for name, got, want in (('lam', lam0.grad, gl), ('mu', mu0.grad, gm)):
    assert got.shape == ()
    err = abs(float(got) - want.sum()) / np.abs(want).sum()
    print(f'ndim={ndim} {where} {pc} scalar d/d{name}: rel err {err:.2e}')
    assert err <= bound, name


@pytest.mark.parametrize('ndim', [2, 3])
def test_gradient_with_respect_to_displacement(ndim):
  """`recover_stress` on a leaf `u`: the gradient of <sbar, sigma_q(u)> is
  scatter(I^T ubar) with ubar of `SR.grid_stress_vjp`; of <c, sigma_N(u)>
  (lumped) it follows through the recovery's transpose.  1e-10."""
  s = _solve_setup(ndim)
  prob, mesh = s['prob'], s['mesh']
  fes = prob.fes
  rng = np.random.default_rng(17 + ndim)
  nv = SR.num_slots(ndim)
  un = rng.standard_normal(prob.x.shape)
  mu_q = prob.mu_q()
  sbar = rng.standard_normal(prob.lam_q.shape + (nv,))
  uq = np.einsum('qi,eic->eqc', fes.M, fes.gather(un))
  ubar = SR.grid_stress_vjp(fes, sbar, uq, prob.lam_q, mu_q)[0]
  want = fes.scatter(np.einsum('qi,eqc->eic', fes.M, ubar))
  kw = dict(lame_lambda=_dev(prob.lam_q), lame_mu=_dev(prob.mu_e))
  u = _leaf(un)
  sq = recover_stress(mesh, u, at='quadrature', **kw)
  assert sq.grad_fn is not None
  (sq * _dev(sbar)).sum().backward()
  assert _rel(_np(u.grad), want) <= 1e-10
  c = rng.standard_normal((len(un), nv))
  for recovery in ('lumped', 'l2'):
    u = _leaf(un)
    sn = recover_stress(mesh, u, recovery=recovery, **kw)
    (sn * _dev(c)).sum().backward()
    if recovery == 'lumped':
      cot = c / SR.lumped_weights(fes)[:, None]
    else:
      cot = np.linalg.solve(SR.mass_matrix(fes), c)
    sb = ER._wdet(fes)[..., None] * np.einsum('qi,eis->eqs', fes.M,
                                              fes.gather(cot))
    ub = SR.grid_stress_vjp(fes, sb, uq, prob.lam_q, mu_q)[0]
    want = fes.scatter(np.einsum('qi,eqc->eic', fes.M, ub))
    err = _rel(_np(u.grad), want)
    print(f'ndim={ndim} {recovery}: d<c, sigma_N>/du rel err {err:.2e}')
    assert err <= (1e-10 if recovery == 'lumped' else 1e-9)


@pytest.mark.parametrize('ndim', [2, 3])
def test_central_difference_through_solve_and_recovery(ndim):
  """One central difference per coefficient (h = 1e-4, the directions of the
  host test) of J = sum_q W vm^2 through the GPU solve and recovery against
  its own `.grad`, Jacobi, rtol = 1e-15.  The dense reference on the same
  problem, directions and step sets the floor of truncation and rounding
  (`test_elasticity_stress_host`, which asserts it: 2D lam 5.5e-9, mu 7.9e-9,
  force 9.1e-11; 3D lam 5.6e-9, mu 3.6e-8, force 3.9e-11); 10 x that is
  allowed."""
  s = _solve_setup(ndim)
  prob = s['prob']
  cds = SR.central_differences(prob, 'quadrature')
  base = dict(lam=prob.lam_q, mu=prob.mu_q(), force=prob.force)
  leaves = {k: _leaf(v) for k, v in base.items()}
  rtol = 1e-15
  _gpu_functional(s, 'quadrature', 'jacobi', leaves['lam'], leaves['mu'],
                  leaves['force'], rtol=rtol).backward()
  h = EA.CD_H

  def val(**over):
    c = {k: _dev(v) for k, v in {**base, **over}.items()}
    return float(_gpu_functional(s, 'quadrature', 'jacobi', c['lam'], c['mu'],
                                 c['force'], rtol=rtol))
  worst = []
  for name, leaf in leaves.items():
    ref_rel, dirn, _ = cds[name]
    an = float((leaf.grad * _dev(dirn)).sum())
    cd = (val(**{name: base[name] + h * dirn}) -
          val(**{name: base[name] - h * dirn})) / (2 * h)
    rel = abs(cd - an) / abs(an)
    print(f'ndim={ndim} {name}: {rel:.2e} (reference {ref_rel:.2e})')
    worst.append((name, rel, ref_rel))
  for name, rel, ref_rel in worst:
    assert rel <= 10.0 * ref_rel, (name, rel, ref_rel)


def test_von_mises_p_norm_against_youngs_modulus():
  """The stress constraint of topology optimisation: J = (sum_q W vm^p)^(1/p),
  p = 6, with a per-element Young's modulus through `lame_parameters`: dJ/dE
  from `.backward()` through solve and recovery against the reference."""
  ndim, nu, p = 2, 0.3, 6
  s = _solve_setup(ndim)
  prob, mesh = s['prob'], s['mesh']
  E, nq = prob.lam_q.shape
  rng = np.random.default_rng(23)
  young = 1.0 + rng.random(E)
  lam_e, mu_e = operators.lame_parameters(young, nu)
  expand = lambda c: EA.expand_coefficient(c, E, nq)
  J_ref, _, _, gl, gm, cond = SR.functional_gradients(
      prob.dense(expand(lam_e), expand(mu_e)), ('pnorm', p), prob.force,
      prob.fixed, prob.values, [(prob.facets, prob.trac)], 0.0,
      want_cond=True)
  want = gl.sum(1) * nu / ((1 + nu) * (1 - 2 * nu)) + \
      gm.sum(1) / (2 * (1 + nu))
  bound = 100.0 * cond * 1e-12
  Et = _leaf(young)
  lam_t, mu_t = operators.lame_parameters(Et, nu)
  u = solve_elasticity(mesh, _dev(prob.force), s['bcs'], lame_lambda=lam_t,
                       lame_mu=mu_t, rtol=1e-13, preconditioner='jacobi')
  _, vm = recover_stress(mesh, u, lame_lambda=lam_t, lame_mu=mu_t,
                         at='quadrature', von_mises=True)
  J = (s['W'] * vm ** p).sum() ** (1.0 / p)
  assert abs(float(J.detach()) - J_ref) <= bound * J_ref
  J.backward()
  err = _rel(_np(Et.grad), want)
  print(f'p-norm: dJ/dE rel err {err:.2e} (bound {bound:.2e})')
  assert err <= bound


def test_point_stress_and_its_gradient():
  """`mesh.point_evaluator(points)(recover_stress(...))`: the values against
  the evaluator on the reference's nodal stress, and a least-squares misfit at
  the sensors differentiated to a per-element lame_mu against the dense
  adjoint with the cotangent the evaluator's transpose gives."""
  s = _solve_setup(2)
  prob, mesh = s['prob'], s['mesh']
  J_ref, u_ref, *_ , cond = _reference_gradients(2, 'nodes')
  bound = 100.0 * cond * 1e-12
  pts = _dev([[0.21, 0.33], [0.5, 0.5], [0.77, 0.12], [0.9, 0.95],
              [0.34, 0.81]])
  ev = mesh.point_evaluator(pts)
  sn_ref = SR.nodal_stress(prob.fes, u_ref, prob.lam_q, prob.mu_q())
  obs = _dev(0.1 * np.arange(20.0).reshape(5, 4))
  mu = _leaf(prob.mu_e)
  lam = _dev(prob.lam_q)
  u = solve_elasticity(mesh, _dev(prob.force), s['bcs'], lame_lambda=lam,
                       lame_mu=mu, rtol=1e-13, preconditioner='jacobi')
  at_pts = ev(recover_stress(mesh, u, lame_lambda=lam, lame_mu=mu))
  assert tuple(at_pts.shape) == (5, 4)
  assert _rel(_np(at_pts), _np(ev(_dev(sn_ref)))) <= bound
  misfit = at_pts - obs
  (0.5 * (misfit ** 2).sum()).backward()
  c = _np(ev.transpose(misfit.detach()))
  gm = SR.functional_gradients(
      prob.dense(), ('linear_nodes', c), prob.force, prob.fixed, prob.values,
      [(prob.facets, prob.trac)], 0.0)[4]
  err = _rel(_np(mu.grad), gm.sum(axis=1))
  print(f'point stress: d/dmu rel err {err:.2e} (bound {bound:.2e})')
  assert err <= bound


# ------------------------------------------------------ 6. unchanged behaviour
def test_no_node_without_grad():
  """With nothing requiring grad, or under `torch.no_grad()`, no autograd node
  is built and the quadrature stress is bitwise what the tracked call's
  forward gives (one launch of the same kernel on the same values); the nodal
  stress sums shared nodes with atomics, so two calls already differ in the
  last bits: 1e-13 there.  With grad the von Mises output is
  `von_mises(sigma)` and agrees with the fused one."""
  s = _solve_setup(2)
  prob, mesh = s['prob'], s['mesh']
  rng = np.random.default_rng(29)
  un = rng.standard_normal(prob.x.shape)
  lam, mu = _dev(prob.lam_q), _dev(prob.mu_e)
  for at in ('quadrature', 'nodes'):
    plain, vm = recover_stress(mesh, _dev(un), lame_lambda=lam, lame_mu=mu,
                               at=at, von_mises=True)
    assert plain.grad_fn is None and not plain.requires_grad
    assert vm.grad_fn is None
    for kw in (dict(u=_leaf(un), lame_lambda=lam, lame_mu=mu),
               dict(u=_dev(un), lame_lambda=_leaf(prob.lam_q), lame_mu=mu),
               dict(u=_dev(un), lame_lambda=lam, lame_mu=_leaf(prob.mu_e))):
      tracked, tvm = recover_stress(mesh, kw.pop('u'), at=at, von_mises=True,
                                    **kw)
      assert tracked.grad_fn is not None and tvm.grad_fn is not None
      if at == 'quadrature':
        assert torch.equal(tracked.detach(), plain)
      else:
        assert _rel(_np(tracked), _np(plain)) <= 1e-13
      assert _rel(_np(tvm), _np(vm)) <= 1e-13
      with torch.no_grad():
        quiet = recover_stress(mesh, _dev(un), at=at, **kw)
      assert quiet.grad_fn is None


# ----------------------------------------------------------------- 7. refusals
def test_refusals():
  """Partitioned, ensemble and periodic meshes, a bad `at` / `recovery`,
  wrong shapes; `op.apply` on a field that requires grad still raises; the
  wrappers' own checks."""
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
  with pytest.raises(ValueError, match='at='):
    op.stress(u, at='points')
  with pytest.raises(ValueError, match='recovery='):
    op.stress(u, recovery='spr')
  with pytest.raises(ValueError):
    op.stress(u[:, :2])
  with pytest.raises(ValueError):
    op.stress(u[:, 0])
  with pytest.raises(ValueError):
    op.stress_local(u)
  with pytest.raises(ValueError):
    recover_stress(mesh, u, lame_lambda=1.0, lame_mu=1.0, at='cells')
  pm = unit_cube_mesh(3, ndim=2, periodic_dims=(0,))
  periodic = refine_premesh(pm, Nodes1D.create(4, GLL)).finalize(device=DEV)
  part = blocks.build_block_partition(2, 3, (2, 1, 1), 0, device='cpu')
  plain = refine_premesh(unit_cube_mesh(2, ndim=2),
                         Nodes1D.create(3, GLL)).finalize(device=DEV)
  for bad, d, what in ((periodic, 2, 'periodic'), (part.mesh, 3, 'partitioned'),
                       (plain.replicate(2), 2, 'ensemble')):
    z = torch.zeros((bad.num_nodes, d), dtype=F64, device=bad.device)
    for v in (z, z.clone().requires_grad_(True)):
      with pytest.raises(NotImplementedError, match=what):
        recover_stress(bad, v, lame_lambda=1.0, lame_mu=1.0)
  E, nq = mesh.num_elements, Q ** 3
  z = torch.zeros((E, nq, 3), dtype=F64, device=DEV)
  s = torch.zeros((E, nq, 6), dtype=F64, device=DEV)
  args = (op.parts, op.host, 3, Q, op.point_weights(), 1.0, 1.0)
  with pytest.raises(ValueError, match='want'):
    _ops.elasticity_stress(z, *args, want=(False, False))
  with pytest.raises(ValueError, match='want'):
    _ops.elasticity_stress_vjp(s, z, *args, want=(False, False, False))
  with pytest.raises(ValueError):
    _ops.elasticity_stress(z[:, :, :2], *args)
  with pytest.raises(ValueError):
    _ops.elasticity_stress_vjp(s[:, :, :4], z, *args)
  with pytest.raises(ValueError, match='displacement'):
    _ops.elasticity_stress_vjp(s, None, *args)
  big = 13 ** 3
  with pytest.raises(_lib.SfemError, match='status -3'):
    _ops.elasticity_stress(
        z[:, :1].expand(E, big, 3), op.parts, op.host, 3, 13,
        op.point_weights()[:, :1].expand(E, big), 1.0, 1.0)


def test_entry_point_refusals():
  """Status codes of the raw entry points: one valid call each, then one
  field wrong at a time; nothing that is refused launches."""
  case = G.affine(2, 3, MESH_P)
  mesh, _, rp = case.finalize(DEV, F64)
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(4, GL))
  op = fes.elasticity_operator(lame_lambda=1.0, lame_mu=1.0)
  part, = op.parts
  assert part['geo_mode'] == _lib.GEO_AFFINE
  E, nq = mesh.num_elements, 64
  z = lambda *s: torch.zeros(s, dtype=F64, device=DEV)
  keep = dict(u=z(E, nq, 3), sig=z(E, nq, 6), vm=z(E, nq), sb=z(E, nq, 6),
              ub=z(E, nq, 3), dl=z(E, nq), dm=z(E, nq),
              lst=torch.zeros(E, dtype=torch.int32, device=DEV),
              host={k: _ops._host(v, F64) for k, v in op.host.items()})
  lst = keep['lst'].data_ptr()
  lib = _lib.load()
  common = dict(wdet=op.point_weights().data_ptr(), lam_const=1.0,
                mu_const=1.0, num_elements=E, ndim=3, P=4,
                dtype=_lib.SFEM_F64,
                **_ops._launch_fields(part, keep['host'], 'kfac'))

  def caller(fn, cls, **fields):
    def call(**over):
      a = cls(**common, **fields)
      for k, v in over.items():
        setattr(a, k, v)
      return fn(ctypes.byref(a), None)
    return call
  fwd = caller(lib.sfem_elasticity_stress, _lib.ElasticityStressArgs,
               u=keep['u'].data_ptr(), sigma=keep['sig'].data_ptr(),
               vm=keep['vm'].data_ptr())
  vjp = caller(lib.sfem_elasticity_stress_vjp, _lib.ElasticityStressVjpArgs,
               sbar=keep['sb'].data_ptr(), u=keep['u'].data_ptr(),
               ubar=keep['ub'].data_ptr(), dlam=keep['dl'].data_ptr(),
               dmu=keep['dm'].data_ptr())
  assert fwd() == 0 and vjp() == 0
  torch.cuda.synchronize()
  assert fwd(sigma=None) == 0 and fwd(vm=None) == 0
  assert vjp(u=None, dlam=None, dmu=None) == 0 and vjp(ubar=None) == 0
  torch.cuda.synchronize()
  shared = (dict(wdet=None), dict(dmat=None), dict(geo_elem=None),
            dict(weights=None), dict(nodes=None),
            dict(geo_mode=_lib.GEO_POINT), dict(dtype=5),
            dict(num_elements=-1), dict(elem_list=lst, num_listed=E + 1),
            dict(elem_list=lst, num_listed=-1))
  for call, own in (
      (fwd, (dict(u=None), dict(sigma=None, vm=None))),
      (vjp, (dict(sbar=None), dict(u=None), dict(u=None, dlam=None),
             dict(ubar=None, dlam=None, dmu=None)))):
    # outside the compiled range: SFEM_EUNSUPPORTED
    for over in (dict(P=13), dict(P=1), dict(ndim=1), dict(ndim=4),
                 dict(geo_mode=_lib.GEO_BOX), dict(geo_mode=7)):
      assert call(**over) == -3, over
    # a missing required pointer or no output at all: SFEM_EINVAL
    for over in own + shared:
      assert call(**over) == -1, over
  assert vjp(ubar=None, dlam=None, dmu=None) == -1
  msg = lib.sfem_last_error().decode(errors='replace')
  assert 'sfem_elasticity_stress_vjp' in msg and 'output' in msg
  assert lib.sfem_elasticity_stress(None, None) == -1
  # nothing to do is not an error
  assert fwd(num_elements=0, u=None) == 0
  assert vjp(num_elements=0, sbar=None, u=None) == 0
