"""The adjoint of scalar transport on the GPU: the kernel
`sfem_transport_rhs_vjp` at every Q = 2..12 against the NumPy reference
(`tests/transport_adjoint_reference.py`), the adjoint identity between the
forward and the VJP kernel, one cotangent component per velocity component and
reference axis, fp32, `TransportRhs.apply` under autograd for every input
form, differentiable steps against the reference's reverse sweep, one central
difference on the device, and the opt-in semantics."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from swirl_fem_amd import _lib, _ops
from swirl_fem_amd.core import layout, operators
from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import NodeType, Quadrature1D
from swirl_fem_amd.examples.transport import BCType, ScalarTransport
from tests import adjoint_reference as AJ
from tests import advection_reference as AR
from tests import geometry_cases as G
from tests import transport_adjoint_reference as TA
from tests import transport_reference as TR
from tests.fp32util import F32Rng, f32r, tolerance
from tests.test_gpu_transport import KERNEL_COMBOS, MESH_P, _kernel_setup

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GL = NodeType.GAUSS_LEGENDRE
D, N, RB = BCType.DIRICHLET, BCType.NEUMANN, BCType.ROBIN


def _dev(a, dtype=torch.float64):
  return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _np(t):
  return t.detach().double().cpu().numpy()


def _rel(a, b):
  return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _t(fn):
  return lambda x: _dev(fn(_np(x)))


def _pad(a, pad, rng):
  return np.concatenate([a, rng.standard_normal((pad,) + a.shape[1:])])


# ------------------------------------------------ 1. kernel vs reference
def _output_sets(spec, with_source):
  """(name, [(dscalar?, dvelocity?) per level], dsource?): all outputs,
  dscalar only, dvelocity only, dsource only, one level's outputs withheld."""
  vel = [v for v, _, _ in spec]
  sets = [('all', [(True, v) for v in vel], with_source),
          ('dscalar', [(True, False)] * len(spec), False),
          ('dvelocity', [(False, v) for v in vel], False),
          ('dsource', [(False, False)] * len(spec), True),
          ('withheld', [(n != 0, v and n != 0) for n, v in enumerate(vel)],
           with_source)]
  return sets


def _run_vjp_combos(op, ref, ndim, Q, pad, rng, dtype, tol, rnd=lambda a: a):
  E, nq = ref.num_elements, ref.Q
  worst = 0.0
  for spec, with_source, with_wdet in KERNEL_COMBOS:
    levels_ref, levels_dev = [], []
    for vel, mc, cc in spec:
      Tq = rnd(rng.standard_normal((E, nq)))
      uq = rnd(rng.standard_normal((E, nq, ndim))) if vel else None
      levels_ref.append((Tq, uq, mc, cc))
      levels_dev.append((_dev(_pad(Tq, pad, rng), dtype),
                         None if uq is None else
                         _dev(_pad(uq, pad, rng), dtype), mc, cc))
    lam = rnd(rng.standard_normal((E, nq)))
    lam_dev = _dev(_pad(lam, pad, rng), dtype)
    want_levels, want_source = TA.vjp(ref, lam, levels_ref)
    for name, wants, ws in _output_sets(spec, with_source):
      needs_wdet = with_wdet or ws
      got_levels, got_source = _ops.transport_rhs_vjp(
          lam_dev, levels_dev, op.parts, op.host, ndim, Q,
          op.point_weights() if needs_wdet else None, (wants, ws))
      assert (got_source is not None) == ws
      pairs = []
      if ws:
        pairs.append((got_source, want_source))
      for (gT, gu), (wT, wu), (aT, au) in zip(got_levels, want_levels, wants):
        assert (gT is not None) == aT and (gu is not None) == au
        if aT:
          pairs.append((gT, wT))
        if au:
          pairs.append((gu, wu))
      for got, want in pairs:
        assert got.shape[0] == E + pad and got.dtype == dtype
        assert tuple(got.shape[1:]) == want.shape[1:]
        if np.abs(want).max() == 0.0:      # conv_coef = 0: no effect at all
          assert not _np(got)[:E].any()
          continue
        err = _rel(_np(got)[:E], want)
        worst = max(worst, err)
        assert err <= tol, (ndim, Q, spec, name, err)
  return worst


@pytest.mark.parametrize('Q', range(2, 13))
@pytest.mark.parametrize('ndim', [2, 3])
def test_vjp_kernel_matches_reference(ndim, Q):
  """fp64, every Q, the level sets of the forward kernel's test, five output
  sets each, on multilinear and curved elements with a padded row (list
  launches, a partial workgroup); 1e-11 of max |ref| per output, the forward
  test's figure for the same arithmetic at the same sizes."""
  case = G.three_kinds(2, ndim, MESH_P, pad=1)
  mesh, fes, ref, op = _kernel_setup(case, Q)
  assert len(op.parts) >= 2 and all('elem_list' in p for p in op.parts)
  assert {G.CURVED, G.MULTILINEAR} <= {p['geo_mode'] for p in op.parts}
  rng = np.random.default_rng(300 * ndim + Q)
  worst = _run_vjp_combos(op, ref, ndim, Q, 1, rng, torch.float64, 1e-11)
  print(f'fp64 ndim={ndim} Q={Q}: worst rel err {worst:.3e}')


@pytest.mark.parametrize('Q', [2, 5, 8, 9, 12])
@pytest.mark.parametrize('ndim', [2, 3])
def test_vjp_kernel_affine_elements(ndim, Q):
  """The affine instantiations (one launch over all elements, no list)."""
  case = G.affine(2, ndim, MESH_P)
  mesh, fes, ref, op = _kernel_setup(case, Q)
  assert [p['geo_mode'] for p in op.parts] == [G.AFFINE]
  assert 'elem_list' not in op.parts[0]
  rng = np.random.default_rng(17 * ndim + Q)
  _run_vjp_combos(op, ref, ndim, Q, 0, rng, torch.float64, 1e-11)


def test_unlisted_rows_stay_zero():
  """One launch of a list part: the rows of the other elements are zero."""
  Q, ndim = 4, 3
  case = G.three_kinds(2, ndim, MESH_P)
  mesh, fes, ref, op = _kernel_setup(case, Q)
  part = max(op.parts, key=lambda p: p['elem_list'].numel())
  listed = part['elem_list'].cpu().numpy()
  E = mesh.num_elements
  assert 0 < len(listed) < E
  rng = np.random.default_rng(1)
  T, lam = (_dev(rng.standard_normal((E, Q ** 3))) for _ in range(2))
  u = _dev(rng.standard_normal((E, Q ** 3, 3)))
  (pair,), ds = _ops.transport_rhs_vjp(
      lam, [(T, u, 0.5, 1.0)], [part], op.host, ndim, Q, op.point_weights(),
      ([(True, True)], True))
  other = np.setdiff1d(np.arange(E), listed)
  for t in pair + (ds,):
    assert not _np(t)[other].any()
    assert all(_np(t)[e].any() for e in listed)


# --------------------------------------- 2. adjoint identity on the device
@pytest.mark.parametrize('Q', [4, 9])
@pytest.mark.parametrize('ndim', [2, 3])
def test_adjoint_identity_on_device(ndim, Q):
  """<lam, J d> with the forward kernel against <J^T lam, d> with the VJP
  kernel, three levels, all three geometry kinds: 1e-12 of the product of
  norms."""
  case = G.three_kinds(3, ndim, MESH_P)
  mesh, fes, ref, op = _kernel_setup(case, Q)
  kinds = {p['geo_mode'] for p in op.parts}
  assert {G.CURVED, G.MULTILINEAR} <= kinds
  assert ndim == 2 or G.AFFINE in kinds
  E, nq = mesh.num_elements, Q ** ndim
  rng = np.random.default_rng(ndim + Q)
  r = lambda *s: _dev(rng.standard_normal(s))
  coefs = [(1.5, -1.0), (-2.0, 0.7), (0.5, 3.0)]
  T = [r(E, nq) for _ in coefs]
  u = [r(E, nq, ndim) for _ in coefs]
  dT = [r(E, nq) for _ in coefs]
  du = [r(E, nq, ndim) for _ in coefs]
  s, ds, lam = r(E, nq), r(E, nq), r(E, nq)
  W = op.point_weights()
  run = lambda lev, src: _ops.transport_rhs(lev, op.parts, op.host, ndim, Q,
                                            source=src, wdet=W)
  base = run([(T[j], u[j]) + coefs[j] for j in range(3)], s)
  tangent = (run([(dT[j], u[j]) + coefs[j] for j in range(3)], ds) +
             run([(T[j], du[j], 0.0, coefs[j][1]) for j in range(3)], None))
  # the forward map is what the tangent says: bilinear
  eps = 0.5
  moved = run([(T[j] + eps * dT[j], u[j] + eps * du[j]) + coefs[j]
               for j in range(3)], s + eps * ds)
  second = run([(dT[j], du[j], 0.0, coefs[j][1]) for j in range(3)], None)
  assert _rel(_np(moved), _np(base + eps * tangent + eps ** 2 * second)) <= 1e-12
  bars, s_bar = _ops.transport_rhs_vjp(
      lam, [(T[j], u[j]) + coefs[j] for j in range(3)], op.parts, op.host,
      ndim, Q, W, ([(True, True)] * 3, True))
  left = float((_np(lam) * _np(tangent)).sum())
  right = float((_np(s_bar) * _np(ds)).sum())
  for j in range(3):
    right += float((_np(bars[j][0]) * _np(dT[j])).sum())
    right += float((_np(bars[j][1]) * _np(du[j])).sum())
  scale = np.linalg.norm(_np(lam)) * np.linalg.norm(_np(tangent))
  print(f'ndim={ndim} Q={Q}: {left:.10e} against {right:.10e}, '
        f'{abs(left - right) / scale:.2e} of the norms')
  assert abs(left - right) <= 1e-12 * scale


# ------------------------- 3. one component per velocity component and axis
@pytest.mark.parametrize('c', [0, 1, 2])
@pytest.mark.parametrize('axis', [0, 1, 2])
def test_one_cotangent_component_one_axis(c, axis):
  """A velocity with the single non-zero component c, a scalar that varies
  along one reference axis only and a cotangent that varies along another, on
  sheared elements of all three kinds: a transposed cofactor or a swapped
  point or component order fails."""
  Q = 4
  case = G.three_kinds(3, 3, MESH_P)
  mesh, fes, ref, op = _kernel_setup(case, Q)
  assert {p['geo_mode'] for p in op.parts} == {G.CURVED, G.MULTILINEAR,
                                              G.AFFINE}
  E, nq = ref.num_elements, ref.Q
  xq = AR.quad_points(ref)
  uq = np.zeros((E, nq, 3))
  uq[..., c] = 1.0 + 4.0 * xq[..., (c + 1) % 3] ** 2
  xi = np.asarray(fes.quadrature.nodes.node_values, np.float64)

  def along(ax):
    g = np.zeros((Q, Q, Q)) + xi.reshape([-1 if a == ax else 1
                                          for a in range(3)])
    return g.reshape(-1)
  Tq = np.broadcast_to(np.sin(1.3 * along(axis)) + along(axis) ** 2,
                       (E, nq)).copy()
  lam = np.broadcast_to(np.cos(0.9 * along((axis + 1) % 3)) +
                        along((axis + 1) % 3), (E, nq)).copy()
  (want,), _ = TA.vjp(ref, lam, [(Tq, uq, 0.0, 1.0)], want_source=False)
  (got,), none = _ops.transport_rhs_vjp(
      _dev(lam), [(_dev(Tq), _dev(uq), 0.0, 1.0)], op.parts, op.host, 3, Q,
      None, ([(True, True)], False))
  assert none is None
  for g, w in zip(got, want):
    assert np.abs(w).max() > 1e-3
    assert _rel(_np(g), w) <= 1e-11
  # every velocity component has a cotangent of its own (the three cofactors
  # of reference axis `axis` differ on sheared elements)
  for a in range(3):
    for b in range(a + 1, 3):
      assert _rel(want[1][..., a], want[1][..., b]) > 1e-3


# ------------------------------------------------------------------ 4. fp32
@pytest.mark.parametrize('Q', range(2, 13))
@pytest.mark.parametrize('ndim', [2, 3])
def test_vjp_fp32_within_policy(ndim, Q):
  case = G.three_kinds(3, ndim, MESH_P)
  mesh, fes, ref, op = _kernel_setup(case, Q, torch.float32)
  rng = F32Rng(50 + Q)
  worst = _run_vjp_combos(op, ref, ndim, Q, 0, rng, torch.float32,
                          tolerance(torch.float32, Q), rnd=f32r)
  print(f'fp32 ndim={ndim} Q={Q}: worst rel err {worst:.3e}')


# --------------------------------- 5. TransportRhs.apply under autograd
def _field(x):
  d = x.shape[-1]
  comps = [1.0 + x[..., 0] * x[..., d - 1], np.sin(2.0 * x[..., 0]) - 0.5]
  if d == 3:
    comps.append(0.5 - x[..., 1] ** 2 + x[..., 2])
  return np.stack(comps, axis=-1)


@functools.lru_cache(maxsize=None)
def _assembled(ndim, P):
  rp = TR.box_with_sides(3, ndim, P, three_kinds=True)
  mesh = rp.finalize(device=DEV)
  st = ScalarTransport.create(mesh, {})
  return rp, mesh, st.rhs_op, TR.Dense(rp, P)


def _rhs_gradient(dense, w, levels, source):
  """Reference gradients of w . dense.rhs(levels, source): ([(T_bar, u_bar in
  the form of u)], s_bar in the form of the source)."""
  fes = dense.fes
  out = []
  for T, u, mc, cc in levels:
    gT = mc * (dense.B.T @ w)
    gu = None
    if u is not None:
      if cc != 0.0:
        gT = gT + cc * (dense.convection(u).T @ w)
      db = AJ.sensitivities(fes, T, w, 0.0, 0.0)[2]
      gu = TA._velocity_cotangent(fes, u, cc * db)
    out.append((gT, gu))
  gs = None
  if source is not None:
    gs = (dense.B.T @ w if source.shape == (fes.num_nodes,)
          else TR.wdet(fes) * AJ.value(fes, fes.gather(w)))
  return out, gs


@pytest.mark.parametrize('ndim,P', [(2, 4), (3, 3)])
def test_apply_under_autograd_matches_reference(ndim, P):
  """w . TransportRhs.apply(levels, source) differentiated by autograd for
  every velocity form (nodal contiguous, component-major, strided, constant,
  point values) with the gradient in that form, nodal and per-point sources,
  and one tensor used at two levels: 1e-11 of the maximum."""
  rp, mesh, op, dense = _assembled(ndim, P)
  ref = dense.fes
  rng = np.random.default_rng(40 + ndim)
  x = np.asarray(rp.node_coords, np.float64)
  nodal = _field(x)
  point = _field(AR.quad_points(ref)) * 0.7
  const = np.array([0.7, -1.1, 0.4][:ndim])
  w = rng.standard_normal(mesh.num_nodes)
  Ts = rng.standard_normal((3, mesh.num_nodes))
  s_nodal = rng.standard_normal(mesh.num_nodes)
  s_point = rng.standard_normal((ref.num_elements, ref.Q))
  coefs = [(-1.5, 1.0), (2.0, -3.0), (-0.5, 0.7)]
  leaf = lambda a: _dev(a).requires_grad_()

  def forms():
    cm = layout.component_major(_dev(nodal)).detach().requires_grad_()
    assert not cm.is_contiguous()
    wide = leaf(np.concatenate([nodal, 2.0 * nodal], axis=1))
    return [('nodal', leaf(nodal), None, nodal),
            ('component-major', cm, None, nodal),
            ('strided', wide, wide[:, :ndim], nodal),
            ('constant', leaf(const), None, const),
            ('point', leaf(point), None, point)]
  for name, u_leaf, u_used, u_ref in forms():
    u_used = u_leaf if u_used is None else u_used
    for source in (s_nodal, s_point):
      u_leaf.grad = None
      T = [leaf(Ts[j]) for j in range(3)]
      s = leaf(source)
      # the velocity serves levels 0 and 2, level 1 has none
      lev_dev = [(T[0], u_used) + coefs[0], (T[1], None) + coefs[1],
                 (T[2], u_used) + coefs[2]]
      lev_ref = [(Ts[0], u_ref) + coefs[0], (Ts[1], None) + coefs[1],
                 (Ts[2], u_ref) + coefs[2]]
      out = op.apply(lev_dev, s)
      assert out.grad_fn is not None
      assert _rel(_np(out), dense.rhs(lev_ref, source)) <= 1e-11
      (out * _dev(w)).sum().backward()
      want, want_s = _rhs_gradient(dense, w, lev_ref, source)
      for j in range(3):
        err = _rel(_np(T[j].grad), want[j][0])
        assert err <= 1e-11, (name, 'T', j, err)
      got_u = _np(u_leaf.grad)
      assert u_leaf.grad.shape == u_leaf.shape
      if name == 'strided':
        assert not got_u[:, ndim:].any()
        got_u = got_u[:, :ndim]
      elif name != 'constant':
        assert u_leaf.grad.stride() == u_leaf.stride(), name
      err = _rel(got_u, want[0][1] + want[2][1])
      assert err <= 1e-11, (name, 'u', err)
      err = _rel(_np(s.grad), want_s)
      assert err <= 1e-11, (name, 's', err)
  # one scalar at two levels receives the sum
  Tl, u = leaf(Ts[0]), _dev(nodal)
  out = op.apply([(Tl, u) + coefs[0], (Tl, _dev(const)) + coefs[1]])
  (out * _dev(w)).sum().backward()
  want, _ = _rhs_gradient(dense, w, [(Ts[0], nodal) + coefs[0],
                                     (Ts[0], const) + coefs[1]], None)
  assert _rel(_np(Tl.grad), want[0][0] + want[1][0]) <= 1e-11
  # nothing requires grad: the plain path, no node
  assert op.apply([(_dev(Ts[0]), u) + coefs[0]]).grad_fn is None


# ------------------------------------ 6. steps against the reference sweep
K_FORMS = ('scalar', 'elem', 'point')


@functools.lru_cache(maxsize=None)
def _step_case(ndim, form, periodic=()):
  """The reference problem with the diffusivity in one of the three forms,
  its device mesh and the boundary conditions."""
  prob = TA.step_problem(ndim, periodic)
  E, nq = prob['k_q'].shape
  k = {'scalar': np.float64(1.3), 'elem': prob['k_q'][:, 0].copy(),
       'point': prob['k_q']}[form]
  dense = prob['make'](AJ.expand_coefficient(k, E, nq))
  mesh = prob['rp'].finalize(device=DEV)
  bcs = {}
  if not periodic:
    alpha, gr = TA.ROBIN[0][1:]
    bcs = {'x0': (D, _dev(np.nan_to_num(prob['dvals']))),
           'x1': (RB, (alpha, _t(gr))), 'y1': (N, _t(TA.NEUMANN[0][1]))}
  conds = [np.linalg.cond(dense.step_matrix(TR.coefficients(o)[0][-1] / TA.DT))
           for o in TA.ORDERS]
  return prob, k, dense, mesh, bcs, max(conds)


def _rollout(st, T0, u, s, pc, rtol=1e-12):
  Ts = [T0]
  for order in TA.ORDERS:
    T, info = st.step(Ts, [u] * order, TA.DT, order, s, rtol=rtol,
                      preconditioner=pc, return_info=True)
    assert info['status'] == 'converged', info
    Ts.append(T)
  return Ts


@pytest.mark.parametrize('form', K_FORMS)
@pytest.mark.parametrize('pc', [None, 'jacobi', 'pmg'])
@pytest.mark.parametrize('ndim', [2, 3])
def test_step_gradients_match_reference_sweep(ndim, pc, form):
  """w . T after three steps (orders 1, 2, 3, rtol 1e-12) on the Dirichlet /
  Neumann / Robin three-kinds box; gradients with respect to T0, a nodal
  velocity used at every level, the source and the diffusivity as a scalar,
  per element and per point, within 100 cond 1e-12 steps of the maximum, cond
  the largest condition number of the three step matrices."""
  prob, k, dense, mesh, bcs, cond = _step_case(ndim, form)
  bound = 100.0 * cond * 1e-12 * len(TA.ORDERS)
  assert bound <= 1e-6
  kd = torch.tensor(k, dtype=torch.float64, device=DEV, requires_grad=True)
  assert kd.dim() == np.ndim(k)
  st = ScalarTransport.create(mesh, bcs, diffusivity=kd, differentiable=True)
  T0 = _dev(prob['T0']).requires_grad_()
  u = _dev(prob['u_nodal']).requires_grad_()
  s = _dev(prob['s_nodal']).requires_grad_()
  Ts = _rollout(st, T0, u, s, pc)
  want = TA.rollout_gradient(dense, prob['w'], prob['T0'],
                             [prob['u_nodal']] * 3, TA.DT, TA.ORDERS,
                             prob['s_nodal'])
  assert _rel(_np(Ts[-1]), want['levels'][-1]) <= bound
  (Ts[-1] * _dev(prob['w'])).sum().backward()
  free = np.isnan(prob['dvals'])
  pairs = {'T0': (_np(T0.grad) * free, want['T0'] * free),
           'u': (_np(u.grad), sum(want['vels'])),
           's': (_np(s.grad), want['source']),
           'k': (_np(kd.grad), AJ.reduce_coefficient(want['k'], form))}
  assert kd.grad.shape == kd.shape
  for name, (got, ref) in pairs.items():
    err = _rel(np.asarray(got), np.asarray(ref))
    print(f'ndim={ndim} {pc} k {form}: d/d{name} rel err {err:.2e} '
          f'(bound {bound:.2e}, cond {cond:.1f})')
    assert err <= bound, (name, err, bound)
  # the Dirichlet rows of T0 enter the right-hand side like any other row of
  # the level: their cotangent is the reference's too
  assert _rel(_np(T0.grad), want['T0']) <= bound


def test_step_gradients_on_a_periodic_box():
  """Box periodic in x, no preconditioner: T0, velocity and source against
  the reference with `node_indices`; a diffusivity with grad raises."""
  prob, k, dense, mesh, bcs, cond = _step_case(2, 'point', (0,))
  ni = mesh.node_indices.cpu().numpy()
  assert (ni != np.arange(len(ni))).any()
  bound = 100.0 * cond * 1e-12 * len(TA.ORDERS)
  st = ScalarTransport.create(mesh, {}, diffusivity=_dev(k),
                              differentiable=True)
  T0 = _dev(prob['T0']).requires_grad_()
  u = _dev(prob['u_nodal']).requires_grad_()
  s = _dev(prob['s_nodal']).requires_grad_()
  Ts = _rollout(st, T0, u, s, None)
  want = TA.rollout_gradient(dense, prob['w'], prob['T0'],
                             [prob['u_nodal']] * 3, TA.DT, TA.ORDERS,
                             prob['s_nodal'])
  assert _rel(_np(Ts[-1]), want['levels'][-1]) <= bound
  (Ts[-1] * _dev(prob['w'])).sum().backward()
  for name, got, ref in (('T0', T0.grad, want['T0']),
                         ('u', u.grad, sum(want['vels'])),
                         ('s', s.grad, want['source'])):
    err = _rel(_np(got), ref)
    print(f'periodic d/d{name}: rel err {err:.2e} (bound {bound:.2e})')
    assert err <= bound, (name, err)
  with pytest.raises(NotImplementedError):
    ScalarTransport.create(mesh, {}, diffusivity=_dev(k).requires_grad_(),
                           differentiable=True)


# --------------------------------- 7. one central difference on the device
@pytest.mark.parametrize('name', ['T0', 'u_nodal', 'k'])
def test_central_difference_on_device(name):
  """The device's own central difference (solves at rtol 1e-15, Jacobi) along
  the reference's direction and at its step against the device's gradient:
  10 x the discrepancy the host test recorded for the reference."""
  prob, k, dense, mesh, bcs, cond = _step_case(3, 'point')
  _, dirn, an_ref = TA.central_differences(prob, [name])[name]
  h = TA.CD_H[name]
  w = _dev(prob['w'])

  def loss(T0=prob['T0'], u=prob['u_nodal'], kq=prob['k_q'], grad=False):
    leaves = [_dev(a).requires_grad_(grad) for a in (T0, u, kq)]
    st = ScalarTransport.create(mesh, bcs, diffusivity=leaves[2],
                                differentiable=grad)
    T = _rollout(st, leaves[0], leaves[1], _dev(prob['s_nodal']), 'jacobi',
                 rtol=1e-15)[-1]
    return (T * w).sum(), leaves
  value, leaves = loss(grad=True)
  value.backward()
  key = {'T0': 'T0', 'u_nodal': 'u', 'k': 'kq'}[name]
  base = {'T0': prob['T0'], 'u': prob['u_nodal'], 'kq': prob['k_q']}[key]
  g = _np(leaves[['T0', 'u', 'kq'].index(key)].grad)
  an = float((g * dirn).sum())
  with torch.no_grad():
    cd = (float(loss(**{key: base + h * dirn})[0]) -
          float(loss(**{key: base - h * dirn})[0])) / (2 * h)
  got = abs(cd - an) / abs(an)
  print(f'{name}: h = {h:g}, device gradient {an:.10e} (reference '
        f'{an_ref:.10e}), device central difference {cd:.10e}, relative '
        f'discrepancy {got:.2e}, reference recorded '
        f'{TA.CD_OBSERVED[name]:.2e}')
  assert got <= 10.0 * TA.CD_OBSERVED[name]


# ------------------------------------------------------ 8. opt-in semantics
def test_opt_in_semantics():
  prob, k, dense, mesh, bcs, cond = _step_case(3, 'elem')
  rtol = 1e-10
  Tn, u = _dev(prob['T0']), _dev(prob['u_const'])
  s, kd = _dev(prob['s_nodal']), _dev(k)
  leaf = lambda t: t.clone().requires_grad_()
  # a default instance refuses each of the four grad-carrying inputs
  with pytest.raises(NotImplementedError):
    ScalarTransport.create(mesh, bcs, diffusivity=leaf(kd))
  plain = ScalarTransport.create(mesh, bcs, diffusivity=kd)
  assert not plain.differentiable
  for kw in (dict(Ts=[leaf(Tn)]), dict(us=[leaf(u)]), dict(source=leaf(s))):
    args = dict(Ts=[Tn], us=[u], source=s)
    args.update(kw)
    with pytest.raises(NotImplementedError):
      plain.step(args['Ts'], args['us'], TA.DT, 1, args['source'])
  want = plain.step([Tn], [u], TA.DT, 1, s, rtol=rtol, preconditioner='jacobi')
  assert want.grad_fn is None
  # a differentiable instance without grad in play runs the plain body
  st = ScalarTransport.create(mesh, bcs, diffusivity=kd, differentiable=True)
  got = st.step([Tn], [u], TA.DT, 1, s, rtol=rtol, preconditioner='jacobi')
  assert got.grad_fn is None and not got.requires_grad
  assert _rel(_np(got), _np(want)) <= 2.0 * cond * rtol
  std = ScalarTransport.create(mesh, bcs, diffusivity=leaf(kd),
                               differentiable=True)
  with torch.no_grad():
    got = std.step([leaf(Tn)], [leaf(u)], TA.DT, 1, leaf(s), rtol=rtol,
                   preconditioner='jacobi')
  assert got.grad_fn is None and not got.requires_grad
  assert _rel(_np(got), _np(want)) <= 2.0 * cond * rtol
  # inside one differentiable call the value is what the body computes from
  # the detached inputs
  seen = {}
  body = std._implicit

  def spy(rhs, lambda0, **kw):
    assert not rhs.requires_grad
    seen['T'], info = body(rhs, lambda0, **kw)
    return seen['T'], info
  std._implicit = spy
  T0 = leaf(Tn)
  out, info = std.step([T0], [u], TA.DT, 1, s, rtol=rtol,
                       preconditioner='jacobi', return_info=True)
  std._implicit = body
  assert out.grad_fn is not None and info['status'] == 'converged'
  assert torch.equal(out.detach(), seen['T'])
  assert _rel(_np(out), _np(want)) <= 2.0 * cond * rtol
  # backward twice through one graph: the usual torch error, not a fault
  loss = out.sum()
  loss.backward()
  assert T0.grad is not None and std.diffusivity.grad is not None
  with pytest.raises(RuntimeError, match='backward through the graph a second'):
    loss.backward()
  torch.cuda.synchronize()
  # second derivatives are refused
  T0 = leaf(Tn)
  out = std.step([T0], [u], TA.DT, 1, s, rtol=rtol, preconditioner='jacobi')
  g, = torch.autograd.grad(out.sum(), T0, create_graph=True)
  with pytest.raises(RuntimeError):
    g.sum().backward()
  # partitioned meshes and ensembles stay refused
  with pytest.raises(NotImplementedError):
    ScalarTransport.create(mesh.replicate(2), {}, differentiable=True)


def test_vjp_refusals():
  """The C-ABI's codes, and the same refusals through `_ops` as ValueError /
  NotImplementedError."""
  case = G.affine(2, 3, MESH_P)
  mesh, _, rp = case.finalize(DEV, torch.float64)
  Q = 4
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(Q, GL))
  op = operators.TransportRhs.create(fes)
  E, nq = mesh.num_elements, Q ** 3
  z = lambda *s: torch.zeros(s, dtype=torch.float64, device=DEV)
  keep = dict(lam=z(E, nq), T=z(E, nq), u=z(E, nq, 3), dT=z(E, nq),
              du=z(E, nq, 3), ds=z(E, nq),
              host={k: np.ascontiguousarray(v, np.float64)
                    for k, v in op.host.items()})
  part = op.parts[0]

  def raw(**over):
    a = _lib.TransportVjpArgs(
        cotangent=keep['lam'].data_ptr(), wdet=op.point_weights().data_ptr(),
        dsource=keep['ds'].data_ptr(), geo_elem=part['geo_elem'].data_ptr(),
        dmat=keep['host']['dmat'].ctypes.data,
        weights=keep['host']['weights'].ctypes.data,
        nodes=keep['host']['nodes'].ctypes.data, num_elements=E, num_levels=1,
        ndim=3, P=Q, dtype=_lib.SFEM_F64, geo_mode=part['geo_mode'])
    a.scalar[0], a.velocity[0] = keep['T'].data_ptr(), keep['u'].data_ptr()
    a.dscalar[0], a.dvelocity[0] = keep['dT'].data_ptr(), keep['du'].data_ptr()
    a.mass_coef[0], a.conv_coef[0] = 1.0, 1.0
    for k, v in over.items():
      if isinstance(v, tuple):
        getattr(a, k)[0] = v[0]
      else:
        setattr(a, k, v)
    return a
  call = lambda a: _lib.load().sfem_transport_rhs_vjp(ctypes.byref(a), None)
  assert call(raw()) == 0
  torch.cuda.synchronize()
  for over in (dict(P=13), dict(P=1), dict(ndim=1), dict(ndim=4),
               dict(num_levels=4), dict(geo_mode=_lib.GEO_BOX),
               dict(geo_mode=7)):
    assert call(raw(**over)) == -3, over
  for over in (dict(cotangent=None), dict(dmat=None), dict(wdet=None),
               dict(geo_elem=None), dict(weights=None),
               dict(geo_mode=_lib.GEO_POINT), dict(dtype=5),
               dict(scalar=(None,)), dict(velocity=(None,))):
    assert call(raw(**over)) == -1, over
  # without dvelocity the scalar may be missing; without mass terms and
  # dsource so may wdet
  assert call(raw(scalar=(None,), dvelocity=(None,))) == 0
  assert call(raw(wdet=None, dsource=None, mass_coef=(0.0,))) == 0
  assert call(raw(dscalar=(None,), dvelocity=(None,), dsource=None,
                  wdet=None)) == 0
  torch.cuda.synchronize()
  # the Python layer
  lam, T, u = keep['lam'], keep['T'], keep['u']
  W = op.point_weights()
  run = lambda levels, want, P=Q, ndim=3, wdet=W, lam=lam: (
      _ops.transport_rhs_vjp(lam, levels, op.parts, op.host, ndim, P, wdet,
                             want))
  with pytest.raises(NotImplementedError):
    run([(T, u, 1.0, 1.0)], ([(True, True)], True), P=13)
  with pytest.raises(NotImplementedError):
    run([(T, u, 1.0, 1.0)], ([(True, True)], True), ndim=4)
  with pytest.raises(ValueError):
    run([(T, u, 1.0, 1.0)] * 4, ([(True, True)] * 4, True))
  with pytest.raises(ValueError):
    run([(T, u, 1.0, 1.0)], ([(True, True)] * 2, True))
  with pytest.raises(ValueError):
    run([(None, u, 1.0, 1.0)], ([(True, True)], False))
  with pytest.raises(ValueError):
    run([(T, None, 1.0, 1.0)], ([(False, True)], False))
  with pytest.raises(ValueError):
    run([(T, u, 1.0, 1.0)], ([(True, False)], False), wdet=None)
  with pytest.raises(ValueError):
    run([(T, u, 0.0, 1.0)], ([(False, False)], True), wdet=None)
  with pytest.raises(ValueError):
    run([(T, T, 0.0, 1.0)], ([(True, False)], False))
  with pytest.raises(ValueError):
    run([(T, u, 0.0, 1.0)], ([(True, False)], False), lam=lam[:-1])
  (pair,), ds = run([(None, u, 0.0, 1.0)], ([(True, False)], False), wdet=None)
  assert pair[1] is None and ds is None and tuple(pair[0].shape) == (E, nq)
