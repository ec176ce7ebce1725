"""The adjoint of J2 plasticity on the GPU: the kernel
`sfem_plasticity_vjp`, displacement and state modes, at every Q = 2..12
against the NumPy reference (`tests/plasticity_adjoint_reference.py`) and
against the forward kernels; `PlasticityOperator.history_vjp` and
`.sensitivity`; `.grad` through `solve_plasticity(..., differentiable=True)`
against the dense path adjoint of the reference.

The VJP jumps at the yield surface and the displacement mode mixes the points
of an element, so every kernel comparison takes its history from
`_away_from_yield` and asserts, from the reference, that no point lies within
`MARGIN[dtype]` of the surface: nothing is excluded.  The virgin combination
passes a zero history moved away in the same way, and separately checks that
a NULL history gives bitwise what an explicit zero history gives."""
import functools

import numpy as np
import pytest
import torch

from swirl_fem_amd import _ops
from swirl_fem_amd.core import layout
from swirl_fem_amd.examples.plasticity import BCType, solve_plasticity
from swirl_fem_amd.linalg.pmg_elasticity import ElasticityPMultigrid
from tests import geometry_cases as G
from tests import plasticity_adjoint_reference as PA
from tests import plasticity_reference as PR
from tests.fp32util import F32Rng, f32r, tolerance
from tests.test_gpu_plasticity import (DEV, FP64_TOL, KERNEL_COMBOS, MARGIN,
                                       MESH_P, VIRGIN_COMBO, _away_from_yield,
                                       _assembled, _check, _dev,
                                       _half_plastic, _kernel_setup,
                                       _nodal_state, _np, _rel, _t)

pytestmark = pytest.mark.gpu
F64 = torch.float64
D, N = BCType.DIRICHLET, BCType.NEUMANN
STATE_NAMES = ('hbar_prev', 'dlam', 'dmu', 'dyield', 'dhard', 'drho')


def _draw(combo, ref, rng, rnd):
  E, nq = ref.num_elements, ref.Q

  def coef(c):
    if isinstance(c, tuple):
      return rnd(c[1] * (1.0 + 0.2 * rng.uniform(-1, 1, (E, nq))))
    return c
  return tuple(coef(c) if k != 3 else c for k, c in enumerate(combo))


def _clear_state(ref, ndim, rng, rnd, mat, margin, virgin):
  """(u on the grid, a history) with about half of the points plastic and no
  point within `margin` of the yield surface, asserted from the reference."""
  E, nq = ref.num_elements, ref.Q
  hist = PR.virgin(ref) if virgin else PR.random_history(ref, rng, rnd=rnd)
  uq = _half_plastic(ref, rng.standard_normal((E, nq, ndim)), hist, mat, rnd,
                     margin)
  hist = _away_from_yield(ref, uq, hist, mat, margin, rnd)
  f, plastic = PR.yield_margin(ref, uq, hist, *mat)
  assert (np.abs(f) >= margin).all()
  assert 0.2 <= plastic.mean() <= 0.8
  return uq, hist


def _run_vjp_combos(op, ref, ndim, Q, pad, rng, dtype, tol, combos,
                    rnd=lambda a: a):
  """Each combination, both modes, against `grid_vjp_displacement` and
  `grid_vjp_state`.  The `pad` trailing rows carry zero fields, a non-zero
  history and a non-zero cotangent: every output is exactly zero there."""
  E, nq = ref.num_elements, ref.Q
  NH = PR.NH[ndim]
  npd = np.float32 if dtype == torch.float32 else np.float64
  rows = []
  for n, combo in combos:
    lam, mu, rho, l0, sy, Hh = _draw(combo, ref, rng, rnd)
    mat = (lam, mu, sy, Hh)
    uq, hist = _clear_state(ref, ndim, rng, rnd, mat, MARGIN[dtype],
                            n == VIRGIN_COMBO)
    wq = rnd(rng.standard_normal((E, nq, ndim)))
    hbar = rnd(rng.standard_normal((E, nq, NH)))
    print(f'{dtype} ndim={ndim} Q={Q} combo {n}')

    def dev(c):
      if isinstance(c, np.ndarray):
        return _dev(np.concatenate([c, np.ones((pad, nq))]), dtype)
      return c

    def padded(a, fill=0.0):
      return _dev(np.concatenate([a, np.full((pad,) + a.shape[1:], fill)]),
                  dtype)
    args = (op.parts, op.host, ndim, Q, op.point_weights(), dev(lam), dev(mu),
            dev(sy), dev(Hh))
    u_d, w_d = padded(uq), padded(wq)
    hist_d, hbar_d = padded(hist, 0.01), padded(hbar, 1.0)
    before = hist_d.clone(), hbar_d.clone()

    # displacement mode
    want_u = PA.grid_vjp_displacement(ref, uq, hist, hbar, *mat)
    got_u = _ops.plasticity_vjp(u_d, *args, mode='displacement', hist=hist_d,
                                hbar=hbar_d)
    assert got_u.shape == (E + pad, nq, ndim) and got_u.dtype == dtype
    assert bool((got_u[E:] == 0).all())
    _check('displacement', _np(got_u)[:E], want_u, tol, dtype,
           lambda: PA.grid_vjp_displacement(ref, uq, hist, hbar, *mat,
                                            dtype=npd), rows)

    # state mode, every output
    want_s = PA.grid_vjp_state(ref, uq, wq, hist, hbar, *mat, lambda0=l0)
    f32 = lambda: PA.grid_vjp_state(ref, uq, wq, hist, hbar, *mat, lambda0=l0,
                                    dtype=npd)
    got_s = _ops.plasticity_vjp(u_d, *args, mode='state', hist=hist_d,
                                hbar=hbar_d, w_q=w_d, lambda0=l0)
    assert got_s[0].shape == (E + pad, nq, NH)
    for k, name in enumerate(STATE_NAMES):
      g = got_s[k]
      assert g.dtype == dtype and g.shape[:2] == (E + pad, nq)
      assert bool((g[E:] == 0).all()), name      # the padded row: exact zeros
      if name == 'drho' and l0 == 0.0:
        assert bool((g == 0).all())
        continue
      _check(name, _np(g)[:E], want_s[k], tol, dtype,
             lambda k=k: f32()[k], rows)
    assert torch.equal(hist_d, before[0]) and torch.equal(hbar_d, before[1])

    # each output alone: bitwise the full launch, the others None
    for k, name in enumerate(STATE_NAMES):
      want = tuple(j == k - 1 for j in range(5))
      alone = _ops.plasticity_vjp(u_d, *args, mode='state', hist=hist_d,
                                  hbar=hbar_d, w_q=w_d, lambda0=l0,
                                  want=want, want_history=k == 0)
      for j, t in enumerate(alone):
        if j == k:
          assert torch.equal(t, got_s[k]), name
        else:
          assert t is None, (name, STATE_NAMES[j])

    # hbar = None is a zero cotangent
    zero = _ops.plasticity_vjp(u_d, *args, mode='state', hist=hist_d,
                               hbar=torch.zeros_like(hbar_d), w_q=w_d,
                               lambda0=l0)
    none = _ops.plasticity_vjp(u_d, *args, mode='state', hist=hist_d,
                               w_q=w_d, lambda0=l0)
    for a, b in zip(zero, none):
      assert torch.equal(a, b)

    if n == VIRGIN_COMBO:   # a NULL history is a zero history
      z = torch.zeros_like(hist_d)
      assert torch.equal(
          _ops.plasticity_vjp(u_d, *args, mode='displacement', hbar=hbar_d),
          _ops.plasticity_vjp(u_d, *args, mode='displacement', hist=z,
                              hbar=hbar_d))
      for a, b in zip(
          _ops.plasticity_vjp(u_d, *args, mode='state', hbar=hbar_d, w_q=w_d,
                              lambda0=l0),
          _ops.plasticity_vjp(u_d, *args, mode='state', hist=z, hbar=hbar_d,
                              w_q=w_d, lambda0=l0)):
        assert torch.equal(a, b)
  return rows


@pytest.mark.parametrize('Q', range(2, 13))
@pytest.mark.parametrize('ndim', [2, 3])
def test_vjp_kernel_matches_reference(ndim, Q):
  """fp64, every Q, both modes, every combination of `KERNEL_COMBOS` (scalar
  and per-point coefficients, Hh = 0, virgin), on multilinear and curved
  elements with a padded row (list launches, a partial workgroup)."""
  case = G.three_kinds(2, ndim, MESH_P, pad=1)
  mesh, fes, ref, op = _kernel_setup(case, Q)
  assert len(op.parts) >= 2 and all('elem_list' in p for p in op.parts)
  assert {G.CURVED, G.MULTILINEAR} <= {p['geo_mode'] for p in op.parts}
  rng = np.random.default_rng(300 * ndim + Q)
  _run_vjp_combos(op, ref, ndim, Q, 1, rng, torch.float64,
                  tolerance(torch.float64, Q), list(enumerate(KERNEL_COMBOS)))


@pytest.mark.parametrize('Q', range(2, 13))
@pytest.mark.parametrize('ndim', [2, 3])
def test_vjp_kernel_affine_elements(ndim, Q):
  """The affine instantiations at every Q, both modes (one launch over all
  elements, no list)."""
  case = G.affine(2, ndim, MESH_P)
  mesh, fes, ref, op = _kernel_setup(case, Q)
  assert [p['geo_mode'] for p in op.parts] == [G.AFFINE]
  assert 'elem_list' not in op.parts[0]
  rng = np.random.default_rng(11 * ndim + Q)
  combos = list(enumerate(KERNEL_COMBOS))
  _run_vjp_combos(op, ref, ndim, Q, 0, rng, torch.float64,
                  tolerance(torch.float64, Q),
                  combos[:3] + combos[VIRGIN_COMBO:])


@pytest.mark.parametrize('Q', [2, 5, 8, 9, 12])
@pytest.mark.parametrize('ndim', [2, 3])
def test_vjp_kernel_fp32(ndim, Q):
  """fp32 with float32-representable meshes and inputs against the fp64
  reference at `tolerance(torch.float32, Q)`, every combination, both modes.
  A case above that is held to 4 times the error of the NumPy reference
  evaluated in float32."""
  case = G.three_kinds(2, ndim, MESH_P)
  mesh, fes, ref, op = _kernel_setup(case, Q, torch.float32)
  rng = F32Rng(Q + 50)
  rows = _run_vjp_combos(op, ref, ndim, Q, 0, rng, torch.float32,
                         tolerance(torch.float32, Q),
                         list(enumerate(KERNEL_COMBOS)), rnd=f32r)
  for name, err, allowed in rows:
    if err > tolerance(torch.float32, Q):
      print(f'EXCEPTION ndim={ndim} Q={Q} {name}: {err:.3e} <= {allowed:.3e}')


# ------------------------------------------------ kernel against kernel
@pytest.mark.parametrize('ndim', [2, 3])
def test_state_mode_is_the_derivative_of_the_residual_launch(ndim):
  """With hbar = 0 the state mode is the derivative of v . r of
  `sfem_plasticity_local` along a direction in (lam, mu, sigma_y, Hh,
  history): a central difference of that residual launch at h = 1e-4 (relative
  one-signed directions for the coefficients; the history direction keeps
  eps_p trace-free) against the contraction of the kernel's outputs.  The
  plastic set is asserted, from the reference, to be the same at +h, 0, -h.
  Bound: 10 times the error of the same quotient in the reference, which at
  this step is its truncation."""
  Q = 5
  case = G.three_kinds(2, ndim, MESH_P)
  mesh, fes, ref, op = _kernel_setup(case, Q)
  rng = np.random.default_rng(40 + ndim)
  E, nq = ref.num_elements, ref.Q
  lam, mu, rho, l0, sy, Hh = _draw(KERNEL_COMBOS[1], ref, rng, lambda a: a)
  mat = (lam, mu, sy, Hh)
  uq, hist = _clear_state(ref, ndim, rng, lambda a: a, mat, 5e-3, False)
  vq = rng.standard_normal((E, nq, ndim))
  dirs = [c * rng.uniform(0.5, 1.5, c.shape) for c in mat]
  dh = 0.002 * rng.standard_normal(hist.shape)
  if ndim == 3:
    dh[..., :3] -= dh[..., :3].mean(axis=-1, keepdims=True)
  dh[..., -1] = np.abs(dh[..., -1])
  h = 1e-4

  def moved(t):
    return tuple(c + t * dc for c, dc in zip(mat, dirs)), hist + t * dh
  sets = [PR.yield_margin(ref, uq, moved(t)[1], *moved(t)[0])[1]
          for t in (h, 0.0, -h)]
  assert (sets[0] == sets[1]).all() and (sets[2] == sets[1]).all()

  geo = (op.parts, op.host, ndim, Q, op.point_weights())

  def gpu_vr(t):
    m, hh = moved(t)
    r = _ops.plasticity_local(_dev(uq), *geo, _dev(m[0]), _dev(m[1]), None,
                              0.0, _dev(m[2]), _dev(m[3]), mode='residual',
                              hist=_dev(hh))[0]
    return float((_np(r) * vq).sum())

  def ref_vr(t):
    m, hh = moved(t)
    return float((PR.grid_residual(ref, uq, hh, *m)[0] * vq).sum())

  def contract(out):
    return float((out[0] * dh).sum() +
                 sum((o * dc).sum() for o, dc in zip(out[1:5], dirs)))
  got = _ops.plasticity_vjp(_dev(uq), *geo, *(_dev(c) for c in mat),
                            mode='state', hist=_dev(hist), w_q=_dev(vq))
  an_gpu = contract([_np(g) for g in got])
  an_ref = contract(PA.grid_vjp_state(ref, uq, vq, hist, None, *mat))
  err_gpu = abs((gpu_vr(h) - gpu_vr(-h)) / (2 * h) - an_gpu) / abs(an_gpu)
  err_ref = abs((ref_vr(h) - ref_vr(-h)) / (2 * h) - an_ref) / abs(an_ref)
  print(f'ndim={ndim}: quotient against the VJP: kernel {err_gpu:.3e}, '
        f'reference {err_ref:.3e}')
  assert err_ref < 1e-5
  assert err_gpu <= 10.0 * err_ref


@pytest.mark.parametrize('Q', [3, 8])
@pytest.mark.parametrize('ndim', [2, 3])
def test_state_mode_below_yield_is_the_elastic_sensitivity(ndim, Q):
  """Below yield and from virgin material dlam, dmu and drho are those of
  `sfem_elasticity_sens` (two kernels with different orders of operations:
  `FP64_TOL`), dyield and dhard are exactly zero."""
  case = G.three_kinds(2, ndim, MESH_P)
  mesh, fes, ref, op = _kernel_setup(case, Q)
  rng = np.random.default_rng(60 + ndim)
  E, nq = ref.num_elements, ref.Q
  uq, wq = (_dev(rng.standard_normal((E, nq, ndim))) for _ in range(2))
  geo = (op.parts, op.host, ndim, Q, op.point_weights())
  lam = _dev(rng.uniform(0.5, 1.5, (E, nq)))
  got = _ops.plasticity_vjp(uq, *geo, lam, 0.7, 1e30, 0.2, mode='state',
                            w_q=wq, lambda0=1.3)
  want = _ops.elasticity_sens(uq, wq, *geo, lambda0=1.3)
  for k, j, name in ((1, 0, 'dlam'), (2, 1, 'dmu'), (5, 2, 'drho')):
    err = _rel(_np(got[k]), _np(want[j]))
    print(f'ndim={ndim} Q={Q} {name}: {err:.3e}')
    assert err <= FP64_TOL, (name, err)
  assert bool((got[3] == 0).all()) and bool((got[4] == 0).all())


def test_vjp_refusals():
  """Wrong shapes, modes and missing inputs are refused before a launch."""
  ndim, Q = 2, 3
  case = G.affine(2, ndim, MESH_P)
  mesh, fes, ref, op = _kernel_setup(case, Q)
  E, nq, NH = ref.num_elements, ref.Q, PR.NH[ndim]
  u = torch.zeros((E, nq, ndim), dtype=torch.float64, device=DEV)
  geo = (op.parts, op.host, ndim, Q, op.point_weights(), 1.0, 1.0, 1.0, 0.1)
  good = torch.zeros((E, nq, NH), dtype=torch.float64, device=DEV)
  with pytest.raises(ValueError, match='hbar'):
    _ops.plasticity_vjp(u, *geo, mode='displacement',
                        hbar=torch.zeros((E, nq, NH + 1), dtype=torch.float64,
                                         device=DEV))
  with pytest.raises(ValueError, match='hbar'):
    _ops.plasticity_vjp(u, *geo, mode='displacement')
  with pytest.raises(ValueError, match='mode'):
    _ops.plasticity_vjp(u, *geo, mode='residual', hbar=good)
  with pytest.raises(ValueError, match='second field'):
    _ops.plasticity_vjp(u, *geo, mode='state', hbar=good)
  with pytest.raises(ValueError, match='state mode only'):
    _ops.plasticity_vjp(u, *geo, mode='displacement', hbar=good, w_q=u)
  with pytest.raises(ValueError, match='output'):
    _ops.plasticity_vjp(u, *geo, mode='state', w_q=u, want=(False,) * 5,
                        want_history=False)


# ------------------------------------------------ the assembled operator
def _leaf(a):
  return _tensor(a).requires_grad_()


def _tensor(a):
  """A NumPy array or a number as an fp64 device tensor (0-dim for a number)."""
  if np.ndim(a) == 0:
    return torch.tensor(float(a), dtype=F64, device=DEV)
  return _dev(a)


@pytest.mark.parametrize('ndim', [2, 3])
def test_operator_history_vjp_and_sensitivity(ndim):
  """`history_vjp` and `sensitivity` against the dense reference
  (`PA.history_vjp`, `PA.state_vjp`) on a mesh with all three geometry kinds,
  away from yield (1e-6, asserted): a per-component mask, dense and
  component-major layouts, scalar, (E,), (E, Q^d) and callable sources, an
  absent density, `want` subsets, `want_history`, a virgin history, and the
  shape refusals.  Bound 1e-10, that of the forward operator's test."""
  mesh, fes, ref, rp, fns, vals = _assembled(ndim)
  rng = np.random.default_rng(20 + ndim)
  E, nq = mesh.num_elements, ref.Q
  lam = 1.0 + 0.5 * rng.random((E, nq))
  mu_e = 0.7 + 0.3 * rng.random(E)
  mu = PA.expand_coefficient(mu_e, E, nq)
  sy, Hh, rho = vals[2], 0.25, 1.5
  u, hist = _nodal_state(ref, (lam, mu, sy, Hh, rho), rng, 1e-6)
  w = rng.standard_normal(u.shape)
  hbar = rng.standard_normal(hist.shape)
  fixed = rng.uniform(size=(mesh.num_nodes, ndim)) < 0.25
  keep = (~fixed).astype(float)
  l0 = 0.9
  op = fes.plasticity_operator(
      _dev(fixed, torch.bool), lame_lambda=_dev(lam), lame_mu=_dev(mu_e),
      yield_stress=_dev(sy), hardening_modulus=Hh, density=rho)
  ud, wd, hd, hb = _dev(u), _dev(w), _dev(hist), _dev(hbar)
  before = hd.clone(), hb.clone()

  want_u = PA.history_vjp(ref, u, hist, hbar, lam, mu, sy, Hh, keep)
  got = op.history_vjp(ud, hd, hb)
  assert got.is_contiguous() and _rel(_np(got), want_u) <= 1e-10
  cm = layout.component_major(ud)
  got = op.history_vjp(cm, hd, hb)
  assert layout.is_component_major(got) and _rel(_np(got), want_u) <= 1e-10
  want_v = PA.history_vjp(ref, u, PR.virgin(ref), hbar, lam, mu, sy, Hh, keep)
  assert _rel(_np(op.history_vjp(ud, None, hb)), want_v) <= 1e-10

  want_s = PA.state_vjp(ref, u, w, hist, hbar, lam, mu, sy, Hh, l0)
  forms = ('point', 'elem', 'point', 'scalar', 'scalar')
  for fields in ((ud, wd), (cm, layout.component_major(wd))):
    grads, hprev = op.sensitivity(*fields, hd, hb, l0)
    assert _rel(_np(hprev), want_s[0]) <= 1e-10
    for g, ws, f in zip(grads, want_s[1:], forms):
      ws = PA.reduce_coefficient(ws, f)
      assert tuple(g.shape) == np.shape(ws), f
      assert _rel(_np(g), np.asarray(ws)) <= 1e-10, f
  assert torch.equal(hd, before[0]) and torch.equal(hb, before[1])
  # hbar = None and history = None
  grads, hprev = op.sensitivity(ud, wd, None, None, l0)
  want0 = PA.state_vjp(ref, u, w, PR.virgin(ref), np.zeros_like(hist), lam, mu,
                       sy, Hh, l0)
  assert _rel(_np(hprev), want0[0]) <= 1e-10
  assert _rel(_np(grads[1]), PA.reduce_coefficient(want0[2], 'elem')) <= 1e-10
  # subsets
  for subset in ((True, False, False, False, False),
                 (False, False, True, True, False),
                 (False, True, False, False, True)):
    grads, hprev = op.sensitivity(ud, wd, hd, hb, l0, want=subset,
                                  want_history=False)
    assert hprev is None
    for g, on in zip(grads, subset):
      assert (g is not None) == on
  assert op.sensitivity(ud, wd, hd, hb, want=(False,) * 5,
                        want_history=False) == ((None,) * 5, None)
  # callables and an absent density give None; a per-point hardening modulus
  op2 = fes.plasticity_operator(
      lame_lambda=_t(fns[0]), lame_mu=0.8, yield_stress=_t(fns[2]),
      hardening_modulus=_dev(np.full((E, nq), Hh)))
  grads, hprev = op2.sensitivity(ud, wd, hd, hb)
  assert grads[0] is None and grads[2] is None and grads[4] is None
  assert grads[1].shape == () and tuple(grads[3].shape) == (E, nq)
  assert hprev is not None
  with pytest.raises(ValueError, match='hbar'):
    op.history_vjp(ud, hd, hb[:, :, :-1])
  with pytest.raises(ValueError, match='hbar'):
    op.history_vjp(ud, hd, None)
  with pytest.raises(ValueError, match='hbar'):
    op.sensitivity(ud, wd, hd, hb[:-1])
  with pytest.raises(ValueError, match='history'):
    op.sensitivity(ud, wd, hd[:, :-1], hb)
  with pytest.raises(ValueError, match='want'):
    op.sensitivity(ud, wd, hd, hb, want=(True, True, True))
  with pytest.raises(ValueError):
    op.sensitivity(ud, wd[:-1], hd, hb)


# -------------------------------------------- gradients through the solve
# Newton to 1e-11 of the residual at the start of each entry, inexact steps to
# 1e-8, the adjoint CG to 1e-12: the adjoint solves' accuracy is the
# gradient's.
SOLVE_KW = dict(newton_rtol=1e-11, linear_rtol=1e-8, adjoint_rtol=1e-12,
                max_newton=40)
INPUTS = ('force', 'lam', 'mu', 'sy', 'Hh', 'rho', 'history')


@functools.lru_cache(maxsize=None)
def _solve_setup(ndim, lambda0):
  """`PA.SolveProblem` on the GPU next to its dense reference; the reference
  path and its adjoint are computed once."""
  rp, _, _ = PA.EA.AJ.solve_problem(ndim)
  mesh = rp.finalize(device=DEV)
  facets = mesh.boundary_facets['x1'].cpu().numpy().astype(np.int64)
  prob = PA.SolveProblem(ndim, lambda0, facets)
  roller = [None] * ndim
  roller[1] = _t(prob.roll)
  bcs = {'y0': (D, tuple(roller)),
         'x0': (D, tuple(_t(g) for g in prob.gD)),
         'x1': (N, tuple(g if not callable(g) else _t(g) for g in prob.trac))}
  return dict(mesh=mesh, prob=prob, bcs=bcs)


def _leaves(prob, history=False):
  out = dict(force=_leaf(prob.force), lam=_leaf(prob.lam_q),
             mu=_leaf(prob.mu_e), sy=_leaf(prob.sy_q), Hh=_leaf(prob.Hh),
             rho=_leaf(prob.rho))
  out['history'] = _leaf(PR.virgin(prob.fes)) if history else None
  return out


def _gpu_solve(s, pc, c, differentiable=True, **kw):
  prob = s['prob']
  kw = {**SOLVE_KW, 'load_factors': prob.PATH, **kw}
  if not differentiable:
    kw.pop('adjoint_rtol', None)
  u, h, info = solve_plasticity(
      s['mesh'], c['force'], s['bcs'], lame_lambda=c['lam'], lame_mu=c['mu'],
      yield_stress=c['sy'], hardening_modulus=c['Hh'], density=c['rho'],
      history=c.get('history'), lambda0=prob.lambda0, preconditioner=pc,
      return_info=True, differentiable=differentiable, **kw)
  assert info['status'] == 'converged'
  return u, h, info


def _detached(c):
  return {k: (v.detach() if isinstance(v, torch.Tensor) else v)
          for k, v in c.items()}


def _bound(s, pc, c, path=None):
  """100 sum_k cond_k max(rho_k, 1e-12): cond_k of the reference's dense free
  tangent at entry k, rho_k the relative residual the reference finds at the
  GPU's u_k, which comes from following the path one entry per call through
  `history=` and `u0=`; rho_k <= 1e-9 is asserted."""
  prob = s['prob']
  path = prob.PATH if path is None else path
  conds = prob.gradients()['cond']
  c = _detached(c)
  u, h = None, c.get('history')
  total, rhos = 0.0, []
  for k, scale in enumerate(path):
    h_prev = PR.virgin(prob.fes) if h is None else _np(h)
    u, h, _ = _gpu_solve(s, pc, {**c, 'history': h}, differentiable=False,
                         load_factors=(scale,), u0=u)
    rho_k = prob.relative_residual(_np(u), h_prev, scale)
    assert rho_k <= 1e-9, (k, rho_k)
    rhos.append(rho_k)
    total += conds[k] * max(rho_k, 1e-12)
  return 100.0 * total, rhos


def _check_grads(c, g, bound, names, lambda0):
  forms = dict(force=None, lam=None, mu='elem', sy=None, Hh='scalar',
               rho='scalar', history=None)
  errs = {}
  for name in names:
    got = c[name].grad
    assert got is not None, name
    want = g[name] if forms[name] is None else np.asarray(
        PA.reduce_coefficient(g[name], forms[name]))
    assert tuple(got.shape) == np.shape(want), name
    if name == 'rho' and not lambda0:
      assert float(got) == 0.0
      continue
    errs[name] = _rel(_np(got), want)
    print(f'  d/d{name}: rel err {errs[name]:.2e}')
    assert errs[name] <= bound, (name, errs[name], bound)
  return errs


def _adjoint_statuses(info):
  """One CG info per entry, converged; 'skipped' (nothing launched) only for
  an entry before the last in which no point yielded: its history update does
  not depend on u, so its right-hand side is exactly zero."""
  path = info['load_path']
  assert len(info['adjoint']) == len(path)
  for k, (i, e) in enumerate(zip(info['adjoint'], path)):
    if i['status'] == 'skipped':
      assert k < len(path) - 1 and e['plastic_points'] == 0
      assert i['num_iterations'] == 0
    else:
      assert i['status'] == 'converged', (k, i['status'])
  return [int(i['num_iterations']) for i in info['adjoint']]


@pytest.mark.parametrize('lambda0', [0.0, 0.8])
@pytest.mark.parametrize('pc', [None, 'jacobi'])
@pytest.mark.parametrize('ndim', [2, 3])
def test_solve_gradients_match_path_adjoint(ndim, pc, lambda0):
  """`.grad` of the (N, d) body force, a per-point lame_lambda, a per-element
  lame_mu, a per-point yield_stress, a scalar hardening_modulus and a scalar
  density of the loss (w_u * u).sum() + (w_h * history).sum() over the path
  (0.6, 1.0, 0.3) against `PA.path_adjoint` on the dense Newton path.  Bound:
  100 sum_k cond_k max(rho_k, 1e-12) (`_bound`).  Measured on an MI355X:
  rho_k 7e-15 .. 1.6e-12, cond_k 1.0e3 .. 6.4e3, bounds 3.9e-7 .. 1.0e-6; u
  within 4.9e-13 and the history within 1.9e-12 of the dense path; force
  3.2e-14 .. 1.6e-12, lam 2.7e-13 .. 2.4e-12, mu 2.8e-13 .. 2.2e-12, sigma_y
  1.3e-13 .. 1.8e-12, Hh 1.6e-14 .. 1.3e-12, rho 1.7e-13 .. 1.0e-12 (DESIGN
  §3.23).  In 3D with lambda0 = 0.8 no point yields in the first entry, whose
  adjoint solve is skipped."""
  s = _solve_setup(ndim, lambda0)
  prob = s['prob']
  c = _leaves(prob)
  u, h, info = _gpu_solve(s, pc, c)
  assert u.grad_fn is not None and h.grad_fn is not None
  assert 'adjoint' not in info
  bound, rhos = _bound(s, pc, c)
  entries, h_ref = prob.entries()
  err_u, err_h = _rel(_np(u), entries[-1][0]), _rel(_np(h), h_ref)
  print(f'ndim={ndim} lambda0={lambda0} {pc}: cond '
        f'{[f"{x:.2e}" for x in prob.gradients()["cond"]]}, rho_k '
        f'{[f"{x:.1e}" for x in rhos]}, bound {bound:.2e}, u rel err '
        f'{err_u:.2e}, history {err_h:.2e}, plastic points '
        f'{[e["plastic_points"] for e in info["load_path"]]}')
  assert err_u <= bound and err_h <= bound
  ((u * _dev(prob.w_u)).sum() + (h * _dev(prob.w_h)).sum()).backward()
  _adjoint_statuses(info)
  _check_grads(c, prob.gradients(), bound, INPUTS[:-1], lambda0)


@functools.lru_cache(maxsize=None)
def _cd_base():
  """The 2D problem with lambda0 = 0.8 under Jacobi, solved once to a tight
  tolerance with every input a leaf (the history included)."""
  s = _solve_setup(2, 0.8)
  prob = s['prob']
  c = _leaves(prob, history=True)
  u, h, _ = _gpu_solve(s, 'jacobi', c, newton_rtol=1e-13, linear_rtol=1e-10,
                       adjoint_rtol=1e-13)
  ((u * _dev(prob.w_u)).sum() + (h * _dev(prob.w_h)).sum()).backward()
  return s, c


@pytest.mark.parametrize('name', INPUTS)
def test_central_difference_through_the_solve(name):
  """One central difference per input (h = `PA.CD_H`, the directions of the
  host test) through the GPU solve against its own `.grad`: 2D, lambda0 = 0.8,
  Jacobi.  10 times the floor that the host test asserts for the dense
  reference's own quotient (`PA.CD_FLOOR`) is allowed.  Measured on an MI355X:
  force 9.8e-11, lam 2.5e-9, mu 8.1e-9, sigma_y 2.1e-9, Hh 1.0e-8, rho 6.7e-10,
  history 4.1e-10."""
  s, c = _cd_base()
  prob = s['prob']
  rng = np.random.default_rng(11)
  rel = lambda a: a * rng.uniform(0.5, 1.5, np.shape(a))
  mq = prob.mu_q()
  dirs = dict(force=rel(prob.force), lam=rel(prob.lam_q), mu=rel(mq),
              sy=rel(prob.sy_q), Hh=prob.Hh * 1.2,
              history=0.01 * PR.random_history(prob.fes, rng, size=1.0),
              rho=1.0)
  base = dict(force=prob.force, lam=prob.lam_q, mu=mq, sy=prob.sy_q,
              Hh=prob.Hh, rho=prob.rho, history=PR.virgin(prob.fes))
  dirn = dirs[name]
  grad = c[name].grad
  if name == 'mu':    # the leaf is per element: the direction's element sums
    an = float((grad * _dev(dirn).sum(dim=1) / mq.shape[1]).sum())
    dirn = np.repeat((dirn.sum(axis=1) / mq.shape[1])[:, None], mq.shape[1], 1)
  else:
    an = float((grad * _tensor(dirn)).sum())
  h = PA.CD_H
  w_u, w_h = _dev(prob.w_u), _dev(prob.w_h)

  def val(t):
    cc = {k: _tensor(v) for k, v in base.items()}
    cc[name] = _tensor(base[name] + t * dirn)
    u, hh, _ = _gpu_solve(s, 'jacobi', cc, differentiable=False,
                          newton_rtol=1e-13, linear_rtol=1e-10)
    return float((u * w_u).sum() + (hh * w_h).sum())
  cd = (val(h) - val(-h)) / (2 * h)
  err = abs(cd - an) / abs(an)
  print(f'{name}: quotient {cd:+.8e}, .grad {an:+.8e}, rel {err:.2e} '
        f'(allowed {10.0 * PA.CD_FLOOR[name]:.0e})')
  assert err <= 10.0 * PA.CD_FLOOR[name], (name, err)


def test_pmultigrid_in_forward_and_adjoint():
  """`ElasticityPMultigrid` (built once on the linear operator) preconditions
  the Newton steps and the adjoint solves of the 3D problem: gradients within
  the bound of `test_solve_gradients_match_path_adjoint`; the adjoint CG
  counts are printed next to Jacobi's.  Measured on an MI355X: 24, 51 and 24
  adjoint CG iterations per entry against Jacobi's 173, 256 and 174."""
  s = _solve_setup(3, 0.0)
  prob = s['prob']
  its = {}
  for pc in ('jacobi', ElasticityPMultigrid):
    c = _leaves(prob)
    u, h, info = _gpu_solve(s, pc, c)
    bound, rhos = _bound(s, pc, c)
    ((u * _dev(prob.w_u)).sum() + (h * _dev(prob.w_h)).sum()).backward()
    its[pc] = _adjoint_statuses(info)
    print(f'{getattr(pc, "__name__", pc)}: adjoint CG iterations {its[pc]}, '
          f'forward CG {info["num_cg"]}, bound {bound:.2e}')
    _check_grads(c, prob.gradients(), bound, INPUTS[:-1], 0.0)
  print(f'adjoint CG iterations per entry: p-multigrid '
        f'{its[ElasticityPMultigrid]}, Jacobi {its["jacobi"]}')


@pytest.mark.parametrize('ndim', [2, 3])
def test_chaining_through_history(ndim):
  """Following (0.6, 1.0) in one differentiable call gives the gradients of
  two calls linked through the returned history (which carries a grad_fn
  into `history=`) and u (detached into `u0=`), to the bound of
  `test_solve_gradients_match_path_adjoint`: the second call's gradient with
  respect to its input history drives the first call's backward.  Measured on
  an MI355X: at most 2.3e-13."""
  s = _solve_setup(ndim, 0.8)
  prob = s['prob']
  w_u, w_h = _dev(prob.w_u), _dev(prob.w_h)
  one = _leaves(prob)
  u, h, _ = _gpu_solve(s, 'jacobi', one, load_factors=(0.6, 1.0))
  bound, _ = _bound(s, 'jacobi', one, path=(0.6, 1.0))
  ((u * w_u).sum() + (h * w_h).sum()).backward()
  two = _leaves(prob)
  u1, h1, _ = _gpu_solve(s, 'jacobi', two, load_factors=(0.6,))
  assert h1.grad_fn is not None
  u2, h2, info = _gpu_solve(s, 'jacobi', {**two, 'history': h1},
                            load_factors=(1.0,), u0=u1.detach())
  assert _rel(_np(u2), _np(u)) <= bound and _rel(_np(h2), _np(h)) <= bound
  ((u2 * w_u).sum() + (h2 * w_h).sum()).backward()
  for name in INPUTS[:-1]:
    a, b = one[name].grad, two[name].grad
    err = _rel(_np(b), _np(a))
    print(f'ndim={ndim} d/d{name}: one call against two, rel {err:.2e} '
          f'(bound {bound:.2e})')
    assert err <= bound, name


@pytest.mark.parametrize('ndim', [2, 3])
def test_loss_on_alpha_alone(ndim):
  """A loss on the equivalent plastic strain alone: ubar_K = 0, so the
  displacement mode of the VJP kernel carries everything into the adjoint
  solves.  Against `PA.path_adjoint` with the same cotangents."""
  s = _solve_setup(ndim, 0.0)
  prob = s['prob']
  rng = np.random.default_rng(90 + ndim)
  hbar = np.zeros_like(prob.w_h)
  hbar[..., -1] = rng.uniform(0.5, 1.5, hbar.shape[:2])
  entries, _ = prob.entries()
  want = PA.path_adjoint(prob.dense(), entries, prob.fixed,
                         np.zeros_like(prob.w_u), hbar)
  c = _leaves(prob)
  u, h, info = _gpu_solve(s, 'jacobi', c)
  bound, _ = _bound(s, 'jacobi', c)
  (h[..., -1] * _dev(hbar[..., -1])).sum().backward()
  # the third entry is elastic: its history update does not depend on u, its
  # right-hand side is exactly zero and nothing is solved there
  assert [i['status'] for i in info['adjoint']] == ['converged', 'converged',
                                                    'skipped']
  print(f'ndim={ndim}: bound {bound:.2e}')
  _check_grads(c, want, bound, INPUTS[:-1], 0.0)


def test_unchanged_behaviour_and_refusals(monkeypatch):
  """Without the keyword inputs that require grad are refused as before.  With
  it and nothing requiring grad (or under `torch.no_grad()`) the body runs
  exactly as by default: one call of `_solve` with the caller's own arguments
  and no `_state`, whose (u, history) are returned as they are -- the very
  tensors, so bitwise what the plain body computed -- without a `grad_fn`.
  With a leaf the node hands the body detached inputs and returns bitwise
  what the body computed.  Two separate calls are compared to 2 sum_k cond_k
  newton_rtol, not bitwise: shared nodes and inner products are summed with
  float atomics in this project, so two identical plain calls already differ
  in the last bits (as `tests/test_gpu_hyperelastic_adjoint.py` notes);
  whether they were equal is printed.  A `u0` that requires grad and a wrong
  `hbar` shape are refused."""
  from swirl_fem_amd.examples import plasticity as pl
  body = pl._solve
  seen = []

  def recording(mesh, force, bcs, **kw):
    out = body(mesh, force, bcs, **kw)
    seen.append((force, kw, out, out[0].clone(), out[1].clone()))
    return out
  monkeypatch.setattr(pl, '_solve', recording)
  s = _solve_setup(2, 0.0)
  prob = s['prob']
  c = _detached(_leaves(prob))
  for name in INPUTS[:-1]:
    with pytest.raises(NotImplementedError, match='autograd'):
      _gpu_solve(s, None, {**c, name: c[name].clone().requires_grad_()},
                 differentiable=False)
  with pytest.raises(NotImplementedError, match='autograd'):
    _gpu_solve(s, None, {**c, 'history': _leaf(PR.virgin(prob.fes))},
               differentiable=False)
  assert not seen
  bound = 2.0 * sum(prob.gradients()['cond']) * SOLVE_KW['newton_rtol']
  u_a, h_a, info_a = _gpu_solve(s, 'jacobi', c, differentiable=False)
  del seen[:]
  u_b, h_b, info_b = _gpu_solve(s, 'jacobi', c, differentiable=True)
  assert len(seen) == 1
  assert seen[0][2][0] is u_b and seen[0][2][1] is h_b
  assert torch.equal(u_b, seen[0][3]) and torch.equal(h_b, seen[0][4])
  assert '_state' not in seen[0][1] and 'adjoint' not in info_b
  assert seen[0][0] is c['force'] and seen[0][1]['lame_lambda'] is c['lam']
  assert seen[0][1]['yield_stress'] is c['sy']
  assert u_b.grad_fn is None and h_b.grad_fn is None
  assert not u_b.requires_grad and not h_b.requires_grad
  print(f'flagged against plain call: bitwise equal {torch.equal(u_a, u_b)}, '
        f'rel diff u {_rel(_np(u_b), _np(u_a)):.2e}, history '
        f'{_rel(_np(h_b), _np(h_a)):.2e} (bound {bound:.2e})')
  assert _rel(_np(u_b), _np(u_a)) <= bound
  assert _rel(_np(h_b), _np(h_a)) <= bound
  # a leaf: the node hands the body detached inputs, returns what it computed
  leaves = _leaves(prob)
  del seen[:]
  u_t, h_t, _ = _gpu_solve(s, 'jacobi', leaves)
  assert u_t.grad_fn is not None and len(seen) == 1
  force, kw, _, u_body, h_body = seen[0]
  assert not force.requires_grad and not kw['yield_stress'].requires_grad
  assert isinstance(kw['_state'], dict)
  assert torch.equal(u_t.detach(), u_body)
  assert torch.equal(h_t.detach(), h_body)
  assert _rel(_np(u_t), _np(u_a)) <= bound
  del seen[:]
  with torch.no_grad():   # leaves under no_grad: the plain body as well
    u_c, h_c, _ = _gpu_solve(
        s, 'jacobi', {**c, 'lam': leaves['lam'], 'sy': leaves['sy']},
        differentiable=True)
  assert len(seen) == 1 and '_state' not in seen[0][1]
  assert seen[0][2][0] is u_c and u_c.grad_fn is None and h_c.grad_fn is None
  assert _rel(_np(u_c), _np(u_a)) <= bound
  with pytest.raises(NotImplementedError, match='u0'):
    _gpu_solve(s, None, c, u0=u_a.clone().requires_grad_())
  mesh, fes, ref, rp, fns, vals = _assembled(2)
  op = fes.plasticity_operator(lame_lambda=1.0, lame_mu=1.0, yield_stress=1.0)
  u = torch.zeros((mesh.num_nodes, 2), dtype=F64, device=DEV)
  bad = torch.zeros(op.history_shape()[:2] + (3,), dtype=F64, device=DEV)
  with pytest.raises(ValueError, match='hbar'):
    op.history_vjp(u, None, bad)
  with pytest.raises(ValueError, match='hbar'):
    op.sensitivity(u, u, None, bad)
