"""J2 plasticity on the GPU: the kernel `sfem_plasticity_local`,
residual and tangent modes, at every Q = 2..12 against the NumPy reference
(`tests/plasticity_reference.py`); the assembled operator (masks, layouts,
symmetry, the derivative relation away from yield, linear elasticity below
yield); `solve_plasticity` against the closed-form uniaxial curve and the
dense Newton of the reference over load-unload paths, the preconditioners on
a clamped box, continuation through `history`, and the refusals.

Random displacement fields are scaled, from the reference, so that about half
of the points yield; each test asserts a share between 20 % and 80 % before
it looks at the kernel.  Residual, trial history and stress are continuous in
the input and are compared everywhere.  `lin` = (a, b, n) jumps at the yield
surface, so it is compared at the points with |f| / sigma_y >= MARGIN[dtype]
only; the share of excluded points is asserted, from the reference, to be at
most 1 %."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from swirl_fem_amd import _lib, _ops
from swirl_fem_amd.core import layout, operators
from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import NodeType, Quadrature1D
from swirl_fem_amd.examples.plasticity import BCType, solve_plasticity
from swirl_fem_amd.linalg.pmg_elasticity import ElasticityPMultigrid
from tests import elasticity_reference as ER
from tests import geometry_cases as G
from tests import plasticity_reference as PR
from tests import transport_reference as TR
from tests.fp32util import F32Rng, f32r, tolerance

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GL = NodeType.GAUSS_LEGENDRE
D, N = BCType.DIRICHLET, BCType.NEUMANN
MESH_P = 3       # nodes per direction of the kernel tests' meshes
FP64_TOL = 1e-11
MARGIN = {torch.float64: 1e-9, torch.float32: 1e-3}
MAX_EXCLUDED = 0.01

# (lambda, mu, rho: 'p' per point around the number, or the scalar; lambda0;
# sigma_y, Hh likewise): the combinations of the hyperelastic kernel's test,
# extended; the third has Hh = 0, the last passes no history (virgin)
KERNEL_COMBOS = [
    (1.3, 0.7, None, 0.0, 0.05, 0.2),
    (('p', 1.0), ('p', 0.8), ('p', 1.5), 2.5, ('p', 0.05), ('p', 0.2)),
    (('p', 0.9), 0.6, ('p', 2.0), 0.0, 0.04, 0.0),
    (0.0, ('p', 0.8), 1.5, 0.7, ('p', 0.06), 0.3),
    (50.0, 1.0, None, 0.0, 0.05, ('p', 0.1)),
    (('p', 50.0), ('p', 1.0), None, 1.1, 0.05, 0.2),
]
VIRGIN_COMBO = 5


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
  ref = PR.space(rp.node_coords, rp.elements, MESH_P, (Q, 'gl'))
  op = fes.plasticity_operator(lame_lambda=1.0, lame_mu=1.0, yield_stress=1.0)
  return mesh, fes, ref, op


def _half_plastic(ref, uq, hist, mat, rnd, margin=0.0, share=0.5):
  """`uq` scaled, from the reference, so that about `share` of the points
  yield (asserted to lie in [0.2, 0.8]).  Bisection on the scale alone would
  put the median point exactly on the yield surface, so the scale found is
  raised by 2 to 8 %: by the step that leaves the fewest points within
  `margin` (relative to sigma_y) of the surface."""
  h = PR.virgin(ref) if hist is None else hist
  frac = lambda s: PR.yield_margin(ref, s * uq, h, *mat)[1].mean()
  lo, hi = 0.0, 1.0
  while frac(hi) < share:
    hi *= 2.0
  for _ in range(25):
    mid = 0.5 * (lo + hi)
    lo, hi = (mid, hi) if frac(mid) < share else (lo, mid)
  best = None
  for step in (0.02, 0.035, 0.05, 0.065, 0.08):
    cand = rnd(hi * (1.0 + step) * uq)
    f, plastic = PR.yield_margin(ref, cand, h, *mat)
    near = int((np.abs(f) < margin).sum())
    if best is None or near < best[0]:
      best = (near, cand, plastic.mean())
  assert 0.2 <= best[2] <= 0.8, best[2]
  return best[1]


def _away_from_yield(ref, uq, hist, mat, margin, rnd):
  """The history with eps_p redrawn nearby (by a trace-free step that moves f
  by a few margins) at the points within `margin` of the yield surface, until
  none is left there."""
  hist = hist.copy()
  rng = np.random.default_rng(0)
  ne = hist.shape[-1] - 1
  size = 5.0 * margin * np.max(mat[2]) / np.min(mat[1])
  for _ in range(60):
    f = PR.yield_margin(ref, uq, hist, *mat)[0]
    near = np.abs(f) < 2.0 * margin
    if not near.any():
      return hist
    step = size * rng.standard_normal((int(near.sum()), ne))
    if ref.ndim == 3:
      step[:, :3] -= step[:, :3].mean(axis=1, keepdims=True)
    hist[near, :-1] = rnd(hist[near, :-1] + step)
  raise AssertionError('could not move every point away from yield')


def _check(name, got, want, tol, dtype, ref32, rows, where=None):
  """`got` against the fp64 reference `want` at `tol`; above it in fp32 the
  project's exception rule: 4 times the error of the NumPy reference
  evaluated in float32 (`ref32`, a thunk).  `where`: the points compared."""
  sel = (lambda a: a) if where is None else (lambda a: a[where])
  err = _rel(sel(got), sel(want))
  allowed = tol
  if err > tol and dtype == torch.float32:
    allowed = max(tol, 4.0 * _rel(sel(ref32().astype(np.float64)), sel(want)))
  print(f'  {name}: rel err {err:.3e} (allowed {allowed:.3e})')
  rows.append((name, err, allowed))
  assert err <= allowed, (name, err, allowed)


def _run_combos(op, ref, ndim, Q, pad, rng, dtype, tol, combos,
                rnd=lambda a: a):
  """Each combination, both modes, against `grid_residual` / `grid_tangent`.
  The `pad` trailing rows carry zero displacement and a non-zero history."""
  E, nq = ref.num_elements, ref.Q
  NH, NL, NV = PR.NH[ndim], PR.NL[ndim], PR.NV[ndim]
  margin = MARGIN[dtype]
  rows = []
  for n, combo in combos:
    def coef(c):
      if isinstance(c, tuple):
        return rnd(c[1] * (1.0 + 0.2 * rng.uniform(-1, 1, (E, nq))))
      return c
    lam, mu, rho, l0, sy, Hh = (coef(c) if k != 3 else c
                                for k, c in enumerate(combo))
    mat = (lam, mu, sy, Hh)
    hist = None if n == VIRGIN_COMBO else PR.random_history(ref, rng, rnd=rnd)
    uq = _half_plastic(ref, rng.standard_normal((E, nq, ndim)), hist, mat, rnd,
                       margin)
    wq = rnd(rng.standard_normal((E, nq, ndim)))
    # the cap on the points whose lin is not compared, from the reference
    f, plastic = PR.yield_margin(ref, uq, PR.virgin(ref) if hist is None
                                 else hist, *mat)
    included = np.abs(f) >= margin
    excluded = 1.0 - included.mean()
    print(f'{dtype} ndim={ndim} Q={Q} combo {n}: plastic {plastic.mean():.3f}, '
          f'excluded {excluded:.2e}')
    assert excluded <= MAX_EXCLUDED
    want = PR.grid_residual(ref, uq, hist, lam, mu, sy, Hh, rho, l0)
    want_t = PR.grid_tangent(ref, wq, want[2], lam, mu, rho, l0)
    f32 = lambda: PR.grid_residual(ref, uq, hist, lam, mu, sy, Hh, rho, l0,
                                   dtype=np.float32)

    def dev(c):
      if isinstance(c, np.ndarray):
        return _dev(np.concatenate([c, np.ones((pad, nq))]), dtype)
      return c

    def padded(a, fill=0.0):
      return _dev(np.concatenate([a, np.full((pad,) + a.shape[1:], fill)]),
                  dtype)
    args = (op.parts, op.host, ndim, Q, op.point_weights(), dev(lam), dev(mu),
            dev(rho), l0, dev(sy), dev(Hh))
    hist_d = None if hist is None else padded(hist, 0.01)
    before = None if hist is None else hist_d.clone()
    got_r, got_h, got_l, got_s = _ops.plasticity_local(
        padded(uq), *args, mode='residual', hist=hist_d, want_hist=True,
        want_lin=True, want_stress=True)
    assert got_r.shape == (E + pad, nq, ndim) and got_r.dtype == dtype
    assert got_h.shape == (E + pad, nq, NH) and got_l.shape == (E + pad, nq, NL)
    assert got_s.shape == (E + pad, nq, NV)
    for t in (got_r, got_h, got_l, got_s):   # the padded row holds finite values
      assert bool(torch.isfinite(t).all())
    if hist is not None:                     # the committed history is read only
      assert torch.equal(hist_d, before)
    _check('residual', _np(got_r)[:E], want[0], tol, dtype, lambda: f32()[0],
           rows)
    _check('history', _np(got_h)[:E], want[1], tol, dtype, lambda: f32()[1],
           rows)
    _check('stress', _np(got_s)[:E], want[3], tol, dtype, lambda: f32()[3],
           rows)
    _check('lin', _np(got_l)[:E], want[2], tol, dtype, lambda: f32()[2], rows,
           where=included)
    # without the optional outputs the residual is the same
    only_r, *none = _ops.plasticity_local(padded(uq), *args, mode='residual',
                                          hist=hist_d)
    assert none == [None, None, None]
    assert torch.equal(only_r[:E], got_r[:E])
    # the tangent with the state of the reference: a wrong state cannot
    # cancel a wrong tangent
    t32 = lambda: PR.grid_tangent(ref, wq, want[2], lam, mu, rho, l0,
                                  dtype=np.float32)
    got_t = _ops.plasticity_local(padded(wq), *args, mode='tangent',
                                  lin=padded(want[2]))
    assert got_t.shape == (E + pad, nq, ndim) and got_t.dtype == dtype
    assert bool(torch.isfinite(got_t).all())
    _check('tangent, reference lin', _np(got_t)[:E], want_t, tol, dtype, t32,
           rows)
    # and with the state of the kernel, from a history that leaves no point
    # within the margin: the excluded set is empty
    clear = _away_from_yield(
        ref, uq, PR.random_history(ref, rng, rnd=rnd) if hist is None else hist,
        mat, margin, rnd)
    f2 = PR.yield_margin(ref, uq, clear, *mat)[0]
    assert (np.abs(f2) >= margin).all()
    want2 = PR.grid_residual(ref, uq, clear, lam, mu, sy, Hh, rho, l0)
    _, _, lin2, _ = _ops.plasticity_local(
        padded(uq), *args, mode='residual', hist=padded(clear), want_lin=True)
    got_t = _ops.plasticity_local(padded(wq), *args, mode='tangent', lin=lin2)
    _check('tangent, kernel lin', _np(got_t)[:E],
           PR.grid_tangent(ref, wq, want2[2], lam, mu, rho, l0), tol, dtype,
           lambda: PR.grid_tangent(ref, wq, want2[2], lam, mu, rho, l0,
                                   dtype=np.float32), rows)
  return rows


@pytest.mark.parametrize('Q', range(2, 13))
@pytest.mark.parametrize('ndim', [2, 3])
def test_kernel_matches_reference(ndim, Q):
  """fp64, every Q, both modes: scalar and per-point coefficients, rho with
  and without a mass term, lambda = 0, lambda / mu = 50, Hh = 0, a virgin
  (NULL) history, on multilinear and curved elements with a padded row (list
  launches, a partial workgroup)."""
  case = G.three_kinds(2, ndim, MESH_P, pad=1)
  mesh, fes, ref, op = _kernel_setup(case, Q)
  assert len(op.parts) >= 2 and all('elem_list' in p for p in op.parts)
  assert {G.CURVED, G.MULTILINEAR} <= {p['geo_mode'] for p in op.parts}
  rng = np.random.default_rng(100 * ndim + Q)
  _run_combos(op, ref, ndim, Q, 1, rng, torch.float64, FP64_TOL,
              list(enumerate(KERNEL_COMBOS)))


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
  combos = list(enumerate(KERNEL_COMBOS))
  _run_combos(op, ref, ndim, Q, 0, rng, torch.float64, FP64_TOL,
              combos[:3] + combos[VIRGIN_COMBO:])


@pytest.mark.parametrize('Q', [2, 5, 8, 9, 12])
@pytest.mark.parametrize('ndim', [2, 3])
def test_kernel_fp32(ndim, Q):
  """fp32 with float32-representable meshes and inputs against the fp64
  reference at `tolerance(torch.float32, Q)`, every combination, both modes.
  A case above that is held to 4 times the error of the NumPy reference
  evaluated in float32 (DESIGN §3.22 lists them)."""
  case = G.three_kinds(2, ndim, MESH_P)
  mesh, fes, ref, op = _kernel_setup(case, Q, torch.float32)
  rng = F32Rng(Q)
  rows = _run_combos(op, ref, ndim, Q, 0, rng, torch.float32,
                     tolerance(torch.float32, Q),
                     list(enumerate(KERNEL_COMBOS)), rnd=f32r)
  for name, err, allowed in rows:
    if err > tolerance(torch.float32, Q):
      print(f'EXCEPTION ndim={ndim} Q={Q} {name}: {err:.3e} <= {allowed:.3e}')


# ------------------------------------------------ 2. assembled operator
def _coef_fns(ndim):
  lam = lambda x: 1.0 + 0.5 * np.sin(2.0 * x[..., 0]) * x[..., 1]
  mu = lambda x: 0.7 + 0.3 * x[..., ndim - 1] ** 2
  sy = lambda x: 0.05 * (1.0 + 0.2 * np.cos(x[..., 0]))
  Hh = lambda x: 0.2 + 0.1 * x[..., 1]
  rho = lambda x: 1.5 + np.cos(x[..., 0])
  return lam, mu, sy, Hh, rho


@functools.lru_cache(maxsize=None)
def _assembled(ndim):
  """A mesh with all three geometry kinds, the space of a solve on it, the
  reference space and variable coefficients (callables, values)."""
  P = 4 if ndim == 2 else 3
  case = G.three_kinds(3, ndim, P)
  mesh, _, rp = case.finalize(DEV, torch.float64)
  q = P - 1 + (ndim + 1) // 2
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(q, GL))
  ref = PR.space(rp.node_coords, rp.elements, P, (q, 'gl'))
  fns = _coef_fns(ndim)
  xq = PR.quad_points(ref)
  return mesh, fes, ref, rp, fns, tuple(f(xq) for f in fns)


def _operator(ndim, fixed=None, **over):
  mesh, fes, ref, rp, fns, vals = _assembled(ndim)
  kw = dict(lame_lambda=_t(fns[0]), lame_mu=_t(fns[1]),
            yield_stress=_t(fns[2]), hardening_modulus=_t(fns[3]),
            density=_t(fns[4]))
  kw.update(over)
  op = fes.plasticity_operator(
      None if fixed is None else _dev(fixed, torch.bool), **kw)
  assert isinstance(op, operators.PlasticityOperator)
  assert {p['geo_mode'] for p in op.parts} == {G.CURVED, G.MULTILINEAR,
                                              G.AFFINE}
  return op


def _nodal_state(ref, vals, rng, margin):
  """(u, history) with about half of the points plastic and every point at
  least `margin` (relative to sigma_y) away from yield."""
  lam, mu, sy, Hh, rho = vals
  mat = (lam, mu, sy, Hh)
  hist = PR.random_history(ref, rng)
  u = rng.standard_normal((ref.num_nodes, ref.ndim))
  to_grid = lambda v: np.einsum('qi,eic->eqc', ref.M, ref.gather(v))
  uq = _half_plastic(ref, to_grid(u), hist, mat, lambda a: a)
  u = u * (np.abs(uq).max() / np.abs(to_grid(u)).max())
  hist = _away_from_yield(ref, to_grid(u), hist, mat, margin, lambda a: a)
  f, plastic = PR.yield_margin(ref, to_grid(u), hist, *mat)
  assert np.abs(f).min() >= margin and 0.2 <= plastic.mean() <= 0.8
  return u, hist


@pytest.mark.parametrize('ndim', [2, 3])
def test_operator_matches_reference(ndim):
  """`residual`, `linearize`, `tangent.apply` and `stress` against the
  reference: a per-component mask, dense and component-major layouts,
  callable coefficients, with and without the mass term."""
  mesh, fes, ref, rp, fns, vals = _assembled(ndim)
  lam, mu, sy, Hh, rho = vals
  rng = np.random.default_rng(ndim)
  fixed = rng.uniform(size=(mesh.num_nodes, ndim)) < 0.25
  keep = (~fixed).astype(float)
  op = _operator(ndim, fixed)
  u, hist = _nodal_state(ref, vals, rng, 1e-6)
  w = rng.standard_normal(u.shape)
  hd = _dev(hist)
  assert tuple(op.virgin_history().shape) == hist.shape
  assert not bool(op.virgin_history().any())
  for l0 in (0.0, 1.7):
    want, wh, wl, ws = PR.residual(ref, u, hist, lam, mu, sy, Hh, rho, l0,
                                   keep=keep)
    dense = op.residual(_dev(u), hd, l0)
    assert dense.is_contiguous()
    assert _rel(_np(dense), want) <= 1e-10
    cm = layout.component_major(_dev(u))
    got = op.residual(cm, hd, l0)
    assert layout.is_component_major(got) and got.stride() == cm.stride()
    assert _rel(_np(got), want) <= 1e-10
    lin = op.linearize(_dev(u), hd, l0)
    assert _rel(_np(lin.residual), want) <= 1e-10
    assert tuple(lin.lin.shape) == (mesh.num_elements, ref.Q, PR.NL[ndim])
    assert _rel(_np(lin.lin), wl) <= 1e-10
    assert _rel(_np(lin.history), wh) <= 1e-10
    assert lin.num_plastic() == int((wl[..., 1] != 0).sum())
    assert np.array_equal(_np(hd), hist)
    T = op.tangent(lin, l0)
    want_t = PR.tangent(ref, w, wl, lam, mu, rho, l0, keep=keep)
    assert _rel(_np(T.apply(_dev(w))), want_t) <= 1e-10
    got = T.apply(layout.component_major(_dev(w)))
    assert layout.is_component_major(got)
    assert _rel(_np(got), want_t) <= 1e-10
    assert _rel(_np(T.linear_operator()(_dev(w))), want_t) <= 1e-10
    assert _rel(_np(op.tangent(lin.lin, l0).apply(_dev(w))), want_t) <= 1e-10
  sigma, trial = op.stress(_dev(u), hd)
  assert _rel(_np(sigma), ws) <= 1e-10 and _rel(_np(trial), wh) <= 1e-10
  # at the plastic points the von Mises stress sits on the hardened surface
  vm = _np(operators.von_mises(sigma, ndim))
  pl = wl[..., 1] != 0
  assert np.abs(vm - (sy + Hh * wh[..., -1]))[pl].max() <= 1e-12
  # virgin material through None; (N,) mask; scalar coefficients
  nodes = rng.uniform(size=mesh.num_nodes) < 0.3
  op1 = fes.plasticity_operator(_dev(nodes, torch.bool), lame_lambda=2.0,
                                lame_mu=0.5, yield_stress=0.03)
  keep = np.repeat((~nodes)[:, None], ndim, axis=1).astype(float)
  want = PR.residual(ref, u, PR.virgin(ref), 2.0, 0.5, 0.03, 0.0, keep=keep)[0]
  assert _rel(_np(op1.residual(_dev(u))), want) <= 1e-10
  assert _rel(_np(op1.residual(_dev(u), op1.virgin_history())), want) <= 1e-10


@pytest.mark.parametrize('ndim', [2, 3])
def test_tangent_symmetry_and_derivative(ndim):
  """|v . T w - w . T v| <= 1e-12 |v| |T w|; T w against the central
  difference of the residual on the device (h = 1e-6, 1e-6 relative) on a
  state whose points are all at least 1e-2 sigma_y away from yield, so that
  no point changes branch within the difference."""
  mesh, fes, ref, rp, fns, vals = _assembled(ndim)
  op = _operator(ndim)
  rng = np.random.default_rng(3)
  u, hist = _nodal_state(ref, vals, rng, 1e-2)
  u, hd = _dev(u), _dev(hist)
  v = _dev(rng.standard_normal((mesh.num_nodes, ndim)))
  w = _dev(rng.standard_normal((mesh.num_nodes, ndim)))
  h = 1e-6
  for l0 in (0.0, 0.9):
    T = op.tangent(op.linearize(u, hd, l0), l0)
    Tw, Tv = T.apply(w), T.apply(v)
    a, b = float((v * Tw).sum()), float((w * Tv).sum())
    scale = float(v.norm() * Tw.norm())
    print(f'{ndim}D lambda0={l0}: |vTw - wTv| / (|v||Tw|) = '
          f'{abs(a - b) / scale:.2e}')
    assert abs(a - b) <= 1e-12 * scale
    fd = (op.residual(u + h * w, hd, l0) -
          op.residual(u - h * w, hd, l0)) / (2 * h)
    err = _rel(_np(fd), _np(Tw))
    print(f'{ndim}D lambda0={l0}: central difference vs tangent {err:.2e}')
    assert err <= 1e-6


@pytest.mark.parametrize('ndim', [2, 3])
def test_below_yield_is_linear_elasticity(ndim):
  """With sigma_y above every trial stress, `residual` and `tangent.apply`
  equal `ElasticityOperator.apply` to 1e-12 and nothing yields."""
  mesh, fes, ref, rp, fns, vals = _assembled(ndim)
  rng = np.random.default_rng(5)
  fixed = rng.uniform(size=(mesh.num_nodes, ndim)) < 0.2
  op = _operator(ndim, fixed, yield_stress=1e6)
  u = _dev(rng.standard_normal((mesh.num_nodes, ndim)))
  w = _dev(rng.standard_normal((mesh.num_nodes, ndim)))
  for l0 in (0.0, 1.3):
    lin = op.linearize(u, None, l0)
    want = op.linear.apply(u, l0)
    assert _rel(_np(lin.residual), _np(want)) <= 1e-12
    assert lin.num_plastic() == 0 and not bool(lin.history.any())
    got = op.tangent(lin, l0).apply(w)
    assert _rel(_np(got), _np(op.linear.apply(w, l0))) <= 1e-12


# -------------------------------------------------------------- 3. solves
def _facets(mesh, group):
  return mesh.boundary_facets[group].cpu().numpy().astype(np.int64)


def _on(x, axis, value):
  return np.abs(x[:, axis] - value) < 1e-9


def test_uniaxial_bar():
  """A 3D bar with rollers on x0, y0, z0, free sides and a prescribed end
  displacement, on a mesh with a moved interior vertex: loaded past yield,
  unloaded to zero stress, reloaded beyond.  The state is homogeneous, so
  every quadrature point must follow `uniaxial_curve`: sigma_xx, alpha and
  eps_p,xx to 1e-7 sigma_y (newton_rtol = 1e-10), the other stresses zero."""
  ndim = 3
  Em, nu, sy, Hh = 2.0, 0.3, 0.01, 0.5
  lam, mu = operators.lame_parameters(Em, nu)
  rp = ER.jittered_box(2, ndim, 3)
  mesh = rp.finalize(device=DEV)
  top = 4 * sy / Em
  bcs = {'x0': (D, (0.0, None, None)), 'y0': (D, (None, 0.0, None)),
         'z0': (D, (None, None, 0.0)), 'x1': (D, (top, None, None))}
  _, _, ep_top = PR.uniaxial_curve(Em, nu, sy, Hh, [top])
  factors = (0.5, 1.0, 0.8, ep_top[0] / top, 1.0, 1.2)
  want_s, want_a, want_e = PR.uniaxial_curve(Em, nu, sy, Hh,
                                             [s * top for s in factors])
  assert abs(want_s[3]) <= 1e-15 and want_a[5] > want_a[1] > 0
  kw = dict(lame_lambda=lam, lame_mu=mu, yield_stress=sy,
            hardening_modulus=Hh, newton_rtol=1e-10, linear_rtol=1e-10,
            preconditioner='jacobi')
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(2 + 2, GL))
  op = fes.plasticity_operator(lame_lambda=lam, lame_mu=mu, yield_stress=sy,
                               hardening_modulus=Hh)
  u, hist = None, None
  for k, s in enumerate(factors):
    prev = hist
    u, hist, info = solve_plasticity(mesh, (0.0,) * 3, bcs, load_factors=(s,),
                                     history=hist, u0=u, return_info=True, **kw)
    assert info['status'] == 'converged'
    sigma, trial = op.stress(u, prev)
    sigma, h = _np(sigma), _np(hist)
    errs = (np.abs(sigma[..., 0] - want_s[k]).max(),
            np.abs(sigma[..., 1:]).max(), np.abs(h[..., -1] - want_a[k]).max(),
            np.abs(h[..., 0] - want_e[k]).max())
    print(f'entry {k} (factor {s:.3f}): Newton '
          f'{len(info["load_path"][0]["step_lengths"])}, plastic points '
          f'{info["load_path"][0]["plastic_points"]}, errors {errs}')
    assert _rel(_np(trial), h) <= 1e-12 or np.abs(_np(trial) - h).max() <= 1e-14
    assert max(errs[:2]) <= 1e-7 * sy and max(errs[2:]) <= 1e-7 * sy / Em
  # the whole path in one call gives the same state
  u1, hist1 = solve_plasticity(mesh, (0.0,) * 3, bcs, load_factors=factors,
                               **kw)
  assert np.abs(_np(u1) - _np(u)).max() <= 1e-9 * top
  assert np.abs(_np(hist1) - _np(hist)).max() <= 1e-9 * top


def _mixed_problem(ndim, P):
  """2 x 2 (x 2) elements of mixed geometry, variable coefficients, a body
  force, a clamp on x0 and a traction on x1; sigma_y is 0.6 times the largest
  von Mises stress of the elastic solution, so the full load yields."""
  rp = TR.box_with_sides(2, ndim, P, three_kinds=True)
  mesh = rp.finalize(device=DEV)
  x = np.asarray(rp.node_coords, np.float64)
  lam, mu, _, Hh, _ = _coef_fns(ndim)
  force = lambda y: 0.5 * np.stack(
      [0.3 * np.sin(2.0 * y[:, 0]), -0.4 + 0.0 * y[:, 0],
       0.2 * y[:, 0] * y[:, 1]][:ndim], axis=-1)
  trac = [0.125, -0.075, 0.05][:ndim]
  fixed = np.zeros(x.shape, bool)
  fixed[_on(x, 0, 0.0)] = True
  tractions = [(_facets(mesh, 'x1'), trac)]
  elastic = PR.DenseNewton(rp, P, lam, mu, 1e6, Hh)
  u_el = ER.Dense.solve(elastic, force(x), fixed, np.zeros(x.shape), tractions)
  s = PR.residual(elastic.fes, u_el, PR.virgin(elastic.fes),
                  *elastic.coefs[:2], 1e6, 0.0)[3]
  vm = _np(operators.von_mises(torch.as_tensor(s), ndim))
  sy = 0.6 * vm.max()
  dense = PR.DenseNewton(rp, P, lam, mu, sy, Hh)
  bcs = {'x0': (D, (0.0,) * ndim), 'x1': (N, tuple(trac))}
  return mesh, x, dense, force, fixed, tractions, bcs, (lam, mu, sy, Hh)


@pytest.mark.parametrize('ndim,order', [(2, 2), (2, 3), (3, 2)])
def test_solve_matches_dense_newton(ndim, order):
  """The mixed mesh over the load-unload path (0.6, 1.0, 0.0) against the
  dense Newton of the reference (plane strain in 2D): displacement and
  history to 1e-8, and with linear_rtol = 1e-12 at most one Newton iteration
  more per entry than the reference needs."""
  P = order + 1
  mesh, x, dense, force, fixed, tractions, bcs, (lam, mu, sy, Hh) = \
      _mixed_problem(ndim, P)
  path = (0.6, 1.0, 0.0)
  want, want_h, counts = dense.solve(force(x), fixed, np.zeros(x.shape),
                                     tractions, load_factors=path, rtol=1e-10)
  assert want_h[..., -1].max() > 0 and (want_h[..., -1] > 0).mean() < 0.9
  u, hist, info = solve_plasticity(
      mesh, _t(force), bcs, lame_lambda=_t(lam), lame_mu=_t(mu),
      yield_stress=sy, hardening_modulus=_t(Hh), load_factors=path,
      newton_rtol=1e-10, linear_rtol=1e-12, preconditioner='jacobi',
      return_info=True)
  its = [len(s['step_lengths']) for s in info['load_path']]
  err, err_h = _rel(_np(u), want), _rel(_np(hist), want_h)
  print(f'{ndim}D order {order}: Newton iterations {its} (reference {counts}), '
        f'plastic points {[s["plastic_points"] for s in info["load_path"]]}, '
        f'rel err u {err:.2e}, history {err_h:.2e}')
  assert [s['factor'] for s in info['load_path']] == list(path)
  assert err <= 1e-8 and err_h <= 1e-8
  assert all(i <= c + 1 for i, c in zip(its, counts))
  assert not _np(u)[fixed].any()
  # the residual displacement after unloading is not zero: permanent set
  assert np.abs(_np(u)).max() >= 1e-6


@functools.lru_cache(maxsize=None)
def _clamped_box():
  """4^3 elements of order 2, clamped on x0, a transverse traction on x1;
  sigma_y is half of the largest von Mises stress of the elastic answer."""
  rp = TR.box_with_sides(4, 3, 3)
  mesh = rp.finalize(device=DEV)
  bcs = {'x0': (D, (0.0, 0.0, 0.0)), 'x1': (N, (None, None, 0.01))}
  kw = dict(lame_lambda=1.5, lame_mu=1.0, hardening_modulus=0.1)
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(2 + 2, GL))
  u, _ = solve_plasticity(mesh, (0.0,) * 3, bcs, yield_stress=1e6,
                          linear_rtol=1e-10, preconditioner='jacobi', **kw)
  op = fes.plasticity_operator(yield_stress=1e6, **kw)
  vm = operators.von_mises(op.stress(u)[0], 3)
  return mesh, bcs, dict(yield_stress=0.5 * float(vm.max()), **kw)


def test_clamped_box_preconditioners():
  """The clamped box in two load steps: None, 'jacobi' and
  `ElasticityPMultigrid` agree to 1e-7, and the material yields somewhere."""
  mesh, bcs, kw = _clamped_box()
  out = {}
  for pc in (None, 'jacobi', ElasticityPMultigrid):
    u, hist, info = solve_plasticity(
        mesh, (0.0,) * 3, bcs, load_factors=2, newton_rtol=1e-10,
        linear_rtol=1e-8, preconditioner=pc, return_info=True, **kw)
    assert info['status'] == 'converged'
    assert [s['status'] for s in info['load_path']] == ['converged'] * 2
    assert [s['factor'] for s in info['load_path']] == [0.5, 1.0]
    out[pc] = (_np(u), _np(hist), info)
    print(f'{getattr(pc, "__name__", pc)}: Newton '
          f'{[len(s["step_lengths"]) for s in info["load_path"]]}, CG '
          f'iterations {info["num_cg"]}, plastic points '
          f'{[s["plastic_points"] for s in info["load_path"]]}')
  u0, h0, info0 = out[None]
  assert h0[..., -1].max() > 0 and h0[..., -1].min() == 0.0
  assert info0['load_path'][-1]['plastic_points'] > 0
  for pc in ('jacobi', ElasticityPMultigrid):
    assert np.abs(out[pc][0] - u0).max() <= 1e-7 * np.abs(u0).max()
    assert np.abs(out[pc][1] - h0).max() <= 1e-7 * np.abs(h0).max()


def test_history_continues_a_solve():
  """(0.5, 1.0) in one call equals (0.5,) and then (1.0,) with the returned
  history and u0."""
  mesh, bcs, kw = _clamped_box()
  kw = dict(newton_rtol=1e-10, linear_rtol=1e-10, preconditioner='jacobi',
            **kw)
  u, hist = solve_plasticity(mesh, (0.0,) * 3, bcs, load_factors=(0.5, 1.0),
                             **kw)
  ua, ha = solve_plasticity(mesh, (0.0,) * 3, bcs, load_factors=(0.5,), **kw)
  keep = ha.clone()
  ub, hb = solve_plasticity(mesh, (0.0,) * 3, bcs, load_factors=(1.0,),
                            history=ha, u0=ua, **kw)
  assert torch.equal(ha, keep)            # the caller's history is not written
  assert _rel(_np(ub), _np(u)) <= 1e-12 and _rel(_np(hb), _np(hist)) <= 1e-12
  assert float(hb[..., -1].max()) > float(ha[..., -1].max())


def test_max_newton_names_the_entry():
  mesh, bcs, kw = _clamped_box()
  with pytest.raises(RuntimeError, match='entry 2 of 2 of the load path'):
    solve_plasticity(mesh, (0.0,) * 3, bcs, load_factors=(0.4, 1.0),
                     max_newton=1, linear_rtol=1e-10, preconditioner='jacobi',
                     **kw)


# ----------------------------------------------------------- 4. refusals
def test_operator_refusals():
  case = G.affine(2, 2, MESH_P)
  mesh, _, rp = case.finalize(DEV, torch.float64)
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(3, GL))
  ok = dict(lame_lambda=1.0, lame_mu=1.0, yield_stress=0.1)
  E = mesh.num_elements
  bad_sy = torch.full((E, 9), 0.1)
  bad_sy[1, 4] = 0.0
  for bad in (dict(lame_mu=0.0), dict(yield_stress=0.0),
              dict(yield_stress=-1.0), dict(yield_stress=bad_sy),
              dict(yield_stress=None), dict(hardening_modulus=-0.1),
              dict(hardening_modulus=-torch.ones(E)),
              dict(yield_stress=torch.ones(E + 1)), dict(yield_stress='mild')):
    with pytest.raises(ValueError):
      fes.plasticity_operator(**{**ok, **bad})
  with pytest.raises(ValueError, match='geometry'):
    fes.plasticity_operator(geometry='multilinear', **ok)
  op = fes.plasticity_operator(**ok)
  u = torch.zeros((mesh.num_nodes, 2), dtype=torch.float64, device=DEV)
  with pytest.raises(ValueError):
    op.residual(u[:, 0])
  with pytest.raises(ValueError, match='history'):
    op.residual(u, torch.zeros((E, 9, 7), dtype=torch.float64, device=DEV))
  grad_u = u.clone().requires_grad_(True)
  for call in (op.residual, op.linearize, op.stress):
    with pytest.raises(NotImplementedError, match='autograd'):
      call(grad_u)
  with pytest.raises(NotImplementedError, match='autograd'):
    op.residual(u, op.virgin_history().requires_grad_(True))
  with pytest.raises(NotImplementedError, match='autograd'):
    op.tangent(op.linearize(u)).apply(grad_u)
  with pytest.raises(NotImplementedError, match='ensemble'):
    FiniteElementSpace.create(mesh.replicate(2), Quadrature1D.create(
        3, GL)).plasticity_operator(**ok)
  # the launcher
  uq = torch.zeros((E, 9, 2), dtype=torch.float64, device=DEV)
  args = (uq, op.parts, op.host, 2, 3, op.point_weights(), 1.0, 1.0, None, 0.0,
          0.1, 0.0)
  lin = torch.zeros((E, 9, 5), dtype=torch.float64, device=DEV)
  with pytest.raises(ValueError, match='lin'):
    _ops.plasticity_local(*args, mode='tangent')
  with pytest.raises(ValueError, match='residual mode'):
    _ops.plasticity_local(*args, mode='tangent', want_stress=True, lin=lin)
  with pytest.raises(ValueError, match='tangent mode only'):
    _ops.plasticity_local(*args, mode='residual', lin=lin)
  with pytest.raises(ValueError, match='mode'):
    _ops.plasticity_local(*args, mode='stress')
  with pytest.raises(ValueError, match='hist'):
    _ops.plasticity_local(*args, mode='residual', hist=lin)
  bm = TR.box_with_sides(2, 2, MESH_P).finalize(device=DEV)
  with pytest.raises(ValueError, match='rigid-body'):
    solve_plasticity(bm, (0.0, 1.0), {}, lambda0=1.0, density=0.0, **ok)
  with pytest.raises(ValueError, match='body_force'):
    solve_plasticity(bm, (0.0, 1.0, 2.0), {'x0': (D, (0.0, 0.0))}, **ok)
  with pytest.raises(ValueError, match='history'):
    solve_plasticity(bm, (0.0, 1.0), {'x0': (D, (0.0, 0.0))},
                     history=torch.zeros(3, 3), **ok)
  with pytest.raises(ValueError, match='load_factors'):
    solve_plasticity(bm, (0.0, 1.0), {'x0': (D, (0.0, 0.0))}, load_factors=(),
                     **ok)


def _raw_args(op, fes, **over):
  """A valid residual-mode `PlasticityArgs` for the first launch of `op`, with
  overrides; returns (args, what must stay alive)."""
  mesh = fes.mesh
  d, Q = mesh.ndim, fes.quadrature.num_points
  E, nq = mesh.num_elements, Q ** d
  NH, NL, NV = _ops.plasticity_sizes(d)
  zeros = lambda *s: torch.zeros(s, dtype=torch.float64, device=DEV)
  keep = dict(
      u=zeros(E, nq, d), out=zeros(E, nq, d), hist_in=zeros(E, nq, NH),
      hist_out=zeros(E, nq, NH), lin=zeros(E, nq, NL), stress=zeros(E, nq, NV),
      host={k: np.ascontiguousarray(v, np.float64)
            for k, v in op.host.items()})
  part = op.parts[0]
  args = _lib.PlasticityArgs(
      u=keep['u'].data_ptr(), out=keep['out'].data_ptr(),
      wdet=op.point_weights().data_ptr(), lam_const=1.0, mu_const=1.0,
      rho_const=1.0, yield_const=0.1, hard_const=0.2,
      geo_elem=part['geo_elem'].data_ptr(),
      dmat=keep['host']['dmat'].ctypes.data,
      weights=keep['host']['weights'].ctypes.data,
      nodes=keep['host']['nodes'].ctypes.data, num_elements=E, ndim=d, P=Q,
      dtype=_lib.SFEM_F64, geo_mode=part['geo_mode'],
      hist_in=keep['hist_in'].data_ptr(), hist_out=keep['hist_out'].data_ptr(),
      lin=keep['lin'].data_ptr(), stress=keep['stress'].data_ptr(),
      mode=_lib.SFEM_PLAST_RESIDUAL)
  for k, v in over.items():
    setattr(args, k, v)
  return args, keep


def test_entry_point_refusals():
  """Status codes of the raw entry point; nothing that is refused launches."""
  case = G.affine(2, 3, MESH_P)
  mesh, _, rp = case.finalize(DEV, torch.float64)
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(4, GL))
  op = fes.plasticity_operator(lame_lambda=1.0, lame_mu=1.0, yield_stress=0.1)
  call = lambda a: _lib.load().sfem_plasticity_local(ctypes.byref(a), None)
  TANGENT = _lib.SFEM_PLAST_TANGENT
  none = dict(hist_in=None, hist_out=None, stress=None)
  ok, keep = _raw_args(op, fes)
  assert call(ok) == 0
  torch.cuda.synchronize()
  # zero displacement, virgin material: elastic, lin = (2 mu, 0, 0)
  ln = _np(keep['lin'])
  assert np.array_equal(ln[0, 0], [2.0, 0, 0, 0, 0, 0, 0, 0])
  for name in ('out', 'hist_out', 'stress'):
    assert not _np(keep[name]).any()
  ok, keep = _raw_args(op, fes, lin=None, **none)
  assert call(ok) == 0
  ok, keep = _raw_args(op, fes, mode=TANGENT, **none)
  assert call(ok) == 0
  torch.cuda.synchronize()
  # outside the compiled range: SFEM_EUNSUPPORTED
  for over in (dict(P=13), dict(P=1), dict(ndim=1), dict(ndim=4),
               dict(geo_mode=_lib.GEO_BOX), dict(geo_mode=7), dict(mode=2),
               dict(mode=-1), dict(P=13, mode=TANGENT, **none),
               dict(ndim=4, mode=TANGENT, **none)):
    a, keep = _raw_args(op, fes, **over)
    assert call(a) == -3, over
  # a missing required pointer; the tangent without lin, or with a history
  # or a stress; aliased histories: SFEM_EINVAL
  ok, keep = _raw_args(op, fes)
  for over in (dict(u=None), dict(out=None), dict(dmat=None), dict(wdet=None),
               dict(geo_elem=None), dict(weights=None), dict(nodes=None),
               dict(geo_mode=_lib.GEO_POINT), dict(dtype=5),
               dict(num_elements=-1),
               dict(mode=TANGENT, lin=None, **none),
               dict(mode=TANGENT),
               dict(mode=TANGENT, **{**none, 'hist_in': ok.hist_in}),
               dict(mode=TANGENT, **{**none, 'hist_out': ok.hist_out}),
               dict(mode=TANGENT, **{**none, 'stress': ok.stress}),
               dict(hist_out=ok.hist_in),
               dict(elem_list=keep['u'].data_ptr(), num_listed=10 ** 6)):
    a, keep2 = _raw_args(op, fes, **over)
    if 'hist_out' in over and over['hist_out'] == ok.hist_in:
      a.hist_in = ok.hist_in
    assert call(a) == -1, over
  assert _lib.load().sfem_plasticity_local(None, None) == -1
  # nothing to do is not an error
  a, keep = _raw_args(op, fes, num_elements=0, u=None, out=None)
  assert call(a) == 0
