"""NumPy reference of the adjoint side of scalar transport, on
top of `tests/transport_reference.py` and `tests/advection_reference.py`.

* `vjp`: the cotangents of `transport_reference.integrand`, what the kernel
  `sfem_transport_rhs_vjp` computes on the Q^d grid.  With lam the cotangent
  of `out`, W = w detJ and Kw[a][c] = W d xi_a / d x_c,
      s_bar[q]      = W[q] lam[q]
      T_bar_j[q]    = m_j W[q] lam[q] + c_j sum_a (D_a^T (U_j,a lam))[q],
                      U_j,a = sum_c Kw[a][c] u_j,c
      u_bar_j[q][c] = c_j lam[q] sum_a Kw[a][c][q] (D_a T_j)[q]
  sum-factorised with the 1D derivative matrix of the Q points, the geometry
  from the oracle space.
* `rollout` / `rollout_gradient`: n `Dense.step`s in sequence and the gradient
  of w . T_n by a hand-written reverse sweep: per step one dense solve with
  the (symmetric) reduced matrix, then the transposes of the dense right-hand
  side.  With respect to every input level (only T_0 is an input of a
  rollout; the later levels collect their cotangents on the way), the
  velocity of every level in the form it was given (nodal, constant, per
  point), the source (nodal or per point) and a per-point diffusivity.
"""

import numpy as np

from tests import adjoint_reference as AJ
from tests import advection_reference as AR
from tests import transport_reference as TR
from tests.sumfact_reference import _along


# ------------------------------------------------------------ the kernel
def vjp(fes, lam, levels, want_source=True):
  """`levels` as for `integrand` (T_q may be None: no velocity cotangent).
  Returns ([(T_bar (E, Q^d), u_bar (E, Q^d, d) or None)], s_bar or None)."""
  d = fes.ndim
  W = TR.wdet(fes)
  E, nq = W.shape
  Q = round(nq ** (1.0 / d))
  assert Q ** d == nq
  D = TR.quadrature_dmat(Q)
  lam = np.asarray(lam, np.float64)
  grid = lambda v: v.reshape((E,) + (Q,) * d)
  out = []
  for Tq, uq, mc, cc in levels:
    dT = mc * W * lam
    du = None
    if uq is not None:
      du = np.zeros((E, nq, d))
    if uq is not None and cc != 0.0:
      uq = np.asarray(uq, np.float64)
      # invjacs[e,q,c,a] = d xi_a / d x_c: the contravariant velocity
      U = W[..., None] * np.einsum('eqca,eqc->eqa', fes.invjacs, uq)
      for a in range(d):
        dT = dT + cc * _along(D.T, grid(U[..., a] * lam), 1 + a).reshape(E, nq)
      if Tq is not None:
        g = grid(np.asarray(Tq, np.float64))
        ref = np.stack([_along(D, g, 1 + a).reshape(E, nq) for a in range(d)],
                       axis=-1)
        du = cc * (W * lam)[..., None] * np.einsum('eqca,eqa->eqc',
                                                   fes.invjacs, ref)
      else:
        du = None
    out.append((dT, du))
  return out, (W * lam if want_source else None)


# ------------------------------------------------------------ the stepper
def with_diffusivity(rp, P, k_q, **kwargs):
  """`TR.Dense` with the per-point diffusivity `k_q` (E, Q^d)."""
  return TR.Dense(rp, P, lambda xq: np.asarray(k_q, np.float64), **kwargs)


def rollout(dense, T0, vels, dt, orders, source=None):
  """Steps of the given orders in sequence from T0; `vels[n]` is the velocity
  of level n.  Returns every level, T0 first."""
  Ts = [np.asarray(T0, np.float64)]
  for n, k in enumerate(orders):
    Ts.append(dense.step(Ts[-k:], vels[n + 1 - k:n + 1], dt, k, source))
  return Ts


def _adjoint_solve(dense, Kfull, Tbar):
  """lam (N,) with d(w . T_new)/df = lam for T_new = expand(K^-1 reduce(f))."""
  free = ~dense.isd
  N = len(free)
  if dense.R is None:
    lam = np.zeros(N)
    lam[free] = np.linalg.solve(Kfull[np.ix_(free, free)].T, Tbar[free])
    return lam
  R = dense.R[:, free[dense.masters]]
  return R @ np.linalg.solve((R.T @ Kfull @ R).T, R.T @ Tbar)


def _velocity_cotangent(fes, u, g_q):
  """The per-point cotangent (E, Q, d) in the form of `u`."""
  u = np.asarray(u, np.float64)
  E, nq, d = fes.num_elements, fes.Q, fes.ndim
  if u.shape == (d,):
    return g_q.sum(axis=(0, 1))
  if u.shape == (E, nq, d):
    return g_q
  nodal = np.einsum('qi,eqc->eic', fes.M, g_q)
  return np.stack([fes.scatter(nodal[..., c]) for c in range(d)], axis=-1)


def rollout_gradient(dense, w, T0, vels, dt, orders, source=None):
  """The gradient of w . T_n, T_n the last level of `rollout`.  Returns a
  dict: 'T0' (N,), 'vels' (one entry per level of `vels`, in its form, None
  for a level without velocity), 'source' (in its form, or None), 'k' (E, Q^d)
  per point."""
  fes = dense.fes
  Ts = rollout(dense, T0, vels, dt, orders, source)
  W = TR.wdet(fes)
  Tbar = [np.zeros_like(Ts[0]) for _ in Ts]
  Tbar[-1] = np.asarray(w, np.float64).copy()
  gv = [None] * len(vels)
  gs = None
  gk = np.zeros_like(W)
  s = None if source is None else np.asarray(source, np.float64)
  for n in reversed(range(len(orders))):
    k = orders[n]
    bdf, ext = TR.coefficients(k)
    lam = _adjoint_solve(dense, (bdf[-1] / dt) * dense.B + dense.A,
                         Tbar[n + 1])
    # the matrix: -lam . dA_k T_new with the whole T_new (lift included)
    gk -= AJ.sensitivities(fes, Ts[n + 1], lam, 0.0, 1.0)[0]
    # the right-hand side f = B s + sum_j (m_j B + c_j C(u_j)) T_j + b
    if s is not None:
      if s.shape == (fes.num_nodes,):
        g = dense.B.T @ lam
      else:
        g = W * AJ.value(fes, fes.gather(lam))
        g = g.sum() if s.ndim == 0 else g
      gs = g if gs is None else gs + g
    for j in range(k):
      lev = n + 1 - k + j
      mc, cc = -bdf[j] / dt, -ext[j]
      Tbar[lev] += mc * (dense.B.T @ lam)
      u = vels[lev]
      if u is None or cc == 0.0:
        continue
      Tbar[lev] += cc * (dense.convection(u).T @ lam)
      # d(lam . C(u) T)/du[e,q,c] = W lam(q) d_c T(q)
      db = AJ.sensitivities(fes, Ts[lev], lam, 0.0, 0.0)[2]
      g = _velocity_cotangent(fes, u, cc * db)
      gv[lev] = g if gv[lev] is None else gv[lev] + g
  return {'T0': Tbar[0], 'vels': gv, 'source': gs, 'k': gk, 'levels': Ts}


# ------------------------------------- the step-gradient problem of the tests
DT = 0.0025
ORDERS = (1, 2, 3)
ROBIN = [('x1', 2.0, lambda y: 1.0 + y[:, 1])]
NEUMANN = [('y1', lambda y: np.cos(2.0 * y[:, 0]))]

# Central differences of the reference rollout (three steps, orders 1, 2, 3)
# along one random direction per input against `rollout_gradient`, on
# `step_problem(3)` (three-kinds mesh of 2^3 elements, P = 3).  CD_H: the step,
# of the decades 1e3 .. 1e-5, that minimises the discrepancy; CD_OBSERVED: the
# relative discrepancy seen there (DESIGN 3.14 has the whole scan).  w . T_3
# is linear in T_0 and in the source: their central differences are exact at
# any step and the figures are rounding alone, eps cond |loss| / (h
# |derivative|), which levels off at about 1e-15 once h |derivative| exceeds
# |loss| (at h = 1e3 the per-point source happened to give 0 exactly; h = 1e2
# is kept for all three).  A velocity used at every level enters as a cubic
# (truncation: third derivative times h^2 / 6, 1.3e-4 h^2 for the nodal one)
# and k is curved, as in 3.12.  The host test asserts 10 x these figures, the
# GPU test 10 x them for its own central difference of the same input along
# the same direction.
CD_H = {'T0': 1e2, 'u_nodal': 1e-3, 'u_const': 1e-4, 'u_point': 1e-3,
        's_nodal': 1e2, 's_point': 1e2, 'k': 1e-4}
CD_OBSERVED = {'T0': 8.08e-16, 'u_nodal': 1.59e-10, 'u_const': 9.00e-11,
               'u_point': 6.92e-10, 's_nodal': 1.77e-15, 's_point': 1.17e-15,
               'k': 8.92e-10}


def step_problem(ndim, periodic=()):
  """The step-gradient problem shared with `tests/test_gpu_transport_adjoint
  .py`: the three-kinds box of 2^d elements, P = 3, Dirichlet on x0 (with
  values), Robin on x1, Neumann on y1 (a plain box periodic along `periodic`
  without boundary data otherwise), deterministic data.  Returns a dict."""
  P, n = 3, 2
  rp = TR.box_with_sides(n, ndim, P, periodic=periodic,
                         three_kinds=not periodic)
  mesh = rp.finalize(device='cpu')
  x = np.asarray(rp.node_coords, np.float64)
  facets = {g: f.cpu().numpy().astype(np.int64)
            for g, f in mesh.boundary_facets.items()}
  rng = np.random.default_rng(11 + ndim)
  kw = {}
  if periodic:
    dvals = np.full(len(x), np.nan)
    kw['node_indices'] = mesh.node_indices.cpu().numpy().astype(np.int64)
    robin, neumann = [], []
  else:
    dmask = mesh.physical_masks['x0'].cpu().numpy().astype(bool)
    dvals = np.where(dmask, 1.0 + x[:, 1] ** 2, np.nan)
    robin, neumann = ROBIN, NEUMANN
  fes = AR.space(x, rp.elements, P, ((P - 1) + (ndim + 1) // 2, 'gl'))
  xq = AR.quad_points(fes)
  E, nq, d = xq.shape
  k_q = 1.0 + 0.5 * xq[..., 0] ** 2 + 0.3 * rng.random((E, nq))
  N = len(x)

  def make(kq):
    return with_diffusivity(rp, P, kq, dvals=dvals, facets=facets,
                            robin=robin, neumann=neumann, **kw)

  def field(y):
    comps = [1.0 + y[..., 1], 0.5 - y[..., 0]]
    if d == 3:
      comps.append(0.3 + 0.0 * y[..., 0])
    return np.stack(comps, axis=-1)
  T0 = np.where(np.isnan(dvals), np.sin(2.0 * x[:, 0]) + x[:, -1] ** 2, dvals)
  if periodic:
    T0 = T0[kw['node_indices']]           # one value per periodic class
  return dict(
      rp=rp, P=P, x=x, dvals=dvals, facets=facets, robin=robin,
      neumann=neumann, k_q=k_q, make=make, dense=make(k_q), T0=T0,
      w=rng.standard_normal(N), u_nodal=field(x) + 0.2 *
      rng.standard_normal((N, d)), u_const=np.array([0.7, -1.1, 0.4][:d]),
      u_point=field(xq) + 0.2 * rng.standard_normal((E, nq, d)),
      s_nodal=rng.standard_normal(N), s_point=rng.standard_normal((E, nq)),
      node_indices=kw.get('node_indices'))


def central_differences(prob, names=None, hs=None, seed=3):
  """{name: (relative discrepancy, direction, analytic directional
  derivative)} of the rollout of `prob` (orders ORDERS, step DT) for each
  input in `names` (keys of CD_H), one standard normal direction each.  The
  velocity inputs are used at every level, the other velocity-free inputs run
  with the nodal velocity."""
  hs = dict(CD_H, **(hs or {}))
  out = {}
  nlev = len(ORDERS)
  for name in (names or list(CD_H)):
    # a direction of its own per input, whichever inputs are asked for
    rng = np.random.default_rng([seed, list(CD_H).index(name)])
    u = prob[name] if name.startswith('u_') else prob['u_nodal']
    s = prob[name] if name.startswith('s_') else prob['s_nodal']

    def loss(T0=prob['T0'], u=u, s=s, kq=None):
      dense = prob['dense'] if kq is None else prob['make'](kq)
      return float(prob['w'] @ rollout(dense, T0, [u] * nlev, DT, ORDERS,
                                       s)[-1])
    g = rollout_gradient(prob['dense'], prob['w'], prob['T0'], [u] * nlev, DT,
                         ORDERS, s)
    if name == 'T0':
      grad, base, key = g['T0'], prob['T0'], 'T0'
      # the Dirichlet values are data of the problem, not of the level
      grad = np.where(np.isnan(prob['dvals']), grad, 0.0)
    elif name.startswith('u_'):
      grad, base, key = sum(g['vels']), u, 'u'
    elif name.startswith('s_'):
      grad, base, key = g['source'], s, 's'
    else:
      grad, base, key = g['k'], prob['k_q'], 'kq'
    dirn = rng.standard_normal(np.shape(base))
    if name == 'T0':
      dirn = np.where(np.isnan(prob['dvals']), dirn, 0.0)
    h = hs[name]
    cd = (loss(**{key: base + h * dirn}) - loss(**{key: base - h * dirn})) / (
        2 * h)
    an = float((grad * dirn).sum())
    out[name] = (abs(cd - an) / abs(an), dirn, an)
  return out
