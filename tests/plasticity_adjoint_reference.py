"""NumPy float64 reference of the adjoint side of J2 plasticity
on `tests/plasticity_reference.py`.

The point map is (eps, eps_p, alpha; lam, mu, sigma_y, Hh) -> (sigma, eps_p',
alpha').  With cotangents S of sigma, Pb of eps_p' (symmetric 3 x 3) and ab of
alpha', r32 = sqrt(3/2), e = eps - eps_p, s = 2 mu dev(e), sn = |s|, n = s /
sn, f = r32 sn - sigma_y - Hh alpha, c = 1 / (3 mu + Hh), dg = c f:

    common:   eps_b = lam tr(S) I + 2 mu S;  lam_b = tr(eps) tr(S);
              Z = Pb - 2 mu S
    f <= 0:   epsp_b = Z;  alpha_b = ab;  mu_b = 2 (eps - eps_p) : S;
              sy_b = Hh_b = 0
    f >  0:   mu_b   = 2 (eps - eps_p') : S
              dg_b   = ab + r32 (n : Z);      n_b = r32 dg Z
              f_b    = c dg_b;   mu_b -= 3 c dg dg_b
              Hh_b   = -c dg dg_b - alpha f_b
              sy_b   = -f_b;     alpha_b = ab - Hh f_b
              s_b    = (n_b - (n : n_b) n) / sn + r32 f_b n
              e_b    = 2 mu dev(s_b);   mu_b += (s : s_b) / mu
              eps_b += e_b;   epsp_b = Z - e_b

Cotangents of histories refer to the stored arrays: Pb_xy = hbar[xy] / 2 on
input and hbar_prev[xy] = 2 epsp_b_xy on output; in 2D Pb_zz = 0 and
hbar_prev[xx] = epsp_b_xx - epsp_b_zz, likewise yy.

* `tensor_vjp`: the formulas above on 3 x 3 tensors;
* `point_vjp`: the same in the stored layouts;
* `grid_vjp_displacement`, `grid_vjp_state`: what the two modes of
  `sfem_plasticity_vjp` compute on the Q^d grid, sum-factorised, in a `dtype`;
* `path_adjoint`: the dense recurrence over a load path on
  `plasticity_reference.DenseNewton`;
* `SolveProblem`: the solve-gradient problem that the host and the GPU tests
  share.
"""

import numpy as np

from tests import elasticity_adjoint_reference as EA
from tests import elasticity_reference as ER
from tests import hyperelastic_reference as HR
from tests import plasticity_reference as PR

reduce_coefficient = EA.reduce_coefficient
expand_coefficient = EA.expand_coefficient
_b = PR._b


def _dd(a, b):
  return (a * b).sum((-2, -1))


def tensor_vjp(eps, ep, alpha, lam, mu, sy, Hh, S, Pb, ab):
  """(eps_b, epsp_b (..., 3, 3), alpha_b, lam_b, mu_b, sy_b, Hh_b (...)) of
  the point map at strains eps (..., 3, 3) from the committed (ep, alpha),
  for the cotangents S, Pb (..., 3, 3) and ab (...); all in eps.dtype."""
  dt = eps.dtype
  T = dt.type
  lam, mu, sy, Hh, alpha, ab = (np.asarray(c, dt)
                                for c in (lam, mu, sy, Hh, alpha, ab))
  S, Pb, ep = np.asarray(S, dt), np.asarray(Pb, dt), np.asarray(ep, dt)
  I = np.eye(3, dtype=dt)
  r32 = np.sqrt(T(1.5))
  e = eps - ep
  s = _b(T(2) * mu) * PR.dev(e)
  sn = np.sqrt(_dd(s, s))
  f = r32 * sn - (sy + Hh * alpha)
  pl = f > 0
  c = T(1) / (T(3) * mu + Hh)
  dg = np.where(pl, c * f, T(0))
  with np.errstate(invalid='ignore', divide='ignore'):
    isn = np.where(pl, T(1) / sn, T(0))
  n = _b(isn) * s
  trS = np.trace(S, axis1=-2, axis2=-1)
  eps_b = _b(lam * trS) * I + _b(T(2) * mu) * S
  lam_b = np.trace(eps, axis1=-2, axis2=-1) * trS
  Z = Pb - _b(T(2) * mu) * S
  ep_new = ep + _b(r32 * dg) * n
  mu_b = T(2) * _dd(eps - ep_new, S)
  dg_b = ab + r32 * _dd(n, Z)
  n_b = _b(r32 * dg) * Z
  f_b = np.where(pl, c * dg_b, T(0))
  mu_b = mu_b - T(3) * c * dg * dg_b
  Hh_b = -c * dg * dg_b - alpha * f_b
  sy_b = -f_b
  alpha_b = ab - Hh * f_b
  s_b = (n_b - _b(_dd(n, n_b)) * n) * _b(isn) + _b(r32 * f_b) * n
  e_b = _b(T(2) * mu) * PR.dev(s_b)
  mu_b = mu_b + _dd(s, s_b) / mu
  eps_b = eps_b + e_b
  epsp_b = Z - e_b
  return tuple(x.astype(dt) for x in
               (eps_b, epsp_b, alpha_b, lam_b, mu_b, sy_b, Hh_b))


def cotangent_tensor(hbar, d):
  """(Pb (..., 3, 3), ab (...)) of a cotangent of a stored history."""
  hbar = np.asarray(hbar)
  Pb = np.zeros(hbar.shape[:-1] + (3, 3), hbar.dtype)
  for k, (i, j) in enumerate(PR.VOIGT[d]):
    if i == j:
      Pb[..., i, i] = hbar[..., k]
    else:
      Pb[..., i, j] = Pb[..., j, i] = hbar[..., k] * hbar.dtype.type(0.5)
  return Pb, hbar[..., -1]


def cotangent_array(epsp_b, alpha_b, d):
  """The cotangent of the stored committed history from (epsp_b, alpha_b)."""
  two = epsp_b.dtype.type(2)
  cols = []
  for i, j in PR.VOIGT[d]:
    if i != j:
      cols.append(two * epsp_b[..., i, j])
    elif d == 2:
      cols.append(epsp_b[..., i, i] - epsp_b[..., 2, 2])
    else:
      cols.append(epsp_b[..., i, i])
  return np.stack(cols + [alpha_b], axis=-1)


def point_vjp(eps, hist, lam, mu, sy, Hh, S, hbar, d):
  """The point VJP in the stored layouts: strains eps and the stress
  cotangent S (..., 3, 3), the committed history `hist` and the cotangent
  `hbar` of the trial history (..., NH) -> (eps_b (..., 3, 3), hbar_prev
  (..., NH), lam_b, mu_b, sy_b, Hh_b)."""
  ep, alpha = PR.history_tensor(np.asarray(hist, eps.dtype), d)
  Pb, ab = cotangent_tensor(np.asarray(hbar, eps.dtype), d)
  eps_b, epsp_b, alpha_b, lam_b, mu_b, sy_b, Hh_b = tensor_vjp(
      eps, ep, alpha, lam, mu, sy, Hh, S, Pb, ab)
  return (eps_b, cotangent_array(epsp_b, alpha_b, d), lam_b, mu_b, sy_b, Hh_b)


# ------------------------------------------------------- collocated grid
def _grid_coefs(fes, lam, mu, sy, Hh, dtype):
  return tuple(c.astype(dtype) for c in PR._coefs(fes, lam, mu, sy, Hh)[:4])


def grid_vjp_displacement(fes, u_q, hist, hbar, lam, mu, sy, Hh,
                          dtype=np.float64):
  """`u_q` (E, Q^d, d), the committed `hist` (E, Q^d, NH) or None and the
  cotangent `hbar` (E, Q^d, NH) -> d(hbar . Phi)/du (E, Q^d, d) on the grid:
  the point VJP with S = 0, eps_b / W folded (0 where W = 0)."""
  d = fes.ndim
  lam, mu, sy, Hh = _grid_coefs(fes, lam, mu, sy, Hh, dtype)
  hist = PR.virgin(fes) if hist is None else hist
  eps = PR.strain(HR.grid_gradients(fes, u_q, dtype))
  eps_b = point_vjp(eps, hist, lam, mu, sy, Hh, np.zeros_like(eps), hbar,
                    d)[0]
  W = ER._wdet(fes).astype(dtype)
  with np.errstate(invalid='ignore', divide='ignore'):
    iw = np.where(W != 0, dtype(1) / W, dtype(0))
  Sg = np.where(_b(W != 0), _b(iw) * eps_b, dtype(0)).astype(dtype)
  return HR._fold(fes, Sg[..., :d, :d], u_q, None, 0.0, dtype)


def grid_vjp_state(fes, u_q, w_q, hist, hbar, lam, mu, sy, Hh, lambda0=0.0,
                   dtype=np.float64):
  """`u_q`, `w_q` (E, Q^d, d), the committed `hist` and the cotangent `hbar`
  (E, Q^d, NH), None for virgin and for zero -> (hbar_prev (E, Q^d, NH), dlam,
  dmu, dyield, dhard, drho (E, Q^d) each): the point VJP with S = W sym(H_w);
  exact zeros where W = 0."""
  d = fes.ndim
  lam, mu, sy, Hh = _grid_coefs(fes, lam, mu, sy, Hh, dtype)
  hist = PR.virgin(fes) if hist is None else hist
  hbar = np.zeros_like(np.asarray(hist, dtype)) if hbar is None else hbar
  W = ER._wdet(fes).astype(dtype)
  eps = PR.strain(HR.grid_gradients(fes, u_q, dtype))
  S = (_b(W) * PR.strain(HR.grid_gradients(fes, w_q, dtype))).astype(dtype)
  _, hprev, lam_b, mu_b, sy_b, Hh_b = point_vjp(eps, hist, lam, mu, sy, Hh, S,
                                                hbar, d)
  drho = dtype(lambda0) * W * (np.asarray(u_q, dtype) *
                               np.asarray(w_q, dtype)).sum(-1)
  live = W != 0
  z = lambda a: np.where(live, a, dtype(0)).astype(dtype)
  return (np.where(live[..., None], hprev, dtype(0)).astype(dtype), z(lam_b),
          z(mu_b), z(sy_b), z(Hh_b), z(drho))


# ---------------------------------------------------------- dense, nodal
def history_vjp(fes, u, hist, hbar, lam, mu, sy, Hh, keep=None):
  """d(hbar . Phi)/du (N, d) of nodal u for the history update Phi from the
  committed `hist`: the point VJP with S = 0, through the physical gradients of
  the basis, no quadrature weight."""
  lam, mu, sy, Hh, _ = PR._coefs(fes, lam, mu, sy, Hh)
  d = fes.ndim
  eps = PR.strain(PR.gradients(fes, fes.gather(u)))
  eps_b = point_vjp(eps, hist, lam, mu, sy, Hh, np.zeros_like(eps), hbar, d)[0]
  out = fes.scatter(np.einsum('eqcj,eqij->eic', eps_b[..., :d, :d],
                              PR._phys(fes), optimize=True))
  return out if keep is None else out * keep


def state_vjp(fes, u, w, hist, hbar, lam, mu, sy, Hh, lambda0=0.0):
  """(hbar_prev (E, Q, NH), dlam, dmu, dsy, dHh, drho (E, Q) each) of w . R(u;
  hist, theta) + hbar . Phi(u; hist, theta) for nodal u, w (N, d)."""
  lam, mu, sy, Hh, _ = PR._coefs(fes, lam, mu, sy, Hh)
  d = fes.ndim
  W = PR._wdet(fes)
  ul, wl = fes.gather(u), fes.gather(w)
  eps = PR.strain(PR.gradients(fes, ul))
  S = _b(W) * PR.strain(PR.gradients(fes, wl))
  _, hprev, lam_b, mu_b, sy_b, Hh_b = point_vjp(eps, hist, lam, mu, sy, Hh, S,
                                                hbar, d)
  uq = np.einsum('qi,eic->eqc', fes.M, ul)
  wq = np.einsum('qi,eic->eqc', fes.M, wl)
  return hprev, lam_b, mu_b, sy_b, Hh_b, lambda0 * W * (uq * wq).sum(-1)


def load_vector(dense, force, tractions=()):
  """(N, d): B f plus the traction covectors, as `DenseNewton.solve` forms
  it."""
  f = (dense.B @ np.asarray(force, np.float64).reshape(-1)).reshape(
      dense.x.shape)
  for facets, t in tractions:
    f = f + dense.traction(facets, t)
  return f


def follow_path(dense, force, fixed, values, tractions, load_factors,
                history=None, u0=None, **newton):
  """The load path one entry at a time on a `plasticity_reference.
  DenseNewton`: [(u_k, h_{k-1}, s_k)] and the final history."""
  fes = dense.fes
  h = PR.virgin(fes) if history is None else np.asarray(history, np.float64)
  u = u0
  entries = []
  for s in PR._path(load_factors):
    u, h_new, _ = dense.solve(force, fixed, values, tractions, history=h,
                              load_factors=(s,), u0=u, **newton)
    entries.append((u, h, s))
    h = h_new
  return entries, h


def path_adjoint(dense, entries, fixed, ubar, hbar):
  """The path adjoint of the module docstring's recurrence, dense: for the
  entries [(u_k, h_{k-1}, s_k)] of `follow_path` and the cotangents `ubar`
  (N, d) of the last u and `hbar` (E, Q, NH) of the last history, returns a
  dict with 'force' (N, d) = B sum_k s_k v_k, 'lam', 'mu', 'sy', 'Hh', 'rho'
  (E, Q) each, 'history' (E, Q, NH) = hbar_0, 'cond' [cond of the free
  tangent per entry] and 'v' [v_k]."""
  fes = dense.fes
  lam, mu, rho = dense.coefs
  sy, Hh, l0 = dense.sy, dense.Hh, dense.lambda0
  fixed = np.asarray(fixed, bool)
  free = ~fixed.reshape(-1)
  keep = (~fixed).astype(np.float64)
  ubar = np.asarray(ubar, np.float64) * keep
  hbar = np.asarray(hbar, np.float64)
  theta = [0.0] * 5
  vsum = np.zeros(ubar.shape)
  conds, vs = [], []
  for u, h_prev, s in reversed(entries):
    rhs = ubar + history_vjp(fes, u, h_prev, hbar, lam, mu, sy, Hh, keep)
    ubar = np.zeros_like(ubar)
    T = PR.assemble_tangent(fes, u, h_prev, lam, mu, sy, Hh, rho, l0)[
        np.ix_(free, free)]
    assert np.abs(T - T.T).max() <= 1e-12 * np.abs(T).max()
    v = np.zeros(free.shape)
    v[free] = np.linalg.solve(T, rhs.reshape(-1)[free])
    v = v.reshape(u.shape)
    conds.insert(0, float(np.linalg.cond(T)))
    vs.insert(0, v)
    vsum += s * v
    out = state_vjp(fes, u, -v, h_prev, hbar, lam, mu, sy, Hh, l0)
    hbar = out[0]
    theta = [t + g for t, g in zip(theta, out[1:])]
  names = ('lam', 'mu', 'sy', 'Hh', 'rho')
  res = dict(zip(names, theta))
  res.update(force=(dense.B @ vsum.reshape(-1)).reshape(vsum.shape),
             history=hbar, cond=conds, v=vs)
  return res


# ------------------------------------ the solve-gradient problem of the tests
# Central differences of the dense Newton path along relative one-signed
# directions (dtheta = theta * uniform(0.5, 1.5), as in
# `EA.central_differences`).  Inside a fixed plastic set the loss is smooth in
# the inputs with derivatives of the size of the linear problem's, so the
# truncation of the quotient at step h is about h^2 r^2 with r <= 1.5: 2e-8 at
# CD_H = 1e-4, a deterministic number that the dense reference and the GPU
# solve share; the rounding of a loss known to the Newton residual 1e-13 |f|
# is 1e-13 cond / h = 1e-6 times |loss| / |derivative| at worst and is
# measured far below that.  The host test prints and asserts what it finds
# against CD_BOUND; those figures are the floor of the GPU test.
CD_H = 1e-4
CD_BOUND = 1e-6
# What the dense reference itself reaches per input (2D and 3D, lambda0 = 0 and
# 0.8, measured 8e-12 .. 1.3e-7 and rounded up): asserted by the host test, and
# the GPU solve's own quotient is allowed 10 times as much.
CD_FLOOR = {'force': 1e-9, 'lam': 1e-7, 'mu': 3e-7, 'sy': 2e-8, 'Hh': 5e-8,
            'history': 3e-9, 'rho': 3e-9}


class SolveProblem(EA.SolveProblem):
  """`EA.SolveProblem` (the jittered box, clamped on x0 with values, a roller
  with a value on y0, a traction on x1, a nodal body force; per-point lam,
  per-element mu, a scalar rho) with a per-point yield stress and a scalar
  hardening modulus, over the path (0.6, 1.0, 0.3): load, load further,
  unload.  The loss is (w_u * u).sum() + (w_h * history).sum().  The
  constructor asserts, from the dense reference alone, that between 10 % and
  90 % of the points yield in the second entry, none in the third, and that
  min |f| / sigma_y >= 1e-6 at every entry."""
  PATH = (0.6, 1.0, 0.3)
  SY = {2: 1.2, 3: 1.7}       # against von Mises stresses with medians 1.19
                              # and 1.62 in the elastic solution at full load
  HH = 0.3
  NEWTON_ATOL = 1e-13

  def __init__(self, ndim, lambda0, facets=None):
    super().__init__(ndim, lambda0, facets)
    xq = ER.quad_points(self.fes)
    rng = np.random.default_rng(70 + ndim)
    self.sy_q = self.SY[ndim] * (1.0 + 0.15 * np.cos(3.0 * xq[..., 0]) +
                                 0.05 * rng.random(xq.shape[:2]))
    self.Hh = self.HH
    self.w_u = self.w
    self.w_h = rng.standard_normal(xq.shape[:2] + (PR.NH[ndim],))
    self._entries = self._adj = None
    shares = self.plastic_shares()
    assert 0.1 <= shares[1][0] <= 0.9, shares
    assert shares[2][0] == 0.0, shares
    assert min(s[1] for s in shares) >= 1e-6, shares

  @property
  def tractions(self):
    return [(self.facets, self.trac)]

  def dense(self, lam_q=None, mu_q=None, rho=None, sy_q=None, Hh=None):
    if self._dense is None:
      self._dense = PR.DenseNewton(self.rp, self.P, self.lam_q, self.mu_q(),
                                   self.sy_q, self.Hh, self.rho, self.lambda0)
    if all(c is None for c in (lam_q, mu_q, rho, sy_q, Hh)):
      return self._dense
    import copy
    other = copy.copy(self._dense)
    other.coefs = (self.lam_q if lam_q is None else lam_q,
                   self.mu_q() if mu_q is None else mu_q,
                   self.rho if rho is None else rho)
    other.sy = self.sy_q if sy_q is None else sy_q
    other.Hh = self.Hh if Hh is None else Hh
    return other

  def newton_kw(self, dense, force):
    keep = (~self.fixed).astype(np.float64)
    fn = np.linalg.norm(keep * load_vector(dense, force, self.tractions))
    return dict(rtol=0.0, atol=self.NEWTON_ATOL * fn, max_newton=40)

  def follow(self, dense=None, force=None, history=None, path=None):
    """([(u_k, h_{k-1}, s_k)], final history) of the dense Newton path."""
    dense = self.dense() if dense is None else dense
    force = self.force if force is None else force
    return follow_path(dense, force, self.fixed, self.values, self.tractions,
                       self.PATH if path is None else path, history=history,
                       **self.newton_kw(dense, force))

  def entries(self):
    if self._entries is None:
      self._entries = self.follow()
    return self._entries

  def plastic_sets(self, entries, dense=None):
    """Per entry (plastic (E, Q) bool, min |f| / sigma_y)."""
    dense = self.dense() if dense is None else dense
    lam, mu, _ = dense.coefs
    out = []
    for u, h, _ in entries:
      f = PR.point_state(self.fes, self.fes.gather(u), h, lam, mu, dense.sy,
                         dense.Hh)[4]
      out.append((f > 0, float((np.abs(f) / dense.sy).min())))
    return out

  def plastic_shares(self):
    return [(float(p.mean()), m) for p, m in
            self.plastic_sets(self.entries()[0])]

  def loss_of(self, entries, history):
    return float((self.w_u * entries[-1][0]).sum() +
                 (self.w_h * history).sum())

  def loss(self, force=None, history=None, **coefs):
    """(loss, plastic sets) of other coefficients, another force or another
    initial history."""
    dense = self.dense(**coefs)
    entries, h = self.follow(dense, force, history)
    return (self.loss_of(entries, h),
            [p for p, _ in self.plastic_sets(entries, dense)])

  def gradients(self):
    """`path_adjoint` of the loss at the problem's own inputs; computed once."""
    if self._adj is None:
      entries, _ = self.entries()
      self._adj = path_adjoint(self.dense(), entries, self.fixed, self.w_u,
                               self.w_h)
    return self._adj

  def relative_residual(self, u, history, scale):
    """|keep (R(u; history) - s f)| / |keep f| on the dense problem."""
    dense = self.dense()
    keep = (~self.fixed).astype(np.float64)
    f = load_vector(dense, self.force, self.tractions)
    lam, mu, rho = dense.coefs
    r = keep * (PR.residual(self.fes, u, history, lam, mu, dense.sy, dense.Hh,
                            rho, self.lambda0)[0] - scale * f)
    return float(np.linalg.norm(r) / np.linalg.norm(keep * f))


def central_differences(prob, seed=11, loss=None, names=None):
  """{name: (relative discrepancy, direction, analytic directional
  derivative)} for force, lam, mu, sy, Hh, history and (where lambda0 != 0)
  rho: central differences at step CD_H of `loss(**inputs) -> (value, plastic
  sets)` (default: the dense Newton path, `prob.loss`) against the analytic
  `prob.gradients()`.  The plastic set of every entry is asserted to be the
  same at +h, 0 and -h.  The history direction perturbs the initial (virgin)
  history with a trace-free eps_p and alpha >= 0."""
  rng = np.random.default_rng(seed)
  loss = prob.loss if loss is None else loss
  g = prob.gradients()
  base_sets = [p for p, _ in prob.plastic_sets(prob.entries()[0])]
  d = prob.ndim
  h = CD_H
  mq = prob.mu_q()
  rel = lambda a: a * rng.uniform(0.5, 1.5, np.shape(a))
  dh = PR.random_history(prob.fes, rng, size=1.0)
  cases = {
      'force': ('force', prob.force, rel(prob.force), g['force']),
      'lam': ('lam_q', prob.lam_q, rel(prob.lam_q), g['lam']),
      'mu': ('mu_q', mq, rel(mq), g['mu']),
      'sy': ('sy_q', prob.sy_q, rel(prob.sy_q), g['sy']),
      'Hh': ('Hh', prob.Hh, prob.Hh * 1.2, g['Hh'].sum()),
      'history': ('history', PR.virgin(prob.fes), 0.01 * dh, g['history']),
  }
  if prob.lambda0:
    cases['rho'] = ('rho', prob.rho, 1.0, g['rho'].sum())
  out = {}
  for name in (cases if names is None else names):
    kw, base, dirn, grad = cases[name]
    lp, sp = loss(**{kw: base + h * dirn})
    lm, sm = loss(**{kw: base - h * dirn})
    for a, b, c in zip(sp, base_sets, sm):
      assert (a == b).all() and (c == b).all(), name
    cd = (lp - lm) / (2 * h)
    an = float(np.sum(grad * dirn))
    out[name] = (abs(cd - an) / abs(an), dirn, an)
  return out
