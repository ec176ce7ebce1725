"""NumPy float64 reference of the adjoint side of neo-Hookean elasticity
 on the oracle space of `tests/elasticity_reference.py`, built on
`tests/hyperelastic_reference.py` and `tests/elasticity_adjoint_reference.py`.

The first Piola-Kirchhoff stress P = mu (F - F^-T) + lam ln J F^-T is linear in
theta = (lam, mu, rho), so for the internal force R(u; theta), a second field
v and per point q, with H_v[c][j] = d v_c / d X_j,

    d(v . R)/dlam[q] = W ln J tr(F^-1 H_v)
    d(v . R)/dmu[q]  = W (F : H_v - tr(F^-1 H_v))
    d(v . R)/drho[q] = lambda0 W u . v

(tr(F^-1 H_v) = sum_{c,j} Fi[j][c] H_v[c][j] = F^-T : H_v).

* `point_sensitivities`: from the physical gradients of the basis, nodal
  fields;
* `grid_sens`: what the kernel `sfem_hyperelastic_sens` computes from a field
  on the Q^d grid and a state array, F recovered as the inverse of the state's
  F^-1, optionally in float32;
* `solve_gradients`: the gradient of w . u for the discrete solve of
  `solve_hyperelasticity`: the dense Newton of `hyperelastic_reference`, then
  one dense adjoint solve with the tangent at the solution;
* `SolveProblem`, `central_differences`: the solve-gradient problem that the
  host and the GPU tests share.
"""

import numpy as np

from tests import elasticity_adjoint_reference as EA
from tests import elasticity_reference as ER
from tests import hyperelastic_reference as HR

reduce_coefficient = EA.reduce_coefficient
expand_coefficient = EA.expand_coefficient
# Central differences of the dense solve along the relative one-signed
# directions of `EA.central_differences` (dtheta = theta * uniform(0.5, 1.5)).
# The loss t -> w . u(theta + t dtheta) is analytic with n-th derivatives of
# size n! r^n |f|, r = |T^-1 dT| <= max |dtheta / theta| <= 1.5 (the tangent is
# linear in theta as the residual is), so the truncation of the quotient is
# about h^2 r^2.  Its rounding is that of a loss known only to the Newton
# residual left, rho_res cond |loss| / (2 h |derivative|): with rho_res =
# 1e-13 and cond = 2e3 that is 1e-10 / h times |loss| / |derivative|, which
# for the density (a small share of the loss) reaches the truncation at the
# linear adjoint's h = 1e-4: there the measured discrepancy of rho moved
# between 2e-11 and 4e-10 with the iteration that solved the perturbed
# problems, a noise sample and no floor.  So the step is h = 1e-3: truncation
# 1e-6 r^2 = 2.3e-6, a deterministic number that the dense reference and the
# GPU solve share, rounding ten times smaller than at 1e-4, and the bound
# CD_BOUND = 1e-5.
CD_H = 1e-3
CD_BOUND = 1e-5


def _contract(W, F, Fi, lnJ, Hv):
  tr = np.einsum('...jc,...cj->...', Fi, Hv)
  fh = np.einsum('...cj,...cj->...', F, Hv)
  return W * lnJ * tr, W * (fh - tr)


def local_point_sensitivities(fes, u_local, v_local, lambda0):
  """(E, n, d) element values -> per-point (dlam, dmu, drho), (E, Q) each."""
  W = ER._wdet(fes)
  F, Fi, lnJ = HR.deformation(HR.gradients(fes, u_local))
  dlam, dmu = _contract(W, F, Fi, lnJ, HR.gradients(fes, v_local))
  uq = np.einsum('qi,eic->eqc', fes.M, u_local)
  vq = np.einsum('qi,eic->eqc', fes.M, v_local)
  return dlam, dmu, lambda0 * W * (uq * vq).sum(-1)


def point_sensitivities(fes, u, v, lambda0):
  """Nodal u, v (N, d) -> per-point (dlam, dmu, drho) of v . R(u; theta)."""
  return local_point_sensitivities(fes, fes.gather(u), fes.gather(v), lambda0)


def grid_sens(fes, v_q, state, u_q, lambda0, dtype=np.float64):
  """`v_q` (E, Q^d, d) on the quadrature grid of `fes`, `state` (E, Q^d,
  d*d + 1) of a residual launch at u, `u_q` (E, Q^d, d) or None (drho is then
  None) -> (dlam, dmu, drho), the steps of the kernel evaluated in `dtype`:
  H_v = J^-T G_v, F = (F^-1)^-1 from the state, then the products."""
  d = fes.ndim
  W = ER._wdet(fes).astype(dtype)
  st = np.asarray(state, dtype)
  Fi = st[..., :d * d].reshape(st.shape[:-1] + (d, d))
  lnJ = st[..., d * d]
  F = np.linalg.inv(Fi).astype(dtype)
  Hv = HR.grid_gradients(fes, v_q, dtype)
  dlam, dmu = _contract(W, F, Fi, lnJ, Hv)
  drho = None
  if u_q is not None:
    drho = (dtype(lambda0) * W * (np.asarray(u_q, dtype) *
                                  np.asarray(v_q, dtype)).sum(-1)).astype(dtype)
  return dlam.astype(dtype), dmu.astype(dtype), drho


# -------------------------------------------------------------- dense solves
def load_vector(dense, force, tractions=()):
  """(N, d): B f plus the traction covectors, as `DenseNewton.solve` forms
  it."""
  f = (dense.B @ np.asarray(force, np.float64).reshape(-1)).reshape(
      dense.x.shape)
  for facets, t in tractions:
    f = f + dense.traction(facets, t)
  return f


def relative_residual(dense, u, force, fixed, tractions=()):
  """|keep (R(u) - f)| / |keep f| of nodal `u` (N, d) on the dense problem."""
  keep = (~np.asarray(fixed, bool)).astype(np.float64)
  f = load_vector(dense, force, tractions)
  lam, mu, rho = dense.coefs
  r = keep * (HR.residual(dense.fes, u, lam, mu, rho, dense.lambda0) - f)
  return float(np.linalg.norm(r) / np.linalg.norm(keep * f))


def adjoint_gradients(dense, u, w, fixed):
  """The gradient of w . u at a converged state `u` (N, d): (d/dforce (N, d),
  d/dlam, d/dmu, d/drho (E, Q) each, cond of the free tangent block), by one
  dense adjoint solve (the tangent is symmetric: dead loads)."""
  lam, mu, rho = dense.coefs
  free = ~np.asarray(fixed, bool).reshape(-1)
  T = HR.assemble_tangent(dense.fes, u, lam, mu, rho, dense.lambda0)[
      np.ix_(free, free)]
  v = np.zeros(free.shape)
  v[free] = np.linalg.solve(T.T, np.asarray(w, np.float64).reshape(-1)[free])
  v = v.reshape(u.shape)
  dl, dm, dr = point_sensitivities(dense.fes, u, v, dense.lambda0)
  gf = (dense.B @ v.reshape(-1)).reshape(u.shape)
  return gf, -dl, -dm, -dr, float(np.linalg.cond(T))


def solve_gradients(dense, w, force, fixed, values, tractions=(), **newton):
  """(u, d/dforce (N, d), d/dlam (E, Q), d/dmu (E, Q), d/drho (E, Q), cond of
  the free tangent block) of the loss w . u for u = `dense.solve(force, fixed,
  values, tractions, **newton)` (`dense` a `hyperelastic_reference.
  DenseNewton`)."""
  u, _ = dense.solve(force, fixed, values, tractions, **newton)
  return (u,) + adjoint_gradients(dense, u, w, fixed)


# ------------------------------------ the solve-gradient problem of the tests
class SolveProblem(EA.SolveProblem):
  """`EA.SolveProblem` (the jittered box, clamped on x0 with values, a roller
  with a value on y0, a traction on x1, a nodal body force; per-point lam,
  per-element mu, a scalar rho) with its loads scaled into the finite-strain
  regime: the tests assert max |H| >= 0.1 and min J >= 0.3 of the reference
  solution, since a problem that stays in the linear regime would not tell a
  missing F^-T term from rounding.  Two load steps; Newton stops on the
  absolute residual NEWTON_ATOL |keep f|, and so does the chord iteration
  that solves the perturbed problems of the central differences."""
  LOAD = {2: 0.12, 3: 0.15}      # factor on the body force and the traction
  LOAD_STEPS = 2
  NEWTON_ATOL = 1e-13

  def __init__(self, ndim, lambda0, facets=None):
    super().__init__(ndim, lambda0, facets)
    s = self.LOAD[ndim]
    self.force = s * self.force
    scaled = lambda g: (None if g is None else
                        (lambda y, g=g: s * g(y)) if callable(g) else s * g)
    self.trac = [scaled(g) for g in self.trac]
    self._solution = self._grads = None

  def dense(self, lam_q=None, mu_q=None, rho=None):
    if self._dense is None:
      self._dense = HR.DenseNewton(self.rp, self.P, self.lam_q, self.mu_q(),
                                   self.rho, self.lambda0)
    if lam_q is None and mu_q is None and rho is None:
      return self._dense
    import copy
    other = copy.copy(self._dense)
    other.coefs = (self.lam_q if lam_q is None else lam_q,
                   self.mu_q() if mu_q is None else mu_q,
                   self.rho if rho is None else rho)
    return other

  @property
  def tractions(self):
    return [(self.facets, self.trac)]

  def newton_kw(self, dense, force):
    keep = (~self.fixed).astype(np.float64)
    fn = np.linalg.norm(keep * load_vector(dense, force, self.tractions))
    return dict(rtol=0.0, atol=self.NEWTON_ATOL * fn, max_newton=40)

  def solve(self, dense, force=None):
    """The dense Newton solution from zero, in LOAD_STEPS load steps."""
    force = self.force if force is None else force
    return dense.solve(force, self.fixed, self.values, self.tractions,
                       load_steps=self.LOAD_STEPS,
                       **self.newton_kw(dense, force))[0]

  def solution(self):
    if self._solution is None:
      self._solution = self.solve(self.dense())
    return self._solution

  def _adjoint(self):
    """(gradients, inverse of the free tangent block) at the solution."""
    if self._grads is None:
      u = self.solution()
      lam, mu, rho = self.dense().coefs
      free = ~self.fixed.reshape(-1)
      T = HR.assemble_tangent(self.fes, u, lam, mu, rho, self.lambda0)[
          np.ix_(free, free)]
      self._grads = (adjoint_gradients(self.dense(), u, self.w, self.fixed),
                     np.linalg.inv(T))
    return self._grads

  def nearby_solution(self, dense, force=None):
    """The solution of a problem next to the problem's own (other
    coefficients or another force, as the central differences take them) by
    the chord iteration u <- u - T0^-1 r(u) from the problem's solution with
    its tangent T0: it stops on the same absolute residual as `solve`, and
    what it converges to does not depend on T0."""
    force = self.force if force is None else force
    target = self.newton_kw(dense, force)['atol']
    keep = (~self.fixed).astype(np.float64)
    free = ~self.fixed.reshape(-1)
    f = load_vector(dense, force, self.tractions)
    lam, mu, rho = dense.coefs
    Ti = self._adjoint()[1]
    u = self.solution().copy()
    for _ in range(40):
      r = keep * (HR.residual(self.fes, u, lam, mu, rho, self.lambda0) - f)
      if np.linalg.norm(r) <= target:
        return u
      du = np.zeros(free.shape)
      du[free] = -Ti @ r.reshape(-1)[free]
      u = u + du.reshape(u.shape)
    raise RuntimeError('chord iteration: no convergence')

  def loss(self, lam_q=None, mu_q=None, rho=None, force=None):
    """w . u of other coefficients or another force."""
    u = self.nearby_solution(self.dense(lam_q, mu_q, rho), force)
    return float((self.w * u).sum())

  def strain_measures(self):
    """(max |H|, min J) of the reference solution at the quadrature points."""
    H = HR.gradients(self.fes, self.fes.gather(self.solution()))
    return (float(np.sqrt((H * H).sum((-2, -1))).max()),
            float(np.linalg.det(H + np.eye(self.ndim)).min()))

  def relative_residual(self, u, dense=None, force=None):
    dense = self.dense() if dense is None else dense
    return relative_residual(dense, u, self.force if force is None else force,
                             self.fixed, self.tractions)

  def gradients(self, want_cond=False):
    """(u, d/dforce (N, d), d/dlam (E, Q), d/dmu (E, Q), d/drho (E, Q), cond
    of the free tangent block); computed once."""
    return (self.solution(),) + self._adjoint()[0]


def central_differences(prob, seed=11):
  """{name: (relative discrepancy, direction, analytic directional
  derivative)} for lam, mu and (where lambda0 != 0) rho: central differences
  of the dense Newton solve at step CD_H against the analytic gradient, with
  the relative one-signed directions of `EA.central_differences`."""
  rng = np.random.default_rng(seed)
  _, _, gl, gm, gr, _ = prob.gradients()
  h = CD_H
  out = {}
  mq = prob.mu_q()
  for name, g, base in (('lam', gl, prob.lam_q), ('mu', gm, mq)):
    dirn = base * rng.uniform(0.5, 1.5, base.shape)
    kw = {name + '_q': base + h * dirn}, {name + '_q': base - h * dirn}
    cd = (prob.loss(**kw[0]) - prob.loss(**kw[1])) / (2 * h)
    an = float((g * dirn).sum())
    out[name] = (abs(cd - an) / abs(an), dirn, an)
  if prob.lambda0:
    cd = (prob.loss(rho=prob.rho + h) - prob.loss(rho=prob.rho - h)) / (2 * h)
    an = float(gr.sum())
    out['rho'] = (abs(cd - an) / abs(an), 1.0, an)
  return out
