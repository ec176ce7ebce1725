"""NumPy float64 reference of the adjoint side of linear elasticity (DESIGN
§3.17) on the oracle space of `tests/elasticity_reference.py`:

    A(theta) = K(lam, mu) + lambda0 M_rho,   theta = (lam, mu, rho)

is linear in theta, so for two displacement fields u, v and per point q

    d(v . A u)/dlam[q] = W tr(H_u) tr(H_v)
    d(v . A u)/dmu[q]  = W (H_u + H_u^T) : H_v      (= 2 W eps(u) : eps(v))
    d(v . A u)/drho[q] = lambda0 W u . v

with H[c][j] = d u_c / d x_j.

* `point_sensitivities`: from the physical gradients of the basis (the
  (E, Q, n, d) table of the dense reference), nodal fields;
* `grid_sens`: what the kernel `sfem_elasticity_sens` computes for fields
  given on the Q^d grid, sum-factorised with the 1D derivative matrix of the Q
  points (as `elasticity_reference.grid_apply`), optionally in float32;
* `solve_gradients`: the exact gradient of w . u for the discrete solve of
  `solve_elasticity` by one dense adjoint solve on `elasticity_reference.Dense`;
* the reductions to the forms of a coefficient and the solve-gradient problem
  that the host and the GPU tests share.
"""

import copy

import numpy as np

from tests import adjoint_reference as AJ
from tests import elasticity_reference as ER
from tests.sumfact_reference import _along
from tests.transport_reference import quadrature_dmat

reduce_coefficient = AJ.reduce_coefficient
expand_coefficient = AJ.expand_coefficient


def _contract(W, Hu, Hv):
  tru = np.trace(Hu, axis1=-2, axis2=-1)
  trv = np.trace(Hv, axis1=-2, axis2=-1)
  dlam = W * tru * trv
  dmu = W * np.einsum('...cj,...cj->...', Hu + np.swapaxes(Hu, -1, -2), Hv)
  return dlam, dmu


def local_point_sensitivities(fes, u_local, v_local, lambda0):
  """(E, n, d) element values -> per-point (dlam, dmu, drho), (E, Q) each."""
  W, ph = ER._wdet(fes), ER._phys(fes)
  Hu = np.einsum('eqij,eic->eqcj', ph, u_local, optimize=True)
  Hv = np.einsum('eqij,eic->eqcj', ph, v_local, optimize=True)
  dlam, dmu = _contract(W, Hu, Hv)
  uq = np.einsum('qi,eic->eqc', fes.M, u_local)
  vq = np.einsum('qi,eic->eqc', fes.M, v_local)
  return dlam, dmu, lambda0 * W * (uq * vq).sum(-1)


def point_sensitivities(fes, u, v, lambda0):
  """Nodal u, v (N, d) -> per-point (dlam, dmu, drho) of v . A(theta) u."""
  return local_point_sensitivities(fes, fes.gather(u), fes.gather(v), lambda0)


def grid_sens(fes, u_q, v_q, lambda0, dtype=np.float64):
  """`u_q`, `v_q` (E, Q^d, d) on the quadrature grid of `fes` -> (dlam, dmu,
  drho), the steps of the kernel evaluated in `dtype`: G[c][a] = D_a u_c,
  H = (1/W) Kw G with Kw = W d xi / d x, then the products."""
  d = fes.ndim
  W = ER._wdet(fes).astype(dtype)
  E, nq = W.shape
  Q = round(nq ** (1.0 / d))
  assert Q ** d == nq
  D = quadrature_dmat(Q).astype(dtype)
  kw = (W[..., None, None] * fes.invjacs.astype(dtype)).astype(dtype)
  iw = (dtype(1) / W).astype(dtype)

  def gradient(f_q):
    f_q = np.asarray(f_q, dtype)
    grid = np.moveaxis(f_q, -1, 1).reshape((E, d) + (Q,) * d)
    G = np.stack([_along(D, grid, 2 + a).reshape(E, d, nq) for a in range(d)],
                 axis=-1)                               # (E, c, q, a)
    H = np.einsum('eqja,ecqa->eqcj', kw, G).astype(dtype)
    return (iw[..., None, None] * H).astype(dtype)
  Hu, Hv = gradient(u_q), gradient(v_q)
  dlam, dmu = _contract(W, Hu, Hv)
  drho = dtype(lambda0) * W * (np.asarray(u_q, dtype) *
                               np.asarray(v_q, dtype)).sum(-1)
  return dlam.astype(dtype), dmu.astype(dtype), drho.astype(dtype)


def bilinear(fes, v, u, lam, mu, rho=None, lambda0=0.0):
  """v . A(theta) u from `elasticity_reference.apply`."""
  return float((v * ER.apply(fes, u, lam, mu, rho, lambda0)).sum())


def rigid_modes(x):
  """Translations and infinitesimal rotations at the nodes x (N, d)."""
  n, d = x.shape
  modes = [np.tile(np.eye(d)[c], (n, 1)) for c in range(d)]
  for a in range(d):
    for b in range(a + 1, d):
      r = np.zeros((n, d))
      r[:, a], r[:, b] = -x[:, b], x[:, a]
      modes.append(r)
  return modes


# -------------------------------------------------------------- dense solves
def solve_gradients(dense, w, force, fixed, values, tractions=(), lambda0=0.0,
                    want_cond=False):
  """The exact gradient of w . u (w (N, d)) for u = `dense.solve(force, fixed,
  values, tractions)`: (u, d/dforce (N, d), d/dlam (E, Q), d/dmu (E, Q),
  d/drho (E, Q), cond of the free matrix or None), per point, by one dense
  adjoint solve (the matrix is symmetric).  `lambda0` is that of `dense`."""
  K, b, expand = dense.system(force, fixed, values, tractions)
  u = expand(np.linalg.solve(K, b))
  free = ~np.asarray(fixed, bool).reshape(-1)
  lam = np.zeros(free.shape)
  lam[free] = np.linalg.solve(K.T, np.asarray(w, np.float64).reshape(-1)[free])
  lam = lam.reshape(u.shape)
  dl, dm, dr = point_sensitivities(dense.fes, u, lam, lambda0)
  gf = (dense.B @ lam.reshape(-1)).reshape(u.shape)
  return u, gf, -dl, -dm, -dr, (np.linalg.cond(K) if want_cond else None)


# ------------------------------------ the solve-gradient problem of the tests
# Central differences of the dense reference solve along one random direction
# per coefficient, step CD_H, against the reference's analytic gradient.  The
# loss f(t) = w . K(theta + t dtheta)^-1 b is analytic in t with n-th
# derivatives of size n! r^n |f|, r = |K^-1 dK| <= max |dtheta / theta| (each
# coefficient's share of K is at most K in the energy norm), so the
# truncation h^2 f''' / (6 f') is about h^2 r^2 and rounding adds eps cond /
# h.  The directions are drawn RELATIVE to the coefficient and of one sign,
# dtheta = theta * uniform(0.5, 1.5): r <= 1.5 whatever the coefficient's
# size, 2.3e-8 + 2e-16 * 1e4 / 1e-4 = 4e-8, within the CD_BOUND = 1e-7 of
# `tests/adjoint_reference.py`.  One sign, because a direction that stiffens
# everywhere is close to scaling the coefficient, theta (1 + t), for which f
# behaves like 1 / (1 + t) and the truncation is h^2 = 1e-8 itself: a
# deterministic number, the same for the dense reference and for the GPU
# solve, and above the rounding noise of either (1e-9 on these problems).
# The GPU test allows 10 x the MEASURED discrepancy of the reference on the
# same problem, not CD_BOUND; were that discrepancy rounding noise (as it is
# for directions of mixed sign, measured 2e-10 .. 8e-9), the rule would
# compare two independent noise samples.  (A standard normal direction
# against mu >= 0.7 has r near 5.7 on these meshes and would need 3e-7.)
CD_H = 1e-4
CD_BOUND = 1e-7


class SolveProblem:
  """The solve-gradient problem shared by the host and the GPU tests: the
  jittered box of `adjoint_reference.solve_problem` (2D: 3^2 elements, p = 4;
  3D: 2^3, p = 3), clamped on x0 with inhomogeneous values, a roller with a
  value on y0, a traction on x1, a nodal body force; per-point lam, per-
  element mu, a scalar rho."""

  def __init__(self, ndim, lambda0, facets=None):
    self.ndim, self.lambda0 = ndim, float(lambda0)
    self._dense = None
    self.rp, self.P, self.quad = AJ.solve_problem(ndim)
    rp = self.rp
    self.x = x = np.asarray(rp.node_coords, np.float64)
    if facets is None:
      mesh = rp.finalize(device='cpu')
      facets = mesh.boundary_facets['x1'].cpu().numpy().astype(np.int64)
    self.facets = facets
    self.fes = fes = ER.space(x, rp.elements, self.P, (self.quad, 'gl'))
    rng = np.random.default_rng(40 + ndim)
    xq = ER.quad_points(fes)
    E, Q = xq.shape[:2]
    self.lam_q = 1.0 + 0.5 * xq[..., 0] ** 2 + 0.3 * rng.random((E, Q))
    self.mu_e = 0.7 + 0.4 * rng.random(E)
    self.rho = 1.5
    self.force = rng.standard_normal(x.shape)
    self.w = rng.standard_normal(x.shape)
    on = lambda a, v: np.abs(x[:, a] - v) < 1e-9
    self.gD = [lambda y: 0.01 * y[:, 1] ** 2, lambda y: 0.02 * np.sin(y[:, 1]),
               lambda y: 0.01 * y[:, 0] * y[:, 1]][:ndim]
    self.roll = lambda y: 0.005 * np.cos(2.0 * y[:, 0])
    self.trac = [lambda y: 1.0 + y[:, 1], None, 0.3][:ndim]
    self.fixed = np.zeros(x.shape, bool)
    self.values = np.zeros(x.shape)
    y0, x0 = on(1, 0.0), on(0, 0.0)
    self.fixed[y0, 1], self.values[y0, 1] = True, self.roll(x)[y0]
    self.fixed[x0] = True
    self.values[x0] = np.stack([g(x) for g in self.gD], axis=-1)[x0]

  def mu_q(self, mu_e=None):
    mu_e = self.mu_e if mu_e is None else mu_e
    return expand_coefficient(mu_e, *self.lam_q.shape)

  def dense(self, lam_q=None, mu_q=None, rho=None):
    """`elasticity_reference.Dense` of the problem, or of other coefficients
    (the mass matrix and the rules of the first one are shared)."""
    if self._dense is None:
      self._dense = ER.Dense(self.rp, self.P, self.lam_q, self.mu_q(),
                             self.rho, self.lambda0)
    if lam_q is None and mu_q is None and rho is None:
      return self._dense
    other = copy.copy(self._dense)
    other.coefs = (self.lam_q if lam_q is None else lam_q,
                   self.mu_q() if mu_q is None else mu_q,
                   self.rho if rho is None else rho)
    other.A = ER.assemble(self.fes, ER.element_matrices(
        self.fes, *other.coefs, self.lambda0))
    return other

  def solve(self, dense, force=None):
    return dense.solve(self.force if force is None else force, self.fixed,
                       self.values, [(self.facets, self.trac)])

  def loss(self, lam_q=None, mu_q=None, rho=None, force=None):
    return float((self.w * self.solve(self.dense(lam_q, mu_q, rho),
                                      force)).sum())

  def gradients(self, want_cond=False):
    """(u, d/dforce (N, d), d/dlam (E, Q), d/dmu (E, Q), d/drho (E, Q),
    cond)."""
    return solve_gradients(self.dense(), self.w, self.force, self.fixed,
                           self.values, [(self.facets, self.trac)],
                           self.lambda0, want_cond)


def central_differences(prob, seed=11):
  """{name: (relative discrepancy, direction, analytic directional
  derivative)} for lam, mu and (where lambda0 != 0) rho: central differences
  of the dense solve at step CD_H against the analytic gradient."""
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
