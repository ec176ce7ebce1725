"""NumPy float64 reference of stress recovery for linear elasticity (DESIGN
§3.18) on the oracle space of `tests/elasticity_reference.py`:

    sigma = lam tr(H) I + mu (H + H^T),   H[c][j] = d u_c / d x_j

in Voigt slots: 3D (xx, yy, zz, xy, xz, yz); 2D (xx, yy, xy, zz) with
sigma_zz = lam tr(H) (plane strain) or 0 (`plane_stress`, lam then being the
modified lambda).

* `point_stress`, `point_stress_vjp`: from the physical gradients of the basis
  (the (E, Q, n, d) table of the dense reference), element values (E, n, d);
* `grid_stress`, `grid_stress_vjp`: what the kernels `sfem_elasticity_stress`
  and `sfem_elasticity_stress_vjp` compute for fields given on the Q^d grid,
  sum-factorised with the 1D derivative matrix of the Q points, optionally in
  float32;
* `von_mises`, `von_mises_sq_gradient`;
* `lumped_weights`, `lumped_recovery`, `mass_matrix`, `l2_recovery`: dense
  nodal recovery;
* `functional_gradients`: the exact gradients of J = sum_q W vm^2 and of
  J = sum_i m_i vm_i^2 on u = `Dense.solve(...)`.
"""

import numpy as np

from tests import elasticity_adjoint_reference as EA
from tests import elasticity_reference as ER
from tests.sumfact_reference import _along
from tests.transport_reference import quadrature_dmat


def num_slots(ndim):
  return 6 if ndim == 3 else 4


def _pairs(ndim):
  """(slot, c, j) of the in-plane components, c <= j."""
  if ndim == 3:
    return [(0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 0, 1), (4, 0, 2), (5, 1, 2)]
  return [(0, 0, 0), (1, 1, 1), (2, 0, 1)]


def voigt(S, zz=None):
  """(..., d, d) symmetric -> (..., NV); `zz` (...) fills the 2D zz slot."""
  d = S.shape[-1]
  out = np.zeros(S.shape[:-2] + (num_slots(d),), S.dtype)
  for s, c, j in _pairs(d):
    out[..., s] = S[..., c, j]
  if d == 2:
    out[..., 3] = 0.0 if zz is None else zz
  return out


def work_conjugate(sigma):
  """`sigma` (..., NV) as the cotangent s with <s, voigt(eps)> = sigma : eps
  for a symmetric in-plane eps: shear slots doubled, the 2D zz slot zero."""
  s = np.array(sigma, copy=True)
  if s.shape[-1] == 6:
    s[..., 3:] *= 2
  else:
    s[..., 2] *= 2
    s[..., 3] = 0
  return s


def _stress_of(H, lam, mu, plane_stress):
  S = ER.stress(H, lam, mu)
  zz = None
  if H.shape[-1] == 2 and not plane_stress:
    zz = np.asarray(lam) * np.trace(H, axis1=-2, axis2=-1)
  return voigt(S.astype(H.dtype), zz)


def _cotangent_of(sbar, lam, mu, plane_stress):
  """Hbar (..., d, d) = d<sbar, sigma>/dH and the pieces of the explicit
  coefficient derivatives: (Hbar, dbar, sym) with sym[c][c] = 2 sbar_cc,
  sym[c][j] = sbar_cj."""
  d = 3 if sbar.shape[-1] == 6 else 2
  sym = np.zeros(sbar.shape[:-1] + (d, d), sbar.dtype)
  dbar = np.zeros(sbar.shape[:-1], sbar.dtype)
  for s, c, j in _pairs(d):
    if c == j:
      sym[..., c, c] = 2 * sbar[..., s]
      dbar = dbar + sbar[..., s]
    else:
      sym[..., c, j] = sbar[..., s]
      sym[..., j, c] = sbar[..., s]
  if d == 2 and not plane_stress:
    dbar = dbar + sbar[..., 3]
  eye = np.eye(d, dtype=sbar.dtype)
  Hbar = (np.asarray(lam) * dbar)[..., None, None] * eye + \
      np.asarray(mu)[..., None, None] * sym
  return Hbar.astype(sbar.dtype), dbar, sym


# ------------------------------------------------- from the physical gradients
def point_gradient(fes, u_local):
  """(E, n, d) -> H (E, Q, d, d)."""
  return np.einsum('eqij,eic->eqcj', ER._phys(fes), u_local, optimize=True)


def point_stress(fes, u_local, lam, mu, plane_stress=False):
  """(E, n, d) element displacements -> sigma (E, Q, NV)."""
  lam, mu = ER._points(fes, lam), ER._points(fes, mu)
  return _stress_of(point_gradient(fes, u_local), lam, mu, plane_stress)


def point_stress_vjp(fes, sbar, u_local, lam, mu, plane_stress=False):
  """Cotangent `sbar` (E, Q, NV) -> (ubar (E, n, d), dlam (E, Q), dmu
  (E, Q))."""
  lam, mu = ER._points(fes, lam), ER._points(fes, mu)
  Hbar, dbar, sym = _cotangent_of(np.asarray(sbar, np.float64), lam, mu,
                                  plane_stress)
  ubar = np.einsum('eqij,eqcj->eic', ER._phys(fes), Hbar, optimize=True)
  H = point_gradient(fes, u_local)
  dlam = np.trace(H, axis1=-2, axis2=-1) * dbar
  dmu = np.einsum('eqcj,eqcj->eq', H, sym)
  return ubar, dlam, dmu


# ------------------------------------------------------ the kernels' own steps
def _grid(fes, dtype):
  d = fes.ndim
  W = ER._wdet(fes).astype(dtype)
  E, nq = W.shape
  Q = round(nq ** (1.0 / d))
  assert Q ** d == nq
  D = quadrature_dmat(Q).astype(dtype)
  kw = (W[..., None, None] * fes.invjacs.astype(dtype)).astype(dtype)
  with np.errstate(divide='ignore'):
    iw = np.where(W != 0, dtype(1) / W, dtype(0)).astype(dtype)
  return d, E, nq, Q, D, kw, iw


def _grid_gradient(fes, f_q, dtype):
  d, E, nq, Q, D, kw, iw = _grid(fes, dtype)
  f_q = np.asarray(f_q, dtype)
  grid = np.moveaxis(f_q, -1, 1).reshape((E, d) + (Q,) * d)
  G = np.stack([_along(D, grid, 2 + a).reshape(E, d, nq) for a in range(d)],
               axis=-1)                               # (E, c, q, a)
  H = np.einsum('eqja,ecqa->eqcj', kw, G).astype(dtype)
  return (iw[..., None, None] * H).astype(dtype)


def grid_stress(fes, u_q, lam, mu, plane_stress=False, dtype=np.float64):
  """`u_q` (E, Q^d, d) on the quadrature grid of `fes` -> sigma (E, Q^d, NV),
  the steps of the kernel evaluated in `dtype`: G[c][a] = D_a u_c, H = (1/W)
  Kw G with Kw = W d xi / d x, then the stress."""
  lam = ER._points(fes, lam).astype(dtype)
  mu = ER._points(fes, mu).astype(dtype)
  H = _grid_gradient(fes, u_q, dtype)
  return _stress_of(H, lam, mu, plane_stress).astype(dtype)


def grid_stress_vjp(fes, sbar, u_q, lam, mu, plane_stress=False,
                    dtype=np.float64):
  """`sbar` (E, Q^d, NV), `u_q` (E, Q^d, d) -> (ubar (E, Q^d, d), dlam, dmu
  (E, Q^d)), the steps of the vjp kernel in `dtype`: Hbar, Gbar[c][a] = (1/W)
  sum_j Kw[a][j] Hbar[c][j], ubar_c = sum_a D_a^T Gbar[c][a]; dlam = tr(H_u)
  dbar, dmu = H_u : sym."""
  d, E, nq, Q, D, kw, iw = _grid(fes, dtype)
  lam = ER._points(fes, lam).astype(dtype)
  mu = ER._points(fes, mu).astype(dtype)
  sbar = np.asarray(sbar, dtype)
  Hbar, dbar, sym = _cotangent_of(sbar, lam, mu, plane_stress)
  Gb = (iw[:, None, :, None] *
        np.einsum('eqja,eqcj->ecqa', kw, Hbar)).astype(dtype)
  out = np.zeros((E, d, nq), dtype)
  Dt = np.ascontiguousarray(D.T)
  for a in range(d):
    ga = np.ascontiguousarray(Gb[..., a]).reshape((E, d) + (Q,) * d)
    out += _along(Dt, ga, 2 + a).reshape(E, d, nq)
  ubar = np.moveaxis(out, 1, -1)
  H = _grid_gradient(fes, u_q, dtype)
  dlam = (np.trace(H, axis1=-2, axis2=-1) * dbar).astype(dtype)
  dmu = np.einsum('eqcj,eqcj->eq', H, sym).astype(dtype)
  return ubar.astype(dtype), dlam, dmu


# ----------------------------------------------------------------- von Mises
def von_mises_sq(sigma):
  s = np.asarray(sigma)
  if s.shape[-1] == 6:
    xx, yy, zz, xy, xz, yz = np.moveaxis(s, -1, 0)
    shear = xy ** 2 + xz ** 2 + yz ** 2
  else:
    xx, yy, xy, zz = np.moveaxis(s, -1, 0)
    shear = xy ** 2
  return 0.5 * ((xx - yy) ** 2 + (yy - zz) ** 2 + (zz - xx) ** 2) + 3 * shear


def von_mises(sigma):
  return np.sqrt(von_mises_sq(sigma))


def von_mises_sq_gradient(sigma):
  """d(vm^2)/d sigma, slot by slot."""
  s = np.asarray(sigma, np.float64)
  g = np.zeros_like(s)
  if s.shape[-1] == 6:
    ix, iy, iz, shear = 0, 1, 2, (3, 4, 5)
  else:
    ix, iy, iz, shear = 0, 1, 3, (2,)
  xx, yy, zz = s[..., ix], s[..., iy], s[..., iz]
  g[..., ix] = 2 * xx - yy - zz
  g[..., iy] = 2 * yy - zz - xx
  g[..., iz] = 2 * zz - xx - yy
  for k in shear:
    g[..., k] = 6 * s[..., k]
  return g


# ------------------------------------------------------------ nodal recovery
def lumped_weights(fes):
  """m_i = scatter(I^T W): the row sums of the mass matrix."""
  W = ER._wdet(fes)
  return fes.scatter(np.einsum('qi,eq->ei', fes.M, W))


def nodal_rhs(fes, sigma_q):
  """scatter(I^T (W sigma_q)) (N, NV)."""
  W = ER._wdet(fes)
  return fes.scatter(np.einsum('qi,eqs->eis', fes.M, W[..., None] * sigma_q))


def lumped_recovery(fes, sigma_q):
  return nodal_rhs(fes, sigma_q) / lumped_weights(fes)[:, None]


def mass_matrix(fes):
  """The dense (N, N) scalar mass matrix; padding slots skipped."""
  W = ER._wdet(fes)
  A = np.zeros((fes.num_nodes, fes.num_nodes))
  for row, w in zip(np.asarray(fes.elements, np.int64), W):
    ok = row >= 0
    m = (fes.M.T * w) @ fes.M
    A[np.ix_(row[ok], row[ok])] += m[np.ix_(ok, ok)]
  return A


def l2_recovery(fes, sigma_q):
  return np.linalg.solve(mass_matrix(fes), nodal_rhs(fes, sigma_q))


def nodal_stress(fes, u, lam, mu, recovery='lumped', plane_stress=False):
  sq = point_stress(fes, fes.gather(u), lam, mu, plane_stress)
  return (lumped_recovery if recovery == 'lumped' else l2_recovery)(fes, sq)


# ------------------------------------------------- functionals of a dense solve
def _functional(fes, sq, where):
  """(J, dJ/d sigma_q (E, Q, NV)) of the stress `sq` at the quadrature points.
  `where`: 'quadrature', J = sum_q W vm^2; 'nodes', J = sum_i m_i vm_i^2 with
  the lumped nodal stress; ('pnorm', p), J = (sum_q W vm^p)^(1/p);
  ('linear_nodes', c), J = <c, lumped nodal stress> for c (N, NV)."""
  W = ER._wdet(fes)
  if where == 'quadrature':
    return (float((W * von_mises_sq(sq)).sum()),
            W[..., None] * von_mises_sq_gradient(sq))
  if where[0] == 'pnorm':
    p = where[1]
    vm2 = von_mises_sq(sq)
    S = float((W * vm2 ** (p / 2)).sum())
    # d vm^p = (p / 2) vm^(p - 2) d vm^2
    g = S ** (1.0 / p - 1.0) / p * (p / 2) * (W * vm2 ** (p / 2 - 1))
    return S ** (1.0 / p), g[..., None] * von_mises_sq_gradient(sq)
  m = lumped_weights(fes)
  sn = nodal_rhs(fes, sq) / m[:, None]
  if where == 'nodes':
    # J = sum_i m_i vm2(num_i / m_i): dJ/dnum_i = vm2'(sigma_i)
    J, cot = float((m * von_mises_sq(sn)).sum()), von_mises_sq_gradient(sn)
  else:
    c = np.asarray(where[1], np.float64)
    J, cot = float((c * sn).sum()), c / m[:, None]
  loc = np.einsum('qi,eis->eqs', fes.M, fes.gather(cot))
  return J, W[..., None] * loc


def functional(fes, u, lam, mu, where, plane_stress=False):
  sq = point_stress(fes, fes.gather(u), lam, mu, plane_stress)
  return _functional(fes, sq, where)[0]


def functional_gradients(dense, where, force, fixed, values, tractions=(),
                         lambda0=0.0, plane_stress=False, want_cond=False):
  """For u = `dense.solve(force, fixed, values, tractions)` and the functional
  `where` (`_functional`) of its stress: (J, u, dJ/dforce (N, d), dJ/dlam
  (E, Q), dJ/dmu (E, Q), cond): the implicit part through the dense adjoint
  solve (`elasticity_adjoint_reference.solve_gradients` with w = dJ/du) plus
  the explicit dependence of sigma on lam and mu at fixed u."""
  fes = dense.fes
  lam, mu = dense.coefs[0], dense.coefs[1]
  K, b, expand = dense.system(force, fixed, values, tractions)
  u = expand(np.linalg.solve(K, b))
  ul = fes.gather(u)
  J, sbar = _functional(fes, point_stress(fes, ul, lam, mu, plane_stress),
                        where)
  ubar, dlam, dmu = point_stress_vjp(fes, sbar, ul, lam, mu, plane_stress)
  _, gf, gl, gm, _, cond = EA.solve_gradients(
      dense, fes.scatter(ubar), force, fixed, values, tractions, lambda0,
      want_cond)
  return J, u, gf, gl + dlam, gm + dmu, cond


def central_differences(prob, where, seed=11):
  """{name: (relative discrepancy, direction, analytic directional
  derivative)} for lam, mu and the force of an
  `elasticity_adjoint_reference.SolveProblem`: central differences (h =
  `EA.CD_H`, one-signed relative directions as `EA.central_differences`) of
  the functional `where` of the dense solve against `functional_gradients`."""
  rng = np.random.default_rng(seed)
  args = (prob.fixed, prob.values, [(prob.facets, prob.trac)])
  _, _, gf, gl, gm, _ = functional_gradients(
      prob.dense(), where, prob.force, *args, prob.lambda0)
  h = EA.CD_H

  def value(lam_q=None, mu_q=None, force=None):
    dense = prob.dense(lam_q, mu_q)
    return functional(dense.fes, prob.solve(dense, force), dense.coefs[0],
                      dense.coefs[1], where)
  out = {}
  for name, g, base in (('lam', gl, prob.lam_q), ('mu', gm, prob.mu_q()),
                        ('force', gf, prob.force)):
    dirn = base * rng.uniform(0.5, 1.5, base.shape)
    key = name if name == 'force' else name + '_q'
    cd = (value(**{key: base + h * dirn}) -
          value(**{key: base - h * dirn})) / (2 * h)
    an = float((g * dirn).sum())
    out[name] = (abs(cd - an) / abs(an), dirn, an)
  return out


def tension_problem(ndim, plane_stress=False):
  """Uniaxial tension of `tests/test_gpu_elasticity.py` (rollers on the
  coordinate planes through the origin, traction t on x1, the jittered box of
  2^d elements, P = 4): (rp, P, (lam, mu), t, dense solution u, the analytic
  constant stress (NV,), cond of the free matrix)."""
  from swirl_fem_amd.core.operators import lame_parameters
  young, nu, t = 3.0, 0.3, 0.7
  lam, mu = lame_parameters(young, nu, plane_stress=plane_stress)
  P = 4
  rp = ER.jittered_box(2, ndim, P)
  dense = ER.Dense(rp, P, lam, mu)
  x = dense.x
  mesh = rp.finalize(device='cpu')
  facets = mesh.boundary_facets['x1'].cpu().numpy().astype(np.int64)
  fixed = np.zeros(x.shape, bool)
  for a in range(ndim):
    fixed[np.abs(x[:, a]) < 1e-9, a] = True
  trac = [t] + [None] * (ndim - 1)
  K, b, expand = dense.system(0.0 * x, fixed, 0.0 * x, [(facets, trac)])
  u = expand(np.linalg.solve(K, b))
  want = np.zeros(num_slots(ndim))
  want[0] = t
  if ndim == 2 and not plane_stress:
    want[3] = nu * t
  return rp, P, (lam, mu), t, u, want, np.linalg.cond(K)
