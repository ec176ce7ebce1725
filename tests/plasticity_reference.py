"""NumPy reference (fp64) of small-strain von Mises (J2) plasticity with linear
isotropic hardening, on the oracle space of
`tests/elasticity_reference.py`.  With eps = sym(H) embedded in 3 x 3 (plane
strain in 2D: the z row and column are zero) and the committed history
(eps_p, alpha):

    e = eps - eps_p,  s_tr = 2 mu dev(e),  q = sqrt(3/2) |s_tr|
    f = q - (sigma_y + Hh alpha)
    f <= 0: sigma = lam tr(eps) I + 2 mu e, history unchanged, (a, b, n) =
            (2 mu, 0, 0)
    f >  0: dg = f / (3 mu + Hh), n = s_tr / |s_tr|,
            eps_p' = eps_p + sqrt(3/2) dg n, alpha' = alpha + dg,
            sigma = (lam + 2 mu / 3) tr(eps) I + (1 - 3 mu dg / q) s_tr,
            theta = 1 - 2 mu sqrt(3/2) dg / |s_tr|, a = 2 mu theta,
            b = 2 mu (1 / (1 + Hh / (3 mu)) - (1 - theta))
    dsigma = lam tr(deps) I + 2 mu deps - (2 mu - a) dev(deps) - b (n:deps) n

    R(u)   = int sigma : grad v + lambda0 int rho u . v,
    T(u) w = int dsigma[sym grad w] : grad v + lambda0 int rho w . v.

Index conventions are those of the linear reference: H[..., c, j] = d u_c /
d x_j, element values (E, n, d), element matrices (n d, n d) with the unknown
(node i, component c) at i d + c; `lam`, `mu`, `rho`, `sy`, `Hh` a scalar or
(E, Q).  Stored layouts are those of `sfem_plasticity_local`: Voigt slots 3D
(xx, yy, zz, xy, xz, yz), 2D (xx, yy, xy); history (eps_p slots, alpha); lin
(a, b, n slots); stress 3D the six slots, 2D (xx, yy, xy, zz).

* `return_map`, `tangent_moduli`, `dsigma`: pointwise on 3 x 3 tensors;
* `history_tensor` / `history_array`, `lin_array` / `lin_tensor`,
  `stress_array`: the stored layouts;
* `local_residual`, `local_tangent_matrix`, `residual`, `assemble_tangent`:
  dense, from the physical gradients of the basis at the quadrature points
  (the matrix from the fourth-order moduli, the grid tangent from `dsigma`);
* `grid_residual`, `grid_tangent`: what the kernel computes on the Q^d
  quadrature grid, sum-factorised, in a `dtype`;
* `newton`, `DenseNewton`: dense Newton with the line search, load path and
  history commit of `solve_plasticity`;
* `uniaxial_curve`: the closed form of a uniaxial-stress strain path.
"""

import numpy as np

from tests import elasticity_reference as ER
from tests import hyperelastic_reference as HR

space = ER.space
quad_points = ER.quad_points
_phys, _wdet, _points = ER._phys, ER._wdet, ER._points
gradients = HR.gradients

VOIGT = {3: ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)),
         2: ((0, 0), (1, 1), (0, 1))}
STRESS = {3: VOIGT[3], 2: ((0, 0), (1, 1), (0, 1), (2, 2))}
NH = {2: 4, 3: 7}
NL = {2: 5, 3: 8}
NV = {2: 4, 3: 6}


# ------------------------------------------------------------------ pointwise
def _b(c):
  return np.asarray(c)[..., None, None]


def strain(H):
  """eps (..., 3, 3) of displacement gradients H (..., d, d)."""
  d = H.shape[-1]
  eps = np.zeros(H.shape[:-2] + (3, 3), H.dtype)
  eps[..., :d, :d] = (H + np.swapaxes(H, -1, -2)) * H.dtype.type(0.5)
  return eps


def dev(t):
  tr = np.trace(t, axis1=-2, axis2=-1)
  return t - _b(tr / t.dtype.type(3)) * np.eye(3, dtype=t.dtype)


def return_map(eps, ep, alpha, lam, mu, sy, Hh):
  """(sigma, eps_p', alpha', (a, b, n), f) of strains eps (..., 3, 3) from
  the committed (ep (..., 3, 3), alpha (...)); everything in eps.dtype."""
  T = eps.dtype.type
  lam, mu, sy, Hh = (np.asarray(c, eps.dtype) for c in (lam, mu, sy, Hh))
  I = np.eye(3, dtype=eps.dtype)
  e = eps - ep
  s = _b(T(2) * mu) * dev(e)
  sn = np.sqrt((s * s).sum((-2, -1)))
  r32 = np.sqrt(T(1.5))
  q = r32 * sn
  f = q - (sy + Hh * alpha)
  pl = f > 0
  tr = np.trace(eps, axis1=-2, axis2=-1)
  dg = np.where(pl, f / (T(3) * mu + Hh), T(0))
  with np.errstate(invalid='ignore', divide='ignore'):
    isn = np.where(pl, T(1) / sn, T(0))
  n = _b(isn) * s
  theta = T(1) - T(2) * mu * r32 * dg * isn
  sig_e = _b(lam * tr) * I + _b(T(2) * mu) * e
  sig_p = _b((lam + T(2) * mu / T(3)) * tr) * I + _b(theta) * s
  sigma = np.where(_b(pl), sig_p, sig_e)
  a = T(2) * mu * theta
  b = np.where(pl, T(2) * mu * (T(1) / (T(1) + Hh / (T(3) * mu)) -
                                (T(1) - theta)), T(0))
  ep_new = ep + _b(r32 * dg) * n
  return (sigma.astype(eps.dtype), ep_new.astype(eps.dtype),
          (alpha + dg).astype(eps.dtype),
          (a.astype(eps.dtype), b.astype(eps.dtype), n.astype(eps.dtype)),
          f.astype(eps.dtype))


def dsigma(deps, lam, mu, a, b, n):
  """The algorithmic tangent applied to deps (..., 3, 3)."""
  T = deps.dtype.type
  lam, mu = np.asarray(lam, deps.dtype), np.asarray(mu, deps.dtype)
  I = np.eye(3, dtype=deps.dtype)
  tr = np.trace(deps, axis1=-2, axis2=-1)
  nd = (n * deps).sum((-2, -1))
  return (_b(lam * tr) * I + _b(T(2) * mu) * deps -
          _b(T(2) * mu - a) * dev(deps) - _b(b * nd) * n).astype(deps.dtype)


def tangent_moduli(lam, mu, a, b, n):
  """C[..., i, j, k, l] = d sigma_ij / d eps_kl (3 x 3 x 3 x 3), with the
  minor symmetries."""
  I = np.eye(3)
  II = np.einsum('ij,kl->ijkl', I, I)
  Is = 0.5 * (np.einsum('ik,jl->ijkl', I, I) + np.einsum('il,jk->ijkl', I, I))
  c = lambda x: np.asarray(x, np.float64)[..., None, None, None, None]
  return (c(lam) * II + c(2.0 * np.asarray(mu)) * Is -
          c(2.0 * np.asarray(mu) - a) * (Is - II / 3.0) -
          c(b) * np.einsum('...ij,...kl->...ijkl', n, n))


# ------------------------------------------------------------ stored layouts
def history_tensor(hist, d):
  """(eps_p (..., 3, 3), alpha (...)) of a history array (..., NH)."""
  hist = np.asarray(hist)
  ep = np.zeros(hist.shape[:-1] + (3, 3), hist.dtype)
  for k, (i, j) in enumerate(VOIGT[d]):
    ep[..., i, j] = ep[..., j, i] = hist[..., k]
  if d == 2:
    ep[..., 2, 2] = -(hist[..., 0] + hist[..., 1])
  return ep, hist[..., -1]


def history_array(ep, alpha, d):
  return np.stack([ep[..., i, j] for i, j in VOIGT[d]] + [alpha], axis=-1)


def lin_array(a, b, n, d):
  return np.stack([a, b] + [n[..., i, j] for i, j in VOIGT[d]], axis=-1)


def lin_tensor(lin, d):
  """(a, b, n (..., 3, 3)) of a lin array; in 2D only the in-plane entries
  of n are stored, and only they meet a plane-strain deps."""
  lin = np.asarray(lin)
  n = np.zeros(lin.shape[:-1] + (3, 3), lin.dtype)
  for k, (i, j) in enumerate(VOIGT[d]):
    n[..., i, j] = n[..., j, i] = lin[..., 2 + k]
  return lin[..., 0], lin[..., 1], n


def stress_array(sigma, d):
  return np.stack([sigma[..., i, j] for i, j in STRESS[d]], axis=-1)


def virgin(fes):
  return np.zeros((fes.num_elements, fes.Q, NH[fes.ndim]))


def random_history(fes, rng, size=0.01, rnd=lambda a: a):
  """A random admissible history: eps_p symmetric and trace-free, alpha >= 0."""
  shape = (fes.num_elements, fes.Q)
  A = rng.standard_normal(shape + (3, 3)) * size
  ep = dev(0.5 * (A + np.swapaxes(A, -1, -2)))
  if fes.ndim == 2:
    ep[..., 2, :2] = ep[..., :2, 2] = 0.0
  alpha = np.abs(rng.standard_normal(shape)) * 2.0 * size
  return rnd(history_array(ep, alpha, fes.ndim))


# ------------------------------------------------ dense, physical gradients
def _coefs(fes, lam, mu, sy, Hh, rho=None):
  return (_points(fes, lam), _points(fes, mu), _points(fes, sy),
          _points(fes, Hh), _points(fes, rho, 1.0))


def point_state(fes, u_local, hist, lam, mu, sy, Hh):
  """`return_map` at the quadrature points of element values (E, n, d)."""
  lam, mu, sy, Hh, _ = _coefs(fes, lam, mu, sy, Hh)
  ep, alpha = history_tensor(np.asarray(hist, np.float64), fes.ndim)
  return return_map(strain(gradients(fes, u_local)), ep, alpha, lam, mu, sy,
                    Hh)


def local_residual(fes, u_local, hist, lam, mu, sy, Hh, rho=None,
                   lambda0=0.0):
  """(E, n, d), trial history (E, Q, NH), lin (E, Q, NL), stress (E, Q, NV)."""
  d = fes.ndim
  W, ph = _wdet(fes), _phys(fes)
  sigma, ep, alpha, (a, b, n), _ = point_state(fes, u_local, hist, lam, mu,
                                                sy, Hh)
  out = np.einsum('eq,eqcj,eqij->eic', W, sigma[..., :d, :d], ph,
                  optimize=True)
  if lambda0:
    out = out + HR._mass(fes, u_local, _points(fes, rho, 1.0), lambda0)
  return (out, history_array(ep, alpha, d), lin_array(a, b, n, d),
          stress_array(sigma, d))


def local_tangent_matrix(fes, u_local, hist, lam, mu, sy, Hh, rho=None,
                         lambda0=0.0):
  """(E, n d, n d) element tangent matrices from the fourth-order moduli."""
  W, ph = _wdet(fes), _phys(fes)
  E, Q = W.shape
  nn, d = fes.M.shape[1], fes.ndim
  _, _, _, (a, b, n), _ = point_state(fes, u_local, hist, lam, mu, sy, Hh)
  C = tangent_moduli(_points(fes, lam), _points(fes, mu), a, b, n)[
      ..., :d, :d, :d, :d]
  half = np.einsum('eqcjbl,eqkl->eqcjkb', C, ph)
  out = np.einsum('eq,eqij,eqcjkb->eickb', W, ph, half, optimize=True)
  if lambda0:
    rho = _points(fes, rho, 1.0)
    mm = lambda0 * np.einsum('qi,eq,qk->eik', fes.M, W * rho, fes.M)
    for c in range(d):
      out[:, :, c, :, c] += mm
  return out.reshape(E, nn * d, nn * d)


def local_tangent(fes, w_local, lin, lam, mu, rho=None, lambda0=0.0):
  """(E, n, d): the element tangent of the state `lin` applied to w_local,
  from `dsigma`."""
  d = fes.ndim
  W, ph = _wdet(fes), _phys(fes)
  a, b, n = lin_tensor(np.asarray(lin, np.float64), d)
  ds = dsigma(strain(gradients(fes, w_local)), _points(fes, lam),
              _points(fes, mu), a, b, n)
  out = np.einsum('eq,eqcj,eqij->eic', W, ds[..., :d, :d], ph, optimize=True)
  if lambda0:
    out = out + HR._mass(fes, w_local, _points(fes, rho, 1.0), lambda0)
  return out


def residual(fes, u, hist, lam, mu, sy, Hh, rho=None, lambda0=0.0, keep=None):
  """(assembled (N, d) residual, trial history, lin, stress)."""
  out, h, l, s = local_residual(fes, fes.gather(u), hist, lam, mu, sy, Hh, rho,
                                lambda0)
  out = fes.scatter(out)
  return (out if keep is None else out * keep), h, l, s


def tangent(fes, w, lin, lam, mu, rho=None, lambda0=0.0, keep=None):
  out = fes.scatter(local_tangent(fes, fes.gather(w), lin, lam, mu, rho,
                                  lambda0))
  return out if keep is None else out * keep


def assemble_tangent(fes, u, hist, lam, mu, sy, Hh, rho=None, lambda0=0.0):
  """(N d, N d) dense algorithmic tangent at u from the committed `hist`."""
  return ER.assemble(fes, local_tangent_matrix(fes, fes.gather(u), hist, lam,
                                               mu, sy, Hh, rho, lambda0))


# ------------------------------------------------------- collocated grid
def yield_margin(fes, u_q, hist, lam, mu, sy, Hh):
  """(f / sigma_y (E, Q^d), plastic (E, Q^d) bool) of grid values, fp64."""
  lam, mu, sy, Hh, _ = _coefs(fes, lam, mu, sy, Hh)
  ep, alpha = history_tensor(np.asarray(hist, np.float64), fes.ndim)
  f = return_map(strain(HR.grid_gradients(fes, u_q)), ep, alpha, lam, mu, sy,
                 Hh)[4]
  return f / sy, f > 0


def grid_residual(fes, u_q, hist, lam, mu, sy, Hh, rho=None, lambda0=0.0,
                  dtype=np.float64):
  """`u_q` (E, Q^d, d) on the quadrature grid and the committed history `hist`
  (E, Q^d, NH) or None -> (residual (E, Q^d, d), trial history, lin, stress),
  evaluated in `dtype`."""
  d = fes.ndim
  lam, mu, sy, Hh, rho = (c.astype(dtype)
                          for c in _coefs(fes, lam, mu, sy, Hh, rho))
  u_q = np.asarray(u_q, dtype)
  hist = virgin(fes) if hist is None else hist
  ep, alpha = history_tensor(np.asarray(hist, dtype), d)
  H = HR.grid_gradients(fes, u_q, dtype)
  sigma, ep, alpha, (a, b, n), _ = return_map(strain(H), ep, alpha, lam, mu,
                                              sy, Hh)
  out = HR._fold(fes, sigma[..., :d, :d], u_q, rho, lambda0, dtype)
  return (out, history_array(ep, alpha, d).astype(dtype),
          lin_array(a, b, n, d).astype(dtype),
          stress_array(sigma, d).astype(dtype))


def grid_tangent(fes, w_q, lin, lam, mu, rho=None, lambda0=0.0,
                 dtype=np.float64):
  """`w_q` (E, Q^d, d) and a lin array (E, Q^d, NL) -> the tangent (E, Q^d, d)
  on the grid in `dtype`; a, b and n come from `lin` alone."""
  d = fes.ndim
  lam = _points(fes, lam).astype(dtype)
  mu = _points(fes, mu).astype(dtype)
  rho = _points(fes, rho, 1.0).astype(dtype)
  a, b, n = lin_tensor(np.asarray(lin, dtype), d)
  ds = dsigma(strain(HR.grid_gradients(fes, w_q, dtype)), lam, mu, a, b, n)
  return HR._fold(fes, ds[..., :d, :d], w_q, rho, lambda0, dtype)


# ------------------------------------------------------------------ Newton
def _path(load_factors):
  if isinstance(load_factors, int):
    return tuple(k / load_factors for k in range(1, load_factors + 1))
  return tuple(float(s) for s in load_factors)


def newton(residual_fn, tangent_fn, f_ext, fixed, values, history, *,
           load_factors=(1.0,), rtol=1e-8, atol=0.0, max_newton=25, u0=None):
  """Dense Newton with the load path, line search and history commit of
  `solve_plasticity`: for each factor s the loads `f_ext` (N, d) and the
  Dirichlet `values` on `fixed` (N, d) bool are scaled by s; r = keep (R(u;
  history) - s f); stop at |r| <= max(rtol |r_0|, atol); else solve T dw = -r
  on the free unknowns and backtrack t = 1, 1/2, .., 2^-10 until |r(u + t
  dw)| is finite and <= (1 - 1e-4 t) |r|; at convergence the accepted trial
  history is committed.  `residual_fn(u, history) -> ((N, d), trial
  history)`, `tangent_fn(u, history) -> (N d, N d)`.  Returns (u, history,
  [Newton iterations per entry])."""
  fixed = np.asarray(fixed, bool)
  free = ~fixed.reshape(-1)
  keep = (~fixed).astype(np.float64)
  u = np.zeros(fixed.shape) if u0 is None else np.array(u0, np.float64)
  counts = []
  for k, s in enumerate(_path(load_factors), start=1):
    u = np.where(fixed, s * np.asarray(values, np.float64), u)

    def res(v):
      R, trial = residual_fn(v, history)
      return keep * (R - s * f_ext), trial
    r, trial = res(u)
    rn = np.linalg.norm(r)
    target = max(rtol * rn, atol)
    it = 0
    while rn > target:
      if it == max_newton:
        raise RuntimeError(f'dense Newton: entry {k}: no convergence')
      it += 1
      T = tangent_fn(u, history)[np.ix_(free, free)]
      dw = np.zeros(u.size)
      dw[free] = np.linalg.solve(T, -r.reshape(-1)[free])
      dw = dw.reshape(u.shape)
      t = 1.0
      for _ in range(11):
        rt, trial_t = res(u + t * dw)
        nt = np.linalg.norm(rt)
        if np.isfinite(nt) and nt <= (1.0 - 1e-4 * t) * rn:
          break
        t *= 0.5
      else:
        raise RuntimeError(f'dense Newton: entry {k}: line search')
      u, r, rn, trial = u + t * dw, rt, nt, trial_t
    history = trial
    counts.append(it)
  return u, history, counts


class DenseNewton(ER.Dense):
  """The dense J2 problem on a refined premesh: the mass matrix B and the
  tractions of `elasticity_reference.Dense`, the residual and the tangent of
  this module."""

  def __init__(self, rp, P, lam, mu, sy, Hh, rho=None, lambda0=0.0):
    super().__init__(rp, P, lam, mu, rho, lambda0)
    self.lambda0 = lambda0
    xq = quad_points(self.fes)
    val = lambda c: c(xq) if callable(c) else c
    self.sy, self.Hh = val(sy), val(Hh)

  def solve(self, force, fixed, values, tractions=(), history=None, **kw):
    """(u (N, d), history (E, Q, NH), Newton iterations per entry) for nodal
    `force` (N, d), `fixed` (N, d) bool, `values` (N, d) and [(facets, t)]
    tractions, from the committed `history` (None: virgin)."""
    f = (self.B @ np.asarray(force, np.float64).reshape(-1)).reshape(
        self.x.shape)
    for facets, t in tractions:
      f = f + self.traction(facets, t)
    lam, mu, rho = self.coefs
    fes, sy, Hh, l0 = self.fes, self.sy, self.Hh, self.lambda0
    history = virgin(fes) if history is None else np.asarray(history)
    return newton(
        lambda u, h: residual(fes, u, h, lam, mu, sy, Hh, rho, l0)[:2],
        lambda u, h: assemble_tangent(fes, u, h, lam, mu, sy, Hh, rho, l0),
        f, fixed, values, history, **kw)


def uniaxial_curve(E, nu, sigma_y, Hh, strain_path):
  """(stress, alpha, eps_p) after each entry of `strain_path` (axial strains)
  of a bar under uniaxial stress with J2 plasticity and linear isotropic
  hardening: slope E up to sigma_y, E Hh / (E + Hh) beyond, elastic unloading
  with slope E, residual strain eps_p after full unloading.  Under uniaxial
  stress q = |sigma| and the backward-Euler return is exact for any step, so
  this is what the discrete solve must give; `nu` fixes the lateral strain
  only and does not enter the axial response."""
  del nu
  ep, alpha = 0.0, 0.0
  out = []
  for eps in strain_path:
    sig = E * (eps - ep)
    f = abs(sig) - (sigma_y + Hh * alpha)
    if f > 0:
      dg = f / (E + Hh)
      ep += dg * np.sign(sig)
      alpha += dg
      sig = E * (eps - ep)
    out.append((sig, alpha, ep))
  return tuple(np.array(c) for c in zip(*out))
