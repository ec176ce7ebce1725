"""The adjoint reference of J2 plasticity (`tests/plasticity_adjoint_reference.
py`) against central differences, on the CPU: the point VJP in
the stored layouts against `plasticity_reference.return_map`, and the refusals
of the public interface that need no GPU."""
import numpy as np
import pytest

from tests import plasticity_adjoint_reference as PA
from tests import plasticity_reference as PR


def _sym(rng, shape, d, size):
  """Random symmetric 3 x 3 tensors; in 2D the z row and column are zero."""
  A = rng.standard_normal(shape + (3, 3)) * size
  A = 0.5 * (A + np.swapaxes(A, -1, -2))
  if d == 2:
    A[..., 2, :] = A[..., :, 2] = 0.0
  return A


def _stored_map(eps, hist, lam, mu, sy, Hh, d):
  """(sigma (..., 3, 3), trial history (..., NH), f) through the stored
  layouts."""
  ep, alpha = PR.history_tensor(hist, d)
  sigma, ep2, al2, _, f = PR.return_map(eps, ep, alpha, lam, mu, sy, Hh)
  return sigma, PR.history_array(ep2, al2, d), f


@pytest.mark.parametrize('hard', [0.2, 0.0])
@pytest.mark.parametrize('d', [2, 3])
def test_point_vjp_against_central_differences(d, hard):
  """Every output of `point_vjp`, contracted with a random direction of its
  input, against the central difference of S : sigma + hbar . history' along
  that direction, at elastic and at plastic points, with and without
  hardening.  The direction of eps is symmetric and in-plane in 2D, that of
  the history moves the stored slots (so the factor 2 of the off-diagonal
  slots and the implied zz of 2D are exercised; in 3D it keeps eps_p
  trace-free).  The loss is piecewise
  smooth with third derivatives of order mu / sn^2, so with h = 1e-6 relative
  to the inputs the quotient is good to about 1e-9; the bound is 1e-7, and
  the points are asserted to keep their side of the yield surface."""
  rng = np.random.default_rng(10 * d + int(hard > 0))
  npt = 400
  lam = rng.uniform(0.5, 2.0, npt)
  mu = rng.uniform(0.5, 1.5, npt)
  sy = rng.uniform(0.03, 0.06, npt)
  Hh = np.full(npt, hard) * rng.uniform(0.5, 1.5, npt)
  eps = _sym(rng, (npt,), d, 0.015 if d == 2 else 0.008)
  ep = PR.dev(_sym(rng, (npt,), 3, 0.01 if d == 2 else 0.006))
  if d == 2:
    ep[..., 2, :2] = ep[..., :2, 2] = 0.0
  hist = PR.history_array(ep, np.abs(rng.standard_normal(npt)) * 0.02, d)
  S = _sym(rng, (npt,), d, 1.0)
  hbar = rng.standard_normal((npt, PR.NH[d]))
  # the points within 1e-3 sigma_y of the yield surface are left out: the
  # quotient must not cross it
  f0 = _stored_map(eps, hist, lam, mu, sy, Hh, d)[2]
  far = np.abs(f0) / sy > 1e-3
  assert far.mean() > 0.95
  lam, mu, sy, Hh, eps, hist, S, hbar, f0 = (
      a[far] for a in (lam, mu, sy, Hh, eps, hist, S, hbar, f0))
  npt = int(far.sum())
  share = (f0 > 0).mean()
  assert 0.2 <= share <= 0.8, share

  def loss(eps, hist, lam, mu, sy, Hh):
    sigma, h2, f = _stored_map(eps, hist, lam, mu, sy, Hh, d)
    assert ((f > 0) == (f0 > 0)).all()
    return (S * sigma).sum((-2, -1)) + (hbar * h2).sum(-1)

  eps_b, hprev, lam_b, mu_b, sy_b, Hh_b = PA.point_vjp(eps, hist, lam, mu, sy,
                                                       Hh, S, hbar, d)
  base = [eps, hist, lam, mu, sy, Hh]
  dirs = [_sym(rng, (npt,), d, 0.03), rng.standard_normal(hist.shape) * 0.01,
          lam * rng.uniform(0.5, 1.5, npt), mu * rng.uniform(0.5, 1.5, npt),
          sy * rng.uniform(0.5, 1.5, npt), 0.2 * rng.uniform(0.5, 1.5, npt)]
  if d == 3:
    # admissible histories keep eps_p trace-free, and the plastic stress of
    # `return_map`, (lam + 2 mu / 3) tr(eps) I + theta s, is lam tr(eps) I +
    # 2 mu (eps - eps_p') on those alone: the direction stays among them
    dirs[1][:, :3] -= dirs[1][:, :3].mean(axis=1, keepdims=True)
  analytic = [(eps_b * dirs[0]).sum((-2, -1)), (hprev * dirs[1]).sum(-1),
              lam_b * dirs[2], mu_b * dirs[3], sy_b * dirs[4], Hh_b * dirs[5]]
  h = 1e-6
  for k, name in enumerate(('eps', 'history', 'lam', 'mu', 'sy', 'Hh')):
    if name == 'Hh' and hard == 0.0:
      plus = list(base)
      plus[k] = base[k] + 2 * h * dirs[k]      # Hh >= 0: a shifted centre
      mid = list(base)
      mid[k] = base[k] + h * dirs[k]
      an = PA.point_vjp(*mid[:6], S, hbar, d)[5] * dirs[5]
      cd = (loss(*plus) - loss(*base)) / (2 * h)
    else:
      plus, minus = list(base), list(base)
      plus[k] = base[k] + h * dirs[k]
      minus[k] = base[k] - h * dirs[k]
      an = analytic[k]
      cd = (loss(*plus) - loss(*minus)) / (2 * h)
    for side, sel in (('elastic', f0 <= 0), ('plastic', f0 > 0)):
      scale = np.abs(an[sel]).max()
      if scale == 0.0:
        assert np.abs(cd[sel]).max() < 1e-9, (name, side)
        continue
      err = np.abs(cd[sel] - an[sel]).max() / scale
      print(f'd={d} Hh={hard} {name} {side}: rel err {err:.2e}')
      assert err < 1e-7, (name, side, err)
  # the elastic side: no dependence on the yield stress and the hardening
  assert (sy_b[f0 <= 0] == 0).all() and (Hh_b[f0 <= 0] == 0).all()


@pytest.mark.parametrize('ndim,lambda0', [(2, 0.0), (2, 0.8), (3, 0.8)])
def test_path_adjoint_against_central_differences(ndim, lambda0):
  """`path_adjoint` on the `SolveProblem` (load, load further, unload; the
  constructor asserts the plastic shares) against central differences of the
  dense Newton path for every differentiated input: the body force, lam, mu,
  sigma_y, Hh, the input history and, with lambda0 != 0, the density.  The
  plastic set of every entry is asserted to be the same at +h, 0 and -h.  The
  errors found are printed and held to `PA.CD_FLOOR`, the floor that the GPU
  test of the solve's own quotient uses.  In 3D, where a dense path costs
  seconds, the inputs are mu, sigma_y and the history (all seven were
  measured once: `PA.CD_FLOOR`)."""
  prob = PA.SolveProblem(ndim, lambda0)
  print(f'ndim={ndim} lambda0={lambda0}: plastic shares and min |f| / sigma_y '
        f'per entry {prob.plastic_shares()}')
  cd = PA.central_differences(
      prob, names=('mu', 'sy', 'history') if ndim == 3 else None)
  if ndim == 2:
    assert set(cd) == {'force', 'lam', 'mu', 'sy', 'Hh', 'history'} | (
        {'rho'} if lambda0 else set())
  for name, (err, _, an) in cd.items():
    print(f'  {name}: derivative {an:+.6e}, rel err {err:.2e} '
          f'(floor {PA.CD_FLOOR[name]:.0e})')
    assert err <= PA.CD_FLOOR[name] <= PA.CD_BOUND, (name, err)


def test_path_adjoint_of_a_single_elastic_entry_is_the_linear_adjoint():
  """Below yield one entry is a linear solve: the path adjoint's gradients are
  those of `elasticity_adjoint_reference.solve_gradients`, and the yield
  stress and the hardening modulus get exactly zero."""
  from tests import elasticity_adjoint_reference as EA
  prob = EA.SolveProblem(2, 0.8)
  dense = PR.DenseNewton(prob.rp, prob.P, prob.lam_q, prob.mu_q(), 1e30, 0.3,
                         prob.rho, prob.lambda0)
  tr = [(prob.facets, prob.trac)]
  entries, hist = PA.follow_path(dense, prob.force, prob.fixed, prob.values,
                                 tr, (1.0,), rtol=1e-13)
  assert (hist == 0).all()
  got = PA.path_adjoint(dense, entries, prob.fixed, prob.w,
                        np.zeros_like(hist))
  _, gf, gl, gm, gr, _ = prob.gradients()
  for name, a, b in (('force', got['force'], gf), ('lam', got['lam'], gl),
                     ('mu', got['mu'], gm), ('rho', got['rho'], gr)):
    err = np.abs(a - b).max() / np.abs(b).max()
    print(f'{name}: {err:.2e}')
    assert err < 1e-9, (name, err)
  assert (got['sy'] == 0).all() and (got['Hh'] == 0).all()


def test_solve_refusals_without_a_gpu():
  """What `solve_plasticity` refuses before it touches the mesh: inputs that
  require grad without the keyword, and a `u0` that requires grad with it."""
  import torch
  from swirl_fem_amd.examples.plasticity import solve_plasticity
  g = torch.ones(3, requires_grad=True)
  kw = dict(lame_lambda=1.0, lame_mu=1.0, yield_stress=1.0)
  with pytest.raises(NotImplementedError, match='autograd'):
    solve_plasticity(None, g, {}, **kw)
  with pytest.raises(NotImplementedError, match='autograd'):
    solve_plasticity(None, None, {}, **dict(kw, yield_stress=g))
  with pytest.raises(NotImplementedError, match='autograd'):
    solve_plasticity(None, None, {}, u0=g, **kw)
  with pytest.raises(NotImplementedError, match='u0'):
    solve_plasticity(None, None, {}, u0=g, differentiable=True, **kw)
