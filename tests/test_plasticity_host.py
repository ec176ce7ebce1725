"""J2 plasticity without a GPU: the NumPy reference
(`tests/plasticity_reference.py`) against itself -- the algorithmic tangent
against the central difference of the stress, its symmetry, consistency on
the yield surface, the elastic branch, continuity across f = 0, the collocated
grid against the dense element quantities, plane strain against the 3D
formulas -- the stored layouts and the struct against the header, the
refusals of `solve_plasticity`, and the dense Newton under uniaxial stress
against the closed form."""
import ctypes
import os
import re

import numpy as np
import pytest

from swirl_fem_amd import _lib
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType
from swirl_fem_amd.examples.plasticity import BCType, solve_plasticity
from tests import elasticity_reference as ER
from tests import geometry_cases as G
from tests import plasticity_reference as PR
from tests import transport_reference as TR
from tests.test_hyperelastic_host import _declared

P = 3
CASES = [('multilinear', 2), ('three_kinds', 2), ('three_kinds', 3),
         ('affine', 3)]
LAM, MU, SY, HH = 1.3, 0.7, 0.05, 0.2


def _points(rng, M, plane=False):
  """M random strains (size 0.014), admissible histories and the margin f."""
  H = rng.standard_normal((M, 3, 3)) * 0.014
  eps = 0.5 * (H + np.swapaxes(H, -1, -2))
  A = rng.standard_normal((M, 3, 3)) * 0.01
  ep = PR.dev(0.5 * (A + np.swapaxes(A, -1, -2)))
  if plane:
    eps[:, 2, :] = eps[:, :, 2] = 0.0
    ep[:, 2, :2] = ep[:, :2, 2] = 0.0
  alpha = np.abs(rng.standard_normal(M)) * 0.02
  return eps, ep, alpha


def _sym(rng, M):
  d = rng.standard_normal((M, 3, 3))
  return 0.5 * (d + np.swapaxes(d, -1, -2))


# ------------------------------------------------------------ pointwise
@pytest.mark.parametrize('Hh', [HH, 0.0])
def test_tangent_is_derivative_of_stress(Hh):
  """dsigma against the central difference of `return_map` (h = 1e-7) to 1e-6
  at the points with |f| / sigma_y > 1e-2; both branches are present."""
  rng = np.random.default_rng(0)
  eps, ep, alpha = _points(rng, 4000)
  sig, _, _, (a, b, n), f = PR.return_map(eps, ep, alpha, LAM, MU, SY, Hh)
  far = np.abs(f) / SY > 1e-2
  assert 0.2 < (f > 0).mean() < 0.8 and far.mean() > 0.8
  d = _sym(rng, len(eps))
  h = 1e-7
  fd = (PR.return_map(eps + h * d, ep, alpha, LAM, MU, SY, Hh)[0] -
        PR.return_map(eps - h * d, ep, alpha, LAM, MU, SY, Hh)[0]) / (2 * h)
  T = PR.dsigma(d, LAM, MU, a, b, n)
  err = (np.abs(fd - T).max((-2, -1)) / np.abs(fd).max((-2, -1)))[far].max()
  print(f'Hh={Hh}: tangent vs central difference {err:.2e}')
  assert err <= 1e-6
  C = PR.tangent_moduli(LAM, MU, a, b, n)
  assert np.abs(np.einsum('pijkl,pkl->pij', C, d) - T).max() <= 1e-13


def test_tangent_symmetry():
  rng = np.random.default_rng(1)
  eps, ep, alpha = _points(rng, 2000)
  _, _, _, (a, b, n), _ = PR.return_map(eps, ep, alpha, LAM, MU, SY, HH)
  C = PR.tangent_moduli(LAM, MU, a, b, n)
  assert np.abs(C - np.einsum('pijkl->pklij', C)).max() <= 1e-13
  assert np.abs(C - np.einsum('pijkl->pjikl', C)).max() <= 1e-13
  v, w = _sym(rng, len(eps)), _sym(rng, len(eps))
  vw = (v * PR.dsigma(w, LAM, MU, a, b, n)).sum((-2, -1))
  wv = (w * PR.dsigma(v, LAM, MU, a, b, n)).sum((-2, -1))
  assert np.abs(vw - wv).max() <= 1e-13 * np.abs(vw).max()


@pytest.mark.parametrize('Hh', [HH, 0.0])
def test_plastic_points_lie_on_the_yield_surface(Hh):
  """sqrt(3/2) |dev sigma| = sigma_y + Hh alpha' and tr eps_p' = 0, to 1e-13."""
  rng = np.random.default_rng(2)
  eps, ep, alpha = _points(rng, 4000)
  sig, ep1, al1, (a, b, n), f = PR.return_map(eps, ep, alpha, LAM, MU, SY, Hh)
  pl = f > 0
  assert pl.sum() > 500
  s = PR.dev(sig)
  q = np.sqrt(1.5 * (s * s).sum((-2, -1)))
  assert np.abs(q - (SY + Hh * al1))[pl].max() <= 1e-13
  assert np.abs(np.trace(ep1, axis1=-2, axis2=-1)).max() <= 1e-13
  assert np.abs(ep1 - np.swapaxes(ep1, -1, -2)).max() == 0.0
  assert (al1[pl] > alpha[pl]).all()
  assert np.abs((n * n).sum((-2, -1))[pl] - 1.0).max() <= 1e-13


def test_elastic_points_are_linear():
  """f <= 0: the linear stress of eps - eps_p, the history unchanged bitwise,
  (a, b, n) = (2 mu, 0, 0); |s_tr| = 0 divides nothing."""
  rng = np.random.default_rng(3)
  eps, ep, alpha = _points(rng, 4000)
  eps[0], ep[0] = 0.01 * np.eye(3), 0.0      # hydrostatic: |s_tr| = 0
  with np.errstate(all='raise'):
    sig, ep1, al1, (a, b, n), f = PR.return_map(eps, ep, alpha, LAM, MU, SY, HH)
  el = f <= 0
  assert el[0] and el.sum() > 500
  want = LAM * np.trace(eps, axis1=-2, axis2=-1)[:, None, None] * np.eye(3) + \
      2 * MU * (eps - ep)
  assert np.abs(sig - want)[el].max() <= 1e-15
  assert np.array_equal(ep1[el], ep[el]) and np.array_equal(al1[el], alpha[el])
  assert np.all(a[el] == 2 * MU) and not b[el].any() and not n[el].any()
  # virgin material below yield is `elasticity_reference.stress`
  H = rng.standard_normal((50, 3, 3)) * 1e-3
  sig = PR.return_map(PR.strain(H), np.zeros((50, 3, 3)), np.zeros(50), LAM, MU,
                      SY, HH)[0]
  assert np.abs(sig - ER.stress(H, LAM, MU)).max() <= 1e-16


def test_return_map_is_continuous_across_yield():
  """Scaling a strain to f = -t and f = +t (t -> 0): stress and history
  differ by O(t), while (a, b, n) jump."""
  rng = np.random.default_rng(4)
  eps, ep, alpha = _points(rng, 200)
  ep[:], alpha[:] = 0.0, 0.0
  e = PR.dev(eps)                       # deviatoric: q is linear in the scale
  q = np.sqrt(1.5) * 2 * MU * np.sqrt((e * e).sum((-2, -1)))
  on = e * (SY / q)[:, None, None]
  for t in (1e-6, 1e-9):
    lo = PR.return_map(on * (1 - t), ep, alpha, LAM, MU, SY, HH)
    hi = PR.return_map(on * (1 + t), ep, alpha, LAM, MU, SY, HH)
    assert (lo[4] <= 0).all() and (hi[4] > 0).all()
    assert np.abs(hi[0] - lo[0]).max() <= 4 * t * SY
    assert np.abs(hi[1] - lo[1]).max() <= 4 * t * SY / MU
    assert np.abs(hi[2] - lo[2]).max() <= 4 * t * SY / MU
    assert np.abs(hi[3][1]).min() > 0.1 and not lo[3][1].any()


def test_plane_strain_is_3d_with_zero_z_strains():
  """The 2D layouts round-trip through the 3 x 3 formulas: eps_p,zz = -(xx +
  yy) is implied, sigma_zz is stored last, and n : deps needs the in-plane n
  only."""
  rng = np.random.default_rng(5)
  eps, ep, alpha = _points(rng, 3000, plane=True)
  sig, ep1, al1, (a, b, n), f = PR.return_map(eps, ep, alpha, LAM, MU, SY, HH)
  assert 0.2 < (f > 0).mean() < 0.8
  hist = PR.history_array(ep1, al1, 2)
  assert hist.shape == (3000, 4)
  back, al = PR.history_tensor(hist, 2)
  assert np.abs(back - ep1).max() <= 1e-16 and np.array_equal(al, al1)
  assert np.abs(sig[:, 2, :2]).max() == 0.0 and np.abs(sig[:, 2, 2]).max() > 0
  st = PR.stress_array(sig, 2)
  assert np.array_equal(st[:, 3], sig[:, 2, 2])
  assert np.array_equal(st[:, 2], sig[:, 0, 1])
  lin = PR.lin_array(a, b, n, 2)
  assert lin.shape == (3000, 5)
  a2, b2, n2 = PR.lin_tensor(lin, 2)
  d = _sym(rng, 3000)
  d[:, 2, :] = d[:, :, 2] = 0.0
  full = PR.dsigma(d, LAM, MU, a, b, n)
  plane = PR.dsigma(d, LAM, MU, a2, b2, n2)
  assert np.abs(full[:, :2, :2] - plane[:, :2, :2]).max() <= 1e-15


def test_layouts():
  """History (eps_p xx, yy, zz, xy, xz, yz, alpha), lin (a, b, n in those
  slots) and stress in the slots of `sfem_elasticity_stress`."""
  t = np.arange(9.0).reshape(3, 3)
  t = t + t.T
  h = PR.history_array(t, 7.0, 3)
  assert list(h) == [t[0, 0], t[1, 1], t[2, 2], t[0, 1], t[0, 2], t[1, 2], 7.0]
  assert np.array_equal(PR.history_tensor(h, 3)[0], t)
  l = PR.lin_array(1.0, 2.0, t, 3)
  assert list(l) == [1.0, 2.0] + list(h[:6]) and len(l) == PR.NL[3] == 8
  assert list(PR.stress_array(t, 3)) == list(h[:6])
  assert list(PR.stress_array(t, 2)) == [t[0, 0], t[1, 1], t[0, 1], t[2, 2]]
  assert list(PR.history_array(t, 7.0, 2)) == [t[0, 0], t[1, 1], t[0, 1], 7.0]
  assert (PR.NH, PR.NL, PR.NV) == ({2: 4, 3: 7}, {2: 5, 3: 8}, {2: 4, 3: 6})
  from swirl_fem_amd import _ops
  for d in (2, 3):
    assert _ops.plasticity_sizes(d) == (PR.NH[d], PR.NL[d], PR.NV[d])


# ---------------------------------------------------- element quantities
def _space(kind, ndim):
  case = getattr(G, kind)(2, ndim, P)
  q = P - 1 + (ndim + 1) // 2
  return case.rp, ER.space(case.rp.node_coords, case.rp.elements, P, (q, 'gl'))


def _coefficients(fes, rng):
  xq = ER.quad_points(fes)
  lam = 1.0 + 0.5 * np.sin(2.0 * xq[..., 0]) + rng.uniform(
      0, 0.2, xq.shape[:2])
  mu = 0.7 + 0.3 * xq[..., 1] ** 2
  sy = 0.05 * (1.0 + 0.2 * np.cos(xq[..., 0]))
  Hh = 0.2 + 0.1 * xq[..., 0]
  rho = 1.5 + np.cos(xq[..., 0])
  return lam, mu, sy, Hh, rho


def _field(fes, rng, hist, coefs, share=0.5):
  """A random nodal field scaled so that `share` of the points yield."""
  u = rng.standard_normal((fes.num_nodes, fes.ndim))
  lo, hi = 0.0, 1.0
  frac = lambda s: (PR.point_state(fes, fes.gather(s * u), hist,
                                   *coefs[:4])[4] > 0).mean()
  while frac(hi) < share:
    hi *= 2.0
  for _ in range(40):
    mid = 0.5 * (lo + hi)
    lo, hi = (mid, hi) if frac(mid) < share else (lo, mid)
  return hi * u


@pytest.mark.parametrize('kind,ndim', CASES)
def test_grid_agrees_with_local(kind, ndim):
  """`grid_*` (the kernel's steps, sum-factorised) between interpolation and
  its transpose equals the dense element quantities to 1e-12; the matrix from
  the moduli equals the apply from `dsigma`."""
  rp, fes = _space(kind, ndim)
  rng = np.random.default_rng(20 + ndim)
  coefs = _coefficients(fes, rng)
  lam, mu, sy, Hh, rho = coefs
  hist = PR.random_history(fes, rng)
  u = _field(fes, rng, hist, coefs)
  ul = fes.gather(u)
  wl = fes.gather(rng.standard_normal(u.shape))
  to_grid = lambda v: np.einsum('qi,eic->eqc', fes.M, v)
  back = lambda r: np.einsum('qi,eqc->eic', fes.M, r)
  for l0 in (0.0, 1.7):
    rq, hq, lq, sq = PR.grid_residual(fes, to_grid(ul), hist, lam, mu, sy, Hh,
                                      rho, l0)
    want, wh, wl_, ws = PR.local_residual(fes, ul, hist, lam, mu, sy, Hh, rho,
                                          l0)
    share = (lq[..., 1] != 0).mean()
    assert 0.3 < share < 0.7
    assert np.abs(back(rq) - want).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(hq - wh).max() <= 1e-12 * np.abs(wh).max()
    assert np.abs(sq - ws).max() <= 1e-12 * np.abs(ws).max()
    assert np.abs(lq - wl_).max() <= 1e-12 * np.abs(wl_).max()
    tq = PR.grid_tangent(fes, to_grid(wl), lq, lam, mu, rho, l0)
    want = PR.local_tangent(fes, wl, wl_, lam, mu, rho, l0)
    assert np.abs(back(tq) - want).max() <= 1e-12 * np.abs(want).max()
    A = PR.local_tangent_matrix(fes, ul, hist, lam, mu, sy, Hh, rho, l0)
    assert np.abs(A - np.swapaxes(A, 1, 2)).max() <= 1e-13 * np.abs(A).max()
    E = fes.num_elements
    Aw = np.einsum('eab,eb->ea', A, wl.reshape(E, -1)).reshape(wl.shape)
    assert np.abs(Aw - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize('kind,ndim', CASES[:2])
def test_below_yield_is_linear_elasticity(kind, ndim):
  rp, fes = _space(kind, ndim)
  rng = np.random.default_rng(7)
  lam, mu, sy, Hh, rho = _coefficients(fes, rng)
  ul = fes.gather(1e-4 * rng.standard_normal((fes.num_nodes, ndim)))
  out, hist, lin, _ = PR.local_residual(fes, ul, PR.virgin(fes), lam, mu, 1e3,
                                        Hh, rho, 0.9)
  want = ER.local_apply(fes, ul, lam, mu, rho, 0.9)
  assert np.abs(out - want).max() <= 1e-13 * np.abs(want).max()
  assert not hist.any() and not lin[..., 1:].any()
  A = PR.local_tangent_matrix(fes, ul, PR.virgin(fes), lam, mu, 1e3, Hh, rho,
                              0.9)
  K = ER.element_matrices(fes, lam, mu, rho, 0.9)
  assert np.abs(A - K).max() <= 1e-13 * np.abs(K).max()


# ------------------------------------------------------- header and ABI
def test_struct_layout():
  """`sfem_plasticity_args` in the header and its ctypes mirror: the fields of
  `sfem_elasticity_args` in the same order, then the plasticity fields; the
  mode values; the ABI number is unchanged (a pure addition)."""
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  text = open(os.path.join(root, 'include', 'sfem.h')).read()
  assert '#define SFEM_ABI_VERSION 10' in text and _lib.ABI_VERSION == 10
  names = _declared(text, 'sfem_plasticity_args')
  parent = _declared(text, 'sfem_elasticity_args')
  own = ['yield_const', 'hard_const', 'yield', 'hard', 'hist_in', 'hist_out',
         'lin', 'stress', 'mode']
  assert names == parent + own
  fields = _lib.PlasticityArgs._fields_
  assert names == [f[0] for f in fields], (names, fields)
  kinds = dict(fields)
  assert kinds['yield_const'] is _lib.c_dbl and kinds['hard_const'] is _lib.c_dbl
  for name in own[2:8]:
    assert kinds[name] is _lib.c_ptr
  assert kinds['mode'] is _lib.c_i32
  # the parent, 2 doubles, 6 pointers, one int32 padded to the alignment
  assert ctypes.sizeof(_lib.PlasticityArgs) == \
      ctypes.sizeof(_lib.ElasticityArgs) + 2 * 8 + 6 * 8 + 8
  assert _lib.PlasticityArgs.yield_const.offset == ctypes.sizeof(
      _lib.ElasticityArgs)
  assert re.search(r'#define SFEM_PLAST_RESIDUAL 0\b', text)
  assert re.search(r'#define SFEM_PLAST_TANGENT 1\b', text)
  assert (_lib.SFEM_PLAST_RESIDUAL, _lib.SFEM_PLAST_TANGENT) == (0, 1)
  sig = _lib.SIGNATURES['sfem_plasticity_local']
  assert sig[0]._type_ is _lib.PlasticityArgs and sig[1] is _lib.c_ptr
  assert re.search(r'int sfem_plasticity_local\(const '
                   r'sfem_plasticity_args\* args,\s*sfem_stream_t stream\);',
                   text)


# ------------------------------------------------------------- refusals
@pytest.fixture(scope='module')
def cpu_mesh():
  return TR.box_with_sides(2, 2, P).finalize(device='cpu')


def test_solve_refusals(cpu_mesh):
  """What `solve_plasticity` refuses before it touches a device."""
  import torch
  D, N = BCType.DIRICHLET, BCType.NEUMANN
  kw = dict(lame_lambda=1.0, lame_mu=1.0, yield_stress=0.1)
  clamp = {'x0': (D, (0.0, 0.0))}
  f = (0.0, -1.0)
  solve = solve_plasticity
  with pytest.raises(ValueError, match='rigid-body'):
    solve(cpu_mesh, f, {}, **kw)
  with pytest.raises(ValueError, match='rigid-body'):
    solve(cpu_mesh, f, {'x1': (N, (1.0, None))}, **kw)
  with pytest.raises(ValueError, match='DIRICHLET or NEUMANN'):
    solve(cpu_mesh, f, {'x0': (BCType.ROBIN, (0.0, 0.0))}, **kw)
  with pytest.raises(KeyError):
    solve(cpu_mesh, f, {'nowhere': (D, (0.0, 0.0))}, **kw)
  with pytest.raises(NotImplementedError, match='pmg'):
    solve(cpu_mesh, f, clamp, preconditioner='pmg', **kw)
  with pytest.raises(ValueError, match='unknown preconditioner'):
    solve(cpu_mesh, f, clamp, preconditioner='ilu', **kw)
  for bad in ((), [], 0, -2, 'up'):
    with pytest.raises(ValueError, match='load_factors'):
      solve(cpu_mesh, f, clamp, load_factors=bad, **kw)
  with pytest.raises(ValueError, match='finite'):
    solve(cpu_mesh, f, clamp, load_factors=(0.5, float('nan')), **kw)
  with pytest.raises(ValueError, match='max_newton'):
    solve(cpu_mesh, f, clamp, max_newton=0, **kw)
  with pytest.raises(NotImplementedError, match='ensemble'):
    solve(cpu_mesh.replicate(2), f, clamp, **kw)
  with pytest.raises(NotImplementedError, match='autograd'):
    solve(cpu_mesh, torch.tensor(f, requires_grad=True), clamp, **kw)
  for name in ('lame_mu', 'yield_stress', 'hardening_modulus'):
    with pytest.raises(NotImplementedError, match='autograd'):
      solve(cpu_mesh, f, clamp,
            **{**kw, name: torch.tensor(1.0, requires_grad=True)})
  with pytest.raises(TypeError):                      # there is no such mode
    solve(cpu_mesh, f, clamp, plane_stress=True, **kw)


def test_solve_refuses_partitions_and_periodic_images():
  from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
  from swirl_fem_amd.core.mesh_refiner import refine_premesh
  from swirl_fem_amd.distributed import blocks
  kw = dict(lame_lambda=1.0, lame_mu=1.0, yield_stress=0.1)
  part = blocks.build_block_partition(2, 3, (2, 1, 1), 0, device='cpu')
  with pytest.raises(NotImplementedError, match='partitioned'):
    solve_plasticity(part.mesh, (0.0, 0.0, 1.0), {}, lambda0=1.0, **kw)
  pm = unit_cube_mesh(2, ndim=2, periodic_dims=(0,))
  mesh = refine_premesh(pm, Nodes1D.create(
      P, NodeType.GAUSS_LOBATTO_LEGENDRE)).finalize(device='cpu')
  with pytest.raises(NotImplementedError, match='periodic'):
    solve_plasticity(mesh, (0.0, 1.0), {}, lambda0=1.0, **kw)


# ----------------------------------------------------------- dense Newton
def _on(x, axis, value):
  return np.abs(x[:, axis] - value) < 1e-9


def test_uniaxial_curve():
  """Slope E to sigma_y, then E Hh / (E + Hh); unloading with slope E leaves
  the plastic strain; reloading yields at the hardened stress."""
  E, sy, Hh = 2.0, 0.01, 0.5
  ey = sy / E
  path = [0.5 * ey, ey, 3 * ey, 2.5 * ey, 1.5 * ey, 3 * ey, 4 * ey]
  sig, alpha, ep = PR.uniaxial_curve(E, 0.3, sy, Hh, path)
  Et = E * Hh / (E + Hh)
  assert np.allclose(sig[:3], [0.5 * sy, sy, sy + Et * 2 * ey], atol=1e-16)
  assert alpha[1] == 0.0 and np.isclose(alpha[2], 2 * ey * E / (E + Hh))
  assert np.isclose(sig[3], sig[2] - E * 0.5 * ey) and alpha[3] == alpha[2]
  # past zero stress, still inside the hardened surface: no reverse yield
  assert -sig[2] < sig[4] < 0 and ep[4] == ep[2] > 0
  assert np.isclose(sig[5], sig[2]) and np.isclose(alpha[5], alpha[2])
  assert np.isclose(sig[6] - sig[5], Et * ey)


def test_dense_newton_reaches_uniaxial_curve():
  """One 3D element with rollers on x0, y0, z0 and a prescribed end
  displacement on x1 (free sides: uniaxial stress), loaded past yield, partly
  unloaded to zero stress... and reloaded: sigma_xx and alpha at every point
  against `uniaxial_curve` to 1e-10 sigma_y, the other stresses zero; the
  strain at zero axial stress is the residual strain eps_p."""
  from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
  from swirl_fem_amd.core.mesh_refiner import refine_premesh
  from tests import bvp_reference as BR
  ndim, Pn = 3, 2
  Em, nu, sy, Hh = 2.0, 0.3, 0.01, 0.5
  lam = Em * nu / ((1 + nu) * (1 - 2 * nu))
  mu = Em / (2 * (1 + nu))
  pm = unit_cube_mesh(1, ndim=ndim)
  pm = pm.replace(physical_groups=BR.boundary_groups(pm, TR._sides(ndim)))
  rp = refine_premesh(pm, Nodes1D.create(Pn, NodeType.GAUSS_LOBATTO_LEGENDRE))
  x = np.asarray(rp.node_coords, np.float64)
  dense = PR.DenseNewton(rp, Pn, lam, mu, sy, Hh)
  fixed = np.zeros(x.shape, bool)
  values = np.zeros(x.shape)
  for ax in range(ndim):
    fixed[_on(x, ax, 0.0), ax] = True
  end = _on(x, 0, 1.0)
  ey = sy / Em
  top = 4 * ey
  fixed[end, 0], values[end, 0] = True, top
  sig_top, al_top, ep_top = PR.uniaxial_curve(Em, nu, sy, Hh, [top])
  factors = [0.2, 0.6, 1.0, 0.8, ep_top[0] / top, 1.0, 1.2]
  want_s, want_a, want_e = PR.uniaxial_curve(Em, nu, sy, Hh,
                                             [s * top for s in factors])
  assert abs(want_s[4]) <= 1e-15 and want_a[6] > want_a[2] > 0
  hist, u = None, None
  for k, s in enumerate(factors):
    u, hist, counts = dense.solve(np.zeros(x.shape), fixed, values,
                                  history=hist, load_factors=(s,), u0=u,
                                  rtol=1e-12)
    _, trial, _, st = PR.residual(dense.fes, u, hist, lam, mu, sy, Hh)
    assert np.abs(trial - hist).max() <= 1e-14   # the state is admissible
    assert np.abs(st[..., 0] - want_s[k]).max() <= 1e-10 * sy, k
    assert np.abs(st[..., 1:]).max() <= 1e-10 * sy, k
    assert np.abs(hist[..., -1] - want_a[k]).max() <= 1e-10, k
    assert np.abs(hist[..., 0] - want_e[k]).max() <= 1e-10, k
  # the same path in one call
  u1, hist1, counts = dense.solve(np.zeros(x.shape), fixed, values,
                                  load_factors=factors, rtol=1e-12)
  assert len(counts) == len(factors)
  assert np.abs(u1 - u).max() <= 1e-12 and np.abs(hist1 - hist).max() <= 1e-12
