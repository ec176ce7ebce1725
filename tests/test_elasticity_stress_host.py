"""Host checks of the stress-recovery reference
(`tests/elasticity_stress_reference.py`) that the GPU tests compare against,
of `operators.von_mises`, of the struct layouts of
`sfem_elasticity_stress_args` / `sfem_elasticity_stress_vjp_args` and of the
entry points' refusals before a device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from swirl_fem_amd import _lib
from swirl_fem_amd.core import operators
from tests import elasticity_adjoint_reference as EA
from tests import elasticity_reference as ER
from tests import elasticity_stress_reference as SR
from tests import geometry_cases as G

CASES = ((2, 4, (5, 'gl')), (3, 3, (4, 'gl')))


def _space(ndim, P, quad, kind='three_kinds', n=None):
  n = (3 if ndim == 2 else 2) if n is None else n
  rp = getattr(G, kind)(n, ndim, P).rp
  return ER.space(rp.node_coords, rp.elements, P, quad), rp


def _coefs(fes, rng):
  xq = ER.quad_points(fes)
  lam = 1.0 + 0.5 * xq[..., 0] ** 2 + 0.2 * rng.random(xq.shape[:2])
  mu = 0.5 + xq[..., -1] + 0.2 * rng.random(xq.shape[:2])
  return lam, mu


def _rel(a, b):
  return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _analytic(A, lam, mu, plane_stress=False):
  """Voigt stress of the constant displacement gradient A."""
  return SR._stress_of(np.asarray(A, np.float64), np.float64(lam),
                       np.float64(mu), plane_stress)


def test_grid_stress_matches_point_stress():
  """The kernels' steps on the P + 1 Gauss grid (which differentiates the
  interpolated degree-(P - 1) field exactly) against the physical-gradient
  form, forward and vjp, plane strain and plane stress; float32 evaluation
  stays within 1e-4 of it."""
  rng = np.random.default_rng(3)
  for ndim, P in ((2, 5), (3, 4)):
    rp = G.three_kinds(2, ndim, P).rp
    fes = ER.space(rp.node_coords, rp.elements, P, (P + 1, 'gl'))
    lam, mu = _coefs(fes, rng)
    E, n, nv = fes.num_elements, fes.M.shape[1], SR.num_slots(ndim)
    ul = rng.standard_normal((E, n, ndim))
    uq = np.einsum('qi,eic->eqc', fes.M, ul)
    sbar = rng.standard_normal((E, fes.Q, nv))
    for ps in ((False, True) if ndim == 2 else (False,)):
      want = SR.point_stress(fes, ul, lam, mu, ps)
      got = SR.grid_stress(fes, uq, lam, mu, ps)
      got32 = SR.grid_stress(fes, uq, lam, mu, ps, dtype=np.float32)
      assert got.shape == want.shape == (E, fes.Q, nv)
      assert _rel(got, want) <= 1e-12
      assert got32.dtype == np.float32 and _rel(got32, want) <= 1e-4
      ub, dl, dm = SR.point_stress_vjp(fes, sbar, ul, lam, mu, ps)
      gub, gdl, gdm = SR.grid_stress_vjp(fes, sbar, uq, lam, mu, ps)
      # ubar of the grid form is a cotangent on the grid: I^T takes it to the
      # element's nodes
      assert _rel(np.einsum('qi,eqc->eic', fes.M, gub), ub) <= 1e-12
      assert _rel(gdl, dl) <= 1e-12 and _rel(gdm, dm) <= 1e-12
      for a, b in zip(SR.grid_stress_vjp(fes, sbar, uq, lam, mu, ps,
                                         dtype=np.float32), (gub, gdl, gdm)):
        assert a.dtype == np.float32 and _rel(a, b) <= 1e-4


def test_adjoint_linearity_and_stiffness_identities():
  """<sbar, sigma(u)> = <ubar, u> to 1e-12; sum_q (lam dlam + mu dmu) =
  <sbar, sigma(u)> (sigma is linear in (lam, mu)); B^T W sigma = K u:
  `grid_stress_vjp(W sigma(u)).ubar` equals `ER.grid_apply(u)` with lambda0 =
  0.  B^T alone is the vjp at lam = 0, mu = 1/2 (sigma = eps there), and the
  Voigt pairing counts a shear slot once where sigma : eps counts it twice,
  so the cotangent is `SR.work_conjugate(W sigma)`: shear slots doubled, the
  2D zz slot (no in-plane strain is conjugate to it) set to zero.  With the
  material's own lam and mu the vjp would apply the constitutive law a
  second time."""
  rng = np.random.default_rng(5)
  for ndim, P, quad in CASES:
    fes, _ = _space(ndim, P, quad)
    lam, mu = _coefs(fes, rng)
    E, nq, nv = fes.num_elements, fes.Q, SR.num_slots(ndim)
    W = ER._wdet(fes)
    uq = rng.standard_normal((E, nq, ndim))
    sbar = rng.standard_normal((E, nq, nv))
    for ps in ((False, True) if ndim == 2 else (False,)):
      sig = SR.grid_stress(fes, uq, lam, mu, ps)
      ub, dl, dm = SR.grid_stress_vjp(fes, sbar, uq, lam, mu, ps)
      pair = float((sbar * sig).sum())
      scale = np.linalg.norm(sbar) * np.linalg.norm(sig)
      assert abs(pair - float((ub * uq).sum())) <= 1e-12 * scale
      assert abs(pair - float((lam * dl + mu * dm).sum())) <= 1e-12 * scale
      got = SR.grid_stress_vjp(fes, SR.work_conjugate(W[..., None] * sig),
                               uq, 0.0, 0.5)[0]
      assert _rel(got, ER.grid_apply(fes, uq, lam, mu)) <= 1e-12
    # the same identities for the physical-gradient form
    ul = rng.standard_normal((E, fes.M.shape[1], ndim))
    sig = SR.point_stress(fes, ul, lam, mu)
    ub, dl, dm = SR.point_stress_vjp(fes, sbar, ul, lam, mu)
    pair = float((sbar * sig).sum())
    scale = np.linalg.norm(sbar) * np.linalg.norm(sig)
    assert abs(pair - float((ub * ul).sum())) <= 1e-12 * scale
    assert abs(pair - float((lam * dl + mu * dm).sum())) <= 1e-12 * scale


def test_rigid_motions_and_linear_fields():
  """Rigid motions give zero stress; a linear displacement gives the constant
  analytic stress on affine, multilinear and curved elements, and lumped
  recovery reproduces it at every node (relative 1e-11: the inverse
  Jacobians of the curved elements)."""
  rng = np.random.default_rng(6)
  for ndim, P, quad in CASES:
    fes, rp = _space(ndim, P, quad)
    x = np.asarray(rp.node_coords, np.float64)
    lam, mu = 1.3, 0.7
    v = rng.standard_normal((fes.num_nodes, ndim))
    size = np.abs(SR.point_stress(fes, fes.gather(v), lam, mu)).max()
    for m in EA.rigid_modes(x):
      s = SR.point_stress(fes, fes.gather(m), lam, mu)
      assert np.abs(s).max() <= 1e-12 * size
    A = rng.standard_normal((ndim, ndim))
    u = x @ A.T + rng.standard_normal(ndim)
    for ps in ((False, True) if ndim == 2 else (False,)):
      want = _analytic(A, lam, mu, ps)
      assert np.abs(want[:ndim]).min() > 0 and abs(want[ndim]) > 0
      sq = SR.point_stress(fes, fes.gather(u), lam, mu, ps)
      assert np.abs(sq - want).max() <= 1e-11 * np.abs(want).max()
      sn = SR.lumped_recovery(fes, sq)
      assert sn.shape == (fes.num_nodes, SR.num_slots(ndim))
      assert np.abs(sn - want).max() <= 1e-11 * np.abs(want).max()
      vm = SR.von_mises(sn)
      assert np.abs(vm - SR.von_mises(want)).max() <= 1e-11 * vm.max()


def test_l2_recovery_reproduces_polynomials():
  """On an affine mesh a displacement of total degree p has a stress of
  degree p - 1, which lies in the space, and the solve's Gauss rule
  integrates mass matrix and right-hand side exactly: the 'l2' nodal stress
  is the analytic polynomial (1e-10).  So is the lumped one here: phi_i sigma
  has degree 2 p - 1, which the GLL rule on the element's own nodes
  integrates exactly, so int phi_i sigma = sigma(x_i) int phi_i."""
  for ndim, P in ((2, 4), (3, 3)):
    p = P - 1
    q = p + (ndim + 1) // 2
    fes, rp = _space(ndim, P, (q, 'gl'), 'affine', 2)
    x = np.asarray(rp.node_coords, np.float64)
    lam, mu = 1.1, 0.9
    # u_c = (a_c . x)^p + x_0 x_1^(p-1): H analytic
    a = np.array([[0.7, -0.4, 0.3], [0.2, 0.9, -0.5], [-0.6, 0.1, 0.8]])
    a = a[:ndim, :ndim]

    def fields(y):
      s = y @ a.T                                  # (M, d): a_c . y
      u = s ** p
      u[:, 0] += y[:, 0] * y[:, 1] ** (p - 1)
      H = p * s[:, :, None] ** (p - 1) * a[None]
      H[:, 0, 0] += y[:, 1] ** (p - 1)
      H[:, 0, 1] += (p - 1) * y[:, 0] * y[:, 1] ** (p - 2)
      return u, H
    u, H = fields(x)
    want = SR._stress_of(H, np.float64(lam), np.float64(mu), False)
    sq = SR.point_stress(fes, fes.gather(u), lam, mu)
    l2 = SR.l2_recovery(fes, sq)
    err = _rel(l2, want)
    lumped = _rel(SR.lumped_recovery(fes, sq), want)
    print(f'{ndim}D p={p}: l2 {err:.2e}, lumped {lumped:.2e}')
    assert err <= 1e-10 and lumped <= 1e-10


def test_plane_strain_and_plane_stress_slots():
  """2D: sigma_zz = lam tr(H) under plane strain and 0 under plane stress; the
  von Mises stress takes the zz slot into account; with the modified lambda
  of `lame_parameters(..., plane_stress=True)` the in-plane stress is that of
  the 3D law with sigma_zz = 0."""
  young, nu = 2.5, 0.3
  A = np.array([[0.3, -0.2], [0.5, 0.1]])
  lam, mu = operators.lame_parameters(young, nu)
  s = _analytic(A, lam, mu)
  assert np.isclose(s[3], lam * np.trace(A), rtol=1e-14)
  assert np.isclose(s[3], nu * (s[0] + s[1]), rtol=1e-13)
  lam_ps, _ = operators.lame_parameters(young, nu, plane_stress=True)
  t = _analytic(A, lam_ps, mu, True)
  assert t[3] == 0.0
  # 3D Hooke with sigma_zz = 0: eps_zz = -lam (exx + eyy) / (lam + 2 mu)
  ezz = -lam * np.trace(A) / (lam + 2 * mu)
  full = np.zeros((3, 3))
  full[:2, :2] = A
  full[2, 2] = ezz
  want = ER.stress(full, lam, mu)
  assert abs(want[2, 2]) <= 1e-14
  assert np.allclose(t[:3], [want[0, 0], want[1, 1], want[0, 1]], rtol=1e-13)
  vm = lambda v: np.sqrt(0.5 * ((v[0] - v[1]) ** 2 + (v[1] - v[3]) ** 2 +
                                (v[3] - v[0]) ** 2) + 3 * v[2] ** 2)
  assert np.isclose(SR.von_mises(s), vm(s), rtol=1e-14)
  assert np.isclose(SR.von_mises(t), np.sqrt(t[0] ** 2 - t[0] * t[1] +
                                             t[1] ** 2 + 3 * t[2] ** 2),
                    rtol=1e-14)
  assert abs(SR.von_mises(s) - SR.von_mises(t)) > 1e-3


# --------------------------------------------------------- solve functionals
@pytest.mark.parametrize('where', ['quadrature', 'nodes'])
@pytest.mark.parametrize('ndim', [2, 3])
def test_functional_gradients_match_central_differences(ndim, where):
  """`SR.functional_gradients` (implicit part through the dense adjoint solve
  plus the explicit dependence of sigma on lam and mu) against the
  reference's own central difference with the set-up of
  `test_elasticity_adjoint_host`: h = 1e-4, one-signed relative directions,
  bound 1e-7 (`EA.CD_BOUND`; J is quadratic in u and in the coefficients, so
  along theta (1 + t) it behaves like a rational function of 1 + t as the
  loss there does).  The problem's fields have a non-zero deviatoric stress.
  Measured, relative: 2D quadrature lam 5.5e-9, mu 7.9e-9, force 9.1e-11;
  2D nodes lam 5.4e-9, mu 4.0e-9, force 8.3e-11; 3D quadrature lam 5.6e-9,
  mu 3.6e-8, force 3.9e-11; 3D nodes lam 5.4e-9, mu 4.6e-9, force 3.6e-11."""
  prob = EA.SolveProblem(ndim, 0.0)
  dense = prob.dense()
  u = prob.solve(dense)
  sq = SR.point_stress(dense.fes, dense.fes.gather(u), *dense.coefs[:2])
  assert SR.von_mises(sq).min() > 1e-3 * np.abs(sq).max()
  for name, (rel, _, an) in SR.central_differences(prob, where).items():
    print(f'ndim={ndim} {where} {name}: central difference vs analytic '
          f'{rel:.2e} (directional derivative {an:.3e})')
    assert rel <= EA.CD_BOUND, (ndim, where, name, rel)


def test_tension_reference_stress():
  """The dense reference's own stress error on the uniaxial-tension and the
  plane-stress problem of the GPU tests, at quadrature points and lumped
  nodes, relative to the traction: the GPU tests allow 10 times what they
  measure here, and never less than their solver bound.  Bound: 100 cond eps
  (the linear solution lies in the space, so only rounding is left).
  Measured: 2D 7.8e-15, 3D 2.3e-14, plane stress 1.2e-14 (cond 3.0e2, 6.5e2,
  2.7e2)."""
  for ndim, ps in ((2, False), (3, False), (2, True)):
    rp, P, (lam, mu), t, u, want, cond = SR.tension_problem(ndim, ps)
    fes = ER.Dense(rp, P, lam, mu).fes
    sq = SR.point_stress(fes, fes.gather(u), lam, mu, ps)
    sn = SR.lumped_recovery(fes, sq)
    err = max(np.abs(sq - want).max(), np.abs(sn - want).max()) / t
    print(f'tension {ndim}D plane_stress={ps}: stress error {err:.2e}, cond '
          f'{cond:.2e}')
    assert err <= 100.0 * cond * 1e-16


@pytest.mark.parametrize('ndim', [2, 3])
def test_lumped_weights_positive(ndim):
  """The denominator of lumped recovery on the meshes of the GPU tests, with
  the solve's Gauss rule: minima 1.3e-5 .. 6.9e-3, all > 0."""
  for kind in ('three_kinds', 'affine', 'multilinear'):
    for P in (3, 5):
      q = P - 1 + (ndim + 1) // 2
      fes, _ = _space(ndim, P, (q, 'gl'), kind, 2)
      m = SR.lumped_weights(fes)
      print(f'{kind} {ndim}D P={P}: min lumped weight {m.min():.2e}')
      assert m.min() > 0
      assert np.isclose(m.sum(), ER._wdet(fes).sum(), rtol=1e-13)


def test_von_mises_on_cpu_tensors():
  rng = np.random.default_rng(8)
  for ndim in (2, 3):
    s = rng.standard_normal((7, 5, SR.num_slots(ndim)))
    got = operators.von_mises(torch.as_tensor(s), ndim)
    assert tuple(got.shape) == (7, 5)
    assert np.allclose(got.numpy(), SR.von_mises(s), rtol=1e-14, atol=0)
    t = torch.as_tensor(s).requires_grad_(True)
    (operators.von_mises(t, ndim) ** 2).sum().backward()
    assert np.allclose(t.grad.numpy(), SR.von_mises_sq_gradient(s),
                       rtol=1e-12, atol=1e-13)
  with pytest.raises(ValueError):
    operators.von_mises(torch.zeros(3, 6), 2)
  with pytest.raises(ValueError):
    operators.von_mises(torch.zeros(3, 4), 3)


# ------------------------------------------------------------------ C ABI
def _declared(text, struct):
  body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (struct, struct),
                   text, flags=re.S).group(1)
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  names = []
  for decl in body.split(';'):
    decl = decl.strip()
    if decl:
      first, *rest = decl.split(',')
      names.append(re.findall(r'\w+', first)[-1])
      names += [r.strip() for r in rest]
  return names


def test_struct_layouts():
  """Both argument structs in the header against their ctypes mirrors: data
  pointers first, then lam_const / mu_const, then the geometry and launch
  fields of `sfem_elasticity_args` in the same order, then `plane_stress`;
  the ABI number stays 10."""
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  text = open(os.path.join(root, 'include', 'sfem.h')).read()
  assert '#define SFEM_ABI_VERSION 10' in text and _lib.ABI_VERSION == 10
  parent = _declared(text, 'sfem_elasticity_args')
  tail = parent[parent.index('kfac'):] + ['plane_stress']
  for struct, mirror, head, entry in (
      ('sfem_elasticity_stress_args', _lib.ElasticityStressArgs,
       ['u', 'sigma', 'vm', 'wdet', 'lam', 'mu', 'lam_const', 'mu_const'],
       'sfem_elasticity_stress'),
      ('sfem_elasticity_stress_vjp_args', _lib.ElasticityStressVjpArgs,
       ['sbar', 'u', 'ubar', 'dlam', 'dmu', 'wdet', 'lam', 'mu', 'lam_const',
        'mu_const'], 'sfem_elasticity_stress_vjp')):
    names = _declared(text, struct)
    fields = [f[0] for f in mirror._fields_]
    assert names == fields == head + tail, struct
    kinds = dict(mirror._fields_)
    assert kinds['lam_const'] is _lib.c_dbl
    assert kinds['num_elements'] is _lib.c_i64
    assert kinds['plane_stress'] is _lib.c_i32
    # pointers and doubles, 7 geometry pointers, 2 int64, 5 int32 (+ padding)
    assert ctypes.sizeof(mirror) == len(head) * 8 + 7 * 8 + 2 * 8 + 6 * 4
    assert _lib.SIGNATURES[entry][0]._type_ is mirror
    assert re.search(r'int %s\(const %s\*' % (entry, struct), text)


def test_entry_points_refuse_without_a_gpu():
  """The status codes and messages of both entry points for calls that are
  refused before anything touches a device (the pointers are host memory
  that is never read)."""
  lib = _lib.load()
  buf = np.zeros(64)
  p = buf.ctypes.data
  common = dict(wdet=p, geo_elem=p, dmat=p, weights=p, nodes=p,
                num_elements=1, ndim=3, P=4, dtype=_lib.SFEM_F64,
                geo_mode=_lib.GEO_AFFINE)

  def caller(name, cls, **fields):
    def call(**over):
      a = cls(**common, **fields)
      for k, v in over.items():
        setattr(a, k, v)
      rc = getattr(lib, name)(ctypes.byref(a), None)
      return rc, lib.sfem_last_error().decode(errors='replace')
    return call
  fwd = caller('sfem_elasticity_stress', _lib.ElasticityStressArgs, u=p,
               sigma=p, vm=p)
  vjp = caller('sfem_elasticity_stress_vjp', _lib.ElasticityStressVjpArgs,
               sbar=p, u=p, ubar=p, dlam=p, dmu=p)
  invalid = {
      fwd: (dict(u=None), dict(wdet=None), dict(dmat=None),
            dict(sigma=None, vm=None), dict(geo_elem=None),
            dict(num_elements=-1), dict(dtype=5)),
      vjp: (dict(sbar=None), dict(wdet=None), dict(dmat=None),
            dict(ubar=None, dlam=None, dmu=None), dict(u=None),
            dict(u=None, dlam=None), dict(geo_elem=None),
            dict(num_elements=-1), dict(dtype=5)),
  }
  for call, name in ((fwd, 'sfem_elasticity_stress:'),
                     (vjp, 'sfem_elasticity_stress_vjp:')):
    for over in (dict(P=13), dict(P=1), dict(ndim=1), dict(ndim=4),
                 dict(geo_mode=_lib.GEO_BOX), dict(geo_mode=7)):
      rc, msg = call(**over)
      assert rc == -3 and msg.startswith(name), (over, msg)
    for over in invalid[call]:
      rc, msg = call(**over)
      assert rc == -1 and msg.startswith(name), (over, msg)
  rc, msg = fwd(sigma=None, vm=None)
  assert rc == -1 and 'output' in msg
  assert lib.sfem_elasticity_stress(None, None) == -1
  assert lib.sfem_elasticity_stress_vjp(None, None) == -1
  # nothing to do is not an error
  assert fwd(num_elements=0, u=None)[0] == 0
  assert vjp(num_elements=0, sbar=None, u=None)[0] == 0
