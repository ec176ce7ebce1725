"""Host checks of the elasticity adjoint reference
(`tests/elasticity_adjoint_reference.py`) that the GPU tests compare against,
of the form reductions of `ElasticityOperator.sensitivity` and of the struct
layout of `sfem_elasticity_sens_args`."""
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
from tests import geometry_cases as G

CASES = ((2, 4, (5, 'gl')), (3, 3, (4, 'gl')))


def _space(ndim, P, quad):
  rp = G.three_kinds(3 if ndim == 2 else 2, ndim, P).rp
  return ER.space(rp.node_coords, rp.elements, P, quad)


def _coefs(fes, rng):
  xq = ER.quad_points(fes)
  lam = 1.0 + 0.5 * xq[..., 0] ** 2 + 0.2 * rng.random(xq.shape[:2])
  mu = 0.5 + xq[..., -1] + 0.2 * rng.random(xq.shape[:2])
  rho = 1.0 + rng.random(xq.shape[:2])
  return lam, mu, rho


@pytest.mark.parametrize('lambda0', [0.0, 1.7])
def test_solve_gradient_matches_central_differences(lambda0):
  """The analytic gradient of the dense solve against the reference's own
  central difference, h = 1e-4, one random direction per coefficient, to
  1e-7 (`EA.CD_BOUND`, reasoned there).  Measured, relative: 2D lam 3.1e-9,
  mu 2.6e-9 (lambda0 = 0), lam 2.8e-9, mu 2.7e-9, rho 3.7e-10 (lambda0 =
  1.7); 3D lam 3.4e-9, mu 1.1e-8 and lam 3.0e-9, mu 6.3e-10, rho 8.5e-9.
  The force gradient is exact (the loss is linear in the force)."""
  for ndim in (2, 3):
    prob = EA.SolveProblem(ndim, lambda0)
    cds = EA.central_differences(prob)
    assert set(cds) == ({'lam', 'mu', 'rho'} if lambda0 else {'lam', 'mu'})
    for name, (rel, _, an) in cds.items():
      print(f'ndim={ndim} lambda0={lambda0} {name}: central difference vs '
            f'analytic {rel:.2e} (directional derivative {an:.3e})')
      assert rel <= EA.CD_BOUND, (ndim, name, rel)
    _, gf, *_ = prob.gradients()
    df = np.random.default_rng(12).standard_normal(gf.shape)
    cd = (prob.loss(force=prob.force + df) -
          prob.loss(force=prob.force - df)) / 2
    assert abs(cd - (gf * df).sum()) <= 1e-10 * abs((gf * df).sum())


def test_linearity_symmetry_rigid_motions():
  """sum_q (lam dlam + mu dmu + rho drho) = v . A u against
  `elasticity_reference.apply` to 1e-12 relative; sens(u, v) = sens(v, u);
  dlam = dmu = 0 for a rigid motion u."""
  rng = np.random.default_rng(1)
  for ndim, P, quad in CASES:
    fes = _space(ndim, P, quad)
    lam, mu, rho = _coefs(fes, rng)
    u = rng.standard_normal((fes.num_nodes, ndim))
    v = rng.standard_normal((fes.num_nodes, ndim))
    for l0 in (0.0, 1.3):
      dl, dm, dr = EA.point_sensitivities(fes, u, v, l0)
      Au = ER.apply(fes, u, lam, mu, rho, l0)
      want = float((v * Au).sum())
      got = float((lam * dl + mu * dm).sum() + (rho * dr).sum())
      scale = np.linalg.norm(v) * np.linalg.norm(Au)
      assert abs(got - want) <= 1e-12 * scale
      if not l0:
        assert np.abs(dr).max() == 0.0
      for a, b in zip((dl, dm, dr), EA.point_sensitivities(fes, v, u, l0)):
        assert np.abs(a - b).max() <= 1e-13 * max(np.abs(a).max(), 1e-300)
    coords = _node_coords(ndim, P)
    Hv = np.abs(EA.point_sensitivities(fes, v, v, 0.0)[1]).max()
    for m in EA.rigid_modes(coords):
      dl, dm, _ = EA.point_sensitivities(fes, m, v, 0.0)
      assert max(np.abs(dl).max(), np.abs(dm).max()) <= 1e-12 * Hv


def _node_coords(ndim, P):
  rp = G.three_kinds(3 if ndim == 2 else 2, ndim, P).rp
  return np.asarray(rp.node_coords, np.float64)


def test_sensitivities_match_differences_of_the_bilinear_form():
  """v . A(theta) u is linear in each coefficient, so a central difference is
  exact up to rounding: a random sample of points."""
  rng = np.random.default_rng(2)
  for ndim, P, quad in CASES:
    fes = _space(ndim, P, quad)
    lam, mu, rho = _coefs(fes, rng)
    u = rng.standard_normal((fes.num_nodes, ndim))
    v = rng.standard_normal((fes.num_nodes, ndim))
    l0 = 0.9
    grads = EA.point_sensitivities(fes, u, v, l0)
    f = lambda c: EA.bilinear(fes, v, u, c[0], c[1], c[2], l0)
    base = [lam, mu, rho]
    scale = abs(f(base)) + max(np.abs(g).max() for g in grads)
    E, Q = lam.shape
    for _ in range(4):
      e, q = rng.integers(E), rng.integers(Q)
      for n in range(3):
        step = np.zeros((E, Q))
        step[e, q] = 0.5
        up = [c + step if k == n else c for k, c in enumerate(base)]
        dn = [c - step if k == n else c for k, c in enumerate(base)]
        assert abs((f(up) - f(dn)) - grads[n][e, q]) <= 1e-11 * scale


def test_grid_sens_matches_point_sensitivities():
  """The kernel's steps on the P + 1 Gauss grid (which differentiates the
  interpolated degree-(P - 1) field exactly) against the physical-gradient
  form; float32 evaluation stays within 1e-4 of it."""
  rng = np.random.default_rng(3)
  for ndim, P in ((2, 5), (3, 4)):
    rp = G.three_kinds(2, ndim, P).rp
    fes = ER.space(rp.node_coords, rp.elements, P, (P + 1, 'gl'))
    real = (np.asarray(fes.elements) >= 0).all(axis=1)
    n = fes.M.shape[1]
    ul = rng.standard_normal((fes.num_elements, n, ndim))
    vl = rng.standard_normal((fes.num_elements, n, ndim))
    want = EA.local_point_sensitivities(fes, ul, vl, 1.1)
    uq = np.einsum('qi,eic->eqc', fes.M, ul)
    vq = np.einsum('qi,eic->eqc', fes.M, vl)
    got = EA.grid_sens(fes, uq, vq, 1.1)
    got32 = EA.grid_sens(fes, uq, vq, 1.1, dtype=np.float32)
    for a, b, c in zip(got, want, got32):
      assert a.shape == b.shape == (fes.num_elements, fes.Q)
      assert np.abs(a - b)[real].max() <= 1e-12 * np.abs(b)[real].max()
      assert c.dtype == np.float32
      assert np.abs(c - b)[real].max() <= 1e-4 * np.abs(b)[real].max()


def test_form_reductions():
  rng = np.random.default_rng(4)
  E, Q = 5, 7
  g = rng.standard_normal((E, Q))
  t = torch.as_tensor
  for form, src in (('scalar', 2.0), ('elem', rng.random(E)),
                    ('point', rng.random((E, Q)))):
    full = EA.expand_coefficient(src, E, Q)
    assert full.shape == (E, Q)
    want = EA.reduce_coefficient(g, form)
    eps = rng.standard_normal(np.shape(src))
    lin = (g * EA.expand_coefficient(np.asarray(src) + eps, E, Q)).sum() - \
        (g * full).sum()
    assert abs(lin - (want * eps).sum()) <= 1e-12 * abs(lin)
    got = operators.reduce_coefficient_gradient(t(g), t(src))
    assert tuple(got.shape) == np.shape(src)
    assert np.allclose(got.numpy(), want, rtol=1e-14, atol=0)
  for src in (None, lambda x: x[:, 0]):
    assert operators.reduce_coefficient_gradient(t(g), src) is None
  # the operator remembers its sources, and stays constructible without them
  names = [f.name for f in operators.dataclasses.fields(
      operators.ElasticityOperator)]
  assert 'coef_source' in names
  op = operators.ElasticityOperator(fespace=None, parts=[], host={}, lam=1.0,
                                    mu=1.0, rho=1.0)
  assert op.coef_source == (None, None, None)


def test_lame_parameters_chain():
  """`lame_parameters` is plain arithmetic: tensors E, nu that require grad
  chain through it."""
  E = torch.tensor([2.0, 3.0], dtype=torch.float64, requires_grad=True)
  nu = torch.tensor(0.3, dtype=torch.float64, requires_grad=True)
  for ps in (False, True):
    lam, mu = operators.lame_parameters(E, nu, plane_stress=ps)
    assert lam.requires_grad and mu.requires_grad
    gE, gnu = torch.autograd.grad((lam * torch.tensor([1.0, 2.0])).sum() +
                                  mu.sum(), (E, nu))
    n = 0.3
    dlam = n / ((1 + n) * (1 - 2 * n)) if not ps else n / (1 - n * n)
    dmu = 1 / (2 * (1 + n))
    assert np.allclose(gE.numpy(), [dlam + dmu, 2 * dlam + dmu], rtol=1e-13)
    assert gnu.shape == ()


def test_entry_point_refuses_without_a_gpu():
  """The status codes and messages of `sfem_elasticity_sens` for calls that
  are refused before anything touches a device (the pointers are host
  memory that is never read)."""
  lib = _lib.load()
  buf = np.zeros(64)
  p = buf.ctypes.data

  def call(**over):
    a = _lib.ElasticitySensArgs(
        u=p, v=p, wdet=p, dlam=p, dmu=p, drho=p, lambda0=1.0, geo_elem=p,
        dmat=p, weights=p, nodes=p, num_elements=1, ndim=3, P=4,
        dtype=_lib.SFEM_F64, geo_mode=_lib.GEO_AFFINE)
    for k, v in over.items():
      setattr(a, k, v)
    rc = lib.sfem_elasticity_sens(ctypes.byref(a), None)
    return rc, lib.sfem_last_error().decode(errors='replace')
  for over in (dict(P=13), dict(P=1), dict(ndim=1), dict(ndim=4)):
    rc, msg = call(**over)
    assert rc == -3 and msg.startswith('sfem_elasticity_sens:'), (over, msg)
  for over in (dict(u=None), dict(v=None), dict(wdet=None),
               dict(dlam=None, dmu=None, drho=None)):
    rc, msg = call(**over)
    assert rc == -1 and msg.startswith('sfem_elasticity_sens:'), (over, msg)
  assert lib.sfem_elasticity_sens(None, None) == -1
  assert call(num_elements=0, u=None, v=None)[0] == 0


def test_struct_layout():
  """`sfem_elasticity_sens_args` in the header against its ctypes mirror; the
  geometry and launch fields are those of `sfem_elasticity_args` in the same
  order; the ABI number stays 10."""
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  text = open(os.path.join(root, 'include', 'sfem.h')).read()
  assert '#define SFEM_ABI_VERSION 10' in text and _lib.ABI_VERSION == 10

  def declared(struct):
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
  names = declared('sfem_elasticity_sens_args')
  fields = [f[0] for f in _lib.ElasticitySensArgs._fields_]
  assert names == fields
  assert fields[:7] == ['u', 'v', 'wdet', 'dlam', 'dmu', 'drho', 'lambda0']
  parent = declared('sfem_elasticity_args')
  assert fields[7:] == parent[parent.index('kfac'):]
  kinds = dict(_lib.ElasticitySensArgs._fields_)
  assert kinds['lambda0'] is _lib.c_dbl and kinds['num_elements'] is _lib.c_i64
  assert kinds['geo_mode'] is _lib.c_i32
  assert ctypes.sizeof(_lib.ElasticitySensArgs) == 7 * 8 + 7 * 8 + 2 * 8 + 4 * 4
  assert _lib.SIGNATURES['sfem_elasticity_sens'][0]._type_ is \
      _lib.ElasticitySensArgs
  assert re.search(r'int sfem_elasticity_sens\(const sfem_elasticity_sens_args',
                   text)
