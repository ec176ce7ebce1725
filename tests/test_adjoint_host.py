"""Host checks of the adjoint reference (`tests/adjoint_reference.py`) that the
GPU tests compare against, of the form reductions of `op.sensitivity`, and of
the struct layout of the transposed-mode field."""
import os
import re

import numpy as np
import torch

from swirl_fem_amd import _lib
from swirl_fem_amd.core import operators
from tests import adjoint_reference as AJ
from tests import geometry_cases as G

def _fields(fes, rng):
  xq = AJ.quad_points(fes)
  k = 1.0 + 0.5 * xq[..., 0] ** 2 + 0.2 * rng.random(xq.shape[:2])
  c = 0.5 + xq[..., -1] + 0.2 * rng.random(xq.shape[:2])
  b = rng.standard_normal(xq.shape)
  return k, c, b


CASES = ((2, 4, (5, 'gl')), (3, 3, (4, 'gl')), (2, 5, (5, 'gll')))


def test_factored_form_equals_dense_matrices():
  rng = np.random.default_rng(0)
  for ndim, P, quad in CASES:
    rp = G.three_kinds(3, ndim, P).rp
    fes = AJ.space(rp.node_coords, rp.elements, P, quad)
    k, c, b = _fields(fes, rng)
    ul = rng.standard_normal((fes.num_elements, fes.n))
    m = AJ.element_matrices(fes, 0.7, 1.3, k, c, b)
    mt = AJ.element_matrices_transpose(fes, 0.7, 1.3, k, c, b)
    want = np.einsum('eij,ej->ei', m, ul)
    got = AJ.local_apply(fes, ul, 0.7, 1.3, k, c, b)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    want = np.einsum('eij,ej->ei', mt, ul)
    got = AJ.local_apply_transpose(fes, ul, 0.7, 1.3, k, c, b)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # the assembled transpose is the transpose of the assembled matrix
    A = AJ.matrix(fes, 0.7, 1.3, k, c, b)
    v = rng.standard_normal(fes.num_nodes)
    got = AJ.apply_transpose(fes, v, 0.7, 1.3, k, c, b)
    assert np.abs(got - A.T @ v).max() <= 1e-12 * np.abs(A.T @ v).max()
    assert np.abs(A - A.T).max() > 1e-3 * np.abs(A).max()


def test_sensitivities_match_central_differences():
  """lam . A(theta) u is linear in each of k, c, b, so a central difference is
  exact up to rounding: every entry of a random sample of points."""
  rng = np.random.default_rng(1)
  for ndim, P, quad in CASES:
    rp = G.three_kinds(3, ndim, P).rp
    fes = AJ.space(rp.node_coords, rp.elements, P, quad)
    k, c, b = _fields(fes, rng)
    u = rng.standard_normal(fes.num_nodes)
    lam = rng.standard_normal(fes.num_nodes)
    l0, l1 = 0.7, 1.3
    dk, dc, db = AJ.sensitivities(fes, u, lam, l0, l1)
    f = lambda k_, c_, b_: AJ.bilinear(fes, lam, u, l0, l1, k_, c_, b_)
    scale = abs(f(k, c, b)) + np.abs(dk).max()
    h = 0.5
    E, Q = k.shape
    for _ in range(6):
      e, q, j = rng.integers(E), rng.integers(Q), rng.integers(ndim)
      d = np.zeros_like(k); d[e, q] = h
      assert abs((f(k + d, c, b) - f(k - d, c, b)) / (2 * h) - dk[e, q]) \
          <= 1e-11 * scale
      assert abs((f(k, c + d, b) - f(k, c - d, b)) / (2 * h) - dc[e, q]) \
          <= 1e-11 * scale
      d = np.zeros_like(b); d[e, q, j] = h
      assert abs((f(k, c, b + d) - f(k, c, b - d)) / (2 * h) - db[e, q, j]) \
          <= 1e-11 * scale
    # the kernel's form of the velocity gradient: d/dbeta, chained through
    # the fold, is d/db
    ul, ll = fes.gather(u), fes.gather(lam)
    if quad[1] == 'gll':
      _, _, dbeta = AJ.kernel_sensitivities(fes, ul, ll, l0, l1)
      back = AJ.wdet(fes)[..., None] * np.einsum('eqd,eqjd->eqj', dbeta,
                                                 fes.invjacs)
      assert np.abs(back - db).max() <= 1e-12 * np.abs(db).max()


def test_solve_gradient_matches_central_differences():
  for ndim in (2, 3):
    rp, P, quad, dmask, facets, x = AJ.dense_problem(ndim)
    fes = AJ.space(x, rp.elements, P, (quad, 'gl'))
    f, w, dvals, k_q, c_e, b_q = AJ.problem_data(fes, x, dmask, ndim, True)
    E, Q = k_q.shape
    c_q = AJ.expand_coefficient(c_e, E, Q)
    prob = AJ.DenseProblem(rp, facets, P, quad, AJ.L0, AJ.L1, dvals, AJ.ROBIN, AJ.NEUMANN)
    rk, rb, *_ = AJ.central_difference(prob, w, f, k_q, c_q, b_q,
                                    np.random.default_rng(11))
    print(f'ndim={ndim}: central difference vs analytic, k {rk:.2e} b {rb:.2e}')
    assert rk <= AJ.CD_BOUND and rb <= AJ.CD_BOUND
    # the forcing and the reaction, entry by entry (the loss is linear in f)
    gf, _, gc, _ = prob.gradient(w, f, k_q, c_q, b_q)
    rng = np.random.default_rng(12)
    df = rng.standard_normal(len(f))
    cd = (prob.loss(w, f + df, k_q, c_q, b_q) -
          prob.loss(w, f - df, k_q, c_q, b_q)) / 2
    assert abs(cd - gf @ df) <= 1e-10 * abs(gf @ df)
    dc = rng.standard_normal(c_q.shape)
    h = 1e-3
    cd = (prob.loss(w, f, k_q, c_q + h * dc, b_q) -
          prob.loss(w, f, k_q, c_q - h * dc, b_q)) / (2 * h)
    assert abs(cd - (gc * dc).sum()) <= AJ.CD_BOUND * abs((gc * dc).sum()) * 10


def test_form_reductions():
  rng = np.random.default_rng(2)
  E, Q, d = 5, 7, 3
  g = rng.standard_normal((E, Q))
  gb = rng.standard_normal((E, Q, d))
  t = torch.as_tensor
  # the reference's reductions are the chain rule of its expansions
  for form, src in (('scalar', 2.0), ('elem', rng.random(E)),
                    ('point', rng.random((E, Q)))):
    full = AJ.expand_coefficient(src, E, Q)
    assert full.shape == (E, Q)
    want = AJ.reduce_coefficient(g, form)
    eps = rng.standard_normal(np.shape(src))
    lin = (g * AJ.expand_coefficient(np.asarray(src) + eps, E, Q)).sum() - \
        (g * full).sum()
    assert abs(lin - (want * eps).sum()) <= 1e-12 * abs(lin)
    got = operators.reduce_coefficient_gradient(t(g), t(src))
    assert tuple(got.shape) == np.shape(src)
    assert np.allclose(got.numpy(), want, rtol=1e-14, atol=0)
  assert operators.reduce_coefficient_gradient(t(g), 2.0).shape == ()
  for form, src in (('constant', rng.random(d)), ('elem', rng.random((E, d))),
                    ('point', rng.random((E, Q, d)))):
    full = AJ.expand_velocity(src, E, Q)
    assert full.shape == (E, Q, d)
    want = AJ.reduce_velocity(gb, form)
    eps = rng.standard_normal(np.shape(src))
    lin = (gb * AJ.expand_velocity(src + eps, E, Q)).sum() - (gb * full).sum()
    assert abs(lin - (want * eps).sum()) <= 1e-12 * abs(lin)
    got = operators.reduce_velocity_gradient(t(gb), t(src))
    assert tuple(got.shape) == np.shape(src)
    assert np.allclose(got.numpy(), want, rtol=1e-14, atol=0)
  # absent and callable coefficients have no gradient
  for src in (None, lambda x: x[:, 0]):
    assert operators.reduce_coefficient_gradient(t(g), src) is None
    assert operators.reduce_velocity_gradient(t(gb), src) is None


def test_struct_layout():
  """`adv_transpose` directly after `beta`; `kappa, sigma, coef_mode` stay the
  tail, in the header and in the ctypes mirror; the new entry point's struct
  mirrors its header too."""
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  text = open(os.path.join(root, 'include', 'sfem.h')).read()
  assert '#define SFEM_ABI_VERSION 10' in text and _lib.ABI_VERSION == 10
  for struct, cls in (('sfem_helmholtz_args', _lib.HelmholtzArgs),
                      ('sfem_helmholtz_sens_args', _lib.HelmholtzSensArgs)):
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
    fields = [f[0] for f in cls._fields_]
    assert names == fields, (struct, names, fields)
  fields = [f[0] for f in _lib.HelmholtzArgs._fields_]
  assert fields[-3:] == ['kappa', 'sigma', 'coef_mode']
  assert fields[-5:-3] == ['beta', 'adv_transpose']
  assert dict(_lib.HelmholtzArgs._fields_)['adv_transpose'] is _lib.c_i32
  assert 'sfem_helmholtz_sens' in _lib.SIGNATURES
