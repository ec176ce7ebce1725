"""Host-side checks of scalar transport: the NumPy reference
(`tests/transport_reference.py`) against the dense advection reference, the
BDF/EXT coefficient conventions, the ctypes mirror of the new argument
struct, and the reference stepper's temporal order against the exact
semi-discrete solution."""
import ctypes
import os
import re

import numpy as np
import pytest

from swirl_fem_amd import _lib
from swirl_fem_amd.navier_stokes.navier_stokes import bdfk_coeffs, extk_coeffs
from tests import advection_reference as AR
from tests import transport_reference as TR


@pytest.mark.parametrize('ndim,P,Q', [(2, 4, 5), (3, 3, 4), (2, 3, 3)])
def test_integrand_matches_dense_reference(ndim, P, Q):
  """M^T integrand = sum_j (m_j B + c_j C(u_j))_local T_j + M^T W s with the
  element matrices of `advection_reference` (Q >= P: the derivative of the
  interpolant on the q-grid is exact)."""
  rp = TR.box_with_sides(2, ndim, P, three_kinds=True)
  fes = AR.space(rp.node_coords, rp.elements, P, (Q, 'gl'))
  rng = np.random.default_rng(ndim + P)
  E, n = fes.num_elements, fes.n
  Bl = AR.element_matrices(fes, 1.0, 0.0)
  levels, want = [], np.zeros((E, n))
  for j, (mc, cc, vel) in enumerate([(0.7, -1.3, True), (-2.0, 0.0, True),
                                     (0.4, 0.9, False)]):
    Tl = rng.standard_normal((E, n))
    uq = rng.standard_normal((E, fes.Q, ndim)) if vel else None
    levels.append((np.einsum('qi,ei->eq', fes.M, Tl), uq, mc, cc))
    want += mc * np.einsum('eij,ej->ei', Bl, Tl)
    if vel and cc:
      want += cc * AR.advection_local(fes, Tl, uq)
  sq = rng.standard_normal((E, fes.Q))
  want += np.einsum('qi,eq->ei', fes.M, TR.wdet(fes) * sq)
  got = np.einsum('qi,eq->ei', fes.M, TR.integrand(fes, levels, sq))
  assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
  # one level, no source, no mass: the convective term alone
  Tl = rng.standard_normal((E, n))
  uq = rng.standard_normal((E, fes.Q, ndim))
  got = np.einsum('qi,eq->ei', fes.M, TR.integrand(
      fes, [(np.einsum('qi,ei->eq', fes.M, Tl), uq, 0.0, 1.0)]))
  want = AR.advection_local(fes, Tl, uq)
  assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_coefficient_conventions():
  """A step of order k takes bdfk_coeffs(k) (k + 1 entries, the new level's
  last) and extk_coeffs(k - 1) (k entries), oldest first."""
  bdf = {1: [-1.0, 1.0], 2: [0.5, -2.0, 1.5],
         3: [-1.0 / 3.0, 1.5, -3.0, 11.0 / 6.0]}
  ext = {1: [1.0], 2: [-1.0, 2.0], 3: [1.0, -3.0, 3.0]}
  for k in (1, 2, 3):
    b, e = bdfk_coeffs(k), extk_coeffs(k - 1)
    assert b.shape == (k + 1,) and e.shape == (k,)
    np.testing.assert_allclose(b, bdf[k], rtol=0, atol=1e-13)
    np.testing.assert_allclose(e, ext[k], rtol=0, atol=1e-13)
    rb, re_ = TR.coefficients(k)
    np.testing.assert_allclose(rb, b, rtol=0, atol=1e-13)
    np.testing.assert_allclose(re_, e, rtol=0, atol=1e-13)
    # steady consistency
    assert abs(b.sum()) <= 1e-13 and abs(e.sum() - 1.0) <= 1e-13
  # oldest first: a linear history t_j = j is extrapolated to the next level
  # and differentiated to 1
  for k in (2, 3):
    t = np.arange(k, dtype=float)
    assert abs(extk_coeffs(k - 1) @ t - k) <= 1e-13
    assert abs(bdfk_coeffs(k) @ np.arange(k + 1.0) - 1.0) <= 1e-13


def test_struct_layout():
  """`sfem_transport_args` in the header and its ctypes mirror: the same
  fields in the same order, arrays of SFEM_TRANSPORT_LEVELS; the ABI number
  is unchanged (a pure addition)."""
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  text = open(os.path.join(root, 'include', 'sfem.h')).read()
  assert '#define SFEM_ABI_VERSION 10' in text and _lib.ABI_VERSION == 10
  levels = int(re.search(r'#define SFEM_TRANSPORT_LEVELS (\d+)', text).group(1))
  assert levels == _lib.SFEM_TRANSPORT_LEVELS == 3
  body = re.search(r'typedef struct sfem_transport_args \{(.*?)\} '
                   r'sfem_transport_args;', text, flags=re.S).group(1)
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  names, arrays = [], set()
  for decl in body.split(';'):
    decl = decl.strip()
    if not decl:
      continue
    first, *rest = decl.split(',')
    m = re.search(r'(\w+)\s*\[\s*SFEM_TRANSPORT_LEVELS\s*\]$', first)
    if m:
      names.append(m.group(1))
      arrays.add(m.group(1))
    else:
      names.append(re.findall(r'\w+', first)[-1])
    names += [r.strip() for r in rest]
  fields = _lib.TransportArgs._fields_
  assert names == [f[0] for f in fields], (names, fields)
  for name, ctype in fields:
    is_array = issubclass(ctype, ctypes.Array)
    assert is_array == (name in arrays), name
    if is_array:
      assert ctype._length_ == levels
  kinds = dict(fields)
  assert kinds['mass_coef']._type_ is ctypes.c_double
  assert kinds['conv_coef']._type_ is ctypes.c_double
  assert kinds['num_elements'] is _lib.c_i64 and kinds['P'] is _lib.c_i32
  # 4 arrays of 3 eight-byte entries, 10 pointers, 2 int64, 5 int32 (+ pad)
  assert ctypes.sizeof(_lib.TransportArgs) == 4 * 24 + 10 * 8 + 16 + 24
  assert _lib.SIGNATURES['sfem_transport_rhs'][0]._type_ is _lib.TransportArgs


# ------------------------------------------------ the reference stepper
K3 = lambda x: 0.05 * (1.0 + 0.5 * x[..., 0] ** 2)


def _b3(x):
  return np.stack([1.0 + x[..., 1], 0.5 - x[..., 0],
                   0.3 + 0.0 * x[..., 0]], axis=-1)


@pytest.fixture(scope='module')
def problem3d():
  """Three-kinds mesh of 2^3 elements, P = 3, Dirichlet on x0 (with values),
  k = 0.05 (1 + x^2 / 2), b = (1 + y, 0.5 - x, 0.3), a nodal source."""
  P = 3
  rp = TR.box_with_sides(2, 3, P, three_kinds=True)
  x = np.asarray(rp.node_coords, np.float64)
  dvals = np.where(np.abs(x[:, 0]) < 1e-9, 1.0 + x[:, 1] ** 2, np.nan)
  prob = TR.Dense(rp, P, K3, dvals)
  uq = _b3(AR.quad_points(prob.fes))
  T0 = (1.0 + x[:, 1] ** 2) * np.cos(2.0 * x[:, 0]) + \
      np.sin(3.0 * x[:, 0]) * (x[:, 2] - 0.5)
  s = 1.0 + np.sin(2.0 * x[:, 1]) * x[:, 0]
  return prob, uq, T0, s


def test_reference_stepper_temporal_order(problem3d):
  """BDFk/EXTk against the exact semi-discrete solution at t = 0.2 with 20,
  40, 80 steps and an exact start-up: the observed order is within 0.15 of
  k."""
  prob, uq, T0, s = problem3d
  t_end = 0.2
  for order in (1, 2, 3):
    errs = []
    for steps in (20, 40, 80):
      dt = t_end / steps
      Ts = prob.exact(T0, uq, [j * dt for j in range(order)], s)
      for _ in range(steps - (order - 1)):
        Ts.append(prob.step(Ts, [uq] * order, dt, order, s))
        Ts = Ts[-order:]
      want = prob.exact(T0, uq, [t_end], s)[0]
      errs.append(np.abs(Ts[-1] - want).max() / np.abs(want).max())
    rates = [np.log2(errs[i] / errs[i + 1]) for i in range(2)]
    print(f'order {order}: errors {errs}, observed {rates}')
    for r in rates:
      assert abs(r - order) <= 0.15, (order, errs, rates)


def test_reference_step_keeps_steady_state(problem3d):
  """sum(bdf) = 0 and sum(ext) = 1: a step of any order from the steady state
  returns it to 2e-15 in the relative 2-norm (measured 0.5e-15..1.4e-15 over
  dt = 0.05..0.0025; the largest entry is off by 1.2e-15..3.7e-15 of
  max |T|, under 20 units in the last place after two dense solves)."""
  prob, uq, T0, s = problem3d
  Ts = prob.steady(uq, s)
  assert np.abs(prob.exact(Ts, uq, [0.3], s)[0] - Ts).max() <= 1e-12
  for order in (1, 2, 3):
    got = prob.step([Ts] * order, [uq] * order, 0.01, order, s)
    err = np.linalg.norm(got - Ts) / np.linalg.norm(Ts)
    print(f'order {order}: {err:.2e} (max norm '
          f'{np.abs(got - Ts).max() / np.abs(Ts).max():.2e})')
    assert err <= 2e-15
