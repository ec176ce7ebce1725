"""Variable coefficients without a GPU: argument validation of
`operators.coefficient`, the p-multigrid coarse-level rule against its NumPy
restatement, the stored-factor folding, the byte model and the refusals."""
import numpy as np
import pytest
import torch

from swirl_fem_amd import _lib
from swirl_fem_amd.core import operators
from swirl_fem_amd.linalg import pmg
from tests import coefficient_reference as R

E, Q, D = 5, 8, 3


def _points():
  g = torch.Generator().manual_seed(0)
  return torch.rand((E, Q, D), generator=g, dtype=torch.float64)


def _coef(value, name='diffusivity'):
  return operators.coefficient(value, name, E, Q, _points, torch.float64,
                               'cpu')


def test_forms_normalise():
  assert _coef(None) is None
  assert _coef(2) == 2.0 and isinstance(_coef(2), float)
  mode, t = _coef(torch.full((E,), 3.0))
  assert mode == _lib.COEF_ELEM and tuple(t.shape) == (E,)
  mode, t = _coef(np.ones((E, Q)))
  assert mode == _lib.COEF_POINT and tuple(t.shape) == (E, Q)
  mode, t = _coef(lambda x: 1.0 + x[:, 2])
  assert mode == _lib.COEF_POINT
  np.testing.assert_allclose(t.numpy(), 1.0 + _points()[..., 2].numpy())
  assert _coef(0.0, 'reaction') == 0.0


@pytest.mark.parametrize('value', [
    np.ones(E + 1), np.ones((E, Q + 1)), np.ones((E, Q, 1)),
    lambda x: torch.ones(3), 'abc'])
def test_bad_shapes(value):
  with pytest.raises(ValueError):
    _coef(value)


@pytest.mark.parametrize('value', [
    0.0, -1.0, float('nan'), float('inf'), np.array([1, 1, 0, 1, 1.]),
    np.full((E, Q), np.nan), lambda x: -x[:, 0]])
def test_diffusivity_must_be_positive_and_finite(value):
  with pytest.raises(ValueError):
    _coef(value)


@pytest.mark.parametrize('value', [-1e-3, float('nan'),
                                   np.array([1, 1, -1, 1, 1.])])
def test_reaction_must_be_nonnegative_and_finite(value):
  with pytest.raises(ValueError):
    _coef(value, 'reaction')


def test_coarse_rule_matches_numpy():
  rng = np.random.default_rng(1)
  w = rng.random((E, Q)) + 0.1
  k = rng.random((E, Q)) + 0.5
  got = pmg.coarse_coefficient((_lib.COEF_POINT, torch.as_tensor(k)),
                               torch.as_tensor(w))
  np.testing.assert_allclose(got.numpy(), R.coarse_coefficient(k, w),
                             rtol=1e-15)
  ke = torch.as_tensor(rng.random(E))
  assert pmg.coarse_coefficient((_lib.COEF_ELEM, ke), None) is ke
  assert pmg.coarse_coefficient(2.5, None) == 2.5
  assert pmg.coarse_coefficient(None, None) is None
  # a constant per-point coefficient stays that constant
  c = pmg.coarse_coefficient((_lib.COEF_POINT, torch.full((E, Q), 7.0,
                                                          dtype=torch.float64)),
                             torch.as_tensor(w))
  np.testing.assert_allclose(c.numpy(), 7.0, rtol=1e-15)


@pytest.mark.parametrize('ndim', [2, 3])
def test_fold_point_factors(ndim):
  """k scales the G planes, c the W plane of the stored factor layout."""
  rng = np.random.default_rng(ndim)
  ng = ndim * (ndim + 1) // 2
  S = 4
  geo = torch.as_tensor(rng.random((S, ng + 1, Q)))
  kp = torch.as_tensor(rng.random((S, Q)) + 1)
  cp = torch.as_tensor(rng.random((S, Q)) + 1)
  out = operators._fold_point_factors(geo, ndim, kp, cp)
  flat, res = geo.reshape(S, -1).numpy(), out.reshape(S, -1).numpy()
  if ndim == 3:
    g = flat[:, :6 * Q].reshape(S, 3, Q, 2)
    np.testing.assert_allclose(res[:, :6 * Q].reshape(S, 3, Q, 2),
                               g * kp.numpy()[:, None, :, None])
    np.testing.assert_allclose(res[:, 6 * Q:], flat[:, 6 * Q:] * cp.numpy())
  else:
    p = flat.reshape(S, 2, Q, 2)
    r = res.reshape(S, 2, Q, 2)
    np.testing.assert_allclose(r[:, 0], p[:, 0] * kp.numpy()[..., None])
    np.testing.assert_allclose(r[:, 1, :, 0], p[:, 1, :, 0] * kp.numpy())
    np.testing.assert_allclose(r[:, 1, :, 1], p[:, 1, :, 1] * cp.numpy())
  # the input stays untouched (the space's factors are shared)
  assert not torch.equal(out, geo)


def test_byte_model():
  part = {'geo_mode': 1, 'coef_mode': _lib.COEF_ELEM,
          'kappa': torch.ones(E), 'sigma': torch.ones(E)}
  assert operators._coefficient_bytes(part, 8, 512, 0.0) == 8
  assert operators._coefficient_bytes(part, 8, 512, 1.0) == 16
  part = dict(part, coef_mode=_lib.COEF_POINT, sigma=None)
  assert operators._coefficient_bytes(part, 8, 512, 1.0) == 8 * 512
  assert operators._coefficient_bytes({'geo_mode': 0}, 8, 512, 1.0) == 0
  # 64^3 elements, p = 7, fp64: a per-point coefficient is 1.07 GB per apply
  assert 64 ** 3 * operators._coefficient_bytes(
      dict(part, sigma=None), 8, 512, 0.0) == 262144 * 512 * 8


def test_scalars_fold_into_lambdas():
  assert operators._scaled(None, 0.5, 2.0) == (0.5, 2.0)
  assert operators._scaled((3.0, 0.25), 0.5, 2.0) == (0.125, 6.0)
  arr = (_lib.COEF_ELEM, torch.ones(E))
  assert operators._scaled((arr, 4.0), 0.5, 2.0) == (2.0, 2.0)


def test_refusals():
  class _Mesh:
    axis_name = None
    neighbor_plan = None
  with pytest.raises(NotImplementedError):
    operators._check_coefficient_mesh(_Mesh(), 'cluster')
  part = _Mesh()
  part.neighbor_plan = object()
  with pytest.raises(NotImplementedError):
    operators._check_coefficient_mesh(part, 'atomic')
  with pytest.raises(NotImplementedError):
    operators._check_scalar_field(torch.zeros((4, 3)))
  operators._check_scalar_field(torch.zeros((4, 1)))


def test_abi_mirrors_the_header():
  import os
  import re
  header = open(os.path.join(os.path.dirname(os.path.dirname(
      os.path.abspath(__file__))), 'include', 'sfem.h')).read()
  for struct, cls in (('sfem_helmholtz_args', _lib.HelmholtzArgs),
                      ('sfem_diag_args', _lib.DiagArgs)):
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (struct, struct),
                     header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = re.findall(r'(\w+)\s*(?:,\s*\w+\s*)*;', body)
    fields = [f[0] for f in cls._fields_]
    assert fields[-3:] == ['kappa', 'sigma', 'coef_mode']
    assert names[-3:] == ['kappa', 'sigma', 'coef_mode']
