"""The sum-factorised reference (`tests/sumfact_reference.py`) against the two
dense float64 references at the orders they reach, and on its own at 3D
P = 12 through properties of the continuous operator: symmetry, zero interior
rows on linear functions, exact volumes.  Two references are compared here,
no code under test."""
import functools

import numpy as np
import pytest

from tests import coefficient_reference as R
from tests import geometry_cases as G
from tests import sumfact_reference as S

# Two float64 evaluations of the same operator.  Measured on these meshes
# (curved elements included): <= 2.9e-14 against `coefficient_reference`
# (2D, P = 12) and <= 2.0e-14 against the oracle's forms, so the bound of
# 1e-12 stands as it is.
BOUND = 1e-12


def _rel(a, b):
  return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _boundary(x):
  """Nodes on the faces of the unit box (the meshes of `geometry_cases` move
  interior nodes only)."""
  return (np.minimum(x, 1.0 - x).min(axis=1) < 1e-12)


@functools.lru_cache(maxsize=None)
def _setup(ndim, P):
  rp = G.three_kinds(3, ndim, P).rp
  sf = S.Space(rp.node_coords, rp.elements, P)
  dense = R.space(rp.node_coords, rp.elements, P, (P, 'gll'))
  xq = sf.quad_points()
  k = 1.0 + xq[..., 0] ** 2 + 0.5 * np.sin(3.0 * xq[..., 0])
  c = 0.5 + xq[..., ndim - 1] ** 2
  return rp, sf, dense, k, c


CASES = [(2, 2), (2, 5), (2, 12), (3, 2), (3, 4), (3, 6)]


@pytest.mark.parametrize('ndim,P', CASES)
def test_matches_coefficient_reference(ndim, P):
  rp, sf, dense, k, c = _setup(ndim, P)
  assert _rel(sf.quad_points(), R.quad_points(dense)) <= 1e-14
  rng = np.random.default_rng(10 * ndim + P)
  u = rng.standard_normal(rp.node_coords.shape[0])
  keep = 1.0 - _boundary(rp.node_coords)
  assert 0 < keep.sum() < keep.size
  for l0, l1, kq, cq in ((0.0, 1.0, k, c), (0.7, 1.3, k, c),
                         (0.7, 1.3, None, c), (1.0, 0.0, k, c),
                         (0.6, 1.4, None, None)):
    err = _rel(sf.apply(u, l0, l1, kq, cq, keep),
               R.apply(dense, u, l0, l1, kq, cq, keep))
    assert err <= BOUND, (l0, l1, err)
    err = _rel(sf.diagonal(l0, l1, kq, cq, keep),
               R.diagonal(dense, l0, l1, kq, cq, keep))
    assert err <= BOUND, ('diagonal', l0, l1, err)
  ul = rng.standard_normal(rp.elements.shape)
  err = _rel(sf.local_apply(ul, 0.7, 1.3, k, c),
             R.local_apply(dense, ul, 0.7, 1.3, k, c))
  assert err <= BOUND, err


@pytest.mark.parametrize('ndim,P', CASES)
def test_matches_oracle_forms(ndim, P):
  rp, sf, dense, k, c = _setup(ndim, P)
  rng = np.random.default_rng(P)
  ul = rng.standard_normal(rp.elements.shape + (2,))
  for comp in (ul[..., 0], ul):
    err = _rel(sf.local_apply(comp, 1.0, 0.0), dense.mass_local(comp))
    assert err <= BOUND, ('mass', err)
    err = _rel(sf.local_apply(comp, 0.0, 1.0), dense.stiffness_local(comp))
    assert err <= BOUND, ('stiffness', err)
  # assembled, vector field, padded element and a padding slot ignored
  u = rng.standard_normal((rp.node_coords.shape[0], 2))
  want = dense.scatter(0.6 * dense.mass_local(dense.gather(u)) +
                       1.4 * dense.stiffness_local(dense.gather(u)))
  el = np.concatenate([rp.elements, np.full((1, rp.elements.shape[1]), -1)])
  padded = S.Space(rp.node_coords, el, P)
  assert _rel(padded.apply(u, 0.6, 1.4), want) <= BOUND
  assert _rel(padded.diagonal(0.6, 1.4), sf.diagonal(0.6, 1.4)) <= 1e-15


# ------------------------------------------- 3D, P = 12: properties only
@functools.lru_cache(maxsize=None)
def _high(name):
  rp = getattr(G, name)(3, 3, 12).rp
  return rp, S.Space(rp.node_coords, rp.elements, 12)


def _affine_map():
  """The map x -> A x + 0.1 of `geometry_cases.affine` (seed 0), restated."""
  rng = np.random.default_rng(0)
  return np.eye(3) + 0.3 * rng.uniform(-1, 1, (3, 3))


def test_symmetric_at_p12():
  rp, sf = _high('three_kinds')
  xq = sf.quad_points()
  k = 1.0 + xq[..., 1] ** 2
  c = 0.5 + np.sin(xq[..., 2]) ** 2
  rng = np.random.default_rng(12)
  u, v = rng.standard_normal((2, rp.node_coords.shape[0]))
  for l0, l1 in ((0.0, 1.0), (0.7, 1.3)):
    a = v @ sf.apply(u, l0, l1, k, c)
    b = u @ sf.apply(v, l0, l1, k, c)
    scale = np.abs(v * sf.apply(u, l0, l1, k, c)).sum()
    assert abs(a - b) <= 1e-13 * scale, (a, b)
  # positive: u . A u > 0, and A annihilates constants
  assert u @ sf.apply(u, 0.0, 1.0, k, c) > 0
  one = np.ones_like(u)
  flat = sf.apply(one, 0.0, 1.0, k, c)
  assert np.abs(flat).max() <= 1e-11 * np.abs(sf.apply(u, 0.0, 1.0, k, c)).max()


def test_linear_functions_at_p12():
  """On an all-affine mesh with k = 1 a linear u has a constant gradient g:
  the interior rows of A u vanish (integration by parts, exact quadrature)
  and u . A u = |g|^2 vol."""
  rp, sf = _high('affine')
  x = rp.node_coords
  g = np.array([0.3, -1.1, 0.7])
  u = x @ g + 0.2
  Au = sf.apply(u, 0.0, 1.0)
  A = _affine_map()
  s = np.linalg.solve(A, (x - 0.1).T).T           # back on the unit box
  interior = np.minimum(s, 1.0 - s).min(axis=1) > 1e-9
  assert 0 < interior.sum() < len(x)
  scale = np.abs(sf.local_apply(sf.gather(u), 0.0, 1.0)).max()
  assert np.abs(Au[interior]).max() <= 1e-11 * scale
  assert np.abs(Au[~interior]).max() > 1e-3 * scale
  vol = abs(np.linalg.det(A))
  assert abs(u @ Au - (g @ g) * vol) <= 1e-11 * (g @ g) * vol


def test_mass_sums_to_volumes_at_p12():
  rp, sf = _high('affine')
  one = np.ones(rp.elements.shape)
  per_elem = sf.local_apply(one, 1.0, 0.0).sum(axis=1)
  vol = abs(np.linalg.det(_affine_map())) / 27              # one element
  assert np.abs(per_elem - vol).max() <= 1e-13 * vol
  # multilinear elements: det J has degree 2 per direction, still exact; the
  # mesh fills the unit box
  rp, sf = _high('vertex')
  total = sf.apply(np.ones(rp.node_coords.shape[0]), 1.0, 0.0).sum()
  assert abs(total - 1.0) <= 1e-13
  # with a per-element reaction the sum weights the volumes
  c = np.arange(1.0, 28.0)
  got = sf.local_apply(np.ones(rp.elements.shape), 1.0, 0.0,
                       c_q=np.repeat(c[:, None], 12 ** 3, 1)).sum(axis=1)
  vols = sf.local_apply(np.ones(rp.elements.shape), 1.0, 0.0).sum(axis=1)
  assert np.abs(got - c * vols).max() <= 1e-14 * np.abs(got).max()
