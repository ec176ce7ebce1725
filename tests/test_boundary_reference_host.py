"""`tests/boundary_reference.py` against second formulations, so that the GPU
tests of the boundary facet kernels (`tests/test_gpu_boundary_kernels.py`)
can trust it: the dense facet quadrature of `tests/bvp_reference.py` and the
dense Robin matrices of `tests/robin_reference.py` on real meshes, plain loops
for `add_rows`, and a list of deliberate mistakes that the synthetic inputs of
the sweep must tell from the right answer.  No GPU."""
import numpy as np
import pytest

from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
from swirl_fem_amd.core import interpolation
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType, Quadrature1D
from swirl_fem_amd.core.mesh_refiner import refine_premesh
from tests import boundary_reference as R
from tests import bvp_reference, robin_reference
from tests.fp32util import tolerance

GLL, GL = NodeType.GAUSS_LOBATTO_LEGENDRE, NodeType.GAUSS_LEGENDRE


# --------------------------------------------------------------- real mesh
def _jittered_box(ndim, P, seed=0):
  """(coords, facets of every side, gridpoints_1d) of a 2^d box whose inner
  order-1 node is moved."""
  pm = unit_cube_mesh(2, ndim=ndim)

  def side(c):
    for a in range(ndim):
      if abs(c[a]) < 1e-9 or abs(c[a] - 1) < 1e-9:
        return 'side'
    return None
  pm = pm.replace(physical_groups=bvp_reference.boundary_groups(pm, side))
  rng = np.random.default_rng(seed)
  x = pm.node_coords.copy()
  # every node moves, the outer ones too: facets that are not flat
  x += 0.1 * rng.uniform(-1, 1, x.shape)
  rp = refine_premesh(pm.replace(node_coords=x), Nodes1D.create(P + 1, GLL))
  mesh = rp.finalize(device='cpu')
  facets = mesh.boundary_facets['side'].numpy().astype(np.int32)
  return np.asarray(rp.node_coords, np.float64), facets, mesh.gridpoints_1d


def _rule(name, P, ndim):
  if name == 'gll':
    return Quadrature1D.create(P + 1, GLL)
  return Quadrature1D.create(P + (ndim + 1) // 2, GL)


def _matrices(grid, quad):
  i1, d1 = interpolation.matrices_1d(grid, quad.nodes)
  i1 = np.asarray(i1)
  return i1, i1 @ np.asarray(d1), np.asarray(quad.weights)


def _close(got, want, tol=1e-13):
  err = R.relerr(got, want)
  assert err <= tol, err


@pytest.mark.parametrize('rule', ['gll', 'gauss'])
@pytest.mark.parametrize('ndim,P', [(2, 3), (3, 2)])
def test_reference_on_a_real_mesh(ndim, P, rule):
  coords, facets, grid = _jittered_box(ndim, P, seed=P)
  quad = _rule(rule, P, ndim)
  B, Dq, w = _matrices(grid, quad)
  N, F = len(coords), len(facets)
  assert F == 2 * ndim * 2 ** (ndim - 1)
  rng = np.random.default_rng(ndim + P)
  # geom
  xq, wJ = R.geom(coords, facets, B, Dq, w)
  rx, rw = bvp_reference.facet_quadrature(coords, facets, grid, quad)
  _close(xq, rx)
  _close(wJ, rw)
  # covector, nodal and at points
  for nodal, g in ((True, rng.standard_normal(N)),
                   (False, rng.standard_normal(rw.shape))):
    local = R.covector_local(g, nodal, facets, wJ, B)
    assert local.shape == facets.shape
    got = np.zeros(N)
    np.add.at(got, facets.reshape(-1), local.reshape(-1))
    _close(got, bvp_reference.covector(coords, facets, grid, quad, g,
                                       nodal=nodal))
  # facet mass, with and without Dirichlet slots
  alpha = rng.uniform(0.5, 1.5, rw.shape)
  mats = robin_reference.facet_mass(coords, facets, grid, quad, alpha)
  u = rng.standard_normal(N)
  dirichlet = rng.uniform(size=N) < 0.3
  dirichlet[facets[0, 0]] = True
  scale = -1.7
  for dir_ in (None, dirichlet):
    enc = facets if dir_ is None else np.where(dir_[facets], ~facets, facets)
    A = robin_reference.assemble(mats, facets, N, dir_)
    for diag, want in ((False, scale * (A @ u)), (True, scale * np.diag(A))):
      local = R.mass_local(u, enc, alpha * wJ, B, scale, diag)
      if dir_ is not None:
        assert np.all(local[dir_[facets]] == 0)
      got = np.zeros(N)
      np.add.at(got, facets.reshape(-1), local.reshape(-1))
      _close(got, want)


def test_kronecker_layout():
  """The first Kronecker factor sits on the slow index, as
  `bvp_reference.facet_matrices`: `interp` against `np.kron` with two
  different matrices' worth of asymmetry (non-square B)."""
  rng = np.random.default_rng(0)
  B = rng.standard_normal((4, 3))
  v = rng.standard_normal((2, 9))
  _close(R.interp(B, v, 2), v @ np.kron(B, B).T)
  _close(R.interp(B.T, R.interp(B, v, 2), 2),
         v @ np.kron(B, B).T @ np.kron(B, B))
  _close(R.interp(B, v[:, :3], 1), v[:, :3] @ B.T)
  # one axis at a time: e_i (x) e_j sits at i * 3 + j
  e = np.zeros((1, 9))
  e[0, 1 * 3 + 2] = 1.0
  _close(R.interp(B, e, 2), np.outer(B[:, 1], B[:, 2]).reshape(1, -1))
  _close(R.swap_axes(e, 3), np.eye(9)[[2 * 3 + 1]])


# ---------------------------------------------------------------- add_rows
@pytest.mark.parametrize('num_rows', [0, 1, 7, 257])
def test_add_rows(num_rows):
  local, rows, offsets, slots, out = R.add_rows_inputs(num_rows)
  got = R.add_rows(local, rows, offsets, slots, out)
  want = out.copy()
  counts = np.diff(offsets)
  np.add.at(want, np.repeat(rows, counts), local[slots])
  assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
  untouched = np.setdiff1d(np.arange(len(out)), rows[counts > 0])
  assert np.array_equal(got[untouched], out[untouched])
  assert out[0] == 1000.5                                # the input is kept
  # float32: every partial sum rounded, an explicit loop
  local, rows, offsets, slots, out = R.add_rows_inputs(num_rows, f32=True)
  got = R.add_rows(local, rows, offsets, slots, out, dtype=np.float32)
  assert got.dtype == np.float32
  want = [np.float32(v) for v in out]
  for r in range(num_rows):
    acc = np.float32(0)
    for s in range(offsets[r], offsets[r + 1]):
      acc = np.float32(acc + np.float32(local[slots[s]]))
    want[rows[r]] = np.float32(want[rows[r]] + acc)
  assert np.array_equal(got, np.asarray(want, np.float32))
  if num_rows > 1:                                       # rounding is seen
    wide = R.add_rows(local, rows, offsets, slots, out)
    assert not np.array_equal(got.astype(np.float64), wide)


# ---------------------------------------------------------- discrimination
DISCRIMINATION = [(2, 4, 4), (2, 4, 5), (2, 14, 14), (2, 5, 3),
                  (3, 4, 4), (3, 4, 5), (3, 14, 14), (3, 5, 3)]


def _gap(bad, want):
  return R.relerr(bad, want)


@pytest.mark.parametrize('ndim,p1,q', DISCRIMINATION)
def test_inputs_discriminate(ndim, p1, q):
  """Every deliberate mistake applied to the reference moves its result by
  1e-2 relative or more on the inputs of the sweep: B^T for B (square pairs),
  the facet axes exchanged on the way in (3D), D_q and B exchanged in `geom`,
  w[a] w[a] for w[a] w[c] (3D), the mask ignored on read or on write."""
  assert (p1, q) in R.PAIRS
  a = R.synthetic(ndim, p1, q)
  k = a['k']
  masked, enc = R.mask_nodes(a)
  assert (enc == -1).any() and (enc >= 0).any()
  want = R.evaluate(a, encoded=enc)
  gaps = {}

  def wrong(name, b, encoded=None, u=None, keys=None):
    bad = R.evaluate(b, encoded=enc if encoded is None else encoded, u=u)
    for key in keys or want:
      gaps[f'{name}: {key}'] = _gap(bad[key], want[key])

  if p1 == q:
    # both matrices read transposed (wJ of an edge depends on D_q alone)
    wrong('B^T', dict(a, B=a['B'].T, Dq=a['Dq'].T))
  if k == 2:
    sw = dict(a, facets=R.swap_axes(a['facets'], p1),
              wJ=R.swap_axes(a['wJ'], q), aw=R.swap_axes(a['aw'], q),
              g_points=R.swap_axes(a['g_points'], q))
    wrong('axes', sw, encoded=R.swap_axes(enc, p1))
    xq, jac = R.facet_jacobian(a['coords'], a['facets'], a['B'], a['Dq'])
    gaps['w[a] w[a]: geom.wJ'] = _gap(np.repeat(a['w'] ** 2, q)[None] * jac,
                                      want['geom.wJ'])
  # on a face the exchange turns (x_s, x_t) into (x_t, x_s) and |x_s x x_t|
  # is the same for any input: there the points show it, on an edge both do
  wrong('D_q for B', dict(a, B=a['Dq'], Dq=a['B']),
        keys=['geom.xq'] if k == 2 else ['geom.xq', 'geom.wJ'])
  # the mask ignored on read: masked nodes' values enter, the slots still
  # write 0; ignored on write: they read 0 and the slots get their values
  read = R.mass_local(a['u'], a['facets'], a['aw'], a['B'], a['scale'], False)
  gaps['mask on read: mass_apply'] = _gap(np.where(enc >= 0, read, 0.0),
                                          want['mass_apply'])
  for diag, key in ((False, 'mass_apply'), (True, 'mass_diag')):
    write = R.mass_local(np.where(masked, 0.0, a['u']), a['facets'], a['aw'],
                         a['B'], a['scale'], diag)
    gaps[f'mask on write: {key}'] = _gap(write, want[key])
  assert len(gaps) >= 5
  for name, gap in gaps.items():
    assert gap >= 1e-2, (name, gap)


# -------------------------------------------- the float32 allowance, sized
@pytest.mark.parametrize('ndim', [2, 3])
@pytest.mark.parametrize('p1,q', R.PAIRS)
def test_float32_reference_within_tolerance(ndim, p1, q):
  """On the float32-representable inputs of the sweep the reference evaluated
  in float32 stays within `fp32util.tolerance` of the float64 one for every
  pair, so the bound of the GPU sweep is not out of reach of float32
  arithmetic to begin with."""
  import torch
  a = R.synthetic(ndim, p1, q, f32=True)
  want = R.evaluate(a)
  got = R.evaluate(a, dtype=np.float32)
  tol = tolerance(torch.float32, p1)
  for key in want:
    assert got[key].dtype == np.float32, key
    err = R.relerr(got[key], want[key])
    assert err < tol, (key, err)


def test_synthetic_inputs():
  """What section a of the GPU file relies on."""
  for ndim, (p1, q) in [(2, (2, 1)), (3, (16, 16)), (3, (5, 6))]:
    a = R.synthetic(ndim, p1, q)
    nf = p1 ** (ndim - 1)
    assert a['N'] == 3 * 5 * nf + 7 and a['facets'].shape == (5, nf)
    assert a['facets'].dtype == np.int32
    assert a['facets'].min() == 0 and a['facets'].max() == a['N'] - 1
    assert not np.allclose(a['B'], a['Dq'])
    if p1 == q:
      assert np.abs(a['B'] - a['B'].T).max() > 0.1
    f = R.synthetic(ndim, p1, q, f32=True)
    for key in ('B', 'Dq', 'w', 'coords', 'wJ', 'aw', 'g_nodal', 'g_points',
                'u'):
      assert np.array_equal(f[key], f[key].astype(np.float32)), key
    assert f['scale'] == float(np.float32(-1.7))
