"""Shared fixture: small hex meshes that mix the geometry kinds of the fused
Helmholtz operator (`core/operators.py:classify_geometry`: affine elements,
multilinear images of the reference cube, curved elements with stored
factors).  Each launch group of an operator holds one kind, so these meshes
exercise the order of the launches across groups, which single-kind meshes
cannot.

Every builder returns a `Case`: the refined premesh, the geometry counts that
fp64 `geometry='auto'` must find (`check_counts`), and how many all -1
element rows to append (partition-style padding).  `numpy_kinds` restates
the classification from the corner coordinates for host-only tests.
"""
import dataclasses

import numpy as np

from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType
from swirl_fem_amd.core.mesh_refiner import refine_premesh
from tests.fp32util import f32_mesh

CURVED, AFFINE, MULTILINEAR = 0, 1, 3       # operators._GEO_* codes
KIND_ATTR = {CURVED: 'num_curved', AFFINE: 'num_affine',
             MULTILINEAR: 'num_multilinear'}


@dataclasses.dataclass
class Case:
  name: str
  rp: object              # refined premesh (oracle: rp.node_coords, elements)
  counts: dict            # kind -> element count, 'some' = > 0, absent = 0
  pad: int = 0            # trailing all -1 element rows

  def finalize(self, device, dtype):
    """(mesh, boundary mask or None, premesh the oracle must use)."""
    import torch
    from swirl_fem_amd.core.mesh import Mesh
    rp = f32_mesh(self.rp, dtype)
    mesh = rp.finalize(device=device, dtype=dtype)
    bm = mesh.physical_masks.get('boundary')
    if self.pad:
      n = rp.elements.shape[1]
      el = np.concatenate([rp.elements, np.full((self.pad, n), -1, np.int32)])
      mesh = Mesh.create(rp.node_coords, el, gridpoints_1d=rp.gridpoints_1d,
                         physical_masks=None if bm is None else
                         {'boundary': bm}, device=device, dtype=dtype)
      assert mesh.num_elements == rp.elements.shape[0] + self.pad
    if bm is not None:
      bm = bm.to(torch.bool)
    return mesh, bm, rp

  def check_counts(self, op):
    """The fp64 'auto' operator split the elements as this case expects."""
    real = self.rp.elements.shape[0]
    got = {k: getattr(op, a) for k, a in KIND_ATTR.items()}
    assert sum(got.values()) == real + self.pad, (self.name, got)
    for k, v in got.items():
      want = self.counts.get(k, 0)
      if want == 'some':
        assert v > 0, (self.name, got)
      elif self.pad:
        # padded rows (no slot ever written) join one of the groups
        assert v in (want, want + self.pad), (self.name, got)
      else:
        assert v == want, (self.name, got)

  @property
  def mixed(self):
    return sum(1 for v in self.counts.values() if v) > 1


def _refine(pm, P):
  return refine_premesh(pm, Nodes1D.create(P, NodeType.GAUSS_LOBATTO_LEGENDRE))


def _move_centre_vertex(x, n):
  """One interior vertex moved: its 2^d elements become multilinear."""
  x = x.copy()
  centre = np.argmin(((x - 0.5) ** 2).sum(-1))
  x[centre] += 0.1 / n
  return x


def _bend_first_layer(rp, n):
  """Curve the high-order nodes of the first layer of elements (x0 < 1/n)."""
  xc = rp.node_coords.copy()
  ndim = xc.shape[1]
  bump = 0.03 * np.sin(np.pi * xc[:, 0]) * np.sin(2 * np.pi * xc[:, 1])
  bump = bump * (xc[:, 0] < 1.0 / n + 1e-9)
  xc[:, -1] += bump * np.prod(xc * (1 - xc), axis=1) * 4 ** ndim
  return rp.replace(node_coords=xc)


def affine(n, ndim, P, seed=0):
  """Every element affine: an affine map of the whole box."""
  rng = np.random.default_rng(seed)
  pm = unit_cube_mesh(n, ndim=ndim)
  A = np.eye(ndim) + 0.3 * rng.uniform(-1, 1, (ndim, ndim))
  rp = _refine(pm.replace(node_coords=pm.node_coords @ A.T + 0.1), P)
  return Case('affine', rp, {AFFINE: n ** ndim})


def multilinear(n, ndim, P, seed=0):
  """Every element multilinear: every vertex jittered at random."""
  rng = np.random.default_rng(seed)
  pm = unit_cube_mesh(n, ndim=ndim)
  x = pm.node_coords + 0.1 / n * rng.uniform(-1, 1, pm.node_coords.shape)
  return Case('multilinear', _refine(pm.replace(node_coords=x), P),
              {MULTILINEAR: n ** ndim})


def vertex(n, ndim, P):
  """Affine + multilinear: one interior vertex moved (n >= 3: some elements
  stay affine)."""
  pm = unit_cube_mesh(n, ndim=ndim)
  rp = _refine(pm.replace(node_coords=_move_centre_vertex(pm.node_coords, n)),
               P)
  return Case('vertex', rp, {AFFINE: n ** ndim - 2 ** ndim,
                             MULTILINEAR: 2 ** ndim})


def block_jitter(n, ndim, P, scramble=False, seed=0):
  """Affine + multilinear: the smooth jitter of
  `distributed.blocks.build_block_partition(..., jitter=0.1)` on a single
  block.  It vanishes on the box boundary and, per direction, wherever a
  coordinate is 1/4 or 3/4, so some elements stay affine."""
  from swirl_fem_amd.distributed import blocks
  part = blocks.build_block_partition(n, P, (1,) * ndim, 0, device='cpu',
                                      jitter=0.1)
  pm = part.premesh
  name = 'block_jitter'
  if scramble:
    rng = np.random.default_rng(seed)
    pm = pm.replace(elements=pm.elements[rng.permutation(pm.num_elements)])
    name = 'scrambled'
  return Case(name, _refine(pm, P), {AFFINE: 'some', MULTILINEAR: 'some'})


def curved_multilinear(n, ndim, P, seed=0):
  """Multilinear + curved: jittered vertices, first layer of elements bent."""
  case = multilinear(n, ndim, P, seed)
  rp = _bend_first_layer(case.rp, n)
  return Case('curved_multilinear', rp, {MULTILINEAR: 'some', CURVED: 'some'})


def affine_curved(n, ndim, P):
  """Affine + curved: the uniform box with its first layer of elements bent
  (at P >= 9 the facet kernels keep multilinear elements on index rows, so
  this is the mix that layered assembly takes there)."""
  rp = _bend_first_layer(_refine(unit_cube_mesh(n, ndim=ndim), P), n)
  return Case('affine_curved', rp, {AFFINE: 'some', CURVED: 'some'})


def three_kinds(n, ndim, P, pad=0):
  """Affine + multilinear + curved (n >= 3): one interior vertex moved, the
  first layer of elements bent."""
  pm = unit_cube_mesh(n, ndim=ndim)
  rp = _refine(pm.replace(node_coords=_move_centre_vertex(pm.node_coords, n)),
               P)
  rp = _bend_first_layer(rp, n)
  return Case('three_kinds' + ('_padded' if pad else ''), rp,
              {AFFINE: 'some', MULTILINEAR: 'some', CURVED: 'some'}, pad)


def periodic(n, ndim, P):
  """Affine + multilinear on a box periodic in x0 (images are separate nodes
  joined by the exchange indices; the operator does not exchange)."""
  pm = unit_cube_mesh(n, ndim=ndim, periodic_dims=(0,))
  x = pm.node_coords.copy()
  centre = np.argmin(((x - 0.5) ** 2).sum(-1))
  x[centre] += 0.1 / n
  rp = _refine(pm.replace(node_coords=x), P)
  return Case('periodic', rp, {AFFINE: n ** ndim - 2 ** ndim,
                               MULTILINEAR: 2 ** ndim})


# ------------------------------------------------ host restatement (NumPy)
def numpy_kinds(coords, elements, ndim, P):
  """Geometry kind per element from its corner vertices alone, with the
  grouping rule of `classify_geometry` (a few affine elements among
  multilinear ones join the multilinear group).  Valid for meshes whose
  high-order nodes are the multilinear interpolant of the corners (no
  curved elements): affine iff the bilinear / trilinear coefficients of the
  corner map vanish.  Padded rows (all -1) are reported as -1."""
  el = np.asarray(elements)
  E = el.shape[0]
  idx = np.arange(P ** ndim).reshape((P,) * ndim)
  corner = idx[(slice(0, P, P - 1),) * ndim].reshape(-1)   # lexicographic
  kinds = np.full(E, -1, np.int64)
  real = (el >= 0).any(axis=1)
  xc = np.asarray(coords, np.float64)[el[real][:, corner]]  # (E', 2^d, d)
  size = np.abs(xc - xc[:, :1]).max(axis=(1, 2))
  # corner t has bits (b_0 .. b_{d-1}), b_0 the most significant: the affine
  # map through corners 0 and 2^(d-1-a) predicts every corner
  bits = (np.arange(2 ** ndim)[:, None] >> np.arange(ndim)[::-1]) & 1
  edges = xc[:, [2 ** (ndim - 1 - a) for a in range(ndim)]] - xc[:, :1]
  pred = xc[:, :1] + np.einsum('ta,ead->etd', bits.astype(np.float64), edges)
  aff = np.abs(xc - pred).max(axis=(1, 2)) <= 1e-11 * size
  k = np.full(len(xc), MULTILINEAR)
  n_aff, n_multi = int(aff.sum()), len(xc)
  if n_aff >= 0.02 * max(n_multi, 1) or n_aff == n_multi:
    k[aff] = AFFINE
  kinds[real] = k
  return kinds
