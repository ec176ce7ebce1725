"""Shared fixture: the same refined box under other global node numberings.

`refine_premesh` numbers vertices, then edge, face and element interiors, each
facet's nodes in one contiguous run; several fast paths of the fused
Helmholtz operator were written with that numbering in mind.  `Mesh.create`
takes any numbering, so the cases below rename the nodes of a refined box and
say which launch path each numbering is meant to reach:

* `refiner`: the identity.  Facet tables, layered assembly, chains (P <= 8).
* `lexicographic(axes)`: a global (i, j, k) order, `axes[0]` slowest.  Every
  facet is still an affine map of node ids, with strides of about M and M^2
  (M nodes per line): facet tables, layered assembly and chains as on the
  refiner numbering, but a facet's nodes span many `SFEM_LAYER_CHUNK` chunks.
* `reversed`: `N - 1 - id`.  Every stride negative (the 16-bit strides of the
  layered table sign-extend), the most shared nodes last: the layers grow to
  about N.  Facet tables, layered assembly, chains.
  `reversed_lexicographic`: the same on the lexicographic numbering (negative
  strides of about M and M^2).
* `far_stride`: lexicographic on a thin box (`thin_box`) whose slowest global
  axis is an element's third local axis with >= 182 nodes on each other axis:
  a stride of 182^2 >= 32768 does not fit the layered table.  Facet tables
  and chains, no layer plan.
* `random`: a full random permutation.  No element is 27 affine facet maps:
  every element stays on its index row (no facet launches, no layer plan).
* `half_random`: the element-interior nodes of every second element shuffled
  among themselves.  Those elements keep their index rows, the others run
  from facet tables; the launches mix both, so there is no layer plan.

Stokes pairs (`build_pair`): the velocity mesh (P Gauss-Lobatto-Legendre
points) and the pressure mesh (P - 2 Gauss-Legendre points) of ONE premesh,
the velocity under any numbering above, the pressure under one of its own
(`PRESSURE_NUMBERINGS`).  The refiner numbers the element-interior pressure
nodes `e * np + k`, which the Stokes kernels address without an index row;
every other pressure numbering gives `elements != arange` and so the
index-row (`penc`) branch of those kernels and of the Schwarz local solve.
`stokes_spaces` / `stokes_sem` build the device objects from a pair.

Lexicographic orders come from the rounded coordinates of the UNDEFORMED
refined box; the builders of `tests/geometry_cases.py` then deform it (they
move coordinates only, so the refiner's numbering is the same).
"""
import dataclasses

import numpy as np

from swirl_fem_amd.common.premesh_commons import box_mesh, unit_cube_mesh
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType, Quadrature1D
from swirl_fem_amd.core.mesh_refiner import refine_premesh
from tests import geometry_cases as G

# what each numbering reaches: (facet launches, layer plan)
EXPECT = {'refiner': ('all', True), 'lexicographic': ('all', True),
          'reversed': ('all', True), 'far_stride': ('all', False),
          'random': ('none', False), 'half_random': ('some', False)}


def renumber(rp, perm):
  """`rp` with node `perm[i]` renamed to `i`: (premesh, perm).  Elements,
  physical groups and periodic links go through the inverse permutation,
  node coordinates are reordered."""
  perm = np.asarray(perm, dtype=np.int64)
  N = rp.node_coords.shape[0]
  assert perm.shape == (N,) and np.array_equal(np.sort(perm), np.arange(N))
  inv = np.empty(N, dtype=np.int64)
  inv[perm] = np.arange(N)

  def remap(a):
    a = np.asarray(a)
    return np.where(a >= 0, inv[np.maximum(a, 0)], a).astype(a.dtype)

  links = rp.periodic_links
  return rp.replace(
      node_coords=np.ascontiguousarray(rp.node_coords[perm]),
      elements=remap(rp.elements),
      physical_groups={k: remap(v) for k, v in rp.physical_groups.items()},
      periodic_links=None if links is None else remap(links)), perm


def grid_index(rp):
  """(N, d) integer line index of every node of an undeformed box."""
  x = np.round(np.asarray(rp.node_coords, np.float64), 9)
  return np.stack([np.unique(x[:, d], return_inverse=True)[1].reshape(-1)
                   for d in range(x.shape[1])], axis=1)


def lexicographic(rp, axes=None):
  """Global (i, j, k) order of the undeformed box `rp`, `axes[0]` slowest
  (default: axis 0; in 2D an axis list of three keeps its first two that
  exist, so `(1, 2, 0)` is `(1, 0)` there)."""
  idx = grid_index(rp)
  d = idx.shape[1]
  axes = tuple(range(d)) if axes is None else tuple(a for a in axes if a < d)
  return np.lexsort(tuple(idx[:, a] for a in axes[::-1]))


def reversed_ids(rp, rng=None):
  return np.arange(rp.node_coords.shape[0])[::-1].copy()


def reversed_lexicographic(rp, rng=None):
  return lexicographic(rp)[::-1].copy()


def far_stride(rp, rng=None):
  """Lexicographic with global axis 2 slowest (a thin box: `thin_box`)."""
  return lexicographic(rp, (2, 0, 1))


def random_ids(rp, rng):
  return rng.permutation(rp.node_coords.shape[0])


def half_random(rp, rng):
  """Element-interior nodes of every second element shuffled in place."""
  el = np.asarray(rp.elements)
  P = rp.gridpoints_1d.num_points
  d = rp.node_coords.shape[1]
  perm = np.arange(rp.node_coords.shape[0])
  for e in range(0, el.shape[0], 2):
    ids = el[e].reshape((P,) * d)[(slice(1, -1),) * d].reshape(-1)
    perm[ids] = ids[rng.permutation(ids.size)]
  return perm


NUMBERINGS = {'refiner': lambda rp, rng: np.arange(rp.node_coords.shape[0]),
              'lexicographic': lambda rp, rng: lexicographic(rp),
              'lexicographic_yzx': lambda rp, rng: lexicographic(rp, (1, 2, 0)),
              'reversed': reversed_ids,
              'reversed_lexicographic': reversed_lexicographic,
              'far_stride': far_stride,
              'random': random_ids, 'half_random': half_random}


def kind(numbering):
  """The `EXPECT` key of a numbering name."""
  for k in ('lexicographic', 'reversed'):
    if numbering.startswith(k):
      return k
  return numbering


def thin_box(P):
  """A box of one element in x2 and >= 182 nodes per line in x0 and x1,
  stretched per axis (every element a box)."""
  m = -(-181 // (P - 1))
  pm = box_mesh((m, m, 1), (0.0, 0.0, 0.0), (1.0, 1.3, 0.05))
  return G._refine(pm, P)


@dataclasses.dataclass
class Numbered:
  name: str
  rp: object         # renumbered refined premesh (deformed)
  base: object       # the same mesh in the refiner's numbering
  perm: np.ndarray   # node i of `rp` is node perm[i] of `base`
  numbering: str

  def to_base(self, v):
    """Nodal values on `rp` -> the same values in the refiner numbering."""
    out = np.empty_like(v)
    out[self.perm] = v
    return out

  def from_base(self, v):
    return np.asarray(v)[self.perm]


def build(numbering, geometry, n, P, seed=0, ndim=3):
  """`geometry`: a cube builder of `tests/geometry_cases.py` by name
  ('affine', 'multilinear', 'vertex', 'three_kinds', 'affine_curved', ...)
  on n^ndim elements, or 'thin' (`thin_box`, n ignored, 3D).  `far_stride`
  and 'thin' are 3D only."""
  rng = np.random.default_rng(seed)
  if geometry == 'thin':
    assert ndim == 3
    base = plain = thin_box(P)
  else:
    base = getattr(G, geometry)(n, ndim, P).rp
    plain = G._refine(unit_cube_mesh(n, ndim=ndim), P)
    assert np.array_equal(plain.elements, base.elements), geometry
  perm = NUMBERINGS[numbering](plain, rng)
  rp, perm = renumber(base, perm)
  return Numbered(f'{numbering}-{geometry}', rp, base, perm, numbering)


# ------------------------------------------------------------- Stokes pairs
GLL, GL = NodeType.GAUSS_LOBATTO_LEGENDRE, NodeType.GAUSS_LEGENDRE


def _p_identity(E, npe, rng):
  return np.arange(E * npe)


def _p_reversed(E, npe, rng):
  return np.arange(E * npe)[::-1].copy()


def _p_random(E, npe, rng):
  return rng.permutation(E * npe)


def _p_block_shuffled(E, npe, rng):
  """Element e's nodes stay one contiguous run, at the offset of element
  `(e + 1) % E` (no element keeps its own): new id = ((e + 1) % E) np + k."""
  base = np.arange(E * npe).reshape(E, npe)
  perm = np.empty(E * npe, dtype=np.int64)
  perm[np.roll(base, -1, axis=0).reshape(-1)] = base.reshape(-1)
  return perm


def _p_interleaved(E, npe, rng):
  """new id = k E + e: stride E inside an element."""
  return np.arange(E * npe).reshape(E, npe).T.reshape(-1).copy()


# perm[new id] = refiner id (= e np + k), as for `renumber`
PRESSURE_NUMBERINGS = {'identity': _p_identity, 'reversed': _p_reversed,
                       'random': _p_random,
                       'block_shuffled': _p_block_shuffled,
                       'interleaved': _p_interleaved}

# premesh builders of the Stokes pairs: name -> (n, ndim) -> (premesh, bend)
def _unit(n, ndim, periodic=()):
  return unit_cube_mesh(n, ndim=ndim, periodic_dims=periodic)


def _moved_vertex(pm, n):
  """The interior vertex nearest (2/3, 1/2, ...) moved: its 2^d elements
  become multilinear, none of them in the first layer x0 < 1/n (n >= 3)."""
  x = pm.node_coords.copy()
  target = np.full(x.shape[1], 0.5)
  target[0] = 2.0 / 3.0
  x[np.argmin(((x - target) ** 2).sum(-1))] += 0.1 / n
  return pm.replace(node_coords=x)


def bend_first_layer(rp, n):
  """Curves the elements of the first layer (x0 < 1/n) of a refined box whose
  first-layer elements are axis-aligned boxes: the last coordinate moves by
  0.3 / n * s (1 - s) t (1 - t), s = n x0 and t = frac(n x1) the elements'
  reference coordinates.  The displacement is of degree 2 per reference
  direction, so a velocity mesh of P >= 3 points and a pressure mesh of
  P - 2 >= 3 points hold the SAME geometry exactly (what the fused Stokes
  kernels require of a pair); it vanishes on the elements' x0- and x1-faces,
  so the mesh stays conforming."""
  x = np.asarray(rp.node_coords, np.float64).copy()
  s = n * x[:, 0]
  t = n * x[:, 1] - np.floor(np.minimum(n * x[:, 1], n - 1e-9))
  first = s <= 1.0 + 1e-9
  x[:, -1] += np.where(first, 0.3 / n * s * (1 - s) * t * (1 - t), 0.0)
  return rp.replace(node_coords=x)


def plain_premesh(geometry, n, ndim):
  """The undeformed box a geometry of `pair_premesh` deforms (same elements,
  distinct grid lines): where the lexicographic orders are read from."""
  if geometry == 'box':
    return box_mesh((n,) * ndim, (0.0,) * ndim, (1.0, 1.3, 0.7)[:ndim])
  periodic = {'periodic': (0,), 'periodic_box': tuple(range(ndim))}.get(
      geometry, ())
  return _unit(n, ndim, periodic)


def pair_premesh(geometry, n, ndim, seed=0):
  """(order-1 premesh, whether the refined meshes are bent) of a Stokes
  geometry: 'box' (axis-aligned, unequal edges: box kernels), 'affine'
  (sheared), 'multilinear' (every vertex jittered), 'vertex' (affine +
  multilinear), 'three_kinds' / 'affine_curved' (with curved elements,
  P >= 5), 'periodic' (x0 periodic, one vertex moved), 'periodic_box' (all
  directions periodic, uniform), 'walled_box' (uniform unit box)."""
  rng = np.random.default_rng(seed)
  if geometry == 'box':
    return plain_premesh(geometry, n, ndim), False
  if geometry == 'walled_box':
    return _unit(n, ndim), False
  if geometry == 'periodic_box':
    return _unit(n, ndim, tuple(range(ndim))), False
  if geometry == 'affine':
    pm = _unit(n, ndim)
    A = np.eye(ndim) + 0.3 * rng.uniform(-1, 1, (ndim, ndim))
    return pm.replace(node_coords=pm.node_coords @ A.T + 0.1), False
  if geometry == 'multilinear':
    pm = _unit(n, ndim)
    return pm.replace(node_coords=pm.node_coords + 0.1 / n * rng.uniform(
        -1, 1, pm.node_coords.shape)), False
  if geometry == 'vertex':
    return _moved_vertex(_unit(n, ndim), n), False
  if geometry == 'three_kinds':
    assert n >= 3
    return _moved_vertex(_unit(n, ndim), n), True
  if geometry == 'affine_curved':
    return _unit(n, ndim), True
  if geometry == 'periodic':
    return _moved_vertex(_unit(n, ndim, (0,)), n), False
  raise ValueError(geometry)


@dataclasses.dataclass
class Pair:
  name: str
  v: Numbered        # velocity mesh, P GLL points
  p: Numbered        # pressure mesh, P - 2 GL points
  P: int
  vnum: str
  pnum: str
  geometry: str


def build_pair(vnum, pnum, geometry, n, P, ndim=3, seed=0, premesh=None,
               f32=False):
  """The velocity / pressure pair of one premesh under the numberings `vnum`
  (`NUMBERINGS`) and `pnum` (`PRESSURE_NUMBERINGS`), chosen independently.
  `premesh`: an order-1 premesh of a box-like grid instead of a named
  geometry (its lexicographic orders come from its own coordinates, so it
  must not be deformed beyond what keeps grid lines distinct).  `f32`: node
  coordinates rounded to float32 (both numberings of both meshes alike)."""
  from tests.fp32util import f32r
  rng = np.random.default_rng(seed)
  if premesh is None:
    pm, bend = pair_premesh(geometry, n, ndim, seed)
    plain_pm = plain_premesh(geometry, n, ndim)
  else:
    pm, bend, plain_pm = premesh, False, premesh
  gv, gp = Nodes1D.create(P, GLL), Nodes1D.create(P - 2, GL)
  vbase, pbase = refine_premesh(pm, gv), refine_premesh(pm, gp)
  if bend:
    assert P >= 5, 'a curved pair needs P - 2 >= 3 pressure points'
    vbase, pbase = bend_first_layer(vbase, n), bend_first_layer(pbase, n)
  if f32:
    vbase = vbase.replace(node_coords=f32r(vbase.node_coords))
    pbase = pbase.replace(node_coords=f32r(pbase.node_coords))
  plain = refine_premesh(plain_pm, gv)
  assert np.array_equal(plain.elements, vbase.elements), geometry
  vrp, vperm = renumber(vbase, NUMBERINGS[vnum](plain, rng))
  E, npe = pbase.elements.shape
  assert np.array_equal(pbase.elements, np.arange(E * npe).reshape(E, npe))
  prp, pperm = renumber(pbase, PRESSURE_NUMBERINGS[pnum](E, npe, rng))
  name = f'{vnum}-{pnum}-{geometry}'
  return Pair(name, Numbered(name, vrp, vbase, vperm, vnum),
              Numbered(name, prp, pbase, pperm, pnum), P, vnum, pnum, geometry)


def stokes_spaces(pair, device, dtype=None):
  """(velocity space, pressure space) on the renumbered meshes of a pair."""
  from swirl_fem_amd.core.fespace import FiniteElementSpace
  quad = Quadrature1D.create(pair.P, GLL)
  vsp = FiniteElementSpace.create(
      pair.v.rp.finalize(device=device, dtype=dtype), quad)
  psp = FiniteElementSpace.create(
      pair.p.rp.finalize(device=device, dtype=dtype), quad)
  return vsp, psp


def stokes_sem(pair, boundary_conditions, device, dtype=None, base=False):
  """`StokesSEM` on the renumbered meshes of a pair (`base`: on the refiner's
  numbering of the same meshes)."""
  from swirl_fem_amd.navier_stokes.navier_stokes import StokesSEM
  v, p = (pair.v.base, pair.p.base) if base else (pair.v.rp, pair.p.rp)
  return StokesSEM.from_meshes(v.finalize(device=device, dtype=dtype),
                               p.finalize(device=device, dtype=dtype),
                               boundary_conditions)


def oracle_spaces(vrp, prp, P):
  """The oracle's velocity and pressure spaces on two refined premeshes."""
  from oracle import sfem_oracle as O
  return (O.FESpace(vrp.node_coords, vrp.elements, (P, 'gll'), (P, 'gll')),
          O.FESpace(prp.node_coords, prp.elements, (P - 2, 'gl'), (P, 'gll')))


def stokes_oracle(vrp, prp, P, dirichlet=None):
  """`StokesOracle` on two refined premeshes (`dirichlet`: name of the
  physical group with homogeneous Dirichlet rows, or None)."""
  from oracle import sfem_oracle as O
  v, p = vrp.finalize_all(), prp.finalize_all()
  mask = (np.zeros(len(v['node_coords']), bool) if dirichlet is None
          else v['physical_masks'][dirichlet])
  return O.StokesOracle(v, p, P - 1, mask)
