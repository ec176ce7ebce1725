"""NumPy restatement of the boundary-facet quadrature (tests only).

Dense per-facet matrices from `core.interpolation` (whose 1D matrices are
pinned against the reference): B (x) B interpolates a facet's nodes to its
points, D_q (x) B and B (x) D_q give the tangents.  Also the boundary groups
of an order-1 premesh read off its element faces, for meshes (Gmsh files)
whose reader carries no physical groups.
"""
import functools

import numpy as np

from swirl_fem_amd.core import interpolation
from swirl_fem_amd.core.premesh import Premesh


def element_faces(elements: np.ndarray, ndim: int) -> np.ndarray:
  """(E, 2 ndim, 2^(ndim-1)) corner rows of the faces of order-1 elements,
  face 2a + s on side s of axis a, corners in lexicographic order."""
  corners = np.array(np.meshgrid(*([[0, 1]] * ndim), indexing='ij')).reshape(
      ndim, -1).T                                    # (2^d, d), lexicographic
  faces = []
  for a in range(ndim):
    for s in (0, 1):
      faces.append(np.nonzero(corners[:, a] == s)[0])
  return np.asarray(elements)[:, np.array(faces)]


def boundary_groups(pm: Premesh, classify) -> dict:
  """Unshared faces of the order-1 premesh `pm` that no periodic link joins,
  grouped by `classify(centroid (d,)) -> name` (None: no group)."""
  faces = element_faces(pm.elements, pm.ndim).reshape(
      -1, 2 ** (pm.ndim - 1))
  key = np.sort(faces, axis=1)
  _, inv, counts = np.unique(key, axis=0, return_inverse=True,
                             return_counts=True)
  outer = counts[inv.reshape(-1)] == 1
  if pm.periodic_links is not None:
    links = np.sort(np.asarray(pm.periodic_links).reshape(
        -1, 2 ** (pm.ndim - 1)), axis=1)
    linked = {tuple(r) for r in links}
    outer &= np.array([tuple(r) not in linked for r in key])
  groups = {}
  for f in faces[outer]:
    name = classify(np.asarray(pm.node_coords)[f].mean(axis=0))
    if name is not None:
      groups.setdefault(name, []).append(f)
  return {k: np.asarray(v, np.int32) for k, v in groups.items()}


def facet_matrices(gridpoints_1d, quadrature, k):
  """(B_k, [dB_k per facet axis], w_k) dense over a k-dim facet."""
  i1, d1 = interpolation.matrices_1d(gridpoints_1d, quadrature.nodes)
  i1 = np.asarray(i1)
  g1 = i1 @ np.asarray(d1)
  kron = lambda ms: functools.reduce(np.kron, ms)
  B = kron([i1] * k)
  dB = [kron([g1 if j == a else i1 for j in range(k)]) for a in range(k)]
  w = functools.reduce(np.outer, [quadrature.weights] * k).reshape(-1)
  return B, dB, w


def facet_quadrature(coords, facets, gridpoints_1d, quadrature):
  """(xq (F, Q^k, d), wJ (F, Q^k)) of facets (F, P^k) of a d-dim mesh."""
  coords = np.asarray(coords, np.float64)
  facets = np.asarray(facets)
  d = coords.shape[1]
  k = d - 1
  B, dB, w = facet_matrices(gridpoints_1d, quadrature, k)
  X = coords[facets]                                   # (F, P^k, d)
  xq = np.einsum('qi,fid->fqd', B, X)
  ts = [np.einsum('qi,fid->fqd', m, X) for m in dB]
  if k == 1:
    jac = np.linalg.norm(ts[0], axis=-1)
  else:
    jac = np.linalg.norm(np.cross(ts[0], ts[1]), axis=-1)
  return xq, w[None, :] * jac


def facet_normals(coords, facets, elements, gridpoints_1d, quadrature):
  """Unit outward normals (F, Q^k, d) at the facet points: the facet's normal
  pointing away from the centroid of the element that owns the facet."""
  coords = np.asarray(coords, np.float64)
  d = coords.shape[1]
  B, dB, _ = facet_matrices(gridpoints_1d, quadrature, d - 1)
  X = coords[np.asarray(facets)]
  ts = [np.einsum('qi,fid->fqd', m, X) for m in dB]
  if d == 2:
    n = np.stack([ts[0][..., 1], -ts[0][..., 0]], axis=-1)
  else:
    n = np.cross(ts[0], ts[1])
  n /= np.linalg.norm(n, axis=-1, keepdims=True)
  # the element holding every node of the facet
  elements = np.asarray(elements)
  owner = []
  for f in np.asarray(facets):
    hit = np.nonzero(np.isin(elements, f).sum(axis=1) == len(f))[0]
    owner.append(hit[0])
  cen = coords[elements[np.array(owner)]].mean(axis=1)       # (F, d)
  xq = np.einsum('qi,fid->fqd', B, X)
  sign = np.sign(np.einsum('fqd,fqd->fq', xq - cen[:, None, :], n))
  return n * sign[..., None]


def exchange(u, node_indices):
  """QQ^T on nodal values: the sum over every periodic class."""
  u = np.asarray(u, np.float64)
  node_indices = np.asarray(node_indices)
  sums = np.zeros(len(u))
  np.add.at(sums, node_indices, u)
  return sums[node_indices]


def covector(coords, facets, gridpoints_1d, quadrature, g, node_indices=None,
             nodal=False):
  """Assembled (N,) int g phi_i over the facets; g (F, Q^k) at the points or
  (N,) nodal (`nodal`)."""
  coords = np.asarray(coords, np.float64)
  facets = np.asarray(facets)
  B, _, _ = facet_matrices(gridpoints_1d, quadrature, coords.shape[1] - 1)
  _, wj = facet_quadrature(coords, facets, gridpoints_1d, quadrature)
  gq = np.einsum('qi,fi->fq', B, np.asarray(g)[facets]) if nodal else g
  local = np.einsum('qi,fq->fi', B, wj * gq)
  out = np.zeros(len(coords))
  np.add.at(out, facets.reshape(-1), local.reshape(-1))
  if node_indices is not None:
    out = exchange(out, node_indices)
  return out
