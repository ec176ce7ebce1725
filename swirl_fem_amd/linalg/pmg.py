"""p-multigrid preconditioning of the fused Helmholtz / Poisson solves.

`PMultigridPreconditioner(op, lambda0, lambda1)` is one V-cycle over a
hierarchy of polynomial orders on the same elements (default p -> p // 2 ->
... -> 1), with Chebyshev-Jacobi smoothing on every level but the coarsest and
a fixed Chebyshev polynomial of the assembled order-1 matrix there -- the
standard preconditioner of matrix-free spectral-element Poisson solvers
(nekRS, deal.II, libCEED).  The V-cycle is a fixed linear operator: symmetric
and positive definite, so plain PCG takes it as it is.

Hierarchy (setup):
* a coarse `Mesh` per order, derived from the fine `Mesh` alone.  A coarse
  node is keyed by the fine nodes around it: per direction the two fine
  points next to it (`_bracket`), over the directions in which it lies inside
  its element; a vertex by its fine vertex, an element-interior node by its
  element.  The same point seen from two elements gives the same fine nodes,
  so a coarse node is shared by exactly the elements that share that point on
  the fine mesh, periodic images included (they stay separate nodes, joined by
  the exchange indices as on the fine mesh);
* coarse geometry: the fine element map evaluated at the coarse GLL points,
  exact for affine and multilinear elements (the register-geometry kernels
  stay in use); a shared node takes the value of its lowest-numbered element;
* coarse Dirichlet mask: a coarse node is Dirichlet iff every fine node of the
  smallest closed element facet that contains it is;
* owner map: every fine node belongs to its lowest-numbered element, stored as
  one bit per local node (`sfem_pmg_prolong` writes through it).

Operators: the smoother of the finest level applies the operator CG solves
with; a collocated one through a coloured-assembly copy (on a partition the
operator itself, and default assembly on the coarse levels), a two-grid one
element-locally with a fixed-order sum (`sfem_scatter_csr`), so that every
sum in the V-cycle has a fixed order and the preconditioner is bitwise
reproducible.  Coarse levels are collocated GLL `HelmholtzOperator`s with the
same (lambda0, lambda1), coloured assembly.  Coloured assembly launches colour
by colour across the geometry kinds (`operators.colored_launch_order`): it was
once launched kind by kind, which on meshes mixing affine and multilinear
elements added some shared slots before their node's first store and left
the one-rank V-cycle about 24 % off the operator there.

`CGRunner` recognises the preconditioner through `stops_on_residual`: it then
stops on the true-residual norm r.r <= max(tol^2 b.b, atol^2) instead of the
reference's r.Mr (an energy norm when M ~ A^-1), with inner products summed in
a fixed order.

Robin terms (`boundary_terms`: `fespace.boundary_mass` operators with their
scales): the finest level adds them to its apply and diagonal.
A coarse level gets the same groups on its own nodes: each fine facet is
matched to its (element, local face) by its corner ids (`coarse_facets`), the
face's coarse nodes are taken from the coarse element rows, and the coarse
alpha wJ is the facet mean of the fine alpha, sum(alpha wJ) / sum(wJ), times
the coarse wJ.  The coarsest level's assembled matrix adds the facet matrices,
so its spectrum bounds see them.  Without the term a pure Robin problem with
lambda0 = 0 has singular coarse operators.

Block partitions (`distributed.blocks.build_block_partition`, world > 1): every
rank builds the hierarchy of its own block, and every vector of the V-cycle is
*consistent* (equal on all ranks that hold a node), as in the partitioned CG:
* each coarse mesh carries a coarse `NeighborPlan` derived from the fine one
  without communication (`coarse_plan`): a coarse node is shared with rank q
  iff all the fine nodes of its key are in the fine list for q, and the shared
  coarse nodes are ordered by the sorted positions of those fine nodes in that
  list -- the same on both sides;
* level operators are QQ^T A_local (the exchange after the local apply);
* restriction: every fine node also has one owning RANK, the lowest that holds
  it (`restrict_owner`), so the local restrictions summed by the coarse
  exchange are the global P^T r; prolongation writes every local fine node;
* Lanczos runs with global inner products from a start vector that is a
  function of the node coordinates, so every rank gets the same estimates;
* the coarsest level keeps its rank-local (unassembled) order-1 matrix and
  applies the polynomial of `sfem_ell_chebyshev` step by step: y = QQ^T A_loc x
  (`sfem_ell_spmv` on the interface rows, exchange posted, interior rows,
  exchange finished), then `sfem_cheb_step`.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from swirl_fem_amd import _ops
from swirl_fem_amd.core.interpolation import BarycentricInterpolator
from swirl_fem_amd.core.interpolation import Nodes1D
from swirl_fem_amd.core.interpolation import NodeType
from swirl_fem_amd.core.interpolation import Quadrature1D

# Chebyshev interval of the smoothers: [LOW lambda_hat, HIGH lambda_hat]
SMOOTHER_LOW = 0.1
SMOOTHER_HIGH = 1.1
LANCZOS_STEPS = 16          # estimate of lambda_max(D^-1 A) per level
COARSE_REDUCTION = 0.1      # the coarse polynomial's error bound (steps=None)
COARSE_MAX_STEPS = 256
# Lanczos on the partitioned coarse matrix: checked every COARSE_LANCZOS_CHECK
# steps, stopped when both extreme Ritz values move less than
# COARSE_LANCZOS_RTOL, at most COARSE_LANCZOS_MAX steps (see `_coarse_bounds`)
COARSE_LANCZOS_CHECK = 10
COARSE_LANCZOS_RTOL = 1e-3
COARSE_LANCZOS_MAX = 300


def default_orders(p: int) -> list:
  """p, p // 2, ..., 1."""
  orders = [int(p)]
  while orders[-1] > 1:
    orders.append(orders[-1] // 2)
  return orders


def _bracket(pc: int, pf: int):
  """Per coarse 1D index a: the fine indices floor / ceil of a pf / pc (the
  fine points around the coarse point, one of them when they coincide);
  symmetric: bracket(pc - a) = pf - bracket(a)."""
  a = np.arange(pc + 1)
  return (a * pf) // pc, -((-a * pf) // pc)


def _lex(shape):
  """(n, len(shape)) multi-indices in the mesh's lexicographic order (axis 0
  slowest)."""
  return np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing='ij'),
                  axis=-1).reshape(-1, len(shape))


def _flat(idx, P):
  """Local node number of multi-indices idx (..., d) on P points."""
  out = np.zeros(idx.shape[:-1], dtype=np.int64)
  for a in range(idx.shape[-1]):
    out = out * P + idx[..., a]
  return out


def _check_mesh(mesh):
  plan = mesh.neighbor_plan
  if plan is None and mesh.axis_name is not None:
    raise NotImplementedError(
        'p-multigrid on a partitioned mesh without a NeighborPlan (the coarse '
        'exchange is derived from the fine plan)')
  if plan is not None and mesh.axis_name is None:
    raise NotImplementedError(
        'p-multigrid on a partitioned mesh without an axis_name')
  if plan is not None and plan.has_local_images:
    raise NotImplementedError(
        'p-multigrid on a partitioned mesh whose plan has local periodic '
        'images (a direction that is periodic with a single block)')
  if mesh._cache.get('replicas', 1) > 1:
    raise NotImplementedError('p-multigrid on an ensemble (Mesh.replicate)')
  if mesh.ndim not in (2, 3):
    raise NotImplementedError(f'p-multigrid needs ndim 2 or 3, got {mesh.ndim}')
  if mesh.gridpoints_1d.node_type != NodeType.GAUSS_LOBATTO_LEGENDRE:
    raise NotImplementedError('p-multigrid needs a GLL mesh')
  if bool((mesh.elements < 0).any()):
    raise NotImplementedError('p-multigrid on padded (partitioned) elements')


def coarse_numbering(elements: np.ndarray, reps: np.ndarray | None, ndim: int,
                     pf: int, pc: int):
  """Coarse element index rows (E, (pc + 1)^d) from the fine ones (E,
  (pf + 1)^d), orders pf > pc >= 1, and the coarse node classes (the lowest
  coarse id of every node's periodic class; None without `reps`, the fine
  node classes).  Returns (celems, creps, num_coarse_nodes)."""
  E = elements.shape[0]
  Pf, Pc = pf + 1, pc + 1
  lo, hi = _bracket(pc, pf)
  cloc = _lex((Pc,) * ndim)                                # (nc, d)
  inner = (cloc > 0) & (cloc < pc)
  k_of = inner.sum(axis=1)
  celems = np.empty((E, Pc ** ndim), dtype=np.int64)
  creps = np.empty((E, Pc ** ndim), dtype=np.int64) if reps is not None \
      else None
  start = 0
  for k in range(ndim + 1):
    sel = np.nonzero(k_of == k)[0]
    if not sel.size:
      continue
    if k == ndim:                  # element interiors: never shared
      ids = start + np.arange(E * sel.size).reshape(E, sel.size)
      celems[:, sel] = ids
      if creps is not None:
        creps[:, sel] = ids
      start += E * sel.size
      continue
    cols = _key_columns(sel, k, cloc, inner, lo, hi, ndim, Pf)
    keys = np.sort(elements[:, cols], axis=-1).reshape(-1, 2 ** k)
    ids, n_new = _number_rows(keys)
    celems[:, sel] = start + ids.reshape(E, sel.size)
    if creps is not None:
      rkeys = np.sort(reps[elements[:, cols]], axis=-1).reshape(-1, 2 ** k)
      rid, _ = _number_rows(rkeys)
      # the class representative: the lowest coarse id with the same key
      low = np.full(rid.max() + 1 if rid.size else 0, np.iinfo(np.int64).max)
      np.minimum.at(low, rid, ids)
      creps[:, sel] = start + low[rid].reshape(E, sel.size)
    start += n_new
  return celems, creps, start


def _key_columns(sel, k, cloc, inner, lo, hi, ndim, Pf):
  """(ns, 2^k) fine element-local columns of the key of every coarse local
  node in `sel` (k directions inside the element): the 2^k fine nodes around
  it."""
  combos = []
  for bits in range(2 ** k):
    f = np.empty((sel.size, ndim), dtype=np.int64)
    for j, s in enumerate(sel):
      axes = np.nonzero(inner[s])[0]
      for a in range(ndim):
        f[j, a] = (lo if a not in axes else
                   (hi if (bits >> list(axes).index(a)) & 1 else lo))[
                       cloc[s, a]]
    combos.append(_flat(f, Pf))
  return np.stack(combos, axis=-1)


def coarse_keys(elements, celems: np.ndarray, num_coarse: int, ndim: int,
                pf: int, pc: int) -> np.ndarray:
  """(num_coarse, 2^ndim) int64: the fine nodes of every coarse node's key
  (those of `coarse_numbering`, sorted, padded with -1; all -1 for element
  interiors, which no other element or rank shares)."""
  Pc = pc + 1
  lo, hi = _bracket(pc, pf)
  cloc = _lex((Pc,) * ndim)
  inner = (cloc > 0) & (cloc < pc)
  k_of = inner.sum(axis=1)
  out = np.full((num_coarse, 2 ** ndim), -1, dtype=np.int64)
  for k in range(ndim):
    sel = np.nonzero(k_of == k)[0]
    if not sel.size:
      continue
    cols = _key_columns(sel, k, cloc, inner, lo, hi, ndim, Pf=pf + 1)
    keys = np.sort(elements[:, cols], axis=-1)               # (E, ns, 2^k)
    out[celems[:, sel].reshape(-1), :2 ** k] = keys.reshape(-1, 2 ** k)
  return out


def coarse_plan(fine_plan, keys: np.ndarray):
  """The coarse `NeighborPlan` from the fine one, without communication.

  For neighbour q the fine list `indices[q]` numbers the fine nodes shared
  with q in an order both sides agree on.  A coarse node is shared with q iff
  every fine node of its key (`coarse_keys`) is in that list, and the shared
  coarse nodes are ordered by the sorted tuple of those list positions: the
  same fine nodes give the same tuple on both sides, so the same order."""
  from swirl_fem_amd.distributed import comm
  nf = max([int(np.max(ix)) + 1 for ix in fine_plan.indices if len(ix)] +
           [int(keys.max()) + 1 if keys.size else 0])
  valid = keys >= 0
  neighbors, indices = [], []
  for q, ix in zip(fine_plan.neighbors, fine_plan.indices):
    pos = np.full(nf, -1, dtype=np.int64)
    pos[np.asarray(ix, dtype=np.int64)] = np.arange(len(ix))
    kp = np.where(valid, pos[np.where(valid, keys, 0)], -1)
    shared = valid[:, 0] & ((kp >= 0) | ~valid).all(axis=1)
    nodes = np.nonzero(shared)[0]
    tup = np.sort(kp[nodes], axis=1)             # -1 padding sorts first
    order = np.lexsort(tup.T[::-1]) if nodes.size else nodes
    if nodes.size:
      neighbors.append(int(q))
      indices.append(nodes[order].astype(np.int32))
  return comm.NeighborPlan(rank=fine_plan.rank, neighbors=neighbors,
                           indices=indices)


def rank_owned(plan, num_nodes: int) -> np.ndarray:
  """(num_nodes,) bool: this rank owns the node for the restriction -- it is
  the lowest-numbered rank that holds it."""
  mine = np.ones(num_nodes, dtype=bool)
  for q, ix in zip(plan.neighbors, plan.indices):
    if q < plan.rank:
      mine[np.asarray(ix, dtype=np.int64)] = False
  return mine


def _number_rows(keys: np.ndarray):
  """Ids 0.. of the distinct rows of `keys` in order of first occurrence."""
  keys = np.ascontiguousarray(keys)
  view = keys.view(np.dtype((np.void, keys.dtype.itemsize * keys.shape[1])))
  _, first, inv = np.unique(view.reshape(-1), return_index=True,
                            return_inverse=True)
  rank = np.empty(first.size, dtype=np.int64)
  rank[np.argsort(first, kind='stable')] = np.arange(first.size)
  return rank[inv.reshape(-1)], first.size


def interpolation_1d(pc: int, pf: int) -> np.ndarray:
  """(pf + 1, pc + 1): the Lagrange basis of the coarse GLL points at the fine
  GLL points (prolongation along one direction)."""
  coarse = Nodes1D.create(pc + 1, NodeType.GAUSS_LOBATTO_LEGENDRE)
  fine = Nodes1D.create(pf + 1, NodeType.GAUSS_LOBATTO_LEGENDRE)
  return np.asarray(BarycentricInterpolator(
      ndim=1, gridpoints_1d=coarse,
      evalpoints_1d=fine)._interpolation_matrix_1d(), dtype=np.float64)


def _kron(m, ndim):
  out = m
  for _ in range(ndim - 1):
    out = np.kron(out, m)
  return out


def coarse_dirichlet(fine_dirichlet_local: torch.Tensor, ndim, pf, pc):
  """(E, (pc + 1)^d) bool: the facet rule on element-local fine masks
  (E, (pf + 1)^d)."""
  Pf, Pc = pf + 1, pc + 1
  cloc = _lex((Pc,) * ndim)
  out = torch.zeros((fine_dirichlet_local.shape[0], Pc ** ndim),
                    dtype=torch.bool, device=fine_dirichlet_local.device)
  # facet of a coarse node: per direction 0 (first), 2 (last) or 1 (inside)
  kind = np.where(cloc == 0, 0, np.where(cloc == pc, 2, 1))
  for sig in np.unique(kind, axis=0):
    ranges = [[0] if s == 0 else ([pf] if s == 2 else list(range(Pf)))
              for s in sig]
    fl = _flat(np.stack(np.meshgrid(*ranges, indexing='ij'), axis=-1).reshape(
        -1, ndim), Pf)
    facet = fine_dirichlet_local[:, torch.as_tensor(fl, device=out.device)]
    val = facet.all(dim=1)
    cols = np.nonzero((kind == sig).all(axis=1))[0]
    out[:, torch.as_tensor(cols, device=out.device)] = val[:, None]
  return out


def encode_rows(elements: torch.Tensor, dirichlet: torch.Tensor | None):
  """int32 index rows with Dirichlet nodes stored as ~id."""
  el = elements.to(torch.int32)
  if dirichlet is None:
    return el.contiguous()
  return torch.where(dirichlet[elements.to(torch.int64)], ~el, el).contiguous()


def owner_bits(elements: torch.Tensor, num_nodes: int,
               node_mask: torch.Tensor | None = None) -> torch.Tensor:
  """(E, ceil(n / 32)) int32 words (bit t of word t // 32: element e owns its
  local node t): every node is owned by the lowest-numbered element that
  contains it.  `node_mask` (num_nodes,) bool: nodes outside it have no owner
  at all (the restriction of a partition: nodes another rank owns)."""
  E, n = elements.shape
  el = elements.to(torch.int64)
  eidx = torch.arange(E, device=el.device)[:, None].expand(E, n)
  first = torch.full((num_nodes,), E, dtype=torch.int64, device=el.device)
  first.scatter_reduce_(0, el.reshape(-1), eidx.reshape(-1), reduce='amin')
  owned = first[el] == eidx
  if node_mask is not None:
    owned = owned & node_mask.to(el.device)[el]
  words = (n + 31) // 32
  pad = torch.zeros((E, words * 32), dtype=torch.int64, device=el.device)
  pad[:, :n] = owned.to(torch.int64)
  shift = torch.arange(32, device=el.device, dtype=torch.int64)
  w = (pad.view(E, words, 32) << shift).sum(dim=2)
  w = torch.where(w >= 2 ** 31, w - 2 ** 32, w)
  return w.to(torch.int32).contiguous()


def coarse_facets(fine_facets: np.ndarray, fine_corners: np.ndarray,
                  celems: np.ndarray, ndim: int, pf: int,
                  pc: int) -> np.ndarray:
  """(F, (pc + 1)^(d-1)) coarse node rows of the facets (F, (pf + 1)^(d-1))
  of the fine mesh: each fine facet is matched to the (element, local face)
  whose corners it has (`fine_corners` (E, 2^d): the fine ids of the element
  vertices in lexicographic order), and gets that face's coarse nodes from
  `celems` in the element's lexicographic face order (its orientation may
  differ from the fine facet's)."""
  k = ndim - 1
  fac = np.asarray(fine_facets, np.int64)
  fine_corners = np.asarray(fine_corners, np.int64)
  E = fine_corners.shape[0]
  cl = _lex((2,) * ndim)
  faces = np.stack([np.nonzero(cl[:, a] == s)[0] for a in range(ndim)
                    for s in (0, 1)])                       # (2d, 2^k)
  fkeys = np.sort(fine_corners[:, faces], axis=-1).reshape(-1, 2 ** k)
  qkeys = np.sort(fac[:, _flat(_lex((2,) * k) * pf, pf + 1)], axis=-1)
  ids, n_ids = _number_rows(np.concatenate([fkeys, qkeys]))
  pos = np.full(n_ids, -1, dtype=np.int64)
  pos[ids[:fkeys.shape[0]]] = np.arange(fkeys.shape[0])
  face = pos[ids[fkeys.shape[0]:]]
  if (face < 0).any():
    raise ValueError('a boundary facet is not a face of any element')
  e, fa = face // (2 * ndim), face % (2 * ndim)
  cel = np.asarray(celems).reshape((E,) + (pc + 1,) * ndim)
  out = np.empty((fac.shape[0], (pc + 1) ** k), dtype=np.int64)
  for t in range(2 * ndim):
    sel = np.nonzero(fa == t)[0]
    if sel.size:
      side = np.take(cel[e[sel]], 0 if t % 2 == 0 else pc, axis=1 + t // 2)
      out[sel] = side.reshape(sel.size, -1)
  return out


def coarse_mesh(mesh, pc: int):
  """(coarse Mesh of order pc, coarse element index rows (E, (pc+1)^d) int64
  device tensor) derived from `mesh` (order > pc)."""
  from swirl_fem_amd.core import gather_scatter
  from swirl_fem_amd.core.mesh import Mesh
  _check_mesh(mesh)
  d, pf = mesh.ndim, mesh.order
  if not 1 <= pc < pf:
    raise ValueError(f'coarse order {pc} must be in 1..{pf - 1}')
  dev = mesh.device
  plan = mesh.neighbor_plan
  # (on a partition the exchange indices are the plan's, not periodic images)
  periodic = (plan is None and mesh.exchange_gather_indices is not None and
              mesh.exchange_gather_indices.numel() > 0)
  # only the fine columns the keys need travel to the host
  Pf = pf + 1
  lo, hi = _bracket(pc, pf)
  need = np.unique(np.concatenate([
      _flat(_lex((2,) * d) * pf, Pf),
      _flat(np.stack(np.meshgrid(*([np.unique(np.concatenate([lo, hi]))] * d),
                                 indexing='ij'), -1).reshape(-1, d), Pf)]))
  sub = mesh.elements[:, torch.as_tensor(need, device=dev)].cpu().numpy()
  remap = np.full(Pf ** d, -1, dtype=np.int64)
  remap[need] = np.arange(need.size)
  # fine ids compressed to the columns in use: rebuild a (E, Pf^d) view lazily
  el_full = _ColumnView(sub.astype(np.int64), remap)
  reps = (mesh.node_indices.cpu().numpy().astype(np.int64) if periodic
          else None)
  celems, creps, nc = coarse_numbering(el_full, reps, d, pf, pc)
  celems_t = torch.as_tensor(celems, device=dev)
  # geometry: the fine element map at the coarse GLL points, evaluated in
  # fp64 and rounded once (an fp32 sum of p + 1 terms per direction would
  # move affine elements outside classify_geometry's tolerance)
  J = torch.as_tensor(_kron(interpolation_1d_geometry(pf, pc), d),
                      dtype=torch.float64, device=dev)       # (nc_loc, nf_loc)
  xe = mesh.node_coords.double()[mesh.elements.to(torch.int64)]  # (E, nf, d)
  xc_loc = torch.einsum('cf,efd->ecd', J, xe).to(mesh.dtype)
  E, ncl = celems.shape
  first = torch.full((nc,), E, dtype=torch.int64, device=dev)
  eidx = torch.arange(E, device=dev)[:, None].expand(E, ncl)
  first.scatter_reduce_(0, celems_t.reshape(-1), eidx.reshape(-1),
                        reduce='amin')
  mine = (first[celems_t] == eidx).reshape(-1)
  coords = torch.empty((nc, d), dtype=mesh.dtype, device=dev)
  coords[celems_t.reshape(-1)[mine]] = xc_loc.reshape(-1, d)[mine]
  kw = {}
  if periodic:
    node_indices = np.empty(nc, dtype=np.int64)
    node_indices[celems.reshape(-1)] = creps.reshape(-1)
    gi, ui = gather_scatter.get_exchange_indices(node_indices)
    kw = dict(node_indices=node_indices.astype(np.int32),
              exchange_gather_indices=gi, exchange_unique_indices=ui)
  if plan is not None:
    cplan = coarse_plan(plan, coarse_keys(el_full, celems, nc, d, pf, pc))
    kw = dict(axis_name=mesh.axis_name, neighbor_plan=cplan,
              exchange_gather_indices=(
                  np.concatenate(cplan.indices).astype(np.int32)
                  if cplan.indices else None))
  cmesh = Mesh.create(
      node_coords=coords, elements=celems.astype(np.int32),
      gridpoints_1d=Nodes1D.create(pc + 1, NodeType.GAUSS_LOBATTO_LEGENDRE),
      device=dev, dtype=mesh.dtype, **kw)
  return cmesh, celems_t


class _ColumnView:
  """`elements[:, cols]` of the fine index rows from the columns kept."""

  def __init__(self, sub, remap):
    self.sub, self.remap = sub, remap
    self.shape = (sub.shape[0], remap.size)

  def __getitem__(self, key):
    rows, cols = key
    assert rows == slice(None)
    return self.sub[:, self.remap[cols]]


def interpolation_1d_geometry(pf: int, pc: int) -> np.ndarray:
  """(pc + 1, pf + 1): the fine Lagrange basis at the coarse GLL points."""
  coarse = Nodes1D.create(pc + 1, NodeType.GAUSS_LOBATTO_LEGENDRE)
  fine = Nodes1D.create(pf + 1, NodeType.GAUSS_LOBATTO_LEGENDRE)
  return np.asarray(BarycentricInterpolator(
      ndim=1, gridpoints_1d=fine,
      evalpoints_1d=coarse)._interpolation_matrix_1d(), dtype=np.float64)


def _cheb_coefficients(lo, hi, degree):
  """[(a_k, c_k)]: d_k = a_k d_{k-1} + c_k D^-1 r_k, x += d_k (the Chebyshev
  iteration for the interval [lo, hi])."""
  theta, delta = 0.5 * (hi + lo), 0.5 * (hi - lo)
  sigma = theta / delta
  rho = 1.0 / sigma
  out = [(0.0, 1.0 / theta)]
  for _ in range(1, degree):
    rho_new = 1.0 / (2.0 * sigma - rho)
    out.append((rho_new * rho, 2.0 * rho_new / delta))
    rho = rho_new
  return out


def lanczos_max(apply_fn, dinv):
  """Largest eigenvalue of D^-1 A (rows with dinv > 0) from LANCZOS_STEPS
  steps of Lanczos on D^-1/2 A D^-1/2 from a fixed start vector, on one rank.
  `apply_fn(u, out)`: out = A u on vectors of `dinv`'s size and dtype."""
  sq = dinv.double().sqrt()
  n = sq.numel()
  g = torch.Generator().manual_seed(12345)
  v = torch.rand(n, generator=g, dtype=torch.float64).to(dinv.device) - 0.5
  v = v * (sq > 0)
  v = v / v.norm()
  v_prev = torch.zeros_like(v)
  alphas, betas = [], []
  beta = 0.0
  ax = torch.empty(n, dtype=dinv.dtype, device=dinv.device)
  for _ in range(min(LANCZOS_STEPS, int((sq > 0).sum()))):
    apply_fn((sq * v).to(dinv.dtype).contiguous(), ax)
    w = sq * ax.double()
    alpha = float(torch.dot(w, v))
    w = w - alpha * v - beta * v_prev
    alphas.append(alpha)
    beta = float(w.norm())
    if beta <= 1e-14 * abs(alpha):
      break
    betas.append(beta)
    v_prev, v = v, w / beta
  k = len(alphas)
  T = np.diag(alphas) + np.diag(betas[:k - 1], 1) + np.diag(betas[:k - 1], -1)
  return float(np.linalg.eigvalsh(T).max())


def jacobi_scaled_extremes(S, ndim):
  """(lmin, lmax) of the Jacobi-scaled coarse matrix S (scipy sparse,
  symmetric): exact for up to 400 rows, else a few Lanczos steps from either
  end (no factorisation of S; the coarse polynomial stays positive definite
  for any 0 < lmin)."""
  import scipy.sparse.linalg as spla
  if S.shape[0] <= 400:
    ev = np.linalg.eigvalsh(S.toarray())
    return float(ev[0]), float(ev[-1])
  lmax = float(spla.eigsh(S, k=1, which='LA', tol=1e-3,
                          return_eigenvectors=False)[0])
  try:
    lmin = float(spla.eigsh(S, k=1, which='SA', tol=1e-2,
                            maxiter=20 * S.shape[0],
                            return_eigenvectors=False)[0])
  except spla.ArpackNoConvergence as exc:
    got = np.sort(exc.eigenvalues)
    lmin = (float(got[0]) if got.size else
            lmax / (4.0 * S.shape[0] ** (2.0 / ndim)))
  return lmin, lmax


def coarse_coefficient(coef, weights):
  """A diffusivity / reaction coefficient of the fine operator as the coarse
  levels take it (the same elements on every level): None, a scalar or an
  (E,) tensor unchanged; per-point values (E, Q) become the per-element mean
  weighted by W = w detJ at those points, `weights` (E, Q):
  sum_q k_q W_q / sum_q W_q (as the facet mean of the Robin alpha in
  `_coarse_terms`).  `coef` in the normal form of `operators.coefficient`;
  returns what `helmholtz_operator` accepts."""
  from swirl_fem_amd import _lib
  if coef is None or isinstance(coef, float):
    return coef
  mode, t = coef
  if mode == _lib.COEF_ELEM:
    return t
  w = weights.to(torch.float64)
  mean = (t.to(torch.float64) * w).sum(dim=1) / w.sum(dim=1)
  return mean.to(t.dtype).contiguous()


class _Level:
  """Operator, smoother data and work vectors of one order."""

  def __init__(self, mesh, op, apply_fn, dirichlet, dinv):
    self.mesh, self.op, self.apply = mesh, op, apply_fn
    self.dirichlet = dirichlet            # (N,) bool or None
    self.dinv = dinv
    N, dt, dev = mesh.num_nodes, dinv.dtype, dinv.device
    self.x, self.d, self.ax, self.r, self.b = (
        torch.zeros(N, dtype=dt, device=dev) for _ in range(5))
    self.cheb = None
    self.lam_max = None
    self.boundary = []          # [(BoundaryMassOperator, scale)]
    # (diffusivity, reaction) of the coarser levels (`coarse_coefficient`)
    self.coefs = (None, None)
    # transfer from the next coarser level (set by the hierarchy)
    self.transfer = None


class PMultigridPreconditioner:
  """One V-cycle of p-multigrid for `lambda0 B + lambda1 A`.

  `op`: the `HelmholtzOperator` or `TwoGridHelmholtzOperator` CG solves with
  (GLL nodes, one partition, no ensemble).  `orders`: the order of every
  level, finest first (default p, p // 2, ..., 1).  `smoother_degree`:
  Chebyshev steps before and after the coarse correction on every level but
  the coarsest.  `coarse_steps`: degree of the coarsest level's polynomial
  (None: enough to reduce its error bound to COARSE_REDUCTION).

  M r: pre-smooth from x = 0, residual, restrict, recurse, prolong and add,
  post-smooth with the same polynomial; the coarsest level (order 1) applies
  a fixed Chebyshev polynomial of its Jacobi-scaled assembled matrix
  (`sfem_ell_chebyshev`, the spectrum bounds from Lanczos at setup).  No host
  synchronisation: `capturable`.  The result lives in a buffer of the
  preconditioner, valid until the next call.

  On a block partition (the mesh has a `neighbor_plan`; collocated GLL
  `HelmholtzOperator` only) M maps consistent vectors to consistent vectors
  (`consistent`) and is the V-cycle of the whole mesh; `group` is the process
  group of the exchanges and reductions.  Its exchanges go through the host
  transport: not `capturable`.

  `boundary_terms`: None, or [(BoundaryMassOperator, scale)]: Robin terms
  `scale * M` that the operator CG solves with adds to `op` (built with the
  same Dirichlet mask); every level carries them (one partition only).

  `bounds`: None, or the spectrum estimates to use instead of computing them,
  as `spectral_bounds()` returns them (e.g. from the preconditioner of the
  same problem on one rank): {'lam_max': one per smoothed level, 'coarse':
  (lmin, lmax) of the coarsest level's polynomial}.
  """

  capturable = True
  stops_on_residual = True
  consistent = True        # consistent vectors in, consistent vectors out

  def __init__(self, op, lambda0=0.0, lambda1=1.0, *, orders=None,
               smoother_degree=2, coarse_steps=None, bounds=None, group=None,
               boundary_terms=None):
    from swirl_fem_amd.core import operators
    if not isinstance(op, (operators.HelmholtzOperator,
                           operators.TwoGridHelmholtzOperator)):
      raise TypeError('PMultigridPreconditioner takes a HelmholtzOperator or '
                      f'a TwoGridHelmholtzOperator, got {type(op).__name__}')
    fes = op.fespace
    mesh = fes.mesh
    _check_mesh(mesh)
    self.plan, self.group = mesh.neighbor_plan, group
    self.boundary_terms = [(b, float(s)) for b, s in (boundary_terms or [])]
    if self.boundary_terms and self.plan is not None:
      raise NotImplementedError('p-multigrid with Robin terms on a '
                                'partitioned mesh')
    if self.plan is not None:
      if not isinstance(op, operators.HelmholtzOperator):
        raise NotImplementedError('p-multigrid on a partitioned mesh takes a '
                                  'collocated HelmholtzOperator')
      self.capturable = False
    p = mesh.order
    orders = default_orders(p) if orders is None else [int(o) for o in orders]
    if (orders[0] != p or orders[-1] != 1 or
        any(b >= a for a, b in zip(orders, orders[1:]))):
      raise ValueError(f'orders must fall strictly from {p} to 1; got {orders}')
    if smoother_degree < 1:
      raise ValueError('smoother_degree must be >= 1')
    self.lambda0, self.lambda1 = float(lambda0), float(lambda1)
    self.orders, self.degree = orders, int(smoother_degree)
    self.dtype, self.device = fes.dtype, fes.device
    keep = op.keep if isinstance(op, operators.HelmholtzOperator) else op.mask
    fine_dir = None if keep is None else (keep == 0)
    self.levels = [self._fine_level(op, fine_dir)]
    for i, pc in enumerate(orders[1:]):
      self.levels.append(self._coarse_level(self.levels[-1], pc,
                                            i == len(orders) - 2))
    if bounds is not None and len(bounds['lam_max']) != len(orders) - 1:
      raise ValueError(f"bounds: {len(bounds['lam_max'])} lam_max values for "
                       f'{len(orders) - 1} smoothed levels')
    for i, lev in enumerate(self.levels[:-1]):
      lev.lam_max = (float(bounds['lam_max'][i]) if bounds is not None
                     else self._lanczos_max(lev))
      lev.cheb = _cheb_coefficients(SMOOTHER_LOW * lev.lam_max,
                                    SMOOTHER_HIGH * lev.lam_max, self.degree)
    coarse = None if bounds is None else tuple(bounds['coarse'])
    if self.plan is None:
      self._coarse_setup(self.levels[-1], coarse_steps, coarse)
    else:
      self._coarse_setup_partitioned(self.levels[-1], coarse_steps, coarse)

  def spectral_bounds(self):
    """The spectrum estimates this preconditioner uses (the `bounds` argument
    that reproduces them)."""
    return {'lam_max': [lev.lam_max for lev in self.levels[:-1]],
            'coarse': tuple(self.coarse_bounds)}

  # ------------------------------------------------------------ partitions
  def _exchange_(self, u, mesh):
    """QQ^T in place (nothing without a partition)."""
    if mesh.neighbor_plan is None:
      return u
    from swirl_fem_amd.distributed import comm
    return comm.neighbor_exchange_(u, mesh.neighbor_plan, self.group)

  def _allreduce(self, t):
    from swirl_fem_amd.distributed import comm
    return comm.all_reduce_sum_(t, self.group)

  def _gdots(self, lev, pairs):
    """Global inner products of consistent fp64 vectors (one all-reduce):
    the local dot minus the interface terms weighted by 1 - 1/holders."""
    idx, w = lev.mesh.neighbor_plan.interface_weights(self.device)
    vals = torch.stack([torch.dot(a, b) - (w * a[idx] * b[idx]).sum()
                        for a, b in pairs])
    return self._allreduce(vals).tolist()

  def _start_vector(self, lev, mask):
    """A fixed pseudo-random vector (fp64, consistent): on a partition a
    hash of the node coordinates, so that every rank starts Lanczos from the
    restriction of one global vector; else the seeded generator of one rank."""
    n = lev.mesh.num_nodes
    if lev.mesh.neighbor_plan is None:
      g = torch.Generator().manual_seed(12345)
      v = torch.rand(n, generator=g, dtype=torch.float64).to(self.device) - 0.5
      return v * mask
    q = np.round(lev.mesh.node_coords.double().cpu().numpy() *
                 2.0 ** 20).astype(np.int64)
    h = np.zeros(n, dtype=np.uint64)
    for a, m in zip(range(q.shape[1]), (0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F,
                                         0x165667B19E3779F9)):
      h = (h ^ (q[:, a].astype(np.uint64) * np.uint64(m))) * np.uint64(
          0xFF51AFD7ED558CCD)
      h ^= h >> np.uint64(33)
    v = torch.as_tensor((h >> np.uint64(11)).astype(np.float64) / 2.0 ** 53 -
                        0.5, device=self.device) * mask
    # average the copies of shared nodes (equal unless coordinates computed
    # in different elements round differently)
    idx, w = lev.mesh.neighbor_plan.interface_weights(self.device)
    v[idx] = v[idx] * (1.0 - w)
    return self._exchange_(v, lev.mesh)

  def _lanczos(self, lev, apply_fn, sq, steps, check=None):
    """Ritz values of D^-1/2 A D^-1/2 (`apply_fn(u, out)` = A u, `sq` =
    D^-1/2, 0 on Dirichlet rows) after at most `steps` Lanczos steps with the
    global inner product; `check(k, ritz)` may end it early."""
    n = sq.numel()
    partitioned = lev.mesh.neighbor_plan is not None
    dot = ((lambda a, b: self._gdots(lev, [(a, b)])[0]) if partitioned
           else (lambda a, b: float(torch.dot(a, b))))
    v = self._start_vector(lev, (sq > 0).double())
    v = v / math.sqrt(dot(v, v))
    v_prev = torch.zeros_like(v)
    alphas, betas = [], []
    beta = 0.0
    ax = torch.empty(n, dtype=self.dtype, device=self.device)
    interior = int((sq > 0).sum())
    if partitioned:
      t = torch.tensor([float(interior)], dtype=torch.float64,
                       device=self.device)
      interior = int(self._allreduce(t).item())    # (an upper bound)
    for k in range(min(steps, interior)):
      apply_fn((sq * v).to(self.dtype).contiguous(), ax)
      w = sq * ax.double()
      alpha = dot(w, v)
      w = w - alpha * v - beta * v_prev
      alphas.append(alpha)
      beta = math.sqrt(max(dot(w, w), 0.0))
      if beta <= 1e-14 * abs(alpha):
        break
      betas.append(beta)
      v_prev, v = v, w / beta
      if check is not None and check(k + 1, alphas, betas):
        break
    k = len(alphas)
    T = np.diag(alphas) + np.diag(betas[:k - 1], 1) + np.diag(betas[:k - 1], -1)
    return np.linalg.eigvalsh(T)

  # ---------------------------------------------------------------- setup
  def _fine_level(self, op, dirichlet):
    from swirl_fem_amd.core import operators
    fes, mesh = op.fespace, op.fespace.mesh
    l0, l1 = self.lambda0, self.lambda1
    if isinstance(op, operators.HelmholtzOperator) and self.plan is not None:
      # a partition: the operator CG solves with (the exchange adds with
      # atomics, so the fixed-order coloured copy would buy nothing here)
      apply_fn = lambda u, out: self._exchange_(op.apply(u, l0, l1, out=out),
                                                mesh)
    elif isinstance(op, operators.HelmholtzOperator):
      k, c = op.coef_source
      colored = fes.helmholtz_operator(dirichlet, assembly='colored',
                                       diffusivity=k, reaction=c)
      self._fine_colored = colored
      apply_fn = lambda u, out: colored.apply(u, l0, l1, out=out)
    else:
      offsets, slots = mesh.assembly_plan().csr()

      def apply_fn(u, out):
        loc = op.apply_local(mesh.gather(u), l0, l1)
        return _ops.scatter_csr(loc.reshape(-1), offsets, slots,
                                mesh.num_nodes, out=out)
    diag = op.diagonal(l0, l1)
    if self.boundary_terms:
      base, terms = apply_fn, self.boundary_terms

      def apply_fn(u, out):
        base(u, out)
        for b, s in terms:
          b.apply(u, s, out=out)
        return out
      for b, s in terms:
        diag = diag + s * b.diagonal()
    lev = _Level(mesh, op, apply_fn, dirichlet, self._dinv(diag))
    lev.boundary = self.boundary_terms
    if op.coefs is not None:
      k, c = op.coefs
      w = (op.point_weights() if any(
          operators._point_coefficient(x) for x in op.coefs) else None)
      lev.coefs = (coarse_coefficient(k, w), coarse_coefficient(c, w))
    return lev

  def _dinv(self, d):
    interior = d != 0
    if bool((d[interior] < 0).any()):
      raise ValueError('the diagonal has negative entries: the operator is '
                       'not positive definite')
    return torch.where(interior, 1.0 / torch.where(interior, d,
                                                   torch.ones_like(d)),
                       torch.zeros_like(d)).contiguous()

  def _coarse_level(self, fine, pc, coarsest):
    from swirl_fem_amd.core.fespace import FiniteElementSpace
    fmesh = fine.mesh
    d, pf = fmesh.ndim, fmesh.order
    cmesh, celems = coarse_mesh(fmesh, pc)
    fel = fmesh.elements.to(torch.int64)
    if fine.dirichlet is not None:
      cdir_loc = coarse_dirichlet(fine.dirichlet[fel], d, pf, pc)
      cdir = torch.zeros(cmesh.num_nodes, dtype=torch.bool,
                         device=self.device)
      cdir[celems.reshape(-1)] = cdir_loc.reshape(-1)
    else:
      cdir = None
    fes = FiniteElementSpace.create(
        cmesh, Quadrature1D.create(pc + 1, NodeType.GAUSS_LOBATTO_LEGENDRE))
    l0, l1 = self.lambda0, self.lambda1
    # (the coarsest level only assembles its element matrices)
    k, c = fine.coefs
    cop = fes.helmholtz_operator(cdir, assembly='auto' if (
        coarsest or self.plan is not None) else 'colored', diffusivity=k,
        reaction=c)
    cterms = self._coarse_terms(fine, fes, celems, cdir)
    diag = cop.diagonal(l0, l1)
    if cterms:
      def apply_fn(u, out):
        cop.apply(u, l0, l1, out=out)
        for b, s in cterms:
          b.apply(u, s, out=out)
        return out
      for b, s in cterms:
        diag = diag + s * b.diagonal()
    else:
      apply_fn = lambda u, out: self._exchange_(cop.apply(u, l0, l1, out=out),
                                                cmesh)
    lev = _Level(cmesh, cop, apply_fn, cdir, self._dinv(diag))
    lev.boundary = cterms
    lev.coefs = fine.coefs
    lev.fespace = fes
    offsets, slots = cmesh.assembly_plan().csr()
    owner = owner_bits(fel, fmesh.num_nodes)
    rowner = owner
    if fmesh.neighbor_plan is not None:
      rowner = owner_bits(fel, fmesh.num_nodes, torch.as_tensor(
          rank_owned(fmesh.neighbor_plan, fmesh.num_nodes)))
    fine.transfer = dict(
        cidx=encode_rows(celems, cdir), fidx=encode_rows(fel, fine.dirichlet),
        owner=owner, restrict_owner=rowner,
        mat=torch.as_tensor(interpolation_1d(pc, pf), dtype=self.dtype,
                            device=self.device).contiguous(),
        local=torch.zeros(celems.numel(), dtype=self.dtype,
                          device=self.device),
        offsets=offsets, slots=slots, pc=pc + 1, pf=pf + 1)
    return lev

  def _coarse_terms(self, fine, fes, celems, cdir):
    """The Robin terms of the fine level on the coarse space `fes`."""
    from swirl_fem_amd.core.fespace import BoundaryMassOperator
    if not fine.boundary:
      return []
    fmesh, cmesh = fine.mesh, fes.mesh
    d, pf, pc = fmesh.ndim, fmesh.order, cmesh.order
    corners = torch.as_tensor(_flat(_lex((2,) * d) * pf, pf + 1),
                              device=self.device)
    fcorners = fmesh.elements[:, corners].cpu().numpy()
    chost = celems.cpu().numpy()
    i1, g1 = fes._matrices()
    w = torch.as_tensor(fes.quadrature.weights, dtype=self.dtype,
                        device=self.device)
    out = []
    for b, s in fine.boundary:
      cf = coarse_facets(b.facets.cpu().numpy(), fcorners, chost, d, pf, pc)
      cf = torch.as_tensor(cf, dtype=torch.int32, device=self.device)
      _, wj = _ops.boundary_geom(cmesh.node_coords.contiguous(), cf, i1, g1, w)
      den = b.wj.double().sum(dim=1)
      mean = torch.where(den > 0, b.aw.double().sum(dim=1) /
                         torch.where(den > 0, den, torch.ones_like(den)),
                         torch.zeros_like(den))
      aw = (mean[:, None].to(self.dtype) * wj).contiguous()
      out.append((BoundaryMassOperator(fes, cf, wj, aw, cdir), s))
    return out

  def _lanczos_max(self, lev):
    """Largest eigenvalue of D^-1 A (interior rows) from LANCZOS_STEPS steps
    of Lanczos on D^-1/2 A D^-1/2 from a fixed start vector."""
    if lev.mesh.neighbor_plan is not None:
      sq = lev.dinv.double().sqrt()
      return float(self._lanczos(lev, lev.apply, sq, LANCZOS_STEPS).max())
    return lanczos_max(lev.apply, lev.dinv)

  def _local_matrix(self, lev):
    """The order-1 matrix of this rank's elements (CSR, fp64; Dirichlet rows
    and columns zero).  On a partition its interface rows are this rank's
    share only."""
    import scipy.sparse as sp
    mesh = lev.mesh
    E, n = mesh.elements.shape
    N = mesh.num_nodes
    l0, l1 = self.lambda0, self.lambda1
    cols_k = []
    for j in range(n):
      u = torch.zeros((E, n), dtype=self.dtype, device=self.device)
      u[:, j] = 1.0
      cols_k.append(lev.op.apply_local(u, l0, l1).double().cpu().numpy())
    K = np.stack(cols_k, axis=-1)                    # (E, n_i, n_j)
    el = mesh.elements.cpu().numpy().astype(np.int64)
    rows = np.repeat(el[:, :, None], n, axis=2).reshape(-1)
    cols = np.repeat(el[:, None, :], n, axis=1).reshape(-1)
    A = sp.csr_matrix((K.reshape(-1), (rows, cols)), shape=(N, N))
    for b, s in lev.boundary:          # Robin facet matrices
      Kf = s * b.local_matrices().double().cpu().numpy()
      fr = b.facets.cpu().numpy().astype(np.int64)
      nf = fr.shape[1]
      A = A + sp.csr_matrix((Kf.reshape(-1), (
          np.repeat(fr[:, :, None], nf, axis=2).reshape(-1),
          np.repeat(fr[:, None, :], nf, axis=1).reshape(-1))), shape=(N, N))
    A = A.tocsr()
    A.sum_duplicates()
    # periodic images: the fine operator keeps them apart, so does this one
    if lev.dirichlet is not None:
      keep = (~lev.dirichlet).cpu().numpy().astype(np.float64)
      A = (sp.diags(keep) @ A @ sp.diags(keep)).tocsr()
      A.eliminate_zeros()
    return A

  def _store_ell(self, lev, A, dinv):
    """ELL form of A (column-major) and the coarse work vectors."""
    N = A.shape[0]
    width = int(np.diff(A.indptr).max()) if A.nnz else 1
    ecols = np.repeat(np.arange(N)[:, None], width, axis=1)
    evals = np.zeros((N, width))
    row = np.repeat(np.arange(N), np.diff(A.indptr))
    slot = np.arange(A.nnz) - np.repeat(A.indptr[:-1], np.diff(A.indptr))
    ecols[row, slot] = A.indices
    evals[row, slot] = A.data
    lev.ell_cols = torch.as_tensor(ecols.T.copy(), dtype=torch.int32,
                                   device=self.device).contiguous()
    lev.ell_vals = torch.as_tensor(evals.T.copy(), dtype=self.dtype,
                                   device=self.device).contiguous()
    lev.ell_dinv = torch.as_tensor(dinv, dtype=self.dtype, device=self.device)
    lev.ell_work = torch.zeros(3 * N, dtype=self.dtype, device=self.device)

  def _steps_for(self, steps):
    if steps is None:
      kappa = self.coarse_bounds[1] / self.coarse_bounds[0]
      steps = math.ceil(0.5 * math.sqrt(kappa) *
                        math.log(2.0 / COARSE_REDUCTION))
      steps = max(2, min(COARSE_MAX_STEPS, steps))
    return int(steps)

  def _coarse_setup_partitioned(self, lev, steps, bounds):
    """The rank-local order-1 matrix in ELL form, the assembled (exchanged)
    diagonal, the interface / interior row lists of the overlapped step, and
    the bounds of the Jacobi-scaled spectrum of the global matrix.

    The bounds come from Lanczos on D^-1/2 A D^-1/2 with global inner
    products, run until both extreme Ritz values change by less than
    COARSE_LANCZOS_RTOL over COARSE_LANCZOS_CHECK steps (at most
    COARSE_LANCZOS_MAX).  That is enough because the two bounds matter
    differently: the largest Ritz value converges first (a well-separated
    end of the spectrum: error ~ exp(-2 k sqrt(gap))), and the 5 % margin
    above it keeps the polynomial positive; the smallest needs about
    sqrt(kappa) steps (~100 for the order-1 matrix of a 128^3-element box),
    and an estimate that is still too large leaves the polynomial positive
    definite -- it only weakens the coarse solve (see `_coarse_setup`)."""
    A = self._local_matrix(lev)
    N = A.shape[0]
    diag = self._exchange_(torch.as_tensor(A.diagonal(), dtype=torch.float64,
                                           device=self.device), lev.mesh)
    dinv = torch.where(diag > 0, 1.0 / torch.where(diag > 0, diag,
                                                   torch.ones_like(diag)),
                       torch.zeros_like(diag))
    self._store_ell(lev, A, dinv.cpu().numpy())
    iface = np.zeros(N, dtype=bool)
    iface[lev.mesh.neighbor_plan.interface_nodes('cpu').numpy()] = True
    lev.rows_iface = torch.as_tensor(np.nonzero(iface)[0].astype(np.int32),
                                     device=self.device)
    lev.rows_inner = torch.as_tensor(np.nonzero(~iface)[0].astype(np.int32),
                                     device=self.device)
    if bounds is None:
      last = {}

      def check(k, alphas, betas):
        if k % COARSE_LANCZOS_CHECK:
          return False
        T = (np.diag(alphas) + np.diag(betas[:k - 1], 1) +
             np.diag(betas[:k - 1], -1))
        ev = np.linalg.eigvalsh(T)
        prev, last['ev'] = last.get('ev'), (ev[0], ev[-1])
        return prev is not None and all(
            abs(a - b) <= COARSE_LANCZOS_RTOL * abs(b)
            for a, b in zip(last['ev'], prev))

      apply_fn = lambda u, out: self._coarse_matvec(lev, u, out)
      ev = self._lanczos(lev, apply_fn, dinv.sqrt(), COARSE_LANCZOS_MAX, check)
      lmin, lmax = float(ev[0]), float(ev[-1])
      if not lmin > 1e-12 * lmax:
        raise NotImplementedError(
            'p-multigrid needs a positive definite operator (the coarse '
            'matrix is singular: no Dirichlet nodes and lambda0 = 0?)')
      bounds = (0.9 * lmin, 1.05 * lmax)
    self.coarse_bounds = tuple(float(b) for b in bounds)
    self.coarse_steps = self._steps_for(steps)
    lev.coarse_cheb = _cheb_coefficients(*self.coarse_bounds,
                                         self.coarse_steps)

  def _coarse_matvec(self, lev, x, out):
    """out = QQ^T A_loc x: interface rows, exchange posted, interior rows,
    exchange finished."""
    from swirl_fem_amd.distributed import comm
    _ops.ell_spmv(lev.ell_cols, lev.ell_vals, x, out, rows=lev.rows_iface)
    handle = comm.neighbor_exchange_start(out, lev.mesh.neighbor_plan,
                                          self.group)
    _ops.ell_spmv(lev.ell_cols, lev.ell_vals, x, out, rows=lev.rows_inner)
    return comm.neighbor_exchange_finish(handle, out)

  def _coarse_partitioned(self, lev, b):
    """The polynomial of `sfem_ell_chebyshev` (same bounds and steps) on the
    global order-1 matrix, one overlapped product per step."""
    x, d, ax, dinv = lev.x, lev.d, lev.ax, lev.ell_dinv
    for k, (a, c) in enumerate(lev.coarse_cheb):
      if k == 0:
        _ops.cheb_step(x, d, None, b, dinv, None, 0.0, c, _ops.CHEB_FIRST)
        continue
      self._coarse_matvec(lev, x, ax)
      _ops.cheb_step(x, d, ax, b, dinv, None, a, c, _ops.CHEB_GENERAL)
    return x

  def _coarse_setup(self, lev, steps, bounds=None):
    """The order-1 matrix in ELL form (Dirichlet rows and columns zero) and
    the bounds of its Jacobi-scaled spectrum (`bounds`: given instead)."""
    import scipy.sparse as sp
    mesh = lev.mesh
    N = mesh.num_nodes
    A = self._local_matrix(lev)
    diag = A.diagonal()
    interior = np.nonzero(diag > 0)[0]
    if interior.size == 0:
      raise ValueError('the coarse operator has no interior rows')
    Ai = A[interior][:, interior]
    dm = 1.0 / np.sqrt(Ai.diagonal())
    S = sp.diags(dm) @ Ai @ sp.diags(dm)
    if bounds is not None:
      lmin, lmax = None, None
    else:
      lmin, lmax = jacobi_scaled_extremes(S, mesh.ndim)
    if bounds is not None:
      self.coarse_bounds = tuple(float(b) for b in bounds)
    elif not lmin > 1e-12 * lmax:
      raise NotImplementedError(
          'p-multigrid needs a positive definite operator (the coarse matrix '
          'is singular: no Dirichlet nodes and lambda0 = 0?)')
    else:
      self.coarse_bounds = (0.9 * lmin, 1.05 * lmax)
    self.coarse_steps = self._steps_for(steps)
    dinv = np.zeros(N)
    dinv[interior] = 1.0 / diag[interior]
    self._store_ell(lev, A, dinv)

  # ----------------------------------------------------------------- apply
  def restrict(self, l, r, out):
    """out (level l + 1) = P^T r (level l)."""
    t = self.levels[l].transfer
    _ops.pmg_restrict(r, t['local'], t['cidx'], t['fidx'],
                      t['restrict_owner'], t['mat'], self.levels[l].mesh.ndim,
                      t['pc'], t['pf'])
    _ops.scatter_csr(t['local'], t['offsets'], t['slots'], out.numel(),
                     out=out)
    # (a partition: this rank's share of P^T r, summed over the ranks)
    return self._exchange_(out, self.levels[l + 1].mesh)

  def prolong(self, l, xc, out, add=False):
    """out (level l) = P xc (level l + 1); add: out += P xc."""
    t = self.levels[l].transfer
    return _ops.pmg_prolong(xc, out, t['cidx'], t['fidx'], t['owner'],
                            t['mat'], self.levels[l].mesh.ndim, t['pc'],
                            t['pf'], add)

  def smooth(self, l, b, from_zero):
    """x of level l after `smoother_degree` Chebyshev steps on b."""
    lev = self.levels[l]
    for k, (a, c) in enumerate(lev.cheb):
      if k == 0 and from_zero:
        _ops.cheb_step(lev.x, lev.d, None, b, lev.dinv, None, 0.0, c,
                       _ops.CHEB_FIRST)
        continue
      lev.apply(lev.x, lev.ax)
      _ops.cheb_step(lev.x, lev.d, lev.ax, b, lev.dinv, None, a, c,
                     _ops.CHEB_RESTART if k == 0 else _ops.CHEB_GENERAL)
    return lev.x

  def _cycle(self, l, b):
    lev = self.levels[l]
    if l == len(self.levels) - 1:
      if self.plan is not None:
        return self._coarse_partitioned(lev, b)
      lo, hi = self.coarse_bounds
      return _ops.ell_chebyshev(lev.ell_cols, lev.ell_vals, lev.ell_dinv, b,
                                self.coarse_steps, lo, hi, work=lev.ell_work,
                                out=lev.x)
    self.smooth(l, b, from_zero=True)
    lev.apply(lev.x, lev.ax)
    _ops.cheb_step(None, None, lev.ax, b, None, lev.r, 0.0, 0.0,
                   _ops.CHEB_RESIDUAL)
    coarse = self.levels[l + 1]
    self.restrict(l, lev.r, coarse.b)
    xc = self._cycle(l + 1, coarse.b)
    self.prolong(l, xc, lev.x, add=True)
    return self.smooth(l, b, from_zero=False)

  def __call__(self, r):
    if r.dim() != 1 or r.numel() != self.levels[0].mesh.num_nodes:
      raise ValueError('PMultigridPreconditioner takes an (N,) vector')
    r = r.to(self.dtype).contiguous()
    return self._cycle(0, r)
