"""Fused element operators (build-side fast paths behind the reference API).

* `HelmholtzOperator`: the collocated  H = lambda0 * B + lambda1 * A  of the
  reference's callers -- examples/poisson.py:141-154 (A, B),
  navier_stokes/navier_stokes.py:220-236, :295-307, :431 -- as ONE kernel:
  gather, sum-factorised apply, Dirichlet mask and direct-stiffness summation
  (`sfem_helmholtz_apply`).  The geometric factors of affine / multilinear
  elements are evaluated in registers, curved elements read 6 (+1) stored
  factors per point (`classify_geometry`).
* `TwoGridHelmholtzOperator`: the same operator when the quadrature differs
  from the nodes (interpolate -> fused kernel on the quadrature grid ->
  transposed interpolation).
* `StokesDivGrad`: D and D^T of the P_N - P_{N-2} pair (navier_stokes.py:
  313-338), one kernel each.
* `ConvectionOperator`: the over-integrated convection term (:238-245).

Every class has a `supports_*` predicate; callers fall back to the generic
q-function path (`FiniteElementSpace.local_covector`) when it says no.
"""

from __future__ import annotations

import dataclasses
import os

import numpy as np
import torch

from swirl_fem_amd import switches
from swirl_fem_amd import _ops
from swirl_fem_amd.core import autodiff

MAX_FUSED_P = 12


def supports_fused(fespace) -> str | None:
  """None if the fused kernel applies, else the reason it does not."""
  P = fespace.mesh.gridpoints_1d.num_points
  if not fespace.is_collocated:
    return 'quadrature points differ from the nodes'
  if fespace.mesh.ndim not in (2, 3):
    return f'ndim={fespace.mesh.ndim}'
  if not 2 <= P <= MAX_FUSED_P:
    return f'P={P} outside 2..{MAX_FUSED_P}'
  d = fespace.interpolator._differentiation_matrix_1d()
  if not np.allclose(d[::-1, ::-1], -d, rtol=0,
                     atol=1e-12 * max(1.0, np.abs(d).max())):
    return 'node set is not symmetric about 0'
  return None


MULTILINEAR_RTOL = {torch.float64: 1e-12, torch.float32: 2e-6}
AFFINE_RTOL = {torch.float64: 1e-11, torch.float32: 1e-5}


def classify_geometry(fespace):
  """Per element: 0 = curved (stored per-point factors), 1 = affine,
  3 = multilinear image of the reference cube; plus the (E, 24) coefficients.

  An element is multilinear when its nodes coincide with the multilinear
  interpolant of its 2^d corner nodes (every `refine_premesh` mesh); it is
  affine when the bilinear/trilinear coefficients vanish as well.
  """
  mesh = fespace.mesh
  d, P = mesh.ndim, mesh.gridpoints_1d.num_points
  xe = mesh.element_coords()                                   # (E, n, d)
  coef = _ops.helmholtz_setup_multilinear(xe, d, P)            # (E, 24)
  x1 = torch.as_tensor(mesh.gridpoints_1d.node_values, dtype=xe.dtype,
                       device=xe.device)
  grids = torch.meshgrid(*([x1] * d), indexing='ij')
  r = [g.reshape(-1) for g in grids]                           # (n,) each
  if d == 3:
    mono = torch.stack([r[0], r[1], r[2], r[0] * r[1], r[1] * r[2],
                        r[0] * r[2], r[0] * r[1] * r[2]], dim=1)   # (n, 7)
    A = coef[:, :21].reshape(-1, 7, 3)
    lin, nonlin = A[:, :3], A[:, 3:]
  else:
    mono = torch.stack([r[0], r[1], r[0] * r[1]], dim=1)          # (n, 3)
    A = coef[:, :6].reshape(-1, 3, 2)
    lin, nonlin = A[:, :2], A[:, 2:]
  centre = xe.mean(dim=1, keepdim=True) - torch.einsum(
      'nm,emd->ed', mono, A)[:, None, :] / mono.shape[0]
  recon = centre + torch.einsum('nm,emd->end', mono, A)
  size = lin.abs().amax(dim=(1, 2))
  err = (recon - xe).abs().amax(dim=(1, 2))
  # coordinates carry rounding of their own magnitude (matters in fp32)
  noise = 8 * torch.finfo(xe.dtype).eps * xe.abs().amax(dim=(1, 2))
  multi = err <= MULTILINEAR_RTOL[xe.dtype] * size + noise
  affine = multi & (nonlin.abs().amax(dim=(1, 2)) <=
                    AFFINE_RTOL[xe.dtype] * size + noise)
  kind = torch.zeros(xe.shape[0], dtype=torch.int32, device=xe.device)
  kind[multi] = _GEO_MULTILINEAR
  # a handful of affine elements among multilinear ones (a jittered mesh in
  # fp32: 39 of 32768 pass the tolerance) are not worth a launch of their own
  # and an element list for everybody else: the multilinear kernels evaluate
  # them exactly
  n_affine, n_multi = int(affine.sum()), int(multi.sum())
  if n_affine >= 0.02 * max(n_multi, 1) or n_affine == n_multi:
    kind[affine] = _GEO_AFFINE
  return kind, coef


_GEO_POINT, _GEO_AFFINE, _GEO_MULTILINEAR, _GEO_BOX = 0, 1, 3, 5
FACET_P = tuple(range(6, 13))  # orders the facet-table kernels are compiled for
STOKES_FACET_P = (6, 7, 8)     # ... and the facet-table Stokes kernels
BOX_TOL = {torch.float64: 1e-13, torch.float32: 5e-7}


def _geometry_parts(fespace, key, point_setup, geometry, *, multilinear=False,
                    corners=False):
  """One launch description per geometry kind present, for kernels on the
  quadrature grid of `fespace`: `geo_mode`; `elem_list` when the kind is a
  strict subset of the elements; for curved elements the stored per-point
  data `point_setup(invjacs, jacdets, w)` under `key` ('geo' or 'kfac') with
  `geo_index` (element -> row) when they are a subset; otherwise `geo_elem`,
  the multilinear coefficients.  `geometry`: 'auto', 'stored' (per-point data
  for every element) and, where the caller accepts it (`multilinear`),
  'multilinear' (no affine shortcut).  `corners`: node families without end
  points have no corner nodes to read the coefficients from and take 'stored'.
  Returns (parts, the (E, 24) coefficients or None, elements per kind)."""
  mesh = fespace.mesh
  E, dev = mesh.num_elements, fespace.device
  if corners:
    from swirl_fem_amd.core.interpolation import NodeType
    if mesh.gridpoints_1d.node_type not in (
        NodeType.GAUSS_LOBATTO_LEGENDRE, NodeType.NEWTON_COTES):
      geometry = 'stored'
  if geometry == 'stored':
    kind = torch.zeros(E, dtype=torch.int32, device=dev)
    coef = None
  else:
    kind, coef = classify_geometry(fespace)
    if multilinear and geometry == 'multilinear':
      kind = torch.where(kind == _GEO_AFFINE,
                         torch.full_like(kind, _GEO_MULTILINEAR), kind)
  w = torch.as_tensor(fespace.quadrature.weights_nd(mesh.ndim),
                      dtype=fespace.dtype, device=dev)
  counts = {k: int((kind == k).sum()) for k in
            (_GEO_POINT, _GEO_AFFINE, _GEO_MULTILINEAR)}
  parts = []
  for k in (_GEO_AFFINE, _GEO_MULTILINEAR, _GEO_POINT):
    if counts[k] == 0:
      continue
    part = {'geo_mode': k}
    sel = kind == k
    if counts[k] < E:
      part['elem_list'] = torch.nonzero(sel).reshape(-1).to(
          torch.int32).contiguous()
    if k != _GEO_POINT:
      part['geo_elem'] = coef
    elif counts[k] < E:
      part[key] = point_setup(fespace.invjacs[sel].contiguous(),
                              fespace.jacdets[sel].contiguous(), w)
      part['geo_index'] = (torch.cumsum(sel, 0) - 1).to(
          torch.int32).contiguous()
    else:
      part[key] = point_setup(fespace.invjacs, fespace.jacdets, w)
    parts.append(part)
  return parts, coef, counts


def _host_tables(fespace, quadrature_grid):
  """The host tables of a launch (NumPy): differentiation matrix, weights and
  points of the grid the kernels work on -- the nodes of a collocated
  operator, or the quadrature points (`quadrature_grid`)."""
  if quadrature_grid:
    dmat, grid = _quadrature_dmat(fespace), fespace.quadrature.nodes
  else:
    dmat = fespace.interpolator._differentiation_matrix_1d()
    grid = fespace.mesh.gridpoints_1d
  return {'dmat': dmat, 'weights': np.asarray(fespace.quadrature.weights),
          'nodes': np.asarray(grid.node_values)}


def chain_segment_length(num_elements):
  """Elements per chain segment (= per workgroup of a chain launch): 8 on
  large meshes; shorter when that would leave the 256 CUs x 16 waves of an
  MI355X with fewer than ~4 rounds of workgroups (16^3 elements in chains of
  8 are 512 workgroups: the Taylor-Green step at 16^3 went from 33 to 50 ms).
  `SFEM_CHAIN_LEN` overrides."""
  env = switches.get('SFEM_CHAIN_LEN')
  if env:
    return max(1, int(env))
  return max(1, min(8, num_elements // 16384))


def facet_chains(elements, ids, P, seg_len):
  """Walks the elements `ids` (int64, device) as chains for the chain launches
  of the facet kernels (`sfem_helmholtz_args.chain_offsets`): element y follows
  x when the face a = P-1 of x is the face a = 0 of y, node for node in the
  lane layout, i.e. `elements[x, (P-1) P^2 + t] == elements[y, t]` for all
  t < P^2 (on a refiner mesh: the neighbour across that face, met with the
  same orientation).  Chains are cut into segments of at most `seg_len`
  elements.  Returns (offsets (S + 1,), elems) int32; elements without a
  neighbour of that kind are segments of their own."""
  m = ids.numel()
  dev = ids.device
  n2 = P * P
  first = elements[ids, :n2].to(torch.int64)
  last = elements[ids, (P - 1) * n2:].to(torch.int64)
  gen = torch.Generator(device='cpu').manual_seed(1234)
  wts = torch.randint(1, 1 << 31, (n2,), generator=gen).to(dev)
  hf, hl = (first * wts).sum(1), (last * wts).sum(1)
  hs, order = torch.sort(hf)
  pos = torch.searchsorted(hs, hl).clamp(max=m - 1)
  cand = order[pos]
  me = torch.arange(m, device=dev)
  ok = (hs[pos] == hl) & (cand != me)
  ok &= (first[cand] == last).all(dim=1)
  ok &= (last >= 0).all(dim=1)
  succ = torch.where(ok, cand, torch.full_like(cand, -1))
  # a face has two elements, so successors are distinct; keep it true anyway
  pred = torch.full((m,), -1, dtype=torch.int64, device=dev)
  src = torch.nonzero(succ >= 0).reshape(-1)
  pred[succ[src]] = src
  valid = torch.zeros(m, dtype=torch.bool, device=dev)
  valid[src] = pred[succ[src]] == src
  succ = torch.where(valid, succ, torch.full_like(succ, -1))
  pred.fill_(-1)
  src = torch.nonzero(succ >= 0).reshape(-1)
  pred[succ[src]] = src
  # list ranking by pointer jumping: head and distance to it
  p = torch.where(pred >= 0, pred, me)
  d = (pred >= 0).to(torch.int64)
  for _ in range(max(1, int(m).bit_length())):
    d = d + d[p]
    p = p[p]
  loop = pred[p] >= 0            # closed rings never reach a head
  if bool(loop.any()):           # members of a ring walk alone
    p = torch.where(loop, me, p)
    d = torch.where(loop, torch.zeros_like(d), d)
  key = p * (int(d.max()) + 1 if m else 1) + d
  walk = torch.argsort(key)
  rank = d[walk]
  starts = torch.nonzero(rank % seg_len == 0).reshape(-1)
  offsets = torch.cat([starts, torch.tensor([m], device=dev)])
  return (offsets.to(torch.int32).contiguous(),
          ids[walk].to(torch.int32).contiguous())


def _facet_parts(fespace, parts, mask, multiplicity, coef):
  """`parts` re-expressed on compact connectivity (`sfem_facet_table_build`):
  elements whose index row is 27 affine facet maps (every `refine_premesh`
  mesh, reference core/mesh_refiner.py:143-251) are applied from their
  432-byte table, affine ones with a diagonal metric as boxes; the remaining
  elements keep their index rows.  None if no element qualifies."""
  mesh = fespace.mesh
  E = mesh.num_elements
  tab, ok = _ops.facet_table(mesh.elements, mask, multiplicity,
                             mesh.gridpoints_1d.num_points)
  if not bool(ok.any()):
    return None
  every = torch.arange(E, device=ok.device)
  cst = None
  out = []
  P = mesh.gridpoints_1d.num_points
  seg_len = chain_segment_length(E)

  def add(part, ids, mode, facet):
    if ids.numel() == 0:
      return
    new = {k: v for k, v in part.items() if k != 'elem_list'}
    new['geo_mode'] = mode
    if ids.numel() < E:
      new['elem_list'] = ids.to(torch.int32).contiguous()
    if facet:
      new.pop('shared_order', None)
      new['facet_table'] = tab
      new['geo_const'] = cst
      # chains (one-wave elements): box 0.72 -> 0.58 ms, affine 0.72 -> 0.66,
      # multilinear 0.92 -> 0.87, stored 1.86 -> 1.80 at config 2; elements
      # that span several waves (P >= 9) lose with them (p = 11 fp32 box 1.74
      # vs 1.46 ms)
      # (P >= 9 has chain instantiations for box / affine elements only:
      # FacetElem::CHAINS; the library refuses the others)
      if seg_len > 1 and (P <= 8 or (
          switches.get('SFEM_CHAIN_HI') == '1' and
          mode in (_GEO_BOX, _GEO_AFFINE))):
        new['chains'] = facet_chains(mesh.elements, ids, P, seg_len)
        new['chain_len'] = seg_len
    out.append(new)

  use_box = switches.get('SFEM_BOX') != '0'
  for part in parts:
    ids = every if 'elem_list' not in part else part['elem_list'].long()
    good = ok[ids]
    mode = part['geo_mode']
    if mode == _GEO_MULTILINEAR and P >= 9:
      # 12 nodes per lane plus the multilinear geometry state need 203 VGPRs
      # on the facet kernel (2 waves per SIMD): measured 3.97 vs 2.99 ms for
      # the index-row kernel at p = 11 fp32, which therefore keeps them
      good = torch.zeros_like(good)
    if mode == _GEO_AFFINE:
      if cst is None:
        cst = _ops.helmholtz_setup_affine(coef, BOX_TOL[fespace.dtype])
      box = (cst[ids, 7] != 0) & good if use_box else torch.zeros_like(good)
      add(part, ids[box], _GEO_BOX, True)
      add(part, ids[good & ~box], _GEO_AFFINE, True)
    else:
      add(part, ids[good], mode, True)
    add(part, ids[~good], mode, False)
  return out


@dataclasses.dataclass(eq=False)
class LayerPlan:
  """Layered assembly of an operator's facet launches (`build_layer_plan`).

  `layers[k] = (length, offset)`: layer k + 1 of the extended output
  [N nodal values | layer 1 | layer 2 | ...] covers the nodes [0, length) and
  starts at element `offset`; `extent` = size of the extended vector;
  `parts` = the launches with their `layered_table`; `written` = number of
  slots the launches store per apply (layer 0 included)."""
  layers: list
  extent: int
  parts: list
  written: int
  num_nodes: int
  # (uint8 device tensor, per-layer offsets): byte c of a layer = 1 iff some
  # element writes into its nodes [512 c, 512 (c + 1)); the consumers skip the
  # other chunks (zeros).  `read` = layer values they then read per pass.
  masks: tuple | None = None
  read: int = 0


def build_layer_plan(facet_parts, num_elements, num_nodes, P):
  """Gives every (element, facet) that writes a facet of the mesh a LAYER of
  its own for it, so that the direct-stiffness sum (reference
  core/gather_scatter.py:130-133) needs neither atomics nor a cleared range:
  the kernels store every result plainly, the consumer adds the layers of a
  node in layer order (`sfem_cg_update_r_layered`, `sfem_fold_layers`).

  Writers of a facet: every element that holds it, except -- inside a chain
  segment -- the element that hands its last face (and that face's edges and
  vertices) on to its successor, which stores the sum.  Layer = rank of the
  writer among the writers of the facet (0 = the nodal vector itself).  Layer
  k is an array over the nodes [0, n_k), n_k = 1 + the largest node id that
  one of its writers stores.  The refiner numbers vertices, then edge, face
  and element interiors, so there the nodes with k + 1 or more writers come
  first and n_k is short (config 2: n_1 = 37 % of N, n_2 = n_3 = 5 %,
  n_4.. = 0.3 %); other numberings whose facets are affine maps of node ids
  reach this path as well, and there n_k can approach N.  Slots nobody writes (a facet with fewer writers than the layer's other
  facets) stay zero from the allocation.

  Returns None when the launches do not cover every element from a facet table
  (index-row elements accumulate with atomics), when a stride does not fit
  the 16 bits of the layered table, or when a facet has more than
  SFEM_MAX_LAYERS + 1 writers."""
  from swirl_fem_amd import _lib
  if not facet_parts or any('facet_table' not in q for q in facet_parts):
    return None
  tab = facet_parts[0]['facet_table']
  dev = tab.device
  E, N = num_elements, num_nodes
  use_chains = switches.get('SFEM_CHAIN') != '0'
  has_succ = torch.zeros(E, dtype=torch.bool, device=dev)
  covered = torch.zeros(E, dtype=torch.int32, device=dev)
  for q in facet_parts:
    if q['facet_table'] is not tab:
      return None
    if 'elem_list' in q:
      covered[q['elem_list'].long()] += 1
    else:
      covered += 1
    if 'chains' in q and use_chains:
      off, elems = q['chains']
      succ = torch.ones(elems.numel(), dtype=torch.bool, device=dev)
      succ[off[1:].long() - 1] = False           # last element of a segment
      has_succ[elems.long()] = succ
  if not bool((covered == 1).all()):
    return None
  t = tab.to(torch.int64)                                    # (E, 27, 4)
  code = t[..., 0] & 0xFFFFFFFF
  id0, dflag = code & 0x3FFFFFFF, code & 0x80000000
  strides = t[..., 1:]                                       # (E, 27, 3)
  if int(strides[..., 1:].abs().max()) >= 32768:
    return None
  f = torch.arange(27, device=dev)
  inner = torch.stack([f // 9 == 1, (f // 3) % 3 == 1, f % 3 == 1], dim=1)
  span = strides * (P - 3) * inner[None].to(torch.int64)     # (index - 1) max
  lo = id0 + span.clamp(max=0).sum(-1)                       # smallest node id
  hi = id0 + span.clamp(min=0).sum(-1) + 1                   # largest + 1
  count = torch.where(inner, P - 2, 1).prod(dim=1)           # nodes per facet
  writer = torch.ones((E, 27), dtype=torch.bool, device=dev)
  writer[:, 18:] &= ~has_succ[:, None]                       # a-class LAST
  idx = torch.nonzero(writer.reshape(-1)).reshape(-1)
  key, perm = torch.sort(lo.reshape(-1)[idx], stable=True)
  first = torch.ones_like(key, dtype=torch.bool)
  first[1:] = key[1:] != key[:-1]
  pos = torch.arange(key.numel(), device=dev)
  start = torch.cummax(torch.where(first, pos, torch.zeros_like(pos)), 0).values
  layer = torch.zeros(E * 27, dtype=torch.int64, device=dev)
  layer[idx[perm]] = pos - start
  nl = int(layer.max())
  if nl > _lib.SFEM_MAX_LAYERS:
    return None
  hi_w = torch.where(writer, hi, torch.zeros_like(hi)).reshape(-1)
  lens = [int(hi_w[layer == k].max()) for k in range(1, nl + 1)]
  for k in range(nl - 2, -1, -1):
    lens[k] = max(lens[k], lens[k + 1])
  pad = lambda v: (v + 3) // 4 * 4                 # 16 bytes in fp32 and fp64
  lens = [pad(v) for v in lens]
  offs, at = [], pad(N)
  for v in lens:
    offs.append(at)
    at += v
  extent = at
  if extent > 0x3FFFFFFF:
    return None
  base = torch.tensor([0] + offs, dtype=torch.int64, device=dev)
  pos_out = (base[layer].reshape(E, 27) + id0) | dflag
  packed = (strides[..., 1] & 0xFFFF) | ((strides[..., 2] & 0xFFFF) << 16)
  wrap = lambda v: ((v + (1 << 31)) % (1 << 32) - (1 << 31)).to(torch.int32)
  tab2 = torch.stack([t[..., 0].to(torch.int32), wrap(pos_out),
                      strides[..., 0].to(torch.int32), wrap(packed)],
                     dim=-1).contiguous()
  written = int((writer.to(torch.int64) * count[None]).sum())
  parts = [dict(q, layered_table=tab2, layered_chains=use_chains and
                'chains' in q) for q in facet_parts]
  # which chunks of each layer are written at all: every chunk of a writer's
  # id range [lo, hi), marked through a difference array summed over the
  # layer's chunks.  A superset of the chunks it stores into, exact when a
  # facet spans fewer than `chunk` ids (refiner numbering: one run of at most
  # (P - 2)^2 ids).  A facet of a lexicographic numbering spans ~M^2 ids with
  # gaps, and its nodes fall into chunks between those of its two ends.
  chunk = _lib.SFEM_LAYER_CHUNK
  flat_layer, flat_w = layer, writer.reshape(-1)
  lo_f, hi_f = lo.reshape(-1), hi.reshape(-1)
  bytes_, moffs, read = [], [], 0
  for k, ln in enumerate(lens, start=1):
    nc = (ln + chunk - 1) // chunk
    sel = flat_w & (flat_layer == k)
    first, last = lo_f[sel] // chunk, (hi_f[sel] - 1) // chunk
    d = torch.zeros(nc + 1, dtype=torch.int64, device=dev)
    d.index_add_(0, first, torch.ones_like(first))
    d.index_add_(0, last + 1, -torch.ones_like(last))
    m = (torch.cumsum(d, 0)[:nc] > 0).to(torch.uint8)
    moffs.append(sum(b.numel() for b in bytes_))
    bytes_.append(m)
    read += min(int(m.sum()) * chunk, ln)
  masks = (torch.cat(bytes_), moffs) if bytes_ else None
  return LayerPlan(layers=list(zip(lens, offs)), extent=extent, parts=parts,
                   written=written, num_nodes=N, masks=masks, read=read)


def _cluster_limits(fespace):
  """(cluster_size, max_shared) if the cluster kernels cover this space."""
  mesh = fespace.mesh
  if mesh.ndim != 3:
    return None
  return _ops.helmholtz_cluster_limits(mesh.gridpoints_1d.num_points,
                                       fespace.dtype)


def _attach_clusters(fespace, enc, multiplicity, parts):
  """`parts` with a `ClusterPlan` each (`core/clusters.py`): every launch then
  sums the shared nodes of 8 neighbouring elements in LDS."""
  from swirl_fem_amd.core import clusters
  size, kmax = _cluster_limits(fespace)
  ids = [None if 'elem_list' not in p else p['elem_list'].to(torch.int64)
         for p in parts]
  plans = clusters.build_cluster_plan(fespace.mesh, enc, multiplicity, ids,
                                      size, kmax)
  out = []
  for part, plan in zip(parts, plans):
    if plan is not None:
      out.append(dict({k: v for k, v in part.items() if k != 'shared_order'},
                      cluster=plan))
  return out


def colored_launch_order(colors, num_colors, group, num_groups):
  """Launches of coloured assembly: [(group, element ids int64)], one per
  non-empty (colour, group) pair, colour-major.  `colors` (E,) from
  `AssemblyPlan.coloring`, `group` (E,) the launch group (geometry kind) of
  every element, -1 for none.

  The kernel stores the first toucher of a node (the slot of least colour)
  and adds every other slot to what is there, so all launches of colour c
  must run before any of colour c + 1.  Within a colour the groups share no
  node and may go in any order.  (Group-major order ran an affine element of
  colour 3 before the multilinear element of colour 0 that first touches a
  shared node: its sum was read from a stale value and then overwritten.)"""
  colors = colors.to(torch.int64)
  group = group.to(torch.int64)
  out = []
  for c in range(num_colors):
    for g in range(num_groups):
      lst = torch.nonzero((colors == c) & (group == g)).reshape(-1)
      if lst.numel():
        out.append((g, lst))
  return out


def first_toucher_violations(elements, first, launches):
  """Slots of `elements` (E, n) that are not their node's first toucher
  (`first`, from `AssemblyPlan.coloring`) but whose element runs no later
  than the first toucher's in `launches` (`colored_launch_order`): 0 when
  the coloured assembly is correct."""
  el = elements.to(torch.int64)
  E = el.shape[0]
  launch = torch.full((E,), -1, dtype=torch.int64, device=el.device)
  for i, (_, lst) in enumerate(launches):
    launch[lst.to(device=el.device, dtype=torch.int64)] = i
  ok = el >= 0
  if not bool(ok.any()):
    return 0
  if bool((launch[ok.any(dim=1)] < 0).any()):
    raise RuntimeError('coloured assembly: an element is in no launch')
  slot_launch = launch[:, None].expand_as(el)
  num_nodes = int(el[ok].max()) + 1
  first_launch = torch.full((num_nodes,), -1, dtype=torch.int64,
                            device=el.device)
  first_launch.scatter_reduce_(0, el[first & ok], slot_launch[first & ok],
                               'amax')
  later = ok & ~first
  return int((slot_launch[later] <= first_launch[el[later]]).sum())


def coefficient(value, name, num_elements, npts, points, dtype, device,
                positive=None):
  """A diffusivity (`name` 'diffusivity': finite, > 0) or reaction coefficient
  ('reaction': finite, >= 0) in normal form: None, a float, or
  (mode, tensor) with mode `_lib.COEF_ELEM` and an (E,) tensor or
  `_lib.COEF_POINT` and an (E, npts) tensor at the operator's points
  (lexicographic, axis 0 slowest).  `value` is one of those, or a callable
  that maps (M, d) coordinates to (M,) values: it is evaluated once at
  `points()` (E, npts, d).  Anything else raises ValueError.  `positive`
  states the sign rule of a coefficient with another `name`."""
  from swirl_fem_amd import _lib
  if value is None:
    return None
  if positive is None:
    positive = name == 'diffusivity'
  what = '> 0' if positive else '>= 0'

  def check(t):
    if not bool(torch.isfinite(t).all()):
      raise ValueError(f'{name}: values must be finite')
    if bool((t <= 0).any() if positive else (t < 0).any()):
      raise ValueError(f'{name}: values must be {what}')

  if callable(value) and not isinstance(value, torch.Tensor):
    x = points()
    vals = value(x.reshape(-1, x.shape[-1]))
    t = torch.as_tensor(vals, dtype=dtype, device=device)
    if tuple(t.shape) != (num_elements * npts,):
      raise ValueError(f'{name}: the callable returned shape '
                       f'{tuple(t.shape)}, expected ({num_elements * npts},)')
    t = t.reshape(num_elements, npts).contiguous()
    check(t)
    return (_lib.COEF_POINT, t)
  if isinstance(value, (int, float, np.floating, np.integer)) and not \
      isinstance(value, bool):
    v = float(value)
    check(torch.tensor(v, dtype=torch.float64))
    return v
  try:
    t = torch.as_tensor(value).detach()     # the checks and the kernels read
  except (TypeError, ValueError, RuntimeError):   # values, not a graph
    t = torch.zeros((), dtype=torch.bool)
  numeric = t.is_floating_point() or t.dtype in (torch.int32, torch.int64)
  if t.dim() == 0 and numeric:
    return coefficient(float(t), name, num_elements, npts, points, dtype,
                       device, positive)
  if t.dim() == 0 or not (t.is_floating_point() or t.dtype in (
      torch.int32, torch.int64)):
    raise ValueError(f'{name}: expected a scalar, an (E,) or (E, Q^d) '
                     'tensor or a callable')
  t = t.to(dtype=dtype, device=device)
  if tuple(t.shape) == (num_elements,):
    mode = _lib.COEF_ELEM
  elif tuple(t.shape) == (num_elements, npts):
    mode = _lib.COEF_POINT
  else:
    raise ValueError(f'{name}: shape {tuple(t.shape)}; expected '
                     f'({num_elements},) or ({num_elements}, {npts})')
  t = t.contiguous()
  check(t)
  return (mode, t)


def _fold_point_factors(geo, ndim, kp, cp):
  """Stored factors (S, ng + 1, Q) with G scaled by kp and W by cp ((S, Q)
  each, or None): pairs (G00, G01) (G02, G11) (G12, G22), W in 3D; (G00, G01)
  (G11, W) in 2D (`sfem_helmholtz_setup`)."""
  S, Q = geo.shape[0], geo.shape[2]
  flat = geo.reshape(S, -1).clone()
  if ndim == 3:
    g = flat[:, :6 * Q].view(S, 3, Q, 2)
    w = flat[:, 6 * Q:]
    if kp is not None:
      g.mul_(kp[:, None, :, None])
  else:
    pairs = flat.view(S, 2, Q, 2)
    w = pairs[:, 1, :, 1]
    if kp is not None:
      pairs[:, 0].mul_(kp[:, :, None])
      pairs[:, 1, :, 0].mul_(kp)
  if cp is not None:
    w.mul_(cp)
  return flat.view(geo.shape).contiguous()


def _coefficient_parts(parts, kappa, sigma, num_elements, npts, ndim):
  """`parts` with the array coefficients attached: affine / multilinear
  launches carry `kappa` / `sigma` / `coef_mode` (one mode for both: an (E,)
  array next to a per-point one is expanded), curved launches get them folded
  into a copy of their stored factors.  Scalars stay out (see `apply`)."""
  from swirl_fem_amd import _lib
  arrays = [c for c in (kappa, sigma) if isinstance(c, tuple)]
  if not arrays:
    return parts
  mode = (_lib.COEF_POINT if any(c[0] == _lib.COEF_POINT for c in arrays)
          else _lib.COEF_ELEM)

  def full(c, m):
    if not isinstance(c, tuple):
      return None
    if m == _lib.COEF_POINT and c[0] == _lib.COEF_ELEM:
      return c[1][:, None].expand(num_elements, npts).contiguous()
    return c[1]

  K, C = full(kappa, mode), full(sigma, mode)
  out = []
  for part in parts:
    if part['geo_mode'] == _GEO_POINT:
      Kp, Cp = full(kappa, _lib.COEF_POINT), full(sigma, _lib.COEF_POINT)
      if 'elem_list' in part:      # slots in ascending element order
        lst = part['elem_list'].to(torch.int64)
        Kp = None if Kp is None else Kp[lst]
        Cp = None if Cp is None else Cp[lst]
      part = dict(part, geo=_fold_point_factors(part['geo'], ndim, Kp, Cp))
    else:
      part = dict(part, kappa=K, sigma=C, coef_mode=mode)
    out.append(part)
  return out


def _coefficient_bytes(part, s, npts, lambda0):
  """Bytes a coefficient launch reads per element beyond the constant
  operator: `s` per (E,) coefficient, `s npts` per per-point one (sigma only
  with a mass term)."""
  mode = part.get('coef_mode')
  if not mode:
    return 0
  from swirl_fem_amd import _lib
  per = s if mode == _lib.COEF_ELEM else s * npts
  arrays = [part.get('kappa')] + ([part.get('sigma')] if lambda0 else [])
  return per * sum(a is not None for a in arrays)


def _scaled(coefs, lambda0, lambda1):
  """lambda0, lambda1 times the scalar reaction / diffusivity, if any."""
  if coefs is None:
    return lambda0, lambda1
  k, c = coefs
  return (lambda0 * c if isinstance(c, float) else lambda0,
          lambda1 * k if isinstance(k, float) else lambda1)


def _check_coefficient_mesh(mesh, assembly):
  """The refusals of operators with coefficients."""
  if assembly == 'cluster':
    raise NotImplementedError('coefficients run on index rows: no cluster '
                              'assembly')
  if mesh.axis_name is not None or mesh.neighbor_plan is not None:
    raise NotImplementedError('coefficients on a partitioned mesh')


def _check_scalar_field(u, who='coefficients take'):
  if u.dim() > 1 and u.shape[-1] != 1:
    raise NotImplementedError(f'{who} scalar fields')


def _point_coefficient(c):
  """True if a normal-form coefficient holds per-point values."""
  from swirl_fem_amd import _lib
  return isinstance(c, tuple) and c[0] == _lib.COEF_POINT


def velocity_field(value, num_elements, npts, ndim, points, dtype, device):
  """An advecting velocity b in normal form, an (E, npts, d) tensor at the
  operator's points (lexicographic, axis 0 slowest), or None.  `value`: a
  (d,) constant, an (E, d) tensor of per-element values, an (E, npts, d)
  tensor, or a callable that maps (M, d) coordinates to (M, d) values,
  evaluated once at `points()` (E, npts, d).  Anything else raises
  ValueError."""
  if value is None:
    return None
  E, d = num_elements, ndim
  if callable(value) and not isinstance(value, torch.Tensor):
    x = points()
    t = torch.as_tensor(value(x.reshape(-1, x.shape[-1])), dtype=dtype,
                        device=device)
    if tuple(t.shape) != (E * npts, d):
      raise ValueError(f'velocity: the callable returned shape '
                       f'{tuple(t.shape)}, expected ({E * npts}, {d})')
    t = t.reshape(E, npts, d)
  else:
    try:
      t = torch.as_tensor(value).detach()
    except (TypeError, ValueError, RuntimeError):
      t = torch.zeros((), dtype=torch.bool)
    if not (t.is_floating_point() or t.dtype in (torch.int32, torch.int64)):
      raise ValueError('velocity: expected a (d,), (E, d) or (E, Q^d, d) '
                       'tensor or a callable')
    t = t.to(dtype=dtype, device=device)
    if tuple(t.shape) == (d,):
      t = t[None, None, :].expand(E, npts, d)
    elif tuple(t.shape) == (E, d):
      t = t[:, None, :].expand(E, npts, d)
    elif tuple(t.shape) != (E, npts, d):
      raise ValueError(f'velocity: shape {tuple(t.shape)}; expected ({d},), '
                       f'({E}, {d}) or ({E}, {npts}, {d})')
  if not bool(torch.isfinite(t).all()):
    raise ValueError('velocity: values must be finite')
  return t.contiguous()


def fold_velocity(fespace, b):
  """beta[e,q,d] = W[e,q] sum_j b[e,q,j] invjacs[e,q,j,d]: the velocity (E,
  Q^d, d) at the quadrature points with the geometry folded in, so that the
  advective term at a point is beta . (reference-space derivatives of u)."""
  beta = torch.einsum('eqj,eqjd->eqd', b, fespace.invjacs)
  return (beta * fespace.wdet()[..., None]).contiguous()


def unfold_velocity_gradient(fespace, dbeta):
  """The transpose of `fold_velocity`: the gradient (E, Q^d, d) with respect
  to the folded velocity beta as the gradient with respect to b,
  db[e,q,j] = W[e,q] sum_d dbeta[e,q,d] invjacs[e,q,j,d]."""
  db = torch.einsum('eqd,eqjd->eqj', dbeta, fespace.invjacs)
  return db * fespace.wdet()[..., None]


def _is_callable_source(value):
  return callable(value) and not isinstance(value, torch.Tensor)


def reduce_coefficient_gradient(g, source):
  """A per-point gradient `g` (E, npts) in the form of the coefficient the
  caller passed (`coefficient`): a scalar gives the sum over all points (a
  0-dim tensor), an (E,) tensor the sum over each element's points, an
  (E, npts) tensor `g` itself.  None for None and for a callable."""
  if source is None or _is_callable_source(source) or g is None:
    return None
  shape = tuple(torch.as_tensor(source).shape)
  if shape == ():
    return g.sum()
  if shape == (g.shape[0],):
    return g.sum(dim=1)
  if shape == tuple(g.shape):
    return g
  raise ValueError(f'coefficient of shape {shape} against a gradient of '
                   f'shape {tuple(g.shape)}')


def reduce_velocity_gradient(g, source):
  """A per-point gradient `g` (E, npts, d) in the form of the velocity the
  caller passed (`velocity_field`): (d,) gives the sum over elements and
  points, (E, d) the sum over each element's points, (E, npts, d) `g`
  itself.  None for None and for a callable."""
  if source is None or _is_callable_source(source) or g is None:
    return None
  shape = tuple(torch.as_tensor(source).shape)
  E, _, d = g.shape
  if shape == (d,):
    return g.sum(dim=(0, 1))
  if shape == (E, d):
    return g.sum(dim=1)
  if shape == tuple(g.shape):
    return g
  raise ValueError(f'velocity of shape {shape} against a gradient of shape '
                   f'{tuple(g.shape)}')


def _sensitivity(op, u, lam, lambda0, lambda1, want):
  """Shared by the two operator classes: nodal `u`, `lam` (N,), taken to the
  operator's points -> the three gradients in the callers' forms."""
  fes = op.fespace
  mesh = fes.mesh
  for v in (u, lam):
    if tuple(v.shape) != (mesh.num_nodes,):
      raise ValueError(f'expected ({mesh.num_nodes},) nodal values, got '
                       f'{tuple(v.shape)}')
  src_k, src_c = op.coef_source
  src_b = op.velocity_source
  tensor = lambda v: v is not None and not _is_callable_source(v)
  wk = want[0] and tensor(src_k)
  wc = want[1] and tensor(src_c)
  wb = want[2] and tensor(src_b)
  if not (wk or wc or wb):
    return None, None, None
  ul, ll = (fes._interpolate(mesh.gather(v.detach().to(fes.dtype))[..., None])
            [..., 0].contiguous() for v in (u, lam))
  # the launches without coefficients: curved launches of `parts` carry k and
  # c folded into their stored factors, the sensitivities need bare G and W
  dk, dc, dbeta = _ops.helmholtz_sens(
      ul, ll, op._geo_parts, op.host, mesh.ndim, len(op.host['nodes']),
      lambda0, lambda1, want=(wk, wc, wb))
  db = None if dbeta is None else unfold_velocity_gradient(fes, dbeta)
  return (reduce_coefficient_gradient(dk, src_k),
          reduce_coefficient_gradient(dc, src_c),
          reduce_velocity_gradient(db, src_b))


def _check_velocity_mesh(mesh, assembly):
  """The refusals of operators with an advective term."""
  if assembly not in ('auto', 'atomic', 'colored'):
    raise NotImplementedError(
        f'a velocity runs on index rows: no {assembly!r} assembly')
  if mesh.axis_name is not None or mesh.neighbor_plan is not None:
    raise NotImplementedError('velocity on a partitioned mesh')
  if mesh._cache.get('replicas', 1) > 1:
    raise NotImplementedError('velocity on an ensemble (Mesh.replicate)')


def _advection_parts(parts, beta, num_elements, npts):
  """`parts` with the folded velocity attached.  The advective kernels take
  kappa / sigma per point only: per-element arrays are expanded."""
  from swirl_fem_amd import _lib
  out = []
  for part in parts:
    part = dict(part, beta=beta)
    if part.get('coef_mode') == _lib.COEF_ELEM:
      full = lambda c: None if c is None else (
          c[:, None].expand(num_elements, npts).contiguous())
      part.update(kappa=full(part.get('kappa')), sigma=full(part.get('sigma')),
                  coef_mode=_lib.COEF_POINT)
    out.append(part)
  return out


def _coefficient_intake(fespace, assembly, npts, points, parts, diffusivity,
                        reaction, velocity):
  """What `create` makes of its coefficients and velocity at the operator's
  `npts` points per element (`points()`: their coordinates (E, npts, d),
  built only if a callable asks for them): (coefs, velocity, beta, parts) --
  the normal forms of `coefficient` and `velocity_field`, the folded velocity
  and `parts` with all of them attached; None / `parts` itself without."""
  mesh = fespace.mesh
  E = mesh.num_elements
  coefs = beta = None
  if diffusivity is not None or reaction is not None:
    _check_coefficient_mesh(mesh, assembly)
    coefs = tuple(coefficient(value, name, E, npts, points, fespace.dtype,
                              fespace.device)
                  for value, name in ((diffusivity, 'diffusivity'),
                                      (reaction, 'reaction')))
    parts = _coefficient_parts(parts, *coefs, E, npts, mesh.ndim)
  if velocity is not None:
    _check_velocity_mesh(mesh, assembly)
    velocity = velocity_field(velocity, E, npts, mesh.ndim, points,
                              fespace.dtype, fespace.device)
    beta = fold_velocity(fespace, velocity)
    parts = _advection_parts(parts, beta, E, npts)
  return coefs, velocity, beta, parts


def _advection_diagonal(fespace, parts, beta, dq, keep, bmat):
  """Assembled diagonal (N,) of C_b over the elements of `parts`:
  C_e[i,i] = sum_q I[q,i] beta[e,q,:] . (D I)[q,i] with I the (Q, P)
  interpolation (`bmat`; None: collocated) and D the q-grid differentiation
  matrix `dq`.  Tensor structure: the factor of direction d is I (D I)
  elementwise along axis d and I^2 along the others.  Computed once per
  operator with dense contractions, summed per node like the other parts."""
  mesh = fespace.mesh
  E, d = mesh.num_elements, mesh.ndim
  dev, dtype = fespace.device, fespace.dtype
  dq = np.asarray(dq, dtype=np.float64)
  i1 = np.eye(dq.shape[0]) if bmat is None else np.asarray(bmat, np.float64)
  Q = i1.shape[0]
  S = torch.as_tensor(i1 * i1, dtype=dtype, device=dev)
  T = torch.as_tensor(i1 * (dq @ i1), dtype=dtype, device=dev)
  b = beta.reshape((E,) + (Q,) * d + (d,))
  if d == 2:
    loc = (torch.einsum('eab,ai,bj->eij', b[..., 0], T, S) +
           torch.einsum('eab,ai,bj->eij', b[..., 1], S, T))
  else:
    loc = (torch.einsum('eabc,ai,bj,ck->eijk', b[..., 0], T, S, S) +
           torch.einsum('eabc,ai,bj,ck->eijk', b[..., 1], S, T, S) +
           torch.einsum('eabc,ai,bj,ck->eijk', b[..., 2], S, S, T))
  loc = loc.reshape(E, -1)
  if any('elem_list' in part for part in parts):
    sel = torch.zeros(E, dtype=dtype, device=dev)
    for part in parts:
      if 'elem_list' in part:
        sel[part['elem_list'].to(torch.int64)] = 1
      else:
        sel[:] = 1
    loc = loc * sel[:, None]
  offsets, slots = mesh.assembly_plan().csr()
  out = _ops.scatter_csr(loc.contiguous().reshape(-1), offsets, slots,
                         mesh.num_nodes)
  return out if keep is None else out * keep


class _PlainLinearOperator:
  """`u -> op.apply(u, lambda0, lambda1)` without a fused `u . A(u)`: what
  `linalg.bicgstab` takes (it needs no p . Ap)."""

  def __init__(self, op, lambda0, lambda1, transpose=False):
    self.op, self.lambda0, self.lambda1 = op, lambda0, lambda1
    self.transpose = transpose

  def __call__(self, u):
    if self.transpose:
      return self.op.apply_transpose(u, self.lambda0, self.lambda1)
    return self.op.apply(u, self.lambda0, self.lambda1)


@dataclasses.dataclass(eq=False)
class HelmholtzOperator:
  fespace: object
  parts: list                    # one launch description per geometry kind
  enc: torch.Tensor              # (E, n) encoded indices
  host: dict                     # dmat (P,P), weights (P,), nodes (P,) NumPy
  zero_range: tuple
  num_affine: int = 0
  num_multilinear: int = 0
  num_curved: int = 0
  # the same launches on compact connectivity (scalar / component-major
  # fields), or None: see `_facet_parts`
  facet_parts: list | None = None
  _vector_parts: list | None = None   # launches of vector fields (`_parts_for`)
  _layer_plan: object = None          # LayerPlan, False = none (`layer_plan`)
  keep: torch.Tensor | None = None    # (N,) 1 inside, 0 on Dirichlet nodes
  _diag: tuple | None = None          # assembled (diag B, diag A), `diagonal`
  # variable coefficients: (k, c) in the normal form of `coefficient`, or
  # None; `coef_source` the (diffusivity, reaction) the caller passed
  coefs: tuple | None = None
  coef_source: tuple = (None, None)
  _geo_parts: list | None = None      # the launches without coefficients
  # advective term C_b: the velocity in normal form (`velocity_field`) and
  # with the geometry folded in (`fold_velocity`), or None
  velocity: torch.Tensor | None = None
  beta: torch.Tensor | None = None
  _diag_adv: torch.Tensor | None = None   # assembled diag C_b, `diagonal`
  velocity_source: object = None      # the `velocity` the caller passed

  @classmethod
  def create(cls, fespace, dirichlet_mask=None, geometry='auto',
             assembly='auto', *, diffusivity=None, reaction=None,
             velocity=None) -> 'HelmholtzOperator':
    """geometry: 'auto' (per element: affine / multilinear / stored factors),
    'multilinear' (no affine shortcut) or 'stored' (6 factors per point for
    every element, the general-geometry path).

    assembly (direct-stiffness summation of the shared nodes):
    'atomic': one HBM atomic per shared slot, issued in ascending node order
    (the fastest measured: DESIGN 3.1); 'cluster': clusters of 8 elements
    summed in LDS, HBM atomics only on the cluster surfaces (3D, P = 4..8;
    `core/clusters.py`: half the atomic traffic, but 1.04 vs 0.78 ms at
    config 2 -- the waves of a cluster wait for each other); 'colored': one
    launch per conflict-free colour class, no atomics, bitwise reproducible;
    'auto': 'atomic' (or 'cluster' with SFEM_CLUSTER=1 in the environment).

    diffusivity k, reaction c (`coefficient`): the operator becomes
    lambda0 B_c + lambda1 A_k.  With either one it runs on index rows
    ('atomic' or 'colored' assembly, no facet tables or layers); scalar
    fields on one unpartitioned mesh only.

    velocity b (`velocity_field`): adds the plain Galerkin convective form
    C_b[i,j] = sum_q W_q phi_i(q) b_q . grad phi_j(q), not scaled by either
    lambda: `apply` computes (lambda0 B_c + lambda1 A_k + C_b) u.  The
    operator is then not symmetric (`linalg.bicgstab`); it runs on index rows
    like one with coefficients.  No stabilisation: the Galerkin form needs
    the boundary layers of an advection-dominated problem to be resolved by
    the mesh."""
    why = supports_fused(fespace)
    if why is not None:
      raise NotImplementedError(f'fused Helmholtz kernel unavailable: {why}')
    if geometry not in ('auto', 'multilinear', 'stored'):
      raise ValueError(f'unknown geometry mode {geometry!r}')
    if velocity is not None:
      _check_velocity_mesh(fespace.mesh, assembly)
    if assembly not in ('auto', 'cluster', 'atomic', 'colored'):
      raise ValueError(f'unknown assembly mode {assembly!r}')
    mesh = fespace.mesh
    E = mesh.num_elements
    geo_parts, coef, counts = _geometry_parts(
        fespace, 'geo', _ops.helmholtz_setup, geometry, multilinear=True)
    velocity_source = velocity
    coefs, velocity, beta, parts = _coefficient_intake(
        fespace, assembly, mesh.num_nodes_per_element, mesh.element_coords,
        geo_parts, diffusivity, reaction, velocity)
    if assembly == 'auto' and (coefs is not None or beta is not None):
      assembly = 'atomic'
    requested = assembly
    if assembly == 'auto':
      assembly = ('cluster' if _cluster_limits(fespace) is not None and
                  switches.get('SFEM_CLUSTER') == '1' else 'atomic')
    elif assembly == 'cluster' and _cluster_limits(fespace) is None:
      raise NotImplementedError('cluster assembly needs ndim = 3, P = 4..8')
    plan = mesh.assembly_plan()
    mask = None
    if dirichlet_mask is not None:
      mask = torch.as_tensor(dirichlet_mask, device=fespace.device)
      mask = (mask != 0).to(torch.uint8).contiguous()
    enc = _ops.encode_elements(mesh.elements, mask, plan.multiplicity)
    zero_range = plan.zero_range
    if assembly == 'colored':
      # One launch per (colour class, geometry kind): elements of a class share
      # no node, shared slots read-modify-write `out` in colour order (no
      # atomics, no zero-fill of the shared range, bitwise reproducible).
      # The launches are colour-major, so that every node's first toucher
      # (its plain store) runs before the other elements that add to it.
      colors, num_colors, first = plan.coloring()
      slot_shared = ((mesh.elements >= 0) & ~first).to(torch.uint8).contiguous()
      enc = _ops.encode_elements(mesh.elements, mask, None, slot_shared)
      group = torch.full((E,), -1, dtype=torch.int64, device=fespace.device)
      for g, part in enumerate(parts):
        group[part['elem_list'].to(torch.int64)
              if 'elem_list' in part else slice(None)] = g
      launches = colored_launch_order(colors, num_colors, group, len(parts))
      bad = first_toucher_violations(mesh.elements, first, launches)
      if bad:
        raise RuntimeError(f'coloured assembly: {bad} shared slots would be '
                           'added before their node\'s first store')
      parts = [dict(parts[g], elem_list=lst.to(torch.int32).contiguous(),
                    colored=True) for g, lst in launches]
      unref = torch.nonzero(plan.multiplicity == 0).reshape(-1)
      zero_range = ((int(unref.min()), int(unref.max()) + 1)
                    if unref.numel() else (0, 0))
    if assembly == 'cluster':
      from swirl_fem_amd.core import clusters
      why = clusters.supports_clusters(mesh, enc)
      if why is None:
        parts = _attach_clusters(fespace, enc, plan.multiplicity, parts)
      elif requested == 'cluster':
        raise NotImplementedError(f'cluster assembly unavailable: {why}')
      else:
        assembly = 'atomic'

    if (assembly == 'atomic' and mesh.ndim == 3 and coefs is None and
        beta is None and
        mesh.gridpoints_1d.num_points <= 8 and      # one wave per element
        switches.get('SFEM_SORTED_SCATTER') != '0'):
      # 3D: most slots of an element are shared; issue their atomics in node
      # order (better coalesced, see the kernel)
      so = shared_slot_order(enc)
      if so is not None:
        parts = [dict(part, shared_order=so) for part in parts]
    facet_parts = None
    if (assembly == 'atomic' and mesh.ndim == 3 and coefs is None and
        beta is None and
        mesh.gridpoints_1d.num_points in FACET_P and
        switches.get('SFEM_FACET') != '0'):
      facet_parts = _facet_parts(fespace, parts, mask, plan.multiplicity, coef)
    return cls(fespace=fespace, parts=parts, enc=enc,
               host=_host_tables(fespace, False), zero_range=zero_range,
               num_affine=counts[_GEO_AFFINE],
               num_multilinear=counts[_GEO_MULTILINEAR],
               num_curved=counts[_GEO_POINT], facet_parts=facet_parts,
               keep=None if mask is None else (mask == 0).to(fespace.dtype),
               coefs=coefs, coef_source=(diffusivity, reaction),
               _geo_parts=geo_parts, velocity=velocity, beta=beta,
               velocity_source=velocity_source,
               _layer_plan=(False if coefs is not None or beta is not None
                            else None))

  def split(self, element_mask):
    """Two operators over the elements inside / outside `element_mask` (E,)
    that together equal this one; they share all device data.  Used to apply
    the partition-boundary elements first so that the interface exchange
    overlaps with the interior elements (`distributed/solver.py`)."""
    if any(p.get('colored') for p in self.parts):
      raise NotImplementedError('split() of a coloured operator')
    if self.coefs is not None:
      raise NotImplementedError('split() of an operator with coefficients')
    mask = torch.as_tensor(element_mask, device=self.enc.device).to(torch.bool)
    E = self.enc.shape[0]
    if mask.shape != (E,):
      raise ValueError(f'expected an ({E},) element mask')
    clustered = any(p.get('cluster') is not None for p in self.parts)

    def restrict(part_list, keep):
      parts = []
      for part in part_list:
        part = {k: v for k, v in part.items() if k != 'cluster'}
        if 'elem_list' in part:
          lst = part['elem_list']
          lst = lst[keep[lst.to(torch.int64)]]
        else:
          lst = torch.nonzero(keep).reshape(-1).to(torch.int32)
        if lst.numel():
          new = dict(part, elem_list=lst.contiguous())
          if 'chains' in new:
            new['chains'] = facet_chains(
                self.fespace.mesh.elements, lst.to(torch.int64),
                self.fespace.mesh.gridpoints_1d.num_points, new['chain_len'])
          parts.append(new)
      return parts

    halves = []
    for keep in (mask, ~mask):
      parts = restrict(self.parts, keep)
      if clustered:     # each half clusters its own elements
        parts = _attach_clusters(
            self.fespace, self.enc,
            self.fespace.mesh.assembly_plan().multiplicity, parts)
      facet = (None if self.facet_parts is None
               else restrict(self.facet_parts, keep))
      # (each half covers part of the mesh only: no layer plan)
      geo = (None if self._geo_parts is None
             else restrict(self._geo_parts, keep))
      halves.append(dataclasses.replace(self, parts=parts, facet_parts=facet,
                                        _vector_parts=None, _layer_plan=False,
                                        _diag=None, _diag_adv=None,
                                        _geo_parts=geo))
    return tuple(halves)

  def apply(self, u, lambda0=0.0, lambda1=1.0, out=None, *, zero=True,
            dot_out=None, _transpose=False):
    """u (N,) or (N, nc) -> mask * scatter((l0 B + l1 A)_local(gather(u))).

    `zero=False` skips clearing the shared-node range of `out` (the caller has
    cleared it; used by bench.py to time the kernel alone).  `dot_out`: a
    device tensor of `_lib.SFEM_DOT_SLOTS` doubles that accumulates partial
    sums of `u . out` (CG's p.Ap for free inside the scatter stage).
    """
    mesh = self.fespace.mesh
    if u.shape[0] != mesh.num_nodes:
      raise ValueError(f'expected {mesh.num_nodes} nodal values, got '
                       f'{tuple(u.shape)}')
    if self.coefs is not None:
      _check_scalar_field(u)
      lambda0, lambda1 = _scaled(self.coefs, lambda0, lambda1)
    if self.beta is not None:
      _check_scalar_field(u, 'a velocity takes')
      if dot_out is not None:
        raise NotImplementedError('dot_out of an operator with a velocity')
    u = u.to(self.fespace.dtype)
    if not (u.is_contiguous() or _ops.is_component_major(u)):
      u = u.contiguous()
    if out is None:
      out = torch.empty_like(u)        # same (dense) memory layout as u
    return _ops.helmholtz_apply(
        u, out, self.enc, self._parts_for(u), self.host, mesh.ndim,
        mesh.gridpoints_1d.num_points, lambda0, lambda1,
        self.zero_range if zero else (0, 0), dot_out, transpose=_transpose)

  def apply_transpose(self, u, lambda0=0.0, lambda1=1.0, out=None):
    """`apply` with the advective term transposed: mask * scatter((l0 B_c +
    l1 A_k + C_b)^T_local(gather(u))).  Without a velocity the operator is
    symmetric and this is `apply`.  With a Dirichlet mask the Dirichlet rows
    of the result are zero, as `apply` zeroes them: this is the transpose of
    `apply` on vectors that vanish on the Dirichlet nodes; without a mask it
    is the exact transpose."""
    if self.beta is None:
      return self.apply(u, lambda0, lambda1, out)
    return self.apply(u, lambda0, lambda1, out, _transpose=True)

  def sensitivity(self, u, lam, lambda0=0.0, lambda1=1.0,
                  want=(True, True, True)):
    """The gradient of lam . (A(k, c, b) u), A = lambda0 B_c + lambda1 A_k +
    C_b WITHOUT the Dirichlet mask, with respect to (diffusivity, reaction,
    velocity), each in the form the caller passed to `create`: a scalar gives
    a 0-dim tensor (the sum over all points), (E,) / (E, d) the sum over each
    element's points, (E, n[, d]) per-point values, a (d,) velocity the sum
    over elements and points.  None for a coefficient that was absent or a
    callable, and where `want` is false.  `u`, `lam`: nodal (N,)."""
    return _sensitivity(self, u, lam, lambda0, lambda1, want)

  def layer_plan(self):
    """The `LayerPlan` of this operator's facet launches (made on first use),
    or None: see `build_layer_plan`; `SFEM_LAYERED=0` switches it off."""
    if self._layer_plan is None:
      plan = None
      if (self.facet_parts is not None and
          switches.get('SFEM_LAYERED') != '0'):
        mesh = self.fespace.mesh
        plan = build_layer_plan(self.facet_parts, mesh.num_elements,
                                mesh.num_nodes, mesh.gridpoints_1d.num_points)
      self._layer_plan = plan if plan is not None else False
    return self._layer_plan or None

  def new_extended(self):
    """A zeroed extended output for `apply_layered` (slots that no element
    writes must stay zero: keep one such buffer per consumer)."""
    plan = self.layer_plan()
    return torch.zeros(plan.extent, dtype=self.fespace.dtype,
                       device=self.enc.device)

  def apply_layered(self, u, ext, lambda0=0.0, lambda1=1.0, *, dot_out=None,
                    per_wave=False):
    """`apply` for a scalar field with layered assembly: the unassembled
    contributions go to `ext` (from `new_extended`) as plain stores; the
    assembled value of node i is `ext[i]` plus its layers
    (`_ops.fold_layers(ext, N, plan.layers)`, or inside the consumer:
    `_ops.cg_update_r_layered`).  Dirichlet rows are zero in every layer.
    `per_wave`: `dot_out` has `layered_dot_slots()` doubles and every wave
    stores its share of u . out there (reproducible sum) instead of adding it
    to one of SFEM_DOT_SLOTS slots atomically."""
    plan = self.layer_plan()
    if plan is None:
      raise NotImplementedError('this operator has no layer plan')
    mesh = self.fespace.mesh
    if tuple(u.shape) != (mesh.num_nodes,):
      raise ValueError(f'expected ({mesh.num_nodes},) nodal values, got '
                       f'{tuple(u.shape)}')
    if tuple(ext.shape) != (plan.extent,):
      raise ValueError(f'expected an extended output of {plan.extent} values')
    return _ops.helmholtz_apply_layered(
        u.to(self.fespace.dtype).contiguous(), ext, self.enc, plan.parts,
        self.host, mesh.ndim, mesh.gridpoints_1d.num_points, lambda0, lambda1,
        dot_out, per_wave)

  def layered_dot_slots(self):
    """Waves of one `apply_layered` (size of a per-wave `dot_out`)."""
    mesh = self.fespace.mesh
    return sum(_ops.layered_dot_waves(self.layer_plan().parts,
                                      mesh.gridpoints_1d.num_points,
                                      mesh.num_elements))

  def _parts_for(self, u):
    """Facet-table launches for scalar / component-major fields (the kernels
    address node n of component k at n + k * stride), index rows otherwise."""
    if self.facet_parts is None or not (
        u.dim() == 1 or u.shape[-1] == 1 or _ops.is_component_major(u)):
      return self.parts
    if u.dim() == 1 or u.shape[-1] == 1:
      return self.facet_parts
    # Vector fields walk the chains component by component: the geometry is
    # evaluated once per component, which is nothing for box / affine /
    # multilinear elements (48^3, 3 components: 0.77 / 1.21 ms against 1.47 /
    # 2.63 on index rows) but re-reads the stored factors of curved elements
    # three times (2.57 against 2.10 ms): those stay on the index rows in
    # fp64 and on the one-element facet kernel in fp32 (1.14 against 1.23 /
    # 1.32 ms) -- scripts/sweep_vector_fields.py.
    if self._vector_parts is None:
      if not any(q['geo_mode'] == _GEO_POINT and 'facet_table' in q
                 for q in self.facet_parts):
        self._vector_parts = self.facet_parts
      elif self.fespace.dtype == torch.float64:
        self._vector_parts = (
            [q for q in self.facet_parts if q['geo_mode'] != _GEO_POINT] +
            [q for q in self.parts if q['geo_mode'] == _GEO_POINT])
      else:
        self._vector_parts = [
            {k: v for k, v in q.items() if k != 'chains'}
            if q['geo_mode'] == _GEO_POINT else q for q in self.facet_parts]
    return self._vector_parts

  def diagonal(self, lambda0=0.0, lambda1=1.0, assembled=True):
    """The assembled diagonal (N,) of what `apply(u, lambda0, lambda1)`
    computes: Dirichlet rows 0, shared nodes and periodic images summed as the
    mesh's scatter sums them, and on a partitioned mesh summed over the
    partitions by the exchange (`assembled=False`: this partition's share).
    The element diagonals use the factors of the index-row launches: affine
    / box elements evaluate G and W from their multilinear coefficients, as
    the index-row kernels do, where the facet kernels read per-element
    constants -- the same values up to rounding.  The mass and stiffness
    parts are computed once per operator (`sfem_helmholtz_diag`) and combined
    here."""
    return _diagonal(self, self.keep, None, lambda0, lambda1, assembled)

  def point_weights(self):
    """W = w detJ (E, n) at the operator's points, without coefficients (the
    weights of the coarse-level mean in `linalg/pmg.py`)."""
    return _point_weights(self)

  def apply_local(self, u_local, lambda0=0.0, lambda1=1.0, *,
                  transpose=False):
    """Element-local action (E, n[, nc]) -> (E, n[, nc]); no gather/scatter.
    `transpose`: the advective term transposed (`apply_transpose`)."""
    mesh = self.fespace.mesh
    if self.coefs is not None:
      if u_local.dim() == 3 and u_local.shape[-1] != 1:
        raise NotImplementedError('coefficients take scalar fields')
      lambda0, lambda1 = _scaled(self.coefs, lambda0, lambda1)
    if self.beta is not None and u_local.dim() == 3 and u_local.shape[-1] != 1:
      raise NotImplementedError('a velocity takes scalar fields')
    return _ops.helmholtz_local(
        u_local.to(self.fespace.dtype), self.parts, self.host, mesh.ndim,
        mesh.gridpoints_1d.num_points, lambda0, lambda1,
        transpose=transpose and self.beta is not None)

  def linear_operator(self, lambda0=0.0, lambda1=1.0, transpose=False):
    """`u -> apply(u, lambda0, lambda1)` as an object that `cg` recognises:
    it also offers `apply_with_dot(u, partials)` (fused p.Ap).  With a
    velocity the operator is not symmetric and goes to `linalg.bicgstab`,
    which needs no p.Ap: a plain callable; `transpose=True` then gives
    `u -> apply_transpose(u, lambda0, lambda1)` (without a velocity the
    operator is its own transpose)."""
    if self.beta is not None:
      return _PlainLinearOperator(self, lambda0, lambda1, transpose)
    return FusedLinearOperator(self, lambda0, lambda1)

  def bytes_per_apply(self, lambda0=0.0, ncomp=1, layered=False):
    """Bytes one `apply` HAS to move, launch by launch (what the roofline of
    bench.py divides by): the field in and out once (`2 s N ncomp`), the
    connectivity each launch reads -- 432 bytes per element from a facet
    table (+ 4 per element of a chain list), or `4 n` per element of index
    rows plus `2 S` of sorted shared slots -- and the geometry it reads: 64
    bytes (affine / box constants) or `24 s` (multilinear coefficients) per
    element, `(6 or 7) s n` for elements with stored factors (which
    carry their coefficients folded in).  Coefficients of the other
    elements add `s` (per element) or `s n` (per point) per element each;
    the reaction only with a mass term.  `layered`
    (`apply_layered`): the field in once, and every slot the launches store
    (`LayerPlan.written`: the nodal values plus the further layers of shared
    facets) instead of the field out once."""
    mesh = self.fespace.mesh
    E, n = mesh.elements.shape
    s = 8 if self.fespace.dtype == torch.float64 else 4
    total = 2 * s * mesh.num_nodes * ncomp
    parts = self.facet_parts if self.facet_parts is not None else self.parts
    if layered:
      plan = self.layer_plan()
      total = s * (mesh.num_nodes + plan.written)
      parts = plan.parts
    for part in parts:
      count = part['elem_list'].numel() if 'elem_list' in part else E
      mode = part['geo_mode']
      if 'facet_table' in part:
        conn = 27 * 16 + (4 if 'chains' in part and ncomp == 1 else 0)
      else:
        conn = 4 * n + (4 if 'elem_list' in part else 0)
        if part.get('shared_order') is not None:
          conn += 2 * part['shared_order'].shape[1]
      if mode == _GEO_POINT:
        geo = (7 if lambda0 else 6) * s * n
      elif 'facet_table' in part and mode in (_GEO_AFFINE, _GEO_BOX):
        geo = 8 * s
      else:
        geo = 24 * s
      geo += _coefficient_bytes(part, s, n, lambda0)
      if part.get('beta') is not None:     # the folded velocity
        geo += s * n * mesh.ndim
      total += count * (conn + geo)
    return total

  def kernel_name(self, lambda0=0.0, lambda1=1.0, ncomp=1, layered=False):
    """Name(s) of the kernel instantiation(s) `apply` (`apply_layered`)
    launches, as they appear in a rocprofv3 kernel trace (one per geometry
    kind present)."""
    mesh = self.fespace.mesh
    real = 'double' if self.fespace.dtype == torch.float64 else 'float'
    P = mesh.gridpoints_1d.num_points
    names = []
    parts = (self.layer_plan().parts if layered else
             self.parts if self.facet_parts is None else self.facet_parts)
    for part in parts:
      gm = part['geo_mode']
      names.append(_ops.helmholtz_kernel_name(
          real, P, mesh.ndim, ncomp == 1, gm, part,
          _scaled(self.coefs, lambda0, lambda1)[0] != 0, layered))
    return ' + '.join(sorted(set(names)))


class FusedLinearOperator:
  """Callable operator with a fused `u . A(u)` for `linalg.cg.cg`."""

  def __init__(self, op, lambda0, lambda1):
    self.op, self.lambda0, self.lambda1 = op, lambda0, lambda1
    self._ext = None

  def __call__(self, u):
    return self.op.apply(u, self.lambda0, self.lambda1)

  def apply_with_dot(self, u, partials):
    """Returns A(u) and accumulates partial sums of u . A(u)."""
    return self.op.apply(u, self.lambda0, self.lambda1, dot_out=partials)

  def layer_plan(self):
    """The operator's layer plan if a Krylov iteration gains from it: the
    apply loses its atomics and the clearing of the shared range, the
    `r -= alpha Ap` that adds the layers up reads 0.5 GB more at config 2
    (`scripts/time_layered.py`, ms per CG iteration atomic -> layered: box
    1.556 -> 1.523, multilinear 1.769 -> 1.751, p = 11 fp32 3.249 -> 3.188;
    elements that stream stored factors 2.710 -> 2.738: those keep the
    atomics unless SFEM_LAYERED=force)."""
    plan = self.op.layer_plan()
    if plan is not None and switches.get('SFEM_LAYERED') != 'force' and any(
        q['geo_mode'] == _GEO_POINT for q in plan.parts):
      return None
    return plan

  def apply_layered_with_dot(self, u, partials, per_wave=False):
    """A(u) in layered form (an extended vector owned by this object, see
    `HelmholtzOperator.apply_layered`) + partial sums of u . A(u): for
    consumers that add the layers up themselves (`linalg.cg`)."""
    if self._ext is None:
      self._ext = self.op.new_extended()
    return self.op.apply_layered(u, self._ext, self.lambda0, self.lambda1,
                                 dot_out=partials, per_wave=per_wave)

  def layered_dot_slots(self):
    return self.op.layered_dot_slots()


# ---------------------------------------------------------------------------
# Fused Stokes divergence / pressure gradient (P_N - P_{N-2})
# ---------------------------------------------------------------------------
def supports_fused_stokes(vspace, pspace) -> str | None:
  """None if `sfem_stokes_div` / `sfem_stokes_grad_t` apply, else the reason."""
  why = supports_fused(vspace)
  if why is not None:
    return why
  P = vspace.mesh.gridpoints_1d.num_points
  if P < 4:
    return f'P={P} < 4'
  if pspace.mesh.gridpoints_1d.num_points != P - 2:
    return 'pressure space is not P - 2 points per direction'
  if pspace.interpolator.evalpoints_1d != vspace.mesh.gridpoints_1d:
    return 'pressure quadrature differs from the velocity nodes'
  if pspace.mesh.num_elements != vspace.mesh.num_elements:
    return 'velocity and pressure meshes have different elements'
  # the kernels take w detJ at the quadrature points from the velocity
  # geometry; the reference takes it from the pressure space (:313-320).  The
  # two agree whenever both meshes refine one premesh; checked on a sample of
  # elements (the full factor arrays are never needed by the fused kernels).
  E = vspace.mesh.num_elements
  sample = torch.unique(torch.linspace(
      0, max(E - 1, 0), steps=min(E, 512), device=vspace.device).round().long())
  jv, jp = _sample_jacdets(vspace, sample), _sample_jacdets(pspace, sample)
  # what rounding alone does to det J: the nodal coordinates carry eps |x|,
  # differentiating them over an element of size h with P points amplifies
  # that by ~ P^2 |x| / h (fp32, 40 elements across a unit cube, P = 8: 1.5e-4)
  ndim = vspace.mesh.ndim
  if jv.numel():
    h = 2.0 * float(jv.abs().amax()) ** (1.0 / ndim)
    xmax = float(vspace.mesh.node_coords.abs().amax())
    P = vspace.mesh.gridpoints_1d.num_points
    rounding = 32 * torch.finfo(jv.dtype).eps * P * P * max(xmax / h, 1.0)
  else:
    rounding = 0.0
  tight = 1e-10 if jv.dtype == torch.float64 else 1e-4
  # ... which excuses only elements that ARE images of one premesh in both
  # spaces (affine / multilinear: exact up to that rounding); elements with
  # nodes of their own (curved) must agree tightly, or a pressure geometry that
  # really differs would slip through on fine fp32 meshes.  Tightly, not
  # beyond what rounding does to them too: a quarter of the allowance above.
  # Curved elements of one premesh in fp32, 3 elements across the unit cube,
  # differ by 2.5 .. 3.5 eps P^2 |x| / h at P = 9 .. 12 (1.4e-4 at P = 12,
  # which the fixed 1e-4 alone refused); nothing changes in fp64 or while
  # 8 eps P^2 |x| / h stays below `tight`.
  kind = _cached_geometry_kind(vspace)[sample]
  tol = torch.where(kind != _GEO_POINT, max(tight, rounding),
                    max(tight, rounding / 4)).to(jv.dtype)
  if jv.shape != jp.shape or not bool(
      ((jv - jp).abs() <= tol[:, None] * jv.abs().amax()).all()):
    return 'velocity and pressure spaces carry different geometry'
  return None


def _cached_geometry_kind(fespace):
  """`classify_geometry(fespace)[0]`, kept in the space's cache."""
  cache = fespace._cache
  if 'geometry_kind' not in cache:
    cache['geometry_kind'] = classify_geometry(fespace)[0]
  return cache['geometry_kind']


def _sample_jacdets(space, elements):
  """det J at the quadrature points of the listed elements."""
  mesh = space.mesh
  i1, g1 = space._matrices()
  xe = _ops.gather_rows(mesh.node_coords,
                        mesh.elements[elements].contiguous())
  _, jacdets, _ = _ops.geom_factors(
      xe, i1, g1, mesh.ndim, mesh.gridpoints_1d.num_points,
      space.quadrature.num_points, want_quad_coords=False)
  return jacdets


def shared_slot_order(enc):
  """Per element, the slots of its SHARED non-Dirichlet nodes in ascending
  node order: `(E, S)` int16 (bit pattern of uint16, 0xFFFF padded), S = the
  largest count.  The assembled kernels issue their atomics in this order
  (`sfem_helmholtz_args.shared_order`); None when no slot is shared."""
  E, n = enc.shape
  chunks, smax = [], 0
  step = max(1, (1 << 25) // n)
  for lo in range(0, E, step):
    e64 = enc[lo:lo + step].to(torch.int64)
    ids = e64 & 0x3FFFFFFF
    take = ((e64 & (1 << 30)) != 0) & (e64 >= 0) & (ids != 0x3FFFFFFF)
    key = torch.where(take, ids, torch.full_like(ids, 1 << 40))
    order = torch.argsort(key, dim=1, stable=True)
    count = take.sum(dim=1)
    smax = max(smax, int(count.max()) if count.numel() else 0)
    chunks.append((order, count))
  if smax == 0:
    return None
  out = torch.empty((E, smax), dtype=torch.int16, device=enc.device)
  col = torch.arange(smax, device=enc.device)[None, :]
  at = 0
  for order, count in chunks:
    tab = order[:, :smax].to(torch.int32)
    tab = torch.where(col < count[:, None], tab, torch.full_like(tab, 0xFFFF))
    out[at:at + len(tab)] = tab.to(torch.int16)      # 0xFFFF wraps to -1
    at += len(tab)
  return out.contiguous()


@dataclasses.dataclass(eq=False)
class StokesDivGrad:
  """`D` and `D^T` of navier_stokes/navier_stokes.py:313-338 as one kernel
  each (`sfem_stokes_div`, `sfem_stokes_grad_t`)."""
  vspace: object
  pspace: object
  parts: list
  enc: torch.Tensor               # (E, n) encoded velocity indices
  penc: torch.Tensor | None       # (E, np) pressure node ids; None = identity
  host: dict
  zero_range: tuple
  num_pressure_nodes: int
  dirichlet_u8: torch.Tensor | None = None
  shared_order: torch.Tensor | None = None   # see `shared_slot_order`
  _split: tuple | None = None
  # the launches on compact connectivity + chains (component-major fields,
  # 3D, P = 6..8: `csrc/sfem_stokes_facet.h`), or None
  facet_parts: list | None = None
  _div_parts: list | None = None      # what `div` launches, see `_parts_for`
  _lay: object = None                 # see `_layered_plan`
  _lay_scale: tuple | None = None

  @classmethod
  def create(cls, vspace, pspace, dirichlet_mask=None,
             geometry='auto') -> 'StokesDivGrad':
    why = supports_fused_stokes(vspace, pspace)
    if why is not None:
      raise NotImplementedError(f'fused Stokes kernels unavailable: {why}')
    if geometry not in ('auto', 'multilinear', 'stored'):
      raise ValueError(f'unknown geometry mode {geometry!r}')
    mesh = vspace.mesh
    parts, _, _ = _geometry_parts(vspace, 'kfac', _ops.stokes_setup, geometry,
                                  multilinear=True)
    plan = mesh.assembly_plan()
    mask = None
    if dirichlet_mask is not None:
      mask = torch.as_tensor(dirichlet_mask, device=vspace.device)
      mask = (mask != 0).to(torch.uint8).contiguous()
    enc = _ops.encode_elements(mesh.elements, mask, plan.multiplicity)
    pel = pspace.mesh.elements
    ident = torch.arange(pel.numel(), device=pel.device,
                         dtype=pel.dtype).reshape(pel.shape)
    penc = None if torch.equal(pel, ident) else pel.to(torch.int32).contiguous()
    host = dict(_host_tables(vspace, False),
                interp=pspace.interpolator._interpolation_matrix_1d())
    facet_parts = None
    if (mesh.ndim == 3 and mesh.gridpoints_1d.num_points in STOKES_FACET_P and
        switches.get('SFEM_FACET') != '0' and
        switches.get('SFEM_STOKES_FACET') != '0'):
      facet_parts = cls._facet_parts(mesh, parts, mask, plan.multiplicity)
    return cls(vspace=vspace, pspace=pspace, parts=parts, enc=enc, penc=penc,
               host=host, zero_range=plan.zero_range,
               num_pressure_nodes=pspace.mesh.num_nodes, dirichlet_u8=mask,
               shared_order=cls._order(mesh, enc), facet_parts=facet_parts)

  @staticmethod
  def _facet_parts(mesh, parts, mask, multiplicity):
    """`parts` on the velocity mesh's facet table, every launch a list of chain
    segments (`facet_chains`); elements the table builder refuses keep their
    index rows.  None if no element qualifies."""
    E = mesh.num_elements
    P = mesh.gridpoints_1d.num_points
    tab, ok = _ops.facet_table(mesh.elements, mask, multiplicity, P)
    if not bool(ok.any()):
      return None
    seg_len = chain_segment_length(E)
    if switches.get('SFEM_CHAIN') == '0':
      seg_len = 1
    every = torch.arange(E, device=ok.device)
    use_box = switches.get('SFEM_BOX') != '0'
    out = []
    for part in parts:
      ids = every if 'elem_list' not in part else part['elem_list'].long()
      good = ok[ids]
      box = torch.zeros_like(good)
      if part['geo_mode'] == _GEO_AFFINE and use_box:
        box = good & _diagonal_jacobian(part['geo_elem'][ids])
      for sel, facet, mode in ((ids[box], True, _GEO_BOX),
                               (ids[good & ~box], True, part['geo_mode']),
                               (ids[~good], False, part['geo_mode'])):
        if sel.numel() == 0:
          continue
        new = {k: v for k, v in part.items() if k != 'elem_list'}
        new['geo_mode'] = mode
        if sel.numel() < E:
          new['elem_list'] = sel.to(torch.int32).contiguous()
        if facet:
          new['facet_table'] = tab
          new['chains'] = facet_chains(mesh.elements, sel, P, seg_len)
        out.append(new)
    return out

  def _parts_for(self, field, div=False):
    """Facet / chain launches for component-major fields.  The divergence
    takes them for box elements only: its general-geometry chain kernels hold
    three gathered components next to nine cofactors per point and spill
    (multilinear, 48^3 elements: 1.98 ms against 0.62 for the index-row kernel;
    affine with the fused dot 0.61 against 0.56), while `grad_t`, whose cost is
    the shared-node atomics, gains a quarter from the chains on every geometry
    (`scripts/time_stokes_jitter.py`).  `SFEM_STOKES_FACET_DIV=all` sends the
    divergence through them regardless (tests)."""
    if self.facet_parts is None or not _ops.is_component_major(field):
      return self.parts
    if not div or switches.get('SFEM_STOKES_FACET_DIV') == 'all':
      return self.facet_parts
    if self._div_parts is None:
      # (fp32: the box divergence measures 0.20 against 0.18 ms on index rows
      # at 40^3, so it keeps them too -- scripts/sweep_stokes_facet_vs_rows.py)
      box_ok = self.vspace.dtype == torch.float64
      def rows(q):      # the same elements from their index rows
        q = {k: v for k, v in q.items() if k not in ('facet_table', 'chains')}
        if q['geo_mode'] == _GEO_BOX:
          q['geo_mode'] = _GEO_AFFINE
        return q
      self._div_parts = [
          q if (q['geo_mode'] == _GEO_BOX and box_ok) or
          'facet_table' not in q else rows(q) for q in self.facet_parts]
    return self._div_parts

  @staticmethod
  def _order(mesh, enc):
    if (mesh.ndim == 3 and mesh.gridpoints_1d.num_points <= 8 and
        switches.get('SFEM_SORTED_SCATTER') != '0'):
      return shared_slot_order(enc)
    return None

  def _split_encoding(self):
    """`enc` with every node of the periodic / partition exchange flagged
    SHARED too, and the node range that then needs clearing: what the split
    `E` (`sfem_stokes_e_first` / `_second`) assumes."""
    if self._split is None:
      mesh = self.vspace.mesh
      mult = mesh.assembly_plan().multiplicity.clone()
      ids = []
      gi = mesh.exchange_gather_indices
      if gi is not None and gi.numel():
        ids.append(gi[gi >= 0].to(torch.int64))
      if mesh.neighbor_plan is not None:
        ids.append(mesh.neighbor_plan.interface_nodes(mult.device).to(
            torch.int64))
      if ids:
        idx = torch.cat(ids)
        mult[idx] = torch.clamp(mult[idx], min=2)
      other = torch.nonzero(mult != 1).reshape(-1)
      rng = (int(other.min()), int(other.max()) + 1) if other.numel() else (0, 0)
      enc = _ops.encode_elements(mesh.elements, self.dirichlet_u8, mult)
      self._split = (enc, rng, self._order(mesh, enc))
    return self._split

  def e_apply(self, p, scale=None, exchange=None):
    """(Np,) -> (Np,):  D [ scale * QQ^T (mask * D^T p) ] = `StokesSEM.E` for a
    diagonal Q, with the element-interior velocity nodes kept in registers
    (`sfem_stokes_e_first` / `sfem_stokes_e_second`).  `exchange(w)` applies
    QQ^T in place to the (N, d) component-major intermediate, of which only
    the shared nodes are defined; None on a mesh without periodic images or
    partitions."""
    mesh = self.vspace.mesh
    if self.penc is not None:
      raise NotImplementedError('split E needs element-local pressure nodes')
    if tuple(p.shape) != (self.num_pressure_nodes,):
      raise ValueError(f'expected ({self.num_pressure_nodes},) pressure, got '
                       f'{tuple(p.shape)}')
    from swirl_fem_amd.core import layout
    p = p.to(self.vspace.dtype).contiguous()
    enc, zero_range, order = self._split_encoding()
    w = layout.empty_component_major((mesh.num_nodes, mesh.ndim), p.dtype,
                                     p.device)
    if scale is not None:
      scale = scale.to(p.dtype)
      scale = (scale.contiguous() if scale.dim() == 1
               else _like_layout(scale.expand_as(w), w))
    out = torch.empty(self.num_pressure_nodes, dtype=p.dtype, device=p.device)
    args = (enc, self.penc, self.parts, self.host, mesh.ndim,
            mesh.gridpoints_1d.num_points)
    _ops.stokes_e_first(p, w, out, *args, zero_range, scale, order)
    if exchange is not None:
      w = exchange(w)
    return _ops.stokes_e_second(w, out, *args, scale)

  # Layered D^T inside E (index-row kernels: 2D, and 3D outside the facet
  # kernels' range).  The scatter of `sfem_stokes_grad_t` waits on the
  # memory-side atomic unit as soon as a launch has enough elements (an
  # ensemble of 8 Kolmogorov flows: 1.17 M requests in 72 us, 16 G/s).  The
  # kernel needs no change to lose them: a second index row per element in
  # which every (element, slot) writer of a shared node has a position of its
  # OWN -- the first writer keeps the node, the others get positions behind
  # the N nodes -- and no SHARED flag, so every slot takes the kernel's
  # plain-store branch (nothing to clear either).  The sums are then formed by
  # the class kernel that applies QQ^T to periodic images anyway
  # (`sfem_exchange_classes`): a class is all positions of all images of a
  # node.  `sfem_stokes_div` reads the first N positions of each component.
  def _layered_plan(self):
    """None, or (enc, n_ext, node_of_pos, members, offsets, num_classes)."""
    if self._lay is None:
      mesh = self.vspace.mesh
      ok = (self.facet_parts is None and mesh.axis_name is None and
            mesh.neighbor_plan is None and
            mesh.elements.numel() <= (1 << 28))
      self._lay = self._build_layered(mesh) if ok else False
    return self._lay or None

  def _build_layered(self, mesh):
    dev = mesh.device
    N = mesh.num_nodes
    el = mesh.elements.to(torch.int64).reshape(-1)
    order = torch.argsort(el, stable=True)
    ids = el[order]
    first = torch.ones_like(ids, dtype=torch.bool)
    first[1:] = ids[1:] != ids[:-1]
    extra = ~first
    pos_sorted = torch.where(first, ids, N + torch.cumsum(extra, 0) - 1)
    pos = torch.empty_like(el)
    pos[order] = pos_sorted
    n_ext = N + int(extra.sum())
    if n_ext >= _lib_idx_mask():
      return False
    node_of_pos = torch.cat([torch.arange(N, device=dev), ids[extra]])
    pos32 = pos.to(torch.int32)
    dirichlet = self.enc.reshape(-1) < 0           # SFEM_IDX_DIRICHLET: bit 31
    enc = torch.where(dirichlet, pos32 | torch.tensor(
        -2 ** 31, dtype=torch.int32, device=dev), pos32).reshape(
            self.enc.shape).contiguous()
    # classes: positions of one node and of its periodic images
    key = torch.arange(N, device=dev)
    gi, ui = mesh.exchange_gather_indices, mesh.exchange_unique_indices
    if gi is not None and gi.numel() and ui is not None:
      g = gi.to(torch.int64)
      u = torch.as_tensor(np.asarray(ui).astype(np.int64), device=dev)
      keep = g >= 0
      key[g[keep]] = N + u[keep]
    pkey = key[node_of_pos]
    korder = torch.argsort(pkey, stable=True)
    _, counts = torch.unique_consecutive(pkey[korder], return_counts=True)
    big = counts > 1
    members = korder[torch.repeat_interleave(big, counts)]
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev),
                         torch.cumsum(counts[big], 0)])
    return (enc, n_ext, node_of_pos, members.to(torch.int32).contiguous(),
            offsets.to(torch.int32).contiguous(), int(big.sum()))

  def supports_layered_e(self) -> bool:
    return self._layered_plan() is not None

  def e_layered(self, p, scale=None, dot_with=None, dot_out=None):
    """(Np,) -> (Np,):  D [ QQ^T ( scale * mask * D^T p ) ]  = `StokesSEM.E`
    for a diagonal Q, the direct-stiffness sum of D^T without atomics (see
    `_layered_plan`); periodic images included, one partition."""
    plan = self._layered_plan()
    if plan is None:
      raise NotImplementedError(
          'layered E needs index-row launches on one partition (no facet '
          'launches, positions within the index range)')
    enc, n_ext, node_of_pos, members, offsets, num_classes = plan
    mesh = self.vspace.mesh
    if tuple(p.shape) != (self.num_pressure_nodes,):
      raise ValueError(f'expected ({self.num_pressure_nodes},) pressure, got '
                       f'{tuple(p.shape)}')
    from swirl_fem_amd.core import layout
    p = p.to(self.vspace.dtype).contiguous()
    w = layout.empty_component_major((n_ext, mesh.ndim), p.dtype, p.device)
    if scale is not None:
      if self._lay_scale is None or self._lay_scale[0] is not scale:
        ext = scale.to(p.dtype).index_select(0, node_of_pos)
        ext = (ext.contiguous() if ext.dim() == 1
               else _like_layout(ext.expand_as(w), w))
        self._lay_scale = (scale, ext)
      scale = self._lay_scale[1]
    P = mesh.gridpoints_1d.num_points
    _ops.stokes_grad_t(p, w, enc, self.penc, self.parts, self.host, mesh.ndim,
                       P, (0, 0), None, scale)
    _ops.exchange_classes_(w, members, offsets, num_classes)
    out = (torch.empty if self.penc is None else torch.zeros)(
        self.num_pressure_nodes, dtype=p.dtype, device=p.device)
    if dot_out is not None:
      dot_with = dot_with.to(p.dtype).contiguous()
    return _ops.stokes_div(w, out, self.enc, self.penc, self.parts, self.host,
                           mesh.ndim, P, None, dot_with, dot_out)

  def div(self, u, scale=None, out=None, dot_with=None, dot_out=None):
    """(N, d) -> (Np,):  D (scale * u); `scale` is (N, d) or (N,).
    `dot_out`: SFEM_DOT_SLOTS doubles accumulating `dot_with . result`."""
    mesh = self.vspace.mesh
    if tuple(u.shape) != (mesh.num_nodes, mesh.ndim):
      raise ValueError(f'expected ({mesh.num_nodes}, {mesh.ndim}) velocity, '
                       f'got {tuple(u.shape)}')
    u = u.to(self.vspace.dtype)
    if not (u.is_contiguous() or _ops.is_component_major(u)):
      u = u.contiguous()
    if scale is not None:
      scale = scale.to(u.dtype)
      if scale.dim() == 1:           # one factor per node for all components
        scale = scale.contiguous()
      else:
        scale = _like_layout(scale.expand_as(u), u)
    if out is None:
      # pressure nodes that no element references (none on refiner meshes)
      out = (torch.empty if self.penc is None else torch.zeros)(
          self.num_pressure_nodes, dtype=u.dtype, device=u.device)
    if dot_out is not None:
      dot_with = dot_with.to(u.dtype).contiguous()
      if tuple(dot_with.shape) != (self.num_pressure_nodes,):
        raise ValueError('dot_with must be a pressure vector')
    return _ops.stokes_div(u, out, self.enc, self.penc,
                           self._parts_for(u, div=True),
                           self.host, mesh.ndim, mesh.gridpoints_1d.num_points,
                           scale, dot_with, dot_out)

  def grad_t(self, p, out=None, component_major=False, scale=None):
    """(Np,) -> (N, d):  mask * (scale * D^T p), the factor applied to every
    element's contribution before assembly (it must be equal on all copies
    of a node; then it commutes with the direct-stiffness sum and QQ^T)."""
    mesh = self.vspace.mesh
    if tuple(p.shape) != (self.num_pressure_nodes,):
      raise ValueError(f'expected ({self.num_pressure_nodes},) pressure, got '
                       f'{tuple(p.shape)}')
    p = p.to(self.vspace.dtype).contiguous()
    if out is None:
      shape = (mesh.num_nodes, mesh.ndim)
      if component_major:
        from swirl_fem_amd.core import layout
        out = layout.empty_component_major(shape, p.dtype, p.device)
      else:
        out = torch.empty(shape, dtype=p.dtype, device=p.device)
    if scale is not None:
      scale = scale.to(p.dtype)
      scale = (scale.contiguous() if scale.dim() == 1
               else _like_layout(scale.expand_as(out), out))
    return _ops.stokes_grad_t(p, out, self.enc, self.penc,
                              self._parts_for(out), self.host, mesh.ndim,
                              mesh.gridpoints_1d.num_points, self.zero_range,
                              self.shared_order, scale)


def _lib_idx_mask():
  from swirl_fem_amd import _lib
  return _lib.SFEM_IDX_MASK


def _diagonal_jacobian(coef):
  """(E,) bool: rows of the (E, 24) multilinear coefficients whose map is
  x_c = x0_c + h_c * xi_c (axis-aligned boxes in the element's own axis order):
  the Stokes kernels then need one derivative per component
  (`SFEM_GEO_BOX`)."""
  lin = coef[:, :9].reshape(-1, 3, 3)            # d x_c / d xi_k at [k, c]
  diag = torch.diagonal(lin, dim1=1, dim2=2).abs()
  scale = diag.max(dim=1).values
  tol = BOX_TOL[coef.dtype] * scale
  off = lin.abs() * (1 - torch.eye(3, dtype=coef.dtype, device=coef.device))
  higher = coef[:, 9:21].abs().max(dim=1).values
  return ((off.reshape(-1, 9).max(dim=1).values <= tol) & (higher <= tol) &
          (diag.min(dim=1).values > 0))


def _like_layout(t, ref):
  """`t` (same shape as `ref`) materialised in the memory layout of `ref`."""
  if t.stride() == ref.stride() and (t.is_contiguous() or
                                     _ops.is_component_major(t)):
    return t
  out = torch.empty_like(ref)        # preserves the dense layout of ref
  out.copy_(t)
  return out


# ---------------------------------------------------------------------------
# Helmholtz operator with a quadrature that differs from the nodes
# ---------------------------------------------------------------------------
def _assembled_diagonal(fespace, parts, host, keep, bmat):
  """(diag B, diag A) of a fused operator on this partition, (N,) each:
  element diagonals from `sfem_helmholtz_diag`, summed per node in ascending
  slot order by `sfem_scatter_csr` (deterministic: no atomics), Dirichlet
  rows zeroed.  `bmat` (Q, P): the interpolation of a two-grid operator."""
  mesh = fespace.mesh
  P = mesh.gridpoints_1d.num_points
  dq = np.asarray(host['dmat'], dtype=np.float64)
  dtil = dq if bmat is None else dq @ bmat
  mass, stiff = _ops.helmholtz_diag(
      parts, mesh.num_elements, mesh.ndim, P, dtil, host['weights'],
      host['nodes'], bmat, dtype=fespace.dtype, device=fespace.device)
  offsets, slots = mesh.assembly_plan().csr()
  out = []
  for loc in (mass, stiff):
    d = _ops.scatter_csr(loc.reshape(-1), offsets, slots, mesh.num_nodes)
    if keep is not None:
      d = d * keep
    out.append(d)
  return tuple(out)


def _combine_diagonal(parts, lambda0, lambda1, assembled, mesh):
  """lambda0 diag B + lambda1 diag A; summed over the partitions (the mesh's
  exchange, a collective) when `assembled` and the mesh is partitioned."""
  mass, stiff = parts
  if lambda0 == 0.0:
    d = stiff * lambda1
  elif lambda1 == 0.0:
    d = mass * lambda0
  else:
    d = mass * lambda0 + stiff * lambda1
  if assembled and (mesh.axis_name is not None or
                    mesh.neighbor_plan is not None):
    d = mesh.exchange(d)
  return d


def _diagonal(op, keep, interpolator, lambda0, lambda1, assembled):
  """`diagonal` of both operator classes.  `keep` (N,) zeroes the Dirichlet
  rows; `interpolator`: that of a two-grid operator, whose (Q, P) matrix
  enters the element diagonals, None for a collocated one.  The parts that
  no lambda scales are computed once and kept on `op`."""
  fes = op.fespace
  bmat = lambda: None if interpolator is None else np.asarray(
      interpolator._interpolation_matrix_1d(), dtype=np.float64)
  if op._diag is None:
    op._diag = _assembled_diagonal(fes, op.parts, op.host, keep, bmat())
  lambda0, lambda1 = _scaled(op.coefs, lambda0, lambda1)
  d = _combine_diagonal(op._diag, lambda0, lambda1, assembled, fes.mesh)
  if op.beta is not None:      # + diag C_b, which no lambda scales
    if op._diag_adv is None:
      op._diag_adv = _advection_diagonal(fes, op.parts, op.beta,
                                         op.host['dmat'], keep, bmat())
    d = d + op._diag_adv
  return d


def _point_weights(op):
  """`point_weights` of both operator classes: the mass diagonal of the
  launches without coefficients on the grid of `op.host`."""
  fes, host = op.fespace, op.host
  mass, _ = _ops.helmholtz_diag(
      op._geo_parts or op.parts, fes.mesh.num_elements, fes.mesh.ndim,
      len(host['nodes']), host['dmat'], host['weights'], host['nodes'], None,
      want_stiff=False, dtype=fes.dtype, device=fes.device)
  return mass


def supports_two_grid(fespace) -> str | None:
  """None if `TwoGridHelmholtzOperator` applies, else the reason."""
  mesh = fespace.mesh
  q = fespace.quadrature.num_points
  if mesh.ndim not in (2, 3):
    return f'ndim={mesh.ndim}'
  if not 2 <= q <= MAX_FUSED_P:
    return f'q={q} outside 2..{MAX_FUSED_P}'
  d = _quadrature_dmat(fespace)
  if not np.allclose(d[::-1, ::-1], -d, rtol=0,
                     atol=1e-12 * max(1.0, np.abs(d).max())):
    return 'quadrature points are not symmetric about 0'
  return None


def _quadrature_dmat(fespace):
  """Differentiation matrix of the Lagrange basis ON the quadrature points."""
  from swirl_fem_amd.core.interpolation import BarycentricInterpolator
  qn = fespace.quadrature.nodes
  return BarycentricInterpolator(ndim=fespace.mesh.ndim, gridpoints_1d=qn,
                                 evalpoints_1d=qn)._differentiation_matrix_1d()


@dataclasses.dataclass(eq=False)
class TwoGridHelmholtzOperator:
  """`mask * scatter((l0 B + l1 A)_local(gather(u)))` when the quadrature is
  not the node set (the reference's Poisson example integrates with
  `order + (ndim+1)//2` Gauss points, examples/poisson.py:112-114).

  With I the (Q, n) interpolation to the quadrature points,
  `A_local = I^T A_q I` where `A_q` is the *collocated* operator of the
  Lagrange basis on the quadrature points (the gradient of the interpolant is
  exact there because q >= P).  So the element work is: interpolate
  (`sfem_basis_eval`), the fused element-local kernel on the q-grid
  (`sfem_helmholtz_local` with the q-point differentiation matrix, weights and
  nodes; geometry of multilinear elements evaluated in registers), transposed
  interpolation (`sfem_basis_eval_t`).  Replaces the generic chain basis_eval
  (values + physical gradients) -> pointwise form -> basis_eval_t."""
  fespace: object
  parts: list
  host: dict
  mask: torch.Tensor | None        # (N,) 1 inside, 0 on Dirichlet nodes
  _diag: tuple | None = None       # assembled (diag B, diag A), `diagonal`
  # variable coefficients at the Q^d quadrature points, as in
  # `HelmholtzOperator`
  coefs: tuple | None = None
  coef_source: tuple = (None, None)
  _geo_parts: list | None = None
  # advective term, as in `HelmholtzOperator` (at the Q^d quadrature points)
  velocity: torch.Tensor | None = None
  beta: torch.Tensor | None = None
  _diag_adv: torch.Tensor | None = None
  velocity_source: object = None

  @classmethod
  def create(cls, fespace, dirichlet_mask=None, geometry='auto', *,
             diffusivity=None, reaction=None,
             velocity=None) -> 'TwoGridHelmholtzOperator':
    """`diffusivity`, `reaction`, `velocity`: see `HelmholtzOperator.create`;
    per-point values and callables live on the Q^d quadrature points.  The
    advective term is I^T C_q I with C_q the collocated term of the q-grid:
    the q-grid kernel adds beta . (derivatives of the interpolant)."""
    why = supports_two_grid(fespace)
    if why is not None:
      raise NotImplementedError(f'two-grid Helmholtz unavailable: {why}')
    if geometry not in ('auto', 'stored'):
      raise ValueError(f'unknown geometry mode {geometry!r}')
    mesh = fespace.mesh
    geo_parts, _, _ = _geometry_parts(fespace, 'geo', _ops.helmholtz_setup,
                                      geometry, corners=True)
    # the values-only interpolation of the element coordinates, not
    # `quad_coords` (which builds the whole geometry)
    points = lambda: fespace._interpolate(mesh.element_coords())
    velocity_source = velocity
    coefs, velocity, beta, parts = _coefficient_intake(
        fespace, 'atomic', fespace.quadrature.num_points ** mesh.ndim, points,
        geo_parts, diffusivity, reaction, velocity)
    mask = None
    if dirichlet_mask is not None:
      mask = (torch.as_tensor(dirichlet_mask, device=fespace.device) == 0).to(
          fespace.dtype)
    return cls(fespace=fespace, parts=parts, host=_host_tables(fespace, True),
               mask=mask, coefs=coefs, coef_source=(diffusivity, reaction),
               _geo_parts=geo_parts, velocity=velocity, beta=beta,
               velocity_source=velocity_source)

  def point_weights(self):
    """W = w detJ (E, Q^d) at the quadrature points, without coefficients."""
    return _point_weights(self)

  def apply_local(self, u_local, lambda0=0.0, lambda1=1.0, *,
                  transpose=False):
    """(E, n[, nc]) -> (E, n[, nc]).  `transpose`: I^T (A_q)^T I, the
    advective term of the q-grid kernel transposed."""
    fes = self.fespace
    scalar = u_local.dim() == 2
    u3 = (u_local[..., None] if scalar else u_local).to(fes.dtype)
    nc = u3.shape[-1]
    if self.coefs is not None:
      if nc != 1:
        raise NotImplementedError('coefficients take scalar fields')
      lambda0, lambda1 = _scaled(self.coefs, lambda0, lambda1)
    if self.beta is not None and nc != 1:
      raise NotImplementedError('a velocity takes scalar fields')
    rq = _ops.helmholtz_local(
        fes._interpolate(u3).contiguous(), self.parts, self.host,
        fes.mesh.ndim, fes.quadrature.num_points, lambda0, lambda1,
        transpose=transpose and self.beta is not None)
    r3 = fes._interpolate_t(rq)
    return r3[..., 0] if scalar else r3

  def apply(self, u, lambda0=0.0, lambda1=1.0, *, _transpose=False):
    """u (N,) or (N, nc) -> mask * scatter(local(gather(u)))."""
    mesh = self.fespace.mesh
    if u.shape[0] != mesh.num_nodes:
      raise ValueError(f'expected {mesh.num_nodes} nodal values, got '
                       f'{tuple(u.shape)}')
    u = u.to(self.fespace.dtype)
    if u.dim() == 1:
      out = mesh.scatter(self.apply_local(mesh.gather(u), lambda0, lambda1,
                                          transpose=_transpose))
      return out if self.mask is None else out * self.mask
    loc = self.apply_local(_ops.gather_rows(u.contiguous(), mesh.elements),
                           lambda0, lambda1)
    out = _ops.scatter_add(loc, mesh.elements, mesh.num_nodes, ncomp=u.shape[1])
    return out if self.mask is None else out * self.mask[:, None]

  def apply_transpose(self, u, lambda0=0.0, lambda1=1.0):
    """`apply` with the advective term transposed, I^T (A_q)^T I element by
    element; see `HelmholtzOperator.apply_transpose` for the mask."""
    return self.apply(u, lambda0, lambda1,
                      _transpose=self.beta is not None)

  def sensitivity(self, u, lam, lambda0=0.0, lambda1=1.0,
                  want=(True, True, True)):
    """`HelmholtzOperator.sensitivity` at the Q^d quadrature points: `u` and
    `lam` (N,) are interpolated there."""
    return _sensitivity(self, u, lam, lambda0, lambda1, want)

  def linear_operator(self, lambda0=0.0, lambda1=1.0, transpose=False):
    if transpose:
      return lambda u: self.apply_transpose(u, lambda0, lambda1)
    return lambda u: self.apply(u, lambda0, lambda1)

  def diagonal(self, lambda0=0.0, lambda1=1.0, assembled=True):
    """The assembled diagonal of `apply(u, lambda0, lambda1)` (N,), see
    `HelmholtzOperator.diagonal`: the element diagonals of I^T H_q I with
    I the (Q, P) interpolation and D_q I its derivative."""
    return _diagonal(self, self.mask, self.fespace.interpolator, lambda0,
                     lambda1, assembled)


# ---------------------------------------------------------------------------
# Over-integrated convection
# ---------------------------------------------------------------------------
def _grid_geometry_parts(fespace, point_setup, geometry='auto'):
  """The launches (`_geometry_parts`) of the cofactor kernels that work on the
  quadrature grid of `fespace`."""
  return _geometry_parts(fespace, 'kfac', point_setup, geometry,
                         corners=True)[0]


@dataclasses.dataclass(eq=False)
class ConvectionOperator:
  """`C_local(u)_{i,c} = int phi_i u_j d_j u_c` on the over-integration space
  (navier_stokes.py:238-245) as: interpolate the nodal velocity to the
  quadrature grid (`sfem_basis_eval`), one fused kernel there
  (`sfem_stokes_convect_local`: collocated derivative lines, cofactor
  geometry, contravariant velocity, product), transposed interpolation
  (`sfem_basis_eval_t`).  Nothing of size (E, Q, d, d) is ever stored."""
  fespace: object
  parts: list
  host: dict

  @classmethod
  def create(cls, fespace, geometry='auto') -> 'ConvectionOperator':
    why = supports_two_grid(fespace)
    q = fespace.quadrature.num_points
    if why is None and q < 4:
      why = f'q={q} < 4'
    if why is not None:
      raise NotImplementedError(f'fused convection unavailable: {why}')
    parts = _grid_geometry_parts(fespace, _ops.stokes_setup, geometry)
    return cls(fespace=fespace, parts=parts, host=_host_tables(fespace, True))

  def apply_local(self, u_local):
    """(E, n, d) nodal velocity -> (E, n, d) local convection covector."""
    fes = self.fespace
    uq = fes._interpolate(u_local.to(fes.dtype))
    cq = _ops.stokes_convect_local(uq, self.parts, self.host, fes.mesh.ndim,
                                   fes.quadrature.num_points)
    return fes._interpolate_t(cq)


# ---------------------------------------------------------------------------
# Scalar transport: the explicit right-hand side of a BDF/EXT step
# ---------------------------------------------------------------------------
@dataclasses.dataclass(eq=False)
class TransportRhs:
  """`sum_j (m_j B T_j + c_j C(u_j) T_j) + B s` for up to three time levels
  in one pass: B the mass matrix, `C(u)[i,k] = sum_q W_q phi_i(q) u_q . grad
  phi_k(q)` the convective form of `TwoGridHelmholtzOperator`.
  Interpolate each level's scalar and nodal velocity to the quadrature grid
  (`sfem_basis_eval`, d + 1 components), one fused kernel there
  (`sfem_transport_rhs`: collocated derivative lines, cofactor geometry,
  contravariant velocity, product, mass terms), transposed interpolation
  (`sfem_basis_eval_t`).  No folded velocity (E, Q^d, d) is built."""
  fespace: object
  parts: list
  host: dict
  _wdet: torch.Tensor | None = None

  @classmethod
  def create(cls, fespace, geometry='auto') -> 'TransportRhs':
    why = supports_two_grid(fespace)
    if why is not None:
      raise NotImplementedError(f'fused transport unavailable: {why}')
    parts = _grid_geometry_parts(fespace, _ops.stokes_setup, geometry)
    return cls(fespace=fespace, parts=parts, host=_host_tables(fespace, True))

  def point_weights(self):
    """W = w detJ (E, Q^d), what `TwoGridHelmholtzOperator.point_weights`
    returns."""
    if self._wdet is None:
      self._wdet = self.fespace.wdet()
    return self._wdet

  def apply_local(self, levels, source_q=None):
    """`levels`: tuples (T_q (E, Q^d), u_q (E, Q^d, d) or None, mass_coef,
    conv_coef) on the quadrature grid -> (E, Q^d), the integrand times W."""
    fes = self.fespace
    levels = list(levels)
    if autodiff.needs_grad(source_q, *[t for l in levels for t in l[:2]]):
      return autodiff.transport_rhs_local(self, levels, source_q)
    mass = source_q is not None or any(float(l[2]) != 0.0 for l in levels)
    return _ops.transport_rhs(
        levels, self.parts, self.host, fes.mesh.ndim,
        fes.quadrature.num_points, source=source_q,
        wdet=self.point_weights() if mass else None)

  def _point_velocity(self, u):
    """A level's velocity that needs no interpolation as (E, Q^d, d), or
    None for nodal values."""
    fes = self.fespace
    mesh = fes.mesh
    E, d = mesh.num_elements, mesh.ndim
    nq = fes.quadrature.num_points ** d
    u = torch.as_tensor(u, dtype=fes.dtype, device=fes.device)
    if tuple(u.shape) == (d,):
      return u[None, None, :].expand(E, nq, d).contiguous()
    if tuple(u.shape) == (E, nq, d):
      return u
    if tuple(u.shape) == (mesh.num_nodes, d):
      return None
    raise ValueError(f'velocity: shape {tuple(u.shape)}; expected ({d},), '
                     f'({mesh.num_nodes}, {d}) or ({E}, {nq}, {d})')

  def apply(self, levels, source=None):
    """`levels`: tuples (T (N,), u, mass_coef, conv_coef) with `u` nodal (N, d)
    in any strides, a (d,) constant, (E, Q^d, d) point values or None;
    `source`: None, (N,) nodal or (E, Q^d) point values.  Returns the
    assembled (N,) vector  B s + sum_j (m_j B + c_j C(u_j)) T_j."""
    fes = self.fespace
    mesh = fes.mesh
    d = mesh.ndim
    nq = fes.quadrature.num_points ** d

    levels = list(levels)
    # under autograd the gather and the transposed interpolation take the
    # routes that carry their transposes; `_basis` and `scatter` switch alone
    grad = autodiff.needs_grad(source, *[t for l in levels for t in l[:2]])
    gather_rows = autodiff.gather_rows if grad else _ops.gather_rows

    def at_points(nodal):      # (N, nc) -> (E, Q^d, nc)
      return fes._interpolate(gather_rows(nodal.contiguous(), mesh.elements))
    local = []
    for T, u, mc, cc in levels:
      T = torch.as_tensor(T, dtype=fes.dtype, device=fes.device)
      if tuple(T.shape) != (mesh.num_nodes,):
        raise ValueError(f'expected ({mesh.num_nodes},) nodal values, got '
                         f'{tuple(T.shape)}')
      uq = None if u is None else self._point_velocity(u)
      if u is not None and uq is None and float(cc) != 0.0:
        u = torch.as_tensor(u, dtype=fes.dtype, device=fes.device)
        both = at_points(torch.cat([T[:, None], u], dim=1))
        Tq, uq = both[..., 0].contiguous(), both[..., 1:].contiguous()
      else:
        Tq = at_points(T[:, None])[..., 0].contiguous()
      local.append((Tq, uq, mc, cc))
    sq = None
    if source is not None:
      s = torch.as_tensor(source, dtype=fes.dtype, device=fes.device)
      if tuple(s.shape) == (mesh.num_elements, nq):
        sq = s
      elif tuple(s.shape) == (mesh.num_nodes,):
        sq = at_points(s[:, None])[..., 0].contiguous()
      else:
        raise ValueError(f'source: shape {tuple(s.shape)}; expected '
                         f'({mesh.num_nodes},) or ({mesh.num_elements}, {nq})')
    rq = self.apply_local(local, sq)
    return mesh.scatter(fes._interpolate_t(rq[..., None], grad)[..., 0])


# ---------------------------------------------------------------------------
# Linear elasticity
# ---------------------------------------------------------------------------
def lame_parameters(youngs_modulus, poisson_ratio, plane_stress=False):
  """(lambda, mu) of an isotropic material from Young's modulus E and
  Poisson's ratio nu: mu = E / (2 (1 + nu)), lambda = E nu / ((1 + nu)
  (1 - 2 nu)).  `plane_stress`: the modified lambda = 2 lambda mu / (lambda +
  2 mu) = E nu / (1 - nu^2) with which the 2D (plane-strain) operator solves
  the plane-stress problem."""
  E, nu = youngs_modulus, poisson_ratio
  mu = E / (2.0 * (1.0 + nu))
  lam = E * nu / ((1.0 + nu) * (1.0 - 2.0 * nu))
  if plane_stress:
    lam = 2.0 * lam * mu / (lam + 2.0 * mu)
  return lam, mu


def von_mises(sigma, ndim):
  """The von Mises stress of `sigma` (..., NV) in the Voigt slots of
  `ElasticityOperator.stress`: NV = 6, (xx, yy, zz, xy, xz, yz) for ndim 3;
  NV = 4, (xx, yy, xy, zz) for ndim 2.  Plain torch arithmetic on the last
  axis, so autograd differentiates it; the gradient does not exist where the
  result is zero (a square root at zero): use `von_mises(...) ** 2` or a
  p-norm in an objective that can reach it."""
  nv = {2: 4, 3: 6}.get(ndim)
  if nv is None or sigma.shape[-1] != nv:
    raise ValueError(f'von_mises: ndim={ndim} takes {nv} stress slots on the '
                     f'last axis, got shape {tuple(sigma.shape)}')
  if ndim == 3:
    sxx, syy, szz, sxy, sxz, syz = sigma.unbind(-1)
    shear = sxy ** 2 + sxz ** 2 + syz ** 2
  else:
    sxx, syy, sxy, szz = sigma.unbind(-1)
    shear = sxy ** 2
  return torch.sqrt(0.5 * ((sxx - syy) ** 2 + (syy - szz) ** 2 +
                           (szz - sxx) ** 2) + 3.0 * shear)


_von_mises = von_mises   # `ElasticityOperator.stress` has a flag of that name


def _elastic_coefficient(fespace, value, name, positive):
  """A coefficient of the elasticity family as its kernels read it: a float,
  or an (E, Q^d) tensor (per-element values are expanded here: the kernels
  read per-point arrays only)."""
  if value is None:
    raise ValueError(f'{name} is required')
  mesh = fespace.mesh
  E = mesh.num_elements
  npts = fespace.quadrature.num_points ** mesh.ndim
  points = lambda: fespace._interpolate(mesh.element_coords())
  c = coefficient(value, name, E, npts, points, fespace.dtype, fespace.device,
                  positive)
  if isinstance(c, tuple):
    mode, t = c
    from swirl_fem_amd import _lib
    if mode == _lib.COEF_ELEM:
      t = t[:, None].expand(E, npts)
    return t.contiguous()
  return c


class _DisplacementOperator:
  """Intake and assembly of nodal displacements (N, d) for an operator with a
  `fespace` and a `mask`; the refusals carry the subclass's name."""

  def _to_grid(self, u_local):
    """(E, n, d) element values -> (E, Q^d, d) on the quadrature grid."""
    fes = self.fespace
    if autodiff.needs_grad(u_local):
      raise NotImplementedError(f'autograd through {type(self).__name__}')
    d = fes.mesh.ndim
    if u_local.dim() != 3 or u_local.shape[-1] != d:
      raise ValueError(f'expected (E, n, {d}) local values, got '
                       f'{tuple(u_local.shape)}')
    return fes._interpolate(u_local.to(fes.dtype)).contiguous()

  def _nodal(self, u):
    mesh = self.fespace.mesh
    if tuple(u.shape) != (mesh.num_nodes, mesh.ndim):
      raise ValueError(f'expected ({mesh.num_nodes}, {mesh.ndim}) nodal '
                       f'displacements, got {tuple(u.shape)}')
    if autodiff.needs_grad(u):
      raise NotImplementedError(f'autograd through {type(self).__name__}')
    return _ops.gather_rows(u.to(self.fespace.dtype).contiguous(),
                            mesh.elements)

  def _assembled(self, u, local):
    """mask * scatter(local(gather(u))) in the layout of `u`."""
    mesh = self.fespace.mesh
    loc = local(self._nodal(u))
    out = _ops.scatter_add(loc, mesh.elements, mesh.num_nodes, ncomp=mesh.ndim)
    if self.mask is not None:
      out = out * self.mask
    return _like_layout(out, u) if u.dtype == out.dtype else out


@dataclasses.dataclass(eq=False)
class ElasticityOperator(_DisplacementOperator):
  """`K u + lambda0 M_rho u` for displacements u (N, d), with `v^T K u = int
  sigma(u) : grad v`, sigma = lambda tr(eps) I + 2 mu eps (plane strain in
  2D) and M_rho the mass matrix with density rho.  Interpolate
  the element's displacement to the quadrature grid (`sfem_basis_eval`, d
  components), one fused kernel there (`sfem_elasticity_local`: collocated
  derivative lines, cofactor geometry, stress, transposed derivative lines,
  mass term), transposed interpolation (`sfem_basis_eval_t`).  Nothing of
  size (E, Q^d, d, d) is stored.  `lam`, `mu`, `rho`: a float or an (E, Q^d)
  tensor each; `mask` (N, d): 0 on the fixed components."""
  fespace: object
  parts: list
  host: dict
  lam: object
  mu: object
  rho: object
  mask: torch.Tensor | None = None
  _wdet: torch.Tensor | None = None
  _diag: tuple | None = None
  _lumped: torch.Tensor | None = None
  # (lame_lambda, lame_mu, density) as the caller passed them: `sensitivity`
  # returns its gradients in these forms
  coef_source: tuple = (None, None, None)

  @classmethod
  def create(cls, fespace, dirichlet_mask=None, *, lame_lambda, lame_mu,
             density=None, geometry='auto') -> 'ElasticityOperator':
    return cls._intake(fespace, dirichlet_mask, lame_lambda, lame_mu, density,
                       geometry, 'ElasticityOperator', 'fused elasticity')

  @classmethod
  def _intake(cls, fespace, dirichlet_mask, lame_lambda, lame_mu, density,
              geometry, who, what):
    """The body of `create`, shared with `HyperelasticOperator.create`: `who`
    and `what` name the operator in the refusals."""
    mesh = fespace.mesh
    if mesh.axis_name is not None or mesh.neighbor_plan is not None:
      raise NotImplementedError(f'{who} on a partitioned mesh')
    if mesh._cache.get('replicas', 1) > 1:
      raise NotImplementedError(f'{who} on an ensemble (Mesh.replicate)')
    why = supports_two_grid(fespace)
    if why is not None:
      raise NotImplementedError(f'{what} unavailable: {why}')
    if geometry not in ('auto', 'stored'):
      raise ValueError(f'unknown geometry mode {geometry!r}')
    d = mesh.ndim
    if lame_lambda is None or lame_mu is None:
      raise ValueError('lame_lambda and lame_mu are required')
    lam = _elastic_coefficient(fespace, lame_lambda, 'lame_lambda', False)
    mu = _elastic_coefficient(fespace, lame_mu, 'lame_mu', True)
    rho = _elastic_coefficient(fespace, 1.0 if density is None else density,
                               'density', False)
    mask = None
    if dirichlet_mask is not None:
      m = torch.as_tensor(dirichlet_mask, device=fespace.device)
      if tuple(m.shape) == (mesh.num_nodes,):
        m = m[:, None].expand(mesh.num_nodes, d)
      if tuple(m.shape) != (mesh.num_nodes, d):
        raise ValueError(f'dirichlet_mask: shape {tuple(m.shape)}; expected '
                         f'({mesh.num_nodes}, {d}) or ({mesh.num_nodes},)')
      mask = (m == 0).to(fespace.dtype).contiguous()
    parts = _grid_geometry_parts(fespace, _ops.stokes_setup, geometry)
    return cls(fespace=fespace, parts=parts, host=_host_tables(fespace, True),
               lam=lam, mu=mu, rho=rho, mask=mask,
               coef_source=(lame_lambda, lame_mu, density))

  def point_weights(self):
    """W = w detJ (E, Q^d)."""
    if self._wdet is None:
      self._wdet = self.fespace.wdet()
    return self._wdet

  def apply_local(self, u_local, lambda0=0.0):
    """(E, n, d) element displacements -> (E, n, d) local covector."""
    fes = self.fespace
    uq = self._to_grid(u_local)
    rq = _ops.elasticity_local(uq, self.parts, self.host, fes.mesh.ndim,
                               fes.quadrature.num_points,
                               self.point_weights(), self.lam, self.mu,
                               self.rho, lambda0)
    return fes._interpolate_t(rq)

  def apply(self, u, lambda0=0.0):
    """u (N, d), dense or component-major -> mask * scatter(local(gather(u)))
    in the layout of `u`."""
    return self._assembled(u, lambda v: self.apply_local(v, lambda0))

  def linear_operator(self, lambda0=0.0):
    return lambda u: self.apply(u, lambda0)

  def sensitivity(self, u, v, lambda0=0.0, want=(True, True, True)):
    """The gradient of v . (K + lambda0 M_rho) u WITHOUT the Dirichlet mask
    with respect to (lame_lambda, lame_mu, density), each in the form the
    caller passed to `create` (`reduce_coefficient_gradient`): a scalar gives
    a 0-dim tensor (the sum over all points), (E,) the sum over each
    element's points, (E, Q^d) per-point values.  None for a callable, for an
    absent density and where `want` is false.  `u`, `v`: nodal (N, d), dense
    or component-major; they are gathered and interpolated to the quadrature
    grid as in `apply_local`, then one launch of `sfem_elasticity_sens` per
    part.  Nothing of size (E, Q^d, d, d) is stored."""
    fes = self.fespace
    mesh = fes.mesh
    d = mesh.ndim
    for w in (u, v):
      if tuple(w.shape) != (mesh.num_nodes, d):
        raise ValueError(f'expected ({mesh.num_nodes}, {d}) nodal '
                         f'displacements, got {tuple(w.shape)}')
    tensor = lambda s: s is not None and not _is_callable_source(s)
    wanted = tuple(bool(w) and tensor(s)
                   for w, s in zip(want, self.coef_source))
    if not any(wanted):
      return None, None, None
    uq, vq = (fes._interpolate(_ops.gather_rows(
        w.detach().to(fes.dtype).contiguous(), mesh.elements)).contiguous()
              for w in (u, v))
    grads = _ops.elasticity_sens(uq, vq, self.parts, self.host, d,
                                 fes.quadrature.num_points,
                                 self.point_weights(), lambda0, want=wanted)
    return tuple(reduce_coefficient_gradient(g, s)
                 for g, s in zip(grads, self.coef_source))

  # ------------------------------------------------------------------ stress
  def _stress_q(self, uq, von_mises, plane_stress):
    """(sigma, von Mises or None) at the quadrature points from `uq`
    (E, Q^d, d) there: the kernel alone, or its autograd node where `uq` or a
    Lame parameter the operator was created with requires grad."""
    fes = self.fespace
    lam_src, mu_src = self.coef_source[:2]
    if autodiff.needs_grad(uq, lam_src, mu_src):
      sigma = autodiff.elasticity_stress_local(self, uq.contiguous(),
                                               plane_stress)
      # the fused von Mises output has no adjoint: sqrt is taken by autograd
      vm = _von_mises(sigma, fes.mesh.ndim) if von_mises else None
      return sigma, vm
    return _ops.elasticity_stress(
        uq.contiguous(), self.parts, self.host, fes.mesh.ndim,
        fes.quadrature.num_points, self.point_weights(), self.lam, self.mu,
        want=(True, bool(von_mises)), plane_stress=plane_stress)

  def stress_local(self, u_local, *, von_mises=False, plane_stress=False):
    """(E, n, d) element displacements -> the stress (E, Q^d, NV) at the
    quadrature points; with `von_mises` the pair (stress, von Mises (E, Q^d)).
    NV = 6, slots (xx, yy, zz, xy, xz, yz) in 3D; NV = 4, slots (xx, yy, xy,
    zz) in 2D with sigma_zz = lambda tr(eps) (plane strain) or, with
    `plane_stress`, 0 (the operator then holds the modified lambda of
    `lame_parameters(..., plane_stress=True)`).  Interpolation
    (`sfem_basis_eval`) and one fused kernel (`sfem_elasticity_stress`, DESIGN
    §3.18); nothing of size (E, Q^d, d, d) is stored.

    Differentiable with respect to `u_local` and to `lame_lambda` / `lame_mu`
    given to `create` as tensors that require grad; backward is one launch of
    `sfem_elasticity_stress_vjp`.  Without grad the von Mises value is the
    kernel's fused output, with grad it is `von_mises(sigma)`.  The von Mises
    stress has no gradient where it is zero (a square root at zero):
    differentiate `vm ** 2` or a p-norm there."""
    fes = self.fespace
    d = fes.mesh.ndim
    if u_local.dim() != 3 or tuple(u_local.shape[::2]) != (
        fes.mesh.num_elements, d):
      raise ValueError(f'expected ({fes.mesh.num_elements}, n, {d}) local '
                       f'values, got {tuple(u_local.shape)}')
    uq = fes._interpolate(u_local.to(fes.dtype))
    sigma, vm = self._stress_q(uq, von_mises, bool(plane_stress))
    return (sigma, vm) if von_mises else sigma

  def _lumped_weights(self):
    """scatter(I^T W) (N,), the row sums of the mass matrix; checked > 0."""
    if self._lumped is None:
      fes = self.fespace
      mesh = fes.mesh
      W = self.point_weights()
      den = _ops.scatter_add(fes._interpolate_t(W[..., None].contiguous()),
                             mesh.elements, mesh.num_nodes, ncomp=1)
      den = den.reshape(mesh.num_nodes)
      if not float(den.min()) > 0.0:
        raise ValueError(
            'lumped stress recovery: a node has a non-positive lumped weight '
            f'(min {float(den.min()):.3e}); use recovery=\'l2\'')
      self._lumped = den
    return self._lumped

  def stress(self, u, *, at='nodes', recovery='lumped', von_mises=False,
             plane_stress=False, rtol=None):
    """The stress of nodal displacements `u` (N, d), dense or component-major.

    `at='quadrature'`: what `stress_local` gives, (E, Q^d, NV).
    `at='nodes'`: (N, NV) by `recovery`
      'lumped': scatter(I^T (W sigma_q)) / scatter(I^T W), the quadrature
        values averaged with the weights of the lumped mass matrix;
      'l2': the L2 projection M sigma_N = scatter(I^T (W sigma_q)) with the
        plain mass matrix of the space, one CG solve per column (relative
        tolerance `rtol`, default 1e-12 in fp64 and 1e-6 in fp32).
    With `von_mises` the pair (stress, von Mises); at nodes the von Mises
    stress is `von_mises` of the nodal stress.  Differentiable as
    `stress_local` is ('l2' through `linalg.cg.symmetric_solve`)."""
    fes = self.fespace
    mesh = fes.mesh
    d, N = mesh.ndim, mesh.num_nodes
    if at not in ('nodes', 'quadrature'):
      raise ValueError(f"at={at!r}: expected 'nodes' or 'quadrature'")
    if recovery not in ('lumped', 'l2'):
      raise ValueError(f"recovery={recovery!r}: expected 'lumped' or 'l2'")
    if not isinstance(u, torch.Tensor) or tuple(u.shape) != (N, d):
      raise ValueError(f'expected ({N}, {d}) nodal displacements, got '
                       f'{tuple(getattr(u, "shape", ()))}')
    grad = autodiff.needs_grad(u, *self.coef_source[:2])
    gather_rows = autodiff.gather_rows if grad else _ops.gather_rows
    v = u.to(fes.dtype).contiguous()
    uq = fes._interpolate(gather_rows(v, mesh.elements))
    quad = at == 'quadrature'
    sigma, vm = self._stress_q(uq, von_mises and quad, bool(plane_stress))
    if quad:
      return (sigma, vm) if von_mises else sigma
    W = self.point_weights()
    loc = fes._interpolate_t(sigma * W[..., None], grad)
    scatter = autodiff.scatter_add if grad else _ops.scatter_add
    rhs = scatter(loc.contiguous(), mesh.elements, N, ncomp=sigma.shape[-1])
    if recovery == 'lumped':
      nodal = rhs / self._lumped_weights()[:, None]
    else:
      from swirl_fem_amd.linalg.cg import cg, symmetric_solve
      mass = fes.helmholtz_operator(None)
      A = lambda x: mass.apply(x, 1.0, 0.0)
      if rtol is None:
        rtol = 1e-12 if fes.dtype == torch.float64 else 1e-6
      cols = []
      for k in range(rhs.shape[1]):
        b = rhs[:, k].contiguous()
        cols.append(symmetric_solve(A, b, tol=rtol) if grad
                    else cg(A, b, tol=rtol)[0])
      nodal = torch.stack(cols, dim=1)
    if von_mises:
      return nodal, _von_mises(nodal, d)
    return nodal

  def _component_factors(self, i):
    """Stored per-point factors of the scalar operator that is the diagonal
    block of component i: the tensor mu I + (lambda + mu) e_i e_i^T folded as
    G_i = W J^-1 (.) J^-T, and rho W, in the layout of `sfem_helmholtz_setup`
    for every element."""
    fes = self.fespace
    d = fes.mesh.ndim
    ij, W = fes.invjacs, self.point_weights()    # ij[e,q,j,a] = d xi_a / d x_j
    lm = self.lam + self.mu
    vals = []
    for a in range(d):
      for b in range(a, d):
        g = (ij[..., a] * ij[..., b]).sum(-1) * self.mu
        vals.append(W * (g + lm * ij[..., i, a] * ij[..., i, b]))
    Wm = W * self.rho
    E, Q = W.shape
    if d == 3:
      pairs = torch.stack(vals).view(3, 2, E, Q).permute(2, 0, 3, 1)
      return torch.cat([pairs.reshape(E, 6 * Q), Wm], dim=1).view(
          E, 7, Q).contiguous()
    pairs = torch.stack(vals + [Wm]).view(2, 2, E, Q).permute(2, 0, 3, 1)
    return pairs.reshape(E, 4, Q).contiguous()

  def diagonal(self, lambda0=0.0):
    """The assembled (N, d) diagonal of `apply(u, lambda0)`: per component the
    element diagonals of I^T K_ii I from `sfem_helmholtz_diag` on stored
    factors, summed per node in a fixed order, fixed components zero."""
    fes = self.fespace
    mesh = fes.mesh
    d = mesh.ndim
    if self._diag is None:
      P = mesh.gridpoints_1d.num_points
      bmat = None if fes.is_collocated else np.asarray(
          fes.interpolator._interpolation_matrix_1d(), dtype=np.float64)
      dq = np.asarray(self.host['dmat'], dtype=np.float64)
      dtil = dq if bmat is None else dq @ bmat
      offsets, slots = mesh.assembly_plan().csr()
      mass, stiff = None, []
      for i in range(d):
        part = {'geo_mode': _GEO_POINT, 'geo': self._component_factors(i)}
        m, k = _ops.helmholtz_diag(
            [part], mesh.num_elements, d, P, dtil, self.host['weights'],
            self.host['nodes'], bmat, want_mass=i == 0, dtype=fes.dtype,
            device=fes.device)
        stiff.append(_ops.scatter_csr(k.reshape(-1), offsets, slots,
                                      mesh.num_nodes))
        if i == 0:
          mass = _ops.scatter_csr(m.reshape(-1), offsets, slots,
                                  mesh.num_nodes)
      self._diag = (mass, torch.stack(stiff, dim=1).contiguous())
    mass, stiff = self._diag
    out = stiff if lambda0 == 0.0 else stiff + lambda0 * mass[:, None]
    return out if self.mask is None else out * self.mask


# ---------------------------------------------------------------------------
# Finite-strain (neo-Hookean) elasticity
# ---------------------------------------------------------------------------
@dataclasses.dataclass(eq=False)
class HyperelasticLinearization:
  """What `HyperelasticOperator.linearize(u)` leaves: `state` (E, Q^d,
  d*d + 1), per quadrature point F^-1 row-major and ln J, which the tangent
  kernel reads; `residual`, mask * R(u) (N, d) from the same launch, and the
  `lambda0` it was formed with."""
  state: torch.Tensor
  residual: torch.Tensor
  lambda0: float


class _OnLinearElasticity(_DisplacementOperator):
  """An operator built on a linear `ElasticityOperator`, its field `linear`:
  geometry, coefficients, mask and point weights are that operator's."""
  fespace = property(lambda self: self.linear.fespace)
  parts = property(lambda self: self.linear.parts)
  host = property(lambda self: self.linear.host)
  lam = property(lambda self: self.linear.lam)
  mu = property(lambda self: self.linear.mu)
  rho = property(lambda self: self.linear.rho)
  mask = property(lambda self: self.linear.mask)

  def point_weights(self):
    """W = w detJ (E, Q^d)."""
    return self.linear.point_weights()

  def _grid_args(self, lambda0):
    """What a launch on the quadrature grid takes after the values there."""
    fes = self.fespace
    return (self.parts, self.host, fes.mesh.ndim, fes.quadrature.num_points,
            self.point_weights(), self.lam, self.mu, self.rho, lambda0)


class _Tangent:
  """`T w` at a linearisation: `apply(w)` (N, d) in any layout, returned in
  the layout given; `linear_operator()` the callable CG takes.  `launch(wq)`
  is the tangent-mode launch on the quadrature grid."""

  def __init__(self, op, lambda0, launch):
    self.op, self.lambda0, self._launch = op, float(lambda0), launch

  def apply_local(self, w_local):
    return self.op.fespace._interpolate_t(
        self._launch(self.op._to_grid(w_local)))

  def apply(self, w):
    return self.op._assembled(w, self.apply_local)

  def linear_operator(self):
    return self.apply


class HyperelasticTangent(_Tangent):
  """`T(u) w` at the linearisation `state`."""

  def __init__(self, op, state, lambda0):
    super().__init__(op, lambda0, lambda wq: _ops.hyperelastic_local(
        wq, *op._grid_args(self.lambda0), mode='tangent', state=state))
    self.state = state


@dataclasses.dataclass(eq=False)
class HyperelasticOperator(_OnLinearElasticity):
  """The internal force of a compressible neo-Hookean solid in the total-
  Lagrangian formulation, for displacements u (N, d):

      R(u) = int P(F) : grad v + lambda0 int rho u . v,   F = I + grad u,
      P = mu (F - F^-T) + lambda ln J F^-T,  J = det F,

  its energy `Psi(u) = int psi + lambda0/2 int rho |u|^2` with psi = mu/2
  (F:F - d) - mu ln J + lambda/2 (ln J)^2, and its tangent `T(u) w = int
  dP[grad w] : grad v + lambda0 int rho w . v` (plane strain in 2D).  The
  geometry is the reference mesh.  Interpolation to the quadrature grid, one
  launch of `sfem_hyperelastic_local` there, transposed interpolation; the
  tangent reads F^-1 and ln J of the linearisation from the state the
  residual launch stored.  `linear` is the `ElasticityOperator` with the same
  mask and coefficients: the tangent at u = 0, and what preconditioners are
  built on."""
  linear: ElasticityOperator

  @classmethod
  def create(cls, fespace, dirichlet_mask=None, *, lame_lambda, lame_mu,
             density=None, geometry='auto') -> 'HyperelasticOperator':
    return cls(linear=ElasticityOperator._intake(
        fespace, dirichlet_mask, lame_lambda, lame_mu, density, geometry,
        'HyperelasticOperator', 'fused hyperelasticity'))

  def _launch(self, u_local, lambda0, want_state=False, want_psi=False):
    return _ops.hyperelastic_local(
        self._to_grid(u_local), *self._grid_args(lambda0), mode='residual',
        want_state=want_state, want_psi=want_psi)

  def residual_local(self, u_local, lambda0=0.0):
    """(E, n, d) element displacements -> (E, n, d) local internal force."""
    return self.fespace._interpolate_t(self._launch(u_local, lambda0)[0])

  def residual(self, u, lambda0=0.0):
    """u (N, d), dense or component-major -> mask * R(u) in that layout.  An
    inverted state (J <= 0 at a point) gives non-finite entries."""
    return self._assembled(u, lambda v: self.residual_local(v, lambda0))

  def energy(self, u, lambda0=0.0) -> float:
    """Psi(u), a Python float: the kernel's per-point values summed in fp64.
    Non-finite for an inverted state."""
    _, _, psi = self._launch(self._nodal(u), lambda0, want_psi=True)
    return float(torch.sum(psi, dtype=torch.float64))

  def linearize(self, u, lambda0=0.0) -> HyperelasticLinearization:
    """One residual launch at `u` that also stores the state of the tangent;
    the result carries the residual, so a Newton step launches once."""
    box = {}

    def local(v):
      rq, box['state'], _ = self._launch(v, lambda0, want_state=True)
      return self.fespace._interpolate_t(rq)
    res = self._assembled(u, local)
    return HyperelasticLinearization(state=box['state'], residual=res,
                                     lambda0=float(lambda0))

  def tangent(self, state, lambda0=0.0) -> HyperelasticTangent:
    """The tangent at the linearisation `state` (a `HyperelasticLinearization`
    or its state tensor): one tangent-mode launch per apply."""
    if isinstance(state, HyperelasticLinearization):
      state = state.state
    return HyperelasticTangent(self, state, lambda0)

  def sensitivity(self, u, v, lambda0=0.0, want=(True, True, True),
                  linearization=None):
    """The gradient of v . R(u) WITHOUT the Dirichlet mask with respect to
    (lame_lambda, lame_mu, density), each in the form the caller passed to
    `create` (`reduce_coefficient_gradient`): a scalar gives a 0-dim tensor
    (the sum over all points), (E,) the sum over each element's points,
    (E, Q^d) per-point values.  None for a callable, for an absent density and
    where `want` is false.  `u`, `v`: nodal (N, d), dense or component-major.
    P is linear in the coefficients, so per point the gradients are W ln J
    tr(F^-1 H_v), W (F : H_v - tr(F^-1 H_v)) and lambda0 W u . v (DESIGN
    §3.21): `v` is gathered and interpolated to the quadrature grid, then one
    launch of `sfem_hyperelastic_sens` per part reads F^-1 and ln J from the
    state of `linearization` (a `HyperelasticLinearization` at `u`, or its
    state tensor); without one, one `linearize(u)` launch forms it.  `u` itself
    is interpolated for the density alone."""
    fes = self.fespace
    mesh = fes.mesh
    d = mesh.ndim
    for w in (u, v):
      if tuple(w.shape) != (mesh.num_nodes, d):
        raise ValueError(f'expected ({mesh.num_nodes}, {d}) nodal '
                         f'displacements, got {tuple(w.shape)}')
    source = self.linear.coef_source
    if len(tuple(want)) != 3:
      raise ValueError('`want` names (lame_lambda, lame_mu, density)')
    tensor = lambda s: s is not None and not _is_callable_source(s)
    wanted = tuple(bool(w) and tensor(s) for w, s in zip(want, source))
    if not any(wanted):
      return None, None, None
    if linearization is None:
      linearization = self.linearize(u.detach(), lambda0)
    state = (linearization.state
             if isinstance(linearization, HyperelasticLinearization)
             else linearization)
    grid = lambda w: fes._interpolate(_ops.gather_rows(
        w.detach().to(fes.dtype).contiguous(), mesh.elements)).contiguous()
    grads = _ops.hyperelastic_sens(
        grid(v), state, self.parts, self.host, d, fes.quadrature.num_points,
        self.point_weights(), grid(u) if wanted[2] else None, lambda0,
        want=wanted)
    return tuple(reduce_coefficient_gradient(g, s)
                 for g, s in zip(grads, source))


# ---------------------------------------------------------------------------
# Small-strain J2 plasticity
# ---------------------------------------------------------------------------
@dataclasses.dataclass(eq=False)
class PlasticityLinearization:
  """What `PlasticityOperator.linearize(u, history)` leaves: `lin` (E, Q^d,
  NL), per quadrature point (a, b, n) of the algorithmic tangent; `residual`,
  mask * R(u) (N, d); `history`, the trial history (E, Q^d, NH) that becomes
  the committed one if this state is accepted -- all from one launch -- and
  the `lambda0` it was formed with."""
  lin: torch.Tensor
  residual: torch.Tensor
  history: torch.Tensor
  lambda0: float

  def num_plastic(self) -> int:
    """Points that yielded in this step (b != 0 or a != 2 mu: n is non-zero
    exactly there)."""
    return int((self.lin[..., 2:] != 0).any(dim=-1).sum())


class PlasticityTangent(_Tangent):
  """The algorithmic tangent at the linearisation `lin`."""

  def __init__(self, op, lin, lambda0):
    super().__init__(op, lambda0, lambda wq: _ops.plasticity_local(
        wq, *op._grid_args(self.lambda0), op.yield_stress, op.hardening,
        mode='tangent', lin=lin))
    self.lin = lin


@dataclasses.dataclass(eq=False)
class PlasticityOperator(_OnLinearElasticity):
  """The internal force of a small-strain von Mises (J2) elastoplastic solid
  with linear isotropic hardening, for displacements u (N, d)
  and a committed history (E, Q^d, NH) at the quadrature points:

      R(u) = int sigma(eps(u); eps_p, alpha) : grad v + lambda0 int rho u . v

  with sigma from the radial return of `sfem_plasticity_local` (plane strain
  in 2D), and its algorithmic tangent `T w = int dsigma[sym grad w] : grad v +
  lambda0 int rho w . v`.  Per point the history is eps_p in the Voigt slots
  of `ElasticityOperator.stress` (3D: xx, yy, zz, xy, xz, yz; 2D: xx, yy, xy)
  and then alpha, the accumulated plastic strain.  Interpolation to the
  quadrature grid, one launch there, transposed interpolation; the tangent
  reads (a, b, n) from the `lin` state the residual launch stored.  The
  committed history is never written: every launch returns a trial history.
  `linear` is the `ElasticityOperator` with the same mask and coefficients:
  the tangent of unyielded material, and what preconditioners are built on."""
  linear: ElasticityOperator
  yield_stress: object
  hardening: object
  # (yield_stress, hardening_modulus) as the caller passed them: `sensitivity`
  # returns its gradients in these forms
  plastic_source: tuple = (None, None)

  @classmethod
  def create(cls, fespace, dirichlet_mask=None, *, lame_lambda, lame_mu,
             yield_stress, hardening_modulus=0.0, density=None,
             geometry='auto') -> 'PlasticityOperator':
    linear = ElasticityOperator._intake(
        fespace, dirichlet_mask, lame_lambda, lame_mu, density, geometry,
        'PlasticityOperator', 'fused plasticity')
    return cls(linear=linear,
               yield_stress=_elastic_coefficient(fespace, yield_stress,
                                                 'yield_stress', True),
               hardening=_elastic_coefficient(fespace, hardening_modulus,
                                              'hardening_modulus', False),
               plastic_source=(yield_stress, hardening_modulus))

  def history_shape(self):
    mesh = self.fespace.mesh
    return (mesh.num_elements, self.fespace.quadrature.num_points ** mesh.ndim,
            _ops.plasticity_sizes(mesh.ndim)[0])

  def virgin_history(self):
    """Zeros (E, Q^d, NH): no plastic strain."""
    return torch.zeros(self.history_shape(), dtype=self.fespace.dtype,
                       device=self.fespace.device)

  def _history(self, history):
    if history is None:
      return None
    if autodiff.needs_grad(history):
      raise NotImplementedError('autograd through PlasticityOperator')
    if tuple(history.shape) != self.history_shape():
      raise ValueError(f'history: expected {self.history_shape()}, got '
                       f'{tuple(history.shape)}')
    return history.to(self.fespace.dtype).contiguous()

  def _launch(self, u_local, history, lambda0, **want):
    return _ops.plasticity_local(
        self._to_grid(u_local), *self._grid_args(lambda0), self.yield_stress,
        self.hardening, mode='residual', hist=self._history(history), **want)

  def residual_local(self, u_local, history=None, lambda0=0.0):
    """(E, n, d) element displacements -> (E, n, d) local internal force."""
    return self.fespace._interpolate_t(
        self._launch(u_local, history, lambda0)[0])

  def residual(self, u, history=None, lambda0=0.0):
    """u (N, d), dense or component-major -> mask * R(u) in that layout, from
    the committed `history` (None: virgin material)."""
    return self._assembled(
        u, lambda v: self.residual_local(v, history, lambda0))

  def linearize(self, u, history=None, lambda0=0.0) -> PlasticityLinearization:
    """One residual launch at `u` that also stores the state of the tangent
    and the trial history, so a Newton step launches once and an accepted
    step commits its history without another launch."""
    box = {}

    def local(v):
      rq, box['hist'], box['lin'], _ = self._launch(
          v, history, lambda0, want_hist=True, want_lin=True)
      return self.fespace._interpolate_t(rq)
    res = self._assembled(u, local)
    return PlasticityLinearization(lin=box['lin'], residual=res,
                                   history=box['hist'],
                                   lambda0=float(lambda0))

  def tangent(self, lin, lambda0=0.0) -> PlasticityTangent:
    """The algorithmic tangent at the linearisation `lin` (a
    `PlasticityLinearization` or its lin tensor): one tangent-mode launch per
    apply."""
    if isinstance(lin, PlasticityLinearization):
      lin = lin.lin
    return PlasticityTangent(self, lin, lambda0)

  def stress(self, u, history=None):
    """(sigma (E, Q^d, NV), trial history (E, Q^d, NH)) at the quadrature
    points for nodal u (N, d) from the committed `history`: sigma in the slots
    that `von_mises` takes (3D: xx, yy, zz, xy, xz, yz; 2D: xx, yy, xy, zz)."""
    _, hist, _, sigma = self._launch(self._nodal(u), history, 0.0,
                                     want_hist=True, want_stress=True)
    return sigma, hist

  # ----------------------------------------------------------------- adjoint
  def _cotangent(self, hbar):
    if hbar is None:
      return None
    if tuple(hbar.shape) != self.history_shape():
      raise ValueError(f'hbar: expected {self.history_shape()}, got '
                       f'{tuple(hbar.shape)}')
    return hbar.detach().to(self.fespace.dtype).contiguous()

  def _vjp_args(self):
    fes = self.fespace
    return (self.parts, self.host, fes.mesh.ndim, fes.quadrature.num_points,
            self.point_weights(), self.lam, self.mu, self.yield_stress,
            self.hardening)

  def history_vjp(self, u, history, hbar):
    """mask * d(hbar . Phi)/du (N, d) in the layout of `u`, for the history
    update Phi: (u, committed `history`) -> trial history and a cotangent
    `hbar` (E, Q^d, NH) of the trial history.  Interpolation
    to the quadrature grid, one displacement-mode launch of
    `sfem_plasticity_vjp` per part, transposed interpolation and scatter, as
    in `residual`.  The return mapping is repeated from `u` and `history`
    (None: virgin material)."""
    if hbar is None:
      raise ValueError('history_vjp needs the cotangent `hbar`')
    hbar = self._cotangent(hbar)
    hist = self._history(history)

    def local(v):
      return self.fespace._interpolate_t(_ops.plasticity_vjp(
          self._to_grid(v), *self._vjp_args(), mode='displacement', hist=hist,
          hbar=hbar))
    return self._assembled(u, local)

  def sensitivity(self, u, w, history=None, hbar=None, lambda0=0.0,
                  want=(True, True, True, True, True), want_history=True):
    """((d/dlame_lambda, d/dlame_mu, d/dyield_stress, d/dhardening_modulus,
    d/ddensity), hbar_prev): the gradient of w . R(u; history) + hbar .
    Phi(u; history) WITHOUT the Dirichlet mask, Phi the history update, with
    respect to the coefficients and to the committed `history` (None: virgin;
    `hbar` None: zero).  Each coefficient gradient comes in the form the
    caller passed to `create` (`reduce_coefficient_gradient`): a scalar gives
    a 0-dim tensor (the sum over all points), (E,) the sum over each
    element's points, (E, Q^d) per-point values; None for a callable, for an
    absent density and where `want` is false.  `hbar_prev` (E, Q^d, NH) is
    None unless `want_history`.  `u`, `w`: nodal (N, d), dense or component-
    major; both are gathered and interpolated to the quadrature grid, then
    one state-mode launch of `sfem_plasticity_vjp` per part repeats the
    return mapping and forms the point VJP with S = W sym(grad w) (DESIGN
    §3.23).  Nothing of size (E, Q^d, d, d) is stored."""
    fes = self.fespace
    mesh = fes.mesh
    d = mesh.ndim
    for x in (u, w):
      if tuple(x.shape) != (mesh.num_nodes, d):
        raise ValueError(f'expected ({mesh.num_nodes}, {d}) nodal '
                         f'displacements, got {tuple(x.shape)}')
    if len(tuple(want)) != 5:
      raise ValueError('`want` names (lame_lambda, lame_mu, yield_stress, '
                       'hardening_modulus, density)')
    lam_s, mu_s, rho_s = self.linear.coef_source
    source = (lam_s, mu_s) + tuple(self.plastic_source) + (rho_s,)
    tensor = lambda s: s is not None and not _is_callable_source(s)
    wanted = tuple(bool(k) and tensor(s) for k, s in zip(want, source))
    if not (any(wanted) or want_history):
      return (None,) * 5, None
    hbar = self._cotangent(hbar)
    hist = self._history(history)
    grid = lambda x: fes._interpolate(_ops.gather_rows(
        x.detach().to(fes.dtype).contiguous(), mesh.elements)).contiguous()
    out = _ops.plasticity_vjp(
        grid(u), *self._vjp_args(), mode='state', hist=hist, hbar=hbar,
        w_q=grid(w), lambda0=lambda0, want=wanted,
        want_history=bool(want_history))
    return (tuple(reduce_coefficient_gradient(g, s)
                  for g, s in zip(out[1:], source)), out[0])
