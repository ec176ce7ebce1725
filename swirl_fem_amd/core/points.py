"""Fields at arbitrary points: locate once, then sample and
spread.

`locate_points` finds the element and the reference coordinates of each point
(`sfem_point_locate`: a uniform cell grid for candidates, Newton on the
element's nodal map).  `PointEvaluator` keeps the location as a plan (points
sorted by element, segments, chunks) and applies

    ev(u)[m]        = sum_n u[elements[e_m, n]] l_n(xi_m)        (M,) / (M, C)
    ev.transpose(w) = sum_m w[m] l_n(xi_m) at node elements[e_m, n]   (N,) / (N, C)

through `sfem_point_eval` and `sfem_point_eval_t` + `sfem_scatter_csr`.  Both
are linear and each is the other's backward.  The candidate lists and the
plan are built with vectorised torch / NumPy and work for a mesh on the CPU
(the host tests check them there); the kernels need the GPU.
"""

from __future__ import annotations

import dataclasses

import numpy as np
import torch

from swirl_fem_amd import _lib

CHUNK = _lib.SFEM_POINT_CHUNK
XI_LIMIT = 1.5          # the locator clamps to it; from_location refuses more


def basis_tables(gridpoints_1d):
  """(nodes (P1,), bary (P1,)) float64 with bary[i] = 1 / prod_{k != i}
  (x_i - x_k): l_i(x) = bary[i] prod_{k != i} (x - x_k) for any node family."""
  x = np.asarray(gridpoints_1d.node_values, dtype=np.float64)
  diff = x[:, None] - x[None, :]
  np.fill_diagonal(diff, 1.0)
  return x, 1.0 / diff.prod(axis=1)


def _check_mesh(mesh, who):
  if mesh.axis_name is not None or mesh.neighbor_plan is not None:
    raise NotImplementedError(f'{who} on a partitioned mesh')
  if mesh._cache.get('replicas', 1) > 1:
    raise NotImplementedError(f'{who} on an ensemble (Mesh.replicate)')
  if mesh.ndim not in (2, 3):
    raise NotImplementedError(f'{who} needs ndim 2 or 3, got {mesh.ndim}')
  p1 = mesh.gridpoints_1d.num_points
  if not 2 <= p1 <= 12:
    raise NotImplementedError(f'{who} needs 2..12 points per direction, got '
                              f'{p1}')
  if mesh.dtype not in (torch.float32, torch.float64):
    raise TypeError(f'unsupported mesh dtype {mesh.dtype}')


def _check_points(mesh, points, who):
  if not isinstance(points, torch.Tensor):
    raise ValueError(f'{who}: points must be a torch.Tensor')
  if points.requires_grad:
    raise NotImplementedError(
        f'{who}: derivatives with respect to point positions')
  if points.dim() != 2 or points.shape[1] != mesh.ndim:
    raise ValueError(f'{who}: expected points of shape (M, {mesh.ndim}), got '
                     f'{tuple(points.shape)}')
  if points.dtype != mesh.dtype or points.device != mesh.device:
    raise ValueError(f'{who}: points must have the dtype and device of the '
                     f'mesh ({mesh.dtype}, {mesh.device}); got {points.dtype}, '
                     f'{points.device}')


@dataclasses.dataclass(frozen=True, eq=False)
class CandidateGrid:
  """Cell grid over the real elements' inflated boxes: CSR cell -> candidate
  elements (ascending ids), the boxes and the extents."""
  lo: np.ndarray             # (d,) grid box
  hi: np.ndarray
  ncell: np.ndarray          # (d,) int
  inv_cell: np.ndarray       # (d,)
  cell_offsets: torch.Tensor  # (cells + 1,) int64
  cell_elems: torch.Tensor    # int32
  boxes: torch.Tensor         # (E, 2, d) float64, inflated
  extent: torch.Tensor        # (E,) float64: largest side of the plain box

  @classmethod
  def build(cls, mesh, inflate=0.1) -> 'CandidateGrid':
    if not inflate >= 0.0:
      raise ValueError(f'inflate must be >= 0, got {inflate}')
    el, dev, d = mesh.elements, mesh.device, mesh.ndim
    E = el.shape[0]
    if E and int(el.max()) >= mesh.num_nodes:
      raise ValueError('element rows hold node ids outside the mesh')
    real = (el >= 0).all(dim=1)
    idx = el.clamp(min=0).long()
    lo = torch.empty((E, d), dtype=torch.float64, device=dev)
    hi = torch.empty((E, d), dtype=torch.float64, device=dev)
    for a in range(d):
      xa = mesh.node_coords[:, a].to(torch.float64)[idx]
      lo[:, a], hi[:, a] = xa.amin(dim=1), xa.amax(dim=1)
    side = hi - lo
    boxes = torch.stack([lo - inflate * side, hi + inflate * side], dim=1)
    extent = side.amax(dim=1)
    boxes[~real] = 0.0
    extent = torch.where(real, extent, torch.zeros_like(extent))

    ids = np.flatnonzero(real.cpu().numpy())
    bx = boxes.cpu().numpy()[ids]                      # (Er, 2, d)
    if len(ids) == 0:
      glo, ghi = np.zeros(d), np.zeros(d)
    else:
      glo, ghi = bx[:, 0].min(axis=0), bx[:, 1].max(axis=0)
    length = ghi - glo
    pos = length > 0
    if len(ids) and pos.all():
      h = (length.prod() / len(ids)) ** (1.0 / d)
      ncell = np.clip(np.rint(length / h), 1, 1 << 20).astype(np.int64)
    else:
      ncell = np.ones(d, np.int64)
    inv_cell = np.where(pos, ncell / np.where(pos, length, 1.0), 0.0)
    grid = cls(glo, ghi, ncell, inv_cell, None, None, boxes.contiguous(),
               extent.contiguous())
    c_lo = grid._axis_cells(bx[:, 0])                  # (Er, d)
    c_hi = grid._axis_cells(bx[:, 1])
    span = c_hi - c_lo + 1
    count = span.prod(axis=1)
    total = int(count.sum())
    if total >= 2 ** 31:
      raise ValueError('candidate lists too long for int32')
    owner = np.repeat(np.arange(len(ids)), count)
    local = np.arange(total) - np.repeat(np.cumsum(count) - count, count)
    cell = np.zeros(total, np.int64)
    stride = 1
    for a in reversed(range(d)):
      sa = span[owner, a]
      cell += (c_lo[owner, a] + local % sa) * stride
      local = local // sa
      stride *= int(ncell[a])
    elem = ids[owner]
    order = np.lexsort((elem, cell))
    num_cells = int(ncell.prod())
    offsets = np.zeros(num_cells + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(cell, minlength=num_cells))
    return dataclasses.replace(
        grid, cell_offsets=torch.as_tensor(offsets, device=dev),
        cell_elems=torch.as_tensor(elem[order].astype(np.int32), device=dev))

  def _axis_cells(self, x):
    """Per-axis cell of coordinates (..., d), clamped: the kernel's rule."""
    f = np.floor((np.asarray(x, np.float64) - self.lo) * self.inv_cell)
    return np.clip(f, 0, self.ncell - 1).astype(np.int64)

  def cell_of(self, points):
    """Cell index (M,) of points (M, d) (lexicographic, axis 0 slowest)."""
    c = self._axis_cells(points)
    cell = np.zeros(c.shape[0], np.int64)
    for a in range(c.shape[1]):
      cell = cell * int(self.ncell[a]) + c[:, a]
    return cell


@dataclasses.dataclass(frozen=True, eq=False)
class PointLocation:
  """Result of `locate_points`: `element` (M,) int32 (-1: not found), `xi`
  (M, d) reference coordinates (0 where not found), `found` (M,) bool."""
  element: torch.Tensor
  xi: torch.Tensor
  found: torch.Tensor


def candidate_grid(mesh, inflate=0.1) -> CandidateGrid:
  """The candidate grid of `mesh`, cached per `inflate`."""
  key = ('point_grid', float(inflate))
  if key not in mesh._cache:
    mesh._cache[key] = CandidateGrid.build(mesh, inflate)
  return mesh._cache[key]


def locate_points(mesh, points, *, inflate=0.1, max_iter=10, tol_xi=None,
                  tol_x=None) -> PointLocation:
  """Element and reference coordinates of each of `points` (M, d).

  Candidates are the elements whose node bounding box, inflated by `inflate`
  of its extent per axis, overlaps the point's cell of a uniform grid.  Each
  is tried with at most `max_iter` Newton steps from xi = 0 in double
  arithmetic (and, when they end outside the reference cube, as many again
  from the nearest point of the cube) and accepted when max |xi| <= 1 + `tol_xi` and the residual is
  at most `tol_x` times the element's extent (defaults 1e-10 in float64,
  1e-5 in float32); the lowest accepted element id wins."""
  from swirl_fem_amd import _ops
  _check_mesh(mesh, 'locate_points')
  _check_points(mesh, points, 'locate_points')
  default = 1e-10 if mesh.dtype == torch.float64 else 1e-5
  tol_xi = default if tol_xi is None else float(tol_xi)
  tol_x = default if tol_x is None else float(tol_x)
  if not (tol_xi >= 0.0 and tol_x >= 0.0):
    raise ValueError('tolerances must be >= 0')
  if not 0 <= int(max_iter) <= 64:
    raise ValueError(f'max_iter must be in 0..64, got {max_iter}')
  grid = candidate_grid(mesh, inflate)
  nodes, bary = basis_tables(mesh.gridpoints_1d)
  element, xi, found = _ops.point_locate(
      points.detach(), mesh.node_coords, mesh.elements, grid, nodes, bary,
      max_iter, tol_xi, tol_x)
  return PointLocation(element, xi, found)


@dataclasses.dataclass(frozen=True, eq=False)
class PointPlan:
  """The found points sorted stably by element, cut into segments (one per
  touched element) and chunks (at most `CHUNK` points of one element)."""
  elements: torch.Tensor      # the mesh's (E, n) int32
  xi: torch.Tensor            # (F, d) in sorted order
  perm: torch.Tensor          # (F,) int64: sorted position -> point
  seg_elem: torch.Tensor      # (S,) int32, ascending
  seg_offsets: torch.Tensor   # (S + 1,) int64
  chunk_elem: torch.Tensor    # (K,) int32
  chunk_start: torch.Tensor   # (K,) int64
  chunk_count: torch.Tensor   # (K,) int32
  nodes: np.ndarray
  bary: np.ndarray
  num_points: int
  num_nodes: int
  ndim: int
  _cache: dict = dataclasses.field(default_factory=dict, repr=False,
                                   compare=False)

  @property
  def num_found(self) -> int:
    return self.perm.numel()

  @classmethod
  def build(cls, mesh, element, xi) -> 'PointPlan':
    dev = mesh.device
    hit = torch.nonzero(element >= 0).reshape(-1)
    order = torch.sort(element[hit], stable=True).indices
    perm = hit[order].to(torch.int64).contiguous()
    sorted_elem = element[perm]
    seg_elem, counts = torch.unique_consecutive(sorted_elem,
                                                return_counts=True)
    counts = counts.to(torch.int64)
    seg_offsets = torch.zeros(seg_elem.numel() + 1, dtype=torch.int64,
                              device=dev)
    seg_offsets[1:] = torch.cumsum(counts, 0)
    nchunk = (counts + CHUNK - 1) // CHUNK
    seg_of = torch.repeat_interleave(
        torch.arange(seg_elem.numel(), device=dev), nchunk)
    first = torch.cumsum(nchunk, 0) - nchunk
    within = torch.arange(seg_of.numel(), device=dev) - first[seg_of]
    chunk_start = seg_offsets[seg_of] + within * CHUNK
    chunk_count = torch.clamp(seg_offsets[seg_of + 1] - chunk_start, max=CHUNK)
    nodes, bary = basis_tables(mesh.gridpoints_1d)
    return cls(
        elements=mesh.elements, xi=xi[perm].contiguous(), perm=perm,
        seg_elem=seg_elem.to(torch.int32).contiguous(),
        seg_offsets=seg_offsets,
        chunk_elem=seg_elem[seg_of].to(torch.int32).contiguous(),
        chunk_start=chunk_start.to(torch.int64).contiguous(),
        chunk_count=chunk_count.to(torch.int32).contiguous(),
        nodes=nodes, bary=bary, num_points=element.numel(),
        num_nodes=mesh.num_nodes, ndim=mesh.ndim)

  @property
  def scatter_csr(self):
    """(offsets (N + 1,) int64, slots int32): the inverse map of the rows
    `elements[seg_elem]`, slots ascending per node, for `sfem_scatter_csr`."""
    if 'csr' not in self._cache:
      flat = self.elements[self.seg_elem.long()].reshape(-1).long()
      if flat.numel() >= 2 ** 31:
        raise ValueError('too many touched element slots for int32')
      slots = torch.sort(flat, stable=True).indices.to(torch.int32)
      offsets = torch.zeros(self.num_nodes + 1, dtype=torch.int64,
                            device=flat.device)
      offsets[1:] = torch.cumsum(
          torch.bincount(flat, minlength=self.num_nodes), 0)
      self._cache['csr'] = (offsets.contiguous(), slots.contiguous())
    return self._cache['csr']


class _Eval(torch.autograd.Function):
  """ev(u); backward is the transpose (not-found points carry no gradient)."""

  @staticmethod
  def forward(ctx, u, ev, fill):
    ctx.ev = ev
    return ev._eval(u, fill)

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, g):
    return ctx.ev._transpose(g), None, None


class _Transpose(torch.autograd.Function):
  """ev.transpose(w); backward is the evaluation (0 at not-found points)."""

  @staticmethod
  def forward(ctx, w, ev):
    ctx.ev = ev
    return ev._transpose(w)

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, g):
    return ctx.ev._eval(g, 0.0), None


class PointEvaluator:
  """Evaluation of nodal fields at fixed points and its transpose.

  `found` (M,) bool, `element` (M,) int32 and `xi` (M, d) are the location;
  `ev(u)` samples, `ev.transpose(w)` spreads point weights to the nodes as
  `Mesh.scatter` would (periodic images are not summed)."""

  def __init__(self, mesh, element, xi):
    self.mesh = mesh
    self.element = element
    self.xi = xi
    self.found = element >= 0
    self.plan = PointPlan.build(mesh, element, xi)

  @classmethod
  def create(cls, mesh, points, **locate_kwargs) -> 'PointEvaluator':
    """Locates `points` (M, d) in `mesh` and builds the plan."""
    loc = locate_points(mesh, points, **locate_kwargs)
    return cls(mesh, loc.element, loc.xi)

  @classmethod
  def from_location(cls, mesh, element, xi) -> 'PointEvaluator':
    """Builds the plan from a given location.  Everything a kernel would
    dereference is checked here, on the host, before any launch."""
    who = 'PointEvaluator.from_location'
    _check_mesh(mesh, who)
    if not (isinstance(element, torch.Tensor) and isinstance(xi, torch.Tensor)):
      raise ValueError(f'{who}: element and xi must be torch.Tensors')
    if xi.requires_grad:
      raise NotImplementedError(
          f'{who}: derivatives with respect to point positions')
    if element.dim() != 1 or element.dtype not in (torch.int32, torch.int64):
      raise ValueError(f'{who}: element must be an (M,) int32 or int64 '
                       f'tensor; got {tuple(element.shape)}, {element.dtype}')
    if tuple(xi.shape) != (element.shape[0], mesh.ndim):
      raise ValueError(f'{who}: expected xi of shape '
                       f'({element.shape[0]}, {mesh.ndim}), got '
                       f'{tuple(xi.shape)}')
    if xi.dtype != mesh.dtype:
      raise ValueError(f'{who}: xi must have the mesh dtype {mesh.dtype}, '
                       f'got {xi.dtype}')
    if element.device != mesh.device or xi.device != mesh.device:
      raise ValueError(f'{who}: element and xi must be on the mesh device '
                       f'{mesh.device}')
    E = mesh.num_elements
    if bool(((element < -1) | (element >= E)).any()):
      raise ValueError(f'{who}: element ids must be -1 or in [0, {E})')
    found = element >= 0
    rows = mesh.elements[element[found].long()]
    if bool((rows < 0).any()) or bool((rows >= mesh.num_nodes).any()):
      raise ValueError(f'{who}: a point lies in a padded element row (-1) or '
                       'a row with node ids outside the mesh')
    xf = xi[found]
    if not bool(torch.isfinite(xf).all()) or bool((xf.abs() > XI_LIMIT).any()):
      raise ValueError(f'{who}: xi must be finite with |xi| <= {XI_LIMIT}')
    return cls(mesh, element.to(torch.int32).contiguous(),
               xi.detach().contiguous())

  # ------------------------------------------------------------------ apply
  def _field_check(self, t, rows, what, name):
    if not isinstance(t, torch.Tensor):
      raise ValueError(f'{name}: expected a torch.Tensor')
    if t.dim() not in (1, 2) or t.shape[0] != rows:
      raise ValueError(f'{name}: expected {what} of shape ({rows},) or '
                       f'({rows}, C), got {tuple(t.shape)}')
    if t.dtype != self.mesh.dtype or t.device != self.mesh.device:
      raise ValueError(f'{name}: expected the dtype and device of the mesh '
                       f'({self.mesh.dtype}, {self.mesh.device}); got '
                       f'{t.dtype}, {t.device}')

  def _eval(self, u, fill):
    from swirl_fem_amd import _ops
    from swirl_fem_amd.core.layout import is_component_major
    u = u.detach()
    if not (u.is_contiguous() or is_component_major(u)):
      u = u.contiguous()
    return _ops.point_eval(u, self.plan, float(fill))

  def _transpose(self, w):
    from swirl_fem_amd import _ops
    return _ops.point_eval_t(w.detach(), self.plan)

  def __call__(self, u, fill=float('nan')):
    """`u` (N,) or (N, C) (row-major or component-major) at the points:
    (M,) or (M, C); not-found points get `fill`."""
    self._field_check(u, self.mesh.num_nodes, 'a nodal field', 'ev(u)')
    if torch.is_grad_enabled() and u.requires_grad:
      return _Eval.apply(u, self, fill)
    return self._eval(u, fill)

  def transpose(self, w):
    """Point weights `w` (M,) or (M, C) spread to the nodes: (N,) or (N, C)
    with out[n] = sum_m w[m] l_n(x_m).  Weights of not-found points are
    ignored; the sum runs in a fixed order (bitwise reproducible)."""
    self._field_check(w, self.element.numel(), 'point weights',
                      'ev.transpose(w)')
    if torch.is_grad_enabled() and w.requires_grad:
      return _Transpose.apply(w, self)
    return self._transpose(w)


__all__ = ['CandidateGrid', 'PointEvaluator', 'PointLocation', 'PointPlan',
           'basis_tables', 'candidate_grid', 'locate_points']
