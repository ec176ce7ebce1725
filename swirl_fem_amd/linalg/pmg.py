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
with; a collocated one through a coloured-assembly copy, a two-grid one
element-locally with a fixed-order sum (`sfem_scatter_csr`), so that every
sum in the V-cycle has a fixed order and the preconditioner is bitwise
reproducible.  Coarse levels are collocated GLL `HelmholtzOperator`s with the
same (lambda0, lambda1), coloured assembly.

`CGRunner` recognises the preconditioner through `stops_on_residual`: it then
stops on the true-residual norm r.r <= max(tol^2 b.b, atol^2) instead of the
reference's r.Mr (an energy norm when M ~ A^-1), with inner products summed in
a fixed order.
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
  if mesh.axis_name is not None or mesh.neighbor_plan is not None:
    raise NotImplementedError('p-multigrid on a partitioned mesh')
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
    # the 2^k fine nodes around each coarse node (k directions inside)
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
    cols = np.stack(combos, axis=-1)                         # (ns, 2^k)
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


def owner_bits(elements: torch.Tensor, num_nodes: int) -> torch.Tensor:
  """(E, ceil(n / 32)) int32 words (bit t of word t // 32: element e owns its
  local node t): every node is owned by the lowest-numbered element that
  contains it."""
  E, n = elements.shape
  el = elements.to(torch.int64)
  eidx = torch.arange(E, device=el.device)[:, None].expand(E, n)
  first = torch.full((num_nodes,), E, dtype=torch.int64, device=el.device)
  first.scatter_reduce_(0, el.reshape(-1), eidx.reshape(-1), reduce='amin')
  owned = first[el] == eidx
  words = (n + 31) // 32
  pad = torch.zeros((E, words * 32), dtype=torch.int64, device=el.device)
  pad[:, :n] = owned.to(torch.int64)
  shift = torch.arange(32, device=el.device, dtype=torch.int64)
  w = (pad.view(E, words, 32) << shift).sum(dim=2)
  w = torch.where(w >= 2 ** 31, w - 2 ** 32, w)
  return w.to(torch.int32).contiguous()


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
  periodic = (mesh.exchange_gather_indices is not None and
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
  xe = mesh.element_coords().double()                        # (E, nf, d)
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
  """

  capturable = True
  stops_on_residual = True

  def __init__(self, op, lambda0=0.0, lambda1=1.0, *, orders=None,
               smoother_degree=2, coarse_steps=None):
    from swirl_fem_amd.core import operators
    if not isinstance(op, (operators.HelmholtzOperator,
                           operators.TwoGridHelmholtzOperator)):
      raise TypeError('PMultigridPreconditioner takes a HelmholtzOperator or '
                      f'a TwoGridHelmholtzOperator, got {type(op).__name__}')
    fes = op.fespace
    mesh = fes.mesh
    _check_mesh(mesh)
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
    for lev in self.levels[:-1]:
      lev.lam_max = self._lanczos_max(lev)
      lev.cheb = _cheb_coefficients(SMOOTHER_LOW * lev.lam_max,
                                    SMOOTHER_HIGH * lev.lam_max, self.degree)
    self._coarse_setup(self.levels[-1], coarse_steps)

  # ---------------------------------------------------------------- setup
  def _fine_level(self, op, dirichlet):
    from swirl_fem_amd.core import operators
    fes, mesh = op.fespace, op.fespace.mesh
    l0, l1 = self.lambda0, self.lambda1
    if isinstance(op, operators.HelmholtzOperator):
      colored = fes.helmholtz_operator(dirichlet, assembly='colored')
      self._fine_colored = colored
      apply_fn = lambda u, out: colored.apply(u, l0, l1, out=out)
    else:
      offsets, slots = mesh.assembly_plan().csr()

      def apply_fn(u, out):
        loc = op.apply_local(mesh.gather(u), l0, l1)
        return _ops.scatter_csr(loc.reshape(-1), offsets, slots,
                                mesh.num_nodes, out=out)
    dinv = self._dinv(op.diagonal(l0, l1))
    return _Level(mesh, op, apply_fn, dirichlet, dinv)

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
    cop = fes.helmholtz_operator(cdir, assembly='auto' if coarsest
                                 else 'colored')
    dinv = self._dinv(cop.diagonal(l0, l1))
    lev = _Level(cmesh, cop, lambda u, out: cop.apply(u, l0, l1, out=out),
                 cdir, dinv)
    lev.fespace = fes
    offsets, slots = cmesh.assembly_plan().csr()
    fine.transfer = dict(
        cidx=encode_rows(celems, cdir), fidx=encode_rows(fel, fine.dirichlet),
        owner=owner_bits(fel, fmesh.num_nodes),
        mat=torch.as_tensor(interpolation_1d(pc, pf), dtype=self.dtype,
                            device=self.device).contiguous(),
        local=torch.zeros(celems.numel(), dtype=self.dtype,
                          device=self.device),
        offsets=offsets, slots=slots, pc=pc + 1, pf=pf + 1)
    return lev

  def _lanczos_max(self, lev):
    """Largest eigenvalue of D^-1 A (interior rows) from LANCZOS_STEPS steps
    of Lanczos on D^-1/2 A D^-1/2 from a fixed start vector."""
    sq = lev.dinv.double().sqrt()
    n = sq.numel()
    g = torch.Generator().manual_seed(12345)
    v = torch.rand(n, generator=g, dtype=torch.float64).to(self.device) - 0.5
    v = v * (sq > 0)
    v = v / v.norm()
    v_prev = torch.zeros_like(v)
    alphas, betas = [], []
    beta = 0.0
    ax = torch.empty(n, dtype=self.dtype, device=self.device)
    for _ in range(min(LANCZOS_STEPS, int((sq > 0).sum()))):
      lev.apply((sq * v).to(self.dtype).contiguous(), ax)
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

  def _coarse_setup(self, lev, steps):
    """The order-1 matrix in ELL form (Dirichlet rows and columns zero) and
    the bounds of its Jacobi-scaled spectrum."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
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
    A.sum_duplicates()
    # periodic images: the fine operator keeps them apart, so does this one
    if lev.dirichlet is not None:
      keep = (~lev.dirichlet).cpu().numpy().astype(np.float64)
      A = (sp.diags(keep) @ A @ sp.diags(keep)).tocsr()
      A.eliminate_zeros()
    diag = A.diagonal()
    interior = np.nonzero(diag > 0)[0]
    if interior.size == 0:
      raise ValueError('the coarse operator has no interior rows')
    Ai = A[interior][:, interior]
    dm = 1.0 / np.sqrt(Ai.diagonal())
    S = sp.diags(dm) @ Ai @ sp.diags(dm)
    if S.shape[0] <= 400:
      ev = np.linalg.eigvalsh(S.toarray())
      lmin, lmax = float(ev[0]), float(ev[-1])
    else:
      lmax = float(spla.eigsh(S, k=1, which='LA', tol=1e-3,
                              return_eigenvectors=False)[0])
      # a few Lanczos steps from the low end (no factorisation of S); the
      # polynomial stays positive definite for any 0 < lmin
      try:
        lmin = float(spla.eigsh(S, k=1, which='SA', tol=1e-2,
                                maxiter=20 * S.shape[0],
                                return_eigenvectors=False)[0])
      except spla.ArpackNoConvergence as exc:
        got = np.sort(exc.eigenvalues)
        lmin = (float(got[0]) if got.size else
                lmax / (4.0 * S.shape[0] ** (2.0 / mesh.ndim)))
    if not lmin > 1e-12 * lmax:
      raise NotImplementedError(
          'p-multigrid needs a positive definite operator (the coarse matrix '
          'is singular: no Dirichlet nodes and lambda0 = 0?)')
    self.coarse_bounds = (0.9 * lmin, 1.05 * lmax)
    if steps is None:
      kappa = self.coarse_bounds[1] / self.coarse_bounds[0]
      steps = math.ceil(0.5 * math.sqrt(kappa) *
                        math.log(2.0 / COARSE_REDUCTION))
      steps = max(2, min(COARSE_MAX_STEPS, steps))
    self.coarse_steps = int(steps)
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
    dinv = np.zeros(N)
    dinv[interior] = 1.0 / diag[interior]
    lev.ell_dinv = torch.as_tensor(dinv, dtype=self.dtype, device=self.device)
    lev.ell_work = torch.zeros(3 * N, dtype=self.dtype, device=self.device)

  # ----------------------------------------------------------------- apply
  def restrict(self, l, r, out):
    """out (level l + 1) = P^T r (level l)."""
    t = self.levels[l].transfer
    _ops.pmg_restrict(r, t['local'], t['cidx'], t['fidx'], t['owner'],
                      t['mat'], self.levels[l].mesh.ndim, t['pc'], t['pf'])
    return _ops.scatter_csr(t['local'], t['offsets'], t['slots'], out.numel(),
                            out=out)

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
