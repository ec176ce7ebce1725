"""p-multigrid preconditioning of the fused elasticity solves.

`ElasticityPMultigrid(op, lambda0)` is one V-cycle over polynomial orders of
the same elements (default p -> p // 2 -> ... -> 1) for `K + lambda0 M_rho`
(`ElasticityOperator`), acting on the flat (N d,) vectors
`solve_elasticity` gives CG: dof (node i, component c) at i d + c.  It is the
vector analogue of `linalg/pmg.py` and takes everything scalar from there:
coarse meshes and numbering, the facet rule, owner bits, the 1D interpolation,
the Chebyshev coefficients, the fused smoother step `sfem_cheb_step`, the
ELL coarse polynomial `sfem_ell_chebyshev` and the r.r-stopping CG path.

What is its own:
* fixed components are per component (a roller fixes one, a clamp all): the
  facet rule runs on every component's mask, and the transfers
  (`sfem_pmg_prolong_vec`, `sfem_pmg_restrict_vec`) take plain index rows and
  one flag byte per node, bit c set when component c is fixed;
* every level is a `FiniteElementSpace` with the Gauss rule of the solve for
  its order (p_c + (d + 1) // 2 points) and an `ElasticityOperator` on it.
  Scalar coefficients pass through; (E, Q^d) arrays of lambda, mu and rho
  become per-element means weighted by W = w detJ (`pmg.coarse_coefficient`'s
  rule);
* a level applies its operator element-locally and sums with
  `sfem_scatter_csr(ncomp = d)`, the finest level included
  (`ElasticityOperator.apply` assembles with atomics), so every sum of the
  V-cycle has a fixed order and M is bitwise reproducible;
* the coarsest level's matrix is the block matrix of order 1, assembled on
  the host from d 2^d element-local applies on unit vectors, fixed rows and
  columns zero, stored in ELL (at most 81 entries per row in 3D, 18 in 2D).

The smoother is point Jacobi under Chebyshev: it degrades as nu -> 0.5 (the
iteration counts grow about fivefold from nu = 0.3 to 0.49).
"""

from __future__ import annotations

import numpy as np
import torch

from swirl_fem_amd import _ops
from swirl_fem_amd.core.interpolation import NodeType
from swirl_fem_amd.core.interpolation import Quadrature1D
from swirl_fem_amd.linalg import pmg
from swirl_fem_amd.linalg.pmg import PMultigridPreconditioner


def flag_bytes(fixed: torch.Tensor) -> torch.Tensor:
  """(N,) uint8 from (N, d) bool: bit c set iff component c is fixed."""
  d = fixed.shape[1]
  w = torch.tensor([1 << c for c in range(d)], dtype=torch.int32,
                   device=fixed.device)
  return (fixed.to(torch.int32) * w).sum(dim=1).to(torch.uint8).contiguous()


def coarse_fixed(fixed: torch.Tensor, fel: torch.Tensor, celems: torch.Tensor,
                 num_coarse: int, ndim: int, pf: int, pc: int) -> torch.Tensor:
  """(N_c, d) bool: `pmg.coarse_dirichlet` (the facet rule) on each
  component's mask.  `fixed` (N_f, d) bool, `fel` / `celems` the fine / coarse
  index rows (int64)."""
  out = torch.zeros((num_coarse, ndim), dtype=torch.bool, device=fixed.device)
  flat = celems.reshape(-1)
  for c in range(fixed.shape[1]):
    loc = pmg.coarse_dirichlet(fixed[:, c][fel], ndim, pf, pc)
    out[flat, c] = loc.reshape(-1)
  return out


def element_mean(coef, weights):
  """A Lame parameter or density as the coarse levels take it: a scalar
  unchanged, (E, Q) point values as the (E,) means weighted by `weights`."""
  if not isinstance(coef, torch.Tensor):
    return coef
  w = weights.to(torch.float64)
  mean = (coef.to(torch.float64) * w).sum(dim=1) / w.sum(dim=1)
  return mean.to(coef.dtype).contiguous()


class _Level:
  """Operator, smoother data and work vectors of one order."""

  def __init__(self, mesh, op, lambda0, dinv):
    self.mesh, self.op = mesh, op
    self.N, self.d = mesh.num_nodes, mesh.ndim
    self.mask = None if op.mask is None else op.mask.reshape(-1)
    self.fixed = (torch.zeros((self.N, self.d), dtype=torch.bool,
                              device=dinv.device) if op.mask is None
                  else op.mask == 0)
    self.lambda0 = lambda0
    self.offsets, self.slots = mesh.assembly_plan().csr()
    self.dinv = dinv
    n, dt, dev = dinv.numel(), dinv.dtype, dinv.device
    self.x, self.d_, self.ax, self.r, self.b = (
        torch.zeros(n, dtype=dt, device=dev) for _ in range(5))
    self.cheb = None
    self.lam_max = None
    self.transfer = None

  def apply(self, u, out):
    """out = mask * (fixed-order sum of the element-local operator on u)."""
    N, d = self.N, self.d
    loc = self.op.apply_local(
        _ops.gather_rows(u.view(N, d), self.mesh.elements), self.lambda0)
    _ops.scatter_csr(loc.reshape(-1, d), self.offsets, self.slots, N, ncomp=d,
                     out=out.view(N, d))
    if self.mask is not None:
      out.mul_(self.mask)
    return out


class ElasticityPMultigrid:
  """One V-cycle of p-multigrid for `K + lambda0 M_rho`.

  `op`: the `ElasticityOperator` CG solves with (GLL nodes, one partition, no
  ensemble, no periodic images).  `orders`: the order of every level, finest
  first (default p, p // 2, ..., 1).  `smoother_degree`: Chebyshev-Jacobi
  steps before and after the coarse correction on every level but the
  coarsest.  `coarse_steps`: degree of the coarsest level's polynomial (None:
  enough to reduce its error bound to `pmg.COARSE_REDUCTION`).  `bounds`: the
  spectrum estimates to use instead of computing them, as `spectral_bounds()`
  returns them.

  M r for a flat (N d,) vector r: pre-smooth from x = 0, residual, restrict,
  recurse, prolong and add, post-smooth with the same polynomial; order 1
  applies a fixed Chebyshev polynomial of its Jacobi-scaled block matrix.
  Symmetric positive definite, bitwise reproducible; the result lives in a
  buffer of the preconditioner, valid until the next call.  As a callable
  `(op, lambda0) -> M` the class itself is what `solve_elasticity(...,
  preconditioner=)` takes; `functools.partial` sets the options.
  """

  capturable = False        # graph capture is out of scope
  stops_on_residual = True
  # a solve takes 10-20 iterations of many launches each: CG polls its flag
  # every other one (the default of 16 would issue up to 15 V-cycles too many)
  check_every = 2

  _dinv = PMultigridPreconditioner._dinv
  _store_ell = PMultigridPreconditioner._store_ell
  _steps_for = PMultigridPreconditioner._steps_for

  def __init__(self, op, lambda0=0.0, *, orders=None, smoother_degree=2,
               coarse_steps=None, bounds=None):
    from swirl_fem_amd.core import operators
    if not isinstance(op, operators.ElasticityOperator):
      raise TypeError('ElasticityPMultigrid takes an ElasticityOperator, got '
                      f'{type(op).__name__}')
    fes = op.fespace
    mesh = fes.mesh
    if mesh.axis_name is not None or mesh.neighbor_plan is not None:
      raise NotImplementedError('elasticity p-multigrid on a partitioned mesh')
    gi = mesh.exchange_gather_indices
    if gi is not None and gi.numel() > 0:
      raise NotImplementedError('elasticity p-multigrid on a mesh with '
                                'periodic images')
    pmg._check_mesh(mesh)      # ensembles, ndim, GLL nodes, padded elements
    p = mesh.order
    orders = (pmg.default_orders(p) if orders is None
              else [int(o) for o in orders])
    if (not orders or orders[0] != p or orders[-1] != 1 or
        any(b >= a for a, b in zip(orders, orders[1:]))):
      raise ValueError(f'orders must fall strictly from {p} to 1; got {orders}')
    if smoother_degree < 1:
      raise ValueError('smoother_degree must be >= 1')
    self.lambda0 = float(lambda0)
    self.orders, self.degree = orders, int(smoother_degree)
    self.dtype, self.device = fes.dtype, fes.device
    self.ndim = mesh.ndim
    self.levels = [_Level(mesh, op, self.lambda0,
                          self._dinv(op.diagonal(self.lambda0).reshape(-1)))]
    if len(orders) > 1:
      W = op.point_weights()
      self._coefs = tuple(element_mean(c, W) for c in (op.lam, op.mu, op.rho))
    for pc in orders[1:]:
      self.levels.append(self._coarse_level(self.levels[-1], pc))
    if bounds is not None and len(bounds['lam_max']) != len(orders) - 1:
      raise ValueError(f"bounds: {len(bounds['lam_max'])} lam_max values for "
                       f'{len(orders) - 1} smoothed levels')
    for i, lev in enumerate(self.levels[:-1]):
      lev.lam_max = (float(bounds['lam_max'][i]) if bounds is not None
                     else pmg.lanczos_max(lev.apply, lev.dinv))
      lev.cheb = pmg._cheb_coefficients(pmg.SMOOTHER_LOW * lev.lam_max,
                                        pmg.SMOOTHER_HIGH * lev.lam_max,
                                        self.degree)
    self._coarse_setup(self.levels[-1], coarse_steps,
                       None if bounds is None else tuple(bounds['coarse']))

  def spectral_bounds(self):
    """The spectrum estimates this preconditioner uses (the `bounds` argument
    that reproduces them)."""
    return {'lam_max': [lev.lam_max for lev in self.levels[:-1]],
            'coarse': tuple(self.coarse_bounds)}

  # ---------------------------------------------------------------- setup
  def _coarse_level(self, fine, pc):
    from swirl_fem_amd.core.fespace import FiniteElementSpace
    fmesh = fine.mesh
    d, pf = fmesh.ndim, fmesh.order
    cmesh, celems = pmg.coarse_mesh(fmesh, pc)
    fel = fmesh.elements.to(torch.int64)
    cfixed = coarse_fixed(fine.fixed, fel, celems, cmesh.num_nodes, d, pf, pc)
    fes = FiniteElementSpace.create(cmesh, Quadrature1D.create(
        num_points=pc + (d + 1) // 2, quadrature_type=NodeType.GAUSS_LEGENDRE))
    lam, mu, rho = self._coefs
    cop = fes.elasticity_operator(cfixed if bool(cfixed.any()) else None,
                                  lame_lambda=lam, lame_mu=mu, density=rho)
    lev = _Level(cmesh, cop, self.lambda0,
                 self._dinv(cop.diagonal(self.lambda0).reshape(-1)))
    lev.fespace = fes
    fine.transfer = dict(
        cidx=celems.to(torch.int32).contiguous(),
        fidx=fel.to(torch.int32).contiguous(),
        owner=pmg.owner_bits(fel, fmesh.num_nodes),
        cfix=flag_bytes(cfixed), ffix=flag_bytes(fine.fixed),
        mat=torch.as_tensor(pmg.interpolation_1d(pc, pf), dtype=self.dtype,
                            device=self.device).contiguous(),
        local=torch.zeros(celems.numel() * d, dtype=self.dtype,
                          device=self.device),
        pc=pc + 1, pf=pf + 1)
    return lev

  def _local_matrix(self, lev):
    """The order-1 block matrix (CSR, fp64; dof (i, c) at i d + c; fixed rows
    and columns zero) from d 2^d element-local applies on unit vectors."""
    import scipy.sparse as sp
    mesh = lev.mesh
    E, n = mesh.elements.shape
    d, nd = lev.d, n * lev.d
    cols_k = []
    for j in range(n):
      for c in range(d):
        u = torch.zeros((E, n, d), dtype=self.dtype, device=self.device)
        u[:, j, c] = 1.0
        cols_k.append(lev.op.apply_local(u, self.lambda0).double()
                      .reshape(E, nd).cpu().numpy())
    K = np.stack(cols_k, axis=-1)                    # (E, n d, n d)
    el = mesh.elements.cpu().numpy().astype(np.int64)
    dofs = (el[:, :, None] * d + np.arange(d)[None, None, :]).reshape(E, nd)
    rows = np.repeat(dofs[:, :, None], nd, axis=2).reshape(-1)
    cols = np.repeat(dofs[:, None, :], nd, axis=1).reshape(-1)
    A = sp.csr_matrix((K.reshape(-1), (rows, cols)),
                      shape=(lev.N * d, lev.N * d))
    A.sum_duplicates()
    keep = (~lev.fixed).reshape(-1).cpu().numpy().astype(np.float64)
    A = (sp.diags(keep) @ A @ sp.diags(keep)).tocsr()
    A.eliminate_zeros()
    return A

  def _coarse_setup(self, lev, steps, bounds=None):
    """The order-1 matrix in ELL form and the bounds of its Jacobi-scaled
    spectrum (`bounds`: given instead), as the scalar `_coarse_setup`."""
    import scipy.sparse as sp
    A = self._local_matrix(lev)
    diag = A.diagonal()
    interior = np.nonzero(diag > 0)[0]
    if interior.size == 0:
      raise ValueError('the coarse operator has no free rows')
    if bounds is not None:
      self.coarse_bounds = tuple(float(b) for b in bounds)
    else:
      Ai = A[interior][:, interior]
      dm = 1.0 / np.sqrt(Ai.diagonal())
      lmin, lmax = pmg.jacobi_scaled_extremes(
          sp.diags(dm) @ Ai @ sp.diags(dm), self.ndim)
      if not lmin > 1e-12 * lmax:
        raise NotImplementedError(
            'p-multigrid needs a positive definite operator (the coarse '
            'matrix is singular: no fixed component and lambda0 rho = 0?)')
      self.coarse_bounds = (0.9 * lmin, 1.05 * lmax)
    self.coarse_steps = self._steps_for(steps)
    dinv = np.zeros(A.shape[0])
    dinv[interior] = 1.0 / diag[interior]
    self._store_ell(lev, A, dinv)

  # ----------------------------------------------------------------- apply
  def restrict(self, l, r, out):
    """out (level l + 1) = P^T r (level l)."""
    t, coarse = self.levels[l].transfer, self.levels[l + 1]
    d = self.ndim
    _ops.pmg_restrict_vec(r, t['local'], t['cidx'], t['fidx'], t['owner'],
                          t['cfix'], t['ffix'], t['mat'], d, t['pc'], t['pf'])
    _ops.scatter_csr(t['local'].view(-1, d), coarse.offsets, coarse.slots,
                     coarse.N, ncomp=d, out=out.view(coarse.N, d))
    return out

  def prolong(self, l, xc, out, add=False):
    """out (level l) = P xc (level l + 1); add: out += P xc."""
    t = self.levels[l].transfer
    return _ops.pmg_prolong_vec(xc, out, t['cidx'], t['fidx'], t['owner'],
                                t['cfix'], t['ffix'], t['mat'], self.ndim,
                                t['pc'], t['pf'], add)

  def smooth(self, l, b, from_zero):
    """x of level l after `smoother_degree` Chebyshev steps on b."""
    lev = self.levels[l]
    for k, (a, c) in enumerate(lev.cheb):
      if k == 0 and from_zero:
        _ops.cheb_step(lev.x, lev.d_, None, b, lev.dinv, None, 0.0, c,
                       _ops.CHEB_FIRST)
        continue
      lev.apply(lev.x, lev.ax)
      _ops.cheb_step(lev.x, lev.d_, lev.ax, b, lev.dinv, None, a, c,
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
    if r.dim() != 1 or r.numel() != self.levels[0].dinv.numel():
      raise ValueError('ElasticityPMultigrid takes a flat (N d,) vector')
    r = r.to(self.dtype).contiguous()
    return self._cycle(0, r)
