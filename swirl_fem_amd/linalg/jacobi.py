"""Jacobi (diagonal) preconditioning of the fused Helmholtz / Poisson solves.

`JacobiPreconditioner(op, lambda0, lambda1)` is `z = dinv (.) r` with `dinv`
the inverse of the assembled diagonal of `lambda0 B + lambda1 A`, computed
matrix-free by `op.diagonal` (`sfem_helmholtz_diag`, the element diagonals in
exactly the form the fused apply uses, assembled in a fixed order).  It is the
standard preconditioner of matrix-free spectral-element Helmholtz solves
(Nek5000's default for them, the CEED bake-off problems' with CG).

`linalg.cg.CGRunner` recognises it through `jacobi_diagonal()` and folds it
into its two vector updates (`sfem_cg_update_r_jacobi`,
`sfem_cg_update_xp_jacobi`): z is never stored.  Everything else (ensemble CG,
`symmetric_solve`, callers with a `dot_fn`) calls it as a plain function.
"""

from __future__ import annotations

import torch

from swirl_fem_amd.core import layout


class JacobiPreconditioner:
  """`z = dinv (.) r`, dinv = 1 / d on interior nodes and 0 on Dirichlet nodes
  (the rows the operator zeroes; d = 0 there).

  `op_or_diag`: an operator with `diagonal(lambda0, lambda1)`
  (`HelmholtzOperator`, `TwoGridHelmholtzOperator`) or the assembled diagonal
  itself, an (N,) device tensor.

  `reduce_max`: in-place maximum over the partitions of a 1-element device
  tensor, for d_max.  None: taken from the operator's mesh -- the maximum over
  all ranks (`comm.all_reduce_max_`) when the mesh is partitioned -- or no
  reduction for a bare diagonal.  Every rank then scales by the same global
  d_max, so the copies of a shared node get the same dinv and M is one
  symmetric operator.

  strict=True scales dinv by d_max = max_i d_i (as the stepper's lumped-mass
  preconditioner does): every entry of dinv is then >= 1 on interior nodes,
  so  r . M r >= r . r  for every r that vanishes on the Dirichlet nodes (the
  residuals of these solves do), and the reference's stopping rule
  r . M r <= max(tol^2 b . b, atol^2) is at least as strict as with M = None.
  The iterates are those of PCG with the SPD diagonal preconditioner dinv:
  the scale changes the stopping test only.  strict=False: dinv = 1 / d.

  A vector field (N, nc) -- either memory layout -- is preconditioned
  component by component with the one (N,) diagonal.
  """

  capturable = True
  # consistent vectors in, consistent vectors out (on a partition dinv is the
  # same on every holder of a node): partitioned CG accepts it
  consistent = True

  def __init__(self, op_or_diag, lambda0=0.0, lambda1=1.0, strict=True,
               reduce_max=None):
    if isinstance(op_or_diag, torch.Tensor):
      d = op_or_diag
    else:
      d = op_or_diag.diagonal(lambda0, lambda1)
      mesh = op_or_diag.fespace.mesh
      if reduce_max is None and (mesh.axis_name is not None or
                                 mesh.neighbor_plan is not None):
        from swirl_fem_amd.distributed import comm
        reduce_max = comm.all_reduce_max_
    if d.dim() != 1:
      raise ValueError(f'expected an (N,) diagonal, got {tuple(d.shape)}')
    interior = d != 0
    if bool((d[interior] < 0).any()):
      raise ValueError('the diagonal has negative entries: the operator is '
                       'not positive definite')
    dinv = torch.where(interior, 1.0 / torch.where(interior, d,
                                                   torch.ones_like(d)),
                       torch.zeros_like(d))
    if strict:
      top = (d.max() if d.numel() else d.new_zeros(())).reshape(1).clone()
      if reduce_max is not None:
        reduce_max(top)
      dinv = dinv * top
    self.strict = strict
    self._dinv = dinv.contiguous()
    self._laid_out = {}

  def jacobi_diagonal(self) -> torch.Tensor:
    """dinv (N,): the hook through which `CGRunner` fuses the preconditioner
    into its vector updates."""
    return self._dinv

  def __call__(self, r):
    if r.dim() == 1:
      return self._dinv.to(r.dtype) * r
    key = (tuple(r.shape), r.stride(), r.dtype)
    f = self._laid_out.get(key)
    if f is None:        # (the solve's vectors: one layout per caller)
      f = layout.like(self._dinv.to(r.dtype)[:, None].expand(r.shape), r)
      f = self._laid_out[key] = f.clone()
    return f * r
