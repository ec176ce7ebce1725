"""Right-preconditioned BiCGStab on MI355X device tensors.

The Krylov method for the non-symmetric systems an advective term produces
(`HelmholtzOperator` with `velocity=`); the design mirrors `linalg/cg.py`.
With right preconditioning, A M y = b and x = M y, the recurrence's r is the
true residual b - A x, so the solve stops on

    r . r <= max(tol^2 b . b, atol^2)

whatever M is.  The scalars (rho, alpha, omega, beta, the inner products, a
done flag and a status) live in a small device array
(`_lib.SFEM_BICGSTAB_NSCALARS` doubles, include/sfem.h "BiCGStab"); every
vector update is a fused HIP kernel that reads them there, so an iteration
issues no host synchronisation.  The stop test runs on the device each
iteration, every kernel after it is a no-op, and the host polls the flag every
`check_every` iterations: iterates and counts equal those of a loop that tests
every iteration.

One iteration, with phat = M p and shat = M s:

    1. p = r + beta (p - omega v)             [phat = dinv p]
       v = A phat;  r0 . v  ->  alpha = rho / r0 . v
    2. s = r - alpha v, with s . s            [shat = dinv s]
       t = A shat
    3. one pass for (t . s, t . t)            omega = t . s / t . t
    4. x += alpha phat + omega shat;  r = s - omega t, with r . r and r0 . r

that is four fused vector kernels, the reduction r0 . v (which has to sit
between the first apply and kernel 2: alpha is needed to form s), two applies
and three one-thread scalar launches.  A preconditioner that offers
`jacobi_diagonal()` (`linalg/jacobi.py`) is folded into kernels 1, 2 and 4;
any other M is called as a function on p and s.

If s . s is already under the threshold the iteration ends after its first
half (x += alpha phat, r = s) and counts as one iteration.  rho = 0 and
omega = 0 end the solve with the status 'breakdown_rho' / 'breakdown_omega'
(r0 . v = 0: 'breakdown_alpha') and a warning; nothing is divided by them and
x is the last iterate.
"""

from __future__ import annotations

import torch

from swirl_fem_amd import _lib
from swirl_fem_amd import _ops
from swirl_fem_amd.linalg import _driver


class _Scalars:
  """Slots of the device scalar array (include/sfem.h)."""
  RHO, RHO_NEW, ALPHA, OMEGA, BETA, R0V, SS, TS, TT, RR, BB = range(11)
  THRESHOLD, DONE, ITERS, STATUS, HALF, RESIDUAL = range(11, 17)


class BiCGStabRunner:
  """State of one solve; `step()` enqueues exactly one iteration."""

  def __init__(self, A, b, x0=None, *, tol=1e-5, atol=0.0, maxiter=None,
               M=None):
    if not isinstance(b, torch.Tensor):
      raise TypeError(f'bicgstab operates on device tensors, got {type(b)}')
    if not b.is_cuda:
      raise RuntimeError('swirl_fem_amd.linalg.bicgstab runs on MI355X device '
                         'tensors (there is no CPU fallback)')
    if b.dtype not in (torch.float32, torch.float64):
      raise TypeError(f'unsupported dtype {b.dtype}')
    self.A, self.M = A, M
    self.tol, self.atol = float(tol), float(atol)
    self.maxiter = 10 * b.numel() if maxiter is None else int(maxiter)
    self.shape = tuple(b.shape)
    b = b.contiguous()
    S = _Scalars
    self.s = torch.zeros(_lib.SFEM_BICGSTAB_NSCALARS, dtype=torch.float64,
                         device=b.device)
    flat = lambda t: t.reshape(-1)
    self.x = (torch.zeros_like(b) if x0 is None
              else x0.to(b.dtype).contiguous().clone())
    self.r = (b.clone() if x0 is None
              else (b - A(self.x).reshape(self.shape)).contiguous())
    self.r0 = self.r.clone()          # the shadow residual
    self.p = torch.zeros_like(b)
    self.v = torch.zeros_like(b)
    self.sv = torch.empty_like(b)
    self.dinv = None
    probe = getattr(M, 'jacobi_diagonal', None)
    if probe is not None:
      dinv = probe()
      if dinv is not None and dinv.numel() == b.numel():
        self.dinv = dinv.to(b.dtype).reshape(-1).contiguous()
    if self.dinv is not None:
      self.phat, self.shat = torch.empty_like(b), torch.empty_like(b)
    else:
      self.phat, self.shat = self.p, self.sv
    _ops.bicgstab_dot(flat(b), flat(b), self.s, S.BB)
    _ops.bicgstab_dot(flat(self.r), flat(self.r), self.s, S.RR)
    _ops.bicgstab_dot(flat(self.r0), flat(self.r), self.s, S.RHO_NEW)
    _ops.bicgstab_scalars(self.s, 0, self.maxiter, self.tol, self.atol)
    self.issued = 0

  def _apply(self, u):
    out = self.A(u)
    if tuple(out.shape) != self.shape or out.dtype != u.dtype:
      raise ValueError('bicgstab: A must map a vector to one of the same '
                       'shape and dtype')
    return out.contiguous()

  def _precondition(self, u):
    """M u for a preconditioner that is not folded into the kernels."""
    if self.M is None or self.dinv is not None:
      return None
    return self.M(u).reshape(self.shape).contiguous()

  def step(self):
    """Enqueues one iteration (no-ops on the device once the solve is done)."""
    S = _Scalars
    f = lambda t: t.reshape(-1)
    s = self.s
    _ops.bicgstab_update_p(f(self.p), f(self.phat), f(self.r), f(self.v),
                           self.dinv, s)
    phat = self._precondition(self.p)
    phat = self.phat if phat is None else phat
    self.v = self._apply(phat)
    _ops.bicgstab_dot(f(self.r0), f(self.v), s, S.R0V)
    _ops.bicgstab_scalars(s, 1, self.maxiter, self.tol, self.atol)
    _ops.bicgstab_update_s(f(self.sv), f(self.shat), f(self.r), f(self.v),
                           self.dinv, s)
    _ops.bicgstab_scalars(s, 2, self.maxiter, self.tol, self.atol)
    shat = self._precondition(self.sv)
    shat = self.shat if shat is None else shat
    t = self._apply(shat)
    _ops.bicgstab_dot(f(t), f(self.sv), s, S.TS, two=True)
    _ops.bicgstab_update_xr(f(self.x), f(self.r), f(phat), f(shat),
                            f(self.sv), f(t), f(self.r0), s)
    _ops.bicgstab_scalars(s, 3, self.maxiter, self.tol, self.atol)
    self.issued += 1

  def done(self) -> bool:
    """Synchronising poll of the device flag."""
    return bool(self.s[_Scalars.DONE].item() != 0.0)

  def info(self):
    scal = self.s.cpu()
    status = _lib.BICGSTAB_STATUS.get(int(scal[_Scalars.STATUS].item()),
                                      'unknown')
    if status == 'running' and self.issued >= self.maxiter:
      status = 'maxiter'
    return {'residual': self.s[_Scalars.RESIDUAL].clone(),
            'num_iterations': int(scal[_Scalars.ITERS].item()),
            'status': status}


def bicgstab(A, b, x0=None, *, tol=1e-5, atol=0.0, maxiter=None, M=None,
             check_every=16):
  """Solves A x = b for a general (non-symmetric) A with right-preconditioned
  BiCGStab.

  Args:
    A: callable, device tensor -> device tensor of the same shape.
    b: right-hand side, a float32 / float64 device tensor.
    x0: initial guess (zeros if None).
    tol, atol: stop when r . r <= max(tol^2 b . b, atol^2), r = b - A x.
    maxiter: maximum number of iterations (default 10 * size).
    M: right preconditioner, a callable approximating A^-1; one that offers
      `jacobi_diagonal()` is fused into the vector updates.
    check_every: the host polls the device flag this often.

  Returns:
    `(x, info)`, info = {'residual': r . r (0-dim device tensor),
    'num_iterations': full iterations (a stop after the first half-step counts
    as one), 'status': 'converged' | 'maxiter' | 'breakdown_rho' |
    'breakdown_omega' | 'breakdown_alpha'}.  After a breakdown x is the last
    iterate, not a solution to `tol`; a RuntimeWarning says so.
  """
  run = BiCGStabRunner(A, b, x0, tol=tol, atol=atol, maxiter=maxiter, M=M)
  check_every = max(1, int(check_every))
  while not run.done() and run.issued < run.maxiter:
    for _ in range(min(check_every, run.maxiter - run.issued)):
      run.step()
  info = run.info()
  _driver.warn_on_breakdown('bicgstab', info)
  return run.x, info


class _TransposeSolve(torch.autograd.Function):
  """x = A^-1 b with the adjoint A^-T g solved by the same routine on At."""

  @staticmethod
  def forward(ctx, b, A, At, kwargs, info_out):
    x, info = bicgstab(A, b.detach(), **kwargs)
    if info_out is not None:
      info_out.update(info)
    ctx.At, ctx.kwargs = At, kwargs
    return x

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, grad_x):
    # d<x, g>/db = A^-T g
    grad_b, _ = bicgstab(ctx.At, grad_x.detach().contiguous(), **ctx.kwargs)
    return grad_b, None, None, None, None


def transpose_solve(A, At, b, info_out=None, **kwargs):
  """`bicgstab(A, b, **kwargs)[0]` that autograd can differentiate with
  respect to `b`: the cotangent is obtained by a second BiCGStab solve with
  `At`, a callable that applies the transpose of `A` (for a Helmholtz
  operator with a velocity: `op.linear_operator(l0, l1, transpose=True)`) --
  the counterpart of `linalg.cg.symmetric_solve` for operators that are not
  symmetric.  The same `kwargs` (tolerances, `M`, `maxiter`) serve both
  solves; a preconditioner `M` should suit both A and A^T, as a Jacobi
  diagonal does.  Gradients with respect to tensors hidden inside `A` are not
  propagated.  `info_out`: a dict that receives the forward solve's `info`."""
  return _TransposeSolve.apply(b, A, At, kwargs, info_out)


__all__ = ['BiCGStabRunner', 'bicgstab', 'transpose_solve']
