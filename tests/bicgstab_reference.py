"""NumPy restatement of right-preconditioned BiCGStab (tests only).

A M y = b, x = M y: r is the true residual b - A x, the shadow residual is
r0 = b - A x0, the stop rule r . r <= max(tol^2 b . b, atol^2).  Returns every
iterate.  The same recurrence as `linalg/bicgstab.py`, including the stop
after the first half-step (x += alpha phat, counted as an iteration)."""

import numpy as np


def bicgstab(A, b, x0=None, tol=1e-5, atol=0.0, maxiter=None, M=None):
  """A, M: callables on (N,) arrays (M None: identity).  Returns
  (x, iterates [x_1, x_2, ...], status)."""
  b = np.asarray(b, np.float64)
  M = M or (lambda v: v)
  x = np.zeros_like(b) if x0 is None else np.array(x0, np.float64)
  r = b - A(x) if x0 is not None else b.copy()
  r0 = r.copy()
  threshold = max(tol * tol * (b @ b), atol * atol)
  maxiter = 10 * b.size if maxiter is None else maxiter
  iterates = []
  if not r @ r > threshold:
    return x, iterates, 'converged'
  rho = r0 @ r
  if rho == 0.0:
    return x, iterates, 'breakdown_rho'
  p = np.zeros_like(b)
  v = np.zeros_like(b)
  alpha = omega = 1.0
  beta = 0.0
  while True:
    p = r + beta * (p - omega * v)
    phat = M(p)
    v = A(phat)
    r0v = r0 @ v
    if r0v == 0.0:
      return x, iterates, 'breakdown_alpha'
    alpha = rho / r0v
    s = r - alpha * v
    if not s @ s > threshold:
      x = x + alpha * phat
      iterates.append(x.copy())
      return x, iterates, 'converged'
    shat = M(s)
    t = A(shat)
    tt = t @ t
    omega = (t @ s) / tt if tt > 0.0 else 0.0
    x = x + alpha * phat + omega * shat
    r = s - omega * t
    iterates.append(x.copy())
    if not r @ r > threshold:
      return x, iterates, 'converged'
    if omega == 0.0:
      return x, iterates, 'breakdown_omega'
    rho_new = r0 @ r
    if rho_new == 0.0:
      return x, iterates, 'breakdown_rho'
    if len(iterates) >= maxiter:
      return x, iterates, 'maxiter'
    beta = (rho_new / rho) * (alpha / omega)
    rho = rho_new
