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


# ----------------------------------------------- the recurrence piece by piece
# The device solver keeps the scalars of the recurrence in one array (the
# slots of include/sfem.h, "BiCGStab") and splits an iteration into four
# vector updates with one-thread scalar phases between them.  The same split
# in NumPy: `update_*` restate the vector updates (what they add to the
# scalars is returned, not stored), `scalar_phase` the phases.  Every sum is
# cleared by the phase that precedes the kernels which add to it: phase 0
# clears r0.v, s.s, t.s, t.t and moves r0.r to rho; phase 1 clears s.s;
# phase 2 clears t.s, t.t, r.r and r0.r; phase 3 clears r0.v.
(RHO, RHO_NEW, ALPHA, OMEGA, BETA, R0V, SS, TS, TT, RR, BB, THRESHOLD, DONE,
 ITERS, STATUS, HALF, RESIDUAL) = range(17)
NSLOTS = 17
STATUS_CODE = {'running': 0.0, 'converged': 1.0, 'maxiter': 2.0,
               'breakdown_rho': 3.0, 'breakdown_omega': 4.0,
               'breakdown_alpha': 5.0}


def omega_of(s):
  """omega = t.s / t.t of the open iteration; 0 after a half-step stop, for
  t.t = 0 (or NaN) and for a quotient that is not finite."""
  if s[HALF] != 0.0 or not s[TT] > 0.0:
    return 0.0
  with np.errstate(all='ignore'):
    w = s[TS] / s[TT]
  return float(w) if np.isfinite(w) else 0.0


def update_p(p, r, v, dinv, s):
  """1.  (p, phat): p = r + beta (p - omega v), phat = dinv p (None: p)."""
  p = r + s[BETA] * (p - s[OMEGA] * v)
  return p, (p if dinv is None else dinv * p)


def update_s(r, v, dinv, s):
  """2.  (s, shat, s.s): s = r - alpha v, shat = dinv s (None: s)."""
  sv = r - s[ALPHA] * v
  return sv, (sv if dinv is None else dinv * sv), sv @ sv


def update_xr(x, phat, shat, sv, t, r0, s):
  """4.  (x, r, r.r, r0.r): x += alpha phat + omega shat, r = s - omega t.
  With omega = 0 (`omega_of`: the half-step stop, t.t = 0) the iteration
  ends after its first half, x += alpha phat and r = s; `t` and `shat` are
  not read (t was never formed after a half-step stop)."""
  omega = omega_of(s)
  x = x + s[ALPHA] * phat
  r = np.array(sv)
  if omega != 0.0:
    x = x + omega * shat
    r = sv - omega * t
  return x, r, r @ r, r0 @ r


def _stop(s, status):
  s[STATUS] = STATUS_CODE[status]
  s[DONE] = 1.0


def scalar_phase(s, phase, maxiter, tol, atol):
  """The scalar array after phase 0..3 (a copy; entries from `NSLOTS` on are
  kept).  Phases 1 to 3 change nothing once `DONE` is set.

  0 starts a solve from BB = b.b, RR = r.r, RHO_NEW = r0.r: threshold
    max(tol^2 b.b, atol^2), rho = r0.r, alpha = omega = 1, beta = 0, counters
    and flags cleared; stops 'converged' on a finite r.r under the threshold,
    'breakdown_rho' on rho = 0 or not finite, 'maxiter' on maxiter <= 0.
  1 alpha = rho / r0.v; r0.v = 0 or an alpha that is not finite stops
    'breakdown_alpha' with alpha untouched.
  2 HALF = (s.s finite and not over the threshold).
  3 closes the iteration: omega, the residual and the count are recorded,
    then in this order a non-finite r.r ('breakdown_omega' if it follows
    omega = 0 in a full step, else 'breakdown_rho'), convergence, omega = 0,
    r0.r = 0 or not finite, maxiter; otherwise beta = (rho_new / rho)
    (alpha / omega) and rho = rho_new."""
  s = np.array(s, np.float64)
  if phase != 0 and s[DONE] != 0.0:
    return s
  with np.errstate(all='ignore'):
    if phase == 0:
      s[THRESHOLD] = max(tol * tol * s[BB], atol * atol)
      s[RHO] = s[RHO_NEW]
      s[[RHO_NEW, R0V, SS, TS, TT]] = 0.0
      s[ALPHA] = s[OMEGA] = 1.0
      s[BETA] = 0.0
      s[RESIDUAL] = s[RR]
      s[[DONE, ITERS, HALF]] = 0.0
      s[STATUS] = STATUS_CODE['running']
      if np.isfinite(s[RR]) and not s[RR] > s[THRESHOLD]:
        _stop(s, 'converged')
      elif s[RHO] == 0.0 or not np.isfinite(s[RHO]):
        _stop(s, 'breakdown_rho')
      elif maxiter <= 0:
        _stop(s, 'maxiter')
    elif phase == 1:
      alpha = s[RHO] / s[R0V]
      if s[R0V] == 0.0 or not np.isfinite(alpha):
        _stop(s, 'breakdown_alpha')
      else:
        s[ALPHA] = alpha
        s[SS] = 0.0
    elif phase == 2:
      s[HALF] = float(np.isfinite(s[SS]) and not s[SS] > s[THRESHOLD])
      s[[TS, TT, RR, RHO_NEW]] = 0.0
    elif phase == 3:
      omega = omega_of(s)
      rr, rho_new, half = s[RR], s[RHO_NEW], s[HALF] != 0.0
      s[OMEGA] = omega
      s[RESIDUAL] = rr
      s[ITERS] += 1.0
      s[R0V] = 0.0
      if not np.isfinite(rr):
        _stop(s, 'breakdown_omega' if omega == 0.0 and not half
              else 'breakdown_rho')
      elif not rr > s[THRESHOLD]:
        _stop(s, 'converged')
      elif omega == 0.0:
        _stop(s, 'breakdown_omega')
      elif rho_new == 0.0 or not np.isfinite(rho_new):
        _stop(s, 'breakdown_rho')
      elif s[ITERS] >= maxiter:
        _stop(s, 'maxiter')
      else:
        s[BETA] = (rho_new / s[RHO]) * (s[ALPHA] / omega)
        s[RHO] = rho_new
    else:
      raise ValueError(f'phase {phase}')
  return s


def bicgstab_by_pieces(A, b, x0=None, tol=1e-5, atol=0.0, maxiter=None,
                       dinv=None):
  """`bicgstab` (with M = diag(dinv)) as the device solver runs it: the
  pieces above in the order of `BiCGStabRunner.step`.  Returns (x, iterates,
  status, iteration count of the scalar array)."""
  b = np.asarray(b, np.float64)
  x = np.zeros_like(b) if x0 is None else np.array(x0, np.float64)
  r = b - A(x) if x0 is not None else b.copy()
  r0 = r.copy()
  p, v = np.zeros_like(b), np.zeros_like(b)
  maxiter = 10 * b.size if maxiter is None else maxiter
  s = np.zeros(NSLOTS)
  s[BB], s[RR], s[RHO_NEW] = b @ b, r @ r, r0 @ r
  phase = lambda s, k: scalar_phase(s, k, maxiter, tol, atol)
  s = phase(s, 0)
  iterates = []
  while s[DONE] == 0.0:
    p, phat = update_p(p, r, v, dinv, s)
    v = A(phat)
    s[R0V] += r0 @ v
    s = phase(s, 1)
    if s[DONE] != 0.0:
      break
    sv, shat, ss = update_s(r, v, dinv, s)
    s[SS] += ss
    s = phase(s, 2)
    t = None
    if s[HALF] == 0.0:
      t = A(shat)
      s[TS] += t @ sv
      s[TT] += t @ t
    x, r, rr, rho_new = update_xr(x, phat, shat, sv, t, r0, s)
    s[RR] += rr
    s[RHO_NEW] += rho_new
    s = phase(s, 3)
    iterates.append(x.copy())
  status = {v: k for k, v in STATUS_CODE.items()}[s[STATUS]]
  return x, iterates, status, int(s[ITERS])
