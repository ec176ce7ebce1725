"""NumPy restatement of the device CG, piece by piece (tests only).

The device solver (`linalg/cg.py` over csrc/sfem_core.hip and sfem_pmg.hip)
keeps the scalars of preconditioned CG in one block of 80 doubles (the slots of
include/sfem.h, "CG kernels") and splits an iteration into vector updates with
one-thread scalar phases between them.  The same split in float64 NumPy:
`scalar_phase` / `pmg_scalar_phase` restate the phases, `update_*`, `flush_x`
and `cheb_step` the vector kernels, `cg_by_pieces` loops them in the orders
`CGRunner` issues them.  Vectors are float64 arrays; `dtype` is the type the
device vectors have: alpha and beta are rounded to it where the kernels cast
them, nothing else is.

What a reducing kernel adds to the block goes to ONE address here (the named
slot, or the striped slot `stripe`); the kernels spread it over workgroups and
stripes, which a test compares by the total."""

import numpy as np

(GAMMA, PAP, GAMMA_NEW, ALPHA, BETA, BB, ATOL2, DONE, ITERS, OPEN, STATUS,
 CORR, MEAN, RR) = range(14)
NAMED = 16                    # [0..16): the named scalars
RR_SLOTS = 64                 # [16..80): partial sums of gamma_new
NSLOTS = NAMED + RR_SLOTS
STRIPES = slice(NAMED, NSLOTS)
DOT_SLOTS = 1024              # partial sums of p.Ap an operator accumulates
FOLD_GROUPS = 256
MEAN_SUMS = 4 * RR_SLOTS      # 2 parities x (64 of 1.r, 64 of w.r)
LAZY_MAX = 8
STATUS_CODE = {'running': 0.0, 'converged': 1.0, 'maxiter': 2.0,
               'breakdown_pAp': 3.0, 'breakdown_gamma': 4.0}
DBL_MAX = np.finfo(np.float64).max


def bad_gamma(g):
  """r.Mr that stops the solve: negative or not finite."""
  return not g >= 0.0 or not g <= DBL_MAX


def bad_pap(v):
  """p.Ap that stops the solve: zero or not finite (a negative one is
  divided by)."""
  return v == 0.0 or not v >= -DBL_MAX or not v <= DBL_MAX


def total(values):
  """Sum in extended precision, rounded once."""
  return float(np.sum(np.asarray(values, np.longdouble)))


def _stop(s, status):
  s[STATUS] = STATUS_CODE[status]
  s[DONE] = 1.0


def gamma_new_of(s):
  """gamma_new as every consumer reads it: the named slot plus the stripes."""
  return s[GAMMA_NEW] + s[STRIPES].sum()


def close_iteration(s, maxiter):
  """beta, gamma <- gamma_new (named slot + stripes + [11]), the counter and
  the stop test; the stripes and [11] are cleared."""
  with np.errstate(all='ignore'):
    g = s[GAMMA_NEW]
    for q in range(NAMED, NSLOTS):
      g = g + s[q]
    s[STRIPES] = 0.0
    g = g + s[CORR]
    s[CORR] = 0.0
    s[BETA] = g / s[GAMMA]
    s[GAMMA] = g
    s[ITERS] += 1.0
    if bad_gamma(g):
      _stop(s, 'breakdown_gamma')
    elif not g > s[ATOL2]:
      _stop(s, 'converged')
    elif s[ITERS] >= maxiter:
      _stop(s, 'maxiter')


def set_alpha(s, pap):
  """alpha = gamma / p.Ap and gamma_new cleared, or 'breakdown_pAp' with
  neither touched."""
  if bad_pap(pap):
    _stop(s, 'breakdown_pAp')
    return
  with np.errstate(all='ignore'):
    s[ALPHA] = s[GAMMA] / pap
  s[GAMMA_NEW] = 0.0


def scalar_phase(s, phase, maxiter, tol, atol, partials=None, stored=False):
  """(scalars, partials) after `sfem_cg_scalars` (`stored` False: `partials`
  are the DOT_SLOTS sums an operator accumulates into) or `sfem_cg_scalars_n`
  (`stored` True: any number of stored sums, never written) -- copies.

  2 starts a solve from [5] = b.b and [0] = gamma_0: atol2, counters, flags,
    stripes, [11], [12] cleared; stops on a bad gamma_0 ('breakdown_gamma'),
    gamma_0 <= atol2 ('converged'), maxiter <= 0 ('maxiter').
  0 alpha = gamma / [1] and gamma_new = 0; a bad p.Ap stops with 'breakdown_pAp'
    and leaves alpha and gamma_new alone.
  1 closes the iteration (`close_iteration`) and clears [1].
  3 [1] = sum of the partials;  4 = 3 then 0.
  5 closes the open iteration ([9]) if there is one; unless that stopped the
    solve, 4, and [9] is raised unless p.Ap was bad.
  6 closes the open iteration if there is one.
  7 folds the stripes into [2] and clears them.
  8 [2] = sum of the (stored) partials.
  Once `DONE` is set every phase but 2 leaves the scalars alone.  Partials
  that are accumulated into (not `stored`) are workspace, cleared whether the
  solve is done or not: by phases 1 and 2 when given, and by phase 5."""
  s = np.array(s, np.float64)
  if partials is not None:
    partials = np.array(partials, np.float64)
  if phase in (3, 4, 5, 8) and partials is None:
    raise ValueError(f'phase {phase} needs partials')
  if stored and phase not in (3, 4, 5, 8):
    raise ValueError(f'phase {phase} over stored partials')
  if not 0 <= phase <= 8 or (phase == 8 and not stored):
    raise ValueError(f'phase {phase}')
  psum = None
  if phase in (3, 4, 5, 8):
    count = len(partials) if stored else DOT_SLOTS
    psum = total(partials[:count])
    if phase == 5 and not stored:
      partials[:count] = 0.0
  if phase in (1, 2) and partials is not None and not stored:
    partials[:DOT_SLOTS] = 0.0
  if phase == 2:
    s[ATOL2] = max(tol * tol * s[BB], atol * atol)
    s[[PAP, GAMMA_NEW, ITERS, OPEN, CORR, MEAN]] = 0.0
    s[STRIPES] = 0.0
    s[STATUS] = STATUS_CODE['running']
    s[DONE] = 0.0
    if bad_gamma(s[GAMMA]):
      _stop(s, 'breakdown_gamma')
    elif not s[GAMMA] > s[ATOL2]:
      _stop(s, 'converged')
    elif maxiter <= 0:
      _stop(s, 'maxiter')
    return s, partials
  if s[DONE] != 0.0:
    return s, partials
  if phase == 0:
    set_alpha(s, s[PAP])
  elif phase == 1:
    s[PAP] = 0.0
    close_iteration(s, maxiter)
  elif phase in (3, 4):
    s[PAP] = psum
    if phase == 4:
      set_alpha(s, psum)
  elif phase in (5, 6):
    if s[OPEN] != 0.0:
      s[OPEN] = 0.0
      close_iteration(s, maxiter)
      if s[DONE] != 0.0:
        return s, partials
    if phase == 5:
      s[PAP] = psum
      set_alpha(s, psum)
      if s[DONE] == 0.0:
        s[OPEN] = 1.0
  elif phase == 7:
    g = s[GAMMA_NEW]
    for q in range(NAMED, NSLOTS):
      g = g + s[q]
    s[STRIPES] = 0.0
    s[GAMMA_NEW] = g
  elif phase == 8:
    s[GAMMA_NEW] = psum
  return s, partials


def pmg_scalar_phase(s, phase, partials, n, maxiter, tol, atol):
  """The block after `sfem_pmg_cg_scalars` (CG that stops on r.r, slot [13]):
  first = sum partials[0, n), second = sum partials[n, 2n).
  3 [5] = first (b.b), whatever `DONE` says.
  2 starts: [13] = first (r.r), [0] = second (r.z), the rest as phase 2 of
    `scalar_phase` but 'converged' on r.r <= atol2.
  0 [1] = first, then phase 0 of `scalar_phase`.
  4 [13] = first, [2] = second.
  1 closes: beta = [2] / gamma, gamma <- [2], [1] cleared, the counter; stops
    on a bad r.z, r.r <= atol2, maxiter.  Stripes and [11] are not read."""
  s = np.array(s, np.float64)
  if not 0 <= phase <= 4:
    raise ValueError(f'phase {phase}')
  partials = np.asarray(partials, np.float64)
  first = total(partials[:n])
  second = total(partials[n:2 * n]) if phase in (2, 4) else 0.0
  if phase == 3:
    s[BB] = first
    return s
  if phase == 2:
    s[ATOL2] = max(tol * tol * s[BB], atol * atol)
    s[GAMMA] = second
    s[RR] = first
    s[[PAP, GAMMA_NEW, ITERS, OPEN, CORR, MEAN]] = 0.0
    s[STRIPES] = 0.0
    s[STATUS] = STATUS_CODE['running']
    s[DONE] = 0.0
    if bad_gamma(s[GAMMA]):
      _stop(s, 'breakdown_gamma')
    elif not s[RR] > s[ATOL2]:
      _stop(s, 'converged')
    elif maxiter <= 0:
      _stop(s, 'maxiter')
    return s
  if s[DONE] != 0.0:
    return s
  with np.errstate(all='ignore'):
    if phase == 0:
      s[PAP] = first
      set_alpha(s, first)
    elif phase == 4:
      s[RR] = first
      s[GAMMA_NEW] = second
    else:
      g = s[GAMMA_NEW]
      s[BETA] = g / s[GAMMA]
      s[GAMMA] = g
      s[PAP] = 0.0
      s[ITERS] += 1.0
      if bad_gamma(g):
        _stop(s, 'breakdown_gamma')
      elif not s[RR] > s[ATOL2]:
        _stop(s, 'converged')
      elif s[ITERS] >= maxiter:
        _stop(s, 'maxiter')
  return s


# ------------------------------------------------------------ the vector pieces
def _cast(v, dtype):
  return float(np.dtype(dtype).type(v))


def alpha_of(s, dtype=np.float64):
  """alpha as the update kernels form it: gamma / p.Ap, cast to the vectors'
  type (slot [3] is for the host)."""
  with np.errstate(all='ignore'):
    return _cast(s[GAMMA] / s[PAP], dtype)


def beta_of(s, dtype=np.float64, corr=0.0):
  with np.errstate(all='ignore'):
    return _cast((gamma_new_of(s) + corr) / s[GAMMA], dtype)


def update_xr(x, r, p, ap, s, dtype=np.float64):
  """(x, r, r.r): x += alpha p, r -= alpha Ap; with fuse_rr the kernel adds
  r.r to [2]."""
  if s[DONE] != 0.0:
    return x, r, 0.0
  a = alpha_of(s, dtype)
  r = r - a * ap
  return x + a * p, r, np.vdot(r, r)


def update_p(p, z, s, dtype=np.float64):
  """p = z + beta p."""
  if s[DONE] != 0.0:
    return p
  return z + beta_of(s, dtype) * p


def update_r(r, ap, s, dtype=np.float64):
  """(r, r.r): r -= alpha Ap; fuse_rr 1 adds r.r to [2], 2 to the stripes."""
  if s[DONE] != 0.0:
    return r, 0.0
  r = r - alpha_of(s, dtype) * ap
  return r, np.vdot(r, r)


def update_xp(x, p, z, s, dtype=np.float64):
  """(x, p): x += alpha p, p = z + beta p."""
  if s[DONE] != 0.0:
    return x, p
  return x + alpha_of(s, dtype) * p, z + beta_of(s, dtype) * p


def update_xp_lazy(x, ring, z, s, lazy, dtype=np.float64):
  """(x, ring, lazy) after `sfem_cg_update_xp_lazy`.  ring (m, n): p_k lives in
  row k mod m, k = [8]; p_{k+1} = z + beta p_k goes to the next row and alpha_k
  to lazy[1 + k mod m].  When (k + 1) mod m = 0 the pending terms
  max(lazy[0], k + 1 - m) .. k are added to x, oldest first."""
  if s[DONE] != 0.0:
    return x, ring, lazy
  ring, lazy = np.array(ring), np.array(lazy, np.float64)
  m = len(ring)
  k = int(s[ITERS])
  slot, nxt = k % m, (k + 1) % m
  a, beta = alpha_of(s, dtype), beta_of(s, dtype)
  if nxt == 0:
    for j in range(max(int(lazy[0]), k + 1 - m), k):
      x = x + _cast(lazy[1 + j % m], dtype) * ring[j % m]
    x = x + a * ring[slot]
  lazy[1 + slot] = a
  ring[nxt] = z + beta * ring[slot]
  return x, ring, lazy


def flush_x(x, ring, s, lazy, dtype=np.float64):
  """(x, lazy) after `sfem_cg_flush_x`: the terms of the iterations
  [max(lazy[0], iters - iters mod m), iters) are added, lazy[0] = iters.  Not
  guarded by `DONE`: it runs after the solve has stopped."""
  lazy = np.array(lazy, np.float64)
  m = len(ring)
  iters = int(s[ITERS])
  for j in range(max(int(lazy[0]), iters - iters % m), iters):
    x = x + _cast(lazy[1 + j % m], dtype) * ring[j % m]
  lazy[0] = s[ITERS]
  return x, lazy


def mean_set(s):
  """Where in `sums` the iteration's parity keeps (1.r, w.r)."""
  lo = (int(s[ITERS]) & 1) * 2 * RR_SLOTS
  return slice(lo, lo + RR_SLOTS), slice(lo + RR_SLOTS, lo + 2 * RR_SLOTS)


def update_r_mean(r, ap, w, s, sums, dtype=np.float64, stripe=0):
  """(r, s, sums): r -= alpha Ap; r.r goes to the stripes, 1.r and w.r to the
  set of `sums` of the iteration's parity."""
  s, sums = np.array(s, np.float64), np.array(sums, np.float64)
  if s[DONE] != 0.0:
    return r, s, sums
  r = r - alpha_of(s, dtype) * ap
  one, wr = mean_set(s)
  s[NAMED + stripe] += np.vdot(r, r)
  sums[one.start + stripe] += r.sum()
  sums[wr.start + stripe] += np.vdot(w, r)
  return r, s, sums


def update_xp_mean(x, p, r, s, sums, total_w, dtype=np.float64):
  """(x, p, s, sums) for M r = r - (w.r / total) 1: c = w.r / total,
  gamma_new = r.r - c 1.r, x += alpha p, p = (r - c) + beta p; [11] = -c 1.r
  (picked up by the close), [12] = c, the other parity's sums cleared."""
  s, sums = np.array(s, np.float64), np.array(sums, np.float64)
  if s[DONE] != 0.0:
    return x, p, s, sums
  one, wr = mean_set(s)
  c = sums[wr].sum() / total_w
  corr = -c * sums[one].sum()
  a, beta = alpha_of(s, dtype), beta_of(s, dtype, corr)
  x = x + a * p
  p = (r - _cast(c, dtype)) + beta * p
  s[CORR], s[MEAN] = corr, c
  other = ((int(s[ITERS]) & 1) ^ 1) * 2 * RR_SLOTS
  sums[other:other + 2 * RR_SLOTS] = 0.0
  return x, p, s, sums


def _per_component(dinv, n):
  return np.tile(dinv, n // len(dinv))


def update_r_jacobi(r, ap, dinv, s, dtype=np.float64):
  """(r, r.(dinv r)): component-major r, Ap of ncomp = len(r) / len(dinv)
  components sharing dinv; the sum goes to the stripes."""
  if s[DONE] != 0.0:
    return r, 0.0
  r = r - alpha_of(s, dtype) * ap
  return r, np.vdot(r * _per_component(dinv, len(r)), r)


def update_xp_jacobi(x, p, r, dinv, s, dtype=np.float64):
  """(x, p): x += alpha p, p = dinv r + beta p."""
  if s[DONE] != 0.0:
    return x, p
  d = _per_component(dinv, len(r))
  return x + alpha_of(s, dtype) * p, d * r + beta_of(s, dtype) * p


def axpby(a, x, b, y, dtype=np.float64):
  """a x + b y with a, b cast; y is not read when b = 0."""
  a, b = _cast(a, dtype), _cast(b, dtype)
  return a * x if b == 0.0 else a * x + b * y


def subtract_weighted_mean(w, b, total_w):
  """(out, w.out): out = w - (b.w / total) 1."""
  out = w - np.vdot(b, w) * (1.0 / total_w)
  return out, np.vdot(w, out)


def cheb_step(x, d, ax, b, dinv, a, c, mode, dtype=np.float64):
  """(x, d, r) after `sfem_cheb_step`: 0 d = a d + c dinv (b - ax), x += d;
  1 d = c dinv b, x = d; 2 r = b - ax; 3 d = c dinv (b - ax), x += d.  What
  a mode does not write comes back as it went in (r: None)."""
  a, c = _cast(a, dtype), _cast(c, dtype)
  if mode == 2:
    return x, d, b - ax
  if mode == 1:
    d = c * dinv * b
    return d.copy(), d, None
  d = (a * d if mode == 0 else 0.0) + c * dinv * (b - ax)
  return x + d, d, None


# ------------------------------------------------------- the loop, in pieces
SCHEDULES = ('nine', 'eight', 'deferred')


def cg_by_pieces(A, b, x0=None, tol=1e-5, atol=0.0, maxiter=None, M=None,
                 schedule='nine', lazy_m=0, mean=None, dtype=np.float64):
  """`oracle.sfem_oracle.cg` as the device solver runs it.  Schedules:
    'nine'     dot(p, Ap), phase 0, update_xr, z = M r, dot(r, z), update_p,
               phase 1;
    'eight'    dot, phase 0, update_r (r.r to a stripe; M = None), update_xp,
               phase 1;
    'deferred' p.Ap left in `partials` by the apply, phase 5, update_r,
               update_xp; phase 6 before the host looks.
  lazy_m >= 2: update_xp_lazy with a ring of that many directions in place of
  update_xp, flush_x before x is read.  mean = (w, total): the mean pair in
  place of update_r / update_xp (M r = r - (w.r / total) 1).
  Returns (x, iterates, status, iteration count)."""
  b = np.asarray(b, np.float64)
  n = b.size
  fused = schedule != 'nine'
  if fused and M is not None:
    raise ValueError('the fused r.r is r.z only for M = identity')
  if (lazy_m or mean) and not fused:
    raise ValueError('lazy and mean updates replace update_xp')
  x = np.zeros_like(b) if x0 is None else np.array(x0, np.float64)
  r = b - A(x)
  maxiter = 10 * n if maxiter is None else maxiter
  s = np.zeros(NSLOTS)
  sums = np.zeros(MEAN_SUMS)
  partials = np.zeros(DOT_SLOTS)
  lazy = np.zeros(1 + LAZY_MAX)
  if mean is not None:
    w, total_w = mean
    z = r - np.vdot(w, r) / total_w
  else:
    z = r if M is None else M(r)
  p = np.array(z)
  ring = None
  if lazy_m:
    ring = np.zeros((lazy_m, n))
    ring[0] = p
  s[BB], s[GAMMA] = np.vdot(b, b), np.vdot(r, z)
  args = (maxiter, tol, atol)
  s, partials = scalar_phase(s, 2, *args, partials)

  def solution(x, s, lazy):
    """x as the host reads it: the open iteration closed, the ring flushed
    (on copies: looking changes nothing the loop goes on with)."""
    if schedule == 'deferred':
      s, _ = scalar_phase(s, 6, *args)
    if lazy_m:
      x, _ = flush_x(x, ring, s, lazy, dtype)
    return x

  iterates = []
  while s[DONE] == 0.0:
    # the host's own count picks the direction: with the deferred close [8]
    # is one behind until phase 5 has run
    pk = ring[len(iterates) % lazy_m] if lazy_m else p
    ap = A(pk)
    if schedule == 'deferred':
      partials[n % DOT_SLOTS] += np.vdot(pk, ap)
      s, partials = scalar_phase(s, 5, *args, partials)
    else:
      s[PAP] += np.vdot(pk, ap)
      s, _ = scalar_phase(s, 0, *args)
    if s[DONE] != 0.0:      # (deferred: the flag comes one apply late)
      break
    if not fused:
      x, r, _ = update_xr(x, r, pk, ap, s, dtype)
      z = r if M is None else M(r)
      s[GAMMA_NEW] += np.vdot(r, z)
      p = update_p(p, z, s, dtype)
    elif mean is not None:
      r, s, sums = update_r_mean(r, ap, w, s, sums, dtype, stripe=n % RR_SLOTS)
      x, p, s, sums = update_xp_mean(x, p, r, s, sums, total_w, dtype)
    else:
      r, rr = update_r(r, ap, s, dtype)
      s[NAMED + n % RR_SLOTS] += rr
      if lazy_m:
        x, ring, lazy = update_xp_lazy(x, ring, r, s, lazy, dtype)
      else:
        x, p = update_xp(x, p, r, s, dtype)
    if schedule != 'deferred':
      s, _ = scalar_phase(s, 1, *args)
    iterates.append(solution(x, s, lazy))
  s_end = scalar_phase(s, 6, *args)[0] if schedule == 'deferred' else s
  x = solution(x, s_end, lazy)
  status = {v: k for k, v in STATUS_CODE.items()}[s_end[STATUS]]
  return x, iterates, status, int(s_end[ITERS])
