"""Preconditioned conjugate gradients on MI355X device tensors.

Signature and semantics of the reference `swirl_fem/linalg/cg.py:30-97`:
residual measured as r^T M r (:68-73), `maxiter = 10 * size` (:57-59),
tolerance `max(tol^2 b.b, atol^2)` (:65-66), pytrees of arrays, user `dot_fn`,
returns `(x, {'residual', 'num_iterations'})`.

The reference keeps the loop on the device with `lax.while_loop` (:94-95).
Here the five scalars of the recurrence live in a small device array and every
vector update is a fused HIP kernel that reads them there (`sfem_dot*`,
`sfem_cg_update_r`, `sfem_cg_update_xp`, `sfem_cg_scalars`), so an iteration
issues no host synchronisation.  The stopping test is evaluated on the device
each iteration; once it fires every later kernel is a no-op, and the host only
polls the flag every `check_every` iterations.  Iterates and iteration count
are therefore identical to a loop that tests every iteration.

A preconditioner with `stops_on_residual = True` (`linalg/pmg.py`, a V-cycle:
M ~ A^-1, so r . M r is an energy norm) switches the stopping test to the true
residual, r . r <= max(tol^2 b.b, atol^2), and sums every inner product of the
solve in a fixed order (`sfem_pmg_dot2`, `sfem_pmg_cg_scalars`); with a
layered operator the iteration is then bitwise reproducible.

On partitions (`interface`) a preconditioner is accepted when it maps
consistent vectors to consistent vectors (`consistent = True`: Jacobi with the
exchanged diagonal, p-multigrid on a block partition).  Every inner product is
then the plain local sum minus the interface correction, all-reduced: r . z
as r . r is; the fused Jacobi update corrects r . (dinv r) on the interface
nodes only; the r.r-stopping path corrects and all-reduces its stored partial
sums before they are added up, so every rank adds the same numbers.

A preconditioner that offers `mean_projection()` (M r = r - (w.r / total) 1,
the nullspace projection of the pressure solve) is folded into the two vector
updates: z = M r is never stored and r . z comes out of the sums update_r takes
anyway -- 9 vector passes per iteration instead of 12.  A preconditioner that
offers `jacobi_diagonal()` (M r = dinv r, `linalg/jacobi.py`) is folded in the
same way: the r update sums r . (dinv r) in place of r . r and the p update
forms p = dinv r + beta p -- 10 vector passes instead of 8 + 4.

Per iteration (M = identity): A(p) with p.Ap fused into the operator's scatter
stage when it offers `apply_with_dot`; r -= a Ap fused with r.r; then
x += a p and p = r + b p in one kernel  ->  8 N-vector passes besides the
apply (SURVEY 8d's fused model: 11; the reference's un-fused loop: 13).

The modes of `CGRunner`.  Each is an attribute that holds the mode's state,
or None / False / 0 when the mode is off; `__init__` selects them in the
order of the table (a mode's test names only modes above it), `_step_eager`
runs the four stages -- apply A and alpha, update r and gamma_new, update x
and p, close the iteration -- and each stage asks the attributes.  `_ops`
calls are named without their prefix.

| mode | selected when | r update, gamma_new | x / p update | excludes |
|---|---|---|---|---|
| `fused_dot` | `dot_fn` is None, A has `apply_with_dot`, one tensor | (p.Ap from the apply's partial sums: `cg_scalars` phase 3, or 5 when `merged`) | | -- (`rr_stop` switches it off) |
| `merged` | `fused_dot` and no `reduce_fn` | (one scalar launch per iteration: phase 5 gives alpha and closes the iteration before; `_flush` closes the last) | | |
| `fuse_rr` (= 2) | M is None, `dot_fn` is None | `cg_update_r` sums r.r over 64 slots; otherwise z = M(r) and `dot` (or `M.apply_with_dot`, or `dot_fn`) | `cg_update_xp` | |
| `fold_rr` | `fuse_rr` with `reduce_fn` or `interface` | + `cg_scalars` phase 7, `dot_indexed`, `reduce_fn` | | |
| `rr_stop` | M has `stops_on_residual`, `dot_fn` is None, one 1-D tensor | `_step_residual_stop`: `cg_update_r` (`_layered`), z = M(r), `pmg_dot2`, `pmg_cg_scalars` | `cg_update_xp` | `fused_dot`, and every mode below |
| `mean` | M has `mean_projection()`, no `dot_fn` / `reduce_fn` / `interface`, one tensor, `SFEM_FUSED_MEAN` | `cg_update_r_mean` | `cg_update_xp_mean` | `jacobi`, `layered`, `lazy` |
| `jacobi` | M has `jacobi_diagonal()` of r's length, `dot_fn` is None, `interface` or no `reduce_fn`, a scalar or component-major field, `SFEM_FUSED_JACOBI` | `cg_update_r_jacobi` (with the layers and, with `det`, `cg_scalars_n` phase 8); with `reduce_fn`: phase 7, `dot_indexed` with `jacobi_interface`, `reduce_fn` | `cg_update_xp_jacobi` | `lazy` |
| `layered` | `fused_dot`, a 1-D field, A has `apply_layered_with_dot` and a layer plan | `cg_update_r_layered` | | |
| `det` | `layered`, no `reduce_fn` / `interface`, `SFEM_DETERMINISTIC` | `cg_scalars_n` phase 5 after the apply; `cg_update_r_layered_det`, `cg_scalars_n` phase 8 | | |
| `lazy` | `SFEM_LAZY_X` >= 2, p one contiguous tensor of `SFEM_LAZY_X_MIN_MB` or more | | `cg_update_xp_lazy`; `cg_flush_x` when x is read | dropped by `capture` |

Known limitation: `det` is also selected when a preconditioner M is given
(`fuse_rr` = 0).  The r update is then `cg_update_r_layered` and r . M r a
plain `dot`, which accumulates with atomics: such an iteration is NOT bitwise
reproducible, only its p.Ap is summed in a fixed order.  (The fused Jacobi
update does take the fixed-order sums.)
"""

from __future__ import annotations

from typing import NamedTuple

import torch

from swirl_fem_amd import switches
from swirl_fem_amd import _lib
from swirl_fem_amd import _ops
from swirl_fem_amd.core import layout
from swirl_fem_amd.linalg import _driver


def _leaves(t):
  if isinstance(t, dict):
    return [l for k in sorted(t) for l in _leaves(t[k])]
  if isinstance(t, (list, tuple)):
    return [l for x in t for l in _leaves(x)]
  return [t]


def _map(f, *ts):
  t0 = ts[0]
  if isinstance(t0, dict):
    return {k: _map(f, *[t[k] for t in ts]) for k in t0}
  if isinstance(t0, (list, tuple)):
    return type(t0)(_map(f, *xs) for xs in zip(*ts))
  return f(*ts)


def _as_vec(t):
  if not isinstance(t, torch.Tensor):
    raise TypeError(f'cg operates on device tensors, got {type(t)}')
  return t


MAX_KEPT_RUNNERS = 6   # solver states a `workspace` of `cg` holds at most
# vectors below this size are served by the caches: the lazy x update would
# only cost memory there (same threshold as the non-temporal vector kernels;
# SFEM_LAZY_X_MIN_MB overrides it, the tests set 0)
LAZY_X_MIN_BYTES = 1 << 28
RR_PARTIALS = 1 << 16      # stored r.r sums: one per workgroup of the r update
RESIDUAL_STOP_GROUPS = 512  # stored partial sums per inner product (r.r stop)
# `fuse_rr` of the r updates: r.r spread over 64 slots, update_r then streams
# with 128 workgroups per CU.  When something needs the complete sum in the
# named slot right after the update (an all-reduce, the interface correction)
# one tiny scalar launch folds the slots first (`fold_rr`).
FUSE_RR_SPREAD = 2


def _lazy_min_bytes():
  mb = switches.get('SFEM_LAZY_X_MIN_MB')
  return LAZY_X_MIN_BYTES if mb is None else int(float(mb) * (1 << 20))


# The states of the modes (`CGRunner.rr_stop`, `.mean`, `.jacobi`, `.det`,
# `.lazy`).  rr_stop: stored partial sums of the inner products; `layered`:
# the operator's layer plan (its apply then stores per-wave p.Ap sums in
# `waves`) or None.  det: one double per wave of the apply, one per workgroup
# of the r update.  lazy: the (m, n padded) ring of directions.
_ResidualStop = NamedTuple('_ResidualStop', [
    ('groups', int), ('layered', object), ('parts', torch.Tensor),
    ('waves', torch.Tensor), ('num_waves', int)])
_Mean = NamedTuple('_Mean', [('w', torch.Tensor), ('total', float),
                             ('sums', torch.Tensor)])
_Jacobi = NamedTuple('_Jacobi', [('dinv', torch.Tensor), ('ncomp', int)])
_Det = NamedTuple('_Det', [('wave_sums', torch.Tensor),
                           ('rr_sums', torch.Tensor)])
_Lazy = NamedTuple('_Lazy', [('ring', torch.Tensor), ('n', int),
                             ('state', torch.Tensor)])


class _Scalars:
  """Device-resident CG scalars (see include/sfem.h, SFEM_CG_NSCALARS)."""
  GAMMA, PAP, GAMMA_NEW, ALPHA, BETA, BB, ATOL2, DONE, ITERS = range(9)
  STATUS = 10

  def __init__(self, device):
    self.t = torch.zeros(_lib.SFEM_CG_NSCALARS, dtype=torch.float64,
                         device=device)
    # strip of partial sums for operators that fuse p.Ap into their scatter
    self.partials = torch.zeros(_lib.SFEM_DOT_SLOTS, dtype=torch.float64,
                                device=device)

  def interface_correction(self, slot, a, b, interface):
    """scalars[slot] -= sum_interface w a b: turns the plain local dot of two
    *consistent* vectors into this rank's share of the global inner product
    (`NeighborPlan.interface_weights`); the interface is O(N^(2/3)) nodes."""
    idx, w = interface
    if idx.numel() == 0:
      return
    for x, y in zip(_leaves(a), _leaves(b)):
      _ops.dot_indexed(x, layout.like(y, x), idx, w, self.t, slot, -1.0)

  def complete(self, slot, a, b, reduce_fn, interface):
    """What turns the local sum of a . b in `slot` into the inner product:
    the interface correction, then the reduction over the partitions."""
    if interface is not None:
      self.interface_correction(slot, a, b, interface)
    if reduce_fn is not None:
      reduce_fn(self.t[slot:slot + 1])

  def dot_into(self, slot, a, b, dot_fn, reduce_fn, interface=None,
               cleared=False):
    """scalars[slot] = <a, b> summed over the leaves of the pytrees.
    `cleared`: the slot is zero already (a scalar phase cleared it), so the
    device dot of the first leaf accumulates as well."""
    la, lb = _leaves(a), _leaves(b)
    if dot_fn is None:
      first = not cleared
      for x, y in zip(la, lb):
        _ops.dot(layout.flat(x), layout.flat(layout.like(y, x)), self.t, slot,
                 accumulate=not first)
        first = False
    else:
      total = sum(dot_fn(x, y) for x, y in zip(la, lb))
      self.t[slot] = torch.as_tensor(total, dtype=torch.float64,
                                     device=self.t.device)
    self.complete(slot, a, b, reduce_fn, interface)


class CGRunner:
  """State of one CG solve; `step()` enqueues exactly one iteration.

  `cg()` drives it until the device flag reports convergence; `bench.py`
  steps it a fixed number of times.  The module docstring lists the modes.
  """

  def __init__(self, A, b, x0=None, *, tol=1e-5, atol=0.0, maxiter=None,
               M=None, dot_fn=None, reduce_fn=None, interface=None):
    if interface is not None and (
        dot_fn is not None or
        (M is not None and not getattr(M, 'consistent', False))):
      raise ValueError('interface weights apply to the plain dot of consistent '
                       'vectors (M = None or a preconditioner that maps '
                       'consistent vectors to consistent ones, dot_fn = None)')
    b_leaves = [_as_vec(l) for l in _leaves(b)]
    if not all(l.is_cuda for l in b_leaves):
      raise RuntimeError('swirl_fem_amd.linalg.cg runs on MI355X device '
                         'tensors (there is no CPU fallback)')
    self.A, self.M, self.dot_fn, self.reduce_fn = A, M, dot_fn, reduce_fn
    self.interface = interface
    self.tol, self.atol = tol, atol
    if maxiter is None:
      maxiter = 10 * sum(l.numel() for l in b_leaves)
    self.maxiter = maxiter
    dense = lambda t: t if (t.is_contiguous() or
                            layout.is_component_major(t)) else t.contiguous()
    b = _map(dense, b)
    self._x = (_map(torch.zeros_like, b) if x0 is None
               else _map(lambda t, bb: layout.like(t, bb).clone(), x0, b))
    self.s = _Scalars(b_leaves[0].device)
    self.identity_m = M is None
    self.issued = 0
    self._graph = None
    self._capture_failed = False
    z = self._start_vectors(b, allocate=True)
    # operators exposing `apply_with_dot` hand back p.Ap with the apply
    self.fused_dot = (dot_fn is None and hasattr(A, 'apply_with_dot') and
                      isinstance(self._p, torch.Tensor))
    self.fuse_rr = FUSE_RR_SPREAD if self.identity_m and dot_fn is None else 0
    self.fold_rr = bool(self.fuse_rr) and (reduce_fn is not None or
                                           interface is not None)
    self.parts = self.s.partials if self.fused_dot else None
    self._start_scalars(z)
    self.rr_stop = self._select_residual_stop()
    if self.rr_stop is not None:
      self.fused_dot, self.parts = False, None
    self._args = (self.maxiter, self.tol, self.atol, self.parts)
    # Without an all-reduce between the sum of the partials and alpha the
    # iteration needs ONE scalar launch: phase 5 also closes the previous
    # iteration (beta, gamma, counter, convergence flag) -- see `_flush`.
    self.merged = self.fused_dot and reduce_fn is None
    self.mean = self._select_mean()
    self.jacobi = self._select_jacobi()
    # r . (dinv r) of consistent vectors: its interface correction is the
    # r . r one with the weights w dinv (dinv is the same on every holder)
    self.jacobi_interface = None
    if self.jacobi is not None and interface is not None:
      idx, w = interface
      self.jacobi_interface = (
          idx, (w * self.jacobi.dinv[idx].double()).contiguous())
    self.layered = self._select_layered()
    self.det = self._select_det()
    self.lazy = self._select_lazy()
    self._start_fixed_order_sums(b, z)

  # --------------------------------------------------------- mode selection
  def _select_residual_stop(self):
    """Stop on r.r with fixed-order sums: the preconditioner asks for it.
    State: stored partial sums of the inner products, and the layered apply
    (per-wave p.Ap sums) when A has one."""
    A = self.A
    if not (getattr(self.M, 'stops_on_residual', False) and
            self.dot_fn is None and isinstance(self.r, torch.Tensor) and
            self.r.dim() == 1):
      return None
    dev = self.r.device
    G = RESIDUAL_STOP_GROUPS
    layered = None
    if (hasattr(A, 'apply_layered_with_dot') and hasattr(A, 'layer_plan') and
        self.reduce_fn is None and self.interface is None):
      layered = A.layer_plan()
    waves = A.layered_dot_slots() if layered is not None else 0
    return _ResidualStop(
        groups=G, layered=layered,
        parts=torch.zeros(2 * G, dtype=torch.float64, device=dev),
        waves=torch.zeros(waves + _lib.SFEM_FOLD_GROUPS, dtype=torch.float64,
                          device=dev), num_waves=waves)

  def _select_mean(self):
    """M r = r - (w . r / total) 1 folded into the two vector updates."""
    probe = getattr(self.M, 'mean_projection', None)
    if not (probe is not None and self.rr_stop is None and
            self.dot_fn is None and self.reduce_fn is None and
            self.interface is None and isinstance(self.r, torch.Tensor) and
            switches.get('SFEM_FUSED_MEAN') != '0'):
      return None
    found = probe()
    if found is None:
      return None
    w, total = found
    return _Mean(layout.flat(layout.like(w.to(self.r.dtype), self.r)),
                 float(total),
                 torch.zeros(_lib.SFEM_CG_MEAN_SUMS, dtype=torch.float64,
                             device=self.r.device))

  def _select_jacobi(self):
    """M r = dinv (.) r folded into the two vector updates: (dinv, components)
    of a scalar or component-major field (one dinv for all components)."""
    probe = getattr(self.M, 'jacobi_diagonal', None)
    r = self.r
    if not (probe is not None and self.mean is None and
            self.rr_stop is None and self.dot_fn is None and
            (self.interface is not None or self.reduce_fn is None) and
            isinstance(r, torch.Tensor) and
            switches.get('SFEM_FUSED_JACOBI') != '0'):
      return None
    dinv = probe()
    dinv = None if dinv is None else dinv.to(r.dtype).contiguous()
    n = -1 if dinv is None else dinv.numel()
    vn = 16 // r.element_size()
    if r.dim() == 1 or (r.dim() == 2 and r.shape[1] == 1 and
                        r.is_contiguous()):
      ncomp = 1
    elif (r.dim() == 2 and layout.is_component_major(r) and
          self._p.stride() == r.stride() and n % vn == 0):
      ncomp = r.shape[1]
    else:
      return None          # (row-major fields: M is called as a function)
    return _Jacobi(dinv, ncomp) if r.shape[0] == n else None

  def _select_layered(self):
    """Layered assembly: the operator leaves the contributions of shared nodes
    in layers of an extended Ap (plain stores: no atomics, no cleared range)
    and `r -= alpha Ap` adds them up where it streams Ap anyway, in a fixed
    order -- same sums, bitwise reproducible.  One partition, scalar field.
    On partitions (`reduce_fn`, `interface`) the operator hands back the
    layered result with its interface nodes already whole and exchanged."""
    if (self.fused_dot and self.mean is None and self.rr_stop is None and
        self._p.dim() == 1 and hasattr(self.A, 'apply_layered_with_dot')):
      return self.A.layer_plan()
    return None

  def _select_det(self):
    """... and with the two inner products of the iteration summed from STORED
    partial sums in a fixed order (one double per wave of the apply, one per
    workgroup of the r update) the whole iteration is bitwise reproducible
    from run to run; costs one more scalar launch per iteration."""
    if not (self.layered is not None and self.reduce_fn is None and
            self.interface is None and
            switches.get('SFEM_DETERMINISTIC') != '0'):
      return None
    # (+ SFEM_FOLD_GROUPS: scratch of the two-stage sums behind the slots)
    pad = _lib.SFEM_FOLD_GROUPS
    dev = self.r.device
    return _Det(torch.zeros(self.A.layered_dot_slots() + pad,
                            dtype=torch.float64, device=dev),
                torch.zeros(RR_PARTIALS + pad, dtype=torch.float64,
                            device=dev))

  def _select_lazy(self):
    """Lazy solution update (`sfem_cg_update_xp_lazy`): x is touched every
    m-th iteration only, the directions in between wait in a ring -- bitwise
    the same x, 4.25 instead of 5 vector passes in the x / p update at m = 4.
    Worth m - 1 more vectors only where the iteration streams from HBM.
    (With the fused Jacobi updates x is updated every iteration.)  The ring
    takes the place of `_p`."""
    m = int(switches.get('SFEM_LAZY_X'))
    p = self._p
    if not (m >= 2 and self.mean is None and self.jacobi is None and
            self.rr_stop is None and isinstance(p, torch.Tensor) and
            p.is_contiguous() and
            p.numel() * p.element_size() >= _lazy_min_bytes()):
      return None
    m = min(m, _lib.SFEM_CG_LAZY_MAX)
    n = p.numel()
    ring = torch.empty((m, (n + 3) // 4 * 4), dtype=p.dtype, device=p.device)
    ring[0, :n] = p.reshape(-1)
    self._p = None
    self._shape = tuple(self.r.shape)
    return _Lazy(ring, n, torch.zeros(1 + _lib.SFEM_CG_LAZY_MAX,
                                      dtype=torch.float64, device=p.device))

  # ------------------------------------------------------------------ start
  def _start_vectors(self, b, allocate=False):
    """b.b, r = b - A x, z = M r and p = z for the x in place; returns z.
    `__init__` allocates r and p here, `restart` rewrites them in place."""
    s, S = self.s, _Scalars
    s.dot_into(S.BB, b, b, self.dot_fn, self.reduce_fn, self.interface)
    Ax = self.A(self._x)
    if allocate:
      self.r = _map(lambda bb, ax: bb - layout.like(ax, bb), b, Ax)
    else:
      _map(lambda rr, bb, ax: rr.copy_(layout.like(bb, rr) -
                                       layout.like(ax, rr)), self.r, b, Ax)
    z = self.r if self.identity_m else self.M(self.r)
    if allocate:
      self._p = _map(lambda t, rr: layout.like(t, rr).clone(), z, self.r)
    else:
      _map(lambda pp, zz: pp.copy_(layout.like(zz, pp)), self.p, z)
    return z

  def _start_scalars(self, z):
    """gamma_0 = r.z and the stopping rule (phase 2)."""
    s = self.s
    s.dot_into(_Scalars.GAMMA, self.r, z, self.dot_fn, self.reduce_fn,
               self.interface)
    _ops.cg_scalars(s.t, 2, self.maxiter, self.tol, self.atol, self.parts)

  def _start_fixed_order_sums(self, b, z):
    """The modes that sum in a fixed order take b.b and gamma_0 again."""
    if self.det is not None:
      self._reproducible_start(b, z)
    if self.rr_stop is not None:
      self._residual_stop_start(b, z)

  def _residual_stop_start(self, b, z):
    """b.b, r.r and gamma_0 = r.z as fixed-order sums; the stop rule on r.r."""
    st = self.rr_stop
    args = (self.maxiter, self.tol, self.atol)
    self._dot2(b, b, None)
    _ops.pmg_cg_scalars(self.s.t, 3, st.parts, st.groups, *args)
    self._dot2(self.r, self.r, layout.like(z, self.r).contiguous())
    _ops.pmg_cg_scalars(self.s.t, 2, st.parts, st.groups, *args)

  def _dot2(self, a, b, c):
    """Stored partial sums of a.b (and a.c) for `sfem_pmg_cg_scalars`; on
    partitions the interface correction goes into the first partial of each
    and the partials are all-reduced, so every rank adds the same numbers."""
    G, parts = self.rr_stop.groups, self.rr_stop.parts
    _ops.pmg_dot2(a, b, c, parts, G)
    if self.interface is not None:
      idx, w = self.interface
      if idx.numel():
        _ops.dot_indexed(a, b, idx, w, parts, 0, -1.0)
        if c is not None:
          _ops.dot_indexed(a, c, idx, w, parts, G, -1.0)
    if self.reduce_fn is not None:
      self.reduce_fn(parts[:G if c is None else 2 * G])

  def _reproducible_start(self, b, z):
    """b.b and gamma_0 = r.z again, as tree reductions without atomics (the
    device dot accumulates its workgroups' sums in arrival order), and the
    stopping rule re-initialised from them: the start of a reproducible solve."""
    s, S = self.s, _Scalars
    tree = lambda u, v: (u.double() * v.double()).sum()
    s.t[S.BB] = tree(b, b)
    s.t[S.GAMMA] = tree(self.r, z)
    _ops.cg_scalars(s.t, 2, self.maxiter, self.tol, self.atol, self.parts)

  @property
  def vector_passes(self):
    """N-vector reads + writes of one iteration outside the operator (M = I):
    r -= alpha Ap reads r, Ap and writes r; the x / p update reads x, p, r and
    writes x, p -- or, lazily, (4 m + 1) / m of them on average.  The fused
    Jacobi updates read dinv once more in each: 10."""
    if self.jacobi is not None:
      return 10
    if self.lazy is None:
      return 8
    m = self.lazy.ring.shape[0]
    return 3 + (4 * m + 1) / m

  @property
  def p(self):
    """The current search direction p_k (k = iterations issued)."""
    if self.lazy is None:
      return self._p
    ring, n, _ = self.lazy
    return ring[self.issued % ring.shape[0], :n].view(self._shape)

  @property
  def x(self):
    """The iterate after the iterations issued so far (with the lazy update:
    after adding the terms that were still held back)."""
    if self.lazy is not None:
      self._flush()
      _ops.cg_flush_x(layout.flat(self._x), self.lazy.ring, self.s.t,
                      self.lazy.state)
    return self._x

  def matches(self, b, tol, atol, maxiter) -> bool:
    """Whether `restart(b)` can take this right-hand side: same leaves
    (shape, dtype, device, memory layout) and the same stopping rule (a
    captured iteration carries tol / atol / maxiter as kernel arguments)."""
    mine, theirs = _leaves(self.r), _leaves(b)
    if len(mine) != len(theirs) or (tol, atol) != (self.tol, self.atol):
      return False
    if maxiter is None:
      maxiter = 10 * sum(l.numel() for l in theirs)
    if maxiter != self.maxiter:
      return False
    # (component-major and row-major (N, d) fields have the same shape: the
    # strides tell them apart; `restart` repacks a dense b of another layout)
    return all(isinstance(t, torch.Tensor) and t.shape == m.shape and
               t.dtype == m.dtype and t.device == m.device and
               (t.stride() == m.stride() or t.is_contiguous())
               for m, t in zip(mine, theirs))

  def restart(self, b, x0=None):
    """The same solve (A, M, stopping rule) for a new right-hand side: x, r,
    p and the scalars are rewritten IN PLACE, so an iteration captured into a
    HIP graph stays valid -- a time stepper that solves with the same
    operators every step then records each of them once (recording costs
    about 1 ms per solve, a third of a Kolmogorov-generator step)."""
    if x0 is None:
      _map(lambda xx: xx.zero_(), self._x)
    else:
      _map(lambda xx, t: xx.copy_(layout.like(t, xx)), self._x, x0)
    self.issued = 0
    if self.lazy is not None:
      self.lazy.state.zero_()
    z = self._start_vectors(b)
    self._start_scalars(z)
    self._start_fixed_order_sums(b, z)
    if self.mean is not None:
      self.mean.sums.zero_()

  # -------------------------------------------------------------- iteration
  def step(self):
    """One iteration of cg.py:75-86, all on the device."""
    if self._graph is not None:
      self._graph.replay()
      self.issued += 1
      return
    self._step_eager()

  def _step_eager(self):
    if self.rr_stop is not None:
      self._step_residual_stop()
      return
    Ap = self._apply_and_alpha()
    z = self._update_r(Ap)
    self._update_xp(z)
    self._close()

  def _apply_and_alpha(self):
    """Ap = A p, p.Ap and alpha = gamma / p.Ap (scalar phase 0, or 5)."""
    s, S, A = self.s, _Scalars, self.A
    if self.det is not None:
      sums = self.det.wave_sums
      Ap = A.apply_layered_with_dot(self.p, sums, per_wave=True)
      _ops.cg_scalars_n(s.t, 5, self.maxiter, self.tol, self.atol, sums,
                        sums.numel() - _lib.SFEM_FOLD_GROUPS)
      return Ap
    if self.fused_dot:
      Ap = (A.apply_layered_with_dot(self.p, s.partials)
            if self.layered is not None
            else A.apply_with_dot(self.p, s.partials))
      _ops.cg_scalars(s.t, 5 if self.merged else 3, *self._args)
      if self.reduce_fn is not None:
        # (p . unassembled Ap: nothing to correct on the interface)
        self.reduce_fn(s.t[S.PAP:S.PAP + 1])
    else:
      Ap = A(self.p)
      # slot PAP is zero here: cleared by phase 2 / phase 1
      s.dot_into(S.PAP, self.p, Ap, self.dot_fn, self.reduce_fn,
                 self.interface, cleared=True)
    if not self.merged:
      _ops.cg_scalars(s.t, 0, *self._args)
    return Ap

  def _update_r(self, Ap):
    """r -= alpha Ap and gamma_new = r . M r; returns z = M r, or None when
    M is folded into the vector updates (`mean`, `jacobi`)."""
    s, S, M = self.s, _Scalars, self.M
    if self.mean is not None:
      _ops.cg_update_r_mean(layout.flat(self.r),
                            layout.flat(layout.like(Ap, self.r)), self.mean.w,
                            s.t, self.mean.sums)
      return None
    if self.jacobi is not None:
      self._update_r_jacobi(Ap)
      return None
    plan = self.layered
    if plan is not None and self.det is not None and self.fuse_rr:
      n = _ops.cg_update_r_layered_det(
          self.r, Ap, plan.layers, s.t, self.det.rr_sums[:RR_PARTIALS],
          masks=plan.masks)
      _ops.cg_scalars_n(s.t, 8, self.maxiter, self.tol, self.atol,
                        self.det.rr_sums, n)
    elif plan is not None:
      _ops.cg_update_r_layered(self.r, Ap, plan.layers, s.t, self.fuse_rr,
                               masks=plan.masks)
    else:
      for rr, aa in zip(_leaves(self.r), _leaves(Ap)):
        _ops.cg_update_r(layout.flat(rr), layout.flat(layout.like(aa, rr)),
                         s.t, self.fuse_rr)
    if self.fuse_rr:
      if self.fold_rr:             # (an all-reduce or a correction follows)
        _ops.cg_scalars(s.t, 7, *self._args)
        s.complete(S.GAMMA_NEW, self.r, self.r, self.reduce_fn,
                   self.interface)
      return self.r
    if (self.dot_fn is None and hasattr(M, 'apply_with_dot') and
        isinstance(self.r, torch.Tensor)):
      # the preconditioner accumulates r . M r itself (slot is zero here)
      z = M.apply_with_dot(self.r, s.t, S.GAMMA_NEW)
      s.complete(S.GAMMA_NEW, self.r, z, self.reduce_fn, self.interface)
    else:
      # (slot zero here too; with a `dot_fn`: after convergence the done flag
      # guards every consumer of this slot)
      z = self.r if self.identity_m else M(self.r)
      s.dot_into(S.GAMMA_NEW, self.r, z, self.dot_fn, self.reduce_fn,
                 self.interface, cleared=True)
    return z

  def _update_r_jacobi(self, Ap):
    """r -= alpha Ap with r . (dinv r) (`sfem_cg_update_r_jacobi`)."""
    s, plan = self.s, self.layered
    dinv, ncomp = self.jacobi
    if plan is None:
      r, Ap = layout.flat(self.r), layout.flat(layout.like(Ap, self.r))
      layers, masks = (), None
    else:                          # (a 1-D field: ncomp = 1)
      r, layers, masks = self.r, plan.layers, plan.masks
    sums = (self.det.rr_sums[:RR_PARTIALS]
            if plan is not None and self.det is not None else None)
    n = _ops.cg_update_r_jacobi(r, Ap, dinv, s.t, ncomp, layers, masks, sums)
    if sums is not None:
      _ops.cg_scalars_n(s.t, 8, self.maxiter, self.tol, self.atol,
                        self.det.rr_sums, n)
    if self.reduce_fn is not None:
      # the striped r . (dinv r) into [2], corrected on the interface nodes,
      # summed over the partitions
      _ops.cg_scalars(s.t, 7, *self._args)
      s.complete(_Scalars.GAMMA_NEW, self.r, self.r, self.reduce_fn,
                 self.jacobi_interface)

  def _update_xp(self, z):
    """x += alpha p and p = z + beta p in one kernel: x += alpha p rides with
    the p update (p is in registers there), 8 vector passes per iteration
    instead of 9, same arithmetic."""
    s = self.s
    if self.mean is not None:
      _ops.cg_update_xp_mean(layout.flat(self._x), layout.flat(self.p),
                             layout.flat(self.r), s.t, self.mean.sums,
                             self.mean.total)
    elif self.jacobi is not None:
      dinv, ncomp = self.jacobi
      _ops.cg_update_xp_jacobi(layout.flat(self._x), layout.flat(self.p),
                               layout.flat(self.r), dinv, s.t, ncomp)
    elif self.lazy is not None:
      _ops.cg_update_xp_lazy(layout.flat(self._x), self.lazy.ring,
                             layout.flat(layout.like(z, self.r)), s.t,
                             self.lazy.state)
    else:
      for xx, pp, zz in zip(_leaves(self._x), _leaves(self.p), _leaves(z)):
        _ops.cg_update_xp(layout.flat(xx), layout.flat(pp),
                          layout.flat(layout.like(zz, pp)), s.t)

  def _close(self):
    """beta, gamma, the counter and the convergence flag (phase 1) -- unless
    the next iteration's phase 5 does it (`merged`)."""
    if not self.merged:
      _ops.cg_scalars(self.s.t, 1, *self._args)
    self.issued += 1

  def _step_residual_stop(self):
    """One PCG iteration that stops on r.r (see the module docstring)."""
    s, st = self.s, self.rr_stop
    G, parts = st.groups, st.parts
    args = (self.maxiter, self.tol, self.atol)
    if st.layered is not None:
      Ap = self.A.apply_layered_with_dot(self.p, st.waves, per_wave=True)
      _ops.pmg_cg_scalars(s.t, 0, st.waves, st.num_waves, *args)
      _ops.cg_update_r_layered(self.r, Ap, st.layered.layers, s.t, 0,
                               masks=st.layered.masks)
    else:
      Ap = layout.like(self.A(self.p), self.r).contiguous()
      self._dot2(self.p, Ap, None)
      _ops.pmg_cg_scalars(s.t, 0, parts, G, *args)
      _ops.cg_update_r(self.r, Ap, s.t, 0)
    z = layout.like(self.M(self.r), self.r).contiguous()
    self._dot2(self.r, self.r, z)
    _ops.pmg_cg_scalars(s.t, 4, parts, G, *args)
    _ops.cg_update_xp(self._x, self.p, z, s.t)
    _ops.pmg_cg_scalars(s.t, 1, parts, G, *args)
    self.issued += 1

  def capture(self) -> bool:
    """Records one iteration into a HIP graph; later `step()` calls replay it.

    A CG iteration on a small mesh is a few dozen short launches (kernels,
    memsets, scalar updates) and is bound by launch overhead, not by the GPU;
    one graph launch per iteration removes that.  Everything an iteration
    touches lives at fixed addresses (x, r, p, the scalars; temporaries come
    from the graph's private pool) and no kernel needs the host, so the replay
    is exact.  Returns False (and stays eager) if the operator or the
    preconditioner does something that cannot be captured.
    """
    if self._graph is not None:
      return True
    if self.reduce_fn is not None:
      return False                 # collectives stay on the eager path
    if self.lazy is not None:
      # a recorded iteration has fixed operands; the ring rotates them
      if self.issued:
        return False
      ring, n, _ = self.lazy
      self._p = ring[0, :n].view(self._shape).clone()
      self.lazy = None
    self.step()                    # warm caches / lazy setup eagerly
    torch.cuda.synchronize()
    issued = self.issued
    self._graph = _driver.capture_graph(self._step_eager)
    self.issued = issued           # capture records, it does not execute
    if self._graph is None:
      self._capture_failed = True  # (a kept runner does not try again)
    return self._graph is not None

  def _flush(self):
    """Closes the iteration that the single-scalar-launch scheme leaves open
    (no-op otherwise), so that the scalars describe the last `step()`."""
    if self.merged:
      _ops.cg_scalars(self.s.t, 6, self.maxiter, self.tol, self.atol, None)

  def done(self) -> bool:
    """Synchronising poll of the device convergence flag."""
    self._flush()
    return bool(self.s.t[_Scalars.DONE].item() != 0.0)

  def info(self):
    self._flush()
    scal = self.s.t.cpu()
    status = _lib.CG_STATUS.get(int(scal[_Scalars.STATUS].item()), 'unknown')
    if status == 'running' and self.issued >= self.maxiter:
      status = 'maxiter'
    # 'residual' and 'num_iterations' as the reference returns them
    # (cg.py:96-97); 'status' says why the loop ended: 'converged', 'maxiter',
    # or a breakdown the reference would have reported as convergence
    # ('breakdown_gamma': r.Mr negative / not finite, 'breakdown_pAp': p.Ap
    # zero / not finite) -- x is then the last iterate, NOT a solution to `tol`.
    return {'residual': self.s.t[_Scalars.GAMMA].clone(),
            'num_iterations': int(scal[_Scalars.ITERS].item()),
            'status': status}


def cg(A, b, x0=None, *, tol=1e-5, atol=0.0, maxiter=None, M=None,
       dot_fn=None, reduce_fn=None, interface=None, check_every=16,
       graph=False, workspace=None, key=None):
  """Solves A x = b with (preconditioned) conjugate gradients.

  Args:
    A: linear operator on pytrees of device tensors.
    b: right-hand side pytree.
    x0: initial guess (default zeros).
    tol, atol: stop when r^T M r <= max(tol^2 b.b, atol^2) (r^T r with a
      preconditioner that sets `stops_on_residual`, e.g. p-multigrid).
    maxiter: iteration cap (default 10 * size).
    M: preconditioner (default identity).
    dot_fn: optional custom inner product `(a, b) -> scalar tensor`; the default
      is the fused device dot.
    reduce_fn: optional in-place reduction applied to every inner product
      (partitioned meshes pass an RCCL all-reduce; reference callers pass a
      psum-ing `dot_fn`).
    interface: optional `(idx, w)` from `NeighborPlan.interface_weights`: all
      vectors are consistent across partitions (A returns the *assembled*
      result) and every plain dot is corrected on the interface nodes to count
      each global node once.  Mathematically the same iterates as the
      reference's partitioned convention (unassembled A, M = exchange,
      navier_stokes.py:436-438) without the extra vector z = M r.
    graph: replay the iteration as one HIP graph launch (`CGRunner.capture`);
      worth it when an iteration is launch-bound (small meshes, long solves).
      `A` and `M` must then be pure device work on fixed operands.
    check_every: the host polls the device convergence flag this often.
    workspace, key: with `graph=True`, a dict owned by the caller and a
      hashable key that stands for (A, M): the solver state and the recorded
      iteration are kept under `workspace[key]` and reused by later calls with
      the same key, stopping rule and vector shapes (`CGRunner.restart`).  The
      caller promises that A and M of those calls are the same operators.
  Returns:
    (x, info) with info = {'residual': gamma, 'num_iterations': k,
    'status': 'converged' | 'maxiter' | 'breakdown_gamma' | 'breakdown_pAp'}.
  """
  if not _leaves(b):
    return b, {'residual': 0.0, 'num_iterations': 0, 'status': 'converged'}
  reuse = (graph and workspace is not None and key is not None and
           dot_fn is None and reduce_fn is None and interface is None)
  run, kept = _driver.kept_runner(
      workspace if reuse else None, key, MAX_KEPT_RUNNERS,
      lambda run: run.matches(b, tol, atol, maxiter),
      lambda: CGRunner(A, b, x0, tol=tol, atol=atol, maxiter=maxiter, M=M,
                       dot_fn=dot_fn, reduce_fn=reduce_fn,
                       interface=interface))
  if kept:
    run.restart(b, x0)
  if (graph and dot_fn is None and run.maxiter > 2 and run._graph is None and
      not run._capture_failed and not run.done()):
    run.capture()
  _driver.drive(run, check_every)
  info = run.info()
  _driver.warn_on_breakdown('cg', info)
  # (a kept runner overwrites its x in the next solve)
  return (_map(lambda t: t.clone(), run.x) if reuse else run.x), info


class _SymmetricSolve(torch.autograd.Function):
  """x = A^-1 b with the adjoint solved by the same routine (A symmetric)."""

  @staticmethod
  def forward(ctx, b, A, kwargs, info_out):
    x, info = cg(A, b.detach(), **kwargs)
    if info_out is not None:
      info_out.update(info)
    ctx.A, ctx.kwargs = A, kwargs
    return x

  @staticmethod
  def backward(ctx, grad_x):
    # d<x, g>/db = A^-T g = A^-1 g
    grad_b, _ = cg(ctx.A, grad_x.detach().contiguous(), **ctx.kwargs)
    return grad_b, None, None, None


def symmetric_solve(A, b, info_out=None, **kwargs):
  """`cg(A, b, **kwargs)[0]` that autograd can differentiate with respect to
  `b`: the cotangent is obtained by a second solve with the same symmetric
  operator, which is what `lax.custom_linear_solve(symmetric=True)` does for
  the reference's solves (navier_stokes/navier_stokes.py:436-452).  Gradients
  with respect to tensors hidden inside `A` are not propagated.  `info_out`: a
  dict that receives the forward solve's `info`."""
  return _SymmetricSolve.apply(b, A, kwargs, info_out)
