"""The BiCGStab device kernels (csrc/sfem_bicgstab.hip) called directly: the
reduction, the three fused vector updates and the one-thread scalar phases,
against their NumPy restatements (`tests/bicgstab_reference.py`), in both
precisions and at the sizes where the launches change shape -- a second
workgroup appears at 1025 for `update_p` (1024 entries per workgroup) and at
2049 for the reducing kernels (2048), above 1024 every grid-stride loop makes
more than one trip, and 100003 gives many workgroups adding into one slot and
an odd tail.

Bounds are derived, not measured.  A sum of m numbers in double precision, in
any order, is within m 2^-53 (1 + ...) sum |terms| of the exact one; with the
rounding of each product that is (m + 1) 2^-52 sum |terms| at most
(`sum_bound`).  An output entry of a vector update is within 8 eps(dtype)
(sum of the magnitudes of its terms) of the float64 value: a handful of
roundings, FMA contraction or not, and the cast of the scalars to the vectors'
type.
"""
import numpy as np
import pytest
import torch

from swirl_fem_amd import _lib, _ops
from tests import bicgstab_reference as BS
from tests.test_gpu_advection import _Diag

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64, F32 = torch.float64, torch.float32
NS = _lib.SFEM_BICGSTAB_NSCALARS
SIZES = (1, 7, 513, 1025, 2049, 100003)
EPS = {F64: 2.0 ** -52, F32: 2.0 ** -23}
both = pytest.mark.parametrize('dtype', [F64, F32], ids=['fp64', 'fp32'])
sizes = pytest.mark.parametrize('n', SIZES)
assert NS >= BS.NSLOTS


def scalars(**slots):
  """A scalar array with every entry distinct and non-zero (a stray write or
  a missed one shows), `DONE` and `HALF` clear, then `slots` by name."""
  s = np.concatenate([0.5 + 0.01 * np.arange(BS.NSLOTS),
                      100.0 + np.arange(NS - BS.NSLOTS)])
  s[[BS.DONE, BS.HALF, BS.STATUS]] = 0.0
  for name, value in slots.items():
    s[getattr(BS, name)] = value
  return s


def to_dev(a, dtype=F64):
  return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def host(t):
  return t.detach().double().cpu().numpy()


class Vectors:
  """Named random vectors: the stored float / double values as float64 NumPy
  arrays (`v.np`) and on the device (`v.dev`)."""

  def __init__(self, n, dtype, seed, names):
    rng = np.random.default_rng(seed)
    self.dev, self.np = {}, {}
    for name in names:
      a = rng.standard_normal(n)
      if name == 'dinv':
        a = 0.5 + rng.random(n)
      self.dev[name] = to_dev(a, dtype)
      self.np[name] = host(self.dev[name])

  def unchanged(self, *names):
    for name in names:
      got = host(self.dev[name])
      assert np.array_equal(got, self.np[name], equal_nan=True), name


def exact_sum(terms):
  return float(np.sum(np.asarray(terms, np.longdouble)))


def sum_bound(terms):
  terms = np.asarray(terms, np.float64)
  return (len(terms) + 1) * 2.0 ** -52 * float(np.abs(terms).sum())


def check_sum(got, start, a, b, what):
  """got = start + a . b within the bound of a double-precision sum of the
  start value and the len(a) products (the reference sum in extended
  precision, 2^-64: nothing next to the bound)."""
  prod = a.astype(np.longdouble) * b.astype(np.longdouble)
  terms = np.concatenate([[np.longdouble(start)], prod])
  want = float(terms.sum())
  bound = sum_bound(terms.astype(np.float64))
  assert abs(got - want) <= bound, (what, got, want, abs(got - want), bound)


def check_entries(got, want, magnitude, dtype, what):
  bad = ~(np.abs(got - want) <= 8.0 * EPS[dtype] * magnitude)
  assert not bad.any(), (what, int(bad.sum()), int(np.argmax(bad)),
                         float(np.abs(got - want).max()))


def others_unchanged(got, before, *changed):
  """Every scalar but the named ones is bitwise what it was."""
  mask = np.ones(NS, dtype=bool)
  mask[[getattr(BS, c) for c in changed]] = False
  assert np.array_equal(got[mask], before[mask], equal_nan=True), \
      (got, before)


# ------------------------------------------------------------ 1. the reduction
@both
@sizes
def test_dot(n, dtype):
  v = Vectors(n, dtype, n, ('a', 'b'))
  a, b = v.np['a'], v.np['b']
  s0 = scalars()
  s = to_dev(s0)
  _ops.bicgstab_dot(v.dev['a'], v.dev['b'], s, BS.R0V)
  got = host(s)
  check_sum(got[BS.R0V], s0[BS.R0V], a, b, 'one slot')
  others_unchanged(got, s0, 'R0V')
  s = to_dev(s0)
  _ops.bicgstab_dot(v.dev['a'], v.dev['b'], s, BS.TS, two=True)
  got = host(s)
  check_sum(got[BS.TS], s0[BS.TS], a, b, 'two: a.b')
  check_sum(got[BS.TT], s0[BS.TT], a, a, 'two: a.a')
  others_unchanged(got, s0, 'TS', 'TT')
  # after a half-step stop the (t.s, t.t) pass is skipped, a plain dot is not
  s0 = scalars(HALF=1.0)
  s = to_dev(s0)
  _ops.bicgstab_dot(v.dev['a'], v.dev['b'], s, BS.TS, two=True)
  assert np.array_equal(host(s), s0)
  _ops.bicgstab_dot(v.dev['a'], v.dev['b'], s, BS.R0V)
  got = host(s)
  check_sum(got[BS.R0V], s0[BS.R0V], a, b, 'one slot, HALF set')
  others_unchanged(got, s0, 'R0V')
  v.unchanged('a', 'b')


# ------------------------------------------------------- 2. the vector updates
@pytest.mark.parametrize('fused', [True, False], ids=['dinv', 'alias'])
@both
@sizes
def test_update_p(n, dtype, fused):
  v = Vectors(n, dtype, 10 + n, ('p', 'phat', 'r', 'v', 'dinv'))
  dinv = v.np['dinv'] if fused else None
  s0 = scalars(BETA=0.6, OMEGA=-0.8)
  s = to_dev(s0)
  p = v.dev['p']
  phat = v.dev['phat'] if fused else p      # as BiCGStabRunner passes them
  _ops.bicgstab_update_p(p, phat, v.dev['r'], v.dev['v'],
                         v.dev['dinv'] if fused else None, s)
  want_p, want_phat = BS.update_p(v.np['p'], v.np['r'], v.np['v'], dinv, s0)
  mag = np.abs(v.np['r']) + 0.6 * (np.abs(v.np['p']) +
                                   0.8 * np.abs(v.np['v']))
  check_entries(host(p), want_p, mag, dtype, 'p')
  if fused:
    check_entries(host(phat), want_phat, dinv * mag, dtype, 'phat')
  else:
    v.unchanged('phat')
  v.unchanged('r', 'v', 'dinv')
  assert np.array_equal(host(s), s0)


@pytest.mark.parametrize('fused', [True, False], ids=['dinv', 'alias'])
@both
@sizes
def test_update_s(n, dtype, fused):
  v = Vectors(n, dtype, 20 + n, ('s', 'shat', 'r', 'v', 'dinv'))
  dinv = v.np['dinv'] if fused else None
  s0 = scalars(ALPHA=0.75)
  s = to_dev(s0)
  sv = v.dev['s']
  shat = v.dev['shat'] if fused else sv
  _ops.bicgstab_update_s(sv, shat, v.dev['r'], v.dev['v'],
                         v.dev['dinv'] if fused else None, s)
  want_s, want_shat, _ = BS.update_s(v.np['r'], v.np['v'], dinv, s0)
  mag = np.abs(v.np['r']) + 0.75 * np.abs(v.np['v'])
  got_s = host(sv)
  check_entries(got_s, want_s, mag, dtype, 's')
  if fused:
    check_entries(host(shat), want_shat, dinv * mag, dtype, 'shat')
  else:
    v.unchanged('shat')
  v.unchanged('r', 'v', 'dinv')
  got = host(s)
  check_sum(got[BS.SS], s0[BS.SS], got_s, got_s, 's.s of the stored s')
  others_unchanged(got, s0, 'SS')


@pytest.mark.parametrize('fused', [True, False], ids=['dinv', 'alias'])
@both
@sizes
def test_update_xr(n, dtype, fused):
  v = Vectors(n, dtype, 30 + n, ('x', 'r', 'phat', 'shat', 's', 't', 'r0'))
  alpha, ts, tt = 0.75, -0.9, 1.7
  s0 = scalars(ALPHA=alpha, TS=ts, TT=tt)
  omega = BS.omega_of(s0)
  assert omega == ts / tt
  s = to_dev(s0)
  # not fused: phat is p (any vector here) and shat is s itself
  shat_name = 'shat' if fused else 's'
  _ops.bicgstab_update_xr(v.dev['x'], v.dev['r'], v.dev['phat'],
                          v.dev[shat_name], v.dev['s'], v.dev['t'],
                          v.dev['r0'], s)
  w = v.np
  want_x, want_r, _, _ = BS.update_xr(w['x'], w['phat'], w[shat_name], w['s'],
                                      w['t'], w['r0'], s0)
  got_x, got_r = host(v.dev['x']), host(v.dev['r'])
  check_entries(got_x, want_x, np.abs(w['x']) + alpha * np.abs(w['phat']) +
                abs(omega) * np.abs(w[shat_name]), dtype, 'x')
  check_entries(got_r, want_r, np.abs(w['s']) + abs(omega) * np.abs(w['t']),
                dtype, 'r')
  v.unchanged('phat', 'shat', 's', 't', 'r0')
  got = host(s)
  check_sum(got[BS.RR], s0[BS.RR], got_r, got_r, 'r.r of the stored r')
  check_sum(got[BS.RHO_NEW], s0[BS.RHO_NEW], w['r0'], got_r, 'r0.r')
  others_unchanged(got, s0, 'RR', 'RHO_NEW')


@pytest.mark.parametrize('why', ['HALF', 'TT'])
@both
@sizes
def test_update_xr_half_step_reads_neither_t_nor_shat(n, dtype, why):
  """After a half-step stop (and when t.t = 0) x += alpha phat and r = s: t
  was never formed, so with t and shat full of NaN nothing may become NaN."""
  v = Vectors(n, dtype, 40 + n, ('x', 'r', 'phat', 's', 'r0'))
  nan = torch.full((n,), float('nan'), dtype=dtype, device=DEV)
  shat, t = nan.clone(), nan.clone()
  alpha = 0.75
  s0 = (scalars(ALPHA=alpha, HALF=1.0, TS=-0.9, TT=1.7) if why == 'HALF'
        else scalars(ALPHA=alpha, TS=-0.9, TT=0.0))
  s = to_dev(s0)
  _ops.bicgstab_update_xr(v.dev['x'], v.dev['r'], v.dev['phat'], shat,
                          v.dev['s'], t, v.dev['r0'], s)
  w = v.np
  got_x, got_r, got = host(v.dev['x']), host(v.dev['r']), host(s)
  assert np.isfinite(got_x).all() and np.isfinite(got_r).all()
  assert np.isfinite(got).all()
  want_x, want_r, _, _ = BS.update_xr(w['x'], w['phat'], host(shat), w['s'],
                                      host(t), w['r0'], s0)
  check_entries(got_x, want_x, np.abs(w['x']) + alpha * np.abs(w['phat']),
                dtype, 'x')
  assert np.array_equal(got_r, w['s']) and np.array_equal(want_r, w['s'])
  check_sum(got[BS.RR], s0[BS.RR], got_r, got_r, 'r.r')
  check_sum(got[BS.RHO_NEW], s0[BS.RHO_NEW], w['r0'], got_r, 'r0.r')
  others_unchanged(got, s0, 'RR', 'RHO_NEW')
  v.unchanged('phat', 's', 'r0')


# ------------------------------------------------------------- 3. `DONE` set
@both
def test_a_finished_solve_is_left_alone(dtype):
  n = 2049
  names = ('x', 'r', 'p', 'phat', 's', 'shat', 'v', 't', 'r0', 'dinv')
  v = Vectors(n, dtype, 5, names)
  d = v.dev
  s0 = scalars(DONE=1.0, STATUS=1.0, TS=-0.9, TT=1.7)
  s = to_dev(s0)
  _ops.bicgstab_dot(d['r0'], d['v'], s, BS.R0V)
  _ops.bicgstab_dot(d['t'], d['s'], s, BS.TS, two=True)
  _ops.bicgstab_update_p(d['p'], d['phat'], d['r'], d['v'], d['dinv'], s)
  _ops.bicgstab_update_p(d['p'], d['p'], d['r'], d['v'], None, s)
  _ops.bicgstab_update_s(d['s'], d['shat'], d['r'], d['v'], d['dinv'], s)
  _ops.bicgstab_update_s(d['s'], d['s'], d['r'], d['v'], None, s)
  _ops.bicgstab_update_xr(d['x'], d['r'], d['phat'], d['shat'], d['s'],
                          d['t'], d['r0'], s)
  for phase in (1, 2, 3):
    _ops.bicgstab_scalars(s, phase, 10, 1e-5, 0.0)
  assert np.array_equal(host(s), s0)
  v.unchanged(*names)
  # phase 0 starts a new solve: it clears the flag
  _ops.bicgstab_scalars(s, 0, 10, 1e-5, 0.0)
  got = host(s)
  want = BS.scalar_phase(s0, 0, 10, 1e-5, 0.0)
  assert np.array_equal(got, want)
  assert got[BS.DONE] == 0.0 and got[BS.STATUS] == 0.0
  _ops.bicgstab_dot(d['r0'], d['v'], s, BS.R0V)
  assert host(s)[BS.R0V] != 0.0


# ------------------------------------------------------- 4. the scalar phases
_T = dict(THRESHOLD=1e-10)
PHASE_TABLE = [
    # (name, phase, slots, maxiter, tol, atol, status afterwards)
    ('start', 0, dict(BB=2.0, RR=1.5, RHO_NEW=1.5), 10, 1e-5, 0.0, 'running'),
    ('start converged', 0, dict(BB=1.0, RR=1e-12, RHO_NEW=1e-12), 10, 1e-5,
     0.0, 'converged'),
    ('start at the threshold', 0, dict(BB=1.0, RR=0.25, RHO_NEW=0.25), 10,
     0.5, 0.0, 'converged'),
    ('start b = 0', 0, dict(BB=0.0, RR=0.0, RHO_NEW=0.0), 10, 1e-5, 0.0,
     'converged'),
    ('start rho = 0', 0, dict(BB=1.0, RR=1.0, RHO_NEW=0.0), 10, 1e-5, 0.0,
     'breakdown_rho'),
    ('start r.r inf', 0, dict(BB=1.0, RR=np.inf, RHO_NEW=np.inf), 10, 1e-5,
     0.0, 'breakdown_rho'),
    ('start r.r nan', 0, dict(BB=1.0, RR=np.nan, RHO_NEW=np.nan), 10, 1e-5,
     0.0, 'breakdown_rho'),
    ('start maxiter 0', 0, dict(BB=1.0, RR=1.0, RHO_NEW=1.0), 0, 1e-5, 0.0,
     'maxiter'),
    ('start maxiter < 0', 0, dict(BB=1.0, RR=1.0, RHO_NEW=1.0), -3, 1e-5,
     0.0, 'maxiter'),
    ('start atol wins', 0, dict(BB=1.0, RR=5e-5, RHO_NEW=5e-5), 10, 1e-5,
     1e-2, 'converged'),
    ('start tol alone', 0, dict(BB=1.0, RR=5e-5, RHO_NEW=5e-5), 10, 1e-5,
     0.0, 'running'),
    ('alpha', 1, dict(RHO=0.9, R0V=0.7), 10, 1e-5, 0.0, 'running'),
    ('alpha r0.v = 0', 1, dict(RHO=0.9, R0V=0.0), 10, 1e-5, 0.0,
     'breakdown_alpha'),
    ('alpha overflows', 1, dict(RHO=1e300, R0V=1e-300), 10, 1e-5, 0.0,
     'breakdown_alpha'),
    ('half on', 2, dict(SS=1e-11, **_T), 10, 1e-5, 0.0, 'running'),
    ('half at the threshold', 2, dict(SS=1e-10, **_T), 10, 1e-5, 0.0,
     'running'),
    ('half off', 2, dict(SS=1e-9, HALF=1.0, **_T), 10, 1e-5, 0.0, 'running'),
    ('half s.s nan', 2, dict(SS=np.nan, HALF=1.0, **_T), 10, 1e-5, 0.0,
     'running'),
    ('close r.r inf after a half step', 3,
     dict(RR=np.inf, HALF=1.0, TS=0.3, TT=0.7, **_T), 10, 1e-5, 0.0,
     'breakdown_rho'),
    ('close r.r nan, omega != 0', 3, dict(RR=np.nan, TS=0.3, TT=0.7, **_T),
     10, 1e-5, 0.0, 'breakdown_rho'),
    ('close r.r inf, omega = 0', 3, dict(RR=np.inf, TS=0.3, TT=0.0, **_T), 10,
     1e-5, 0.0, 'breakdown_omega'),
    ('close converged', 3, dict(RR=1e-11, TS=0.3, TT=0.7, **_T), 10, 1e-5,
     0.0, 'converged'),
    ('close converged in the half step', 3,
     dict(RR=1e-11, HALF=1.0, TS=0.3, TT=0.7, **_T), 10, 1e-5, 0.0,
     'converged'),
    ('close t.t = 0', 3, dict(RR=1.0, TS=0.0, TT=0.0, **_T), 10, 1e-5, 0.0,
     'breakdown_omega'),
    ('close t.s = 0', 3, dict(RR=1.0, TS=0.0, TT=0.7, **_T), 10, 1e-5, 0.0,
     'breakdown_omega'),
    ('close omega overflows', 3, dict(RR=1.0, TS=1e300, TT=1e-300, **_T), 10,
     1e-5, 0.0, 'breakdown_omega'),
    ('close rho_new = 0', 3, dict(RR=1.0, RHO_NEW=0.0, TS=0.3, TT=0.7, **_T),
     10, 1e-5, 0.0, 'breakdown_rho'),
    ('close rho_new inf', 3,
     dict(RR=1.0, RHO_NEW=np.inf, TS=0.3, TT=0.7, **_T), 10, 1e-5, 0.0,
     'breakdown_rho'),
    ('close maxiter', 3,
     dict(RR=1.0, RHO_NEW=0.4, ITERS=9.0, TS=0.3, TT=0.7, **_T), 10, 1e-5,
     0.0, 'maxiter'),
    ('close and go on', 3,
     dict(RR=1.0, RHO=0.9, RHO_NEW=0.4, ALPHA=0.75, ITERS=3.0, TS=0.3, TT=0.7,
          **_T), 10, 1e-5, 0.0, 'running'),
]
QUOTIENTS = (BS.ALPHA, BS.OMEGA, BS.BETA)


def test_the_table_reaches_every_status():
  assert {row[-1] for row in PHASE_TABLE} == set(_lib.BICGSTAB_STATUS.values())
  assert set(BS.STATUS_CODE) == set(_lib.BICGSTAB_STATUS.values())
  assert all(BS.STATUS_CODE[name] == code
             for code, name in _lib.BICGSTAB_STATUS.items())


@pytest.mark.parametrize('row', PHASE_TABLE, ids=[r[0] for r in PHASE_TABLE])
def test_scalar_phase(row):
  name, phase, slots, maxiter, tol, atol, status = row
  s0 = scalars(**slots)
  want = BS.scalar_phase(s0, phase, maxiter, tol, atol)
  assert want[BS.STATUS] == BS.STATUS_CODE[status]
  assert want[BS.DONE] == float(status != 'running')
  s = to_dev(s0)
  _ops.bicgstab_scalars(s, phase, maxiter, tol, atol)
  got = host(s)
  print(name, got[:BS.NSLOTS])
  exact = np.ones(NS, dtype=bool)
  exact[list(QUOTIENTS)] = False
  assert np.array_equal(got[exact], want[exact], equal_nan=True), (got, want)
  for q in QUOTIENTS:
    assert abs(got[q] - want[q]) <= np.spacing(abs(want[q])), (q, got, want)
  if name == 'close and go on':
    omega = 0.3 / 0.7
    assert abs(got[BS.BETA] - (0.4 / 0.9) * (0.75 / omega)) <= 1e-15
    assert got[BS.RHO] == 0.4 and got[BS.ITERS] == 4.0
    assert got[BS.RESIDUAL] == 1.0 and got[BS.R0V] == 0.0


# ------------------------------------------------------- 5. the entry points
def test_entry_point_refusals():
  """Return codes of the five C entry points; nothing that is refused
  launches (the scalars and the vectors keep their values)."""
  lib = _lib.load()
  n = 100
  names = ('x', 'r', 'p', 'phat', 's', 'shat', 'v', 't', 'r0', 'dinv')
  v = Vectors(n, F64, 9, names)
  q = {k: t.data_ptr() for k, t in v.dev.items()}
  s0 = scalars(TS=0.3, TT=0.7)
  s = to_dev(s0)
  sp = s.data_ptr()
  OK, EINVAL = 0, -1
  D = _lib.SFEM_F64

  def dot(a=q['r0'], b=q['v'], count=n, scal=sp, slot=BS.R0V, two=0, dtype=D):
    return lib.sfem_bicgstab_dot(a, b, count, scal, slot, two, dtype, None)

  def up(count=n, scal=sp, dtype=D, p=q['p']):
    return lib.sfem_bicgstab_update_p(p, q['phat'], q['r'], q['v'],
                                      q['dinv'], count, scal, dtype, None)

  def us(count=n, scal=sp, dtype=D, sv=q['s']):
    return lib.sfem_bicgstab_update_s(sv, q['shat'], q['r'], q['v'],
                                      q['dinv'], count, scal, dtype, None)

  def uxr(count=n, scal=sp, dtype=D, x=q['x']):
    return lib.sfem_bicgstab_update_xr(x, q['r'], q['phat'], q['shat'],
                                       q['s'], q['t'], q['r0'], count, scal,
                                       dtype, None)

  def phase(k, scal=sp):
    return lib.sfem_bicgstab_scalars(scal, k, 10.0, 1e-5, 0.0, None)

  for call in (dot, up, us, uxr):
    assert call(scal=None) == EINVAL
    assert call(count=-1) == EINVAL
    assert call(dtype=7) == EINVAL and call(dtype=-1) == EINVAL
  assert dot(a=None) == EINVAL and dot(b=None) == EINVAL
  assert up(p=None) == EINVAL and us(sv=None) == EINVAL
  assert uxr(x=None) == EINVAL
  for slot, two in ((-1, 0), (NS, 0), (NS - 1, 1), (-1, 1), (NS, 1)):
    assert dot(slot=slot, two=two) == EINVAL
  for k in (-1, 4, 17):
    assert phase(k) == EINVAL
  assert phase(0, scal=None) == EINVAL
  # count = 0: nothing to do, whatever the vectors
  assert dot(a=None, b=None, count=0) == OK
  for call in (up, us, uxr):
    assert call(count=0) == OK
  assert lib.sfem_bicgstab_update_p(None, None, None, None, None, 0, sp, D,
                                    None) == OK
  assert lib.sfem_bicgstab_update_s(None, None, None, None, None, 0, sp, D,
                                    None) == OK
  assert lib.sfem_bicgstab_update_xr(None, None, None, None, None, None, None,
                                     0, sp, D, None) == OK
  torch.cuda.synchronize()
  assert np.array_equal(host(s), s0)
  v.unchanged(*names)
  # the last slot is a valid single slot
  assert dot(slot=NS - 1) == OK
  got = host(s)
  check_sum(got[NS - 1], s0[NS - 1], v.np['r0'], v.np['v'], 'last slot')
  assert np.array_equal(got[:NS - 1], s0[:NS - 1])


# ------------------------------------------- 6. one solve above a workgroup
def _roll_system(n=100003, seed=11):
  rng = np.random.default_rng(seed)
  d = 2.0 + rng.random(n)
  b = rng.standard_normal(n)
  A = lambda v: d * v + 0.5 * np.roll(v, 1) - 0.3 * np.roll(v, -1)
  dd = to_dev(d)
  Ad = lambda v: dd * v + 0.5 * torch.roll(v, 1) - 0.3 * torch.roll(v, -1)
  return A, Ad, d, b


@pytest.mark.parametrize('precond', [None, 'fused'])
def test_solve_above_a_workgroup(precond):
  """A v = d v + 0.5 roll(v, 1) - 0.3 roll(v, -1), d in [2, 3], n = 100003:
  strictly diagonally dominant, |A| <= 3.8, |A^-1| <= 1 / 1.2, condition
  number below 4.  The first 10 iterates against the NumPy recurrence to
  1e-10 (the bound of the n = 200 test, whose condition number is larger),
  then a solve to 1e-12."""
  from swirl_fem_amd.linalg.bicgstab import BiCGStabRunner, bicgstab
  A, Ad, d, b = _roll_system()
  n = len(b)
  dinv = 1.0 / d
  M = None if precond is None else _Diag(to_dev(dinv))
  Mh = None if precond is None else (lambda v: dinv * v)
  _, iterates, _ = BS.bicgstab(A, b, tol=1e-30, maxiter=10, M=Mh)
  assert len(iterates) == 10
  run = BiCGStabRunner(Ad, to_dev(b), tol=1e-30, M=M)
  assert (run.dinv is not None) == (precond == 'fused')
  for k, want in enumerate(iterates):
    run.step()
    got = host(run.x)
    err = np.abs(got - want).max() / np.abs(want).max()
    assert err <= 1e-10, (k, err)
  assert run.info()['num_iterations'] == 10
  x, info = bicgstab(Ad, to_dev(b), tol=1e-12, M=M)
  assert info['status'] == 'converged'
  res = b - A(host(x))
  print('n=%d %s: %d iterations, |b - A x|^2 / b.b = %.3e' % (
      n, precond, info['num_iterations'], (res @ res) / (b @ b)))
  assert res @ res <= 1e-22 * (b @ b)
