"""The CG device kernels (csrc/sfem_core.hip; `sfem_pmg_dot2`,
`sfem_pmg_cg_scalars` and `sfem_cheb_step` of csrc/sfem_pmg.hip) called
directly, against their NumPy restatements (`tests/cg_reference.py`), in both
precisions, at three kinds of sizes:

  small   1 .. 100003: scalar tails (1, 2, 3, 5, 7), one workgroup and the
          first entry of a second (1023, 1025, 2049), many workgroups adding
          into the same slots and an odd tail (100003);
  middle  8 388 613: `reduce_grid` caps a launch at 4096 workgroups of 512
          lanes, one 16-byte access per lane and trip, so the grid-stride loop
          of `dot_kernel`, `cg_update_xr_kernel` and `cg_update_r_kernel`
          (fuse 0 / 1) makes a second trip above 4 194 304 (fp64) / 8 388 608
          (fp32) entries;
  large   2^25 + 3 (fp64), 2^26 + 5 (fp32): just past 256 MiB per vector,
          where `streams_past_caches` picks the non-temporal instantiations
          and `stream_grid` (32768 workgroups) makes its second trip.

Bounds are derived, as in `test_gpu_bicgstab_kernels.py`: a double-precision
sum of m terms, in any order, is within (m + 1) 2^-52 sum |terms|
(`sum_bound`); an entry of a vector update is within 8 eps(dtype) (sum of the
magnitudes of its terms).  At the middle and large sizes the reference is
torch float64 on the device, whose own sums round: twice `sum_bound` there.
Every check prints `CGERR kernel n dtype error/bound` (profiles/
cg_kernel_errors.md is the table of those)."""
import numpy as np
import pytest
import torch

from swirl_fem_amd import _lib, _ops
from tests import cg_reference as CG
from tests.test_gpu_bicgstab_kernels import (
    EPS, Vectors, check_entries, host, sum_bound, to_dev)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64, F32 = torch.float64, torch.float32
NPT = {F64: np.float64, F32: np.float32}
NAME = {F64: 'fp64', F32: 'fp32'}
NS = _lib.SFEM_CG_NSCALARS
SMALL = (1, 2, 3, 5, 7, 1023, 1025, 2049, 100003)
MIDDLE = 8388613
LARGE = {F64: 2 ** 25 + 3, F32: 2 ** 26 + 5}
both = pytest.mark.parametrize('dtype', [F64, F32], ids=['fp64', 'fp32'])
small = pytest.mark.parametrize('n', SMALL)
ARGS = (10, 1e-5, 0.0)                        # maxiter, tol, atol
assert (NS, _lib.SFEM_CG_NSCALARS_NAMED) == (CG.NSLOTS, CG.NAMED)
assert _lib.SFEM_DOT_SLOTS == CG.DOT_SLOTS
assert _lib.SFEM_FOLD_GROUPS == CG.FOLD_GROUPS
assert _lib.SFEM_CG_MEAN_SUMS == CG.MEAN_SUMS
assert _lib.SFEM_CG_LAZY_MAX == CG.LAZY_MAX
STRIPE_IDX = list(range(CG.NAMED, NS))


def block(**slots):
  """A scalar block with every entry distinct and non-zero (a stray write or
  a missed one shows), the flags `DONE`, `OPEN`, `STATUS` clear, three
  iterations done; then `slots` by name.  gamma_new lies partly in [2] and
  partly in the stripes; the stripes are multiples of 2^-10, so their sum is
  the same in any order."""
  s = np.concatenate([0.5 + 0.01 * np.arange(CG.NAMED),
                      (1.0 + np.arange(CG.RR_SLOTS)) / 1024.0])
  s[[CG.DONE, CG.OPEN, CG.STATUS]] = 0.0
  s[CG.ITERS] = 3.0
  s[CG.GAMMA_NEW] = 0.75
  for name, value in slots.items():
    s[getattr(CG, name)] = value
  return s


def note(kernel, n, dtype, err, bound):
  ratio = 0.0 if err == 0.0 else err / bound if bound > 0.0 else np.inf
  print('CGERR %s %d %s %.3g' % (kernel, n, NAME.get(dtype, dtype), ratio))


def entries(kernel, dtype, got, want, magnitude, what=''):
  with np.errstate(all='ignore'):
    ratio = np.abs(got - want) / (8.0 * EPS[dtype] * magnitude)
  ratio = ratio[np.abs(got - want) > 0.0]
  note(kernel, len(got), dtype, float(ratio.max()) if ratio.size else 0.0, 1.0)
  check_entries(got, want, magnitude, dtype, (kernel, what))


def summed(kernel, dtype, got, starts, a, b, scale=1.0, factor=1.0, n=None):
  """got = sum(starts) + scale a.b within `factor` x the bound of a
  double-precision sum of those terms, in any order."""
  prod = (np.longdouble(scale) * np.asarray(a, np.longdouble) *
          np.asarray(b, np.longdouble))
  terms = np.concatenate([np.atleast_1d(starts).astype(np.longdouble), prod])
  want = float(terms.sum())
  bound = factor * sum_bound(terms.astype(np.float64))
  note(kernel, len(prod) if n is None else n, dtype, abs(got - want), bound)
  assert abs(got - want) <= bound, (kernel, got, want, abs(got - want), bound)


def same_but(got, before, *changed):
  """Every scalar but those at the positions `changed` is bitwise what it
  was."""
  mask = np.ones(len(before), dtype=bool)
  mask[list(changed)] = False
  assert np.array_equal(got[mask], before[mask], equal_nan=True), \
      (np.flatnonzero(~((got == before) | ~mask)), got, before)


def vectors(n, dtype, seed, names):
  """`Vectors`, with w (a weight) positive like dinv."""
  v = Vectors(n, dtype, seed, names)
  if 'w' in names:
    v.dev['w'] = v.dev['w'].abs() + 0.5
    v.np['w'] = host(v.dev['w'])
  return v


def nan_like(t):
  return torch.full_like(t, float('nan'))


# ------------------------------------------------------------ 1. reductions
@both
@small
def test_dot(n, dtype):
  v = vectors(n, dtype, n, ('a', 'b'))
  s0 = block()
  s = to_dev(s0)
  _ops.dot(v.dev['a'], v.dev['b'], s, CG.PAP)            # clears the slot first
  got = host(s)
  summed('dot', dtype, got[CG.PAP], 0.0, v.np['a'], v.np['b'])
  same_but(got, s0, CG.PAP)
  s = to_dev(s0)
  _ops.dot(v.dev['a'], v.dev['b'], s, CG.GAMMA_NEW, accumulate=True)
  got = host(s)
  summed('dot_accumulate', dtype, got[CG.GAMMA_NEW], s0[CG.GAMMA_NEW],
         v.np['a'], v.np['b'])
  same_but(got, s0, CG.GAMMA_NEW)
  v.unchanged('a', 'b')


@pytest.mark.parametrize('ncomp,layout', [(1, 'node_major'), (3, 'node_major'),
                                          (3, 'component_major')])
@pytest.mark.parametrize('count', [1, 255, 257, 100003])
@both
def test_dot_indexed(dtype, count, ncomp, layout):
  """result += scale sum_i w[i] <a[idx[i]], b[idx[i]]> over an index list with
  repeats (100003 entries into 1000 nodes), both field layouts.  A term is
  two products and the scale: three roundings, (m + 3) 2^-53 in all, which
  `sum_bound` covers."""
  nodes = 1000
  rng = np.random.default_rng(count + ncomp)
  shape = (nodes,) if ncomp == 1 else (nodes, ncomp)

  def field():
    t = to_dev(rng.standard_normal(shape), dtype)
    if layout == 'component_major':
      t = t.T.contiguous().T
      assert _ops.is_component_major(t) and not t.is_contiguous()
    return t

  a, b = field(), field()
  idx_np = rng.integers(0, nodes, count)
  if count > 1:
    idx_np[1] = idx_np[0]                                # a repeat for sure
  w_np = rng.random(count) - 0.3
  idx, w = to_dev(idx_np, torch.int64), to_dev(w_np)
  an, bn = host(a).reshape(nodes, ncomp), host(b).reshape(nodes, ncomp)
  s0 = block()
  for scale in (-1.0, 0.5):
    s = to_dev(s0)
    _ops.dot_indexed(a, b, idx, w, s, CG.GAMMA_NEW, scale)
    got = host(s)
    summed('dot_indexed', dtype, got[CG.GAMMA_NEW], s0[CG.GAMMA_NEW],
           np.repeat(w_np, ncomp),
           (an[idx_np].astype(np.longdouble) * bn[idx_np]).reshape(-1),
           scale=scale, n=count)
    same_but(got, s0, CG.GAMMA_NEW)
  # a total of exactly zero is not added.  The one place where adding it
  # would show: a slot that holds -0.0, which -0.0 + (0.5 * 0.0) turns into
  # +0.0; on any other value x + 0.0 leaves the bits, guard or no guard
  s0 = block(GAMMA_NEW=-0.0)
  s = to_dev(s0)
  _ops.dot_indexed(a, b, idx, torch.zeros_like(w), s, CG.GAMMA_NEW, 0.5)
  got = host(s)
  assert np.array_equal(got, s0) and np.signbit(got[CG.GAMMA_NEW])
  assert np.array_equal(host(a).reshape(nodes, ncomp), an)


@both
@small
def test_axpby(n, dtype):
  v = vectors(n, dtype, 3 + n, ('x', 'y'))
  a, b = 0.37, -1.9
  y = v.dev['y'].clone()
  _ops.axpby(a, v.dev['x'], b, y)
  want = CG.axpby(a, v.np['x'], b, v.np['y'], NPT[dtype])
  entries('axpby', dtype, host(y), want,
          abs(a) * np.abs(v.np['x']) + abs(b) * np.abs(v.np['y']))
  y = nan_like(v.dev['y'])                               # b = 0: y is not read
  _ops.axpby(a, v.dev['x'], 0.0, y)
  want = CG.axpby(a, v.np['x'], 0.0, None, NPT[dtype])
  entries('axpby', dtype, host(y), want, abs(a) * np.abs(v.np['x']), 'b = 0')
  v.unchanged('x')


@pytest.mark.parametrize('alias', [False, True], ids=['out', 'in_place'])
@pytest.mark.parametrize('with_dot', [False, True], ids=['plain', 'dot'])
@both
@small
def test_subtract_weighted_mean(n, dtype, with_dot, alias):
  """out = w - (b.w / total) 1.  The mean is a double-precision sum of n
  terms times 1 / total (its error: `sum_bound` / |total|, one rounding for
  the reciprocal, one for the product), cast to the vectors' type."""
  v = vectors(n, dtype, 7 + n, ('v', 'w'))
  vec, bw = v.np['v'], v.np['w']                 # "w" of the kernel, "b"
  total = float(bw.sum())
  partials = torch.full((CG.DOT_SLOTS,), float('nan'), dtype=F64, device=DEV)
  s0 = block()
  s = to_dev(s0)
  src = v.dev['v'].clone()
  out = src if alias else nan_like(src)
  res = _ops.subtract_weighted_mean(
      src, v.dev['w'], total, partials, out=out,
      dot_result=(s, CG.GAMMA_NEW) if with_dot else None)
  assert res.data_ptr() == out.data_ptr()
  want, _ = CG.subtract_weighted_mean(vec, bw, total)
  mean = abs(float(np.vdot(bw, vec)) / total)
  slack = (sum_bound(bw * vec) + 4 * 2.0 ** -52 * abs(np.vdot(bw, vec))) \
      / abs(total)
  got_out = host(out)
  entries('subtract_weighted_mean', dtype, got_out, want,
          np.abs(vec) + mean + slack / (8.0 * EPS[dtype]))
  got = host(s)
  if with_dot:
    summed('subtract_weighted_mean.dot', dtype, got[CG.GAMMA_NEW],
           s0[CG.GAMMA_NEW], vec, got_out)
    same_but(got, s0, CG.GAMMA_NEW)
  else:
    assert np.array_equal(got, s0)
  if not alias:
    assert np.array_equal(host(src), vec)
  v.unchanged('w')


# --------------------------------------------------------- 2. vector updates
def _alpha_beta(s0, dtype):
  return abs(CG.alpha_of(s0, NPT[dtype])), abs(CG.beta_of(s0, NPT[dtype]))


@pytest.mark.parametrize('fuse', [0, 1])
@both
@small
def test_update_xr(n, dtype, fuse):
  v = vectors(n, dtype, 10 + n, ('x', 'r', 'p', 'ap'))
  w = v.np
  s0 = block()
  s = to_dev(s0)
  _ops.cg_update_xr(v.dev['x'], v.dev['r'], v.dev['p'], v.dev['ap'], s, fuse)
  want_x, want_r, _ = CG.update_xr(w['x'], w['r'], w['p'], w['ap'], s0,
                                   NPT[dtype])
  a, _ = _alpha_beta(s0, dtype)
  got_r = host(v.dev['r'])
  entries('update_xr', dtype, host(v.dev['x']), want_x,
          np.abs(w['x']) + a * np.abs(w['p']), 'x')
  entries('update_xr', dtype, got_r, want_r,
          np.abs(w['r']) + a * np.abs(w['ap']), 'r')
  got = host(s)
  if fuse:
    summed('update_xr.rr', dtype, got[CG.GAMMA_NEW], s0[CG.GAMMA_NEW], got_r,
           got_r)
    same_but(got, s0, CG.GAMMA_NEW)
  else:
    assert np.array_equal(got, s0)
  v.unchanged('p', 'ap')


@pytest.mark.parametrize('fuse', [0, 1, 2])
@both
@small
def test_update_r(n, dtype, fuse):
  """r -= alpha Ap; r.r of the stored r goes nowhere (0), to [2] (1) or to
  the 64 stripes (2) -- on top of what is there, nothing else touched."""
  v = vectors(n, dtype, 20 + n, ('r', 'ap'))
  w = v.np
  s0 = block()
  s = to_dev(s0)
  _ops.cg_update_r(v.dev['r'], v.dev['ap'], s, fuse)
  want_r, _ = CG.update_r(w['r'], w['ap'], s0, NPT[dtype])
  a, _ = _alpha_beta(s0, dtype)
  got_r, got = host(v.dev['r']), host(s)
  entries('update_r', dtype, got_r, want_r,
          np.abs(w['r']) + a * np.abs(w['ap']))
  if fuse == 0:
    assert np.array_equal(got, s0)
  elif fuse == 1:
    summed('update_r.rr', dtype, got[CG.GAMMA_NEW], s0[CG.GAMMA_NEW], got_r,
           got_r)
    same_but(got, s0, CG.GAMMA_NEW)
  else:
    summed('update_r.rr_striped', dtype, CG.total(got[CG.STRIPES]),
           s0[CG.STRIPES], got_r, got_r)
    same_but(got, s0, *STRIPE_IDX)
    # workgroup g adds to stripe g mod 64.  A workgroup's 512 lanes take one
    # 16-byte access each: 1024 (fp64) / 2048 (fp32) entries; the tail is
    # workgroup 0's, and a workgroup without work adds 0.0
    per_group = 512 * (16 // dtype.itemsize)
    used = min(CG.RR_SLOTS, max(1, -(-(n - n % (16 // dtype.itemsize))
                                     // per_group)))
    assert np.array_equal(got[CG.NAMED + used:], s0[CG.NAMED + used:])
  v.unchanged('ap')


@both
@small
def test_update_p(n, dtype):
  """beta = gamma_new / gamma with gamma_new partly in [2], partly in the
  stripes (`block`)."""
  v = vectors(n, dtype, 30 + n, ('p', 'z'))
  w = v.np
  s0 = block()
  assert s0[CG.GAMMA_NEW] != 0.0 and s0[CG.STRIPES].all()
  s = to_dev(s0)
  _ops.cg_update_p(v.dev['p'], v.dev['z'], s)
  _, beta = _alpha_beta(s0, dtype)
  entries('update_p', dtype, host(v.dev['p']),
          CG.update_p(w['p'], w['z'], s0, NPT[dtype]),
          np.abs(w['z']) + beta * np.abs(w['p']))
  assert np.array_equal(host(s), s0)
  v.unchanged('z')


@both
@small
def test_update_xp(n, dtype):
  v = vectors(n, dtype, 40 + n, ('x', 'p', 'z'))
  w = v.np
  s0 = block()
  s = to_dev(s0)
  _ops.cg_update_xp(v.dev['x'], v.dev['p'], v.dev['z'], s)
  want_x, want_p = CG.update_xp(w['x'], w['p'], w['z'], s0, NPT[dtype])
  a, beta = _alpha_beta(s0, dtype)
  entries('update_xp', dtype, host(v.dev['x']), want_x,
          np.abs(w['x']) + a * np.abs(w['p']), 'x')
  entries('update_xp', dtype, host(v.dev['p']), want_p,
          np.abs(w['z']) + beta * np.abs(w['p']), 'p')
  assert np.array_equal(host(s), s0)
  v.unchanged('z')


def _ring(n, m, dtype, seed):
  """A ring of m directions with a stride larger than n (a multiple of 16
  bytes), the padding filled with a marker."""
  stride = n + (-n) % 4 + 4
  rng = np.random.default_rng(seed)
  ring = np.full((m, stride), 77.0)
  ring[:, :n] = rng.standard_normal((m, n))
  dev = to_dev(ring, dtype)
  return dev, host(dev)


def _lazy_states(m):
  """(iterations closed, iterations already in x): the state the update
  itself leaves (every full turn of the ring is in x), and the one after the
  host has looked at x in between (`flush_x`: everything is in x)."""
  for k in range(2 * m + 1):
    yield k, k - k % m
    if k % m:
      yield k, k


@pytest.mark.parametrize('m', [2, 3, 4, 8])
@both
@small
def test_update_xp_lazy_and_flush(n, dtype, m):
  """`scalars[8]` = 0 .. 2m: launches that only write the next direction,
  launches that add the pending terms, and the wrap of the ring; then
  `flush_x` with every number of terms pending."""
  v = vectors(n, dtype, 50 + n, ('x', 'z'))
  ring_dev, ring_np = _ring(n, m, dtype, n + m)
  alphas = 0.3 + 0.1 * np.arange(CG.LAZY_MAX)
  pending = set()
  for k, in_x in _lazy_states(m):
    s0 = block(ITERS=float(k))
    lazy0 = np.concatenate([[float(in_x)], alphas])
    s, lazy = to_dev(s0), to_dev(lazy0)
    x, ring = v.dev['x'].clone(), ring_dev.clone()
    _ops.cg_update_xp_lazy(x, ring, v.dev['z'], s, lazy)
    want_x, want_ring, want_lazy = CG.update_xp_lazy(
        v.np['x'], ring_np[:, :n], v.np['z'], s0, lazy0, NPT[dtype])
    a, beta = _alpha_beta(s0, dtype)
    got_ring = host(ring)
    nxt = (k + 1) % m
    if nxt == 0:
      mag = np.abs(v.np['x']) + a * np.abs(ring_np[k % m, :n])
      for j in range(max(in_x, k + 1 - m), k):
        mag = mag + alphas[j % m] * np.abs(ring_np[j % m, :n])
      entries('update_xp_lazy', dtype, host(x), want_x, mag, ('x', k, in_x))
    else:
      assert np.array_equal(host(x), v.np['x']), (k, in_x)
    entries('update_xp_lazy', dtype, got_ring[nxt, :n], want_ring[nxt],
            np.abs(v.np['z']) + beta * np.abs(ring_np[k % m, :n]),
            ('p', k, in_x))
    keep = np.ones_like(ring_np, dtype=bool)
    keep[nxt, :n] = False
    assert np.array_equal(got_ring[keep], ring_np[keep]), (k, in_x)
    assert np.array_equal(host(lazy), want_lazy), (k, in_x)
    assert np.array_equal(host(s), s0)
    # flush_x from the same state
    lazy = to_dev(lazy0)
    x, ring = v.dev['x'].clone(), ring_dev.clone()
    _ops.cg_flush_x(x, ring, s, lazy)
    want_x, want_lazy = CG.flush_x(v.np['x'], ring_np[:, :n], s0, lazy0,
                                   NPT[dtype])
    lo = max(in_x, k - k % m)
    pending.add(k - lo)
    if k > lo:
      mag = np.abs(v.np['x'])
      for j in range(lo, k):
        mag = mag + alphas[j % m] * np.abs(ring_np[j % m, :n])
      entries('flush_x', dtype, host(x), want_x, mag, (k, in_x))
    else:
      assert np.array_equal(host(x), v.np['x']), (k, in_x)
    assert np.array_equal(host(lazy), want_lazy), (k, in_x)
    assert np.array_equal(host(ring), ring_np)
    assert np.array_equal(host(s), s0)
  assert pending == set(range(m))
  v.unchanged('z')


def _sum64_bound(values):
  return sum_bound(np.asarray(values, np.float64))


@both
@small
def test_mean_pair_three_iterations(n, dtype):
  """`update_r_mean`, `update_xp_mean` and the close (phase 1), three
  iterations in a row from `scalars[8]` = 0: both parities of `sums` are
  added to, read and cleared.  Every step is compared with the restatement
  applied to what the device held before it.

  c = w.r / total and -c 1.r are formed from sums of 64 slots taken in the
  kernel's own order: each within `sum_bound` of those 64 values (and two
  roundings)."""
  v = vectors(n, dtype, 60 + n, ('x', 'r', 'p', 'w'))
  d = v.dev
  total_w = float(v.np['w'].sum())
  s = to_dev(block(ITERS=0.0, CORR=0.0, MEAN=0.0, GAMMA_NEW=0.0,
                   STRIPES=0.0, ATOL2=0.0))
  sums = torch.zeros(CG.MEAN_SUMS, dtype=F64, device=DEV)
  rng = np.random.default_rng(n)
  T = NPT[dtype]
  for it in range(3):
    ap = to_dev(rng.standard_normal(n), dtype)
    s[CG.PAP] = 0.9 + it
    # ---- update_r_mean
    s0, sums0 = host(s), host(sums)
    r0, apn = host(d['r']), host(ap)
    assert int(s0[CG.ITERS]) == it
    _ops.cg_update_r_mean(d['r'], ap, d['w'], s, sums)
    want_r, _, _ = CG.update_r_mean(r0, apn, v.np['w'], s0, sums0, T)
    a = abs(CG.alpha_of(s0, T))
    got_r, got, got_sums = host(d['r']), host(s), host(sums)
    entries('update_r_mean', dtype, got_r, want_r,
            np.abs(r0) + a * np.abs(apn), it)
    one, wr = CG.mean_set(s0)
    summed('update_r_mean.rr', dtype, CG.total(got[CG.STRIPES]),
           s0[CG.STRIPES], got_r, got_r)
    summed('update_r_mean.1r', dtype, CG.total(got_sums[one]), sums0[one],
           got_r, np.ones(n))
    summed('update_r_mean.wr', dtype, CG.total(got_sums[wr]), sums0[wr],
           got_r, v.np['w'])
    same_but(got, s0, *STRIPE_IDX)
    same_but(got_sums, sums0, *range(one.start, wr.stop))
    # ---- update_xp_mean
    s0, sums0 = got, got_sums
    x0, p0 = host(d['x']), host(d['p'])
    _ops.cg_update_xp_mean(d['x'], d['p'], d['r'], s, sums, total_w)
    want_x, want_p, want_s, want_sums = CG.update_xp_mean(
        x0, p0, got_r, s0, sums0, total_w, T)
    c, corr = want_s[CG.MEAN], want_s[CG.CORR]
    beta = abs(CG.beta_of(s0, T, corr))
    entries('update_xp_mean', dtype, host(d['x']), want_x,
            np.abs(x0) + a * np.abs(p0), ('x', it))
    entries('update_xp_mean', dtype, host(d['p']), want_p,
            np.abs(got_r) + abs(c) + beta * np.abs(p0), ('p', it))
    got, got_sums = host(s), host(sums)
    c_bound = _sum64_bound(sums0[wr]) / abs(total_w) + 2 * np.spacing(abs(c))
    corr_bound = (abs(c) * _sum64_bound(sums0[one]) +
                  abs(sums0[one].sum()) * c_bound + 2 * np.spacing(abs(corr)))
    note('update_xp_mean.c', n, dtype, abs(got[CG.MEAN] - c), c_bound)
    note('update_xp_mean.corr', n, dtype, abs(got[CG.CORR] - corr), corr_bound)
    assert abs(got[CG.MEAN] - c) <= c_bound, (it, got[CG.MEAN], c)
    assert abs(got[CG.CORR] - corr) <= corr_bound, (it, got[CG.CORR], corr)
    same_but(got, s0, CG.MEAN, CG.CORR)
    assert np.array_equal(got_sums, want_sums), it       # other parity cleared
    assert not got_sums[(1 - it % 2) * 128:(2 - it % 2) * 128].any()
    assert np.array_equal(host(d['r']), got_r)
    # ---- the close picks [11] up and clears it, with the stripes
    _ops.cg_scalars(s, 1, 10 ** 9, 0.0, 0.0)
    want, _ = CG.scalar_phase(got, 1, 10 ** 9, 0.0, 0.0)
    _same_block(host(s), want, (it, 'close'))
    assert host(s)[CG.CORR] == 0.0 and not host(s)[CG.STRIPES].any()
    if host(s)[CG.DONE] != 0.0:
      # a handful of entries: r.z = r.r - c 1.r is 0 up to rounding at n = 1
      # (the projection leaves nothing) and can be negative for random r and
      # uneven weights; the solve stops, as the restatement says.  Go on as
      # a new one would
      assert n <= 7
      s[CG.DONE], s[CG.STATUS], s[CG.GAMMA] = 0.0, 0.0, 0.5
  v.unchanged('w')


def _period(n, ncomp):
  return n if ncomp == 1 else n + (-n) % 4


@pytest.mark.parametrize('ncomp', [1, 3])
@both
@small
def test_jacobi_pair(n, dtype, ncomp):
  """No layers; 3 components share dinv (the period is then a multiple of the
  16-byte vector width: n rounded up to one)."""
  period = _period(n, ncomp)
  v = vectors(period * ncomp, dtype, 70 + n, ('x', 'r', 'p', 'ap'))
  dinv = to_dev(0.5 + np.random.default_rng(n).random(period), dtype)
  dn, w, T = host(dinv), v.np, NPT[dtype]
  s0 = block()
  s = to_dev(s0)
  assert _ops.cg_update_r_jacobi(v.dev['r'], v.dev['ap'], dinv, s, ncomp) == 0
  want_r, _ = CG.update_r_jacobi(w['r'], w['ap'], dn, s0, T)
  a, beta = _alpha_beta(s0, dtype)
  got_r, got = host(v.dev['r']), host(s)
  entries('update_r_jacobi', dtype, got_r, want_r,
          np.abs(w['r']) + a * np.abs(w['ap']))
  # (r dinv) r: two roundings per term, within `sum_bound` ((m + 2) 2^-53)
  summed('update_r_jacobi.rz', dtype, CG.total(got[CG.STRIPES]),
         s0[CG.STRIPES], got_r.astype(np.longdouble) * np.tile(dn, ncomp),
         got_r)
  same_but(got, s0, *STRIPE_IDX)
  v.unchanged('ap')
  _ops.cg_update_xp_jacobi(v.dev['x'], v.dev['p'], v.dev['r'], dinv, s, ncomp)
  want_x, want_p = CG.update_xp_jacobi(w['x'], w['p'], got_r, dn, got, T)
  beta = abs(CG.beta_of(got, T))
  entries('update_xp_jacobi', dtype, host(v.dev['x']), want_x,
          np.abs(w['x']) + a * np.abs(w['p']), 'x')
  entries('update_xp_jacobi', dtype, host(v.dev['p']), want_p,
          np.tile(dn, ncomp) * np.abs(got_r) + beta * np.abs(w['p']), 'p')
  assert np.array_equal(host(s), got)
  assert np.array_equal(host(dinv), dn)
  assert np.array_equal(host(v.dev['r']), got_r)


CHEB_A, CHEB_C = 0.37, 1.9


def _cheb_magnitudes(w, mode):
  res = np.abs(w['b']) + np.abs(w['ax'])
  if mode == 2:
    return None, None, res
  if mode == 1:
    d = CHEB_C * w['dinv'] * np.abs(w['b'])
    return d, d, None
  d = CHEB_C * w['dinv'] * res + (CHEB_A * np.abs(w['d']) if mode == 0 else 0)
  return np.abs(w['x']) + d, d, None


@pytest.mark.parametrize('mode', [0, 1, 2, 3])
@both
@small
def test_cheb_step(n, dtype, mode):
  """What a mode does not read is full of NaN (1: x, d, ax; 3: d; 2 gets no
  x, d, dinv at all), what it does not write stays."""
  v = vectors(n, dtype, 80 + n, ('x', 'd', 'ax', 'b', 'dinv'))
  w, dev = v.np, v.dev
  x = nan_like(dev['x']) if mode == 1 else dev['x'].clone()
  d = nan_like(dev['d']) if mode in (1, 3) else dev['d'].clone()
  ax = nan_like(dev['ax']) if mode == 1 else dev['ax']
  r = nan_like(dev['b'])
  if mode == 2:
    _ops.cheb_step(None, None, ax, dev['b'], None, r, CHEB_A, CHEB_C, 2)
  else:
    _ops.cheb_step(x, d, ax, dev['b'], dev['dinv'], None, CHEB_A, CHEB_C, mode)
  want_x, want_d, want_r = CG.cheb_step(w['x'], w['d'], w['ax'], w['b'],
                                        w['dinv'], CHEB_A, CHEB_C, mode,
                                        NPT[dtype])
  mx, md, mr = _cheb_magnitudes(w, mode)
  if mode == 2:
    entries('cheb_step.2', dtype, host(r), want_r, mr)
  else:
    entries('cheb_step.%d' % mode, dtype, host(x), want_x, mx, 'x')
    entries('cheb_step.%d' % mode, dtype, host(d), want_d, md, 'd')
    assert np.isnan(host(r)).all()
  v.unchanged('b', 'dinv', *(() if mode == 1 else ('ax',)))


# --------------------------------------------------------------- 3. `done`
@both
def test_a_finished_solve_is_left_alone(dtype):
  """With `done` set every update kernel leaves every vector and every
  scalar bitwise as it was -- and reads nothing: the vectors it would only
  read are full of NaN."""
  n, m = 2049, 3
  out_names = ('x', 'r', 'p')
  v = vectors(n, dtype, 5, out_names)
  d = v.dev
  nan = torch.full((n,), float('nan'), dtype=dtype, device=DEV)
  ring_dev, ring_np = _ring(n, m, dtype, 6)
  lazy0 = np.concatenate([[3.0], 0.3 + 0.1 * np.arange(CG.LAZY_MAX)])
  sums0 = 1.0 + np.arange(CG.MEAN_SUMS)
  s0 = block(DONE=1.0, STATUS=1.0, OPEN=1.0)
  s, lazy, sums = to_dev(s0), to_dev(lazy0), to_dev(sums0)
  _ops.cg_update_xr(d['x'], d['r'], nan, nan, s, 0)
  _ops.cg_update_xr(d['x'], d['r'], nan, nan, s, 1)
  _ops.cg_update_p(d['p'], nan, s)
  for fuse in (0, 1, 2):
    _ops.cg_update_r(d['r'], nan, s, fuse)
  _ops.cg_update_xp(d['x'], d['p'], nan, s)
  _ops.cg_update_xp_lazy(d['x'], ring_dev, nan, s, lazy)
  _ops.cg_update_r_mean(d['r'], nan, nan, s, sums)
  _ops.cg_update_xp_mean(d['x'], d['p'], nan, s, sums, 3.0)
  _ops.cg_update_r_jacobi(d['r'], nan, nan, s)
  _ops.cg_update_xp_jacobi(d['x'], d['p'], nan, nan, s)
  assert np.array_equal(host(s), s0)
  assert np.array_equal(host(lazy), lazy0)
  assert np.array_equal(host(sums), sums0)
  assert np.array_equal(host(ring_dev), ring_np)
  v.unchanged(*out_names)
  # the restatement says the same
  w = v.np
  T = NPT[dtype]
  assert CG.update_xr(w['x'], w['r'], None, None, s0, T)[0] is w['x']
  assert CG.update_xp(w['x'], w['p'], None, s0, T)[1] is w['p']
  assert CG.update_xp_lazy(w['x'], ring_np, None, s0, lazy0, T)[2] is lazy0


# ------------------------------------------------------ 4. the scalar phases
def dyadic(count, seed=0):
  """`count` non-zero multiples of 1 / 128 below 1 in magnitude: their sum is
  exact in double precision in any order, and dropping or repeating any one
  of them changes it."""
  i = np.arange(count, dtype=np.int64) + seed
  return ((i * 37) % 101 - 50.5) / 64.0


def _same_block(got, want, what, quotients=(CG.ALPHA, CG.BETA)):
  """Bitwise, but for the two quotients: within one spacing."""
  exact = np.ones(NS, dtype=bool)
  exact[list(quotients)] = False
  assert np.array_equal(got[exact], want[exact], equal_nan=True), \
      (what, np.flatnonzero(~((got == want) | ~exact)), got, want)
  for q in quotients:
    if np.isfinite(want[q]):
      assert abs(got[q] - want[q]) <= np.spacing(abs(want[q])), (what, q)
    else:
      assert np.array_equal(got[q], want[q], equal_nan=True), (what, q)


_G = 2.03125 + 0.25       # stripes of `block` + GAMMA_NEW = 0.25, CORR = 0
NAN, INF = float('nan'), float('inf')
# (name, phase, slots, partials, maxiter, tol, atol, status afterwards).
# partials: None, 'sum' (DOT_SLOTS dyadic values), or a list that is padded
# with zeros.
PHASE_TABLE = [
    ('start', 2, dict(BB=2.0, GAMMA=1.5), None, 10, 1e-5, 0.0, 'running'),
    ('start clears partials', 2, dict(BB=2.0, GAMMA=1.5), 'sum', 10, 1e-5,
     0.0, 'running'),
    ('start after a finished solve', 2,
     dict(BB=2.0, GAMMA=1.5, DONE=1.0, STATUS=2.0, OPEN=1.0), None, 10, 1e-5,
     0.0, 'running'),
    ('start converged', 2, dict(BB=1.0, GAMMA=1e-12), None, 10, 1e-5, 0.0,
     'converged'),
    ('start gamma0 = atol2', 2, dict(BB=1.0, GAMMA=0.25), None, 10, 0.5, 0.0,
     'converged'),
    ('start b = 0', 2, dict(BB=0.0, GAMMA=0.0), None, 10, 1e-5, 0.0,
     'converged'),
    ('start gamma0 < 0', 2, dict(BB=1.0, GAMMA=-1.0), None, 10, 1e-5, 0.0,
     'breakdown_gamma'),
    ('start gamma0 nan', 2, dict(BB=1.0, GAMMA=NAN), None, 10, 1e-5, 0.0,
     'breakdown_gamma'),
    ('start gamma0 inf', 2, dict(BB=1.0, GAMMA=INF), None, 10, 1e-5, 0.0,
     'breakdown_gamma'),
    ('start maxiter 0', 2, dict(BB=1.0, GAMMA=1.0), None, 0, 1e-5, 0.0,
     'maxiter'),
    ('start maxiter < 0', 2, dict(BB=1.0, GAMMA=1.0), None, -3, 1e-5, 0.0,
     'maxiter'),
    ('start atol wins', 2, dict(BB=1.0, GAMMA=5e-5), None, 10, 1e-5, 1e-2,
     'converged'),
    ('start tol alone', 2, dict(BB=1.0, GAMMA=5e-5), None, 10, 1e-5, 0.0,
     'running'),
    ('alpha', 0, dict(PAP=0.7), None, 10, 1e-5, 0.0, 'running'),
    ('alpha keeps partials', 0, dict(PAP=0.7), 'sum', 10, 1e-5, 0.0,
     'running'),
    ('alpha p.Ap < 0', 0, dict(PAP=-0.7), None, 10, 1e-5, 0.0, 'running'),
    ('alpha p.Ap = 0', 0, dict(PAP=0.0), None, 10, 1e-5, 0.0,
     'breakdown_pAp'),
    ('alpha p.Ap nan', 0, dict(PAP=NAN), None, 10, 1e-5, 0.0,
     'breakdown_pAp'),
    ('alpha p.Ap +inf', 0, dict(PAP=INF), None, 10, 1e-5, 0.0,
     'breakdown_pAp'),
    ('alpha p.Ap -inf', 0, dict(PAP=-INF), None, 10, 1e-5, 0.0,
     'breakdown_pAp'),
    ('close and go on', 1, dict(), None, 10, 1e-5, 0.0, 'running'),
    ('close clears partials', 1, dict(), 'sum', 10, 1e-5, 0.0, 'running'),
    ('close gamma_new < 0', 1, dict(GAMMA_NEW=-5.0), None, 10, 1e-5, 0.0,
     'breakdown_gamma'),
    ('close gamma_new < 0 by [11]', 1, dict(CORR=-5.0), None, 10, 1e-5, 0.0,
     'breakdown_gamma'),
    ('close gamma_new nan', 1, dict(GAMMA_NEW=NAN), None, 10, 1e-5, 0.0,
     'breakdown_gamma'),
    ('close gamma_new inf', 1, dict(GAMMA_NEW=INF), None, 10, 1e-5, 0.0,
     'breakdown_gamma'),
    ('close inf in a stripe', 1, dict(STRIPES=INF), None, 10, 1e-5, 0.0,
     'breakdown_gamma'),
    ('close gamma = atol2', 1, dict(GAMMA_NEW=0.25, CORR=0.0, ATOL2=_G), None,
     10, 1e-5, 0.0, 'converged'),
    ('close gamma just above atol2', 1,
     dict(GAMMA_NEW=0.25, CORR=0.0, ATOL2=_G - 2.0 ** -40), None, 10, 1e-5,
     0.0, 'running'),
    ('close converged', 1, dict(ATOL2=100.0), None, 10, 1e-5, 0.0,
     'converged'),
    ('close maxiter', 1, dict(ITERS=9.0), None, 10, 1e-5, 0.0, 'maxiter'),
    ('close one before maxiter', 1, dict(ITERS=8.0), None, 10, 1e-5, 0.0,
     'running'),
    ('p.Ap from partials', 3, dict(), 'sum', 10, 1e-5, 0.0, 'running'),
    ('p.Ap from partials, nan', 3, dict(), [1.0, NAN], 10, 1e-5, 0.0,
     'running'),
    ('p.Ap and alpha', 4, dict(), 'sum', 10, 1e-5, 0.0, 'running'),
    ('p.Ap and alpha, < 0', 4, dict(), [-0.75, 0.25], 10, 1e-5, 0.0,
     'running'),
    ('p.Ap and alpha, 0', 4, dict(), [0.75, -0.75], 10, 1e-5, 0.0,
     'breakdown_pAp'),
    ('p.Ap and alpha, nan', 4, dict(), [0.75, NAN], 10, 1e-5, 0.0,
     'breakdown_pAp'),
    ('p.Ap and alpha, +inf', 4, dict(), [0.75, INF], 10, 1e-5, 0.0,
     'breakdown_pAp'),
    ('p.Ap and alpha, -inf', 4, dict(), [0.75, -INF], 10, 1e-5, 0.0,
     'breakdown_pAp'),
    ('deferred, nothing open', 5, dict(), 'sum', 10, 1e-5, 0.0, 'running'),
    ('deferred, closes and goes on', 5, dict(OPEN=1.0), 'sum', 10, 1e-5, 0.0,
     'running'),
    ('deferred, the close converges', 5, dict(OPEN=1.0, ATOL2=100.0), 'sum',
     10, 1e-5, 0.0, 'converged'),
    ('deferred, the close hits maxiter', 5, dict(OPEN=1.0, ITERS=9.0), 'sum',
     10, 1e-5, 0.0, 'maxiter'),
    ('deferred, the close finds gamma_new < 0', 5,
     dict(OPEN=1.0, GAMMA_NEW=-5.0), 'sum', 10, 1e-5, 0.0, 'breakdown_gamma'),
    ('deferred, p.Ap = 0', 5, dict(), [0.75, -0.75], 10, 1e-5, 0.0,
     'breakdown_pAp'),
    ('deferred, closes, then p.Ap nan', 5, dict(OPEN=1.0), [0.75, NAN], 10,
     1e-5, 0.0, 'breakdown_pAp'),
    ('look, open', 6, dict(OPEN=1.0), None, 10, 1e-5, 0.0, 'running'),
    ('look, open, converges', 6, dict(OPEN=1.0, ATOL2=100.0), None, 10, 1e-5,
     0.0, 'converged'),
    ('look, nothing open', 6, dict(), None, 10, 1e-5, 0.0, 'running'),
    ('look keeps partials', 6, dict(OPEN=1.0), 'sum', 10, 1e-5, 0.0,
     'running'),
    ('fold the stripes', 7, dict(), None, 10, 1e-5, 0.0, 'running'),
]


def _table_partials(spec):
  if spec is None:
    return None
  if isinstance(spec, str):
    return dyadic(CG.DOT_SLOTS)
  p = np.zeros(CG.DOT_SLOTS)
  p[[3, 700][:len(spec)]] = spec
  return p


def test_the_table_reaches_every_status_and_phase():
  assert {row[-1] for row in PHASE_TABLE} == set(_lib.CG_STATUS.values())
  assert all(CG.STATUS_CODE[name] == code
             for code, name in _lib.CG_STATUS.items())
  assert {row[1] for row in PHASE_TABLE} == set(range(8))


@pytest.mark.parametrize('row', PHASE_TABLE, ids=[r[0] for r in PHASE_TABLE])
def test_scalar_phase(row):
  name, phase, slots, spec, maxiter, tol, atol, status = row
  s0, p0 = block(**slots), _table_partials(spec)
  want, want_p = CG.scalar_phase(s0, phase, maxiter, tol, atol, p0)
  assert want[CG.STATUS] == CG.STATUS_CODE[status]
  assert want[CG.DONE] == float(status != 'running')
  s = to_dev(s0)
  parts = None if p0 is None else to_dev(p0)
  _ops.cg_scalars(s, phase, maxiter, tol, atol, parts)
  got = host(s)
  _same_block(got, want, name)
  if p0 is not None:
    assert np.array_equal(host(parts), want_p, equal_nan=True)
    assert want_p.any() == (phase in (0, 3, 4, 6))
  if status == 'breakdown_pAp':          # nothing else moves (but [1] = sum)
    same_but(got, s0, CG.DONE, CG.STATUS, CG.PAP,
             *((CG.OPEN, CG.GAMMA, CG.BETA, CG.ITERS, CG.CORR, *STRIPE_IDX)
               if slots.get('OPEN') else ()))
  if name == 'close and go on':
    g = 0.75 + 2.03125 + s0[CG.CORR]
    assert got[CG.GAMMA] == g and got[CG.ITERS] == 4.0
    assert abs(got[CG.BETA] - g / s0[CG.GAMMA]) <= 1e-15
    assert got[CG.CORR] == 0.0 and got[CG.PAP] == 0.0
    assert not got[CG.STRIPES].any()
  if name == 'fold the stripes':
    assert got[CG.GAMMA_NEW] == 0.75 + 2.03125 and not got[CG.STRIPES].any()
    same_but(got, s0, CG.GAMMA_NEW, *STRIPE_IDX)
  if name == 'deferred, the close converges':   # no alpha, not reopened
    assert got[CG.ALPHA] == s0[CG.ALPHA] and got[CG.OPEN] == 0.0
    assert got[CG.PAP] == s0[CG.PAP] and got[CG.GAMMA_NEW] == s0[CG.GAMMA_NEW]


STORED_COUNTS = (1, 255, 257, 4096, 4097, 70001)


def _stored(count, values):
  """`count` stored sums and the scratch behind them, full of NaN."""
  buf = np.full(count + CG.FOLD_GROUPS, NAN)
  buf[:count] = values
  return buf


def _stored_untouched(parts, buf, count):
  got = host(parts)
  assert np.array_equal(got[:count], buf[:count], equal_nan=True)
  if count <= 4096:                      # one stage: the scratch is not used
    assert np.isnan(got[count:]).all()


@pytest.mark.parametrize('phase,slots', [
    (3, dict()), (4, dict()), (5, dict()), (5, dict(OPEN=1.0)), (8, dict())],
    ids=['3', '4', '5', '5-open', '8'])
@pytest.mark.parametrize('count', STORED_COUNTS)
def test_scalar_phase_over_stored_partials(count, phase, slots):
  """`sfem_cg_scalars_n`: 4097 and 70001 sums go through
  `fold_partials_kernel` first.  Dyadic sums: the block bitwise (any sum
  dropped or taken twice shows); random sums: [1] / [2] within `sum_bound`
  and alpha to match."""
  s0 = block(**slots)
  buf = _stored(count, dyadic(count, seed=count))
  s, parts = to_dev(s0), to_dev(buf)
  _ops.cg_scalars_n(s, phase, *ARGS, parts, count)
  want, want_p = CG.scalar_phase(s0, phase, *ARGS, buf[:count], stored=True)
  assert np.array_equal(want_p, buf[:count])
  _same_block(host(s), want, (count, phase))
  _stored_untouched(parts, buf, count)
  # random values
  values = np.random.default_rng(count).standard_normal(count)
  buf = _stored(count, values)
  s, parts = to_dev(s0), to_dev(buf)
  _ops.cg_scalars_n(s, phase, *ARGS, parts, count)
  want, _ = CG.scalar_phase(s0, phase, *ARGS, values, stored=True)
  got = host(s)
  slot = CG.GAMMA_NEW if phase == 8 else CG.PAP
  bound = sum_bound(values)
  note('cg_scalars_n.%d' % phase, count, 'fp64', abs(got[slot] - want[slot]),
       bound)
  assert abs(got[slot] - want[slot]) <= bound
  if phase in (4, 5):        # alpha = gamma / p.Ap of the device's own sum
    assert abs(got[CG.ALPHA] - want[CG.GAMMA] / got[CG.PAP]) <= \
        np.spacing(abs(got[CG.ALPHA]))
    same_but(got, want, slot, CG.ALPHA, CG.BETA)
  else:
    same_but(got, want, slot)
  _stored_untouched(parts, buf, count)


def test_unstored_phase_5_zeroes_its_partials():
  p0 = np.random.default_rng(1).standard_normal(CG.DOT_SLOTS + 8)
  s0 = block(OPEN=1.0)
  s, parts = to_dev(s0), to_dev(p0)
  _ops.cg_scalars(s, 5, *ARGS, parts)
  got, got_p = host(s), host(parts)
  assert not got_p[:CG.DOT_SLOTS].any()
  assert np.array_equal(got_p[CG.DOT_SLOTS:], p0[CG.DOT_SLOTS:])
  want, _ = CG.scalar_phase(s0, 5, *ARGS, p0[:CG.DOT_SLOTS])
  bound = sum_bound(p0[:CG.DOT_SLOTS])
  note('cg_scalars.5', CG.DOT_SLOTS, 'fp64', abs(got[CG.PAP] - want[CG.PAP]),
       bound)
  assert abs(got[CG.PAP] - want[CG.PAP]) <= bound
  same_but(got, want, CG.PAP, CG.ALPHA, CG.BETA)
  assert abs(got[CG.ALPHA] - want[CG.GAMMA] / got[CG.PAP]) <= \
      np.spacing(abs(got[CG.ALPHA]))


def test_done_freezes_the_scalars():
  """Every phase but 2 leaves a finished solve's block alone.  Accumulated
  partials are workspace: phases 1 and 5 still clear them (the apply that ran
  ahead of the flag has added to them), stored ones are never written."""
  s0 = block(DONE=1.0, STATUS=1.0, OPEN=1.0)
  p0 = dyadic(CG.DOT_SLOTS)
  for phase in (0, 1, 3, 4, 5, 6, 7):
    for spec in (None, p0):
      if spec is None and phase in (3, 4, 5):
        continue
      s = to_dev(s0)
      parts = None if spec is None else to_dev(spec)
      _ops.cg_scalars(s, phase, *ARGS, parts)
      assert np.array_equal(host(s), s0), phase
      if spec is not None:
        _, want_p = CG.scalar_phase(s0, phase, *ARGS, spec)
        assert np.array_equal(host(parts), want_p), phase
        assert want_p.any() == (phase not in (1, 5))
  for count in (257, 4097):
    buf = _stored(count, dyadic(count))
    for phase in (3, 4, 5, 8):
      s, parts = to_dev(s0), to_dev(buf)
      _ops.cg_scalars_n(s, phase, *ARGS, parts, count)
      assert np.array_equal(host(s), s0), (count, phase)
      _stored_untouched(parts, buf, count)


def test_scalar_entry_point_refusals():
  lib = _lib.load()
  s0 = block()
  s = to_dev(s0)
  p0 = dyadic(CG.DOT_SLOTS + CG.FOLD_GROUPS)
  parts = to_dev(p0)
  sp, pp = s.data_ptr(), parts.data_ptr()
  OK, EINVAL = 0, -1

  def plain(phase, scal=sp, partials=None):
    return lib.sfem_cg_scalars(scal, phase, 10.0, 1e-5, 0.0, partials, None)

  def stored(phase, count=4, scal=sp, partials=pp):
    return lib.sfem_cg_scalars_n(scal, phase, 10.0, 1e-5, 0.0, partials,
                                 count, None)

  for phase in (-1, 8, 9, 100):
    assert plain(phase) == EINVAL and plain(phase, partials=pp) == EINVAL
  for phase in (3, 4, 5):
    assert plain(phase) == EINVAL
  assert plain(0, scal=None) == EINVAL
  for phase in (-1, 0, 1, 2, 6, 7, 9):
    assert stored(phase) == EINVAL
  for phase in (3, 4, 5, 8):
    assert stored(phase, count=0) == EINVAL
    assert stored(phase, count=-1) == EINVAL
    assert stored(phase, partials=None) == EINVAL
    assert stored(phase, scal=None) == EINVAL
  torch.cuda.synchronize()
  assert np.array_equal(host(s), s0) and np.array_equal(host(parts), p0)
  assert plain(7) == OK and stored(3) == OK
  assert host(s)[CG.PAP] == p0[:4].sum()


# -------------------------------------------------- 5. CG that stops on r.r
@pytest.mark.parametrize('with_c', [False, True], ids=['ab', 'ab_ac'])
@pytest.mark.parametrize('groups', [1, 3, 256])
@both
@small
def test_pmg_dot2(n, dtype, groups, with_c):
  """Stored, never accumulated: `partials` starts full of NaN."""
  v = vectors(n, dtype, 90 + n, ('a', 'b', 'c'))
  parts = torch.full((2 * groups + 5,), NAN, dtype=F64, device=DEV)
  c = v.dev['c'] if with_c else None
  _ops.pmg_dot2(v.dev['a'], v.dev['b'], c, parts, groups)
  got = host(parts)
  written = (2 if with_c else 1) * groups
  assert np.isfinite(got[:written]).all() and np.isnan(got[written:]).all()
  summed('pmg_dot2', dtype, CG.total(got[:groups]), 0.0, v.np['a'], v.np['b'])
  if with_c:
    summed('pmg_dot2', dtype, CG.total(got[groups:written]), 0.0, v.np['a'],
           v.np['c'])
  again = nan_like(parts)
  _ops.pmg_dot2(v.dev['a'], v.dev['b'], c, again, groups)
  assert np.array_equal(host(again), got, equal_nan=True)
  v.unchanged('a', 'b', 'c')


PMG_COUNTS = (1, 255, 257, 3 * 256 + 1)
# (name, phase, slots, first, second, maxiter, tol, atol, status): `first` /
# `second` are None (dyadic sums) or the value the n sums add up to.
PMG_TABLE = [
    ('b.b', 3, dict(), None, None, 10, 1e-5, 0.0, 'running'),
    ('b.b of a finished solve', 3, dict(DONE=1.0, STATUS=1.0), None, None, 10,
     1e-5, 0.0, 'converged'),
    ('start', 2, dict(BB=2.0), 1.5, 1.25, 10, 1e-5, 0.0, 'running'),
    ('start after a finished solve', 2,
     dict(BB=2.0, DONE=1.0, STATUS=2.0, OPEN=1.0), 1.5, 1.25, 10, 1e-5, 0.0,
     'running'),
    ('start converged on r.r', 2, dict(BB=1.0), 2.0 ** -40, 1.25, 10, 1e-5,
     0.0, 'converged'),
    ('start r.r = atol2', 2, dict(BB=1.0), 0.25, 1.25, 10, 0.5, 0.0,
     'converged'),
    ('start r.z small, r.r not', 2, dict(BB=1.0), 1.5, 2.0 ** -40, 10, 1e-5,
     0.0, 'running'),
    ('start r.z < 0', 2, dict(BB=1.0), 1.5, -1.25, 10, 1e-5, 0.0,
     'breakdown_gamma'),
    ('start r.z nan', 2, dict(BB=1.0), 1.5, NAN, 10, 1e-5, 0.0,
     'breakdown_gamma'),
    ('start r.z inf', 2, dict(BB=1.0), 1.5, INF, 10, 1e-5, 0.0,
     'breakdown_gamma'),
    ('start maxiter 0', 2, dict(BB=1.0), 1.5, 1.25, 0, 1e-5, 0.0, 'maxiter'),
    ('start atol wins', 2, dict(BB=1.0), 2.0 ** -14, 1.25, 10, 1e-5, 1e-2,
     'converged'),
    ('start tol alone', 2, dict(BB=1.0), 2.0 ** -14, 1.25, 10, 1e-5, 0.0,
     'running'),
    ('alpha', 0, dict(), None, None, 10, 1e-5, 0.0, 'running'),
    ('alpha p.Ap < 0', 0, dict(), -0.75, None, 10, 1e-5, 0.0, 'running'),
    ('alpha p.Ap = 0', 0, dict(), 0.0, None, 10, 1e-5, 0.0, 'breakdown_pAp'),
    ('alpha p.Ap nan', 0, dict(), NAN, None, 10, 1e-5, 0.0, 'breakdown_pAp'),
    ('alpha p.Ap +inf', 0, dict(), INF, None, 10, 1e-5, 0.0, 'breakdown_pAp'),
    ('alpha p.Ap -inf', 0, dict(), -INF, None, 10, 1e-5, 0.0,
     'breakdown_pAp'),
    ('alpha of a finished solve', 0, dict(DONE=1.0, STATUS=1.0), None, None,
     10, 1e-5, 0.0, 'converged'),
    ('r.r and r.z', 4, dict(), None, None, 10, 1e-5, 0.0, 'running'),
    ('r.r and r.z of a finished solve', 4, dict(DONE=1.0, STATUS=2.0), None,
     None, 10, 1e-5, 0.0, 'maxiter'),
    ('close and go on', 1, dict(RR=1.0), None, None, 10, 1e-5, 0.0,
     'running'),
    ('close converged on r.r', 1, dict(RR=0.125, ATOL2=0.25), None, None, 10,
     1e-5, 0.0, 'converged'),
    ('close r.r = atol2', 1, dict(RR=0.25, ATOL2=0.25), None, None, 10, 1e-5,
     0.0, 'converged'),
    ('close r.z small, r.r not', 1, dict(RR=1.0, GAMMA_NEW=2.0 ** -40), None,
     None, 10, 1e-5, 0.0, 'running'),
    ('close r.z < 0', 1, dict(RR=1.0, GAMMA_NEW=-1.0), None, None, 10, 1e-5,
     0.0, 'breakdown_gamma'),
    ('close r.z nan', 1, dict(RR=1.0, GAMMA_NEW=NAN), None, None, 10, 1e-5,
     0.0, 'breakdown_gamma'),
    ('close r.z inf', 1, dict(RR=1.0, GAMMA_NEW=INF), None, None, 10, 1e-5,
     0.0, 'breakdown_gamma'),
    ('close maxiter', 1, dict(RR=1.0, ITERS=9.0), None, None, 10, 1e-5, 0.0,
     'maxiter'),
    ('close of a finished solve', 1, dict(RR=1.0, DONE=1.0, STATUS=3.0), None,
     None, 10, 1e-5, 0.0, 'breakdown_pAp'),
]


def _pmg_partials(n, first, second):
  """2 n stored sums and 5 NaN behind them; a prescribed total sits in one
  entry of an otherwise cancelling (or empty) list."""
  p = np.full(2 * n + 5, NAN)
  for half, value in enumerate((first, second)):
    vals = dyadic(n, seed=half * 7)
    if value is not None:
      vals = np.zeros(n)
      if n > 2:
        vals[0], vals[n - 1] = 0.5, -0.5
      vals[n // 2] = value
    p[half * n:(half + 1) * n] = vals
  return p


def test_the_pmg_table_reaches_every_status_and_phase():
  assert {row[-1] for row in PMG_TABLE} == set(_lib.CG_STATUS.values())
  assert {row[1] for row in PMG_TABLE} == set(range(5))


@pytest.mark.parametrize('n', PMG_COUNTS)
@pytest.mark.parametrize('row', PMG_TABLE, ids=[r[0] for r in PMG_TABLE])
def test_pmg_scalar_phase(row, n):
  name, phase, slots, first, second, maxiter, tol, atol, status = row
  s0 = block(**slots)
  p0 = _pmg_partials(n, first, second)
  want = CG.pmg_scalar_phase(s0, phase, p0, n, maxiter, tol, atol)
  assert want[CG.STATUS] == CG.STATUS_CODE[status]
  assert want[CG.DONE] == float(status != 'running')
  s, parts = to_dev(s0), to_dev(p0)
  _ops.pmg_cg_scalars(s, phase, parts, n, maxiter, tol, atol)
  got = host(s)
  _same_block(got, want, (name, n))
  assert np.array_equal(host(parts), p0, equal_nan=True)
  if slots.get('DONE') and phase != 2:
    same_but(got, s0, *((CG.BB,) if phase == 3 else ()))
  if status == 'breakdown_pAp' and not slots.get('DONE'):
    same_but(got, s0, CG.DONE, CG.STATUS, CG.PAP)
  if name == 'close and go on':      # stripes and [11] are not this CG's
    same_but(got, s0, CG.BETA, CG.GAMMA, CG.PAP, CG.ITERS)
    assert got[CG.GAMMA] == s0[CG.GAMMA_NEW]


def test_pmg_scalar_sums_are_bounded():
  """Random stored sums: within `sum_bound`, the same bits on a second call."""
  n = 3 * 256 + 1
  values = np.random.default_rng(2).standard_normal(2 * n)
  s0 = block()
  out = []
  for _ in range(2):
    s = to_dev(s0)
    _ops.pmg_cg_scalars(s, 4, to_dev(values), n, *ARGS)
    out.append(host(s))
  assert np.array_equal(out[0], out[1])
  for slot, part in ((CG.RR, values[:n]), (CG.GAMMA_NEW, values[n:])):
    err = abs(out[0][slot] - CG.total(part))
    note('pmg_cg_scalars.4', n, 'fp64', err, sum_bound(part))
    assert err <= sum_bound(part)
  same_but(out[0], s0, CG.RR, CG.GAMMA_NEW)


# ------------------------------------------------- 6. one chained solve
def _dense_spd(n, dtype):
  """2 I + Q Q^T / (2 n): eigenvalues in [2, 4), condition number below 2.
  The matrix is held in float64 on both sides (the apply is torch's, in
  float64, rounded to the vectors' type once)."""
  g = torch.Generator(device='cpu').manual_seed(n)
  q = torch.randn(n, n, generator=g, dtype=F64)
  a = 2.0 * torch.eye(n, dtype=F64) + q @ q.T / (2 * n)
  b = torch.randn(n, generator=g, dtype=F64).to(dtype)
  return a, b


def _solve_by_kernels(a_dev, b, schedule, maxiter, tol):
  dtype = b.dtype
  A = lambda v: (a_dev @ v.double()).to(dtype)
  n = b.numel()
  x, r, p = torch.zeros_like(b), b.clone(), b.clone()
  s = torch.zeros(NS, dtype=F64, device=DEV)
  parts = torch.zeros(CG.DOT_SLOTS, dtype=F64, device=DEV)
  args = (maxiter, tol, 0.0)
  _ops.dot(b, b, s, CG.BB)
  _ops.dot(r, r, s, CG.GAMMA)
  _ops.cg_scalars(s, 2, *args, parts)
  for _ in range(maxiter + 2):
    if float(s[CG.DONE]) != 0.0:
      break
    ap = A(p)
    if schedule == 'deferred':
      _ops.dot(p, ap, parts, n % CG.DOT_SLOTS, accumulate=True)
      _ops.cg_scalars(s, 5, *args, parts)
    else:
      _ops.dot(p, ap, s, CG.PAP, accumulate=True)
      _ops.cg_scalars(s, 0, *args)
    if schedule == 'nine':
      _ops.cg_update_xr(x, r, p, ap, s, 0)
      _ops.dot(r, r, s, CG.GAMMA_NEW, accumulate=True)
      _ops.cg_update_p(p, r, s)
    else:
      _ops.cg_update_r(r, ap, s, 2)
      _ops.cg_update_xp(x, p, r, s)
    if schedule != 'deferred':
      _ops.cg_scalars(s, 1, *args)
  if schedule == 'deferred':
    _ops.cg_scalars(s, 6, *args)
  return x, host(s)


@pytest.mark.parametrize('schedule', CG.SCHEDULES)
@both
def test_chained_solve(dtype, schedule):
  """2049 unknowns, dense, condition number below 2: the kernels chained in
  the three orders of `linalg/cg.py` take the iteration count of
  `cg_by_pieces` and give its x to (iterations) x the entry bound.  A dense
  operator spreads every entry's rounding over all others, so the magnitude
  of the bound is the largest entry's: 8 eps sum_k max |x_k - x_{k-1}|."""
  n = 2049
  a, b = _dense_spd(n, dtype)
  tol = 1e-10 if dtype == F64 else 1e-5
  an, bn = a.numpy(), b.double().numpy()
  want, iterates, status, iters = CG.cg_by_pieces(
      lambda v: an @ v, bn, tol=tol, schedule=schedule, dtype=NPT[dtype])
  assert status == 'converged' and 5 <= iters <= 30
  x, s = _solve_by_kernels(a.to(DEV), b.to(DEV), schedule, 10 * n, tol)
  assert s[CG.STATUS] == CG.STATUS_CODE['converged'] and s[CG.DONE] == 1.0
  assert int(s[CG.ITERS]) == iters
  steps = [np.abs(cur - prev).max()
           for prev, cur in zip([0.0 * want] + iterates, iterates)]
  bound = iters * 8.0 * EPS[dtype] * float(np.sum(steps))
  err = float(np.abs(host(x) - want).max())
  note('chained.' + schedule, n, dtype, err, bound)
  assert err <= bound, (err, bound, iters)


# ------------------------------------ 7. the second trip of the reduce grid
def randn(n, dtype, gen):
  return torch.randn(n, dtype=dtype, device=DEV, generator=gen)


def dev_sum(kernel, dtype, got, start, a, b, n):
  """got = start + a.b (float64 device tensors a, b) within twice
  `sum_bound`: the reference sum is torch's, in float64."""
  prod = a * b
  want, mag = (float(t) for t in
               torch.stack([prod.sum(), prod.abs().sum()]).tolist())
  bound = 2.0 * (n + 2) * 2.0 ** -52 * (mag + abs(start))
  note(kernel, n, dtype, abs(got - (start + want)), bound)
  assert abs(got - (start + want)) <= bound, (kernel, got, start + want, bound)


def dev_entries(kernel, dtype, got, want, magnitude, what=''):
  """`check_entries`' rule on the device; one transfer, two temporaries."""
  err = got.to(F64, copy=True).sub_(want).abs_()
  limit = magnitude * (8.0 * EPS[dtype])
  nbad = (~(err <= limit)).sum().double()
  ratio = err.div_(limit).nan_to_num_(nan=0.0)         # (0 / 0: no error)
  nbad, worst = torch.stack([nbad, ratio.max()]).tolist()
  note(kernel, got.numel(), dtype, worst, 1.0)
  assert nbad == 0, (kernel, what, int(nbad), worst)


@both
def test_reduce_grid_second_trip(dtype):
  n = MIDDLE
  assert n > 4096 * 512 * (16 // dtype.itemsize)
  gen = torch.Generator(device=DEV).manual_seed(11)
  a, b = randn(n, dtype, gen), randn(n, dtype, gen)
  s0 = block()
  alpha = CG.alpha_of(s0, NPT[dtype])
  s = to_dev(s0)
  _ops.dot(a, b, s, CG.PAP)
  _ops.dot(a, b, s, CG.GAMMA_NEW, accumulate=True)
  got = host(s)
  dev_sum('dot', dtype, got[CG.PAP], 0.0, a.double(), b.double(), n)
  dev_sum('dot_accumulate', dtype, got[CG.GAMMA_NEW], s0[CG.GAMMA_NEW],
          a.double(), b.double(), n)
  same_but(got, s0, CG.PAP, CG.GAMMA_NEW)
  for fuse in (0, 1):
    x, r = randn(n, dtype, gen), randn(n, dtype, gen)
    want_x = x.double() + alpha * a.double()
    mag_x = x.double().abs() + abs(alpha) * a.double().abs()
    want_r = r.double() - alpha * b.double()
    mag_r = r.double().abs() + abs(alpha) * b.double().abs()
    r2 = r.clone()
    s = to_dev(s0)
    _ops.cg_update_xr(x, r, a, b, s, fuse)
    dev_entries('update_xr', dtype, x, want_x, mag_x, 'x')
    dev_entries('update_xr', dtype, r, want_r, mag_r, 'r')
    got = host(s)
    if fuse:
      dev_sum('update_xr.rr', dtype, got[CG.GAMMA_NEW], s0[CG.GAMMA_NEW],
              r.double(), r.double(), n)
      same_but(got, s0, CG.GAMMA_NEW)
    else:
      assert np.array_equal(got, s0)
    s = to_dev(s0)
    _ops.cg_update_r(r2, b, s, fuse)
    dev_entries('update_r', dtype, r2, want_r, mag_r, fuse)
    got = host(s)
    if fuse:
      dev_sum('update_r.rr', dtype, got[CG.GAMMA_NEW], s0[CG.GAMMA_NEW],
              r2.double(), r2.double(), n)
      same_but(got, s0, CG.GAMMA_NEW)
    else:
      assert np.array_equal(got, s0)


# ------------------------- 8. past 256 MiB: non-temporal, second stream trip
@pytest.fixture
def large(request):
  """(n, generator) for one large item; what the item allocated goes back to
  the device afterwards."""
  dtype = request.node.callspec.params['dtype']
  n = LARGE[dtype]
  assert n * dtype.itemsize >= 256 << 20            # streams_past_caches
  assert n > 32768 * 512 * (16 // dtype.itemsize)   # stream_grid: second trip
  yield n, torch.Generator(device=DEV).manual_seed(n % 1000)
  torch.cuda.empty_cache()


@both
def test_large_update_r(dtype, large):
  n, gen = large
  ap, r0 = randn(n, dtype, gen), randn(n, dtype, gen)
  s0 = block()
  alpha = CG.alpha_of(s0, NPT[dtype])
  want = r0.double() - alpha * ap.double()
  mag = r0.double().abs() + abs(alpha) * ap.double().abs()
  for fuse in (0, 1, 2):
    r = r0.clone()
    s = to_dev(s0)
    _ops.cg_update_r(r, ap, s, fuse)
    dev_entries('update_r', dtype, r, want, mag, fuse)
    got = host(s)
    if fuse == 0:
      assert np.array_equal(got, s0)
    elif fuse == 1:
      dev_sum('update_r.rr', dtype, got[CG.GAMMA_NEW], s0[CG.GAMMA_NEW],
              r.double(), r.double(), n)
      same_but(got, s0, CG.GAMMA_NEW)
    else:
      dev_sum('update_r.rr_striped', dtype, CG.total(got[CG.STRIPES]),
              CG.total(s0[CG.STRIPES]), r.double(), r.double(), n)
      same_but(got, s0, *STRIPE_IDX)
      assert (got[CG.STRIPES] != s0[CG.STRIPES]).all()
    del r


@both
def test_large_update_xp_and_p(dtype, large):
  n, gen = large
  x, p0, z = (randn(n, dtype, gen) for _ in range(3))
  s0 = block()
  T = NPT[dtype]
  alpha, beta = CG.alpha_of(s0, T), CG.beta_of(s0, T)
  s = to_dev(s0)
  want_x = x.double() + alpha * p0.double()
  mag_x = x.double().abs() + abs(alpha) * p0.double().abs()
  p = p0.clone()
  _ops.cg_update_xp(x, p, z, s)
  dev_entries('update_xp', dtype, x, want_x, mag_x, 'x')
  del want_x, mag_x, x
  want_p = z.double() + beta * p0.double()
  mag_p = z.double().abs() + abs(beta) * p0.double().abs()
  dev_entries('update_xp', dtype, p, want_p, mag_p, 'p')
  p.copy_(p0)
  _ops.cg_update_p(p, z, s)
  dev_entries('update_p', dtype, p, want_p, mag_p)
  assert np.array_equal(host(s), s0)


@both
def test_large_update_xp_lazy_and_flush(dtype, large):
  """m = 2, `scalars[8]` = 1: a launch that adds both pending terms; then
  `flush_x` with one term pending."""
  n, gen = large
  stride = n + (-n) % 4 + 4
  ring = torch.randn(2, stride, dtype=dtype, device=DEV, generator=gen)
  x, z = randn(n, dtype, gen), randn(n, dtype, gen)
  s0 = block(ITERS=1.0)
  lazy0 = np.concatenate([[0.0], 0.3 + 0.1 * np.arange(CG.LAZY_MAX)])
  T = NPT[dtype]
  alpha, beta = CG.alpha_of(s0, T), CG.beta_of(s0, T)
  a0 = float(T(lazy0[1]))
  s, lazy = to_dev(s0), to_dev(lazy0)
  p0, p1 = ring[0, :n].double(), ring[1, :n].double()
  want_x = (x.double() + a0 * p0) + alpha * p1
  mag_x = x.double().abs() + a0 * p0.abs() + abs(alpha) * p1.abs()
  del p0
  pad = ring[:, n:].clone()
  keep = ring[1].clone()
  _ops.cg_update_xp_lazy(x, ring, z, s, lazy)
  dev_entries('update_xp_lazy', dtype, x, want_x, mag_x, 'x')
  del want_x, mag_x
  assert torch.equal(ring[1], keep) and torch.equal(ring[:, n:], pad)
  del keep
  want_p = z.double() + beta * p1
  mag_p = z.double().abs() + abs(beta) * p1.abs()
  del p1
  dev_entries('update_xp_lazy', dtype, ring[0, :n], want_p, mag_p, 'p')
  want_lazy = lazy0.copy()
  want_lazy[2] = alpha
  assert np.array_equal(host(lazy), want_lazy)
  assert np.array_equal(host(s), s0)
  del want_p, mag_p, z
  # three iterations closed, two of them in x: slot 0 (alpha lazy[1]) pending
  s0 = block(ITERS=3.0)
  s, lazy = to_dev(s0), to_dev(lazy0)
  want_x = x.double() + a0 * ring[0, :n].double()
  mag_x = x.double().abs() + a0 * ring[0, :n].double().abs()
  _ops.cg_flush_x(x, ring, s, lazy)
  dev_entries('flush_x', dtype, x, want_x, mag_x)
  want_lazy = lazy0.copy()
  want_lazy[0] = 3.0
  assert np.array_equal(host(lazy), want_lazy)


@both
def test_large_mean_pair(dtype, large):
  n, gen = large
  r, ap = randn(n, dtype, gen), randn(n, dtype, gen)
  w = torch.rand(n, dtype=dtype, device=DEV, generator=gen) + 0.5
  s0 = block(ITERS=1.0, CORR=0.0, MEAN=0.0)       # parity 1
  sums0 = np.zeros(CG.MEAN_SUMS)
  sums0[:128] = 1.0 + np.arange(128)              # parity 0: to be cleared
  T = NPT[dtype]
  alpha = CG.alpha_of(s0, T)
  s, sums = to_dev(s0), to_dev(sums0)
  want = r.double() - alpha * ap.double()
  mag = r.double().abs() + abs(alpha) * ap.double().abs()
  _ops.cg_update_r_mean(r, ap, w, s, sums)
  dev_entries('update_r_mean', dtype, r, want, mag)
  del want, mag, ap
  got, got_sums = host(s), host(sums)
  rd = r.double()
  dev_sum('update_r_mean.rr', dtype, CG.total(got[CG.STRIPES]),
          CG.total(s0[CG.STRIPES]), rd, rd, n)
  dev_sum('update_r_mean.1r', dtype, CG.total(got_sums[128:192]), 0.0, rd,
          torch.ones_like(rd), n)
  dev_sum('update_r_mean.wr', dtype, CG.total(got_sums[192:]), 0.0, rd,
          w.double(), n)
  same_but(got, s0, *STRIPE_IDX)
  assert np.array_equal(got_sums[:128], sums0[:128])
  total_w = float(w.double().sum())
  del w
  x, p = randn(n, dtype, gen), randn(n, dtype, gen)
  _, _, want_s, want_sums = CG.update_xp_mean(
      np.zeros(1), np.zeros(1), np.zeros(1), got, got_sums, total_w, T)
  c, corr = want_s[CG.MEAN], want_s[CG.CORR]
  beta = CG.beta_of(got, T, corr)
  want_x = x.double() + alpha * p.double()
  mag_x = x.double().abs() + abs(alpha) * p.double().abs()
  p0 = p.clone()
  _ops.cg_update_xp_mean(x, p, r, s, sums, total_w)
  dev_entries('update_xp_mean', dtype, x, want_x, mag_x, 'x')
  del want_x, mag_x, x
  want_p = (rd - float(T(c))) + beta * p0.double()
  mag_p = rd.abs() + abs(c) + abs(beta) * p0.double().abs()
  del rd, p0
  dev_entries('update_xp_mean', dtype, p, want_p, mag_p, 'p')
  after = host(s)
  assert abs(after[CG.MEAN] - c) <= (
      _sum64_bound(got_sums[192:]) / total_w + 2 * np.spacing(abs(c)))
  same_but(after, got, CG.MEAN, CG.CORR)
  assert np.array_equal(host(sums), want_sums)


@both
def test_large_jacobi_pair(dtype, large):
  n, gen = large
  r, ap = randn(n, dtype, gen), randn(n, dtype, gen)
  dinv = torch.rand(n, dtype=dtype, device=DEV, generator=gen) + 0.5
  s0 = block()
  T = NPT[dtype]
  alpha = CG.alpha_of(s0, T)
  s = to_dev(s0)
  want = r.double() - alpha * ap.double()
  mag = r.double().abs() + abs(alpha) * ap.double().abs()
  assert _ops.cg_update_r_jacobi(r, ap, dinv, s) == 0
  dev_entries('update_r_jacobi', dtype, r, want, mag)
  del want, mag, ap
  got = host(s)
  rd = r.double()
  dev_sum('update_r_jacobi.rz', dtype, CG.total(got[CG.STRIPES]),
          CG.total(s0[CG.STRIPES]), rd * dinv.double(), rd, n)
  same_but(got, s0, *STRIPE_IDX)
  x, p = randn(n, dtype, gen), randn(n, dtype, gen)
  beta = CG.beta_of(got, T)
  want_x = x.double() + alpha * p.double()
  mag_x = x.double().abs() + abs(alpha) * p.double().abs()
  p0 = p.clone()
  _ops.cg_update_xp_jacobi(x, p, r, dinv, s)
  dev_entries('update_xp_jacobi', dtype, x, want_x, mag_x, 'x')
  del want_x, mag_x, x
  want_p = dinv.double() * rd + beta * p0.double()
  mag_p = dinv.double() * rd.abs() + abs(beta) * p0.double().abs()
  del rd, p0
  dev_entries('update_xp_jacobi', dtype, p, want_p, mag_p, 'p')
  assert np.array_equal(host(s), got)


@both
def test_large_axpby(dtype, large):
  n, gen = large
  x, y = randn(n, dtype, gen), randn(n, dtype, gen)
  T = NPT[dtype]
  a, b = float(T(0.37)), float(T(-1.9))
  want = a * x.double() + b * y.double()
  mag = abs(a) * x.double().abs() + abs(b) * y.double().abs()
  _ops.axpby(0.37, x, -1.9, y)
  dev_entries('axpby', dtype, y, want, mag)
  y.fill_(float('nan'))
  _ops.axpby(0.37, x, 0.0, y)
  dev_entries('axpby', dtype, y, a * x.double(), abs(a) * x.double().abs(),
              'b = 0')


@pytest.mark.parametrize('mode', [0, 1, 2, 3])
@both
def test_large_cheb_step(dtype, mode, large):
  n, gen = large
  T = NPT[dtype]
  a, c = float(T(CHEB_A)), float(T(CHEB_C))
  b = randn(n, dtype, gen)
  if mode == 2:
    ax = randn(n, dtype, gen)
    r = torch.full_like(b, NAN)
    _ops.cheb_step(None, None, ax, b, None, r, CHEB_A, CHEB_C, 2)
    dev_entries('cheb_step.2', dtype, r, b.double() - ax.double(),
                b.double().abs() + ax.double().abs())
    return
  dinv = torch.rand(n, dtype=dtype, device=DEV, generator=gen) + 0.5
  if mode == 1:
    x, d = torch.full_like(b, NAN), torch.full_like(b, NAN)
    want_d = c * dinv.double() * b.double()
    want_x, mag_d = want_d, want_d.abs()
    mag_x = mag_d
    _ops.cheb_step(x, d, None, b, dinv, None, CHEB_A, CHEB_C, 1)
  else:
    ax, x = randn(n, dtype, gen), randn(n, dtype, gen)
    d = randn(n, dtype, gen) if mode == 0 else torch.full_like(b, NAN)
    want_d = c * dinv.double() * (b.double() - ax.double())
    mag_d = c * dinv.double() * (b.double().abs() + ax.double().abs())
    if mode == 0:
      want_d += a * d.double()
      mag_d += a * d.double().abs()
    want_x = x.double() + want_d
    mag_x = x.double().abs() + mag_d
    _ops.cheb_step(x, d, ax, b, dinv, None, CHEB_A, CHEB_C, mode)
    del ax
  dev_entries('cheb_step.%d' % mode, dtype, x, want_x, mag_x, 'x')
  dev_entries('cheb_step.%d' % mode, dtype, d, want_d, mag_d, 'd')
