"""The launch sequence of `linalg.cg.CGRunner`, mode by mode.

Every configuration below is constructed, stepped, read and (some) restarted
or captured while a recorder notes each call into `swirl_fem_amd._ops` -- the
function and, per argument, which tensor (shape, stride, dtype and its rank of
first appearance in the segment), which number, which flag -- and each call of
the test's own A / M / reduce_fn / dot_fn.  The recorded sequences are compared
with `tests/golden/cg_launch_traces.json`: a swapped operand, another ring row,
another scalar slot or phase, a missing or an extra launch all show.  No
pointer, no timing and no value is recorded.

  python tests/test_gpu_cg_launch_trace.py --write

records the file again (on the GPU); pytest only compares.
"""

import functools
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from swirl_fem_amd import _ops, switches                      # noqa: E402
from swirl_fem_amd.core import layout                         # noqa: E402
from swirl_fem_amd.linalg.cg import CGRunner                  # noqa: E402
from swirl_fem_amd.linalg.jacobi import JacobiPreconditioner  # noqa: E402
from tests.test_gpu_jacobi import DEV, dev, premesh, spaces   # noqa: E402
from tests.test_gpu_parity import make_case                   # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'cg_launch_traces.json')
F64, F32 = torch.float64, torch.float32
L0, L1 = 0.2, 1.0            # the Helmholtz coefficients of every case


# ------------------------------------------------------------------ recorder
class Recorder:
  """Events of one configuration, segment by segment (a segment: the
  construction, one step / restart / capture, one read of x / info / done)."""

  def __init__(self):
    self.segments = []
    self._events = None        # (None: between segments nothing is recorded)

  def segment(self, name, fn):
    # labels are ranks of first appearance within the segment; every tensor
    # seen is held until its end, so that the allocator cannot hand one
    # address to two temporaries: the trace does not depend on its history
    self._events, self._labels, self._held = [], {}, []
    try:
      return fn()
    finally:
      self.segments.append([name, self._events])
      self._events = self._labels = self._held = None

  def enc(self, v):
    if isinstance(v, torch.Tensor):
      key = (v.untyped_storage().data_ptr(), v.storage_offset(),
             tuple(v.shape), v.stride())
      if key not in self._labels:
        self._labels[key] = len(self._labels)
        self._held.append(v)
      return [self._labels[key], list(v.shape), list(v.stride()), str(v.dtype)]
    if v is None or isinstance(v, (bool, int, float, str)):
      return v
    if isinstance(v, (list, tuple)):
      return [self.enc(x) for x in v]
    return type(v).__name__    # (a layer plan, a part dict, host tables)

  def log(self, name, *operands):
    if self._events is not None:
      self._events.append([name] + [self.enc(o) for o in operands])

  def logged(self, name, fn):
    """`fn` as a callable that notes its call and operands first."""
    def call(*operands):
      self.log(name, *operands)
      return fn(*operands)
    return call

  def wrap(self, name, fn):
    sig = inspect.signature(fn)

    @functools.wraps(fn)
    def call(*args, **kwargs):
      if self._events is not None:
        # (by parameter name: positional or keyword is the caller's business)
        bound = sig.bind(*args, **kwargs)
        bound.apply_defaults()
        self._events.append([name] + [[k, self.enc(v)]
                                      for k, v in bound.arguments.items()])
      return fn(*args, **kwargs)
    return call

  def patch(self, mp):
    """Wraps every public function that `_ops` defines (cg.py, operators.py,
    jacobi.py and distributed/solver.py call through the module attribute)."""
    for name, fn in list(vars(_ops).items()):
      if (not name.startswith('_') and inspect.isfunction(fn) and
          fn.__module__ == _ops.__name__):
        mp.setattr(_ops, name, self.wrap(name, fn))


# --------------------------------------------------------------------- stubs
class LoggedJacobi(JacobiPreconditioner):
  def __init__(self, rec, *args):
    super().__init__(*args)
    self.rec = rec

  def __call__(self, r):
    self.rec.log('M', r)
    return super().__call__(r)


class DotStub:
  """A preconditioner that accumulates r . M r itself."""

  def __init__(self, rec):
    self.rec = rec

  def __call__(self, r):
    self.rec.log('M', r)
    return 0.5 * r

  def apply_with_dot(self, r, scalars, slot):
    self.rec.log('M.apply_with_dot', r, scalars, slot)
    z = 0.5 * r
    _ops.dot(r, z, scalars, slot, accumulate=True)
    return z


class MeanStub:
  """M r = r - (w . r / total) 1 with w = 1."""

  def __init__(self, rec, like):
    self.rec, self.w = rec, torch.ones_like(like)

  def mean_projection(self):
    self.rec.log('M.mean_projection')
    return self.w, float(self.w.numel())

  def __call__(self, r):
    self.rec.log('M', r)
    return r - r.mean()


class ResidualStopStub:
  stops_on_residual = True

  def __init__(self, rec, dinv, consistent):
    self.rec, self.dinv, self.consistent = rec, dinv, consistent

  def __call__(self, r):
    self.rec.log('M', r)
    return self.dinv * r


# ------------------------------------------------------------ configurations
@functools.lru_cache(maxsize=None)
def _problem(mesh_name, dtype, layered):
  """(mesh, op, b, b2) -- `layered`: the value of SFEM_LAYERED the operator
  meets on first use (it keeps its layer plan, or the lack of one)."""
  del layered
  if mesh_name == 'quad':                   # tests/test_gpu_parity.py
    P, rp = 5, make_case(2, 4, 5)
  else:                                     # tests/test_gpu_jacobi.py
    P = {'box6': 6, 'box4': 4}[mesh_name]
    rp = premesh(3, 3, P, 'jitter', seed=0)
  mesh, fes, _ = spaces(rp, P, P, 'gll', dtype)
  op = fes.helmholtz_operator(mesh.physical_masks['boundary'])
  rng = np.random.default_rng(1)
  b, b2 = (op.apply(dev(rng.standard_normal(mesh.num_nodes), dtype), 1.0, 0.0)
           for _ in range(2))
  return mesh, op, b, b2


# name: (mesh, A, M, keywords); keywords: env = SFEM_* switches, reduce /
# interface / dot_fn = pass that argument, b = 'cm3' | 'dict', script,
# fp32 = also in float32
CASES = {
    '01_unfused': ('box4', 'lambda', None, {}),
    '02_fused_dot': ('box4', 'fused', None, dict(fp32=True)),
    '03_reduce': ('box4', 'fused', None, dict(reduce=True)),
    # (with the fused dot p.Ap is p . unassembled Ap and takes no interface
    # correction: the one on PAP is pinned by 17 and 21, whose A is a lambda)
    '04_interface': ('box4', 'fused', None, dict(reduce=True, interface=True)),
    '05_layered_det': ('box6', 'fused', None, dict(fp32=True)),
    '06_layered': ('box6', 'fused', None,
                   dict(env={'SFEM_DETERMINISTIC': '0'})),
    '07_atomic_p6': ('box6', 'fused', None, dict(env={'SFEM_LAYERED': '0'})),
    '08_lazy4': ('box6', 'fused', None,
                 dict(env={'SFEM_LAZY_X_MIN_MB': '0'}, fp32=True)),
    '09_lazy2': ('box6', 'fused', None,
                 dict(env={'SFEM_LAZY_X_MIN_MB': '0', 'SFEM_LAZY_X': '2'})),
    '10_layered_m': ('box6', 'fused', 'half', {}),
    '11_m_with_dot': ('box4', 'lambda', 'dot_stub', {}),
    '12_jacobi': ('box4', 'lambda', 'jacobi', {}),
    '13_jacobi_unfused_lazy': (
        'box4', 'lambda', 'jacobi',
        dict(env={'SFEM_FUSED_JACOBI': '0', 'SFEM_LAZY_X_MIN_MB': '0'})),
    '14_jacobi_layered_det': ('box6', 'fused', 'jacobi', dict(fp32=True)),
    '15_jacobi_layered': ('box6', 'fused', 'jacobi',
                          dict(env={'SFEM_DETERMINISTIC': '0'})),
    '16_jacobi_ncomp3': ('box4', 'lambda', 'jacobi', dict(b='cm3')),
    '17_jacobi_interface': ('box4', 'lambda', 'jacobi',
                            dict(reduce=True, interface=True)),
    '18_mean': ('quad', 'lambda', 'mean', {}),
    '19_mean_unfused': ('quad', 'lambda', 'mean',
                        dict(env={'SFEM_FUSED_MEAN': '0'})),
    '20_rr_stop_layered': ('box6', 'fused', 'rr_stop', {}),
    '21_rr_stop_interface': ('box4', 'lambda', 'rr_stop_consistent',
                             dict(reduce=True, interface=True)),
    '22_dot_fn': ('box4', 'lambda', None, dict(dot_fn=True)),
    '23_pytree': ('box4', 'lambda', None, dict(b='dict')),
    '24_restart_det': ('box6', 'fused', None, dict(script='restart')),
    '25_restart_lazy_x0': ('box6', 'fused', None,
                           dict(env={'SFEM_LAZY_X_MIN_MB': '0'},
                                script='restart_x0')),
    '26_restart_rr_stop': ('box6', 'fused', 'rr_stop',
                           dict(script='restart_only')),
    '27_capture_lazy': ('box6', 'fused', None,
                        dict(env={'SFEM_LAZY_X_MIN_MB': '0'},
                             script='capture')),
    '28_capture_merged': ('box4', 'fused', None, dict(script='capture')),
}
PARAMS = [(name, dtype) for name, row in CASES.items()
          for dtype in ((F64, F32) if row[3].get('fp32') else (F64,))]


def _make_runner(rec, name, dtype):
  """The case's right-hand sides and a function that constructs its runner."""
  mesh_name, a_kind, m_kind, kw = CASES[name]
  mesh, op, b, b2 = _problem(mesh_name, dtype,
                             switches.get('SFEM_LAYERED'))
  interior = (~mesh.physical_masks['boundary']).to(dtype)
  if kw.get('b') == 'cm3':
    if mesh.num_nodes % 2:
      pytest.skip('odd node count: the fused vector path needs N even in fp64')
    b, b2 = (layout.component_major(torch.stack([v, 2 * v, -v], dim=1))
             for v in (b, b2))
  apply = lambda u: op.apply(u, L0, L1)
  if kw.get('b') == 'dict':
    b, b2 = ({'u': v, 'v': 2 * v} for v in (b, b2))
    A = rec.logged('A', lambda t: {k: apply(v) for k, v in t.items()})
  elif a_kind == 'lambda':
    A = rec.logged('A', apply)
  else:
    A = op.linear_operator(L0, L1)
  M = None
  if m_kind == 'half':
    M = rec.logged('M', lambda r: 0.5 * r)
  elif m_kind == 'dot_stub':
    M = DotStub(rec)
  elif m_kind == 'jacobi':
    M = LoggedJacobi(rec, op, L0, L1)
  elif m_kind == 'mean':
    M = MeanStub(rec, b)
  elif m_kind in ('rr_stop', 'rr_stop_consistent'):
    M = ResidualStopStub(rec, 0.5 + interior, m_kind == 'rr_stop_consistent')
  args = dict(M=M, tol=1e-14)
  if kw.get('reduce'):
    args['reduce_fn'] = rec.logged('reduce', lambda t: t)
  if kw.get('interface'):
    # five interior nodes with weight zero: every correction is launched and
    # none changes a sum
    idx = torch.nonzero(interior).reshape(-1)[:5].contiguous()
    args['interface'] = (idx, torch.zeros(5, dtype=F64, device=DEV))
  if kw.get('dot_fn'):
    args['dot_fn'] = rec.logged('dot_fn', lambda u, v: (u * v).sum())
  return b, b2, lambda: CGRunner(A, b, **args)


def _play(name, dtype):
  """The segments of one configuration."""
  rec = Recorder()
  env = CASES[name][3].get('env', {})
  script = CASES[name][3].get('script', 'standard')
  with pytest.MonkeyPatch.context() as mp:
    for k in switches.SWITCHES:             # only the switches the row names
      if k not in ('SFEM_LIB', 'SFEM_HDF5_LIB'):
        mp.delenv(k, raising=False)
    for k, v in env.items():
      mp.setenv(k, v)
    b, b2, make = _make_runner(rec, name, dtype)
    rec.patch(mp)
    run = rec.segment('init', make)
    steps = lambda n: [rec.segment('step', run.step) for _ in range(n)]
    if script == 'capture':
      assert rec.segment('capture', run.capture)
      steps(3)
      rec.segment('info', run.info)
    else:
      # (six steps: the lazy ring goes through one full turn at m = 4)
      steps(6)
      rec.segment('x', lambda: run.x)
      rec.segment('info', run.info)
      rec.segment('done', run.done)
      steps(1)
    if script.startswith('restart'):
      x0 = run.x.clone() if script == 'restart_x0' else None
      rec.segment('restart', lambda: run.restart(b2, x0))
      if script != 'restart_only':
        steps(2)
    torch.cuda.synchronize()
  return rec.segments


def _record(name, dtype):
  # Once unrecorded first: whatever the operator or the library sets up on
  # first use (a layer plan, per-process self tests) is then in place, and
  # the trace does not depend on which tests ran before.
  _play(name, dtype)
  return _play(name, dtype)


def _case_id(name, dtype):
  return f'{name}-{str(dtype).split(".")[-1]}'


# -------------------------------------------------------------- golden file
def _load():
  with open(GOLDEN) as f:
    doc = json.load(f)
  events = doc['events']
  return {cid: [[seg, [events[i] for i in idx]] for seg, idx in segs]
          for cid, segs in doc['cases'].items()}


def _write():
  """Events are stored once and referred to by index: most steps of a
  configuration repeat the same few."""
  table, cases = {}, {}
  for name, dtype in PARAMS:
    segs = json.loads(json.dumps(_record(name, dtype)))
    cases[_case_id(name, dtype)] = [
        [seg, [table.setdefault(json.dumps(e), len(table)) for e in events]]
        for seg, events in segs]
  lines = ['{"events": [']
  lines.append(',\n'.join(table))
  lines.append('],\n"cases": {')
  lines.append(',\n'.join(
      json.dumps(cid) + ': [\n' + ',\n'.join(
          '  ' + json.dumps(seg) for seg in segs) + ']'
      for cid, segs in cases.items()))
  lines.append('}}')
  with open(GOLDEN, 'w') as f:
    f.write('\n'.join(lines) + '\n')
  print(f'{len(cases)} configurations, {len(table)} distinct events -> '
        f'{GOLDEN}')


@pytest.fixture(scope='module')
def golden():
  return _load()


@pytest.mark.parametrize('name,dtype', PARAMS,
                         ids=[_case_id(*p) for p in PARAMS])
def test_cg_launch_sequence(name, dtype, golden):
  want = golden[_case_id(name, dtype)]
  got = json.loads(json.dumps(_record(name, dtype)))
  for s, ((wseg, wev), (gseg, gev)) in enumerate(zip(want, got)):
    assert wseg == gseg, f'segment {s}: recorded {wseg!r}, now {gseg!r}'
    for i, (w, g) in enumerate(zip(wev, gev)):
      assert w == g, (f'segment {s} ({wseg}), event {i}:\n  recorded {w}\n'
                      f'  now      {g}')
    assert len(wev) == len(gev), (
        f'segment {s} ({wseg}): {len(wev)} events recorded, now {len(gev)}; '
        f'first unmatched: {max(wev, gev, key=len)[min(len(wev), len(gev))]}')
  assert len(want) == len(got)


if __name__ == '__main__':
  if sys.argv[1:] != ['--write']:
    sys.exit('usage: python tests/test_gpu_cg_launch_trace.py --write')
  _write()
