"""The boundary facet kernels, called through `_ops` against the plain NumPy
reference `tests/boundary_reference.py` (no mesh, no `FiniteElementSpace`):
`sfem_boundary_geom`, `sfem_boundary_covector`, `sfem_boundary_mass_apply`,
`sfem_boundary_mass_diag` and `sfem_boundary_add_rows`
(`swirl_fem_amd/csrc/sfem_boundary.hip`).

a. every instantiation: the 24 compiled (P+1, Q) pairs and ten pairs of the
   run-time path, edges and faces, both precisions, on inputs that turn an
   indexing mistake into an O(1) error (`test_boundary_reference_host.py`
   shows that they do): non-symmetric B, another D_q, distinct weights, facet
   ids shared between facets with ids 0 and N - 1 among them;
b. the slot rule: ~id slots read 0 and write 0, ~0 == -1 included, NaN behind
   every masked node;
c. one facet axis at a time, where exchanging the axes is shown to give
   another answer;
d. `add_rows` on its own, bit for bit;
e. no facets, one facet;
f. what the wrappers and the library refuse before anything is launched.  The
   library's "does not fit in LDS" answer is unreachable: the largest legal
   size, 16 x 16 points on faces in fp64, needs about 41 KB of the 64 KB;
g. `geom` in fp32 with real GLL / Gauss matrices, whose derivative entries
   reach 53 at 13 points (the random D_q of a. has O(1) entries).

Bounds.  fp64 against the float64 reference: 1e-12 relative to the largest
entry of the expected array (a, b, e; the bound of `test_gpu_boundary.py`),
1e-13 where the inputs are one line (c), bitwise (d).  fp32:
`fp32util.tolerance` on float32-representable inputs; a case above it would
get max(tolerance, 4 x the error of the reference evaluated in float32 on the
same inputs), the factor covering another summation order and fused
multiply-adds.  The measured numbers, and whether any case needed that, are
in `profiles/boundary_kernel_errors.md`.

Needs a real MI355X."""
import numpy as np
import pytest
import torch

from swirl_fem_amd import _lib, _ops
from swirl_fem_amd.core import interpolation
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType, Quadrature1D
from tests import boundary_reference as R
from tests.fp32util import f32r, tolerance

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64, F32 = torch.float64, torch.float32
NAME = {F64: 'fp64', F32: 'fp32'}
NP = {F64: np.float64, F32: np.float32}
KEYS = ('geom.xq', 'geom.wJ', 'covector.nodal', 'covector.points',
        'mass_apply', 'mass_diag')


def dev(x, dtype=None):
  t = torch.as_tensor(np.array(x), device=DEV)   # a copy: inputs are cached
  return t if dtype is None else t.to(dtype)


def _np(t):
  return t.detach().double().cpu().numpy()


def run_all(a, dtype, encoded=None, u=None):
  """Every output of `boundary_reference.evaluate` from the kernels."""
  f = dev(a['facets'])
  enc = f if encoded is None else dev(encoded)
  B = dev(a['B'], dtype)
  ndim = a['ndim']
  xq, wJ = _ops.boundary_geom(dev(a['coords'], dtype), f, B,
                              dev(a['Dq'], dtype), dev(a['w'], dtype))
  wj_in, aw = dev(a['wJ'], dtype), dev(a['aw'], dtype)
  return {
      'geom.xq': xq, 'geom.wJ': wJ,
      'covector.nodal': _ops.boundary_covector(dev(a['g_nodal'], dtype), True,
                                               f, wj_in, B, ndim),
      'covector.points': _ops.boundary_covector(dev(a['g_points'], dtype),
                                                False, f, wj_in, B, ndim),
      'mass_apply': _ops.boundary_mass(
          dev(a['u'] if u is None else u, dtype), enc, aw, B, ndim,
          scale=a['scale']),
      'mass_diag': _ops.boundary_mass(None, enc, aw, B, ndim,
                                      scale=a['scale'], diag=True)}


def shapes(a):
  F, d = a['F'], a['ndim']
  nf, nq = a['p1'] ** a['k'], a['q'] ** a['k']
  return {'geom.xq': (F, nq, d), 'geom.wJ': (F, nq),
          'covector.nodal': (F, nf), 'covector.points': (F, nf),
          'mass_apply': (F, nf), 'mass_diag': (F, nf)}


def check(tag, a, dtype, got, want, fp64_tol=1e-12, keys=KEYS):
  """Shape, dtype and error of every output; one line per output.  fp32: the
  float32 reference is evaluated only to size the exception."""
  ref32 = R.evaluate(a, np.float32) if dtype == F32 and a['F'] else None
  worst = {}
  for key in keys:
    assert got[key].dtype == dtype, key
    assert tuple(got[key].shape) == shapes(a)[key], key
    assert bool(torch.isfinite(got[key]).all()), key
    err = R.relerr(_np(got[key]), want[key])
    if dtype == F64:
      tol, note = fp64_tol, ''
    else:
      base = tolerance(dtype, a['p1'])
      e_ref = R.relerr(ref32[key], want[key]) if ref32 else 0.0
      tol = base if err < base else max(base, 4 * e_ref)
      note = f' float32 reference {e_ref:.2e}' + (
          ' EXCEPTION' if err >= base else '')
    print(f'BNDERR {tag} {key} ndim={a["ndim"]} p1={a["p1"]} q={a["q"]} '
          f'{NAME[dtype]}: err {err:.2e} (bound {tol:.1e}){note}')
    worst[key] = (err, tol)
  for key, (err, tol) in worst.items():
    assert err < tol, (tag, key, a['ndim'], a['p1'], a['q'], dtype, err, tol)


# ------------------------------------------------- a. every instantiation
def test_pairs_are_the_compiled_table_and_the_run_time_cases():
  assert len(R.COMPILED_PAIRS) == 24 and len(R.PAIRS) == 34
  assert set(R.COMPILED_PAIRS) == {(n, n) for n in range(2, 14)} | {
      (n, n + 1) for n in range(2, 14)}
  assert not set(R.RUNTIME_PAIRS) & set(R.COMPILED_PAIRS)


@pytest.mark.parametrize('dtype', [F64, F32], ids=NAME.get)
@pytest.mark.parametrize('p1,q', R.PAIRS)
@pytest.mark.parametrize('ndim', [2, 3])
def test_every_instantiation(ndim, p1, q, dtype):
  a = R.synthetic(ndim, p1, q, f32=dtype == F32)
  assert a['F'] == 5 and a['N'] == 3 * 5 * p1 ** (ndim - 1) + 7
  want = R.evaluate(a)
  got = run_all(a, dtype)
  kind = 'compiled' if (p1, q) in R.COMPILED_PAIRS else 'run-time'
  check(f'a {kind}', a, dtype, got, want)
  again = run_all(a, dtype)
  for key in KEYS:
    assert torch.equal(got[key], again[key]), key


# -------------------------------------------------------- b. the slot rule
@pytest.mark.parametrize('dtype', [F64, F32], ids=NAME.get)
@pytest.mark.parametrize('fraction', [0.3, 1.0, 0.0],
                         ids=['some', 'all', 'none'])
@pytest.mark.parametrize('p1,q', [(2, 2), (5, 6), (13, 14), (14, 14)])
@pytest.mark.parametrize('ndim', [2, 3])
def test_slot_rule(ndim, p1, q, fraction, dtype):
  """Masked nodes hold NaN in u and their slots are stored as ~id (node 0:
  -1): the apply is finite, exactly 0 in those slots and the reference's
  elsewhere; the diagonal is exactly 0 there."""
  a = R.synthetic(ndim, p1, q, f32=dtype == F32)
  masked, enc = R.mask_nodes(a, fraction)
  if fraction == 1.0:
    masked[:] = True
    enc = (~a['facets']).astype(np.int32)
  hidden = enc < 0
  if fraction > 0:
    assert (enc == -1).any() and masked[0]
    assert fraction == 1.0 or (0.1 < hidden.mean() < 0.6)
  else:
    assert not hidden.any()
  u = np.where(masked, np.nan, a['u'])
  keys = ('mass_apply', 'mass_diag')
  want = {k: v for k, v in R.evaluate(a, encoded=enc, u=u).items()
          if k in keys}
  B, aw = dev(a['B'], dtype), dev(a['aw'], dtype)
  nan = torch.full(a['facets'].shape, float('nan'), dtype=dtype, device=DEV)
  got = {
      'mass_apply': _ops.boundary_mass(dev(u, dtype), dev(enc), aw, B, ndim,
                                       scale=a['scale'], out=nan.clone()),
      'mass_diag': _ops.boundary_mass(None, dev(enc), aw, B, ndim,
                                      scale=a['scale'], diag=True,
                                      out=nan.clone())}
  for key in keys:
    g = _np(got[key])
    assert np.isfinite(g).all(), key
    assert np.all(g[hidden] == 0.0), key
    assert np.all(want[key][hidden] == 0.0), key
  if fraction == 1.0:
    for key in keys:
      assert float(got[key].abs().max()) == 0.0, key
  else:
    ref32 = None
    for key in keys:
      err = R.relerr(_np(got[key]), want[key])
      if dtype == F64:
        tol = 1e-12
      else:
        tol = tolerance(dtype, p1)
        if err >= tol:                      # the exception, sized when needed
          ref32 = ref32 or R.evaluate(a, np.float32, encoded=enc, u=u)
          tol = max(tol, 4 * R.relerr(ref32[key], want[key]))
      print(f'BNDERR b {key} ndim={ndim} p1={p1} q={q} {NAME[dtype]} masked '
            f'{hidden.mean():.2f}: err {err:.2e} (bound {tol:.1e})')
      assert err < tol, (key, err)


# --------------------------------------------------- c. one axis at a time
def axis_inputs(p1, q, axis, seed=0):
  """3D inputs with F = 3 facets of distinct ids in which every field is one
  line along facet axis `axis` (0: the slow index): u and g nodal on the
  nodes (i, j0) or (i0, j), the point fields on (a, c0) or (a0, c), and
  coordinates that depend on the index along `axis` alone."""
  rng = np.random.default_rng(1000 * seed + 100 * p1 + 10 * q + axis)
  F, nf, nq = 3, p1 * p1, q * q
  N = F * nf + 5
  B, Dq, w = R.matrices(rng, p1, q)
  facets = rng.permutation(N)[:F * nf].reshape(F, nf).astype(np.int32)

  def line(n, values):
    """(F, n * n): `values` (F, n) along `axis`, at one index of the other."""
    t = np.zeros((F, n, n))
    other = int(rng.integers(0, n))
    if axis == 0:
      t[:, :, other] = values
    else:
      t[:, other, :] = values
    return t.reshape(F, n * n)

  def nodal(values):
    v = np.zeros(N)
    v[facets.reshape(-1)] = values.reshape(-1)
    return v

  along = np.broadcast_to(
      rng.standard_normal((F, p1, 1, 3)) if axis == 0 else
      rng.standard_normal((F, 1, p1, 3)), (F, p1, p1, 3))
  coords = np.zeros((N, 3))
  coords[facets.reshape(-1)] = along.reshape(-1, 3)
  a = dict(ndim=3, p1=p1, q=q, k=2, N=N, F=F, B=B, Dq=Dq, w=w, facets=facets,
           coords=coords, wJ=rng.uniform(0.5, 1.5, (F, nq)),
           aw=line(q, rng.uniform(0.5, 1.5, (F, q))),
           g_nodal=nodal(line(p1, rng.standard_normal((F, p1)))),
           g_points=line(q, rng.standard_normal((F, q))),
           u=nodal(line(p1, rng.standard_normal((F, p1)))), scale=-1.7)
  # the same fields with the facet axes exchanged on the way in
  s = dict(a, facets=R.swap_axes(facets, p1), wJ=R.swap_axes(a['wJ'], q),
           aw=R.swap_axes(a['aw'], q), g_points=R.swap_axes(a['g_points'], q))
  return a, s


@pytest.mark.parametrize('p1,q', [(4, 4), (4, 5), (6, 3)])
@pytest.mark.parametrize('axis', [0, 1])
def test_one_axis_at_a_time(axis, p1, q):
  """The kernels must give the reference's answer; the reference that reads
  its inputs with the facet axes exchanged must not (else the case shows
  nothing)."""
  a, swapped = axis_inputs(p1, q, axis)
  want, wrong = R.evaluate(a), R.evaluate(swapped)
  gaps = {key: R.relerr(wrong[key], want[key]) for key in KEYS}
  for key, gap in gaps.items():
    assert gap >= 1e-2, (key, gap)
  got = run_all(a, F64)
  print(f'BNDERR c axis={axis} p1={p1} q={q}: axes exchanged at '
        + ', '.join(f'{k}: {v:.2e}' for k, v in gaps.items()))
  check(f'c axis={axis}', a, F64, got, want, fp64_tol=1e-13)


# ------------------------------------------------------------- d. add_rows
def _bits(t):
  return t.view(torch.int64 if t.dtype == F64 else torch.int32)


@pytest.mark.parametrize('dtype', [F64, F32], ids=NAME.get)
@pytest.mark.parametrize('num_rows', [0, 1, 255, 256, 257, 1000])
def test_add_rows(num_rows, dtype):
  """Bitwise the sequential loop of the reference in the same dtype; entries
  of `out` that `rows` does not list keep their pattern; no rows: `out` as it
  was."""
  local, rows, offsets, slots, out = R.add_rows_inputs(num_rows,
                                                     f32=dtype == F32)
  assert len(out) > num_rows
  counts = np.diff(offsets)
  if num_rows > 1:
    assert counts[0] == counts[-1] == counts[num_rows // 2] == 0
    assert counts.max() == 9
  want = R.add_rows(local, rows, offsets, slots, out, dtype=NP[dtype])
  outd = dev(out, dtype)
  before = outd.clone()
  ret = _ops.boundary_add_rows(dev(local, dtype), dev(rows), dev(offsets),
                               dev(slots), outd)
  assert ret is outd
  assert torch.equal(_bits(outd), _bits(dev(want)))
  listed = np.zeros(len(out), bool)
  listed[rows] = True
  rest = dev(~listed)
  assert torch.equal(_bits(outd)[rest], _bits(before)[rest])
  if num_rows == 0:
    assert torch.equal(_bits(outd), _bits(before))
  else:
    assert not torch.equal(outd, before)


# ----------------------------------------------------- e. empty and partial
@pytest.mark.parametrize('dtype', [F64, F32], ids=NAME.get)
@pytest.mark.parametrize('ndim,p1,q', [(2, 3, 4), (3, 3, 3), (3, 14, 15)])
def test_no_facets(ndim, p1, q, dtype):
  a = R.synthetic(ndim, p1, q, f32=dtype == F32, F=0)
  got = run_all(a, dtype)
  for key in KEYS:
    assert got[key].dtype == dtype and got[key].numel() == 0
    assert tuple(got[key].shape) == shapes(a)[key], key
  torch.cuda.synchronize()


@pytest.mark.parametrize('dtype', [F64, F32], ids=NAME.get)
@pytest.mark.parametrize('ndim,p1,q', [(2, 3, 4), (3, 3, 3), (3, 14, 15)])
def test_one_facet(ndim, p1, q, dtype):
  a = R.synthetic(ndim, p1, q, f32=dtype == F32, F=1)
  assert a['facets'].shape[0] == 1
  check('e one facet', a, dtype, run_all(a, dtype), R.evaluate(a))


# ------------------------------------------------------------- f. refusals
def _args(ndim=3, p1=3, q=4, dtype=F64):
  a = R.synthetic(ndim, p1, q)
  t = {k: dev(a[k], dtype) for k in ('coords', 'B', 'Dq', 'w', 'wJ', 'aw',
                                     'g_nodal', 'g_points', 'u')}
  t.update(facets=dev(a['facets']), ndim=ndim)
  return t


def _geom(t):
  return _ops.boundary_geom(t['coords'], t['facets'], t['B'], t['Dq'], t['w'])


def _covector(t, nodal=False):
  return _ops.boundary_covector(t['g_nodal'] if nodal else t['g_points'],
                                nodal, t['facets'], t['wJ'], t['B'], t['ndim'])


def _mass(t, diag=False):
  return _ops.boundary_mass(None if diag else t['u'], t['facets'], t['aw'],
                            t['B'], t['ndim'], scale=-1.7, diag=diag,
                            out=t.get('out'))


def _wider(x):
  return torch.cat([x, x[:, :1]], dim=1).contiguous()


REFUSALS = {
    'geom: B float32': (_geom, lambda t: t.update(B=t['B'].float())),
    'geom: D_q float32': (_geom, lambda t: t.update(Dq=t['Dq'].float())),
    'geom: weights float32': (_geom, lambda t: t.update(w=t['w'].float())),
    'geom: facets int64': (_geom, lambda t: t.update(
        facets=t['facets'].long())),
    'geom: facets wider': (_geom, lambda t: t.update(
        facets=_wider(t['facets']))),
    'geom: facets of an edge': (_geom, lambda t: t.update(
        facets=t['facets'][:, :3].contiguous())),
    'geom: coords not contiguous': (_geom, lambda t: t.update(
        coords=t['coords'].repeat(1, 2)[:, ::2])),
    'covector: B float32': (_covector, lambda t: t.update(B=t['B'].float())),
    'covector: g float32': (_covector, lambda t: t.update(
        g_points=t['g_points'].float())),
    'covector: wJ float32': (_covector, lambda t: t.update(
        wJ=t['wJ'].float())),
    'covector: facets int64': (_covector, lambda t: t.update(
        facets=t['facets'].long())),
    'covector: facets wider': (_covector, lambda t: t.update(
        facets=_wider(t['facets']))),
    'covector: wJ wider': (_covector, lambda t: t.update(wJ=_wider(t['wJ']))),
    'covector: wJ of fewer facets': (_covector, lambda t: t.update(
        wJ=t['wJ'][:-1].contiguous())),
    'covector: point values wider': (_covector, lambda t: t.update(
        g_points=_wider(t['g_points']))),
    'covector: point values flat': (_covector, lambda t: t.update(
        g_points=t['g_points'].reshape(-1))),
    'mass: B float32': (_mass, lambda t: t.update(B=t['B'].float())),
    'mass: u float32': (_mass, lambda t: t.update(u=t['u'].float())),
    'mass: aw float32': (_mass, lambda t: t.update(aw=t['aw'].float())),
    'mass: facets int64': (_mass, lambda t: t.update(
        facets=t['facets'].long())),
    'mass: facets wider': (_mass, lambda t: t.update(
        facets=_wider(t['facets']))),
    'mass: aw wider': (_mass, lambda t: t.update(aw=_wider(t['aw']))),
    'mass: aw of fewer facets': (_mass, lambda t: t.update(
        aw=t['aw'][:-1].contiguous())),
    'mass: u not contiguous': (_mass, lambda t: t.update(
        u=t['u'].repeat_interleave(2)[::2])),
    'mass: u 2-D': (_mass, lambda t: t.update(u=t['u'].reshape(-1, 1))),
    'mass: out wider': (_mass, lambda t: t.update(
        out=torch.empty((5, 10), dtype=F64, device=DEV))),
    'mass: out flat': (_mass, lambda t: t.update(
        out=torch.empty(45, dtype=F64, device=DEV))),
    'mass: out float32': (_mass, lambda t: t.update(
        out=torch.empty((5, 9), dtype=F32, device=DEV))),
    'mass: out not contiguous': (_mass, lambda t: t.update(
        out=torch.empty((5, 18), dtype=F64, device=DEV)[:, ::2])),
}


@pytest.mark.parametrize('what', REFUSALS)
def test_wrappers_refuse(what):
  call, spoil = REFUSALS[what]
  t = _args()
  call(t)                                   # the unspoilt call is accepted
  spoil(t)
  with pytest.raises(ValueError):
    call(t)
  if what.startswith('mass') and 'u ' not in what:
    with pytest.raises(ValueError):
      _mass(t, diag=True)
  torch.cuda.synchronize()


def _sized(ndim, p1, q, F=2):
  """Tensors whose shapes are consistent for (p1, q), so that they pass the
  wrappers and reach the library's range check."""
  k = ndim - 1
  z = lambda *s: torch.zeros(s, dtype=F64, device=DEV)
  return dict(coords=z(8, ndim), B=z(q, p1), Dq=z(q, p1), w=z(q),
              wJ=z(F, q ** k), aw=z(F, q ** k), g_nodal=z(8),
              g_points=z(F, q ** k), u=z(8), ndim=ndim,
              facets=torch.zeros((F, p1 ** k), dtype=torch.int32, device=DEV))


@pytest.mark.parametrize('ndim', [2, 3])
@pytest.mark.parametrize('p1,q', [(1, 2), (17, 3), (3, 17), (17, 17), (3, 0)])
def test_library_refuses_sizes(ndim, p1, q):
  """P+1 = 1 or 17 and Q = 0 or 17 have no kernel: the library's own range
  check answers (SFEM_EINVAL, with the range in the message) for facets and
  for none, and nothing is launched.  (A (0, p1) matrix does reach the
  library, so Q = 0 is among the cases.)"""
  msg = r'need 2 <= P\+1 <= 16 and 1 <= Q <= 16'
  for F in (2, 0):
    t = _sized(ndim, p1, q, F)
    for call in (_geom, _covector, lambda t: _covector(t, True), _mass,
                 lambda t: _mass(t, True)):
      with pytest.raises(_lib.SfemError, match=msg):
        call(t)
  torch.cuda.synchronize()


def test_geom_refuses_four_columns():
  """coords (N, 4): facets that are consistent with it ((F, p1^3)) pass the
  wrapper and the library answers; the facets of a face do not pass."""
  t = _sized(3, 3, 3)
  t['coords'] = torch.zeros((8, 4), dtype=F64, device=DEV)
  with pytest.raises(ValueError):
    _geom(t)
  t['facets'] = torch.zeros((2, 27), dtype=torch.int32, device=DEV)
  with pytest.raises(_lib.SfemError, match=r'ndim=4 \(2 or 3\)'):
    _geom(t)
  torch.cuda.synchronize()


def test_add_rows_refuses():
  local, rows, offsets, slots, out = R.add_rows_inputs(7)
  good = dict(local=dev(local), rows=dev(rows), offsets=dev(offsets),
              slots=dev(slots), out=dev(out))
  before = good['out'].clone()
  spoilt = {
      'rows int64': dict(rows=good['rows'].long()),
      'slots int64': dict(slots=good['slots'].long()),
      'offsets int32': dict(offsets=good['offsets'].int()),
      'offsets short': dict(offsets=good['offsets'][:-1].contiguous()),
      'offsets long': dict(offsets=torch.cat([good['offsets'],
                                              good['offsets'][-1:]])),
      'local float32': dict(local=good['local'].float()),
      'out 2-D': dict(out=good['out'].reshape(-1, 1)),
      'out not contiguous': dict(out=good['out'].repeat_interleave(2)[::2]),
  }
  for what, change in spoilt.items():
    with pytest.raises(ValueError):
      _ops.boundary_add_rows(**dict(good, **change))
  assert torch.equal(good['out'], before)


# ------------------------------------------- g. real matrices in fp32, geom
def real_case(p1, q, F=5, seed=0):
  """GLL nodes with p1 points; the GLL rule (q = p1) or the Gauss rule
  (q = p1 + 1); F bilinear faces with jittered corners in 3D, their nodes
  rounded to float32 and numbered at random."""
  grid = Nodes1D.create(p1, NodeType.GAUSS_LOBATTO_LEGENDRE)
  quad = Quadrature1D.create(q, NodeType.GAUSS_LOBATTO_LEGENDRE if q == p1
                             else NodeType.GAUSS_LEGENDRE)
  i1, d1 = interpolation.matrices_1d(grid, quad.nodes)
  B = f32r(np.asarray(i1))
  Dq = f32r(np.asarray(i1) @ np.asarray(d1))
  w = f32r(np.asarray(quad.weights))
  rng = np.random.default_rng(100 * p1 + q + seed)
  s = (np.asarray(grid.node_values) + 1) / 2             # [0, 1]
  h = 0.5
  X = np.empty((F, p1, p1, 3))
  for f in range(F):
    c = np.array([[f * h, 0, 0], [f * h, h, 0], [(f + 1) * h, 0, 0],
                  [(f + 1) * h, h, 0]], float).reshape(2, 2, 3)
    c += 0.2 * h * rng.uniform(-1, 1, c.shape)
    l = np.stack([1 - s, s])                             # (2, p1)
    X[f] = np.einsum('ai,bj,abd->ijd', l, l, c)
  N = F * p1 * p1
  facets = rng.permutation(N).reshape(F, p1 * p1).astype(np.int32)
  coords = np.empty((N, 3))
  coords[facets.reshape(-1)] = X.reshape(-1, 3)
  return dict(ndim=3, p1=p1, q=q, k=2, N=N, F=F, B=B, Dq=Dq, w=w,
              facets=facets, coords=f32r(coords))


@pytest.mark.parametrize('p1,q', R.COMPILED_PAIRS)
def test_geom_fp32_real_matrices(p1, q):
  a = real_case(p1, q)
  if q == p1:           # the corner entry of the GLL derivative matrix
    assert np.abs(a['Dq']).max() >= (p1 * (p1 - 1) / 4) * (1 - 1e-6)
  args = (a['coords'], a['facets'], a['B'], a['Dq'], a['w'])
  want = dict(zip(('geom.xq', 'geom.wJ'), R.geom(*args)))
  ref32 = dict(zip(('geom.xq', 'geom.wJ'), R.geom(*args, dtype=np.float32)))
  assert want['geom.wJ'].min() > 0
  got = dict(zip(('geom.xq', 'geom.wJ'), _ops.boundary_geom(
      dev(a['coords'], F32), dev(a['facets']), dev(a['B'], F32),
      dev(a['Dq'], F32), dev(a['w'], F32))))
  base = tolerance(F32, p1)
  for key in want:
    assert got[key].dtype == F32
    err = R.relerr(_np(got[key]), want[key])
    e_ref = R.relerr(ref32[key], want[key])
    tol = base if err < base else max(base, 4 * e_ref)
    print(f'BNDERR g real {key} ndim=3 p1={p1} q={q} fp32: err {err:.2e} '
          f'(bound {tol:.1e}) float32 reference {e_ref:.2e} max |D_q| '
          f'{np.abs(a["Dq"]).max():.0f}' + (' EXCEPTION' if err >= base
                                            else ''))
    assert err < tol, (key, p1, q, err, e_ref)
