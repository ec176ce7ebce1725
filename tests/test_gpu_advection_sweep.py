"""The FORWARD advective Helmholtz kernels (`helmholtz_adv_kernel<T, P, DIM,
GS, GM, TR = false>`, csrc/sfem_helmholtz_adv.h) at every order P = 2..12, in
2D and 3D, in both precisions, against the factored float64 NumPy reference
(`tests/adjoint_reference.py`: `apply`, `local_apply`): the assembled apply on
every geometry path, in every coefficient form, masked and unmasked, atomic
and coloured; the advective term alone; the element-local action; the
assembled diagonal (`tests/advection_reference.py`).  The transposed
instantiations are swept by `test_gpu_adjoint.py`.

The mesh is `geometry_cases.three_kinds(3, ndim, P)`: 27 (9) elements of all
three geometry kinds.  The kernels take their tile from `HelmholtzTile<T, P,
DIM>`, so by the packing rule of `test_gpu_order_sweep.padding` (ndim, P) =
(2, 7) is the one mesh whose element count the workgroup size divides; there
one all -1 row is appended and the last workgroup is partial.  The operator
accepts the padded row (nothing of it is scattered); the reference space is
built on the real elements, the padded row's inputs are ones.

Tolerances: fp64 1e-11, the bound of the forward and transposed advection
tests; fp32 `fp32util.tolerance`; the diagonal 1e-12 / 1e-5 of
`test_gpu_jacobi.py`.  Relative errors are max-norm over the whole vector.
The observed errors are recorded in profiles/advection_sweep_errors.md.
"""
import functools

import numpy as np
import pytest
import torch

from swirl_fem_amd.core import operators
from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import NodeType, Quadrature1D
from tests import adjoint_reference as AJ
from tests import advection_reference as AR
from tests import geometry_cases as G
from tests.fp32util import F32Rng, f32_mesh, f32r, tolerance
from tests.test_gpu_advection import _field_np
from tests.test_gpu_order_sweep import check_kinds, dev, padding, relerr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GLL = NodeType.GAUSS_LOBATTO_LEGENDRE
F64, F32 = torch.float64, torch.float32
DIAG_TOL = {F64: 1e-12, F32: 1e-5}                       # test_gpu_jacobi.py
GEOMETRIES = ('auto', 'multilinear', 'stored')
FORMS = (('point', 'elem'), ('point', None), (None, 'point'), (None, None))
LAMBDAS = ((0.7, 1.3), (0.0, 1.3), (0.7, 0.0))
# `advection_reference.diagonal` holds (E, Q, n, d) gradients: beyond this
# many bytes (3D from P = 7 on) the collocated closed form stands in, which
# tests/test_advection_host.py pins to it
DENSE_DIAGONAL_BYTES = 64 << 20

# fp32 cases beyond the policy where the float32-evaluated reference is too:
# (ndim, P, section) -> 2 x that reference's error on the item's inputs, both
# numbers in profiles/advection_sweep_errors.md
# (scripts/advection_sweep_fp32.py evaluates the reference in float32).  The
# diagonal at P = 12 only, as in `test_gpu_order_sweep.FP32_EXCEPTIONS` and
# for its reason: sum_q G_q D[q, i]^2 squares derivative-matrix entries of
# 1e2 that float32 holds to 6e-8 each.
FP32_EXCEPTIONS = {
    (2, 12, 'd'): 2 * 1.961e-5,
    (3, 12, 'd'): 2 * 1.906e-5,
}


def tol_of(dtype, P):
  return 1e-11 if dtype == F64 else tolerance(F32, P)


def test_the_padded_order_follows_the_tile_of_the_advective_kernels():
  # HelmholtzTile<T, P, DIM>, the tile of helmholtz_kernel: the same rule
  assert {(d, P) for d in (2, 3) for P in range(2, 13) for s in (4, 8)
          if padding(d, P, s)} == {(2, 7)}


@functools.lru_cache(maxsize=None)
def premesh(ndim, P):
  return G.three_kinds(3, ndim, P, pad=padding(ndim, P))


def one_component(xq, P):
  """Only component j = P % ndim is non-zero, and varies along the next
  axis: a transposed point or component order fails."""
  ndim = xq.shape[-1]
  j = P % ndim
  b = np.zeros(xq.shape)
  b[..., j] = 1.0 + 4.0 * xq[..., (j + 1) % ndim] ** 2
  return b


@functools.lru_cache(maxsize=None)
def reference(ndim, P, dtype):
  """Everything the item compares with, computed once on the CPU: inputs
  (float32-representable in fp32; the rows of a padded element hold ones) and
  the float64 reference results, term by term -- the operator is linear in
  l0, l1 and has the advective term added unscaled.  The reference space
  (71 MB of gradients in 3D at P = 12) is dropped."""
  case = premesh(ndim, P)
  rp = f32_mesh(case.rp, dtype)
  fes = AJ.space(rp.node_coords, rp.elements, P, (P, 'gll'))
  real, n = rp.elements.shape
  E, N = real + case.pad, rp.node_coords.shape[0]
  seed = 2000 * ndim + 10 * P
  rng = F32Rng(seed) if dtype == F32 else np.random.default_rng(seed)
  rnd = f32r if dtype == F32 else (lambda a: a)
  xq = AJ.quad_points(fes)
  x0, x1 = xq[..., 0], xq[..., ndim - 1]
  r = dict(case=case, rp=rp, E=E, N=N, real=real)
  u = r['u'] = rng.standard_normal(N)
  ul = r['ul'] = rng.standard_normal((E, n))
  # per-element values all distinct, per-point values along one axis only
  sig = rnd(0.25 + rng.permutation(E) / E)
  r['b'] = rnd(_field_np(xq))
  r['b1'] = rnd(one_component(xq, P))
  r['k'] = {'point': rnd(1.0 + x0 ** 2 + 0.5 * np.sin(3.0 * x0)), None: None}
  r['c'] = {'point': rnd(0.5 + x1 ** 2 + 0.4 * np.cos(2.0 * x1)),
            'elem': sig, None: None}
  cq = {f: (None if v is None else AJ.expand_coefficient(v[:real], real, n))
        for f, v in r['c'].items()}
  kq = r['k']
  b, b1, uloc = r['b'], r['b1'], ul[:real]
  r['M'] = {f: AJ.apply(fes, u, 1.0, 0.0, c_q=v) for f, v in cq.items()}
  r['K'] = {f: AJ.apply(fes, u, 0.0, 1.0, k_q=v) for f, v in kq.items()}
  r['C'] = AJ.apply(fes, u, 0.0, 0.0, b_q=b)
  r['C1'] = AJ.apply(fes, u, 0.0, 0.0, b_q=b1)
  some = (None, 'elem')
  r['Ml'] = {f: AJ.local_apply(fes, uloc, 1.0, 0.0, c_q=cq[f]) for f in some}
  r['Kl'] = {f: AJ.local_apply(fes, uloc, 0.0, 1.0, k_q=kq[f])
             for f in (None, 'point')}
  r['Cl'] = AJ.local_apply(fes, uloc, 0.0, 0.0, b_q=b)
  dense = real * n * n * ndim * 8 <= DENSE_DIAGONAL_BYTES
  diag = AR.diagonal if dense else AR.collocated_diagonal
  r['diag_form'] = 'diagonal' if dense else 'collocated_diagonal'
  r['dM'] = {f: diag(fes, 1.0, 0.0, c_q=cq[f]) for f in some}
  r['dK'] = {f: diag(fes, 0.0, 1.0, k_q=kq[f]) for f in (None, 'point')}
  r['dC'] = diag(fes, 0.0, 0.0, b_q=b)

  def device_rows(v):       # (real, ...) -> (E, ...): ones in a padded row
    return np.concatenate([v, np.ones((case.pad,) + v.shape[1:])])
  for key in ('b', 'b1'):
    r[key] = device_rows(r[key])
  r['k']['point'] = device_rows(r['k']['point'])
  r['c']['point'] = device_rows(r['c']['point'])
  for v in r.values():
    for a in (v.values() if isinstance(v, dict) else (v,)):
      if isinstance(a, np.ndarray):
        a.setflags(write=False)
  return r


class Tally:
  """Largest error per section, and every miss (the item reports them all)."""

  def __init__(self, ndim, P, dtype):
    self.key = (ndim, P, 'fp64' if dtype == F64 else 'fp32')
    self.worst, self.missed = {}, []

  def check(self, section, what, err, tol):
    if not err <= self.worst.get(section, (-1.0, None))[0]:
      self.worst[section] = (err, what)
    if not err <= tol:
      self.missed.append((section, what, '%.3g > %.3g' % (err, tol)))

  def report(self):
    for section in sorted(self.worst):
      err, what = self.worst[section]
      print('ADVSWEEP %d %2d %s %s %.3e %s' % (self.key + (section, err,
                                                           what)))
    for section, what, how in self.missed:
      print('ADVSWEEP-MISS %d %2d %s %s %s %s' % (self.key + (section, what,
                                                              how)))


@pytest.mark.parametrize('dtype', [F64, F32], ids=['fp64', 'fp32'])
@pytest.mark.parametrize('P', range(2, 13))
@pytest.mark.parametrize('ndim', [2, 3])
def test_advection_sweep(ndim, P, dtype):
  r = reference(ndim, P, dtype)
  case = r['case']
  mesh, bm, _ = case.finalize(DEV, dtype)
  assert mesh.num_elements == r['E'] and mesh.num_nodes == r['N']
  assert np.array_equal(mesh.node_coords.double().cpu().numpy(),
                        r['rp'].node_coords)
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(P, GLL))
  keep = 1.0 - bm.double().cpu().numpy()
  tol, dtol = tol_of(dtype, P), DIAG_TOL[dtype]
  t = Tally(ndim, P, dtype)
  if dtype == F32:
    check = t.check
    t.check = lambda section, what, err, bound: check(
        section, what, err, FP32_EXCEPTIONS.get((ndim, P, section), bound))
  arg = lambda v: None if v is None else dev(v, dtype)
  ud, bd = dev(r['u'], dtype), dev(r['b'], dtype)

  def want(kf, cf, l0, l1, mask=True, C='C'):
    w = l0 * r['M'][cf] + l1 * r['K'][kf] + r[C]
    return w * keep if mask else w

  def make(mask, g, kf, cf, assembly='auto', b=bd):
    op = fes.helmholtz_operator(mask, g, assembly, diffusivity=arg(r['k'][kf]),
                                reaction=arg(r['c'][cf]), velocity=b)
    assert isinstance(op, operators.HelmholtzOperator)
    assert op.facet_parts is None and op.layer_plan() is None
    return op

  # ---- a. the assembled forward apply
  ops = {}
  for g in GEOMETRIES:
    for kf, cf in FORMS:
      op = ops[g, kf, cf] = make(bm, g, kf, cf)
      if dtype == F64:
        if g == 'auto':
          check_kinds(case, op, P)
        for l0, l1 in LAMBDAS:
          assert 'helmholtz_adv_kernel<double, %d, %d, true' % (P, ndim) in \
              op.kernel_name(l0, l1)
      for l0, l1 in LAMBDAS:
        err = relerr(op.apply(ud, l0, l1), want(kf, cf, l0, l1))
        t.check('a', (g, kf, cf, l0, l1), err, tol)
    kf, cf = FORMS[0]
    op = make(None, g, kf, cf)
    for l0, l1 in LAMBDAS:
      err = relerr(op.apply(ud, l0, l1), want(kf, cf, l0, l1, mask=False))
      t.check('a', (g, 'unmasked', l0, l1), err, tol)
  # once per item: coloured assembly (no atomics) of the same operator
  kf, cf = FORMS[0]
  col = make(bm, 'auto', kf, cf, assembly='colored')
  assert all(p.get('colored') for p in col.parts)
  l0, l1 = LAMBDAS[0]
  got = col.apply(ud, l0, l1)
  atomic = ops['auto', kf, cf].apply(ud, l0, l1).double().cpu().numpy()
  t.check('a', ('auto', 'colored'), relerr(got, want(kf, cf, l0, l1)), tol)
  t.check('a.colored', ('auto', 'colored vs atomic'), relerr(got, atomic),
          1e-13 if dtype == F64 else tol)

  # ---- b. the term alone: one component, one axis, both lambdas zero
  for g in ('auto', 'stored'):
    op = make(None, g, None, None, b=dev(r['b1'], dtype))
    err = relerr(op.apply(ud, 0.0, 0.0), r['C1'])
    t.check('b', (g, 'component %d' % (P % ndim)), err, tol)

  # ---- c. apply_local (GS = false); a padded element holds nothing to compare
  rows = slice(0, r['real'])
  uld = dev(r['ul'], dtype)
  for g in ('auto', 'stored'):
    for kf, cf in (('point', 'elem'), (None, None)):
      op = ops[g, kf, cf]
      for l0, l1 in LAMBDAS:
        got = op.apply_local(uld, l0, l1)
        assert got.shape == uld.shape
        ref = l0 * r['Ml'][cf] + l1 * r['Kl'][kf] + r['Cl']
        t.check('c', (g, kf, cf, l0, l1), relerr(got[rows], ref), tol)

  # ---- d. the assembled diagonal with its advective part
  for g, kf, cf in (('auto', 'point', 'elem'), ('auto', None, None),
                    ('stored', 'point', 'elem')):
    op = ops[g, kf, cf]
    for l0, l1 in LAMBDAS:
      got = op.diagonal(l0, l1)
      assert float(got[bm].abs().max()) == 0.0
      ref = (l0 * r['dM'][cf] + l1 * r['dK'][kf] + r['dC']) * keep
      t.check('d', (g, kf, cf, l0, l1, r['diag_form']), relerr(got, ref),
              dtol)

  t.report()
  assert not t.missed, t.missed
