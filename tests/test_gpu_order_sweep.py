"""The index-row Helmholtz kernels (`helmholtz_kernel<T, P, DIM, GS, SCALAR,
GM, SORTED, MASS, COEF>`, csrc/sfem_helmholtz.h) at every order P = 2..12, in
2D and 3D, in both precisions, against the sum-factorised float64 reference
(`tests/sumfact_reference.py`): constant operators on every geometry path and
field layout, coefficient operators in every coefficient form, the
element-local action and the assembled diagonal.

The mesh is `geometry_cases.three_kinds(3, ndim, P)`: 27 (9) elements of all
three geometry kinds, one launch with an `elem_list` per kind.  Tolerances:
`fp32util.tolerance` for the operators, the diagonal's own of
`test_gpu_jacobi.py` (1e-12 / 1e-5); relative errors are max-norm over the
whole vector.
"""
import functools

import numpy as np
import pytest
import torch

from swirl_fem_amd import _lib
from swirl_fem_amd.core import operators
from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import NodeType, Quadrature1D
from tests import geometry_cases as G
from tests import sumfact_reference as S
from tests.fp32util import F32Rng, f32_mesh, f32r, tolerance
from tests.packing import epb

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GLL = NodeType.GAUSS_LOBATTO_LEGENDRE
DIAG_TOL = {torch.float64: 1e-12, torch.float32: 1e-5}   # test_gpu_jacobi.py
LAMBDAS = ((0.0, 1.0), (0.6, 1.4), (1.0, 0.0))
COEF_LAMBDAS = ((0.0, 1.0), (0.7, 1.3))
DIAG_LAYER_FROM_P = 12      # 3D: the diagonal on one layer of elements
COEF_PAIRS = (('elem', 'elem'), ('point', 'point'), ('point', None),
              (None, 'point'), ('elem', 'point'))

# fp32 cases whose float32 REFERENCE ALGORITHM is itself beyond the policy
# (`sumfact_reference.Space(dtype=float32)` against its float64 self on the
# item's inputs): (ndim, P, section, operator) -> 2 x that reference's error.
# Both numbers of each entry are in profiles/order_sweep_fp32_errors.md.  The
# diagonal at P = 12 only: sum_q G_q D[q, i]^2 squares derivative-matrix
# entries of 1e2 that float32 holds to 6e-8 each.
FP32_EXCEPTIONS = {
    (2, 12, 'd', 'constant'): 2 * 1.075e-5,
    (2, 12, 'd', 'point'): 2 * 1.227e-5,
    (3, 12, 'd', 'constant'): 2 * 1.199e-5,
    (3, 12, 'd', 'point'): 2 * 1.208e-5,
}


def padding(ndim, P, itemsize=8):
  """All -1 element rows to append so that the last workgroup is a partial
  one.  By the rule above EPB is 32, 16, 16, 12, 10, 9, 8, 7, 6, 11, 16 for
  P = 2..12 in 2D and 16, 7, 4, 5, 1, ... in 3D (1 from P = 6 on), the same
  in both precisions: of those only 9 divides the element count (9 in 2D, 27
  in 3D), and no order gives 3.  So (ndim, P) = (2, 7) is the one padded
  mesh."""
  n = epb(ndim, P, itemsize)
  return 1 if n > 1 and 3 ** ndim % n == 0 else 0


def test_padded_orders_follow_the_packing_rule():
  padded = {(d, P) for d in (2, 3) for P in range(2, 13) for s in (4, 8)
            if padding(d, P, s)}
  assert padded == {(2, 7)}
  assert [epb(2, P, 8) for P in range(2, 13)] == [32, 16, 16, 12, 10, 9, 8, 7,
                                                  6, 11, 16]
  assert [epb(3, P, 4) for P in range(2, 13)] == [16, 7, 4, 5] + [1] * 7


def dev(a, dtype):
  return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def relerr(a, b):
  a = a.detach().cpu().numpy().astype(np.float64)
  assert a.shape == b.shape, (a.shape, b.shape)
  return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@functools.lru_cache(maxsize=None)
def premesh(ndim, P):
  return G.three_kinds(3, ndim, P, pad=padding(ndim, P))


@functools.lru_cache(maxsize=None)
def reference(ndim, P, dtype):
  """Everything the item compares with, computed once on the CPU: inputs
  (float32-representable in fp32) and the float64 reference results, the
  mass and the stiffness part apart (the operator is linear in l0, l1)."""
  case = premesh(ndim, P)
  rp = f32_mesh(case.rp, dtype)
  n = rp.elements.shape[1]
  el = np.concatenate([rp.elements, np.full((case.pad, n), -1, np.int32)])
  sf = S.Space(rp.node_coords, el, P)
  E, N = el.shape[0], rp.node_coords.shape[0]
  seed = 1000 * ndim + 10 * P
  rng = F32Rng(seed) if dtype == torch.float32 else np.random.default_rng(seed)
  rnd = f32r if dtype == torch.float32 else (lambda a: a)
  xq = sf.quad_points()
  r = dict(case=case, rp=rp, sf=sf, E=E, N=N, real=rp.elements.shape[0])
  r['u'] = rng.standard_normal((N, 6))       # scalar | 3 components | 2
  r['ul'] = rng.standard_normal((E, n))
  # per-element values all distinct; per-point values vary along one axis
  # only, another one for k than for c: a transposed point order fails
  x0, x1 = xq[..., 0], xq[..., ndim - 1]
  coef = {'k': {'elem': rnd(0.5 + rng.permutation(E) / E),
                'point': rnd(1.0 + x0 ** 2 + 0.5 * np.sin(3.0 * x0)),
                None: None},
          'c': {'elem': rnd(0.25 + rng.permutation(E) / E),
                'point': rnd(0.5 + x1 ** 2 + 0.4 * np.cos(2.0 * x1)),
                None: None}}
  r['coef'] = coef
  full = lambda v: (None if v is None else v if v.ndim == 2
                    else np.repeat(v[:, None], n, 1))
  r['M'] = sf.apply(r['u'], 1.0, 0.0)
  r['K'] = sf.apply(r['u'], 0.0, 1.0)
  u0 = r['u'][:, 0]
  r['Kk'] = {f: sf.apply(u0, 0.0, 1.0, k_q=full(v))
             for f, v in coef['k'].items()}
  r['Mc'] = {f: sf.apply(u0, 1.0, 0.0, c_q=full(v))
             for f, v in coef['c'].items()}
  kp, cp = coef['k']['point'], coef['c']['point']
  r['Ml'] = sf.local_apply(r['ul'], 1.0, 0.0)
  r['Kl'] = sf.local_apply(r['ul'], 0.0, 1.0)
  r['Mlc'] = sf.local_apply(r['ul'], 1.0, 0.0, c_q=cp)
  r['Klk'] = sf.local_apply(r['ul'], 0.0, 1.0, k_q=kp)
  # The diagonal applies the element operator to n unit vectors per element:
  # n^2 P work.  In 3D at P = 12 that is most of the item's time, so
  # there it is computed on the 9 elements of the layer x1 > 2/3, which holds
  # all three kinds, and compared on the nodes that only those elements touch.
  lay, nodes = None, np.ones(N, dtype=bool)
  if ndim == 3 and P >= DIAG_LAYER_FROM_P:
    centre = xq[:r["real"], :, 1].mean(axis=1)
    lay = np.nonzero(centre > 2.0 / 3)[0]
    assert len(lay) == 9
    rest = np.setdiff1d(np.arange(r['real']), lay)
    nodes = np.zeros(N, dtype=bool)
    nodes[rp.elements[lay].reshape(-1)] = True
    nodes[rp.elements[rest].reshape(-1)] = False
  r['diag_layer'], r['diag_nodes'] = lay, nodes
  r['dM'] = sf.diagonal(1.0, 0.0, elements=lay)
  r['dK'] = sf.diagonal(0.0, 1.0, elements=lay)
  r['dMc'] = sf.diagonal(1.0, 0.0, c_q=cp, elements=lay)
  r['dKk'] = sf.diagonal(0.0, 1.0, k_q=kp, elements=lay)
  for v in r.values():
    if isinstance(v, np.ndarray):
      v.setflags(write=False)
  return r


class Tally:
  """Largest error per section, and every miss (the item reports them all)."""

  def __init__(self, ndim, P, dtype):
    self.key = (ndim, P, 'fp64' if dtype == torch.float64 else 'fp32')
    self.worst, self.missed = {}, []

  def check(self, section, what, err, tol):
    if err > self.worst.get(section, (-1.0, None))[0]:
      self.worst[section] = (err, what)
    if not err <= tol:
      self.missed.append((section, what, '%.3g > %.3g' % (err, tol)))

  def report(self):
    for section in sorted(self.worst):
      err, what = self.worst[section]
      print('SWEEP %d %2d %s %s %.3e %s' % (self.key + (section, err, what)))


def check_kinds(case, op, P):
  """fp64 'auto' finds all three kinds; at P = 2 there is no high-order node
  to bend, so the first layers are multilinear and nothing is curved."""
  if P > 2:
    case.check_counts(op)
  else:
    assert (op.num_curved, op.num_affine > 0, op.num_multilinear > 0) == \
        (0, True, True)


def expected_names(op, real, P, ndim, mass, coef_mode):
  """The instantiations the coefficient operator must launch: GM = affine /
  multilinear with COEF, stored factors (coefficients folded in) without."""
  b = 'true' if mass else 'false'
  names = set()
  for part in op.parts:
    gm = part['geo_mode']
    if gm == G.CURVED:
      assert 'coef_mode' not in part and 'kappa' not in part
      names.add('sfem::helmholtz_kernel<%s, %d, %d, true, true, 0, false, %s>'
                % (real, P, ndim, b))
    else:
      assert part['coef_mode'] == coef_mode
      names.add('sfem::helmholtz_kernel<%s, %d, %d, true, true, %d, false, '
                '%s, %d>' % (real, P, ndim, gm, b, coef_mode))
  return ' + '.join(sorted(names))


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32],
                         ids=['fp64', 'fp32'])
@pytest.mark.parametrize('P', range(2, 13))
@pytest.mark.parametrize('ndim', [2, 3])
def test_order_sweep(ndim, P, dtype, monkeypatch):
  monkeypatch.setenv('SFEM_FACET', '0')
  r = reference(ndim, P, dtype)
  case = r['case']
  mesh, bm, _ = case.finalize(DEV, dtype)
  assert mesh.num_elements == r['E'] and mesh.num_nodes == r['N']
  assert np.array_equal(mesh.node_coords.double().cpu().numpy(),
                        r['rp'].node_coords)
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(P, GLL))
  keep = 1.0 - bm.double().cpu().numpy()
  tol = tolerance(dtype, P)
  dtol = DIAG_TOL[dtype]
  real = 'double' if dtype == torch.float64 else 'float'
  t = Tally(ndim, P, dtype)
  u = r['u']
  fields = (('scalar', dev(u[:, 0], dtype), slice(0, 1)),
            ('component-major', dev(u[:, 1:4].T, dtype).t(), slice(1, 4)),
            ('interleaved', dev(u[:, 4:6], dtype), slice(4, 6)))
  assert not fields[1][1].is_contiguous() and fields[2][1].is_contiguous()

  def want(name, l0, l1, cols):
    w = (l0 * r['M'][:, cols] + l1 * r['K'][:, cols]) * keep[:, None]
    return w[:, 0] if name == 'scalar' else w

  # ---- a. constant operator on index rows
  ops = {}
  for g in ('auto', 'multilinear', 'stored'):
    op = ops[g] = operators.HelmholtzOperator.create(fes, bm, g)
    assert op.facet_parts is None
    assert 'helmholtz_kernel<%s, %d, %d, true, true' % (real, P, ndim) in \
        op.kernel_name()
    if g == 'auto' and dtype == torch.float64:
      check_kinds(case, op, P)
    for l0, l1 in LAMBDAS:
      for name, ud, cols in fields:
        err = relerr(op.apply(ud, l0, l1), want(name, l0, l1, cols))
        t.check('a', (g, name, l0, l1), err, tol)
    # the fused u . A u
    ref = want('scalar', 0.0, 1.0, slice(0, 1))
    dot, scale = float(u[:, 0] @ ref), float(np.abs(u[:, 0] * ref).sum())
    parts = torch.zeros(_lib.SFEM_DOT_SLOTS, dtype=torch.float64, device=DEV)
    got = op.apply(fields[0][1], 0.0, 1.0, dot_out=parts)
    t.check('a', (g, 'dot_out field'), relerr(got, ref), tol)
    t.check('a.dot', (g, 'dot_out sum'),
            abs(float(parts.sum()) - dot) / scale, 10 * tol)

  # ---- b. coefficient operators
  u0 = fields[0][1]
  coef = r['coef']
  arg = lambda v: None if v is None else dev(v, dtype)
  colored = False
  for g in ('auto', 'multilinear'):
    for kf, cf in COEF_PAIRS:
      kw = dict(diffusivity=arg(coef['k'][kf]), reaction=arg(coef['c'][cf]))
      op = fes.helmholtz_operator(bm, g, **kw)
      assert isinstance(op, operators.HelmholtzOperator)
      assert op.facet_parts is None and op.layer_plan() is None
      if g == 'auto' and dtype == torch.float64:
        check_kinds(case, op, P)
      mode = (_lib.COEF_POINT if 'point' in (kf, cf) else _lib.COEF_ELEM)
      outs = {}
      for l0, l1 in COEF_LAMBDAS:
        assert op.kernel_name(l0, l1) == expected_names(
            op, real, P, ndim, l0 != 0, mode), (g, kf, cf, op.kernel_name(l0, l1))
        ref = (l0 * r['Mc'][cf] + l1 * r['Kk'][kf]) * keep
        outs[l0] = op.apply(u0, l0, l1)
        t.check('b', (g, kf, cf, l0, l1), relerr(outs[l0], ref), tol)
      if not colored and (kf, cf) == ('point', 'point'):
        # once per item: coloured assembly (no atomics) of the same operator
        colored = True
        col = fes.helmholtz_operator(bm, g, assembly='colored', **kw)
        assert all(p.get('colored') for p in col.parts)
        l0, l1 = COEF_LAMBDAS[1]
        ref = (l0 * r['Mc'][cf] + l1 * r['Kk'][kf]) * keep
        got = col.apply(u0, l0, l1)
        t.check('b', (g, 'colored'), relerr(got, ref), tol)
        t.check('b', (g, 'colored vs atomic'),
                relerr(got, outs[l0].double().cpu().numpy()), tol)
      if (kf, cf) == ('point', 'point') and g == 'auto':
        point_op = op
  assert colored

  # ---- c. apply_local (GS = false); padded elements hold nothing to compare
  rows = slice(0, r['real'])
  uld = dev(r['ul'], dtype)
  for l0, l1 in ((0.0, 1.0), (0.6, 1.4)):
    for name, op, Ml, Kl in (('constant', ops['auto'], r['Ml'], r['Kl']),
                             ('stored', ops['stored'], r['Ml'], r['Kl']),
                             ('point', point_op, r['Mlc'], r['Klk'])):
      got = op.apply_local(uld, l0, l1)
      assert got.shape == uld.shape
      err = relerr(got[rows], (l0 * Ml + l1 * Kl)[rows])
      t.check('c', (name, l0, l1), err, tol)

  # ---- d. the assembled diagonal
  at = r['diag_nodes']
  at_dev = torch.as_tensor(at, device=DEV)
  assert (at & (keep > 0)).sum() > 0
  if r['diag_layer'] is not None and dtype == torch.float64:
    for part in ops['auto'].parts:       # the layer holds every kind
      assert np.isin(part['elem_list'].cpu().numpy(), r['diag_layer']).any()
  for l0, l1 in ((0.0, 1.0), (0.7, 1.3), (1.0, 0.0)):
    for name, op, form, dM, dK in (
        ('constant', ops['auto'], 'constant', r['dM'], r['dK']),
        ('stored', ops['stored'], 'constant', r['dM'], r['dK']),
        ('point', point_op, 'point', r['dMc'], r['dKk'])):
      got = op.diagonal(l0, l1)
      assert float(got[bm].abs().max()) == 0.0
      ref = ((l0 * dM + l1 * dK) * keep)[at]
      bound = dtol
      if dtype == torch.float32:
        bound = FP32_EXCEPTIONS.get((ndim, P, 'd', form), dtol)
      t.check('d', (name, l0, l1), relerr(got[at_dev], ref), bound)

  t.report()
  assert not t.missed, t.missed
