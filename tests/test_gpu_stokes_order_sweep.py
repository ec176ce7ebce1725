"""The index-row Stokes kernels of `csrc/sfem_stokes.h` (`stokes_div_kernel`
plain and SECOND, `stokes_grad_t_kernel` and `stokes_e_first_kernel` sorted
and unsorted, `stokes_convect_kernel`) at every order P = 4..12, in 2D and 3D,
in both precisions, against the sum-factorised float64 reference
(`tests/sumfact_stokes_reference.py`; meshes, inputs and reference results:
`tests/stokes_sweep_cases.py`).

The meshes are velocity / pressure pairs on 3^ndim elements of all three
geometry kinds (two at P = 4), one launch with an `elem_list` per kind;
`SFEM_STOKES_FACET=0` keeps every launch on index rows.  Tolerances:
`fp32util.tolerance`, relative max-norm over the whole vector; an fp32 case
may take 2 x the float32 reference's own error where that reference is
beyond the policy on the item's inputs (`FP32_EXCEPTIONS`: none is).
"""
import numpy as np
import pytest
import torch

from swirl_fem_amd import _lib
from swirl_fem_amd.core import layout, operators
from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import Nodes1D, Quadrature1D
from tests import numbering_cases as NC
from tests import stokes_sweep_cases as C
from tests.fp32util import tolerance
from tests.test_gpu_order_sweep import Tally

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64, F32 = torch.float64, torch.float32
POINT, AFFINE, MULTI = 0, 1, 3                  # operators._GEO_* codes
KINDS = {'three_kinds': {AFFINE, MULTI, POINT}, 'vertex': {AFFINE, MULTI}}
GEOMETRIES = ('auto', 'multilinear', 'stored')

# fp32 cases whose float32 REFERENCE ALGORITHM is itself beyond the policy
# (`stokes_sweep_cases.f32_reference_errors`: `sumfact_stokes_reference` in
# float32 against its float64 self on the item's inputs): (ndim, P, section)
# -> 2 x that reference's error.  None needed: the float32 reference is
# within 1e-5 on every item (worst 9.7e-6, convection, 2D, P = 12, where the
# policy is 2e-5); profiles/order_sweep_fp32_errors.md has the numbers.
FP32_EXCEPTIONS = {}


def dev(a, dtype):
  return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _np(t):
  return t.detach().double().cpu().numpy()


def relerr(a, b):
  a = _np(a) if isinstance(a, torch.Tensor) else np.asarray(a)
  assert a.shape == b.shape, (a.shape, b.shape)
  return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def launch_counts(parts, E):
  return [int(q['elem_list'].numel()) if 'elem_list' in q else E
          for q in parts]


def expected_kinds(geometry, name):
  kinds = KINDS[name]
  if geometry == 'stored':
    return {POINT}
  if geometry == 'multilinear':
    return {MULTI if k == AFFINE else k for k in kinds}
  return kinds


@pytest.mark.parametrize('dtype', [F64, F32], ids=['fp64', 'fp32'])
@pytest.mark.parametrize('P', range(4, 13))
@pytest.mark.parametrize('ndim', [2, 3])
def test_stokes_order_sweep(ndim, P, dtype, monkeypatch):
  monkeypatch.setenv('SFEM_STOKES_FACET', '0')
  monkeypatch.delenv('SFEM_SORTED_SCATTER', raising=False)
  f32 = dtype == F32
  r = C.reference(ndim, P, f32)
  ref, c, c2 = r['ref'], r['pair'], r['pair2']
  assert c.geometry == ('three_kinds' if P >= 5 else 'vertex')
  vsp, psp = NC.stokes_spaces(c, DEV, dtype)
  mesh = vsp.mesh
  E, N, Np = mesh.num_elements, r['N'], r['Np']
  assert (E, mesh.num_nodes, psp.mesh.num_nodes) == (3 ** ndim, N, Np)
  assert np.array_equal(_np(mesh.node_coords), c.v.rp.node_coords)
  tol = tolerance(dtype, P)
  bound = lambda s: FP32_EXCEPTIONS.get((ndim, P, s), tol) if f32 else tol
  sorting = ndim == 3 and P <= 8
  t = Tally(ndim, P, dtype)
  counts = set()

  bm = r['bm']
  keep = (~bm)[:, None]
  u, p, sc, s1 = r['u'], r['p'], r['sc'], r['s1']
  ud, pd = dev(u, dtype), dev(p, dtype)
  ucm = layout.component_major(ud)
  assert ud.is_contiguous() and layout.is_component_major(ucm)
  scales = {None: None, 's1': dev(s1, dtype), 'sc': dev(sc, dtype)}
  factor = {None: 1.0, 's1': s1[:, None], 'sc': sc}
  g_free = ref['grad_t']
  pnorm = float(np.linalg.norm(p))

  def create(geometry, mask, pspace=psp):
    op = operators.StokesDivGrad.create(
        vsp, pspace, None if mask is None else dev(mask, torch.bool), geometry)
    assert op.facet_parts is None
    counts.update(launch_counts(op.parts, E))
    if not f32:
      assert {q['geo_mode'] for q in op.parts} == expected_kinds(
          geometry, c.geometry), (geometry, op.parts)
      if geometry == 'auto':
        assert set(launch_counts(op.parts, E)) == {
            n for n in C.expected_kind_counts(ndim, P).values() if n}
    return op

  for geometry in GEOMETRIES:
    for mask in (bm, None):
      m = 'masked' if mask is not None else 'free'
      fused = create(geometry, mask)
      assert fused.penc is None
      assert (fused.shared_order is not None) == sorting
      # ---- a. div (the mask does not enter it)
      for form, sd in scales.items():
        for name, field in (('interleaved', ud), ('component-major', ucm)):
          t.check('a', (geometry, m, form, name),
                  relerr(fused.div(field, scale=sd), ref['div'][form]),
                  bound('a'))
      for name, field in (('interleaved', ud), ('component-major', ucm)):
        want = ref['div']['s1']
        dots = torch.zeros(_lib.SFEM_DOT_SLOTS, dtype=F64, device=DEV)
        got = fused.div(field, scale=scales['s1'], dot_with=pd, dot_out=dots)
        t.check('a', (geometry, m, 'dot_out field', name), relerr(got, want),
                bound('a'))
        t.check('a.dot', (geometry, m, name),
                abs(float(dots.sum()) - float(p @ want)) /
                (pnorm * float(np.linalg.norm(want))), tol)
      # ---- b. grad_t
      g_want = g_free * keep if mask is not None else g_free
      ops = [('default', fused)]
      if sorting:
        monkeypatch.setenv('SFEM_SORTED_SCATTER', '0')
        plain = create(geometry, mask)
        monkeypatch.delenv('SFEM_SORTED_SCATTER')
        assert plain.shared_order is None
        ops.append(('unsorted', plain))
      outs = {}
      for scatter, op in ops:
        for form, sd in scales.items():
          for cm in (False, True):
            got = op.grad_t(pd, component_major=cm, scale=sd)
            assert layout.is_component_major(got) == cm
            outs[scatter, form, cm] = got
            t.check('b', (geometry, m, scatter, form, cm),
                    relerr(got, factor[form] * g_want), bound('b'))
      if sorting:
        for (scatter, form, cm), got in outs.items():
          if scatter == 'unsorted':
            t.check('b', (geometry, m, 'sorted vs unsorted', form, cm),
                    relerr(outs['default', form, cm], _np(got)), bound('b'))
      # ---- c. adjointness of the unmasked pair
      if mask is None:
        size = float(np.linalg.norm(u) * np.linalg.norm(g_free))
        for field, cm in ((ud, False), (ucm, True)):
          lhs = float((fused.div(field).double() * pd.double()).sum())
          rhs = float((fused.grad_t(pd, component_major=cm).double() *
                       ud.double()).sum())
          t.check('c', (geometry, cm), abs(lhs - rhs) / size, tol)
      # ---- e. E = D scale mask D^T on every route
      if mask is not None:
        assert fused.supports_layered_e()
        for form, sd in scales.items():
          want = ref['E'][form]
          got = {'e_apply': fused.e_apply(pd, scale=sd),
                 'e_layered': fused.e_layered(pd, scale=sd),
                 'two kernels': fused.div(
                     fused.grad_t(pd, component_major=True), scale=sd)}
          if sorting:
            # (the split encoding takes its order when it is first built)
            monkeypatch.setenv('SFEM_SORTED_SCATTER', '0')
            got['e_apply unsorted'] = ops[1][1].e_apply(pd, scale=sd)
            monkeypatch.delenv('SFEM_SORTED_SCATTER')
            assert ops[1][1]._split[2] is None and fused._split[2] is not None
          else:
            assert fused._split[2] is None
          for route, val in got.items():
            t.check('e', (geometry, route, form), relerr(val, want), bound('e'))
          first = _np(got['e_apply'])
          for route, val in got.items():
            if route != 'e_apply':
              t.check('e', (geometry, 'e_apply vs ' + route, form),
                      relerr(val, first), bound('e'))

  # ---- d. a second pair with random pressure numbering: penc given
  psp2 = FiniteElementSpace.create(
      c2.p.rp.finalize(device=DEV, dtype=dtype), Quadrature1D.create(P, NC.GLL))
  p2d = dev(r['p2'], dtype)
  for mask in (bm, None):
    fused = create('auto', mask, psp2)
    assert fused.penc is not None
    assert (fused.shared_order is not None) == sorting
    for name, field in (('interleaved', ud), ('component-major', ucm)):
      t.check('d', ('div', name), relerr(fused.div(field), ref['div2']),
              bound('d'))
    g_want = ref['grad_t2'] * keep if mask is not None else ref['grad_t2']
    for cm in (False, True):
      t.check('d', ('grad_t', mask is not None, cm),
              relerr(fused.grad_t(p2d, component_major=cm), g_want), bound('d'))

  # ---- f. convection on q = P GLL points
  quad = Quadrature1D.create_from_nodes_1d(Nodes1D.create(P, NC.GLL))
  orp = r['orp']
  over = FiniteElementSpace.create(orp.finalize(device=DEV, dtype=dtype), quad)
  assert vsp.is_collocated and not over.is_collocated
  assert over.mesh.gridpoints_1d.num_points == P - 2
  assert over.mesh.num_elements == E
  for name, fes, ul, want in (('collocated', vsp, r['ul'], ref['conv']),
                              ('over-integrated', over, r['ul_over'],
                               ref['conv_over'])):
    for geometry in ('auto', 'stored'):
      op = operators.ConvectionOperator.create(fes, geometry)
      counts.update(launch_counts(op.parts, E))
      if not f32:
        assert {q['geo_mode'] for q in op.parts} == expected_kinds(
            geometry, c.geometry), (name, geometry)
      got = op.apply_local(dev(ul, dtype))
      t.check('f', (name, geometry), relerr(got, want), bound('f'))

  # ---- packing of the launches this item made
  C.check_packing(ndim, P, 8 if dtype == F64 else 4, counts)
  if not f32:
    assert counts == C.expected_launch_counts(ndim, P), counts

  t.report()
  assert not t.missed, t.missed
