"""Every assembly path of the fused Helmholtz apply against the fp64 oracle on
meshes that mix geometry kinds (`tests/geometry_cases.py`).

An operator launches one element list per geometry kind, so the order of the
launches across kinds only matters on mixed meshes: coloured assembly stores
a node's first toucher and adds the others, and had run an affine element of
a late colour before the multilinear element that first touches a shared
node (finite, silently wrong).  Each case below picks one assembly path
(atomic sorted / unsorted, cluster, coloured, facet table with and without
chains, layered), one geometry argument, a mesh, an order and a precision,
chosen so that the cases together reach every instantiation and launch path;
each runs the three (lambda0, lambda1) kinds of kernel, scalar, row-major
and component-major fields, with and without a Dirichlet mask.  Needs a real
MI355X."""
import numpy as np
import pytest
import torch

from oracle import sfem_oracle as O
from swirl_fem_amd import _lib, _ops
from swirl_fem_amd.core import operators
from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import Quadrature1D
from tests import geometry_cases as G
from tests.fp32util import F32Rng, tolerance

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64, F32 = torch.float64, torch.float32
LAMBDAS = ((0.0, 1.0), (0.6, 1.2), (1.0, 0.0))

# (id, mesh builder and arguments (n, ndim, P), assembly, geometry, dtype)
CASES = [
    # coloured: one launch per (colour, kind); mixed kinds are the hard part
    ('colored-block-p5', G.block_jitter, (4, 3, 5), 'colored', 'auto', F64),
    ('colored-block-p9', G.block_jitter, (4, 3, 9), 'colored', 'auto', F64),
    ('colored-three-p4-f32', G.three_kinds, (3, 3, 4), 'colored', 'auto', F32),
    ('colored-three-p8-ml', G.three_kinds, (3, 3, 8), 'colored',
     'multilinear', F64),
    ('colored-vertex-2d-p3', G.vertex, (4, 2, 3), 'colored', 'auto', F64),
    ('colored-three-2d-p12-f32', G.three_kinds, (4, 2, 12), 'colored', 'auto',
     F32),
    ('colored-scrambled-p5', G.block_jitter, (3, 3, 5, True), 'colored',
     'auto', F64),
    ('colored-padded-p4', G.three_kinds, (3, 3, 4, 3), 'colored', 'auto',
     F64),
    ('colored-periodic-p5-stored', G.periodic, (3, 3, 5), 'colored', 'stored',
     F64),
    # atomic on index rows: sorted shared slots (3D, P <= 8) or not
    ('atomic-three-p5', G.three_kinds, (3, 3, 5), 'atomic', 'auto', F64),
    ('atomic-block-p4-f32', G.block_jitter, (3, 3, 4), 'atomic', 'auto', F32),
    ('unsorted-block-p4-f32', G.block_jitter, (3, 3, 4), 'unsorted', 'auto',
     F32),
    ('unsorted-three-p5', G.three_kinds, (3, 3, 5), 'unsorted', 'multilinear',
     F64),
    ('atomic-scrambled-p9', G.block_jitter, (3, 3, 9, True), 'atomic', 'auto',
     F64),
    ('atomic-padded-p5-f32', G.three_kinds, (3, 3, 5, 3), 'atomic', 'stored',
     F32),
    ('atomic-curved-2d-p8', G.curved_multilinear, (4, 2, 8), 'atomic', 'auto',
     F64),
    ('atomic-vertex-2d-p2-f32', G.vertex, (4, 2, 2), 'atomic', 'multilinear',
     F32),
    ('atomic-periodic-2d-p5', G.periodic, (4, 2, 5), 'atomic', 'auto', F64),
    # cluster (3D, P = 4..8)
    ('cluster-block-p5', G.block_jitter, (4, 3, 5), 'cluster', 'auto', F64),
    ('cluster-three-p8-f32', G.three_kinds, (3, 3, 8), 'cluster', 'auto', F32),
    ('cluster-scrambled-p4-stored', G.block_jitter, (3, 3, 4, True),
     'cluster', 'stored', F64),
    # facet tables (3D, P = 6..12), chained and not
    ('facet-three-p6', G.three_kinds, (3, 3, 6), 'facet', 'auto', F64),
    ('facet-block-p8-f32', G.block_jitter, (4, 3, 8), 'facet', 'auto', F32),
    ('nochain-scrambled-p7', G.block_jitter, (3, 3, 7, True), 'nochain',
     'auto', F64),
    ('nochain-three-p12-f32', G.three_kinds, (3, 3, 12), 'nochain', 'auto',
     F32),
    ('nochain-periodic-p9-ml', G.periodic, (3, 3, 9), 'nochain',
     'multilinear', F64),
    # layered (facet launches, plain stores into layers, folded)
    ('layered-three-p6', G.three_kinds, (3, 3, 6), 'layered', 'auto', F64),
    ('layered-affcurved-p9-f32', G.affine_curved, (3, 3, 9), 'layered',
     'auto', F32),
    ('layered-periodic-p8-stored', G.periodic, (3, 3, 8), 'layered', 'stored',
     F64),
]


def _np(t):
  return t.detach().double().cpu().numpy()


def _relerr(a, b):
  return np.abs(_np(a) - b).max() / max(np.abs(b).max(), 1e-300)


def _oracle_parts(ofes, u):
  """(B u, A u) of the fp64 oracle, assembled, one component at a time."""
  cols = [u] if u.ndim == 1 else [u[:, k] for k in range(u.shape[1])]
  parts = []
  for f in (ofes.mass_local, ofes.stiffness_local):
    out = [ofes.scatter(f(ofes.gather(c))) for c in cols]
    parts.append(out[0] if u.ndim == 1 else np.stack(out, axis=-1))
  return parts


# switches of each path, set for the whole test (they are read at setup)
# (meshes this small get no chains by default: `chain_segment_length`)
ENV = {'atomic': {'SFEM_FACET': '0'},
       'unsorted': {'SFEM_FACET': '0', 'SFEM_SORTED_SCATTER': '0'},
       'facet': {'SFEM_CHAIN_LEN': '3'},
       'nochain': {'SFEM_CHAIN': '0'},
       'layered': {'SFEM_CHAIN_LEN': '2'}}


def _create(fes, mask, geometry, path):
  assembly = path if path in ('cluster', 'colored') else 'atomic'
  op = operators.HelmholtzOperator.create(fes, mask, geometry, assembly)
  P = fes.mesh.gridpoints_1d.num_points
  sorted_parts = [p.get('shared_order') is not None for p in op.parts]
  if path == 'colored':
    assert all(p.get('colored') for p in op.parts)
    assert op.facet_parts is None
  if path == 'cluster':
    assert all(p.get('cluster') is not None for p in op.parts)
  if path in ('atomic', 'unsorted'):
    assert op.facet_parts is None
    sort = path == 'atomic' and fes.mesh.ndim == 3 and P <= 8
    assert all(s == sort for s in sorted_parts), (path, sorted_parts)
  if path in ('facet', 'nochain', 'layered'):
    assert op.facet_parts is not None
    chained = [('chains' in q) for q in op.facet_parts]
    if path == 'nochain' or P > 8:
      assert not any(chained)
    else:
      assert any(chained)
  if path == 'layered':
    assert op.layer_plan() is not None
  return op


def _fields(rng, N, dtype, path):
  """[(name, host array (N,) or (N, 3), device tensor)]."""
  u1 = rng.standard_normal(N)
  out = [('scalar', u1, torch.as_tensor(u1, device=DEV, dtype=dtype))]
  if path != 'layered':
    u3 = rng.standard_normal((N, 3))
    out.append(('rows', u3, torch.as_tensor(u3, device=DEV,
                                            dtype=dtype).contiguous()))
    out.append(('components', u3, torch.as_tensor(
        np.ascontiguousarray(u3.T), device=DEV, dtype=dtype).t()))
  return out


def _apply(op, ud, l0, l1, path, rng, dot):
  N = op.fespace.mesh.num_nodes
  if path == 'layered':
    ext = op.new_extended()
    op.apply_layered(ud, ext, l0, l1, dot_out=dot)
    return _ops.fold_layers(ext, N, op.layer_plan().layers)
  # finite garbage in the output: every entry must be written
  garbage = torch.as_tensor(1e3 * rng.standard_normal(tuple(ud.shape)),
                            device=DEV, dtype=ud.dtype)
  out = torch.empty_like(ud)          # same (dense) layout as u
  out.copy_(garbage)
  got = op.apply(ud, l0, l1, out=out, dot_out=dot)
  assert got.data_ptr() == out.data_ptr()
  return got


@pytest.mark.parametrize('cid,build,args,path,geometry,dtype', CASES,
                         ids=[c[0] for c in CASES])
def test_assembly_path_matches_oracle(cid, build, args, path, geometry, dtype,
                                      monkeypatch):
  n, ndim, P = args[:3]
  for k, v in ENV.get(path, {}).items():
    monkeypatch.setenv(k, v)
  case = build(*args)
  mesh, bm, rp = case.finalize(DEV, dtype)
  fes = FiniteElementSpace.create(
      mesh, Quadrature1D.create_from_nodes_1d(rp.gridpoints_1d))
  ofes = O.FESpace(rp.node_coords, rp.elements, (P, 'gll'), (P, 'gll'))
  tol = tolerance(dtype, P)
  N = mesh.num_nodes
  rng = F32Rng(len(cid) * 31 + P)
  masks = [None] if bm is None else [bm, None]
  fields = _fields(rng, N, dtype, path)
  oracle = {id(u): _oracle_parts(ofes, u) for _, u, _ in fields}
  for mask in masks:
    op = _create(fes, mask, geometry, path)
    # the case is the geometry mix it claims to be
    E = mesh.num_elements
    assert op.num_affine + op.num_multilinear + op.num_curved == E
    if geometry == 'stored':
      assert op.num_curved == E
    elif dtype == F64 and geometry == 'auto':
      case.check_counts(op)
    elif geometry == 'auto' and case.mixed:
      assert sum(1 for v in (op.num_affine, op.num_multilinear,
                             op.num_curved) if v) >= 2, cid
    if geometry == 'multilinear':
      assert op.num_affine == 0
    keep = None if mask is None else 1.0 - _np(mask)
    for name, u, ud in fields:
      bu, au = oracle[id(u)]
      for l0, l1 in LAMBDAS:
        ref = l0 * bu + l1 * au
        if keep is not None:
          ref = ref * (keep if ref.ndim == 1 else keep[:, None])
        dot = torch.zeros(_lib.SFEM_DOT_SLOTS, dtype=torch.float64,
                          device=DEV)
        got = _apply(op, ud, l0, l1, path, rng, dot)
        what = (cid, mask is not None, name, l0, l1)
        assert tuple(got.shape) == ref.shape, what
        err = _relerr(got, ref)
        assert err < tol, what + (err,)
        # u . (mask * A u): the Dirichlet rows of `ref` are zero already
        want, scale = float((u * ref).sum()), float(np.abs(u * ref).sum())
        assert abs(float(dot.sum()) - want) <= 10 * tol * scale, what
        if path in ('colored', 'layered'):
          again = _apply(op, ud, l0, l1, path, rng, None)
          assert torch.equal(got, again), what


# ---------------------------------------------------------------------------
# One launch list per geometry kind, the same for every operator of a mesh
# ---------------------------------------------------------------------------
# name -> key of the per-point data of its curved launches
LAUNCH_DATA = {'helmholtz': 'geo', 'two_grid': 'geo', 'stokes': 'kfac',
               'convection': 'kfac', 'transport': 'kfac'}


def _launch_lists(mesh_kind, ndim, geometry):
  """({operator: parts}, E) of the five operators that launch once per
  geometry kind, on one mesh: the collocated Helmholtz operator with atomic
  assembly, and the two-grid Helmholtz, convection and transport operators on
  4 Gauss points per direction.  'three_kinds_padded' is the padded mixed mesh
  at 3 points per direction; the Stokes pair needs P >= 4 and a pressure mesh
  that holds the same geometry, so it joins on 'stokes_pair', the velocity mesh
  of the smallest curved P_N - P_{N-2} pair (`numbering_cases`)."""
  from swirl_fem_amd.core.interpolation import NodeType
  from tests import numbering_cases as NC
  pair = None
  if mesh_kind == 'three_kinds_padded':
    mesh, _, _ = G.three_kinds(2, ndim, 3, pad=1).finalize(DEV, F64)
  else:
    pair = NC.stokes_spaces(
        NC.build_pair('refiner', 'identity', 'three_kinds', 3, 5, ndim), DEV,
        F64)
    mesh = pair[0].mesh
  fes = FiniteElementSpace.create(
      mesh, Quadrature1D.create_from_nodes_1d(mesh.gridpoints_1d))
  grid = FiniteElementSpace.create(
      mesh, Quadrature1D.create(4, NodeType.GAUSS_LEGENDRE))
  ops = {
      'helmholtz': operators.HelmholtzOperator.create(fes, None, geometry,
                                                      'atomic'),
      'two_grid': operators.TwoGridHelmholtzOperator.create(grid, None,
                                                            geometry),
      'convection': operators.ConvectionOperator.create(grid, geometry),
      'transport': operators.TransportRhs.create(grid, geometry)}
  if pair is None:
    assert operators.supports_fused_stokes(fes, fes) == 'P=3 < 4'
  else:
    ops['stokes'] = operators.StokesDivGrad.create(*pair, None, geometry)
  return {name: op.parts for name, op in ops.items()}, mesh.num_elements


@pytest.mark.parametrize('ndim', [2, 3])
@pytest.mark.parametrize('mesh_kind', ['three_kinds_padded', 'stokes_pair'])
def test_operators_share_one_launch_list(mesh_kind, ndim):
  POINT = operators._GEO_POINT
  lists, E = _launch_lists(mesh_kind, ndim, 'auto')
  ref = lists['helmholtz']
  modes = [q['geo_mode'] for q in ref]
  assert len(modes) >= 2 and len(set(modes)) == len(modes), modes
  # the kinds split the elements; curved rows are numbered in element order
  every = torch.cat([q['elem_list'] for q in ref]).sort().values
  assert torch.equal(every, torch.arange(E, dtype=torch.int32, device=DEV))
  for q in ref:
    if q['geo_mode'] == POINT:
      rows = q['geo_index'][q['elem_list'].long()]
      assert torch.equal(rows, torch.arange(
          rows.numel(), dtype=torch.int32, device=DEV))
  for name, parts in lists.items():
    assert [q['geo_mode'] for q in parts] == modes, name
    for q, r in zip(parts, ref):
      curved = q['geo_mode'] == POINT
      assert 'elem_list' in q and ('geo_index' in q) == curved, name
      assert ('geo_elem' in q) == (not curved), name
      assert (LAUNCH_DATA[name] in q) == curved, name
      for key in ('elem_list', 'geo_index', 'geo_elem'):
        assert (key in q) == (key in r), (name, key)
        if key in q:
          assert torch.equal(q[key], r[key]), (name, key)
      if curved:
        assert q[LAUNCH_DATA[name]].shape[0] == q['elem_list'].numel(), name
  lists, E = _launch_lists(mesh_kind, ndim, 'stored')
  for name, parts in lists.items():
    assert [q['geo_mode'] for q in parts] == [POINT], name
    assert not {'elem_list', 'geo_index', 'geo_elem'} & set(parts[0]), name
    assert parts[0][LAUNCH_DATA[name]].shape[0] == E, name
