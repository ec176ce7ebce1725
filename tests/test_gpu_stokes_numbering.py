"""The Stokes operators under other node numberings and on mixed geometry.

Every other Stokes test meshes with `refine_premesh`: velocity facets are
contiguous runs of node ids, and the element-interior pressure nodes are
`e * np + k`, so `StokesDivGrad.penc` and the Schwarz preconditioner's
`pel_arg` are None and the index-row branch of every Stokes kernel never runs.
Here the velocity / pressure pairs of `tests/numbering_cases.py` rename the
nodes of both meshes independently.  The reference is always the float64
oracle on the REFINER numbering, mapped through the two permutations.

Bounds: fp64 1e-11 relative to the largest entry (operators), fp32
`fp32util.tolerance` on float32-representable inputs; whole steps use the
bounds of the same cases in `tests/test_gpu_stokes.py`.

What was pruned from the full product of section b, and why.  The kernels
see a velocity numbering only through (i) facet table or index row per
element and (ii) the sign and size of the facet strides, and a pressure
numbering only through `penc` NULL or given (an index row is an index row:
the kernel reads `penc[slot]` whatever the ids are).  So per kernel family
-- 3D index rows (P = 4, 5, 12), 3D chains (P = 6, 7, 8, general geometry),
3D box chains (P = 6, 7, 8, axis-aligned elements), 2D index rows (P = 4, 6,
12) -- the cases keep {refiner, a positive stride (lexicographic), a negative
stride (reversed / reversed_lexicographic), random} x {penc NULL, penc
given}, and the four non-identity pressure numberings rotate over them
instead of multiplying them.  `random` velocity ids have no facet table at
all, so for the chain and box families the random representative is
`half_random` (every second element back on its index row: the `ids[~good]`
launch next to chains), and plain `random` is checked to stay on index rows
at P = 7.  `lexicographic_yzx` and `reversed_lexicographic` appear once per
family at most (same code as their plain twins, other strides).  Geometries:
each of box, affine, multilinear, three_kinds, affine_curved and periodic
runs with chains and with index rows once; curved pairs start at P = 5 (a
2-point pressure space cannot hold a curved element, and the fused kernels
refuse a pair whose spaces carry different geometry).  fp32 runs once per
family.  P = 12 keeps two cases per dimension (the oracle is dense).

`penc` with negative ids (e): partition padding is the public route.  An
unevenly partitioned premesh pads the shorter ranks' element rows with -1 in
both meshes, so that rank's pressure elements are not `arange` and the
kernels get a `penc` with whole -1 rows next to padded velocity rows and
padded nodes: `test_partition_padding_gives_negative_pressure_rows` finalises
such a rank and compares with the oracle restricted to its elements.
Scattered single -1 slots have no public route and are tested through the
operator's own launch on a hand-made `penc`.

Needs a real MI355X."""
import dataclasses
import itertools

import numpy as np
import pytest
import torch

from oracle import sfem_oracle as O
from swirl_fem_amd import _lib
from swirl_fem_amd.core import layout, operators
from swirl_fem_amd.navier_stokes import pressure_preconditioner as pc
from swirl_fem_amd.navier_stokes.navier_stokes import BCType
from tests import numbering_cases as NC
from tests import stokes_case as SC
from tests.fp32util import F32Rng, tolerance

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64, F32 = torch.float64, torch.float32
TOL64 = 1e-11
POINT, AFFINE, MULTI, BOX = 0, 1, 3, 5          # operators._GEO_* codes
WALLS = {'boundary': (BCType.DIRICHLET, 0.0)}
# geometry kinds that `classify_geometry` must find in fp64 (before the box
# split of the facet launches), and whether axis-aligned elements exist
KINDS = {'box': {AFFINE}, 'walled_box': {AFFINE}, 'periodic_box': {AFFINE},
         'affine': {AFFINE}, 'multilinear': {MULTI},
         'vertex': {AFFINE, MULTI}, 'periodic': {AFFINE, MULTI},
         'three_kinds': {AFFINE, MULTI, POINT},
         'affine_curved': {AFFINE, POINT}}
HAS_BOX = {'box', 'walled_box', 'periodic_box', 'vertex', 'periodic',
           'three_kinds', 'affine_curved'}


def dev(x, dtype=None):
  t = torch.as_tensor(np.ascontiguousarray(x), device=DEV)
  return t if dtype is None else t.to(dtype)


def _np(t):
  return t.detach().double().cpu().numpy()


def relerr(a, b):
  a = _np(a) if isinstance(a, torch.Tensor) else np.asarray(a)
  assert a.shape == b.shape, (a.shape, b.shape)
  return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _tol(dtype, P):
  return TOL64 if dtype == F64 else tolerance(dtype, P)


def _bmask(c):
  """Boundary mask in the renumbered frame, from the refiner's mesh."""
  return c.v.from_base(c.v.base.finalize_all()['physical_masks']['boundary'])


def _facet_expected(c, ndim):
  if ndim != 3 or c.P not in operators.STOKES_FACET_P:
    return 'none'
  return NC.EXPECT[NC.kind(c.vnum)][0]


def check_paths(fused, c, ndim, dtype, box=True, sort=True):
  """What this numbering / geometry / order is meant to launch."""
  facet = _facet_expected(c, ndim)
  fp = fused.facet_parts
  if facet == 'none':
    assert fp is None, c.name
  else:
    assert fp is not None, c.name
    tabled = ['facet_table' in q for q in fp]
    if facet == 'all':
      assert all(tabled), c.name
    else:
      # chains next to the index-row fall-back of the refused elements
      assert any(tabled) and not all(tabled), c.name
    assert all(('chains' in q) == ('facet_table' in q) for q in fp), c.name
  assert (fused.penc is None) == (c.pnum == 'identity'), c.name
  assert (fused.shared_order is not None) == (
      sort and ndim == 3 and c.P <= 8), c.name
  assert fused.supports_layered_e() == (fp is None), c.name
  if dtype == F64:
    assert {q['geo_mode'] for q in fused.parts} == KINDS[c.geometry], c.name
    if fp is not None:
      modes = {q['geo_mode'] for q in fp if 'facet_table' in q}
      assert (BOX in modes) == (box and c.geometry in HAS_BOX), (c.name, modes)
      assert {AFFINE if m == BOX else m for m in
              {q['geo_mode'] for q in fp}} == KINDS[c.geometry], c.name


class Ref:
  """The oracle on the refiner numbering, answers in the renumbered frame."""

  def __init__(self, c):
    self.c = c
    self.ov, self.op = NC.oracle_spaces(c.v.base, c.p.base, c.P)

  def div(self, u):
    ov, op, c = self.ov, self.op, self.c
    return c.p.from_base(op.scatter(O.div_local(
        ov, op, ov.gather(c.v.to_base(u)))))

  def grad_t(self, p):
    ov, op, c = self.ov, self.op, self.c
    return c.v.from_base(ov.scatter(O.div_t_local(
        ov, op, op.gather(c.p.to_base(p)))))


def check_div_grad(c, ndim, dtype, monkeypatch, box=True):
  """Section b on one pair: scale forms, layouts, mask, fused dot, adjoint."""
  P, tol = c.P, _tol(dtype, c.P)
  rng = F32Rng(5)
  vsp, psp = NC.stokes_spaces(c, DEV, dtype)
  N, Np = vsp.mesh.num_nodes, psp.mesh.num_nodes
  ref = Ref(c)
  bm = _bmask(c)
  u = rng.standard_normal((N, ndim))
  p = rng.standard_normal(Np)
  sc = rng.uniform(0.5, 2.0, (N, ndim))
  s1 = np.ascontiguousarray(sc[:, 0])
  d_ref, ds_ref = ref.div(u), ref.div(sc * u)
  d1_ref = ref.div(s1[:, None] * u)
  g_free = ref.grad_t(p)
  g_ref = (~bm)[:, None] * g_free
  ud, pd = dev(u, dtype), dev(p, dtype)
  scd, s1d = dev(sc, dtype), dev(s1, dtype)
  ucm = layout.component_major(ud)
  chain_eligible = ndim == 3 and P in operators.STOKES_FACET_P
  for mask in (dev(bm), None):
    fused = operators.StokesDivGrad.create(vsp, psp, mask)
    check_paths(fused, c, ndim, dtype, box)
    g_want = g_ref if mask is not None else g_free
    for route in (('box', 'all') if chain_eligible else (None,)):
      if route is not None:
        monkeypatch.setenv('SFEM_STOKES_FACET_DIV', route)
      assert relerr(fused.div(ud), d_ref) < tol, (c.name, route)
      assert relerr(fused.div(ud, scale=scd), ds_ref) < tol, (c.name, route)
      assert relerr(fused.div(ud, scale=s1d), d1_ref) < tol, (c.name, route)
      assert relerr(fused.div(ucm), d_ref) < tol, (c.name, route)
      assert relerr(fused.div(ucm, scale=scd), ds_ref) < tol, (c.name, route)
      assert relerr(fused.div(ucm, scale=s1d), d1_ref) < tol, (c.name, route)
      # fused dot against a float64 dot of the reference
      for field in (ud, ucm):
        dots = torch.zeros(_lib.SFEM_DOT_SLOTS, dtype=F64, device=DEV)
        got = fused.div(field, scale=s1d, dot_with=pd, dot_out=dots)
        assert relerr(got, d1_ref) < tol, (c.name, route)
        want = float(np.dot(p, d1_ref))
        scale = float(np.linalg.norm(p) * np.linalg.norm(d1_ref))
        assert abs(float(dots.sum()) - want) < tol * scale, (c.name, route)
    assert relerr(fused.grad_t(pd), g_want) < tol, c.name
    assert relerr(fused.grad_t(pd, scale=s1d), s1[:, None] * g_want) < tol
    assert relerr(fused.grad_t(pd, scale=scd), sc * g_want) < tol, c.name
    gcm = fused.grad_t(pd, component_major=True)
    assert layout.is_component_major(gcm)
    assert relerr(gcm, g_want) < tol, c.name
    assert relerr(fused.grad_t(pd, component_major=True, scale=s1d),
                  s1[:, None] * g_want) < tol, c.name
    assert relerr(fused.grad_t(pd, component_major=True, scale=scd),
                  sc * g_want) < tol, c.name
    if mask is None:
      # adjointness <D u, p> = <u, D^T p> of the unmasked operator
      for field, cm in ((ud, False), (ucm, True)):
        lhs = float((fused.div(field).double() * pd.double()).sum())
        rhs = float((fused.grad_t(pd, component_major=cm).double() *
                     ud.double()).sum())
        size = float(np.linalg.norm(u) * np.linalg.norm(g_free))
        assert abs(lhs - rhs) < tol * size, (c.name, cm)


# (vnum, pnum, geometry, n, P), see the module docstring
CASES_3D = [
    # index rows
    ('refiner', 'identity', 'vertex', 3, 4),
    ('refiner', 'random', 'vertex', 3, 4),
    ('lexicographic', 'identity', 'vertex', 3, 4),
    ('lexicographic', 'interleaved', 'box', 2, 4),
    ('reversed', 'identity', 'affine', 2, 4),
    ('reversed', 'reversed', 'multilinear', 2, 4),
    ('random', 'identity', 'vertex', 3, 4),
    ('random', 'block_shuffled', 'periodic', 3, 4),
    ('lexicographic_yzx', 'random', 'three_kinds', 3, 5),
    ('half_random', 'reversed', 'three_kinds', 3, 5),
    ('refiner', 'interleaved', 'affine_curved', 2, 5),
    ('reversed_lexicographic', 'random', 'multilinear', 2, 12),
    ('random', 'identity', 'affine', 2, 12),
    # chains on general geometry
    ('refiner', 'identity', 'affine', 2, 7),
    ('refiner', 'reversed', 'multilinear', 2, 7),
    ('lexicographic', 'identity', 'multilinear', 2, 7),
    ('lexicographic', 'random', 'affine', 2, 7),
    ('reversed_lexicographic', 'identity', 'affine', 2, 7),
    ('reversed', 'interleaved', 'multilinear', 2, 7),
    ('half_random', 'identity', 'multilinear', 2, 7),
    ('half_random', 'block_shuffled', 'affine', 2, 7),
    ('random', 'random', 'affine', 2, 7),            # stays on index rows
    ('refiner', 'identity', 'three_kinds', 3, 6),
    ('lexicographic_yzx', 'random', 'three_kinds', 3, 6),
    ('half_random', 'block_shuffled', 'three_kinds', 3, 6),
    ('reversed', 'interleaved', 'three_kinds', 3, 8),
    ('lexicographic', 'random', 'affine_curved', 2, 8),
    ('reversed_lexicographic', 'random', 'periodic', 3, 7),
    ('half_random', 'reversed', 'periodic', 3, 6),
    # box chains
    ('refiner', 'identity', 'box', 2, 6),
    ('refiner', 'random', 'box', 2, 6),
    ('lexicographic', 'identity', 'box', 2, 7),
    ('lexicographic', 'interleaved', 'box', 2, 6),
    ('reversed', 'identity', 'box', 2, 6),
    ('reversed_lexicographic', 'block_shuffled', 'box', 2, 8),
    ('half_random', 'identity', 'box', 2, 6),
    ('half_random', 'reversed', 'box', 2, 7),
]
CASES_2D = [
    ('refiner', 'identity', 'vertex', 3, 4),
    ('refiner', 'interleaved', 'vertex', 3, 4),
    ('lexicographic', 'identity', 'box', 3, 4),
    ('lexicographic', 'random', 'vertex', 3, 4),
    ('reversed', 'identity', 'affine', 3, 4),
    ('reversed', 'block_shuffled', 'multilinear', 3, 4),
    ('random', 'identity', 'vertex', 3, 4),
    ('random', 'reversed', 'periodic', 3, 4),
    ('lexicographic', 'block_shuffled', 'three_kinds', 3, 6),
    ('random', 'random', 'three_kinds', 3, 6),
    ('reversed_lexicographic', 'interleaved', 'affine_curved', 3, 6),
    ('half_random', 'identity', 'periodic', 3, 6),
    ('reversed', 'random', 'multilinear', 2, 12),
    ('random', 'interleaved', 'periodic', 3, 12),
]
CASES = [(3,) + c for c in CASES_3D] + [(2,) + c for c in CASES_2D]
# fp32: each kernel family once, with an index row for the pressure
CASES_F32 = [(3, 'lexicographic', 'interleaved', 'vertex', 3, 4),
             (3, 'random', 'reversed', 'three_kinds', 3, 5),
             (3, 'reversed_lexicographic', 'random', 'affine', 2, 7),
             (3, 'half_random', 'block_shuffled', 'three_kinds', 3, 6),
             (3, 'lexicographic', 'interleaved', 'box', 2, 6),
             (3, 'reversed', 'random', 'multilinear', 2, 12),
             (2, 'reversed', 'block_shuffled', 'vertex', 3, 4),
             (2, 'random', 'random', 'three_kinds', 3, 6),
             (2, 'lexicographic', 'interleaved', 'multilinear', 2, 12)]
_ids = lambda cs: [f'{c[0]}d-{c[1]}-{c[2]}-{c[3]}-p{c[5]}' for c in cs]


# ------------------------------------------------- a + b. paths, div, grad_t
@pytest.mark.parametrize('ndim,vnum,pnum,geometry,n,P', CASES, ids=_ids(CASES))
def test_div_and_grad_t_match_oracle(ndim, vnum, pnum, geometry, n, P,
                                     monkeypatch):
  monkeypatch.setenv('SFEM_CHAIN_LEN', '2')     # several segments per launch
  c = NC.build_pair(vnum, pnum, geometry, n, P, ndim=ndim)
  check_div_grad(c, ndim, F64, monkeypatch)


@pytest.mark.parametrize('ndim,vnum,pnum,geometry,n,P', CASES_F32,
                         ids=_ids(CASES_F32))
def test_div_and_grad_t_match_oracle_fp32(ndim, vnum, pnum, geometry, n, P,
                                          monkeypatch):
  monkeypatch.setenv('SFEM_CHAIN_LEN', '2')
  c = NC.build_pair(vnum, pnum, geometry, n, P, ndim=ndim, f32=True)
  check_div_grad(c, ndim, F32, monkeypatch)


# ------------------------------------------------------ c. switches agree
SWITCH_CASES = [('lexicographic', 'random', 'box', 2, 6),
                ('reversed_lexicographic', 'interleaved', 'affine', 2, 7),
                ('half_random', 'block_shuffled', 'multilinear', 2, 7),
                ('reversed', 'random', 'three_kinds', 3, 6),
                ('lexicographic_yzx', 'reversed', 'affine_curved', 2, 8),
                ('half_random', 'interleaved', 'periodic', 3, 6)]


@pytest.mark.parametrize('vnum,pnum,geometry,n,P', SWITCH_CASES,
                         ids=[f'{c[0]}-{c[1]}-{c[2]}-p{c[4]}'
                              for c in SWITCH_CASES])
def test_switches_agree_with_the_oracle(vnum, pnum, geometry, n, P,
                                        monkeypatch):
  """SFEM_STOKES_FACET x SFEM_STOKES_FACET_DIV x SFEM_BOX x SFEM_CHAIN x
  SFEM_SORTED_SCATTER: every combination within the bound of the oracle."""
  c = NC.build_pair(vnum, pnum, geometry, n, P)
  rng = np.random.default_rng(8)
  vsp, psp = NC.stokes_spaces(c, DEV, F64)
  N, Np = vsp.mesh.num_nodes, psp.mesh.num_nodes
  ref, bm = Ref(c), _bmask(c)
  u, p = rng.standard_normal((N, 3)), rng.standard_normal(Np)
  s1 = rng.uniform(0.5, 2.0, N)
  d_ref = ref.div(s1[:, None] * u)
  g_ref = (~bm)[:, None] * ref.grad_t(p) * s1[:, None]
  ucm, pd, s1d = layout.component_major(dev(u)), dev(p), dev(s1)
  for facet, div, box, chain, sort in itertools.product(
      '01', ('box', 'all'), '01', '01', '01'):
    env = {'SFEM_STOKES_FACET': facet, 'SFEM_STOKES_FACET_DIV': div,
           'SFEM_BOX': box, 'SFEM_CHAIN': chain, 'SFEM_SORTED_SCATTER': sort}
    for k, v in env.items():
      monkeypatch.setenv(k, v)
    fused = operators.StokesDivGrad.create(vsp, psp, dev(bm))
    assert (fused.facet_parts is not None) == (facet == '1'), env
    assert (fused.shared_order is not None) == (sort == '1'), env
    if facet == '1':
      check_paths(fused, c, 3, F64, box == '1', sort == '1')
      segs = [q['chains'] for q in fused.facet_parts if 'chains' in q]
      assert segs, env
    dots = torch.zeros(_lib.SFEM_DOT_SLOTS, dtype=F64, device=DEV)
    got = fused.div(ucm, scale=s1d, dot_with=pd, dot_out=dots)
    assert relerr(got, d_ref) < TOL64, env
    assert abs(float(dots.sum()) - float(np.dot(p, d_ref))) < TOL64 * float(
        np.linalg.norm(p) * np.linalg.norm(d_ref)), env
    assert relerr(fused.grad_t(pd, component_major=True, scale=s1d),
                  g_ref) < TOL64, env
    assert relerr(fused.grad_t(pd, scale=s1d), g_ref) < TOL64, env


# ------------------------------------------------- d. pressure operator E
E_CASES = [(2, 'refiner', 'identity', 'periodic', 3, 6),
           (2, 'lexicographic', 'interleaved', 'periodic', 3, 6),
           (2, 'random', 'random', 'three_kinds', 3, 6),
           (2, 'reversed', 'block_shuffled', 'periodic', 3, 4),
           (3, 'random', 'reversed', 'periodic', 3, 4),
           (3, 'lexicographic', 'identity', 'periodic', 3, 5),
           (3, 'reversed_lexicographic', 'random', 'three_kinds', 3, 5),
           (3, 'reversed_lexicographic', 'identity', 'periodic', 3, 7),
           (3, 'half_random', 'interleaved', 'periodic', 3, 7),
           (3, 'random', 'block_shuffled', 'affine_curved', 2, 7)]


@pytest.mark.parametrize('ndim,vnum,pnum,geometry,n,P', E_CASES,
                         ids=_ids(E_CASES))
def test_pressure_operator_matches_oracle(ndim, vnum, pnum, geometry, n, P,
                                          monkeypatch):
  """`StokesSEM.E` on every route (plain pair, layered, split) and the
  operator-level `e_apply` / `e_layered` with the three scale forms, against
  D Q D^T of the oracle with the periodic exchange."""
  c = NC.build_pair(vnum, pnum, geometry, n, P, ndim=ndim)
  sem = NC.stokes_sem(c, WALLS, DEV, F64)
  orc = NC.stokes_oracle(c.v.base, c.p.base, P, 'boundary')
  rng = np.random.default_rng(12)
  Np = sem.pressure.pspace.mesh.num_nodes
  N = sem.velocity.mesh.num_nodes
  p = rng.standard_normal(Np)
  dt, k = 1e-2, 2
  e_ref = c.p.from_base(orc.E(c.p.to_base(p), dt, k))
  op = sem._divgrad()
  assert op is not None
  check_paths(op, c, ndim, F64)
  calls = []
  for name in ('e_apply', 'e_layered'):
    inner = getattr(operators.StokesDivGrad, name)
    def spy(self, *a, _inner=inner, _name=name, **kw):
      calls.append(_name)
      return _inner(self, *a, **kw)
    monkeypatch.setattr(operators.StokesDivGrad, name, spy)
  pd = dev(p)
  # E of the stepper loses two digits to Q's scaling (test_gpu_stokes.py uses
  # 1e-9 for it); the bound here stays that of the operators
  for lay, split in (('0', '0'), (None, '0'), ('1', '0'), ('0', '1')):
    if lay is None:
      monkeypatch.delenv('SFEM_STOKES_LAYERED', raising=False)
    else:
      monkeypatch.setenv('SFEM_STOKES_LAYERED', lay)
    monkeypatch.setenv('SFEM_SPLIT_E', split)
    del calls[:]
    dots = torch.zeros(_lib.SFEM_DOT_SLOTS, dtype=F64, device=DEV)
    got = sem.E(pd, dt, k) if split == '1' else sem.E(pd, dt, k, dot_out=dots)
    assert relerr(got, e_ref) < TOL64, (c.name, lay, split)
    if split == '1':
      # with a pressure index row the stepper must leave the split alone
      assert calls == (['e_apply'] if pnum == 'identity' else []), calls
    else:
      want = float(np.dot(p, e_ref))
      assert abs(float(dots.sum()) - want) < TOL64 * float(
          np.linalg.norm(p) * np.linalg.norm(e_ref)), (c.name, lay)
      layered = op.supports_layered_e() and (
          lay == '1' or (lay is None and ndim == 2))
      assert calls == (['e_layered'] if layered else []), (calls, lay)
  # operator level: scale None / (N,) / (N, d), equal on periodic images
  one = np.ones((N, ndim))
  sc = c.v.from_base(orc.vexchange(c.v.to_base(rng.uniform(0.5, 2.0, (N, ndim))))
                     / orc.vexchange(c.v.to_base(one)))
  exch = lambda w: sem.velocity.exchange(w, inplace=True)
  for scale in (None, np.ascontiguousarray(sc[:, 0]), sc):
    s = 1.0 if scale is None else (scale[:, None] if scale.ndim == 1 else scale)
    want = c.p.from_base(orc.D(c.v.to_base(s * c.v.from_base(orc.vexchange(
        orc.Dt(c.p.to_base(p)))))))
    sd = None if scale is None else dev(scale)
    if op.supports_layered_e():
      assert relerr(op.e_layered(pd, scale=sd), want) < TOL64, c.name
    else:
      with pytest.raises(NotImplementedError, match='index-row'):
        op.e_layered(pd, scale=sd)
    if pnum == 'identity':
      assert relerr(op.e_apply(pd, scale=sd, exchange=exch), want) < TOL64
    else:
      with pytest.raises(NotImplementedError, match='element-local'):
        op.e_apply(pd, scale=sd, exchange=exch)


@pytest.mark.parametrize('ndim,vnum,pnum,P', [
    (2, 'reversed', 'random', 6), (3, 'lexicographic', 'interleaved', 4),
    (3, 'reversed_lexicographic', 'block_shuffled', 7),
    (3, 'random', 'reversed', 7)])
def test_pressure_operator_is_symmetric_semidefinite(ndim, vnum, pnum, P):
  """On the periodic box: <E a, b> = <a, E b>, <a, E a> >= 0, E 1 = 0."""
  c = NC.build_pair(vnum, pnum, 'periodic_box', 3, P, ndim=ndim)
  sem = NC.stokes_sem(c, {}, DEV, F64)
  g = torch.Generator(device=DEV).manual_seed(4)
  Np = sem.pressure.pspace.mesh.num_nodes
  a = torch.randn(Np, dtype=F64, device=DEV, generator=g)
  b = torch.randn(Np, dtype=F64, device=DEV, generator=g)
  Ea, Eb = sem.E(a, 1e-2, 3), sem.E(b, 1e-2, 3)
  size = float(a.norm() * Eb.norm())
  assert abs(float(torch.dot(Ea, b) - torch.dot(a, Eb))) < TOL64 * size
  assert float(torch.dot(a, Ea)) > 0.0
  assert float(torch.dot(b, Eb)) > 0.0
  E1 = sem.E(torch.ones_like(a), 1e-2, 3)
  assert float(E1.abs().max()) < TOL64 * float(Ea.abs().max())


# ------------------------------------------ e. penc with skipped entries
@pytest.mark.parametrize('ndim,vnum,geometry,n,P', [
    (3, 'lexicographic', 'vertex', 3, 4), (3, 'reversed', 'multilinear', 2, 7),
    (3, 'half_random', 'box', 2, 6), (2, 'random', 'vertex', 3, 4)])
def test_negative_pressure_ids_are_skipped(ndim, vnum, geometry, n, P,
                                           monkeypatch):
  """`include/sfem.h`: negative `penc` entries are skipped.  A skipped slot
  adds nothing to `grad_t`, and `div` stores nothing for it."""
  monkeypatch.setenv('SFEM_STOKES_FACET_DIV', 'all')
  c = NC.build_pair(vnum, 'random', geometry, n, P, ndim=ndim)
  vsp, psp = NC.stokes_spaces(c, DEV, F64)
  fused = operators.StokesDivGrad.create(vsp, psp, None)
  check_paths(fused, c, ndim, F64)
  rng = np.random.default_rng(21)
  pel = np.asarray(c.p.rp.elements).copy()
  skip = rng.random(pel.shape) < 0.2
  skip[1] = True                                 # a whole padded row
  skip[0, 0], skip[0, 1] = True, False
  penc = np.where(skip, -1, pel).astype(np.int32)
  cut = dataclasses.replace(fused, penc=dev(penc), _div_parts=None)
  N, Np = vsp.mesh.num_nodes, psp.mesh.num_nodes
  u, p = rng.standard_normal((N, ndim)), rng.standard_normal(Np)
  ref = Ref(c)
  gone = np.zeros(Np, bool)
  gone[pel[skip]] = True
  g_ref = ref.grad_t(np.where(gone, 0.0, p))
  d_ref = ref.div(u)
  ud, pd = dev(u), dev(p)
  for field, cm in ((ud, False), (layout.component_major(ud), True)):
    out = torch.full((Np,), -7.5, dtype=F64, device=DEV)
    got = cut.div(field, out=out)
    assert np.array_equal(_np(got)[gone], np.full(int(gone.sum()), -7.5))
    # (relative to the largest live entry of D u, not to the sentinel)
    assert relerr(_np(got)[~gone], d_ref[~gone]) < TOL64, (c.name, cm)
    dots = torch.zeros(_lib.SFEM_DOT_SLOTS, dtype=F64, device=DEV)
    out = torch.full((Np,), -7.5, dtype=F64, device=DEV)
    cut.div(field, out=out, dot_with=pd, dot_out=dots)
    want = float(np.dot(p[~gone], d_ref[~gone]))
    assert abs(float(dots.sum()) - want) < TOL64 * float(
        np.linalg.norm(p) * np.linalg.norm(d_ref[~gone]))
    assert relerr(cut.grad_t(pd, component_major=cm), g_ref) < TOL64, (
        c.name, cm)


@pytest.mark.parametrize('ndim,n,P', [(2, 3, 4), (3, 2, 4), (3, 2, 7)])
def test_partition_padding_gives_negative_pressure_rows(ndim, n, P,
                                                        monkeypatch):
  """The public route to negative pressure ids: an unevenly partitioned
  premesh.  The shorter rank's meshes carry all -1 element rows (velocity and
  pressure) and padded nodes; `div` and the rank-local part of `grad_t` (no
  communication) against the oracle restricted to that rank's elements."""
  from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
  from swirl_fem_amd.core.fespace import FiniteElementSpace
  from swirl_fem_amd.core.interpolation import Nodes1D, Quadrature1D
  from swirl_fem_amd.core.mesh_refiner import refine_premesh
  monkeypatch.setenv('SFEM_STOKES_FACET_DIV', 'all')
  rng = np.random.default_rng(3)
  pm = unit_cube_mesh(n, ndim=ndim)
  pm = pm.replace(node_coords=pm.node_coords + 0.1 / n * rng.uniform(
      -1, 1, pm.node_coords.shape))
  E = pm.num_elements
  parts = np.array([0] * (E // 2 + 1) + [1] * (E - E // 2 - 1), np.int32)
  pp = pm.replace(partitions=parts)
  gv, gp = Nodes1D.create(P, NC.GLL), Nodes1D.create(P - 2, NC.GL)
  rv, rq = refine_premesh(pp, gv), refine_premesh(pp, gp)
  av, aq = rv.finalize_all('parts'), rq.finalize_all('parts')
  ov, op = NC.oracle_spaces(refine_premesh(pm, gv), refine_premesh(pm, gp), P)
  ug = rng.standard_normal((ov.num_nodes, ndim))
  pg = rng.standard_normal(op.num_nodes)
  d_glob = op.scatter(O.div_local(ov, op, ov.gather(ug)))
  g_loc = O.div_t_local(ov, op, op.gather(pg))
  quad = Quadrature1D.create(P, NC.GLL)
  pad = 2 * (E // 2 + 1) - E
  for rank in (0, 1):
    vsp = FiniteElementSpace.create(
        rv.finalize('parts', rank=rank, device=DEV), quad)
    psp = FiniteElementSpace.create(
        rq.finalize('parts', rank=rank, device=DEV), quad)
    assert operators.supports_fused_stokes(vsp, psp) is None
    vid, pid = av['global_node_ids'][rank], aq['global_node_ids'][rank]
    vreal, preal = vid >= 0, pid >= 0
    # the stepper's mask: Dirichlet walls and the padding nodes
    mask = av['physical_masks']['boundary'][rank] | (
        av['node_indices'][rank] < 0)
    fused = operators.StokesDivGrad.create(vsp, psp, dev(mask))
    pel = _np(psp.mesh.elements)
    if rank == 0:
      assert fused.penc is None and preal.all()
    else:
      assert fused.penc is not None
      assert int((pel < 0).all(axis=1).sum()) == pad > 0
      assert int((_np(vsp.mesh.elements) < 0).all(axis=1).sum()) == pad
      assert not preal.all() and not vreal.all()
    assert (fused.facet_parts is not None) == (P == 7)
    if P == 7:     # the real elements on chains, the padded rows on index rows
      assert sum('facet_table' in q for q in fused.facet_parts) >= 1
      assert all('facet_table' in q for q in fused.facet_parts) == (rank == 0)
    ei = aq['element_indices'][rank]
    assert np.array_equal(ei, av['element_indices'][rank])
    mine = np.zeros_like(g_loc)
    mine[ei[ei >= 0]] = g_loc[ei[ei >= 0]]
    g_glob = ov.scatter(mine)
    u = np.where(vreal[:, None], ug[np.maximum(vid, 0)], 0.0)
    p = np.where(preal, pg[np.maximum(pid, 0)], 0.0)
    d_ref = np.where(preal, d_glob[np.maximum(pid, 0)], 0.0)
    g_ref = np.where((vreal & ~mask)[:, None], g_glob[np.maximum(vid, 0)], 0.0)
    ud, pd = dev(u), dev(p)
    for field, cm in ((ud, False), (layout.component_major(ud), True)):
      got = fused.div(field)
      # zero-filled output: the padded pressure nodes hold exact zeros
      assert not _np(got)[~preal].any()
      assert relerr(got, d_ref) < TOL64, (rank, cm)
      dots = torch.zeros(_lib.SFEM_DOT_SLOTS, dtype=F64, device=DEV)
      fused.div(field, dot_with=pd, dot_out=dots)
      assert abs(float(dots.sum()) - float(np.dot(p, d_ref))) < TOL64 * float(
          np.linalg.norm(p) * np.linalg.norm(d_ref)), (rank, cm)
      g = fused.grad_t(pd, component_major=cm)
      assert relerr(_np(g)[vreal], g_ref[vreal]) < TOL64, (rank, cm)
      assert not _np(g)[~vreal].any()


# ----------------------------------------------------------- f. convection
@pytest.mark.parametrize('ndim,vnum,pnum,P', [
    (3, 'reversed_lexicographic', 'random', 6), (3, 'random', 'reversed', 5),
    (2, 'lexicographic', 'interleaved', 6)])
def test_convection_matches_oracle(ndim, vnum, pnum, P):
  c = NC.build_pair(vnum, pnum, 'three_kinds', 3, P, ndim=ndim)
  sem = NC.stokes_sem(c, WALLS, DEV, F64)
  orc = NC.stokes_oracle(c.v.base, c.p.base, P, 'boundary')
  u = np.random.default_rng(2).standard_normal(
      (sem.velocity.mesh.num_nodes, ndim))
  want = c.v.from_base(orc.C(c.v.to_base(u)))
  assert relerr(sem.C(dev(u)), want) < TOL64
  assert sem.velocity.overint_space._cache['convection'] is not None


# -------------------------------------------- g. Schwarz preconditioner
@pytest.mark.parametrize('ndim,vnum,pnum,geometry,P', [
    (3, 'refiner', 'identity', 'periodic_box', 5),
    (3, 'lexicographic', 'reversed', 'periodic_box', 5),
    (3, 'random', 'random', 'periodic_box', 5),
    (3, 'reversed_lexicographic', 'block_shuffled', 'periodic_box', 7),
    (3, 'refiner', 'interleaved', 'walled_box', 5),
    (2, 'reversed', 'random', 'walled_box', 6),
    (2, 'lexicographic', 'block_shuffled', 'walled_box', 6),
    (2, 'random', 'interleaved', 'periodic_box', 6),
    (2, 'refiner', 'identity', 'walled_box', 6)])
def test_schwarz_preconditioner_under_numberings(ndim, vnum, pnum, geometry,
                                                 P, monkeypatch):
  n = 4 if ndim == 2 else 3
  # (small coarse problems are solved by a dense pseudo-inverse: switch that
  # off for the periodic boxes -> FFT, and for the walled 3D box -> Chebyshev)
  sparse = geometry == 'periodic_box' or ndim == 3
  if sparse:
    monkeypatch.setattr(pc, 'DENSE_COARSE_MAX', 0)
  c = NC.build_pair(vnum, pnum, geometry, n, P, ndim=ndim)
  bcs = WALLS if geometry == 'walled_box' else {}
  sem = NC.stokes_sem(c, bcs, DEV, F64)
  base = NC.stokes_sem(c, bcs, DEV, F64, base=True)
  dt, k = 2e-3, 3
  M = pc.SchwarzPressurePreconditioner(sem, dt, k)
  Mb = pc.SchwarzPressurePreconditioner(base, dt, k)
  assert (M.pel_arg is None) == (pnum == 'identity')
  assert Mb.pel_arg is None
  if geometry == 'periodic_box':
    assert M.E0_fft is not None and Mb.E0_fft is not None    # FFT coarse solve
  else:
    assert M.E0_fft is None and (M.E0_pinv is None) == sparse
  Np = sem.pressure.pspace.mesh.num_nodes
  r = np.random.default_rng(6).standard_normal(Np)
  rd = dev(r)
  z = M.local_solve(rd)
  zt = M.local_solve_torch(rd)
  assert float((z - zt).abs().max()) < 1e-12 * float(zt.abs().max())
  zb = Mb.local_solve_torch(dev(c.p.to_base(r)))
  assert relerr(z, c.p.from_base(_np(zb))) < 1e-12
  # which closing route ran: the fused sums need element-contiguous ids
  called = []
  from swirl_fem_amd import _ops
  inner = _ops.fdm_solve_sums
  monkeypatch.setattr(_ops, 'fdm_solve_sums',
                      lambda *a, **kw: (called.append(1), inner(*a, **kw))[1])
  gi = sem.pressure.pspace.mesh.exchange_gather_indices
  assert gi is None or gi.numel() == 0
  got = M(rd)
  assert bool(called) == (pnum == 'identity'), (pnum, called)
  assert (M._fused_setup() is not None) == (pnum == 'identity')
  want = c.p.from_base(_np(Mb(dev(c.p.to_base(r)))))
  assert relerr(got, want) < TOL64
  if pnum == 'identity':
    # the separate pieces agree with the fused closing
    monkeypatch.setenv('SFEM_PC_FUSED', '0')
    M2 = pc.SchwarzPressurePreconditioner(sem, dt, k)
    assert M2._fused_setup() is None
    assert relerr(M2(rd), want) < TOL64


# ------------------------------------------------------------ h. whole steps
STEP_NUMBERINGS = [('refiner', 'identity'),
                   ('reversed_lexicographic', 'random'), ('random', 'random')]
# Iteration counts against the refiner numbering of the same run.  A
# renumbering changes the order of sums only.  ITER_SPREAD is the largest
# difference that one run on an MI355X showed between the refiner numbering
# and the two renumbered meshes, (Helmholtz, pressure) iterations per step;
# the assertion allows it plus 2:
#   vortex, projection:  (55, 170) on all three numberings
#   vortex, schwarz:     (55, 67) on all three
#   cavity, projection:  [(20, 135), (20, 135)] on all three
#   cavity, schwarz:     refiner [(20, 70), (20, 70)], renumbered
#                        [(20, 69), (20, 70)]
#   Taylor-Green, projection: [(33, 45), (33, 47)] on all three
#   Taylor-Green, schwarz:    refiner [(33, 32), (33, 33)], renumbered
#                             [(33, 32), (33, 32)]
ITER_SPREAD = {'vortex': 0, 'cavity': 1, 'taylor_green': 1}


def _converged(*infos):
  for info in infos:
    assert info['status'] == 'converged', info


def _close_counts(got, base, case):
  print(f'iterations {case}: renumbered {got} refiner {base}')
  for a, b in zip(np.ravel(got), np.ravel(base)):
    assert abs(int(a) - int(b)) <= ITER_SPREAD[case] + 2, (case, got, base)


@pytest.fixture(scope='module')
def vortex():
  order, K, DT = 7, 3, 1e-3
  pm = SC.make_premesh()
  out = {}
  for vnum, pnum in STEP_NUMBERINGS:
    out[vnum] = NC.build_pair(vnum, pnum, 'vortex', 9, order + 1, ndim=2,
                              premesh=pm)
  c = out['refiner']
  orc = NC.stokes_oracle(c.v.base, c.p.base, order + 1, 'boundary')
  xv, xp = c.v.base.node_coords, c.p.base.node_coords
  us, ps = zip(*[SC.reference_soln(xv, xp, i * DT) for i in range(K + 1)])
  uo, po, auxo = orc.stokes_one_step(list(us[:-1]), list(ps[:-1]), 0, 1, DT, K,
                                     alpha=0.05, tol=1e-12, atol=1e-12)
  return out, us, ps, uo, po, (K, DT)


@pytest.mark.parametrize('schwarz', [False, True], ids=['projection',
                                                       'schwarz'])
def test_stokes_one_step_under_numberings(vortex, schwarz):
  """The analytic vortex of `tests/stokes_case.py`: one step on renumbered
  meshes against the oracle's step (bounds of
  test_gpu_stokes.py::test_stokes_one_step)."""
  pairs, us, ps, uo, po, (K, DT) = vortex
  counts = {}
  for vnum, c in pairs.items():
    sem = NC.stokes_sem(c, WALLS, DEV, F64)
    M = pc.make_pressure_preconditioner(sem, 'schwarz', DT, K) if schwarz \
        else None
    u, p, aux = sem.stokes_one_step(
        [dev(c.v.from_base(x)) for x in us[:-1]],
        [dev(c.p.from_base(x)) for x in ps[:-1]], f=0, mu=1, dt=DT,
        time_order=K, alpha=0.05, pressure_preconditioner=M, tol=1e-12,
        atol=1e-12)
    _converged(aux['u_star_info'], aux['dp_info'])
    assert float(aux['u_star_info']['residual']) < 1e-7
    assert float(aux['dp_info']['residual']) < 1e-7
    assert relerr(u, c.v.from_base(uo)) < 1e-8, vnum
    assert np.abs(_np(p) - c.p.from_base(po)).max() < 1e-7, vnum
    assert float((u - dev(c.v.from_base(us[-1]))).abs().max()) < 5 * DT ** 2
    counts[vnum] = (aux['u_star_info']['num_iterations'],
                    aux['dp_info']['num_iterations'])
  for vnum in pairs:
    # observed: identical counts, see ITER_SPREAD
    _close_counts(counts[vnum], counts['refiner'], 'vortex')


def test_ensemble_step_under_numberings(vortex):
  """Two members on a renumbered mesh: member 1 is the vortex, member 2 half
  of it (the step is linear), each against the oracle's step."""
  pairs, us, ps, uo, po, (K, DT) = vortex
  c = pairs['random']
  ens = NC.stokes_sem(c, WALLS, DEV, F64).ensemble(2)
  stack = lambda x, m: ens.flatten(torch.stack([dev(m(x)), 0.5 * dev(m(x))]))
  u, p, aux = ens.stokes_one_step(
      [stack(x, c.v.from_base) for x in us[:-1]],
      [stack(x, c.p.from_base) for x in ps[:-1]], f=0, mu=1, dt=DT,
      time_order=K, alpha=0.05, tol=1e-12, atol=1e-12)
  _converged(aux['u_star_info'], aux['dp_info'])
  for info in (aux['u_star_info'], aux['dp_info']):
    assert info['member_status'] == ['converged', 'converged'], info
  u, p = ens.unflatten(u), ens.unflatten(p)
  for m, f in ((0, 1.0), (1, 0.5)):
    assert relerr(u[m], f * c.v.from_base(uo)) < 1e-8, m
    assert np.abs(_np(p[m]) - f * c.p.from_base(po)).max() < 1e-7, m


def _oracle_run(orc, u0, ub, reynolds, dt, steps, K, tol):
  us = (u0,) * K
  ps = (np.zeros(orc.ps.num_nodes),) * K
  Cus = (orc.C(u0),) * K
  for _ in range(steps):
    uo, po, Co, _ = O.navier_stokes_step(orc, us, ps, Cus, reynolds, dt, K,
                                         u_boundary=ub, tol=tol, atol=0.0)
    us, ps, Cus = us[1:] + (uo,), ps[1:] + (po,), Cus[1:] + (Co,)
  return us[-1], ps[-1]


@pytest.fixture(scope='module')
def cavity():
  from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
  n, order = 4, 5
  pm = unit_cube_mesh(n, ndim=2)
  pairs = {v: NC.build_pair(v, p, 'cavity', n, order + 1, ndim=2, premesh=pm)
           for v, p in STEP_NUMBERINGS}
  c = pairs['refiner']
  orc = NC.stokes_oracle(c.v.base, c.p.base, order + 1, 'boundary')
  xc = c.v.base.node_coords
  lid = (xc[:, 1] > 1 - 1e-12).astype(float)
  ub = np.stack([lid * 16 * xc[:, 0] ** 2 * (1 - xc[:, 0]) ** 2,
                 np.zeros(len(xc))], axis=-1)
  uo, po = _oracle_run(orc, ub, ub, 100.0, 1e-3, 2, 3, 1e-11)
  return pairs, order, ub, uo, po


@pytest.mark.parametrize('schwarz', [None, 'schwarz'], ids=['projection',
                                                           'schwarz'])
def test_lid_driven_cavity_under_numberings(cavity, schwarz):
  """Two cavity steps (2D, walls) on renumbered meshes against the oracle's
  (bounds of test_gpu_stokes.py::test_lid_driven_cavity_steps_match_oracle)."""
  from swirl_fem_amd.examples import navier_stokes_driver as drv
  pairs, order, ub, uo, po = cavity
  counts = {}
  for vnum, c in pairs.items():
    sem = NC.stokes_sem(c, WALLS, DEV, F64)
    _, u, p, diag = drv.lid_driven_cavity(
        order=order, reynolds=100.0, dt=1e-3, steps=2, device=DEV, tol=1e-11,
        sem=sem, pressure_preconditioner=schwarz)
    assert all(s == ('converged', 'converged') for s in diag['cg_status']), \
        diag['cg_status']
    assert relerr(u, c.v.from_base(uo)) < 1e-7, vnum
    assert np.abs(_np(p) - c.p.from_base(po)).max() < 1e-6 * max(
        1.0, np.abs(po).max()), vnum
    bm = _bmask(c)
    assert np.abs(_np(u)[bm] - c.v.from_base(ub)[bm]).max() < 1e-12
    assert diag['max_divergence'] < 1e-6
    counts[vnum] = diag['cg_iterations']
  for vnum in pairs:
    _close_counts(counts[vnum], counts['refiner'], 'cavity')


@pytest.fixture(scope='module')
def taylor_green():
  from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
  n, order = 2, 7
  pm = unit_cube_mesh(n, ndim=3, a=0.0, b=2 * np.pi, periodic_dims=(0, 1, 2))
  pairs = {v: NC.build_pair(v, p, 'tg', n, order + 1, premesh=pm)
           for v, p in STEP_NUMBERINGS}
  c = pairs['refiner']
  orc = NC.stokes_oracle(c.v.base, c.p.base, order + 1, None)
  x = c.v.base.node_coords
  u0 = np.stack([np.sin(x[:, 0]) * np.cos(x[:, 1]) * np.cos(x[:, 2]),
                 -np.cos(x[:, 0]) * np.sin(x[:, 1]) * np.cos(x[:, 2]),
                 np.zeros(len(x))], axis=-1)
  uo, po = _oracle_run(orc, u0, None, 1600.0, 1e-3, 2, 3, 1e-12)
  return pairs, order, uo, po


@pytest.mark.parametrize('schwarz', [None, 'schwarz'], ids=['projection',
                                                           'schwarz'])
def test_taylor_green_under_numberings(taylor_green, schwarz):
  """Two Taylor-Green steps (3D, periodic, P = 8: chains under the reversed
  lexicographic numbering, index rows under the random one) against the
  oracle's (bounds of test_taylor_green_3d_p7_step_matches_oracle)."""
  from swirl_fem_amd.examples import navier_stokes_driver as drv
  pairs, order, uo, po = taylor_green
  counts = {}
  for vnum, c in pairs.items():
    sem = NC.stokes_sem(c, {}, DEV, F64)
    op = sem._divgrad()
    assert (op.facet_parts is not None) == (vnum != 'random')
    assert (op.penc is None) == (vnum == 'refiner')
    _, u, p, diag = drv.taylor_green(
        n=2, order=order, reynolds=1600.0, dt=1e-3, steps=2, time_order=3,
        device=DEV, tol=1e-12, sem=sem, pressure_preconditioner=schwarz)
    assert all(s == ('converged', 'converged') for s in diag['cg_status']), \
        diag['cg_status']
    assert relerr(u, c.v.from_base(uo)) < 1e-8, vnum
    assert np.abs(_np(p) - c.p.from_base(po)).max() < 1e-7 * max(
        1.0, np.abs(po).max()), vnum
    assert diag['max_divergence'] < 1e-6
    counts[vnum] = diag['cg_iterations']
  for vnum in pairs:
    _close_counts(counts[vnum], counts['refiner'], 'taylor_green')
