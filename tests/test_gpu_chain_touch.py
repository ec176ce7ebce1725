"""The touch of the Helmholtz chain kernels (`facet_touch`,
`csrc/sfem_helmholtz_facet.h`, switch `SFEM_CHAIN_TOUCH`): a wave loads the
nodes of its next element one compute phase before it gathers them and throws
the result away.  Nothing the program reads may depend on it:

* operator applies with `SFEM_CHAIN_TOUCH=1` against `=0` on the same operator
  and input -- layered assembly bit for bit (extended output and per-wave
  partial sums of u . out), atomic assembly within the tolerance of the
  assembly-mode tests (`tests/fp32util.tolerance`: atomics reorder);
* the touched result against `tests/sumfact_reference.py`;
* 20 CG iterations bit for bit;
* the rule that switches it on (`sfem_chain_touch_enabled`, no GPU).

Mesh: 6 x 6 x 6 hexahedra (79 507 nodes at p = 7).  The touch is shipped
switched off (it measured slower, `profiles/chain_touch_notes.md`) and its
`auto` setting starts at 256 MiB, so every case sets the switch; the library
reads it per launch.

Orders: p = 2, 4, 7 (P = 3, 5, 8 points per direction).  The chain kernels
exist for P = 6..8 only -- P = 3 and 5 run the index-row kernels, which the
switch must leave alone -- so P = 6 and 7, the chain sizes that leave lanes
of the wave without a line of the element (36 and 49 of 64), are added.
"""
import ctypes

import numpy as np
import pytest
import torch

from swirl_fem_amd import _lib
from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
from swirl_fem_amd.core import operators
from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType, Quadrature1D
from swirl_fem_amd.core.mesh_refiner import refine_premesh
from tests.fp32util import F32Rng, f32_mesh, tolerance
from tests.sumfact_reference import Space

DEV = 'cuda:0'
GLL = NodeType.GAUSS_LOBATTO_LEGENDRE
N_ELEMS = 6
F64, F32 = torch.float64, torch.float32
# (mesh deformation, geometry argument of the operator)
GEOMETRIES = {'box': ('box', 'auto'), 'affine': ('sheared', 'auto'),
              'multilinear': ('jitter', 'auto'), 'stored': ('jitter', 'stored')}
# no successor (one element per wave: the kernel that never touches), one
# successor, the table request two ahead live, a full line
CHAIN_LENS = ('1', '2', '3', '6')


def _premesh(kind):
  pm = unit_cube_mesh(N_ELEMS, ndim=3)
  x = pm.node_coords.copy()
  if kind == 'sheared':
    shear = np.array([[0.0, 0.25, -0.125], [0.125, 0.0, 0.25],
                      [-0.25, 0.125, 0.0]])
    x = x @ (np.eye(3) + shear).T + 0.125
  elif kind == 'jitter':    # the smooth deformation of `bench.py --jitter 0.2`
    s = np.prod(np.sin(np.pi * x), axis=1)
    x = x + 0.2 / N_ELEMS * s[:, None] * np.cos(2 * np.pi * x[:, ::-1])
  return pm.replace(node_coords=x)


_CASES = {}


def _case(P, geo, dtype):
  """(refined premesh, mesh, space, mask, u on the host, u on the device),
  built once per (P, geometry, dtype) and left unchanged."""
  key = (P, geo, dtype)
  if key not in _CASES:
    rp = f32_mesh(refine_premesh(_premesh(GEOMETRIES[geo][0]),
                                 Nodes1D.create(P, GLL)), dtype)
    mesh = rp.finalize(device=DEV, dtype=dtype)
    fes = FiniteElementSpace.create(
        mesh, Quadrature1D.create_from_nodes_1d(Nodes1D.create(P, GLL)))
    u = F32Rng(17 * P + len(geo)).standard_normal(mesh.num_nodes)
    ud = torch.as_tensor(u, device=DEV, dtype=dtype)
    _CASES.clear()                       # one case alive at a time
    _CASES[key] = (rp, mesh, fes, mesh.physical_masks['boundary'], u, ud)
  return _CASES[key]


def _operator(fes, mask, geo, P, chain_len, monkeypatch):
  """A fresh (not cached) operator: the chain length is read at setup."""
  monkeypatch.setenv('SFEM_CHAIN_LEN', chain_len)
  op = operators.HelmholtzOperator.create(fes, mask, GEOMETRIES[geo][1])
  if 6 <= P <= 8:
    # (segments of one element are launched one element per wave)
    chained = chain_len != '1'
    assert op.facet_parts
    assert all(('chains' in q) == chained for q in op.facet_parts)
    assert ('helmholtz_chain_kernel' in op.kernel_name()) == chained
  else:
    assert op.facet_parts is None
  return op


def _apply(op, ud, l0, l1, layered, touch, monkeypatch):
  """(result, partial sums of u . out) with the switch set to `touch`."""
  monkeypatch.setenv('SFEM_CHAIN_TOUCH', touch)
  if layered:
    ext = op.new_extended()
    dot = torch.zeros(op.layered_dot_slots(), dtype=F64, device=DEV)
    op.apply_layered(ud, ext, l0, l1, dot_out=dot, per_wave=True)
    return ext, dot
  dot = torch.zeros(_lib.SFEM_DOT_SLOTS, dtype=F64, device=DEV)
  return op.apply(ud, l0, l1, dot_out=dot), dot


def _relerr(a, b):
  a, b = a.double(), b.double()
  return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
@pytest.mark.parametrize('geo', list(GEOMETRIES))
@pytest.mark.parametrize('P', [3, 5, 6, 7, 8])
def test_apply_with_touch_equals_apply_without(P, geo, dtype, monkeypatch):
  """Every chain length x assembly x mass coefficient of one (order,
  geometry, precision), Dirichlet mask on."""
  rp, mesh, fes, mask, u, ud = _case(P, geo, dtype)
  tol = tolerance(dtype, P)
  for chain_len in CHAIN_LENS:
    for layered in (True, False):
      monkeypatch.setenv('SFEM_LAYERED', '1' if layered else '0')
      op = _operator(fes, mask, geo, P, chain_len, monkeypatch)
      if layered and op.layer_plan() is None:
        assert not 6 <= P <= 8      # index rows have no layers
        continue
      for l0 in (0.0, 1.0):
        what = (chain_len, layered, l0)
        off, dot_off = _apply(op, ud, l0, 1.0, layered, '0', monkeypatch)
        on, dot_on = _apply(op, ud, l0, 1.0, layered, '1', monkeypatch)
        assert bool(torch.isfinite(on).all()), what
        assert float(off.abs().max()) > 0, what
        if layered:
          assert torch.equal(on, off), what
          assert torch.equal(dot_on, dot_off), what
        else:
          err = _relerr(on, off)
          print('touch 1 vs 0, atomic', P, geo, dtype, what, 'relerr', err)
          assert err < tol, what + (err,)
          scale = float((ud.double() * off.double()).abs().sum())
          assert abs(float(dot_on.sum()) - float(dot_off.sum())) <= \
              10 * tol * scale, what


@pytest.mark.gpu
@pytest.mark.parametrize('layered', [True, False], ids=['layered', 'atomic'])
def test_touch_with_64_bit_addresses(layered, monkeypatch):
  """The touch forms the address the gather forms: here the 64-bit one."""
  P = 8
  monkeypatch.setenv('SFEM_FACET_OFF64', '1')
  monkeypatch.setenv('SFEM_LAYERED', '1' if layered else '0')
  for geo in ('box', 'multilinear'):
    rp, mesh, fes, mask, u, ud = _case(P, geo, F64)
    op = _operator(fes, mask, geo, P, '3', monkeypatch)
    off, dot_off = _apply(op, ud, 0.5, 1.0, layered, '0', monkeypatch)
    on, dot_on = _apply(op, ud, 0.5, 1.0, layered, '1', monkeypatch)
    if layered:
      assert torch.equal(on, off) and torch.equal(dot_on, dot_off), geo
    else:
      assert _relerr(on, off) < tolerance(F64, P), geo


@pytest.mark.gpu
@pytest.mark.parametrize('geo', ['box', 'multilinear'])
def test_touched_apply_matches_the_reference(geo, monkeypatch):
  """`tests/sumfact_reference.py`, tolerance of the chain tests of
  `tests/test_gpu_facet.py`."""
  P = 8
  rp, mesh, fes, mask, u, ud = _case(P, geo, F64)
  keep = 1.0 - mask.cpu().numpy().astype(np.float64)
  ref = Space(rp.node_coords, rp.elements, P).apply(u, 0.6, 1.4, keep=keep)
  for layered in (True, False):
    monkeypatch.setenv('SFEM_LAYERED', '1' if layered else '0')
    op = _operator(fes, mask, geo, P, '3', monkeypatch)
    got, _ = _apply(op, ud, 0.6, 1.4, layered, '1', monkeypatch)
    if layered:
      from swirl_fem_amd import _ops
      got = _ops.fold_layers(got, mesh.num_nodes, op.layer_plan().layers)
    err = np.abs(got.cpu().numpy() - ref).max() / np.abs(ref).max()
    print('touch 1 vs sumfact reference', geo, layered, 'relerr', err)
    assert err < tolerance(F64, P), (geo, layered, err)


@pytest.mark.gpu
def test_cg_with_touch_is_bitwise_the_same(monkeypatch):
  """20 iterations of the layered, deterministic CG: x and the residual."""
  from swirl_fem_amd.linalg.cg import CGRunner
  P = 8
  monkeypatch.setenv('SFEM_LAZY_X_MIN_MB', '0')
  rp, mesh, fes, mask, u, ud = _case(P, 'box', F64)
  op = _operator(fes, mask, 'box', P, '3', monkeypatch)
  A = op.linear_operator(0.0, 1.0)
  b = ud * ~mask
  got = {}
  for touch in ('0', '1'):
    monkeypatch.setenv('SFEM_CHAIN_TOUCH', touch)
    run = CGRunner(A, b, tol=0.0, maxiter=10 ** 6)
    assert run.layered is not None and run.det is not None
    assert run.lazy is not None
    for _ in range(20):
      run.step()
    info = run.info()
    assert info['num_iterations'] == 20
    got[touch] = (run.x.clone(), info['residual'])
  assert torch.equal(got['1'][0], got['0'][0])
  assert got['1'][1] == got['0'][1]
  assert float(got['1'][0].abs().max()) > 0


def test_auto_touches_fields_that_do_not_stay_in_the_caches(monkeypatch):
  """`sfem_chain_touch_enabled`: auto = from 1 << 28 bytes on (the threshold
  of the non-temporal vector kernels), 1 always, 0 and unset never (the touch
  measured slower: it is shipped switched off)."""
  lib = _lib.load()
  on = lambda nbytes: lib.sfem_chain_touch_enabled(ctypes.c_int64(nbytes))
  edge = 1 << 28
  monkeypatch.setenv('SFEM_CHAIN_TOUCH', 'auto')
  assert [on(0), on(edge - 1), on(edge), on(edge + 1), on(1 << 40)] == \
      [0, 0, 1, 1, 1]
  monkeypatch.setenv('SFEM_CHAIN_TOUCH', '1')
  assert [on(0), on(edge - 1), on(edge)] == [1, 1, 1]
  from swirl_fem_amd import switches
  assert switches.active().get('SFEM_CHAIN_TOUCH') == '1'
  monkeypatch.setenv('SFEM_CHAIN_TOUCH', '0')
  assert [on(0), on(edge), on(1 << 40)] == [0, 0, 0]
  monkeypatch.delenv('SFEM_CHAIN_TOUCH')
  assert [on(0), on(edge), on(1 << 40)] == [0, 0, 0]
  assert switches.SWITCHES['SFEM_CHAIN_TOUCH'][0] == '0'
  assert 'SFEM_CHAIN_TOUCH' not in switches.active()
