"""Host-side checks of fields at points: the NumPy reference
(`tests/point_reference.py`) against itself, the candidate grid and the plan
on CPU meshes, the ctypes mirrors of the argument structs and the refusals of
`PointEvaluator.from_location`.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from swirl_fem_amd import _lib
from swirl_fem_amd.core import points as PT
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType
from tests import geometry_cases as G
from tests import point_reference as PR

F64 = torch.float64
GLL = NodeType.GAUSS_LOBATTO_LEGENDRE


def _case(name, ndim, P1):
  if name == 'three_kinds':
    return G.three_kinds(3, ndim, P1, pad=2)
  return getattr(G, name)(3, ndim, P1)


def _cpu_mesh(name, ndim, P1):
  case = _case(name, ndim, P1)
  mesh, _, rp = case.finalize('cpu', F64)
  return mesh, rp


# ------------------------------------------------------ reference self-checks
@pytest.mark.parametrize('ndim,P1', [(2, 2), (2, 5), (3, 4)])
def test_reference_rows(ndim, P1):
  """Rows of the dense matrix sum to 1, rows at the nodes are unit vectors,
  and the matrix-free forms are the matrix's action."""
  rp = G.three_kinds(3, ndim, P1).rp
  nodes = rp.gridpoints_1d.node_values
  rng = np.random.default_rng(1)
  e0, xi0, _ = PR.make_points(rng, rp.node_coords, rp.elements, nodes, 200)
  N = rp.node_coords.shape[0]
  D = PR.dense_matrix(rp.elements, nodes, e0, xi0, N)
  assert np.abs(D.sum(axis=1) - 1.0).max() <= 1e-12
  # every node of element 3, as a point of element 3
  grid = np.stack(np.meshgrid(*[nodes] * ndim, indexing='ij'), -1)
  xin = grid.reshape(-1, ndim)
  en = np.full(len(xin), 3)
  Dn = PR.dense_matrix(rp.elements, nodes, en, xin, N)
  want = np.zeros_like(Dn)
  want[np.arange(len(xin)), rp.elements[3]] = 1.0
  assert np.abs(Dn - want).max() <= 1e-13
  u = rng.standard_normal((N, 3))
  w = rng.standard_normal((200, 3))
  assert np.abs(PR.evaluate(rp.elements, nodes, e0, xi0, u) - D @ u).max() \
      <= 1e-13
  assert np.abs(PR.evaluate_t(rp.elements, nodes, e0, xi0, w, N) -
                D.T @ w).max() <= 1e-13
  # derivatives of the 1D basis against a central difference
  x = rng.uniform(-1, 1, 7)
  _, der = PR.lagrange(nodes, x)
  h = 1e-6
  cd = (PR.lagrange(nodes, x + h)[0] - PR.lagrange(nodes, x - h)[0]) / (2 * h)
  assert np.abs(der - cd).max() <= 1e-8 * max(1.0, np.abs(der).max())


@pytest.mark.parametrize('ndim,P1', [(2, 4), (3, 3), (3, 5)])
def test_reference_reproduces_polynomials(ndim, P1):
  """A polynomial in x of total degree <= P on an affine mesh is in the
  space: the dense matrix reproduces it to 1e-12."""
  rp = G.affine(3, ndim, P1).rp
  nodes = rp.gridpoints_1d.node_values
  rng = np.random.default_rng(2)
  e0, xi0, x = PR.make_points(rng, rp.node_coords, rp.elements, nodes, 300)
  P = P1 - 1

  def poly(y):
    return (1.0 + y @ np.arange(1, ndim + 1)) ** P - 0.5 * y[:, 0] ** P

  u = poly(np.asarray(rp.node_coords, np.float64))
  got = PR.evaluate(rp.elements, nodes, e0, xi0, u)
  want = poly(x)
  assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize('name,ndim,P1', [
    ('three_kinds', 2, 5), ('curved_multilinear', 3, 3)])
def test_reference_locator(name, ndim, P1):
  """The NumPy locator finds every inside point with the residual at
  rounding, returns e0 away from the faces and rejects outside points."""
  rp = _case(name, ndim, P1).rp
  nodes = rp.gridpoints_1d.node_values
  rng = np.random.default_rng(3)
  e0, xi0, x = PR.make_points(rng, rp.node_coords, rp.elements, nodes, 300)
  out = PR.outside_points(rng, rp.node_coords, 20)
  element, xi, found = PR.locate(rp.node_coords, rp.elements, nodes,
                                 np.concatenate([x, out]))
  assert found[:300].all() and not found[300:].any()
  assert np.abs(xi).max() <= 1 + 1e-10
  back, _ = PR.nodal_map(rp.node_coords, rp.elements, nodes, element[:300],
                         xi[:300])
  ext = PR.extents(rp.node_coords, rp.elements)[element[:300]]
  assert (np.abs(back - x).max(axis=1) <= 1e-12 * ext).all()
  inner = np.abs(xi0).max(axis=1) <= 0.9
  assert (element[:300][inner] == e0[inner]).all()


# ------------------------------------------------------ plan logic on the CPU
@pytest.mark.parametrize('name', ['three_kinds', 'curved_multilinear',
                                  'periodic'])
@pytest.mark.parametrize('ndim,P1', [(2, 2), (2, 5), (3, 4)])
def test_candidate_grid_is_complete(name, ndim, P1):
  """The candidate list of every test point's cell contains e0, holds real
  elements only, in ascending order; about one element per cell."""
  mesh, rp = _cpu_mesh(name, ndim, P1)
  nodes = rp.gridpoints_1d.node_values
  rng = np.random.default_rng(4)
  e0, _, x = PR.make_points(rng, rp.node_coords, mesh.elements.numpy(), nodes,
                            400)
  grid = PT.CandidateGrid.build(mesh)
  real = (mesh.elements.numpy() >= 0).all(axis=1)
  cells = int(grid.ncell.prod())
  assert 0.5 * real.sum() <= cells <= 2 * real.sum()
  offsets = grid.cell_offsets.numpy()
  elems = grid.cell_elems.numpy()
  assert offsets[0] == 0 and offsets[-1] == len(elems)
  assert len(offsets) == cells + 1 and (np.diff(offsets) >= 0).all()
  assert real[elems].all()
  for c in range(cells):
    assert (np.diff(elems[offsets[c]:offsets[c + 1]]) > 0).all()
  assert ((x >= grid.lo) & (x <= grid.hi)).all()
  cell = grid.cell_of(x)
  for m in range(len(x)):
    assert e0[m] in elems[offsets[cell[m]]:offsets[cell[m] + 1]], m
  # boxes: the inflated node boxes of the reference; padded rows empty
  lo, hi, _ = PR.element_boxes(rp.node_coords, mesh.elements.numpy())
  side = hi - lo
  boxes = grid.boxes.numpy()
  assert np.abs(boxes[real, 0] - (lo - 0.1 * side)[real]).max() <= 1e-15
  assert np.abs(boxes[real, 1] - (hi + 0.1 * side)[real]).max() <= 1e-15
  assert np.abs(grid.extent.numpy()[real] - side.max(axis=1)[real]).max() == 0
  assert (grid.extent.numpy()[~real] == 0).all()


@pytest.mark.parametrize('name', ['three_kinds', 'curved_multilinear',
                                  'periodic'])
@pytest.mark.parametrize('ndim,P1', [(2, 3), (3, 2)])
def test_plan_is_a_partition(name, ndim, P1):
  """perm, segments and chunks partition the found points: stable order by
  element, one segment per touched element, chunks of at most 64 points of
  one element; the CSR of the touched rows is their inverse map."""
  mesh, rp = _cpu_mesh(name, ndim, P1)
  nodes = rp.gridpoints_1d.node_values
  rng = np.random.default_rng(5)
  el = mesh.elements.numpy()
  e0, xi0, _ = PR.make_points(rng, rp.node_coords, el, nodes, 500)
  e0[rng.integers(0, 500, 40)] = -1              # some points not found
  e0[100:200] = e0[100]                          # 100 points in one element
  e0[e0 == 1] = 2                                # element 1 has no point
  ev = PT.PointEvaluator.from_location(
      mesh, torch.as_tensor(e0, dtype=torch.int32), torch.as_tensor(xi0))
  assert (ev.found.numpy() == (e0 >= 0)).all()
  plan = ev.plan
  perm = plan.perm.numpy()
  hit = np.flatnonzero(e0 >= 0)
  assert sorted(perm) == list(hit)
  want = hit[np.argsort(e0[hit], kind='stable')]
  assert (perm == want).all()
  assert (plan.xi.numpy() == xi0[perm]).all()
  seg_elem, so = plan.seg_elem.numpy(), plan.seg_offsets.numpy()
  assert (np.diff(seg_elem) > 0).all() and 1 not in seg_elem
  assert so[0] == 0 and so[-1] == len(perm)
  for s, e in enumerate(seg_elem):
    assert (e0[perm[so[s]:so[s + 1]]] == e).all() and so[s + 1] > so[s]
  ce, cs, cc = (plan.chunk_elem.numpy(), plan.chunk_start.numpy(),
                plan.chunk_count.numpy())
  assert (cc >= 1).all() and (cc <= PT.CHUNK).all() and cc.sum() == len(perm)
  assert cs[0] == 0 and (cs[1:] == np.cumsum(cc)[:-1]).all()
  for k in range(len(ce)):
    assert (e0[perm[cs[k]:cs[k] + cc[k]]] == ce[k]).all()
  # a full chunk is followed by the rest of the same element
  assert cc.max() == PT.CHUNK and (np.bincount(ce)[e0[100]] == 2 or
                                   np.bincount(ce)[e0[100]] == 3)
  offsets, slots = plan.scatter_csr
  offsets, slots = offsets.numpy(), slots.numpy()
  flat = el[seg_elem].reshape(-1)
  assert len(offsets) == mesh.num_nodes + 1 and offsets[-1] == len(flat)
  for v in rng.integers(0, mesh.num_nodes, 50):
    mine = slots[offsets[v]:offsets[v + 1]]
    assert (flat[mine] == v).all() and (np.diff(mine) > 0).all()
    assert len(mine) == (flat == v).sum()


def test_plan_without_points():
  mesh, _ = _cpu_mesh('three_kinds', 2, 3)
  ev = PT.PointEvaluator.from_location(
      mesh, torch.full((5,), -1, dtype=torch.int32),
      torch.zeros((5, 2), dtype=F64))
  assert ev.plan.num_found == 0 and ev.plan.chunk_elem.numel() == 0
  assert ev.plan.seg_offsets.tolist() == [0] and not ev.found.any()


@pytest.mark.parametrize('node_type', [GLL, NodeType.NEWTON_COTES,
                                       NodeType.GAUSS_LEGENDRE])
def test_basis_tables_any_node_family(node_type):
  """bary = 1 / prod (x_i - x_k) for any Nodes1D: the product form gives the
  cardinal property and a partition of unity."""
  grid = Nodes1D.create(6, node_type)
  x, w = PT.basis_tables(grid)
  assert (x == grid.node_values).all()
  val, _ = PR.lagrange(x, x)
  assert np.abs(val - np.eye(6)).max() <= 1e-13
  y = np.linspace(-1, 1, 11)
  d = y[:, None] - x[None, :]
  l = np.stack([w[i] * np.delete(d, i, axis=1).prod(axis=1)
                for i in range(6)], axis=1)
  assert np.abs(l.sum(axis=1) - 1.0).max() <= 1e-13
  assert np.abs(l - PR.lagrange(x, y)[0]).max() <= 1e-14


# ------------------------------------------------------------- struct layouts
def _header_struct(name):
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  text = open(os.path.join(root, 'include', 'sfem.h')).read()
  assert '#define SFEM_ABI_VERSION 10' in text and _lib.ABI_VERSION == 10
  body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), text,
                   flags=re.S).group(1)
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  fields = []                                    # (name, array length or 0)
  for decl in body.split(';'):
    decl = decl.strip()
    if not decl:
      continue
    first, *rest = decl.split(',')
    m = re.search(r'(\w+)\s*\[\s*(\d+)\s*\]$', first)
    if m:
      fields.append((m.group(1), int(m.group(2))))
    else:
      fields.append((re.findall(r'\w+', first)[-1], 0))
    fields += [(r.strip(), 0) for r in rest]
  return text, fields


@pytest.mark.parametrize('cname,mirror,size', [
    # 12 pointers, 3 arrays of 3 doubles, 2 doubles, 3 int64, 7 int32 (+ pad)
    ('sfem_point_locate_args', _lib.PointLocateArgs,
     12 * 8 + 72 + 16 + 24 + 32),
    # 13 pointers, 8 int64, 4 int32
    ('sfem_point_args', _lib.PointArgs, 13 * 8 + 64 + 16)])
def test_struct_layout(cname, mirror, size):
  """The header's struct and its ctypes mirror: the same fields in the same
  order, the same arrays; the ABI number is unchanged (a pure addition)."""
  text, fields = _header_struct(cname)
  assert [f[0] for f in fields] == [f[0] for f in mirror._fields_]
  for (name, length), (_, ctype) in zip(fields, mirror._fields_):
    if length:
      assert issubclass(ctype, ctypes.Array) and ctype._length_ == length, name
    else:
      assert not issubclass(ctype, ctypes.Array), name
  assert ctypes.sizeof(mirror) == size
  chunk = int(re.search(r'#define SFEM_POINT_CHUNK (\d+)', text).group(1))
  assert chunk == _lib.SFEM_POINT_CHUNK == PT.CHUNK == 64
  for fn in ('sfem_point_eval', 'sfem_point_eval_t'):
    assert _lib.SIGNATURES[fn][0]._type_ is _lib.PointArgs
  assert _lib.SIGNATURES['sfem_point_locate'][0]._type_ is _lib.PointLocateArgs


def test_entry_points_refuse_bad_arguments():
  """SFEM_EINVAL / SFEM_EUNSUPPORTED with a message, without a GPU."""
  lib = _lib.load()
  x = (ctypes.c_double * 2)(-1.0, 1.0)
  ptr = ctypes.cast(x, ctypes.c_void_p)
  assert lib.sfem_point_eval(None, None) == -1
  assert b'null args' in lib.sfem_last_error()
  a = _lib.PointArgs(ncomp=1, ndim=3, P1=13, dtype=1, nodes=ptr, bary=ptr)
  assert lib.sfem_point_eval(ctypes.byref(a), None) == -3
  assert b'P1=13' in lib.sfem_last_error()
  a = _lib.PointArgs(ncomp=1, ndim=4, P1=2, dtype=1, nodes=ptr, bary=ptr)
  assert lib.sfem_point_eval_t(ctypes.byref(a), None) == -3
  a = _lib.PointArgs(ncomp=0, ndim=3, P1=2, dtype=1, nodes=ptr, bary=ptr)
  assert lib.sfem_point_eval(ctypes.byref(a), None) == -1
  assert b'ncomp' in lib.sfem_last_error()
  a = _lib.PointArgs(ncomp=1, ndim=3, P1=2, dtype=1, nodes=ptr, bary=ptr,
                     num_points=4, num_found=4, num_chunks=1, num_segments=1)
  assert lib.sfem_point_eval(ctypes.byref(a), None) == -1
  assert b'null pointer' in lib.sfem_last_error()
  assert lib.sfem_point_eval_t(ctypes.byref(a), None) == -1
  a.num_found = 5
  assert lib.sfem_point_eval(ctypes.byref(a), None) == -1
  b = _lib.PointLocateArgs(ndim=3, P1=2, dtype=1, nodes=ptr, bary=ptr,
                           max_iter=10, num_points=3)
  b.ncell[0] = b.ncell[1] = b.ncell[2] = 1
  assert lib.sfem_point_locate(ctypes.byref(b), None) == -1
  assert b'null pointer' in lib.sfem_last_error()
  b.max_iter = 1000
  assert lib.sfem_point_locate(ctypes.byref(b), None) == -1
  assert b'max_iter' in lib.sfem_last_error()
  b.max_iter, b.P1 = 10, 13
  assert lib.sfem_point_locate(ctypes.byref(b), None) == -3
  b.P1, b.ncell[1] = 2, 0
  assert lib.sfem_point_locate(ctypes.byref(b), None) == -1
  assert b'ncell' in lib.sfem_last_error()
  b.ncell[1], b.tol_x = 1, -1.0
  assert lib.sfem_point_locate(ctypes.byref(b), None) == -1
  b.tol_x, b.num_points = 0.0, 0
  assert lib.sfem_point_locate(ctypes.byref(b), None) == 0


# ------------------------------------------------------------------ refusals
def test_from_location_refusals():
  mesh, _ = _cpu_mesh('three_kinds', 2, 3)      # 9 real + 2 padded rows
  E = mesh.num_elements
  i32 = lambda v: torch.as_tensor(v, dtype=torch.int32)
  xi = torch.zeros((3, 2), dtype=F64)
  ok = i32([0, -1, 8])
  PT.PointEvaluator.from_location(mesh, ok, xi)
  bad = [
      (i32([[0, 1, 2]]), xi),                        # element shape
      (ok.to(torch.float64), xi),                    # element dtype
      (ok, torch.zeros((3, 3), dtype=F64)),          # xi shape
      (ok, torch.zeros((2, 2), dtype=F64)),          # xi length
      (ok, xi.to(torch.float32)),                    # xi dtype
      (i32([0, -2, 8]), xi),                         # below -1
      (i32([0, 1, E]), xi),                          # beyond E
      (i32([0, 1, E - 1]), xi),                      # a padded row
      (ok, torch.tensor([[0., 0.], [0., 0.], [0., 1.6]], dtype=F64)),
      (ok, torch.tensor([[0., 0.], [0., 0.], [np.nan, 0.]], dtype=F64)),
      (ok, torch.tensor([[np.inf, 0.], [0., 0.], [0., 0.]], dtype=F64)),
  ]
  for element, x in bad:
    with pytest.raises(ValueError):
      PT.PointEvaluator.from_location(mesh, element, x)
  if torch.cuda.is_available():
    with pytest.raises(ValueError):                  # device
      PT.PointEvaluator.from_location(mesh, ok.cuda(), xi.cuda())
  # xi of a not-found point is not read
  PT.PointEvaluator.from_location(
      mesh, ok, torch.tensor([[0., 0.], [np.nan, 9.], [0., 1.5]], dtype=F64))
  with pytest.raises(NotImplementedError):
    PT.PointEvaluator.from_location(mesh, ok, xi.clone().requires_grad_(True))
  with pytest.raises(NotImplementedError):
    PT.PointEvaluator.from_location(mesh.replicate(2), ok, xi)
  with pytest.raises(NotImplementedError):
    PT.PointEvaluator.from_location(mesh.replace(axis_name='i'), ok, xi)
  with pytest.raises(NotImplementedError):
    PT.locate_points(mesh.replicate(2), torch.zeros((3, 2), dtype=F64))
  with pytest.raises(NotImplementedError):
    PT.locate_points(mesh, torch.zeros((3, 2), dtype=F64, requires_grad=True))
  for pts in (torch.zeros((3, 3), dtype=F64), torch.zeros(3, dtype=F64),
              torch.zeros((3, 2), dtype=torch.float32)):
    with pytest.raises(ValueError):
      PT.locate_points(mesh, pts)
  # the kernels have no CPU fallback
  ev = PT.PointEvaluator.from_location(mesh, ok, xi)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    ev(torch.zeros(mesh.num_nodes, dtype=F64))
  with pytest.raises(ValueError):
    ev(torch.zeros(mesh.num_nodes + 1, dtype=F64))
  with pytest.raises(ValueError):
    ev.transpose(torch.zeros(4, dtype=F64))
  with pytest.raises(ValueError):
    ev(torch.zeros(mesh.num_nodes, dtype=torch.float32))
