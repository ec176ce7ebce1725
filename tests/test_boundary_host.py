"""Boundary facets on the `Mesh` (host side of the boundary integrals): every
facet is a face of exactly one element and a consistent tensor grid, periodic
directions carry none, the facet CSR sums every slot once, and the refusals
of `boundary_covector` / `solve_helmholtz`.  Runs without a GPU."""
import itertools
import os

import numpy as np
import pytest
import torch

from swirl_fem_amd.common import mesh_reader
from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
from swirl_fem_amd.core import interpolation as I
from swirl_fem_amd.core.fespace import FiniteElementSpace, boundary_csr
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType, Quadrature1D
from swirl_fem_amd.core.mesh_refiner import refine_premesh
from swirl_fem_amd.core.premesh import Premesh
from swirl_fem_amd.examples.helmholtz import BCType, solve_helmholtz
from tests import bvp_reference as R

MSH = os.path.join(os.path.dirname(__file__), 'golden', 'msh')
GLL = NodeType.GAUSS_LOBATTO_LEGENDRE


def _faces_of_refined(elements, ndim, P):
  """(E * 2 ndim, P^(ndim-1)) node rows of every face of refined elements."""
  el = np.asarray(elements).reshape([-1] + [P] * ndim)
  out = []
  for a in range(ndim):
    for s in (0, P - 1):
      out.append(np.take(el, s, axis=1 + a).reshape(len(el), -1))
  return np.concatenate(out, axis=0)


def _check_facets(rp, mesh, P, ndim):
  """Face of exactly one element; nodes = multilinear image of the corners."""
  faces = np.sort(_faces_of_refined(rp.elements, ndim, P), axis=1)
  fkeys = {tuple(r) for r in faces}
  counts = {}
  for r in map(tuple, faces):
    counts[r] = counts.get(r, 0) + 1
  k = ndim - 1
  grid = Nodes1D.create(P, GLL)
  i1, _ = I.matrices_1d(Nodes1D.create(2, NodeType.NEWTON_COTES), grid)
  interp = np.asarray(i1)
  for _ in range(k - 1):
    interp = np.kron(interp, np.asarray(i1))
  corner_pos = [0, P - 1] if k == 1 else [0, P - 1, P * (P - 1), P * P - 1]
  x = np.asarray(rp.node_coords)
  for name, f in mesh.boundary_facets.items():
    f = f.cpu().numpy()
    assert f.dtype == np.int32 and f.shape[1] == P ** k
    for row in f:
      key = tuple(np.sort(row))
      assert key in fkeys and counts[key] == 1, name
    want = np.einsum('ij,fjd->fid', interp, x[f[:, corner_pos]])
    np.testing.assert_allclose(x[f], want, atol=1e-12)


def _csr_check(facets, n):
  offsets, slots = boundary_csr(facets, n)
  assert offsets[-1] == facets.size
  assert sorted(slots.tolist()) == list(range(facets.size))
  flat = facets.reshape(-1)
  for v in range(n):
    seg = slots[offsets[v]:offsets[v + 1]]
    assert (np.diff(seg) > 0).all() and (flat[seg] == v).all()


@pytest.mark.parametrize('ndim,n,P,periodic,jitter', [
    (2, 3, 4, (), 0.0), (3, 2, 3, (), 0.1), (2, 3, 5, (0,), 0.0),
    (3, 2, 4, (0, 1), 0.1), (3, 2, 2, (2,), 0.0)])
def test_unit_cube_facets(ndim, n, P, periodic, jitter):
  rng = np.random.default_rng(P)
  pm = unit_cube_mesh(n, ndim=ndim, periodic_dims=periodic)
  if jitter:
    pm = pm.replace(node_coords=pm.node_coords + jitter / n * rng.uniform(
        -1, 1, pm.node_coords.shape))
  rp = refine_premesh(pm, Nodes1D.create(P, GLL))
  mesh = rp.finalize(device='cpu')
  f = mesh.boundary_facets['boundary'].numpy()
  assert f.shape[0] == 2 * (ndim - len(periodic)) * n ** (ndim - 1)
  _check_facets(rp, mesh, P, ndim)
  # a periodic direction contributes no facets: no facet lies on x_a = 0 / 1
  x = np.asarray(rp.node_coords)
  for a in periodic:
    on_side = np.all(np.isclose(x[f][..., a], 0.0), axis=1) | np.all(
        np.isclose(x[f][..., a], 1.0), axis=1)
    assert not on_side.any()
  _csr_check(f, mesh.num_nodes)


@pytest.mark.parametrize('ndim,n', [(2, 3), (3, 2)])
def test_random_orientations_facets(ndim, n):
  """Elements with random vertex orderings (the default 'corrected' refiner):
  every facet stays a consistent tensor grid."""
  rng = np.random.default_rng(7)
  base = unit_cube_mesh(n, ndim=ndim)
  x = base.node_coords + 0.1 / n * rng.uniform(-1, 1, base.node_coords.shape)
  orients = [(perm, axes) for perm in itertools.permutations(range(ndim))
             for r in range(ndim + 1)
             for axes in itertools.combinations(range(ndim), r)]
  for _ in range(5):
    el = []
    for e in base.elements[rng.permutation(base.num_elements)]:
      perm, axes = orients[rng.integers(len(orients))]
      el.append(np.flip(e.reshape([2] * ndim).transpose(perm),
                        axes).reshape(-1))
    pm = base.replace(node_coords=x, elements=np.array(el, dtype=np.int32))
    rp = refine_premesh(pm, Nodes1D.create(4, GLL))
    _check_facets(rp, rp.finalize(device='cpu'), 4, ndim)


def _gmsh_groups(name, ndim):
  pm = mesh_reader.read(os.path.join(MSH, name), ndim=ndim)
  x = np.asarray(pm.node_coords)
  lo, hi = x.min(axis=0), x.max(axis=0)
  if ndim == 2:
    def classify(c):
      for nm, ax, v in (('left', 0, lo[0]), ('right', 0, hi[0]),
                        ('bottom', 1, lo[1]), ('top', 1, hi[1])):
        if abs(c[ax] - v) < 1e-9:
          return nm
      return None
  else:
    def classify(c):
      if abs(c[2] - hi[2]) < 1e-9:
        return 'top'
      if abs(c[2] - lo[2]) < 1e-9:
        return 'bottom'
      return 'sides'
  return pm.replace(physical_groups=R.boundary_groups(pm, classify))


@pytest.mark.parametrize('name,ndim', [('kovasznay.msh', 2), ('cube.msh', 3)])
def test_gmsh_facets(name, ndim):
  pm = _gmsh_groups(name, ndim)
  rp = refine_premesh(pm, Nodes1D.create(3, GLL))
  mesh = rp.finalize(device='cpu')
  assert set(mesh.boundary_facets) == set(pm.physical_groups)
  _check_facets(rp, mesh, 3, ndim)
  for f in mesh.boundary_facets.values():
    _csr_check(f.numpy(), mesh.num_nodes)


def test_facet_fields_follow_the_mesh():
  rp = refine_premesh(unit_cube_mesh(2, ndim=2), Nodes1D.create(3, GLL))
  mesh = rp.finalize(device='cpu')
  assert 'boundary' in mesh.replace().boundary_facets
  assert mesh.replicate(1).boundary_facets is mesh.boundary_facets
  assert mesh.replicate(3).boundary_facets == {}
  # partitioned finalisation leaves the facets empty
  pp = unit_cube_mesh(4, ndim=2, partitions=np.arange(2).reshape(2, 1))
  part = pp.finalize('x', rank=0, device='cpu')
  assert part.boundary_facets == {}


def test_unreadable_groups_get_no_facets():
  # 1D: every id of a group is a boundary point, whatever the array's shape
  nn = 9
  pm = Premesh.create(np.linspace(0, 1, nn).reshape(nn, 1),
                      np.array([[i, i + 1] for i in range(nn - 1)]),
                      physical_groups={'boundary': [[0, nn - 1]]})
  f = pm.finalize(device='cpu').boundary_facets['boundary']
  assert f.tolist() == [[0], [nn - 1]]
  # 2D: a group that is not (F, P^(d-1)) facet rows has a mask but no facets
  base = unit_cube_mesh(2, ndim=2)
  pm = base.replace(physical_groups={'corners': np.array([0, 2, 6, 8]),
                                     'boundary': base.physical_groups[
                                         'boundary']})
  mesh = pm.finalize(device='cpu')
  assert 'corners' in mesh.physical_masks
  assert 'corners' not in mesh.boundary_facets
  fes = FiniteElementSpace.create(
      mesh, Quadrature1D.create(2, NodeType.GAUSS_LEGENDRE))
  with pytest.raises(ValueError, match='no facets'):
    fes.boundary_covector('corners', 1.0)
  with pytest.raises(KeyError):
    fes.boundary_covector('nowhere', 1.0)


def test_refusals():
  grid = Nodes1D.create(3, GLL)
  rp = refine_premesh(unit_cube_mesh(2, ndim=2), grid)
  mesh = rp.finalize(device='cpu')
  quad = Quadrature1D.create_from_nodes_1d(grid)
  ens = mesh.replicate(2)
  with pytest.raises(NotImplementedError):
    FiniteElementSpace.create(ens, quad).boundary_points('boundary')
  with pytest.raises(NotImplementedError):
    solve_helmholtz(ens, torch.zeros(ens.num_nodes, dtype=torch.float64),
                    {'boundary': (BCType.DIRICHLET, 0.0)})
  pp = unit_cube_mesh(4, ndim=2, partitions=np.arange(2).reshape(2, 1))
  part = pp.finalize('x', rank=0, device='cpu')
  with pytest.raises(NotImplementedError):
    FiniteElementSpace.create(
        part, Quadrature1D.create(2, NodeType.GAUSS_LEGENDRE)
    ).boundary_covector('boundary', 1.0)
  with pytest.raises(NotImplementedError):
    solve_helmholtz(part, torch.zeros(part.num_nodes, dtype=torch.float64),
                    {'boundary': (BCType.DIRICHLET, 0.0)})
  f = torch.zeros(mesh.num_nodes, dtype=torch.float64)
  with pytest.raises(ValueError, match='singular'):
    solve_helmholtz(mesh, f, {'boundary': (BCType.NEUMANN, 1.0)})
  with pytest.raises(ValueError, match='singular'):
    solve_helmholtz(mesh, f, {})
  with pytest.raises(ValueError, match='unsupported'):
    solve_helmholtz(mesh, f, {'boundary': ('robin', 1.0)})
  with pytest.raises(KeyError):
    solve_helmholtz(mesh, f, {'nowhere': (BCType.DIRICHLET, 1.0)})
  with pytest.raises(ValueError, match='preconditioner'):
    solve_helmholtz(mesh, f, {'boundary': (BCType.DIRICHLET, 1.0)},
                    preconditioner='ilu')
