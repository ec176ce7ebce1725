"""Host side of Robin conditions: `BCType.ROBIN`, the refusals of
`solve_helmholtz` / `FiniteElementSpace.boundary_mass` before any kernel
launch, the coarse facets of p-multigrid (`pmg.coarse_facets`) and the
compact row-sum plan (`fespace.boundary_rows`).  Runs without a GPU."""
import itertools

import numpy as np
import pytest
import torch

from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
from swirl_fem_amd.core.fespace import FiniteElementSpace, boundary_rows
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType, Quadrature1D
from swirl_fem_amd.core.mesh_refiner import refine_premesh
from swirl_fem_amd.examples import helmholtz
from swirl_fem_amd.examples import poisson
from swirl_fem_amd.examples.helmholtz import BCType, solve_helmholtz
from swirl_fem_amd.linalg import pmg

GLL = NodeType.GAUSS_LOBATTO_LEGENDRE


def test_robin_type():
  assert BCType.ROBIN.value == 'robin'
  assert helmholtz.BCType is poisson.BCType
  assert BCType('robin') is BCType.ROBIN
  assert BCType.ROBIN != 'robin'


def _square():
  grid = Nodes1D.create(3, GLL)
  rp = refine_premesh(unit_cube_mesh(2, ndim=2), grid)
  return rp.finalize(device='cpu'), Quadrature1D.create_from_nodes_1d(grid)


def test_refusals():
  mesh, quad = _square()
  f = torch.zeros(mesh.num_nodes, dtype=torch.float64)
  R = BCType.ROBIN
  with pytest.raises(ValueError, match='>= 0'):
    solve_helmholtz(mesh, f, {'boundary': (R, (-1.0, 0.0))}, lambda0=1.0)
  with pytest.raises(ValueError, match='>= 0'):
    FiniteElementSpace.create(mesh, quad).boundary_mass('boundary', -0.5)
  with pytest.raises(ValueError, match='negative'):
    FiniteElementSpace.create(mesh, quad).boundary_mass(
        'boundary', -torch.ones(mesh.num_nodes, dtype=torch.float64))
  for bad in (1.0, (1.0,), (1.0, 2.0, 3.0), 'ab', None):
    with pytest.raises(ValueError, match='pair'):
      solve_helmholtz(mesh, f, {'boundary': (R, bad)}, lambda0=1.0)
  with pytest.raises(ValueError, match='unsupported'):
    solve_helmholtz(mesh, f, {'boundary': ('robin', (1.0, 0.0))})
  with pytest.raises(ValueError, match='unsupported'):
    solve_helmholtz(mesh, f, {'boundary': ('robin', 1.0)})
  # lambda0 = 0, no Dirichlet node and every alpha 0: singular
  with pytest.raises(ValueError, match='singular'):
    solve_helmholtz(mesh, f, {'boundary': (R, (0.0, 1.0))})
  with pytest.raises(ValueError, match='singular'):
    solve_helmholtz(mesh, f, {'boundary': (R, (0, 0))})
  # ensembles and partitions
  ens = mesh.replicate(2)
  with pytest.raises(NotImplementedError):
    FiniteElementSpace.create(ens, quad).boundary_mass('boundary', 1.0)
  with pytest.raises(NotImplementedError):
    solve_helmholtz(ens, torch.zeros(ens.num_nodes, dtype=torch.float64),
                    {'boundary': (R, (1.0, 0.0))})
  pp = unit_cube_mesh(4, ndim=2, partitions=np.arange(2).reshape(2, 1))
  part = pp.finalize('x', rank=0, device='cpu')
  with pytest.raises(NotImplementedError):
    FiniteElementSpace.create(
        part, Quadrature1D.create(2, NodeType.GAUSS_LEGENDRE)
    ).boundary_mass('boundary', 1.0)
  with pytest.raises(NotImplementedError):
    solve_helmholtz(part, torch.zeros(part.num_nodes, dtype=torch.float64),
                    {'boundary': (R, (1.0, 0.0))})


def test_solve_poisson_unchanged():
  mesh, _ = _square()
  f = torch.zeros(mesh.num_nodes, dtype=torch.float64)
  with pytest.raises(NotImplementedError):
    poisson.solve_poisson(mesh, f, {'boundary': (BCType.ROBIN, (1.0, 0.0))})


def _rotated(ndim, n, P, seed):
  """A jittered refined box whose elements have random vertex orderings."""
  rng = np.random.default_rng(seed)
  base = unit_cube_mesh(n, ndim=ndim)
  x = base.node_coords + 0.1 / n * rng.uniform(-1, 1, base.node_coords.shape)
  orients = [(perm, axes) for perm in itertools.permutations(range(ndim))
             for r in range(ndim + 1)
             for axes in itertools.combinations(range(ndim), r)]
  el = []
  for e in base.elements[rng.permutation(base.num_elements)]:
    perm, axes = orients[rng.integers(len(orients))]
    el.append(np.flip(e.reshape([2] * ndim).transpose(perm),
                      axes).reshape(-1))
  pm = base.replace(node_coords=x, elements=np.array(el, dtype=np.int32))
  return refine_premesh(pm, Nodes1D.create(P + 1, GLL))


def _plain(ndim, n, P, seed):
  return refine_premesh(unit_cube_mesh(n, ndim=ndim), Nodes1D.create(P + 1,
                                                                     GLL))


@pytest.mark.parametrize('ndim,n,P,build', [
    (2, 3, 4, _plain), (3, 2, 6, _plain), (2, 3, 7, _rotated),
    (3, 2, 4, _rotated), (3, 2, 5, _rotated)])
def test_coarse_facets(ndim, n, P, build):
  rp = build(ndim, n, P, seed=P)
  mesh = rp.finalize(device='cpu')
  el = mesh.elements.numpy().astype(np.int64)
  x = np.asarray(rp.node_coords)
  fine = mesh.boundary_facets['boundary'].numpy().astype(np.int64)
  k = ndim - 1
  pf = P
  while pf > 1:
    pc = pf // 2
    celems, _, nc = pmg.coarse_numbering(el, None, ndim, pf, pc)
    corners = el[:, pmg._flat(pmg._lex((2,) * ndim) * pf, pf + 1)]
    got = pmg.coarse_facets(fine, corners, celems, ndim, pf, pc)
    assert got.shape == (fine.shape[0], (pc + 1) ** k)
    # every element face: its fine nodes -> its coarse nodes
    faces = {}
    fel = el.reshape((-1,) + (pf + 1,) * ndim)
    cel = celems.reshape((-1,) + (pc + 1,) * ndim)
    for a in range(ndim):
      for s in (0, 1):
        fs = np.take(fel, s * pf, axis=1 + a).reshape(len(el), -1)
        cs = np.take(cel, s * pc, axis=1 + a).reshape(len(el), -1)
        for fr, cr in zip(fs, cs):
          faces.setdefault(tuple(np.sort(fr)), []).append(tuple(np.sort(cr)))
    for fr, cr in zip(fine, got):
      hit = faces[tuple(np.sort(fr))]
      assert len(hit) == 1                      # one element face
      assert tuple(np.sort(cr)) == hit[0]       # exactly its coarse nodes
      assert len(set(cr.tolist())) == cr.size
    # corner coordinates: the coarse geometry is the fine element map at the
    # coarse GLL points
    J = pmg._kron(pmg.interpolation_1d_geometry(pf, pc), ndim)
    xc = np.zeros((nc, ndim))
    xc[celems.reshape(-1)] = np.einsum('cf,efd->ecd', J, x[el]).reshape(
        -1, ndim)
    fpos = pmg._flat(pmg._lex((2,) * k) * pf, pf + 1)
    cpos = pmg._flat(pmg._lex((2,) * k) * pc, pc + 1)
    for fr, cr in zip(fine, got):
      a = np.sort(x[fr[fpos]].round(12).view(
          [('', float)] * ndim).reshape(-1))
      b = np.sort(xc[cr[cpos]].round(12).view(
          [('', float)] * ndim).reshape(-1))
      np.testing.assert_allclose(np.array(a.tolist()), np.array(b.tolist()),
                                 atol=1e-11)
    # the next level starts from these
    fine, el, x, pf = got, celems, xc, pc


def test_coarse_facets_refuses_strangers():
  rp = _plain(2, 2, 2, 0)
  mesh = rp.finalize(device='cpu')
  el = mesh.elements.numpy().astype(np.int64)
  celems, _, _ = pmg.coarse_numbering(el, None, 2, 2, 1)
  corners = el[:, pmg._flat(pmg._lex((2, 2)) * 2, 3)]
  bad = np.array([[el[0, 0], el[0, 4], el[0, 8]]])       # a diagonal
  with pytest.raises(ValueError, match='not a face'):
    pmg.coarse_facets(bad, corners, celems, 2, 2, 1)


@pytest.mark.parametrize('masked', [False, True])
def test_row_plan_is_a_dense_sum(masked):
  rng = np.random.default_rng(3)
  for ndim, P in ((2, 5), (3, 3)):
    mesh = _rotated(ndim, 2, P, 1).finalize(device='cpu')
    N = mesh.num_nodes
    facets = mesh.boundary_facets['boundary'].numpy()
    dirichlet = rng.random(N) < 0.3 if masked else None
    rows, offsets, slots = boundary_rows(facets, N, dirichlet)
    assert rows.dtype == np.int32 and slots.dtype == np.int32
    assert offsets.dtype == np.int64 and offsets.size == rows.size + 1
    on = np.zeros(N, bool)
    on[facets.reshape(-1)] = True
    if masked:
      on &= ~dirichlet
    assert rows.tolist() == np.nonzero(on)[0].tolist()
    local = rng.standard_normal(facets.size)
    out = rng.standard_normal(N)
    want = out.copy()
    flat = facets.reshape(-1)
    keep = on[flat]
    np.add.at(want, flat[keep], local[keep])
    got = out.copy()
    for r in range(rows.size):
      seg = slots[offsets[r]:offsets[r + 1]]
      assert (np.diff(seg) > 0).all() and (flat[seg] == rows[r]).all()
      got[rows[r]] += local[seg].sum()
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-13)
    untouched = ~on
    assert np.array_equal(got[untouched], out[untouched])
