"""p-multigrid hierarchy on block partitions (`linalg/pmg.py`), host side: the
coarse `NeighborPlan` derived from the fine one, the rank owners of the
restriction, and the restriction summed over the ranks against the whole-box
P^T of `tests/pmg_reference.py`.  Runs without a GPU."""
import numpy as np
import pytest
import torch

from swirl_fem_amd.distributed import blocks
from swirl_fem_amd.distributed import comm
from swirl_fem_amd.linalg import pmg
from tests import pmg_reference as R

GRIDS = [(2, 1, 1), (2, 2, 1), (2, 2, 2), (2, 1), (2, 2)]


def _key(x):
  """Hashable coordinates (uniform blocks: exact up to rounding)."""
  return tuple(np.round(np.asarray(x, dtype=np.float64), 9))


def _hierarchy(n, P, grid, jitter=0.0):
  """Per rank: [(mesh, plan)] for every order of the default schedule."""
  out = []
  for rank in range(int(np.prod(grid))):
    bp = blocks.build_block_partition(n, P, grid, rank, device='cpu',
                                      jitter=jitter)
    levels = [bp.mesh]
    for pc in pmg.default_orders(P - 1)[1:]:
      levels.append(pmg.coarse_mesh(levels[-1], pc)[0])
    out.append(levels)
  return out


def _coords(mesh):
  return mesh.node_coords.double().numpy()


@pytest.mark.parametrize('grid', GRIDS)
@pytest.mark.parametrize('P', [5, 6])
@pytest.mark.parametrize('jitter', [0.0, 0.3])
def test_coarse_plans_agree_on_both_sides(grid, P, jitter):
  hier = _hierarchy(2, P, grid, jitter)
  for lvl in range(len(hier[0])):
    for r, levels in enumerate(hier):
      mesh = levels[lvl]
      plan = mesh.neighbor_plan
      assert mesh.axis_name is not None and plan is not None
      for q, ix in zip(plan.neighbors, plan.indices):
        other = hier[q][lvl].neighbor_plan
        jx = other.indices[other.neighbors.index(r)]
        assert len(ix) == len(jx) > 0
        np.testing.assert_allclose(_coords(mesh)[ix],
                                   _coords(hier[q][lvl])[jx], rtol=0,
                                   atol=1e-13)
      # the mesh's exchange indices are the plan's
      gi = mesh.exchange_gather_indices.numpy()
      np.testing.assert_array_equal(
          gi, np.concatenate(plan.indices) if plan.indices else gi[:0])


@pytest.mark.parametrize('grid', GRIDS)
@pytest.mark.parametrize('P', [5, 8])
def test_coarse_plan_pairs_the_nodes_of_the_direct_plan(grid, P):
  """On uniform blocks the derived plan shares the same physical nodes with
  each neighbour as the plan built directly at that order."""
  hier = _hierarchy(2, P, grid)
  orders = pmg.default_orders(P - 1)
  for lvl, pc in enumerate(orders[1:], start=1):
    for r, levels in enumerate(hier):
      mesh = levels[lvl]
      direct = blocks.build_block_partition(2, pc + 1, grid, r, device='cpu')
      dplan, dx = direct.plan, _coords(direct.mesh)
      plan, x = mesh.neighbor_plan, _coords(mesh)
      assert plan.neighbors == dplan.neighbors
      for ix, jx in zip(plan.indices, dplan.indices):
        assert len(ix) == len(jx)
        assert sorted(map(_key, x[ix])) == sorted(map(_key, dx[jx]))


@pytest.mark.parametrize('grid', GRIDS)
def test_every_global_node_has_one_restriction_owner(grid):
  hier = _hierarchy(2, 5, grid, jitter=0.2)
  for lvl in range(len(hier[0])):
    count = {}
    for levels in hier:
      mesh = levels[lvl]
      owned = pmg.rank_owned(mesh.neighbor_plan, mesh.num_nodes)
      for k, o in zip(map(_key, _coords(mesh)), owned):
        count[k] = count.get(k, 0) + int(o)
    assert set(count.values()) == {1}


def _rank_levels(mesh):
  """NumPy levels (tests/pmg_reference.py) of one rank's block."""
  x = _coords(mesh)
  el = mesh.elements.numpy().astype(np.int64)
  bnd = mesh.physical_masks.get('boundary')
  bnd = np.zeros(len(x), bool) if bnd is None else bnd.numpy()
  n = el.shape[1]
  fine = R.Level(x, el, mesh.order, bnd, np.zeros((el.shape[0], n, n)))
  return fine


@pytest.mark.parametrize('grid', GRIDS)
@pytest.mark.parametrize('P', [5, 6])
def test_restriction_through_rank_owners_is_global_transpose(grid, P):
  """sum over ranks of P_rank^T (owned r) = P^T r of the whole box, on every
  level, with the owner bits the GPU restriction uses."""
  n = 2
  ndim = len(grid)
  orders = pmg.default_orders(P - 1)
  whole = blocks.build_block_partition(
      [n * g for g in grid], P, (1,) * ndim, 0, device='cpu')
  wl = _rank_levels(whole.mesh)
  hier = _hierarchy(n, P, grid)
  rank_lv = [_rank_levels(levels[0]) for levels in hier]
  rng = np.random.default_rng(7)
  for lvl, pc in enumerate(orders[1:]):
    wc, Pw = R.coarsen(wl, pc, 0.0, 1.0)
    r = rng.standard_normal(wl.N) * wl.keep
    want = Pw.T @ r
    widx = {k: i for i, k in enumerate(map(_key, wc.coords))}
    fidx = {k: i for i, k in enumerate(map(_key, wl.coords))}
    got = np.zeros(wc.N)
    nxt = []
    for levels, fl in zip(hier, rank_lv):
      fmesh = levels[lvl]
      cl, Pr = R.coarsen(fl, pc, 0.0, 1.0)
      # the coarse mesh of the product has the same numbering and coordinates
      np.testing.assert_allclose(cl.coords, _coords(levels[lvl + 1]),
                                 rtol=0, atol=1e-12)
      own = pmg.rank_owned(fmesh.neighbor_plan, fmesh.num_nodes)
      # decoded restriction owner bits: rank and element owner in one
      bits = pmg.owner_bits(fmesh.elements, fmesh.num_nodes,
                            torch.as_tensor(own)).numpy().view(np.uint32)
      E, nloc = fmesh.elements.shape
      t = np.arange(nloc)
      flags = (bits[:, t // 32] >> (t % 32).astype(np.uint32)) & 1
      owned_nodes = np.zeros(fmesh.num_nodes, dtype=np.int64)
      np.add.at(owned_nodes, fmesh.elements.numpy().reshape(-1),
                flags.reshape(-1).astype(np.int64))
      np.testing.assert_array_equal(owned_nodes, own.astype(np.int64))
      rl = r[[fidx[k] for k in map(_key, fl.coords)]]
      share = Pr.T @ (rl * own)
      np.add.at(got, [widx[k] for k in map(_key, cl.coords)], share)
      nxt.append(cl)
    np.testing.assert_allclose(got, want, rtol=0,
                               atol=1e-12 * np.abs(want).max())
    wl, rank_lv = wc, nxt


def test_refusals():
  bp = blocks.build_block_partition(2, 4, (2, 1, 1), 0, device='cpu')
  mesh = bp.mesh
  pmg._check_mesh(mesh)                        # a block partition: accepted
  with pytest.raises(NotImplementedError, match='partitioned'):
    pmg._check_mesh(mesh.replace(neighbor_plan=None))
  with pytest.raises(NotImplementedError, match='partitioned'):
    pmg.coarse_mesh(mesh.replace(neighbor_plan=None), 1)
  plan = mesh.neighbor_plan
  images = comm.NeighborPlan(
      rank=plan.rank, neighbors=plan.neighbors, indices=plan.indices,
      local_gather=np.array([1], np.int32), local_unique=np.array([0]),
      local_rep=np.array([0], np.int32))
  with pytest.raises(NotImplementedError, match='local periodic images'):
    pmg._check_mesh(mesh.replace(neighbor_plan=images))
  padded = mesh.elements.clone()
  padded[-1] = -1
  with pytest.raises(NotImplementedError, match='padded'):
    pmg._check_mesh(mesh.replace(elements=padded))
  whole = blocks.build_block_partition(2, 4, (1, 1, 1), 0, device='cpu').mesh
  with pytest.raises(NotImplementedError, match='ensemble'):
    pmg._check_mesh(whole.replicate(2))
