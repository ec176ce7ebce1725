"""p-multigrid host logic (`linalg/pmg.py`) and its NumPy restatement
(`tests/pmg_reference.py`): coarse numbering, the facet rule for coarse
Dirichlet nodes, the owner map, refusals, and the V-cycle as an operator.
Runs without a GPU."""
import numpy as np
import pytest
import torch

from swirl_fem_amd.linalg import pmg
from tests import pmg_reference as R


def _fine(rp):
  arrays = rp.finalize_all()
  return (np.asarray(rp.node_coords), np.asarray(arrays['elements'], np.int64),
          np.asarray(arrays['node_indices'], np.int64))


def test_default_orders():
  assert pmg.default_orders(7) == [7, 3, 1]
  assert pmg.default_orders(11) == [11, 5, 2, 1]
  assert pmg.default_orders(2) == [2, 1]
  assert pmg.default_orders(1) == [1]


@pytest.mark.parametrize('ndim,n,P,mode,periodic', [
    (3, 3, 8, 'uniform', ()), (3, 2, 6, 'jitter', ()),
    (3, 2, 5, 'sheared', (0, 2)), (3, 3, 4, 'uniform', (0, 1, 2)),
    (3, 1, 8, 'uniform', (0,)), (2, 3, 12, 'jitter', ()),
    (2, 3, 7, 'uniform', (1,)), (2, 2, 11, 'sheared', (0, 1))])
def test_coarse_numbering_is_continuous(ndim, n, P, mode, periodic):
  """Interpolating any coarse field element by element gives one value per
  fine node (and per fine periodic class for class-constant fields)."""
  rp = R.box(n, ndim, P, mode, seed=P, periodic=periodic)
  _, el, reps = _fine(rp)
  pf = P - 1
  rng = np.random.default_rng(0)
  for pc in pmg.default_orders(pf)[1:]:
    celems, creps, nc = pmg.coarse_numbering(el, reps, ndim, pf, pc)
    assert celems.shape == (el.shape[0], (pc + 1) ** ndim)
    assert set(np.unique(celems)) == set(range(nc))
    for e in range(el.shape[0]):
      assert len(set(celems[e])) == celems.shape[1]
    J = R.interp_1d(pc, pf)
    Jd = J
    for _ in range(ndim - 1):
      Jd = np.kron(Jd, J)
    for field, ids in ((rng.standard_normal(nc), el),
                       (None, reps[el])):
      if field is None:
        field = rng.standard_normal(nc)[creps.ravel()]
        full = np.empty(nc)
        full[celems.ravel()] = field
        field = full
      vals = np.einsum('fc,ec->ef', Jd, field[celems])
      lo = np.full(el.max() + 1, np.inf)
      hi = np.full(el.max() + 1, -np.inf)
      np.minimum.at(lo, ids.ravel(), vals.ravel())
      np.maximum.at(hi, ids.ravel(), vals.ravel())
      used = np.isfinite(lo)
      assert np.abs(hi[used] - lo[used]).max() < 1e-12 * np.abs(vals).max()
    el = celems
    reps_new = np.empty(nc, dtype=np.int64)
    reps_new[celems.ravel()] = creps.ravel()
    reps, pf = reps_new, pc


def test_coarse_shared_nodes_match_fine_sharing():
  """Two elements share a coarse node iff they share the fine point there."""
  rp = R.box(2, 3, 6, 'jitter', seed=1)
  x, el, _ = _fine(rp)
  celems, _, nc = pmg.coarse_numbering(el, None, 3, 5, 2)
  Jg = np.asarray(pmg.interpolation_1d_geometry(5, 2))
  Jgd = np.kron(np.kron(Jg, Jg), Jg)
  xc = np.einsum('cf,efd->ecd', Jgd, x[el])
  pos = {}
  for e in range(el.shape[0]):
    for t, c in enumerate(celems[e]):
      pos.setdefault(c, []).append(xc[e, t])
  for c, pts in pos.items():
    assert np.ptp(np.array(pts), axis=0).max() < 1e-12
  # distinct coarse nodes sit at distinct points
  first = np.array([pos[c][0] for c in range(nc)])
  key = np.round(first, 9)
  assert len(np.unique(key, axis=0)) == nc


@pytest.mark.parametrize('ndim,P', [(2, 8), (3, 6), (3, 12)])
def test_facet_rule(ndim, P):
  rp = R.box(2, ndim, P, 'uniform')
  x, el, _ = _fine(rp)
  pf = P - 1
  for pc in pmg.default_orders(pf)[1:]:
    # Dirichlet on the face x0 = 0 and on part of the face x1 = 0
    fdir = (np.abs(x[:, 0]) < 1e-12) | ((np.abs(x[:, 1]) < 1e-12) &
                                        (x[:, 0] < 0.3))
    loc = torch.as_tensor(fdir[el])
    got = pmg.coarse_dirichlet(loc, ndim, pf, pc).numpy()
    ref = R.facet_rule(fdir[el], ndim, pf, pc)
    np.testing.assert_array_equal(got, ref)
    celems, _, nc = pmg.coarse_numbering(el, None, ndim, pf, pc)
    xc = np.zeros((nc, ndim))
    Jg = np.asarray(pmg.interpolation_1d_geometry(pf, pc))
    Jgd = Jg if ndim == 2 else np.kron(Jg, Jg)
    Jgd = np.kron(Jgd, Jg)
    xc[celems] = np.einsum('cf,efd->ecd', Jgd, x[el])
    cd = np.zeros(nc, bool)
    cd[celems.ravel()] = got.ravel()
    # the whole face x0 = 0 is Dirichlet; of x1 = 0 only closed facets whose
    # every fine node has x0 < 0.3: at 2 elements per direction, none but
    # the edges on x0 = 0
    on0 = np.abs(xc[:, 0]) < 1e-12
    assert cd[on0].all() and not cd[~on0].any()
    x, el, pf = xc, celems, pc


def test_owner_bits():
  el = torch.tensor([[0, 1, 2, 3], [2, 3, 4, 5], [4, 5, 0, 1]])
  w = pmg.owner_bits(el, 6)
  assert w.shape == (3, 1)
  assert [int(v) for v in w[:, 0]] == [0b1111, 0b1100, 0b0000]
  big = torch.arange(2 * 40).reshape(2, 40)
  big[1, :5] = big[0, :5]
  w = pmg.owner_bits(big, 80).to(torch.int64) & 0xFFFFFFFF
  assert int(w[0, 0]) == 0xFFFFFFFF and int(w[0, 1]) == 0xFF
  assert int(w[1, 0]) == 0xFFFFFFE0 and int(w[1, 1]) == 0xFF


def test_refuses_partitioned_and_replicated_meshes():
  rp = R.box(2, 2, 4, 'uniform')
  mesh = rp.finalize(device='cpu')
  with pytest.raises(NotImplementedError, match='partitioned'):
    pmg._check_mesh(mesh.replace(axis_name='x'))
  with pytest.raises(NotImplementedError, match='ensemble'):
    pmg._check_mesh(mesh.replicate(2))
  pmg._check_mesh(mesh.replicate(1))


def _hierarchy(n, ndim, P, mode='jitter', l0=0.0, degree=2, periodic=()):
  rp = R.box(n, ndim, P, mode, seed=3, periodic=periodic)
  x, el, _ = _fine(rp)
  arrays = rp.finalize_all()
  bnd = np.asarray(arrays['physical_masks'].get(
      'boundary', np.zeros(len(x), bool)))
  return R.Hierarchy(x, el, P - 1, bnd, l0, 1.0, degree=degree)


@pytest.mark.parametrize('ndim,n,P,l0,periodic', [
    (2, 3, 5, 0.0, ()), (3, 2, 4, 0.5, ()), (2, 2, 7, 0.0, (0,))])
def test_vcycle_is_symmetric_positive_definite(ndim, n, P, l0, periodic):
  H = _hierarchy(n, ndim, P, l0=l0, periodic=periodic)
  lev = H.levels[0]
  inner = np.nonzero(lev.keep > 0)[0]
  M = np.zeros((lev.N, lev.N))
  for i in inner:
    e = np.zeros(lev.N)
    e[i] = 1.0
    M[:, i] = H.vcycle(e)
  Mi = M[np.ix_(inner, inner)]
  assert np.abs(Mi - Mi.T).max() < 1e-10 * np.abs(Mi).max()
  assert np.linalg.eigvalsh(0.5 * (Mi + Mi.T)).min() > 0
  # nothing on the Dirichlet rows
  assert np.abs(np.delete(M, inner, axis=0)).max() == 0.0


def test_pcg_iterations_and_mesh_independence():
  rng = np.random.default_rng(0)
  # 6^3 p = 5 Dirichlet box: at most 1/5 of plain CG's iterations
  H = _hierarchy(6, 3, 6, mode='uniform')
  b = H.levels[0].keep * rng.standard_normal(H.levels[0].N)
  _, it_pmg = H.pcg(b, 1e-8)
  _, it_cg = H.pcg(b, 1e-8, precondition=False)
  assert it_pmg * 5 <= it_cg, (it_pmg, it_cg)
  # 4^3 against 8^3 at p = 3: a few iterations apart
  its = []
  for n in (4, 8):
    H = _hierarchy(n, 3, 4, mode='uniform')
    b = H.levels[0].keep * rng.standard_normal(H.levels[0].N)
    its.append(H.pcg(b, 1e-8)[1])
  assert abs(its[0] - its[1]) <= 4, its
