"""p-multigrid and Jacobi preconditioning of the partitioned Helmholtz solve
(`linalg/pmg.py`, `linalg/cg.py`, `distributed/solver.py`) on the 2 x 2 x 2
block layout of `bench.py --gpus 8`, with ranks as threads on one GPU
(`distributed.inprocess.ThreadWorld`), against the one-rank solve of the
whole box; and `sfem_ell_spmv`, the coarse product of the partitioned
V-cycle, against SciPy.  Needs a real MI355X."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from swirl_fem_amd import _ops
from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType, Quadrature1D
from swirl_fem_amd.distributed import blocks, inprocess, solver
from swirl_fem_amd.linalg import cg as cg_lib
from swirl_fem_amd.linalg.jacobi import JacobiPreconditioner
from swirl_fem_amd.linalg.pmg import PMultigridPreconditioner

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
GRID = (2, 2, 2)
L0, L1 = 0.3, 1.0


# ------------------------------------------------------------ sfem_ell_spmv
def _ell(n, width, dtype, seed):
  rng = np.random.default_rng(seed)
  cols = rng.integers(0, n, size=(width, n)).astype(np.int32)
  vals = rng.standard_normal((width, n))
  vals[:, rng.random(n) < 0.2] = 0.0           # padded entries: value 0
  A = sp.csr_matrix((vals.T.reshape(-1), (np.repeat(np.arange(n), width),
                                          cols.T.reshape(-1))), shape=(n, n))
  return (torch.as_tensor(cols, device=DEV),
          torch.as_tensor(vals, dtype=dtype, device=DEV), A)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
@pytest.mark.parametrize('n', [1000, 1001, 4096 + 6])
def test_ell_spmv_matches_scipy(dtype, n):
  cols, vals, A = _ell(n, 27, dtype, n)
  x = torch.randn(n, dtype=dtype, device=DEV)
  want = A @ x.double().cpu().numpy()
  tol = 1e-12 if dtype == torch.float64 else 2e-5
  scale = np.abs(want).max()
  rng = np.random.default_rng(1)
  cases = [dict(), dict(row_range=(0, n)), dict(row_range=(3, n - 5)),
           dict(row_range=(4, 4 + (n - 8) // 8 * 8)), dict(row_range=(7, 8)),
           dict(row_range=(5, 5))]
  for rows in (np.sort(rng.choice(n, n // 3, replace=False)),
               rng.permutation(n)[:17], np.arange(n)[::-1]):
    cases.append(dict(rows=torch.as_tensor(rows.astype(np.int32),
                                           device=DEV)))
  for kw in cases:
    y = torch.full((n,), 1234.5, dtype=dtype, device=DEV)
    _ops.ell_spmv(cols, vals, x, y, **kw)
    got = y.double().cpu().numpy()
    if 'rows' in kw:
      sel = np.zeros(n, bool)
      sel[kw['rows'].cpu().numpy()] = True
    else:
      b, e = kw.get('row_range', (0, n))
      sel = np.zeros(n, bool)
      sel[b:e] = True
    assert np.abs(got[sel] - want[sel]).max(initial=0.0) <= tol * scale, kw
    assert (got[~sel] == 1234.5).all(), kw           # other rows untouched


def test_ell_spmv_refuses_bad_arguments():
  cols, vals, _ = _ell(64, 4, torch.float64, 0)
  x = torch.zeros(64, dtype=torch.float64, device=DEV)
  with pytest.raises(ValueError):
    _ops.ell_spmv(cols, vals, x, x.clone(), row_range=(0, 65))
  with pytest.raises(TypeError):
    _ops.ell_spmv(cols, vals, x.float(), x.float())


# ------------------------------------------------------ partitioned solves
def _quad(P):
  return Quadrature1D.create_from_nodes_1d(
      Nodes1D.create(P, NodeType.GAUSS_LOBATTO_LEGENDRE))


def _whole(n, P, dtype, jitter):
  """The one-rank problem of the whole box: (partition, op, rhs f, lookup)."""
  whole = blocks.build_block_partition([n * g for g in GRID], P, (1, 1, 1), 0,
                                       device=DEV, jitter=jitter, dtype=dtype)
  gm = whole.mesh
  bm = gm.physical_masks['boundary']
  fes = FiniteElementSpace.create(gm, _quad(P))
  op = fes.helmholtz_operator(bm)
  gx = gm.node_coords.double()
  f = (torch.sin(3 * gx[:, 0]) * torch.cos(2 * gx[:, 1]) +
       gx[:, 2] ** 2).to(dtype)
  b = fes.helmholtz_operator(None).apply(f * ~bm, 1.0, 0.0) * ~bm
  lookup = dict(zip(whole.global_keys.tolist(), range(gm.num_nodes)))
  return whole, op, f, b, lookup


def _rank_problem(rank, n, P, dtype, jitter, f, lookup):
  part = blocks.build_block_partition(n, P, GRID, rank, device=DEV,
                                      jitter=jitter, dtype=dtype)
  mesh = part.mesh
  bm = mesh.physical_masks.get('boundary')
  if bm is None:
    bm = torch.zeros(mesh.num_nodes, dtype=torch.bool, device=DEV)
  fes = FiniteElementSpace.create(mesh, _quad(P))
  op = fes.helmholtz_operator(bm)
  ids = torch.as_tensor([lookup[k] for k in part.global_keys.tolist()],
                        device=DEV)
  b_loc = fes.helmholtz_operator(None).apply(f[ids] * ~bm, 1.0, 0.0) * ~bm
  return part, op, ids, b_loc


@pytest.mark.parametrize('jitter', [0.0, 0.1])
def test_vcycle_on_partitions_equals_whole_box(jitter):
  """The same V-cycle: the whole box's spectrum estimates injected, the
  same coarse steps; applied to one global vector, to 1e-10 in fp64.  The
  one-rank V-cycle smooths with a coloured-assembly copy of the operator, the
  partitioned one applies the operator itself; the jittered box mixes affine
  and multilinear elements."""
  n, P = 2, 5
  whole, gop, _, _, lookup = _whole(n, P, torch.float64, jitter)
  Mg = PMultigridPreconditioner(gop, L0, L1, coarse_steps=12)
  bounds = Mg.spectral_bounds()
  N = whole.mesh.num_nodes
  g = torch.Generator(device=DEV).manual_seed(3)
  v = torch.randn(N, dtype=torch.float64, device=DEV, generator=g)
  want = Mg(v).double().cpu().numpy()

  def rank_main(rank):
    part = blocks.build_block_partition(n, P, GRID, rank, device=DEV,
                                        jitter=jitter)
    mesh = part.mesh
    bm = mesh.physical_masks.get('boundary')
    op = FiniteElementSpace.create(mesh, _quad(P)).helmholtz_operator(bm)
    M = PMultigridPreconditioner(op, L0, L1, coarse_steps=12, bounds=bounds)
    assert M.consistent and not M.capturable
    assert [l.mesh.neighbor_plan is not None for l in M.levels] == [True] * 3
    ids = torch.as_tensor([lookup[k] for k in part.global_keys.tolist()],
                          device=DEV)
    z = M(v[ids].contiguous())
    return ids.cpu().numpy(), z.double().cpu().numpy()

  out = inprocess.ThreadWorld(8).run(rank_main)
  for ids, z in out.values():
    err = np.abs(z - want[ids]).max() / np.abs(want).max()
    assert err <= 1e-10, err


def test_vcycle_on_partitions_is_symmetric():
  n, P, jitter = 2, 5, 0.1
  whole, _, _, _, lookup = _whole(n, P, torch.float64, jitter)
  N = whole.mesh.num_nodes
  g = torch.Generator(device=DEV).manual_seed(5)
  a = torch.randn(N, dtype=torch.float64, device=DEV, generator=g)
  b = torch.randn(N, dtype=torch.float64, device=DEV, generator=g)

  def rank_main(rank):
    part = blocks.build_block_partition(n, P, GRID, rank, device=DEV,
                                        jitter=jitter)
    mesh = part.mesh
    op = FiniteElementSpace.create(mesh, _quad(P)).helmholtz_operator(
        mesh.physical_masks.get('boundary'))
    M = PMultigridPreconditioner(op, L0, L1)
    ids = torch.as_tensor([lookup[k] for k in part.global_keys.tolist()],
                          device=DEV)
    ma = M(a[ids].contiguous()).clone()
    mb = M(b[ids].contiguous()).clone()
    # global inner products of consistent vectors
    idx, w = part.plan.interface_weights(DEV)
    dots = []
    for x, y in ((ma, b[ids]), (a[ids], mb), (a[ids], ma)):
      dots.append(float(torch.dot(x, y) - (w * x[idx] * y[idx]).sum()))
    return np.array(dots)

  tot = sum(inprocess.ThreadWorld(8).run(rank_main).values())
  assert abs(tot[0] - tot[1]) <= 1e-12 * max(abs(tot[0]), 1.0), tot
  assert tot[2] > 0


def _solve_case(n, P, dtype, tol, jitter, kinds):
  """One-rank solves of the whole box and partitioned solves on 8 thread
  ranks, for each preconditioner kind in `kinds` (None / 'jacobi' / 'pmg')."""
  whole, gop, f, b, lookup = _whole(n, P, dtype, jitter)
  N = whole.mesh.num_nodes
  single = {}
  bn = float(torch.linalg.vector_norm(b.double()))
  for kind in kinds:
    M = (None if kind is None else JacobiPreconditioner(gop, L0, L1)
         if kind == 'jacobi' else PMultigridPreconditioner(gop, L0, L1))
    x, info = cg_lib.cg(gop.linear_operator(L0, L1), b, tol=tol,
                        maxiter=5000, M=M)
    r = b.double() - gop.apply(x, L0, L1).double()
    single[kind] = (x.double().cpu().numpy(), info['num_iterations'],
                    float(torch.linalg.vector_norm(r)) / bn)

  def rank_main(rank):
    part, op, ids, b_loc = _rank_problem(rank, n, P, dtype, jitter, f,
                                         lookup)
    res = {}
    for kind in kinds:
      M = (None if kind is None else JacobiPreconditioner(op, L0, L1)
           if kind == 'jacobi' else PMultigridPreconditioner(op, L0, L1))
      A = solver.OverlappedHelmholtz(op, part.plan, L0, L1)
      run = solver.make_runner(A, b_loc, part.plan, tol=tol, maxiter=5000,
                               M=M)
      if kind == 'jacobi':
        assert run.jacobi is not None          # the fused updates
      if kind == 'pmg':
        assert run.rr_stop is not None         # stops on the global r.r
      x, info = solver.cg(A, b_loc, part.plan, tol=tol, maxiter=5000, M=M)
      res[kind] = (x.double().cpu().numpy(), info['num_iterations'],
                   info['status'])
    return ids.cpu().numpy(), res

  out = inprocess.ThreadWorld(8).run(rank_main)
  # true global residual of the gathered solution, with the one-rank operator
  result = {}
  for kind in kinds:
    xg = np.full(N, np.nan)
    iters = set()
    for ids, res in out.values():
      x, it, status = res[kind]
      assert status == 'converged', (kind, status)
      xg[ids] = x
      iters.add(it)
    assert len(iters) == 1                   # one decision on every rank
    assert not np.isnan(xg).any()
    xt = torch.as_tensor(xg, dtype=dtype, device=DEV)
    r = b.double() - gop.apply(xt, L0, L1).double()
    result[kind] = dict(x=xg, iters=iters.pop(),
                        residual=float(torch.linalg.vector_norm(r)) / bn,
                        single=single[kind])
  return result


@pytest.mark.parametrize('P', [5, 9])
def test_partitioned_pmg_and_jacobi_solves(P):
  """fp64, tol 1e-10, p = 4 and p = 8 on the jittered 2 x 2 x 2 box: the
  gathered solution is the one-rank solution, pMG needs at most 2 more
  iterations than on one rank and far fewer than plain CG, and the true
  global residual meets the tolerance."""
  tol = 1e-10
  res = _solve_case(2, P, torch.float64, tol, 0.1, [None, 'jacobi', 'pmg'])
  plain, jac, mg = res[None], res['jacobi'], res['pmg']
  # the reference: one-rank plain CG
  xs = plain['single'][0]
  for kind in (None, 'jacobi', 'pmg'):
    err = np.abs(res[kind]['x'] - xs).max() / np.abs(xs).max()
    assert err <= 1e-8, (kind, err)
  # ... and the one-rank pMG solve, which meets the tolerance itself
  xm = mg['single'][0]
  err = np.abs(mg['x'] - xm).max() / np.abs(xm).max()
  assert err <= 1e-8, err
  assert mg['single'][2] <= 1.1 * tol, mg['single'][2]
  assert mg['iters'] <= mg['single'][1] + 2, (mg['iters'], mg['single'][1])
  assert 4 * mg['iters'] <= plain['iters'], (mg['iters'], plain['iters'])
  assert mg['residual'] <= 1.1 * tol, mg['residual']
  assert jac['residual'] <= 1.1 * tol, jac['residual']
  # Jacobi: the same PCG as on one rank, to rounding
  assert abs(jac['iters'] - jac['single'][1]) <= 3, (jac['iters'],
                                                     jac['single'][1])


def test_config5_miniature_fp32():
  """p = 11 (P = 12), fp32, 2 x 2 x 2, tol 1e-6: the layout and order of
  BASELINE config 5 on one element per block.  CG stops on its recursive
  residual; the true residual of a float32 solution measured with the
  float32 apply is limited by that apply's rounding (1e-5 here, on one rank
  as on eight), so it is held to the one-rank solve's."""
  tol = 1e-6
  res = _solve_case(1, 12, torch.float32, tol, 0.1, [None, 'pmg'])
  plain, mg = res[None], res['pmg']
  xs = plain['single'][0]
  assert np.abs(mg['x'] - xs).max() <= 1e-4 * np.abs(xs).max()
  assert mg['iters'] <= mg['single'][1] + 2, (mg['iters'], mg['single'][1])
  assert 4 * mg['iters'] <= plain['iters'], (mg['iters'], plain['iters'])
  assert mg['residual'] <= 2.0 * mg['single'][2], (mg['residual'],
                                                   mg['single'][2])


def test_unpreconditioned_partitioned_cg_is_unchanged():
  """M = None takes exactly the path it took before preconditioners were
  accepted on partitions (identity M, fused r.r, no r.r-stopping or Jacobi
  state): the iteration count and, to the rounding of the atomic exchange,
  the iterate of the runner built without the M argument."""
  n, P, tol = 2, 5, 1e-10
  _, _, f, _, lookup = _whole(n, P, torch.float64, 0.1)

  def rank_main(rank):
    part, op, _, b_loc = _rank_problem(rank, n, P, torch.float64, 0.1, f,
                                       lookup)
    A = solver.OverlappedHelmholtz(op, part.plan, L0, L1)
    x1, info1 = solver.cg(A, b_loc, part.plan, tol=tol, M=None)
    x1 = x1.clone()
    b = b_loc.clone()
    from swirl_fem_amd.distributed import comm
    comm.neighbor_exchange_(b, part.plan)
    run = cg_lib.CGRunner(
        A, b, None, tol=tol, reduce_fn=comm.all_reduce_sum_,
        interface=part.plan.interface_weights(DEV, num_nodes=b.shape[0]))
    assert run.rr_stop is None and run.jacobi is None and run.fuse_rr
    while not run.done():
      for _ in range(16):
        run.step()
    err = float((x1 - run.x).abs().max() / run.x.abs().max())
    return err, info1['num_iterations'], run.info()['num_iterations']

  for err, i1, i2 in inprocess.ThreadWorld(8).run(rank_main).values():
    assert err <= 1e-10 and i1 == i2, (err, i1, i2)


def test_partitioned_cg_refuses_inconsistent_preconditioners():
  n, P = 2, 5
  _, _, f, _, lookup = _whole(n, P, torch.float64, 0.0)

  def rank_main(rank):
    part, op, _, b_loc = _rank_problem(rank, n, P, torch.float64, 0.0, f,
                                       lookup)
    with pytest.raises(ValueError, match='interface weights'):
      solver.make_runner(op, b_loc, part.plan, M=lambda r: r)
    return True

  assert all(inprocess.ThreadWorld(8).run(rank_main).values())
