"""p-multigrid on the GPU (`linalg/pmg.py`, `csrc/sfem_pmg.hip`): transfers,
the fused Chebyshev step, the V-cycle against the NumPy restatement
(`tests/pmg_reference.py`), PCG stopping on r.r, `solve_poisson(...,
preconditioner='pmg')`, reproducibility and graph capture.  Small meshes
only.  Needs a real MI355X."""
import numpy as np
import pytest
import torch

from swirl_fem_amd import _ops
from swirl_fem_amd.core import operators
from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import NodeType, Quadrature1D
from swirl_fem_amd.linalg import pmg
from swirl_fem_amd.linalg.cg import CGRunner, cg
from swirl_fem_amd.linalg.pmg import PMultigridPreconditioner
from tests import geometry_cases as G
from tests import pmg_reference as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _problem(ndim, n, P, mode='jitter', dtype=torch.float64, quad=None,
             periodic=(), seed=0, dirichlet=True):
  rp = R.box(n, ndim, P, mode, seed=seed, periodic=periodic)
  mesh = rp.finalize(device=DEV, dtype=dtype)
  q = Quadrature1D.create(P, NodeType.GAUSS_LOBATTO_LEGENDRE) if quad is None \
      else Quadrature1D.create(quad, NodeType.GAUSS_LEGENDRE)
  fes = FiniteElementSpace.create(mesh, q)
  bm = mesh.physical_masks.get('boundary') if dirichlet else None
  op = fes.helmholtz_operator(bm)
  return rp, mesh, fes, op, bm


def _np(t):
  return t.detach().double().cpu().numpy()


def _reference(rp, mesh, M, bm, l0, l1, quad=None):
  x = np.asarray(rp.node_coords, dtype=np.float64)
  el = mesh.elements.cpu().numpy().astype(np.int64)
  bnd = np.zeros(len(x), bool) if bm is None else bm.cpu().numpy()
  return R.Hierarchy(
      x, el, mesh.order, bnd, l0, l1, orders=M.orders, degree=M.degree,
      quad=None if quad is None else (quad, 'gl'),
      lam_max=[lev.lam_max for lev in M.levels[:-1]],
      coarse=(M.coarse_steps,) + tuple(M.coarse_bounds))


PAIRS = sorted({(pc, pf) for p in range(2, 13)    # 12: 13 -> 7 points
                for pf, pc in zip(pmg.default_orders(p),
                                  pmg.default_orders(p)[1:])})


@pytest.mark.parametrize('ndim', [2, 3])
@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_transfers_every_default_pair(ndim, dtype):
  """P exact on polynomials of degree <= p_c, equal to the NumPy transfer,
  and <P x, y> = <x, P^T y>."""
  for pc, pf in PAIRS:
    _check_transfer(ndim, dtype, pc, pf)


RUN_TIME_PAIRS = ((2, 7), (1, 4), (3, 9), (4, 12))


@pytest.mark.parametrize('ndim', [2, 3])
def test_transfers_run_time_sizes(ndim):
  """Pairs outside the default schedules (orders=[7, 2, 1], ...) take the
  run-time-size kernels; (4, 12) has the 13 fine points of the largest
  compiled pair."""
  assert not set(RUN_TIME_PAIRS) & set(PAIRS) and (6, 12) in PAIRS
  for dtype in (torch.float64, torch.float32):
    for pc, pf in RUN_TIME_PAIRS:
      _check_transfer(ndim, dtype, pc, pf)


def _check_transfer(ndim, dtype, pc, pf):
  tol = 1e-12 if dtype == torch.float64 else 1e-5
  if ndim == 3 and pf > 8:
    n = 1
  else:
    n = 2
  rp = R.box(n, ndim, pf + 1, 'sheared', seed=pf)
  fmesh = rp.finalize(device=DEV, dtype=dtype)
  cmesh, celems = pmg.coarse_mesh(fmesh, pc)
  fel = fmesh.elements.to(torch.int64)
  bm = fmesh.physical_masks['boundary']
  cdir = torch.zeros(cmesh.num_nodes, dtype=torch.bool, device=DEV)
  cdir[celems.reshape(-1)] = pmg.coarse_dirichlet(
      bm[fel], ndim, pf, pc).reshape(-1)
  cidx, fidx = pmg.encode_rows(celems, cdir), pmg.encode_rows(fel, bm)
  owner = pmg.owner_bits(fel, fmesh.num_nodes)
  mat = torch.as_tensor(pmg.interpolation_1d(pc, pf), dtype=dtype,
                        device=DEV).contiguous()
  # polynomials of degree pc (affine map: still degree pc in x)
  xc = cmesh.node_coords.double()
  xf = fmesh.node_coords.double()
  poly = lambda x: (x[:, 0] ** pc + 0.5 * x[:, 1] ** max(pc - 1, 0) *
                    x[:, 0] + 0.3)
  uc = poly(xc).to(dtype).contiguous()
  uf = torch.full((fmesh.num_nodes,), float('nan'), dtype=dtype, device=DEV)
  nobm = pmg.encode_rows(fel, None)
  nocd = pmg.encode_rows(celems, None)
  _ops.pmg_prolong(uc, uf, nocd, nobm, owner, mat, ndim, pc + 1, pf + 1)
  err = (uf.double() - poly(xf)).abs().max() / poly(xf).abs().max()
  assert float(err) < 50 * tol, (pc, pf, float(err))
  # against the NumPy transfer, Dirichlet nodes included
  fel_np = _np(fel).astype(np.int64)
  fine = R.Level(np.asarray(rp.node_coords, np.float64), fel_np, pf,
                 bm.cpu().numpy(), np.zeros(fel_np.shape + fel_np.shape[1:]))
  _, Pm = R.coarsen(fine, pc, 0.0, 1.0)
  g = torch.Generator(device='cpu').manual_seed(pf)
  a = torch.randn(cmesh.num_nodes, generator=g, dtype=torch.float64)
  y = torch.randn(fmesh.num_nodes, generator=g, dtype=torch.float64)
  uf = torch.full((fmesh.num_nodes,), float('nan'), dtype=dtype, device=DEV)
  _ops.pmg_prolong(a.to(DEV, dtype), uf, cidx, fidx, owner, mat, ndim,
                   pc + 1, pf + 1)
  ref = Pm @ a.numpy()
  assert np.abs(_np(uf) - ref).max() < tol * np.abs(ref).max()
  uf2 = uf.clone()
  _ops.pmg_prolong(a.to(DEV, dtype), uf2, cidx, fidx, owner, mat, ndim,
                   pc + 1, pf + 1, add=True)
  assert np.abs(_np(uf2) - 2 * ref).max() < 2 * tol * np.abs(ref).max()
  loc = torch.zeros(celems.numel(), dtype=dtype, device=DEV)
  offsets, slots = cmesh.assembly_plan().csr()
  _ops.pmg_restrict(y.to(DEV, dtype), loc, cidx, fidx, owner, mat, ndim,
                    pc + 1, pf + 1)
  rc = _ops.scatter_csr(loc, offsets, slots, cmesh.num_nodes)
  ref_t = Pm.T @ y.numpy()
  assert np.abs(_np(rc) - ref_t).max() < tol * np.abs(ref_t).max()
  lhs = float(np.dot(_np(uf), y.numpy()))
  rhs = float(np.dot(a.numpy(), _np(rc)))
  assert abs(lhs - rhs) < 10 * tol * max(abs(lhs), 1.0)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
@pytest.mark.parametrize('n', [1000, 1001, 4099])
def test_cheb_step_modes(dtype, n):
  g = torch.Generator().manual_seed(n)
  v = [torch.randn(n, generator=g, dtype=torch.float64) for _ in range(5)]
  x, d, ax, b, dinv = (t.to(DEV, dtype) for t in v)
  a, c = 0.37, 1.9
  tol = 1e-14 if dtype == torch.float64 else 1e-6
  cases = {
      0: lambda X, D: (X + a * D + c * v[4] * (v[3] - v[2]),
                       a * D + c * v[4] * (v[3] - v[2])),
      1: lambda X, D: (c * v[4] * v[3], c * v[4] * v[3]),
      3: lambda X, D: (X + c * v[4] * (v[3] - v[2]), c * v[4] * (v[3] - v[2])),
  }
  for mode, f in cases.items():
    X, D = x.clone(), d.clone()
    _ops.cheb_step(X, D, None if mode == 1 else ax, b, dinv, None, a, c, mode)
    rx, rd = f(v[0], v[1])
    assert (X.double().cpu() - rx).abs().max() < tol * 10 * rx.abs().max()
    assert (D.double().cpu() - rd).abs().max() < tol * 10 * rd.abs().max()
  r = torch.empty_like(b)
  _ops.cheb_step(None, None, ax, b, None, r, 0.0, 0.0, 2)
  assert (r.double().cpu() - (v[3] - v[2])).abs().max() < tol * 10


def test_smoother_and_vcycle_match_numpy():
  rp, mesh, fes, op, bm = _problem(3, 2, 5, 'jitter')
  M = PMultigridPreconditioner(op, 0.3, 1.0)
  H = _reference(rp, mesh, M, bm, 0.3, 1.0)
  g = torch.Generator().manual_seed(1)
  b = torch.randn(mesh.num_nodes, generator=g, dtype=torch.float64)
  b = b * (~bm.cpu())
  bd = b.to(DEV)
  x = M.smooth(0, bd, from_zero=True).clone()
  ref = R.smooth(H.levels[0], b.numpy(), np.zeros(len(b)), H.cheb[0])
  assert np.abs(_np(x) - ref).max() < 1e-12 * np.abs(ref).max()
  z = M(bd)
  ref = H.vcycle(b.numpy())
  assert np.abs(_np(z) - ref).max() < 1e-11 * np.abs(ref).max()


def _level_reference(mesh, dirichlet, l0, l1, u):
  """fp64 oracle of l0 B + l1 A on a level's own (GLL-collocated) mesh."""
  from oracle import sfem_oracle as O
  P = mesh.order + 1
  ofes = O.FESpace(_np(mesh.node_coords), mesh.elements.cpu().numpy(),
                   (P, 'gll'), (P, 'gll'))
  ul = ofes.gather(u)
  out = ofes.scatter(l0 * ofes.mass_local(ul) + l1 * ofes.stiffness_local(ul))
  return out if dirichlet is None else out * ~dirichlet.cpu().numpy()


@pytest.mark.parametrize('name,n,P', [('block_jitter', 4, 5),
                                      ('block_jitter', 3, 9),
                                      ('three_kinds', 3, 5)])
def test_mixed_geometry_levels_and_vcycle(name, n, P):
  """Meshes that mix affine, multilinear (and curved) elements: the coloured
  fine-level copy and every coarse operator against the oracle on that
  level's mesh, and the V-cycle against the NumPy restatement."""
  case = getattr(G, name)(n, 3, P)
  rp = case.rp
  mesh = rp.finalize(device=DEV)
  bm = mesh.physical_masks['boundary']
  fes = FiniteElementSpace.create(
      mesh, Quadrature1D.create(P, NodeType.GAUSS_LOBATTO_LEGENDRE))
  op = fes.helmholtz_operator(bm)
  case.check_counts(op)
  l0, l1 = 0.3, 1.0
  M = PMultigridPreconditioner(op, l0, l1)
  assert M._fine_colored.num_affine == op.num_affine > 0
  g = torch.Generator().manual_seed(7)
  levels = [(M._fine_colored, mesh, bm)] + [
      (lev.op, lev.mesh, lev.dirichlet) for lev in M.levels[1:]]
  for i, (lop, lmesh, ldir) in enumerate(levels):
    u = torch.randn(lmesh.num_nodes, generator=g, dtype=torch.float64)
    ref = _level_reference(lmesh, ldir, l0, l1, u.numpy())
    got = lop.apply(u.to(DEV), l0, l1,
                    out=torch.full((lmesh.num_nodes,), 7.5,
                                   dtype=torch.float64, device=DEV))
    err = np.abs(_np(got) - ref).max() / np.abs(ref).max()
    assert err < 1e-10, (name, P, i, lmesh.order, err)
  H = _reference(rp, mesh, M, bm, l0, l1)
  b = torch.randn(mesh.num_nodes, generator=g, dtype=torch.float64)
  b = b * (~bm.cpu())
  z = M(b.to(DEV))
  ref = H.vcycle(b.numpy())
  assert np.abs(_np(z) - ref).max() < 1e-11 * np.abs(ref).max()


@pytest.mark.parametrize('ndim,n,P', [(2, 3, 7), (3, 2, 4)])
def test_vcycle_symmetric_positive(ndim, n, P):
  rp, mesh, fes, op, bm = _problem(ndim, n, P, 'jitter')
  M = PMultigridPreconditioner(op)
  g = torch.Generator().manual_seed(2)
  keep = (~bm).double()
  for _ in range(3):
    a = (torch.randn(mesh.num_nodes, generator=g, dtype=torch.float64)
         .to(DEV) * keep)
    b = (torch.randn(mesh.num_nodes, generator=g, dtype=torch.float64)
         .to(DEV) * keep)
    ma = M(a).clone()
    mb = M(b).clone()
    lhs, rhs = float(torch.dot(ma, b)), float(torch.dot(a, mb))
    assert abs(lhs - rhs) < 1e-12 * (abs(lhs) + float(ma.norm() * b.norm()))
    assert float(torch.dot(a, ma)) > 0


CASES = [
    dict(ndim=3, n=3, P=6, mode='jitter'),                      # layered
    dict(ndim=3, n=2, P=5, mode='sheared'),                     # affine
    dict(ndim=3, n=2, P=5, mode='curved'),                      # curved
    dict(ndim=2, n=4, P=8, mode='uniform', periodic=(0,)),      # periodic
    dict(ndim=3, n=3, P=6, mode='jitter', quad=7),              # two-grid
    dict(ndim=3, n=2, P=6, mode='jitter', dtype=torch.float32),
]


@pytest.mark.parametrize('case', CASES, ids=lambda c: '-'.join(
    str(v) for v in c.values()))
def test_pcg_iterations(case):
  case = dict(case)
  dtype = case.pop('dtype', torch.float64)
  quad = case.get('quad')
  rp, mesh, fes, op, bm = _problem(dtype=dtype, **case)
  if quad is not None:
    assert isinstance(op, operators.TwoGridHelmholtzOperator)
  M = PMultigridPreconditioner(op)
  g = torch.Generator().manual_seed(3)
  b = torch.randn(mesh.num_nodes, generator=g, dtype=torch.float64) * (
      ~bm.cpu())
  tol = 1e-8 if dtype == torch.float64 else 1e-5
  A = op.linear_operator(0.0, 1.0) if hasattr(op, 'layer_plan') else (
      lambda u: op.apply(u, 0.0, 1.0))
  bd = b.to(DEV, dtype)
  x, info = cg(A, bd, tol=tol, M=M)
  assert info['status'] == 'converged'
  res = float((bd.double() - op.apply(x, 0.0, 1.0).double()).norm())
  assert res <= tol * float(bd.double().norm()) * 1.001
  _, plain = cg(A, bd, tol=tol)
  assert info['num_iterations'] * 5 <= plain['num_iterations'], (
      info, plain)
  if dtype == torch.float64:
    H = _reference(rp, mesh, M, bm, 0.0, 1.0, quad)
    _, it = H.pcg(b.numpy(), tol)
    assert abs(it - info['num_iterations']) <= 1, (it, info)


def test_geometry_kinds_carry_over_p11_fp32():
  """The p = 11 fp32 block: every level of 11 -> 5 -> 2 -> 1 stays affine."""
  _, mesh, fes, op, _ = _problem(3, 2, 12, 'uniform', dtype=torch.float32)
  M = PMultigridPreconditioner(op)
  assert M.orders == [11, 5, 2, 1]
  for lev in M.levels:
    assert lev.op.num_affine == mesh.num_elements, lev.mesh.order


def test_geometry_kinds_carry_over():
  """Affine and multilinear elements stay so on every level; curved ones stay
  curved on every level above order 1."""
  for mode, kind, dtype in (
      ('sheared', 'num_affine', torch.float64),
      ('jitter', 'num_multilinear', torch.float64),
      ('curved', 'num_curved', torch.float64),
      ('uniform', 'num_affine', torch.float32),
      ('jitter', 'num_multilinear', torch.float32)):
    _, mesh, fes, op, _ = _problem(3, 2, 9, mode, dtype=dtype)
    assert getattr(op, kind) == mesh.num_elements
    M = PMultigridPreconditioner(op)
    assert M.orders == [8, 4, 2, 1]
    for lev in M.levels[1:]:
      if kind == 'num_curved' and lev.mesh.order == 1:
        continue
      assert getattr(lev.op, kind) == mesh.num_elements, (mode, kind)


def test_solve_poisson_pmg_meets_true_residual():
  from swirl_fem_amd.examples.poisson import BCType, solve_poisson
  rp = R.box(3, 3, 6, 'jitter', seed=4)
  mesh = rp.finalize(device=DEV)
  x = mesh.node_coords
  f = torch.sin(3 * x[:, 0]) * torch.cos(2 * x[:, 1]) + x[:, 2]
  bcs = {'boundary': (BCType.DIRICHLET, 0.0)}
  rtol = 1e-9
  u, info = solve_poisson(mesh, f, bcs, rtol=rtol, return_info=True,
                          preconditioner='pmg')
  u0, info0 = solve_poisson(mesh, f, bcs, rtol=rtol, return_info=True)
  assert info['status'] == 'converged'
  assert info['num_iterations'] * 5 <= info0['num_iterations']
  # the operator solve_poisson builds (Gauss quadrature: two-grid)
  quad = Quadrature1D.create(mesh.order + 2, NodeType.GAUSS_LEGENDRE)
  fes = FiniteElementSpace.create(mesh, quad)
  keep = ~mesh.physical_masks['boundary']
  op = fes.helmholtz_operator(~keep)
  b = op.apply(f, 1.0, 0.0)
  res = float((b - op.apply(u, 0.0, 1.0)).norm())
  assert res <= rtol * float(b.norm()) * 1.001
  assert float((u - u0).abs().max()) < 1e-6 * float(u0.abs().max())


def test_reproducible_and_graph_captured():
  rp, mesh, fes, op, bm = _problem(3, 3, 6, 'jitter', seed=5)
  M = PMultigridPreconditioner(op)
  A = op.linear_operator(0.0, 1.0)
  g = torch.Generator().manual_seed(6)
  b = (torch.randn(mesh.num_nodes, generator=g, dtype=torch.float64) *
       (~bm.cpu())).to(DEV)
  x1, i1 = cg(A, b, tol=1e-10, M=M)
  x1 = x1.clone()
  x2, i2 = cg(A, b, tol=1e-10, M=M)
  assert i1['num_iterations'] == i2['num_iterations']
  assert torch.equal(x1, x2)
  x3, i3 = cg(A, b, tol=1e-10, M=M, graph=True)
  assert i3['num_iterations'] == i1['num_iterations']
  assert torch.equal(x1, x3)
  run = CGRunner(A, b, tol=1e-10, M=M)
  assert run.rr_stop is not None and run.rr_stop.layered is not None


def test_refusals():
  _, mesh, fes, op, _ = _problem(2, 2, 4, 'uniform')
  with pytest.raises(ValueError):
    PMultigridPreconditioner(op, orders=[3, 2, 2, 1])
  part = mesh.replace(axis_name='x')
  with pytest.raises(NotImplementedError, match='partitioned'):
    pmg.coarse_mesh(part, 1)
  with pytest.raises(NotImplementedError, match='ensemble'):
    pmg.coarse_mesh(mesh.replicate(2), 1)
