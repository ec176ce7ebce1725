"""Jacobi preconditioning: the assembled operator diagonal (`sfem_helmholtz_diag`)
against the CPU oracle, and CG with the diagonal folded into its vector
updates (`sfem_cg_update_r_jacobi` / `sfem_cg_update_xp_jacobi`) against the
unfused preconditioned CG and the oracle's PCG.  Needs a real MI355X.
"""
import numpy as np
import pytest
import torch

from oracle import sfem_oracle as O
from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType, Quadrature1D
from swirl_fem_amd.core.mesh_refiner import refine_premesh
from swirl_fem_amd.linalg.cg import CGRunner, cg
from swirl_fem_amd.linalg.jacobi import JacobiPreconditioner
from tests.fp32util import f32_mesh

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NT = {'gll': NodeType.GAUSS_LOBATTO_LEGENDRE, 'gl': NodeType.GAUSS_LEGENDRE}


def relerr(a, b):
  a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
  b = np.asarray(b)
  assert a.shape == b.shape, (a.shape, b.shape)
  return np.abs(a.astype(np.float64) - b).max() / max(np.abs(b).max(), 1e-300)


def dev(x, dtype=None):
  t = torch.as_tensor(np.ascontiguousarray(x), device=DEV)
  return t if dtype is None else t.to(dtype)


def premesh(ndim, n, P, mode='jitter', seed=0, periodic=()):
  rng = np.random.default_rng(seed)
  pm = unit_cube_mesh(n, ndim=ndim, periodic_dims=periodic)
  x = pm.node_coords.copy()
  if mode == 'jitter':
    x = x + 0.1 / n * rng.uniform(-1, 1, x.shape)
  elif mode == 'sheared':
    A = np.eye(ndim) + 0.3 * rng.uniform(-1, 1, (ndim, ndim))
    x = x @ A.T + 0.1
  elif mode == 'aniso':
    x = x * np.array([1.0] * (ndim - 1) + [0.125])
  return refine_premesh(pm.replace(node_coords=x),
                        Nodes1D.create(P, NT['gll']))


def spaces(rp, P, q, qt, dtype=torch.float64):
  rp = f32_mesh(rp, dtype)
  mesh = rp.finalize(device=DEV, dtype=dtype)
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(q, NT[qt]))
  ofes = O.FESpace(rp.node_coords, rp.elements, (P, 'gll'), (q, qt))
  return mesh, fes, ofes


def oracle_diagonal(ofes, l0, l1, dirichlet=None):
  """diag(l0 B + l1 A) from the oracle's own matrices and geometric factors:
  sum_q W (M_qi)^2 and sum_q wdet |J^-T grad phi_i|^2 per element, then the
  oracle's scatter."""
  wdet = ofes.jacdets * ofes.weights[None, :]                  # (E, Q)
  mass = np.einsum('eq,qi->ei', wdet, ofes.M ** 2)
  phys = np.einsum('qid,eqjd->eqij', ofes.G, ofes.invjacs)     # (E, Q, n, d)
  stiff = np.einsum('eq,eqij->ei', wdet, phys ** 2)
  d = ofes.scatter(l0 * mass + l1 * stiff)
  if dirichlet is not None:
    d = d * (1.0 - dirichlet.astype(np.float64))
  return d


@pytest.mark.parametrize('ndim,n,P', [(2, 3, 2), (2, 2, 5), (2, 2, 8),
                                      (2, 2, 12), (3, 2, 2), (3, 2, 5),
                                      (3, 1, 8), (3, 1, 12)])
@pytest.mark.parametrize('geometry', ['auto', 'stored'])
@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_collocated_diagonal_matches_oracle(ndim, n, P, geometry, dtype):
  rp = premesh(ndim, n, P, 'jitter', seed=P)
  mesh, fes, ofes = spaces(rp, P, P, 'gll', dtype)
  bm = mesh.physical_masks['boundary']
  tol = 1e-12 if dtype == torch.float64 else 1e-5
  op = fes.helmholtz_operator(None, geometry)
  opb = fes.helmholtz_operator(bm, geometry)
  for l0, l1 in ((1.0, 0.0), (0.0, 1.0), (0.7, 1.3)):
    assert relerr(op.diagonal(l0, l1), oracle_diagonal(ofes, l0, l1)) < tol
    got = opb.diagonal(l0, l1)
    assert relerr(got, oracle_diagonal(ofes, l0, l1,
                                       bm.cpu().numpy())) < tol
    assert float(got[bm].abs().max()) == 0.0


@pytest.mark.parametrize('mode', ['structured', 'sheared', 'aniso'])
@pytest.mark.parametrize('ndim,P', [(2, 4), (3, 3), (3, 7)])
def test_affine_and_box_diagonals(mode, ndim, P):
  rp = premesh(ndim, 2, P, mode, seed=3)
  mesh, fes, ofes = spaces(rp, P, P, 'gll')
  op = fes.helmholtz_operator(mesh.physical_masks['boundary'])
  assert op.num_affine == mesh.num_elements
  ref = oracle_diagonal(ofes, 0.4, 1.1,
                        mesh.physical_masks['boundary'].cpu().numpy())
  assert relerr(op.diagonal(0.4, 1.1), ref) < 1e-12


def test_diagonal_equals_unit_vector_probes_of_apply():
  """d_i = e_i . apply(e_i): the diagonal of exactly what `apply` computes,
  mixed geometry kinds, Dirichlet rows included."""
  rp = premesh(2, 3, 4, 'jitter', seed=5)
  xc = rp.node_coords.copy()
  xc[:, 1] += 0.02 * np.sin(np.pi * xc[:, 0]) * xc[:, 1] * (1 - xc[:, 1]) * (
      xc[:, 0] < 1.0 / 3)
  rp = rp.replace(node_coords=xc)
  mesh, fes, _ = spaces(rp, 4, 4, 'gll')
  op = fes.helmholtz_operator(mesh.physical_masks['boundary'])
  assert op.num_curved > 0 and op.num_multilinear > 0
  N = mesh.num_nodes
  eye = torch.eye(N, dtype=torch.float64, device=DEV)
  probe = torch.stack([op.apply(eye[i], 0.3, 1.7)[i] for i in range(N)])
  assert relerr(op.diagonal(0.3, 1.7), probe.cpu().numpy()) < 1e-13


@pytest.mark.parametrize('ndim,n,P', [(2, 3, 3), (2, 2, 6), (2, 1, 8),
                                      (2, 1, 11), (3, 2, 3), (3, 1, 5)])
@pytest.mark.parametrize('geometry', ['auto', 'stored'])
@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_two_grid_diagonal_matches_oracle(ndim, n, P, geometry, dtype):
  """Gauss quadrature with P - 1 + (d + 1) // 2 points (solve_poisson)."""
  from swirl_fem_amd.core import operators
  q = P - 1 + (ndim + 1) // 2
  rp = premesh(ndim, n, P, 'jitter', seed=7)
  mesh, fes, ofes = spaces(rp, P, q, 'gl', dtype)
  bm = mesh.physical_masks['boundary']
  op = fes.helmholtz_operator(bm, geometry)
  assert isinstance(op, operators.TwoGridHelmholtzOperator)
  tol = 1e-12 if dtype == torch.float64 else 1e-5
  for l0, l1 in ((1.0, 0.0), (0.0, 1.0), (0.5, 2.0)):
    ref = oracle_diagonal(ofes, l0, l1, bm.cpu().numpy())
    assert relerr(op.diagonal(l0, l1), ref) < tol


def test_periodic_box_diagonal():
  P = 4
  rp = premesh(3, 3, P, 'none', periodic=(0, 1))
  mesh, fes, ofes = spaces(rp, P, P, 'gll')
  op = fes.helmholtz_operator(None)
  assert relerr(op.diagonal(0.5, 1.0), oracle_diagonal(ofes, 0.5, 1.0)) < 1e-12


def test_jacobi_preconditioner_values():
  rp = premesh(2, 3, 4, 'jitter')
  mesh, fes, _ = spaces(rp, 4, 4, 'gll')
  bm = mesh.physical_masks['boundary']
  op = fes.helmholtz_operator(bm)
  d = op.diagonal(0.0, 1.0)
  M = JacobiPreconditioner(op, 0.0, 1.0)
  dinv = M.jacobi_diagonal()
  assert float(dinv[bm].abs().max()) == 0.0
  inner = ~bm
  assert torch.allclose(dinv[inner] * d[inner],
                        torch.full_like(d[inner], float(d.max())))
  assert float(dinv[inner].min()) >= 1.0
  r = torch.randn(mesh.num_nodes, dtype=torch.float64, device=DEV) * (~bm)
  assert float(torch.dot(r, M(r))) >= float(torch.dot(r, r))
  loose = JacobiPreconditioner(d, strict=False)
  assert torch.allclose(loose.jacobi_diagonal()[inner], 1.0 / d[inner])


# --------------------------------------------------------------- fused CG
def _box_problem(P=6, n=3, seed=0):
  rp = premesh(3, n, P, 'jitter', seed=seed)
  mesh, fes, _ = spaces(rp, P, P, 'gll')
  bm = mesh.physical_masks['boundary']
  op = fes.helmholtz_operator(bm)
  rng = np.random.default_rng(seed + 1)
  b = op.apply(dev(rng.standard_normal(mesh.num_nodes)), 1.0, 0.0)
  return mesh, op, b


def _run(A, b, M, steps, **kw):
  run = CGRunner(A, b, M=M, tol=1e-14, **kw)
  for _ in range(steps):
    run.step()
  info = run.info()
  return run, run.x.clone(), info


@pytest.mark.parametrize('path', ['plain', 'layered', 'layered_det', 'lazy'])
def test_fused_jacobi_equals_unfused(path, monkeypatch):
  if path == 'lazy':
    monkeypatch.setenv('SFEM_LAZY_X_MIN_MB', '0')
  if path == 'layered':
    monkeypatch.setenv('SFEM_DETERMINISTIC', '0')
  mesh, op, b = _box_problem()
  M = JacobiPreconditioner(op, 0.2, 1.0)
  if path in ('plain', 'lazy'):
    A = lambda u: op.apply(u, 0.2, 1.0)
  else:
    A = op.linear_operator(0.2, 1.0)
  results = {}
  for fused in ('1', '0'):
    monkeypatch.setenv('SFEM_FUSED_JACOBI', fused)
    run, x, info = _run(A, b, M, 25)
    assert (run.jacobi is not None) == (fused == '1')
    if path.startswith('layered'):
      assert run.layered is not None
      assert (run.det is not None) == (path == 'layered_det')
    if path == 'lazy' and fused == '0':
      assert run.lazy is not None
    results[fused] = (x, info)
  (x1, i1), (x0, i0) = results['1'], results['0']
  assert i1['num_iterations'] == i0['num_iterations'] == 25
  assert relerr(x1, x0.cpu().numpy()) < 1e-12
  # and to convergence: same iteration counts
  counts = []
  for fused in ('1', '0'):
    monkeypatch.setenv('SFEM_FUSED_JACOBI', fused)
    _, info = cg(A, b, tol=1e-9, M=M)
    counts.append(info['num_iterations'])
  assert counts[0] == counts[1]


def test_fused_jacobi_component_major_field(monkeypatch):
  from swirl_fem_amd.core import layout
  mesh, op, _ = _box_problem(P=4, n=3)
  if mesh.num_nodes % 2:
    pytest.skip('odd node count: the fused vector path needs N even in fp64')
  rng = np.random.default_rng(4)
  keep = (~mesh.physical_masks['boundary']).to(torch.float64)[:, None]
  b = layout.component_major(dev(rng.standard_normal((mesh.num_nodes, 3))) *
                             keep)
  M = JacobiPreconditioner(op, 2.0, 0.5)
  A = lambda u: op.apply(u, 2.0, 0.5)
  out = {}
  for fused in ('1', '0'):
    monkeypatch.setenv('SFEM_FUSED_JACOBI', fused)
    run, x, info = _run(A, b, M, 12)
    assert (run.jacobi is not None) == (fused == '1')
    if fused == '1':
      assert run.jacobi[1] == 3
    out[fused] = (x, info)
  assert relerr(out['1'][0], out['0'][0].cpu().numpy()) < 1e-12
  assert out['1'][1]['num_iterations'] == out['0'][1]['num_iterations']


def test_jacobi_pcg_matches_oracle_pcg():
  P = 4
  rp = premesh(2, 4, P, 'jitter', seed=9)
  mesh, fes, ofes = spaces(rp, P, P, 'gll')
  bm = mesh.physical_masks['boundary']
  bmask = bm.cpu().numpy()
  keep = 1.0 - bmask.astype(np.float64)
  op = fes.helmholtz_operator(bm)
  rng = np.random.default_rng(10)
  b = keep * ofes.scatter(ofes.mass_local(ofes.gather(
      rng.standard_normal(mesh.num_nodes))))

  def A_o(u):
    return keep * ofes.scatter(ofes.stiffness_local(ofes.gather(u)))

  d = oracle_diagonal(ofes, 0.0, 1.0, bmask)
  dinv = np.where(d != 0, d.max() / np.where(d != 0, d, 1.0), 0.0)
  xo, io = O.cg(A_o, b, tol=1e-10, M=lambda r: dinv * r)
  M = JacobiPreconditioner(op, 0.0, 1.0)
  xg, ig = cg(op.linear_operator(0.0, 1.0), dev(b), tol=1e-10, M=M)
  assert ig['num_iterations'] == io['num_iterations']
  assert relerr(xg, xo) < 1e-9
  xp, ip = cg(op.linear_operator(0.0, 1.0), dev(b), tol=1e-10)
  assert ig['num_iterations'] < ip['num_iterations']


def test_layered_jacobi_solves_are_bitwise_reproducible():
  mesh, op, b = _box_problem(P=7, n=3, seed=2)
  A = op.linear_operator(0.0, 1.0)
  M = JacobiPreconditioner(op, 0.0, 1.0)
  run = CGRunner(A, b, M=M, tol=1e-9)
  assert run.jacobi is not None and run.det is not None
  xs = []
  for graph in (False, False, True, True):
    x, info = cg(A, b, tol=1e-9, M=M, graph=graph)
    assert info['status'] == 'converged'
    xs.append((x.clone(), info['num_iterations']))
  for x, k in xs[1:]:
    assert k == xs[0][1]
    assert torch.equal(x, xs[0][0])


@pytest.mark.parametrize('case', ['aniso', 'jitter7'])
def test_poisson_jacobi_converges_faster(case):
  from swirl_fem_amd.examples.poisson import BCType, solve_poisson
  if case == 'aniso':
    P, n, ndim = 4, 4, 3
    rp = premesh(ndim, n, P, 'aniso')
  else:
    P, n, ndim = 8, 2, 3
    rp = premesh(ndim, n, P, 'jitter', seed=13)
  mesh = rp.finalize(device=DEV)
  rng = np.random.default_rng(14)
  f = rng.standard_normal(mesh.num_nodes)
  bc = {'boundary': (BCType.DIRICHLET, 0.)}
  tol = 1e-12
  u0, i0 = solve_poisson(mesh, dev(f), bc, rtol=tol, return_info=True)
  u1, i1 = solve_poisson(mesh, dev(f), bc, rtol=tol, return_info=True,
                         preconditioner='jacobi')
  assert i1['num_iterations'] < i0['num_iterations'], (i1, i0)
  assert relerr(u1, u0.cpu().numpy()) < 1e-7
  bmask = mesh.physical_masks['boundary'].cpu().numpy()
  uo = O.solve_poisson(rp.node_coords, rp.elements, (P, 'gll'), bmask, f,
                       rtol=tol)
  assert relerr(u1, uo) < 1e-7
  with pytest.raises(ValueError):
    solve_poisson(mesh, dev(f), bc, preconditioner='ilu')


def test_mass_diagonal_equals_the_stokes_lumped_mass():
  """diag(B) on GLL nodes is the lumped mass: equal to the exchanged
  `velocity_mass_diag` of a StokesSEM on a periodic box."""
  from swirl_fem_amd.core import operators
  from swirl_fem_amd.navier_stokes.navier_stokes import StokesSEM
  sem = StokesSEM.create(unit_cube_mesh(3, ndim=3, periodic_dims=(0, 1, 2)),
                         {}, order=4, device=DEV)
  op = operators.HelmholtzOperator.create(sem.velocity.vspace, None)
  d = sem.velocity.exchange(op.diagonal(1.0, 0.0)[:, None].expand(-1, 3)
                            .contiguous())
  want = sem.velocity.exchange(sem.velocity_mass_diag)
  assert float((d - want).abs().max()) <= 1e-14 * float(want.abs().max())


@pytest.mark.parametrize('grid', [(2, 1, 1), (2, 2, 2)])
def test_partitioned_diagonal_equals_single_rank(grid):
  """Thread ranks (`distributed/inprocess.py`) on block partitions: the
  assembled diagonal and the (globally scaled) dinv equal the single-rank
  ones at every node."""
  from swirl_fem_amd.core import operators
  from swirl_fem_amd.distributed import blocks, inprocess
  n, P = 2, 5
  gll = Nodes1D.create(P, NT['gll'])

  def setup(part):
    mesh = part.mesh
    fes = FiniteElementSpace.create(mesh,
                                    Quadrature1D.create_from_nodes_1d(gll))
    op = operators.HelmholtzOperator.create(fes,
                                            mesh.physical_masks['boundary'])
    d = op.diagonal(0.3, 1.0)
    M = JacobiPreconditioner(op, 0.3, 1.0)
    return (np.asarray(part.global_keys), d.cpu().numpy(),
            M.jacobi_diagonal().cpu().numpy())

  total = tuple(n * g for g in grid)
  keys1, d1, dinv1 = setup(blocks.build_block_partition(
      total, P, (1, 1, 1), 0, device=DEV, jitter=0.1))
  order = np.argsort(keys1)
  world = inprocess.ThreadWorld(int(np.prod(grid)))
  out = world.run(lambda rank: setup(blocks.build_block_partition(
      n, P, grid, rank, device=DEV, jitter=0.1)))
  seen = set()
  for rank, (keys, d, dinv) in out.items():
    at = order[np.searchsorted(keys1, keys, sorter=order)]
    assert np.array_equal(keys1[at], keys)
    assert np.abs(d - d1[at]).max() <= 1e-13 * np.abs(d1).max(), rank
    assert np.abs(dinv - dinv1[at]).max() <= 1e-13 * np.abs(dinv1).max()
    seen.update(keys.tolist())
  assert len(seen) == len(keys1)


# ------------------------------------------------------------ the stepper
def _iters(diag):
  return [v for v, _ in diag['cg_iterations']]


def test_stepper_jacobi_lid_driven_cavity_and_taylor_green():
  """`velocity_preconditioner='jacobi'`: the same steps as the default
  M = QQ^T to the solver tolerance, no more velocity iterations."""
  from swirl_fem_amd.examples import navier_stokes_driver as drv
  from swirl_fem_amd.navier_stokes import navier_stokes as ns
  kw = dict(n=4, order=6, reynolds=10.0, dt=5e-3, steps=2, time_order=2,
            device=DEV, tol=1e-11)
  _, u0, p0, d0 = drv.lid_driven_cavity(**kw)
  sem1, u1, p1, d1 = drv.lid_driven_cavity(velocity_preconditioner='jacobi',
                                           **kw)
  assert float((u1 - u0).abs().max()) <= 1e-8 * float(u0.abs().max())
  assert sum(_iters(d1)) <= sum(_iters(d0)), (_iters(d0), _iters(d1))
  pcs = [v for k, v in sem1._cache.items()
         if isinstance(k, tuple) and k[0] == 'velocity_jacobi_pc']
  assert len(pcs) >= 1 and all(
      isinstance(m, ns._JacobiVelocityPreconditioner) for m in pcs)
  # one partition, no periodic images: M is diagonal and cg fuses it
  assert pcs[0].jacobi_diagonal() is not None
  kw = dict(n=3, order=5, reynolds=20.0, dt=1e-2, steps=2, time_order=2,
            device=DEV, tol=1e-11)
  _, u0, p0, d0 = drv.taylor_green(**kw)
  sem2, u1, p1, d1 = drv.taylor_green(velocity_preconditioner='jacobi', **kw)
  assert float((u1 - u0).abs().max()) <= 1e-8 * float(u0.abs().max())
  assert sum(_iters(d1)) <= sum(_iters(d0)), (_iters(d0), _iters(d1))
  # periodic images: M = (d_max / d) QQ^T, symmetric, r.Mr >= r.QQ^T r
  M = [v for k, v in sem2._cache.items()
       if isinstance(k, tuple) and k[0] == 'velocity_jacobi_pc'][0]
  assert M.jacobi_diagonal() is None
  g = torch.Generator(device=DEV).manual_seed(4)
  N = sem2.velocity.mesh.num_nodes
  a = torch.randn(N, 3, dtype=torch.float64, device=DEV, generator=g)
  b = torch.randn(N, 3, dtype=torch.float64, device=DEV, generator=g)
  lhs, rhs = float((a * M(b)).sum()), float((b * M(a)).sum())
  assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)
  assert float((a * M(a)).sum()) >= float(
      (a * sem2.velocity.exchange(a)).sum()) * (1 - 1e-12)


def test_stepper_jacobi_ensemble_equals_members():
  from swirl_fem_amd.examples.navier_stokes_driver import navier_stokes_step
  from swirl_fem_amd.navier_stokes.navier_stokes import StokesSEM
  from swirl_fem_amd.niles.datagen import datagen
  sem = StokesSEM.create(unit_cube_mesh(4, ndim=2, periodic_dims=(0, 1)), {},
                         order=5, device=DEV)
  B = 2
  ens = sem.ensemble(B)
  x = sem.velocity.mesh.node_coords
  u0 = torch.stack([a * datagen.u_init_fn(x) for a in (1.0, 0.5)])
  Np = sem.pressure.pspace.mesh.num_nodes
  p0 = torch.zeros(B, Np, dtype=torch.float64, device=DEV)
  kw = dict(reynolds=50.0, dt=2e-3, time_order=2, tol=1e-11, atol=0.0,
            velocity_preconditioner='jacobi')

  def run(s, u, p, steps=2):
    us, ps = (u, u), (p, p)
    c = s.C(u)
    Cus = (c, c)
    for _ in range(steps):
      f = datagen.forcing(s.velocity.mesh.node_coords, us[-1], 0.1)
      un, pn, cn, _ = navier_stokes_step(s, us, ps, Cus, forcing=f, **kw)
      us, ps, Cus = us[1:] + (un,), ps[1:] + (pn,), Cus[1:] + (cn,)
    return us[-1], ps[-1]

  ue, pe = run(ens, ens.flatten(u0), ens.flatten(p0))
  ue = ens.unflatten(ue)
  for b in range(B):
    ub, _ = run(sem, u0[b], p0[b])
    assert float((ue[b] - ub).abs().max()) <= 1e-9 * float(ub.abs().max()), b
