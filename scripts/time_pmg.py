"""p-multigrid PCG against plain and Jacobi CG on the fused Helmholtz
operator (the cases of profiles/r05_jacobi.jsonl): setup time of the
V-cycle, time per iteration, iterations and time to the same true-residual
tolerance ||b - A x|| <= TOL ||b||, and a per-level breakdown of the V-cycle
(device-event times of each piece, run alone) with the transfers' must-move
bytes and bandwidth.  One JSON line per case.
env: CASES (uniform,jitter,aniso,p11), N (64), P (8), ANISO_N (32),
P11_N (40), REPS (20), TOL (1e-8), MAXITER (none: 10 N), DEGREE (2),
OUT (stdout only if unset), PROBE_TOL (unset: none) -- one more pMG solve to
PROBE_TOL capped at 100 iterations, to see where a solve stagnates (fp32:
1e-8 is below what the true residual of a float32 solve can reach)."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from swirl_fem_amd import _ops, switches
from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
from swirl_fem_amd.core import operators
from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType, Quadrature1D
from swirl_fem_amd.core.mesh_refiner import refine_premesh
from swirl_fem_amd.linalg.cg import CGRunner, cg
from swirl_fem_amd.linalg.jacobi import JacobiPreconditioner
from swirl_fem_amd.linalg import pmg
from swirl_fem_amd.linalg.pmg import PMultigridPreconditioner

reps = int(os.environ.get('REPS', '20'))
tol = float(os.environ.get('TOL', '1e-8'))
maxiter = int(os.environ['MAXITER']) if 'MAXITER' in os.environ else None
probe_tol = os.environ.get('PROBE_TOL')
degree = int(os.environ.get('DEGREE', '2'))
dev = torch.device('cuda:0')
out_path = os.environ.get('OUT')


def build(case):
  """(mesh, dtype) of a case: n^3 box, P points, fp64 unless p11."""
  if case == 'p11':
    n, P, dt = int(os.environ.get('P11_N', '40')), 12, torch.float32
  elif case == 'aniso':
    n, P, dt = int(os.environ.get('ANISO_N', '32')), int(
        os.environ.get('P', '8')), torch.float64
  else:
    n, P, dt = int(os.environ.get('N', '64')), int(
        os.environ.get('P', '8')), torch.float64
  pm = unit_cube_mesh(n, ndim=3)
  x = pm.node_coords.copy()
  if case == 'aniso':
    x = x * np.array([1.0, 1.0, 0.125])
  if case == 'jitter':
    x = x + 0.1 / n * np.random.default_rng(0).uniform(-1, 1, x.shape)
  rp = refine_premesh(pm.replace(node_coords=x),
                      Nodes1D.create(P, NodeType.GAUSS_LOBATTO_LEGENDRE))
  return rp.finalize(device=dev, dtype=dt), dt


def timed(fn, k):
  fn()
  torch.cuda.synchronize()
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(
      enable_timing=True)
  a.record()
  for _ in range(k):
    fn()
  b.record()
  torch.cuda.synchronize()
  return a.elapsed_time(b) / k


def breakdown(M):
  """ms of each piece of one V-cycle, level by level (run alone)."""
  out = []
  s = 8 if M.dtype == torch.float64 else 4
  for l, lev in enumerate(M.levels):
    N = lev.mesh.num_nodes
    row = {'order': lev.mesh.order, 'N': N}
    if l == len(M.levels) - 1:
      row['coarse_steps'] = M.coarse_steps
      row['coarse_ms'] = timed(lambda: M._cycle(l, lev.b), reps)
      out.append(row)
      continue
    row['lambda_max'] = lev.lam_max
    row['apply_ms'] = timed(lambda: lev.apply(lev.x, lev.ax), reps)
    row['cheb_step_ms'] = timed(lambda: _ops.cheb_step(
        lev.x, lev.d, lev.ax, lev.b, lev.dinv, None, 0.1, 0.1, 0), reps)
    row['cheb_step_GBps'] = 7 * N * s / row['cheb_step_ms'] / 1e6
    t = lev.transfer
    nxt = M.levels[l + 1]
    E = lev.mesh.num_elements
    nc_loc, nf_loc = t['pc'] ** lev.mesh.ndim, t['pf'] ** lev.mesh.ndim
    owner_b = t['owner'].numel() * 4
    pro_bytes = (nxt.mesh.num_nodes * s + E * nc_loc * 4 + owner_b +
                 N * 4 + 2 * N * s)            # add: reads and writes u_f
    res_bytes = (N * s + N * 4 + owner_b + E * nc_loc * (4 + s))
    row['prolong_add_ms'] = timed(lambda: M.prolong(l, nxt.x, lev.x, True),
                                  reps)
    row['prolong_bytes'] = pro_bytes
    row['prolong_GBps'] = pro_bytes / row['prolong_add_ms'] / 1e6
    row['restrict_ms'] = timed(lambda: _ops.pmg_restrict(
        lev.r, t['local'], t['cidx'], t['fidx'], t['owner'], t['mat'],
        lev.mesh.ndim, t['pc'], t['pf']), reps)
    row['restrict_bytes'] = res_bytes
    row['restrict_GBps'] = res_bytes / row['restrict_ms'] / 1e6
    row['scatter_csr_ms'] = timed(lambda: _ops.scatter_csr(
        t['local'], t['offsets'], t['slots'], nxt.mesh.num_nodes,
        out=nxt.b), reps)
    out.append(row)
  return out


T0 = time.perf_counter()


def log(msg):
  print(f'[{time.perf_counter() - T0:8.1f} s] {msg}', file=sys.stderr,
        flush=True)


def emit(rec):
  line = json.dumps(rec)
  print(line, flush=True)
  if out_path:
    with open(out_path, 'a') as f:
      f.write(line + '\n')


for case in os.environ.get('CASES', 'uniform,jitter,aniso,p11').split(','):
  log(f'{case}: mesh')
  mesh, dt = build(case)
  log(f'{case}: operator')
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create_from_nodes_1d(
      mesh.gridpoints_1d))
  op = operators.HelmholtzOperator.create(fes, mesh.physical_masks['boundary'])
  A = op.linear_operator(0.0, 1.0)
  g = torch.Generator(device=dev).manual_seed(0)
  rhs = op.apply(torch.rand(mesh.num_nodes, dtype=dt, device=dev,
                            generator=g), 1.0, 0.0)
  torch.cuda.synchronize()
  log(f'{case}: p-multigrid setup')
  t0 = time.perf_counter()
  M = PMultigridPreconditioner(op, 0.0, 1.0, smoother_degree=degree)
  torch.cuda.synchronize()
  rec = {'case': case, 'N': mesh.num_nodes, 'E': mesh.num_elements,
         'P': mesh.order + 1, 'dtype': str(dt), 'orders': M.orders,
         'smoother_degree': degree,
         'smoother_interval': [pmg.SMOOTHER_LOW, pmg.SMOOTHER_HIGH],
         'coarse_steps': M.coarse_steps,
         'pmg_setup_ms': round(1e3 * (time.perf_counter() - t0), 1),
         'geometry_per_level': [
             [getattr(l.op, 'num_affine', None),
              getattr(l.op, 'num_multilinear', None),
              getattr(l.op, 'num_curved', None)] for l in M.levels]}
  J = JacobiPreconditioner(op, 0.0, 1.0)
  for name, MM in (('plain', None), ('jacobi', J), ('pmg', M)):
    log(f'{case}: {name}')
    run = CGRunner(A, rhs, M=MM, tol=1e-30, maxiter=10 ** 6)
    rec[f'ms_per_iter_{name}'] = round(timed(run.step, reps), 4)
    del run
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x, info = cg(A, rhs, tol=tol, M=MM, maxiter=maxiter)
    torch.cuda.synchronize()
    rec[f'solve_ms_{name}'] = round(1e3 * (time.perf_counter() - t0), 2)
    rec[f'iters_{name}'] = info['num_iterations']
    rec[f'status_{name}'] = info['status']
    rel = float((rhs.double() - op.apply(x, 0.0, 1.0).double()).norm() /
                rhs.double().norm())
    rec[f'true_rel_residual_{name}'] = rel
    del x
  if probe_tol is not None:
    log(f'{case}: probe')
    x, info = cg(A, rhs, tol=float(probe_tol), M=M, maxiter=100)
    rec['probe'] = {'tol': float(probe_tol), 'iters': info['num_iterations'],
                    'status': info['status'], 'true_rel_residual': float(
                        (rhs.double() - op.apply(x, 0.0, 1.0).double()).norm()
                        / rhs.double().norm())}
    del x
  log(f'{case}: breakdown')
  rec['levels'] = breakdown(M)
  rec['tol'] = tol
  rec['maxiter'] = maxiter
  rec['switches'] = switches.active()
  emit(rec)
  del op, fes, mesh, M, J, A, rhs
  torch.cuda.empty_cache()
