"""Cost of the Robin term, one JSON line per measurement.

* `apply`: the facet mass apply (`sfem_boundary_mass_apply`) and the row add
  (`sfem_boundary_add_rows`), each alone and together, for Robin on all six
  faces of the N^3 box at order P (default 64^3, p = 7, fp64: 24 576
  facets), with the bytes they must move;
* `cg`: time per CG iteration of the operator `solve_helmholtz` builds
  (Gauss rule of P + 2 points: the two-grid operator), without and with that
  Robin term (lambda0 = 1, lambda1 = 1);
* `pmg`: `solve_helmholtz` iterations with and without preconditioners on a
  jittered SMALL_N^3 box (default 24^3, p = 7), lambda0 = 0: Dirichlet on
  all sides, Dirichlet on x0 with Robin on the other five sides, pure Robin.
env: N (64), P (7), SMALL_N (24), REPS (50), TOL (1e-8), OUT (append here
too), PARTS (apply,cg,pmg)."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from swirl_fem_amd import _ops
from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType, Quadrature1D
from swirl_fem_amd.core.mesh_refiner import refine_premesh
from swirl_fem_amd.examples.helmholtz import BCType, solve_helmholtz
from swirl_fem_amd.linalg.cg import CGRunner

N = int(os.environ.get('N', '64'))
P = int(os.environ.get('P', '7'))
SMALL_N = int(os.environ.get('SMALL_N', '24'))
reps = int(os.environ.get('REPS', '50'))
tol = float(os.environ.get('TOL', '1e-8'))
parts = os.environ.get('PARTS', 'apply,cg,pmg').split(',')
out_path = os.environ.get('OUT')
dev = torch.device('cuda:0')
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


def side_groups(pm):
  """One physical group per side of the unit box (x0, x1, y0, ...): the
  element faces of the order-1 premesh that lie on it."""
  corners = np.array(np.meshgrid(*([[0, 1]] * 3), indexing='ij')).reshape(
      3, -1).T
  x = np.asarray(pm.node_coords)
  groups = {}
  for a in range(3):
    for s in (0, 1):
      face = np.asarray(pm.elements)[:, corners[:, a] == s]   # (E, 4)
      on = np.all(np.abs(x[face][..., a] - s) < 1e-9, axis=1)
      groups['xyz'[a] + str(s)] = face[on].astype(np.int32)
  return groups


def box(n, jitter=0.0):
  pm = unit_cube_mesh(n, ndim=3)
  groups = side_groups(pm)
  groups['boundary'] = np.concatenate([groups[s] for s in SIDES])
  pm = pm.replace(physical_groups=groups)
  if jitter:
    x = pm.node_coords.copy()
    inner = np.all((x > 1e-9) & (x < 1 - 1e-9), axis=1)
    x[inner] += jitter / n * np.random.default_rng(0).uniform(
        -1, 1, x[inner].shape)
    pm = pm.replace(node_coords=x)
  rp = refine_premesh(pm, Nodes1D.create(P + 1, NodeType.GAUSS_LOBATTO_LEGENDRE))
  return rp.finalize(device=dev, dtype=torch.float64)


SIDES = ['x0', 'x1', 'y0', 'y1', 'z0', 'z1']

if 'apply' in parts or 'cg' in parts:
  log(f'{N}^3 box, p = {P}')
  mesh = box(N)
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(
      P + 2, NodeType.GAUSS_LEGENDRE))
  robin = [fes.boundary_mass(g, 1.0) for g in SIDES]
  F = sum(r.facets.shape[0] for r in robin)
  g = torch.Generator(device=dev).manual_seed(0)
  u = torch.rand(mesh.num_nodes, dtype=torch.float64, device=dev,
                 generator=g)
  out = torch.zeros_like(u)
  torch.cuda.synchronize()

if 'apply' in parts:
  s = 8
  rec = {'part': 'apply', 'N': mesh.num_nodes, 'E': mesh.num_elements,
         'P': P, 'dtype': 'float64', 'facets': F,
         'group_nodes': int(sum(r.rows.numel() for r in robin))}
  n, q = (P + 1) ** 2, (P + 2) ** 2
  # per facet: n ids (4 B) + n gathered values, q aw, n results written
  rec['mass_bytes'] = F * (n * 4 + n * s + q * s + n * s)
  # per row: offsets (8 B) + row id + its slots (4 B) + local values + r/w
  rows = sum(r.rows.numel() for r in robin)
  rec['add_rows_bytes'] = rows * (8 + 4 + 2 * s) + F * n * (4 + s)
  rec['mass_us'] = 1e3 * sum(timed(lambda r=r: _ops.boundary_mass(
      u, r.encoded, r.aw, r.bmat, 3, 1.0, out=r._local), reps) for r in robin)
  rec['add_rows_us'] = 1e3 * sum(timed(lambda r=r: _ops.boundary_add_rows(
      r._local, r.rows, r.offsets, r.slots, out), reps) for r in robin)

  def all_sides():
    for r in robin:
      r.apply(u, 1.0, out=out)
  rec['robin_apply_us'] = 1e3 * timed(all_sides, reps)
  # one group holding all six sides: two launches in all
  one = fes.boundary_mass('boundary', 1.0)
  rec['robin_apply_one_group_us'] = 1e3 * timed(
      lambda: one.apply(u, 1.0, out=out), reps)
  rec['mass_GBps'] = rec['mass_bytes'] / rec['mass_us'] / 1e3
  rec['add_rows_GBps'] = rec['add_rows_bytes'] / rec['add_rows_us'] / 1e3
  log('apply done')
  emit(rec)

if 'cg' in parts:
  op = fes.helmholtz_operator(None)
  one = fes.boundary_mass('boundary', 1.0)
  rhs = op.apply(u, 1.0, 0.0)
  rec = {'part': 'cg', 'N': mesh.num_nodes, 'P': P, 'dtype': 'float64',
         'operator': type(op).__name__, 'facets': F}
  rec['operator_ms'] = timed(lambda: op.apply(u, 1.0, 1.0), reps)
  rec['operator_robin_ms'] = timed(
      lambda: one.apply(u, 1.0, out=op.apply(u, 1.0, 1.0)), reps)
  for name, A in (('plain', lambda v: op.apply(v, 1.0, 1.0)),
                  ('robin', lambda v: one.apply(v, 1.0,
                                                out=op.apply(v, 1.0, 1.0)))):
    run = CGRunner(A, rhs, tol=1e-30, maxiter=10 ** 6)
    rec[f'ms_per_iter_{name}'] = timed(run.step, reps)
    del run
  rec['robin_share'] = (rec['ms_per_iter_robin'] / rec['ms_per_iter_plain']
                        - 1.0)
  log('cg done')
  emit(rec)
  del op, one, rhs

if 'apply' in parts or 'cg' in parts:
  del mesh, fes, robin, u, out
  torch.cuda.empty_cache()

if 'pmg' in parts:
  log(f'pmg: {SMALL_N}^3 jittered box, p = {P}')
  mesh = box(SMALL_N, jitter=0.1)
  x = mesh.node_coords
  f = torch.sin(3 * x[:, 0]) + x[:, 1] * x[:, 2]
  gfun = lambda y: torch.cos(2 * y[:, 0]) + y[:, 1]
  cases = {
      'dirichlet': {s: (BCType.DIRICHLET, 0.0) for s in SIDES},
      'robin': dict({s: (BCType.ROBIN, (1.0, gfun)) for s in SIDES[1:]},
                    x0=(BCType.DIRICHLET, 0.0)),
      'pure_robin': {s: (BCType.ROBIN, (1.0, gfun)) for s in SIDES}}
  for name, bcs in cases.items():
    rec = {'part': 'pmg', 'case': name, 'N': mesh.num_nodes,
           'E': mesh.num_elements, 'P': P, 'lambda0': 0.0, 'tol': tol}
    for pc in (None, 'jacobi', 'pmg'):
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      _, info = solve_helmholtz(mesh, f, bcs, lambda0=0.0, rtol=tol,
                                return_info=True, preconditioner=pc)
      torch.cuda.synchronize()
      key = pc or 'plain'
      rec[f'iters_{key}'] = info['num_iterations']
      rec[f'status_{key}'] = info['status']
      rec[f'solve_s_{key}'] = round(time.perf_counter() - t0, 2)
      log(f'{name} {key}: {info["num_iterations"]} iterations')
    emit(rec)
