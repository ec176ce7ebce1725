"""Cost of variable coefficients, one JSON line per measurement
(appended to profiles/coefficients.jsonl, or OUT).

* `apply`: time per apply at N^3, order P, fp64 (default 64^3, p = 7) of the
  collocated index-row operator (facet tables off) without a coefficient,
  with a per-element diffusivity (COEF_ELEM) and a per-point one
  (COEF_POINT), and of the two-grid operator on the Gauss rule of
  `solve_helmholtz` (P + 2 points) without and with a per-point diffusivity;
  the variants alternate, ROUNDS rounds of REPS applies, the median round
  counts.  `hbm_fraction`: `bytes_per_apply` over the time, against 8 TB/s
  (collocated operators only: the two-grid one has no byte model).
* `pmg`: `solve_helmholtz` with p-multigrid and with Jacobi on the
  two-material problem of tests/test_gpu_coefficients.py (SMALL_N^3, y / z
  jittered, default 16^3, p = 7: k = 1 for x < 1/2, k = contrast beyond,
  u = 0 at x = 0, u = 1 at x = 1), contrasts 1, 1e2, 1e4: iterations and
  solve time.
env: N (64), P (7), SMALL_N (16), REPS (20), ROUNDS (5), TOL (1e-10), OUT,
PARTS (apply,pmg)."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from swirl_fem_amd import switches
from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType, Quadrature1D
from swirl_fem_amd.core.mesh_refiner import refine_premesh
from swirl_fem_amd.examples.helmholtz import BCType, solve_helmholtz

N = int(os.environ.get('N', '64'))
P = int(os.environ.get('P', '7'))
SMALL_N = int(os.environ.get('SMALL_N', '16'))
reps = int(os.environ.get('REPS', '20'))
rounds = int(os.environ.get('ROUNDS', '5'))
tol = float(os.environ.get('TOL', '1e-10'))
parts = os.environ.get('PARTS', 'apply,pmg').split(',')
out_path = os.environ.get('OUT', os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
    'coefficients.jsonl'))
dev = torch.device('cuda:0')
HBM = 8e12
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
  """ms per call of k back-to-back calls."""
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(
      enable_timing=True)
  a.record()
  for _ in range(k):
    fn()
  b.record()
  torch.cuda.synchronize()
  return a.elapsed_time(b) / k


def sides(pm, ndim=3):
  names = ['x', 'y', 'z']

  def classify(c):
    for a in range(ndim):
      if abs(c[a]) < 1e-9:
        return names[a] + '0'
      if abs(c[a] - 1) < 1e-9:
        return names[a] + '1'
    return None
  from tests import bvp_reference as BR
  return BR.boundary_groups(pm, classify)


def box(n, jitter_yz=0.0, groups=False):
  pm = unit_cube_mesh(n, ndim=3)
  if groups:
    pm = pm.replace(physical_groups=sides(pm))
  if jitter_yz:
    x = pm.node_coords.copy()
    inner = np.all((x[:, 1:] > 1e-9) & (x[:, 1:] < 1 - 1e-9), axis=1)
    x[inner, 1:] += jitter_yz / n * np.random.default_rng(5).uniform(
        -1, 1, x[inner, 1:].shape)
    pm = pm.replace(node_coords=x)
  rp = refine_premesh(pm, Nodes1D.create(P + 1,
                                         NodeType.GAUSS_LOBATTO_LEGENDRE))
  return rp.finalize(device=dev, dtype=torch.float64)


def apply_part():
  log(f'apply: {N}^3, p = {P}, fp64')
  mesh = box(N)
  E = mesh.num_elements
  fes = FiniteElementSpace.create(
      mesh, Quadrature1D.create(P + 1, NodeType.GAUSS_LOBATTO_LEGENDRE))
  kf = lambda x: 1.0 + x[:, 0] ** 2 + 0.5 * torch.sin(3.0 * x[:, 1])
  ke = 0.5 + torch.rand(E, dtype=torch.float64, device=dev)
  saved = os.environ.get('SFEM_FACET')
  os.environ['SFEM_FACET'] = '0'            # index rows for every variant
  try:
    ops = {'none': fes.helmholtz_operator(None, assembly='atomic'),
           'elem': fes.helmholtz_operator(None, diffusivity=ke),
           'point': fes.helmholtz_operator(None, diffusivity=kf)}
  finally:
    if saved is None:
      del os.environ['SFEM_FACET']
    else:
      os.environ['SFEM_FACET'] = saved
  assert ops['none'].facet_parts is None
  gfes = FiniteElementSpace.create(
      mesh, Quadrature1D.create(P + 2, NodeType.GAUSS_LEGENDRE))
  ops['two_grid_none'] = gfes.helmholtz_operator(None)
  ops['two_grid_point'] = gfes.helmholtz_operator(None, diffusivity=kf)
  u = torch.randn(mesh.num_nodes, dtype=torch.float64, device=dev)
  outs = {k: torch.empty_like(u) for k in ops}
  fns = {}
  for k, op in ops.items():
    if k.startswith('two_grid'):
      fns[k] = (lambda op=op: op.apply(u, 0.0, 1.0))
    else:
      fns[k] = (lambda op=op, o=outs[k]: op.apply(u, 0.0, 1.0, out=o))
  for fn in fns.values():
    fn()
  torch.cuda.synchronize()
  times = {k: [] for k in ops}
  for _ in range(rounds):
    for k, fn in fns.items():
      times[k].append(timed(fn, reps))
  for k, op in ops.items():
    ms = float(np.median(times[k]))
    rec = {'part': 'apply', 'variant': k, 'N': N, 'p': P, 'dtype': 'fp64',
           'lambda0': 0.0, 'ms': round(ms, 4),
           'ms_rounds': [round(t, 4) for t in times[k]],
           'kernel': (op.kernel_name(0.0, 1.0) if hasattr(op, 'kernel_name')
                      else 'basis_eval + helmholtz_kernel(local) + '
                           'basis_eval_t')}
    if hasattr(op, 'bytes_per_apply'):
      nb = op.bytes_per_apply(0.0)
      rec.update(bytes_per_apply=nb,
                 hbm_fraction=round(nb / (ms * 1e-3) / HBM, 4))
    emit(rec)
    log(f'{k}: {ms:.3f} ms')


def pmg_part():
  log(f'pmg: {SMALL_N}^3 y/z-jittered box, p = {P}')
  mesh = box(SMALL_N, jitter_yz=0.2, groups=True)
  centre = mesh.element_coords()[..., 0].mean(dim=1)
  f = torch.zeros(mesh.num_nodes, dtype=torch.float64, device=dev)
  bcs = {'x0': (BCType.DIRICHLET, 0.0), 'x1': (BCType.DIRICHLET, 1.0)}
  for contrast in (1.0, 1e2, 1e4):
    k = torch.where(centre < 0.5, torch.ones_like(centre),
                    torch.full_like(centre, contrast))
    for pc in ('pmg', 'jacobi'):
      solve_helmholtz(mesh, f, bcs, rtol=tol, diffusivity=k,
                      preconditioner=pc)             # warm-up
      torch.cuda.synchronize()
      t = time.perf_counter()
      u, info = solve_helmholtz(mesh, f, bcs, rtol=tol, diffusivity=k,
                                preconditioner=pc, return_info=True)
      torch.cuda.synchronize()
      s = time.perf_counter() - t
      x = mesh.node_coords[:, 0]
      s1, s2 = 2 * contrast / (1 + contrast), 2 / (1 + contrast)
      exact = torch.where(x < 0.5, s1 * x, s1 * 0.5 + s2 * (x - 0.5))
      rec = {'part': 'pmg', 'preconditioner': pc, 'N': SMALL_N, 'p': P,
             'contrast': contrast, 'rtol': tol,
             'iterations': int(info['num_iterations']),
             'solve_s_with_setup': round(s, 3),
             'max_error': float((u - exact).abs().max())}
      emit(rec)
      log(f'contrast {contrast:g} {pc}: {rec["iterations"]} iterations, '
          f'{s:.2f} s')


if 'apply' in parts:
  apply_part()
if 'pmg' in parts:
  pmg_part()
