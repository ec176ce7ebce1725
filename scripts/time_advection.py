"""Cost of the advective term, one JSON line per measurement
(appended to profiles/advection.jsonl, or OUT).

* `apply`: time per apply at N^3, order P, fp64 (default 32^3, p = 7) of the
  collocated index-row operator (facet tables off) without and with a
  velocity (`beta`: ndim more reals per point); the variants alternate, ROUNDS
  rounds of REPS applies after a warm-up, HIP events, the median round counts.
  `hbm_fraction`: `bytes_per_apply` over the time, against 8 TB/s.
* `iteration`: one BiCGStab iteration of the operator with the velocity
  against one CG iteration of its symmetric part (same index-row operator, no
  velocity), lambda0 = 1, no preconditioner, ITERS iterations per round.
env: N (32), P (7), REPS (20), ROUNDS (5), ITERS (20), OUT, PARTS
(apply,iteration)."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType, Quadrature1D
from swirl_fem_amd.core.mesh_refiner import refine_premesh
from swirl_fem_amd.linalg.bicgstab import BiCGStabRunner
from swirl_fem_amd.linalg.cg import CGRunner

N = int(os.environ.get('N', '32'))
P = int(os.environ.get('P', '7'))
reps = int(os.environ.get('REPS', '20'))
rounds = int(os.environ.get('ROUNDS', '5'))
iters = int(os.environ.get('ITERS', '20'))
parts = os.environ.get('PARTS', 'apply,iteration').split(',')
out_path = os.environ.get('OUT', os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
    'advection.jsonl'))
dev = torch.device('cuda:0')
HBM = 8e12
GLL = NodeType.GAUSS_LOBATTO_LEGENDRE


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


pm = unit_cube_mesh(N, ndim=3)
mesh = refine_premesh(pm, Nodes1D.create(P + 1, GLL)).finalize(
    device=dev, dtype=torch.float64)
fes = FiniteElementSpace.create(mesh, Quadrature1D.create(P + 1, GLL))
vel = lambda x: torch.stack([1.0 + x[:, 1], 0.5 - x[:, 0],
                             0.3 + 0.0 * x[:, 2]], dim=-1)
saved = os.environ.get('SFEM_FACET')
os.environ['SFEM_FACET'] = '0'              # index rows for both variants
try:
  ops = {'none': fes.helmholtz_operator(None, assembly='atomic'),
         'velocity': fes.helmholtz_operator(None, velocity=vel)}
finally:
  if saved is None:
    del os.environ['SFEM_FACET']
  else:
    os.environ['SFEM_FACET'] = saved
assert ops['none'].facet_parts is None
u = torch.randn(mesh.num_nodes, dtype=torch.float64, device=dev)

if 'apply' in parts:
  outs = {k: torch.empty_like(u) for k in ops}
  fns = {k: (lambda op=op, o=outs[k]: op.apply(u, 1.0, 1.0, out=o))
         for k, op in ops.items()}
  for fn in fns.values():
    for _ in range(3):
      fn()
  torch.cuda.synchronize()
  times = {k: [] for k in ops}
  for _ in range(rounds):
    for k, fn in fns.items():
      times[k].append(timed(fn, reps))
  ms = {k: float(np.median(v)) for k, v in times.items()}
  for k, op in ops.items():
    nb = op.bytes_per_apply(1.0)
    emit({'part': 'apply', 'variant': k, 'N': N, 'p': P, 'dtype': 'fp64',
          'lambda0': 1.0, 'ms': round(ms[k], 4),
          'ms_rounds': [round(t, 4) for t in times[k]],
          'kernel': op.kernel_name(1.0, 1.0), 'bytes_per_apply': nb,
          'hbm_fraction': round(nb / (ms[k] * 1e-3) / HBM, 4),
          'ratio_to_none': round(ms[k] / ms['none'], 4)})

if 'iteration' in parts:
  b = ops['none'].apply(u, 1.0, 0.0)
  mk = {'cg': lambda: CGRunner(ops['none'].linear_operator(1.0, 1.0), b,
                               tol=0.0, maxiter=10 ** 9),
        'bicgstab': lambda: BiCGStabRunner(
            ops['velocity'].linear_operator(1.0, 1.0), b, tol=0.0,
            maxiter=10 ** 9)}
  times = {k: [] for k in mk}
  for k, make in mk.items():
    run = make()
    for _ in range(3):
      run.step()
    torch.cuda.synchronize()
    for _ in range(rounds):
      times[k].append(timed(run.step, iters))
  ms = {k: float(np.median(v)) for k, v in times.items()}
  for k in mk:
    emit({'part': 'iteration', 'solver': k, 'N': N, 'p': P, 'dtype': 'fp64',
          'ms_per_iteration': round(ms[k], 4),
          'ms_rounds': [round(t, 4) for t in times[k]],
          'ratio_to_cg': round(ms[k] / ms['cg'], 4)})
