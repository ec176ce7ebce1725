"""Cost of the elasticity sensitivity kernel and of one backward pass (DESIGN
§3.17), one JSON line per configuration (profiles/elasticity_adjoint.jsonl, or
OUT, is rewritten).

Size: that of `scripts/time_elasticity.py`: N^3 hex elements of order P,
affine box (default 32^3, p = 7), fp64 and fp32; the solve's Gauss rule, Q = P
+ 2 points per direction.  Per dtype, in one process:

* `sens`: `sfem_elasticity_sens` alone on the Q^3 grid with all three outputs
  ('all'), `dmu` alone ('dmu') and `drho` alone ('drho', no derivative stage),
  next to `sfem_elasticity_local` on the same arrays ('forward', scalar
  coefficients, lambda0 = 1 so that it reads what 'all' reads).
  `bytes_model`: what each must move -- 'all': two fields of d reals per point
  in, `wdet`, three outputs; 'dmu': the fields, `wdet`, one output; 'drho'
  likewise; 'forward': d in, d out, `wdet`.  `hbm_fraction`: that over the
  time, against 8 TB/s.  `ratio_to_forward`: ms / forward ms.
* `backward`: one `solve_elasticity` with a per-element lame_mu that requires
  grad and its `.backward()`, at NS^3 elements (default 8^3) of the same
  order, fp64 only (rtol 1e-8 is below what fp32 CG reaches), clamped on the
  whole boundary under its own weight, Jacobi, rtol 1e-8: iterations of the
  forward and of the adjoint solve and wall clock of each with
  synchronisation (the median of ROUNDS runs after one warm-up run).
Variants alternate; ROUNDS rounds of REPS calls after a warm-up, HIP events,
the median round counts and every round is kept.
env: N (32), NS (8), P (7), REPS (5), ROUNDS (5), OUT, DTYPES (fp64,fp32)."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from swirl_fem_amd import _ops
from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType, Quadrature1D
from swirl_fem_amd.core.mesh_refiner import refine_premesh
from swirl_fem_amd.examples.elasticity import BCType, solve_elasticity

N = int(os.environ.get('N', '32'))
NS = int(os.environ.get('NS', '8'))
P = int(os.environ.get('P', '7'))
reps = int(os.environ.get('REPS', '5'))
rounds = int(os.environ.get('ROUNDS', '5'))
dtypes = os.environ.get('DTYPES', 'fp64,fp32').split(',')
out_path = os.environ.get('OUT', os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
    'elasticity_adjoint.jsonl'))
if out_path:
  open(out_path, 'w').close()     # a run replaces the file
dev = torch.device('cuda:0')
HBM = 8e12
LAM, MU = 1.3, 0.6
GLL, GL = NodeType.GAUSS_LOBATTO_LEGENDRE, NodeType.GAUSS_LEGENDRE


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


def alternate(fns):
  """{name: median ms}, {name: rounds} of the variants run in turn."""
  for fn in fns.values():
    for _ in range(2):
      fn()
  torch.cuda.synchronize()
  times = {k: [] for k in fns}
  for _ in range(rounds):
    for k, fn in fns.items():
      times[k].append(timed(fn, reps))
  return {k: float(np.median(v)) for k, v in times.items()}, times


def rnd(v):
  return [round(t, 4) for t in v]


d = 3
rp = refine_premesh(unit_cube_mesh(N, ndim=d), Nodes1D.create(P + 1, GLL))
rps = refine_premesh(unit_cube_mesh(NS, ndim=d), Nodes1D.create(P + 1, GLL))
for name in dtypes:
  dt = {'fp64': torch.float64, 'fp32': torch.float32}[name]
  size = 8 if name == 'fp64' else 4
  mesh = rp.finalize(device=dev, dtype=dt)
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(
      P + (d + 1) // 2, GL))
  op = fes.elasticity_operator(lame_lambda=LAM, lame_mu=MU)
  assert [p['geo_mode'] for p in op.parts] == [1], 'expected an affine box'
  E, Q = mesh.num_elements, fes.quadrature.num_points
  nq = Q ** d
  base = {'N': N, 'p': P, 'Q': Q, 'dtype': name, 'elements': E}
  uq = torch.randn((E, nq, d), dtype=dt, device=dev)
  vq = torch.randn((E, nq, d), dtype=dt, device=dev)
  wd = op.point_weights()
  sens = lambda want: (lambda: _ops.elasticity_sens(
      uq, vq, op.parts, op.host, d, Q, wd, 1.0, want=want))
  fns = {'all': sens((True, True, True)), 'dmu': sens((False, True, False)),
         'drho': sens((False, False, True)),
         'forward': lambda: _ops.elasticity_local(
             uq, op.parts, op.host, d, Q, wd, LAM, MU, None, 1.0)}
  reals = {'all': 2 * d + 1 + 3, 'dmu': 2 * d + 1 + 1, 'drho': 2 * d + 1 + 1,
           'forward': 2 * d + 1}
  ms, times = alternate(fns)
  for k in fns:
    nb = size * E * nq * reals[k]
    emit(dict(base, part='sens', variant=k, ms=round(ms[k], 4),
              ms_rounds=rnd(times[k]), bytes_model=nb,
              hbm_fraction=round(nb / (ms[k] * 1e-3) / HBM, 4),
              ratio_to_forward=round(ms[k] / ms['forward'], 4)))
  del uq, vq, op, fes, mesh, wd, fns
  torch.cuda.empty_cache()
  if name != 'fp64':
    continue

  mesh = rps.finalize(device=dev, dtype=dt)
  bcs = {'boundary': (BCType.DIRICHLET, (0.0, 0.0, 0.0))}
  fw, bw, its = [], [], None
  for r in range(rounds + 1):
    mu = torch.full((mesh.num_elements,), MU, dtype=dt, device=dev,
                    requires_grad=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    u, info = solve_elasticity(mesh, (0.0, 0.0, -1.0), bcs, lame_lambda=LAM,
                               lame_mu=mu, rtol=1e-8, preconditioner='jacobi',
                               return_info=True)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    u[:, 2].sum().backward()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    if r:                          # the first run warms up
      fw.append(1e3 * (t1 - t0))
      bw.append(1e3 * (t2 - t1))
    its = (int(info['num_iterations']),
           int(info['adjoint']['num_iterations']))
    assert mu.grad is not None and bool(torch.isfinite(mu.grad).all())
  emit(dict(N=NS, p=P, dtype=name, elements=mesh.num_elements,
            nodes=mesh.num_nodes, part='backward', forward_iterations=its[0],
            adjoint_iterations=its[1], forward_ms=round(float(np.median(fw)), 3),
            backward_ms=round(float(np.median(bw)), 3), forward_ms_rounds=rnd(fw),
            backward_ms_rounds=rnd(bw),
            backward_over_forward=round(float(np.median(bw) / np.median(fw)),
                                        4)))
  del mesh
  torch.cuda.empty_cache()
