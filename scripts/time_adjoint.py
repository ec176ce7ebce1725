"""Cost of the adjoint side of the Helmholtz family, one JSON
line per measurement (appended to profiles/adjoint.jsonl, or OUT).

* `apply`: forward and transposed apply of the collocated index-row operator
  with a velocity at N^3, order P, fp64 (default 32^3, p = 7, affine box);
  the variants alternate, ROUNDS rounds of REPS applies after a warm-up, HIP
  events, the median round counts; `spread` = (max - min) / median over the
  rounds of the forward apply.  Run once per library (SFEM_LIB, LABEL) to
  compare builds.
* `sens`: the sensitivity kernel with all outputs and with dkappa alone; its
  must-move bytes are 2 s n in, (2 + DIM) s n (or s n) out per element plus
  the geometry as in `bytes_per_apply`; `hbm_fraction` against 8 TB/s.
* `backward`: one forward `solve_helmholtz` with a velocity and a per-point
  diffusivity (Jacobi, rtol 1e-8) and its `backward()`: iteration counts and
  wall times with a device synchronisation.
env: N (32), P (7), REPS (20), ROUNDS (5), OUT, LABEL, PARTS
(apply,sens,backward), NS (8: elements per side of the solve)."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from swirl_fem_amd import _ops
from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType, Quadrature1D
from swirl_fem_amd.core.mesh_refiner import refine_premesh

N = int(os.environ.get('N', '32'))
P = int(os.environ.get('P', '7'))
reps = int(os.environ.get('REPS', '20'))
rounds = int(os.environ.get('ROUNDS', '5'))
label = os.environ.get('LABEL', 'this')
parts = os.environ.get('PARTS', 'apply,sens,backward').split(',')
out_path = os.environ.get('OUT', os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
    'adjoint.jsonl'))
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


def alternate(fns):
  for fn in fns.values():
    for _ in range(3):
      fn()
  torch.cuda.synchronize()
  times = {k: [] for k in fns}
  for _ in range(rounds):
    for k, fn in fns.items():
      times[k].append(timed(fn, reps))
  return times


vel = lambda x: torch.stack([1.0 + x[:, 1], 0.5 - x[:, 0],
                             0.3 + 0.0 * x[:, 2]], dim=-1)
base = {'N': N, 'p': P, 'dtype': 'fp64', 'label': label}

if 'apply' in parts or 'sens' in parts:
  pm = unit_cube_mesh(N, ndim=3)
  mesh = refine_premesh(pm, Nodes1D.create(P + 1, GLL)).finalize(
      device=dev, dtype=torch.float64)
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(P + 1, GLL))
  op = fes.helmholtz_operator(None, velocity=vel)
  u = torch.randn(mesh.num_nodes, dtype=torch.float64, device=dev)

if 'apply' in parts:
  fns = {'forward': lambda o=torch.empty_like(u): op.apply(u, 1.0, 1.0, out=o)}
  if hasattr(op, 'apply_transpose'):
    fns['transpose'] = lambda o=torch.empty_like(u): op.apply_transpose(
        u, 1.0, 1.0, out=o)
  times = alternate(fns)
  ms = {k: float(np.median(v)) for k, v in times.items()}
  nb = op.bytes_per_apply(1.0)
  for k in fns:
    emit(dict(base, part='apply', variant=k, lambda0=1.0,
              ms=round(ms[k], 4), ms_rounds=[round(t, 4) for t in times[k]],
              spread=round((max(times[k]) - min(times[k])) / ms[k], 4),
              bytes_per_apply=nb,
              hbm_fraction=round(nb / (ms[k] * 1e-3) / HBM, 4),
              ratio_to_forward=round(ms[k] / ms['forward'], 4)))

if 'sens' in parts:
  E, n = mesh.num_elements, mesh.num_nodes_per_element
  ul = mesh.gather(u)
  ll = mesh.gather(torch.randn_like(u))
  outs = (torch.empty((E, n), dtype=u.dtype, device=dev),
          torch.empty((E, n), dtype=u.dtype, device=dev),
          torch.empty((E, n, 3), dtype=u.dtype, device=dev))
  run = lambda want: _ops.helmholtz_sens(
      ul, ll, op._geo_parts, op.host, 3, P + 1, 1.0, 1.0, want=want,
      out=tuple(o if w else None for o, w in zip(outs, want)))
  variants = {'all': (True, True, True), 'dkappa': (True, False, False)}
  times = alternate({k: (lambda w=w: run(w)) for k, w in variants.items()})
  s = 8
  for k, want in variants.items():
    ms = float(np.median(times[k]))
    words_out = want[0] + want[1] + 3 * want[2]
    # affine box: 24 reals of multilinear coefficients per element
    nb = E * (2 * s * n + words_out * s * n + 24 * s)
    emit(dict(base, part='sens', variant=k, ms=round(ms, 4),
              ms_rounds=[round(t, 4) for t in times[k]], bytes=nb,
              hbm_fraction=round(nb / (ms * 1e-3) / HBM, 4)))

if 'backward' in parts:
  from swirl_fem_amd.examples.helmholtz import BCType, solve_helmholtz
  NS = int(os.environ.get('NS', '8'))
  pm = unit_cube_mesh(NS, ndim=3)
  smesh = refine_premesh(pm, Nodes1D.create(P + 1, GLL)).finalize(
      device=dev, dtype=torch.float64)
  f = torch.randn(smesh.num_nodes, dtype=torch.float64, device=dev)
  w = torch.randn_like(f)
  q = P + 2                                        # the solve's Gauss rule
  k = (1.0 + torch.rand((smesh.num_elements, q ** 3), dtype=torch.float64,
                        device=dev)).requires_grad_(True)
  bcs = {'boundary': (BCType.DIRICHLET, 0.0)}
  for trial in range(2):                           # the first warms up
    torch.cuda.synchronize(); t0 = time.perf_counter()
    uu, info = solve_helmholtz(smesh, f, bcs, lambda0=1.0, rtol=1e-8,
                               return_info=True, preconditioner='jacobi',
                               diffusivity=k, velocity=vel)
    torch.cuda.synchronize(); t1 = time.perf_counter()
    node = uu.grad_fn
    (uu * w).sum().backward()
    torch.cuda.synchronize(); t2 = time.perf_counter()
  emit(dict(base, part='backward', elements=NS ** 3,
            nodes=smesh.num_nodes, forward_ms=round((t1 - t0) * 1e3, 2),
            backward_ms=round((t2 - t1) * 1e3, 2),
            forward_iterations=int(info['num_iterations']),
            backward_iterations=int(
                node.state['adjoint_info']['num_iterations'])))
