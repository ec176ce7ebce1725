"""Cost of the scalar-transport right-hand side and step, one
JSON line per measurement (appended to profiles/transport.jsonl, or OUT).

Size: N^3 elements of order P, fp64, affine box (default 32^3, p = 7: the
settings of §3.11); the solve's Gauss rule, Q = P + 2 points per direction.

* `kernel`: `sfem_transport_rhs` alone on the Q^3 grid for 1 / 2 / 3 levels
  (velocity, mass term and `wdet` at every level, no source).
  `bytes_model`: (d + 1) reals per point and level plus `wdet` and the result
  once; `hbm_fraction`: that over the time, against 8 TB/s.
* `rhs`: the assembled right-hand side for 1 / 2 / 3 levels with nodal
  velocities, `TransportRhs.apply` ('fused') against the same vector from
  what the operators offered before it ('beta'): per level `to_quadrature`,
  `fold_velocity`, `sfem_helmholtz_local` with the folded velocity and
  lambda0 = lambda1 = 0, then one transposed interpolation and one mass
  apply.  `rel_diff`: the two vectors, max norm.
* `step`: one `ScalarTransport.step` of order 3 (Dirichlet box, Jacobi,
  rtol = 1e-8) with its CG iteration count.
Variants alternate; ROUNDS rounds of REPS calls after a warm-up, HIP events,
the median round counts and every round is kept.
env: N (32), P (7), REPS (10), ROUNDS (5), OUT, PARTS (kernel,rhs,step)."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from swirl_fem_amd import _ops
from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
from swirl_fem_amd.core import operators
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType
from swirl_fem_amd.core.mesh_refiner import refine_premesh
from swirl_fem_amd.examples.transport import BCType, ScalarTransport

N = int(os.environ.get('N', '32'))
P = int(os.environ.get('P', '7'))
reps = int(os.environ.get('REPS', '10'))
rounds = int(os.environ.get('ROUNDS', '5'))
parts = os.environ.get('PARTS', 'kernel,rhs,step').split(',')
out_path = os.environ.get('OUT', os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
    'transport.jsonl'))
dev = torch.device('cuda:0')
HBM = 8e12
f64 = torch.float64


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


pm = unit_cube_mesh(N, ndim=3)
mesh = refine_premesh(pm, Nodes1D.create(
    P + 1, NodeType.GAUSS_LOBATTO_LEGENDRE)).finalize(device=dev, dtype=f64)
st = ScalarTransport.create(mesh, {'boundary': (BCType.DIRICHLET, 0.0)},
                            diffusivity=0.01)
fes, op = st.fespace, st.rhs_op
E, d = mesh.num_elements, 3
Q = fes.quadrature.num_points
nq = Q ** d
base = {'N': N, 'p': P, 'Q': Q, 'dtype': 'fp64'}
assert [p['geo_mode'] for p in op.parts] == [1], 'expected an affine box'
x = mesh.node_coords
vel = [torch.stack([(1.0 + 0.1 * j) + x[:, 1], 0.5 - x[:, 0],
                    0.3 + 0.0 * x[:, 2]], dim=-1).contiguous()
       for j in range(3)]
Ts = [torch.randn(mesh.num_nodes, dtype=f64, device=dev) for _ in range(3)]
coefs = [(-1.5, 1.0), (2.0, -3.0), (-0.5, 3.0)]

if 'kernel' in parts:
  Tq = [torch.randn((E, nq), dtype=f64, device=dev) for _ in range(3)]
  uq = [torch.randn((E, nq, d), dtype=f64, device=dev) for _ in range(3)]
  wd = op.point_weights()
  fns = {n: (lambda n=n: _ops.transport_rhs(
      [(Tq[j], uq[j]) + coefs[j] for j in range(n)], op.parts, op.host, d, Q,
      wdet=wd)) for n in (1, 2, 3)}
  ms, times = alternate(fns)
  for n in (1, 2, 3):
    nb = 8 * E * nq * ((d + 1) * n + 2)
    emit(dict(base, part='kernel', levels=n, ms=round(ms[n], 4),
              ms_rounds=[round(t, 4) for t in times[n]], bytes_model=nb,
              hbm_fraction=round(nb / (ms[n] * 1e-3) / HBM, 4)))
  del Tq, uq

if 'rhs' in parts:
  plain = fes.helmholtz_operator(None)
  i1, g1 = fes._matrices()
  ones = torch.ones((E, nq), dtype=f64, device=dev)

  def fused(n):
    return op.apply([(Ts[j], vel[j]) + coefs[j] for j in range(n)])

  def beta_route(n):
    acc = None
    for j in range(n):
      beta = operators.fold_velocity(fes, fes.to_quadrature(vel[j]))
      lp = operators._advection_parts(plain.parts, beta, E, nq)
      rq = _ops.helmholtz_local(fes.to_quadrature(Ts[j]).contiguous(), lp,
                                plain.host, d, Q, 0.0, 0.0)
      acc = coefs[j][1] * rq if acc is None else acc + coefs[j][1] * rq
    r3 = _ops.basis_eval_t(acc[..., None], None, i1, g1, None, ones, d, P + 1,
                           Q, 1, False)
    mass = sum(coefs[j][0] * Ts[j] for j in range(n))
    return mesh.scatter(r3[..., 0]) + plain.apply(mass, 1.0, 0.0)
  for n in (1, 2, 3):
    a, b = fused(n), beta_route(n)
    diff = float((a - b).abs().max() / b.abs().max())
    del a, b
    ms, times = alternate({'fused': lambda: fused(n),
                           'beta': lambda: beta_route(n)})
    for k in ('fused', 'beta'):
      emit(dict(base, part='rhs', levels=n, variant=k, ms=round(ms[k], 4),
                ms_rounds=[round(t, 4) for t in times[k]],
                ratio_to_beta=round(ms[k] / ms['beta'], 4),
                rel_diff=diff))

if 'step' in parts:
  dt = 1e-3
  T0 = torch.sin(np.pi * x[:, 0]) * torch.sin(np.pi * x[:, 1]) * \
      torch.sin(np.pi * x[:, 2])
  hist = [T0, 0.99 * T0, 0.98 * T0]
  info = {}

  def step():
    _, info['cg'] = st.step(hist, vel, dt, 3, 1.0, rtol=1e-8,
                            preconditioner='jacobi', return_info=True)
  ms, times = alternate({'step': step})
  emit(dict(base, part='step', time_order=3, dt=dt, preconditioner='jacobi',
            rtol=1e-8, ms=round(ms['step'], 4),
            ms_rounds=[round(t, 4) for t in times['step']],
            cg_iterations=int(info['cg']['num_iterations']),
            cg_status=info['cg']['status']))
