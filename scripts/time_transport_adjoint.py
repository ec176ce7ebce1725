"""Cost of the adjoint of scalar transport, one JSON line per
measurement (appended to profiles/transport_adjoint.jsonl, or OUT).

Size: the configuration of scripts/time_transport.py, N^3 elements of order P,
fp64, affine box (default 32^3, p = 7), Q = P + 2 Gauss points per direction.

* `vjp`: `sfem_transport_rhs_vjp` alone on the Q^3 grid for 1 / 2 / 3 levels
  (velocity, mass term and `wdet` at every level) and three output sets, next
  to the forward kernel `sfem_transport_rhs` of the same build in the same
  rounds.  Byte models, reals per point with d = 3 and n levels:
    forward          (d + 1) n + 2      T and u in; wdet in, out once
    both outputs     (2 d + 2) n + 2    T, u in, dT, du out; lam, wdet in
    dscalar only     (d + 1) n + 2      u in, dT out; lam, wdet in
    dvelocity only   (2 d + 1) n + 1    T, u in, du out; lam in
  `hbm_fraction`: the model over the time, against 8 TB/s; `ratio_to_forward`
  against the forward kernel of the same level count.
* `rollout`: three steps (orders 1, 2, 3) of a differentiable stepper on the
  Dirichlet box of §3.13 (k = 0.01, dt = 1e-3, Jacobi, rtol = 1e-8) with T0, a
  nodal velocity used at every level and the scalar diffusivity requiring
  grad: forward and `backward()` as wall clock with device synchronisation,
  and the iteration counts of the forward and the adjoint solves.
Variants alternate; ROUNDS rounds of REPS calls after a warm-up, HIP events,
the median round counts and every round is kept.
env: N (32), P (7), REPS (10), ROUNDS (5), OUT, PARTS (vjp,rollout)."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from swirl_fem_amd import _ops
from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType
from swirl_fem_amd.core.mesh_refiner import refine_premesh
from swirl_fem_amd.examples.transport import BCType, ScalarTransport

N = int(os.environ.get('N', '32'))
P = int(os.environ.get('P', '7'))
reps = int(os.environ.get('REPS', '10'))
rounds = int(os.environ.get('ROUNDS', '5'))
parts = os.environ.get('PARTS', 'vjp,rollout').split(',')
out_path = os.environ.get('OUT', os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
    'transport_adjoint.jsonl'))
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
kdiff = torch.tensor(0.01, dtype=f64, device=dev, requires_grad=True)
st = ScalarTransport.create(mesh, {'boundary': (BCType.DIRICHLET, 0.0)},
                            diffusivity=kdiff, differentiable=True)
fes, op = st.fespace, st.rhs_op
E, d = mesh.num_elements, 3
Q = fes.quadrature.num_points
nq = Q ** d
base = {'N': N, 'p': P, 'Q': Q, 'dtype': 'fp64'}
assert [p['geo_mode'] for p in op.parts] == [1], 'expected an affine box'
x = mesh.node_coords
coefs = [(-1.5, 1.0), (2.0, -3.0), (-0.5, 3.0)]

if 'vjp' in parts:
  Tq = [torch.randn((E, nq), dtype=f64, device=dev) for _ in range(3)]
  uq = [torch.randn((E, nq, d), dtype=f64, device=dev) for _ in range(3)]
  lam = torch.randn((E, nq), dtype=f64, device=dev)
  wd = op.point_weights()
  sets = {'both': (True, True), 'dscalar': (True, False),
          'dvelocity': (False, True)}
  model = {'forward': lambda n: (d + 1) * n + 2,
           'both': lambda n: (2 * d + 2) * n + 2,
           'dscalar': lambda n: (d + 1) * n + 2,
           'dvelocity': lambda n: (2 * d + 1) * n + 1}
  fns = {}
  for n in (1, 2, 3):
    levels = [(Tq[j], uq[j]) + coefs[j] for j in range(n)]
    fns[('forward', n)] = lambda levels=levels: _ops.transport_rhs(
        levels, op.parts, op.host, d, Q, wdet=wd)
    for name, want in sets.items():
      fns[(name, n)] = lambda levels=levels, want=want, n=n: (
          _ops.transport_rhs_vjp(lam, levels, op.parts, op.host, d, Q, wd,
                                 ([want] * n, False)))
  ms, times = alternate(fns)
  for (name, n), t in ms.items():
    nb = 8 * E * nq * model[name](n)
    emit(dict(base, part='vjp', kernel=name, levels=n, ms=round(t, 4),
              ms_rounds=[round(v, 4) for v in times[(name, n)]],
              bytes_model=nb, hbm_fraction=round(nb / (t * 1e-3) / HBM, 4),
              ratio_to_forward=round(t / ms[('forward', n)], 4),
              bytes_ratio_to_forward=round(
                  model[name](n) / model['forward'](n), 4)))
  del Tq, uq, lam, fns

if 'rollout' in parts:
  dt = 1e-3
  T0 = (torch.sin(np.pi * x[:, 0]) * torch.sin(np.pi * x[:, 1]) *
        torch.sin(np.pi * x[:, 2])).requires_grad_()
  vel = torch.stack([1.0 + x[:, 1], 0.5 - x[:, 0], 0.3 + 0.0 * x[:, 2]],
                    dim=-1).contiguous().requires_grad_()
  w = torch.randn(mesh.num_nodes, dtype=f64, device=dev)

  def rollout():
    Ts, infos = [T0], []
    for k in (1, 2, 3):
      T, info = st.step(Ts, [vel] * k, dt, k, 1.0, rtol=1e-8,
                        preconditioner='jacobi', return_info=True)
      Ts.append(T)
      infos.append(info)
    return (Ts[-1] * w).sum(), infos
  fwd, bwd, last = [], [], None
  for r in range(rounds + 1):          # the first round warms up
    for t in (T0, vel, kdiff):
      t.grad = None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss, infos = rollout()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    loss.backward()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    if r:
      fwd.append((t1 - t0) * 1e3)
      bwd.append((t2 - t1) * 1e3)
    last = infos
  emit(dict(base, part='rollout', steps=3, time_orders=[1, 2, 3], dt=dt,
            preconditioner='jacobi', rtol=1e-8,
            forward_ms=round(float(np.median(fwd)), 3),
            backward_ms=round(float(np.median(bwd)), 3),
            forward_ms_rounds=[round(v, 3) for v in fwd],
            backward_ms_rounds=[round(v, 3) for v in bwd],
            cg_iterations=[int(i['num_iterations']) for i in last],
            adjoint_cg_iterations=[int(a['num_iterations']) for i in last
                                   for a in i.get('adjoint', [])],
            adjoint_status=[a['status'] for i in last
                            for a in i.get('adjoint', [])],
            grad_norms={'T0': float(T0.grad.norm()),
                        'velocity': float(vel.grad.norm()),
                        'diffusivity': float(kdiff.grad)}))
