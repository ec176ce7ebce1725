"""Cost of the neo-Hookean sensitivity kernel and of one backward pass (DESIGN
§3.21), one JSON line per configuration (profiles/hyperelasticity_adjoint.jsonl,
or OUT, is rewritten).  Every time is set against a named counterpart from the
same run.

Size: N^3 hex elements of order P, affine box (default 32^3, p = 7), fp64 and
fp32; the solve's Gauss rule, Q = P + 2 points per direction.  Per dtype, in
one process:

* `sens`: `sfem_hyperelastic_sens` alone on the Q^3 grid with all three
  outputs ('all'), the two Lame outputs without `u` ('lame'), `dmu` alone
  ('dmu') and `drho` alone ('drho', no derivative stage), next to
  `sfem_elasticity_sens` with all three outputs on the same fields
  ('linear_sens') and to the tangent mode of `sfem_hyperelastic_local` reading
  the same state ('tangent'), in the same alternating rounds; lambda0 = 1, a
  displacement with |H| <= 0.3.  `bytes_model`, stated before it is measured:
  per point 'all' moves d (v) + d (u) + d*d + 1 (state) + 1 (`wdet`) reals in
  and 3 out, 'lame' d + d*d + 1 + 1 in and 2 out, 'dmu' the same in and 1 out,
  'drho' 2 d + 1 in and 1 out, 'linear_sens' 2 d + 1 in and 3 out, 'tangent'
  d + d*d + 1 + 1 in and d out; the state row is read once per component pass
  and the model counts it once (the repeats are left to the caches).
  `hbm_fraction`: that over the time, against 8 TB/s.  `ratio_to_linear_sens`,
  `ratio_to_tangent`: median over median, with the ratio of every round;
  `bytes_ratio_to_linear_sens`: the model's.
* `backward`: one `solve_hyperelasticity(..., differentiable=True)` with a
  per-element lame_mu that requires grad and its `.backward()`, a cantilever
  of NS^3 elements (default 8^3) of the same order clamped on x = 0 under a
  transverse body force, fp64 only, two load steps, newton_rtol 1e-8
  (adjoint_rtol the same), linear_rtol 1e-6, with 'jacobi' and with
  `ElasticityPMultigrid`: Newton and CG iterations of the forward solve, CG
  iterations of the adjoint solve and wall clock of each with synchronisation
  (the median of ROUNDS runs after one warm-up run); `backward_over_forward`.
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
from swirl_fem_amd.examples.hyperelasticity import BCType
from swirl_fem_amd.examples.hyperelasticity import solve_hyperelasticity
from swirl_fem_amd.linalg.pmg_elasticity import ElasticityPMultigrid

N = int(os.environ.get('N', '32'))
NS = int(os.environ.get('NS', '8'))
P = int(os.environ.get('P', '7'))
reps = int(os.environ.get('REPS', '5'))
rounds = int(os.environ.get('ROUNDS', '5'))
dtypes = os.environ.get('DTYPES', 'fp64,fp32').split(',')
out_path = os.environ.get('OUT', os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
    'hyperelasticity_adjoint.jsonl'))
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
# the cantilever: the faces of the boundary group that lie on x = 0
pms = unit_cube_mesh(NS, ndim=d)
faces = np.asarray(pms.physical_groups['boundary'])
on_x0 = np.abs(np.asarray(pms.node_coords)[faces][:, :, 0]).max(axis=1) < 1e-9
pms = pms.replace(physical_groups={'x0': faces[on_x0]})
rps = refine_premesh(pms, Nodes1D.create(P + 1, GLL))
for name in dtypes:
  dt = {'fp64': torch.float64, 'fp32': torch.float32}[name]
  size = 8 if name == 'fp64' else 4
  mesh = rp.finalize(device=dev, dtype=dt)
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(
      P + (d + 1) // 2, GL))
  op = fes.hyperelastic_operator(lame_lambda=LAM, lame_mu=MU)
  assert [p['geo_mode'] for p in op.parts] == [1], 'expected an affine box'
  E, Q = mesh.num_elements, fes.quadrature.num_points
  nq = Q ** d
  base = {'N': N, 'p': P, 'Q': Q, 'dtype': name, 'elements': E}
  # a smooth displacement with |H| <= 0.3, interpolated to the grid
  x = mesh.node_coords
  u = 0.05 * torch.stack([torch.sin(2.0 * x[:, 1]), torch.cos(3.0 * x[:, 2]),
                          torch.sin(x[:, 0] + x[:, 1])], dim=1).contiguous()
  uq = fes._interpolate(_ops.gather_rows(u, mesh.elements)).contiguous()
  vq = torch.randn((E, nq, d), dtype=dt, device=dev)
  wd = op.point_weights()
  geo = (op.parts, op.host, d, Q, wd)
  _, state, _ = _ops.hyperelastic_local(uq, *geo, LAM, MU, mode='residual',
                                        want_state=True)
  assert bool(torch.isfinite(state).all())
  sens = lambda want, uu: (lambda: _ops.hyperelastic_sens(
      vq, state, *geo, uu, 1.0, want=want))
  fns = {'all': sens((True, True, True), uq),
         'lame': sens((True, True, False), None),
         'dmu': sens((False, True, False), None),
         'drho': sens((False, False, True), uq),
         'linear_sens': lambda: _ops.elasticity_sens(uq, vq, *geo, 1.0),
         'tangent': lambda: _ops.hyperelastic_local(
             vq, *geo, LAM, MU, None, 1.0, mode='tangent', state=state)}
  st = d * d + 1
  reals = {'all': 2 * d + st + 1 + 3, 'lame': d + st + 1 + 2,
           'dmu': d + st + 1 + 1, 'drho': 2 * d + 1 + 1,
           'linear_sens': 2 * d + 1 + 3, 'tangent': d + st + 1 + d}
  ms, times = alternate(fns)
  for k in fns:
    nb = size * E * nq * reals[k]
    to = lambda other: [a / b for a, b in zip(times[k], times[other])]
    emit(dict(base, part='sens', variant=k, ms=round(ms[k], 4),
              ms_rounds=rnd(times[k]), bytes_model=nb,
              hbm_fraction=round(nb / (ms[k] * 1e-3) / HBM, 4),
              ratio_to_linear_sens=round(ms[k] / ms['linear_sens'], 4),
              ratio_to_linear_sens_rounds=rnd(to('linear_sens')),
              bytes_ratio_to_linear_sens=round(
                  reals[k] / reals['linear_sens'], 4),
              ratio_to_tangent=round(ms[k] / ms['tangent'], 4),
              ratio_to_tangent_rounds=rnd(to('tangent'))))
  del uq, vq, state, op, fes, mesh, wd, fns, u, x
  torch.cuda.empty_cache()
  if name != 'fp64':
    continue

  mesh = rps.finalize(device=dev, dtype=dt)
  bcs = {'x0': (BCType.DIRICHLET, (0.0, 0.0, 0.0))}
  for pc_name, pc in (('jacobi', 'jacobi'), ('pmg', ElasticityPMultigrid)):
    fw, bw, counts = [], [], None
    for r in range(rounds + 1):
      mu = torch.full((mesh.num_elements,), MU, dtype=dt, device=dev,
                      requires_grad=True)
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      u, info = solve_hyperelasticity(
          mesh, (0.0, -0.05, 0.0), bcs, lame_lambda=LAM, lame_mu=mu,
          load_steps=2, newton_rtol=1e-8, linear_rtol=1e-6, preconditioner=pc,
          return_info=True, differentiable=True)
      torch.cuda.synchronize()
      t1 = time.perf_counter()
      u[:, 1].sum().backward()
      torch.cuda.synchronize()
      t2 = time.perf_counter()
      if r:                          # the first run warms up
        fw.append(1e3 * (t1 - t0))
        bw.append(1e3 * (t2 - t1))
      counts = (int(info['num_newton']), int(info['num_cg']),
                int(info['adjoint']['num_iterations']))
      assert info['adjoint']['status'] == 'converged'
      assert mu.grad is not None and bool(torch.isfinite(mu.grad).all())
    emit(dict(N=NS, p=P, dtype=name, elements=mesh.num_elements,
              nodes=mesh.num_nodes, part='backward', preconditioner=pc_name,
              newton_iterations=counts[0], forward_cg_iterations=counts[1],
              adjoint_cg_iterations=counts[2],
              tip_deflection=round(float(u.detach()[:, 1].min()), 5),
              forward_ms=round(float(np.median(fw)), 3),
              backward_ms=round(float(np.median(bw)), 3),
              forward_ms_rounds=rnd(fw), backward_ms_rounds=rnd(bw),
              backward_over_forward=round(
                  float(np.median(bw) / np.median(fw)), 4),
              backward_over_forward_rounds=rnd(
                  [b / f for b, f in zip(bw, fw)])))
  del mesh
  torch.cuda.empty_cache()
