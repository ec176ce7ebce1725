"""Cost of the plasticity adjoint, one JSON line per
configuration (profiles/plasticity_adjoint.jsonl, or OUT, is rewritten).

Run:  python scripts/time_plasticity_adjoint.py
Env:  N (32)  P (7)  SOLVE_N (8)  REPS (5)  ROUNDS (5)  DTYPES (fp64,fp32)  OUT

* `kernel`: `sfem_plasticity_vjp` alone on the Q^3 grid of N^3 elements --
  'vjp_displacement' (u, history and hbar in, a covector out) and 'vjp_state'
  (u, w, history and hbar in, hbar_prev and the five coefficient gradients
  out) -- next to the plasticity residual launch ('residual_state': history
  in, trial history and tangent state out) and `sfem_elasticity_sens` in the
  same run, variants alternating, median over the rounds.  sigma_y is the
  median von Mises stress of the elastic answer, so half of the points are
  plastic.  `bytes_model` is what each mode must move at least: the (E, Q^3)
  arrays it reads and writes once.
* `solve`: a clamped box at SOLVE_N^3 under a body force over three entries
  (load, load further, unload), fp64: forward and backward wall time of
  `solve_plasticity(..., differentiable=True)` with Jacobi and with
  `ElasticityPMultigrid`, the backward-to-forward ratio and the CG counts.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from swirl_fem_amd import _ops
from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
from swirl_fem_amd.core import operators
from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType, Quadrature1D
from swirl_fem_amd.core.mesh_refiner import refine_premesh
from swirl_fem_amd.examples.plasticity import BCType, solve_plasticity
from swirl_fem_amd.linalg.pmg_elasticity import ElasticityPMultigrid

N = int(os.environ.get('N', '32'))
P = int(os.environ.get('P', '7'))
solve_n = int(os.environ.get('SOLVE_N', '8'))
reps = int(os.environ.get('REPS', '5'))
rounds = int(os.environ.get('ROUNDS', '5'))
dtypes = os.environ.get('DTYPES', 'fp64,fp32').split(',')
out_path = os.environ.get('OUT', os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
    'plasticity_adjoint.jsonl'))
if out_path:
  open(out_path, 'w').close()     # a run replaces the file
dev = torch.device('cuda:0')
HBM = 8e12
LAM, MU, HH = 1.3, 0.6, 0.2


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


def alternate(fns, k=None):
  """{name: median ms}, {name: rounds} of the variants run in turn."""
  k = reps if k is None else k
  for fn in fns.values():
    for _ in range(2):
      fn()
  torch.cuda.synchronize()
  times = {name: [] for name in fns}
  for _ in range(rounds):
    for name, fn in fns.items():
      times[name].append(timed(fn, k))
  return {name: float(np.median(v)) for name, v in times.items()}, times


def rnd(v):
  return [round(t, 4) for t in v]


def box(n, dt, clamp=False):
  pm = unit_cube_mesh(n, ndim=3)
  if clamp:   # the face x = 0 as the group 'x0'
    faces = np.asarray(pm.physical_groups['boundary'])
    on_x0 = np.abs(np.asarray(pm.node_coords)[faces][:, :, 0]).max(
        axis=1) < 1e-9
    pm = pm.replace(physical_groups={'x0': faces[on_x0]})
  rp = refine_premesh(pm, Nodes1D.create(P + 1,
                                         NodeType.GAUSS_LOBATTO_LEGENDRE))
  mesh = rp.finalize(device=dev, dtype=dt)
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(
      P + 2, NodeType.GAUSS_LEGENDRE))
  return mesh, fes


d = 3
for name in dtypes:
  dt = {'fp64': torch.float64, 'fp32': torch.float32}[name]
  size = 8 if name == 'fp64' else 4
  mesh, fes = box(N, dt)
  op = fes.plasticity_operator(lame_lambda=LAM, lame_mu=MU, yield_stress=1.0,
                               hardening_modulus=HH)
  E, Q = mesh.num_elements, fes.quadrature.num_points
  nq = Q ** d
  NH, NL, NV = _ops.plasticity_sizes(d)
  base = {'N': N, 'p': P, 'Q': Q, 'dtype': name, 'elements': E,
          'nodes': mesh.num_nodes}
  x = mesh.node_coords
  u = 0.01 * torch.stack([torch.sin(2.0 * x[:, 1]), torch.cos(3.0 * x[:, 2]),
                          torch.sin(x[:, 0] + x[:, 1])], dim=1).contiguous()
  uq = fes._interpolate(_ops.gather_rows(u, mesh.elements)).contiguous()
  wq = torch.randn((E, nq, d), dtype=dt, device=dev)
  hbar = torch.randn((E, nq, NH), dtype=dt, device=dev)
  wd = op.point_weights()
  geo = (op.parts, op.host, d, Q, wd)
  # sigma_y: the median von Mises stress of the elastic answer
  _, _, _, sig = _ops.plasticity_local(uq, *geo, LAM, MU, None, 0.0, 1e30, HH,
                                       mode='residual', want_stress=True)
  sy = float(operators.von_mises(sig, d).median())
  del sig
  fwd = geo + (LAM, MU, None, 0.0, sy, HH)
  vjp = geo + (LAM, MU, sy, HH)
  _, hist, _, _ = _ops.plasticity_local(0.5 * uq, *fwd, mode='residual',
                                        want_hist=True)
  _, _, lin, _ = _ops.plasticity_local(uq, *fwd, mode='residual', hist=hist,
                                       want_lin=True)
  share = float((lin[..., 2:] != 0).any(-1).double().mean())
  del lin
  ms, times = alternate({
      'residual_state': lambda: _ops.plasticity_local(
          uq, *fwd, mode='residual', hist=hist, want_hist=True,
          want_lin=True),
      'elasticity_sens': lambda: _ops.elasticity_sens(uq, wq, *geo,
                                                      lambda0=0.5),
      'vjp_displacement': lambda: _ops.plasticity_vjp(
          uq, *vjp, mode='displacement', hist=hist, hbar=hbar),
      'vjp_state': lambda: _ops.plasticity_vjp(
          uq, *vjp, mode='state', hist=hist, hbar=hbar, w_q=wq, lambda0=0.5)})
  # reals per point read and written once: fields, W, histories, outputs
  reals = {'residual_state': 2 * d + 1 + 2 * NH + NL,
           'elasticity_sens': 2 * d + 1 + 3,
           'vjp_displacement': 2 * d + 1 + 2 * NH,
           'vjp_state': 2 * d + 1 + 3 * NH + 5}
  for k in ms:
    nb = size * E * nq * reals[k]
    emit(dict(base, part='kernel', variant=k, ms=round(ms[k], 4),
              ms_rounds=rnd(times[k]), plastic_share=round(share, 4),
              yield_stress=sy,
              ratio_to_residual=round(ms[k] / ms['residual_state'], 4),
              ratio_to_elasticity_sens=round(ms[k] / ms['elasticity_sens'], 4),
              bytes_model=nb,
              hbm_fraction=round(nb / (ms[k] * 1e-3) / HBM, 4)))
  del uq, wq, hbar, hist, u, op, fes, mesh
  torch.cuda.empty_cache()

  if name != 'fp64':
    continue
  # forward and backward of a three-entry clamped box
  mesh, fes = box(solve_n, dt, clamp=True)
  bcs = {'x0': (BCType.DIRICHLET, (0.0, 0.0, 0.0))}
  force = (0.0, -0.05, 0.0)
  kw = dict(lame_lambda=LAM, lame_mu=MU, hardening_modulus=HH)
  # the elastic answer fixes sigma_y: half of its largest von Mises stress
  u_el, _, el_info = solve_plasticity(
      mesh, force, bcs, yield_stress=1e30,
      preconditioner=ElasticityPMultigrid, return_info=True, **kw)
  # the solve's own Gauss rule: p + 2 points, the rule of `box`
  el = fes.plasticity_operator(yield_stress=1e30, **kw)
  sy = 0.5 * float(operators.von_mises(el.stress(u_el)[0], d).max())
  del el
  for pc_name, pc in (('jacobi', 'jacobi'), ('pmg', ElasticityPMultigrid)):
    fw, bw, rec = [], [], None
    for _ in range(max(2, rounds)):
      leaves = [torch.tensor(v, dtype=dt, device=dev, requires_grad=True)
                for v in (sy, HH)]
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      u, h, info = solve_plasticity(
          mesh, force, bcs, lame_lambda=LAM, lame_mu=MU,
          yield_stress=leaves[0], hardening_modulus=leaves[1],
          load_factors=(0.6, 1.0, 0.3), preconditioner=pc,
          differentiable=True, return_info=True)
      torch.cuda.synchronize()
      t1 = time.perf_counter()
      (u[:, 1].sum() + h[..., -1].sum()).backward()
      torch.cuda.synchronize()
      t2 = time.perf_counter()
      fw.append(1e3 * (t1 - t0))
      bw.append(1e3 * (t2 - t1))
      rec = info
    f_ms, b_ms = float(np.median(fw[1:])), float(np.median(bw[1:]))
    emit(dict(base, N=solve_n, elements=mesh.num_elements,
              nodes=mesh.num_nodes, part='solve', variant=pc_name,
              forward_ms=round(f_ms, 2), backward_ms=round(b_ms, 2),
              backward_to_forward=round(b_ms / f_ms, 4),
              forward_ms_rounds=rnd(fw), backward_ms_rounds=rnd(bw),
              forward_cg=int(rec['num_cg']), newton=int(rec['num_newton']),
              adjoint_cg=[int(i['num_iterations']) for i in rec['adjoint']],
              plastic_points=[e['plastic_points'] for e in rec['load_path']],
              yield_stress=sy))
  del fes, mesh
  torch.cuda.empty_cache()
