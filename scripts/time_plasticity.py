"""Cost of the J2 plasticity residual and tangent, one JSON line
per configuration (profiles/plasticity.jsonl, or OUT, is rewritten).

Size: N^3 hex elements of order P, affine box (default 32^3, p = 7), fp64 and
fp32; the solve's Gauss rule, Q = P + 2 points per direction.  Per dtype, in
one process:

* `kernel`: `sfem_plasticity_local` alone on the Q^3 grid -- 'residual' (no
  optional output, virgin material), 'residual_state' (the launch of
  `linearize`: a committed history in, `hist_out` and `lin` out) and 'tangent'
  -- next to 'linear', `sfem_elasticity_local`, and 'hyper_tangent', the
  tangent mode of `sfem_hyperelastic_local`, in the same alternating rounds;
  scalar coefficients, no mass term.  The yield stress is the median von
  Mises stress of the elastic answer to the input field, so half of the
  points yield; `plastic_share` records what the launch found.
  `ratio_to_linear`, `ratio_to_hyper_tangent`: median over median, with the
  ratio of every round; `bytes_model`: what the variant must move (d reals
  per point in, d out, `wdet`, plus the state reals it reads or writes);
  `hbm_fraction`: that over the time, against 8 TB/s.
* `newton_step`: one Newton step (linearize, CG to 1e-6 on the tangent, one
  residual of the line search) of the box of NEWTON_N^3 elements clamped on
  x = 0 under a transverse body force, at the state the first step from zero
  leaves, with 'jacobi' and with `ElasticityPMultigrid` (fp64 only);
  `cg_iterations` and the plastic share with each.
Variants alternate; ROUNDS rounds of REPS calls after a warm-up, HIP events,
the median round counts and every round is kept.
env: N (32), P (7), NEWTON_N (8), REPS (5), ROUNDS (5), OUT, DTYPES
(fp64,fp32)."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from swirl_fem_amd import _ops
from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
from swirl_fem_amd.core import operators
from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType, Quadrature1D
from swirl_fem_amd.core.mesh_refiner import refine_premesh
from swirl_fem_amd.linalg.cg import cg
from swirl_fem_amd.linalg.jacobi import JacobiPreconditioner
from swirl_fem_amd.linalg.pmg_elasticity import ElasticityPMultigrid

N = int(os.environ.get('N', '32'))
P = int(os.environ.get('P', '7'))
newton_n = int(os.environ.get('NEWTON_N', '8'))
reps = int(os.environ.get('REPS', '5'))
rounds = int(os.environ.get('ROUNDS', '5'))
dtypes = os.environ.get('DTYPES', 'fp64,fp32').split(',')
out_path = os.environ.get('OUT', os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
    'plasticity.jsonl'))
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


def box(n, dt):
  pm = unit_cube_mesh(n, ndim=3)
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
  assert [p['geo_mode'] for p in op.parts] == [1], 'expected an affine box'
  E, Q = mesh.num_elements, fes.quadrature.num_points
  nq = Q ** d
  NH, NL, NV = _ops.plasticity_sizes(d)
  base = {'N': N, 'p': P, 'Q': Q, 'dtype': name, 'elements': E,
          'nodes': mesh.num_nodes}

  # a smooth displacement with strains of a few percent on the grid
  x = mesh.node_coords
  u = 0.01 * torch.stack([torch.sin(2.0 * x[:, 1]), torch.cos(3.0 * x[:, 2]),
                          torch.sin(x[:, 0] + x[:, 1])], dim=1).contiguous()
  uq = fes._interpolate(_ops.gather_rows(u, mesh.elements)).contiguous()
  wq = torch.randn((E, nq, d), dtype=dt, device=dev)
  wd = op.point_weights()
  geo = (op.parts, op.host, d, Q, wd, LAM, MU)
  # sigma_y: the median von Mises stress of the elastic answer
  _, _, _, sig = _ops.plasticity_local(uq, *geo, None, 0.0, 1e30, HH,
                                       mode='residual', want_stress=True)
  sy = float(operators.von_mises(sig, d).median())
  del sig
  args = geo + (None, 0.0, sy, HH)
  # a committed history: the trial history of half the displacement
  _, hist, _, _ = _ops.plasticity_local(0.5 * uq, *args, mode='residual',
                                        want_hist=True)
  _, _, lin, _ = _ops.plasticity_local(uq, *args, mode='residual', hist=hist,
                                       want_lin=True)
  share = float((lin[..., 2:] != 0).any(-1).double().mean())
  assert bool(torch.isfinite(lin).all())
  _, state, _ = _ops.hyperelastic_local(uq, *geo, mode='residual',
                                        want_state=True)
  ms, times = alternate({
      'linear': lambda: _ops.elasticity_local(wq, *geo),
      'hyper_tangent': lambda: _ops.hyperelastic_local(
          wq, *geo, mode='tangent', state=state),
      'residual': lambda: _ops.plasticity_local(uq, *args, mode='residual'),
      'residual_state': lambda: _ops.plasticity_local(
          uq, *args, mode='residual', hist=hist, want_hist=True,
          want_lin=True),
      'tangent': lambda: _ops.plasticity_local(wq, *args, mode='tangent',
                                               lin=lin)})
  extra = {'linear': 0, 'hyper_tangent': d * d + 1, 'residual': 0,
           'residual_state': 2 * NH + NL, 'tangent': NL}
  for k in ms:
    nb = size * E * nq * (2 * d + 1 + extra[k])
    emit(dict(base, part='kernel', variant=k, ms=round(ms[k], 4),
              ms_rounds=rnd(times[k]), plastic_share=round(share, 4),
              yield_stress=sy,
              ratio_to_linear=round(ms[k] / ms['linear'], 4),
              ratio_to_linear_rounds=rnd(
                  [a / b for a, b in zip(times[k], times['linear'])]),
              ratio_to_hyper_tangent=round(ms[k] / ms['hyper_tangent'], 4),
              ratio_to_hyper_tangent_rounds=rnd(
                  [a / b for a, b in zip(times[k], times['hyper_tangent'])]),
              bytes_model=nb,
              hbm_fraction=round(nb / (ms[k] * 1e-3) / HBM, 4)))
  del uq, wq, state, lin, hist, u, op, fes, mesh
  torch.cuda.empty_cache()

  if name != 'fp64':
    continue
  # one Newton step of a clamped box, Jacobi and p-multigrid
  from swirl_fem_amd.examples.elasticity import _load_vector
  mesh, fes = box(newton_n, dt)
  nodes = mesh.num_nodes
  fixed = torch.zeros((nodes, d), dtype=torch.bool, device=dev)
  fixed[mesh.node_coords[:, 0] < 1e-9] = True
  kw = dict(lame_lambda=LAM, lame_mu=MU, hardening_modulus=HH)
  keep = (~fixed).to(dt)
  f_ext = keep * _load_vector(fes, (0.0, -0.05, 0.0), [])
  # the elastic answer fixes sigma_y: half of its largest von Mises stress
  el = fes.plasticity_operator(fixed, yield_stress=1e30, **kw)
  pmg = ElasticityPMultigrid(el.linear, 0.0)
  A0 = lambda y: el.linear.apply(y.view(nodes, d)).reshape(-1)
  u0, _ = cg(A0, f_ext.reshape(-1).contiguous(), tol=1e-8, M=pmg,
             check_every=getattr(pmg, 'check_every', 16))
  u0 = u0.view(nodes, d)
  sy = 0.5 * float(operators.von_mises(el.stress(u0)[0], d).max())
  op = fes.plasticity_operator(fixed, yield_stress=sy, **kw)
  pcs = {'jacobi': JacobiPreconditioner(op.linear.diagonal().reshape(-1)),
         'pmg': pmg}
  its, shares = {}, {}

  def step(v, M, key=None):
    lin = op.linearize(v)
    r = lin.residual - f_ext
    A = lambda y: op.tangent(lin).apply(y.view(nodes, d)).reshape(-1)
    dw, info = cg(A, (-r).reshape(-1).contiguous(), tol=1e-6, M=M,
                  check_every=getattr(M, 'check_every', 16))
    if key is not None:
      its[key] = int(info['num_iterations'])
      shares[key] = lin.num_plastic() / lin.lin[..., 0].numel()
    out = v + dw.view(nodes, d)
    op.residual(out)            # the first trial of the line search
    return out
  u1 = step(torch.zeros((nodes, d), dtype=dt, device=dev), pcs['pmg'])
  ms, times = alternate({k: (lambda k=k: step(u1, pcs[k], k)) for k in pcs},
                        k=1)
  nbase = dict(base, N=newton_n, elements=mesh.num_elements, nodes=nodes)
  for k in ms:
    emit(dict(nbase, part='newton_step', variant=k, ms=round(ms[k], 3),
              ms_rounds=rnd(times[k]), cg_iterations=its[k],
              plastic_share=round(shares[k], 4), yield_stress=sy,
              tip_deflection=round(float(u1[:, 1].min()), 5)))
  del op, el, fes, mesh, pcs
  torch.cuda.empty_cache()
