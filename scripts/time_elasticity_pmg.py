"""p-multigrid against Jacobi and plain CG for elasticity solves (DESIGN
§3.19), one JSON line per record (profiles/elasticity_pmg.jsonl, or OUT, is
rewritten).

(a) `solve`: a cantilever (unit box of N^3 elements of order P, clamped on
x = 0, under its own weight, E = 1, nu = 0.3), fp64 and fp32, for N in NS.
Per method (plain, Jacobi, pMG): iterations and time of a CG solve that
reaches a true relative residual |b - A x| / |b| of RES (1e-8; fp32: 1e-5).
pMG stops on that norm itself; plain and Jacobi stop on r.Mr, so their `tol`
is tightened until the true residual is there (`tol` in the record is the one
used).  After a warm-up of a few iterations the methods alternate, up to
ROUNDS timed solves each (fewer where they would add up to more than LONG_S
seconds, at least one); the median counts and every round is kept.  `setup_s`: the
host time to build the preconditioner, synchronised.  `vcycle`: one M(r) and
its parts per level (operator apply, Chebyshev step, restriction with its
sum, prolongation) and the coarse polynomial, each timed alone with HIP
events.

(b) `transfer`: at N = TN, order P -> P // 2, fp64 and fp32: the vector
transfers (`sfem_pmg_prolong_vec`, `sfem_pmg_restrict_vec` + `sfem_scatter_csr`)
against the composed route of the scalar kernels: copies to d contiguous
strips, d scalar launches on per-component ~id rows, copies back.  `rel_diff`:
the two results.  `spread`: (max - min) / median over the rounds.

env: NS (8,16,32), TN (32), P (7), ROUNDS (3), REPS (10), LONG_S (30), OUT, DTYPES
(fp64,fp32), PARTS (solve,transfer)."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from swirl_fem_amd import _ops
from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
from swirl_fem_amd.core import operators
from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType, Quadrature1D
from swirl_fem_amd.core.mesh_refiner import refine_premesh
from swirl_fem_amd.linalg import pmg
from swirl_fem_amd.linalg.cg import cg
from swirl_fem_amd.linalg.jacobi import JacobiPreconditioner
from swirl_fem_amd.linalg.pmg_elasticity import ElasticityPMultigrid

NS = [int(v) for v in os.environ.get('NS', '8,16,32').split(',')]
TN = int(os.environ.get('TN', '32'))
P = int(os.environ.get('P', '7'))
rounds = int(os.environ.get('ROUNDS', '3'))
reps = int(os.environ.get('REPS', '10'))
LONG_S = float(os.environ.get('LONG_S', '30'))   # see `time_solves`
dtypes = os.environ.get('DTYPES', 'fp64,fp32').split(',')
parts = os.environ.get('PARTS', 'solve,transfer').split(',')
out_path = os.environ.get('OUT', os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
    'elasticity_pmg.jsonl'))
if out_path:
  open(out_path, 'w').close()     # a run replaces the file
dev = torch.device('cuda:0')
DT = {'fp64': torch.float64, 'fp32': torch.float32}
RES = {'fp64': 1e-8, 'fp32': 1e-5}
LAM, MU = operators.lame_parameters(1.0, 0.3)
d = 3


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


def alternate(fns, k):
  """{name: median ms}, {name: rounds} of the variants run in turn."""
  for fn in fns.values():
    for _ in range(2):
      fn()
  torch.cuda.synchronize()
  times = {name: [] for name in fns}
  for _ in range(rounds):
    for name, fn in fns.items():
      times[name].append(timed(fn, k))
  return {name: float(np.median(v)) for name, v in times.items()}, times


def rnd(v, digits=4):
  return [round(t, digits) for t in v]


def spread(v):
  return round((max(v) - min(v)) / float(np.median(v)), 4)


_premesh = {}


def problem(N, dt):
  if N not in _premesh:       # the host refinement is shared by the dtypes
    _premesh.clear()
    _premesh[N] = refine_premesh(unit_cube_mesh(N, ndim=d), Nodes1D.create(
        P + 1, NodeType.GAUSS_LOBATTO_LEGENDRE))
  mesh = _premesh[N].finalize(device=dev, dtype=dt)
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(
      P + (d + 1) // 2, NodeType.GAUSS_LEGENDRE))
  fixed = torch.zeros((mesh.num_nodes, d), dtype=torch.bool, device=dev)
  fixed[mesh.node_coords[:, 0] < 1e-9] = True
  op = fes.elasticity_operator(fixed, lame_lambda=LAM, lame_mu=MU)
  f = torch.zeros((mesh.num_nodes, d), dtype=dt, device=dev)
  f[:, 1] = -1.0
  b = fes.helmholtz_operator(None).apply(f, 1.0, 0.0)
  b = (b * (~fixed).to(dt)).reshape(-1).contiguous()
  A = lambda x: op.apply(x.view(mesh.num_nodes, d)).reshape(-1)
  return mesh, fes, op, fixed, A, b


def run_cg(A, b, M, tol, maxiter=200000):
  """(x, info, seconds) of `linalg.cg` as `solve_elasticity` calls it."""
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  x, info = cg(A, b, tol=tol, M=M, maxiter=maxiter,
               check_every=getattr(M, 'check_every', 16))
  torch.cuda.synchronize()
  return x, info, time.perf_counter() - t0


def solve_to(A, b, M, res, stops_on_residual):
  """(info, tol, true residual, seconds): the CG solve whose true relative
  residual is at most `res`."""
  tol = res
  for _ in range(4):
    x, info, secs = run_cg(A, b, M, tol)
    true = float((b - A(x)).norm() / b.norm())
    if true <= res or stops_on_residual:
      break
    tol *= 0.5 * res / true
  return info, tol, true, secs


def time_solves(N, name):
  dt = DT[name]
  mesh, fes, op, fixed, A, b = problem(N, dt)
  base = {'part': 'solve', 'N': N, 'p': P, 'dtype': name,
          'elements': mesh.num_elements, 'dofs': mesh.num_nodes * d,
          'residual': RES[name]}
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  M = ElasticityPMultigrid(op)
  torch.cuda.synchronize()
  setup_pmg = time.perf_counter() - t0
  t0 = time.perf_counter()
  J = JacobiPreconditioner(op.diagonal().reshape(-1))
  torch.cuda.synchronize()
  setup_jac = time.perf_counter() - t0
  methods = {'plain': (None, 0.0), 'jacobi': (J, setup_jac),
             'pmg': (M, setup_pmg)}
  found, times = {}, {}
  for m, (pre, _) in methods.items():
    run_cg(A, b, pre, 0.0, maxiter=3)                         # warm-up
    found[m] = solve_to(A, b, pre, RES[name], m == 'pmg')
    times[m] = [found[m][3]]       # the solve that got there is a round
    print(f'# N={N} {name} {m}: {found[m][0]["num_iterations"]} iterations, '
          f'{found[m][3]:.2f} s', flush=True)
  # further rounds in turn, while a method's solves stay within LONG_S
  for _ in range(rounds - 1):
    for m, (pre, _) in methods.items():
      if sum(times[m]) + times[m][0] <= LONG_S:
        times[m].append(run_cg(A, b, pre, found[m][1])[2])
  for m, (pre, setup) in methods.items():
    info, tol, true, _ = found[m]
    emit(dict(base, method=m, status=info['status'],
              iterations=int(info['num_iterations']), tol=tol,
              true_residual=true, solve_s=round(float(np.median(times[m])), 4),
              solve_s_rounds=rnd(times[m]), spread=spread(times[m]),
              setup_s=round(setup, 4)))
  # one V-cycle and its parts
  r = b.clone()
  rec = dict(base, part='vcycle', orders=M.orders,
             coarse_steps=M.coarse_steps, lam_max=rnd(
                 M.spectral_bounds()['lam_max']),
             coarse_bounds=rnd(M.spectral_bounds()['coarse'], 6))
  fns = {'vcycle': lambda: M(r)}
  for l, lev in enumerate(M.levels[:-1]):
    a, c = lev.cheb[-1]
    fns[f'apply_{l}'] = lambda lev=lev: lev.apply(lev.x, lev.ax)
    fns[f'cheb_{l}'] = lambda lev=lev, a=a, c=c: _ops.cheb_step(
        lev.x, lev.d_, lev.ax, lev.b, lev.dinv, None, a, c, _ops.CHEB_GENERAL)
    fns[f'restrict_{l}'] = lambda l=l, lev=lev: M.restrict(
        l, lev.r, M.levels[l + 1].b)
    fns[f'prolong_{l}'] = lambda l=l, lev=lev: M.prolong(
        l, M.levels[l + 1].x, lev.x, add=True)
  last = M.levels[-1]
  fns['coarse'] = lambda: M._cycle(len(M.levels) - 1, last.b)
  ms, tms = alternate(fns, reps)
  rec.update({k + '_ms': round(v, 4) for k, v in ms.items()})
  rec['vcycle_ms_rounds'] = rnd(tms['vcycle'])
  # per level: 2 degree - 1 smoother applies + 1 residual apply, 2 degree
  # Chebyshev steps + the residual step
  deg = M.degree
  rec['modelled_ms'] = round(sum(
      2 * deg * ms[f'apply_{l}'] + (2 * deg + 1) * ms[f'cheb_{l}'] +
      ms[f'restrict_{l}'] + ms[f'prolong_{l}']
      for l in range(len(M.levels) - 1)) + ms['coarse'], 4)
  emit(rec)


def time_transfers(N, name):
  dt = DT[name]
  mesh, fes, op, fixed, A, b = problem(N, dt)
  M = ElasticityPMultigrid(op, orders=[P, P // 2, 1], coarse_steps=2,
                           bounds={'lam_max': [1.0, 1.0], 'coarse': (0.1, 1.0)})
  fine, coarse = M.levels[0], M.levels[1]
  t = fine.transfer
  Nf, Nc = fine.N, coarse.N
  fel = mesh.elements.to(torch.int64)
  celems = t['cidx'].to(torch.int64)
  # the composed route: per component ~id rows, strips, scalar kernels
  cid = [pmg.encode_rows(celems, coarse.fixed[:, c].contiguous())
         for c in range(d)]
  fid = [pmg.encode_rows(fel, fine.fixed[:, c].contiguous()) for c in range(d)]
  loc = torch.zeros(celems.numel(), dtype=dt, device=dev)
  tmp = torch.zeros(Nc, dtype=dt, device=dev)
  g = torch.Generator(device=dev).manual_seed(0)
  xc = torch.randn(Nc * d, generator=g, dtype=dt, device=dev)
  xf = torch.randn(Nf * d, generator=g, dtype=dt, device=dev)
  out_c = torch.zeros(Nc * d, dtype=dt, device=dev)

  def prolong_composed(x):
    for c in range(d):
      sc = xc.view(Nc, d)[:, c].contiguous()
      sf = x.view(Nf, d)[:, c].contiguous()
      _ops.pmg_prolong(sc, sf, cid[c], fid[c], t['owner'], t['mat'], d,
                       t['pc'], t['pf'], True)
      x.view(Nf, d)[:, c].copy_(sf)
    return x

  def restrict_composed(out):
    for c in range(d):
      sf = xf.view(Nf, d)[:, c].contiguous()
      _ops.pmg_restrict(sf, loc, cid[c], fid[c], t['owner'], t['mat'], d,
                        t['pc'], t['pf'])
      _ops.scatter_csr(loc, coarse.offsets, coarse.slots, Nc, out=tmp)
      out.view(Nc, d)[:, c].copy_(tmp)
    return out
  a1 = M.prolong(0, xc, xf.clone(), add=True)
  a2 = prolong_composed(xf.clone())
  r1 = M.restrict(0, xf, out_c).clone()
  r2 = restrict_composed(torch.zeros_like(out_c))
  diffs = (float((a1 - a2).abs().max() / a1.abs().max()),
           float((r1 - r2).abs().max() / r1.abs().max()))
  work = xf.clone()
  ms, tms = alternate({
      'prolong_vec': lambda: M.prolong(0, xc, work, add=True),
      'prolong_composed': lambda: prolong_composed(work),
      'restrict_vec': lambda: M.restrict(0, xf, out_c),
      'restrict_composed': lambda: restrict_composed(out_c)}, reps)
  for k, kind in enumerate(('prolong', 'restrict')):
    for variant in ('vec', 'composed'):
      key = f'{kind}_{variant}'
      emit({'part': 'transfer', 'N': N, 'p': P, 'pc': P // 2, 'dtype': name,
            'kind': kind + ('_add' if kind == 'prolong' else '_and_sum'),
            'variant': variant, 'ms': round(ms[key], 4),
            'ms_rounds': rnd(tms[key]), 'spread': spread(tms[key]),
            'ratio_to_composed': round(ms[key] / ms[f'{kind}_composed'], 4),
            'rel_diff': diffs[k]})


sizes = sorted(set((NS if 'solve' in parts else []) +
                   ([TN] if 'transfer' in parts else [])))
for N in sizes:
  for name in dtypes:
    if 'solve' in parts and N in NS:
      time_solves(N, name)
      torch.cuda.empty_cache()
    if 'transfer' in parts and N == TN:
      time_transfers(N, name)
      torch.cuda.empty_cache()
