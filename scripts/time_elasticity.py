"""Cost of the fused linear-elasticity operator, one JSON line
per configuration (profiles/elasticity.jsonl, or OUT, is rewritten).

Size: N^3 hex elements of order P, affine box (default 32^3, p = 7), fp64 and
fp32; the solve's Gauss rule, Q = P + 2 points per direction.  Per dtype, in
one process:

* `kernel`: `sfem_elasticity_local` alone on the Q^3 grid, scalar
  coefficients, no mass term.  `bytes_model`: what it must move -- d reals
  per point in, d out, `wdet` once; `hbm_fraction`: that over the time,
  against 8 TB/s.
* `apply_local`: interpolate, kernel, transposed interpolate, next to the
  scalar two-grid Helmholtz `apply_local` on the same d components
  (`helmholtz_ms`; `helmholtz_fraction` = helmholtz_ms / ms: the scalar
  kernel applies d uncoupled Laplacians and bounds what this one can reach).
* `apply`: the assembled operator, 'fused' against 'generic', the only route
  before it: `local_covector` of sigma(u) : grad v with `vector_function` and
  `grad`, gather and scatter as in the fused route.  `rel_diff`: the two
  results, max norm.
* `cg_iteration`: one iteration of `linalg.cg` on the flat (N d,) vectors of
  `solve_elasticity` with the fused operator (all faces but one free, Jacobi
  off).
Variants alternate; ROUNDS rounds of REPS calls after a warm-up, HIP events,
the median round counts and every round is kept.
env: N (32), P (7), REPS (5), ROUNDS (5), OUT, DTYPES (fp64,fp32)."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from swirl_fem_amd import _ops
from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
from swirl_fem_amd.core.fespace import FiniteElementSpace, grad
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType, Quadrature1D
from swirl_fem_amd.core.mesh_refiner import refine_premesh
from swirl_fem_amd.linalg.cg import CGRunner

N = int(os.environ.get('N', '32'))
P = int(os.environ.get('P', '7'))
reps = int(os.environ.get('REPS', '5'))
rounds = int(os.environ.get('ROUNDS', '5'))
dtypes = os.environ.get('DTYPES', 'fp64,fp32').split(',')
out_path = os.environ.get('OUT', os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
    'elasticity.jsonl'))
if out_path:
  open(out_path, 'w').close()     # a run replaces the file
dev = torch.device('cuda:0')
HBM = 8e12
LAM, MU = 1.3, 0.6


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


pm = unit_cube_mesh(N, ndim=3)
rp = refine_premesh(pm, Nodes1D.create(P + 1, NodeType.GAUSS_LOBATTO_LEGENDRE))
for name in dtypes:
  dt = {'fp64': torch.float64, 'fp32': torch.float32}[name]
  size = 8 if name == 'fp64' else 4
  mesh = rp.finalize(device=dev, dtype=dt)
  d = 3
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(
      P + (d + 1) // 2, NodeType.GAUSS_LEGENDRE))
  op = fes.elasticity_operator(lame_lambda=LAM, lame_mu=MU)
  assert [p['geo_mode'] for p in op.parts] == [1], 'expected an affine box'
  E, Q = mesh.num_elements, fes.quadrature.num_points
  nq, n = Q ** d, (P + 1) ** d
  base = {'N': N, 'p': P, 'Q': Q, 'dtype': name, 'elements': E,
          'nodes': mesh.num_nodes}

  uq = torch.randn((E, nq, d), dtype=dt, device=dev)
  wd = op.point_weights()
  ms, times = alternate({'k': lambda: _ops.elasticity_local(
      uq, op.parts, op.host, d, Q, wd, LAM, MU)})
  nb = size * E * nq * (2 * d + 1)
  emit(dict(base, part='kernel', ms=round(ms['k'], 4),
            ms_rounds=rnd(times['k']), bytes_model=nb,
            hbm_fraction=round(nb / (ms['k'] * 1e-3) / HBM, 4)))
  del uq

  ul = torch.randn((E, n, d), dtype=dt, device=dev)
  helm = fes.helmholtz_operator(None)
  ms, times = alternate({'e': lambda: op.apply_local(ul),
                         'h': lambda: helm.apply_local(ul, 0.0, 1.0)})
  emit(dict(base, part='apply_local', ms=round(ms['e'], 4),
            ms_rounds=rnd(times['e']), helmholtz_ms=round(ms['h'], 4),
            helmholtz_ms_rounds=rnd(times['h']),
            helmholtz_fraction=round(ms['h'] / ms['e'], 4)))
  del ul

  u = torch.randn((mesh.num_nodes, d), dtype=dt, device=dev)

  def form(uf, vf):
    def at(x):
      gu, gv = grad(uf)(x), grad(vf)(x)
      sym = gu + torch.einsum('jk->kj', gu)
      return MU * torch.vdot(sym, gv) + LAM * torch.trace(gu) * torch.trace(gv)
    return at

  def generic():
    loc = fes.local_covector(form, (
        fes.vector_function(_ops.gather_rows(u, mesh.elements)),
        fes.vector_function(None)))
    return _ops.scatter_add(loc.contiguous(), mesh.elements, mesh.num_nodes,
                            ncomp=d)
  a, b = op.apply(u), generic()
  diff = float((a - b).abs().max() / b.abs().max())
  del a, b
  ms, times = alternate({'fused': lambda: op.apply(u), 'generic': generic})
  for k in ('fused', 'generic'):
    emit(dict(base, part='apply', variant=k, ms=round(ms[k], 4),
              ms_rounds=rnd(times[k]),
              ratio_to_generic=round(ms[k] / ms['generic'], 4),
              rel_diff=diff))

  fixed = torch.zeros((mesh.num_nodes, d), dtype=torch.bool, device=dev)
  fixed[mesh.node_coords[:, 0] < 1e-9] = True
  mop = fes.elasticity_operator(fixed, lame_lambda=LAM, lame_mu=MU)
  keep = (~fixed).to(dt)
  rhs = (torch.randn((mesh.num_nodes, d), dtype=dt, device=dev) *
         keep).reshape(-1)
  A = lambda x: mop.apply(x.view(mesh.num_nodes, d)).reshape(-1)
  run = CGRunner(A, rhs, tol=0.0, atol=0.0, maxiter=10 ** 6)
  ms, times = alternate({'it': run.step})
  emit(dict(base, part='cg_iteration', ms=round(ms['it'], 4),
            ms_rounds=rnd(times['it'])))
  del run, mop, op, helm, fes, mesh, u, rhs
  torch.cuda.empty_cache()
