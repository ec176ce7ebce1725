"""Partitioned Helmholtz solves with and without preconditioning on the
2 x 2 x 2 block layout of `bench.py --gpus 8`, ranks as threads on ONE GPU
(`distributed.inprocess.ThreadWorld`): iteration counts of plain, Jacobi and
p-multigrid PCG, the true global residual of each gathered solution (one-rank
operator of the whole box), and the per-rank setup time of the two
preconditioners.  The ranks' kernels serialise on the one GPU, so no time to
solution or scaling is measured here.  One JSON line per case.
env: CASES (p4,p8,p11), N (elements per block and direction: 4), OUT (stdout
only if unset)."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType, Quadrature1D
from swirl_fem_amd.distributed import blocks, inprocess, solver
from swirl_fem_amd.linalg.jacobi import JacobiPreconditioner
from swirl_fem_amd.linalg.pmg import PMultigridPreconditioner

GRID = (2, 2, 2)
L0, L1 = 0.3, 1.0
CASES = {'p4': (5, torch.float64, 1e-10), 'p8': (9, torch.float64, 1e-10),
         'p11': (12, torch.float32, 1e-6)}
dev = torch.device('cuda:0')
n = int(os.environ.get('N', '4'))
out_path = os.environ.get('OUT')


def run_case(name):
  P, dtype, tol = CASES[name]
  quad = Quadrature1D.create_from_nodes_1d(
      Nodes1D.create(P, NodeType.GAUSS_LOBATTO_LEGENDRE))
  whole = blocks.build_block_partition([n * g for g in GRID], P, (1, 1, 1), 0,
                                       device=dev, jitter=0.1, dtype=dtype)
  gm = whole.mesh
  gbm = gm.physical_masks['boundary']
  gfes = FiniteElementSpace.create(gm, quad)
  gop = gfes.helmholtz_operator(gbm)
  gx = gm.node_coords.double()
  f = (torch.sin(3 * gx[:, 0]) * torch.cos(2 * gx[:, 1]) +
       gx[:, 2] ** 2).to(dtype)
  b = gfes.helmholtz_operator(None).apply(f * ~gbm, 1.0, 0.0) * ~gbm
  lookup = dict(zip(whole.global_keys.tolist(), range(gm.num_nodes)))

  def rank_main(rank):
    part = blocks.build_block_partition(n, P, GRID, rank, device=dev,
                                        jitter=0.1, dtype=dtype)
    mesh = part.mesh
    bm = mesh.physical_masks.get('boundary')
    if bm is None:
      bm = torch.zeros(mesh.num_nodes, dtype=torch.bool, device=dev)
    fes = FiniteElementSpace.create(mesh, quad)
    op = fes.helmholtz_operator(bm)
    ids = torch.as_tensor([lookup[k] for k in part.global_keys.tolist()],
                          device=dev)
    b_loc = fes.helmholtz_operator(None).apply(f[ids] * ~bm, 1.0, 0.0) * ~bm
    res = {}
    for kind in ('plain', 'jacobi', 'pmg'):
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      M = (None if kind == 'plain' else JacobiPreconditioner(op, L0, L1)
           if kind == 'jacobi' else PMultigridPreconditioner(op, L0, L1))
      torch.cuda.synchronize()
      setup = time.perf_counter() - t0
      A = solver.OverlappedHelmholtz(op, part.plan, L0, L1)
      x, info = solver.cg(A, b_loc, part.plan, tol=tol, M=M)
      extra = {}
      if kind == 'pmg':
        extra = dict(orders=M.orders, coarse_steps=M.coarse_steps,
                     coarse_bounds=list(M.coarse_bounds),
                     lam_max=[lev.lam_max for lev in M.levels[:-1]])
      res[kind] = dict(x=x.double().cpu().numpy(), setup_s=setup,
                       iterations=info['num_iterations'],
                       status=info['status'], **extra)
    return ids.cpu().numpy(), res

  out = inprocess.ThreadWorld(8).run(rank_main)
  bn = float(torch.linalg.vector_norm(b.double()))
  rec = dict(case=name, grid=list(GRID), elements_per_block=n, P=P,
             dtype=str(dtype).replace('torch.', ''), tol=tol,
             global_nodes=gm.num_nodes, lambda0=L0, lambda1=L1)
  for kind in ('plain', 'jacobi', 'pmg'):
    xg = np.zeros(gm.num_nodes)
    for ids, res in out.values():
      xg[ids] = res[kind]['x']
    r = b.double() - gop.apply(torch.as_tensor(xg, dtype=dtype, device=dev),
                               L0, L1).double()
    first = out[0][1][kind]
    rec[kind] = dict(
        iterations=first['iterations'], status=first['status'],
        true_residual=float(torch.linalg.vector_norm(r)) / bn,
        setup_s_per_rank=[round(out[q][1][kind]['setup_s'], 3)
                          for q in sorted(out)],
        **{k: v for k, v in first.items()
           if k in ('orders', 'coarse_steps', 'coarse_bounds', 'lam_max')})
  return rec


for name in os.environ.get('CASES', 'p4,p8,p11').split(','):
  rec = run_case(name)
  line = json.dumps(rec)
  print(line, flush=True)
  if out_path:
    with open(out_path, 'a') as fh:
      fh.write(line + '\n')
