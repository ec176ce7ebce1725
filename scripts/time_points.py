"""Times the point evaluator on a 32^3, p = 7, fp64 affine box
in two regimes, for 1 and 3 components:

  sensors   10^4 random points, about 0.3 per element
  resample  a uniform 256^3 grid, 512 points per element

Per regime: locate and plan-build time (host clock around a synchronise), and
for ev(u) and ev.transpose(w) the median / min / max over alternating rounds of
HIP-event timings next to a yardstick written here from torch operations
(`u[elements[element]]` contracted with the 1D basis matrices by einsum, and
`index_add_` for the transpose, in batches that fit the memory), plus the
achieved bytes per second against the byte model of DESIGN §3.15.

usage: python scripts/time_points.py [--n 32] [--p1 8] [--grid 256]
                                     [--rounds 7] [--out profiles/points.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from swirl_fem_amd.common.premesh_commons import unit_cube_mesh  # noqa: E402
from swirl_fem_amd.core import points as PT  # noqa: E402
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType  # noqa: E402
from swirl_fem_amd.core.mesh_refiner import refine_premesh  # noqa: E402

DEV = 'cuda:0'
BATCH = 1 << 17          # yardstick points per batch


def basis_matrices(nodes, bary, xi):
  """(M, d, P1): l_i(xi_a) in the product form, torch."""
  d = xi[:, :, None] - nodes[None, None, :]                    # (M, d, P1)
  P1 = nodes.numel()
  out = []
  for i in range(P1):
    keep = [k for k in range(P1) if k != i]
    out.append(bary[i] * d[:, :, keep].prod(dim=-1))
  return torch.stack(out, dim=-1)


def yard_eval(u, elements, element, xi, nodes, bary):
  """torch composition of ev(u) for found points: (M, C)."""
  P1 = nodes.numel()
  C = u.shape[1]
  out = torch.empty((element.numel(), C), dtype=u.dtype, device=u.device)
  for s in range(0, element.numel(), BATCH):
    e = element[s:s + BATCH].long()
    l = basis_matrices(nodes, bary, xi[s:s + BATCH])
    ul = u[elements[e].long()].reshape(-1, P1, P1, P1, C)
    out[s:s + BATCH] = torch.einsum('mijkc,mi,mj,mk->mc', ul, l[:, 0], l[:, 1],
                                    l[:, 2])
  return out


def yard_transpose(w, elements, element, xi, nodes, bary, num_nodes):
  """torch composition of ev.transpose(w): (N, C) by index_add_."""
  C = w.shape[1]
  out = torch.zeros((num_nodes, C), dtype=w.dtype, device=w.device)
  for s in range(0, element.numel(), BATCH):
    e = element[s:s + BATCH].long()
    l = basis_matrices(nodes, bary, xi[s:s + BATCH])
    vals = torch.einsum('mc,mi,mj,mk->mijkc', w[s:s + BATCH], l[:, 0], l[:, 1],
                        l[:, 2])
    out.index_add_(0, elements[e].long().reshape(-1), vals.reshape(-1, C))
  return out


def timed(fn):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(
      enable_timing=True)
  a.record()
  out = fn()
  b.record()
  b.synchronize()
  return a.elapsed_time(b) * 1e-3, out


def compare(ours, yard, rounds):
  """Alternating rounds after one warm-up of each: seconds, [ours, yard]."""
  ours(), yard()
  torch.cuda.synchronize()
  t = [[], []]
  for _ in range(rounds):
    t[0].append(timed(ours)[0])
    t[1].append(timed(yard)[0])
  return [dict(median=float(np.median(x)), min=float(min(x)),
               max=float(max(x))) for x in t]


def byte_model(plan, C, real=8):
  """(eval bytes, transpose bytes incl. the CSR assembly) of DESIGN §3.15."""
  F, K, S = plan.num_found, plan.chunk_elem.numel(), plan.seg_elem.numel()
  n, d, N = plan.elements.shape[1], plan.ndim, plan.num_nodes
  per_point = d * real + 8 + C * real
  ev = F * per_point + K * (n * 4 + n * C * real + 20)
  rows = S * n * C * real
  tr = F * per_point + S * 16 + rows                      # kernel
  tr += rows + S * n * 4 + (N + 1) * 8 + N * C * real     # sfem_scatter_csr
  return ev, tr


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--n', type=int, default=32)
  ap.add_argument('--p1', type=int, default=8)
  ap.add_argument('--grid', type=int, default=256)
  ap.add_argument('--sensors', type=int, default=10000)
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--out', default='profiles/points.jsonl')
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('time_points.py measures on the GPU; none is visible')
  rng = np.random.default_rng(0)
  pm = unit_cube_mesh(a.n, ndim=3)
  A = np.eye(3) + 0.1 * rng.uniform(-1, 1, (3, 3))
  pm = pm.replace(node_coords=pm.node_coords @ A.T)
  grid1 = Nodes1D.create(a.p1, NodeType.GAUSS_LOBATTO_LEGENDRE)
  mesh = refine_premesh(pm, grid1).finalize(device=DEV)
  nodes, bary = (torch.as_tensor(t, device=DEV)
                 for t in PT.basis_tables(grid1))
  N, E = mesh.num_nodes, mesh.num_elements
  dev = lambda x: torch.as_tensor(x, dtype=torch.float64, device=DEV)
  g = (np.arange(a.grid) + 0.5) / a.grid
  regimes = {
      'sensors': rng.uniform(0.0, 1.0, (a.sensors, 3)) @ A.T,
      'resample': np.stack(np.meshgrid(g, g, g, indexing='ij'),
                           -1).reshape(-1, 3) @ A.T,
  }
  os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
  with open(a.out, 'w') as fh:
    for name, pts in regimes.items():
      pts = dev(pts)
      PT.candidate_grid(mesh)                      # built once per mesh
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      loc = PT.locate_points(mesh, pts)
      torch.cuda.synchronize()
      t_locate = time.perf_counter() - t0
      t0 = time.perf_counter()
      ev = PT.PointEvaluator(mesh, loc.element, loc.xi)
      ev.plan.scatter_csr
      torch.cuda.synchronize()
      t_plan = time.perf_counter() - t0
      found = int(ev.found.sum())
      assert found == pts.shape[0], (found, pts.shape[0])
      for C in (1, 3):
        u = dev(rng.standard_normal((N, C)))
        w = dev(rng.standard_normal((pts.shape[0], C)))
        ya = lambda: yard_eval(u, mesh.elements, loc.element, loc.xi, nodes,
                               bary)
        yt = lambda: yard_transpose(w, mesh.elements, loc.element, loc.xi,
                                    nodes, bary, N)
        e_err = float((ev(u) - ya()).abs().max() / u.abs().max())
        t_err = float((ev.transpose(w) - yt()).abs().max() /
                      yt().abs().max())
        te = compare(lambda: ev(u), ya, a.rounds)
        tt = compare(lambda: ev.transpose(w), yt, a.rounds)
        be, bt = byte_model(ev.plan, C)
        row = dict(
            regime=name, n=a.n, P1=a.p1, dtype='float64', components=C,
            points=int(pts.shape[0]), elements=E, nodes=N,
            touched=int(ev.plan.seg_elem.numel()),
            chunks=int(ev.plan.chunk_elem.numel()),
            locate_s=t_locate, plan_s=t_plan,
            eval_s=te[0], eval_yardstick_s=te[1],
            transpose_s=tt[0], transpose_yardstick_s=tt[1],
            eval_model_bytes=be, transpose_model_bytes=bt,
            eval_bytes_per_s=be / te[0]['median'],
            transpose_bytes_per_s=bt / tt[0]['median'],
            transpose_rows_bytes=int(ev.plan.seg_elem.numel()) *
            mesh.num_nodes_per_element * C * 8,
            eval_vs_yardstick_rel=e_err, transpose_vs_yardstick_rel=t_err,
            rounds=a.rounds)
        fh.write(json.dumps(row) + '\n')
        fh.flush()
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
  main()
