"""Cost of the elasticity stress kernels and of `ElasticityOperator.stress`
(DESIGN §3.18), one JSON line per variant (profiles/elasticity_stress.jsonl, or
OUT, is rewritten).

Size: that of `scripts/time_elasticity.py`: N^3 hex elements of order P,
affine box (default 32^3, p = 7), fp64 and fp32; the solve's Gauss rule, Q = P
+ 2 points per direction.  Per dtype, in one process, all variants in turn:

* kernels on the Q^3 grid: `sfem_elasticity_stress` with sigma alone
  ('sigma') and with the von Mises output ('sigma_vm');
  `sfem_elasticity_stress_vjp` with all outputs ('vjp_all') and with ubar
  alone ('vjp_ubar'); `sfem_elasticity_local` on the same arrays ('forward',
  scalar coefficients, lambda0 = 0).  `bytes_model`: what each must move --
  'sigma': d reals per point in, `wdet`, NV out; 'sigma_vm': one more out;
  'vjp_all': NV + d in, `wdet`, d + 2 out; 'vjp_ubar': NV in, `wdet`, d out;
  'forward': d in, d out, `wdet`.  `hbm_fraction`: that over the time, against
  8 TB/s.
* from nodal displacements (N, d): `op.stress(u, at='quadrature')`
  ('op_quadrature': gather, interpolation, kernel), `op.stress(u)` with lumped
  recovery ('op_nodes_lumped': plus W sigma, transposed interpolation, scatter,
  division) and the route a user had without the kernel ('composed': gather,
  `fes._basis` with gradients -- the stored (E, Q^3, d, d) tensor -- and torch
  arithmetic for the six stress slots).
`ratio_to_forward`: ms / 'forward' ms; `ratio_to_composed`: ms / 'composed' ms.
Variants alternate; ROUNDS rounds of REPS calls after a warm-up, HIP events,
the median round counts and every round is kept.
env: N (32), P (7), REPS (5), ROUNDS (5), OUT, DTYPES (fp64,fp32)."""
import json, os, sys
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
reps = int(os.environ.get('REPS', '5'))
rounds = int(os.environ.get('ROUNDS', '5'))
dtypes = os.environ.get('DTYPES', 'fp64,fp32').split(',')
out_path = os.environ.get('OUT', os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
    'elasticity_stress.jsonl'))
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


d, NV = 3, 6
rp = refine_premesh(unit_cube_mesh(N, ndim=d), Nodes1D.create(P + 1, GLL))
for name in dtypes:
  dt = {'fp64': torch.float64, 'fp32': torch.float32}[name]
  size = 8 if name == 'fp64' else 4
  mesh = rp.finalize(device=dev, dtype=dt)
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(
      P + (d + 1) // 2, GL))
  op = fes.elasticity_operator(lame_lambda=LAM, lame_mu=MU)
  assert [p['geo_mode'] for p in op.parts] == [1], 'expected an affine box'
  E, Q = mesh.num_elements, fes.quadrature.num_points
  nq = Q ** d
  base = {'N': N, 'p': P, 'Q': Q, 'dtype': name, 'elements': E,
          'nodes': mesh.num_nodes}
  uq = torch.randn((E, nq, d), dtype=dt, device=dev)
  sb = torch.randn((E, nq, NV), dtype=dt, device=dev)
  u = torch.randn((mesh.num_nodes, d), dtype=dt, device=dev)
  wd = op.point_weights()
  eye = torch.eye(d, dtype=dt, device=dev)
  args = (op.parts, op.host, d, Q, wd, LAM, MU)

  def composed():
    _, g = fes._basis(_ops.gather_rows(u, mesh.elements), False, True)
    H = g.transpose(-1, -2)                  # [e, q, c, j] = d u_c / d x_j
    tr = H.diagonal(dim1=-2, dim2=-1).sum(-1)
    S = LAM * tr[..., None, None] * eye + MU * (H + g)
    return torch.stack([S[..., 0, 0], S[..., 1, 1], S[..., 2, 2],
                        S[..., 0, 1], S[..., 0, 2], S[..., 1, 2]], dim=-1)
  fns = {
      'sigma': lambda: _ops.elasticity_stress(uq, *args),
      'sigma_vm': lambda: _ops.elasticity_stress(uq, *args, want=(True, True)),
      'vjp_all': lambda: _ops.elasticity_stress_vjp(sb, uq, *args),
      'vjp_ubar': lambda: _ops.elasticity_stress_vjp(
          sb, None, *args, want=(True, False, False)),
      'forward': lambda: _ops.elasticity_local(uq, *args),
      'op_quadrature': lambda: op.stress(u, at='quadrature'),
      'op_nodes_lumped': lambda: op.stress(u),
      'composed': composed,
  }
  reals = {'sigma': d + 1 + NV, 'sigma_vm': d + 1 + NV + 1,
           'vjp_all': NV + d + 1 + d + 2, 'vjp_ubar': NV + 1 + d,
           'forward': 2 * d + 1}
  ms, times = alternate(fns)
  for k in fns:
    rec = dict(base, variant=k, ms=round(ms[k], 4),
               ms_rounds=[round(t, 4) for t in times[k]],
               ratio_to_forward=round(ms[k] / ms['forward'], 4),
               ratio_to_composed=round(ms[k] / ms['composed'], 4))
    if k in reals:
      nb = size * E * nq * reals[k]
      rec.update(bytes_model=nb,
                 hbm_fraction=round(nb / (ms[k] * 1e-3) / HBM, 4))
    emit(rec)
  del uq, sb, u, op, fes, mesh, wd, fns
  torch.cuda.empty_cache()
