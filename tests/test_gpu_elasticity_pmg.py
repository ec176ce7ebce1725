"""p-multigrid for elasticity on the GPU (`linalg/pmg_elasticity.py`,
`csrc/sfem_pmg_vec.hip`): the vector transfers, every level's operator, the
coarsest matrix, smoother and V-cycle against the NumPy restatement
(`tests/elasticity_pmg_reference.py`), PCG stopping on r.r,
`solve_elasticity(..., preconditioner=ElasticityPMultigrid)` against the dense
solve, the gradient through it, refusals.  Small meshes only.  Needs a real
MI355X."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from swirl_fem_amd import _lib
from swirl_fem_amd import _ops
from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import NodeType, Quadrature1D
from swirl_fem_amd.examples.elasticity import BCType, solve_elasticity
from swirl_fem_amd.linalg import pmg
from swirl_fem_amd.linalg import pmg_elasticity as PE
from swirl_fem_amd.linalg.cg import cg
from swirl_fem_amd.linalg.jacobi import JacobiPreconditioner
from swirl_fem_amd.linalg.pmg_elasticity import ElasticityPMultigrid
from tests import elasticity_pmg_reference as EP
from tests import elasticity_reference as ER
from tests import pmg_reference as R
from tests import transport_reference as TR

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64 = torch.float64
D, N = BCType.DIRICHLET, BCType.NEUMANN
GL = NodeType.GAUSS_LEGENDRE


def _np(t):
  return t.detach().double().cpu().numpy()


def _dev(a, dtype=F64):
  return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _rel(a, b):
  return float(np.abs(a - b).max() / np.abs(b).max())


def _space(mesh):
  d = mesh.ndim
  return FiniteElementSpace.create(mesh, Quadrature1D.create(
      num_points=mesh.order + (d + 1) // 2, quadrature_type=GL))


# ------------------------------------------------------ 1. vector transfers
PAIRS = sorted({(pc, pf) for p in range(2, 13)    # 12: 13 -> 7 points
                for pf, pc in zip(pmg.default_orders(p),
                                  pmg.default_orders(p)[1:])})
RUN_TIME_PAIRS = ((2, 7), (1, 4), (3, 9), (4, 12))


@pytest.mark.parametrize('ndim', [2, 3])
@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_vector_transfers_every_default_pair(ndim, dtype):
  """P exact on vector polynomials of degree <= p_c, equal to the NumPy
  transfer with clamp + roller flags, add mode, fixed fine components and
  <P x, y> = <x, P^T y>."""
  assert len(PAIRS) == 11
  for pc, pf in PAIRS:
    _check_transfer(ndim, dtype, pc, pf)


@pytest.mark.parametrize('ndim', [2, 3])
@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_vector_transfers_run_time_sizes(ndim, dtype):
  """Pairs outside the default schedules take the run-time-size kernels;
  (4, 12) has the 13 fine points of the largest compiled pair."""
  assert not set(RUN_TIME_PAIRS) & set(PAIRS)
  for pc, pf in RUN_TIME_PAIRS:
    _check_transfer(ndim, dtype, pc, pf)


def _check_transfer(ndim, dtype, pc, pf):
  tol = 1e-12 if dtype == torch.float64 else 1e-5
  n = 1 if ndim == 3 and pf > 8 else 2
  rp = R.box(n, ndim, pf + 1, 'sheared', seed=pf)
  x = np.asarray(rp.node_coords, np.float64)
  # the unit-box coordinates behind the shear of `pmg_reference.box`
  A = np.eye(ndim) + 0.3 * np.random.default_rng(pf).uniform(
      -1, 1, (ndim, ndim))
  unit = (x - 0.1) @ np.linalg.inv(A.T)
  fixed = EP.clamp_and_roller(unit)
  assert fixed[:, 1].sum() > fixed[:, 0].sum() > 0
  fmesh = rp.finalize(device=DEV, dtype=dtype)
  cmesh, celems = pmg.coarse_mesh(fmesh, pc)
  fel = fmesh.elements.to(torch.int64)
  Nf, Nc, d = fmesh.num_nodes, cmesh.num_nodes, ndim
  cfixed = PE.coarse_fixed(_dev(fixed, torch.bool), fel, celems, Nc, d, pf, pc)
  cidx = celems.to(torch.int32).contiguous()
  fidx = fel.to(torch.int32).contiguous()
  owner = pmg.owner_bits(fel, Nf)
  mat = _dev(pmg.interpolation_1d(pc, pf), dtype)
  ffix, cfix = PE.flag_bytes(_dev(fixed, torch.bool)), PE.flag_bytes(cfixed)
  none_f = torch.zeros(Nf, dtype=torch.uint8, device=DEV)
  none_c = torch.zeros(Nc, dtype=torch.uint8, device=DEV)
  args = (cidx, fidx, owner)
  sizes = (d, pc + 1, pf + 1)
  nan = lambda k: torch.full((k,), float('nan'), dtype=dtype, device=DEV)

  # polynomials of degree pc, another one per component (affine map)
  def poly(y):
    cols = [(c + 1.0) * y[:, 0] ** pc - 0.5 * y[:, c] * y[:, 1] ** max(
        pc - 1, 0) + 0.3 * (c + 1) for c in range(d)]
    return torch.stack(cols, dim=1)
  uc = poly(cmesh.node_coords.double()).to(dtype).reshape(-1).contiguous()
  want = poly(fmesh.node_coords.double()).reshape(-1)
  uf = nan(Nf * d)
  _ops.pmg_prolong_vec(uc, uf, *args, none_c, none_f, mat, *sizes)
  err = (uf.double() - want).abs().max() / want.abs().max()
  assert float(err) < 50 * tol, (pc, pf, float(err))

  # against the NumPy transfer, fixed components included
  _, celems_ref, cfixed_ref, Pm = EP.transfer(
      x, _np(fel).astype(np.int64), pf, pc, fixed)
  assert (celems_ref == _np(celems)).all()
  assert (cfixed_ref == cfixed.cpu().numpy()).all()
  g = torch.Generator(device='cpu').manual_seed(pf)
  a = torch.randn(Nc * d, generator=g, dtype=torch.float64)
  y = torch.randn(Nf * d, generator=g, dtype=torch.float64)
  ad = a.to(DEV, dtype)
  ref = Pm @ a.numpy()
  scale = np.abs(ref).max()
  fx = fixed.reshape(-1)
  uf = nan(Nf * d)
  _ops.pmg_prolong_vec(ad, uf, *args, cfix, ffix, mat, *sizes)
  assert np.abs(_np(uf) - ref).max() < tol * scale
  assert not _np(uf)[fx].any()              # store mode: fixed components 0
  # add mode: += P a, fixed fine components untouched
  uf2 = torch.full((Nf * d,), 7.0, dtype=dtype, device=DEV)
  _ops.pmg_prolong_vec(ad, uf2, *args, cfix, ffix, mat, *sizes, add=True)
  assert np.abs(_np(uf2) - (7.0 + ref)).max() < 2 * tol * max(scale, 7.0)
  assert (_np(uf2)[fx] == 7.0).all()
  # restriction: element-local values, then the fixed-order sum
  loc = nan(celems.numel() * d)
  _ops.pmg_restrict_vec(y.to(DEV, dtype), loc, *args, cfix, ffix, mat, *sizes)
  offsets, slots = cmesh.assembly_plan().csr()
  rc = _ops.scatter_csr(loc.view(-1, d), offsets, slots, Nc, ncomp=d)
  ref_t = Pm.T @ y.numpy()
  assert np.abs(_np(rc).reshape(-1) - ref_t).max() < tol * np.abs(ref_t).max()
  assert not _np(rc).reshape(-1)[cfixed_ref.reshape(-1)].any()
  lhs = float(np.dot(_np(uf), y.numpy()))
  rhs = float(np.dot(a.numpy(), _np(rc).reshape(-1)))
  assert abs(lhs - rhs) < 10 * tol * max(abs(lhs), 1.0)


# ------------------------------------------------------- 2. the hierarchy
def _hierarchy_problem(ndim, n, P, lambda0=0.5):
  """Clamp + roller on a `three_kinds` box; lambda per point, mu per element,
  so the coarse levels see the weighted means and the (E,) pass-through."""
  rp = TR.box_with_sides(n, ndim, P, three_kinds=True)
  mesh = rp.finalize(device=DEV)
  x = np.asarray(rp.node_coords, np.float64)
  fixed = EP.clamp_and_roller(x)
  fes = _space(mesh)
  E = mesh.num_elements
  mu_e = 1.0 + 0.5 * (np.arange(E) % 3)
  lam_fn = lambda y: 1.0 + 0.5 * y[..., 0] + 0.25 * y[..., 1] ** 2
  op = fes.elasticity_operator(_dev(fixed, torch.bool), lame_lambda=lam_fn,
                               lame_mu=_dev(mu_e))
  M = ElasticityPMultigrid(op, lambda0)
  ref = ER.space(x, rp.elements, P, (P - 1 + (ndim + 1) // 2, 'gl'))
  lam_q = lam_fn(ER.quad_points(ref))
  return rp, mesh, fixed, op, M, ref, lam_q, mu_e


@pytest.mark.parametrize('ndim,n,P', [(3, 3, 5), (2, 3, 8)])
def test_level_operators_and_coarsest_matrix(ndim, n, P):
  """Every level's fixed-order apply against `elasticity_reference.apply` on
  that level's own mesh and Gauss rule, to 1e-10; the ELL matrix of order 1
  against the dense assembly of its element matrices."""
  rp, mesh, fixed, op, M, ref, lam_q, mu_e = _hierarchy_problem(ndim, n, P)
  l0 = M.lambda0
  assert M.orders == pmg.default_orders(P - 1) and len(M.levels) >= 3
  lam_c = EP.element_means(ref, lam_q)
  rng = np.random.default_rng(3)
  last = None
  for l, lev in enumerate(M.levels):
    order = lev.mesh.order
    q = order + (ndim + 1) // 2
    assert lev.op.fespace.quadrature.num_points == q
    xl = _np(lev.mesh.node_coords)
    fes = ER.space(xl, lev.mesh.elements.cpu().numpy(), order + 1, (q, 'gl'))
    want_fixed = EP.clamp_and_roller(xl)
    assert (lev.fixed.cpu().numpy() == want_fixed).all()
    keep = (~want_fixed).astype(np.float64)
    lam = lam_q if l == 0 else lam_c
    u = rng.standard_normal((lev.N, ndim))
    want = ER.apply(fes, u, lam, mu_e[:, None], None, l0, keep)
    out = torch.full((lev.N * ndim,), float('nan'), dtype=F64, device=DEV)
    lev.apply(_dev(u).reshape(-1), out)
    err = _rel(_np(out).reshape(lev.N, ndim), want)
    print(f'{ndim}D level {l} (order {order}): rel err {err:.2e}')
    assert err <= 1e-10
    dg = ER.diagonal(fes, lam, mu_e[:, None], None, l0, keep).reshape(-1)
    dinv = np.where(dg > 0, 1.0 / np.where(dg > 0, dg, 1.0), 0.0)
    assert _rel(_np(lev.dinv), dinv) <= 1e-10
    last = (fes, lam, keep)
  # the coarsest matrix
  fes, lam, keep = last
  lev = M.levels[-1]
  assert lev.mesh.order == 1
  A = ER.assemble(fes, ER.element_matrices(fes, lam, mu_e[:, None], None, l0))
  k = keep.reshape(-1)
  A = A * k[:, None] * k[None, :]
  cols, vals = lev.ell_cols.cpu().numpy(), _np(lev.ell_vals)
  width, nrows = cols.shape
  assert nrows == lev.N * ndim and width <= (81 if ndim == 3 else 18)
  got = np.zeros_like(A)
  np.add.at(got, (np.tile(np.arange(nrows), width), cols.reshape(-1)),
            vals.reshape(-1))
  assert np.abs(got - A).max() <= 1e-10 * np.abs(A).max()
  assert _rel(_np(lev.ell_dinv), np.where(np.diag(A) > 0, 1.0 / np.where(
      np.diag(A) > 0, np.diag(A), 1.0), 0.0)) <= 1e-10


def _reference(rp, fixed, M, lam, mu, lambda0):
  """The NumPy hierarchy with the spectrum estimates of the GPU object."""
  b = M.spectral_bounds()
  return EP.Hierarchy(rp.node_coords, rp.elements, M.orders[0], fixed, lam, mu,
                      None, lambda0, orders=M.orders, degree=M.degree,
                      lam_max=b['lam_max'],
                      coarse=(M.coarse_steps,) + tuple(b['coarse']))


def _gpu_case(name, dtype=F64):
  rp, order, fixed, lam, mu, l0, b = EP.case(name)
  mesh = rp.finalize(device=DEV, dtype=dtype)
  co = lambda c: c if isinstance(c, float) else _dev(c, dtype)
  op = _space(mesh).elasticity_operator(
      _dev(fixed, torch.bool), lame_lambda=co(lam), lame_mu=co(mu))
  return rp, mesh, op, fixed, lam, mu, l0, b


@pytest.mark.parametrize('name,degree', [('3d_p4', 2), ('2d_p7', 3)])
def test_smoother_and_vcycle_match_numpy(name, degree):
  """Against the reference with the GPU's spectrum estimates, 1e-11; M is
  symmetric and positive; `bounds=` reproduces it; two calls are bitwise
  equal."""
  rp, mesh, op, fixed, lam, mu, l0, _ = _gpu_case(name)
  M = ElasticityPMultigrid(op, l0, smoother_degree=degree)
  H = _reference(rp, fixed, M, lam, mu, l0)
  n = mesh.num_nodes * mesh.ndim
  g = torch.Generator().manual_seed(1)
  free = torch.as_tensor(~fixed.reshape(-1))
  a = torch.randn(n, generator=g, dtype=F64) * free
  b = torch.randn(n, generator=g, dtype=F64) * free
  ad, bd = a.to(DEV), b.to(DEV)
  x = M.smooth(0, ad, from_zero=True).clone()
  ref = R.smooth(H.levels[0], a.numpy(), np.zeros(n), H.cheb[0])
  assert np.abs(_np(x) - ref).max() < 1e-12 * np.abs(ref).max()
  Ma = M(ad).clone()
  ref = H.vcycle(a.numpy())
  err = np.abs(_np(Ma) - ref).max() / np.abs(ref).max()
  print(f'{name}: V-cycle vs reference {err:.2e}')
  assert err < 1e-11
  assert torch.equal(M(ad), Ma)                      # bitwise reproducible
  Mb = M(bd).clone()
  lhs, rhs = float(torch.dot(Ma, bd)), float(torch.dot(ad, Mb))
  # each side is a sum of n products known to 1e-11 relative (above)
  assert abs(lhs - rhs) <= 1e-10 * float(Ma.norm() * bd.norm())
  assert float(torch.dot(ad, Ma)) > 0 and float(torch.dot(bd, Mb)) > 0
  M2 = ElasticityPMultigrid(op, l0, smoother_degree=degree,
                            bounds=M.spectral_bounds())
  assert M2.spectral_bounds() == M.spectral_bounds()
  assert M2.coarse_steps == M.coarse_steps
  assert torch.equal(M2(ad), Ma)
  with pytest.raises(ValueError, match='lam_max'):
    ElasticityPMultigrid(op, l0, bounds={'lam_max': [1.0] * 7,
                                         'coarse': (0.1, 1.0)})


# ------------------------------------------------------------------ 3. PCG
PCG_CASES = [c[0] for c in EP.CASES if c[4] <= 0.45]


def _flat_operator(op, l0):
  n, d = op.fespace.mesh.num_nodes, op.fespace.mesh.ndim
  return lambda v: op.apply(v.view(n, d), l0).reshape(-1)


@pytest.mark.parametrize('name', PCG_CASES)
def test_pcg_iterations_and_residual(name):
  """CG with the V-cycle on the rows of DESIGN §3.19 with nu <= 0.45:
  converged, the true residual within tol |b|, the iteration count within
  one of the reference's PCG with the same spectrum estimates, and at most a
  fifth of Jacobi's."""
  tol = 1e-8
  rp, mesh, op, fixed, lam, mu, l0, b = _gpu_case(name)
  A = _flat_operator(op, l0)
  bd = _dev(b)
  M = ElasticityPMultigrid(op, l0)
  x, info = cg(A, bd, tol=tol, M=M)
  assert info['status'] == 'converged'
  res = float((bd - A(x)).norm() / bd.norm())
  k = int(info['num_iterations'])
  H = _reference(rp, fixed, M, lam, mu, l0)
  k_ref = H.pcg(b, tol)[1]
  _, ij = cg(A, bd, tol=tol,
             M=JacobiPreconditioner(op.diagonal(l0).reshape(-1)))
  kj = int(ij['num_iterations'])
  print(f'{name}: pMG {k} (reference {k_ref}), Jacobi {kj}, true residual '
        f'{res:.2e}')
  assert ij['status'] == 'converged'
  assert res <= tol * 1.001
  assert abs(k - k_ref) <= 1
  assert 5 * k <= kj


def test_pcg_fp32():
  """The 2D order-4 row in float32 at tolerance 1e-5; the true residual is
  that of the float64 operator on the same mesh."""
  tol = 1e-5
  name = '2d_p4'
  rp, mesh, op, fixed, lam, mu, l0, b = _gpu_case(name, torch.float32)
  A = _flat_operator(op, l0)
  bd = _dev(b, torch.float32)
  M = ElasticityPMultigrid(op, l0)
  assert M.dtype == torch.float32 and M.levels[-1].ell_vals.dtype == M.dtype
  x, info = cg(A, bd, tol=tol, M=M)
  assert info['status'] == 'converged'
  _, _, op64, *_ = _gpu_case(name)
  b64 = bd.double()
  res = float((b64 - _flat_operator(op64, l0)(x.double())).norm() / b64.norm())
  _, ij = cg(A, bd, tol=tol,
             M=JacobiPreconditioner(op.diagonal(l0).reshape(-1)))
  k, kj = int(info['num_iterations']), int(ij['num_iterations'])
  print(f'fp32 {name}: pMG {k}, Jacobi {kj}, true residual {res:.2e}')
  assert res <= tol * 1.001
  assert 5 * k <= kj


# ------------------------------------------------- 4. solve_elasticity
def _facets(mesh, group):
  return mesh.boundary_facets[group].cpu().numpy().astype(np.int64)


SOLVE_RTOL = 1e-8


@functools.lru_cache(maxsize=None)
def _solve_problem(kind):
  """(rp, P, bcs, force, dense pieces, solve keywords) of a small 2D / 3D
  solve.  Kinds: 'cantilever' (clamped on x0 under its own weight, 3D),
  'traction' (clamp, roller on y0, traction on x1), 'contrast' (mu per
  element 1 / 100), 'shift' (lambda0 > 0 with a density)."""
  ndim = 3 if kind == 'cantilever' else 2
  P = 4 if ndim == 3 else 5
  rp = ER.jittered_box(2 if ndim == 3 else 3, ndim, P)
  x = np.asarray(rp.node_coords, np.float64)
  E = rp.elements.shape[0]
  fixed = np.zeros(x.shape, bool)
  fixed[np.abs(x[:, 0]) < 1e-9] = True
  bcs = {'x0': (D, (0.0,) * ndim)}
  force = np.zeros(ndim)
  force[1] = -1.0
  lam, mu, rho, l0 = 1.5, 0.8, None, 0.0
  trac = None
  if kind == 'traction':
    fixed[np.abs(x[:, 1]) < 1e-9, 1] = True
    bcs = {'y0': (D, (None, 0.0)), 'x0': (D, (0.0, 0.0))}
    trac = (0.7, -0.2)
  elif kind == 'contrast':
    mu = np.where(np.arange(E) % 2 == 0, 1.0, 100.0)
    lam = 2.0 * mu
  elif kind == 'shift':
    rho, l0 = 2.0, 3.0
  return rp, P, ndim, fixed, bcs, force, lam, mu, rho, l0, trac


def _per_point(c):
  """A per-element array as the (E, Q) callable `Dense` takes."""
  if np.ndim(c) == 0:
    return c
  return lambda xq: np.broadcast_to(np.asarray(c)[:, None], xq.shape[:2])


@pytest.mark.parametrize('kind', ['cantilever', 'traction', 'contrast',
                                  'shift'])
def test_solve_matches_dense_solve(kind):
  """`solve_elasticity` with the V-cycle against `Dense.solve`.  CG stops on
  the true residual |r| <= rtol |b|, so the error on the free dofs is at most
  |K^-1| rtol |b| = rtol |b| / lambda_min(K) in the 2-norm: that is the bound,
  with the 1e-10 of the operator's own rounding relative to |u|."""
  rp, P, ndim, fixed, bcs, force, lam, mu, rho, l0, trac = _solve_problem(kind)
  mesh = rp.finalize(device=DEV)
  x = np.asarray(rp.node_coords, np.float64)
  dense = ER.Dense(rp, P, _per_point(lam), _per_point(mu), rho, l0)
  tr = [] if trac is None else [(_facets(mesh, 'x1'), list(trac))]
  K, b, expand = dense.system(np.tile(force, (len(x), 1)), fixed, 0.0 * x, tr)
  w = np.linalg.solve(K, b)
  want = expand(w)
  if trac is not None:
    bcs = dict(bcs, x1=(N, trac))
  co = lambda c: c if c is None or np.ndim(c) == 0 else _dev(c)
  u, info = solve_elasticity(
      mesh, tuple(force), bcs, lame_lambda=co(lam), lame_mu=co(mu),
      density=rho, lambda0=l0, rtol=SOLVE_RTOL,
      preconditioner=ElasticityPMultigrid, return_info=True)
  assert info['status'] == 'converged'
  free = ~fixed.reshape(-1)
  err = np.linalg.norm((_np(u) - want).reshape(-1)[free])
  lmin = float(np.linalg.eigvalsh(K)[0])
  bound = SOLVE_RTOL * np.linalg.norm(b) / lmin + 1e-10 * np.linalg.norm(w)
  print(f'{kind}: {info["num_iterations"]} iterations, error '
        f'{err / np.linalg.norm(w):.2e} of |u|, bound '
        f'{bound / np.linalg.norm(w):.2e}')
  assert err <= bound
  assert not _np(u)[fixed].any()
  _, ij = solve_elasticity(
      mesh, tuple(force), bcs, lame_lambda=co(lam), lame_mu=co(mu),
      density=rho, lambda0=l0, rtol=SOLVE_RTOL, preconditioner='jacobi',
      return_info=True)
  assert info['num_iterations'] < ij['num_iterations']


def test_gradient_through_the_solve_equals_jacobi():
  """d/d mu_e of sum(u w) through the solve with the V-cycle (forward and
  adjoint solve both use it) against the same with 'jacobi'.  Both solve to
  rtol = 1e-10; a relative residual rtol leaves a relative error of at most
  kappa(K) rtol in u and in the adjoint, so the two gradients differ by at
  most 4 kappa rtol of their size (first order)."""
  rtol = 1e-10
  rp, P, ndim, fixed, bcs, force, lam, mu, rho, l0, _ = _solve_problem(
      'contrast')
  mesh = rp.finalize(device=DEV)
  x = np.asarray(rp.node_coords, np.float64)
  dense = ER.Dense(rp, P, _per_point(lam), _per_point(mu), rho, l0)
  K, _, _ = dense.system(np.tile(force, (len(x), 1)), fixed, 0.0 * x)
  ev = np.linalg.eigvalsh(K)
  kappa = float(ev[-1] / ev[0])
  w = _dev(np.random.default_rng(5).standard_normal(x.shape))
  grads, infos = {}, {}
  for pc in (ElasticityPMultigrid, 'jacobi'):
    mu_t = _dev(mu).requires_grad_(True)
    u, info = solve_elasticity(mesh, tuple(force), bcs, lame_lambda=_dev(lam),
                               lame_mu=mu_t, rtol=rtol, preconditioner=pc,
                               return_info=True)
    (u * w).sum().backward()
    assert info['status'] == 'converged'
    assert info['adjoint']['status'] == 'converged'
    grads[pc], infos[pc] = _np(mu_t.grad), info
  a, b = grads[ElasticityPMultigrid], grads['jacobi']
  diff = np.linalg.norm(a - b) / np.linalg.norm(b)
  print(f'gradient: pMG vs Jacobi {diff:.2e} (kappa {kappa:.2e}); adjoint '
        f'iterations {infos[ElasticityPMultigrid]["adjoint"]["num_iterations"]}'
        f' against {infos["jacobi"]["adjoint"]["num_iterations"]}')
  assert np.linalg.norm(b) > 0
  assert diff <= 4 * kappa * rtol
  assert (infos[ElasticityPMultigrid]['adjoint']['num_iterations'] <
          infos['jacobi']['adjoint']['num_iterations'])


# ------------------------------------------------------------- 5. refusals
def test_refusals_and_the_singular_case():
  rp = ER.jittered_box(2, 2, 5)
  mesh = rp.finalize(device=DEV)
  fes = _space(mesh)
  free = fes.elasticity_operator(None, lame_lambda=1.0, lame_mu=1.0)
  with pytest.raises(NotImplementedError, match='singular'):
    ElasticityPMultigrid(free, 0.0)
  with pytest.raises(NotImplementedError, match='singular'):
    ElasticityPMultigrid(fes.elasticity_operator(
        None, lame_lambda=1.0, lame_mu=1.0, density=0.0), 5.0)
  # lambda0 rho > 0 and nothing fixed: positive definite
  M = ElasticityPMultigrid(free, 2.0)
  r = torch.randn(mesh.num_nodes * 2, dtype=F64, device=DEV)
  assert float(torch.dot(r, M(r))) > 0
  assert not any(bool(l.fixed.any()) for l in M.levels)
  with pytest.raises(TypeError, match='ElasticityOperator'):
    ElasticityPMultigrid(fes.helmholtz_operator(None))
  with pytest.raises(ValueError, match=r'\(N d,\)'):
    M(r[:-1])
  with pytest.raises(ValueError, match='fall strictly'):
    ElasticityPMultigrid(free, 2.0, orders=[4, 3, 3, 1])
  # other schedules run: 4 -> 3 -> 1 takes run-time-size transfers
  M3 = ElasticityPMultigrid(free, 2.0, orders=[4, 3, 1])
  assert float(torch.dot(r, M3(r))) > 0


def test_entry_point_status_codes():
  """The raw entry points on bad arguments (nothing that is refused
  launches), and the wrappers' own checks."""
  ndim, pc, pf = 2, 2, 4
  rp = R.box(2, ndim, pf + 1, 'sheared')
  fmesh = rp.finalize(device=DEV)
  cmesh, celems = pmg.coarse_mesh(fmesh, pc)
  fel = fmesh.elements.to(torch.int64)
  Nf, Nc = fmesh.num_nodes, cmesh.num_nodes
  t = dict(
      uc=torch.zeros(Nc * ndim, dtype=F64, device=DEV),
      uf=torch.zeros(Nf * ndim, dtype=F64, device=DEV),
      cidx=celems.to(torch.int32).contiguous(),
      fidx=fel.to(torch.int32).contiguous(),
      owner=pmg.owner_bits(fel, Nf),
      cfix=torch.zeros(Nc, dtype=torch.uint8, device=DEV),
      ffix=torch.zeros(Nf, dtype=torch.uint8, device=DEV),
      mat=_dev(pmg.interpolation_1d(pc, pf)))
  loc = torch.zeros(celems.numel() * ndim, dtype=F64, device=DEV)
  lib = _lib.load()
  E = celems.shape[0]
  names = ('uc', 'uf', 'cidx', 'fidx', 'owner', 'cfix', 'ffix', 'mat')

  def call(restrict_=False, **over):
    """The prolongation uc -> uf, or the restriction uf -> loc (an override
    uc=None then stands for a null output)."""
    v = dict(t, E=E, ndim=ndim, pc=pc + 1, pf=pf + 1, dtype=_lib.SFEM_F64)
    v.update(over)
    if restrict_:
      v['uc'], v['uf'] = v['uf'], (None if v['uc'] is None else loc)
    p = [None if v[k] is None else ctypes.c_void_p(v[k].data_ptr())
         for k in names]
    if restrict_:
      return lib.sfem_pmg_restrict_vec(*p, v['E'], v['ndim'], v['pc'],
                                       v['pf'], v['dtype'], None)
    return lib.sfem_pmg_prolong_vec(*p, v['E'], v['ndim'], v['pc'], v['pf'],
                                    0, v['dtype'], None)
  for r in (False, True):
    assert call(r) == 0
    torch.cuda.synchronize()
    for over in (dict(ndim=1), dict(ndim=4), dict(pc=1), dict(pf=pc + 1),
                 dict(pf=14), dict(dtype=5), dict(E=-1), dict(E=2 ** 31)):
      assert call(r, **over) == -1, (r, over)
    assert b'pmg vector transfer' in lib.sfem_last_error()
    for k in names:
      assert call(r, **{k: None}) == -1, (r, k)
    assert b'null pointer' in lib.sfem_last_error()
    # nothing to do is not an error
    assert call(r, E=0, uc=None, uf=None, cfix=None, ffix=None) == 0
  torch.cuda.synchronize()
  # the wrappers
  args = [t[k] for k in names]
  sizes = (ndim, pc + 1, pf + 1)
  _ops.pmg_prolong_vec(*args, *sizes)
  bad = lambda k, v: [v if n == k else t[n] for n in names]
  with pytest.raises(TypeError, match='int32'):
    _ops.pmg_prolong_vec(*bad('cidx', celems), *sizes)
  with pytest.raises(TypeError, match='uint8'):
    _ops.pmg_prolong_vec(*bad('ffix', t['ffix'].to(torch.bool)), *sizes)
  with pytest.raises(ValueError, match='one dtype'):
    _ops.pmg_prolong_vec(*bad('mat', t['mat'].float()), *sizes)
  with pytest.raises(ValueError, match='per node'):
    _ops.pmg_prolong_vec(*bad('uf', t['uf'][:-1]), *sizes)
  with pytest.raises(ValueError, match='expected'):
    _ops.pmg_prolong_vec(*bad('owner', t['owner'][:-1]), *sizes)
  with pytest.raises(ValueError, match='rc_local'):
    _ops.pmg_restrict_vec(t['uf'], loc[:-1], *args[2:], *sizes)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    _ops.pmg_prolong_vec(*bad('uc', t['uc'].cpu()), *sizes)
  with pytest.raises(_lib.SfemError, match='pmg vector transfer'):
    _ops.pmg_prolong_vec(*args, 2, 1, 5)     # P_c = 1 point
