"""GPU: `StokesSEM` (HIP path) vs the oracle and vs the analytic answers of
the reference's navier_stokes_test.py:79-358."""
import os
import numpy as np
import pytest
import torch

from oracle import sfem_oracle as O
from swirl_fem_amd.linalg.cg import cg
from swirl_fem_amd.navier_stokes.navier_stokes import (BCType, StokesSEM,
                                                       bdfk_coeffs,
                                                       extk_coeffs)
from tests import stokes_case as SC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ORDER, K, DT = 7, 3, 1e-3


def dev(x):
  return torch.as_tensor(np.ascontiguousarray(x), device=DEV)


def relerr(a, b):
  a = a.detach().cpu().numpy()
  return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def all_converged(*diags):
  """Every solve of every step of the driver runs ended 'converged'."""
  for d in diags:
    assert d['cg_status'] and all(
        s == ('converged', 'converged') for s in d['cg_status']), d['cg_status']


@pytest.fixture(scope='module')
def case():
  pm = SC.make_premesh()
  sem = StokesSEM.create(pm, {'boundary': (BCType.DIRICHLET, 0.0)},
                         order=ORDER, device=DEV)
  v, p = SC.staged_meshes(pm, ORDER)
  orc = O.StokesOracle(v, p, ORDER, v['physical_masks']['boundary'])
  return sem, orc, v, p


def test_coefficients_and_errors():
  np.testing.assert_allclose(bdfk_coeffs(3), [-1 / 3, 3 / 2, -3, 11 / 6],
                             atol=1e-12)
  np.testing.assert_allclose(extk_coeffs(2), [1, -3, 3], atol=1e-12)
  # exact rationals here, barycentric evaluation in the reference / oracle:
  # equal to rounding (the reference's own values carry ~1e-15)
  for k in range(1, 5):
    np.testing.assert_allclose(bdfk_coeffs(k), O.bdfk_coeffs(k), rtol=0,
                               atol=1e-13)
    np.testing.assert_allclose(extk_coeffs(k), O.extk_coeffs(k), rtol=0,
                               atol=1e-13)
  np.testing.assert_array_equal(bdfk_coeffs(2), [0.5, -2.0, 1.5])
  np.testing.assert_array_equal(extk_coeffs(3), [-1.0, 4.0, -6.0, 4.0])
  from swirl_fem_amd.core.interpolation import Nodes1D, NodeType
  from swirl_fem_amd.core.mesh_refiner import refine_premesh
  hi = refine_premesh(SC.make_premesh(2), Nodes1D.create(
      3, NodeType.GAUSS_LOBATTO_LEGENDRE))
  with pytest.raises(ValueError, match='order 1'):
    StokesSEM.create(hi, {}, order=3, device=DEV)


def test_operators_match_oracle(case):
  sem, orc, v, p = case
  rng = np.random.default_rng(0)
  nv, npr = len(v['node_coords']), len(p['node_coords'])
  assert sem.velocity.mesh.num_nodes == nv
  assert sem.pressure.pspace.mesh.num_nodes == npr
  u = rng.standard_normal((nv, 2))
  pr = rng.standard_normal(npr)
  ud, pd = dev(u), dev(pr)
  assert relerr(sem.velocity_mass_diag, orc.mass_diag) < 1e-12
  assert relerr(sem.velocity.diag_qqt, orc.diag_qqt) == 0.0
  assert relerr(sem.B(ud), orc.B(u)) < 1e-12
  assert relerr(sem.Bi(ud), orc.Bi(u)) < 1e-12
  assert relerr(sem.A(ud), orc.A(u)) < 1e-10
  assert relerr(sem.C(ud), orc.C(u)) < 1e-10
  assert relerr(sem.D(ud), orc.D(u)) < 1e-10
  assert relerr(sem.Dt(pd), orc.Dt(pr)) < 1e-10
  assert relerr(sem.E(pd, DT, K), orc.E(pr, DT, K)) < 1e-9
  assert relerr(sem.pressure.B(pd), orc.pB(pr)) < 1e-10
  assert relerr(sem.filter(ud, 0.05), orc.filter(u, 0.05)) < 1e-11
  assert relerr(sem.vorticity(ud), orc.vorticity(u)) < 1e-10
  assert relerr(sem.velocity.exchange(ud), orc.vexchange(u)) < 1e-14
  bdf = O.bdfk_coeffs(K)
  href = (bdf[-1] / DT) * orc.B(u) + 0.3 * orc.A(u)
  assert relerr(sem.H(ud, bdf[-1] / DT, 0.3), href) < 1e-10
  # local operators (no gather / scatter)
  ul = rng.standard_normal(sem.velocity.local_shape)
  assert relerr(sem.velocity.A_local(dev(ul)),
                orc.vs.stiffness_local(ul)) < 1e-10
  assert relerr(sem.velocity.B_local(dev(ul)), orc.vs.mass_local(ul)) < 1e-12
  assert relerr(sem.velocity.C_local(dev(ul)),
                orc.ov.convection_local(ul, ul)) < 1e-10


def _states(v, p, n):
  us, ps = zip(*[SC.reference_soln(v['node_coords'], p['node_coords'],
                                   t=i * DT) for i in range(n)])
  return [dev(x) for x in us], [dev(x) for x in ps]


def test_stokes_analytical_identities(case):
  """navier_stokes_test.py:79-222 thresholds."""
  sem, _, v, p = case
  us, ps = _states(v, p, K + 1)
  _, sigma = SC.soln_params()
  err = sem.velocity.exchange(sem.B(sigma * us[0]) + sem.A(us[0]) -
                              sem.Dt(ps[0]))
  assert float(err.abs().max()) < 1e-7
  assert float(sem.D(us[0]).abs().max()) < 1e-10
  bdf = bdfk_coeffs(K)
  du_dt = (1 / DT) * sum(float(c) * x for c, x in zip(bdf, us))
  err = sem.velocity.exchange(sem.B(du_dt) + sem.A(us[-1]) - sem.Dt(ps[-1]))
  assert float(err.abs().max()) < 1e-7
  hist, u = us[:-1], us[-1]
  ext = extk_coeffs(1)
  p_ext = sum(float(ext[-i]) * ps[:-1][-i] for i in range(1, len(ext) + 1))
  f = -(1 / DT) * sum(float(c) * x for c, x in zip(bdf[:-1], hist))
  b = sem.B(f) + sem.Dt(p_ext)
  H = lambda w: sem.H(w, float(bdf[-1]) / DT, 1.0)
  Q = lambda w: (DT / float(bdf[-1])) * sem.Bi(w)
  dp = ps[-1] - p_ext
  assert float(sem.velocity.exchange(H(u) - sem.Dt(dp) - b).abs().max()) < 1e-7
  assert float(sem.velocity.exchange(
      H(u) - H(Q(sem.Dt(dp))) - b).abs().max()) < 10 * DT ** 2
  u_star, _ = cg(H, b, M=sem.velocity.exchange, tol=1e-15)
  assert float(sem.velocity.exchange(H(u_star) - b).abs().max()) < 1e-12
  assert float((u_star - u + Q(sem.Dt(dp))).abs().max()) < 5 * DT ** 2


def test_stokes_one_step(case):
  """navier_stokes_test.py:323-358, and agreement with the oracle's step."""
  sem, orc, v, p = case
  us, ps = _states(v, p, K + 1)
  u, pr, aux = sem.stokes_one_step(us[:-1], ps[:-1], f=0, mu=1, dt=DT,
                                   time_order=K, alpha=0.05,
                                   project_out_nullspace=True, tol=1e-12,
                                   atol=1e-12)
  assert float((u - us[-1]).abs().max()) < 5 * DT ** 2
  assert float((pr - ps[-1]).abs().max()) < 50 * DT ** 2
  assert float(aux['u_star_info']['residual']) < 1e-7
  assert float(aux['dp_info']['residual']) < 1e-7
  assert aux['u_star_info']['status'] == 'converged', aux['u_star_info']
  assert aux['dp_info']['status'] == 'converged', aux['dp_info']
  uo, po, auxo = orc.stokes_one_step(
      [x.cpu().numpy() for x in us[:-1]], [x.cpu().numpy() for x in ps[:-1]],
      0, 1, DT, K, alpha=0.05, tol=1e-12, atol=1e-12)
  assert relerr(u, uo) < 1e-8
  assert np.abs(pr.cpu().numpy() - po).max() < 1e-7


# --------------------------------------------- drivers (BASELINE configs 3, 4)
def _staged(pm, order):
  return SC.staged_meshes(pm, order)


def test_lid_driven_cavity_steps_match_oracle():
  """Config 3 in small: 2D cavity, unstructured (jittered, permuted) quads,
  p=5, BDF3/EXT2, lid through u_boundary; three steps vs the oracle."""
  from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
  from swirl_fem_amd.examples import navier_stokes_driver as drv
  rng = np.random.default_rng(3)
  n, order = 4, 5
  pm = unit_cube_mesh(n, ndim=2)
  x = pm.node_coords.copy()
  inner = np.all((x > 1e-9) & (x < 1 - 1e-9), axis=1)
  x[inner] += 0.2 / n * rng.uniform(-1, 1, (int(inner.sum()), 2))
  pm = pm.replace(node_coords=x,
                  elements=pm.elements[rng.permutation(pm.num_elements)])
  sem, u, p, diag = drv.lid_driven_cavity(order=order, reynolds=100.0, dt=1e-3,
                                          steps=3, device=DEV, premesh=pm,
                                          tol=1e-11)
  assert all(s == ('converged', 'converged') for s in diag['cg_status']), \
      diag['cg_status']
  v, pp = _staged(pm, order)
  orc = O.StokesOracle(v, pp, order, v['physical_masks']['boundary'])
  xc = v['node_coords']
  lid = (xc[:, 1] > 1 - 1e-12).astype(float)
  ub = np.stack([lid * 16 * xc[:, 0] ** 2 * (1 - xc[:, 0]) ** 2,
                 np.zeros(len(xc))], axis=-1)
  us = (ub,) * 3
  ps = (np.zeros(len(pp['node_coords'])),) * 3
  Cus = (orc.C(ub),) * 3
  for _ in range(3):
    uo, po, Co, _ = O.navier_stokes_step(orc, us, ps, Cus, 100.0, 1e-3, 3,
                                         u_boundary=ub, tol=1e-11, atol=0.0)
    us, ps, Cus = us[1:] + (uo,), ps[1:] + (po,), Cus[1:] + (Co,)
  assert relerr(u, us[-1]) < 1e-7
  assert np.abs(p.cpu().numpy() - ps[-1]).max() < 1e-6 * max(
      1.0, np.abs(ps[-1]).max())
  # the lid value is kept on the boundary, the flow is discretely solenoidal
  bmask = v['physical_masks']['boundary']
  assert np.abs(u.cpu().numpy()[bmask] - ub[bmask]).max() < 1e-12
  assert diag['max_divergence'] < 1e-6


def test_taylor_green_3d_periodic():
  """Config 4 in small: 3D triply periodic box, operators vs the oracle and a
  few time steps (energy decays, divergence stays small)."""
  from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
  from swirl_fem_amd.examples import navier_stokes_driver as drv
  n, order = 3, 3
  sem, u, p, diag = drv.taylor_green(n=n, order=order, reynolds=50.0, dt=2e-2,
                                     steps=3, device=DEV, tol=1e-10)
  assert all(s == ('converged', 'converged') for s in diag['cg_status']), \
      diag['cg_status']
  e = diag['kinetic_energy']
  assert all(b < a for a, b in zip(e, e[1:]))
  assert e[-1] > 0.8 * e[0]
  assert diag['max_divergence'] < 1e-6
  pm = unit_cube_mesh(n, ndim=3, a=0.0, b=2 * np.pi, periodic_dims=(0, 1, 2))
  v, pp = _staged(pm, order)
  orc = O.StokesOracle(v, pp, order, np.zeros(len(v['node_coords']), bool))
  rng = np.random.default_rng(4)
  w = rng.standard_normal((len(v['node_coords']), 3))
  q = rng.standard_normal(len(pp['node_coords']))
  assert relerr(sem.A(dev(w)), orc.A(w)) < 1e-10
  assert relerr(sem.C(dev(w)), orc.C(w)) < 1e-10
  assert relerr(sem.D(dev(w)), orc.D(w)) < 1e-10
  assert relerr(sem.Dt(dev(q)), orc.Dt(q)) < 1e-10
  assert relerr(sem.Bi(dev(w)), orc.Bi(w)) < 1e-12
  assert relerr(sem.filter(dev(w)), orc.filter(w)) < 1e-11
  assert relerr(sem.velocity.exchange(dev(w)), orc.vexchange(w)) < 1e-13
  assert relerr(sem.E(dev(q), 1e-2, 3), orc.E(q, 1e-2, 3)) < 1e-9


def _taylor_green_oracle(pm, order, reynolds, dt, steps, time_order, tol):
  """The driver's Taylor-Green run restated with the oracle (dense Kronecker
  element matrices, un-fused CG): (u, p) after `steps` steps."""
  v, pp = _staged(pm, order)
  orc = O.StokesOracle(v, pp, order, np.zeros(len(v['node_coords']), bool))
  x = v['node_coords']
  u0 = np.stack([np.sin(x[:, 0]) * np.cos(x[:, 1]) * np.cos(x[:, 2]),
                 -np.cos(x[:, 0]) * np.sin(x[:, 1]) * np.cos(x[:, 2]),
                 np.zeros(len(x))], axis=-1)
  us = (u0,) * time_order
  ps = (np.zeros(len(pp['node_coords'])),) * time_order
  Cus = (orc.C(u0),) * time_order
  for _ in range(steps):
    uo, po, Co, _ = O.navier_stokes_step(orc, us, ps, Cus, reynolds, dt,
                                         time_order, tol=tol, atol=0.0)
    us, ps, Cus = us[1:] + (uo,), ps[1:] + (po,), Cus[1:] + (Co,)
  return us[-1], ps[-1]


def test_taylor_green_3d_p7_step_matches_oracle():
  """BASELINE config 4's workload at ITS order: 3D Taylor-Green vortex, p = 7
  velocity / Gauss pressure on 6^3 points, triply periodic 2^3 box, Re = 1600,
  BDF3 / EXT2, over-integrated convection on 10^3 points -- two full
  `navier_stokes_step`s (navier_stokes.py:350-458, datagen.py:90-102) against
  the oracle's.  At this order every fused kernel of the step is the
  instantiation config 4 runs (facet / chain Helmholtz at P = 8, D and D^T
  with a P = 6 pressure space, the two-grid convection)."""
  from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
  from swirl_fem_amd.examples import navier_stokes_driver as drv
  n, order, steps = 2, 7, 2
  kw = dict(reynolds=1600.0, dt=1e-3, steps=steps, time_order=3)
  sem, u, p, diag = drv.taylor_green(n=n, order=order, device=DEV, tol=1e-12,
                                     **kw)
  assert all(s == ('converged', 'converged') for s in diag['cg_status']), \
      diag['cg_status']
  pm = unit_cube_mesh(n, ndim=3, a=0.0, b=2 * np.pi, periodic_dims=(0, 1, 2))
  uo, po = _taylor_green_oracle(pm, order, tol=1e-12, **kw)
  assert relerr(u, uo) < 1e-8
  pg = p.cpu().numpy()
  assert np.abs(pg - po).max() < 1e-7 * max(1.0, np.abs(po).max())
  assert diag['max_divergence'] < 1e-6
  e = diag['kinetic_energy']
  assert e[-1] < e[0]


def test_config3_unstructured_fixture():
  """BASELINE config 3 in miniature: 4 x 4 quads, vertices
  jittered by +-0.2 h, random element order and random local orientations,
  p = 5 velocity / P-2 pressure, over-integration q = 8, Dirichlet walls with a
  moving lid through `u_boundary`: every operator and one full step against the
  oracle.  Only the four proper rotations are drawn here: a reflected element
  has det J < 0 (the reference keeps the sign, core/fespace.py:346), so the
  lumped mass of a node between a reflected and an unreflected element
  cancels and B^-1 -- hence E and the step -- is undefined for the reference
  too.  Reflections are covered at operator level in test_gpu_stokes_fused.py."""
  import itertools
  from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
  order, n = 5, 4
  rng = np.random.default_rng(2)
  pm = unit_cube_mesh(n, ndim=2)
  x = pm.node_coords.copy()
  inner = (x > 1e-9).all(1) & (x < 1 - 1e-9).all(1)
  x[inner] += 0.2 / n * rng.uniform(-1, 1, (int(inner.sum()), 2))
  rng3 = np.random.default_rng(3)
  orients = [(perm, axes) for perm in itertools.permutations(range(2))
             for r in range(3) for axes in itertools.combinations(range(2), r)
             if (int(perm != (0, 1)) + len(axes)) % 2 == 0]
  assert len(orients) == 4
  el = []
  for e in pm.elements[rng3.permutation(pm.num_elements)]:
    perm, axes = orients[rng3.integers(len(orients))]
    el.append(np.flip(e.reshape(2, 2).transpose(perm), axes).reshape(-1))
  pm = pm.replace(node_coords=x, elements=np.array(el, dtype=np.int32))
  bcs = {'boundary': (BCType.DIRICHLET, 0.0)}
  sem = StokesSEM.create(pm, bcs, order=order, device=DEV)
  assert sem._divgrad() is not None and sem._masked_operator() is not None
  v, p = SC.staged_meshes(pm, order)
  orc = O.StokesOracle(v, p, order, v['physical_masks']['boundary'])
  assert (orc.vs.jacdets > 0).all()
  nv, npr = len(v['node_coords']), len(p['node_coords'])
  u = rng.standard_normal((nv, 2))
  pr = rng.standard_normal(npr)
  ud, pd = dev(u), dev(pr)
  assert relerr(sem.A(ud), orc.A(u)) < 1e-10
  assert relerr(sem.C(ud), orc.C(u)) < 1e-10
  assert relerr(sem.D(ud), orc.D(u)) < 1e-10
  assert relerr(sem.Dt(pd), orc.Dt(pr)) < 1e-10
  assert relerr(sem.E(pd, DT, 2), orc.E(pr, DT, 2)) < 1e-9
  assert relerr(sem.H(ud, 3.0, 0.01), 3.0 * orc.B(u) + 0.01 * orc.A(u)) < 1e-10
  assert relerr(sem.filter(ud, 0.05), orc.filter(u, 0.05)) < 1e-11
  # one Stokes step with the regularised lid as boundary velocity
  xc = v['node_coords']
  lid = (xc[:, 1] > 1 - 1e-12).astype(np.float64)
  ub = np.stack([lid * 16 * xc[:, 0] ** 2 * (1 - xc[:, 0]) ** 2,
                 np.zeros(nv)], axis=-1)
  # a load vector lives on the free nodes only (rows of Dirichlet nodes are
  # removed from the system; a load there could never be balanced)
  f = 0.1 * rng.standard_normal((nv, 2)) * orc.interior
  us, ps = [ub, ub], [np.zeros(npr), np.zeros(npr)]
  ug, pg, _ = sem.stokes_one_step([dev(a) for a in us], [dev(a) for a in ps],
                                  f=dev(f), mu=0.01, dt=1e-3, time_order=2,
                                  u_boundary=dev(ub), tol=1e-10, atol=0.0)
  uo, po, _ = orc.stokes_one_step(us, ps, f, 0.01, 1e-3, 2, alpha=0.05,
                                  u_boundary=ub, tol=1e-10, atol=0.0)
  assert np.isfinite(uo).all() and np.abs(uo).max() < 10
  assert relerr(ug, uo) < 1e-8
  assert np.abs(pg.cpu().numpy() - po).max() < 1e-6 * max(1.0, np.abs(po).max())
  # the same step through the opt-in Schwarz pressure preconditioner: jittered,
  # reordered and rotated elements (its local solves work in each element's
  # own axes, as boxes: an approximation here), same answer, fewer iterations
  from swirl_fem_amd.navier_stokes import pressure_preconditioner as pc
  M = pc.make_pressure_preconditioner(sem, 'schwarz', 1e-3, 2)
  _, _, aux0 = sem.stokes_one_step([dev(a) for a in us], [dev(a) for a in ps],
                                   f=dev(f), mu=0.01, dt=1e-3, time_order=2,
                                   u_boundary=dev(ub), tol=1e-10, atol=0.0)
  us2, ps2, aux = sem.stokes_one_step(
      [dev(a) for a in us], [dev(a) for a in ps], f=dev(f), mu=0.01, dt=1e-3,
      time_order=2, u_boundary=dev(ub), tol=1e-10, atol=0.0,
      pressure_preconditioner=M)
  assert relerr(us2, uo) < 1e-8
  assert np.abs(ps2.cpu().numpy() - po).max() < 1e-6 * max(1.0, np.abs(po).max())
  assert 1.5 * aux['dp_info']['num_iterations'] < aux0['dp_info'][
      'num_iterations'], (aux['dp_info'], aux0['dp_info'])


def test_kept_solver_graphs_give_the_same_steps(monkeypatch):
  """Navier-Stokes steps with the recorded CG iterations kept across steps
  (default) equal the steps that record every solve anew."""
  from swirl_fem_amd.examples.navier_stokes_driver import navier_stokes_step
  pm = SC.make_premesh()

  def run(reuse):
    monkeypatch.setenv('SFEM_GRAPH_REUSE', reuse)
    sem = StokesSEM.create(pm, {'boundary': (BCType.DIRICHLET, 0.0)},
                           order=5, device=DEV)
    x = sem.velocity.mesh.node_coords
    u0 = torch.stack([torch.sin(np.pi * x[:, 0]) * torch.cos(np.pi * x[:, 1]),
                      -torch.cos(np.pi * x[:, 0]) * torch.sin(np.pi * x[:, 1])],
                     dim=1) * sem.velocity.interior_mask
    p0 = torch.zeros(sem.pressure.pspace.mesh.num_nodes, dtype=u0.dtype,
                     device=DEV)
    us, ps = (u0,) * 3, (p0,) * 3
    Cus = tuple(sem.C(u) for u in us)
    its = []
    for _ in range(4):
      u, p, Cu, aux = navier_stokes_step(sem, us, ps, Cus, reynolds=100.0,
                                         dt=1e-3, time_order=3, tol=1e-9,
                                         atol=0.0)
      us, ps, Cus = us[1:] + (u,), ps[1:] + (p,), Cus[1:] + (Cu,)
      its.append((aux['u_star_info']['num_iterations'],
                  aux['dp_info']['num_iterations']))
    kept = len(sem._cache.get('cg_workspaces', {}))
    return us[-1], ps[-1], its, kept

  u1, p1, it1, kept1 = run('1')
  u0_, p0_, it0, kept0 = run('0')
  assert kept1 == 2 and kept0 == 0
  # (sums by atomics: the last iteration of a solve may fall either way)
  assert all(abs(a - b) <= 2 for x, y in zip(it1, it0) for a, b in zip(x, y)), (
      it1, it0)
  assert relerr(u1, u0_.cpu().numpy()) < 1e-8
  assert relerr(p1, p0_.cpu().numpy()) < 1e-6


def test_pressure_projection_cuts_iterations():
  """Successive right-hand-side projection of the pressure solve
  (`stokes_one_step(pressure_projection=L)`, beyond the reference, opt-in).
  (1) The projection itself: right-hand sides in the span of earlier ones are
  solved by the guess alone, others start from their E-orthogonal projection.
  (2) In the stepper: same velocity and pressure as the unprojected run to
  the solver tolerance and never more pressure iterations; how many fewer
  depends on how smooth the pressure increments are in time (3D Taylor-Green
  from rest-consistent histories, 12 steps at 16^3: 221 -> 130..190 per step,
  `scripts/bench_ns.py` with SFEM_PRESSURE_PROJECTION=8)."""
  from swirl_fem_amd.examples import navier_stokes_driver as drv
  from swirl_fem_amd.navier_stokes import navier_stokes as ns
  kw = dict(n=4, order=5, reynolds=100.0, dt=2e-3, steps=10, time_order=3,
            device=DEV, tol=1e-9)
  sem0, u0, p0, d0 = drv.taylor_green(**kw)
  # (1) on the pressure operator of that stepper
  E = ns._PressureOperator(sem0, 2e-3, 3)
  M = ns._NullspaceProjection(sem0)
  g = torch.Generator(device=DEV).manual_seed(4)
  npr = p0.numel()
  rhs = [E(torch.randn(npr, dtype=p0.dtype, device=DEV, generator=g))
         for _ in range(3)]
  hist = ns._SolutionProjection(4)
  base = []
  for b in rhs:
    x0 = hist.guess(b)
    x, info = cg(E, b, x0=x0, M=M, tol=1e-9)
    assert info['status'] == 'converged', info
    base.append(info['num_iterations'])
    hist.update(x, x0, E)
  assert hist.count == 3
  G = hist.X[:3, 0] @ hist.W[:3, 0].t()            # E-orthonormal basis
  assert float((G - torch.eye(3, dtype=G.dtype, device=DEV)).abs().max()) < 1e-6
  b = 0.3 * rhs[0] - 1.7 * rhs[1] + 0.5 * rhs[2]   # in the span
  x, info = cg(E, b, x0=hist.guess(b), M=M, tol=1e-7)
  assert info['num_iterations'] <= 2, info
  assert info['status'] == 'converged', info
  xz, iz = cg(E, b, M=M, tol=1e-7)
  assert iz['num_iterations'] > 10
  assert iz['status'] == 'converged', iz
  mean0 = lambda t: t - t.mean()
  assert float((mean0(x) - mean0(xz)).abs().max()) < 1e-5 * float(
      mean0(xz).abs().max())
  # (2) in the stepper
  sem1, u1, p1, d1 = drv.taylor_green(pressure_projection=6, **kw)
  assert float((u1 - u0).abs().max()) < 1e-7 * float(u0.abs().max())
  assert float((mean0(p1) - mean0(p0)).abs().max()) < 1e-5 * float(
      mean0(p0).abs().max())
  all_converged(d0, d1)
  it0 = [b for _, b in d0['cg_iterations']]
  it1 = [b for _, b in d1['cg_iterations']]
  assert it1[0] == it0[0]                  # nothing to project onto yet
  assert all(a <= b + 2 for a, b in zip(it1, it0)), (it0, it1)
  assert abs(d1['kinetic_energy'][-1] - d0['kinetic_energy'][-1]) < 1e-8 * abs(
      d0['kinetic_energy'][-1])
  # the history lives in the stepper object, keyed by (dt, order, L)
  assert any(isinstance(k, tuple) and k and k[0] == 'pressure_projection'
             for k in sem1._cache)
  assert not any(isinstance(k, tuple) and k and k[0] == 'pressure_projection'
                 for k in sem0._cache)


def test_schwarz_pressure_preconditioner():
  """`pressure_preconditioner='schwarz'` (beyond the reference, opt-in through
  its hook navier_stokes.py:354, :449-452): element-wise fast diagonalisation
  of E's diagonal blocks + the exact piecewise-constant coarse operator.
  Same velocity and pressure as the reference's projection-only solve to the
  solver tolerance and fewer pressure iterations (1.3 - 1.6 x: WITHOUT overlap
  between the element subdomains that is what block Jacobi buys on this
  operator -- DESIGN 3.5); the local solve inverts the element blocks of a
  Cartesian mesh exactly and the coarse matrix is R_0 E R_0^T exactly."""
  from swirl_fem_amd.examples import navier_stokes_driver as drv
  from swirl_fem_amd.navier_stokes import navier_stokes as ns
  from swirl_fem_amd.navier_stokes import pressure_preconditioner as pc
  mean0 = lambda t: t - t.mean()
  kw = dict(n=4, order=5, reynolds=100.0, dt=2e-3, steps=4, time_order=3,
            device=DEV, tol=1e-9)
  sem0, u0, p0, d0 = drv.taylor_green(**kw)
  sem1, u1, p1, d1 = drv.taylor_green(pressure_preconditioner='schwarz', **kw)
  assert float((u1 - u0).abs().max()) < 1e-7 * float(u0.abs().max())
  assert float((mean0(p1) - mean0(p0)).abs().max()) < 1e-5 * float(
      mean0(p0).abs().max())
  all_converged(d0, d1)
  it0 = [b for _, b in d0['cg_iterations']]
  it1 = [b for _, b in d1['cg_iterations']]
  assert 1.15 * sum(it1) <= sum(it0), (it0, it1)
  # the pieces, on the stepper's own operator
  M = pc.make_pressure_preconditioner(sem1, 'schwarz', 2e-3, 3)
  assert M is pc.make_pressure_preconditioner(sem1, 'schwarz', 2e-3, 3)
  E = ns._PressureOperator(sem1, 2e-3, 3)
  g = torch.Generator(device=DEV).manual_seed(9)
  npr = p0.numel()
  a = torch.randn(npr, dtype=p0.dtype, device=DEV, generator=g)
  b = torch.randn(npr, dtype=p0.dtype, device=DEV, generator=g)
  # symmetric on the zero-sum vectors the solve lives in (the closing
  # nullspace projection r - (w . r / total) 1 is an oblique one; the
  # fixed-length coarse CG is linear to its own accuracy)
  a, b = mean0(a), mean0(b)
  lhs, rhs = float(torch.dot(M(a), b)), float(torch.dot(a, M(b)))
  assert abs(lhs - rhs) < 1e-6 * max(abs(lhs), abs(rhs))
  # the one-pass closing (element sums and the mean's shares out of the local
  # solve, `sfem_fdm_solve_sums` + `sfem_add_element_constants`) against the
  # pieces run one after the other
  assert M._fused_setup() is not None
  fused = M(a)
  saved, M._fused = M._fused, None
  pieces = M(a)
  M._fused = saved
  assert float((fused - pieces).abs().max()) < 1e-12 * float(
      pieces.abs().max())
  # Cartesian mesh: local_solve is the pseudo-inverse of E's diagonal blocks.
  # For r supported in ONE element with zero element mean, E_ee z = r there.
  r = torch.zeros(npr, dtype=p0.dtype, device=DEV)
  el = M.pel[5]
  r[el] = torch.randn(el.numel(), dtype=p0.dtype, device=DEV, generator=g)
  r[el] -= r[el].mean()
  z = M.local_solve(r)
  assert float((z - M.local_solve_torch(r)).abs().max()) < 1e-12 * float(
      z.abs().max())
  outside = z.clone()
  outside[el] = 0
  assert float(outside.abs().max()) == 0.0
  Ez = E(z)
  assert float((Ez[el] - Ez[el].mean() - r[el]).abs().max()) < 1e-8 * float(
      r.abs().max())
  # coarse operator = R_0 E R_0^T
  yc = torch.randn(M.pel.shape[0], dtype=p0.dtype, device=DEV, generator=g)
  fine = torch.zeros(npr, dtype=p0.dtype, device=DEV)
  fine[M.pel.reshape(-1)] = yc[:, None].expand(-1, M.pel.shape[1]).reshape(-1)
  want = E(fine)[M.pel].sum(dim=1)
  got = M.coarse_matvec(yc)
  assert float((got - want).abs().max()) < 1e-9 * float(want.abs().max())
  # a deformed Dirichlet mesh in 2D: fewer iterations, same answer
  kw2 = dict(n=6, order=5, reynolds=100.0, dt=1e-3, steps=3, device=DEV,
             tol=1e-9)
  _, ua, pa, da = drv.lid_driven_cavity(**kw2)
  _, ub, pb, db = drv.lid_driven_cavity(pressure_preconditioner='schwarz',
                                        **kw2)
  assert float((ub - ua).abs().max()) < 1e-7 * float(ua.abs().max())
  all_converged(da, db)
  ia = sum(b for _, b in da['cg_iterations'])
  ib = sum(b for _, b in db['cg_iterations'])
  assert ib <= ia, (da['cg_iterations'], db['cg_iterations'])


def test_mass_preconditioned_velocity_solve():
  """Opt-in `velocity_preconditioner='mass'` (beyond the reference's M = QQ^T
  for the stepper's Helmholtz solve): same step to the solver tolerance, a
  fraction of the iterations, and a stopping rule at least as strict as the
  reference's."""
  from swirl_fem_amd.examples.navier_stokes_driver import taylor_green
  from swirl_fem_amd.examples.navier_stokes_driver import navier_stokes_step
  from swirl_fem_amd.navier_stokes import navier_stokes as ns
  kw = dict(n=4, order=6, reynolds=400.0, dt=2e-3, steps=2, time_order=2,
            device=DEV, tol=1e-10)
  sem, u0, p0, d0 = taylor_green(**kw)
  os.environ['SFEM_VELOCITY_PC'] = 'mass'
  try:
    sem1, u1, p1, d1 = taylor_green(**kw)
  finally:
    del os.environ['SFEM_VELOCITY_PC']
  assert float((u1 - u0).abs().max()) <= 1e-8 * float(u0.abs().max())
  assert float((p1 - p0).abs().max()) <= 1e-6 * max(1.0, float(p0.abs().max()))
  all_converged(d0, d1)
  it0 = [v for v, _ in d0['cg_iterations']]
  it1 = [v for v, _ in d1['cg_iterations']]
  assert all(b * 3 <= a for a, b in zip(it0, it1)), (it0, it1)
  # M = (d_max / d) QQ^T: symmetric, and r . M r >= r . QQ^T r
  M = ns._MassPreconditioner(sem)
  g = torch.Generator(device=DEV).manual_seed(4)
  N = sem.velocity.mesh.num_nodes
  a = torch.randn(N, 3, dtype=torch.float64, device=DEV, generator=g)
  b = torch.randn(N, 3, dtype=torch.float64, device=DEV, generator=g)
  lhs, rhs = float((a * M(b)).sum()), float((b * M(a)).sum())
  assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)
  assert float((a * M(a)).sum()) >= float(
      (a * sem.velocity.exchange(a)).sum()) * (1 - 1e-12)


def test_schwarz_coarse_solve_by_fft_on_a_periodic_box(monkeypatch):
  """On a uniform, fully periodic box the coarse operator R_0 E R_0^T is a
  circulant stencil: the preconditioner applies its exact pseudo-inverse by two
  FFTs (found by checking E_0 itself, not assumed); a mesh with walls keeps
  the Chebyshev solve."""
  from swirl_fem_amd.common.premesh_commons import box_mesh, unit_cube_mesh
  from swirl_fem_amd.navier_stokes import pressure_preconditioner as pc
  from swirl_fem_amd.navier_stokes.navier_stokes import BCType, StokesSEM
  monkeypatch.setattr(pc, 'DENSE_COARSE_MAX', 0)
  g = torch.Generator(device=DEV).manual_seed(21)
  for pm in (box_mesh((4, 5, 3), (0.0,) * 3, (1.0, 2.0, 0.5),
                      periodic_dims=(0, 1, 2)),
             unit_cube_mesh(6, ndim=2, periodic_dims=(0, 1))):
    sem = StokesSEM.create(pm, {}, order=4, device=DEV)
    M = pc.SchwarzPressurePreconditioner(sem, 1e-2, 2)
    assert M.E0_fft is not None and M.E0_pinv is None
    E = M.pel.shape[0]
    dense = torch.zeros(E, E, dtype=torch.float64, device=DEV)
    dense.scatter_add_(1, M.E0_cols, M.E0_vals.double())
    pinv = torch.linalg.pinv(dense, hermitian=True, rtol=1e-10)
    b = torch.randn(E, dtype=torch.float64, device=DEV, generator=g)
    want = pinv @ b
    got = M._coarse_solve(b)
    assert float((got - want).abs().max()) <= 1e-9 * float(want.abs().max())
    # ... and the whole preconditioner stays symmetric on zero-sum vectors
    n = sem.pressure.pspace.mesh.num_nodes
    a = torch.randn(n, dtype=torch.float64, device=DEV, generator=g)
    c = torch.randn(n, dtype=torch.float64, device=DEV, generator=g)
    a, c = a - a.mean(), c - c.mean()
    lhs, rhs = float(torch.dot(M(a), c)), float(torch.dot(a, M(c)))
    assert abs(lhs - rhs) <= 1e-9 * max(abs(lhs), abs(rhs))
  walls = StokesSEM.create(unit_cube_mesh(6, ndim=2),
                           {'boundary': (BCType.DIRICHLET, 0.0)}, order=4,
                           device=DEV)
  assert pc.SchwarzPressurePreconditioner(walls, 1e-2, 2).E0_fft is None
  half = StokesSEM.create(unit_cube_mesh(6, ndim=2, periodic_dims=(0,)),
                          {'boundary': (BCType.DIRICHLET, 0.0)}, order=4,
                          device=DEV)
  assert pc.SchwarzPressurePreconditioner(half, 1e-2, 2).E0_fft is None
