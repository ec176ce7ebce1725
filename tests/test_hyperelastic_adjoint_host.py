"""Host tests (no GPU) of the adjoint side of neo-Hookean elasticity (DESIGN
§3.21): the NumPy reference `tests/hyperelastic_adjoint_reference.py` against
the residual it differentiates (linearity in the coefficients), against the
linear sensitivities in the small-strain limit, its nodal and grid forms
against each other, the dense adjoint against its own central differences, and
what `solve_hyperelasticity` decides about autograd before any kernel runs."""
import inspect

import numpy as np
import pytest
import torch

from swirl_fem_amd.core import operators
from swirl_fem_amd.examples.hyperelasticity import BCType
from swirl_fem_amd.examples.hyperelasticity import solve_hyperelasticity
from tests import elasticity_adjoint_reference as EA
from tests import elasticity_reference as ER
from tests import hyperelastic_adjoint_reference as HA
from tests import hyperelastic_reference as HR

SCALE = 0.3      # the largest |H| of a random field
MIN_J = 0.3
CASES = [(2, 3, 4), (2, 4, 6), (3, 3, 4)]      # (ndim, P, Q)


def _space(ndim, P, Q):
  rp = ER.jittered_box(2, ndim, P)
  return HR.space(rp.node_coords, rp.elements, P, (Q, 'gl'))


def _grid_field(fes, rng):
  """A random field on the grid with max |H| = SCALE; min J asserted."""
  uq = rng.standard_normal((fes.num_elements, fes.Q, fes.ndim))
  uq *= SCALE / HR.max_gradient_norm(fes, uq)
  assert HR.min_jacobian(fes, uq) >= MIN_J
  return uq


def _coefs(fes, rng):
  shape = (fes.num_elements, fes.Q)
  return tuple(0.5 + rng.random(shape) for _ in range(3))


@pytest.mark.parametrize('ndim,P,Q', CASES)
def test_linearity_identity(ndim, P, Q):
  """P is linear in (lam, mu, rho): sum_q (lam s_lam + mu s_mu + rho s_rho)
  from `grid_sens`, fed the state of `HR.grid_residual`, equals v_q . r_q of
  that residual to 1e-12 relative to |v| |r|, for per-point and scalar
  coefficients, with and without the mass term."""
  fes = _space(ndim, P, Q)
  rng = np.random.default_rng(ndim + P)
  uq = _grid_field(fes, rng)
  vq = rng.standard_normal(uq.shape)
  for lam, mu, rho in (_coefs(fes, rng), (1.3, 0.7, 1.5)):
    for l0 in (0.0, 1.7):
      rq, state, _ = HR.grid_residual(fes, uq, lam, mu, rho, l0)
      sl, sm, sr = HA.grid_sens(fes, vq, state, uq, l0)
      got = float((lam * sl + mu * sm + rho * sr).sum())
      want = float((vq * rq).sum())
      scale = np.linalg.norm(vq) * np.linalg.norm(rq)
      print(f'{ndim}D Q={Q} lambda0={l0}: |sum - v.r| / (|v||r|) = '
            f'{abs(got - want) / scale:.2e}')
      assert abs(got - want) <= 1e-12 * scale
      if not l0:
        assert not sr.any()
  # without u the density output is absent and the others are unchanged
  sl2, sm2, none = HA.grid_sens(fes, vq, state, None, 1.7)
  assert none is None and np.array_equal(sl, sl2) and np.array_equal(sm, sm2)


@pytest.mark.parametrize('ndim,P,Q', CASES)
def test_small_strain_limit(ndim, P, Q):
  """For u -> eps u the sensitivities divided by eps tend to those of the
  linear operator (`EA.grid_sens`) at first order: the relative difference is
  at most 100 eps (the coefficient is a few times |H| = 0.3 of the unscaled
  field, as in the forward test) and falls by ten, within [5, 20], from eps =
  1e-3 to 1e-4.  The density term is linear in u and agrees to rounding."""
  fes = _space(ndim, P, Q)
  rng = np.random.default_rng(10 + ndim)
  uq = _grid_field(fes, rng)
  vq = rng.standard_normal(uq.shape)
  l0 = 1.3
  want = EA.grid_sens(fes, uq, vq, l0)
  rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()
  errs = {}
  for eps in (1e-3, 1e-4):
    state = HR.state(HR.grid_gradients(fes, eps * uq))
    got = HA.grid_sens(fes, vq, state, eps * uq, l0)
    errs[eps] = [rel(g / eps, w) for g, w in zip(got, want)]
    print(f'{ndim}D Q={Q} eps={eps}: dlam {errs[eps][0]:.2e}, dmu '
          f'{errs[eps][1]:.2e}, drho {errs[eps][2]:.2e}')
    assert errs[eps][0] <= 100 * eps and errs[eps][1] <= 100 * eps
    assert errs[eps][2] <= 1e-13
  for n in (0, 1):
    assert 5.0 <= errs[1e-3][n] / errs[1e-4][n] <= 20.0


@pytest.mark.parametrize('ndim,P,Q', CASES)
def test_nodal_and_grid_forms_agree(ndim, P, Q):
  """`point_sensitivities` of nodal fields (physical gradients of the basis)
  and `grid_sens` of the same fields interpolated to the grid, with the state
  of the grid residual, agree to 1e-11: the grid's derivative of the
  interpolant is exact (Q >= P)."""
  fes = _space(ndim, P, Q)
  rng = np.random.default_rng(20 + ndim)
  u = rng.standard_normal((fes.num_nodes, ndim))
  H = HR.gradients(fes, fes.gather(u))
  u *= SCALE / np.sqrt((H * H).sum((-2, -1))).max()
  v = rng.standard_normal(u.shape)
  grid = lambda w: np.einsum('qi,eic->eqc', fes.M, fes.gather(w))
  _, state, _ = HR.grid_residual(fes, grid(u), 1.0, 1.0)
  want = HA.point_sensitivities(fes, u, v, 0.9)
  got = HA.grid_sens(fes, grid(v), state, grid(u), 0.9)
  for g, w in zip(got, want):
    assert np.abs(g - w).max() <= 1e-11 * np.abs(w).max()


@pytest.mark.parametrize('ndim,lambda0', [(2, 0.0), (2, 1.7), (3, 1.7)])
def test_dense_adjoint_matches_central_differences(ndim, lambda0):
  """The dense adjoint gradient against the reference's own central
  difference, h = 1e-3, one relative one-signed direction per coefficient, to
  1e-5 (`HA.CD_BOUND`, reasoned at `HA.CD_H`); the reference solution is in the
  finite-strain regime (max |H| >= 0.1, min J >= 0.3) and converged to a
  relative residual of 1e-12.  Measured, relative: 2D lambda0 = 0: lam 3.1e-7,
  mu 6.3e-7; 2D lambda0 = 1.7: lam 2.5e-7, mu 4.4e-7, rho 4.0e-8; 3D lambda0 =
  1.7: lam 2.5e-7, mu 2.3e-7, rho 5.1e-6 (the truncation h^2 f''' / (6 f'),
  which quarters when h halves).  These are the floor the GPU central
  differences are held to ten times of."""
  prob = HA.SolveProblem(ndim, lambda0)
  hmax, jmin = prob.strain_measures()
  res = prob.relative_residual(prob.solution())
  print(f'ndim={ndim} lambda0={lambda0}: max |H| {hmax:.3f}, min J {jmin:.3f}, '
        f'relative residual {res:.2e}')
  assert hmax >= 0.1 and jmin >= 0.3
  assert res <= 1e-12
  cds = HA.central_differences(prob)
  assert set(cds) == ({'lam', 'mu', 'rho'} if lambda0 else {'lam', 'mu'})
  for name, (rel, _, an) in cds.items():
    print(f'  {name}: central difference vs analytic {rel:.2e} (directional '
          f'derivative {an:.3e})')
    assert rel <= HA.CD_BOUND, (ndim, name, rel)
  # the force gradient: the loss is not linear in the force here
  _, gf, *_ = prob.gradients()
  df = np.random.default_rng(12).standard_normal(gf.shape)
  h = HA.CD_H
  cd = (prob.loss(force=prob.force + h * df) -
        prob.loss(force=prob.force - h * df)) / (2 * h)
  an = float((gf * df).sum())
  print(f'  force: central difference vs analytic {abs(cd - an) / abs(an):.2e}')
  assert abs(cd - an) <= HA.CD_BOUND * abs(an)
  if not lambda0:
    assert not prob.gradients()[4].any()


# ------------------------------------------------- what the keyword decides
@pytest.fixture(scope='module')
def cpu_mesh():
  from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
  from swirl_fem_amd.core.interpolation import Nodes1D, NodeType
  from swirl_fem_amd.core.mesh_refiner import refine_premesh
  from tests import bvp_reference as BR
  pm = unit_cube_mesh(2, ndim=2)
  side = lambda c: 'x0' if abs(c[0]) < 1e-9 else None
  pm = pm.replace(physical_groups=BR.boundary_groups(pm, side))
  return refine_premesh(pm, Nodes1D.create(
      3, NodeType.GAUSS_LOBATTO_LEGENDRE)).finalize(device='cpu')


def test_keyword_refusals(cpu_mesh):
  """Without `differentiable=True` inputs that require grad are refused and
  the message names the keyword; `u0` that requires grad is refused with and
  without it; the argument checks come first either way.  All of it before
  any kernel runs (the mesh is on the CPU)."""
  D = BCType.DIRICHLET
  clamp = {'x0': (D, (0.0, 0.0))}
  f = (0.0, -1.0)
  kw = dict(lame_lambda=1.0, lame_mu=1.0)
  grad = lambda v: torch.tensor(v, dtype=torch.float64, requires_grad=True)
  N = cpu_mesh.num_nodes
  for name, value in (('lame_lambda', grad(1.0)), ('lame_mu', grad(1.0)),
                      ('density', grad(1.0))):
    with pytest.raises(NotImplementedError, match='differentiable=True'):
      solve_hyperelasticity(cpu_mesh, f, clamp, **{**kw, name: value})
  with pytest.raises(NotImplementedError, match='differentiable=True'):
    solve_hyperelasticity(cpu_mesh, grad(f), clamp, **kw)
  u0 = torch.zeros((N, 2), dtype=torch.float64, requires_grad=True)
  for flag in (False, True):
    with pytest.raises(NotImplementedError, match='u0'):
      solve_hyperelasticity(cpu_mesh, f, clamp, u0=u0, differentiable=flag,
                            **kw)
    with pytest.raises(NotImplementedError, match='pmg'):
      solve_hyperelasticity(cpu_mesh, grad(f), clamp, preconditioner='pmg',
                            differentiable=flag, **kw)
    with pytest.raises(ValueError, match='load_steps'):
      solve_hyperelasticity(cpu_mesh, grad(f), clamp, load_steps=0,
                            differentiable=flag, **kw)
  # under no_grad nothing requires grad: the refusal does not fire, and the
  # next check does
  with torch.no_grad():
    with pytest.raises(ValueError, match='rigid-body'):
      solve_hyperelasticity(cpu_mesh, grad(f), {}, **kw)


def test_public_interface():
  """The keywords, the operator method and the binding exist with the
  documented defaults."""
  from swirl_fem_amd import _lib, _ops
  sig = inspect.signature(solve_hyperelasticity).parameters
  assert sig['differentiable'].default is False
  assert sig['adjoint_rtol'].default is None
  assert sig['differentiable'].kind is inspect.Parameter.KEYWORD_ONLY
  sens = inspect.signature(
      operators.HyperelasticOperator.sensitivity).parameters
  assert list(sens) == ['self', 'u', 'v', 'lambda0', 'want', 'linearization']
  assert sens['want'].default == (True, True, True)
  assert sens['linearization'].default is None and sens['lambda0'].default == 0.0
  names = [n for n, _ in _lib.HyperelasticSensArgs._fields_]
  assert names[:8] == ['v', 'state', 'u', 'wdet', 'dlam', 'dmu', 'drho',
                       'lambda0']
  assert names[8:] == [n for n, _ in _lib.ElasticitySensArgs._fields_][7:]
  assert callable(_ops.hyperelastic_sens)
  assert _lib.ABI_VERSION == 10


def test_struct_layout():
  """`sfem_hyperelastic_sens_args` in the header and its ctypes mirror: `v`,
  `state`, `u`, then the fields of `sfem_elasticity_sens_args` from `wdet` on
  in the same order; the ABI number is unchanged (a pure addition)."""
  import ctypes
  import os
  import re
  from swirl_fem_amd import _lib
  from tests.test_hyperelastic_host import _declared
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  text = open(os.path.join(root, 'include', 'sfem.h')).read()
  assert '#define SFEM_ABI_VERSION 10' in text
  names = _declared(text, 'sfem_hyperelastic_sens_args')
  sibling = _declared(text, 'sfem_elasticity_sens_args')
  assert names == ['v', 'state', 'u'] + sibling[2:]
  fields = _lib.HyperelasticSensArgs._fields_
  assert names == [f[0] for f in fields], (names, fields)
  kinds = dict(fields)
  for name in ('v', 'state', 'u', 'wdet', 'dlam', 'dmu', 'drho'):
    assert kinds[name] is _lib.c_ptr
  assert kinds['lambda0'] is _lib.c_dbl
  # one pointer more than the sibling
  assert ctypes.sizeof(_lib.HyperelasticSensArgs) == \
      ctypes.sizeof(_lib.ElasticitySensArgs) + 8
  sig = _lib.SIGNATURES['sfem_hyperelastic_sens']
  assert sig[0]._type_ is _lib.HyperelasticSensArgs and sig[1] is _lib.c_ptr
  assert re.search(r'int sfem_hyperelastic_sens\(const '
                   r'sfem_hyperelastic_sens_args\* args,\s*sfem_stream_t '
                   r'stream\);', text)
