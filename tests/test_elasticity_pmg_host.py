"""p-multigrid for elasticity without a GPU: the NumPy restatement
(`tests/elasticity_pmg_reference.py`) on its own -- transfers, fixed flags,
the V-cycle as a matrix, the iteration counts of DESIGN §3.19 -- and what
`ElasticityPMultigrid` and `solve_elasticity(..., preconditioner=callable)`
check before they touch a device."""
import dataclasses
import functools
import os
import re

import numpy as np
import pytest
import torch

from swirl_fem_amd import _lib
from swirl_fem_amd.core import operators
from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import Nodes1D, NodeType, Quadrature1D
from swirl_fem_amd.examples.elasticity import BCType, solve_elasticity
from swirl_fem_amd.linalg import pmg
from swirl_fem_amd.linalg import pmg_elasticity as PE
from swirl_fem_amd.linalg.pmg_elasticity import ElasticityPMultigrid
from tests import elasticity_pmg_reference as EP
from tests import pmg_reference as R
from tests import transport_reference as TR


# ------------------------------------------------------------- transfers
@pytest.mark.parametrize('ndim,pf,pc', [(2, 4, 2), (2, 7, 3), (3, 4, 2),
                                        (3, 3, 1)])
def test_prolongation_is_exact_on_vector_polynomials(ndim, pf, pc):
  """On affine elements P reproduces every vector polynomial of degree <= p_c
  (each component another one), and nothing couples the components."""
  rp = R.box(2, ndim, pf + 1, 'sheared', seed=pf)
  x = np.asarray(rp.node_coords, np.float64)
  free = np.zeros(x.shape, bool)
  fine = EP.Level(x, np.asarray(rp.elements, np.int64), pf, free, 1.0, 1.0,
                  None, 0.0)
  coarse, P = EP.coarsen(fine, pc, 1.0, 1.0, None, 0.0)
  assert P.shape == (x.size, coarse.N * ndim)

  def poly(y):
    cols = [(c + 1.0) * y[:, 0] ** pc - 0.5 * y[:, c] * y[:, 1] ** (pc - 1) +
            0.3 * c for c in range(ndim)]
    return np.stack(cols, axis=1)
  got = (P @ poly(coarse.coords).reshape(-1)).reshape(x.shape)
  assert np.abs(got - poly(x)).max() <= 1e-12 * np.abs(poly(x)).max()
  # component c of the result depends on component c of the input alone
  u = np.zeros((coarse.N, ndim))
  u[:, 1] = np.random.default_rng(0).standard_normal(coarse.N)
  out = (P @ u.reshape(-1)).reshape(x.shape)
  assert np.abs(out[:, 1]).max() > 0.1
  assert not out[:, [c for c in range(ndim) if c != 1]].any()


@pytest.mark.parametrize('ndim,n,pf,pc', [(2, 3, 4, 2), (2, 2, 5, 1),
                                          (3, 2, 4, 2), (3, 2, 3, 1)])
def test_coarse_fixed_flags_match_the_planes(ndim, n, pf, pc):
  """Clamp on x = 0, roller (component 1) on y = 0: the facet rule per
  component gives the coarse nodes of those planes, in the module's torch
  code and in the reference; the flag bytes carry bit c for component c."""
  rp = EP.jittered_box(n, ndim, pf + 1)
  x = np.asarray(rp.node_coords, np.float64)
  el = np.asarray(rp.elements, np.int64)
  fixed = EP.clamp_and_roller(x)
  fine = EP.Level(x, el, pf, fixed, 1.0, 1.0, None, 0.0)
  coarse, P = EP.coarsen(fine, pc, 1.0, 1.0, None, 0.0)
  want = EP.clamp_and_roller(coarse.coords)
  assert want[:, 1].sum() > want[:, 0].sum() > 0
  assert (coarse.fixed == want).all()
  got = PE.coarse_fixed(torch.as_tensor(fixed), torch.as_tensor(el),
                        torch.as_tensor(coarse.elements), coarse.N, ndim, pf,
                        pc)
  assert (got.numpy() == want).all()
  bytes_ = PE.flag_bytes(got).numpy()
  assert bytes_.dtype == np.uint8
  assert (bytes_ == (want * (1 << np.arange(ndim))).sum(axis=1)).all()
  assert set(np.unique(bytes_)) == {0, 2, 2 ** ndim - 1}
  # fixed dofs are out of P on both sides
  dense = P.toarray()
  assert not dense[fixed.reshape(-1)].any()
  assert not dense[:, want.reshape(-1)].any()


# ---------------------------------------------------------------- V-cycle
@pytest.mark.parametrize('ndim,n,p,nu,l0', [(2, 2, 4, 0.3, 0.0),
                                            (2, 2, 3, 0.45, 2.0),
                                            (3, 1, 3, 0.3, 0.0)])
def test_vcycle_is_symmetric_positive_definite(ndim, n, p, nu, l0):
  rp = EP.jittered_box(n, ndim, p + 1)
  fixed = EP.clamp_and_roller(rp.node_coords)
  lam, mu = EP.lame(1.0, nu)
  H = EP.Hierarchy(rp.node_coords, rp.elements, p, fixed, float(lam),
                   float(mu), None, l0)
  M = H.operator()
  scale = np.abs(M).max()
  asym = np.abs(M - M.T).max()
  print(f'V-cycle {M.shape}: asymmetry {asym / scale:.2e}')
  assert asym <= 1e-13 * scale
  ev = np.linalg.eigvalsh(0.5 * (M + M.T))
  assert ev[0] > 0


# the reference run of the issue: (free dofs, plain, Jacobi, pMG, coarse
# steps) per row of EP.CASES.  It drew other random numbers (jitter and
# right-hand side), so the counts here may differ by an iteration or two:
# max(2, 5 %) is allowed.  The free dofs and the coarse polynomial's degree
# do not depend on them.
TABLE = {
    '2d_p4': (528, 215, 182, 11, 10),
    '2d_p7': (903, 339, 286, 18, 8),
    '2d_p4_contrast': (528, 887, 256, 12, 38),
    '2d_p4_nu045': (528, 343, 310, 22, 17),
    '2d_p4_shift': (528, 160, 133, 11, 5),
    '3d_p4': (1872, 311, 197, 12, 12),
    '3d_p3_uniform': (840, 213, 132, 16, 12),
    '3d_p4_nu049': (1872, 1097, 839, 63, 41),
}


@functools.lru_cache(maxsize=None)
def reference_counts(name):
  """(free, plain, Jacobi, pMG, coarse steps, true relative residual of the
  pMG solve) of a case, PCG stopping on r.r <= 1e-16 b.b."""
  rp, order, fixed, lam, mu, l0, b = EP.case(name)
  H = EP.Hierarchy(rp.node_coords, rp.elements, order, fixed, lam, mu, None,
                   l0)
  plain = H.pcg(b, 1e-8, precondition=False)[1]
  jac = H.pcg_jacobi(b, 1e-8)[1]
  x, k = H.pcg(b, 1e-8)
  res = np.linalg.norm(b - H.levels[0].apply(x)) / np.linalg.norm(b)
  return int((~fixed).sum()), plain, jac, k, H.coarse[0], res


@pytest.mark.parametrize('name', [c[0] for c in EP.CASES])
def test_reference_iteration_counts(name):
  free, plain, jac, k, steps, res = reference_counts(name)
  print(f'{name}: {free} free dofs, plain {plain}, Jacobi {jac}, pMG {k}, '
        f'{steps} coarse steps')
  t_free, t_plain, t_jac, t_k, t_steps = TABLE[name]
  assert free == t_free and steps == t_steps
  for got, want in ((plain, t_plain), (jac, t_jac), (k, t_k)):
    assert abs(got - want) <= max(2, round(0.05 * want)), (got, want)
  assert res <= 1e-8 * 1.001
  nu = next(c[4] for c in EP.CASES if c[0] == name)
  if nu <= 0.45:
    assert 5 * k <= jac


# ------------------------------------------------------ argument checks
P_ = 5


@pytest.fixture(scope='module')
def cpu_mesh():
  return TR.box_with_sides(2, 2, P_).finalize(device='cpu')


def _stub_operator(mesh):
  """An `ElasticityOperator` that holds the space of `mesh` and nothing of the
  device: enough for the checks that come before any kernel."""
  d = mesh.ndim
  fes = FiniteElementSpace.create(mesh, Quadrature1D.create(
      num_points=mesh.order + (d + 1) // 2,
      quadrature_type=NodeType.GAUSS_LEGENDRE))
  return operators.ElasticityOperator(fespace=fes, parts=[], host={}, lam=1.0,
                                      mu=1.0, rho=1.0)


def test_argument_checks(cpu_mesh):
  op = _stub_operator(cpu_mesh)
  assert cpu_mesh.order == 4
  for orders in ([4, 4, 1], [3, 1], [4, 2], [4, 2, 3, 1], [], [4, 1, 1]):
    with pytest.raises(ValueError, match='fall strictly from 4 to 1'):
      ElasticityPMultigrid(op, orders=orders)
  with pytest.raises(ValueError, match='smoother_degree'):
    ElasticityPMultigrid(op, smoother_degree=0)
  with pytest.raises(TypeError, match='ElasticityOperator'):
    ElasticityPMultigrid(object())
  fes = op.fespace
  with pytest.raises(TypeError, match='ElasticityOperator'):
    ElasticityPMultigrid(operators.HelmholtzOperator.__new__(
        operators.HelmholtzOperator))
  assert ElasticityPMultigrid.stops_on_residual is True
  assert ElasticityPMultigrid.capturable is False
  assert fes.mesh is cpu_mesh


def test_refusals():
  """Partitions, ensembles, periodic images, non-GLL nodes and padded
  elements: NotImplementedError before any device work."""
  from swirl_fem_amd.common.premesh_commons import unit_cube_mesh
  from swirl_fem_amd.core.mesh_refiner import refine_premesh
  from swirl_fem_amd.distributed import blocks
  gll = Nodes1D.create(P_, NodeType.GAUSS_LOBATTO_LEGENDRE)
  plain = refine_premesh(unit_cube_mesh(2, ndim=2), gll).finalize(device='cpu')
  part = blocks.build_block_partition(2, 3, (2, 1, 1), 0, device='cpu')
  with pytest.raises(NotImplementedError, match='partitioned'):
    ElasticityPMultigrid(_stub_operator(part.mesh))
  with pytest.raises(NotImplementedError, match='ensemble'):
    ElasticityPMultigrid(_stub_operator(plain.replicate(2)))
  periodic = refine_premesh(unit_cube_mesh(2, ndim=2, periodic_dims=(0,)),
                            gll).finalize(device='cpu')
  with pytest.raises(NotImplementedError, match='periodic'):
    ElasticityPMultigrid(_stub_operator(periodic))
  gl = refine_premesh(unit_cube_mesh(2, ndim=2), Nodes1D.create(
      P_, NodeType.GAUSS_LEGENDRE)).finalize(device='cpu')
  with pytest.raises(NotImplementedError, match='GLL'):
    ElasticityPMultigrid(_stub_operator(gl))
  rows = plain.elements.clone()
  rows[-1] = -1
  padded = dataclasses.replace(plain, elements=rows)
  with pytest.raises(NotImplementedError, match='padded'):
    ElasticityPMultigrid(_stub_operator(padded))


def test_solve_with_a_callable_on_cpu_meshes(cpu_mesh):
  """The callable spelling passes the argument check of `solve_elasticity`
  (only unknown strings and other objects are refused), its refusals come
  first as for every preconditioner, and 'pmg' names the new spelling."""
  D = BCType.DIRICHLET
  kw = dict(lame_lambda=1.0, lame_mu=1.0)
  clamp = {'x0': (D, (0.0, 0.0))}
  f = (0.0, -1.0)
  called = []

  def factory(op, lambda0):
    called.append((op, lambda0))
    raise AssertionError('not reached without a device')
  for pre in (ElasticityPMultigrid, factory,
              functools.partial(ElasticityPMultigrid, smoother_degree=3)):
    with pytest.raises(NotImplementedError, match='ensemble'):
      solve_elasticity(cpu_mesh.replicate(2), f, clamp, preconditioner=pre,
                       **kw)
    with pytest.raises(ValueError, match='rigid-body'):
      solve_elasticity(cpu_mesh, f, {}, preconditioner=pre, **kw)
    # past every check of the arguments: the first kernel refuses a CPU tensor
    with pytest.raises(RuntimeError, match='no CPU fallback'):
      solve_elasticity(cpu_mesh, f, clamp, preconditioner=pre, **kw)
  assert not called
  with pytest.raises(NotImplementedError, match='ElasticityPMultigrid'):
    solve_elasticity(cpu_mesh, f, clamp, preconditioner='pmg', **kw)
  for bad in ('ilu', 3, ('jacobi',)):
    with pytest.raises(ValueError, match='unknown preconditioner'):
      solve_elasticity(cpu_mesh, f, clamp, preconditioner=bad, **kw)


# ------------------------------------------------------- header and ABI
def test_header_and_bindings():
  """The two entry points are declared in the header with the argument lists
  of the ctypes bindings; the ABI number is unchanged (a pure addition)."""
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  text = open(os.path.join(root, 'include', 'sfem.h')).read()
  assert '#define SFEM_ABI_VERSION 10' in text and _lib.ABI_VERSION == 10
  kinds = {'void*': _lib.c_ptr, 'int32_t*': _lib.c_ptr, 'uint32_t*': _lib.c_ptr,
           'uint8_t*': _lib.c_ptr, 'int64_t': _lib.c_i64, 'int': _lib.c_i32,
           'sfem_stream_t': _lib.c_ptr}
  for name, nargs in (('sfem_pmg_prolong_vec', 15),
                      ('sfem_pmg_restrict_vec', 14)):
    m = re.search(r'int %s\((.*?)\);' % name, text, flags=re.S)
    assert m, name
    args = [a.strip() for a in m.group(1).split(',')]
    types = [kinds[a.replace('const ', '').rsplit(' ', 1)[0]] for a in args]
    assert len(args) == nargs
    assert _lib.SIGNATURES[name] == types, name
  # the flag bytes sit between the owner words and the matrix
  sig = re.search(r'int sfem_pmg_prolong_vec\((.*?)\);', text,
                  flags=re.S).group(1)
  names = [a.split()[-1] for a in sig.split(',')]
  assert names[4:8] == ['owner', 'cfix', 'ffix', 'mat']
  assert pmg.PMultigridPreconditioner._steps_for is \
      ElasticityPMultigrid._steps_for
