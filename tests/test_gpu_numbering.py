"""The fused Helmholtz operator, its assembly paths, the masked CG updates and
the solvers under other global node numberings (`tests/numbering_cases.py`),
against the fp64 oracle and against the same mesh in the refiner's numbering.

Every other GPU test meshes with `refine_premesh`, whose numbering keeps each
facet's nodes in one contiguous run.  Here the same geometry is renumbered
(lexicographic, reversed, random, ...), each numbering asserts which launch
path it reaches, and results are mapped back to the refiner numbering before
they are compared.  The solves check the TRUE residual ||b - A x|| from an
independent apply (the oracle), not CG's recursive one: the masked residual
updates of layered assembly (`sfem_cg_update_r_layered*`,
`sfem_cg_update_r_jacobi`) had skipped chunks that a lexicographic numbering
writes, and CG then reported convergence to a wrong answer.  Needs a real
MI355X."""
import numpy as np
import pytest
import torch

from oracle import sfem_oracle as O
from swirl_fem_amd import _lib, _ops
from swirl_fem_amd.core import operators
from swirl_fem_amd.core.fespace import FiniteElementSpace
from swirl_fem_amd.core.interpolation import NodeType, Quadrature1D
from swirl_fem_amd.linalg import cg as cg_mod
from tests import numbering_cases as NC
from tests.fp32util import F32Rng, f32_mesh, tolerance
from tests.test_layer_plan_host import host_facet_table

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64, F32 = torch.float64, torch.float32
LAMBDAS = ((0.0, 1.0), (0.6, 1.2), (1.0, 0.0))
# switches of each assembly path (as in tests/test_gpu_assembly_modes.py)
ENV = {'atomic': {'SFEM_FACET': '0'},
       'unsorted': {'SFEM_FACET': '0', 'SFEM_SORTED_SCATTER': '0'},
       'cluster': {}, 'colored': {},
       'facet': {'SFEM_CHAIN_LEN': '3'},
       'nochain': {'SFEM_CHAIN': '0'},
       'layered': {'SFEM_CHAIN_LEN': '2'}}


def _np(t):
  return t.detach().double().cpu().numpy()


def _relerr(a, b):
  a = _np(a) if isinstance(a, torch.Tensor) else a
  return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def oracle_diagonal(ofes, l0, l1, dirichlet=None):
  """diag(l0 B + l1 A) from the oracle's matrices and geometric factors
  (as in tests/test_gpu_jacobi.py, one element at a time: the (Q, n, d)
  gradients of every element at once do not fit at P = 12)."""
  wdet = ofes.jacdets * ofes.weights[None, :]                  # (E, Q)
  mass = np.einsum('eq,qi->ei', wdet, ofes.M ** 2)
  stiff = np.stack([
      np.einsum('q,qij->i', wdet[e],
                np.einsum('qid,qjd->qij', ofes.G, ofes.invjacs[e]) ** 2)
      for e in range(wdet.shape[0])])
  d = ofes.scatter(l0 * mass + l1 * stiff)
  if dirichlet is not None:
    d = d * (1.0 - dirichlet.astype(np.float64))
  return d


def _setenv(monkeypatch, path):
  for k, v in ENV[path].items():
    monkeypatch.setenv(k, v)


def _finalize(rp, dtype):
  mesh = rp.finalize(device=DEV, dtype=dtype)
  fes = FiniteElementSpace.create(
      mesh, Quadrature1D.create_from_nodes_1d(rp.gridpoints_1d))
  return mesh, fes


def _geometry(P):
  # (P >= 9 keeps multilinear elements on index rows: no curved-free mix
  # would then cover every element from a table)
  return 'three_kinds' if P <= 8 else 'affine_curved'


def _case(numbering, geometry, n, P, dtype):
  """(numbered case with float32-representable coordinates if fp32)."""
  c = NC.build(numbering, geometry, n, P)
  c.rp, c.base = f32_mesh(c.rp, dtype), f32_mesh(c.base, dtype)
  return c


def _check_paths(op, numbering, P, chains):
  """The operator built the launches its numbering is meant to reach."""
  facet, layered = NC.EXPECT[NC.kind(numbering)]
  fp = op.facet_parts
  if facet == 'none':
    assert fp is None, numbering
  else:
    assert fp is not None, numbering
    tabled = [('facet_table' in q) for q in fp]
    if facet == 'all':
      assert all(tabled), numbering
    else:
      assert any(tabled) and not all(tabled), numbering
    if chains and P <= 8:
      assert any('chains' in q for q in fp if 'facet_table' in q), numbering
    if not chains:
      assert not any('chains' in q for q in fp), numbering
  assert (op.layer_plan() is not None) == layered, numbering


# ------------------------------------------------------------ a. paths
PATH_CASES = [(num, 'affine', n, P)
              for num in ('refiner', 'lexicographic', 'lexicographic_yzx',
                          'reversed', 'reversed_lexicographic', 'random',
                          'half_random')
              for n, P in ((3, 6), (3, 8), (2, 12))] + [
                  ('far_stride', 'thin', 0, P) for P in (6, 8, 12)]


@pytest.mark.parametrize('numbering,geometry,n,P', PATH_CASES,
                         ids=[f'{c[0]}-p{c[3]}' for c in PATH_CASES])
def test_numbering_reaches_its_paths(numbering, geometry, n, P, monkeypatch):
  """Facet launches present / absent, layer plan or none, chains at P <= 8;
  the device facet table equals the host restatement where it accepts."""
  monkeypatch.setenv('SFEM_CHAIN_LEN', '2')
  c = _case(numbering, geometry, n, P, F64)
  mesh, fes = _finalize(c.rp, F64)
  bm = mesh.physical_masks['boundary']
  for mask in (bm, None):
    op = operators.HelmholtzOperator.create(fes, mask)
    _check_paths(op, numbering, P, True)
  mult = mesh.assembly_plan().multiplicity
  tab, ok = _ops.facet_table(mesh.elements, bm.to(torch.uint8).contiguous(),
                             mult, P)
  htab, hok = host_facet_table(c.rp.elements, P)
  assert np.array_equal(ok.cpu().numpy().astype(bool), hok)
  t = tab.cpu().numpy().astype(np.int64)[hok]
  assert np.array_equal(t[..., 0] & 0x3FFFFFFF, htab[hok][..., 0])
  assert np.array_equal(t[..., 1:], htab[hok][..., 1:])


# --------------------------------------------------- b. apply and diagonal
APPLY_NUMBERINGS = ('refiner', 'lexicographic', 'reversed_lexicographic',
                    'reversed', 'random', 'half_random')
PATHS = ('atomic', 'unsorted', 'cluster', 'colored', 'facet', 'nochain',
         'layered')
_P_OF = {'atomic': (5, 8, 12), 'unsorted': (5, 12, 6), 'cluster': (5, 8, 6),
         'colored': (6, 12, 5), 'facet': (6, 8, 12), 'nochain': (12, 6, 8),
         'layered': (8, 6, 12)}
APPLY_CASES = []
for i, num in enumerate(APPLY_NUMBERINGS):
  for j, path in enumerate(PATHS):
    P = _P_OF[path][(i + j) % 3]
    dtype = F64 if (i + j) % 2 == 0 else F32
    APPLY_CASES.append((num, path, P, dtype))
APPLY_CASES += [('far_stride', 'layered', 6, F64),
                ('far_stride', 'facet', 8, F64)]


def _apply(op, ud, l0, l1, path, layered):
  N = op.fespace.mesh.num_nodes
  if path == 'layered' and layered:
    ext = op.new_extended()
    op.apply_layered(ud, ext, l0, l1)
    return _ops.fold_layers(ext, N, op.layer_plan().layers)
  out = torch.full_like(ud, 1e3)       # every entry must be written
  return op.apply(ud, l0, l1, out=out)


def _create(fes, mask, path, numbering, P):
  assembly = path if path in ('cluster', 'colored') else 'atomic'
  op = operators.HelmholtzOperator.create(fes, mask, 'auto', assembly)
  if path in ('atomic', 'unsorted', 'cluster', 'colored'):
    assert op.facet_parts is None
    if path == 'cluster':
      assert all(p.get('cluster') is not None for p in op.parts)
    if path == 'colored':
      assert all(p.get('colored') for p in op.parts)
    sort = path == 'atomic' and P <= 8
    if path in ('atomic', 'unsorted'):
      assert all((p.get('shared_order') is not None) == sort
                 for p in op.parts)
  else:
    _check_paths(op, numbering, P, path != 'nochain')
  return op


@pytest.mark.parametrize(
    'numbering,path,P,dtype', APPLY_CASES,
    ids=[f'{c[0]}-{c[1]}-p{c[2]}-{"f64" if c[3] == F64 else "f32"}'
         for c in APPLY_CASES])
def test_apply_and_diagonal_match_oracle(numbering, path, P, dtype,
                                         monkeypatch):
  _setenv(monkeypatch, path)
  thin = numbering == 'far_stride'
  c = _case(numbering, 'thin' if thin else _geometry(P),
            0 if thin else (3 if P <= 8 else 2), P, dtype)
  mesh, fes = _finalize(c.rp, dtype)
  bmesh, bfes = _finalize(c.base, dtype)
  ofes = O.FESpace(c.rp.node_coords, c.rp.elements, (P, 'gll'), (P, 'gll'))
  tol = tolerance(dtype, P)
  N = mesh.num_nodes
  rng = F32Rng(len(numbering) * 31 + 7 * P + len(path))
  u = rng.standard_normal(N)
  ud = torch.as_tensor(u, device=DEV, dtype=dtype)
  ub = torch.as_tensor(c.to_base(u), device=DEV, dtype=dtype)
  bu = ofes.scatter(ofes.mass_local(ofes.gather(u)))
  au = ofes.scatter(ofes.stiffness_local(ofes.gather(u)))
  for masked in (True, False):
    mask = mesh.physical_masks['boundary'] if masked else None
    bmask = bmesh.physical_masks['boundary'] if masked else None
    if masked:    # the Dirichlet group went through the permutation
      assert np.array_equal(c.to_base(_np(mask)), _np(bmask))
    op = _create(fes, mask, path, numbering, P)
    bop = _create(bfes, bmask, path, 'refiner', P)
    layered = op.layer_plan() is not None
    keep = 1.0 if mask is None else 1.0 - _np(mask)
    for l0, l1 in LAMBDAS:
      what = (numbering, path, masked, l0, l1)
      ref = (l0 * bu + l1 * au) * keep
      got = _apply(op, ud, l0, l1, path, layered)
      assert _relerr(got, ref) < tol, what
      on_base = _apply(bop, ub, l0, l1, path, bop.layer_plan() is not None)
      assert _relerr(c.to_base(_np(got)), _np(on_base)) < tol, what
      d = op.diagonal(l0, l1)
      dref = oracle_diagonal(ofes, l0, l1, None if mask is None else _np(mask))
      assert _relerr(d, dref) < tol, what
      assert _relerr(c.to_base(_np(d)), _np(bop.diagonal(l0, l1))) < tol, what


# ------------------------------------------------- c. masked r updates
LAYERED = ('refiner', 'lexicographic', 'lexicographic_yzx', 'reversed',
           'reversed_lexicographic')
UPDATE_CASES = [(num, n, P, dtype) for num in LAYERED
                for n, P in ((4, 6), (4, 8), (3, 12)) for dtype in (F64, F32)]


@pytest.mark.parametrize(
    'numbering,n,P,dtype', UPDATE_CASES,
    ids=[f'{c[0]}-p{c[2]}-{"f64" if c[3] == F64 else "f32"}'
         for c in UPDATE_CASES])
def test_masked_r_updates(numbering, n, P, dtype, monkeypatch):
  """r -= alpha Ap from the layers of `apply_layered`: the three update
  kernels with `plan.masks` equal the unmasked ones bit for bit, and match
  r - alpha (l0 B + l1 A) u of the oracle."""
  monkeypatch.setenv('SFEM_CHAIN_LEN', '2')
  c = _case(numbering, 'affine' if P > 8 else 'vertex', n, P, dtype)
  mesh, fes = _finalize(c.rp, dtype)
  ofes = O.FESpace(c.rp.node_coords, c.rp.elements, (P, 'gll'), (P, 'gll'))
  tol = tolerance(dtype, P)
  N = mesh.num_nodes
  rng = F32Rng(5 * P + len(numbering))
  u, r0 = rng.standard_normal(N), rng.standard_normal(N)
  dinv = rng.uniform(0.5, 2.0, N)
  ud, rd = (torch.as_tensor(v, device=DEV, dtype=dtype) for v in (u, r0))
  dinvd = torch.as_tensor(dinv, device=DEV, dtype=dtype)
  bm = mesh.physical_masks['boundary']
  for mask in (bm, None):
    op = operators.HelmholtzOperator.create(fes, mask)
    _check_paths(op, numbering, P, True)
    plan = op.layer_plan()
    keep = 1.0 if mask is None else 1.0 - _np(mask)
    for l0, l1 in LAMBDAS:
      what = (numbering, mask is not None, l0, l1)
      ext = op.new_extended()
      op.apply_layered(ud, ext, l0, l1)
      ref = (l0 * ofes.scatter(ofes.mass_local(ofes.gather(u))) +
             l1 * ofes.scatter(ofes.stiffness_local(ofes.gather(u)))) * keep
      want = r0 - (1.0 / 3.0) * ref
      bound = 4 * tol * max(np.abs(want).max(), np.abs(ref).max())

      def scalars():
        s = torch.zeros(_lib.SFEM_CG_NSCALARS, dtype=torch.float64,
                        device=DEV)
        s[0], s[1] = 1.0, 3.0           # alpha = 1 / 3
        return s

      runs = {}
      for m in ('masked', 'plain'):
        masks = plan.masks if m == 'masked' else None
        r = rd.clone()
        _ops.cg_update_r_layered(r, ext, plan.layers, scalars(), 1,
                                 masks=masks)
        runs[('layered', m)] = (r,)
        r = rd.clone()
        parts = torch.zeros(cg_mod.RR_PARTIALS + _lib.SFEM_FOLD_GROUPS,
                            dtype=torch.float64, device=DEV)
        k = _ops.cg_update_r_layered_det(r, ext, plan.layers, scalars(),
                                         parts[:cg_mod.RR_PARTIALS],
                                         masks=masks)
        runs[('det', m)] = (r, parts[:k])
        r = rd.clone()
        _ops.cg_update_r_jacobi(r, ext, dinvd, scalars(), 1, plan.layers,
                                masks)
        runs[('jacobi', m)] = (r,)
        r = rd.clone()
        parts = torch.zeros(cg_mod.RR_PARTIALS + _lib.SFEM_FOLD_GROUPS,
                            dtype=torch.float64, device=DEV)
        k = _ops.cg_update_r_jacobi(r, ext, dinvd, scalars(), 1, plan.layers,
                                    masks, parts[:cg_mod.RR_PARTIALS])
        runs[('jacobi_det', m)] = (r, parts[:k])
      for kern in ('layered', 'det', 'jacobi', 'jacobi_det'):
        a, b = runs[(kern, 'masked')], runs[(kern, 'plain')]
        assert all(torch.equal(x, y) for x, y in zip(a, b)), what + (kern,)
        err = np.abs(_np(a[0]) - want).max()
        assert err <= bound, what + (kern, err)
      # the stored partial sums are r.r and r.(dinv r) of the updated r
      rn = _np(runs[('det', 'masked')][0])
      assert abs(float(runs[('det', 'masked')][1].sum()) - rn @ rn) <= (
          1e-12 if dtype == F64 else 1e-5) * (rn @ rn)
      rj = _np(runs[('jacobi_det', 'masked')][0])
      rz = rj @ (dinv * rj)
      assert abs(float(runs[('jacobi_det', 'masked')][1].sum()) - rz) <= (
          1e-12 if dtype == F64 else 1e-5) * rz


# ---------------------------------------------------------------- d. solves
SOLVE_NUMBERINGS = ('refiner', 'lexicographic', 'reversed_lexicographic',
                    'reversed', 'random', 'half_random')
SOLVE_CASES = [(num, dtype) for num in SOLVE_NUMBERINGS
               for dtype in (F64, F32)]
SOLVE_P, SOLVE_N = 6, 4
RTOL = {F64: 1e-10, F32: 1e-4}


def _split_boundary(rp):
  """'boundary' -> 'left' (the facets on x0 = 0: Neumann) and 'wall'."""
  facets = rp.physical_groups['boundary']
  left = (rp.node_coords[facets][..., 0] < 1e-9).all(axis=1)
  return rp.replace(physical_groups={'left': facets[left],
                                     'wall': facets[~left]})


def _solve_case(numbering, dtype):
  c = _case(numbering, 'vertex', SOLVE_N, SOLVE_P, dtype)
  c.base = _split_boundary(c.base)
  c.rp, _ = NC.renumber(c.base, c.perm)
  return c


_REFINER = {}


def _refiner_runs(dtype, monkeypatch):
  """The solves of `_run_solves` on the refiner numbering (once per dtype)."""
  if dtype not in _REFINER:
    _REFINER[dtype] = _run_solves(_solve_case('refiner', dtype), dtype,
                                  monkeypatch, check=False)
  return _REFINER[dtype]


def _oracle_two_grid(rp, P):
  return O.FESpace(rp.node_coords, rp.elements, (P, 'gll'), (P + 1, 'gl'))


def _run_solves(c, dtype, monkeypatch, check=True):
  """{name: (solution mapped to the refiner numbering, iterations)}; with
  `check`, every solve's true residual against its tolerance."""
  from swirl_fem_amd.examples.helmholtz import solve_helmholtz
  from swirl_fem_amd.examples.poisson import BCType, solve_poisson
  from swirl_fem_amd.linalg.cg import CGRunner, cg
  from swirl_fem_amd.linalg.jacobi import JacobiPreconditioner
  from swirl_fem_amd.linalg.pmg import PMultigridPreconditioner
  P, rtol = SOLVE_P, RTOL[dtype]
  mesh, fes = _finalize(c.rp, dtype)
  N = mesh.num_nodes
  rng = F32Rng(17)
  f_base = rng.standard_normal(N)
  f = c.from_base(f_base)
  fd = torch.as_tensor(f, device=DEV, dtype=dtype)
  wall = _np(mesh.physical_masks['wall']).astype(bool)
  left = _np(mesh.physical_masks['left']).astype(bool)
  assert wall.any() and left.any()
  o2 = _oracle_two_grid(c.rp, P)
  oco = O.FESpace(c.rp.node_coords, c.rp.elements, (P, 'gll'), (P, 'gll'))
  H2 = lambda v, l0, l1: (l0 * o2.scatter(o2.mass_local(o2.gather(v))) +
                          l1 * o2.scatter(o2.stiffness_local(o2.gather(v))))
  Hc = lambda v, l0, l1: (l0 * oco.scatter(oco.mass_local(oco.gather(v))) +
                          l1 * oco.scatter(oco.stiffness_local(oco.gather(v))))
  out = {}

  def true_residual(name, res, b):
    rel = np.linalg.norm(res) / np.linalg.norm(b)
    # CG stops on its recursive residual <= rtol ||b||; the true one may sit
    # a little above it from rounding, by far less than dropped terms put it
    slack = 3.0 if dtype == F64 else 10.0
    assert rel <= slack * rtol, (c.name, name, rel)

  keep_w = 1.0 - wall
  for pc in (None, 'jacobi', 'pmg'):
    # Poisson, homogeneous Dirichlet on the wall group
    x, info = solve_poisson(mesh, fd, {'wall': (BCType.DIRICHLET, 0.0)},
                            rtol=rtol, return_info=True, preconditioner=pc)
    xn = _np(x)
    if check:
      b = H2(f, 1.0, 0.0) * keep_w
      true_residual(('poisson', pc), (b - H2(xn, 0.0, 1.0)) * keep_w, b)
    out[('poisson', pc)] = (c.to_base(xn), info['num_iterations'])
    # Helmholtz, Dirichlet data on the wall, Neumann flux on the left face
    l0, l1, gN = 0.5, 1.3, 0.7
    g = lambda xc: 1.0 + 0.5 * xc[:, 1] - 0.25 * xc[:, 2]
    x, info = solve_helmholtz(
        mesh, fd, {'wall': (BCType.DIRICHLET, g),
                   'left': (BCType.NEUMANN, gN)},
        lambda0=l0, lambda1=l1, rtol=rtol, return_info=True,
        preconditioner=pc)
    xn = _np(x)
    if check:
      xc = c.rp.node_coords
      uD = 1.0 + 0.5 * xc[:, 1] - 0.25 * xc[:, 2]
      assert np.abs(xn[wall] - uD[wall]).max() <= (
          1e-12 if dtype == F64 else 1e-6)
      fes2 = FiniteElementSpace.create(mesh, Quadrature1D.create(
          num_points=P + 1, quadrature_type=NodeType.GAUSS_LEGENDRE))
      flux = _np(fes2.boundary_covector('left', gN))
      rhs = (H2(f, 1.0, 0.0) + l1 * flux) * keep_w
      b = (rhs - H2(np.where(wall, uD, 0.0), l0, l1)) * keep_w
      true_residual(('helmholtz', pc),
                    (rhs - H2(xn, l0, l1)) * keep_w, b)
    out[('helmholtz', pc)] = (c.to_base(xn), info['num_iterations'])
  # linalg.cg on the collocated operator: the layered residual updates
  bmask = mesh.physical_masks['wall']
  keep_b = 1.0 - _np(bmask)
  op = operators.HelmholtzOperator.create(fes, bmask)
  _check_paths(op, c.numbering, P, False)
  b = Hc(f, 1.0, 0.0) * keep_b
  bd = torch.as_tensor(b, device=DEV, dtype=dtype)
  for l0, l1 in ((0.0, 1.0), (0.8, 1.0)):
    A = op.linear_operator(l0, l1)
    layered = NC.EXPECT[NC.kind(c.numbering)][1]
    assert (CGRunner(A, bd, tol=rtol).layered is not None) == layered
    for pc in (None, 'jacobi', 'pmg'):
      M = (None if pc is None else JacobiPreconditioner(op, l0, l1)
           if pc == 'jacobi' else PMultigridPreconditioner(op, l0, l1))
      for det in ('default', '0'):
        if det == '0':
          monkeypatch.setenv('SFEM_DETERMINISTIC', '0')
        x, info = cg(A, bd, tol=rtol, M=M)
        monkeypatch.delenv('SFEM_DETERMINISTIC', raising=False)
        xn = _np(x)
        name = ('cg', l0, pc, det)
        if check:
          true_residual(name, (b - Hc(xn, l0, l1)) * keep_b, b)
        out[name] = (c.to_base(xn), info['num_iterations'])
    if check and dtype == F64:
      xo, io = O.cg(lambda v: Hc(v, l0, l1) * keep_b, b, tol=rtol)
      for det in ('default', '0'):
        assert abs(out[('cg', l0, None, det)][1] -
                   io['num_iterations']) <= 2, (c.name, l0, det)
  if check and dtype == F64:
    xo, io, *_ = O.solve_poisson(c.rp.node_coords, c.rp.elements,
                                 (P, 'gll'), wall, f, rtol=rtol,
                                 return_ops=True)
    assert abs(out[('poisson', None)][1] - io['num_iterations']) <= 2
  return out


@pytest.mark.parametrize(
    'numbering,dtype', SOLVE_CASES,
    ids=[f'{c[0]}-{"f64" if c[1] == F64 else "f32"}' for c in SOLVE_CASES])
def test_solves_match_refiner_numbering(numbering, dtype, monkeypatch):
  """solve_poisson / solve_helmholtz (Dirichlet and Neumann groups through the
  permutation) and linalg.cg on the collocated operator, preconditioner None,
  'jacobi' and 'pmg', SFEM_DETERMINISTIC default and 0: true residual within
  the tolerance, solution equal to the refiner numbering's, and in fp64 the
  iteration counts of the refiner numbering and of the oracle's CG."""
  c = _solve_case(numbering, dtype)
  got = _run_solves(c, dtype, monkeypatch)
  ref = _refiner_runs(dtype, monkeypatch)
  for name, (x, its) in got.items():
    xb, itb = ref[name]
    err = np.abs(x - xb).max() / np.abs(xb).max()
    assert err <= (1e-5 if dtype == F64 else 2e-2), (numbering, name, err)
    if dtype == F64:
      assert abs(its - itb) <= 2, (numbering, name, its, itb)
