"""The kernels of the Schwarz pressure preconditioner, called through `_ops`
against the plain NumPy reference `tests/fdm_reference.py` (no `StokesSEM`
except in section g): `sfem_fdm_solve`, `sfem_fdm_solve_sums`,
`sfem_add_element_constants` and `sfem_ell_chebyshev`
(`swirl_fem_amd/csrc/sfem_fdm.hip`).

a. every instantiation of the local solve (ndim 1..3, Pp 1..10, both
   precisions) on inputs that turn any indexing mistake into an O(1) error:
   an odd number of elements, a bank of non-symmetric matrices, cases drawn
   per axis and element, weights that differ at every point, permuted nodes;
b. one axis at a time with a triangular matrix, where contracting the wrong
   axis or using S for S^T is shown to give another answer;
c. the element sums that ride on the local solve;
d. the closing pass, its grid-stride branch included;
e. the coarse Chebyshev polynomial across block boundaries, odd and even step
   counts, both precisions;
f. what the wrappers refuse before anything is launched;
g. the preconditioner's setup against the operator E itself on graded boxes
   whose axes differ in length, element count and spacing.

Bounds.  fp64 against the float64 reference: 1e-12 relative to the largest
entry (a, e, g: the bound of the kernel-against-torch checks in
`test_gpu_stokes.py`), 1e-13 where the sums are a handful of terms (b, c).
fp32: `fp32util.tolerance` = 1e-5 on float32-representable inputs (a); where
the inputs are not benign (e, g) max(1e-5, 4 x the error of the reference
evaluated in float32 on the same inputs) -- the factor covers another
summation order and fused multiply-adds.  The measured numbers are in
`profiles/schwarz_kernels_fp32_errors.md`.

Needs a real MI355X."""
import numpy as np
import pytest
import torch

from swirl_fem_amd import _lib, _ops
from tests import fdm_reference as R
from tests.fp32util import F32Rng, f32r, tolerance

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64, F32 = torch.float64, torch.float32
NAME = {F64: 'fp64', F32: 'fp32'}


def dev(x, dtype=None):
  t = torch.as_tensor(np.ascontiguousarray(x), device=DEV)
  return t if dtype is None else t.to(dtype)


def _np(t):
  return t.detach().double().cpu().numpy()


def relerr(got, want):
  got = _np(got) if isinstance(got, torch.Tensor) else np.asarray(got)
  assert got.shape == want.shape, (got.shape, want.shape)
  return np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)


def _rng(seed, dtype):
  return F32Rng(seed) if dtype == F32 else np.random.default_rng(seed)


def _round(x, dtype):
  return f32r(x) if dtype == F32 else x


# ------------------------------------------------------------ a. fdm_solve
E_A, C_A = 7, 5


def fdm_inputs(ndim, Pp, dtype, E=E_A, C=C_A, seed=0):
  """(r, pel, S, cases, w) as float64 / integer NumPy arrays (float32-
  representable for fp32)."""
  rng = _rng(1000 * seed + 100 * ndim + Pp, dtype)
  n = Pp ** ndim
  S = _round(np.eye(Pp) + rng.standard_normal((C, Pp, Pp)) / np.sqrt(Pp),
             dtype)
  cases = rng.integers(0, C, (ndim, E)).astype(np.int32)
  w = rng.uniform(0.5, 1.5, (E,) + (Pp,) * ndim)
  pel = rng.permutation(E * n).reshape(E, n).astype(np.int64)
  r = rng.standard_normal(E * n)
  return r, pel, S, cases, w


def run_fdm_solve(r, pel, S, cases, w, ndim, Pp, dtype):
  return _ops.fdm_solve(dev(r, dtype), None if pel is None else dev(pel),
                        dev(S, dtype), dev(cases), dev(w, dtype), ndim, Pp)


@pytest.mark.parametrize('dtype', [F64, F32], ids=NAME.get)
@pytest.mark.parametrize('Pp', range(1, 11))
@pytest.mark.parametrize('ndim', [1, 2, 3])
def test_fdm_solve_every_instantiation(ndim, Pp, dtype):
  r, pel, S, cases, w = fdm_inputs(ndim, Pp, dtype)
  tol = 1e-12 if dtype == F64 else tolerance(dtype, Pp)
  for numbering, p in (('pel', pel), ('contiguous', None)):
    want = R.fdm_solve(r, p, S, cases, w, ndim, Pp)
    got = run_fdm_solve(r, p, S, cases, w, ndim, Pp, dtype)
    assert got.dtype == dtype and got.shape == (r.size,)
    err = relerr(got, want)
    print(f'fdm_solve ndim={ndim} Pp={Pp} {NAME[dtype]} {numbering}: '
          f'err {err:.2e} (bound {tol:.0e})')
    assert err < tol, (ndim, Pp, dtype, numbering, err)


# ------------------------------------------- b. axis and transpose cases
@pytest.mark.parametrize('Pp', [3, 4])
@pytest.mark.parametrize('axis', [0, 1, 2])
def test_fdm_solve_axis_and_transpose(axis, Pp):
  """S = identity on two axes and U = I + strictly upper triangular on the
  third.  The kernel must give the reference's answer; the reference with U on
  another axis, or with U^T for U, must not (else the case shows nothing)."""
  ndim, E = 3, 3
  rng = np.random.default_rng(10 * axis + Pp)
  U = np.eye(Pp) + np.triu(rng.uniform(0.5, 1.5, (Pp, Pp)), 1)
  S = np.stack([np.eye(Pp), U])
  cases = np.zeros((ndim, E), dtype=np.int32)
  cases[axis] = 1
  n = Pp ** ndim
  w = rng.uniform(0.5, 1.5, (E,) + (Pp,) * ndim)
  r = rng.standard_normal(E * n)
  want = R.fdm_solve(r, None, S, cases, w, ndim, Pp)
  scale = np.abs(want).max()
  wrong = {}
  for other in range(ndim):
    if other != axis:
      moved = np.zeros_like(cases)
      moved[other] = 1
      wrong[f'axis {other}'] = R.fdm_solve(r, None, S, moved, w, ndim, Pp)
  wrong['transposed'] = R.fdm_solve(r, None, S.transpose(0, 2, 1), cases, w,
                                    ndim, Pp)
  for name, bad in wrong.items():
    gap = np.abs(bad - want).max() / scale
    assert gap >= 1e-2, (name, gap)
  got = run_fdm_solve(r, None, S, cases, w, ndim, Pp, F64)
  err = relerr(got, want)
  print(f'fdm_solve axis={axis} Pp={Pp}: err {err:.2e}; wrong answers at '
        + ', '.join(f'{k}: {np.abs(v - want).max() / scale:.2e}'
                    for k, v in wrong.items()))
  assert err < 1e-13, (axis, Pp, err)


# ------------------------------------------------------ c. fdm_solve_sums
@pytest.mark.parametrize('dtype', [F64, F32], ids=NAME.get)
@pytest.mark.parametrize('ndim,Pp', [(1, 3), (2, 1), (2, 5), (2, 9), (3, 2),
                                     (3, 4), (3, 7), (3, 10)])
def test_fdm_solve_sums(ndim, Pp, dtype):
  """Same kernel as `fdm_solve` with three more pointers: z bitwise equal;
  the element sums of r and of weights .* z (Pp = 10 in 3D: 15 or 16 values
  per lane; Pp = 1: one value in lane 0) against float64 sums of the same
  terms, relative to the sum of their absolute values: 1e-13 / 1e-6."""
  r, pel, S, cases, w = fdm_inputs(ndim, Pp, dtype, seed=1)
  weights = _rng(77 + Pp, dtype).uniform(0.5, 1.5, r.size)
  tol = 1e-13 if dtype == F64 else 1e-6
  E, n = pel.shape
  rd, Sd, cd, wd, gd = (dev(r, dtype), dev(S, dtype), dev(cases),
                        dev(w, dtype), dev(weights, dtype))
  for numbering, p in (('pel', pel), ('contiguous', None)):
    pd = None if p is None else dev(p)
    z_plain = _ops.fdm_solve(rd, pd, Sd, cd, wd, ndim, Pp)
    nan = lambda k: torch.full((k,), float('nan'), dtype=dtype, device=DEV)
    out = (nan(r.size), nan(E), nan(E))
    z, es, ws = _ops.fdm_solve_sums(rd, pd, Sd, cd, wd, gd, ndim, Pp, out=out)
    assert z is out[0] and es is out[1] and ws is out[2]
    for t in (z, es, ws):
      assert bool(torch.isfinite(t).all())
    assert torch.equal(z, z_plain)
    # fresh outputs give the same numbers
    z2, es2, ws2 = _ops.fdm_solve_sums(rd, pd, Sd, cd, wd, gd, ndim, Pp)
    assert torch.equal(z2, z) and torch.equal(es2, es) and torch.equal(ws2, ws)
    # the sums of the terms the kernel summed (its own z), in float64
    ids = np.arange(E * n).reshape(E, n) if p is None else p
    es_ref, ws_ref = R.fdm_sums(r, _np(z), ids, weights)
    es_abs, ws_abs = R.fdm_sums(np.abs(r), np.abs(_np(z)), ids, weights)
    e1 = (np.abs(_np(es) - es_ref) / es_abs).max()
    e2 = (np.abs(_np(ws) - ws_ref) / ws_abs).max()
    print(f'fdm_solve_sums ndim={ndim} Pp={Pp} {NAME[dtype]} {numbering}: '
          f'elem_sum {e1:.2e} weighted_sum {e2:.2e} (bound {tol:.0e})')
    assert e1 < tol and e2 < tol, (ndim, Pp, dtype, numbering, e1, e2)


# ----------------------------------------------- d. add_element_constants_
def check_add_constants(E, epm, n, dtype, seed=0):
  g = torch.Generator(device=DEV).manual_seed(seed)
  z = torch.randn(E * n, dtype=dtype, device=DEV, generator=g)
  yc = torch.randn(E, dtype=dtype, device=DEV, generator=g)
  shift = torch.randn(E // epm, dtype=dtype, device=DEV, generator=g)
  member = torch.arange(E, device=DEV) // epm
  want = (z.view(E, n) + (yc - shift[member])[:, None]).reshape(-1)
  got = z.clone()
  ret = _ops.add_element_constants_(got, yc, shift, n, epm)
  assert ret is got
  assert torch.equal(got, want)          # one subtraction, one addition
  return z, yc, shift, got


@pytest.mark.parametrize('dtype', [F64, F32], ids=NAME.get)
@pytest.mark.parametrize('E,epm', [(1, 1), (12, 12), (12, 4), (12, 1)])
@pytest.mark.parametrize('n', [1, 27, 1000])
def test_add_element_constants(n, E, epm, dtype):
  z, yc, shift, got = check_add_constants(E, epm, n, dtype, seed=n + E + epm)
  ref = R.add_element_constants(_np(z), _np(yc), _np(shift), n, epm)
  if dtype == F64:
    assert np.array_equal(_np(got), ref)
  else:
    assert relerr(got, ref) < 1e-6


def test_add_element_constants_grid_stride():
  """E n = 8.4e6 > 8192 blocks x 1024: every thread strides on (three
  members of 2800 elements, n = 1000; 67 MB)."""
  assert 8400 * 1000 > 8192 * 1024
  check_add_constants(8400, 2800, 1000, F64)


# -------------------------------------------------------- e. ell_chebyshev
LMIN, LMAX = 0.3, 1.7
CHEB_CASES = [(1, 1, 1), (1, 1, 2), (255, 7, 3), (255, 27, 8), (256, 27, 1),
              (256, 7, 2), (257, 7, 8), (257, 1, 3), (1000, 27, 2),
              (1000, 7, 3), (4099, 27, 3), (4099, 7, 8), (4099, 1, 2)]


def test_chebyshev_cases_cover_the_parameters():
  assert {c[0] for c in CHEB_CASES} == {1, 255, 256, 257, 1000, 4099}
  assert {c[1] for c in CHEB_CASES} == {1, 7, 27}
  assert {c[2] for c in CHEB_CASES} == {1, 2, 3, 8}
  for n in {c[0] for c in CHEB_CASES}:
    assert {c[2] % 2 for c in CHEB_CASES if c[0] == n} == {0, 1}, n


def cheb_matrix(n, width, dtype, seed):
  """(A csr, cols, vals, dinv, b): symmetric, strictly diagonally dominant
  with row sums of |off-diagonal| = rho_i A_ii, rho_i <= 0.55 (Gershgorin: the
  spectrum of D^-1 A inside [0.45, 1.55]); diagonal + (width - 1) / 2
  wrapped off-diagonals on each side, as many as n has room for; ELL rows
  padded to `width` with (column 0, value 0)."""
  import scipy.sparse as sp
  rng = _rng(seed, dtype)
  half = min((width - 1) // 2, (n - 1) // 2)
  offsets = (rng.choice(np.arange(1, (n - 1) // 2 + 1), half, replace=False)
             if half else np.zeros(0, dtype=np.int64))
  i = np.arange(n)
  rows, cols, vals = [], [], []
  for o in offsets:
    v = _round(rng.uniform(-1.0, 1.0, n), dtype)
    rows += [i, (i + o) % n]
    cols += [(i + o) % n, i]
    vals += [v, v]
  if half:
    off = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows),
                                                np.concatenate(cols))),
                        shape=(n, n))
    rowsum = np.asarray(abs(off).sum(axis=1)).reshape(-1)
    diag = _round(rowsum / rng.uniform(0.2, 0.55, n), dtype)
  else:
    off = sp.csr_matrix((n, n))
    diag = _round(rng.uniform(0.5, 1.5, n), dtype)
  A = (off + sp.diags(diag)).tocsr()
  assert np.abs(A - A.T).max() == 0
  ecols, evals = R.ell_from_csr(A)
  assert ecols.shape[0] == 2 * half + 1 <= width
  pad = width - ecols.shape[0]
  ecols = np.concatenate([ecols, np.zeros((pad, n), np.int32)])
  evals = np.concatenate([evals, np.zeros((pad, n))])
  dinv = _round(1.0 / diag, dtype)
  b = rng.standard_normal(n)
  lam = (np.abs(off) @ np.ones(n)) * dinv
  assert lam.max() <= 0.56
  return A, ecols, evals, dinv, b


@pytest.mark.parametrize('dtype', [F64, F32], ids=NAME.get)
@pytest.mark.parametrize('n,width,steps', CHEB_CASES)
def test_ell_chebyshev(n, width, steps, dtype):
  A, cols, vals, dinv, b = cheb_matrix(n, width, dtype, seed=n + width)
  want = R.ell_chebyshev(A, dinv, b, steps, LMIN, LMAX)
  if dtype == F64:
    tol, e_ref = 1e-12, None
  else:
    e_ref = relerr(R.ell_chebyshev(A, dinv, b, steps, LMIN, LMAX,
                                   dtype=np.float32).astype(np.float64), want)
    tol = max(1e-5, 4 * e_ref)
  cd, vd, dd, bd = dev(cols), dev(vals, dtype), dev(dinv, dtype), dev(b, dtype)
  assert cd.shape == (width, n) and cd.dtype == torch.int32
  b0 = bd.clone()
  nan = lambda k: torch.full((k,), float('nan'), dtype=dtype, device=DEV)
  x, work = nan(n), nan(3 * n)
  ret = _ops.ell_chebyshev(cd, vd, dd, bd, steps, LMIN, LMAX, work=work,
                           out=x)
  assert ret is x
  assert bool(torch.isfinite(x).all())
  assert torch.equal(bd, b0)
  err = relerr(x, want)
  print(f'ell_chebyshev n={n} width={width} steps={steps} {NAME[dtype]}: '
        f'err {err:.2e}' + ('' if e_ref is None else
                            f' float32 reference {e_ref:.2e}')
        + f' (bound {tol:.1e})')
  assert err < tol, (n, width, steps, dtype, err, e_ref)
  # again, own scratch and result: the same bits
  x2 = _ops.ell_chebyshev(cd, vd, dd, bd, steps, LMIN, LMAX)
  assert x2 is not x and torch.equal(x2, x)


@pytest.mark.parametrize('dtype', [F64, F32], ids=NAME.get)
def test_ell_chebyshev_of_nothing(dtype):
  empty = torch.empty(0, dtype=dtype, device=DEV)
  cols = torch.empty((3, 0), dtype=torch.int32, device=DEV)
  vals = torch.empty((3, 0), dtype=dtype, device=DEV)
  x = _ops.ell_chebyshev(cols, vals, empty, empty, 4, LMIN, LMAX)
  assert x.numel() == 0
  torch.cuda.synchronize()


# ------------------------------------------------------------ f. refusals
def _fdm_args(ndim=2, Pp=3, dtype=F64, E=4):
  r, pel, S, cases, w = fdm_inputs(ndim, Pp, dtype, E=E)
  return dict(r=dev(r, dtype), pel=dev(pel), S=dev(S, dtype),
              cases=dev(cases), inv_ev=dev(w, dtype), ndim=ndim, Pp=Pp)


def _weights(a):
  return torch.ones_like(a['r'])


FDM_REFUSALS = {
    'cases int64': (TypeError, lambda a: a.update(cases=a['cases'].long())),
    'cases not contiguous': (ValueError, lambda a: a.update(
        cases=a['cases'].repeat(1, 2)[:, ::2])),
    'cases transposed': (ValueError, lambda a: a.update(
        cases=a['cases'].t().contiguous())),
    'cases flat': (ValueError, lambda a: a.update(
        cases=a['cases'].reshape(-1))),
    'pel int32': (TypeError, lambda a: a.update(pel=a['pel'].int())),
    'pel short': (ValueError, lambda a: a.update(
        pel=a['pel'][:-1].contiguous())),
    'S float32': (TypeError, lambda a: a.update(S=a['S'].float())),
    'inv_ev float32': (TypeError, lambda a: a.update(
        inv_ev=a['inv_ev'].float())),
    'inv_ev short': (ValueError, lambda a: a.update(
        inv_ev=a['inv_ev'][:-1].contiguous())),
    'inv_ev long': (ValueError, lambda a: a.update(
        inv_ev=torch.cat([a['inv_ev'], a['inv_ev']]))),
    'r not contiguous': (ValueError, lambda a: a.update(
        r=a['r'].repeat_interleave(2)[::2])),
    'r short without pel': (ValueError, lambda a: a.update(
        pel=None, r=a['r'][:-1].contiguous())),
    'r integer': (TypeError, lambda a: a.update(r=a['r'].long())),
}


@pytest.mark.parametrize('what', FDM_REFUSALS)
@pytest.mark.parametrize('sums', [False, True], ids=['solve', 'sums'])
def test_fdm_solve_refuses(what, sums):
  exc, spoil = FDM_REFUSALS[what]
  a = _fdm_args()
  weights = _weights(a)
  spoil(a)
  with pytest.raises(exc):
    if sums:
      _ops.fdm_solve_sums(a['r'], a['pel'], a['S'], a['cases'], a['inv_ev'],
                          weights, a['ndim'], a['Pp'])
    else:
      _ops.fdm_solve(**a)


def test_fdm_solve_sums_refuses_weights():
  a = _fdm_args()
  args = lambda w: (a['r'], a['pel'], a['S'], a['cases'], a['inv_ev'], w,
                    a['ndim'], a['Pp'])
  with pytest.raises(TypeError):
    _ops.fdm_solve_sums(*args(_weights(a).float()))
  with pytest.raises(ValueError):
    _ops.fdm_solve_sums(*args(_weights(a)[:-1].contiguous()))
  with pytest.raises(ValueError):           # out of another shape
    _ops.fdm_solve_sums(*args(_weights(a)), out=(
        torch.empty_like(a['r']), torch.empty(3, dtype=F64, device=DEV),
        torch.empty(4, dtype=F64, device=DEV)))


def test_fdm_solve_refuses_eleven_points():
  """Pp = 11 has no instantiation.  Sizes that are consistent for Pp = 11 pass
  the wrapper; the library's own range check answers (SFEM_EINVAL, with the
  range in the message), and nothing is launched."""
  a = _fdm_args(ndim=1, Pp=11, E=2)
  with pytest.raises(_lib.SfemError, match=r'1 <= Pp <= 10'):
    _ops.fdm_solve(**a)
  with pytest.raises(_lib.SfemError, match=r'1 <= Pp <= 10'):
    _ops.fdm_solve_sums(a['r'], a['pel'], a['S'], a['cases'], a['inv_ev'],
                        _weights(a), 1, 11)
  torch.cuda.synchronize()


def _cheb_args(n=40, width=7, dtype=F64):
  A, cols, vals, dinv, b = cheb_matrix(n, width, dtype, seed=3)
  return dict(cols=dev(cols), vals=dev(vals, dtype), dinv=dev(dinv, dtype),
              b=dev(b, dtype), steps=3, lmin=LMIN, lmax=LMAX,
              work=torch.empty(3 * n, dtype=dtype, device=DEV))


CHEB_REFUSALS = {
    'work short': (ValueError, lambda a: a.update(work=a['work'][:-1])),
    'work float32': (ValueError, lambda a: a.update(work=torch.empty(
        3 * 40, dtype=F32, device=DEV))),
    'cols int64': (TypeError, lambda a: a.update(cols=a['cols'].long())),
    'vals of another shape': (ValueError, lambda a: a.update(
        vals=a['vals'][:-1].contiguous())),
    'vals float32': (TypeError, lambda a: a.update(vals=a['vals'].float())),
    'cols of another n': (ValueError, lambda a: a.update(
        cols=a['cols'][:, :-1].contiguous(),
        vals=a['vals'][:, :-1].contiguous())),
    'dinv short': (ValueError, lambda a: a.update(
        dinv=a['dinv'][:-1].contiguous())),
    'lmin zero': (ValueError, lambda a: a.update(lmin=0.0)),
    'lmin negative': (ValueError, lambda a: a.update(lmin=-0.3)),
    'lmax equal lmin': (ValueError, lambda a: a.update(lmax=LMIN)),
    'lmax below lmin': (ValueError, lambda a: a.update(lmax=0.1)),
    'no steps': (ValueError, lambda a: a.update(steps=0)),
    'out short': (ValueError, lambda a: a.update(out=torch.empty(
        39, dtype=F64, device=DEV))),
}


@pytest.mark.parametrize('what', CHEB_REFUSALS)
def test_ell_chebyshev_refuses(what):
  exc, spoil = CHEB_REFUSALS[what]
  a = _cheb_args()
  spoil(a)
  with pytest.raises(exc):
    _ops.ell_chebyshev(**a)


def test_add_element_constants_refuses():
  t = lambda k, dtype=F64: torch.zeros(k, dtype=dtype, device=DEV)
  with pytest.raises(ValueError):           # 12 elements, members of 5
    _ops.add_element_constants_(t(12 * 8), t(12), t(3), 8, 5)
  with pytest.raises(ValueError):           # 3 members, 2 shifts
    _ops.add_element_constants_(t(12 * 8), t(12), t(2), 8, 4)
  with pytest.raises(ValueError):           # z of another size
    _ops.add_element_constants_(t(12 * 8 - 1), t(12), t(3), 8, 4)
  with pytest.raises(ValueError):
    _ops.add_element_constants_(t(12 * 8), t(12), t(3), 8, 0)
  with pytest.raises(TypeError):
    _ops.add_element_constants_(t(12 * 8), t(12, F32), t(3), 8, 4)
  with pytest.raises(TypeError):
    _ops.add_element_constants_(t(12 * 8), t(12), t(3, F32), 8, 4)


# ------------------------- g. the preconditioner on boxes whose axes differ
BOXES = {3: ((3, 4, 2), (1.0, 2.0, 0.5)), 2: ((4, 3), (1.0, 2.5))}
# (corner, face, most interior) element of each box, as multi-indices (axis 0
# slowest, `box_mesh`).  The 3D box has two layers along its last axis, so
# every element touches one of its walls there.
ELEMENTS = {3: {'corner': (0, 0, 0), 'face': (1, 0, 1), 'interior': (1, 2, 0)},
            2: {'corner': (0, 0), 'face': (2, 0), 'interior': (2, 1)}}
DT, ORDER = 2e-3, 3
_SETUPS = {}


def graded_setup(ndim, P, walls, dtype):
  """(StokesSEM, preconditioner, E) on the graded box; x_a -> x_a + 0.3 x_a
  (L_a - x_a) / L_a keeps the mesh Cartesian and the ends of every axis in
  place (so it can be periodic) and gives every element its own size."""
  key = (ndim, P, walls, dtype)
  if key not in _SETUPS:
    from swirl_fem_amd.common.premesh_commons import box_mesh
    from swirl_fem_amd.core.interpolation import Nodes1D, NodeType
    from swirl_fem_amd.core.mesh_refiner import refine_premesh
    from swirl_fem_amd.navier_stokes import navier_stokes as ns
    from swirl_fem_amd.navier_stokes import pressure_preconditioner as pc
    counts, L = BOXES[ndim]
    pm = box_mesh(counts, (0.0,) * ndim, L,
                  periodic_dims=() if walls else tuple(range(ndim)))
    x = pm.node_coords.copy()
    for a in range(ndim):
      x[:, a] += 0.3 * x[:, a] * (L[a] - x[:, a]) / L[a]
    pm = pm.replace(node_coords=x)
    meshes = []
    for grid in (Nodes1D.create(P, NodeType.GAUSS_LOBATTO_LEGENDRE),
                 Nodes1D.create(P - 2, NodeType.GAUSS_LEGENDRE)):
      rp = refine_premesh(pm, grid)
      if dtype == F32:
        rp = rp.replace(node_coords=f32r(rp.node_coords))
      meshes.append(rp.finalize(device=DEV, dtype=dtype))
    bcs = {'boundary': (ns.BCType.DIRICHLET, 0.0)} if walls else {}
    sem = ns.StokesSEM.from_meshes(meshes[0], meshes[1], bcs)
    M = pc.SchwarzPressurePreconditioner(sem, DT, ORDER)
    _SETUPS.clear()                       # one setup alive at a time
    _SETUPS[key] = (sem, M, ns._PressureOperator(sem, DT, ORDER))
  return _SETUPS[key]


def element_rhs(M, ndim, where, dtype, seed):
  """(element id, its nodes, r supported there with zero element mean)."""
  counts = BOXES[ndim][0]
  e = int(np.ravel_multi_index(ELEMENTS[ndim][where], counts))
  nodes = _np(M.pel[e]).astype(np.int64)
  v = _rng(seed, dtype).standard_normal(nodes.size)
  v = _round(v - v.mean(), dtype)
  r = np.zeros(M.pel.numel())
  r[nodes] = v
  return e, nodes, r


@pytest.mark.parametrize('walls', [True, False], ids=['walls', 'periodic'])
@pytest.mark.parametrize('ndim,P', [(3, 4), (3, 6), (3, 9), (3, 12), (2, 5),
                                    (2, 8), (2, 11)])
def test_local_solve_inverts_element_blocks(ndim, P, walls):
  """On a Cartesian mesh the local solve is the (pseudo-)inverse of E's
  diagonal block: for r supported in one element with zero element mean,
  z = local_solve(r) vanishes outside the element, equals the reference fed
  the preconditioner's own S, cases and inverted eigenvalues, and
  (E z - mean - r) vanishes in the element to the bound of the isotropic check
  in `test_gpu_stokes.py`.  Element counts, lengths and spacings differ
  between the axes here, so a setup that paired an axis with another axis's
  factors, cofactors or eigenvalues fails the last check: the control at the
  end exchanges the matrices of two axes and must miss it by 1e-3 or more."""
  sem, M, Eop = graded_setup(ndim, P, walls, F64)
  Pp = P - 2
  assert M.Pp == Pp and M.d == ndim and M.pel_arg is None
  assert M.inv_ev.shape == (M.pel.shape[0],) + (Pp,) * ndim
  S, cases, w = _np(M.S), _np(M.case32).astype(np.int64), _np(M.inv_ev)
  for where in ELEMENTS[ndim]:
    e, nodes, r = element_rhs(M, ndim, where, F64, seed=P)
    z = M.local_solve(dev(r))
    outside = z.clone()
    outside[dev(nodes)] = 0
    assert float(outside.abs().max()) == 0.0
    want = R.fdm_solve(r, _np(M.pel).astype(np.int64), S, cases, w, ndim, Pp)
    err = relerr(z, want)
    Ez = Eop(z)[dev(nodes)]
    res = float((Ez - Ez.mean() - dev(r[nodes])).abs().max()) / np.abs(r).max()
    print(f'schwarz ndim={ndim} P={P} {"walls" if walls else "periodic"} '
          f'{where} element {e}: kernel vs reference {err:.2e}, '
          f'|E z - mean - r| / |r| {res:.2e}')
    assert err < 1e-12, (where, err)
    assert res < 1e-8, (where, res)
  # control: the same solve with the matrices of axes 0 and 1 exchanged does
  # NOT invert the block (the axes differ, so the check above can tell)
  swapped = cases.copy()
  swapped[[0, 1]] = cases[[1, 0]]
  zbad = dev(R.fdm_solve(r, _np(M.pel).astype(np.int64), S, swapped, w, ndim,
                         Pp))
  Ez = Eop(zbad)[dev(nodes)]
  bad = float((Ez - Ez.mean() - dev(r[nodes])).abs().max()) / np.abs(r).max()
  print(f'schwarz ndim={ndim} P={P} control, axes 0 and 1 exchanged: {bad:.2e}')
  assert bad > 1e-3, bad


@pytest.mark.parametrize('walls', [True, False], ids=['walls', 'periodic'])
@pytest.mark.parametrize('ndim,P', [(3, 6), (2, 8)])
def test_local_solve_fp32(ndim, P, walls):
  """The float32 kernel on the preconditioner's own float32 S and inverted
  eigenvalues (S = L^-T V is worse conditioned than the matrices of section
  a) against the float64 reference on the same numbers: within max(1e-5,
  4 x the error of the reference evaluated in float32)."""
  sem, M, _ = graded_setup(ndim, P, walls, F32)
  Pp = P - 2
  assert M.S.dtype == F32 and M.inv_ev.dtype == F32
  S, cases, w = _np(M.S), _np(M.case32).astype(np.int64), _np(M.inv_ev)
  pel = _np(M.pel).astype(np.int64)
  for where in ELEMENTS[ndim]:
    e, nodes, r = element_rhs(M, ndim, where, F32, seed=P)
    z = M.local_solve(dev(r, F32))
    assert z.dtype == F32
    outside = z.clone()
    outside[dev(nodes)] = 0
    assert float(outside.abs().max()) == 0.0
    want = R.fdm_solve(r, pel, S, cases, w, ndim, Pp)
    e_ref = relerr(R.fdm_solve(r, pel, S, cases, w, ndim, Pp,
                               dtype=np.float32).astype(np.float64), want)
    err = relerr(z, want)
    tol = max(1e-5, 4 * e_ref)
    print(f'schwarz fp32 ndim={ndim} P={P} {"walls" if walls else "periodic"} '
          f'{where} element {e}: kernel {err:.2e} float32 reference '
          f'{e_ref:.2e} (bound {tol:.1e})')
    assert err < tol, (where, err, e_ref)
