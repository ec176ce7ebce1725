"""Host-side checks of the adjoint of scalar transport: the
NumPy reference of the kernel's cotangents (`tests/transport_adjoint_reference
.py`) against the reference integrand by the adjoint identity, the reverse
sweep through dense steps against central differences, and the ctypes mirror
of the new argument struct."""
import ctypes
import os
import re

import numpy as np
import pytest

from swirl_fem_amd import _lib
from tests import advection_reference as AR
from tests import transport_adjoint_reference as TA
from tests import transport_reference as TR


@pytest.mark.parametrize('ndim,P,Q', [(2, 4, 5), (3, 3, 4), (2, 3, 3),
                                      (3, 3, 7)])
def test_reference_vjp_adjoint_identity(ndim, P, Q):
  """The integrand is bilinear in (T_j, u_j) and linear in s, so
  <lam, rhs(dT, u) + rhs(T, du) + W ds> = <T_bar, dT> + <u_bar, du> +
  <s_bar, ds> to rounding: 1e-12 of the product of norms."""
  rp = TR.box_with_sides(2, ndim, P, three_kinds=True)
  fes = AR.space(rp.node_coords, rp.elements, P, (Q, 'gl'))
  rng = np.random.default_rng(10 * ndim + Q)
  E, nq = fes.num_elements, fes.Q
  spec = [(True, 0.7, -1.3), (True, -2.0, 0.0), (False, 0.4, 0.9),
          (True, 0.0, 2.0)]
  levels, dlevels = [], []
  for vel, mc, cc in spec:
    levels.append((rng.standard_normal((E, nq)),
                   rng.standard_normal((E, nq, ndim)) if vel else None, mc, cc))
    dlevels.append((rng.standard_normal((E, nq)),
                    rng.standard_normal((E, nq, ndim)) if vel else None))
  lam = rng.standard_normal((E, nq))
  ds = rng.standard_normal((E, nq))
  # the directional derivative of the integrand along (dT, du, ds)
  tangent = TR.integrand(fes, [(dT, u, mc, cc) for (T, u, mc, cc), (dT, _)
                               in zip(levels, dlevels)], ds)
  tangent += TR.integrand(fes, [(T, du, 0.0, cc) for (T, u, mc, cc), (_, du)
                                in zip(levels, dlevels) if du is not None])
  bars, s_bar = TA.vjp(fes, lam, levels)
  left = float((lam * tangent).sum())
  right = float((s_bar * ds).sum())
  for (T_bar, u_bar), (dT, du), (_, u, _, _) in zip(bars, dlevels, levels):
    right += float((T_bar * dT).sum())
    assert (u_bar is None) == (u is None)
    if du is not None:
      right += float((u_bar * du).sum())
  scale = np.linalg.norm(lam) * np.linalg.norm(tangent)
  print(f'ndim={ndim} Q={Q}: <lam, J d> = {left:.6e}, <J^T lam, d> = '
        f'{right:.6e}, difference / norms {abs(left - right) / scale:.2e}')
  assert abs(left - right) <= 1e-12 * scale
  # a level whose scalar is withheld has no velocity cotangent, the rest stays
  part, _ = TA.vjp(fes, lam, [(None,) + levels[0][1:]], want_source=False)
  assert part[0][1] is None and _ is None
  assert np.array_equal(part[0][0], bars[0][0])
  # conv_coef = 0: the velocity has no effect
  assert not bars[1][1].any()


@pytest.fixture(scope='module')
def problem3d():
  return TA.step_problem(3)


@pytest.mark.parametrize('name', list(TA.CD_H))
def test_reverse_sweep_matches_central_differences(problem3d, name):
  """Orders 1, 2, 3 in sequence on the three-kinds mesh of 2^3 elements, P = 3,
  with Dirichlet, Neumann and Robin sides; one random direction per input.
  Observed at the steps `TA.CD_H` (the minimisers over the decades): T0
  8.08e-16, nodal / constant / per-point velocity 1.59e-10 / 9.00e-11 /
  6.92e-10, nodal / per-point source 1.77e-15 / 1.17e-15, per-point k
  8.92e-10.  Asserted: 10 x what was observed."""
  got, _, an = TA.central_differences(problem3d, [name])[name]
  print(f'{name}: h = {TA.CD_H[name]:g}, analytic {an:.6e}, relative '
        f'discrepancy {got:.2e} (recorded {TA.CD_OBSERVED[name]:.2e})')
  assert abs(an) > 1e-3
  assert got <= 10.0 * TA.CD_OBSERVED[name]


def test_reverse_sweep_on_a_periodic_box():
  """One unknown per periodic class: the sweep against central differences
  for T0 (linear: rounding alone) on the box periodic in x."""
  prob = TA.step_problem(2, periodic=(0,))
  assert prob['dense'].R is not None
  got, _, an = TA.central_differences(prob, ['T0'])['T0']
  print(f'periodic T0: analytic {an:.6e}, discrepancy {got:.2e}')
  assert got <= 1e-12


def test_vjp_struct_layout():
  """`sfem_transport_vjp_args` in the header and its ctypes mirror: the same
  fields in the same order, arrays of SFEM_TRANSPORT_LEVELS; the ABI number
  is unchanged (a pure addition)."""
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  text = open(os.path.join(root, 'include', 'sfem.h')).read()
  assert '#define SFEM_ABI_VERSION 10' in text and _lib.ABI_VERSION == 10
  levels = int(re.search(r'#define SFEM_TRANSPORT_LEVELS (\d+)', text).group(1))
  assert levels == _lib.SFEM_TRANSPORT_LEVELS == 3
  body = re.search(r'typedef struct sfem_transport_vjp_args \{(.*?)\} '
                   r'sfem_transport_vjp_args;', text, flags=re.S).group(1)
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  names, arrays = [], set()
  for decl in body.split(';'):
    decl = decl.strip()
    if not decl:
      continue
    first, *rest = decl.split(',')
    m = re.search(r'(\w+)\s*\[\s*SFEM_TRANSPORT_LEVELS\s*\]$', first)
    if m:
      names.append(m.group(1))
      arrays.add(m.group(1))
    else:
      names.append(re.findall(r'\w+', first)[-1])
    for r in rest:
      r = r.strip()
      m = re.search(r'(\w+)\s*\[\s*SFEM_TRANSPORT_LEVELS\s*\]$', r)
      names.append(m.group(1) if m else r)
      if m:
        arrays.add(m.group(1))
  fields = _lib.TransportVjpArgs._fields_
  assert names == [f[0] for f in fields], (names, fields)
  for name, ctype in fields:
    is_array = issubclass(ctype, ctypes.Array)
    assert is_array == (name in arrays), name
    if is_array:
      assert ctype._length_ == levels
  assert arrays == {'scalar', 'velocity', 'mass_coef', 'conv_coef', 'dscalar',
                    'dvelocity'}
  kinds = dict(fields)
  assert kinds['mass_coef']._type_ is ctypes.c_double
  assert kinds['conv_coef']._type_ is ctypes.c_double
  assert kinds['num_elements'] is _lib.c_i64 and kinds['P'] is _lib.c_i32
  # 6 arrays of 3 eight-byte entries, 10 pointers, 2 int64, 5 int32 (+ pad)
  assert ctypes.sizeof(_lib.TransportVjpArgs) == 6 * 24 + 10 * 8 + 16 + 24
  assert (_lib.SIGNATURES['sfem_transport_rhs_vjp'][0]._type_ is
          _lib.TransportVjpArgs)
  # the forward struct is as it was
  assert ctypes.sizeof(_lib.TransportArgs) == 4 * 24 + 10 * 8 + 16 + 24
