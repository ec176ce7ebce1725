"""The sum-factorised Stokes reference (`tests/sumfact_stokes_reference.py`)
against the dense float64 oracle (`O.div_local`, `O.div_t_local`,
`O.FESpace.convection_local`) at the orders the oracle reaches, and on its own
at 3D P = 12 through properties of the continuous operators.  Two references
are compared here, no code under test."""
import functools

import numpy as np
import pytest

from oracle import sfem_oracle as O
from tests import numbering_cases as NC
from tests import stokes_sweep_cases as C
from tests import sumfact_stokes_reference as S

# Two float64 evaluations of the same operators.  Measured on these pairs
# (curved elements included), relative to the largest entry: div_local
# <= 3.3e-14 and div assembled through random pressure rows <= 6.3e-14 (both
# 2D, P = 12), grad_t <= 4.1e-15, convection <= 2.9e-15 collocated and
# <= 1.4e-14 over-integrated (2D, 10 -> 12 points), so the bound of
# `test_sumfact_reference_host.py` stands as it is.
BOUND = 1e-12

CASES = [(2, 4), (2, 5), (2, 7), (2, 9), (2, 12), (3, 4), (3, 5), (3, 6)]


def _rel(a, b):
  return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@functools.lru_cache(maxsize=None)
def _setup(ndim, P):
  c = C.pair(ndim, P, 'identity', False)
  ov, op = NC.oracle_spaces(c.v.base, c.p.base, P)
  sf = S.StokesSpace(c.v.rp.node_coords, c.v.rp.elements, c.p.rp.elements, P)
  return c, ov, op, sf


@pytest.mark.parametrize('ndim,P', CASES)
def test_div_and_grad_t_match_oracle(ndim, P):
  c, ov, op, sf = _setup(ndim, P)
  assert c.geometry == ('vertex' if P == 4 else 'three_kinds')
  # the two spaces of a pair carry the same geometry: the oracle takes w detJ
  # from the pressure mesh, the reference here from the velocity nodes
  assert _rel(sf.W, op.jacdets * op.weights[None, :]) <= BOUND
  assert _rel(sf.points, ov.quad_coords) <= 1e-14
  rng = np.random.default_rng(10 * ndim + P)
  ul = rng.standard_normal(c.v.rp.elements.shape + (ndim,))
  pl = rng.standard_normal(c.p.rp.elements.shape)
  err = _rel(sf.div_local(ul), O.div_local(ov, op, ul))
  print('div_local', ndim, P, err)
  assert err <= BOUND, err
  err = _rel(sf.grad_t_local(pl), O.div_t_local(ov, op, pl))
  print('grad_t_local', ndim, P, err)
  assert err <= BOUND, err
  # assembled, through random pressure index rows
  c2 = C.pair(ndim, P, 'random', False)
  assert not np.array_equal(c2.p.rp.elements, c.p.rp.elements)
  sf2 = S.StokesSpace(c2.v.rp.node_coords, c2.v.rp.elements,
                      c2.p.rp.elements, P)
  u = rng.standard_normal((ov.num_nodes, ndim))
  p = rng.standard_normal(op.num_nodes)
  want = c2.p.from_base(op.scatter(O.div_local(ov, op, ov.gather(u))))
  err = _rel(sf2.div(u), want)
  print('div', ndim, P, err)
  assert err <= BOUND, err
  want = ov.scatter(O.div_t_local(ov, op, op.gather(c2.p.to_base(p))))
  err = _rel(sf2.grad_t(p), want)
  print('grad_t', ndim, P, err)
  assert err <= BOUND, err


@pytest.mark.parametrize('ndim,P', CASES)
def test_convection_matches_oracle(ndim, P):
  """Collocated on the P-point velocity mesh, and over-integrated on P points
  from the (P - 2)-point mesh of the same premesh (and on P + 2 from P)."""
  c = C.pair(ndim, P, 'identity', False)
  orp = C.overint_premesh(ndim, P, False)
  rng = np.random.default_rng(20 * ndim + P)
  runs = [(c.v.rp, P, P), (orp, P - 2, P)]
  if P <= 6:
    runs.append((c.v.rp, P, P + 2))
  for rp, Pv, q in runs:
    of = O.FESpace(rp.node_coords, rp.elements, (Pv, 'gll'), (q, 'gll'))
    cs = S.ConvectionSpace(rp.node_coords, rp.elements, Pv, q)
    assert _rel(cs.points, of.quad_coords) <= 1e-14
    assert _rel(cs.det, of.jacdets) <= BOUND
    ul = rng.standard_normal(rp.elements.shape + (ndim,))
    err = _rel(cs.convection_local(ul), of.convection_local(ul, ul))
    print('convection', ndim, Pv, q, err)
    assert err <= BOUND, (Pv, q, err)


def test_float32_carries_the_same_algorithm():
  c, ov, op, sf = _setup(3, 5)
  lo = S.StokesSpace(c.v.rp.node_coords, c.v.rp.elements, c.p.rp.elements, 5,
                     np.float32)
  rng = np.random.default_rng(1)
  ul = rng.standard_normal(c.v.rp.elements.shape + (3,))
  got = lo.div_local(ul)
  assert got.dtype == np.float32 and lo.wK.dtype == np.float32
  assert 1e-9 < _rel(got, sf.div_local(ul)) < 1e-5
  got = lo.grad_t_local(sf.div_local(ul))
  assert got.dtype == np.float32
  co = S.ConvectionSpace(c.v.rp.node_coords, c.v.rp.elements, 5, 7, np.float32)
  assert co.convection_local(ul).dtype == np.float32


# ------------------------------------------- 3D, P = 12: properties only
P_HIGH = 12


@functools.lru_cache(maxsize=None)
def _high():
  c = C.pair(3, P_HIGH, 'random', False)
  sf = S.StokesSpace(c.v.rp.node_coords, c.v.rp.elements, c.p.rp.elements,
                     P_HIGH)
  # the first layer is curved (the bend shears x2 along x0 and x1: det J
  # stays put, the cofactors vary), the moved vertex gives multilinear
  # elements, the rest is affine
  vary = np.ptp(sf.K, axis=1).max(axis=(1, 2)) / np.abs(sf.K).max()
  first = sf.points[:, :, 0].mean(axis=1) < 1.0 / 3
  assert first.sum() == 9 and vary[first].min() > 1e-2
  assert (vary < 1e-11).sum() == 10 and (vary[~first] > 1e-2).sum() == 8
  return c, sf


def test_div_and_grad_t_are_adjoint_at_p12():
  c, sf = _high()
  rng = np.random.default_rng(12)
  u = rng.standard_normal((sf.num_nodes, 3))
  p = rng.standard_normal(sf.num_pressure_nodes)
  g = sf.grad_t(p)
  lhs, rhs = sf.div(u) @ p, (u * g).sum()
  assert abs(lhs - rhs) <= 1e-12 * np.linalg.norm(u) * np.linalg.norm(g)


def test_divergence_of_a_linear_field_at_p12():
  """u = A x has div u = tr(A) at every point of every element, curved ones
  included (the isoparametric gradient of the coordinates is exact):
  D_local(u)_k = tr(A) sum_q phi_k(x_q) w_q detJ_q."""
  c, sf = _high()
  A = np.array([[0.3, -1.1, 0.7], [0.2, 0.9, -0.4], [-0.6, 0.5, 1.7]])
  u = sf.coords @ A.T
  got = sf.div_local(sf.gather(u))
  phi = sf.W.reshape((-1,) + (P_HIGH,) * 3)       # D_local's projection of 1
  for a in range(3):
    phi = S.along(sf.Ip.T, phi, 1 + a)
  phi = phi.reshape(got.shape)
  assert np.abs(got - np.trace(A) * phi).max() <= 1e-11 * np.abs(phi).max()
  # ... and the pressure basis sums to one: the element volumes
  assert np.abs(phi.sum(axis=1) - sf.W.sum(axis=1)).max() <= 1e-14
  assert abs(sf.W.sum() - 1.0) <= 1e-13            # the mesh fills the box


def _boundary_normal_local(sf):
  """(E, n, d): int over the element's boundary of phi_i n_c dS by the GLL
  rule of each face.  On the face xi_a = +-1 the outward normal times the
  surface element is +- K[a, :] (the cofactor row), so node i takes
  +- w_face(i) K[a, c](x_i) from every face it lies on."""
  P, d = sf.P, sf.ndim
  w1 = O.quadrature_weights(P, 'gll')
  out = np.zeros((sf.num_elements,) + (P,) * d + (d,))
  K = sf.K.reshape((sf.num_elements,) + (P,) * d + (d, d))
  for a in range(d):
    wf = np.ones((P,) * d)
    for b in range(d):
      if b != a:
        shape = [1] * d
        shape[b] = P
        wf = wf * w1.reshape(shape)
    for side, sign in ((0, -1.0), (P - 1, 1.0)):
      at = [slice(None)] * (d + 1)
      at[1 + a] = side
      face = tuple(at)
      out[face] += sign * wf[tuple(at[1:])][None, ..., None] * K[face][..., a, :]
  return out.reshape(sf.num_elements, sf.n, d)


def test_gradient_of_a_constant_pressure_at_p12():
  """Dt_local(1)_{i,c} = int d phi_i / d x_c = the boundary integral of
  phi_i n_c (the GLL rule sums by parts exactly, and the cofactors of these
  elements are polynomials the nodes hold, so the metric identities hold
  discretely): zero on the nodes inside an element, the face rule on its
  faces.  Summed over the nodes of an element it is that element's
  boundary-normal integral, and assembled it vanishes on the interior nodes
  of the box."""
  c, sf = _high()
  one = np.ones(sf.pelements.shape)
  got = sf.grad_t_local(one)
  want = _boundary_normal_local(sf)
  scale = np.abs(want).max()
  assert np.abs(got - want).max() <= 1e-11 * scale
  inner = np.zeros((P_HIGH,) * 3, bool)
  inner[1:-1, 1:-1, 1:-1] = True
  assert np.abs(got[:, inner.reshape(-1)]).max() <= 1e-11 * scale
  assert np.abs(got[:, ~inner.reshape(-1)]).max() > 0.1 * scale
  # per element: the closed surface's normal integral (zero)
  assert np.abs(got.sum(axis=1) - want.sum(axis=1)).max() <= 1e-11 * scale
  assert np.abs(want.sum(axis=1)).max() <= 1e-11 * scale
  interior = ~C.boundary_mask(c)      # (the bend moves nodes of the x2 faces)
  assert 0 < interior.sum() < sf.num_nodes
  g = sf.grad_t(np.ones(sf.num_pressure_nodes))
  assert np.abs(g[interior]).max() <= 1e-11 * scale
  assert np.abs(g[~interior]).max() > 0.1 * scale


def test_convection_of_a_constant_field_at_p12():
  c, sf = _high()
  rng = np.random.default_rng(3)
  for rp, Pv in ((c.v.rp, P_HIGH), (C.overint_premesh(3, P_HIGH, False),
                                    P_HIGH - 2)):
    cs = S.ConvectionSpace(rp.node_coords, rp.elements, Pv, P_HIGH)
    const = np.broadcast_to(np.array([0.7, -1.3, 0.4]),
                            rp.elements.shape + (3,))
    size = np.abs(cs.convection_local(
        rng.standard_normal(rp.elements.shape + (3,)))).max()
    assert np.abs(cs.convection_local(const)).max() <= 1e-11 * size


# ------------------------------------ the sweep's meshes against the packing
def test_sweep_launches_fill_and_split_workgroups():
  """The launches the GPU sweep makes on these meshes (one per geometry kind,
  the kinds joined, everything): at every (ndim, P) with a tile of several
  elements one of them ends in a partial workgroup and one puts several
  elements into a workgroup, in both precisions."""
  from tests.packing import epb
  for ndim in (2, 3):
    for P in range(4, 13):
      kinds = C.expected_kind_counts(ndim, P)
      assert sum(kinds.values()) == 3 ** ndim and min(kinds.values()) >= 0
      counts = C.expected_launch_counts(ndim, P)
      for itemsize in (4, 8):
        assert C.check_packing(ndim, P, itemsize, counts) == epb(ndim, P,
                                                                 itemsize)
  assert [epb(3, P, 8) for P in range(4, 13)] == [4, 5] + [1] * 7
  assert [epb(2, P, 4) for P in range(4, 13)] == [16, 12, 10, 9, 8, 7, 6, 11,
                                                  16]
  # the kind counts are those of the reference's geometry at one order
  c, sf = _high()
  vary = np.ptp(sf.K, axis=1).max(axis=(1, 2)) / np.abs(sf.K).max()
  first = sf.points[:, :, 0].mean(axis=1) < 1.0 / 3
  want = C.expected_kind_counts(3, P_HIGH)
  assert (int(first.sum()), int((vary[~first] > 1e-2).sum()),
          int((vary < 1e-11).sum())) == (want['curved'], want['multilinear'],
                                         want['affine'])
