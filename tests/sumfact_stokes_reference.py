"""Sum-factorised NumPy reference of the P_N - P_{N-2} Stokes operators and of
the over-integrated convection term, for any order in 2D and 3D.

Written from the formulas at the top of `csrc/sfem_stokes.h` and of
navier_stokes.py:313-338 / :238-245:

    D_local(u)_k      = sum_q phi_k(x_q) w_q detJ_q div u(x_q)
    Dt_local(p)_{i,c} = sum_q w_q detJ_q p(x_q) d phi_i / d x_c (x_q)
    C_local(u)_{i,c}  = sum_q phi_i(x_q) w_q detJ_q u_j d_j u_c (x_q)

D and D^T on the P velocity GLL points (q = the velocity nodes, phi_k the
pressure basis on PP = P - 2 Gauss points per direction), C on a q-point GLL
grid from P_v-point GLL nodes (q = P_v: collocated, no interpolation).

With J[a, j] = d x_j / d xi_a and K = the cofactor matrix of J,

    detJ d xi_a / d x_c = K[a, c],     detJ = sum_c J[0, c] K[0, c]   (signed),

so  detJ div u = sum_{a,c} K[a, c] d u_c / d xi_a  and
    detJ u_j d_j u_c = sum_a (sum_j K[a, j] u_j) d u_c / d xi_a.

Every reference derivative is one 1D contraction with the differentiation
matrix per axis, every change of basis one 1D contraction with a (P, PP) or
(q, P_v) interpolation matrix per axis: O(E d P^(d+1)) work, no array larger
than O(E P^d d^2); `oracle.sfem_oracle` holds (Q, n) Kronecker tables and
(E, Q, n, d) gradients instead and stops at P = 6 in 3D.  The geometry is
isoparametric from the velocity nodes, as in `sumfact_reference.Space`.  The
1D nodes, weights and matrices come from `oracle.sfem_oracle` (`nodes_1d`,
`quadrature_weights`, `differentiation_matrix_1d`, `interpolation_matrix_1d`).
Local nodes are lexicographic, axis 0 slowest.

`dtype=np.float32` carries the same algorithm in single precision, the 1D
matrices formed in float64 and rounded once: a float32 kernel's error can
then stand next to the algorithm's own.
"""

import numpy as np

from oracle import sfem_oracle as O


def along(mat, v, axis):
  """sum_j mat[i, j] v[..., j, ...] along `axis` of v; `mat` (m, k) may be
  rectangular: that axis changes from k to m."""
  m, k = mat.shape
  shape = v.shape
  assert shape[axis] == k, (shape, axis, mat.shape)
  pre = int(np.prod(shape[:axis]))
  post = int(np.prod(shape[axis + 1:]))
  out = np.matmul(mat, v.reshape(pre, k, post))
  return out.reshape(shape[:axis] + (m,) + shape[axis + 1:])


def cofactors(J):
  """(..., d, d) -> (cofactor matrices (..., d, d), signed determinants)."""
  d = J.shape[-1]
  K = np.empty_like(J)
  if d == 2:
    K[..., 0, 0], K[..., 0, 1] = J[..., 1, 1], -J[..., 1, 0]
    K[..., 1, 0], K[..., 1, 1] = -J[..., 0, 1], J[..., 0, 0]
  else:
    assert d == 3
    for a in range(3):
      K[..., a, :] = np.cross(J[..., (a + 1) % 3, :], J[..., (a + 2) % 3, :])
  return K, (J[..., 0, :] * K[..., 0, :]).sum(axis=-1)


def _weights_nd(w1, d):
  w = w1
  for _ in range(d - 1):
    w = np.multiply.outer(w, w1)
  return w.reshape(-1)


class _Grid:
  """Nodes on P_v GLL points per direction, work on q GLL points."""

  def __init__(self, coords, elements, Pv, q, dtype):
    self.dtype = np.dtype(dtype)
    self.coords = np.asarray(coords, dtype=dtype)
    self.elements = np.asarray(elements).astype(np.int64)
    assert (self.elements >= 0).all(), 'padded rows are not part of this'
    self.Pv, self.q = int(Pv), int(q)
    self.num_nodes, self.ndim = self.coords.shape
    self.num_elements, self.n = self.elements.shape
    d = self.ndim
    assert self.n == self.Pv ** d, (self.n, Pv, d)
    xv, xq = O.nodes_1d(self.Pv, 'gll'), O.nodes_1d(self.q, 'gll')
    # (q, P_v): values of the nodal basis at the work points
    self.I = (None if q == Pv else
              O.interpolation_matrix_1d(xv, 'gll', xq).astype(dtype))
    self.D = O.differentiation_matrix_1d(xq, 'gll').astype(dtype)
    self.w = _weights_nd(O.quadrature_weights(self.q, 'gll'), d).astype(dtype)
    E = self.num_elements
    x = self.to_grid(self.coords[self.elements])            # (E, q.., d)
    # J[e, q, a, j] = d x_j / d xi_a: the coordinates are polynomials of
    # degree P_v - 1 <= q - 1, which the q-point matrix differentiates exactly
    J = np.stack([along(self.D, x, 1 + a) for a in range(d)], axis=-2)
    self.points = x.reshape(E, -1, d)
    self.K, self.det = cofactors(J.reshape(E, -1, d, d))
    self.wK = self.w[None, :, None, None] * self.K          # (E, Q, d, d)
    self.W = self.w[None, :] * self.det                     # (E, Q)

  def to_grid(self, u_local):
    """(E, n, ...) nodal values -> (E, q, .., q, ...) on the work points."""
    d, E = self.ndim, self.num_elements
    v = np.asarray(u_local, dtype=self.dtype)
    v = v.reshape((E,) + (self.Pv,) * d + v.shape[2:])
    if self.I is not None:
      for a in range(d):
        v = along(self.I, v, 1 + a)
    return v

  def from_grid(self, c):
    """Transpose of `to_grid`: (E, q, .., q, ...) -> (E, n, ...)."""
    d, E = self.ndim, self.num_elements
    if self.I is not None:
      for a in range(d):
        c = along(self.I.T, c, 1 + a)
    return c.reshape((E, self.n) + c.shape[1 + d:])

  def ref_grad(self, v, a):
    """d / d xi_a of (E, q, .., q, ...) values on the work points."""
    return along(self.D, v, 1 + a)

  def gather(self, u):
    """(N, ...) -> (E, n, ...)."""
    return np.asarray(u, dtype=self.dtype)[self.elements]

  def scatter(self, u_local):
    out = np.zeros((self.num_nodes,) + u_local.shape[2:], dtype=u_local.dtype)
    np.add.at(out, self.elements, u_local)
    return out


class StokesSpace(_Grid):
  """`vcoords` (Nv, d) and `velements` (E, P^d) of the velocity mesh,
  `pelements` (E, (P-2)^d) any pressure index rows (their node count is
  `num_pressure_nodes`, default max id + 1)."""

  def __init__(self, vcoords, velements, pelements, P, dtype=np.float64,
               num_pressure_nodes=None):
    super().__init__(vcoords, velements, P, P, dtype)
    self.P, self.PP = int(P), int(P) - 2
    self.pelements = np.asarray(pelements).astype(np.int64)
    assert self.pelements.shape == (self.num_elements, self.PP ** self.ndim)
    self.num_pressure_nodes = (int(self.pelements.max()) + 1
                               if num_pressure_nodes is None
                               else int(num_pressure_nodes))
    # (P, PP): phi_k(x_q), the Gauss basis of the pressure at the GLL points
    self.Ip = O.interpolation_matrix_1d(
        O.nodes_1d(self.PP, 'gl'), 'gl', O.nodes_1d(self.P, 'gll')).astype(dtype)

  def div_local(self, u_local):
    """(E, P^d, d) -> (E, PP^d)."""
    d, E = self.ndim, self.num_elements
    u = self.to_grid(u_local)                                # (E, P.., d)
    t = np.zeros((E, self.q ** d), dtype=self.dtype)
    for a in range(d):
      g = self.ref_grad(u, a).reshape(E, -1, d)
      t += (self.wK[:, :, a, :] * g).sum(axis=-1)
    t = t.reshape((E,) + (self.P,) * d)
    for a in range(d):
      t = along(self.Ip.T, t, 1 + a)
    return t.reshape(E, -1)

  def grad_t_local(self, p_local):
    """(E, PP^d) -> (E, P^d, d): the transpose of `div_local`."""
    d, E = self.ndim, self.num_elements
    p = np.asarray(p_local, dtype=self.dtype).reshape((E,) + (self.PP,) * d)
    for a in range(d):
      p = along(self.Ip, p, 1 + a)
    p = p.reshape(E, -1)
    out = np.zeros((E,) + (self.P,) * d + (d,), dtype=self.dtype)
    for a in range(d):
      flux = (self.wK[:, :, a, :] * p[..., None]).reshape(out.shape)
      out += along(self.D.T, flux, 1 + a)
    return out.reshape(E, self.n, d)

  # ---- both spaces assembled
  def pgather(self, p):
    return np.asarray(p, dtype=self.dtype)[self.pelements]

  def pscatter(self, p_local):
    out = np.zeros(self.num_pressure_nodes, dtype=p_local.dtype)
    np.add.at(out, self.pelements, p_local)
    return out

  def div(self, u):
    """(Nv, d) -> (Np,)."""
    return self.pscatter(self.div_local(self.gather(u)))

  def grad_t(self, p):
    """(Np,) -> (Nv, d), no Dirichlet rows removed."""
    return self.scatter(self.grad_t_local(self.pgather(p)))


class ConvectionSpace(_Grid):
  """C_local on a q-point GLL grid from P_v-point GLL nodes (q >= P_v)."""

  def __init__(self, coords, elements, Pv, q, dtype=np.float64):
    assert q >= Pv
    super().__init__(coords, elements, Pv, q, dtype)

  def convection_local(self, u_local):
    """(E, P_v^d, d) -> (E, P_v^d, d)."""
    d, E = self.ndim, self.num_elements
    u = self.to_grid(u_local)                                # (E, q.., d)
    uq = u.reshape(E, -1, d)
    c = np.zeros_like(uq)
    for a in range(d):
      contra = (self.wK[:, :, a, :] * uq).sum(axis=-1)       # w detJ u . grad xi_a
      c += contra[..., None] * self.ref_grad(u, a).reshape(E, -1, d)
    return self.from_grid(c.reshape(u.shape))
