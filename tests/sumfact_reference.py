"""Sum-factorised NumPy reference of the collocated-GLL Helmholtz operator

    lambda0 B_c + lambda1 A_k,   B_c[i,j] = sum_q c_q W_q phi_i phi_j,
                                 A_k[i,j] = sum_q k_q grad phi_i . G_q grad phi_j

(the form stated at the top of `tests/coefficient_reference.py`) for any order
in 2D and 3D.  With the quadrature points on the nodes phi_i(x_q) = delta_iq,
so B_c is diagonal and a reference gradient is one 1D contraction with the
derivative matrix per axis: O(E d P^(d+1)) work and no array larger than
O(E P^d d^2), where `coefficient_reference` and the oracle hold (Q, n) basis
tables and (E, Q, n, d) gradients (P^6 in 3D: p = 6 at most).

The geometry is isoparametric: the Jacobian of every element is the same 1D
contraction applied to its own nodal coordinates, so affine, multilinear and
curved elements take one path.  With J[a, j] = d x_j / d xi_a at a point,

    G = w det(J) J^-1 J^-T   (G[a, b] = w det sum_j dxi_a/dx_j dxi_b/dx_j),
    W = w det(J),

the signed determinant as in the oracle.  Local nodes are lexicographic, axis 0
slowest.  The 1D GLL nodes, weights and derivative matrix come from
`oracle.sfem_oracle` (`nodes_1d`, `quadrature_weights`,
`differentiation_matrix_1d`); everything else is written here from the
formulas above.
"""

import numpy as np

from oracle import sfem_oracle as O


def _along(mat, v, axis):
  """sum_j mat[i, j] v[..., j, ...] along `axis` of v (square `mat`)."""
  shape = v.shape
  pre = int(np.prod(shape[:axis]))
  post = int(np.prod(shape[axis + 1:]))
  if post == 1:
    return (v.reshape(pre, shape[axis]) @ mat.T).reshape(shape)
  return np.matmul(mat, v.reshape(pre, shape[axis], post)).reshape(shape)


class Space:
  """`coords` (N, d), `elements` (E, P^d) rows (-1: a padding slot, whose
  coordinates read as 0 like the oracle's gather; a row of -1 only: a padded
  element, which contributes nothing), P points per direction.  `dtype`
  float32 carries the same algorithm in single precision (the 1D matrices
  rounded once), to put a float32 kernel's error next to the algorithm's own."""

  def __init__(self, coords, elements, P, dtype=np.float64):
    self.dtype = np.dtype(dtype)
    self.coords = np.asarray(coords, dtype=dtype)
    self.elements = np.asarray(elements).astype(np.int64)
    self.P = int(P)
    self.num_nodes, self.ndim = self.coords.shape
    self.num_elements, self.n = self.elements.shape
    d = self.ndim
    assert self.n == self.P ** d, (self.n, P, d)
    x1 = O.nodes_1d(self.P, 'gll')
    self.D = O.differentiation_matrix_1d(x1, 'gll').astype(dtype)
    w1 = O.quadrature_weights(self.P, 'gll')
    w = w1
    for _ in range(d - 1):
      w = np.multiply.outer(w, w1)
    self.valid = self.elements >= 0                              # (E, n)
    self.real = self.valid.any(axis=1)                           # (E,)
    xe = np.where(self.valid[..., None],
                  self.coords[np.where(self.valid, self.elements, 0)],
                  0).astype(dtype)                               # (E, n, d)
    self._points = xe
    E = self.num_elements
    grid = xe.reshape((E,) + (self.P,) * d + (d,))
    # J[e, q, a, j] = d x_j / d xi_a
    J = np.stack([_along(self.D, grid, 1 + a) for a in range(d)],
                 axis=-2).reshape(E, self.n, d, d)
    J[~self.real] = np.eye(d, dtype=dtype)
    det = np.linalg.det(J).astype(dtype)
    inv = np.linalg.inv(J).astype(dtype)             # inv[j, a] = dxi_a/dx_j
    self.W = (w.reshape(-1).astype(dtype)[None, :] * det)        # (E, n)
    self.G = self.W[..., None, None] * np.einsum('eqja,eqjb->eqab', inv, inv)
    self.W[~self.real] = 0
    self.G[~self.real] = 0

  # ------------------------------------------------------------- pieces
  def quad_points(self):
    """(E, P^d, d) physical coordinates of the quadrature points: collocated
    GLL, so the element's own node coordinates."""
    return self._points

  def _apply(self, G, W, u, l0, l1, k_q, c_q):
    """Element action on u (E', n, nc) with geometry G (E', n, d, d), W."""
    d, P = self.ndim, self.P
    Ep, n, nc = u.shape
    out = np.zeros_like(u)
    if l1:
      grid = u.reshape((Ep,) + (P,) * d + (nc,))
      ref = [_along(self.D, grid, 1 + a).reshape(Ep, n, nc) for a in range(d)]
      Gk = G if k_q is None else G * k_q[..., None, None]
      for a in range(d):
        flux = sum(Gk[:, :, a, b, None] * ref[b] for b in range(d))
        flux = flux.reshape((Ep,) + (P,) * d + (nc,))
        out += l1 * _along(self.D.T, flux, 1 + a).reshape(Ep, n, nc)
    if l0:
      Wc = W if c_q is None else W * c_q
      out += l0 * Wc[..., None] * u
    return out

  def local_apply(self, u_local, l0, l1, k_q=None, c_q=None):
    """(E, n[, nc]) -> the same shape: the element action of l0 B_c + l1 A_k;
    k_q, c_q (E, n) values at the points, or None (= 1)."""
    u = np.asarray(u_local, dtype=self.dtype)
    v = u[..., None] if u.ndim == 2 else u
    k_q = None if k_q is None else np.asarray(k_q, dtype=self.dtype)
    c_q = None if c_q is None else np.asarray(c_q, dtype=self.dtype)
    out = self._apply(self.G, self.W, v, l0, l1, k_q, c_q)
    return out[..., 0] if u.ndim == 2 else out

  def gather(self, u):
    """(N,) or (N, nc) -> (E, n[, nc]); padding slots read 0."""
    u = np.asarray(u, dtype=self.dtype)
    ul = u[np.where(self.valid, self.elements, 0)]
    return ul * (self.valid if u.ndim == 1 else self.valid[..., None])

  def scatter(self, u_local):
    out = np.zeros((self.num_nodes,) + u_local.shape[2:], dtype=u_local.dtype)
    np.add.at(out, self.elements[self.valid], u_local[self.valid])
    return out

  def apply(self, u, l0, l1, k_q=None, c_q=None, keep=None):
    """Assembled action on u (N,) or (N, nc); rows with keep = 0 (Dirichlet)
    are zero."""
    out = self.scatter(self.local_apply(self.gather(u), l0, l1, k_q, c_q))
    if keep is None:
      return out
    keep = np.asarray(keep, dtype=self.dtype)
    return out * (keep if out.ndim == 1 else keep[:, None])

  def local_diagonal(self, l0, l1, k_q=None, c_q=None, elements=None):
    """(E, n) element diagonals: `_apply` on the n unit vectors of one element
    at a time (rows of `elements` only, the rest 0)."""
    eye = np.eye(self.n, dtype=self.dtype)[None]                # (1, n, nc=n)
    d = np.zeros((self.num_elements, self.n), dtype=self.dtype)
    todo = range(self.num_elements) if elements is None else elements
    for e in todo:
      if not self.real[e]:
        continue
      s = slice(e, e + 1)
      col = self._apply(self.G[s], self.W[s], eye, l0, l1,
                        None if k_q is None else
                        np.asarray(k_q, dtype=self.dtype)[s],
                        None if c_q is None else
                        np.asarray(c_q, dtype=self.dtype)[s])
      d[e] = np.einsum('ii->i', col[0])
    return d

  def diagonal(self, l0, l1, k_q=None, c_q=None, keep=None, elements=None):
    """Assembled diagonal of l0 B_c + l1 A_k (of the rows of `elements` only,
    if given)."""
    out = self.scatter(self.local_diagonal(l0, l1, k_q, c_q, elements))
    return out if keep is None else out * np.asarray(keep, dtype=self.dtype)
