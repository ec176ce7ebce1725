"""NumPy reference of the Helmholtz operator with an advective term,

    lambda0 B_c + lambda1 A_k + C_b,
    C_b[i,j] = sum_q W_q phi_i(q) b_q . grad phi_j(q),

the plain Galerkin convective form on top of `tests/coefficient_reference.py`
(same geometry, same index convention: phys = einsum('qid,eqjd->eqij', G,
invjacs) are the physical gradients of the basis).  The velocity `b_q` is an
(E, Q, d) array at the quadrature points, or None (no term); it is scaled by
neither lambda."""

import numpy as np

from tests import coefficient_reference as R

space = R.space
quad_points = R.quad_points


def _phys(fes):
  return np.einsum('qid,eqjd->eqij', fes.G, fes.invjacs)        # (E, Q, n, d)


def _wdet(fes):
  return fes.jacdets * fes.weights[None, :]


def advection_matrices(fes, b_q):
  """(E, n, n) element matrices of C_b."""
  return element_matrices(fes, 0.0, 0.0, b_q=b_q)


def element_matrices(fes, l0, l1, k_q=None, c_q=None, b_q=None):
  """(E, n, n) dense element matrices of l0 B_c + l1 A_k + C_b, element by
  element as matrix products (the einsum form of
  `coefficient_reference.element_matrices` takes minutes at 3D order 8)."""
  wdet = _wdet(fes)
  E, Q = wdet.shape
  n, d = fes.M.shape[1], fes.ndim
  out = np.zeros((E, n, n))
  for e in range(E):
    phys = np.einsum('qid,qjd->qij', fes.G, fes.invjacs[e])        # (Q, n, d)
    if l1:
      kw = wdet[e] if k_q is None else wdet[e] * k_q[e]
      g = phys.transpose(0, 2, 1).reshape(Q * d, n)
      out[e] += l1 * (g.T * np.repeat(kw, d)[None, :]) @ g
    if l0:
      cw = wdet[e] if c_q is None else wdet[e] * c_q[e]
      out[e] += l0 * (fes.M.T * cw[None, :]) @ fes.M
    if b_q is not None:
      bg = np.einsum('qj,qij->qi', b_q[e], phys)                   # (Q, n)
      out[e] += (fes.M.T * wdet[e][None, :]) @ bg
  return out


def advection_local(fes, u_local, b_q):
  """(E, n) -> (E, n): out_i = sum_q M[q,i] wdet[e,q] sum_j b[e,q,j] g[e,q,j]
  with g the physical gradient of the element's interpolant."""
  g = np.einsum('eqid,ei->eqd', _phys(fes), u_local, optimize=True)
  return np.einsum('qi,eq->ei', fes.M,
                   _wdet(fes) * np.einsum('eqj,eqj->eq', b_q, g))


def local_apply(fes, u_local, l0, l1, k_q=None, c_q=None, b_q=None):
  out = R.local_apply(fes, u_local, l0, l1, k_q, c_q)
  return out if b_q is None else out + advection_local(fes, u_local, b_q)


def apply(fes, u, l0, l1, k_q=None, c_q=None, b_q=None, keep=None):
  """Assembled (N,) action, Dirichlet rows zero where keep = 0."""
  out = fes.scatter(local_apply(fes, fes.gather(u), l0, l1, k_q, c_q, b_q))
  return out if keep is None else out * keep


def diagonal(fes, l0, l1, k_q=None, c_q=None, b_q=None, keep=None):
  """Assembled diagonal of l0 B_c + l1 A_k + C_b."""
  out = R.diagonal(fes, l0, l1, k_q, c_q)
  if b_q is not None:
    d = np.einsum('qi,eq,eqj,eqij->ei', fes.M, _wdet(fes), b_q, _phys(fes),
                  optimize=True)
    out = out + fes.scatter(d)
  return out if keep is None else out * keep


def collocated_diagonal(fes, l0, l1, k_q=None, c_q=None, b_q=None, keep=None):
  """`diagonal` of a collocated space (quadrature points = nodes, M = I) in
  closed form, with nothing larger than the (Q, n, d) table, so that it
  reaches P = 12 in 3D:

      mass       l0 c_i W_i
      stiffness  l1 sum_q k_q W_q |grad phi_i(q)|^2
                 = l1 sum_{a,b} sum_q G[q,i,a] G[q,i,b] (k W J^-T J^-1)[q,a,b]
      advection  W_i b_i . grad phi_i(x_i)

  (phi_i(q) = delta_iq: of the advective row only the point i itself is
  left, which needs the diagonal G[i,i,:] of the table alone)."""
  Q, n, d = fes.G.shape
  assert Q == n and np.array_equal(fes.M, np.eye(n)), 'collocated spaces only'
  wdet = _wdet(fes)
  out = np.zeros_like(wdet)
  if l0:
    out += l0 * (wdet if c_q is None else wdet * c_q)
  if l1:
    kw = wdet if k_q is None else wdet * k_q
    H = np.einsum('eqja,eqjb->eqab', fes.invjacs, fes.invjacs) * \
        kw[..., None, None]
    for a in range(d):
      for b in range(d):
        out += l1 * H[..., a, b] @ (fes.G[..., a] * fes.G[..., b])
  if b_q is not None:
    i = np.arange(n)
    grad = np.einsum('id,eijd->eij', fes.G[i, i, :], fes.invjacs)   # (E, n, d)
    out += wdet * np.einsum('eij,eij->ei', b_q, grad)
  out = fes.scatter(out)
  return out if keep is None else out * keep


def assemble(fes, mats):
  """(N, N) dense matrix from (E, n, n) element matrices (padding slots of the
  index rows, -1, skipped)."""
  A = np.zeros((fes.num_nodes, fes.num_nodes))
  for row, m in zip(np.asarray(fes.elements, np.int64), mats):
    ok = row >= 0
    A[np.ix_(row[ok], row[ok])] += m[np.ix_(ok, ok)]
  return A
