"""NumPy reference of the Helmholtz operator with variable coefficients,

    lambda0 B_c + lambda1 A_k,   B_c[i,j] = sum_q c_q W_q phi_i phi_j,
                                 A_k[i,j] = sum_q k_q grad phi_i . G_q grad phi_j,

the coefficient form of `pmg_reference.element_matrices` (the oracle's
geometry), applied element by element without forming the (n, n) matrices so
that 3D orders up to p = 6 stay small (above that: the sum-factorised
`tests/sumfact_reference.py`, which holds no (E, Q, n, d) gradients and
reaches P = 12 in 3D).  Also the coarse-level coefficient rule of
`linalg/pmg.py` restated."""

import numpy as np

from oracle import sfem_oracle as O


def space(coords, elements, P, quad):
  """The oracle's space: P GLL points per direction, quad = (num, type)."""
  return O.FESpace(np.asarray(coords, dtype=np.float64), elements, (P, 'gll'),
                   quad)


def quad_points(fes):
  """(E, Q, d) physical coordinates of the quadrature points."""
  return fes.quad_coords


def element_matrices(fes, l0, l1, k_q=None, c_q=None):
  """(E, n, n) element matrices of l0 B_c + l1 A_k; k_q, c_q (E, Q) or None
  (= 1)."""
  wdet = fes.jacdets * fes.weights[None, :]
  kw = wdet if k_q is None else wdet * k_q
  cw = wdet if c_q is None else wdet * c_q
  phys = np.einsum('qid,eqjd->eqij', fes.G, fes.invjacs)     # (E, Q, n, d)
  K = l1 * np.einsum('eqid,eq,eqjd->eij', phys, kw, phys, optimize=True)
  if l0:
    K = K + l0 * np.einsum('eq,qi,qj->eij', cw, fes.M, fes.M, optimize=True)
  return K


def local_apply(fes, u_local, l0, l1, k_q=None, c_q=None):
  """(E, n) -> (E, n): the element action of l0 B_c + l1 A_k."""
  wdet = fes.jacdets * fes.weights[None, :]
  kw = wdet if k_q is None else wdet * k_q
  cw = wdet if c_q is None else wdet * c_q
  phys = np.einsum('qid,eqjd->eqij', fes.G, fes.invjacs)
  g = np.einsum('eqid,ei->eqd', phys, u_local, optimize=True)
  out = l1 * np.einsum('eqid,eq,eqd->ei', phys, kw, g, optimize=True)
  if l0:
    v = np.einsum('qi,ei->eq', fes.M, u_local)
    out = out + l0 * np.einsum('qi,eq->ei', fes.M, cw * v)
  return out


def apply(fes, u, l0, l1, k_q=None, c_q=None, keep=None):
  """Assembled (N,) action, Dirichlet rows zero where keep = 0."""
  out = fes.scatter(local_apply(fes, fes.gather(u), l0, l1, k_q, c_q))
  return out if keep is None else out * keep


def diagonal(fes, l0, l1, k_q=None, c_q=None, keep=None):
  """Assembled diagonal of l0 B_c + l1 A_k."""
  wdet = fes.jacdets * fes.weights[None, :]
  kw = wdet if k_q is None else wdet * k_q
  cw = wdet if c_q is None else wdet * c_q
  phys = np.einsum('qid,eqjd->eqij', fes.G, fes.invjacs)
  d = l1 * np.einsum('eqid,eq,eqid->ei', phys, kw, phys, optimize=True)
  if l0:
    d = d + l0 * np.einsum('eq,qi->ei', cw, fes.M ** 2)
  out = fes.scatter(d)
  return out if keep is None else out * keep


def coarse_coefficient(values, weights):
  """The p-multigrid coarse-level rule: scalars and (E,) values unchanged,
  (E, Q) values -> sum_q k_q W_q / sum_q W_q per element."""
  v = np.asarray(values, dtype=np.float64)
  if v.ndim < 2:
    return v
  w = np.asarray(weights, dtype=np.float64)
  return (v * w).sum(axis=1) / w.sum(axis=1)
