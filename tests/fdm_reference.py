"""NumPy restatement of the Schwarz preconditioner's kernels
(`swirl_fem_amd/csrc/sfem_fdm.hip`) for the tests, written from the formula in
that file's header and not from its loops:

    z_e = (S_0 (x) .. (x) S_{d-1}) [ w_e .* (S_0 (x) .. (x) S_{d-1})^T r_e ]

with S_a = S[cases[a][e]] (rows = nodes, columns = modes) and the LAST axis
of an element's Pp^d values the fastest.  `tests/test_fdm_reference_host.py`
checks it against the dense Kronecker product and against
`SchwarzPressurePreconditioner.local_solve_torch`.

The Chebyshev polynomial of `sfem_ell_chebyshev` is
`tests/pmg_reference.coarse_chebyshev`; `ell_chebyshev` only picks its
precision and `ell_from_csr` lays a sparse matrix out as the kernel reads it.
"""
import numpy as np


def _contract(t, mats, a, transpose):
  """Axis 1 + a of t (E, Pp, ..) with the elements' matrices (E, Pp, Pp):
  out_m = sum_i S[i, m] t_i (`transpose`) or out_i = sum_m S[i, m] t_m."""
  t = np.moveaxis(t, 1 + a, -1)
  spec = 'eim,e...i->e...m' if transpose else 'eim,e...m->e...i'
  return np.moveaxis(np.einsum(spec, mats, t), -1, 1 + a)


def fdm_solve(r, pel, S, cases, w, ndim, Pp, dtype=np.float64):
  """z of `sfem_fdm_solve`.  r (N,); pel (E, Pp^d) node ids or None for
  arange; S (C, Pp, Pp); cases (ndim, E); w (E Pp^d values, any shape).
  `dtype=np.float32`: the same formula with every operand and every sum in
  single precision.  Entries of z outside `pel` are zero."""
  cases = np.asarray(cases).reshape(ndim, -1)
  E = cases.shape[1]
  n = Pp ** ndim
  r = np.asarray(r, dtype=dtype)
  S = np.asarray(S, dtype=dtype).reshape(-1, Pp, Pp)
  pel = (np.arange(E * n) if pel is None else np.asarray(pel)).reshape(E, n)
  shape = (E,) + (Pp,) * ndim
  t = r[pel].reshape(shape)
  for a in range(ndim):
    t = _contract(t, S[cases[a]], a, True)
  t = t * np.asarray(w, dtype=dtype).reshape(shape)
  for a in range(ndim):
    t = _contract(t, S[cases[a]], a, False)
  assert t.dtype == dtype
  z = np.zeros_like(r)
  z[pel.reshape(-1)] = t.reshape(-1)
  return z


def fdm_sums(r, z, pel, weights):
  """(element sums of r, the elements' shares of weights . z) of
  `sfem_fdm_solve_sums`; pel (E, n)."""
  return r[pel].sum(1), (weights[pel] * z[pel]).sum(1)


def add_element_constants(z, yc, shift, n, elems_per_member):
  """z[e n + i] + (yc[e] - shift[e // elems_per_member])."""
  E = len(yc)
  c = yc - shift[np.arange(E) // elems_per_member]
  return (z.reshape(E, n) + c[:, None]).reshape(-1)


def ell_from_csr(A):
  """(cols, vals), each (width, n): the column-major ELL storage of a CSR
  matrix with the padding of the preconditioner's builder (`_build_coarse`:
  column 0, value 0).  Entry k of row i at [k, i]."""
  A = A.tocsr()
  A.sort_indices()
  n = A.shape[0]
  count = np.diff(A.indptr)
  width = max(1, int(count.max()))
  cols = np.zeros((n, width), dtype=np.int32)
  vals = np.zeros((n, width), dtype=np.float64)
  row = np.repeat(np.arange(n), count)
  slot = np.arange(A.nnz) - np.repeat(A.indptr[:-1], count)
  cols[row, slot] = A.indices
  vals[row, slot] = A.data
  return np.ascontiguousarray(cols.T), np.ascontiguousarray(vals.T)


def ell_chebyshev(A, dinv, b, steps, lmin, lmax, dtype=np.float64):
  """x of `sfem_ell_chebyshev` for the CSR matrix A:
  `pmg_reference.coarse_chebyshev`.  `dtype=np.float32`: the same function on
  float32 operands (matrix, vectors and every sum in single precision; the
  scalars of the recurrence are Python floats, which NumPy rounds to the
  arrays' type) -- what single precision costs on these inputs."""
  from tests import pmg_reference
  x = pmg_reference.coarse_chebyshev(
      A.astype(dtype), np.asarray(dinv, dtype), np.asarray(b, dtype), steps,
      float(lmin), float(lmax))
  assert x.dtype == dtype, x.dtype
  return x
