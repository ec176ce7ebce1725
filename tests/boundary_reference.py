"""NumPy restatement of the boundary facet kernels (tests only):
`sfem_boundary_geom`, `sfem_boundary_covector`, `sfem_boundary_mass_apply`,
`sfem_boundary_mass_diag` and `sfem_boundary_add_rows`
(`swirl_fem_amd/csrc/sfem_boundary.hip`, definitions in `include/sfem.h`).

The matrices are arguments (B (q, p1), D_q (q, p1), w (q,)), not a quadrature
object, so that any pair and any matrix can be fed.  A facet of a d-dim mesh
has k = d - 1 axes and p1^k nodes; the layout is that of
`bvp_reference.facet_matrices`: the first Kronecker factor sits on the slow
index.  k is read off the width of `facets` (p1 or p1^2).

float64 by default.  `dtype=np.float32` evaluates the same contractions, one
axis after the other as the kernels do, with every intermediate in float32:
that sizes the fp32 allowance of the GPU tests and is no oracle.  `add_rows`
is the exception: the kernel does pure additions in a fixed order, which the
loop here repeats bit for bit in either dtype.

Checked on the CPU by `tests/test_boundary_reference_host.py`; the synthetic
inputs of the GPU sweep (`tests/test_gpu_boundary_kernels.py`) are here too,
so that both files see the same numbers."""
import functools

import numpy as np

from tests.fp32util import F32Rng, f32r

# (p1, q): the pairs compiled with fixed sizes, and pairs that take the
# run-time path (q < p1, q > p1 + 1, p1 >= 14, the corners of 16 x 16)
COMPILED_PAIRS = [(n, n + e) for n in range(2, 14) for e in (0, 1)]
RUNTIME_PAIRS = [(2, 1), (5, 3), (3, 7), (2, 16), (13, 15), (14, 14),
                 (14, 15), (15, 16), (16, 16), (16, 1)]
PAIRS = COMPILED_PAIRS + RUNTIME_PAIRS


def facet_dim(facets, p1):
  """k = 1 (edges of a 2D mesh) or 2 (faces of a 3D mesh)."""
  width = np.asarray(facets).shape[1]
  if width == p1:
    return 1
  if width == p1 * p1:
    return 2
  raise ValueError(f'facets of width {width} with p1 = {p1}')


def swap_axes(a, n):
  """(F, n * n, ...) with the two facet axes exchanged."""
  a = np.asarray(a)
  t = a.reshape((a.shape[0], n, n) + a.shape[2:])
  return np.ascontiguousarray(np.swapaxes(t, 1, 2)).reshape(a.shape)


def interp(m, v, k):
  """(m (x) m) v: v (F, ni^k, ...) -> (F, no^k, ...), m (no, ni); the slow
  axis first."""
  no, ni = m.shape
  F = v.shape[0]
  if k == 1:
    return np.einsum('ai,fi...->fa...', m, v)
  t = v.reshape((F, ni, ni) + v.shape[2:])
  t = np.einsum('ai,fij...->faj...', m, t)
  t = np.einsum('cj,faj...->fac...', m, t)
  return t.reshape((F, no * no) + v.shape[2:])


def tangents(X, B, Dq, k):
  """[(D_q (x) B) X, (B (x) D_q) X] (k = 2) or [D_q X] (k = 1); X (F, p1^k,
  d)."""
  if k == 1:
    return [np.einsum('ai,fid->fad', Dq, X)]
  F, d = X.shape[0], X.shape[2]
  q, p1 = B.shape
  t = X.reshape(F, p1, p1, d)
  bs = np.einsum('ai,fijd->fajd', B, t)
  ds = np.einsum('ai,fijd->fajd', Dq, t)
  ts = np.einsum('cj,fajd->facd', B, ds).reshape(F, q * q, d)
  tt = np.einsum('cj,fajd->facd', Dq, bs).reshape(F, q * q, d)
  return [ts, tt]


def point_weights(w, k):
  """w[a] (k = 1) or w[a] * w[c] at point (a, c), a slow."""
  w = np.asarray(w)
  return w if k == 1 else (w[:, None] * w[None, :]).reshape(-1)


def facet_jacobian(coords, facets, B, Dq, dtype=np.float64):
  """(xq (F, q^k, d), |x_s| or |x_s x x_t| (F, q^k))."""
  coords, B, Dq = (np.asarray(a, dtype) for a in (coords, B, Dq))
  facets = np.asarray(facets)
  k = facet_dim(facets, B.shape[1])
  X = coords[facets]                                   # (F, p1^k, d)
  xq = interp(B, X, k)
  ts = tangents(X, B, Dq, k)
  if k == 1:
    n2 = (ts[0] * ts[0]).sum(axis=-1, dtype=dtype)
  else:
    n = np.cross(ts[0], ts[1])
    n2 = (n * n).sum(axis=-1, dtype=dtype)
  return xq, np.sqrt(n2)


def geom(coords, facets, B, Dq, w, dtype=np.float64):
  """`sfem_boundary_geom`: (xq (F, q^k, d), wJ (F, q^k))."""
  xq, jac = facet_jacobian(coords, facets, B, Dq, dtype)
  k = facet_dim(facets, np.asarray(B).shape[1])
  return xq, point_weights(np.asarray(w, dtype), k)[None, :] * jac


def covector_local(g, nodal, facets, wJ, B, dtype=np.float64):
  """`sfem_boundary_covector`: (F, p1^k) = (B (x) B)^T (wJ g); g (N,) nodal
  values (`nodal`) or (F, q^k) at the points."""
  g, wJ, B = (np.asarray(a, dtype) for a in (g, wJ, B))
  facets = np.asarray(facets)
  k = facet_dim(facets, B.shape[1])
  gq = interp(B, g[facets], k) if nodal else g
  return interp(B.T, wJ * gq, k)


def mass_local(u, encoded, aw, B, scale, diag, dtype=np.float64):
  """`sfem_boundary_mass_apply` (`diag` false): (F, p1^k) = scale (B (x) B)^T
  (aw (B (x) B) u_f), or `sfem_boundary_mass_diag`: scale (B.B (x) B.B)^T aw
  (u unread).  A slot of `encoded` stored as ~id reads 0 and writes 0."""
  aw, B = np.asarray(aw, dtype), np.asarray(B, dtype)
  encoded = np.asarray(encoded)
  k = facet_dim(encoded, B.shape[1])
  keep = encoded >= 0
  scale = dtype(scale)
  if diag:
    r = interp((B * B).T, scale * aw, k)
  else:
    ids = np.where(keep, encoded, ~encoded)
    uf = np.where(keep, np.asarray(u, dtype)[ids], dtype(0))
    r = interp(B.T, interp(B, uf, k) * (scale * aw), k)
  return np.where(keep, r, dtype(0))


def add_rows(local, rows, offsets, slots, out, dtype=np.float64):
  """`sfem_boundary_add_rows`: a copy of `out` with out[rows[r]] += the sum
  of local[slots[offsets[r]:offsets[r + 1]]] taken in slot order, every
  partial sum rounded to `dtype`."""
  local = np.asarray(local, dtype).reshape(-1)
  out = np.array(out, dtype)
  for r, v in enumerate(np.asarray(rows)):
    acc = dtype(0)
    for s in range(int(offsets[r]), int(offsets[r + 1])):
      acc = dtype(acc + local[slots[s]])
    out[v] = dtype(out[v] + acc)
  return out


# ------------------------------------------------- the inputs of the sweep
def facet_ids(rng, F, nf, N):
  """(F, nf) int32 ids in [0, N): no repetition inside a facet, every facet
  shares ids with the one before it, ids 0 and N - 1 present."""
  rows = []
  for f in range(F):
    row = rng.choice(N, nf, replace=False)
    if f:
      m = max(1, nf // 4)
      shared = rng.choice(rows[-1], m, replace=False)
      rest = rng.permutation(np.setdiff1d(row, shared))[:nf - m]
      row = rng.permutation(np.concatenate([shared, rest]))
    rows.append(row)
  ids = np.asarray(rows, dtype=np.int64).reshape(F, nf)
  for f, want in ((0, 0), (F - 1, N - 1)):
    if F and want not in ids[f]:
      free = np.nonzero((ids[f] != 0) & (ids[f] != N - 1))[0]
      ids[f, rng.choice(free)] = want
  for row in ids:
    assert len(set(row.tolist())) == nf
  if F:
    assert ids.min() == 0 and ids.max() == N - 1
  if F > 1:
    assert len(set(ids.reshape(-1).tolist())) < ids.size      # shared ids
  return ids.astype(np.int32)


def matrices(rng, p1, q, f32=False):
  """(B, D_q, w): B = (eye-like q x p1 block) + randn / sqrt(p1), D_q randn,
  w uniform on (0.5, 1.5): non-symmetric, different from each other, no
  partition of unity."""
  B = np.eye(q, p1) + rng.standard_normal((q, p1)) / np.sqrt(p1)
  B = f32r(B) if f32 else B
  Dq = rng.standard_normal((q, p1))
  w = rng.uniform(0.5, 1.5, q)
  assert len(set(w.tolist())) == q
  return B, Dq, w


@functools.lru_cache(maxsize=None)
def synthetic(ndim, p1, q, f32=False, F=5, seed=0):
  """The inputs of one case as a dict of float64 / int32 arrays (float32-
  representable with `f32`).  Cached: callers must not write into them."""
  rng = (F32Rng if f32 else np.random.default_rng)(
      100000 * seed + 10000 * ndim + 100 * p1 + q)
  k = ndim - 1
  nf, nq = p1 ** k, q ** k
  N = 3 * 5 * nf + 7 if F == 0 else 3 * F * nf + 7
  B, Dq, w = matrices(rng, p1, q, f32)
  scale = -1.7
  a = dict(
      ndim=ndim, p1=p1, q=q, k=k, N=N, F=F, B=B, Dq=Dq, w=w,
      facets=facet_ids(rng, F, nf, N),
      coords=rng.standard_normal((N, ndim)),
      wJ=rng.uniform(0.5, 1.5, (F, nq)), aw=rng.uniform(0.5, 1.5, (F, nq)),
      g_nodal=rng.standard_normal(N), g_points=rng.standard_normal((F, nq)),
      u=rng.standard_normal(N), scale=float(f32r(scale)) if f32 else scale)
  for v in a.values():
    if isinstance(v, np.ndarray):
      v.setflags(write=False)
  return a


def mask_nodes(a, fraction=0.3, seed=0):
  """(masked (N,) bool with about `fraction` of the nodes and node 0 always,
  encoded facets: ~id in every slot that holds a masked node)."""
  rng = np.random.default_rng(seed + a['N'])
  masked = rng.uniform(size=a['N']) < fraction
  if fraction > 0:
    masked[0] = True
  facets = a['facets']
  return masked, np.where(masked[facets], ~facets, facets).astype(np.int32)


def evaluate(a, dtype=np.float64, encoded=None, u=None):
  """Every output of the sweep for the inputs `a`."""
  enc = a['facets'] if encoded is None else encoded
  u = a['u'] if u is None else u
  xq, wJ = geom(a['coords'], a['facets'], a['B'], a['Dq'], a['w'], dtype)
  return {
      'geom.xq': xq, 'geom.wJ': wJ,
      'covector.nodal': covector_local(a['g_nodal'], True, a['facets'],
                                       a['wJ'], a['B'], dtype),
      'covector.points': covector_local(a['g_points'], False, a['facets'],
                                        a['wJ'], a['B'], dtype),
      'mass_apply': mass_local(u, enc, a['aw'], a['B'], a['scale'], False,
                               dtype),
      'mass_diag': mass_local(None, enc, a['aw'], a['B'], a['scale'], True,
                              dtype)}


def add_rows_inputs(num_rows, seed=0, f32=False):
  """(local, rows, offsets, slots, out): `rows` a random subset of a longer
  `out` in random order, 0..9 slots per row with empty rows first, last and
  in the middle (one row: five slots), slots that repeat, `out` a pattern
  that no sum reproduces."""
  rng = (F32Rng if f32 else np.random.default_rng)(seed + num_rows)
  n_out = 2 * num_rows + 13
  rows = rng.choice(n_out, num_rows, replace=False).astype(np.int32)
  counts = rng.integers(0, 10, num_rows)
  if num_rows == 1:
    counts[:] = 5
  elif num_rows:
    counts[[0, num_rows // 2, num_rows - 1]] = 0
    counts[1] = 9
  offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
  n_local = int(offsets[-1]) + 11
  slots = rng.integers(0, n_local, int(offsets[-1])).astype(np.int32)
  local = rng.standard_normal(n_local)
  out = 1000.5 + 0.25 * np.arange(n_out)
  return local, rows, offsets, slots, out


def relerr(got, want):
  """max |got - want| over the largest entry of `want`."""
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  assert got.shape == want.shape, (got.shape, want.shape)
  if want.size == 0:
    return 0.0
  return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))
