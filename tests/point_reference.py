"""NumPy reference for fields at points: the order-P nodal map
of an element and its Jacobian, a Newton locator with the rules of
`sfem_point_locate`, the dense evaluation matrix, and the test points.

Element nodes are lexicographic with axis 0 slowest: node n = (i P1 + j) P1 + k
carries l_i(xi_0) l_j(xi_1) l_k(xi_2).  Everything is float64.
"""
import numpy as np


def lagrange(nodes, x):
  """(values (M, P1), derivatives (M, P1)) of the Lagrange polynomials on
  `nodes` at `x` (M,), in the product form (finite at the nodes)."""
  nodes = np.asarray(nodes, np.float64)
  x = np.asarray(x, np.float64).reshape(-1)
  P1 = len(nodes)
  diff = nodes[:, None] - nodes[None, :]
  np.fill_diagonal(diff, 1.0)
  w = 1.0 / diff.prod(axis=1)
  d = x[:, None] - nodes[None, :]                       # (M, P1)
  val = np.empty((len(x), P1))
  der = np.zeros((len(x), P1))
  for i in range(P1):
    others = [k for k in range(P1) if k != i]
    val[:, i] = w[i] * d[:, others].prod(axis=1)
    for m in others:
      rest = [k for k in others if k != m]
      der[:, i] += w[i] * d[:, rest].prod(axis=1)
  return val, der


def shape_functions(nodes, xi):
  """(phi (M, n), dphi (M, n, d)) of the tensor-product basis at xi (M, d)."""
  xi = np.asarray(xi, np.float64)
  M, d = xi.shape
  ld = [lagrange(nodes, xi[:, a]) for a in range(d)]
  letters = 'ijk'[:d]
  spec = ','.join('m' + c for c in letters) + '->m' + letters
  phi = np.einsum(spec, *[ld[a][0] for a in range(d)]).reshape(M, -1)
  dphi = np.stack([
      np.einsum(spec, *[ld[b][1 if b == a else 0] for b in range(d)]
                ).reshape(M, -1) for a in range(d)], axis=-1)
  return phi, dphi


def nodal_map(coords, elements, nodes, element, xi):
  """x (M, d) and J[m, a, b] = d x_a / d xi_b of the points (element, xi)."""
  X = np.asarray(coords, np.float64)[np.asarray(elements)[element]]  # (M,n,d)
  phi, dphi = shape_functions(nodes, xi)
  return (np.einsum('mn,mna->ma', phi, X),
          np.einsum('mnb,mna->mab', dphi, X))


def element_boxes(coords, elements):
  """(lo (E, d), hi (E, d), real (E,)) of the node bounding boxes; rows with a
  -1 are not real."""
  el = np.asarray(elements)
  real = (el >= 0).all(axis=1)
  X = np.asarray(coords, np.float64)[np.where(el >= 0, el, 0)]
  return X.min(axis=1), X.max(axis=1), real


def extents(coords, elements):
  lo, hi, _ = element_boxes(coords, elements)
  return (hi - lo).max(axis=1)


def locate(coords, elements, nodes, points, inflate=0.1, max_iter=10,
           tol_xi=1e-10, tol_x=1e-10):
  """(element (M,), xi (M, d), found (M,)): every real element whose inflated
  box holds the point is tried in ascending order with `max_iter` Newton
  steps from xi = 0 (clamped to [-1.5, 1.5]) and, when that pass ends outside
  the reference cube, `max_iter` more from its projection onto the cube; the
  first accepted one wins."""
  points = np.asarray(points, np.float64)
  M, d = points.shape
  lo, hi, real = element_boxes(coords, elements)
  side = hi - lo
  ext = side.max(axis=1)
  element = np.full(M, -1, np.int64)
  xi_out = np.zeros((M, d))
  for e in np.flatnonzero(real):
    inbox = ((points >= lo[e] - inflate * side[e]) &
             (points <= hi[e] + inflate * side[e])).all(axis=1)
    todo = np.flatnonzero(inbox & (element < 0))
    if not len(todo):
      continue
    xp = points[todo]
    ee = np.full(len(todo), e)

    def newton(xi):
      for _ in range(max_iter):
        x, J = nodal_map(coords, elements, nodes, ee, xi)
        with np.errstate(all='ignore'):
          try:
            step = np.linalg.solve(J, (x - xp)[..., None])[..., 0]
          except np.linalg.LinAlgError:
            step = np.full_like(xi, np.nan)
        xi = np.clip(np.nan_to_num(xi - step, nan=1.5), -1.5, 1.5)
      x, _ = nodal_map(coords, elements, nodes, ee, xi)
      return xi, np.abs(x - xp).max(axis=1)

    xi, res = newton(np.zeros((len(todo), d)))
    # a curved element's map, continued past the element, can fold back onto
    # the point: a pass that ends outside starts once more from the nearest
    # point of the reference cube
    again = np.abs(xi).max(axis=1) > 1 + tol_xi
    xi2, res2 = newton(np.clip(xi, -1.0, 1.0))
    xi = np.where(again[:, None], xi2, xi)
    res = np.where(again, res2, res)
    ok = (np.abs(xi).max(axis=1) <= 1 + tol_xi) & (res <= tol_x * ext[e])
    element[todo[ok]] = e
    xi_out[todo[ok]] = xi[ok]
  return element, xi_out, element >= 0


def dense_matrix(elements, nodes, element, xi, num_nodes):
  """(M, N) evaluation matrix: row m holds l_n(xi_m) at elements[e_m, n];
  rows of points with element -1 are zero."""
  el = np.asarray(elements)
  element = np.asarray(element)
  M = len(element)
  out = np.zeros((M, num_nodes))
  hit = np.flatnonzero(element >= 0)
  phi, _ = shape_functions(nodes, np.asarray(xi, np.float64)[hit])
  np.add.at(out, (hit[:, None], el[element[hit]]), phi)
  return out


def evaluate(elements, nodes, element, xi, u):
  """dense_matrix(...) @ u without forming the matrix: u (N,) or (N, C)."""
  el = np.asarray(elements)
  element = np.asarray(element)
  u = np.asarray(u, np.float64)
  out = np.zeros((len(element),) + u.shape[1:])
  hit = np.flatnonzero(element >= 0)
  phi, _ = shape_functions(nodes, np.asarray(xi, np.float64)[hit])
  out[hit] = np.einsum('mn,mn...->m...', phi, u[el[element[hit]]])
  return out


def evaluate_t(elements, nodes, element, xi, w, num_nodes):
  """dense_matrix(...).T @ w without forming the matrix: w (M,) or (M, C)."""
  el = np.asarray(elements)
  element = np.asarray(element)
  w = np.asarray(w, np.float64)
  out = np.zeros((num_nodes,) + w.shape[1:])
  hit = np.flatnonzero(element >= 0)
  phi, _ = shape_functions(nodes, np.asarray(xi, np.float64)[hit])
  vals = np.einsum('mn,m...->mn...', phi, w[hit])
  np.add.at(out, el[element[hit]], vals)
  return out


def make_points(rng, coords, elements, nodes, count, rounder=None):
  """(e0 (M,), xi0 (M, d), x (M, d)): an element drawn among the real rows,
  xi0 uniform in [-1, 1]^d, mapped, so every point lies inside the domain.
  In the first fifth of the points each xi0 component is set to +-1 with
  probability one half: points on faces, edges and vertices.  `rounder`
  rounds the uniform xi0 before mapping (float32-representable xi)."""
  el = np.asarray(elements)
  d = np.asarray(coords).shape[1]
  real = np.flatnonzero((el >= 0).all(axis=1))
  e0 = real[rng.integers(0, len(real), count)]
  xi0 = rng.uniform(-1.0, 1.0, (count, d))
  if rounder is not None:
    xi0 = rounder(xi0)
  special = np.arange(count) < count // 5
  snap = (rng.random((count, d)) < 0.5) & special[:, None]
  sign = np.where(rng.random((count, d)) < 0.5, -1.0, 1.0)
  xi0 = np.where(snap, sign, xi0)
  x, _ = nodal_map(coords, elements, nodes, e0, xi0)
  return e0, xi0, x


def outside_points(rng, coords, count, margin=0.05):
  """Points at least `margin` outside the bounding box of `coords`."""
  X = np.asarray(coords, np.float64)
  lo, hi = X.min(axis=0), X.max(axis=0)
  d = X.shape[1]
  p = rng.uniform(lo - 0.3, hi + 0.3, (count, d))
  axis = rng.integers(0, d, count)
  up = rng.random(count) < 0.5
  off = margin + rng.uniform(0.0, 0.3, count)
  rows = np.arange(count)
  p[rows, axis] = np.where(up, hi[axis] + off, lo[axis] - off)
  return p
