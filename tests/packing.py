"""How the index-row kernels pack elements into workgroups: the rule of
`HelmholtzTile::pick_epb` (csrc/sfem_helmholtz.h) restated, shared by the order
sweeps of the Helmholtz and of the Stokes kernels (both families take their
tile from `HelmholtzTile<T, P, DIM>`; the convection kernel with P = the
points of its quadrature grid)."""


def epb(ndim, P, itemsize):
  """Elements per workgroup: the rule of `HelmholtzTile::pick_epb`."""
  tpe = P * P if ndim == 3 else P
  if 64 % tpe == 0:
    return 64 // tpe
  if tpe > 32:                  # more than half a wave, or several waves
    return 1
  sb = P | 1
  lds = 2 * P * (P * sb if ndim == 3 else sb) * itemsize
  best, best_util = 1, 0.0
  for n in range(1, 17):
    thr = -(-n * tpe // 64) * 64
    if thr > 512 or n * lds > 40 * 1024:
      break
    if n * tpe / thr > best_util + 1e-9:
      best, best_util = n, n * tpe / thr
  return best


def workgroups(count, per_group):
  """(full workgroups, elements in the partial last one or 0) of a launch of
  `count` elements."""
  return count // per_group, count % per_group
