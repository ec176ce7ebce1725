"""Meshes, inputs and float64 reference results of the Stokes order sweep
(`tests/test_gpu_stokes_order_sweep.py`), computed on the CPU only: the same
functions give the error of the float32 reference algorithm on each item's
own inputs (`f32_reference_errors`), which is what an fp32 exception of the
sweep has to be derived from.

One item is (ndim, P, precision): the velocity / pressure pair of
`numbering_cases.build_pair` on 3^ndim elements ('three_kinds' from P = 5,
'vertex' at P = 4, where a 2-point pressure space cannot hold a curved
element), once with the refiner's pressure numbering and once with a random
one, and for the over-integrated convection a (P - 2)-point GLL refinement of
the same order-1 premesh, bent like the pair.
"""
import functools

import numpy as np

from swirl_fem_amd.core.interpolation import Nodes1D
from swirl_fem_amd.core.mesh_refiner import refine_premesh
from tests import numbering_cases as NC
from tests import sumfact_stokes_reference as S
from tests.fp32util import F32Rng, f32r

N_ELEM = 3


def geometry_of(P):
  return 'three_kinds' if P >= 5 else 'vertex'


@functools.lru_cache(maxsize=None)
def pair(ndim, P, pnum, f32):
  return NC.build_pair('refiner', pnum, geometry_of(P), N_ELEM, P, ndim=ndim,
                       f32=f32)


@functools.lru_cache(maxsize=None)
def overint_premesh(ndim, P, f32):
  """The (P - 2)-point GLL refinement of the pair's order-1 premesh."""
  pm, bend = NC.pair_premesh(geometry_of(P), N_ELEM, ndim)
  rp = refine_premesh(pm, Nodes1D.create(P - 2, NC.GLL))
  if bend:
    rp = NC.bend_first_layer(rp, N_ELEM)
  if f32:
    rp = rp.replace(node_coords=f32r(rp.node_coords))
  return rp


def boundary_mask(c):
  return np.asarray(
      c.v.base.finalize_all()['physical_masks']['boundary']).astype(bool)


def _results(r, dtype):
  """Every reference result of one item from its inputs `r`, with the
  algorithm carried in `dtype`."""
  c, c2, orp, P = r['pair'], r['pair2'], r['orp'], r['P']
  v = c.v.rp
  sf = S.StokesSpace(v.node_coords, v.elements, c.p.rp.elements, P, dtype,
                     r['Np'])
  keep = (~r['bm'])[:, None].astype(dtype)
  u, p, sc, s1 = r['u'], r['p'], r['sc'], r['s1']
  out = {}
  out['div'] = {None: sf.div(u), 's1': sf.div(s1[:, None] * u),
                'sc': sf.div(sc * u)}
  out['grad_t'] = g = sf.grad_t(p)
  # the same local results through the random pressure rows of the second pair
  rows2 = np.asarray(c2.p.rp.elements).astype(np.int64)
  d2 = np.zeros(r['Np'], dtype=dtype)
  np.add.at(d2, rows2, sf.div_local(sf.gather(u)))
  out['div2'] = d2
  out['grad_t2'] = sf.scatter(sf.grad_t_local(
      np.asarray(r['p2'], dtype=dtype)[rows2]))
  # E = D scale mask D^T
  g = g * keep
  out['E'] = {None: sf.div(g), 's1': sf.div(np.asarray(s1, dtype)[:, None] * g),
              'sc': sf.div(np.asarray(sc, dtype) * g)}
  cs = S.ConvectionSpace(v.node_coords, v.elements, P, P, dtype)
  out['conv'] = cs.convection_local(r['ul'])
  co = S.ConvectionSpace(orp.node_coords, orp.elements, P - 2, P, dtype)
  out['conv_over'] = co.convection_local(r['ul_over'])
  return out


def _freeze(tree):
  for v in tree.values():
    if isinstance(v, dict):
      _freeze(v)
    elif isinstance(v, np.ndarray):
      v.setflags(write=False)


@functools.lru_cache(maxsize=None)
def reference(ndim, P, f32):
  """Inputs (float32-representable when `f32`) and float64 results."""
  c, c2 = pair(ndim, P, 'identity', f32), pair(ndim, P, 'random', f32)
  assert np.array_equal(c.v.rp.node_coords, c2.v.rp.node_coords)
  assert np.array_equal(c.v.rp.elements, c2.v.rp.elements)
  orp = overint_premesh(ndim, P, f32)
  seed = 2000 * ndim + 10 * P
  rng = F32Rng(seed) if f32 else np.random.default_rng(seed)
  N, Np = c.v.rp.node_coords.shape[0], c.p.rp.node_coords.shape[0]
  r = dict(pair=c, pair2=c2, orp=orp, P=P, ndim=ndim, N=N, Np=Np,
           bm=boundary_mask(c))
  r['u'] = rng.standard_normal((N, ndim))
  r['p'] = rng.standard_normal(Np)
  r['p2'] = rng.standard_normal(Np)
  r['sc'] = rng.uniform(0.5, 2.0, (N, ndim))
  r['s1'] = np.ascontiguousarray(r['sc'][:, 0])
  r['ul'] = rng.standard_normal(c.v.rp.elements.shape + (ndim,))
  r['ul_over'] = rng.standard_normal(orp.elements.shape + (ndim,))
  r['ref'] = _results(r, np.float64)
  _freeze(r)
  return r


def _rel(a, b):
  return np.abs(a.astype(np.float64) - b).max() / max(np.abs(b).max(), 1e-300)


def f32_reference_errors(ndim, P):
  """Relative max-norm error of the float32 reference algorithm against the
  float64 one on the fp32 item's inputs, per section of the sweep."""
  r = reference(ndim, P, True)
  lo, hi = _results(r, np.float32), r['ref']
  return {
      'a': max(_rel(lo['div'][k], hi['div'][k]) for k in hi['div']),
      'b': _rel(lo['grad_t'], hi['grad_t']),
      'd': max(_rel(lo['div2'], hi['div2']),
               _rel(lo['grad_t2'], hi['grad_t2'])),
      'e': max(_rel(lo['E'][k], hi['E'][k]) for k in hi['E']),
      'f': max(_rel(lo['conv'], hi['conv']),
               _rel(lo['conv_over'], hi['conv_over'])),
  }


# ------------------------------------------------------------------ packing
def expected_kind_counts(ndim, P):
  """Elements per geometry kind that fp64 'auto' must find: 2^d multilinear
  elements round the moved vertex, from P = 5 the 3^(d-1) curved ones of the
  first layer, the rest affine."""
  total, multi = N_ELEM ** ndim, 2 ** ndim
  curved = N_ELEM ** (ndim - 1) if P >= 5 else 0
  return {'affine': total - multi - curved, 'multilinear': multi,
          'curved': curved}


def expected_launch_counts(ndim, P):
  """Element counts of the launches of one item: one per kind under 'auto',
  affine joined to multilinear under 'multilinear', everything under
  'stored'."""
  k = expected_kind_counts(ndim, P)
  counts = {k['affine'], k['multilinear'], k['affine'] + k['multilinear'],
            N_ELEM ** ndim}
  if k['curved']:
    counts.add(k['curved'])
  return counts


def check_packing(ndim, P, itemsize, counts):
  """Across the launches of an item (`counts`: their element counts) the
  last workgroup is a partial one at least once, and wherever the tile packs
  several elements (EPB > 1) a workgroup holds several at least once.  A
  tile of one element per workgroup (3D from P = 6) has no partial
  workgroup: its only idle lanes are those of the element's last wave, in
  every workgroup of every launch."""
  from tests.packing import epb, workgroups
  per = epb(ndim, P, itemsize)
  if per == 1:
    assert ndim == 3 and P >= 6, (ndim, P)
    return per
  assert any(workgroups(n, per)[1] for n in counts), (ndim, P, per, counts)
  assert any(min(n, per) > 1 for n in counts), (ndim, P, per, counts)
  return per
