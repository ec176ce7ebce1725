"""Tensor-level wrappers over the C-ABI (`include/sfem.h`).

PyTorch is plumbing here: it owns the HBM allocations and the HIP stream; every
number is produced by `libsfem_hip.so`.  All tensors must live on the GPU.
"""

from __future__ import annotations

import ctypes
import os

import numpy as np
import torch

from swirl_fem_amd import switches
from swirl_fem_amd import _lib

_DT = {torch.float32: _lib.SFEM_F32, torch.float64: _lib.SFEM_F64}


def _dtype_code(t: torch.Tensor) -> int:
  try:
    return _DT[t.dtype]
  except KeyError:
    raise TypeError(f'unsupported dtype {t.dtype}; use float32 or float64')


def _dev(*tensors):
  """Checks that all tensors are contiguous GPU tensors on one device."""
  dev = None
  for t in tensors:
    if t is None:
      continue
    if not t.is_cuda:
      raise RuntimeError(
          'swirl_fem_amd kernels run on MI355X device tensors only; got a '
          f'{t.device} tensor (there is no CPU fallback)')
    if not t.is_contiguous():
      raise ValueError('expected a contiguous tensor')
    if dev is None:
      dev = t.device
    elif t.device != dev:
      raise ValueError(f'tensors on different devices: {dev} vs {t.device}')
  return dev


def _ptr(t):
  return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(dev):
  return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _idx(indices: torch.Tensor) -> torch.Tensor:
  if indices.dtype != torch.int32:
    indices = indices.to(torch.int32)
  return indices.contiguous()


# ---------------------------------------------------------------- gather etc
def gather(u, indices, fill):
  indices = _idx(indices)
  u = u.contiguous()
  dev = _dev(u, indices)
  out = torch.empty(indices.shape, dtype=u.dtype, device=dev)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_gather(
        _ptr(u), _ptr(indices), _ptr(out), indices.numel(), float(fill),
        _dtype_code(u), _stream(dev)), 'sfem_gather')
  return out


def gather_rows(x, indices):
  """x (N, nc), indices (...) -> (..., nc); SENTINEL rows are zero.

  A component-major `x` gives a component-major result (one scalar gather per
  contiguous component strip)."""
  indices = _idx(indices)
  if is_component_major(x):
    from swirl_fem_amd.core import layout
    out = layout.empty_component_major(tuple(indices.shape) + (x.shape[-1],),
                                       x.dtype, x.device)
    for k in range(x.shape[-1]):
      out[..., k].copy_(gather(x[:, k], indices, 0.0))
    return out
  x = x.contiguous()
  dev = _dev(x, indices)
  nc = x.shape[-1]
  out = torch.empty(tuple(indices.shape) + (nc,), dtype=x.dtype, device=dev)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_gather_rows(
        _ptr(x), _ptr(indices), _ptr(out), indices.numel(), nc,
        _dtype_code(x), _stream(dev)), 'sfem_gather_rows')
  return out


def scatter_add(u_local, indices, num_nodes, ncomp=1):
  indices = _idx(indices)
  if ncomp > 1 and is_component_major(u_local):
    from swirl_fem_amd.core import layout
    out = layout.empty_component_major((num_nodes, ncomp), u_local.dtype,
                                       u_local.device)
    for k in range(ncomp):
      out[:, k].copy_(scatter_add(u_local[..., k], indices, num_nodes))
    return out
  u_local = u_local.contiguous()
  dev = _dev(u_local, indices)
  shape = (num_nodes,) if ncomp == 1 and u_local.dim() == indices.dim() else (
      num_nodes, ncomp)
  out = torch.empty(shape, dtype=u_local.dtype, device=dev)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_scatter_add(
        _ptr(u_local), _ptr(indices), _ptr(out), indices.numel(), num_nodes,
        ncomp, _dtype_code(u_local), _stream(dev)), 'sfem_scatter_add')
  return out


def scatter_csr(u_local, offsets, slots, num_nodes, ncomp=1, out=None):
  u_local = u_local.contiguous()
  dev = _dev(u_local, offsets, slots)
  shape = (num_nodes,) if ncomp == 1 else (num_nodes, ncomp)
  if out is None:
    out = torch.empty(shape, dtype=u_local.dtype, device=dev)
  elif (tuple(out.shape) != shape or out.dtype != u_local.dtype or
        not out.is_contiguous()):
    raise ValueError('scatter_csr: `out` must be a dense (num_nodes[, ncomp]) '
                     'tensor of the values\' dtype')
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_scatter_csr(
        _ptr(u_local), _ptr(offsets), _ptr(slots), _ptr(out), num_nodes, ncomp,
        _dtype_code(u_local), _stream(dev)), 'sfem_scatter_csr')
  return out


_class_cache = {}


def _exchange_classes(gather_indices, unique_indices, dev):
  """CSR of the periodic classes on `dev`: (members, offsets, num_classes).

  `gather_indices[i]` is a participating node and `unique_indices[i]` its
  class (core/gather_scatter.py:284-315); entries of -1 are padding.  Cached
  per index pair (the arrays of a mesh are static)."""
  key = (id(gather_indices), id(unique_indices), str(dev))
  cached = _class_cache.get(key)
  if (cached is not None and cached[0] is gather_indices and
      cached[1] is unique_indices):
    return cached[2:]
  gi = (gather_indices.detach().cpu().numpy()
        if isinstance(gather_indices, torch.Tensor)
        else np.asarray(gather_indices)).astype(np.int64).reshape(-1)
  ui = np.asarray(unique_indices).astype(np.int64).reshape(-1)
  if gi.shape != ui.shape:
    raise ValueError('gather and unique indices must have the same length')
  keep = gi >= 0
  gi, ui = gi[keep], ui[keep]
  order = np.lexsort((gi, ui))                  # by class, then by node id
  classes, counts = np.unique(ui, return_counts=True)
  offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
  members = torch.as_tensor(gi[order].astype(np.int32), device=dev)
  out = (members, torch.as_tensor(offsets, device=dev), len(classes))
  if len(_class_cache) >= 64:                   # meshes come and go
    _class_cache.pop(next(iter(_class_cache)))
  _class_cache[key] = (gather_indices, unique_indices) + out
  return out


def exchange_local(u, gather_indices, unique_indices, inplace=False):
  """Unpartitioned QQ^T; `unique_indices` is a host array (static).

  One launch for all components, in place on a copy of `u` (or on `u` itself
  with `inplace=True`: only the periodic images change)."""
  cm = is_component_major(u)
  if not cm:
    u = u.contiguous()
  dev = _dev(u.movedim(-1, 0) if cm else u)
  members, offsets, num_classes = _exchange_classes(gather_indices,
                                                    unique_indices, dev)
  out = u if inplace else u.clone()             # clone keeps the dense layout
  ncomp, ns, cs = _node_view(out)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_exchange_classes(
        _ptr(out), _ptr(members), _ptr(offsets), num_classes, ncomp, ns, cs,
        _dtype_code(out), _stream(dev)), 'sfem_exchange_classes')
  return out


def exchange_classes_(u, members, offsets, num_classes):
  """In place: every member position of a class receives the sum over the
  class (`sfem_exchange_classes`; members / offsets: int32 CSR on the device)."""
  if num_classes == 0:
    return u
  cm = is_component_major(u)
  if not (cm or u.is_contiguous()):
    raise ValueError('exchange_classes_: dense field expected')
  dev = _dev(u.movedim(-1, 0) if cm else u, members, offsets)
  ncomp, ns, cs = _node_view(u)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_exchange_classes(
        _ptr(u), _ptr(members), _ptr(offsets), int(num_classes), ncomp, ns, cs,
        _dtype_code(u), _stream(dev)), 'sfem_exchange_classes')
  return u


def exchange_local_atomic(u, gather_indices, unique_indices):
  """The same QQ^T through `sfem_exchange_local` (segment sums by atomics into
  a workspace, then expansion): the C-ABI's out-of-place form."""
  gidx = _idx(gather_indices)
  u = u.contiguous()
  dev = _dev(u, gidx)
  uni = torch.as_tensor(np.ascontiguousarray(unique_indices),
                        dtype=torch.int32, device=dev)
  num_unique = int(np.max(unique_indices)) + 1 if len(unique_indices) else 0
  ncomp = 1 if u.dim() == 1 else u.shape[-1]
  sums = torch.empty((max(num_unique, 1), ncomp), dtype=u.dtype, device=dev)
  out = torch.empty_like(u)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_exchange_local(
        _ptr(u), _ptr(out), _ptr(gidx), _ptr(uni), gidx.numel(), u.shape[0],
        _ptr(sums), num_unique, ncomp, _dtype_code(u), _stream(dev)),
               'sfem_exchange_local')
  return out


def subtract_weighted_mean(w, b, total, partials, out=None, dot_result=None):
  """out = w - (b . w / total) 1 (two launches, no host synchronisation).
  `dot_result = (scalars, slot)`: scalars[slot] += w . out as well."""
  w, b = w.contiguous(), b.contiguous()
  if w.shape != b.shape or w.dtype != b.dtype:
    raise ValueError('subtract_weighted_mean: operands differ in shape / dtype')
  if out is None:
    out = torch.empty_like(w)
  dev = _dev(w, b, out, partials)
  if partials.dtype != torch.float64 or partials.numel() < _lib.SFEM_DOT_SLOTS:
    raise ValueError('partials: SFEM_DOT_SLOTS float64 values')
  with torch.cuda.device(dev):
    dot_ptr = None
    if dot_result is not None:
      scalars, slot = dot_result
      _dev(scalars)
      if scalars.dtype != torch.float64:
        raise ValueError('dot_result: float64 scalars')
      dot_ptr = ctypes.c_void_p(scalars.data_ptr() + 8 * slot)
    _lib.check(_lib.load().sfem_subtract_weighted_mean(
        _ptr(w), _ptr(b), float(total), _ptr(out), _ptr(partials), w.numel(),
        dot_ptr, _dtype_code(w), _stream(dev)), 'sfem_subtract_weighted_mean')
  return out


def pack(u, idx):
  ncomp = 1 if u.dim() == 1 else u.shape[-1]
  u = u.contiguous()
  dev = _dev(u, idx)
  shape = (idx.numel(),) if u.dim() == 1 else (idx.numel(), ncomp)
  buf = torch.empty(shape, dtype=u.dtype, device=dev)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_pack(
        _ptr(u), _ptr(idx), _ptr(buf), idx.numel(), ncomp, _dtype_code(u),
        _stream(dev)), 'sfem_pack')
  return buf


def unpack_add(buf, idx, u):
  """In place: u[idx] += buf."""
  ncomp = 1 if u.dim() == 1 else u.shape[-1]
  dev = _dev(buf, idx, u)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_unpack_add(
        _ptr(buf), _ptr(idx), _ptr(u), idx.numel(), ncomp, _dtype_code(u),
        _stream(dev)), 'sfem_unpack_add')
  return u


def _node_view(u):
  """(ncomp, node_stride, comp_stride) of a dense (N,) / (N, nc) field."""
  if u.dim() == 1:
    if u.stride(0) != 1:
      raise ValueError('nodal vector must be dense')
    return 1, 1, 1
  if u.dim() != 2 or not (u.is_contiguous() or is_component_major(u)):
    raise ValueError('field must be (N,), row-major (N, nc) or component-major')
  return u.shape[1], u.stride(0), u.stride(1)


def pack_strided(u, idx, out=None):
  """buf[i, k] = u[idx[i], k] for any dense field layout (one launch)."""
  ncomp, ns, cs = _node_view(u)
  dev = _dev(u.movedim(-1, 0) if is_component_major(u) else u, idx)
  shape = (idx.numel(),) if u.dim() == 1 else (idx.numel(), ncomp)
  buf = out if out is not None else torch.empty(shape, dtype=u.dtype,
                                                device=dev)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_pack_strided(
        _ptr(u), _ptr(idx), _ptr(buf), idx.numel(), ncomp, ns, cs,
        _dtype_code(u), _stream(dev)), 'sfem_pack_strided')
  return buf


def unpack_add_atomic(buf, idx, u):
  """In place: u[idx[i], k] += buf[i, k]; idx may repeat nodes."""
  ncomp, ns, cs = _node_view(u)
  dev = _dev(buf, idx, u.movedim(-1, 0) if is_component_major(u) else u)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_unpack_add_atomic(
        _ptr(buf), _ptr(idx), _ptr(u), idx.numel(), ncomp, ns, cs,
        _dtype_code(u), _stream(dev)), 'sfem_unpack_add_atomic')
  return u


# ------------------------------------------------------------------ geometry
def geom_factors(elem_coords, interp1, grad1, ndim, P, q, want_quad_coords):
  elem_coords = elem_coords.contiguous()
  dev = _dev(elem_coords, interp1, grad1)
  E = elem_coords.shape[0]
  Q = q ** ndim
  dt = elem_coords.dtype
  invjac = torch.empty((E, Q, ndim, ndim), dtype=dt, device=dev)
  jacdet = torch.empty((E, Q), dtype=dt, device=dev)
  quad = (torch.empty((E, Q, ndim), dtype=dt, device=dev)
          if want_quad_coords else None)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_geom_factors(
        _ptr(elem_coords), _ptr(interp1), _ptr(grad1), E, ndim, P, q,
        _ptr(invjac), _ptr(jacdet), _ptr(quad), _dtype_code(elem_coords),
        _stream(dev)), 'sfem_geom_factors')
  return invjac, jacdet, quad


def basis_eval(u_local, interp1, grad1, invjac, ndim, P, q, collocated,
               want_val, want_grad):
  """u_local (E, n, nc) -> val (E, Q, nc), grad (E, Q, d, nc)."""
  u_local = u_local.contiguous()
  dev = _dev(u_local, interp1, grad1, invjac)
  E, _, nc = u_local.shape
  Q = q ** ndim
  dt = u_local.dtype
  val = torch.empty((E, Q, nc), dtype=dt, device=dev) if want_val else None
  grad = (torch.empty((E, Q, ndim, nc), dtype=dt, device=dev)
          if want_grad else None)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_basis_eval(
        _ptr(u_local), _ptr(interp1), _ptr(grad1), _ptr(invjac), _ptr(val),
        _ptr(grad), E, ndim, P, q, nc, int(collocated), _dtype_code(u_local),
        _stream(dev)), 'sfem_basis_eval')
  return val, grad


def basis_eval_t(c0, c1, interp1, grad1, invjac, wdet, ndim, P, q, nc,
                 collocated):
  """Transpose of `basis_eval` with quadrature: -> (E, n, nc)."""
  c0 = None if c0 is None else c0.contiguous()
  c1 = None if c1 is None else c1.contiguous()
  dev = _dev(c0, c1, interp1, grad1, invjac, wdet)
  E = wdet.shape[0]
  out = torch.empty((E, P ** ndim, nc), dtype=wdet.dtype, device=dev)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_basis_eval_t(
        _ptr(c0), _ptr(c1), _ptr(interp1), _ptr(grad1), _ptr(invjac),
        _ptr(wdet), _ptr(out), E, ndim, P, q, nc, int(collocated),
        _dtype_code(wdet), _stream(dev)), 'sfem_basis_eval_t')
  return out


# ----------------------------------------------------------------- helmholtz
def helmholtz_setup(invjac, jacdet, weights_nd):
  dev = _dev(invjac, jacdet, weights_nd)
  E, Q, ndim, _ = invjac.shape
  ng = ndim * (ndim + 1) // 2
  geo = torch.empty((E, ng + 1, Q), dtype=invjac.dtype, device=dev)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_helmholtz_setup(
        _ptr(invjac), _ptr(jacdet), _ptr(weights_nd), _ptr(geo), E, ndim, Q,
        _dtype_code(invjac), _stream(dev)), 'sfem_helmholtz_setup')
  return geo


def encode_elements(elements, dirichlet_u8, multiplicity, slot_shared=None):
  elements = _idx(elements)
  dev = _dev(elements, dirichlet_u8, multiplicity, slot_shared)
  enc = torch.empty_like(elements)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_encode_elements(
        _ptr(elements), _ptr(dirichlet_u8), _ptr(multiplicity),
        _ptr(slot_shared), _ptr(enc), elements.numel(), _stream(dev)),
        'sfem_encode_elements')
  return enc


def helmholtz_setup_multilinear(elem_coords, ndim, P):
  """elem_coords (E, n, d) -> (E, 24) multilinear-map coefficients."""
  elem_coords = elem_coords.contiguous()
  dev = _dev(elem_coords)
  E = elem_coords.shape[0]
  geo_elem = torch.empty((E, 24), dtype=elem_coords.dtype, device=dev)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_helmholtz_setup_multilinear(
        _ptr(elem_coords), _ptr(geo_elem), E, ndim, P,
        _dtype_code(elem_coords), _stream(dev)),
        'sfem_helmholtz_setup_multilinear')
  return geo_elem


_KERNARG_CHECKED = set()


def kernarg_selftest(dev):
  """Once per process and device: the facet kernels' view of their matrix
  argument through the kernarg segment is what was passed
  (`sfem_kernarg_selftest`); raises otherwise."""
  if dev in _KERNARG_CHECKED:
    return
  bad = torch.zeros(1, dtype=torch.int32, device=dev)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_kernarg_selftest(_ptr(bad), _stream(dev)),
               'sfem_kernarg_selftest')
  if int(bad.item()) != 0:
    raise _lib.SfemError(
        'the kernel-argument layout differs from what the facet kernels '
        f'assume (probe flags {int(bad.item())}): rebuild libsfem_hip.so with '
        'the toolchain it was written for (FacetKernarg::MAT_OFF)')
  _KERNARG_CHECKED.add(dev)


def facet_table(elements, dirichlet_u8, multiplicity, P):
  """Compact connectivity (`sfem_facet_table_build`): `(E, 27, 4)` int32
  table and the `(E,)` bool mask of the elements it describes exactly."""
  elements = _idx(elements)
  dev = _dev(elements, dirichlet_u8, multiplicity)
  kernarg_selftest(dev)      # every facet launch starts from a table
  E = elements.shape[0]
  tab = torch.empty((E, 27, 4), dtype=torch.int32, device=dev)
  ok = torch.empty((E,), dtype=torch.uint8, device=dev)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_facet_table_build(
        _ptr(elements), _ptr(dirichlet_u8), _ptr(multiplicity), _ptr(tab),
        _ptr(ok), E, multiplicity.shape[0], P, _stream(dev)),
        'sfem_facet_table_build')
  return tab, ok != 0


def helmholtz_setup_affine(geo_elem, box_tol):
  """(E, 24) coefficients of affine elements -> (E, 8) constants
  (`sfem_helmholtz_setup_affine`); column 7 flags Cartesian boxes."""
  geo_elem = geo_elem.contiguous()
  dev = _dev(geo_elem)
  E = geo_elem.shape[0]
  out = torch.empty((E, 8), dtype=geo_elem.dtype, device=dev)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_helmholtz_setup_affine(
        _ptr(geo_elem), _ptr(out), E, float(box_tol), _dtype_code(geo_elem),
        _stream(dev)), 'sfem_helmholtz_setup_affine')
  return out


def _host(a, dtype):
  np_dt = np.float64 if dtype == torch.float64 else np.float32
  return None if a is None else np.ascontiguousarray(a, dtype=np_dt)


def _hptr(a):
  return None if a is None else a.ctypes.data


def _dptr(t):
  return None if t is None else t.data_ptr()


def _launch_fields(part, host=None, key='geo'):
  """What every launch description hands to its `*Args` struct, as keyword
  arguments: the per-point data under `key` ('geo' or 'kfac'), the
  multilinear coefficients, the element list with its length and the
  geometry kind; with `host` (`_host`-converted NumPy tables) their
  pointers as well."""
  lst = part.get('elem_list')
  fields = {key: _dptr(part.get(key)), 'geo_elem': _dptr(part.get('geo_elem')),
            'geo_index': _dptr(part.get('geo_index')),
            'elem_list': _dptr(lst),
            'num_listed': 0 if lst is None else lst.numel(),
            'geo_mode': part['geo_mode']}
  if host is not None:
    fields.update(dmat=_hptr(host['dmat']), weights=_hptr(host.get('weights')),
                  nodes=_hptr(host.get('nodes')))
  return fields


def _helmholtz_args(u, out, enc, part, host, ndim, P, num_elements, num_nodes,
                    lambda0, lambda1, zero_range, dot_out=None,
                    layered_extent=0, dot_slots=0, transpose=False):
  """Builds `sfem_helmholtz_args`; `part` = dict(geo_mode, geo, geo_elem,
  geo_index, elem_list), `host` = dict(dmat, weights, nodes) NumPy arrays
  (kept alive by the caller for the duration of the call)."""
  vec = u.dim() != (1 if enc is not None else 2)
  ncomp = u.shape[-1] if vec else 1
  node_stride = comp_stride = 0
  if vec and not u.is_contiguous():
    # component-major storage viewed as (..., ncomp): every component is a
    # contiguous strip
    node_stride, comp_stride = 1, u.stride(-1)
  so = part.get('shared_order')
  cl = part.get('cluster') if enc is not None else None
  if cl is not None:
    enc, so = cl.enc, None
  ft = part.get('facet_table') if enc is not None else None
  ch = None
  if layered_extent:
    # same launches, layered table form; the layer plan was made for exactly
    # these chain segments (or for none)
    ft, so = part['layered_table'], None
    ch = part.get('chains') if part.get('layered_chains') else None
  elif ft is not None:
    so = None
    # chains walk scalar fields; a component-major vector field is walked
    # component by component
    if ((not vec or node_stride == 1) and
        switches.get('SFEM_CHAIN') != '0' and
        (not vec or switches.get('SFEM_CHAIN_VECTOR') != '0')):
      ch = part.get('chains')        # (offsets, elems) int32 device tensors
  return _lib.HelmholtzArgs(
      u=u.data_ptr(), out=out.data_ptr(), enc=_dptr(enc),
      **_launch_fields(part, host), num_elements=num_elements,
      num_nodes=num_nodes, zero_begin=int(zero_range[0]),
      zero_end=int(zero_range[1]), ndim=ndim, P=P, ncomp=ncomp,
      dtype=_dtype_code(u),
      colored=int(bool(part.get('colored', False))), lambda0=float(lambda0),
      lambda1=float(lambda1), node_stride=node_stride,
      comp_stride=comp_stride,
      dot_out=_dptr(dot_out),
      shared_order=_dptr(so if enc is not None else None),
      shared_stride=0 if so is None or enc is None else so.shape[1],
      cluster_elems=_dptr(cl.elems if cl is not None else None),
      cluster_offsets=_dptr(cl.offsets if cl is not None else None),
      cluster_nodes=_dptr(cl.nodes if cl is not None else None),
      num_clusters=0 if cl is None else cl.num_clusters,
      facet_table=_dptr(ft),
      geo_const=_dptr(part.get('geo_const') if ft is not None else None),
      chain_offsets=_dptr(ch[0] if ch is not None else None),
      chain_elems=_dptr(ch[1] if ch is not None else None),
      num_chains=0 if ch is None else ch[0].numel() - 1,
      layered_extent=int(layered_extent), dot_slots=int(dot_slots),
      kappa=_dptr(part.get('kappa')), sigma=_dptr(part.get('sigma')),
      coef_mode=int(part.get('coef_mode', _lib.COEF_NONE)),
      beta=_dptr(part.get('beta')), adv_transpose=int(bool(transpose)))


_CLUSTER_LIMITS = {}


def helmholtz_cluster_limits(P, dtype):
  """(cluster_size, max_shared) of the cluster kernels for (P, dtype), or None
  (`sfem_helmholtz_cluster_limits`)."""
  key = (P, dtype)
  if key not in _CLUSTER_LIMITS:
    size, kmax = ctypes.c_int32(0), ctypes.c_int32(0)
    code = _lib.SFEM_F64 if dtype == torch.float64 else _lib.SFEM_F32
    rc = _lib.load().sfem_helmholtz_cluster_limits(
        P, code, ctypes.byref(size), ctypes.byref(kmax))
    _CLUSTER_LIMITS[key] = None if rc else (size.value, kmax.value)
  return _CLUSTER_LIMITS[key]


def helmholtz_kernel_name(real, P, ndim, scalar, geo_mode, part, mass,
                          layered=False):
  """Mirror of `launch_helmholtz`'s choice (csrc/sfem_helmholtz.h).  Facet
  kernels: the name up to the addressing-width argument; `layered` (scalar
  fields through `helmholtz_apply_layered`) appends `*, true>`: the last
  template argument of those instantiations."""
  b = lambda v: 'true' if v else 'false'
  if part.get('facet_table') is not None:
    elem = ('sfem::BoxElem<%s, %d, %s>' % (real, P, b(mass)) if geo_mode == 5
            else 'sfem::FacetElem<%s, %d, %d, %s>' % (real, P, geo_mode,
                                                     b(mass)))
    if layered:
      if part.get('chains') is not None and part.get('layered_chains'):
        return 'sfem::helmholtz_chain_kernel<%s, %d, %s, *, true>' % (
            real, P, elem)
      return 'sfem::helmholtz_facet_kernel<%s, %d, %s, true, *, true>' % (
          real, P, elem)
    if (scalar and part.get('chains') is not None and
        switches.get('SFEM_CHAIN') != '0'):
      return 'sfem::helmholtz_chain_kernel<%s, %d, %s, ' % (real, P, elem)
    return 'sfem::helmholtz_facet_kernel<%s, %d, %s, %s, ' % (
        real, P, elem, b(scalar))
  if (real == 'float' and P == 12 and ndim == 3 and scalar and
      geo_mode in (1, 3) and part.get('cluster') is None and
      not part.get('colored') and switches.get('SFEM_MFMA') == '1'):
    return 'sfem::helmholtz_mfma_p12_kernel<%d, %s>' % (geo_mode, b(mass))
  if part.get('cluster') is not None:
    return 'sfem::helmholtz_cluster_kernel<%s, %d, %s, %d, %s>' % (
        real, P, b(scalar), geo_mode, b(mass))
  if part.get('beta') is not None:
    return 'sfem::helmholtz_adv_kernel<%s, %d, %d, true, %d, false>' % (
        real, P, ndim, geo_mode)
  if part.get('coef_mode'):
    return ('sfem::helmholtz_kernel<%s, %d, %d, true, true, %d, false, %s, '
            '%d>' % (real, P, ndim, geo_mode, b(mass), part['coef_mode']))
  tpe = P * P if ndim == 3 else P
  can_sort = ndim == 3 and tpe <= 64
  sort = (can_sort and part.get('shared_order') is not None and
          not part.get('colored') and not (geo_mode == 3 and mass))
  b = lambda v: 'true' if v else 'false'
  return 'sfem::helmholtz_kernel<%s, %d, %d, true, %s, %d, %s, %s>' % (
      real, P, ndim, b(scalar), geo_mode, b(sort), b(mass))


def helmholtz_apply(u, out, enc, parts, host, ndim, P, lambda0, lambda1,
                    zero_range, dot_out=None, transpose=False):
  """out <- mask * scatter((l0 B + l1 A)_local(gather(u))).

  `parts`: one dict per geometry kind present in the mesh (see
  `_helmholtz_args`); the shared-node range of `out` is cleared by the first
  launch only.  `transpose`: the advective term of launches that carry a
  `beta` is applied transposed (`adv_transpose`).
  """
  dev = _dev(enc)
  _check_vector_layout(u, out)
  host = {k: _host(v, u.dtype) for k, v in host.items()}
  if not parts and zero_range[1] > zero_range[0]:
    out[zero_range[0]:zero_range[1]].zero_()
  with torch.cuda.device(dev):
    for n, part in enumerate(parts):
      args = _helmholtz_args(u, out, part.get('enc', enc), part, host, ndim,
                             P, enc.shape[0], u.shape[0], lambda0, lambda1,
                             zero_range if n == 0 else (0, 0), dot_out,
                             transpose=transpose)
      _lib.check(_lib.load().sfem_helmholtz_apply(ctypes.byref(args),
                                                  _stream(dev)),
                 'sfem_helmholtz_apply')
  return out


def layered_dot_waves(parts, P, num_elements):
  """Waves each launch of a layered apply starts (its share of a per-wave
  `dot_out`): workgroups (chain segments or elements) x ceil(P^2 / 64)."""
  waves = (P * P + 63) // 64
  out = []
  for part in parts:
    if part.get('layered_chains'):
      groups = part['chains'][0].numel() - 1
    elif 'elem_list' in part:
      groups = part['elem_list'].numel()
    else:
      groups = num_elements
    out.append(groups * waves)
  return out


def helmholtz_apply_layered(u, ext, enc, parts, host, ndim, P, lambda0,
                            lambda1, dot_out=None, per_wave=False):
  """`sfem_helmholtz_apply` with layered assembly: `ext` is the extended
  output [N nodal values | layers] of the operator's layer plan (slots nobody
  writes hold zero), `parts` carry `layered_table`.  Scalar fields; nothing is
  cleared, no atomics are issued.  `per_wave`: `dot_out` has one double per
  wave of all launches (`layered_dot_waves`), stored not accumulated."""
  dev = _dev(enc)
  if u.dim() != 1 or not u.is_contiguous() or not ext.is_contiguous():
    raise ValueError('layered assembly takes contiguous scalar fields')
  if ext.dtype != u.dtype:
    raise ValueError('u and the extended output differ in dtype')
  host = {k: _host(v, u.dtype) for k, v in host.items()}
  waves = (layered_dot_waves(parts, P, enc.shape[0])
           if per_wave and dot_out is not None else None)
  # (the caller's buffer may carry scratch behind the slots)
  if waves is not None and sum(waves) > dot_out.numel():
    raise ValueError(f'{sum(waves)} waves but {dot_out.numel()} dot slots')
  at = 0
  with torch.cuda.device(dev):
    for n, part in enumerate(parts):
      dots = dot_out if waves is None else dot_out[at:at + waves[n]]
      args = _helmholtz_args(u, ext, enc, part, host, ndim, P, enc.shape[0],
                             u.shape[0], lambda0, lambda1, (0, 0), dots,
                             layered_extent=ext.numel(),
                             dot_slots=0 if waves is None else waves[n])
      if waves is not None:
        at += waves[n]
      _lib.check(_lib.load().sfem_helmholtz_apply(ctypes.byref(args),
                                                  _stream(dev)),
                 'sfem_helmholtz_apply')
  return ext


def _layer_arrays(layers):
  """(len, off) int64 ctypes arrays of a layer list [(length, offset), ...]."""
  n = len(layers)
  arr = ctypes.c_int64 * max(n, 1)
  return (arr(*[int(l[0]) for l in layers]) if n else arr(0),
          arr(*[int(l[1]) for l in layers]) if n else arr(0), n)


def _mask_args(masks, n):
  """(device pointer, host offsets) of a `(bytes, offsets)` layer-mask pair."""
  if masks is None:
    return None, None
  data, offs = masks
  arr = ctypes.c_int64 * max(n, 1)
  return _ptr(data), arr(*[int(o) for o in offs])


def cg_update_r_layered(r, ap_ext, layers, scalars, fuse_rr, masks=None):
  """r -= alpha (Ap assembled from its layers) (+ gamma_new += r.r).
  `masks = (uint8 device tensor, per-layer offsets)`: chunks of
  SFEM_LAYER_CHUNK nodes that no element writes are not read."""
  dev = _dev(r, ap_ext, scalars)
  ln, off, n = _layer_arrays(layers)
  mptr, moff = _mask_args(masks, n)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_cg_update_r_layered(
        _ptr(r), _ptr(ap_ext), r.numel(), ln, off, n, mptr, moff,
        _ptr(scalars), int(fuse_rr), _dtype_code(r), _stream(dev)),
        'sfem_cg_update_r_layered')


def cg_update_r_layered_det(r, ap_ext, layers, scalars, rr_partials,
                            masks=None):
  """The same with r.r left as STORED per-workgroup sums in `rr_partials`
  (summed in index order by `cg_scalars_n(..., 8, ...)`): returns how many."""
  dev = _dev(r, ap_ext, scalars, rr_partials)
  ln, off, n = _layer_arrays(layers)
  mptr, moff = _mask_args(masks, n)
  count = ctypes.c_int64(0)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_cg_update_r_layered_det(
        _ptr(r), _ptr(ap_ext), r.numel(), ln, off, n, mptr, moff,
        _ptr(scalars),
        _ptr(rr_partials), rr_partials.numel(), ctypes.byref(count),
        _dtype_code(r), _stream(dev)), 'sfem_cg_update_r_layered_det')
  return count.value


def cg_scalars_n(scalars, phase, maxiter, tol, atol, partials, num_partials):
  """`cg_scalars` over `num_partials` stored partial sums (phases 3, 4, 5, 8)."""
  dev = _dev(scalars, partials)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_cg_scalars_n(
        _ptr(scalars), phase, float(maxiter), float(tol), float(atol),
        _ptr(partials), int(num_partials), _stream(dev)), 'sfem_cg_scalars_n')


def fold_layers_at(ext, idx, count, layers):
  """ext[idx] += its layers there, the folded slots cleared (in place); `idx`:
  distinct node positions (int64 device tensor)."""
  dev = _dev(ext, idx)
  if idx.dtype != torch.int64:
    raise ValueError('fold_layers_at: int64 node positions')
  ln, off, n = _layer_arrays(layers)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_fold_layers_at(
        _ptr(ext), _ptr(idx), idx.numel(), int(count), ln, off, n,
        _dtype_code(ext), _stream(dev)), 'sfem_fold_layers_at')
  return ext


def _fdm_check(who, r, pel, S, cases, inv_ev, ndim, Pp, weights=None):
  """Refuses operands `sfem_fdm_solve` would read out of bounds; returns
  (device, E).  (The range of Pp is the library's own check.)"""
  dev = _dev(r, pel, S, cases, inv_ev, weights)
  ndim, Pp = int(ndim), int(Pp)
  if not 1 <= ndim <= 3 or Pp < 1:
    raise ValueError(f'{who}: ndim 1..3 and Pp >= 1; got {ndim}, {Pp}')
  if cases.dtype != torch.int32:
    raise TypeError(f'{who}: cases must be int32; got {cases.dtype}')
  if cases.dim() != 2 or cases.shape[0] != ndim:
    raise ValueError(f'{who}: cases must be (ndim, E) = ({ndim}, E); got '
                     f'{tuple(cases.shape)}')
  E = cases.shape[1]
  n = Pp ** ndim
  _dtype_code(r)
  if S.dtype != r.dtype or inv_ev.dtype != r.dtype or (
      weights is not None and weights.dtype != r.dtype):
    raise TypeError(f'{who}: S, inv_ev and weights must have the dtype of r '
                    f'({r.dtype})')
  if S.numel() == 0 or S.numel() % (Pp * Pp):
    raise ValueError(f'{who}: S must be (cases, Pp, Pp); got '
                     f'{tuple(S.shape)} for Pp = {Pp}')
  if inv_ev.numel() != E * n:
    raise ValueError(f'{who}: inv_ev must hold E Pp^d = {E * n} values; got '
                     f'{inv_ev.numel()}')
  if pel is None:
    if r.numel() != E * n:
      raise ValueError(f'{who}: r must hold E Pp^d = {E * n} values without '
                       f'pel; got {r.numel()}')
  else:
    if pel.dtype != torch.int64:
      raise TypeError(f'{who}: pel must be int64; got {pel.dtype}')
    if pel.numel() != E * n:
      raise ValueError(f'{who}: pel must hold E Pp^d = {E * n} node ids; got '
                       f'{pel.numel()}')
  if weights is not None and weights.numel() != r.numel():
    raise ValueError(f'{who}: weights must have the size of r')
  return dev, E


def fdm_solve(r, pel, S, cases, inv_ev, ndim, Pp, out=None):
  """z_e = (S (x) ..) [inv_ev_e .* (S (x) ..)^T r_e] for every element
  (`sfem_fdm_solve`); `pel` (E, Pp^d) int64 or None for element-contiguous
  numbering; `cases` (ndim, E) int32; `out`: z to write into."""
  dev, E = _fdm_check('fdm_solve', r, pel, S, cases, inv_ev, ndim, Pp)
  z = _fdm_out('fdm_solve', out, r, r.shape, dev)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_fdm_solve(
        _ptr(r), _ptr(z), _ptr(pel), _ptr(S), _ptr(cases), _ptr(inv_ev),
        E, int(ndim), int(Pp), _dtype_code(r), _stream(dev)),
        'sfem_fdm_solve')
  return z


def _fdm_out(who, out, like, shape, dev):
  """`out` checked against the result's shape, or a fresh tensor."""
  if out is None:
    return torch.empty(shape, dtype=like.dtype, device=like.device)
  if (_dev(out) != dev or out.dtype != like.dtype or
      tuple(out.shape) != tuple(shape)):
    raise ValueError(f'{who}: out must be a contiguous {like.dtype} tensor of '
                     f'shape {tuple(shape)} on {dev}')
  return out


def fdm_solve_sums(r, pel, S, cases, inv_ev, weights, ndim, Pp, out=None):
  """`fdm_solve` that also returns the element sums of r and the elements'
  shares of weights . z (`sfem_fdm_solve_sums`); `out`: (z, elem_sum,
  weighted_sum) to write into."""
  dev, E = _fdm_check('fdm_solve_sums', r, pel, S, cases, inv_ev, ndim, Pp,
                      weights)
  if weights is None:
    raise ValueError('fdm_solve_sums: weights required')
  zo, so, wo = (None, None, None) if out is None else out
  z = _fdm_out('fdm_solve_sums', zo, r, r.shape, dev)
  elem_sum = _fdm_out('fdm_solve_sums', so, r, (E,), dev)
  weighted = _fdm_out('fdm_solve_sums', wo, r, (E,), dev)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_fdm_solve_sums(
        _ptr(r), _ptr(z), _ptr(pel), _ptr(S), _ptr(cases), _ptr(inv_ev),
        _ptr(weights), _ptr(elem_sum), _ptr(weighted), E, int(ndim), int(Pp),
        _dtype_code(r), _stream(dev)), 'sfem_fdm_solve_sums')
  return z, elem_sum, weighted


def add_element_constants_(z, yc, shift, n, elems_per_member):
  """In place: z[e n + i] += yc[e] - shift[e // elems_per_member]."""
  dev = _dev(z, yc, shift)
  n, epm = int(n), int(elems_per_member)
  E = yc.numel()
  if n < 1 or epm < 1 or z.numel() != E * n:
    raise ValueError('add_element_constants_: z is (E n,) contiguous, n >= 1 '
                     'and elems_per_member >= 1')
  if yc.dtype != z.dtype or shift.dtype != z.dtype:
    raise TypeError('add_element_constants_: one real dtype for z, yc, shift')
  if E % epm:
    raise ValueError(f'add_element_constants_: {E} elements are no multiple '
                     f'of elems_per_member = {epm}')
  if shift.numel() < E // epm:
    raise ValueError(f'add_element_constants_: shift holds {shift.numel()} '
                     f'values for {E // epm} members')
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_add_element_constants(
        _ptr(z), _ptr(yc), _ptr(shift), E, n, epm, _dtype_code(z),
        _stream(dev)), 'sfem_add_element_constants')
  return z


def ell_chebyshev(cols, vals, dinv, b, steps, lmin, lmax, work=None,
                  out=None):
  """x = Chebyshev polynomial of the Jacobi-scaled ELL matrix applied to b
  (`sfem_ell_chebyshev`); cols / vals (width, n) int32 / real; `work`: 3 n
  values of scratch."""
  dev = _dev(cols, vals, dinv, b, work, out)
  n = b.numel()
  if (cols.dim() != 2 or cols.shape != vals.shape or cols.shape[0] < 1 or
      cols.shape[1] != n or dinv.numel() != n):
    raise ValueError('ell_chebyshev: cols / vals must be (width, n), dinv and '
                     'b (n,)')
  if cols.dtype != torch.int32 or vals.dtype != b.dtype or (
      dinv.dtype != b.dtype):
    raise TypeError('ell_chebyshev: int32 columns, one real dtype for vals, '
                    'dinv, b')
  steps, lmin, lmax = int(steps), float(lmin), float(lmax)
  if steps < 1 or not 0.0 < lmin < lmax:
    raise ValueError(f'ell_chebyshev: steps >= 1 and 0 < lmin < lmax; got '
                     f'{steps}, {lmin}, {lmax}')
  if out is not None and (out.dtype != b.dtype or out.numel() != n):
    raise ValueError('ell_chebyshev: out must have the dtype and size of b')
  x = torch.empty_like(b) if out is None else out
  if work is None:
    work = torch.empty(3 * n, dtype=b.dtype, device=b.device)
  elif work.dtype != b.dtype or work.numel() < 3 * n:
    raise ValueError(f'ell_chebyshev: work must hold 3 n = {3 * n} values of '
                     f'{b.dtype}; got {work.numel()} of {work.dtype}')
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_ell_chebyshev(
        _ptr(cols), _ptr(vals), _ptr(dinv), _ptr(b), _ptr(x), _ptr(work), n,
        cols.shape[0], steps, lmin, lmax, _dtype_code(b), _stream(dev)),
        'sfem_ell_chebyshev')
  return x


def ell_spmv(cols, vals, x, y, rows=None, row_range=None):
  """y[i] = (A x)[i] for the ELL matrix cols / vals (width, n) int32 / real
  (`sfem_ell_spmv`), on the rows of `rows` (int32 device tensor, each in
  [0, n)) or of `row_range` = (begin, end) (default: all rows); the other
  rows of y are not written.  Returns y."""
  dev = _dev(cols, vals, x, y, rows)
  n = x.numel()
  if cols.shape != vals.shape or cols.shape[1] != n or y.numel() != n:
    raise ValueError('ell_spmv: cols / vals must be (width, n), x and y (n,)')
  if cols.dtype != torch.int32 or vals.dtype != x.dtype or y.dtype != x.dtype:
    raise TypeError('ell_spmv: int32 columns, one real dtype for vals, x, y')
  if not (cols.is_contiguous() and vals.is_contiguous() and
          x.is_contiguous() and y.is_contiguous()):
    raise ValueError('ell_spmv: contiguous operands only')
  if rows is not None:
    if rows.dtype != torch.int32 or not rows.is_contiguous():
      raise TypeError('ell_spmv: rows must be a contiguous int32 tensor')
    begin, end, count = 0, 0, rows.numel()
  else:
    begin, end = (0, n) if row_range is None else (int(row_range[0]),
                                                    int(row_range[1]))
    if not 0 <= begin <= end <= n:
      raise ValueError(f'ell_spmv: row range {(begin, end)} outside [0, {n}]')
    count = 0
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_ell_spmv(
        _ptr(cols), _ptr(vals), _ptr(x), _ptr(y), n, cols.shape[0], begin,
        end, _ptr(rows), count, _dtype_code(x), _stream(dev)),
        'sfem_ell_spmv')
  return y

# ------------------------------------------------------- ensemble CG (vmap)
def _ens_check(members, *vs):
  dev = _dev(*vs)
  n = vs[0].numel()
  if n % members:
    raise ValueError(f'{n} values do not split into {members} members')
  for v in vs:
    if not v.is_contiguous() or v.numel() != n or v.dtype != vs[0].dtype:
      raise ValueError('ensemble vectors: contiguous, same size and dtype '
                       '(member m owns [m len, (m + 1) len))')
  return dev, n // members


def ens_dot(a, b, members, partials, which):
  """partials[m, which, :] = stored partial sums of a_m . b_m."""
  dev, ln = _ens_check(members, a, b)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_ens_dot(
        _ptr(a), _ptr(b), ln, members, _ptr(partials), int(which),
        _dtype_code(a), _stream(dev)), 'sfem_ens_dot')


def ens_init(scalars, partials, members, maxiter, tol, atol):
  dev = _dev(scalars, partials)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_ens_init(
        _ptr(scalars), _ptr(partials), members, float(maxiter), float(tol),
        float(atol), _stream(dev)), 'sfem_ens_init')


def ens_update_r(r, ap, members, scalars, partials):
  dev, ln = _ens_check(members, r, ap)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_ens_update_r(
        _ptr(r), _ptr(ap), ln, members, _ptr(scalars), _ptr(partials),
        _dtype_code(r), _stream(dev)), 'sfem_ens_update_r')


def ens_close(scalars, partials, members, maxiter):
  dev = _dev(scalars, partials)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_ens_close(
        _ptr(scalars), _ptr(partials), members, float(maxiter), _stream(dev)),
        'sfem_ens_close')


def ens_update_xp(x, p, z, members, scalars):
  dev, ln = _ens_check(members, x, p, z)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_ens_update_xp(
        _ptr(x), _ptr(p), _ptr(z), ln, members, _ptr(scalars), _dtype_code(x),
        _stream(dev)), 'sfem_ens_update_xp')


def ens_update_r_mean(r, ap, w, members, scalars, partials, sums):
  dev, ln = _ens_check(members, r, ap)
  if w.numel() != ln or w.dtype != r.dtype or not w.is_contiguous():
    raise ValueError('ens_update_r_mean: weights of one member')
  _dev(w, sums)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_ens_update_r_mean(
        _ptr(r), _ptr(ap), _ptr(w), ln, members, _ptr(scalars), _ptr(partials),
        _ptr(sums), _dtype_code(r), _stream(dev)), 'sfem_ens_update_r_mean')


def ens_close_mean(scalars, partials, sums, total, members, maxiter):
  dev = _dev(scalars, partials, sums)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_ens_close_mean(
        _ptr(scalars), _ptr(partials), _ptr(sums), float(total), members,
        float(maxiter), _stream(dev)), 'sfem_ens_close_mean')


def ens_update_xp_mean(x, p, r, members, scalars):
  dev, ln = _ens_check(members, x, p, r)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_ens_update_xp_mean(
        _ptr(x), _ptr(p), _ptr(r), ln, members, _ptr(scalars), _dtype_code(x),
        _stream(dev)), 'sfem_ens_update_xp_mean')


def ens_subtract_weighted_mean(w, b, total, members, partials, out=None):
  """out_m = w_m - (b . w_m / total) 1 for every member (b: one member)."""
  w, b = w.contiguous(), b.contiguous()
  if out is None:
    out = torch.empty_like(w)
  dev, ln = _ens_check(members, w, out)
  if b.numel() != ln or b.dtype != w.dtype:
    raise ValueError('ens_subtract_weighted_mean: weights of one member')
  _dev(b, partials)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_ens_subtract_weighted_mean(
        _ptr(w), _ptr(b), float(total), _ptr(out), _ptr(partials), ln, members,
        _dtype_code(w), _stream(dev)), 'sfem_ens_subtract_weighted_mean')
  return out


def fold_layers(ext, count, layers):
  """ext[:count] += its layers (in place); returns the view ext[:count]."""
  dev = _dev(ext)
  ln, off, n = _layer_arrays(layers)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_fold_layers(
        _ptr(ext), int(count), ln, off, n, _dtype_code(ext), _stream(dev)),
        'sfem_fold_layers')
  return ext[:count]


def stokes_setup(invjac, jacdet, weights_nd):
  """Weighted cofactor planes (E, d*d, Q) for curved elements."""
  invjac, jacdet = invjac.contiguous(), jacdet.contiguous()
  dev = _dev(invjac, jacdet, weights_nd)
  E, Q, d, _ = invjac.shape
  kfac = torch.empty((E, d * d, Q), dtype=invjac.dtype, device=dev)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_stokes_setup(
        _ptr(invjac), _ptr(jacdet), _ptr(weights_nd), _ptr(kfac), E, d, Q,
        _dtype_code(invjac), _stream(dev)), 'sfem_stokes_setup')
  return kfac


def _stokes_args(vec, enc, penc, part, host, ndim, P, zero_range,
                 shared_order=None, **ptrs):
  node_stride = comp_stride = 0
  if not vec.is_contiguous():
    node_stride, comp_stride = 1, vec.stride(-1)
  ft = part.get('facet_table')
  ch = part.get('chains') if ft is not None else None
  if ft is not None:
    ptrs = dict(ptrs, facet_table=_dptr(ft), chain_offsets=_dptr(ch[0]),
                chain_elems=_dptr(ch[1]), num_chains=ch[0].numel() - 1)
    shared_order = None
  return _lib.StokesArgs(
      enc=_dptr(enc), penc=_dptr(penc), **_launch_fields(part, host, 'kfac'),
      interp=_hptr(host['interp']), num_elements=enc.shape[0],
      num_nodes=vec.shape[0], zero_begin=int(zero_range[0]),
      zero_end=int(zero_range[1]), ndim=ndim, P=P, dtype=_dtype_code(vec),
      node_stride=node_stride,
      comp_stride=comp_stride, shared_order=_dptr(shared_order),
      shared_stride=0 if shared_order is None else shared_order.shape[1],
      **ptrs)


def _check_field(u, ndim):
  if u.dim() != 2 or u.shape[1] != ndim or not (
      u.is_contiguous() or is_component_major(u)):
    raise ValueError(f'expected a dense (N, {ndim}) velocity field')


def stokes_div(u, p_out, enc, penc, parts, host, ndim, P, scale=None,
               dot_with=None, dot_out=None):
  """p_out <- D(scale * u) (navier_stokes.py:313-333), one launch per
  geometry kind.  `dot_out` (SFEM_DOT_SLOTS doubles) accumulates partial sums
  of `dot_with . p_out`."""
  dev = _dev(enc, p_out)
  _check_field(u, ndim)
  per_node = scale is not None and scale.dim() == 1
  if per_node:
    if scale.shape[0] != u.shape[0] or not scale.is_contiguous():
      raise ValueError('per-node scale must be a contiguous (N,) vector')
  elif scale is not None:
    _check_field(scale, ndim)
    if scale.stride() != u.stride():
      raise ValueError('scale must share the layout of u')
  if scale is not None and scale.dtype != u.dtype:
    raise ValueError('scale must share the dtype of u')
  host = {k: _host(v, u.dtype) for k, v in host.items()}
  with torch.cuda.device(dev):
    for part in parts:
      args = _stokes_args(u, enc, penc, part, host, ndim, P, (0, 0),
                          u=u.data_ptr(), p_out=p_out.data_ptr(),
                          scale=_dptr(scale), scale_per_node=int(per_node),
                          p_in=_dptr(dot_with if dot_out is not None else None),
                          dot_out=_dptr(dot_out))
      _lib.check(_lib.load().sfem_stokes_div(ctypes.byref(args), _stream(dev)),
                 'sfem_stokes_div')
  return p_out


def stokes_grad_t(p, out, enc, penc, parts, host, ndim, P, zero_range,
                  shared_order=None, scale=None):
  """out <- mask * QQ^T-ready (scale * D^T p) (navier_stokes.py:322-338);
  `scale`: (N,) or field-shaped factor applied to every contribution before
  it is assembled (valid for factors equal on all copies of a node)."""
  dev = _dev(enc, p)
  _check_field(out, ndim)
  per_node = _scale_args(scale, out, ndim)
  host = {k: _host(v, out.dtype) for k, v in host.items()}
  with torch.cuda.device(dev):
    for n, part in enumerate(parts):
      args = _stokes_args(out, enc, penc, part, host, ndim, P,
                          zero_range if n == 0 else (0, 0), shared_order,
                          out=out.data_ptr(), p_in=p.data_ptr(),
                          scale=_dptr(scale), scale_per_node=int(per_node))
      _lib.check(_lib.load().sfem_stokes_grad_t(ctypes.byref(args),
                                                _stream(dev)),
                 'sfem_stokes_grad_t')
  return out


def _scale_args(scale, field, ndim):
  per_node = scale is not None and scale.dim() == 1
  if per_node:
    if scale.shape[0] != field.shape[0] or not scale.is_contiguous():
      raise ValueError('per-node scale must be a contiguous (N,) vector')
  elif scale is not None:
    _check_field(scale, ndim)
    if scale.stride() != field.stride():
      raise ValueError('scale must share the layout of the velocity field')
  if scale is not None and scale.dtype != field.dtype:
    raise ValueError('scale must share the dtype of the velocity field')
  return per_node


def stokes_e_first(p, w, p_out, enc, penc, parts, host, ndim, P, zero_range,
                   scale=None, shared_order=None):
  """First half of E = D Q D^T (`sfem_stokes_e_first`): `w` receives D^T p at
  the SHARED nodes only, `p_out` = D(scale * complete part)."""
  dev = _dev(enc, p, p_out)
  _check_field(w, ndim)
  per_node = _scale_args(scale, w, ndim)
  host = {k: _host(v, w.dtype) for k, v in host.items()}
  with torch.cuda.device(dev):
    for n, part in enumerate(parts):
      args = _stokes_args(w, enc, penc, part, host, ndim, P,
                          zero_range if n == 0 else (0, 0), shared_order,
                          out=w.data_ptr(), p_in=p.data_ptr(),
                          p_out=p_out.data_ptr(), scale=_dptr(scale),
                          scale_per_node=int(per_node))
      _lib.check(_lib.load().sfem_stokes_e_first(ctypes.byref(args),
                                                 _stream(dev)),
                 'sfem_stokes_e_first')
  return p_out


def stokes_e_second(w, p_out, enc, penc, parts, host, ndim, P, scale=None):
  """Second half: p_out += D(scale * w restricted to the SHARED nodes)."""
  dev = _dev(enc, p_out)
  _check_field(w, ndim)
  per_node = _scale_args(scale, w, ndim)
  host = {k: _host(v, w.dtype) for k, v in host.items()}
  with torch.cuda.device(dev):
    for part in parts:
      args = _stokes_args(w, enc, penc, part, host, ndim, P, (0, 0),
                          u=w.data_ptr(), p_out=p_out.data_ptr(),
                          scale=_dptr(scale), scale_per_node=int(per_node))
      _lib.check(_lib.load().sfem_stokes_e_second(ctypes.byref(args),
                                                  _stream(dev)),
                 'sfem_stokes_e_second')
  return p_out


def stokes_convect_local(u_local, parts, host, ndim, P):
  """(E, P^d, d) values on a collocated grid -> w detJ (u . grad) u there."""
  u_local = u_local.contiguous()
  dev = _dev(u_local)
  E, n, d = u_local.shape
  if d != ndim or n != P ** ndim:
    raise ValueError(f'expected (E, {P ** ndim}, {ndim}) local values, got '
                     f'{tuple(u_local.shape)}')
  out = torch.empty_like(u_local)
  host = {k: _host(v, u_local.dtype) for k, v in host.items()}
  with torch.cuda.device(dev):
    for part in parts:
      args = _lib.StokesArgs(
          u=u_local.data_ptr(), out=out.data_ptr(),
          **_launch_fields(part, host, 'kfac'), num_elements=E, ndim=ndim,
          P=P, dtype=_dtype_code(u_local))
      _lib.check(_lib.load().sfem_stokes_convect_local(ctypes.byref(args),
                                                       _stream(dev)),
                 'sfem_stokes_convect_local')
  return out


def _field(t, name, shape, ref, ref_name, keep):
  """An optional input of the transport entry points: None, or `t` made
  contiguous after checking `shape` and the dtype and device of `ref`
  (`ref_name` in the error text).  `keep` collects the result, which holds a
  possible copy alive until the launches."""
  if t is None:
    return None
  if tuple(t.shape) != shape:
    raise ValueError(f'{name}: expected {shape}, got {tuple(t.shape)}')
  if t.dtype != ref.dtype or t.device != ref.device:
    raise ValueError(f'{name}: expected the dtype and device of the '
                     f'{ref_name}')
  t = t.contiguous()
  keep.append(t)
  return t


def transport_rhs(levels, parts, host, ndim, P, source=None, wdet=None):
  """The BDF/EXT right-hand side of scalar transport on a collocated grid
  (`sfem_transport_rhs`).  `levels`: up to three tuples (T (E, P^d), u
  (E, P^d, d) or None, mass_coef, conv_coef); `source`, `wdet` (E, P^d) or
  None.  Returns (E, P^d):
  wdet (source + sum_j mass_j T_j) + sum_j conv_j w detJ u_j . grad T_j."""
  levels = list(levels)
  if not 1 <= len(levels) <= _lib.SFEM_TRANSPORT_LEVELS:
    raise ValueError(f'expected 1..{_lib.SFEM_TRANSPORT_LEVELS} levels, got '
                     f'{len(levels)}')
  first = levels[0][0]
  dev = _dev(first)
  shape = (first.shape[0], P ** ndim)
  tensors = []
  field = lambda t, name, trailing=(): _field(
      t, name, shape + trailing, first, 'first scalar', tensors)
  args = _lib.TransportArgs(num_levels=len(levels))
  mass = source is not None
  for n, (T, u, mc, cc) in enumerate(levels):
    args.scalar[n] = _dptr(field(T, f'level {n}: scalar'))
    args.velocity[n] = _dptr(field(u, f'level {n}: velocity', (ndim,)))
    args.mass_coef[n], args.conv_coef[n] = float(mc), float(cc)
    mass = mass or float(mc) != 0.0
  if mass and wdet is None:
    raise ValueError('mass terms and a source need `wdet`')
  args.source = _dptr(field(source, 'source'))
  args.wdet = _dptr(field(wdet, 'wdet'))
  out = torch.empty(shape, dtype=first.dtype, device=dev)
  host = {k: _host(v, first.dtype) for k, v in host.items()}
  args.out = out.data_ptr()
  args.num_elements, args.ndim, args.P = shape[0], ndim, P
  args.dtype = _dtype_code(first)
  with torch.cuda.device(dev):
    for part in parts:
      for name, value in _launch_fields(part, host, 'kfac').items():
        setattr(args, name, value)
      _lib.check(_lib.load().sfem_transport_rhs(ctypes.byref(args),
                                                _stream(dev)),
                 'sfem_transport_rhs')
  return out


def transport_rhs_vjp(cotangent, levels, parts, host, ndim, P, wdet, want):
  """The vector-Jacobian product of `transport_rhs`
  (`sfem_transport_rhs_vjp`).  `cotangent` (E, P^d); `levels` as for
  `transport_rhs` (a level's T may be None when its velocity gradient is not
  wanted); `want` = ([(scalar?, velocity?) per level], source?).  One launch
  per geometry part covers all levels.  Returns ([(dT (E, P^d), du (E, P^d,
  d)) per level], dsource (E, P^d)) with None where not wanted; rows of
  elements that no part lists stay zero."""
  levels = list(levels)
  want_levels, want_source = want
  want_levels = [(bool(a), bool(b)) for a, b in want_levels]
  if ndim not in (2, 3) or not 2 <= P <= 12:
    raise NotImplementedError(
        f'transport_rhs_vjp: ndim={ndim}, P={P} outside the compiled range '
        '(ndim 2..3, P 2..12)')
  if not 1 <= len(levels) <= _lib.SFEM_TRANSPORT_LEVELS:
    raise ValueError(f'expected 1..{_lib.SFEM_TRANSPORT_LEVELS} levels, got '
                     f'{len(levels)}')
  if len(want_levels) != len(levels):
    raise ValueError(f'`want` names {len(want_levels)} levels, `levels` has '
                     f'{len(levels)}')
  if cotangent is None:
    raise ValueError('transport_rhs_vjp needs a cotangent')
  dev = _dev(cotangent)
  shape = (cotangent.shape[0], P ** ndim)
  tensors = []
  field = lambda t, name, trailing=(): _field(
      t, name, shape + trailing, cotangent, 'cotangent', tensors)
  lam = field(cotangent, 'cotangent')
  args = _lib.TransportVjpArgs(num_levels=len(levels),
                               cotangent=lam.data_ptr())
  zeros = lambda s: torch.zeros(s, dtype=lam.dtype, device=dev)
  mass = bool(want_source)
  out = []
  for n, ((T, u, mc, cc), (wT, wu)) in enumerate(zip(levels, want_levels)):
    if wu and (T is None or u is None):
      raise ValueError(f'level {n}: the velocity gradient needs the level\'s '
                       'scalar and velocity')
    args.scalar[n] = _dptr(field(T if wu else None, f'level {n}: scalar'))
    args.velocity[n] = _dptr(field(u, f'level {n}: velocity', (ndim,)))
    args.mass_coef[n], args.conv_coef[n] = float(mc), float(cc)
    mass = mass or (wT and float(mc) != 0.0)
    dT = zeros(shape) if wT else None
    du = zeros(shape + (ndim,)) if wu else None
    args.dscalar[n], args.dvelocity[n] = _dptr(dT), _dptr(du)
    out.append((dT, du))
  if mass and wdet is None:
    raise ValueError('mass terms and the source gradient need `wdet`')
  args.wdet = _dptr(field(wdet, 'wdet'))
  dsource = zeros(shape) if want_source else None
  args.dsource = _dptr(dsource)
  host = {k: _host(v, lam.dtype) for k, v in host.items()}
  args.num_elements, args.ndim, args.P = shape[0], ndim, P
  args.dtype = _dtype_code(lam)
  with torch.cuda.device(dev):
    for part in parts:
      for name, value in _launch_fields(part, host, 'kfac').items():
        setattr(args, name, value)
      _lib.check(_lib.load().sfem_transport_rhs_vjp(ctypes.byref(args),
                                                    _stream(dev)),
                 'sfem_transport_rhs_vjp')
  return out, dsource


def _local_shape(x, ndim, P, wdet, who):
  """(E, n, d) of the (E, P^d, d) values `x` of an elasticity-family launch,
  after the checks every one of them makes; `who` needs `wdet`."""
  E, n, d = x.shape
  if d != ndim or n != P ** ndim:
    raise ValueError(f'expected (E, {P ** ndim}, {ndim}) local values, got '
                     f'{tuple(x.shape)}')
  if wdet is None:
    raise ValueError(f'{who} needs `wdet`')
  return E, n, d


def _coefficients(args, field, triples):
  """Coefficients that are a float or an (E, P^d) tensor each: `triples` of
  (field of `args` for the tensor, field for the float, value)."""
  for name, const, value in triples:
    if isinstance(value, torch.Tensor):
      setattr(args, name, field(value, name).data_ptr())
    else:
      setattr(args, const, float(value))


def _lame(lam, mu, rho=None):
  """The triples of `_coefficients` for lam, mu and rho (None = 1)."""
  return (('lam', 'lam_const', lam), ('mu', 'mu_const', mu),
          ('rho', 'rho_const', 1.0 if rho is None else rho))


def _launch_parts(entry, args, ref, E, ndim, P, parts, host):
  """One launch of the entry point `entry` per geometry part, after the sizes
  and the dtype of `ref` are set in `args`."""
  dev = ref.device
  host = {k: _host(v, ref.dtype) for k, v in host.items()}
  args.num_elements, args.ndim, args.P = E, ndim, P
  args.dtype = _dtype_code(ref)
  fn = getattr(_lib.load(), entry)
  with torch.cuda.device(dev):
    for part in parts:
      for name, value in _launch_fields(part, host, 'kfac').items():
        setattr(args, name, value)
      _lib.check(fn(ctypes.byref(args), _stream(dev)), entry)


def elasticity_local(u_q, parts, host, ndim, P, wdet, lam, mu, rho=None,
                     lambda0=0.0):
  """Linear elasticity on a collocated grid (`sfem_elasticity_local`): `u_q`
  (E, P^d, d) -> K u + lambda0 M_rho u there, (E, P^d, d).  `wdet` (E, P^d);
  `lam`, `mu`, `rho`: a float or an (E, P^d) tensor each (`rho` None = 1)."""
  u_q = u_q.contiguous()
  _dev(u_q)
  E, n, d = _local_shape(u_q, ndim, P, wdet, 'elasticity_local')
  tensors = []
  field = lambda t, name: _field(t, name, (E, n), u_q, 'displacement', tensors)
  args = _lib.ElasticityArgs(u=u_q.data_ptr(), lambda0=float(lambda0),
                             wdet=field(wdet, 'wdet').data_ptr())
  _coefficients(args, field, _lame(lam, mu, rho))
  out = torch.empty_like(u_q)
  args.out = out.data_ptr()
  _launch_parts('sfem_elasticity_local', args, u_q, E, ndim, P, parts, host)
  return out


def hyperelastic_local(u_q, parts, host, ndim, P, wdet, lam, mu, rho=None,
                       lambda0=0.0, *, mode, state=None, want_state=False,
                       want_psi=False):
  """The neo-Hookean residual or tangent on a collocated grid
  (`sfem_hyperelastic_local`): `u_q` (E, P^d, d), `wdet` (E, P^d); `lam`,
  `mu`, `rho` as in `elasticity_local`.

  `mode='residual'`: `u_q` is the displacement; returns (R (E, P^d, d), state,
  psi) with `state` (E, P^d, d*d + 1) -- per point F^-1 row-major, then ln J
  -- where `want_state`, and `psi` (E, P^d), whose sum is the energy, where
  `want_psi`; None otherwise.  `mode='tangent'`: `u_q` is the increment and
  `state` that of a residual launch; returns T w (E, P^d, d).  Rows of
  `state` and `psi` of elements that no part lists are zero."""
  if mode not in ('residual', 'tangent'):
    raise ValueError(f"mode: 'residual' or 'tangent', got {mode!r}")
  tangent = mode == 'tangent'
  u_q = u_q.contiguous()
  dev = _dev(u_q)
  E, n, d = _local_shape(u_q, ndim, P, wdet, 'hyperelastic_local')
  if tangent and (want_state or want_psi):
    raise ValueError('the state and psi are outputs of the residual mode')
  if tangent and state is None:
    raise ValueError('the tangent mode needs the `state` of a residual launch')
  if not tangent and state is not None:
    raise ValueError('`state` is an input of the tangent mode only')
  tensors = []
  field = lambda t, name: _field(t, name, (E, n), u_q, 'displacement', tensors)
  if tangent:
    state = _field(state, 'state', (E, n, d * d + 1), u_q, 'displacement',
                   tensors)
  elif want_state:
    state = torch.zeros((E, n, d * d + 1), dtype=u_q.dtype, device=dev)
  psi = (torch.zeros((E, n), dtype=u_q.dtype, device=dev) if want_psi
         else None)
  args = _lib.HyperelasticArgs(
      u=u_q.data_ptr(), lambda0=float(lambda0),
      wdet=field(wdet, 'wdet').data_ptr(), state=_dptr(state), psi=_dptr(psi),
      mode=_lib.SFEM_HYPER_TANGENT if tangent else _lib.SFEM_HYPER_RESIDUAL)
  _coefficients(args, field, _lame(lam, mu, rho))
  out = torch.empty_like(u_q)
  args.out = out.data_ptr()
  _launch_parts('sfem_hyperelastic_local', args, u_q, E, ndim, P, parts, host)
  return out if tangent else (out, state, psi)


def plasticity_sizes(ndim):
  """(NH, NL, NV): reals per point of the history, of the tangent's state
  and of the stress of `sfem_plasticity_local`."""
  return {2: (4, 5, 4), 3: (7, 8, 6)}[ndim]


def plasticity_local(u_q, parts, host, ndim, P, wdet, lam, mu, rho, lambda0,
                     yield_stress, hardening, *, mode, hist=None, lin=None,
                     want_hist=False, want_lin=False, want_stress=False):
  """The J2 plasticity residual or tangent on a collocated grid
  (`sfem_plasticity_local`): `u_q` (E, P^d, d), `wdet` (E, P^d); `lam`, `mu`,
  `rho` as in `elasticity_local`, `yield_stress` and `hardening` likewise a
  float or an (E, P^d) tensor each.

  `mode='residual'`: `u_q` is the displacement and `hist` the committed
  history (E, P^d, NH), None for virgin material; it is read only.  Returns
  (R (E, P^d, d), trial history (E, P^d, NH), lin (E, P^d, NL), stress
  (E, P^d, NV)), the last three where `want_hist`, `want_lin`, `want_stress`
  and None otherwise.  `mode='tangent'`: `u_q` is the increment and `lin`
  that of a residual launch; returns T w (E, P^d, d).  Rows of the optional
  outputs of elements that no part lists are zero."""
  if mode not in ('residual', 'tangent'):
    raise ValueError(f"mode: 'residual' or 'tangent', got {mode!r}")
  tangent = mode == 'tangent'
  u_q = u_q.contiguous()
  dev = _dev(u_q)
  E, n, d = _local_shape(u_q, ndim, P, wdet, 'plasticity_local')
  NH, NL, NV = plasticity_sizes(ndim)
  if tangent and (want_hist or want_lin or want_stress or hist is not None):
    raise ValueError('the history, lin and the stress belong to the residual '
                     'mode')
  if tangent and lin is None:
    raise ValueError('the tangent mode needs the `lin` of a residual launch')
  if not tangent and lin is not None:
    raise ValueError('`lin` is an input of the tangent mode only')
  tensors = []
  field = lambda t, name: _field(t, name, (E, n), u_q, 'displacement', tensors)
  if tangent:
    lin = _field(lin, 'lin', (E, n, NL), u_q, 'displacement', tensors)
  elif hist is not None:
    hist = _field(hist, 'hist', (E, n, NH), u_q, 'displacement', tensors)
  zeros = lambda k: torch.zeros((E, n, k), dtype=u_q.dtype, device=dev)
  hist_out = zeros(NH) if want_hist else None
  if want_lin:
    lin = zeros(NL)
  stress = zeros(NV) if want_stress else None
  args = _lib.PlasticityArgs(
      u=u_q.data_ptr(), lambda0=float(lambda0),
      wdet=field(wdet, 'wdet').data_ptr(), hist_in=_dptr(hist),
      hist_out=_dptr(hist_out), lin=_dptr(lin), stress=_dptr(stress),
      mode=_lib.SFEM_PLAST_TANGENT if tangent else _lib.SFEM_PLAST_RESIDUAL)
  _coefficients(args, field, _lame(lam, mu, rho) + (
      ('yield', 'yield_const', yield_stress),
      ('hard', 'hard_const', hardening)))
  out = torch.empty_like(u_q)
  args.out = out.data_ptr()
  _launch_parts('sfem_plasticity_local', args, u_q, E, ndim, P, parts, host)
  return out if tangent else (out, hist_out, lin, stress)


def plasticity_vjp(u_q, parts, host, ndim, P, wdet, lam, mu, yield_stress,
                   hardening, *, mode, hist=None, hbar=None, w_q=None,
                   lambda0=0.0, want=(True,) * 5, want_history=True):
  """The vector-Jacobian product of the radial return on a collocated grid
  (`sfem_plasticity_vjp`): `u_q` (E, P^d, d) the displacement, `hist` the
  committed history (E, P^d, NH) or None for virgin material, `hbar` the
  cotangent of the trial history (eps_p', alpha') in the stored layout;
  `wdet` and the coefficients as in `plasticity_local`.  The return mapping
  is repeated from `u_q` and `hist`; nothing is written to an input.

  `mode='displacement'`: returns d(hbar . Phi)/du (E, P^d, d) for the history
  update Phi; `hbar` is required.  `mode='state'`: for the second field `w_q`
  (E, P^d, d) returns (hbar_prev (E, P^d, NH), dlam, dmu, dyield, dhard, drho
  (E, P^d) each): the derivatives of w . R(u) + hbar . Phi(u) (`hbar` None =
  0) by the committed history and the point's coefficients, drho = lambda0 W
  u . w; `hbar_prev` is None unless `want_history`, the others where `want`
  is false.  Rows of elements that no part lists are zero."""
  if mode not in ('displacement', 'state'):
    raise ValueError(f"mode: 'displacement' or 'state', got {mode!r}")
  state = mode == 'state'
  u_q = u_q.contiguous()
  dev = _dev(u_q)
  E, n, d = _local_shape(u_q, ndim, P, wdet, 'plasticity_vjp')
  NH = plasticity_sizes(ndim)[0]
  want = tuple(bool(w) for w in want)
  if len(want) != 5:
    raise ValueError('`want` names (dlam, dmu, dyield, dhard, drho)')
  tensors = []
  field = lambda t, name: _field(t, name, (E, n), u_q, 'displacement', tensors)
  hist = _field(hist, 'hist', (E, n, NH), u_q, 'displacement', tensors)
  hbar = _field(hbar, 'hbar', (E, n, NH), u_q, 'displacement', tensors)
  w_q = _field(w_q, 'second field', (E, n, d), u_q, 'displacement', tensors)
  args = _lib.PlasticityVjpArgs(
      u=u_q.data_ptr(), w=_dptr(w_q), lambda0=float(lambda0),
      wdet=field(wdet, 'wdet').data_ptr(), hist_in=_dptr(hist),
      hbar=_dptr(hbar),
      mode=(_lib.SFEM_PLAST_VJP_STATE if state
            else _lib.SFEM_PLAST_VJP_DISPLACEMENT))
  _coefficients(args, field, (
      ('lam', 'lam_const', lam), ('mu', 'mu_const', mu),
      ('yield', 'yield_const', yield_stress),
      ('hard', 'hard_const', hardening)))
  if not state:
    if hbar is None:
      raise ValueError('the displacement mode needs the cotangent `hbar`')
    if w_q is not None:
      raise ValueError('`w_q` is an input of the state mode only')
    out = torch.empty_like(u_q)
    args.out = out.data_ptr()
    _launch_parts('sfem_plasticity_vjp', args, u_q, E, ndim, P, parts, host)
    return out
  if w_q is None:
    raise ValueError('the state mode needs the second field `w_q`')
  if not (any(want) or want_history):
    raise ValueError('the state mode needs an output: `want` or '
                     '`want_history`')
  zeros = lambda *k: torch.zeros((E, n) + k, dtype=u_q.dtype, device=dev)
  hbar_prev = zeros(NH) if want_history else None
  outs = tuple(zeros() if w else None for w in want)
  args.hbar_prev = _dptr(hbar_prev)
  for name, t in zip(('dlam', 'dmu', 'dyield', 'dhard', 'drho'), outs):
    setattr(args, name, _dptr(t))
  _launch_parts('sfem_plasticity_vjp', args, u_q, E, ndim, P, parts, host)
  return (hbar_prev,) + outs


def elasticity_sens(u_q, v_q, parts, host, ndim, P, wdet, lambda0=0.0,
                    want=(True, True, True)):
  """Per-point sensitivities of v . (K + lambda0 M_rho) u with respect to
  (lam, mu, rho) on a collocated grid (`sfem_elasticity_sens`): `u_q`, `v_q`
  (E, P^d, d), `wdet` (E, P^d).  Returns (dlam, dmu, drho), (E, P^d) each,
  None where `want` is false."""
  u_q = u_q.contiguous()
  dev = _dev(u_q)
  E, n, d = _local_shape(u_q, ndim, P, wdet, 'elasticity_sens')
  want = tuple(bool(w) for w in want)
  if len(want) != 3 or not any(want):
    raise ValueError('`want` names (dlam, dmu, drho), at least one of them')
  tensors = []
  v_q = _field(v_q, 'second field', (E, n, d), u_q, 'displacement', tensors)
  if v_q is None:
    raise ValueError('elasticity_sens needs two fields')
  wdet = _field(wdet, 'wdet', (E, n), u_q, 'displacement', tensors)
  out = tuple(torch.zeros((E, n), dtype=u_q.dtype, device=dev) if w else None
              for w in want)
  args = _lib.ElasticitySensArgs(
      u=u_q.data_ptr(), v=v_q.data_ptr(), wdet=wdet.data_ptr(),
      dlam=_dptr(out[0]), dmu=_dptr(out[1]), drho=_dptr(out[2]),
      lambda0=float(lambda0))
  _launch_parts('sfem_elasticity_sens', args, u_q, E, ndim, P, parts, host)
  return out


def hyperelastic_sens(v_q, state, parts, host, ndim, P, wdet, u_q=None,
                      lambda0=0.0, want=(True, True, True)):
  """Per-point sensitivities of v . R(u) of the neo-Hookean residual with
  respect to (lam, mu, rho) on a collocated grid (`sfem_hyperelastic_sens`):
  `v_q` (E, P^d, d), `state` (E, P^d, d*d + 1) as a residual launch of
  `hyperelastic_local` stored it at u, `wdet` (E, P^d); `u_q` (E, P^d, d) is
  read for drho alone.  Returns (dlam, dmu, drho), (E, P^d) each, None where
  `want` is false."""
  v_q = v_q.contiguous()
  dev = _dev(v_q)
  E, n, d = _local_shape(v_q, ndim, P, wdet, 'hyperelastic_sens')
  want = tuple(bool(w) for w in want)
  if len(want) != 3 or not any(want):
    raise ValueError('`want` names (dlam, dmu, drho), at least one of them')
  tensors = []
  state = _field(state, 'state', (E, n, d * d + 1), v_q, 'second field',
                 tensors)
  if state is None:
    raise ValueError('hyperelastic_sens needs the `state` of a residual '
                     'launch')
  u_q = _field(u_q, 'displacement', (E, n, d), v_q, 'second field', tensors)
  if want[2] and u_q is None:
    raise ValueError('drho needs the displacement `u_q`')
  wdet = _field(wdet, 'wdet', (E, n), v_q, 'second field', tensors)
  out = tuple(torch.zeros((E, n), dtype=v_q.dtype, device=dev) if w else None
              for w in want)
  args = _lib.HyperelasticSensArgs(
      v=v_q.data_ptr(), state=state.data_ptr(), u=_dptr(u_q),
      wdet=wdet.data_ptr(), dlam=_dptr(out[0]), dmu=_dptr(out[1]),
      drho=_dptr(out[2]), lambda0=float(lambda0))
  _launch_parts('sfem_hyperelastic_sens', args, v_q, E, ndim, P, parts, host)
  return out


def elasticity_stress(u_q, parts, host, ndim, P, wdet, lam, mu,
                      want=(True, False), plane_stress=False):
  """Stress of a displacement on a collocated grid
  (`sfem_elasticity_stress`): `u_q` (E, P^d, d), `wdet` (E, P^d); `lam`, `mu`:
  a float or an (E, P^d) tensor each.  Returns (sigma (E, P^d, NV), von Mises
  (E, P^d)), None where `want` is false; NV = 6 with slots (xx, yy, zz, xy,
  xz, yz) in 3D, 4 with slots (xx, yy, xy, zz) in 2D, where `plane_stress`
  sets sigma_zz = 0 (lam is then the modified lambda of `lame_parameters`).
  Rows of elements that no part lists and points with wdet = 0 are zero."""
  u_q = u_q.contiguous()
  dev = _dev(u_q)
  E, n, d = _local_shape(u_q, ndim, P, wdet, 'elasticity_stress')
  want = tuple(bool(w) for w in want)
  if len(want) != 2 or not any(want):
    raise ValueError('`want` names (sigma, von Mises), at least one of them')
  nv = 6 if ndim == 3 else 4
  tensors = []
  field = lambda t, name: _field(t, name, (E, n), u_q, 'displacement', tensors)
  zeros = lambda *s: torch.zeros(s, dtype=u_q.dtype, device=dev)
  sigma = zeros(E, n, nv) if want[0] else None
  vm = zeros(E, n) if want[1] else None
  args = _lib.ElasticityStressArgs(
      u=u_q.data_ptr(), sigma=_dptr(sigma), vm=_dptr(vm),
      wdet=field(wdet, 'wdet').data_ptr(), plane_stress=int(bool(plane_stress)))
  _coefficients(args, field, _lame(lam, mu)[:2])
  _launch_parts('sfem_elasticity_stress', args, u_q, E, ndim, P, parts, host)
  return sigma, vm


def elasticity_stress_vjp(s_bar, u_q, parts, host, ndim, P, wdet, lam, mu,
                          want=(True, True, True), plane_stress=False):
  """The vector-Jacobian product of `elasticity_stress`
  (`sfem_elasticity_stress_vjp`): `s_bar` (E, P^d, NV) the cotangent of
  sigma, `u_q` (E, P^d, d) the displacement (needed for dlam / dmu only, else
  it may be None).  Returns (ubar (E, P^d, d), dlam (E, P^d), dmu (E, P^d)),
  None where `want` is false."""
  s_bar = s_bar.contiguous()
  dev = _dev(s_bar)
  nv = 6 if ndim == 3 else 4
  E, n = s_bar.shape[0], P ** ndim
  if tuple(s_bar.shape) != (E, n, nv):
    raise ValueError(f'expected an (E, {n}, {nv}) stress cotangent, got '
                     f'{tuple(s_bar.shape)}')
  if wdet is None:
    raise ValueError('elasticity_stress_vjp needs `wdet`')
  want = tuple(bool(w) for w in want)
  if len(want) != 3 or not any(want):
    raise ValueError('`want` names (ubar, dlam, dmu), at least one of them')
  tensors = []
  field = lambda t, name: _field(t, name, (E, n), s_bar, 'cotangent', tensors)
  u_q = _field(u_q, 'displacement', (E, n, ndim), s_bar, 'cotangent', tensors)
  if u_q is None and (want[1] or want[2]):
    raise ValueError('dlam and dmu need the displacement')
  zeros = lambda *s: torch.zeros(s, dtype=s_bar.dtype, device=dev)
  out = (zeros(E, n, ndim) if want[0] else None,
         zeros(E, n) if want[1] else None, zeros(E, n) if want[2] else None)
  args = _lib.ElasticityStressVjpArgs(
      sbar=s_bar.data_ptr(), u=_dptr(u_q), ubar=_dptr(out[0]),
      dlam=_dptr(out[1]), dmu=_dptr(out[2]),
      wdet=field(wdet, 'wdet').data_ptr(), plane_stress=int(bool(plane_stress)))
  _coefficients(args, field, _lame(lam, mu)[:2])
  _launch_parts('sfem_elasticity_stress_vjp', args, s_bar, E, ndim, P, parts,
                host)
  return out


# ------------------------------------------------------------ fields at points
def point_locate(points, node_coords, elements, grid, nodes, bary, max_iter,
                 tol_xi, tol_x):
  """`sfem_point_locate`: (element (M,) int32, xi (M, d), found (M,) bool) of
  `points` (M, d) in the mesh (`node_coords`, `elements`).  `grid` holds the
  candidate lists of `core.points.CandidateGrid` on the device; `nodes` and
  `bary` are the host tables of the 1D basis."""
  points = points.contiguous()
  dev = _dev(points, node_coords, elements, grid.cell_offsets, grid.cell_elems,
             grid.boxes, grid.extent)
  M, ndim = points.shape
  element = torch.empty(M, dtype=torch.int32, device=dev)
  xi = torch.empty((M, ndim), dtype=points.dtype, device=dev)
  found = torch.empty(M, dtype=torch.uint8, device=dev)
  nodes = np.ascontiguousarray(nodes, dtype=np.float64)
  bary = np.ascontiguousarray(bary, dtype=np.float64)
  args = _lib.PointLocateArgs(
      points=_dptr(points), node_coords=_dptr(node_coords),
      elements=_dptr(elements), cell_offsets=_dptr(grid.cell_offsets),
      cell_elems=_dptr(grid.cell_elems), boxes=_dptr(grid.boxes),
      extent=_dptr(grid.extent), nodes=_hptr(nodes), bary=_hptr(bary),
      element=_dptr(element), xi=_dptr(xi), found=_dptr(found),
      tol_xi=float(tol_xi), tol_x=float(tol_x), num_points=M,
      num_nodes=node_coords.shape[0], num_elements=elements.shape[0],
      max_iter=int(max_iter), ndim=ndim, P1=len(nodes),
      dtype=_dtype_code(points))
  for a in range(ndim):
    args.grid_lo[a], args.grid_hi[a] = float(grid.lo[a]), float(grid.hi[a])
    args.inv_cell[a], args.ncell[a] = float(grid.inv_cell[a]), int(grid.ncell[a])
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_point_locate(ctypes.byref(args), _stream(dev)),
               'sfem_point_locate')
  return element, xi, found.bool()


def _point_args(plan, values, ncomp):
  return _lib.PointArgs(
      values=_dptr(values), elements=_dptr(plan.elements), xi=_dptr(plan.xi),
      perm=_dptr(plan.perm), chunk_elem=_dptr(plan.chunk_elem),
      chunk_start=_dptr(plan.chunk_start), chunk_count=_dptr(plan.chunk_count),
      seg_elem=_dptr(plan.seg_elem), seg_offsets=_dptr(plan.seg_offsets),
      nodes=_hptr(plan.nodes), bary=_hptr(plan.bary),
      num_points=plan.num_points, num_found=plan.num_found,
      num_chunks=plan.chunk_elem.numel(), num_segments=plan.seg_elem.numel(),
      num_elements=plan.elements.shape[0], num_nodes=plan.num_nodes,
      ncomp=ncomp, ndim=plan.ndim, P1=len(plan.nodes),
      dtype=_dtype_code(values))


def point_eval(u, plan, fill):
  """`sfem_point_eval`: a nodal field (N,), row-major (N, C) or
  component-major (N, C) at the points of `plan` (`core.points.PointPlan`):
  (M,) or (M, C), `fill` where a point was not found."""
  ncomp, ns, cs = _node_view(u)
  dev = _dev(u.movedim(-1, 0) if is_component_major(u) else u, plan.elements,
             plan.xi, plan.perm, plan.chunk_elem)
  if u.dtype != plan.xi.dtype:
    raise ValueError(f'field dtype {u.dtype} differs from the mesh dtype '
                     f'{plan.xi.dtype}')
  shape = (plan.num_points,) if u.dim() == 1 else (plan.num_points, ncomp)
  out = torch.full(shape, fill, dtype=u.dtype, device=dev)
  args = _point_args(plan, out, ncomp)
  args.field, args.node_stride, args.comp_stride = _dptr(u), ns, cs
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_point_eval(ctypes.byref(args), _stream(dev)),
               'sfem_point_eval')
  return out


def point_eval_t(w, plan):
  """`sfem_point_eval_t` and the deterministic assembly of its element-local
  rows: point weights (M,) or (M, C) to nodal (N,) or (N, C)."""
  w = w.contiguous()
  dev = _dev(w, plan.elements, plan.xi, plan.perm, plan.seg_elem,
             plan.seg_offsets)
  if w.dtype != plan.xi.dtype:
    raise ValueError(f'weight dtype {w.dtype} differs from the mesh dtype '
                     f'{plan.xi.dtype}')
  ncomp = 1 if w.dim() == 1 else w.shape[1]
  S = plan.seg_elem.numel()
  n = plan.elements.shape[1]
  shape = (plan.num_nodes,) if w.dim() == 1 else (plan.num_nodes, ncomp)
  if S == 0:
    return torch.zeros(shape, dtype=w.dtype, device=dev)
  rows = torch.empty((S, n, ncomp), dtype=w.dtype, device=dev)
  args = _point_args(plan, w, ncomp)
  args.rows = _dptr(rows)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_point_eval_t(ctypes.byref(args), _stream(dev)),
               'sfem_point_eval_t')
  offsets, slots = plan.scatter_csr
  return scatter_csr(rows, offsets, slots, plan.num_nodes, ncomp).reshape(shape)


from swirl_fem_amd.core.layout import is_component_major  # noqa: E402


def _check_vector_layout(u, out):
  for t in (u, out):
    if not t.is_cuda:
      raise RuntimeError(
          'swirl_fem_amd kernels run on MI355X device tensors only; got a '
          f'{t.device} tensor (there is no CPU fallback)')
    if not (t.is_contiguous() or is_component_major(t)):
      raise ValueError('expected a contiguous or component-major tensor')
  if u.stride() != out.stride() or u.shape != out.shape:
    raise ValueError('u and out must share shape and memory layout')


def helmholtz_local(u_local, parts, host, ndim, P, lambda0, lambda1,
                    transpose=False):
  if not (u_local.is_contiguous() or is_component_major(u_local)):
    u_local = u_local.contiguous()
  dev = u_local.device
  host = {k: _host(v, u_local.dtype) for k, v in host.items()}
  out = torch.empty_like(u_local)       # preserves the (dense) layout
  _check_vector_layout(u_local, out)
  with torch.cuda.device(dev):
    for part in parts:
      args = _helmholtz_args(u_local, out, None, part, host, ndim, P,
                             u_local.shape[0], 0, lambda0, lambda1, (0, 0),
                             transpose=transpose)
      _lib.check(_lib.load().sfem_helmholtz_local(ctypes.byref(args),
                                                  _stream(dev)),
                 'sfem_helmholtz_local')
  return out


def helmholtz_sens(u_local, lam_local, parts, host, ndim, P, lambda0, lambda1,
                   want=(True, True, True), out=None, ncomp=1):
  """Per-point sensitivities of lam . (lambda0 B_c + lambda1 A_k + C_beta) u
  (`sfem_helmholtz_sens`): `u_local`, `lam_local` (E, n) at the operator's
  points; `parts` the launches WITHOUT coefficients (bare G and W).  Returns
  (dkappa (E, n), dsigma (E, n), dbeta (E, n, ndim)), None where `want` is
  false; `out`: three tensors (or None) to write instead of new ones."""
  u_local = u_local.contiguous()
  lam_local = lam_local.contiguous()
  _check_vector_layout(u_local, lam_local)
  dev = u_local.device
  host = {k: _host(v, u_local.dtype) for k, v in host.items()}
  E, n = u_local.shape[0], u_local.shape[1]
  shapes = ((E, n), (E, n), (E, n, ndim))
  if out is None:
    out = tuple(torch.zeros(s, dtype=u_local.dtype, device=dev) if w else None
                for s, w in zip(shapes, want))
  for t, s in zip(out, shapes):
    if t is not None and (tuple(t.shape) != s or not t.is_contiguous() or
                          t.dtype != u_local.dtype or t.device != dev):
      raise ValueError(f'sensitivity output: expected a contiguous {s} '
                       'tensor of the field\'s dtype and device')
  with torch.cuda.device(dev):
    for part in parts:
      args = _lib.HelmholtzSensArgs(
          u=u_local.data_ptr(), lam=lam_local.data_ptr(),
          dkappa=_dptr(out[0]), dsigma=_dptr(out[1]), dbeta=_dptr(out[2]),
          **_launch_fields(part, host), num_elements=E, ndim=ndim, P=P,
          ncomp=ncomp, dtype=_dtype_code(u_local),
          lambda0=float(lambda0), lambda1=float(lambda1))
      _lib.check(_lib.load().sfem_helmholtz_sens(ctypes.byref(args),
                                                 _stream(dev)),
                 'sfem_helmholtz_sens')
  return out


# ------------------------------------------------------------------------ CG
def dot(a, b, result, slot, accumulate=False):
  """result[slot] (+)= sum(a * b); result is a float64 device tensor."""
  dev = _dev(a, b, result)
  fn = (_lib.load().sfem_dot_accumulate if accumulate
        else _lib.load().sfem_dot)
  with torch.cuda.device(dev):
    _lib.check(fn(_ptr(a), _ptr(b), a.numel(),
                  ctypes.c_void_p(result.data_ptr() + 8 * slot),
                  _dtype_code(a), _stream(dev)), 'sfem_dot')


def dot_indexed(a, b, idx, w, result, slot, scale):
  """result[slot] += scale * sum_i w[i] <a[idx[i]], b[idx[i]]>."""
  ncomp, ns, cs = _node_view(a)
  if _node_view(b) != (ncomp, ns, cs) or a.dtype != b.dtype:
    raise ValueError('dot_indexed: operands must share layout and dtype')
  flat = lambda t: t.movedim(-1, 0) if is_component_major(t) else t
  dev = _dev(flat(a), flat(b), idx, w, result)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_dot_indexed(
        _ptr(a), _ptr(b), _ptr(idx), _ptr(w), idx.numel(), ncomp, ns, cs,
        float(scale), result.data_ptr() + 8 * slot, _dtype_code(a),
        _stream(dev)), 'sfem_dot_indexed')


def cg_scalars(scalars, phase, maxiter, tol, atol, partials=None):
  dev = _dev(scalars, partials)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_cg_scalars(
        _ptr(scalars), phase, float(maxiter), float(tol), float(atol),
        _ptr(partials), _stream(dev)), 'sfem_cg_scalars')


def cg_update_xr(x, r, p, ap, scalars, fuse_rr):
  dev = _dev(x, r, p, ap, scalars)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_cg_update_xr(
        _ptr(x), _ptr(r), _ptr(p), _ptr(ap), x.numel(), _ptr(scalars),
        int(fuse_rr), _dtype_code(x), _stream(dev)), 'sfem_cg_update_xr')


def cg_update_p(p, z, scalars):
  dev = _dev(p, z, scalars)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_cg_update_p(
        _ptr(p), _ptr(z), p.numel(), _ptr(scalars), _dtype_code(p),
        _stream(dev)), 'sfem_cg_update_p')


def cg_update_r(r, ap, scalars, fuse_rr):
  dev = _dev(r, ap, scalars)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_cg_update_r(
        _ptr(r), _ptr(ap), r.numel(), _ptr(scalars), int(fuse_rr),
        _dtype_code(r), _stream(dev)), 'sfem_cg_update_r')


def cg_update_xp_lazy(x, pring, z, scalars, lazy):
  """p_{k+1} = z + beta p_k into the next slot of the ring `pring` (m, stride);
  x takes its m pending terms every m-th iteration (`sfem_cg_update_xp_lazy`)."""
  dev = _dev(x, pring, z, scalars, lazy)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_cg_update_xp_lazy(
        _ptr(x), _ptr(pring), pring.stride(0), _ptr(z), x.numel(),
        _ptr(scalars), _ptr(lazy), pring.shape[0], _dtype_code(x),
        _stream(dev)), 'sfem_cg_update_xp_lazy')


def cg_flush_x(x, pring, scalars, lazy):
  """Adds the terms of x the lazy update still holds back."""
  dev = _dev(x, pring, scalars, lazy)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_cg_flush_x(
        _ptr(x), _ptr(pring), pring.stride(0), x.numel(), _ptr(scalars),
        _ptr(lazy), pring.shape[0], _dtype_code(x), _stream(dev)),
        'sfem_cg_flush_x')


def cg_update_xp(x, p, z, scalars):
  dev = _dev(x, p, z, scalars)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_cg_update_xp(
        _ptr(x), _ptr(p), _ptr(z), x.numel(), _ptr(scalars), _dtype_code(x),
        _stream(dev)), 'sfem_cg_update_xp')


def cg_update_r_mean(r, ap, w, scalars, sums):
  dev = _dev(r, ap, w, scalars, sums)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_cg_update_r_mean(
        _ptr(r), _ptr(ap), _ptr(w), r.numel(), _ptr(scalars), _ptr(sums),
        _dtype_code(r), _stream(dev)), 'sfem_cg_update_r_mean')


def cg_update_xp_mean(x, p, r, scalars, sums, total):
  dev = _dev(x, p, r, scalars, sums)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_cg_update_xp_mean(
        _ptr(x), _ptr(p), _ptr(r), x.numel(), _ptr(scalars), _ptr(sums),
        float(total), _dtype_code(x), _stream(dev)), 'sfem_cg_update_xp_mean')


def axpby(a, x, b, y):
  """In place: y = a * x + b * y."""
  dev = _dev(x, y)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_axpby(
        float(a), _ptr(x), float(b), _ptr(y), x.numel(), _dtype_code(x),
        _stream(dev)), 'sfem_axpby')
  return y


# ----------------------------------------------------------------- BiCGStab
def bicgstab_scalars(scalars, phase, maxiter, tol, atol):
  dev = _dev(scalars)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_bicgstab_scalars(
        _ptr(scalars), int(phase), float(maxiter), float(tol), float(atol),
        _stream(dev)), 'sfem_bicgstab_scalars')


def bicgstab_dot(a, b, scalars, slot, two=False):
  """scalars[slot] += a . b (`two`: and scalars[slot + 1] += a . a)."""
  dev = _dev(a, b, scalars)
  if a.dtype != b.dtype or a.numel() != b.numel():
    raise ValueError('bicgstab_dot: operands must share size and dtype')
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_bicgstab_dot(
        _ptr(a), _ptr(b), a.numel(), _ptr(scalars), int(slot), int(two),
        _dtype_code(a), _stream(dev)), 'sfem_bicgstab_dot')


def _same(name, *ts):
  first = ts[0]
  for t in ts:
    if t is not None and (t.dtype != first.dtype or
                          t.numel() != first.numel()):
      raise ValueError(f'{name}: vectors must share size and dtype')


def bicgstab_update_p(p, phat, r, v, dinv, scalars):
  """p = r + beta (p - omega v); phat = dinv p (dinv None: phat unused)."""
  dev = _dev(p, phat, r, v, dinv, scalars)
  _same('bicgstab_update_p', p, phat, r, v, dinv)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_bicgstab_update_p(
        _ptr(p), _ptr(phat), _ptr(r), _ptr(v), _ptr(dinv), p.numel(),
        _ptr(scalars), _dtype_code(p), _stream(dev)),
        'sfem_bicgstab_update_p')


def bicgstab_update_s(s, shat, r, v, dinv, scalars):
  """s = r - alpha v; shat = dinv s; s . s into the scalars."""
  dev = _dev(s, shat, r, v, dinv, scalars)
  _same('bicgstab_update_s', s, shat, r, v, dinv)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_bicgstab_update_s(
        _ptr(s), _ptr(shat), _ptr(r), _ptr(v), _ptr(dinv), s.numel(),
        _ptr(scalars), _dtype_code(s), _stream(dev)),
        'sfem_bicgstab_update_s')


def bicgstab_update_xr(x, r, phat, shat, s, t, r0, scalars):
  """x += alpha phat + omega shat; r = s - omega t; r . r and r0 . r."""
  dev = _dev(x, r, phat, shat, s, t, r0, scalars)
  _same('bicgstab_update_xr', x, r, phat, shat, s, t, r0)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_bicgstab_update_xr(
        _ptr(x), _ptr(r), _ptr(phat), _ptr(shat), _ptr(s), _ptr(t), _ptr(r0),
        x.numel(), _ptr(scalars), _dtype_code(x), _stream(dev)),
        'sfem_bicgstab_update_xr')


# ------------------------------------------------------------------- Jacobi
def helmholtz_diag(parts, num_elements, ndim, P, dtil, weights, nodes,
                   bmat=None, want_mass=True, want_stiff=True, dtype=None,
                   device=None):
  """Element diagonals (E, P^d) of the mass and stiffness parts of the fused
  operator described by `parts` (`sfem_helmholtz_diag`): `dtil` (Q, P) the
  derivative of the nodal basis at the quadrature points, `weights`, `nodes`
  (Q,) the quadrature rule, `bmat` (Q, P) the interpolation (None:
  collocated).  Host arrays; returns (mass or None, stiffness or None)."""
  n = P ** ndim
  dev = torch.device(device)
  mk = lambda a: None if a is None else torch.as_tensor(
      np.ascontiguousarray(a), dtype=dtype, device=dev)
  dt_d, w_d, x_d, b_d = mk(dtil), mk(weights), mk(nodes), mk(bmat)
  Q = P if bmat is None else int(np.asarray(bmat).shape[0])
  mass = (torch.zeros((num_elements, n), dtype=dtype, device=dev)
          if want_mass else None)
  stiff = (torch.zeros((num_elements, n), dtype=dtype, device=dev)
           if want_stiff else None)
  with torch.cuda.device(dev):
    for part in parts:
      _dev(part.get('geo'), part.get('geo_elem'), part.get('elem_list'),
           part.get('geo_index'), dt_d)
      args = _lib.DiagArgs(
          mass_out=_ptr(mass), stiff_out=_ptr(stiff), **_launch_fields(part),
          bmat=_ptr(b_d), dtil=_ptr(dt_d), weights=_ptr(w_d), nodes=_ptr(x_d),
          num_elements=num_elements, ndim=ndim, P=P, Q=Q, dtype=_DT[dtype],
          kappa=_ptr(part.get('kappa')), sigma=_ptr(part.get('sigma')),
          coef_mode=int(part.get('coef_mode', _lib.COEF_NONE)))
      _lib.check(_lib.load().sfem_helmholtz_diag(ctypes.byref(args),
                                                 _stream(dev)),
                 'sfem_helmholtz_diag')
  return mass, stiff


def cg_update_r_jacobi(r, ap_ext, dinv, scalars, ncomp=1, layers=(),
                       masks=None, rz_partials=None):
  """r -= alpha Ap (assembled from its `layers`, if any); r . (dinv r) into the
  striped slots of `scalars`, or as stored per-workgroup sums in `rz_partials`
  (returns how many).  `r`, `ap_ext`: flat, `ncomp` components of
  `dinv.numel()` values each."""
  dev = _dev(r, ap_ext, dinv, scalars, rz_partials)
  ln, off, n = _layer_arrays(list(layers))
  mptr, moff = _mask_args(masks, n)
  count = ctypes.c_int64(0)
  if r.dtype != dinv.dtype:
    raise TypeError('cg_update_r_jacobi: r and dinv must share the dtype')
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_cg_update_r_jacobi(
        _ptr(r), _ptr(ap_ext), _ptr(dinv), dinv.numel(), int(ncomp), ln, off,
        n, mptr, moff, _ptr(scalars), _ptr(rz_partials),
        0 if rz_partials is None else rz_partials.numel(),
        ctypes.byref(count), _dtype_code(r), _stream(dev)),
        'sfem_cg_update_r_jacobi')
  return count.value


def cg_update_xp_jacobi(x, p, r, dinv, scalars, ncomp=1):
  """x += alpha p;  p = dinv r + beta p  (flat, `ncomp` components)."""
  dev = _dev(x, p, r, dinv, scalars)
  if r.dtype != dinv.dtype:
    raise TypeError('cg_update_xp_jacobi: r and dinv must share the dtype')
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_cg_update_xp_jacobi(
        _ptr(x), _ptr(p), _ptr(r), _ptr(dinv), dinv.numel(), int(ncomp),
        _ptr(scalars), _dtype_code(r), _stream(dev)),
        'sfem_cg_update_xp_jacobi')


# ------------------------------------------------------------- p-multigrid
def pmg_prolong(uc, uf, cidx, fidx, owner, mat, ndim, pc, pf, add=False):
  """uf = P uc (add: uf += P uc), see `sfem_pmg_prolong`; in place."""
  dev = _dev(uc, uf, cidx, fidx, owner, mat)
  if uc.dtype != uf.dtype or mat.dtype != uf.dtype:
    raise ValueError('pmg_prolong: one dtype for uc, uf and mat')
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_pmg_prolong(
        _ptr(uc), _ptr(uf), _ptr(cidx), _ptr(fidx), _ptr(owner), _ptr(mat),
        cidx.shape[0], int(ndim), int(pc), int(pf), int(bool(add)),
        _dtype_code(uf), _stream(dev)), 'sfem_pmg_prolong')
  return uf


def pmg_restrict(rf, rc_local, cidx, fidx, owner, mat, ndim, pc, pf):
  """rc_local (E, pc^ndim) = element-local P^T rf, see `sfem_pmg_restrict`."""
  dev = _dev(rf, rc_local, cidx, fidx, owner, mat)
  if rf.dtype != rc_local.dtype or mat.dtype != rf.dtype:
    raise ValueError('pmg_restrict: one dtype for rf, rc_local and mat')
  if rc_local.numel() != cidx.numel():
    raise ValueError('pmg_restrict: rc_local must match the coarse index rows')
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_pmg_restrict(
        _ptr(rf), _ptr(rc_local), _ptr(cidx), _ptr(fidx), _ptr(owner),
        _ptr(mat), cidx.shape[0], int(ndim), int(pc), int(pf),
        _dtype_code(rf), _stream(dev)), 'sfem_pmg_restrict')
  return rc_local


def _pmg_vec_check(who, coarse, fine, cidx, fidx, owner, cfix, ffix, mat, ndim,
                   pc, pf):
  """Shapes and dtypes of a vector transfer: `coarse` (N_c ndim,), `fine`
  (N_f ndim,) flat nodal vectors."""
  ndim, pc, pf = int(ndim), int(pc), int(pf)
  if coarse.dtype != fine.dtype or mat.dtype != fine.dtype:
    raise ValueError(f'{who}: one dtype for the two vectors and mat')
  if cidx.dtype != torch.int32 or fidx.dtype != torch.int32:
    raise TypeError(f'{who}: int32 index rows')
  if cfix.dtype != torch.uint8 or ffix.dtype != torch.uint8:
    raise TypeError(f'{who}: uint8 flag bytes, one per node')
  if ndim in (2, 3) and 2 <= pc < pf:
    E = cidx.shape[0]
    if (tuple(cidx.shape) != (E, pc ** ndim) or
        tuple(fidx.shape) != (E, pf ** ndim) or
        owner.numel() != E * ((pf ** ndim + 31) // 32) or
        mat.numel() != pf * pc):
      raise ValueError(f'{who}: cidx (E, pc^d), fidx (E, pf^d), owner '
                       '(E, ceil(pf^d / 32)) and mat (pf, pc) expected')
  if (coarse.numel() != cfix.numel() * ndim or
      fine.numel() != ffix.numel() * ndim):
    raise ValueError(f'{who}: a vector of ndim values per node of its flag '
                     'bytes expected')


def pmg_prolong_vec(uc, uf, cidx, fidx, owner, cfix, ffix, mat, ndim, pc, pf,
                    add=False):
  """uf (N_f ndim,) = P uc (N_c ndim,) per component (add: uf += P uc), see
  `sfem_pmg_prolong_vec`; in place.  Plain int32 index rows; `cfix`, `ffix`:
  uint8 per node, bit c set iff component c is fixed."""
  dev = _dev(uc, uf, cidx, fidx, owner, cfix, ffix, mat)
  _pmg_vec_check('pmg_prolong_vec', uc, uf, cidx, fidx, owner, cfix, ffix, mat,
                 ndim, pc, pf)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_pmg_prolong_vec(
        _ptr(uc), _ptr(uf), _ptr(cidx), _ptr(fidx), _ptr(owner), _ptr(cfix),
        _ptr(ffix), _ptr(mat), cidx.shape[0], int(ndim), int(pc), int(pf),
        int(bool(add)), _dtype_code(uf), _stream(dev)), 'sfem_pmg_prolong_vec')
  return uf


def pmg_restrict_vec(rf, rc_local, cidx, fidx, owner, cfix, ffix, mat, ndim,
                     pc, pf):
  """rc_local (E, pc^ndim, ndim) = element-local P^T rf (N_f ndim,), see
  `sfem_pmg_restrict_vec`."""
  dev = _dev(rf, rc_local, cidx, fidx, owner, cfix, ffix, mat)
  if rc_local.dtype != rf.dtype:
    raise ValueError('pmg_restrict_vec: one dtype for rf and rc_local')
  if rc_local.numel() != cidx.numel() * int(ndim):
    raise ValueError('pmg_restrict_vec: rc_local must hold ndim values per '
                     'slot of the coarse index rows')
  # (the assembled coarse vector is `sfem_scatter_csr`'s: checked by size only)
  coarse = torch.empty(cfix.numel() * int(ndim), dtype=rf.dtype, device='meta')
  _pmg_vec_check('pmg_restrict_vec', coarse, rf, cidx, fidx, owner, cfix, ffix,
                 mat, ndim, pc, pf)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_pmg_restrict_vec(
        _ptr(rf), _ptr(rc_local), _ptr(cidx), _ptr(fidx), _ptr(owner),
        _ptr(cfix), _ptr(ffix), _ptr(mat), cidx.shape[0], int(ndim), int(pc),
        int(pf), _dtype_code(rf), _stream(dev)), 'sfem_pmg_restrict_vec')
  return rc_local


CHEB_GENERAL, CHEB_FIRST, CHEB_RESIDUAL, CHEB_RESTART = 0, 1, 2, 3


def cheb_step(x, d, ax, b, dinv, r, a, c, mode):
  """One fused Chebyshev-Jacobi step (`sfem_cheb_step`); in place."""
  vs = [t for t in (x, d, ax, b, dinv, r) if t is not None]
  dev = _dev(*vs)
  n = b.numel()
  if any(t.numel() != n or t.dtype != b.dtype for t in vs):
    raise ValueError('cheb_step: vectors of one size and dtype')
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_cheb_step(
        _ptr(x), _ptr(d), _ptr(ax), _ptr(b), _ptr(dinv), _ptr(r), float(a),
        float(c), n, int(mode), _dtype_code(b), _stream(dev)),
        'sfem_cheb_step')


def pmg_dot2(a, b, c, partials, groups):
  """partials[:groups] = stored sums of a.b, partials[groups:2 groups] of a.c
  (`sfem_pmg_dot2`)."""
  vs = [t for t in (a, b, c) if t is not None]
  dev = _dev(*vs, partials)
  if partials.dtype != torch.float64 or partials.numel() < 2 * groups:
    raise ValueError('pmg_dot2: partials must hold 2 * groups doubles')
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_pmg_dot2(
        _ptr(a), _ptr(b), _ptr(c), a.numel(), _ptr(partials), int(groups),
        _dtype_code(a), _stream(dev)), 'sfem_pmg_dot2')


def pmg_cg_scalars(scalars, phase, partials, n, maxiter, tol, atol):
  dev = _dev(scalars, partials)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_pmg_cg_scalars(
        _ptr(scalars), int(phase), _ptr(partials), int(n), float(maxiter),
        float(tol), float(atol), _stream(dev)), 'sfem_pmg_cg_scalars')


# ---------------------------------------------------------- boundary facets
def boundary_geom(coords, facets, bmat, dmat, weights):
  """(xq (F, Q^(d-1), d), wJ (F, Q^(d-1))) of the facets, see
  `sfem_boundary_geom`.  `facets` (F, (P+1)^(d-1)) int32 ids in [0, N)."""
  dev = _dev(coords, facets, bmat, dmat, weights)
  if any(t.dtype != coords.dtype for t in (bmat, dmat, weights)):
    raise ValueError('boundary_geom: one dtype for coords and the matrices')
  d = coords.shape[-1]
  q, p1 = bmat.shape
  F, nq = facets.shape[0], q ** (d - 1)
  if facets.dtype != torch.int32 or facets.shape[1] != p1 ** (d - 1):
    raise ValueError(f'boundary_geom: facets must be (F, {p1 ** (d - 1)}) '
                     'int32')
  xq = torch.empty((F, nq, d), dtype=coords.dtype, device=dev)
  wj = torch.empty((F, nq), dtype=coords.dtype, device=dev)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_boundary_geom(
        _ptr(coords), _ptr(facets), F, _ptr(bmat), _ptr(dmat), _ptr(weights),
        d, p1, q, _ptr(xq), _ptr(wj), _dtype_code(coords), _stream(dev)),
        'sfem_boundary_geom')
  return xq, wj


def boundary_covector(g, nodal, facets, wj, bmat, ndim):
  """Facet-local (B (x) B)^T (wJ g), (F, (P+1)^(d-1)); g nodal (N,) when
  `nodal`, else (F, Q^(d-1)) at the points (`sfem_boundary_covector`)."""
  g = g.contiguous()
  dev = _dev(g, facets, wj, bmat)
  if wj.dtype != g.dtype or bmat.dtype != g.dtype:
    raise ValueError('boundary_covector: one dtype for g, wJ and B')
  q, p1 = bmat.shape
  F = facets.shape[0]
  if (facets.dtype != torch.int32 or
      tuple(facets.shape) != (F, p1 ** (ndim - 1))):
    raise ValueError(f'boundary_covector: facets must be (F, '
                     f'{p1 ** (ndim - 1)}) int32')
  if tuple(wj.shape) != (F, q ** (ndim - 1)):
    raise ValueError('boundary_covector: wJ does not match the facets')
  if not nodal and tuple(g.shape) != tuple(wj.shape):
    raise ValueError(f'boundary_covector: point values must be '
                     f'{tuple(wj.shape)}, got {tuple(g.shape)}')
  out = torch.empty((F, p1 ** (ndim - 1)), dtype=g.dtype, device=dev)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_boundary_covector(
        _ptr(g), int(bool(nodal)), _ptr(facets), F, _ptr(wj), _ptr(bmat),
        int(ndim), p1, q, _ptr(out), _dtype_code(g), _stream(dev)),
        'sfem_boundary_covector')
  return out


def boundary_mass(u, facets, aw, bmat, ndim, scale=1.0, diag=False, out=None):
  """Facet-local scale (B (x) B)^T (aw (B (x) B) u_f), (F, (P+1)^(d-1)), or
  with `diag` the facet-local diagonal of that operator (u unread).  Slots of
  `facets` stored as ~id read 0 and write 0 (`sfem_boundary_mass_apply`,
  `sfem_boundary_mass_diag`)."""
  dev = _dev(facets, aw, bmat)
  if bmat.dtype != aw.dtype or (not diag and u.dtype != aw.dtype):
    raise ValueError('boundary_mass: one dtype for u, aw and B')
  q, p1 = bmat.shape
  F = facets.shape[0]
  if (facets.dtype != torch.int32 or
      tuple(facets.shape) != (F, p1 ** (ndim - 1))):
    raise ValueError(f'boundary_mass: facets must be (F, {p1 ** (ndim - 1)}) '
                     'int32')
  if tuple(aw.shape) != (F, q ** (ndim - 1)):
    raise ValueError('boundary_mass: aw does not match the facets')
  shape = (F, p1 ** (ndim - 1))
  if out is None:
    out = torch.empty(shape, dtype=aw.dtype, device=dev)
  elif (tuple(out.shape) != shape or out.dtype != aw.dtype or
        not out.is_contiguous()):
    raise ValueError(f'boundary_mass: `out` must be a dense {shape} tensor')
  with torch.cuda.device(dev):
    if diag:
      _lib.check(_lib.load().sfem_boundary_mass_diag(
          _ptr(facets), F, _ptr(aw), _ptr(bmat), int(ndim), p1, q,
          float(scale), _ptr(out), _dtype_code(aw), _stream(dev)),
          'sfem_boundary_mass_diag')
    else:
      if not u.is_contiguous() or u.dim() != 1:
        raise ValueError('boundary_mass: u must be a dense (N,) vector')
      _lib.check(_lib.load().sfem_boundary_mass_apply(
          _ptr(u), _ptr(facets), F, _ptr(aw), _ptr(bmat), int(ndim), p1, q,
          float(scale), _ptr(out), _dtype_code(aw), _stream(dev)),
          'sfem_boundary_mass_apply')
  return out


def boundary_add_rows(local, rows, offsets, slots, out):
  """out[rows[r]] += sum of local[slots[offsets[r]:offsets[r+1]]] in slot
  order, in place; other entries of `out` untouched
  (`sfem_boundary_add_rows`)."""
  dev = _dev(local, rows, offsets, slots, out)
  if (local.dtype != out.dtype or not local.is_contiguous() or
      not out.is_contiguous() or out.dim() != 1):
    raise ValueError('boundary_add_rows: dense values and an (N,) `out` of '
                     'one dtype')
  if (rows.dtype != torch.int32 or slots.dtype != torch.int32 or
      offsets.dtype != torch.int64 or offsets.numel() != rows.numel() + 1):
    raise ValueError('boundary_add_rows: rows / slots int32, offsets int64 '
                     '(rows + 1)')
  with torch.cuda.device(dev):
    _lib.check(_lib.load().sfem_boundary_add_rows(
        _ptr(local), _ptr(rows), _ptr(offsets), _ptr(slots), rows.numel(),
        _ptr(out), _dtype_code(out), _stream(dev)), 'sfem_boundary_add_rows')
  return out
