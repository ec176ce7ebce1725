"""Host logic of layered assembly (`operators.build_layer_plan`) under other
node numberings (`tests/numbering_cases.py`).

The facet-table builder accepts any element whose 27 facets are affine maps
of node ids, so a lexicographic or reversed global numbering reaches layered
assembly as well.  There a facet's nodes span far more than one
`SFEM_LAYER_CHUNK`, and the chunk masks that let `r -= alpha Ap` skip the
chunks of a layer nobody writes must still cover every slot a writer stores
(a chunk left unmarked drops live contributions from CG's residual).  The
facet table is restated here in NumPy from the index rows (the inverse of
`table_ids` in tests/test_gpu_facet.py), chains come from
`operators.facet_chains` on CPU tensors.  No GPU needed.
"""
import numpy as np
import pytest
import torch

from swirl_fem_amd import _lib
from swirl_fem_amd.core import operators
from tests import numbering_cases as NC

CHUNK = _lib.SFEM_LAYER_CHUNK


def host_facet_table(elements, P):
  """(E, 27, 4) int32 table of `sfem_facet_table_build` without flag bits,
  and the (E,) mask of the elements it describes exactly."""
  el = np.asarray(elements, np.int64).reshape(-1, P, P, P)
  E = el.shape[0]
  tab = np.zeros((E, 27, 4), dtype=np.int64)
  ok = np.ones(E, dtype=bool)
  rng = lambda c: [0] if c == 0 else ([P - 1] if c == 2 else range(1, P - 1))
  for f in range(27):
    c = (f // 9, (f // 3) % 3, f % 3)
    o = [0 if k == 0 else (1 if k == 1 else P - 1) for k in c]
    id0 = el[:, o[0], o[1], o[2]]
    s = np.zeros((E, 3), dtype=np.int64)
    for d in range(3):
      if c[d] == 1:
        q = list(o)
        q[d] += 1
        s[:, d] = el[:, q[0], q[1], q[2]] - id0
    tab[:, f, 0], tab[:, f, 1:] = id0, s
    for a in rng(c[0]):
      for i in rng(c[1]):
        for j in rng(c[2]):
          pred = id0 + s[:, 0] * (a - o[0]) + s[:, 1] * (i - o[1]) + s[:, 2] * (
              j - o[2])
          ok &= el[:, a, i, j] == pred
  ok &= (np.abs(tab[..., 1:]) <= 0x7FFFFF).all(axis=(1, 2))
  return tab.astype(np.int32), ok


def host_facet_parts(elements, P, chains):
  """What `_facet_parts` launches (one geometry kind): the table elements in
  one part (with chains, segments of 3), the others on index rows."""
  tab, ok = host_facet_table(elements, P)
  if not ok.any():
    return None
  el = torch.as_tensor(np.asarray(elements))
  good = torch.as_tensor(np.nonzero(ok)[0])
  part = {'geo_mode': operators._GEO_AFFINE, 'facet_table': torch.as_tensor(tab)}
  if good.numel() < el.shape[0]:
    part['elem_list'] = good.to(torch.int32)
  if chains:
    part['chains'] = operators.facet_chains(el, good, P, 3)
  parts = [part]
  bad = np.nonzero(~ok)[0]
  if bad.size:
    parts.append({'geo_mode': operators._GEO_AFFINE,
                  'elem_list': torch.as_tensor(bad).to(torch.int32)})
  return parts


def writers(parts, E):
  """(E, 27) bool: the (element, facet) pairs that store their facet (all but
  the last face, with its edges and vertices, of an element that hands it on
  to its successor in a chain segment)."""
  w = np.ones((E, 27), dtype=bool)
  for q in parts:
    if 'chains' in q:
      off, elems = (t.numpy() for t in q['chains'])
      succ = np.ones(elems.size, dtype=bool)
      succ[off[1:] - 1] = False
      w[elems[succ], 18:] = False
  return w


def decode(plan, E):
  """Per (element, facet): (layer, slot of its first node in that layer)."""
  tab2 = plan.parts[0]['layered_table'].numpy().astype(np.int64)
  pos = tab2[..., 1] & 0x3FFFFFFF
  layer = np.zeros((E, 27), dtype=np.int64)
  first = pos.copy()
  for k, (ln, off) in enumerate(plan.layers, start=1):
    inside = pos >= off
    layer[inside] = k
    first[inside] = pos[inside] - off
  return layer, first


def slots(tab, P, f):
  """(E, m) node ids of facet f of every element, from the host table."""
  c = (f // 9, (f // 3) % 3, f % 3)
  t = np.arange(P - 2)
  grids = np.meshgrid(*[t if k == 1 else np.zeros(1, np.int64) for k in c],
                      indexing='ij')
  off = sum(tab[:, f, 1 + d, None].astype(np.int64) * grids[d].reshape(1, -1)
            for d in range(3))
  return tab[:, f, 0, None].astype(np.int64) + off


def layer_masks(plan):
  data, offs = plan.masks
  data = data.numpy()
  return [data[o:o + (ln + CHUNK - 1) // CHUNK]
          for (ln, _), o in zip(plan.layers, offs)]


def two_end_masks(plan, tab, wr, layer, P):
  """The chunk marking before numbering-independent masks: the chunks of
  each writer's smallest and largest node only."""
  out = []
  for k, (ln, _) in enumerate(plan.layers, start=1):
    m = np.zeros((ln + CHUNK - 1) // CHUNK, dtype=np.uint8)
    for f in range(27):
      sel = wr[:, f] & (layer[:, f] == k)
      s = slots(tab[sel], P, f)
      if s.size:
        m[s.min(axis=1) // CHUNK] = 1
        m[s.max(axis=1) // CHUNK] = 1
    out.append(m)
  return out


CASES = [(num, n, P) for num in ('refiner', 'lexicographic',
                                 'lexicographic_yzx', 'reversed',
                                 'reversed_lexicographic', 'random',
                                 'half_random')
         for n, P in ((4, 6), (4, 8), (3, 12))] + [
             ('far_stride', 0, P) for P in (6, 8, 12)]


@pytest.mark.parametrize('chains', [True, False], ids=['chains', 'nochain'])
@pytest.mark.parametrize('numbering,n,P', CASES,
                         ids=[f'{c[0]}-p{c[2]}' for c in CASES])
def test_layer_plan_covers_every_slot(numbering, n, P, chains, monkeypatch):
  if not chains:
    monkeypatch.setenv('SFEM_CHAIN', '0')
  case = NC.build(numbering, 'thin' if numbering == 'far_stride' else
                  'affine', n, P)
  el = case.rp.elements
  E, N = el.shape[0], case.rp.node_coords.shape[0]
  parts = host_facet_parts(el, P, chains)
  facet, layered = NC.EXPECT[NC.kind(numbering)]
  if facet == 'none':
    assert parts is None
  else:
    have = 'elem_list' in parts[0]
    assert have == (facet == 'some'), numbering
    if chains:
      off = parts[0]['chains'][0]
      assert int(off.numel()) - 1 < E, 'no element was chained'
  plan = (None if parts is None else
          operators.build_layer_plan(parts, E, N, P))
  assert (plan is not None) == layered, numbering
  if plan is None:
    return
  tab = parts[0]['facet_table'].numpy()
  if NC.kind(numbering) == 'reversed':      # every stride negative
    inner = tab[..., 1:][tab[..., 1:] != 0]
    assert inner.size and (inner < 0).all()
  if numbering == 'reversed':               # the most shared nodes last
    assert plan.layers[0][0] > N // 2
  wr = writers(parts, E)
  layer, first = decode(plan, E)
  masks = layer_masks(plan)
  lens = [ln for ln, _ in plan.layers]
  taken = [np.zeros(ln, dtype=np.int64) for ln in [N] + lens]
  for f in range(27):
    s = slots(tab, P, f)                                   # (E, m) node ids
    # the layered table addresses the same nodes as the facet table
    assert np.array_equal(first[:, f], tab[:, f, 0])
    for k in range(len(lens) + 1):
      sel = wr[:, f] & (layer[:, f] == k)
      if not sel.any():
        continue
      ids = s[sel].reshape(-1)
      assert ids.min() >= 0 and ids.max() < len(taken[k]), (numbering, k, f)
      np.add.at(taken[k], ids, 1)
      if k:
        unmarked = masks[k - 1][ids // CHUNK] == 0
        assert not unmarked.any(), (
            f'{numbering}: layer {k} facet {f}: {int(unmarked.sum())} slots '
            'in chunks the masks skip')
  for k, t in enumerate(taken):
    assert t.max() <= 1, f'{numbering}: a slot of layer {k} has two writers'
  # every node: one slot per element row that holds it, except the rows
  # that hand their last face on to a chain successor
  per_node = sum(np.pad(t, (0, max(0, N - len(t))))[:N] for t in taken)
  rows = np.asarray(el, np.int64).reshape(E, P, P, P)
  holders = np.bincount(rows.reshape(-1), minlength=N)
  carried = ~wr[:, 18]
  holders -= np.bincount(rows[carried, -1].reshape(-1), minlength=N)
  assert np.array_equal(per_node, holders)
  need = sum(min(CHUNK, ln - c * CHUNK) for m, ln in zip(masks, lens)
             for c in np.nonzero(m)[0])
  assert plan.read >= need
  if numbering == 'refiner':
    old = two_end_masks(plan, tab, wr, layer, P)
    assert all(np.array_equal(a, b) for a, b in zip(masks, old))
