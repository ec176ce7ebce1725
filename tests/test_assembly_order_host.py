"""Launch order of coloured assembly (`operators.colored_launch_order`) on the
host: every node's first toucher (its plain store) must run before every
other element that adds to it.  The geometry groups come from the NumPy
restatement of `classify_geometry` (`tests/geometry_cases.py`); no kernel
runs."""
import numpy as np
import pytest
import torch

from swirl_fem_amd.core.operators import (colored_launch_order,
                                          first_toucher_violations)
from tests import geometry_cases as G


def _groups(case, mesh):
  """(group (E,) int64, number of groups) in `HelmholtzOperator.create`'s
  part order: affine, multilinear, curved."""
  el = mesh.elements.numpy()
  kinds = G.numpy_kinds(case.rp.node_coords, el, mesh.ndim,
                        mesh.gridpoints_1d.num_points)
  present = [k for k in (G.AFFINE, G.MULTILINEAR) if (kinds == k).any()]
  group = np.full(len(kinds), -1, np.int64)
  for g, k in enumerate(present):
    group[kinds == k] = g
  return torch.as_tensor(group), len(present)


def _group_major(colors, num_colors, group, num_groups):
  """The order coloured assembly used before: geometry group, then colour."""
  out = []
  for g in range(num_groups):
    for c in range(num_colors):
      lst = torch.nonzero((group == g) & (colors == c)).reshape(-1)
      if lst.numel():
        out.append((g, lst))
  return out


@pytest.mark.parametrize('name,P', [('block_jitter', 5), ('block_jitter', 9),
                                    ('scrambled', 5), ('padded', 4)])
def test_colour_major_order_stores_first(name, P):
  if name == 'padded':
    case = G.vertex(3, 3, P)
    case.pad = 3
  else:
    case = G.block_jitter(4, 3, P, scramble=name == 'scrambled')
  mesh, _, _ = case.finalize('cpu', torch.float64)
  colors, num_colors, first = mesh.assembly_plan().coloring()
  group, ng = _groups(case, mesh)
  assert ng == 2, 'the case must mix affine and multilinear elements'
  if case.pad:
    assert (group[-case.pad:] == -1).all()
  launches = colored_launch_order(colors, num_colors, group, ng)
  # every real element in exactly one launch, colours non-decreasing, and a
  # launch holds one colour and one group
  ids = torch.cat([lst for _, lst in launches])
  real = (mesh.elements >= 0).any(dim=1)
  assert torch.equal(ids.sort().values, torch.nonzero(real).reshape(-1))
  cols = [int(colors[lst].unique().item()) for _, lst in launches]
  assert cols == sorted(cols)
  for g, lst in launches:
    assert bool((group[lst] == g).all())
  assert first_toucher_violations(mesh.elements, first, launches) == 0
  # ... which the group-major order broke on this mesh
  old = _group_major(colors, num_colors, group, ng)
  assert first_toucher_violations(mesh.elements, first, old) > 0


def test_violations_counted_on_a_hand_made_mesh():
  """Two 1D-like 'elements' sharing node 1: the slot of element 1 is not the
  first toucher, so element 1 must launch after element 0."""
  el = torch.tensor([[0, 1], [1, 2]])
  first = torch.tensor([[True, True], [False, True]])
  a = (0, torch.tensor([0]))
  b = (1, torch.tensor([1]))
  assert first_toucher_violations(el, first, [a, b]) == 0
  assert first_toucher_violations(el, first, [b, a]) == 1
  with pytest.raises(RuntimeError, match='no launch'):
    first_toucher_violations(el, first, [a])
