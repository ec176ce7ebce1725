"""Host-side logic of the Jacobi preconditioner (no GPU needed)."""
import pytest
import torch

from swirl_fem_amd import switches
from swirl_fem_amd.core import layout
from swirl_fem_amd.linalg.jacobi import JacobiPreconditioner


def test_inverse_diagonal_is_zero_on_dirichlet_rows_and_strict():
  d = torch.tensor([2.0, 0.0, 4.0, 8.0, 0.0], dtype=torch.float64)
  M = JacobiPreconditioner(d)
  assert M.jacobi_diagonal().tolist() == [4.0, 0.0, 2.0, 1.0, 0.0]
  loose = JacobiPreconditioner(d, strict=False)
  assert loose.jacobi_diagonal().tolist() == [0.5, 0.0, 0.25, 0.125, 0.0]
  # strict: r . M r >= r . r for residuals that vanish on the Dirichlet rows
  g = torch.Generator().manual_seed(0)
  for _ in range(10):
    r = torch.randn(5, dtype=torch.float64, generator=g) * (d != 0)
    assert float(torch.dot(r, M(r))) >= float(torch.dot(r, r))


def test_vector_fields_share_one_diagonal():
  d = torch.tensor([1.0, 2.0, 4.0], dtype=torch.float64)
  M = JacobiPreconditioner(d, strict=False)
  r = torch.arange(6, dtype=torch.float64).reshape(3, 2)
  want = r / d[:, None]
  assert torch.equal(M(r), want)
  rc = layout.component_major(r)
  z = M(rc)
  assert torch.equal(z, want) and z.stride() == rc.stride()


def test_rejects_bad_diagonals():
  with pytest.raises(ValueError):
    JacobiPreconditioner(torch.ones(3, 2, dtype=torch.float64))
  with pytest.raises(ValueError):
    JacobiPreconditioner(torch.tensor([1.0, -1.0], dtype=torch.float64))


def test_fused_jacobi_switch_is_registered():
  assert switches.SWITCHES['SFEM_FUSED_JACOBI'][0] == '1'


def test_vector_fields_of_different_width_keep_their_own_layout():
  d = torch.tensor([1.0, 2.0, 4.0], dtype=torch.float64)
  M = JacobiPreconditioner(d, strict=False)
  for nc in (2, 3, 2):
    r = layout.component_major(torch.ones(3, nc, dtype=torch.float64))
    assert torch.equal(M(r), (1.0 / d)[:, None].expand(3, nc))
