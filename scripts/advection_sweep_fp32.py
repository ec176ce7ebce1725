"""The float32-evaluated reference behind `FP32_EXCEPTIONS` of
tests/test_gpu_advection_sweep.py (CPU only): for the items named on the
command line, the diagonal reference of section d -- the same function, the
same float32-representable inputs, the same Dirichlet mask and operator
combinations -- carried in np.float32 (`oracle.sfem_oracle.FESpace(dtype=
np.float32)`), against its float64 self.  Prints the worst relative error per
item; profiles/advection_sweep_errors.md records them.

    python scripts/advection_sweep_fp32.py 2,12 3,12
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                '..'))
from oracle import sfem_oracle as O                      # noqa: E402
from tests import advection_reference as AR              # noqa: E402
from tests import test_gpu_advection_sweep as T          # noqa: E402


def main(items):
  for ndim, P in items:
    r = T.reference(ndim, P, torch.float32)
    rp, real = r['rp'], r['real']
    n = rp.elements.shape[1]
    mesh = rp.finalize(device='cpu', dtype=torch.float32)
    keep = 1.0 - mesh.physical_masks['boundary'].double().numpy()
    f32 = O.FESpace(rp.node_coords, rp.elements, (P, 'gll'), (P, 'gll'),
                    dtype=np.float32)
    diag = getattr(AR, r['diag_form'])
    cast = lambda v: None if v is None else v.astype(np.float32)
    worst = (0.0, None)
    for kf, cf in (('point', 'elem'), (None, None)):
      k = r['k'][kf]
      k = None if k is None else k[:real]
      c = r['c'][cf]
      c = None if c is None else np.repeat(c[:real, None], n, 1)
      for l0, l1 in T.LAMBDAS:
        ref = (l0 * r['dM'][cf] + l1 * r['dK'][kf] + r['dC']) * keep
        got = diag(f32, np.float32(l0), np.float32(l1), cast(k), cast(c),
                   cast(r['b'][:real]), keep.astype(np.float32))
        assert got.dtype == np.float32
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print('  %d %2d %-5s %-4s %.1f %.1f  %.3e' % (ndim, P, kf, cf, l0, l1,
                                                      err))
        worst = max(worst, (err, (kf, cf, l0, l1)))
    print('FP32REF %d %2d d %s %.3e %s' % ((ndim, P, r['diag_form']) + worst))


if __name__ == '__main__':
  main([tuple(int(v) for v in a.split(',')) for a in sys.argv[1:]]
       or [(2, 12), (3, 12)])
