// Instantiations and launcher of the matrix-core Helmholtz kernel (P = 12, fp32).
#include <stdlib.h>
#include <string.h>

#include "sfem_helmholtz_mfma.h"

namespace sfem {

int launch_helmholtz_mfma_p12(const HelmholtzParams<float>& prm,
                              hipStream_t stream) {
  constexpr int P = 12;
  if (int rc = check_groups("helmholtz (mfma)", prm.num_elements)) return rc;
  MfmaConsts<P> cst;
  memcpy(cst.d, prm.dmat_host, sizeof(cst.d));
  memcpy(cst.w, prm.weights_host, sizeof(cst.w));
  memcpy(cst.x, prm.nodes_host, sizeof(cst.x));
  const dim3 grid((unsigned)prm.num_elements), block(256);
  with_flag(prm.geo_mode == GEO_AFFINE, [&](auto affine) {
    with_flag(prm.lambda0 != 0.f, [&](auto mass) {
      constexpr int GM = decltype(affine)::value ? GEO_AFFINE : GEO_MULTILINEAR;
      hipLaunchKernelGGL(
          (helmholtz_mfma_p12_kernel<GM, decltype(mass)::value>), grid, block,
          0, stream, cst, prm);
    });
  });
  SFEM_LAUNCH_CHECK();
  return SFEM_OK;
}

}  // namespace sfem
