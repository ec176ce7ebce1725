// Instantiations of the J2 plasticity kernel, residual and tangent modes:
// float, 3D, P = 2..12.
#include "sfem_plasticity.h"
namespace sfem {
SFEM_DEFINE_PLASTICITY_DISPATCH(float, 3)
}  // namespace sfem
