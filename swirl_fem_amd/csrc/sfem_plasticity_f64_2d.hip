// Instantiations of the J2 plasticity kernel, residual and tangent modes:
// double, 2D, P = 2..12.
#include "sfem_plasticity.h"
namespace sfem {
SFEM_DEFINE_PLASTICITY_DISPATCH(double, 2)
}  // namespace sfem
