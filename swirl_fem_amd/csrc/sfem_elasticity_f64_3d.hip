// Instantiations of the linear-elasticity kernel: double, 3D, P = 2..12.
#include "sfem_elasticity.h"
namespace sfem {
SFEM_DEFINE_ELASTICITY_DISPATCH(double, 3)
}  // namespace sfem
