// Instantiations of the linear-elasticity kernel: float, 3D, P = 2..12.
#include "sfem_elasticity.h"
namespace sfem {
SFEM_DEFINE_ELASTICITY_DISPATCH(float, 3)
}  // namespace sfem
