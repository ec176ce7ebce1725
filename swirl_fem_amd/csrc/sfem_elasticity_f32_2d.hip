// Instantiations of the linear-elasticity kernel: float, 2D, P = 2..12.
#include "sfem_elasticity.h"
namespace sfem {
SFEM_DEFINE_ELASTICITY_DISPATCH(float, 2)
}  // namespace sfem
