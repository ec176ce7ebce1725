// Instantiations of the linear-elasticity kernel: double, 2D, P = 2..12.
#include "sfem_elasticity.h"
namespace sfem {
SFEM_DEFINE_ELASTICITY_DISPATCH(double, 2)
}  // namespace sfem
