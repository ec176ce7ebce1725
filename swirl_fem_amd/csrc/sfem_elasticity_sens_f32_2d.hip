// Instantiations of the elasticity sensitivity kernel: float, 2D, P = 2..12.
#include "sfem_elasticity_sens.h"
namespace sfem {
SFEM_DEFINE_ELASTICITY_SENS_DISPATCH(float, 2)
}  // namespace sfem
