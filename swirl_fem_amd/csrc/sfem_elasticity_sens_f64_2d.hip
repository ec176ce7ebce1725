// Instantiations of the elasticity sensitivity kernel: double, 2D, P = 2..12.
#include "sfem_elasticity_sens.h"
namespace sfem {
SFEM_DEFINE_ELASTICITY_SENS_DISPATCH(double, 2)
}  // namespace sfem
