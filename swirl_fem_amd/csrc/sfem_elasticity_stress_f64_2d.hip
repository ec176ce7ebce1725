// Instantiations of the elasticity stress kernel and of its vector-Jacobian
// product: double, 2D, P = 2..12.
#include "sfem_elasticity_stress.h"
namespace sfem {
SFEM_DEFINE_ELASTICITY_STRESS_DISPATCH(double, 2)
}  // namespace sfem
