// Instantiations of the elasticity stress kernel and of its vector-Jacobian
// product: float, 3D, P = 2..12.
#include "sfem_elasticity_stress.h"
namespace sfem {
SFEM_DEFINE_ELASTICITY_STRESS_DISPATCH(float, 3)
}  // namespace sfem
