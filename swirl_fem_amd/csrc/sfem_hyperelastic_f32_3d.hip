// Instantiations of the neo-Hookean kernel, residual and tangent modes:
// float, 3D, P = 2..12.
#include "sfem_hyperelastic.h"
namespace sfem {
SFEM_DEFINE_HYPERELASTIC_DISPATCH(float, 3)
}  // namespace sfem
