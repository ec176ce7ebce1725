// Instantiations of the neo-Hookean kernel, residual and tangent modes:
// double, 2D, P = 2..12.
#include "sfem_hyperelastic.h"
namespace sfem {
SFEM_DEFINE_HYPERELASTIC_DISPATCH(double, 2)
}  // namespace sfem
