// Instantiations of the neo-Hookean sensitivity kernel: float, 3D,
// P = 2..12.
#include "sfem_hyperelastic_sens.h"
namespace sfem {
SFEM_DEFINE_HYPERELASTIC_SENS_DISPATCH(float, 3)
}  // namespace sfem
