// Instantiations of the neo-Hookean sensitivity kernel: float, 2D,
// P = 2..12.
#include "sfem_hyperelastic_sens.h"
namespace sfem {
SFEM_DEFINE_HYPERELASTIC_SENS_DISPATCH(float, 2)
}  // namespace sfem
