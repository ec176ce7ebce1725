// Instantiations of the Helmholtz coefficient-sensitivity kernel: float, 2D,
// P = 2..12.
#include "sfem_helmholtz_sens.h"
namespace sfem {
SFEM_DEFINE_HELMHOLTZ_SENS_DISPATCH(float, 2)
}  // namespace sfem
