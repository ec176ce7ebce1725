// Instantiations of the Helmholtz coefficient-sensitivity kernel: float, 3D,
// P = 2..12.
#include "sfem_helmholtz_sens.h"
namespace sfem {
SFEM_DEFINE_HELMHOLTZ_SENS_DISPATCH(float, 3)
}  // namespace sfem
