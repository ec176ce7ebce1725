// Instantiations of the variable-coefficient Helmholtz kernel: float, 2D,
// P = 2..12.
#include "sfem_helmholtz.h"
namespace sfem {
SFEM_DEFINE_HELMHOLTZ_COEF_DISPATCH(float, 2)
}  // namespace sfem
