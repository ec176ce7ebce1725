// Instantiations of the plasticity VJP kernel, displacement and state modes:
// double, 2D, P = 2..12.
#include "sfem_plasticity_vjp.h"
namespace sfem {
SFEM_DEFINE_PLASTICITY_VJP_DISPATCH(double, 2)
}  // namespace sfem
