// Instantiations of the vector-Jacobian product of the scalar-transport
// right-hand side: float, 3D, P = 2..12.
#include "sfem_transport_vjp.h"
namespace sfem {
SFEM_DEFINE_TRANSPORT_VJP_DISPATCH(float, 3)
}  // namespace sfem
