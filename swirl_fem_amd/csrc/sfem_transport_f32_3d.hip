// Instantiations of the scalar-transport right-hand side kernel: float, 3D,
// P = 2..12.
#include "sfem_transport.h"
namespace sfem {
SFEM_DEFINE_TRANSPORT_DISPATCH(float, 3)
}  // namespace sfem
