// Instantiations of the scalar-transport right-hand side kernel: float, 2D,
// P = 2..12.
#include "sfem_transport.h"
namespace sfem {
SFEM_DEFINE_TRANSPORT_DISPATCH(float, 2)
}  // namespace sfem
