// Instantiations of the scalar-transport right-hand side kernel: double, 2D,
// P = 2..12.
#include "sfem_transport.h"
namespace sfem {
SFEM_DEFINE_TRANSPORT_DISPATCH(double, 2)
}  // namespace sfem
