// Instantiations of the scalar-transport right-hand side kernel: double, 3D,
// P = 2..12.
#include "sfem_transport.h"
namespace sfem {
SFEM_DEFINE_TRANSPORT_DISPATCH(double, 3)
}  // namespace sfem
