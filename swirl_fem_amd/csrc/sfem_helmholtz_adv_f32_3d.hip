// Instantiations of the Helmholtz kernel with an advective term: float, 3D,
// P = 2..12.
#include "sfem_helmholtz_adv.h"
namespace sfem {
SFEM_DEFINE_HELMHOLTZ_ADV_DISPATCH(float, 3)
}  // namespace sfem
