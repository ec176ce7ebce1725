// Instantiations of the Helmholtz kernel with an advective term: double, 2D,
// P = 2..12.
#include "sfem_helmholtz_adv.h"
namespace sfem {
SFEM_DEFINE_HELMHOLTZ_ADV_DISPATCH(double, 2)
}  // namespace sfem
