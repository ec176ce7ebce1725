// Instantiations of the point evaluation kernels and their transposes:
// float, 2D, P1 = 2..12.
#include "sfem_points.h"
namespace sfem {
SFEM_DEFINE_POINT_DISPATCH(float, 2)
}  // namespace sfem
