// Instantiations of the point evaluation kernels and their transposes:
// float, 3D, P1 = 2..12.
#include "sfem_points.h"
namespace sfem {
SFEM_DEFINE_POINT_DISPATCH(float, 3)
}  // namespace sfem
