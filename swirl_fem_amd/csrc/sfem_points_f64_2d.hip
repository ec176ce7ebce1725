// Instantiations of the point evaluation kernels and their transposes:
// double, 2D, P1 = 2..12.
#include "sfem_points.h"
namespace sfem {
SFEM_DEFINE_POINT_DISPATCH(double, 2)
}  // namespace sfem
