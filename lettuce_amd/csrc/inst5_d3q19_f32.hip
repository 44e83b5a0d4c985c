// Kernel instantiations: D3Q19, float.  Part 5: the kernels with a body force (unit.inc, LT_PART).
#define LT_S lt::D3Q19
#define LT_T float
#define LT_TAG d3q19_f32
#define LT_HAS_KBC 0
#define LT_IS_3D 1
#define LT_PART 5
#include "unit.inc"
