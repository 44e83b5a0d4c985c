// Kernel instantiations: D3Q19, float.  Part 3: the two-step sweeps with separate producer and consumer waves
// (unit.inc, LT_PART).
#define LT_S lt::D3Q19
#define LT_T float
#define LT_TAG d3q19_f32
#define LT_HAS_KBC 0
#define LT_IS_3D 1
#define LT_PART 3
#include "unit.inc"
