// Vector types of the bf16 matrix-core conv kernel (conv_bf16x6.hip): the MFMA accumulator and the 16-byte operand unit.
#pragma once
#include "kernels.hpp"

namespace mn {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

}  // namespace mn
