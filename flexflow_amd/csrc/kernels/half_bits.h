// half_bits.h -- fp16 values carried as their 16-bit patterns (the row
// kernels of norm.hip and sampling.hip).
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ffmi {

__device__ __forceinline__ float h2f_(uint16_t v) { return __half2float(__ushort_as_half(v)); }
__device__ __forceinline__ uint16_t f2h_(float v) { return __half_as_ushort(__float2half_rn(v)); }

}  // namespace ffmi
