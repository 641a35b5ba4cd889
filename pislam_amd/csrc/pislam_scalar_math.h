// pislam_scalar_math.h — the scalar common ground of the arithmetic headers (pislam_geom_math.h, pislam_recon_math.h,
// pislam_pose_math.h), stated ONCE for the device kernels and for a plain C++ compiler: how a count is read, the
// finiteness tests, the correctly rounded quotient and square root, the clamp of a Q8 level-0 coordinate.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PISLAM_HD __host__ __device__ __forceinline__
#define PISLAM_UNROLL _Pragma("unroll")
#else
#define PISLAM_HD inline
#define PISLAM_UNROLL
#endif

namespace psm {

constexpr uint32_t COUNT_INVALID = 0xffffffffu;              // == PISLAM_COUNT_INVALID
constexpr int32_t Q8_MAX = 1 << 20;

// A count as a batched call reads it: min(count, stride), COUNT_INVALID as 0.
PISLAM_HD uint32_t clamp_count(uint32_t count, size_t stride) {
  return count == COUNT_INVALID ? 0u : (count < stride ? count : (uint32_t)stride);
}

PISLAM_HD bool finite_f(float v) { return fabsf(v) < __builtin_inff(); }   // false for a NaN
PISLAM_HD bool finite_d(double v) { return fabs(v) < __builtin_inf(); }

// The correctly rounded binary32 square root and quotient.  (sqrtf and / are correctly rounded on the device with
// hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt; __fsqrt_rn is the NATIVE square root unless OCML's rounded
// operations are switched on, so it is not used.)
PISLAM_HD float fsqrt(float x) { return __builtin_sqrtf(x); }
PISLAM_HD float fdiv(float a, float b) { return a / b; }

// A Q8 level-0 coordinate as the two-view calls read it: clamped to +- 2^20 (4096 px) first.
PISLAM_HD int32_t clamp_q8(int32_t v) { return v < -Q8_MAX ? -Q8_MAX : (v > Q8_MAX ? Q8_MAX : v); }

}  // namespace psm
