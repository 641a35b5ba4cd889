// Floats as the host checks of the arithmetic headers read and print them (pose_host_check.cpp, recon_host_check.cpp,
// ransac_host_check.cpp): hexadecimal bit patterns, so that a text file carries every word exactly.
#pragma once
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

static inline bool rd_f32(FILE *f, float *v) {
  uint32_t u;
  if (fscanf(f, "%" SCNx32, &u) != 1) return false;
  memcpy(v, &u, 4);
  return true;
}

static inline void pr_f32(float v) {
  uint32_t u;
  memcpy(&u, &v, 4);
  printf(" %08" PRIx32, u);
}
