// The 64 x 64 tile of a product X Y^T on the f64 matrix cores (v_mfma_f64_16x16x4_f64) that fid.hip, featsets.hip and fidinf.hip share:
// the enumeration of the block upper triangle and the step from an LDS operand stage to the accumulators.  What differs between the
// three -- where the operands come from -- stays with each of them.
//
// The f64 MFMA's C/D lane map is NOT the f32 one: col = lane & 15, row = (lane >> 4) + 4 * reg (the f32 16x16 forms have
// row = 4 * (lane >> 4) + reg).  A and B are one f64 per lane: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15].
#pragma once
#include "common.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int SG_F64_FT = 64;                // tile of the product per workgroup of 256 threads: four waves, 2 x 2, each 32 x 32 = 2 x 2 MFMA tiles
constexpr int SG_F64_KB = 32;                // k staged per pass of a row-major stage
constexpr int SG_F64_LDK = SG_F64_KB + 2;    // its LDS row stride in doubles: the 32 lanes of a half wave (16 rows x 2 k) read 32 distinct bank pairs

// tile pair (ti <= tj) number b of the block upper triangle of an nt x nt grid, row by row (wave-uniform scalar loop)
__device__ __forceinline__ void sg_f64_tile_pair(int b, int nt, int& ti, int& tj) {
  int i = 0, len = nt;
  while (b >= len) { b -= len; ++i; --len; }
  ti = i; tj = i + b;
}

__device__ __forceinline__ void sg_f64_tile_zero(f64x4 (&acc)[2][2]) {
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) acc[m][n] = f64x4{0.0, 0.0, 0.0, 0.0};
}

// acc[m][n] += sum_{k < kp} A[i][k] B[j][k] from a row-major stage: ab[i * SG_F64_LDK + k] is row i of the A side, from
// SG_F64_FT * SG_F64_LDK on the B side; kp a multiple of 4, k ascending.  Element reg of acc[m][n] is row
// (wave >> 1) * 32 + m * 16 + (lane >> 4) + 4 * reg, column (wave & 1) * 32 + n * 16 + (lane & 15) of the tile.
__device__ __forceinline__ void sg_f64_tile_mma(const double* ab, int kp, f64x4 (&acc)[2][2]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wi = wave >> 1, wj = wave & 1, fr = lane & 15, fk = lane >> 4;
  for (int ks = 0; ks < kp; ks += 4) {
    double a[2], b[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) a[m] = ab[(wi * 32 + m * 16 + fr) * SG_F64_LDK + ks + fk];
#pragma unroll
    for (int n = 0; n < 2; ++n) b[n] = ab[(SG_F64_FT + wj * 32 + n * 16 + fr) * SG_F64_LDK + ks + fk];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], b[n], acc[m][n], 0, 0, 0);
  }
}

// the butterfly sum of a wave: every lane gets the same value, in an order that depends on nothing but the lane numbers
__device__ __forceinline__ double sg_wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
