// Dataset state normalisation of a device replay (rle_replay_state_stats, rle_replay_normalize_states): the
// column-statistics and transform kernels and their launchers.  A translation unit of its own: the kernels get a
// code object of their own, and the step programs' code object (kernels.hip) holds the kernels it held.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ops.h"

namespace rle {

// Dataset state normalisation (ops.h ReplayStatArgs / ReplayNormArgs).  Every load and store is one 16-byte
// vector per thread, the active threads of a workgroup covering one contiguous run of rpi ring rows.
__global__ __launch_bounds__(kThreads) void rle_replay_colsum(const ReplayStatArgs a) {
  __shared__ double red[kThreads * 4];
  const int c4 = a.Sp >> 2, rpi = stat_rpi(a.Sp), tid = (int)threadIdx.x;
  const int cv = tid % c4, rl = tid / c4;
  const long long r0 = (long long)blockIdx.x * a.rows_wg, r1 = min(a.size, r0 + a.rows_wg);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  if (rl < rpi) {
    double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
    if (a.center) c0 = a.center[4 * cv], c1 = a.center[4 * cv + 1], c2 = a.center[4 * cv + 2], c3 = a.center[4 * cv + 3];
    const float4* x = reinterpret_cast<const float4*>(a.x);
    for (long long r = r0 + rl; r < r1; r += rpi) {
      const float4 v = x[r * c4 + cv];
      if (a.center) {
        const double d0 = (double)v.x - c0, d1 = (double)v.y - c1, d2 = (double)v.z - c2, d3 = (double)v.w - c3;
        s0 += d0 * d0, s1 += d1 * d1, s2 += d2 * d2, s3 += d3 * d3;
      } else {
        s0 += (double)v.x, s1 += (double)v.y, s2 += (double)v.z, s3 += (double)v.w;
      }
    }
  }
  red[tid * 4 + 0] = s0, red[tid * 4 + 1] = s1, red[tid * 4 + 2] = s2, red[tid * 4 + 3] = s3;
  __syncthreads();
  if (tid < c4) {  // the rpi row lanes of this column vector, in ascending order
    double t0 = red[tid * 4], t1 = red[tid * 4 + 1], t2 = red[tid * 4 + 2], t3 = red[tid * 4 + 3];
    for (int l = 1; l < rpi; ++l) {
      const int o = (l * c4 + tid) * 4;
      t0 += red[o], t1 += red[o + 1], t2 += red[o + 2], t3 += red[o + 3];
    }
    double* p = a.part + (long long)blockIdx.x * a.Sp + 4 * tid;
    p[0] = t0, p[1] = t1, p[2] = t2, p[3] = t3;
  }
}
__global__ __launch_bounds__(kThreads) void rle_replay_colfin(const ReplayStatArgs a) {
  const int j = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (j >= a.Sp) return;
  double s = 0.0;
  for (int w = 0; w < a.nwg; ++w) s += a.part[(long long)w * a.Sp + j];
  s /= (double)a.size;
  if (a.sq) s = sqrt(s);
  a.out_d[j] = s;
  a.out_f[j] = (float)s;
}
__global__ __launch_bounds__(kThreads) void rle_replay_normalize(const ReplayNormArgs a) {
  const int c4 = a.Sp >> 2, rpi = stat_rpi(a.Sp), tid = (int)threadIdx.x;
  const int cv = tid % c4, rl = tid / c4;
  if (rl >= rpi) return;
  const int f = (int)blockIdx.x / a.nwg, w = (int)blockIdx.x - f * a.nwg;
  const long long r0 = (long long)w * a.rows_wg, r1 = min(a.size, r0 + a.rows_wg);
  const float4 sh = reinterpret_cast<const float4*>(a.shift)[cv], sc = reinterpret_cast<const float4*>(a.scale)[cv];
  float4* x = reinterpret_cast<float4*>(a.x[f]);
  for (long long r = r0 + rl; r < r1; r += rpi) {
    float4 v = x[r * c4 + cv];
    v.x = __fdiv_rn(__fsub_rn(v.x, sh.x), sc.x);
    v.y = __fdiv_rn(__fsub_rn(v.y, sh.y), sc.y);
    v.z = __fdiv_rn(__fsub_rn(v.z, sh.z), sc.z);
    v.w = __fdiv_rn(__fsub_rn(v.w, sh.w), sc.w);
    x[r * c4 + cv] = v;
  }
}
static bool stat_shape_ok(long long size, long long rows_wg, int Sp, int nwg) {
  return size > 0 && Sp >= 16 && Sp % 16 == 0 && Sp <= 4 * kThreads && rows_wg == stat_rows_wg(size, Sp) &&
         nwg == stat_nwg(size, Sp) && (long long)nwg * rows_wg >= size;
}
hipError_t launch_replay_colsum(const ReplayStatArgs& a, hipStream_t st) {
  if (!a.x || !a.part || !stat_shape_ok(a.size, a.rows_wg, a.Sp, a.nwg)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rle_replay_colsum, dim3((unsigned)a.nwg), dim3(kThreads), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_replay_colfin(const ReplayStatArgs& a, hipStream_t st) {
  if (!a.part || !a.out_d || !a.out_f || !stat_shape_ok(a.size, a.rows_wg, a.Sp, a.nwg)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rle_replay_colfin, dim3((unsigned)((a.Sp + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_replay_normalize(const ReplayNormArgs& a, hipStream_t st) {
  if (!a.x[0] || !a.x[1] || !a.shift || !a.scale || !stat_shape_ok(a.size, a.rows_wg, a.Sp, a.nwg))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(rle_replay_normalize, dim3((unsigned)(2 * a.nwg)), dim3(kThreads), 0, st, a);
  return hipGetLastError();
}

}  // namespace rle
