// Host-side declarations shared by every host source: the error type behind the C ABI's
// return codes and the launchers that kernels.hip and replay_norm.hip define.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "ops.h"
#include "rle.h"

namespace rle {

struct Error {
  int code;
  std::string msg;
};

#define HIPCHK(x)                                                                               \
  do {                                                                                          \
    hipError_t e_ = (x);                                                                        \
    if (e_ != hipSuccess) throw Error{RLE_EHIP, std::string(#x) + ": " + hipGetErrorString(e_)}; \
  } while (0)
#define REQUIRE(c, m)                              \
  do {                                                \
    if (!(c)) throw Error{RLE_EINVAL, std::string(m)}; \
  } while (0)

// ---- kernels.hip
hipError_t launch_packet(const LevelLaunch& L, hipStream_t st);  // one planned rle_level dispatch (dispatch.h)
int level_capacity();
int trace_stride();
const char* level_kernel_symbol(int ks);  // rle_level<false, ks>'s HSA symbol name
hipError_t launch_append(float* state, float* next_state, float* action, float* reward, float* notdone,
                         float* priority, const float* st_s, const float* st_ns, const float* st_a,
                         const float* st_r, const float* st_d, long long ptr, long long cap, int count,
                         int Sp, int Ap, const float* max_priority, int lap, double* bsum, double* ssum,
                         long long size_before, hipStream_t st);
hipError_t launch_act_chain(const ActChainArgs& a, hipStream_t st);
hipError_t launch_fill(float* state, float* next_state, float* action, float* reward, float* notdone,
                       float* priority, long long n, int S, int Sp, int A, int Ap, unsigned long long seed,
                       hipStream_t st);
hipError_t launch_replay_pack(const ReplayPackArgs& a, hipStream_t st);
hipError_t launch_replay_unpack(const ReplayPackArgs& a, hipStream_t st);
hipError_t launch_state_pack(const StatePackArgs& a, hipStream_t st);
hipError_t launch_state_unpack(const StatePackArgs& a, hipStream_t st);
// (drop_level.hip: the critic dropout's mask stream, [rows][width] row-major, 0 or s; rows <= 2^20, width as LnArgs')
hipError_t launch_dropout_mask(float* out, int rows, int width, unsigned long long seed, unsigned long long step,
                               int site, float p, float s, hipStream_t st);
// ---- replay_norm.hip
hipError_t launch_replay_colsum(const ReplayStatArgs& a, hipStream_t st);
hipError_t launch_replay_colfin(const ReplayStatArgs& a, hipStream_t st);
hipError_t launch_replay_normalize(const ReplayNormArgs& a, hipStream_t st);

}  // namespace rle
