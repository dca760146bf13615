// The KS_NSTEP instance of rle_level (ops.h KernelSet: the kernel of the step programs with n-step returns,
// rle_set_n_step, and of rle_replay_gather_nstep) as a translation unit -- and so a code object -- of its own, as
// drop_level.hip is KS_DROP's: kernels.hip up to its dispatch kernel, instantiated for KS_NSTEP alone.  The code
// objects of kernels.hip, clip_level.hip, ln_level.hip and drop_level.hip then hold what they held before n-step
// returns existed (DESIGN "n-step returns").
#define RLE_NSTEP_TU 1
#include "kernels.hip"
