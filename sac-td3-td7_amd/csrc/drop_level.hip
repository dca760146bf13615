// The KS_DROP instance of rle_level (ops.h KernelSet: the kernel of the step programs with critic dropout,
// rle_set_critic_dropout) as a translation unit -- and so a code object -- of its own, as ln_level.hip is KS_LN's:
// kernels.hip up to its dispatch kernel, instantiated for KS_DROP alone, and the mask stream's stand-alone kernel
// (rle_dropout_mask).  The code objects of kernels.hip, clip_level.hip and ln_level.hip then hold what they held
// before critic dropout existed (DESIGN "Critic dropout").
#define RLE_DROP_TU 1
#include "kernels.hip"
