// The KS_CLIP instance of rle_level (ops.h KernelSet: the clipped step programs' kernel, rle_set_grad_clip) as a
// translation unit -- and so a code object -- of its own: kernels.hip up to its dispatch kernel, instantiated for
// KS_CLIP alone.  kernels.hip's own code object then holds what it held before clipped programs existed, byte for
// byte, so the programs of every other instance run at the addresses they ran at (DESIGN "Gradient clipping").
#define RLE_CLIP_TU 1
#include "kernels.hip"
