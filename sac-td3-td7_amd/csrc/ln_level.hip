// The KS_LN instance of rle_level (ops.h KernelSet: the LayerNorm critics' step programs' kernel,
// rle_set_layer_norm) as a translation unit -- and so a code object -- of its own, as clip_level.hip is KS_CLIP's:
// kernels.hip up to its dispatch kernel, instantiated for KS_LN alone.  The code objects of kernels.hip and
// clip_level.hip then hold what they held before LayerNorm critics existed (DESIGN "LayerNorm critics").
#define RLE_LN_TU 1
#include "kernels.hip"
